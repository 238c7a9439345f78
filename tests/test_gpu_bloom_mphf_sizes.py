"""The Bloom filter (csrc/gkc_bloom.hip) and the MPHF (csrc/gkc_mphf.hip) at exact array sizes, against the oracle bit for bit: Bloom arrays on both sides of a
2^20-bit region border (a last region that receives its neighbour's spill only, or owns 1 / 100 positions; the power-of-two totals), 1 and 10 hash functions, k = 3 .. 5
and the first 16-byte keys, the atomic insert and the gather contains8 on their own; solid k-mers that lie in 1, 2-16 and >= 17 device arrays; MPHF level-0 arrays of
448 / 512 / 2^19 / 2^19 + 64 bits and key lists around the flag scan's chunk of 8192, built three ways; every border of the abundance table and the cell beyond it.
Inputs and expected values: tests/bloom_mphf_inputs.py (tests/test_bloom_mphf_cpu.py pins that each input reaches its edge). Every comparison is exact. The switches
are re-read by every entry point of the library. Run with `pytest -m gpu`."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests import bloom_mphf_inputs as bm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


@pytest.fixture(scope="module")
def counter(gkc):
    c = gkc.Counter(0)
    yield c
    c.close()


def first_difference(got, want):
    """where two byte arrays part, as text (region and bit of the first differing byte)"""
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return "equal"
    i = int(bad[0])
    return "%d bytes differ, the first at byte %d (bit %d = region %d + %d): got %#x, expected %#x" % (len(bad), i, 8 * i, 8 * i // bm.R, 8 * i % bm.R, got[i], want[i])


def same(got, want):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), first_difference(got.view(np.uint8).ravel(), want.view(np.uint8).ravel())


def check_contains8(monkeypatch, bl, queried8, want, gather=False):
    """contains8 by gathers (few k-mers: the default), by region (the threshold lowered to one k-mer), and with the region path switched off"""
    monkeypatch.delenv("GKC_BLOOM_QUERY_REGIONS_MIN", raising=False); monkeypatch.delenv("GKC_BLOOM_GATHER", raising=False)
    same(bl.contains8(queried8), want)
    monkeypatch.setenv("GKC_BLOOM_QUERY_REGIONS_MIN", "1")
    same(bl.contains8(queried8), want)
    if gather:
        monkeypatch.setenv("GKC_BLOOM_GATHER", "1")
        same(bl.contains8(queried8), want)
        monkeypatch.delenv("GKC_BLOOM_GATHER")
    monkeypatch.delenv("GKC_BLOOM_QUERY_REGIONS_MIN")


def build_bloom(gkc, counter, e, chunks):
    bl = gkc.Bloom(counter, e.kind, e.tai_bits, e.nb_hash, e.k)
    assert (bl.nbytes, bl.bitsize) == (e.nbytes, e.bitsize)
    for chunk in chunks:
        bl.insert(chunk)
    return bl


def check_bloom(gkc, counter, monkeypatch, e, chunks, queried, queried8, gather=False):
    """the region build and the atomic build against the oracle's array; contains and contains8 of the region build"""
    monkeypatch.delenv("GKC_BLOOM_ATOMIC", raising=False)
    bl = build_bloom(gkc, counter, e, chunks)
    try:
        same(bl.array(), e.array)
        same(bl.contains(queried), e.contains)
        if e.kind == "neighbor":
            check_contains8(monkeypatch, bl, queried8, e.contains8, gather)
    finally:
        bl.close()
    monkeypatch.setenv("GKC_BLOOM_ATOMIC", "1")
    bl = build_bloom(gkc, counter, e, chunks)
    try:
        same(bl.array(), e.array)                                          # the oracle's bytes, not merely the region build's
    finally:
        bl.close()
        monkeypatch.delenv("GKC_BLOOM_ATOMIC")


# ------------------------------------------------------------------------------------------------ A. array sizes on region borders
@pytest.mark.parametrize("k", bm.A_K)
@pytest.mark.parametrize("kind,tai_bits", bm.A_CASES)
def test_bloom_array_sizes_on_region_borders(gkc, counter, monkeypatch, kind, tai_bits, k):
    """30000 keys inserted in two calls that part at an odd index, 7 hash functions: nbytes, bitsize, array, contains (keys + 2000 others), contains8 (neighbor: 2000
    keys + 2000 others, by gathers and by region; at R + 100 with GKC_BLOOM_GATHER as well), and the array of the atomic insert"""
    e = bm.a_expected(kind, tai_bits, k)
    keys, others = bm.a_keys(k)
    check_bloom(gkc, counter, monkeypatch, e, (keys[: bm.A_SPLIT], keys[bm.A_SPLIT:]), keys + others, bm.a_queried8(k),
                gather=kind == "neighbor" and tai_bits == bm.A_GATHER_SIZE)


# ------------------------------------------------------------------------------------------------ B. nb_hash and k edges
@pytest.mark.parametrize("k", bm.B_HASH_K)
@pytest.mark.parametrize("nb_hash", bm.B_HASHES)
@pytest.mark.parametrize("kind", bm.KINDS)
def test_bloom_one_and_ten_hash_functions(gkc, counter, monkeypatch, kind, nb_hash, k):
    """nb_hash = 1 (no offset at all) and 10 (the documented maximum: every seed, the whole offset table of the region query)"""
    e = bm.b_hash_expected(kind, nb_hash, k)
    check_bloom(gkc, counter, monkeypatch, e, (e.inserted,), e.queried, e.queried8, gather=True)


@pytest.mark.parametrize("k", bm.B_SMALL_K + bm.B_WIDE_K)
@pytest.mark.parametrize("kind", bm.KINDS)
def test_bloom_smallest_k_and_first_wide_keys(gkc, counter, monkeypatch, kind, k):
    """k = 3, 4, 5: all 4^k values queried, every second one inserted (a core of 1 .. 3 nucleotides); k = 32, 33: the core is hashed as a 16-byte value whose high
    word is zero or nearly so, with the all-zero, all-one and word-border keys and a (nearly) palindromic core"""
    e = bm.b_k_expected(kind, k)
    check_bloom(gkc, counter, monkeypatch, e, (e.inserted,), e.queried, e.queried8, gather=True)


# ------------------------------------------------------------------------------------------------ C. results spread over several device arrays
def counted(gkc, k, name):
    """-> (Counter, keys in dataset order, their abundances, number of device arrays the records lie in)"""
    bases, offs, rep, _, _ = bm.c_input(k)
    passes = bm.C_PASSES[name]
    c = gkc.Counter(0); c.set_solidity(2, bm.INF, 10000); c.configure(k, bm.C_M, bm.C_PARTS, rep, nb_passes=passes)
    c.count(bases, offs)
    keys = []; ab = []; where = []
    for ps in range(passes):
        for p in range(bm.C_PARTS):
            lo, hi, a = c.partition(ps, p)
            keys += [int(x) | (int(y) << 64) for x, y in zip(lo.tolist(), hi.tolist())]; ab += a.tolist()
            where.append(c.partition_device(ps, p))
            assert where[-1][1] == len(lo)
    return c, keys, ab, bm.count_arrays(where, c.rec_bytes)


@pytest.mark.parametrize("k,name", bm.C_CASES)
def test_solid_kmers_in_several_device_arrays(gkc, monkeypatch, k, name):
    """the solid k-mers of 1 / 4 / 24 passes lie in one / 2-16 / >= 17 device arrays (counted here from the datasets' device pointers): insert_solid of every kind,
    query_solid with contains8 by gathers and by region (beyond 16 arrays the region path hands over to the gathers), the MPHF of the counter and its abundance map"""
    import torch
    _, _, _, want_keys, want_ab = bm.c_input(k)
    c, keys, ab, n_arrays = counted(gkc, k, name)
    try:
        lo, hi = bm.C_CLASSES[name]
        print("k = %d, %s: %d solid k-mers in %d device arrays" % (k, name, len(keys), n_arrays))
        assert n_arrays >= lo and (hi is None or n_arrays <= hi), (name, n_arrays)
        assert dict(zip(keys, ab)) == dict(zip(want_keys, want_ab)) and len(keys) == len(want_keys)          # the one-pass oracle count, in the device's dataset order
        n = len(keys)
        for kind in bm.KINDS:
            ob = gko.Bloom(kind, 11 * n, 7, k); ob.insert(keys)
            for atomic in (False, True):
                monkeypatch.setenv("GKC_BLOOM_ATOMIC", "1") if atomic else monkeypatch.delenv("GKC_BLOOM_ATOMIC", raising=False)
                bl = gkc.Bloom(c, kind, 11 * n, 7, k); bl.insert_solid()
                try:
                    same(bl.array(), ob.array())
                    if atomic:
                        continue
                    assert bl.query_solid(False) == (n, n)                                                   # no false negative
                    if kind == "neighbor":
                        want8 = ob.contains8(keys)
                        for rmin in (None, "1"):
                            monkeypatch.setenv("GKC_BLOOM_QUERY_REGIONS_MIN", rmin) if rmin else monkeypatch.delenv("GKC_BLOOM_QUERY_REGIONS_MIN", raising=False)
                            out = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
                            nq, npos = bl.query_solid(True, d_out=out.data_ptr())
                            same(out.cpu().numpy(), want8)
                            assert (nq, npos) == (n, int(np.unpackbits(want8).sum()))
                        monkeypatch.delenv("GKC_BLOOM_QUERY_REGIONS_MIN", raising=False)
                finally:
                    bl.close()
            monkeypatch.delenv("GKC_BLOOM_ATOMIC", raising=False)
        om, want_map, above = bm.abundance_map_of(keys, ab, k)
        for rmin in (None, "64"):
            monkeypatch.setenv("GKC_MPHF_REGIONS_MIN", rmin) if rmin else monkeypatch.delenv("GKC_MPHF_REGIONS_MIN", raising=False)
            dm = gkc.Mphf(c)
            try:
                assert dm.size == n
                same(dm.save(), om.save())
                amap, got_above = dm.abundance_map()
                same(amap, want_map)
                assert got_above == above == 0
            finally:
                dm.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ D. MPHF exact sizes
@pytest.mark.parametrize("k,n", bm.D_CASES)
def test_mphf_exact_sizes(gkc, counter, monkeypatch, k, n):
    """level-0 arrays of 448 / 512 bits (8 / 9 words: one / two rank samples), of 2^19 and 2^19 + 64 bits (one region / a second one of a single word and the spare
    word), 8191 / 8192 / 8193 keys (the flag scan's chunk): by region from the first key on, by the atomic path, and ordered: the oracle's stream and codes each time"""
    e = bm.d_expected(k, n)
    for switches in bm.D_BUILDS:
        for name in ("GKC_MPHF_REGIONS_MIN", "GKC_MPHF_REGIONS", "GKC_MPHF_ORDERED"):
            monkeypatch.delenv(name, raising=False)
        for name, value in switches.items():
            monkeypatch.setenv(name, value)
        dm = gkc.Mphf(counter, e.keys, k)
        try:
            assert dm.size == n, switches
            same(dm.save(), e.stream)
            codes = dm.lookup(e.sample)
            same(codes, e.codes)
            assert len(set(codes.tolist())) == len(codes) and int(codes.max()) < n, switches
            same(dm.lookup(e.others), e.other_codes)
        finally:
            dm.close()


# ------------------------------------------------------------------------------------------------ E. abundance table borders
@pytest.mark.parametrize("k", bm.E_K)
def test_abundance_map_on_every_table_border(gkc, k):
    """one k-mer per abundance on both sides of every border of the discretisation table, and at 50000, 50001 and 60000 the cell 255 with the counter of
    abundances above the table's precision"""
    bases, offs, rep, values = bm.e_input(k)
    c = gkc.Counter(0); c.set_solidity(1, bm.INF, 10000); c.configure(k, bm.E_M, bm.E_PARTS, rep)
    try:
        c.count(bases, offs)
        assert c.all_counts() == dict(zip(values, bm.ABUNDANCES))
        ref = gko.Dsk(bases, offs, k, bm.E_M, bm.E_PARTS, rep, abundance_min=1)
        order = []
        for p in range(bm.E_PARTS):
            lo, hi, _ = ref.part(p)
            order += [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]
        ref.close()
        ab = dict(zip(values, bm.ABUNDANCES))
        om, want_map, above = bm.abundance_map_of(order, [ab[x] for x in order], k)
        dm = gkc.Mphf(c)
        try:
            same(dm.save(), om.save())
            amap, got_above = dm.abundance_map()
            codes = om.lookup(order)
            for x, cd in zip(order, codes.tolist()):
                assert amap[cd] == gko.abundance_index(ab[x]), (ab[x], int(amap[cd]))
            same(amap, want_map)
            assert got_above == above == 3
        finally:
            dm.close()
    finally:
        c.close()
