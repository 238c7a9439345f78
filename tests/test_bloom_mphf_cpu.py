"""tests/bloom_mphf_inputs.py pinned on the CPU, with the oracle alone: every input of tests/test_gpu_bloom_mphf_sizes.py reaches the edge it is there for. The Bloom
sizes put bits where the region build must carry them (a last region that receives spill only, or owns 100 positions) or must not (the power-of-two sizes), the MPHF key
counts give the level-0 arrays of 448 / 512 / 2^19 / 2^19 + 64 bits, the abundance reads count to exactly the borders of the discretisation table. A change to the
generators that empties the GPU tests of their edges fails here."""
import numpy as np
import pytest

from oracle import gko
from tests import bloom_mphf_inputs as bm
from tests.util import naive_counts, revcomp_int


# ------------------------------------------------------------------------------------------------ A
def test_bloom_size_geometry():
    """what each size is for, from the constructor's arithmetic alone"""
    R = bm.R
    g = {t: bm.geometry("neighbor", t) for t in bm.A_COHERENT_SIZES}
    assert [t for t in bm.A_COHERENT_SIZES if g[t][2]] == [R - 8192, 2 * R - 8192]               # the power-of-two totals
    assert g[R - 8192][:2] == (R - 1, 1040383) and g[R - 8192][4] == 1
    assert g[2 * R - 8192][:2] == (2 * R - 1, 2 * R - 1 - 8192) and g[2 * R - 8192][4] == 2
    assert g[2 * R - 8192 - 1][0] == 2 * R - 1 and not g[2 * R - 8192 - 1][2]                    # the same tai as a plain modulus
    assert [g[t][4] for t in bm.A_COHERENT_SIZES] == [1, 2, 2, 2, 2, 2, 2, 2]
    # positions a second region owns: none, none, one, 100 (reduced_tai - R root positions)
    assert [g[t][1] - R for t in (R - 100, R, R + 1, R + 100)] == [-100, 0, 1, 100]
    assert [bm.last_region_reachable("cache", t) for t in bm.A_COHERENT_SIZES] == [True, False, True, True, True, True, True, True]
    b = {t: bm.geometry("basic", t) for t in bm.A_BASIC_SIZES}
    assert [b[t][2] for t in bm.A_BASIC_SIZES] == [False, True, False, False, True]              # R and 2R take the mask
    assert [b[t][4] for t in bm.A_BASIC_SIZES] == [1, 1, 2, 2, 2] and b[R + 100][0] - R == 100
    assert bm.A_SPLIT % 2 == 1 and 0 < bm.A_SPLIT < bm.A_KEYS


@pytest.mark.parametrize("k", bm.A_K)
@pytest.mark.parametrize("kind,tai_bits", bm.A_CASES)
def test_bloom_sizes_reach_their_region_edge(kind, tai_bits, k):
    e = bm.a_expected(kind, tai_bits, k)
    tai, reduced, pow2, nchar, n_regions = bm.geometry(kind, tai_bits)
    assert (e.nbytes, e.bitsize) == (nchar, reduced) and len(e.array) == nchar
    last = (n_regions - 1) * bm.R
    if pow2 and kind != "basic":
        assert bm.set_bits(e.array, tai, 8 * nchar) == 0                                         # nothing at or beyond tai
    if kind == "basic":
        assert bm.set_bits(e.array, tai + pow2, 8 * nchar) == 0                                  # positions are taken modulo tai, or masked with it (then tai itself is one)
        if tai_bits == bm.R + 100:
            assert bm.set_bits(e.array, last, 8 * nchar) >= 5
    elif n_regions > 1 and bm.last_region_reachable(kind, tai_bits):
        spill = bm.set_bits(e.array, last, last + bm.REACH - 1)                                   # the first 4107 bits of the last region
        assert spill >= 50, spill
        if reduced <= last:                                                                      # the last region owns no position: whatever it holds is spill
            assert bm.set_bits(e.array, last, 8 * nchar) == spill
    elif n_regions > 1:                                                                          # R - 8192 + 1: a second region of two bits that nothing reaches
        assert bm.set_bits(e.array, last - 4000, 8 * nchar) == 0 and bm.set_bits(e.array, 0, last) > 100000
    assert bm.set_bits(e.array, 0, 8 * nchar) > 100000
    keys, others = bm.a_keys(k)
    assert bool(e.contains[: len(keys)].all()) and int(e.contains[len(keys):].sum()) < len(others) // 4             # no false negative
    if kind == "neighbor":
        h = bm.A_OTHERS // 2
        assert len(e.contains8) == 2 * bm.A_OTHERS == len(bm.a_queried8(k))
        assert bool((e.contains8[:h] & 0x0F).all()) and bool((e.contains8[h: 2 * h] & 0xF0).all())                  # a right / a left neighbour of these is a key
        assert int((e.contains8[2 * h:] != 0).sum()) < h


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("k", bm.B_HASH_K)
@pytest.mark.parametrize("nb_hash", bm.B_HASHES)
@pytest.mark.parametrize("kind", bm.KINDS)
def test_bloom_hash_count_inputs(kind, nb_hash, k):
    e = bm.b_hash_expected(kind, nb_hash, k)
    n = bm.set_bits(e.array, 0, 8 * e.nbytes)
    assert bm.B_HASH_KEYS * nb_hash * 0.6 < n <= bm.B_HASH_KEYS * nb_hash                         # every function sets its bit (few coincide at 11 bits per key)
    assert bool(e.contains[: bm.B_HASH_KEYS].all())
    false_pos = int(e.contains[bm.B_HASH_KEYS:].sum())
    assert (false_pos > 20) if nb_hash == 1 else (false_pos < 100)


@pytest.mark.parametrize("k", bm.B_SMALL_K + bm.B_WIDE_K)
@pytest.mark.parametrize("kind", bm.KINDS)
def test_bloom_k_edge_inputs(kind, k):
    e = bm.b_k_expected(kind, k)
    assert all(0 <= x < 4 ** k for x in e.queried) and len(set(e.queried)) == len(e.queried)
    assert bool(e.contains[: len(e.inserted)].all()) if k > 5 else bool(e.contains[::2].all())
    if k <= 5:
        assert len(e.queried) == 4 ** k and len(e.inserted) == 4 ** k // 2 and not bool(e.contains.all())
    else:
        hand = bm.hand_made_keys(k)
        assert set(x for x in hand if x < 4 ** k) <= set(e.inserted) and {0, 4 ** k - 1, (1 << 64) - 1} <= set(e.inserted)
        assert ((1 << 64) in e.inserted) == (k > 32)                                             # (2^64 is no 32-mer)
        core = (hand[4] >> 2) & (4 ** (k - 2) - 1)
        rc = revcomp_int(core, k - 2)
        assert rc == core if k % 2 == 0 else bin(rc ^ core).count("1") == 1
        high = sum(1 for x in e.inserted if x >> 64)                                             # keys whose high word is not zero: none at k = 32, 3 in 4 at k = 33
        assert high == 0 if k == 32 else 2000 < high < len(e.inserted) - 500


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("k", sorted({k for k, _ in bm.C_CASES}))
def test_solid_set_of_the_pass_cases(k):
    bases, offs, rep, keys, ab = bm.c_input(k)
    assert 2000 <= len(keys) <= 9000 and min(ab) >= 2
    assert list(keys) == sorted(keys)
    for name, passes in bm.C_PASSES.items():                                                     # the same solid set however many passes count it
        ref = gko.Dsk(bases, offs, k, bm.C_M, bm.C_PARTS, rep, nb_passes=passes, abundance_min=2)
        got = ref.all_counts()
        nonempty = sum(1 for d in range(passes * bm.C_PARTS) if len(ref.part(d)[0]))
        ref.close()
        assert got == dict(zip(keys, ab)), name
        lo, hi = bm.C_CLASSES[name]
        assert nonempty >= lo, (name, nonempty)                                                  # enough datasets with records for the class
    assert bm.count_arrays([(1000, 5), (1080, 0), (1080, 2), (1112, 1), (5000, 3), (0, 0), (5048, 1), (5070, 1)], 16) == 3
    assert bm.count_arrays([(1000, 5), (1160, 2)], 32) == 1 and bm.count_arrays([], 16) == 0


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("k,n", bm.D_CASES)
def test_mphf_sizes_reach_their_level0_array(k, n):
    e = bm.d_expected(k, n)
    assert len(e.keys) == len(set(e.keys)) == n and not set(e.keys) & set(e.others) and len(e.others) == 500
    gamma, nelem, last, levels, n_final = bm.mphf_levels(e.stream.tobytes())
    assert (gamma, nelem, n_final) == (3.0, n, 0) and last == n and len(levels) == 25
    domain, nchar, nranks = levels[0]
    assert nchar == domain // 64 + 1 and nranks == (nchar + 7) // 8
    if n in bm.D_LEVEL0:
        assert domain == bm.D_LEVEL0[n]
    if n in (149, 150):
        assert (nchar, nranks) == ((8, 1) if n == 149 else (9, 2))
    if n in (174762, 174763):
        assert (domain + bm.MR - 1) // bm.MR == (1 if n == 174762 else 2)
    codes = e.codes.tolist()
    assert len(set(codes)) == len(codes) and max(codes) < n
    if n <= 8193:
        assert sorted(codes) == list(range(n))
    assert len(bm.d_sample(n)) == (n if n <= 8193 else len(set(range(0, n, 8)) | set(range(600)) | set(range(n - 600, n))))


def test_mphf_size_list():
    assert {n for _, n in bm.D_CASES} == set(bm.D_SIZES) and {8191, 8192, 8193} <= set(bm.D_SIZES)          # the flag scan's chunk of 8192 and its neighbours
    assert sorted(n for k, n in bm.D_CASES if k == 63) == [150, 8193, 174763]
    assert [sorted(b) for b in bm.D_BUILDS] == [["GKC_MPHF_REGIONS_MIN"], ["GKC_MPHF_REGIONS"], ["GKC_MPHF_ORDERED"]]


# ------------------------------------------------------------------------------------------------ E
def test_abundance_table_borders():
    """the oracle's index is the plain search of the restated table, and the abundances lie on both sides of a border in every stretch of the table"""
    t = bm.ABUNDANCE_TABLE
    assert len(t) == 257 and t[70] == 70 and t[85] == 100 and t[125] == 500 and t[150] == 1000 and t[190] == 5000 and t[215] == 10000 and t[255] == t[256] == 50000
    for a in list(bm.ABUNDANCES) + list(range(0, 1200)) + [2 ** 31 - 1]:
        assert gko.abundance_index(a) == bm.table_index(a), a
    idx = {a: bm.table_index(a) for a in bm.ABUNDANCES}
    for below, at in ((69, 70), (71, 72), (99, 100), (109, 110), (499, 500), (519, 520), (999, 1000), (1099, 1100), (4999, 5000), (5199, 5200), (9999, 10000),
                      (10999, 11000), (48999, 49000), (49999, 50000)):
        assert idx[at] == idx[below] + 1 and t[idx[at]] == at, (below, at)
    for same in ((70, 71), (72, 73), (100, 101, 102, 109), (110, 111), (500, 501, 519), (1000, 1001, 1099), (5000, 5199), (10000, 10999), (50000, 50001, 60000)):
        assert len({idx[a] for a in same}) == 1, same
    assert idx[49999] == 254 and idx[50000] == 255 and sum(1 for a in bm.ABUNDANCES if a >= t[255]) == 3
    assert len(set(bm.ABUNDANCES)) == len(bm.ABUNDANCES) == 38


@pytest.mark.parametrize("k", bm.E_K)
def test_abundance_reads_count_to_the_borders(k):
    bases, offs, rep, values = bm.e_input(k)
    assert len(offs) - 1 == sum(bm.ABUNDANCES) and len(bases) == k * sum(bm.ABUNDANCES)
    ref = gko.Dsk(bases, offs, k, bm.E_M, bm.E_PARTS, rep, abundance_min=1)
    assert ref.all_counts() == dict(zip(values, bm.ABUNDANCES))
    assert ref.stats["kmers_nb_solid"] == len(bm.ABUNDANCES)
    ref.close()
    reads = bases.reshape(-1, k)
    first = [reads[i].tobytes() for i in range(200)]
    assert len(set(first)) > 10 and set(naive_counts(first, k)) <= set(values)                   # shuffled, both strands, canonical values as chosen
    assert sum(1 for r in first if r[:1] != b"A") > 20
