"""Graph neighbourhoods of the solid k-mers on the device (csrc/gkc_graph.hip: gkc_graph_neighbors_solid / _partition, gkc_graph_branching_solid; gkc.Counter.neighbor_masks,
branching_nodes, graph_topology). Expected values: the reference's own /branching/nodes (tests/golden/reference_run), the numpy / Python statement of the masks in
tests/test_graph_cpu.py (pinned there by those fixtures), and the composed path — eight neighbour keys per record answered by query_kmers_device. Every comparison is exact.
Run with `pytest -m gpu`."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_graph_cpu import branching_from_masks, graph_masks_np, neighbours, pack_branching, revcomp, topology_from_masks
from tests.test_query_cpu import INF, freq_order_of
from tests.test_reference_run import DIR, load
from tests.test_reference_run import freq_order_of as fixture_freq_order
from tests.util import simple_repart

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def repart_for(m, parts):
    """a random table; with 512 partitions every third one gets no minimizer at all, so that some datasets are empty whatever the input"""
    rep = simple_repart(m, parts)
    if parts == 512:
        rep[rep % 3 == 0] += 1
    return rep


def counter_for(gkc, bases, offs, k, m, parts, passes=1, freq=None, amin=1, amax=INF):
    c = gkc.Counter(0); c.configure(k, m, parts, repart_for(m, parts), nb_passes=passes, freq_order=freq)
    if (amin, amax) != (1, INF):
        c.set_solidity(amin, amax)
    c.count(bases, offs)
    return c


def solid_records(c):
    """-> (values as Python ints, abundances, records per dataset), dataset order"""
    vals, abund, sizes = [], [], []
    for ps in range(c.nb_passes):
        for pt in range(c.nb_partitions):
            lo, hi, ab = c.partition(ps, pt)
            vals += [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]
            abund += ab.tolist(); sizes.append(len(lo))
    return vals, abund, sizes


def count_records(values, abundances, k):
    """Count records as gkc_partition_counts lays them out: 16 bytes {value u64, abundance u32, pad} / 32 bytes {value u128, abundance u32, pad}, pad bytes zero"""
    rb = 16 if k <= 31 else 32
    out = np.zeros((len(values), rb), np.uint8)
    for i, (v, a) in enumerate(zip(values, abundances)):
        out[i, : rb // 2] = np.frombuffer(int(v).to_bytes(rb // 2, "little"), np.uint8)
        out[i, rb // 2: rb // 2 + 4] = np.frombuffer(int(a).to_bytes(4, "little"), np.uint8)
    return out


def branching_raw(gkc, c, d_masks, cap, n_alloc=None):
    """gkc_graph_branching_solid with a device buffer of n_alloc records pre-filled with 0xEE -> (rc, n_branching, uint8[n_alloc][record bytes], topology[5][5])"""
    import torch
    n_alloc = cap if n_alloc is None else n_alloc
    t = torch.full((max(1, n_alloc) * c.rec_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = C.c_uint64(); topo = np.zeros(25, np.uint64)
    rc = c.L.gkc_graph_branching_solid(c.h, d_masks, t.data_ptr(), cap, C.byref(nb), topo.ctypes.data_as(C.c_void_p))
    return rc, nb.value, t.cpu().numpy()[: n_alloc * c.rec_bytes].reshape(n_alloc, c.rec_bytes), topo.reshape(5, 5)


# ------------------------------------------------------------------------------------------------ 1. the reference's own /branching/nodes
@pytest.mark.parametrize("name", ["k31_defaults", "k63_defaults", "k21_defaults_parts"])
def test_branching_nodes_equal_the_reference_run(gkc, name):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    c = gkc.Counter(0); c.set_solidity(2, 2147483647, 10000); c.configure(k, m, nbpart, table, freq_order=fixture_freq_order(z, m))
    c.begin_pass(0)
    assert c.push_fastx(bytes(z["fasta"])) == len(z["fasta"])
    c.finish_pass()
    assert c.stats()["kmers_nb_solid"] == int(z["nb_solid_kmers"])
    lo, hi, ab = c.branching_nodes(sort=True)
    values = [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]
    assert values == sorted(values)
    got = pack_branching(values, ab.tolist(), k)
    print("%s: %d solid k-mers, %d branching" % (name, int(z["nb_solid_kmers"]), len(values)))
    assert got == bytes(z["branching_nodes"])
    c.close()


# ------------------------------------------------------------------------------------------------ 2. every mask byte against the statement
MASK_CASES = [
    # k, m, partitions, passes, order, reads, genome, substitutions per 10^6, abundance window
    (5, 3, 3, 1, "lexi", 2000, 5000, 10000, (1, INF)),           # nearly every 5-mer present: masks with many bits, self-loops
    (21, 7, 7, 1, "lexi", 2000, 5000, 10000, (1, INF)),
    (31, 8, 7, 1, "lexi", 2000, 5000, 10000, (1, INF)),          # the left extension lands in bits 60-61
    (32, 8, 7, 1, "lexi", 2000, 5000, 10000, (1, INF)),          # first 16-byte key, the left extension crosses the word boundary; even k: palindromes
    (33, 8, 7, 1, "lexi", 2000, 5000, 10000, (1, INF)),
    (63, 10, 7, 1, "lexi", 2000, 5000, 10000, (1, INF)),         # bits 124-125
    (21, 6, 7, 1, "freq", 2000, 5000, 10000, (1, INF)),          # frequency-order minimizers
    (31, 8, 7, 2, "lexi", 2000, 5000, 10000, (1, INF)),          # neighbours in the other pass's datasets
    (31, 8, 1, 1, "lexi", 2000, 5000, 10000, (1, INF)),
    (31, 8, 512, 1, "lexi", 2000, 5000, 10000, (1, INF)),        # empty datasets, datasets below one index sample of 256 records
    (31, 8, 4, 1, "lexi", 20000, 20000, 2000, (1, INF)),         # datasets of many samples
    (31, 8, 7, 1, "lexi", 2000, 5000, 10000, (3, 50)),           # a neighbour counted outside the window is not a neighbour
]


def case_id(c):
    return "k%d-m%d-P%d-p%d-%s-n%d-a%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[8][0])


@functools.lru_cache(maxsize=None)
def reads_of(gkc_mod, n_reads, genome, sub_ppm, read_len=100):
    return gkc_mod.synth_reads_np(11, n_reads, read_len, genome, sub_ppm)


@pytest.mark.parametrize("case", MASK_CASES, ids=case_id)
def test_masks_against_the_statement(gkc, case):
    k, m, parts, passes, order, n_reads, genome, sub_ppm, (amin, amax) = case
    bases, offs = reads_of(gkc, n_reads, genome, sub_ppm)
    freq = None
    if order == "freq":
        freq = freq_order_of([bases[i * 100:(i + 1) * 100].tobytes() for i in range(n_reads)], m)
    c = counter_for(gkc, bases, offs, k, m, parts, passes, freq, amin, amax)
    vals, _, sizes = solid_records(c)
    assert len(vals) == c.stats()["kmers_nb_solid"] > 0
    exp = graph_masks_np(vals, k)
    got = c.neighbor_masks()
    ins, outs = np.unpackbits((exp >> 4)[:, None], axis=1).sum(1), np.unpackbits((exp & 15)[:, None], axis=1).sum(1)
    print("%s: %d solid k-mers in %d datasets (largest %d, %d empty), %d with in > 1, %d with out > 1" % (case_id(case), len(vals), len(sizes), max(sizes), sizes.count(0), (ins > 1).sum(), (outs > 1).sum()))
    assert (ins > 1).any() and (outs > 1).any()                  # the genome is small enough for degrees above 1
    if parts == 512:
        assert 0 in sizes and 0 < min(s for s in sizes if s) < 256
    if n_reads == 20000:
        assert min(sizes) > 20 * 256
    if k == 5:
        assert any(min(nn, revcomp(nn, k)) == x for x in vals for nn in neighbours(x, k))       # self-loops
    if (amin, amax) != (1, INF):
        full = counter_for(gkc, bases, offs, k, m, parts, passes, freq)
        every, _, _ = solid_records(full); full.close()
        assert len(every) > len(vals) and not np.array_equal(graph_masks_np(vals, k, solid=every), exp)      # neighbours that were counted, outside the window
    bad = np.flatnonzero(got != exp)
    assert len(got) == len(exp) and len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])
    c.close()


# ------------------------------------------------------------------------------------------------ 3. the composed path at size
def neighbour_keys_on_device(lo, hi, k):
    """the eight neighbour keys of every record, built with torch on the device -> int64 tensor [n][8][1 or 2] (8 / 16-byte keys, not canonical: the query takes the
    canonical form). int64 arithmetic: shifts wrap, right shifts are masked"""
    import torch
    tl = torch.from_numpy(lo.view(np.int64).copy()).cuda()
    j = torch.arange(4, dtype=torch.int64, device="cuda")[None, :]
    m62 = (1 << 62) - 1
    if k <= 31:
        x = tl[:, None]
        right = ((x << 2) | j) & ((1 << (2 * k)) - 1)
        left = ((x >> 2) & m62) | (j << (2 * (k - 1)))
        return torch.cat([right, left], 1)[:, :, None].contiguous()
    th = torch.from_numpy(hi.view(np.int64).copy()).cuda()
    xl, xh = tl[:, None], th[:, None]
    r_lo = (xl << 2) | j
    r_hi = (((xh << 2) | ((xl >> 62) & 3)) & ((1 << (2 * k - 64)) - 1)).expand(-1, 4)
    l_lo = (((xl >> 2) & m62) | ((xh & 3) << 62)).expand(-1, 4)
    l_hi = ((xh >> 2) & m62) | (j << (2 * (k - 1) - 64))
    return torch.stack([torch.cat([r_lo, l_lo], 1), torch.cat([r_hi, l_hi], 1)], 2).contiguous()


@pytest.mark.parametrize("k,m", [(31, 10), (63, 11)])
def test_masks_equal_the_composed_path(gkc, k, m):
    import torch
    parts = 16
    bases, offs = gkc.synth_reads_np(7, 20000, 150, 100000, 10000)
    c = counter_for(gkc, bases, offs, k, m, parts)
    recs = [c.partition(0, p) for p in range(parts)]
    lo = np.concatenate([r[0] for r in recs]); hi = np.concatenate([r[1] for r in recs])
    n = len(lo)
    assert n == c.stats()["kmers_nb_solid"] > 500000
    keys = neighbour_keys_on_device(lo, hi, k)
    ans = torch.zeros(8 * n + 4, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    c.query_kmers_device(keys.data_ptr(), 8 * n, 8 if k <= 31 else 16, ans.data_ptr())
    bits = (ans[: 8 * n].reshape(n, 8) > 0).to(torch.int32) << torch.arange(8, dtype=torch.int32, device="cuda")[None, :]
    exp = bits.sum(1).to(torch.uint8).cpu().numpy()
    got = c.neighbor_masks()
    print("k=%d: %d solid k-mers, %d neighbour bits" % (k, n, int(np.unpackbits(exp).sum())))
    assert (exp != 0).any()
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])
    c.close()


# ------------------------------------------------------------------------------------------------ 4. branching nodes, topology, one dataset at a time
@pytest.mark.parametrize("k,m", [(31, 8), (63, 10)])
def test_branching_topology_and_partitions(gkc, k, m):
    import torch
    parts, passes = 7, 2
    bases, offs = reads_of(gkc, 2000, 5000, 10000)
    c = counter_for(gkc, bases, offs, k, m, parts, passes)
    vals, abund, sizes = solid_records(c)
    n = len(vals)
    masks = c.neighbor_masks()
    assert np.array_equal(masks, graph_masks_np(vals, k))
    # the masks where they lie: an unaligned device pointer too
    t = torch.zeros(n + 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    assert c.neighbor_masks(d_out=t.data_ptr() + 1) == n
    on_dev = t.cpu().numpy()
    assert np.array_equal(on_dev[1: n + 1], masks) and on_dev[0] == 0 and not on_dev[n + 1:].any()
    d_masks = t.data_ptr() + 1
    # topology
    topo = c.graph_topology()
    assert int(topo.sum()) == n and np.array_equal(topo, topology_from_masks(masks))
    assert np.array_equal(c.graph_topology(d_masks=d_masks), topo)
    # the records whose mask says branching: dataset order, ascending per dataset, their abundance, zero pad bytes
    br = branching_from_masks(masks)
    exp = count_records([v for v, b in zip(vals, br) if b], [a for a, b in zip(abund, br) if b], k)
    nb = len(exp)
    assert 0 < nb < n
    bounds = np.concatenate([[0], np.cumsum([int(br[s - z: s].sum()) for s, z in zip(np.cumsum(sizes), sizes)])])
    ev = [v for v, b in zip(vals, br) if b]
    assert all(ev[a:b] == sorted(ev[a:b]) for a, b in zip(bounds[:-1], bounds[1:]))
    rc, got_n, got, topo2 = branching_raw(gkc, c, d_masks, nb, nb + 2)
    assert rc == 0 and got_n == nb and np.array_equal(topo2, topo)
    assert np.array_equal(got[:nb], exp) and (got[nb:] == 0xEE).all()
    # d_masks = NULL: computed inside
    rc, got_n, got, topo2 = branching_raw(gkc, c, None, nb, nb + 2)
    assert rc == 0 and got_n == nb and np.array_equal(topo2, topo) and np.array_equal(got[:nb], exp) and (got[nb:] == 0xEE).all()
    # room for one record too few
    rc, got_n, got, _ = branching_raw(gkc, c, d_masks, nb - 1, nb + 2)
    assert rc == 4 and got_n == nb and b"branching" in c.L.gkc_last_error(c.h)
    assert np.array_equal(got[: nb - 1], exp[: nb - 1]) and (got[nb - 1:] == 0xEE).all()
    # the binding: unsorted = the records above, sorted = ascending by value
    lo, hi, ab = c.branching_nodes(sort=False)
    assert [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())] == ev and ab.tolist() == [a for a, b in zip(abund, br) if b]
    lo, hi, ab = c.branching_nodes(sort=True, d_masks=d_masks)
    assert [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())] == sorted(ev)
    # every dataset equals its slice of the whole
    at = 0
    for ps in range(passes):
        for pt in range(parts):
            part = c.neighbor_masks_partition(ps, pt)
            assert np.array_equal(part, masks[at: at + sizes[ps * parts + pt]]), (ps, pt)
            at += sizes[ps * parts + pt]
    assert at == n
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*out of range"):
        c.neighbor_masks_partition(passes, 0)
    c.close()


# ------------------------------------------------------------------------------------------------ 5. state
def test_state_errors_recount_and_empty_results(gkc):
    k, m, parts = 31, 8, 8
    bases, offs = reads_of(gkc, 2000, 5000, 10000)
    calls = [lambda c: c.neighbor_masks(), lambda c: c.neighbor_masks_partition(0, 0), lambda c: c.branching_nodes(), lambda c: c.graph_topology()]
    c = gkc.Counter(0)
    for f in calls:
        with pytest.raises(gkc.GkcError, match="gkc error 1: .*gkc_configure"):
            f(c)
    c.configure(k, m, parts, simple_repart(m, parts))
    c.begin_pass(0); c.push_reads(bases, offs)
    for f in calls:
        with pytest.raises(gkc.GkcError, match="gkc error 1: .*still open"):
            f(c)
    c.finish_pass()
    vals1, _, _ = solid_records(c)
    m1 = c.neighbor_masks()
    assert np.array_equal(m1, graph_masks_np(vals1, k))
    # a recount with another abundance-min: the masks are those of the new results (the index of the first count must not answer)
    c.set_solidity(3, INF)
    c.count(bases, offs)
    vals3, _, _ = solid_records(c)
    assert 0 < len(vals3) < len(vals1)
    m3 = c.neighbor_masks()
    assert np.array_equal(m3, graph_masks_np(vals3, k))
    keep = {v: b for v, b in zip(vals1, m1.tolist())}
    assert any(keep[v] != b for v, b in zip(vals3, m3.tolist()))      # some k-mer lost a neighbour to the new window
    assert np.array_equal(c.graph_topology(), topology_from_masks(m3))
    # a count without any solid k-mer
    c.set_solidity(1000000, INF)
    c.count(bases, offs)
    assert c.stats()["kmers_nb_solid"] == 0
    assert c.neighbor_masks().shape == (0,) and c.neighbor_masks().dtype == np.uint8 and c.neighbor_masks_partition(0, 3).shape == (0,)
    lo, hi, ab = c.branching_nodes()
    assert len(lo) == len(hi) == len(ab) == 0
    assert not c.graph_topology().any() and c.graph_topology().shape == (5, 5)
    rc, nb, _, topo = branching_raw(gkc, c, None, 4)
    assert rc == 0 and nb == 0 and not topo.any()
    # a released pass
    c.set_solidity(1, INF)
    c.count(bases, offs)
    assert np.array_equal(c.neighbor_masks(), m1)
    c.release_pass(0)
    for f in calls:
        with pytest.raises(gkc.GkcError, match="gkc error 1: .*released"):
            f(c)
    c.close()
