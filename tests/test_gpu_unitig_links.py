"""Links between the unitigs on the device (csrc/gkc_unitig_links.hip: gkc_graph_unitigs_links; gkc.Counter.unitig_links, unitig_links_device, write_unitigs_fasta).
Expected values: statement A of tests/test_unitig_links_cpu.py (the definition over the masks and the placement, pinned there by the reference's own links of one input
and by statement B, the overlaps of the sequences) — offsets and entries element for element — and the reference's digest itself. Every comparison is exact.
Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_unitigs import CASES, GENOME, N_READS, READ_LEN, SUB_PPM, case_id, circle_read, fixture_counter, pack, palindrome_reads
from tests.test_query_cpu import INF, freq_order_of
from tests.test_unitig_links_cpu import (assert_symmetric, csr, fixture_links, fork_reads, hairpin_reads, histogram, links_digest, overlap_links, parse_unitigs_fasta,
                                         poly_a_reads, random_sequence, reference_links_digest, slots_of, star_reads, unitig_links_np)
from tests.test_unitigs_cpu import CYCLES, NOT_ISOLATED, circle, split_sequences, unitigs_np
from tests.util import simple_repart

pytestmark = pytest.mark.gpu
TILE = 1024                                                         # slots per tile of the scan (GR_TILE of csrc/gkc_graph.hpp)


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def assert_equals_statement(c, k, u=None, slots=None, d_masks=None):
    """the device's links of the results c holds against statement A over the same records -> (values, the statement's unitigs, its slots)"""
    vals = None
    if slots is None:
        vals, abund, _ = solid_records(c)
        u = unitigs_np(vals, abund, k)
        slots = unitig_links_np(vals, k, u)
    offs, links = c.unitig_links(d_masks)
    assert offs.dtype == np.uint64 and links.dtype == np.uint64
    want_offs, want_links = csr(slots)
    assert len(offs) == 2 * len(u["seqs"]) + 1 and np.array_equal(offs, want_offs)
    assert np.array_equal(links, want_links), (slots_of(offs, links)[:20], slots[:20])
    return vals, u, slots


def counter_of_reads(gkc, reads, k, m, parts=4, passes=1):
    bases, offs = pack(reads)
    return counter_for(gkc, bases, offs, k, m, parts, passes)


def links_raw(c, d_masks, cap_unitigs, cap_links, room_unitigs, room_links, offsets=True, links=True):
    """gkc_graph_unitigs_links into buffers pre-filled with 0xEE -> (rc, *n_links, offsets bytes, links bytes)"""
    import torch
    to = torch.full(((2 * room_unitigs + 1) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    tl = torch.full((max(1, room_links) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nl = C.c_uint64(0xDEAD)
    rc = c.L.gkc_graph_unitigs_links(c.h, d_masks, to.data_ptr() if offsets else None, cap_unitigs, tl.data_ptr() if links else None, cap_links, C.byref(nl))
    return rc, nl.value, to.cpu().numpy(), tl.cpu().numpy()[: room_links * 8]


# ------------------------------------------------------------------------------------------------ 1. the reference's own links, and 16-byte keys
def test_links_equal_the_reference_run(gkc):
    c, k = fixture_counter(gkc, "k21_freq_4parts")
    _, u, slots = fixture_links("k21_freq_4parts")
    assert len(slots) == 1422 > TILE and sum(len(s) for s in slots) == 1528
    assert_equals_statement(c, k, u, slots)
    bases, offs, _ = c.unitigs()
    lo, links = c.unitig_links()
    got = links_digest(split_sequences(bases, offs), slots_of(lo, links))      # from the device's arrays and sequences alone
    print("k21_freq_4parts: %d unitigs, %d links" % (got[0], got[1]))
    assert got == reference_links_digest()
    c.close()


def test_links_equal_the_statement_with_16_byte_keys(gkc):
    c, k = fixture_counter(gkc, "k63_defaults")
    _, u, slots = fixture_links("k63_defaults")
    assert k == 63 and sum(len(s) for s in slots) == 8
    assert_equals_statement(c, k, u, slots)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. small synthetic inputs against the statement
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_links_against_the_statement(gkc, case):
    k, m, parts, passes, order, (amin, amax) = case
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes() for i in range(N_READS)]
    if k == 5:
        reads = reads[:1]
    if k % 2 == 0:
        reads += palindrome_reads(np.random.default_rng(k), k)
    if k == 5 or k % 2 == 0:
        bases, offs = pack(reads)
    freq = freq_order_of(reads, m) if order == "freq" else None
    c = counter_for(gkc, bases, offs, k, m, parts, passes, freq, amin, amax)
    vals, u, slots = assert_equals_statement(c, k)
    h = histogram(slots)
    print("%s: %d unitigs, %d links, sides with 0..4 links: %s" % (case_id(case), len(u["seqs"]), sum(len(s) for s in slots), h))
    assert sum(h[1:]) > 0
    if k % 2 == 1:
        assert slots == overlap_links(u["seqs"], k)
        assert_symmetric(slots)
    if k == 5:
        assert h[4] > 0 and any((e >> 1) == (t >> 1) for t, s in enumerate(slots) for e in s)      # degree-4 sides, self-links
    c.close()


# ------------------------------------------------------------------------------------------------ 3. shapes with known links
def test_one_record_alone_and_a_path_of_two(gkc):
    for n_records in (1, 2):
        read = random_sequence(np.random.default_rng(n_records), n_records + 20)
        c = counter_of_reads(gkc, [read], 21, 7)
        vals, u, slots = assert_equals_statement(c, 21)
        assert len(vals) == n_records and slots == [[], []]
        offs, links = c.unitig_links()
        assert offs.tolist() == [0, 0, 0] and links.shape == (0,)
        c.close()


@pytest.mark.parametrize("shape,n_unitigs,want", [
    ("hairpin", 1, [[1], []]),                                       # L:+:0:-
    ("poly_a", 3, [[0, 2], [1, 5], [], [1, 5], [0, 2], []]),       # the poly-A record links to itself on both sides
    ("fork", 3, [[3, 4], [], [1], [], [], [1]]),
    ("star", 5, None)])
def test_constructed_shapes(gkc, shape, n_unitigs, want):
    reads = {"hairpin": hairpin_reads, "poly_a": poly_a_reads, "fork": fork_reads, "star": star_reads}[shape]()
    c = counter_of_reads(gkc, reads, 21, 7, parts=1)                # one dataset: flat order = ascending values, the numbering of the lists above
    vals, u, slots = assert_equals_statement(c, 21)
    assert len(u["seqs"]) == n_unitigs
    if want is not None:
        assert slots == want
    else:                                                           # one side with exactly four links, ascending, to four unitigs
        assert histogram(slots) == [5, 4, 0, 0, 1]
        offs, links = c.unitig_links()
        t = int(np.flatnonzero(np.diff(offs.astype(np.int64)) == 4)[0])
        four = links[int(offs[t]): int(offs[t + 1])].tolist()
        assert four == sorted(four) and len({e >> 1 for e in four}) == 4
    c.close()


# ------------------------------------------------------------------------------------------------ 4. cycles
@pytest.mark.parametrize("k,L", CYCLES)
def test_a_circle_alone(gkc, k, L):
    seq, want = circle(k, L)
    m = 3 if k == 5 else (4 if k == 7 else 7)
    c = counter_of_reads(gkc, [circle_read(seq, k)], k, m)
    vals, u, slots = assert_equals_statement(c, k)
    if (k, L) not in NOT_ISOLATED:
        assert slots == [[0 << 1 | 0], [0 << 1 | 1]]                # L:+:0:+ and L:-:0:-
        first = c.unitig_links()
        again = c.unitig_links()                                    # a second call gives identical arrays
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
    c.close()


def test_circles_mixed_with_ordinary_reads(gkc):
    k, m, parts = 21, 7, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes().decode() for i in range(N_READS)]
    reads += [circle_read(circle(k, L)[0], k) for L in (k + 3, 40, 200)]
    c = counter_of_reads(gkc, reads, k, m, parts, passes=2)
    vals, u, slots = assert_equals_statement(c, k)
    assert u["n_cycles"] == 3
    for L in (k + 3, 40, 200):
        un = int(u["unitig"][vals.index(circle(k, L)[1][0])])
        assert slots[2 * un] == [un << 1 | 0] and slots[2 * un + 1] == [un << 1 | 1]
    first = c.unitig_links()
    again = c.unitig_links()
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    c.close()


# ------------------------------------------------------------------------------------------------ 5. the borders of the scan's tiles
def forks_and_singles(n_forks, n_singles, k, seed):
    """n_forks disjoint forks (lead + x, lead + y, z + lead: 3 unitigs, 4 links) and n_singles isolated reads of k bases (1 unitig, no link)"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_forks):
        lead = random_sequence(rng, k - 1)
        reads += [lead + "A" + random_sequence(rng, 2), lead + "C" + random_sequence(rng, 2), random_sequence(rng, 3) + lead]
    reads += [random_sequence(rng, k) for _ in range(n_singles)]
    return reads


@pytest.mark.parametrize("n_forks,n_singles", [(100, TILE // 2 - 301), (100, TILE // 2 - 300), (100, TILE // 2 - 299), (100, TILE - 300 + 6)],
                         ids=["T-2", "T", "T+2", "above-2T"])
def test_slot_counts_around_the_scan_tile(gkc, n_forks, n_singles):
    k, m = 31, 8
    n_unitigs = 3 * n_forks + n_singles
    assert 2 * n_unitigs in (TILE - 2, TILE, TILE + 2) or 2 * n_unitigs > 2 * TILE
    c = counter_of_reads(gkc, forks_and_singles(n_forks, n_singles, k, 5 * n_singles), k, m, parts=7)
    assert c.unitigs_build()[0] == n_unitigs                        # the input is what it was meant to be
    vals, u, slots = assert_equals_statement(c, k)
    assert len(slots) == 2 * n_unitigs and sum(len(s) for s in slots) == 4 * n_forks
    assert histogram(slots) == [2 * n_unitigs - 3 * n_forks, 2 * n_forks, n_forks, 0, 0]
    c.close()


# ------------------------------------------------------------------------------------------------ 6. the FASTA with its links
def test_unitigs_fasta_parsed_back(gkc, tmp_path):
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts, amin=2)
    path = str(tmp_path / "out.unitigs.fa")
    nu, nl = c.write_unitigs_fasta(path)
    ub, uo, kc = c.unitigs()
    lo, links = c.unitig_links()
    ids, fields, seqs, slots = parse_unitigs_fasta(path)
    want = [s.decode() for s in split_sequences(ub, uo)]
    assert (nu, nl) == (len(want), len(links)) and nl > 0
    assert ids == list(range(nu)) and seqs == want
    assert slots == slots_of(lo, links)                             # the '+' side's links first, each side in slot order
    for i, f in enumerate(fields):
        assert f["LN"] == len(want[i]) and f["KC"] == int(kc[i]) and f["km"] == "%.1f" % (int(kc[i]) / (len(want[i]) - k + 1))
    c.close()


# ------------------------------------------------------------------------------------------------ 7. interface
def test_masks_given_or_computed_and_capacities(gkc):
    import torch
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    vals, u, slots = assert_equals_statement(c, k)
    want_offs, want_links = csr(slots)
    nu, nl = len(u["seqs"]), len(want_links)
    assert nl > 0
    # the masks where they lie, at an unaligned address, against the masks computed inside
    t = torch.zeros(len(vals) + 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    assert c.neighbor_masks(d_out=t.data_ptr() + 1) == len(vals)
    given = c.unitig_links(d_masks=t.data_ptr() + 1)
    computed = c.unitig_links()
    assert all(np.array_equal(x, y) for x, y in zip(given, computed))
    assert np.array_equal(given[0], want_offs) and np.array_equal(given[1], want_links)
    # exact room: nothing beyond 2 n_unitigs + 1 offsets / n_links links is touched
    rc, n, o, l = links_raw(c, None, nu, nl, nu + 2, nl + 3)
    assert rc == 0 and n == nl
    assert np.array_equal(o[: (2 * nu + 1) * 8].view(np.uint64), want_offs) and (o[(2 * nu + 1) * 8:] == 0xEE).all()
    assert np.array_equal(l[: nl * 8].view(np.uint64), want_links) and (l[nl * 8:] == 0xEE).all()
    # one link / one unitig too few: GKC_ERR_CAPACITY, *n_links still right, nothing written
    for cap_u, cap_l in ((nu, nl - 1), (nu - 1, nl), (0, 0)):
        rc, n, o, l = links_raw(c, None, cap_u, cap_l, nu + 2, nl + 3)
        assert rc == 4 and n == nl and b"links" in c.L.gkc_last_error(c.h)
        assert (o == 0xEE).all() and (l == 0xEE).all()
    # both pointers NULL: only counts
    rc, n, o, l = links_raw(c, None, 0, 0, nu + 2, nl + 3, offsets=False, links=False)
    assert rc == 0 and n == nl and (o == 0xEE).all() and (l == 0xEE).all()
    c.close()


def test_masks_that_name_a_missing_neighbour_are_reported(gkc):
    """masks that are not those of the results (here: every neighbour claimed): the count follows them, the search misses, GKC_ERR_ARG; the next honest call answers"""
    import torch
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    n = c.stats()["kmers_nb_solid"]
    nu, _, _ = c.unitigs_build()
    forged = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    rc, nl, o, l = links_raw(c, forged.data_ptr(), nu, 8 * nu, nu, 8 * nu)
    assert rc == 1 and nl == 8 * nu and b"d_masks" in c.L.gkc_last_error(c.h)
    assert_equals_statement(c, k)
    c.close()


def test_state_errors_recount_and_empty_results(gkc):
    k, m, parts = 31, 8, 8
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = gkc.Counter(0)
    c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    # before a build
    rc, n, o, l = links_raw(c, None, 1 << 16, 1 << 18, 4, 4)
    assert rc == 1 and n == 0 and b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h)
    assert (o == 0xEE).all() and (l == 0xEE).all()
    _, first, _ = assert_equals_statement(c, k)
    # a recount with another abundance-min: the placement of the first count must not answer
    c.set_solidity(3, INF)
    c.count(bases, offs)
    rc, n, o, l = links_raw(c, None, 1 << 16, 1 << 18, 4, 4)
    assert rc == 1 and b"changed" in c.L.gkc_last_error(c.h) and (o == 0xEE).all() and (l == 0xEE).all()
    _, second, _ = assert_equals_statement(c, k)
    assert len(second["seqs"]) != len(first["seqs"])
    # a count without any solid k-mer
    c.set_solidity(1000000, INF)
    c.count(bases, offs)
    assert c.stats()["kmers_nb_solid"] == 0
    o, l = c.unitig_links()
    assert o.tolist() == [0] and l.shape == (0,)
    rc, n, o, l = links_raw(c, None, 0, 0, 2, 2)
    assert rc == 0 and n == 0 and o[:8].view(np.uint64)[0] == 0 and (o[8:] == 0xEE).all() and (l == 0xEE).all()
    # a released pass: the queries' error
    c.set_solidity(1, INF)
    c.count(bases, offs)
    assert_equals_statement(c, k)
    c.release_pass(0)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*released"):
        c.unitig_links()
    rc, n, o, l = links_raw(c, None, 1 << 16, 1 << 18, 4, 4)
    assert rc == 1 and b"released" in c.L.gkc_last_error(c.h) and (o == 0xEE).all()
    c.close()
