"""Tip removal on the device (csrc/gkc_simplify.hip: gkc_graph_tips_remove; csrc/gkc_unitigs.hip: gkc_graph_unitigs_build_alive; gkc.Counter.remove_tips, simplified_unitigs).
Expected values: the statement of tests/test_tips_cpu.py, which recomputes unitigs and links from scratch over the alive values every round and is pinned there by the
reference's own tip test — alive, masks, tips per round, bases / offsets / KC, the placement of every record and the link CSR, byte for byte.
Run with `pytest -m gpu`."""
import ctypes as C
import json

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_unitigs import CASES, GENOME, N_READS, READ_LEN, SUB_PPM, case_id, fixture_counter, pack, palindrome_reads
from tests.test_query_cpu import INF, freq_order_of
from tests.test_graph_cpu import revcomp
from tests.test_tips_cpu import (FIXTURES, GOLDEN, K, canonical, cascade_reads, check_invariants, circle_read, coverage_reads, cycle_with_tip_reads, default_params,
                                 fixture_tips, main_and_branches, tips_np, y_reads)
from tests.test_unitig_links_cpu import csr, hairpin_reads, parse_unitigs_fasta, random_sequence, slots_of, star_reads
from tests.test_unitigs_cpu import circle, split_sequences, unitigs_np
from tests.test_unitig_links_cpu import unitig_links_np
from tests.util import str2int

pytestmark = pytest.mark.gpu
TILE = 1024                                                         # records / slots per tile (GR_TILE of csrc/gkc_graph.hpp)
DEAD = np.uint64((1 << 64) - 1)


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def call_args(params):
    return dict(max_len_topo=params["max_len_topo"], max_len_rc=params["max_len_rc"], rc_ratio=(params["rc_num"], params["rc_den"]), max_rounds=params["max_rounds"])


def assert_placement(c, exp):
    """the placement and the graph the context holds against the statement's final graph exp (tips_np): every array byte for byte"""
    u = exp["u"]
    bases, offs, kc, lo, links = c.simplified_unitigs()
    assert bases.dtype == np.uint8 and offs.dtype == np.uint64 and kc.dtype == np.uint64 and lo.dtype == np.uint64 and links.dtype == np.uint64
    assert np.array_equal(offs, u["offsets"]) and np.array_equal(bases, u["bases"]) and np.array_equal(kc, u["kc"])
    un, rev, pos = c.unitig_of_records()
    want = np.where(exp["unitig"] < 0, DEAD, exp["unitig"].astype(np.uint64))
    assert np.array_equal(un, want) and np.array_equal(rev, exp["reversed"]) and np.array_equal(pos.astype(np.int64), exp["pos"])
    want_lo, want_links = csr(exp["slots"])
    assert np.array_equal(lo, want_lo) and np.array_equal(links, want_links)


def assert_equals_statement(c, k, exp=None, **over):
    """remove_tips on the results c holds against the statement over the same records -> (the statement's result, what remove_tips returned)"""
    params = default_params(k, **over)
    if exp is None:
        vals, abund, _ = solid_records(c)
        exp = tips_np(vals, abund, k, params)
        check_invariants(exp, params)
    got = c.remove_tips(**call_args(params))
    assert got["tips_per_round"] == exp["tips_per_round"] and got["rounds"] == exp["rounds"] and got["records_removed"] == exp["records_removed"]
    assert got["alive"].dtype == bool and np.array_equal(got["alive"], exp["alive"])
    assert np.array_equal(c.simplified_masks(), exp["masks"])
    assert (got["n_unitigs"], got["n_bases"], got["n_cycles"]) == (len(exp["u"]["seqs"]), len(exp["u"]["bases"]), exp["u"]["n_cycles"])
    assert_placement(c, exp)
    return exp, got


def counter_of_reads(gkc, reads, k=K, m=7, parts=1, passes=1):
    bases, offs = pack(reads)
    return counter_for(gkc, bases, offs, k, m, parts, passes)


def upload(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() if len(a) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def tips_raw(c, d_masks, d_alive, prm, per_round=None):
    out = [C.c_uint64(0xDEAD) for _ in range(5)]
    rc = c.L.gkc_graph_tips_remove(c.h, d_masks, d_alive, C.byref(prm) if prm is not None else None, C.byref(out[0]), per_round, *[C.byref(x) for x in out[1:]])
    return rc, [x.value for x in out]


def plain_graph(c):
    return c.unitigs() + c.unitig_of_records() + c.unitig_links()


# ------------------------------------------------------------------------------------------------ 1. the reference's own tip, the fixtures
def test_the_reference_tip_vector_on_the_device(gkc):
    g = json.load(open(GOLDEN))
    c = counter_of_reads(gkc, g["sequences"], g["k"], 7, parts=4)
    exp, got = assert_equals_statement(c, g["k"], max_len_rc=0)
    assert got["tips_per_round"] == [1, 0] and got["records_removed"] == 7 and got["n_unitigs"] == 1
    bases, offs, kc, lo, links = c.simplified_unitigs()
    assert canonical(bases.tobytes().decode()) == canonical(g["traversal"]) and lo.tolist() == [0, 0, 0]
    c.close()


@pytest.mark.parametrize("name", ["k21_freq_4parts", "k63_defaults"])
@pytest.mark.parametrize("coverage", [True, False], ids=["default", "topological"])
def test_tips_equal_the_statement_on_the_fixtures(gkc, name, coverage):
    c, k = fixture_counter(gkc, name)
    _, params, exp = fixture_tips(name, coverage)
    over = {} if coverage else dict(max_len_rc=0)
    _, got = assert_equals_statement(c, k, exp, **over)
    assert (got["tips_per_round"], got["records_removed"], got["n_unitigs"]) == FIXTURES[name][0 if coverage else 1][:3]
    c.close()


# ------------------------------------------------------------------------------------------------ 2. constructed shapes
def isolated_reads():
    return [random_sequence(np.random.default_rng(4), 25), circle_read(circle(K, 40)[0], K)]


SHAPES = {
    # name: (reads, parameters that differ from the defaults, tips per round, records removed, unitigs left)
    "exactly_max_len_topo": (lambda: main_and_branches([32], seed=1)[0], dict(max_len_rc=0), [1, 0], 32, 1),
    "one_base_longer": (lambda: main_and_branches([33], seed=1)[0], dict(max_len_rc=0), [0], 0, 3),
    "one_record_tip": (lambda: main_and_branches([1], seed=2)[0], dict(max_len_rc=0), [1, 0], 1, 1),
    "two_tips_one_junction": (lambda: main_and_branches([5, 9], seed=3)[0], dict(max_len_rc=0), [2, 0], 14, 1),
    "y_vanishes": (y_reads, dict(max_len_rc=0), [3, 0], 17, 0),
    "tip_on_a_cycle": (lambda: cycle_with_tip_reads()[0], dict(max_len_rc=0), [1, 0], 5, 1),
    "hairpin": (hairpin_reads, dict(max_len_rc=0), [1, 0], 31, 0),
    "hairpin_stays": (hairpin_reads, dict(max_len_rc=0, max_len_topo=50), [0], 0, 1),
    "star_vanishes": (star_reads, dict(max_len_rc=0), [5, 0], 134, 0),
    "star_stem": (star_reads, dict(max_len_rc=0, max_len_topo=40), [1, 0], 10, 4),
    "star_coverage_equal": (lambda: star_reads() + [star_reads()[3][10:]] * 7, dict(max_len_topo=0, max_len_rc=40), [0], 0, 5),
    "star_coverage_more": (lambda: star_reads() + [star_reads()[3][10:]] * 8, dict(max_len_topo=0, max_len_rc=40), [1, 0], 10, 4),
    "isolated_stay": (isolated_reads, {}, [0], 0, 2),
    "coverage_equality": (lambda: coverage_reads(6, 6, 3), dict(max_len_topo=0, max_len_rc=100), [0], 0, 3),
    "coverage_one_more": (lambda: coverage_reads(6, 6, 3, extra_right=1), dict(max_len_topo=0, max_len_rc=100), [1, 0], 40, 1),
    "competitor_arrival": (lambda: coverage_reads(7, 1, 3), dict(max_len_topo=0, max_len_rc=100), [1, 0], 40, 1),
    "competitor_sibling": (lambda: coverage_reads(1, 7, 3), dict(max_len_topo=0, max_len_rc=100), [1, 0], 40, 1),
    "competitor_neither": (lambda: coverage_reads(5, 5, 3), dict(max_len_topo=0, max_len_rc=100), [0], 0, 3),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_constructed_shapes(gkc, shape):
    reads, over, per_round, removed, left = SHAPES[shape]
    c = counter_of_reads(gkc, reads())
    exp, got = assert_equals_statement(c, K, **over)
    assert (got["tips_per_round"], got["records_removed"], got["n_unitigs"]) == (per_round, removed, left)
    if left == 0:                                               # nothing alive: every call answers, with nothing
        assert not got["alive"].any() and got["n_bases"] == 0
        bases, offs, kc, lo, links = c.simplified_unitigs()
        assert offs.tolist() == [0] and lo.tolist() == [0] and bases.shape == kc.shape == links.shape == (0,)
        nl = C.c_uint64(7)
        assert c.L.gkc_graph_unitigs_links(c.h, c._tips["masks"].data_ptr(), None, 0, None, 0, C.byref(nl)) == 0 and nl.value == 0
    c.close()


@pytest.mark.parametrize("max_rounds,per_round,n_unitigs,removed", [(0, [], 9, 0), (1, [4], 5, 20), (2, [4, 2], 3, 30), (3, [4, 2, 1], 1, 35), (20, [4, 2, 1, 0], 1, 35)])
def test_a_cascade_stops_at_max_rounds(gkc, max_rounds, per_round, n_unitigs, removed):
    c = counter_of_reads(gkc, cascade_reads())
    before_masks = c.neighbor_masks()
    before = plain_graph(c)
    exp, got = assert_equals_statement(c, K, max_len_rc=0, max_rounds=max_rounds)
    assert (got["tips_per_round"], got["n_unitigs"], got["records_removed"]) == (per_round, n_unitigs, removed)
    if max_rounds == 0:                                         # nothing done: the masks as they were, everything alive, the placement of the plain build
        assert got["alive"].all() and np.array_equal(c.simplified_masks(), before_masks)
        bases, offs, kc, lo, links = c.simplified_unitigs()
        un, rev, pos = c.unitig_of_records()
        for a, b in zip((bases, offs, kc, un, rev, pos, lo, links), before):
            assert np.array_equal(a, b)
    after = plain_graph(c)                                      # the plain build afterwards: the full graph again, byte for byte
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    c.close()


# ------------------------------------------------------------------------------------------------ 3. synthetic reads with substitution errors: tips across datasets
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tips_against_the_statement(gkc, case):
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
    exp, got = assert_equals_statement(c, k)
    print("%s: tips per round %s, %d records removed, %d unitigs left" % (case_id(case), got["tips_per_round"], got["records_removed"], got["n_unitigs"]))
    assert got["tips_per_round"][0] > 0
    c.close()


# ------------------------------------------------------------------------------------------------ 4. the borders of the tiles
def forks_and_paths(n_alive, n_unitigs, n_forks, k, seed):
    """n_forks disjoint forks of three arms of three records (every arm a tip: the fork vanishes in round 1) and n_unitigs isolated paths of n_alive records together
    (two records each, some lengthened or shortened by one), which stay -> reads"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_forks):
        lead = random_sequence(rng, k - 1)
        reads += [lead + "A" + random_sequence(rng, 2), lead + "C" + random_sequence(rng, 2), random_sequence(rng, 3) + lead]
    lens = [2] * n_unitigs
    diff = n_alive - 2 * n_unitigs
    for i in range(abs(diff)):
        lens[i] += 1 if diff > 0 else -1
    assert sum(lens) == n_alive and min(lens) >= 1
    reads += [random_sequence(rng, k - 1 + L) for L in lens]
    return reads, 9 * n_forks


def records_by_construction(reads, n_fork_reads, k):
    """-> (values ascending, alive after round 1 as the construction means it: the k-mers of the fork reads die)"""
    def kmers(rs):
        return {min(x, revcomp(x, k)) for r in rs for x in (str2int(r[i: i + k]) for i in range(len(r) - k + 1))}
    dead = kmers(reads[:n_fork_reads])
    vals = sorted(dead | kmers(reads[n_fork_reads:]))
    return vals, np.array([v not in dead for v in vals])


@pytest.mark.parametrize("n_alive,n_unitigs", [(TILE - 1, TILE // 2 + 1), (TILE, TILE // 2), (TILE + 1, TILE // 2 - 1)], ids=["T-1", "T", "T+1"])
def test_alive_counts_around_the_tile(gkc, n_alive, n_unitigs):
    k, m, n_forks = 31, 8, 120                                   # 1080 dead records: 2100 and some records, three tiles
    for seed in range(400):                                     # an input whose LAST records are dead and that has a dead record on each side of the first tile border
        reads, n_dead = forks_and_paths(n_alive, n_unitigs, n_forks, k, 1000 * n_alive + seed)
        vals, alive = records_by_construction(reads, 3 * n_forks, k)
        if len(vals) == n_alive + n_dead and not alive[-2:].any() and not alive[TILE - 1] and not alive[TILE]:
            break
    else:
        raise AssertionError("no such input found")
    c = counter_of_reads(gkc, reads, k, m, parts=1)
    exp, got = assert_equals_statement(c, k, max_len_rc=0)
    assert got["tips_per_round"] == [3 * n_forks, 0] and got["records_removed"] == n_dead
    assert np.array_equal(got["alive"], alive) and int(got["alive"].sum()) == n_alive and got["n_unitigs"] == n_unitigs
    c.close()


# ------------------------------------------------------------------------------------------------ 5. gkc_graph_unitigs_build_alive directly
def build_alive(c, masks, alive):
    tm, ta = upload(masks), upload(alive.astype(np.uint8))
    nu, nb, nc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = c.L.gkc_graph_unitigs_build_alive(c.h, tm.data_ptr(), ta.data_ptr(), C.byref(nu), C.byref(nb), C.byref(nc))
    return rc, nu.value, nb.value, nc.value, tm


def written(c, nu, nb, d_masks):
    import torch
    bases = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda"); offs = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); kc = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert c.L.gkc_graph_unitigs_write(c.h, bases.data_ptr(), nb, offs.data_ptr(), nu, kc.data_ptr()) == 0
    lo, links = c._unitig_links_of_placement(nu, d_masks)
    return (bases[:nb].cpu().numpy(), offs.cpu().numpy().view(np.uint64), kc[:nu].cpu().numpy().view(np.uint64)) + c.unitig_of_records() + \
           (lo.cpu().numpy().view(np.uint64), links.cpu().numpy().view(np.uint64))


def test_build_alive_with_everything_alive_is_the_plain_build(gkc):
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    masks = c.neighbor_masks()
    before = plain_graph(c)
    rc, nu, nb, nc, tm = build_alive(c, masks, np.ones(len(masks), bool))
    assert rc == 0 and (nu, nb) == (len(before[2]), len(before[0]))
    got = written(c, nu, nb, tm.data_ptr())
    assert all(np.array_equal(a, b) for a, b in zip(got, before))
    c.close()


def test_build_alive_over_a_hand_made_dead_set(gkc):
    from tests.test_graph_cpu import graph_masks_np
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts, passes=2)
    vals, abund, _ = solid_records(c)
    rng = np.random.default_rng(8)
    alive = rng.random(len(vals)) < 0.8
    alive[-3:] = False; alive[TILE - 1: TILE + 1] = False
    idx = np.flatnonzero(alive)
    sub = [vals[i] for i in idx]
    masks = np.zeros(len(vals), np.uint8); masks[idx] = graph_masks_np(sub, k)
    u = unitigs_np(sub, [abund[i] for i in idx], k)
    slots = unitig_links_np(sub, k, u)
    rc, nu, nb, nc, tm = build_alive(c, masks, alive)
    assert rc == 0 and (nu, nb, nc) == (len(u["seqs"]), len(sub) + (k - 1) * len(u["seqs"]), u["n_cycles"])
    b, o, kc, un, rev, pos, lo, links = written(c, nu, nb, tm.data_ptr())
    assert np.array_equal(b, u["bases"]) and np.array_equal(o, u["offsets"]) and np.array_equal(kc, u["kc"])
    assert (un[~alive] == DEAD).all() and not rev[~alive].any() and not pos[~alive].any()
    assert np.array_equal(un[idx].astype(np.int64), u["unitig"]) and np.array_equal(rev[idx], u["reversed"]) and np.array_equal(pos[idx].astype(np.int64), u["pos"])
    want_lo, want_links = csr(slots)
    assert np.array_equal(lo, want_lo) and np.array_equal(links, want_links)
    nl = C.c_uint64()
    assert c.L.gkc_graph_unitigs_links(c.h, None, None, 0, None, 0, C.byref(nl)) == 1 and b"alive" in c.L.gkc_last_error(c.h)      # the library cannot recompute edited masks
    # nothing alive
    rc, nu, nb, nc, tm = build_alive(c, np.zeros(len(vals), np.uint8), np.zeros(len(vals), bool))
    assert (rc, nu, nb, nc) == (0, 0, 0, 0)
    b, o, kc, un, rev, pos, lo, links = written(c, 0, 0, tm.data_ptr())
    assert o.tolist() == [0] and lo.tolist() == [0] and (un == DEAD).all() and len(un) == len(vals)
    c.close()


# ------------------------------------------------------------------------------------------------ 6. errors and state
def test_argument_errors(gkc):
    import torch
    c = counter_of_reads(gkc, cascade_reads())
    n = c.stats()["kmers_nb_solid"]
    before = plain_graph(c)
    tm, ta = upload(c.neighbor_masks()), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = gkc.TipParams(52, 0, 2, 1, 20)
    for d_masks, d_alive, prm, what in ((None, ta.data_ptr(), ok, b"masks"), (tm.data_ptr(), ta.data_ptr(), gkc.TipParams(52, 210, 2, 0, 20), b"rc_den"),
                                        (tm.data_ptr(), ta.data_ptr(), gkc.TipParams(52, 0, 2, 1, 65), b"max_rounds")):
        rc, out = tips_raw(c, d_masks, d_alive, prm)
        assert rc == 1 and out == [0, 0, 0, 0, 0] and what in c.L.gkc_last_error(c.h)
    with pytest.raises(gkc.GkcError, match="gkc error 1"):
        c.remove_tips(rc_ratio=(2, 0))
    with pytest.raises(gkc.GkcError, match="gkc error 1"):
        c.remove_tips(max_rounds=65)
    rc, out = tips_raw(c, tm.data_ptr(), ta.data_ptr(), ok)      # the honest call answers
    assert rc == 0 and out == [4, 35, 1, 300, 0]
    nl = C.c_uint64()
    assert c.L.gkc_graph_unitigs_links(c.h, None, None, 0, None, 0, C.byref(nl)) == 1      # a subset placement: the masks are required
    assert all(np.array_equal(a, b) for a, b in zip(plain_graph(c), before))
    c.close()


def test_masks_that_name_a_missing_neighbour_are_reported(gkc):
    import torch
    c = counter_of_reads(gkc, cascade_reads())
    n = c.stats()["kmers_nb_solid"]
    forged = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"); ta = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, out = tips_raw(c, forged.data_ptr(), ta.data_ptr(), gkc.TipParams(52, 0, 2, 1, 20))
    assert rc == 1 and b"d_masks" in c.L.gkc_last_error(c.h)
    assert_equals_statement(c, K, max_len_rc=0)
    c.close()


def test_a_recount_invalidates_the_placement(gkc):
    k, m, parts = 31, 8, 8
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    first, _ = assert_equals_statement(c, k)
    kept = c._tips["masks"]
    c.set_solidity(3, INF)
    c.count(bases, offs)
    with pytest.raises(gkc.GkcError, match="remove_tips"):
        c.simplified_unitigs()
    nl = C.c_uint64()
    assert c.L.gkc_graph_unitigs_links(c.h, kept.data_ptr(), None, 0, None, 0, C.byref(nl)) == 1 and b"changed" in c.L.gkc_last_error(c.h)
    second, _ = assert_equals_statement(c, k)
    assert second["records_removed"] != first["records_removed"]
    c.close()


# ------------------------------------------------------------------------------------------------ 7. the FASTA of the simplified graph
def test_simplified_fasta_parsed_back(gkc, tmp_path):
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    got = c.remove_tips()
    assert got["records_removed"] > 0
    ub, uo, kc, lo, links = c.simplified_unitigs()
    path = str(tmp_path / "simplified.unitigs.fa")
    nu, nl = c.write_unitigs_fasta(path, simplified=True)
    ids, fields, seqs, slots = parse_unitigs_fasta(path)
    want = [s.decode() for s in split_sequences(ub, uo)]
    assert (nu, nl) == (len(want), len(links)) == (got["n_unitigs"], len(links)) and nl > 0
    assert ids == list(range(nu)) and seqs == want and slots == slots_of(lo, links)
    for i, f in enumerate(fields):
        assert f["LN"] == len(want[i]) and f["KC"] == int(kc[i])
    full = str(tmp_path / "full.unitigs.fa")                     # without the flag: the full graph, as before
    nu_full, _ = c.write_unitigs_fasta(full)
    assert nu_full > nu
    c.close()
