"""Simplification of the compacted graph on the device (csrc/gkc_simplify.hip: gkc_graph_simplify; gkc.Counter.simplify, remove_bulges, remove_erroneous_connections).
Expected values: the statement of tests/test_simplify_cpu.py, which recomputes unitigs and links from scratch over the alive values every round and is pinned there by
the reference's own bubble and EC tests — alive, masks, the log of every round, bases / offsets / KC, the placement of every record and the link CSR, byte for byte.
Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_tips import assert_equals_statement as assert_tips_equal_the_statement, assert_placement, counter_of_reads, plain_graph, upload
from tests.test_gpu_unitigs import GENOME, N_READS, READ_LEN, SUB_PPM, fixture_counter, pack, palindrome_reads
from tests.test_simplify_cpu import (FIXTURES, K, branches_of, bubble_reads, bulges_of, canonical, check_invariants, default_params, fixture_simplify, graph_of, half_z_reads,
                                     hits, one_record_z_reads, only, phases, simplify_np, snp_chain_reads, two_sweep_reads, vectors, z_reads)
from tests.test_tips_cpu import cascade_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def call_args(p, resume=False):
    return dict(max_len_topo=p["max_len_topo"], max_len_rc=p["max_len_rc"], rc_ratio=(p["rc_num"], p["rc_den"]), tip_rounds=p["tip_rounds"], bulge_max_len=p["bulge_max_len"],
                bulge_alt=(p["bulge_alt_num"], p["bulge_alt_den"], p["bulge_alt_add"]), bulge_rounds=p["bulge_rounds"], ec_max_len=p["ec_max_len"],
                ec_ratio=(p["ec_num"], p["ec_den"]), ec_rounds=p["ec_rounds"], max_sweeps=p["max_sweeps"], resume=resume)


def assert_result(c, got, exp):
    assert got["log"] == exp["log"] and got["rounds"] == exp["rounds"] and got["records_removed"] == exp["records_removed"]
    assert got["alive"].dtype == bool and np.array_equal(got["alive"], exp["alive"])
    assert np.array_equal(c.simplified_masks(), exp["masks"])
    assert (got["n_unitigs"], got["n_bases"], got["n_cycles"]) == (len(exp["u"]["seqs"]), len(exp["u"]["bases"]), exp["u"]["n_cycles"])
    assert_placement(c, exp)


def assert_equals_statement(c, k, exp=None, call=None, **over):
    """simplify on the results c holds against the statement over the same records -> (the statement's result, what the call returned)"""
    p = default_params(k, **over)
    if exp is None:
        vals, abund, _ = solid_records(c)
        exp = simplify_np(vals, abund, k, p)
        check_invariants(exp, p)
    got = call() if call else c.simplify(**call_args(p))
    assert_result(c, got, exp)
    return exp, got


def simplify_raw(c, d_masks, d_alive, prm, log=None, cap_log=0):
    out = [C.c_uint64(0xDEAD) for _ in range(5)]
    rc = c.L.gkc_graph_simplify(c.h, d_masks, d_alive, C.byref(prm) if prm is not None else None, log, cap_log, *[C.byref(x) for x in out])
    return rc, [x.value for x in out]


def state_of(c):
    """fresh device copies of the masks of the results c holds and an alive array -> (masks tensor, alive tensor, n)"""
    import torch
    masks = c.neighbor_masks()
    return upload(masks), torch.zeros(max(len(masks), 16), dtype=torch.uint8, device="cuda"), len(masks)


# ------------------------------------------------------------------------------------------------ 1. the reference's own vectors, the fixtures
@pytest.mark.parametrize("name,kind,removed,lengths", [("bubble", "bulges", 21, [633]), ("bubble_snp", "bulges", 21, [633]), ("ec", "ec", 6, [460, 637])])
def test_the_reference_vectors_on_the_device(gkc, name, kind, removed, lengths):
    g = vectors()[name]
    c = counter_of_reads(gkc, g["sequences"], g["k"], 7, parts=4)
    exp, got = assert_equals_statement(c, g["k"])
    assert hits(got) == [(kind, [1, 0])] and got["records_removed"] == removed and g["nodes_after"] == 2 * (got["log"][0][2] - 1)
    bases, offs, kc, lo, links = c.simplified_unitigs()
    text = bases.tobytes().decode()
    seqs = sorted(canonical(text[int(offs[u]): int(offs[u + 1])]) for u in range(got["n_unitigs"]))
    want = g["traversals"][-1:] if name == "bubble_snp" else g["traversals"]
    assert sorted(len(s) for s in seqs) == lengths and seqs == sorted(canonical(t) for t in want) and len(links) == 0
    c.close()


@pytest.mark.parametrize("name", ["k21_freq_4parts", "k63_defaults"])
def test_simplify_equals_the_statement_on_the_fixtures(gkc, name):
    c, k = fixture_counter(gkc, name)
    _, p, exp = fixture_simplify(name)
    _, got = assert_equals_statement(c, k, exp)
    lo = c.simplified_unitigs()[3]
    assert ([h for _, h in phases(got["log"])], got["records_removed"], got["n_unitigs"], int(lo[-1])) == FIXTURES[name]
    c.close()


# ------------------------------------------------------------------------------------------------ 2. constructed shapes
def bubble(records, coverages, seed):
    return lambda: bubble_reads(branches_of(records, coverages, seed=seed), seed=seed)[0]


ONLY_EC = dict(tip_rounds=0, bulge_rounds=0)
SHAPES = {
    # name: (reads, parameters that differ from the defaults, hits of the phases that removed something, records removed, unitigs left)
    "snp_3x_1x": (bubble([K, K], [3, 1], 5), {}, [("bulges", [1, 0])], K, 1),
    "equal_coverage": (bubble([K, K], [2, 2], 6), {}, [("bulges", [1, 0])], K, 1),
    "three_branches": (bubble([K, K, K], [5, 2, 1], 7), {}, [("bulges", [2, 0])], 2 * K, 1),
    "exactly_bulge_max_len": (bubble([101, 101], [3, 1], 8), {}, [("bulges", [1, 0])], 101, 1),
    "one_base_longer": (bubble([102, 102], [3, 1], 8), {}, [], 0, 4),
    "indel_plus_3": (bubble([33, 30], [3, 1], 9), {}, [("bulges", [1, 0])], 30, 1),
    "indel_plus_4": (bubble([34, 30], [3, 1], 9), {}, [], 0, 4),
    "z_equality": (lambda: z_reads(4, 1), ONLY_EC, [], 0, 5),
    "z_one_more": (lambda: z_reads(4, 1, extra=1), ONLY_EC, [("ec", [1, 0])], 30, 2),
    "z_too_long": (lambda: z_reads(4, 1, extra=1), dict(ONLY_EC, ec_max_len=30 + K - 2), [], 0, 5),
    "half_z": (half_z_reads, ONLY_EC, [], 0, 5),
    "one_record_ec": (lambda: one_record_z_reads(5), ONLY_EC, [("ec", [1, 0])], 1, 2),
    "one_record_ec_equality": (lambda: one_record_z_reads(4), ONLY_EC, [], 0, 5),
    "two_sweeps": (lambda: two_sweep_reads()[0], {}, [("bulges", [1, 0]), ("tips", [1, 0]), ("bulges", [1, 0])], 194, 1),
    "two_sweeps_capped": (lambda: two_sweep_reads()[0], dict(max_sweeps=1), [("bulges", [1, 0]), ("tips", [1, 0])], 134, 4),
    "no_sweep": (bubble([K, K, K], [5, 2, 1], 7), dict(max_sweeps=0), [], 0, 5),
    "one_bulge_round": (bubble([K, K, K], [5, 2, 1], 7), dict(bulge_rounds=1), [("bulges", [2])], 2 * K, 1),
    "one_bulge_round_one_sweep": (bubble([K, K, K], [5, 2, 1], 7), dict(bulge_rounds=1, max_sweeps=1), [("bulges", [2])], 2 * K, 1),
    "no_rounds_at_all": (bubble([K, K, K], [5, 2, 1], 7), dict(tip_rounds=0, bulge_rounds=0, ec_rounds=0), [], 0, 5),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_constructed_shapes(gkc, shape):
    reads, over, want_hits, removed, left = SHAPES[shape]
    c = counter_of_reads(gkc, reads())
    before_masks = c.neighbor_masks()
    exp, got = assert_equals_statement(c, K, **over)
    assert hits(got) == want_hits and got["n_unitigs"] == left and got["records_removed"] == removed
    if shape == "no_rounds_at_all":                             # nothing done: the masks as they were, everything alive, no round in the log
        assert got["log"] == [] and got["alive"].all() and np.array_equal(c.simplified_masks(), before_masks)
    if shape == "no_sweep":
        assert got["log"] == [("tips", 0, 5, 0, 0)]
    c.close()


def test_300_bulges_in_one_round(gkc):
    """more hits than a 256-thread block, partial waves, and work lists on both sides: every stretch of the main sequence between two bubbles has a bulge at either end"""
    reads, main = snp_chain_reads(300, seed=3)
    c = counter_of_reads(gkc, reads, parts=4)
    vals, abund, _ = solid_records(c)
    idx, u, slots = graph_of(vals, abund, np.ones(len(vals), bool), K)
    flagged = set(bulges_of(u, slots, K, default_params(K)))
    assert len(flagged) == 300 and len(u["seqs"]) == 2 * 300 + 301
    for side in (0, 1):
        assert any(t >> 1 not in flagged and any(e >> 1 in flagged for e in s) for t, s in enumerate(slots) if t & 1 == side)
    exp, got = assert_equals_statement(c, K, max_sweeps=1)
    assert hits(got) == [("bulges", [300, 0])] and got["records_removed"] == 300 * K and got["n_unitigs"] == 1
    assert canonical(c.simplified_unitigs()[0].tobytes().decode()) == canonical(main)
    c.close()


def test_an_even_k_against_the_statement(gkc):
    k, m, parts = 32, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes() for i in range(N_READS)] + palindrome_reads(np.random.default_rng(k), k)
    bases, offs = pack(reads)
    c = counter_for(gkc, bases, offs, k, m, parts)
    exp, got = assert_equals_statement(c, k, max_sweeps=2)
    print("k = 32: %s, %d records removed, %d unitigs left" % (hits(got), got["records_removed"], got["n_unitigs"]))
    assert got["records_removed"] > 0
    c.close()


# ------------------------------------------------------------------------------------------------ 3. each kind alone, resume
def test_each_kind_alone(gkc):
    c = counter_of_reads(gkc, bubble([K, K, K], [5, 2, 1], 7)())
    exp, got = assert_equals_statement(c, K, call=c.remove_bulges, **only("bulges", K))
    assert got["log"] == [("bulges", 1, 5, 2, 2 * K), ("bulges", 1, 1, 0, 0), ("bulges", 2, 1, 0, 0)]
    c.close()
    c = counter_of_reads(gkc, z_reads(4, 1, extra=1))
    exp, got = assert_equals_statement(c, K, call=c.remove_erroneous_connections, **only("ec", K))
    assert got["log"] == [("ec", 1, 5, 1, 30), ("ec", 1, 2, 0, 0), ("ec", 2, 2, 0, 0)]
    exp, got = assert_equals_statement(c, K, call=lambda: c.remove_erroneous_connections(ec_ratio=(5, 1)), **only("ec", K, ec_num=5))
    assert hits(got) == [] and got["alive"].all()
    c.close()


def test_resume_after_remove_tips(gkc):
    name = "k21_freq_4parts"
    c, k = fixture_counter(gkc, name)
    _, p, full = fixture_simplify(name)
    tips = c.remove_tips()
    assert tips["tips_per_round"] == [200, 0]
    got = c.simplify(resume=True)
    want = dict(full, log=[("tips", 0, 312, 0, 0)] + full["log"][2:], rounds=full["rounds"] - 1, records_removed=full["records_removed"] - tips["records_removed"])
    assert_result(c, got, want)
    got = c.remove_bulges(resume=True)                          # once more on the final state: nothing to do, nothing changes
    assert got["log"] == [("bulges", 1, 40, 0, 0)] and got["records_removed"] == 0
    assert_result(c, dict(got, log=want["log"], rounds=want["rounds"], records_removed=want["records_removed"]), want)
    c.close()


def test_resume_with_masks_that_name_a_dead_record(gkc):
    c = counter_of_reads(gkc, cascade_reads())
    full = c.neighbor_masks()
    tips = c.remove_tips(max_len_rc=0)
    assert tips["records_removed"] == 35
    alive = tips["alive"]
    prm = c.simplify_params(resume=True)
    stale = np.where(alive, full, 0).astype(np.uint8)           # dead records have no mask, but the junctions still name them
    assert not np.array_equal(stale, c.simplified_masks())
    tm, ta = upload(stale), upload(alive.astype(np.uint8))
    rc, out = simplify_raw(c, tm.data_ptr(), ta.data_ptr(), prm)
    assert rc == 1 and b"d_masks name a neighbour" in c.L.gkc_last_error(c.h)
    tm = upload(full)                                           # a dead record with a mask: not a state a call left
    rc, out = simplify_raw(c, tm.data_ptr(), ta.data_ptr(), prm)
    assert rc == 1 and b"dead record" in c.L.gkc_last_error(c.h)
    assert_tips_equal_the_statement(c, K, max_len_rc=0)         # the honest call answers afterwards
    c.close()


# ------------------------------------------------------------------------------------------------ 4. errors, the log, no records, the builds
def test_argument_errors(gkc):
    c = counter_of_reads(gkc, bubble([K, K], [3, 1], 5)())
    before = plain_graph(c)
    tm, ta, n = state_of(c)
    ok = c.simplify_params()
    cases = [(None, ta.data_ptr(), ok, b"masks"), (tm.data_ptr(), None, ok, b"alive"), (tm.data_ptr(), ta.data_ptr(), None, b"parameters")]
    for field, what in (("bulge_alt_den", b"bulge_alt_den"), ("ec_den", b"ec_den"), ("bulge_max_rounds", b"max_rounds"), ("ec_max_rounds", b"max_rounds"), ("max_sweeps", b"max_sweeps")):
        prm = c.simplify_params()
        setattr(prm, field, 0 if field.endswith("den") else 17 if field == "max_sweeps" else 65)
        cases.append((tm.data_ptr(), ta.data_ptr(), prm, what))
    prm = c.simplify_params(rc_ratio=(2, 0)); cases.append((tm.data_ptr(), ta.data_ptr(), prm, b"rc_den"))
    prm = c.simplify_params(tip_rounds=65); cases.append((tm.data_ptr(), ta.data_ptr(), prm, b"max_rounds"))
    for d_masks, d_alive, prm, what in cases:
        rc, out = simplify_raw(c, d_masks, d_alive, prm)
        assert rc == 1 and out == [0, 0, 0, 0, 0] and what in c.L.gkc_last_error(c.h), what
    assert gkc.lib().gkc_graph_simplify(None, tm.data_ptr(), ta.data_ptr(), C.byref(ok), None, 0, None, None, None, None, None) == 1
    with pytest.raises(gkc.GkcError, match="gkc error 1"):
        c.simplify(ec_ratio=(4, 0))
    with pytest.raises(gkc.GkcError, match="gkc error 1"):
        c.remove_bulges(max_rounds=65)
    with pytest.raises(gkc.GkcError, match="remove_tips"):
        c.simplify(resume=True)                                 # no state to resume
    ok.max_sweeps = 16; ok.bulge_max_rounds = 64                # the limits themselves are served
    rc, out = simplify_raw(c, tm.data_ptr(), ta.data_ptr(), ok)
    assert rc == 0 and out == [8, K, 1, 2 * 300 + 1, 0]
    assert all(np.array_equal(a, b) for a, b in zip(plain_graph(c), before))
    c.close()


def test_a_log_smaller_than_the_rounds(gkc):
    c = counter_of_reads(gkc, two_sweep_reads()[0])
    exp, got = assert_equals_statement(c, K)
    assert got["rounds"] == 13
    tm, ta, n = state_of(c)
    log = (gkc.SimplifyRound * 6)()
    for e in log:
        e.kind, e.sweep, e.n_unitigs, e.n_hits, e.n_records_removed = 77, 77, 77, 77, 77
    rc, out = simplify_raw(c, tm.data_ptr(), ta.data_ptr(), c.simplify_params(), log, 4)
    assert rc == 0 and out[0] == 13 and out[1] == exp["records_removed"]
    assert [(gkc.SIMPLIFY_KINDS[e.kind], e.sweep, e.n_unitigs, e.n_hits, e.n_records_removed) for e in log[:4]] == exp["log"][:4]
    assert all((e.kind, e.sweep, e.n_unitigs, e.n_hits, e.n_records_removed) == (77,) * 5 for e in log[4:])
    rc, out = simplify_raw(c, tm.data_ptr(), ta.data_ptr(), c.simplify_params(resume=True), None, 0)      # no log at all, on the state the call left
    assert rc == 0 and out[:3] == [4, 0, 1]
    c.close()


def test_no_solid_kmer_at_all(gkc):
    bases, offs = pack(bubble([K, K], [3, 1], 5)())
    c = counter_for(gkc, bases, offs, K, 7, 4, amin=1000)
    assert c.stats()["kmers_nb_solid"] == 0
    got = c.simplify()
    assert (got["records_removed"], got["n_unitigs"], got["n_bases"], got["n_cycles"]) == (0, 0, 0, 0) and got["alive"].shape == (0,)
    assert got["log"] == [("tips", 0, 0, 0, 0), ("bulges", 1, 0, 0, 0), ("ec", 1, 0, 0, 0), ("tips", 1, 0, 0, 0)] == simplify_np([], [], K, default_params(K))["log"]
    bases, offs, kc, lo, links = c.simplified_unitigs()
    assert offs.tolist() == [0] and lo.tolist() == [0]
    c.close()


@pytest.mark.parametrize("shape,over", [("two_sweeps", {}), ("two_sweeps", dict(max_sweeps=1)), ("one_base_longer", {}), ("three_branches", dict(bulge_rounds=1, max_sweeps=1)),
                                        ("three_branches", dict(tip_rounds=0, bulge_rounds=0, ec_rounds=0))])
def test_one_build_per_round_that_removed_something_and_one_more(gkc, shape, over):
    c = counter_of_reads(gkc, SHAPES[shape][0]())
    c.unitigs_build()                                           # (the index and the first timing entries exist)
    t0 = {name: c.timing(name)[1] for name in ("graph_links", "graph_tips", "graph_bulges", "graph_ec")}
    got = c.simplify(**call_args(default_params(K, **over)))
    t1 = {name: c.timing(name)[1] for name in t0}
    log = got["log"]
    assert t1["graph_links"] - t0["graph_links"] == sum(1 for e in log if e[3]) + 1
    for kind, name in (("tips", "graph_tips"), ("bulges", "graph_bulges"), ("ec", "graph_ec")):
        assert t1[name] - t0[name] == sum(1 for e in log if e[0] == kind)
    c.close()


def test_remove_tips_afterwards_still_gives_the_tips_result(gkc):
    c = counter_of_reads(gkc, two_sweep_reads()[0] + cascade_reads())
    exp, got = assert_equals_statement(c, K)
    assert got["records_removed"] > 35
    tips_exp, tips_got = assert_tips_equal_the_statement(c, K, max_len_rc=0)
    assert tips_got["tips_per_round"] == [4, 2, 1, 0]
    c.close()
