"""Tip removal on the compacted graph (include/gkc.h, "tips"; gkc_graph_tips_remove, gkc_graph_unitigs_build_alive), the part that needs no GPU: a plain Python
statement of the definition that recomputes the unitigs and links of the alive records FROM SCRATCH every round (unitigs_np / unitig_links_np over the alive values),
so it shares nothing with the device code, which threads an alive array through one placement. The reference's own known answer (tests/golden/reference_tip_vector.json,
written by tools/make_tip_vector.py from its unit test debruijn_simplunitigs_tip) pins the topological rule. tests/test_gpu_tips.py imports the statement."""
import collections
import functools
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_graph_cpu import graph_masks_np, revcomp
from tests.test_reference_run import DIR, load
from tests.test_unitig_links_cpu import assert_symmetric, hairpin_reads, random_sequence, rc_str, star_reads, unitig_links_np
from tests.test_unitigs_cpu import circle, unitigs_np
from tests.util import str2int

NAMES = ["gkc_graph_tips_remove", "gkc_graph_unitigs_build_alive"]
GOLDEN = os.path.join(os.path.dirname(DIR), "reference_tip_vector.json")


# ------------------------------------------------------------------------------------------------ the statement
def default_params(k, **over):
    """the reference's constants (Simplifications.cpp: tips up to 2.5 k bases topologically, up to 10 k with the coverage rule, ratio 2)"""
    p = dict(max_len_topo=(5 * k) // 2, max_len_rc=10 * k, rc_num=2, rc_den=1, max_rounds=20)
    p.update(over)
    return p


def tips_of(u, slots, k, params):
    """the definition of one round: u = unitigs_np of the alive records, slots = their links -> the sorted list of the unitigs that are tips"""
    lens = [len(s) - k + 1 for s in u["seqs"]]
    kc = [int(x) for x in u["kc"]]
    tips = []
    for un in range(len(lens)):
        d = [len(slots[2 * un]), len(slots[2 * un + 1])]
        if (d[0] == 0) == (d[1] == 0):                          # isolated, or linked on both sides: no candidate
            continue
        su = 0 if d[0] else 1
        bases = lens[un] + k - 1
        tip = bases <= params["max_len_topo"]
        if not tip and bases <= params["max_len_rc"]:
            for e in slots[2 * un + su]:
                v, m = e >> 1, e & 1
                back = list(slots[2 * v + (1 - m)])
                if (un << 1 | (1 - su)) in back:
                    back.remove(un << 1 | (1 - su))             # the one entry that is u coming back
                for c in [v] + [w >> 1 for w in back]:
                    if kc[c] * lens[un] * params["rc_den"] > params["rc_num"] * kc[un] * lens[c]:
                        tip = True
        if tip:
            tips.append(un)
    return tips


def tips_np(values, abundances, k, params):
    """-> dict: alive bool[n], masks uint8[n] (0 for dead records), tips_per_round (the last, empty round included when it ran), rounds, records_removed, and the
    final graph: u = unitigs_np over the alive values, slots = unitig_links_np over them, unitig / reversed / pos per record of the FULL flat order (unitig -1: dead),
    stopped_by_max_rounds, graphs = (n_unitigs, n_links) at the start of every round"""
    vals = [int(v) for v in values]; ab = [int(a) for a in abundances]
    n = len(vals)
    alive = np.ones(n, bool)
    per_round, graphs = [], []
    u = slots = idx = None
    fresh = False                                               # u / slots describe the alive set as it is now
    for _ in range(params["max_rounds"]):
        idx = np.flatnonzero(alive)
        sub = [vals[i] for i in idx]
        u = unitigs_np(sub, [ab[i] for i in idx], k)
        slots = unitig_links_np(sub, k, u)
        graphs.append((len(u["seqs"]), sum(len(s) for s in slots)))
        tips = tips_of(u, slots, k, params)
        per_round.append(len(tips))
        fresh = not tips
        if not tips:
            break
        alive[idx[np.isin(u["unitig"], tips)]] = False
    if not fresh:
        idx = np.flatnonzero(alive)
        sub = [vals[i] for i in idx]
        u = unitigs_np(sub, [ab[i] for i in idx], k)
        slots = unitig_links_np(sub, k, u)
    masks = np.zeros(n, np.uint8)
    masks[idx] = graph_masks_np([vals[i] for i in idx], k)
    unitig = np.full(n, -1, np.int64); rev = np.zeros(n, bool); pos = np.zeros(n, np.int64)
    unitig[idx] = u["unitig"]; rev[idx] = u["reversed"]; pos[idx] = u["pos"]
    return dict(alive=alive, masks=masks, tips_per_round=per_round, rounds=len(per_round), records_removed=int(n - alive.sum()), u=u, slots=slots, unitig=unitig,
                reversed=rev, pos=pos, stopped_by_max_rounds=bool(per_round) and per_round[-1] != 0, graphs=graphs, values=vals, k=k)


def check_invariants(r, params):
    vals, k = r["values"], r["k"]
    idx = np.flatnonzero(r["alive"])
    assert np.array_equal(r["masks"][idx], graph_masks_np([vals[i] for i in idx], k)) and not r["masks"][~r["alive"]].any()
    assert r["records_removed"] == len(vals) - len(idx) and r["rounds"] <= params["max_rounds"]
    assert all(t > 0 for t in r["tips_per_round"][:-1])
    if not r["stopped_by_max_rounds"] and params["max_rounds"]:
        assert r["tips_per_round"][-1] == 0 and tips_of(r["u"], r["slots"], k, params) == []
    if k % 2 == 1:
        assert_symmetric(r["slots"])


def records_of_reads(reads, k):
    """every k-mer of the reads, one dataset: flat order = ascending -> (values, abundances = occurrences in the reads)"""
    cnt = collections.Counter(min(x, revcomp(x, k)) for r in reads for x in (str2int(r[i: i + k]) for i in range(len(r) - k + 1)))
    vals = sorted(cnt)
    return vals, [cnt[v] for v in vals]


def tips_of_reads(reads, k, **over):
    vals, ab = records_of_reads(reads, k)
    params = default_params(k, **over)
    r = tips_np(vals, ab, k, params)
    check_invariants(r, params)
    return r


def canonical(s):
    return min(s, rc_str(s))


def circle_read(seq, k):
    return seq + seq[: k - 1]                                   # every k-mer of the circle once


# ------------------------------------------------------------------------------------------------ inputs with a known shape (k = 21)
K = 21


def main_and_branches(tails, seed, main_len=300, at=150, k=K):
    """a main read of random bases and, per tail (a number of bases, or a string), a read that leaves it after position ``at``: the k - 1 bases in front of ``at`` and
    then the tail, whose first base differs from the main read's and from the other tails' -> (reads, main). A tail of t bases is a dead-end unitig of t records."""
    rng = np.random.default_rng(seed)
    main = random_sequence(rng, main_len)
    free = [b for b in "ACGT" if b != main[at]]
    reads = [main]
    for i, t in enumerate(tails):
        tail = t if isinstance(t, str) else free[i] + random_sequence(rng, t - 1)
        assert tail[0] == free[i]
        reads.append(main[at - (k - 1): at] + tail)
    return reads, main


def y_reads(k=K):
    """three short arms on one junction: a stem of 25 bases and two arms of 6 records each"""
    rng = np.random.default_rng(12)
    lead = random_sequence(rng, 25)
    return [lead + "A" + random_sequence(rng, 5), lead + "C" + random_sequence(rng, 5)]


def cascade_reads(k=K):
    """off a main read a binary tree of depth three whose seven edges have five records each: the four leaves go in round 1, the two inner edges in round 2, the root
    edge in round 3, and the main read compacts into one unitig"""
    rng = np.random.default_rng(21)
    main = random_sequence(rng, 300)
    reads = [main]

    def grow(prefix, first, depth):
        edge = first + random_sequence(rng, 4)
        reads.append(prefix[-(k - 1):] + edge)
        if depth:
            for b in "AC":
                grow((prefix + edge)[-(k - 1):], b, depth - 1)

    grow(main[:150], [b for b in "ACGT" if b != main[150]][0], 2)
    return reads


def cycle_with_tip_reads(k=K, L=40):
    seq, _ = circle(k, L)
    ext = seq + seq
    at = 30
    first = [b for b in "ACGT" if b != ext[at]][0]
    return [circle_read(seq, k), ext[at - (k - 1): at] + first + random_sequence(np.random.default_rng(2), 4)], seq


def coverage_reads(cov_left, cov_right, cov_tip, extra_right=0, k=K):
    """a main read and a branch of 40 records (60 bases: beyond the topological rule at k = 21) -> reads in which every k-mer left of the junction occurs cov_left
    times, right of it cov_right times, on the branch cov_tip times, and the LAST k-mer of the main read extra_right times more"""
    reads, main = main_and_branches([40], seed=33)
    at = 150
    left, right = main[:at], main[at - (k - 1):]               # the k-mers that end before / at or after position ``at``
    return [left] * cov_left + [right] * cov_right + [reads[1]] * cov_tip + [main[-k:]] * extra_right


# ------------------------------------------------------------------------------------------------ tests
def test_exports_are_declared_mapped_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    for n in NAMES:
        assert n in gkc.SYMBOLS, n
        assert ("int %s(gkc_ctx* ctx, " % n) in hdr, n
        assert "gkc_*" in vmap or n in vmap
    assert "typedef struct gkc_tip_params" in hdr and '"graph_tips"' in hdr
    for meth in ("remove_tips", "simplified_unitigs"):
        assert callable(getattr(gkc.Counter, meth))
    L = gkc.lib()
    assert len(L.gkc_graph_tips_remove.argtypes) == 10 and len(L.gkc_graph_unitigs_build_alive.argtypes) == 6


def test_the_reference_tip_vector():
    """debruijn_simplunitigs_tip: three unitigs (6 extremity nodes), the 27-base read is a tip of 7 records; after it has gone the two others are one path (4 -> the
    reference counts the extremities of what is left before compaction; here the graph is compacted again: ONE unitig), the sequence the reference traverses"""
    g = json.load(open(GOLDEN))
    k = g["k"]
    assert k == 21 and len(g["sequences"]) == 3 and (g["extremity_nodes_before"], g["extremity_nodes_after"]) == (6, 4)
    r = tips_of_reads(g["sequences"], k, max_len_rc=0)
    assert r["graphs"][0][0] == 3 == g["extremity_nodes_before"] // 2
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 7 == len(g["sequences"][1]) - k + 1
    assert len(r["u"]["seqs"]) == 1 and canonical(r["u"]["seqs"][0]) == canonical(g["traversal"])
    assert r["slots"] == [[], []]


FIXTURES = {
    # name: (tips per round, records removed, unitigs, links) with the default parameters / with the coverage rule off — as found by the statement
    "k21_freq_4parts": (([200, 0], 1646, 312, 728), ([200, 0], 1646, 312, 728)),
    "k31_defaults": (([25, 2, 0], 482, 39, 64), ([24, 0], 307, 42, 72)),
    "k63_defaults": (([4, 0], 177, 23, 0), ([4, 0], 177, 23, 0)),
}


@functools.lru_cache(maxsize=None)
def fixture_tips(name, coverage=True):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    values = [v for p in parts for v, _ in p]; ab = [a for p in parts for _, a in p]
    params = default_params(k) if coverage else default_params(k, max_len_rc=0)
    return k, params, tips_np(values, ab, k, params)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_invariants_on_the_fixtures(name):
    for coverage in (True, False):
        k, params, r = fixture_tips(name, coverage)
        check_invariants(r, params)
        got = (r["tips_per_round"], r["records_removed"], len(r["u"]["seqs"]), sum(len(s) for s in r["slots"]))
        print(name, coverage, got)
        assert got == FIXTURES[name][0 if coverage else 1]


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_fuzz_over_random_subsets(k):
    rng = np.random.default_rng(300 + k)
    every = sorted({min(x, revcomp(x, k)) for x in range(4 ** k)})
    removed = 0
    for density in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7):
        vals = [x for x in every if rng.random() < density]
        ab = rng.integers(1, 50, len(vals)).tolist()
        for params in (default_params(k), default_params(k, max_len_rc=0), default_params(k, max_len_topo=0, max_len_rc=4 * k, rc_num=3, rc_den=2), default_params(k, max_rounds=1)):
            r = tips_np(vals, ab, k, params)
            check_invariants(r, params)
            removed += r["records_removed"]
    assert removed > 0


def test_a_tip_of_exactly_max_len_topo_goes_and_one_base_longer_stays():
    assert default_params(K)["max_len_topo"] == 52
    r = tips_of_reads(main_and_branches([32], seed=1)[0], K, max_len_rc=0)              # 32 records: 52 bases
    assert r["graphs"][0] == (3, 4) and r["tips_per_round"] == [1, 0] and r["records_removed"] == 32 and len(r["u"]["seqs"]) == 1 and r["slots"] == [[], []]
    r = tips_of_reads(main_and_branches([33], seed=1)[0], K, max_len_rc=0)              # 53 bases
    assert r["tips_per_round"] == [0] and r["records_removed"] == 0 and len(r["u"]["seqs"]) == 3 and r["alive"].all()


def test_a_one_record_tip():
    reads, main = main_and_branches([1], seed=2)
    r = tips_of_reads(reads, K, max_len_rc=0)
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 1 and r["u"]["seqs"] in ([main], [rc_str(main)])


def test_two_tips_on_one_junction_go_in_the_same_round():
    reads, main = main_and_branches([5, 9], seed=3)
    r = tips_of_reads(reads, K, max_len_rc=0)
    assert r["graphs"][0][0] == 4 and r["tips_per_round"] == [2, 0] and r["records_removed"] == 14
    assert r["u"]["seqs"] in ([main], [rc_str(main)]) and r["graphs"][1] == (1, 0)


def test_a_y_of_three_short_arms_vanishes_whole():
    r = tips_of_reads(y_reads(), K, max_len_rc=0)
    assert r["graphs"] == [(3, 4), (0, 0)] and r["tips_per_round"] == [3, 0] and not r["alive"].any() and r["records_removed"] == 5 + 6 + 6
    assert r["u"]["seqs"] == [] and r["slots"] == [] and r["u"]["offsets"].tolist() == [0]


@pytest.mark.parametrize("max_rounds,per_round,n_unitigs,removed", [(0, [], 9, 0), (1, [4], 5, 20), (2, [4, 2], 3, 30), (3, [4, 2, 1], 1, 35), (20, [4, 2, 1, 0], 1, 35)])
def test_a_cascade_needs_three_rounds(max_rounds, per_round, n_unitigs, removed):
    reads = cascade_reads()
    r = tips_of_reads(reads, K, max_len_rc=0, max_rounds=max_rounds)
    assert r["tips_per_round"] == per_round and r["rounds"] == len(per_round)
    assert len(r["u"]["seqs"]) == n_unitigs and r["records_removed"] == removed
    assert r["stopped_by_max_rounds"] == (max_rounds in (1, 2, 3))
    if n_unitigs == 1:
        assert canonical(r["u"]["seqs"][0]) == canonical(reads[0])


def test_a_tip_hanging_on_an_isolated_cycle():
    reads, seq = cycle_with_tip_reads()
    r = tips_of_reads(reads, K, max_len_rc=0)
    assert r["graphs"][0] == (2, 4)                             # the circle opened at the junction: links to itself and to the tip, the tip links back
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 5
    assert len(r["u"]["seqs"]) == 1 and r["u"]["n_cycles"] == 1 and r["slots"] == [[0], [1]] and len(r["u"]["seqs"][0]) == len(seq) + K - 1


def test_a_hairpin_whose_other_side_is_a_dead_end():
    """the hairpin's end links to itself (L:+:0:-), the other side is a dead end: a candidate like any other, no special case"""
    vals, ab = records_of_reads(hairpin_reads(), K)
    u = unitigs_np(vals, ab, K)
    bases = len(u["seqs"][0])
    assert len(u["seqs"]) == 1 and unitig_links_np(vals, K, u) == [[1], []] and bases == 51
    r = tips_of_reads(hairpin_reads(), K, max_len_rc=0)
    assert r["tips_per_round"] == [1, 0] and not r["alive"].any()
    r = tips_of_reads(hairpin_reads(), K, max_len_rc=0, max_len_topo=bases - 1)
    assert r["tips_per_round"] == [0] and r["alive"].all()


def test_a_side_with_four_links():
    """star_reads: a stem of 10 records (30 bases) whose one side has four links, four arms of 31 records (51 bases)"""
    r = tips_of_reads(star_reads(), K, max_len_rc=0)
    assert r["graphs"][0] == (5, 8) and r["tips_per_round"] == [5, 0] and not r["alive"].any()
    r = tips_of_reads(star_reads(), K, max_len_rc=0, max_len_topo=40)                    # the stem alone: the arms are isolated afterwards and stay
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 10 and len(r["u"]["seqs"]) == 4 and r["slots"] == [[]] * 8
    # the coverage rule through the side with four links: the stem (in all four reads: 4 x) against its four arms at 1 x; one arm at 8 x is equality, at 9 x better
    reads = star_reads()
    assert tips_of_reads(reads, K, max_len_topo=0, max_len_rc=40)["tips_per_round"] == [0]
    assert tips_of_reads(reads + [reads[3][10:]] * 7, K, max_len_topo=0, max_len_rc=40)["tips_per_round"] == [0]
    r = tips_of_reads(reads + [reads[3][10:]] * 8, K, max_len_topo=0, max_len_rc=40)
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 10


def test_an_isolated_short_unitig_and_an_isolated_cycle_stay():
    reads = [random_sequence(np.random.default_rng(4), 25), circle_read(circle(K, 40)[0], K)]
    r = tips_of_reads(reads, K)
    assert r["tips_per_round"] == [0] and r["alive"].all() and len(r["u"]["seqs"]) == 2 and r["u"]["n_cycles"] == 1


def test_the_coverage_rule_is_strict():
    """tip at 3 x, both main arms at 6 x, ratio 2 / 1: equality does not remove; one abundance unit more on one record of the right arm does"""
    rule = dict(max_len_topo=0, max_len_rc=100)
    r = tips_of_reads(coverage_reads(6, 6, 3), K, **rule)
    assert r["graphs"][0] == (3, 4) and r["tips_per_round"] == [0] and r["alive"].all()
    r = tips_of_reads(coverage_reads(6, 6, 3, extra_right=1), K, **rule)
    assert r["tips_per_round"] == [1, 0] and r["records_removed"] == 40 and len(r["u"]["seqs"]) == 1
    r = tips_of_reads(coverage_reads(6, 6, 3, extra_right=1), K, max_len_topo=0, max_len_rc=59)      # the tip has 60 bases
    assert r["tips_per_round"] == [0]


def test_the_competitor_is_the_arrival_unitig_or_a_sibling():
    """the tip arrives at the left arm (the unitig that ends in the junction); the right arm is the other entry of that arm's slot, a sibling"""
    rule = dict(max_len_topo=0, max_len_rc=100)
    assert tips_of_reads(coverage_reads(7, 1, 3), K, **rule)["tips_per_round"] == [1, 0]            # the arrival unitig alone is better covered
    assert tips_of_reads(coverage_reads(1, 7, 3), K, **rule)["tips_per_round"] == [1, 0]            # the sibling alone
    assert tips_of_reads(coverage_reads(5, 5, 3), K, **rule)["tips_per_round"] == [0]               # neither
