"""Simplification of the compacted graph (include/gkc.h, "simplify"; gkc_graph_simplify), the part that needs no GPU: a plain Python statement of the definitions
(names, bulge, erroneous connection, phase, sweep) that recomputes the unitigs and links of the alive records FROM SCRATCH every round (unitigs_np / unitig_links_np
over the alive values), so it shares nothing with the device code. The tip rule is tips_of of tests/test_tips_cpu.py. The reference's own known answers
(tests/golden/reference_simplify_vectors.json, written by tools/make_simplify_vectors.py from its unit tests debruijn_simplunitigs_bubble, _bubble_snp and _ec) pin the
two new rules. tests/test_gpu_simplify.py imports the statement."""
import functools
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_graph_cpu import graph_masks_np, revcomp
from tests.test_reference_run import DIR, load
from tests.test_tips_cpu import K, canonical, default_params as tip_defaults, records_of_reads, tips_of
from tests.test_unitig_links_cpu import assert_symmetric, random_sequence, unitig_links_np
from tests.test_unitigs_cpu import unitigs_np
from tests.util import str2int

GOLDEN = os.path.join(os.path.dirname(DIR), "reference_simplify_vectors.json")
KINDS = ("tips", "bulges", "ec")


# ------------------------------------------------------------------------------------------------ the statement
def default_params(k, **over):
    """the reference's constants (Simplifications.cpp): tips as tests/test_tips_cpu.py; bulges up to max(3 k, k + 100) bases, the alternative up to max(11 / 10 L, L + 3)
    records; erroneous connections up to 9 k bases, ratio 4; 20 rounds per phase, 10 sweeps. ``tip_rounds`` stands for the max_rounds of the tips."""
    p = tip_defaults(k)
    p["tip_rounds"] = p.pop("max_rounds")
    p.update(bulge_max_len=max(3 * k, k + 100), bulge_alt_num=11, bulge_alt_den=10, bulge_alt_add=3, bulge_rounds=20, ec_max_len=9 * k, ec_num=4, ec_den=1, ec_rounds=20,
             max_sweeps=10)
    p.update(over)
    return p


def only(kind, k, **over):
    """the parameters of Counter.remove_bulges / remove_erroneous_connections: the other kinds get no rounds"""
    off = dict(tip_rounds=0, bulge_rounds=0, ec_rounds=0)
    del off[{"tips": "tip_rounds", "bulges": "bulge_rounds", "ec": "ec_rounds"}[kind]]
    off.update(over)
    return default_params(k, **off)


def names(slots, t):
    """the slots that slot t names: entry (v, m) names (v, 1 - m), i.e. slot e ^ 1"""
    return [e ^ 1 for e in slots[t]]


def bulges_of(u, slots, k, p):
    lens = [len(s) - k + 1 for s in u["seqs"]]
    kc = [int(x) for x in u["kc"]]
    hits = []
    for un in range(len(lens)):
        if not slots[2 * un] or not slots[2 * un + 1] or lens[un] + k - 1 > p["bulge_max_len"]:
            continue
        max_len_c = max(lens[un] * p["bulge_alt_num"] // p["bulge_alt_den"], lens[un] + p["bulge_alt_add"])
        hit = False
        for X in names(slots, 2 * un):
            for C in names(slots, X):
                c = C >> 1
                if c == un or X >> 1 in (un, c) or X not in names(slots, C):
                    continue
                if lens[c] > max_len_c:
                    continue
                a, b = kc[un] * lens[c], kc[c] * lens[un]
                if not (a < b or (a == b and c < un)):
                    continue
                for Y in names(slots, 2 * un + 1):
                    if Y >> 1 not in (un, c) and Y in names(slots, C ^ 1):
                        hit = True
        if hit:
            hits.append(un)
    return hits


def ecs_of(u, slots, k, p):
    lens = [len(s) - k + 1 for s in u["seqs"]]
    kc = [int(x) for x in u["kc"]]
    hits = []
    for un in range(len(lens)):
        if not slots[2 * un] or not slots[2 * un + 1] or lens[un] + k - 1 > p["ec_max_len"]:
            continue
        if not all(any(len(slots[t]) >= 2 for t in names(slots, 2 * un + s)) for s in (0, 1)):
            continue
        hit = False
        for s in (0, 1):
            for e in slots[2 * un + s]:
                back = list(slots[e ^ 1])
                if (un << 1 | (1 - s)) in back:
                    back.remove(un << 1 | (1 - s))              # the one entry that is u coming back
                for c in [e >> 1] + [w >> 1 for w in back]:
                    if c != un and kc[c] * lens[un] * p["ec_den"] > p["ec_num"] * kc[un] * lens[c]:
                        hit = True
        if hit:
            hits.append(un)
    return hits


def hits_of(kind, u, slots, k, p):
    if kind == "tips":
        return tips_of(u, slots, k, dict(max_len_topo=p["max_len_topo"], max_len_rc=p["max_len_rc"], rc_num=p["rc_num"], rc_den=p["rc_den"]))
    return bulges_of(u, slots, k, p) if kind == "bulges" else ecs_of(u, slots, k, p)


def graph_of(vals, ab, alive, k):
    idx = np.flatnonzero(alive)
    sub = [vals[i] for i in idx]
    u = unitigs_np(sub, [ab[i] for i in idx], k)
    return idx, u, unitig_links_np(sub, k, u)


def simplify_np(values, abundances, k, params, alive=None):
    """-> dict: alive bool[n], masks uint8[n] (0 for dead records), log = [(kind, sweep, n_unitigs, n_hits, n_records_removed)] of every round run, rounds,
    records_removed (of this call), and the final graph as tips_np gives it: u, slots, unitig / reversed / pos per record of the FULL flat order (unitig -1: dead).
    ``alive``: the state a call resumes (default: every record alive)."""
    vals = [int(v) for v in values]; ab = [int(a) for a in abundances]
    n = len(vals)
    alive = np.ones(n, bool) if alive is None else np.array(alive, bool)
    before = int(alive.sum())
    log = []

    def phase(kind, sweep):
        gone = 0
        for _ in range(params[{"tips": "tip_rounds", "bulges": "bulge_rounds", "ec": "ec_rounds"}[kind]]):
            idx, u, slots = graph_of(vals, ab, alive, k)        # from scratch, every round
            hits = hits_of(kind, u, slots, k, params)
            dead = idx[np.isin(u["unitig"], hits)] if hits else idx[:0]
            alive[dead] = False
            log.append((kind, sweep, len(u["seqs"]), len(hits), len(dead)))
            gone += len(dead)
            if not hits:
                break
        return gone

    phase("tips", 0)
    for sweep in range(1, params["max_sweeps"] + 1):
        if not phase("bulges", sweep) + phase("ec", sweep) + phase("tips", sweep):
            break
    idx, u, slots = graph_of(vals, ab, alive, k)
    masks = np.zeros(n, np.uint8)
    masks[idx] = graph_masks_np([vals[i] for i in idx], k)
    unitig = np.full(n, -1, np.int64); rev = np.zeros(n, bool); pos = np.zeros(n, np.int64)
    unitig[idx] = u["unitig"]; rev[idx] = u["reversed"]; pos[idx] = u["pos"]
    return dict(alive=alive, masks=masks, log=log, rounds=len(log), records_removed=before - int(alive.sum()), u=u, slots=slots, unitig=unitig, reversed=rev, pos=pos,
                values=vals, k=k)


def phases(log):
    """the log grouped: [((kind, sweep), [hits per round])] in order"""
    out = []
    for kind, sweep, _, hits, _ in log:
        if not out or out[-1][0] != (kind, sweep):
            out.append(((kind, sweep), []))
        out[-1][1].append(hits)
    return out


def stopped_by_a_cap(log, p):
    """some phase ended with a round that had hits, or the last sweep allowed removed something"""
    ph = phases(log)
    if any(h[-1] for _, h in ph):
        return True
    last = max(s for (_, s), _ in ph) if ph else 0
    return last == p["max_sweeps"] and any(sum(h) for (_, s), h in ph if s == last and s > 0)


def check_invariants(r, p):
    vals, k = r["values"], r["k"]
    idx = np.flatnonzero(r["alive"])
    assert np.array_equal(r["masks"][idx], graph_masks_np([vals[i] for i in idx], k)) and not r["masks"][~r["alive"]].any()
    assert r["records_removed"] == sum(e[4] for e in r["log"]) and r["rounds"] == len(r["log"])
    cap = dict(tips=p["tip_rounds"], bulges=p["bulge_rounds"], ec=p["ec_rounds"])
    for (kind, sweep), hits in phases(r["log"]):
        assert all(h > 0 for h in hits[:-1]) and 1 <= len(hits) <= cap[kind] and sweep <= p["max_sweeps"]      # every non-final round of a phase has hits
    if not stopped_by_a_cap(r["log"], p):
        for kind in KINDS:
            if cap[kind] and (kind == "tips" or p["max_sweeps"]):
                assert hits_of(kind, r["u"], r["slots"], k, p) == [], kind
    if k % 2 == 1:
        assert_symmetric(r["slots"])


def simplify_of_reads(reads, k, params=None, **over):
    vals, ab = records_of_reads(reads, k)
    p = params if params is not None else default_params(k, **over)
    r = simplify_np(vals, ab, k, p)
    check_invariants(r, p)
    return r


def hits(r):
    """-> [(kind, [hits per round])] of the phases that removed something"""
    return [(kind, h) for (kind, _), h in phases(r["log"]) if sum(h)]


# ------------------------------------------------------------------------------------------------ inputs with a known shape (k = 21)
def bubble_reads(branches, seed, arm=300, k=K):
    """two arms of random bases and, between them, parallel branches: ``branches`` = [(inner bases, coverage)], each inner string placed between the last k - 1 bases of
    the left arm and the first k - 1 of the right one, and the read repeated ``coverage`` times. A branch of b inner bases is a unitig of b + k - 1 records.
    -> (reads, left, right)"""
    rng = np.random.default_rng(1000 + seed)
    left, right = random_sequence(rng, arm), random_sequence(rng, arm)
    reads = [left, right]
    for inner, cov in branches:
        reads += [left[-(k - 1):] + inner + right[: k - 1]] * cov
    return reads, left, right


def branches_of(records, coverages, seed, k=K):
    """-> [(inner bases, coverage)] for bubble_reads: branch i is a unitig of records[i] >= k records; the branches differ in their first and in their last inner base, so
    no two share a k-mer"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (L, cov) in enumerate(zip(records, coverages)):
        n = L - (k - 1)
        assert n >= 1
        out.append(("ACGT"[i] if n == 1 else "ACGT"[i] + random_sequence(rng, n - 2) + "TGCA"[i], cov))
    return out


def snp_chain_reads(n_bubbles, seed, gap=10, flank=300, k=K):
    """one random main sequence (2 x) with an SNP every ``gap`` + k bases between two flanks too long to be tips and, per SNP, a read (1 x) that spells the other allele:
    n_bubbles bulges of k records, gap records of the main sequence between two of them -> (reads, main)"""
    rng = np.random.default_rng(seed)
    main = random_sequence(rng, 2 * flank + (n_bubbles + 1) * (gap + k))
    reads = [main, main]
    for b in range(n_bubbles):
        at = flank + (b + 1) * (gap + k) - k // 2
        other = [x for x in "ACGT" if x != main[at]][int(rng.integers(0, 3))]
        reads.append(main[at - (k - 1): at] + other + main[at + 1: at + k])
    return reads, main


def z_reads(cov_main, cov_ec, extra=0, k=K, ec_inner=10):
    """two main sequences A and B (cov_main x each) and a connector (cov_ec x) from the middle of A to the middle of B: it leaves A after position 150 and joins B at
    position 150, with ``ec_inner`` bases of its own in between: the Z of the reference's comment. ``extra``: that many more reads of the last k-mer of A."""
    rng = np.random.default_rng(77)
    A, B = random_sequence(rng, 300), random_sequence(rng, 300)
    first = [x for x in "ACGT" if x != A[150]][0]
    last = [x for x in "ACGT" if x != B[149]][0]
    inner = first + random_sequence(rng, ec_inner - 2) + last
    conn = A[150 - (k - 1): 150] + inner + B[150: 150 + k - 1]
    return [A] * cov_main + [B] * cov_main + [conn] * cov_ec + [A[-k:]] * extra


def one_record_z_reads(cov_main, k=K):
    """a Z whose connector is ONE k-mer: B repeats the k - 2 bases of A in front of position 150 and goes on with another base, so the k-mer made of A's k - 1 bases and
    that base follows A's left half and precedes B's right half"""
    rng = np.random.default_rng(79)
    A = random_sequence(rng, 300)
    x = [b for b in "ACGT" if b != A[150]][0]
    B = random_sequence(rng, 150) + A[150 - (k - 2): 150] + x + random_sequence(rng, 150)
    return [A] * cov_main + [B] * cov_main + [A[150 - (k - 1): 150] + x]


def half_z_reads(k=K):
    """a connector that leaves the middle of A (8 x) and ends in a fork of its own: two entries on that side, but neither of the slots it names there has a second
    entry, so it has a sibling on A's side only"""
    rng = np.random.default_rng(78)
    A = random_sequence(rng, 300)
    first = [x for x in "ACGT" if x != A[150]][0]
    core = first + random_sequence(rng, 29)
    return [A] * 8 + [A[150 - (k - 1): 150] + core + "A" + random_sequence(rng, 40), core[-(k - 1):] + "C" + random_sequence(rng, 40)]


def two_sweep_reads(k=K):
    """a cascade that needs two sweeps. A main sequence (9 x) with a weak parallel branch W (3 x, 40 bases of its own): the bubble P. Off the middle of W goes a side
    branch (1 x): a stem, an SNP bubble Q at equal coverage, and an end of 60 bases that is too long for the topological rule and no worse covered than Q's branches.
    The side branch cuts W in two, so P is no simple bubble, and nothing is a tip. Sweep 1: one branch of Q is a bulge; the side branch is then one dead-end unitig at
    1 x against W's 3 x, a tip by coverage. Sweep 2: W is whole again and a bulge against the main sequence. -> (reads, main)"""
    rng = np.random.default_rng(91)
    main = random_sequence(rng, 400)
    wf = [x for x in "ACGT" if x != main[150]][0]; wl = [x for x in "ACGT" if x != main[189]][0]
    weak_read = main[150 - (k - 1): 150] + wf + random_sequence(rng, 38) + wl + main[190: 190 + k - 1]
    at = (k - 1) + 20                                           # the side branch leaves W after its 20th base
    tf = [x for x in "ACGT" if x != weak_read[at]][0]
    stem = weak_read[at - (k - 1): at] + tf + random_sequence(rng, 11 + k - 1)
    after = random_sequence(rng, k - 1 + 60)
    return [main] * 9 + [weak_read] * 3 + [stem + "A" + after, stem[-(k - 1):] + "C" + after[: k - 1]], main


# ------------------------------------------------------------------------------------------------ tests
def test_exports_are_declared_mapped_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    n = "gkc_graph_simplify"
    assert n in gkc.SYMBOLS and ("int %s(gkc_ctx* ctx, " % n) in hdr and ("gkc_*" in vmap or n in vmap)
    assert "typedef struct gkc_simplify_params" in hdr and "typedef struct gkc_simplify_round" in hdr and '"graph_bulges"' in hdr and '"graph_ec"' in hdr
    for meth in ("simplify", "remove_bulges", "remove_erroneous_connections", "simplified_masks", "simplified_unitigs"):
        assert callable(getattr(gkc.Counter, meth))
    L = gkc.lib()
    assert len(L.gkc_graph_simplify.argtypes) == 11
    import ctypes as C
    assert C.sizeof(gkc.SimplifyParams) == 4 * (5 + 5 + 4 + 2) and C.sizeof(gkc.SimplifyRound) == 32
    assert [f[0] for f in gkc.SimplifyParams._fields_][:2] == ["tips", "bulge_max_len"] and gkc.SimplifyParams._fields_[-1][0] == "resume"


def vectors():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", ["bubble", "bubble_snp"])
def test_the_reference_bubble_vectors(name):
    g = vectors()[name]
    k = g["k"]
    assert k == 21 and (g["nodes_before"], g["nodes_after"]) == (8, 6)
    r = simplify_of_reads(g["sequences"], k)
    assert r["log"][0][2] == 4 == g["nodes_before"] // 2
    assert hits(r) == [("bulges", [1, 0])] and r["records_removed"] == 21
    assert g["nodes_after"] == 2 * (r["log"][0][2] - 1)
    assert len(r["u"]["seqs"]) == 1 and len(r["u"]["seqs"][0]) == 633
    want = g["traversals"][0] if name == "bubble" else g["traversals"][1]      # bubble_snp: the 4 x path survives, the reference's second accepted answer
    assert canonical(r["u"]["seqs"][0]) == canonical(want)
    assert r["slots"] == [[], []]


def test_the_reference_ec_vector():
    g = vectors()["ec"]
    k = g["k"]
    assert k == 21 and (g["nodes_before"], g["nodes_after"]) == (10, 8)
    r = simplify_of_reads(g["sequences"], k)
    assert r["log"][0][2] == 5 == g["nodes_before"] // 2
    assert hits(r) == [("ec", [1, 0])] and r["records_removed"] == 6          # no tip, no bulge, one EC of 6 records
    assert g["nodes_after"] == 2 * (r["log"][0][2] - 1)
    got = sorted(canonical(s) for s in r["u"]["seqs"])
    assert sorted(len(s) for s in got) == [460, 637] and got == sorted(canonical(t) for t in g["traversals"])


FIXTURES = {
    # name: (hits per round of the phases: the leading tips, then bulges, ec, tips of sweep 1, ...; records removed, unitigs left, links left) with the defaults
    "k21_freq_4parts": ([[200, 0], [82, 0], [9, 0], [0], [0], [0], [0]], 3557, 40, 0),
    "k31_defaults": ([[25, 2, 0], [8, 0], [0], [0], [0], [0], [0]], 730, 15, 0),
    "k63_defaults": ([[4, 0], [0], [0], [0]], 177, 23, 0),
}


@functools.lru_cache(maxsize=None)
def fixture_simplify(name):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    values = [v for p in parts for v, _ in p]; ab = [a for p in parts for _, a in p]
    p = default_params(k)
    return k, p, simplify_np(values, ab, k, p)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_fixtures_with_the_defaults(name):
    k, p, r = fixture_simplify(name)
    check_invariants(r, p)
    got = ([h for _, h in phases(r["log"])], r["records_removed"], len(r["u"]["seqs"]), sum(len(s) for s in r["slots"]))
    print(name, got)
    assert got == FIXTURES[name]
    assert [kind for (kind, _), _ in phases(r["log"])][:4] == ["tips", "bulges", "ec", "tips"]


PARAMETER_SETS = (dict(), dict(tip_rounds=0, ec_rounds=0), dict(tip_rounds=0, bulge_rounds=0), dict(bulge_rounds=0, ec_rounds=0), dict(max_sweeps=1, tip_rounds=1, bulge_rounds=1, ec_rounds=1),
                  dict(max_sweeps=0), dict(ec_num=3, ec_den=2, bulge_alt_num=3, bulge_alt_den=2, bulge_alt_add=0, max_len_rc=0))


def planted_bubbles(rng, k, n):
    """the k-mers of n SNP bubbles between random flanks (random subsets of all k-mers hold next to no simple bubble: its two branches need k records each) ->
    {canonical k-mer: abundance}"""
    out = {}
    for _ in range(n):
        left, right = random_sequence(rng, k + 2), random_sequence(rng, k + 2)
        for b, cov in (("A", 7), ("C", 2)):
            seq = left + b + right
            for i in range(len(seq) - k + 1):
                x = str2int(seq[i: i + k])
                out[min(x, revcomp(x, k))] = cov
    return out


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_fuzz_over_random_subsets(k):
    rng = np.random.default_rng(500 + k)
    every = sorted({min(x, revcomp(x, k)) for x in range(4 ** k)})
    removed = {kind: 0 for kind in KINDS}
    for density in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7):
        cnt = {x: int(rng.integers(1, 50)) for x in every if rng.random() < density}
        if density <= 0.1:
            cnt.update(planted_bubbles(rng, k, 3))
        vals = sorted(cnt); ab = [cnt[v] for v in vals]
        for over in PARAMETER_SETS:
            p = default_params(k, **over)
            r = simplify_np(vals, ab, k, p)
            check_invariants(r, p)
            for e in r["log"]:
                removed[e[0]] += e[4]
    print(k, removed)
    assert removed["tips"] > 0
    if k >= 4:
        assert removed["bulges"] > 0 and removed["ec"] > 0


def test_an_snp_bubble_at_3x_against_1x():
    br = branches_of([K, K], [3, 1], seed=5)
    reads, left, right = bubble_reads(br, seed=5)
    r = simplify_of_reads(reads, K)
    assert r["log"][0][2] == 4 and hits(r) == [("bulges", [1, 0])] and r["records_removed"] == K
    assert [canonical(s) for s in r["u"]["seqs"]] == [canonical(left + br[0][0] + right)]


def test_equal_coverage_the_lower_index_survives():
    reads, left, right = bubble_reads(branches_of([K, K], [2, 2], seed=6), seed=6)
    vals, ab = records_of_reads(reads, K)
    idx, u, slots = graph_of(vals, ab, np.ones(len(vals), bool), K)
    twins = [i for i, s in enumerate(u["seqs"]) if len(s) == 2 * K - 1]
    assert len(twins) == 2 and u["kc"][twins[0]] == u["kc"][twins[1]]
    assert bulges_of(u, slots, K, default_params(K)) == [twins[1]]            # exactly one of the two goes: the higher index
    r = simplify_of_reads(reads, K)
    assert hits(r) == [("bulges", [1, 0])] and len(r["u"]["seqs"]) == 1
    assert not r["alive"][idx[u["unitig"] == twins[1]]].any() and r["alive"][idx[u["unitig"] == twins[0]]].all()


def test_three_parallel_branches_two_go_in_one_round():
    reads, left, right = bubble_reads(branches_of([K, K, K], [5, 2, 1], seed=7), seed=7)
    r = simplify_of_reads(reads, K)
    assert r["log"][0][2] == 5 and hits(r) == [("bulges", [2, 0])] and r["records_removed"] == 2 * K and len(r["u"]["seqs"]) == 1


def test_a_bulge_of_exactly_bulge_max_len_goes_and_one_base_longer_stays():
    assert default_params(K)["bulge_max_len"] == 121
    n = 121 - (K - 1)                                           # records: 121 bases
    reads, _, _ = bubble_reads(branches_of([n, n], [3, 1], seed=8), seed=8)
    r = simplify_of_reads(reads, K)
    assert hits(r) == [("bulges", [1, 0])] and r["records_removed"] == n
    reads, _, _ = bubble_reads(branches_of([n + 1, n + 1], [3, 1], seed=8), seed=8)
    r = simplify_of_reads(reads, K)
    assert hits(r) == [] and r["alive"].all() and len(r["u"]["seqs"]) == 4


def test_an_indel_bubble_up_to_three_records_longer():
    """L_u = 30: max(30 * 11 // 10, 30 + 3) = 33. The short branch is the poorly covered one"""
    reads, _, _ = bubble_reads(branches_of([33, 30], [3, 1], seed=9), seed=9)
    r = simplify_of_reads(reads, K)
    assert hits(r) == [("bulges", [1, 0])] and r["records_removed"] == 30
    reads, _, _ = bubble_reads(branches_of([34, 30], [3, 1], seed=9), seed=9)
    r = simplify_of_reads(reads, K)
    assert hits(r) == [] and r["alive"].all()                   # no eligible alternative: the short, poorly covered branch stays


def test_a_z_shaped_ec_is_strict():
    """the connector at 1 x (30 records), the four arms at 4 x: KC_c L_u > 4 KC_u L_c is equality; one abundance unit more on one arm decides"""
    r = simplify_of_reads(z_reads(4, 1), K, tip_rounds=0, bulge_rounds=0)
    assert r["log"][0][2] == 5 and hits(r) == [] and r["alive"].all()
    r = simplify_of_reads(z_reads(4, 1, extra=1), K, tip_rounds=0, bulge_rounds=0)
    assert hits(r) == [("ec", [1, 0])] and r["records_removed"] == 30 and len(r["u"]["seqs"]) == 2
    r = simplify_of_reads(z_reads(4, 1, extra=1), K, tip_rounds=0, bulge_rounds=0, ec_max_len=30 + K - 2)
    assert hits(r) == []                                        # one base too long for the rule


def test_a_single_record_unitig_can_be_an_ec():
    r = simplify_of_reads(one_record_z_reads(5), K, tip_rounds=0, bulge_rounds=0)
    assert r["log"][0][2] == 5 and hits(r) == [("ec", [1, 0])] and r["records_removed"] == 1 and len(r["u"]["seqs"]) == 2
    r = simplify_of_reads(one_record_z_reads(4), K, tip_rounds=0, bulge_rounds=0)      # 4 x against 1 x: equality
    assert hits(r) == [] and r["alive"].all()


def test_a_connector_with_a_sibling_on_one_side_only_is_no_ec():
    r = simplify_of_reads(half_z_reads(), K, tip_rounds=0, bulge_rounds=0)
    assert r["log"][0][2] == 5 and hits(r) == [] and r["alive"].all()
    vals, ab = records_of_reads(half_z_reads(), K)
    idx, u, slots = graph_of(vals, ab, np.ones(len(vals), bool), K)
    assert sorted(len(s) for s in slots) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]


def test_a_cascade_needs_two_sweeps():
    reads, main = two_sweep_reads()
    r = simplify_of_reads(reads, K)
    assert [(ks, h) for ks, h in phases(r["log"])] == [(("tips", 0), [0]), (("bulges", 1), [1, 0]), (("ec", 1), [0]), (("tips", 1), [1, 0]),
                                                       (("bulges", 2), [1, 0]), (("ec", 2), [0]), (("tips", 2), [0]), (("bulges", 3), [0]), (("ec", 3), [0]), (("tips", 3), [0])]
    assert [canonical(s) for s in r["u"]["seqs"]] == [canonical(main)]
    r = simplify_of_reads(reads, K, max_sweeps=1)               # stopped by the cap: the second bubble is still there
    assert len(r["u"]["seqs"]) == 4 and r["rounds"] == 6


def test_caps_and_the_log_under_them():
    reads, _, _ = bubble_reads(branches_of([K, K, K], [5, 2, 1], seed=7), seed=7)
    r = simplify_of_reads(reads, K, max_sweeps=0)
    assert r["log"] == [("tips", 0, 5, 0, 0)] and r["alive"].all()
    r = simplify_of_reads(reads, K, bulge_rounds=1)             # the phase stops after its one round; sweep 2 sees nothing left to do
    assert [e[:2] + e[3:] for e in r["log"]] == [("tips", 0, 0, 0), ("bulges", 1, 2, 2 * K), ("ec", 1, 0, 0), ("tips", 1, 0, 0), ("bulges", 2, 0, 0), ("ec", 2, 0, 0), ("tips", 2, 0, 0)]
    r = simplify_of_reads(reads, K, bulge_rounds=1, max_sweeps=1)
    assert r["rounds"] == 4 and r["records_removed"] == 2 * K
    r = simplify_of_reads(reads, K, tip_rounds=0, bulge_rounds=0, ec_rounds=0)
    assert r["log"] == [] and r["alive"].all() and len(r["u"]["seqs"]) == 5


def test_resume_tips_alone_then_a_resumed_call_equals_one_full_call():
    k, p, full = fixture_simplify("k31_defaults")
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, "k31_defaults.npz"))
    values = [v for q in parts for v, _ in q]; ab = [a for q in parts for _, a in q]
    first = simplify_np(values, ab, k, default_params(k, max_sweeps=0))
    assert [h for _, h in phases(first["log"])] == [[25, 2, 0]]
    second = simplify_np(values, ab, k, p, alive=first["alive"])
    assert np.array_equal(second["alive"], full["alive"]) and np.array_equal(second["masks"], full["masks"])
    assert first["records_removed"] + second["records_removed"] == full["records_removed"]
    assert [h for _, h in phases(second["log"])] == [[0]] + [h for _, h in phases(full["log"])][1:]
