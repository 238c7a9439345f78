"""tests/graph_inputs.py pinned without a device: its fast numpy statement of the graph (masks, topology, branching records, record links, unitigs, unitig links) equals
the per-record Python statements of tests/test_graph_cpu.py, test_unitigs_cpu.py and test_unitig_links_cpu.py, byte for byte on every array, and each of its
constructions, at about 1 / 500 of the size tests/test_gpu_graph_sizes.py runs it at, has the record count it claims and is simplified by the Python statements of
tests/test_tips_cpu.py and tests/test_simplify_cpu.py exactly as it claims. The Python statements are the authority: where one disagrees, graph_inputs.py is wrong."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import graph_inputs as gi
from tests.test_gpu_graph import count_records
from tests.test_graph_cpu import branching_from_masks, graph_masks_np, revcomp, topology_from_masks
from tests.test_reference_run import DIR, load
from tests.test_simplify_cpu import default_params as simplify_defaults, only, simplify_np
from tests.test_tips_cpu import default_params as tip_defaults, records_of_reads, tips_np
from tests.test_unitig_links_cpu import csr, hairpin_reads, unitig_links_np
from tests.test_unitigs_cpu import CYCLES, circle, unitigs_np

K = 31


def assert_fast_equals_python(values, abundances, k, alive=None):
    """graph_fast over ``values`` (flat order, Python ints) against the Python statements over the alive ones -> the fast result"""
    vals = np.array(values, np.uint64); ab = np.array(abundances, np.int64)
    n = len(vals)
    got = gi.graph_fast(vals, ab, k, alive)
    idx = np.arange(n) if alive is None else np.flatnonzero(alive)
    sub = [int(values[i]) for i in idx]; sub_ab = [int(abundances[i]) for i in idx]
    masks = np.zeros(n, np.uint8); masks[idx] = graph_masks_np(sub, k)
    assert got["masks"].dtype == np.uint8 and np.array_equal(got["masks"], masks)
    assert got["topology"].dtype == np.uint64 and np.array_equal(got["topology"], topology_from_masks(masks[idx]))
    if alive is None:
        br = branching_from_masks(masks)
        want = count_records([v for v, b in zip(sub, br) if b], [a for a, b in zip(sub_ab, br) if b], k)
        assert np.array_equal(got["branching"], want.reshape(-1, 16))
    u = unitigs_np(sub, sub_ab, k)
    link = np.full(2 * n, -1, np.int64)
    t = np.flatnonzero(u["link"] != -1)
    link[2 * idx[t >> 1] + (t & 1)] = 2 * idx[u["link"][t] >> 1] + (u["link"][t] & 1)
    assert np.array_equal(got["link"], link)
    unitig = np.full(n, -1, np.int64); rev = np.zeros(n, bool); pos = np.zeros(n, np.int64)
    unitig[idx], rev[idx], pos[idx] = u["unitig"], u["reversed"], u["pos"]
    assert np.array_equal(got["unitig"], unitig) and np.array_equal(got["reversed"], rev) and np.array_equal(got["pos"], pos) and got["n_cycles"] == u["n_cycles"]
    for name in ("bases", "offsets", "kc"):
        assert got[name].dtype == u[name].dtype and np.array_equal(got[name], u[name]), name
    lo, links = csr(unitig_links_np(sub, k, u))
    assert got["link_offsets"].dtype == np.uint64 and got["links"].dtype == np.uint64
    assert np.array_equal(got["link_offsets"], lo) and np.array_equal(got["links"], links)
    return got


# ------------------------------------------------------------------------------------------------ 1. the fast statement
def test_revcomp_and_windows():
    rng = np.random.default_rng(1)
    for k in (1, 5, 21, 30, 31, 32):
        x = rng.integers(0, 1 << 62, 50, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1)
        assert gi.revcomp_np(x, k).tolist() == [revcomp(int(v), k) for v in x]
        codes = gi.rand(rng, 3, k + 7)
        w = gi.windows(codes, k)
        assert w.shape == (3, 8)
        assert w.tolist() == [[sum(int(c) << (2 * (k - 1 - t)) for t, c in enumerate(row[p: p + k])) for p in range(8)] for row in codes]


@pytest.mark.parametrize("name", ["k31_defaults", "k21_defaults_parts", "k21_freq_4parts"])
def test_fast_statement_on_the_fixtures(name):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    values = [v for p in parts for v, _ in p]; ab = [a for p in parts for _, a in p]
    got = assert_fast_equals_python(values, ab, k)
    assert len(got["lens"]) > 20 and len(got["links"]) > 0 and got["reversed"].any()


@pytest.fixture(scope="module")
def synth_reads():
    gkc = ge.load().gkc
    bases, offs = gkc.synth_reads_np(11, 1000, 100, 3000, 5000)
    return [bases[i * 100:(i + 1) * 100].tobytes().decode() for i in range(1000)]


@pytest.mark.parametrize("k", [5, 21, 31])
def test_fast_statement_on_synthetic_reads(synth_reads, k):
    values, ab = records_of_reads(synth_reads, k)
    got = assert_fast_equals_python(values, ab, k)
    assert (got["masks"] != 0).any() and len(got["links"]) > 0
    if k == 5:                                                  # nearly every 5-mer: self-loops, sides with four links
        assert len(values) > 400 and np.diff(got["link_offsets"].astype(np.int64)).max() == 4


@pytest.mark.parametrize("k,L", CYCLES)
def test_fast_statement_on_the_circles(k, L):
    seq, vals = circle(k, L)
    got = assert_fast_equals_python(vals, [1] * L, k)
    assert got["n_cycles"] == (0 if (k, L) == (5, 200) else 1)


def test_fast_statement_on_circles_in_lock_step_and_in_the_plain_loop():
    """more walkers than LOCK_STEP_MIN and fewer: both branches of paths_fast, with circles left over"""
    b = gi.circles_and_paths([40, 77], gi.lengths_for(600), 21, seed=3)
    assert b.n == 40 + 77 + 600 and b.n_unitigs == 2 + 300
    values, ab = records_of_reads(b.reads(), 21)
    got = assert_fast_equals_python(values, ab, 21)
    assert got["n_cycles"] == 2 and len(got["lens"]) == b.n_unitigs
    b = gi.circles_and_paths([50], [30, 7], 21, seed=3)
    values, ab = records_of_reads(b.reads(), 21)
    got = assert_fast_equals_python(values, ab, 21)
    assert got["n_cycles"] == 1 and sorted(got["lens"].tolist()) == [7, 30, 50]


def test_fast_statement_on_a_hairpin():
    values, ab = records_of_reads(hairpin_reads(), 21)
    got = assert_fast_equals_python(values, ab, 21)
    assert got["link_offsets"].tolist() == [0, 1, 1] and got["links"].tolist() == [1]


def test_fast_statement_over_a_hand_made_alive_subset(synth_reads):
    values, ab = records_of_reads(synth_reads, 21)
    rng = np.random.default_rng(8)
    alive = rng.random(len(values)) < 0.8
    alive[-3:] = False; alive[0] = False
    got = assert_fast_equals_python(values, ab, 21, alive)
    assert (got["unitig"][~alive] == -1).all() and not got["masks"][~alive].any()
    full = gi.masks_fast(np.array(values, np.uint64), 21)
    assert (full[alive] != got["masks"][alive]).any()           # some alive record lost a neighbour: no mask names a dead record


# ------------------------------------------------------------------------------------------------ 2. the constructions at 1 / 500 of their size
def python_graph(b):
    values, ab = records_of_reads(b.reads(), b.k)
    assert np.array_equal(np.array(values, np.uint64), np.sort(b.kmers))
    return values, ab


def test_lengths_for():
    for n in (1, 2, 5, 6, 7, 525, 1049):
        lens = gi.lengths_for(n)
        assert sum(lens) == n and set(lens) <= {1, 2, 3}
    assert sorted(gi.lengths_for(10, 7)) == [1, 1, 1, 1, 2, 2, 2]
    assert gi.lengths_for(7, 7) == [1] * 7 and gi.lengths_for(14, 7) == [2] * 7


@pytest.mark.parametrize("n", [524, 525, 1049])
def test_isolated_paths(n):
    lens = gi.lengths_for(n)
    b = gi.isolated_paths(lens, K, seed=n)
    assert b.n == n and b.n_unitigs == len(lens)
    values, ab = python_graph(b)
    assert len(values) == n and set(ab) == {1}
    got = assert_fast_equals_python(values, ab, K)
    assert sorted(got["lens"].tolist()) == sorted(lens) and len(got["links"]) == 0
    assert set(zip(*(d.tolist() for d in gi.degrees(got["masks"])))) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    bases, offs = b.pack()
    assert len(offs) == len(lens) + 1 and int(offs[-1]) == len(bases) == n + (K - 1) * len(lens) and bases.tobytes().decode() == "".join(b.reads())


def test_a_long_path_and_a_long_circle():
    b = gi.long_path(1200, K, seed=1)
    values, ab = python_graph(b)
    got = assert_fast_equals_python(values, ab, K)
    assert b.n == 1200 and got["lens"].tolist() == [1200] and got["n_cycles"] == 0
    b = gi.circles_and_paths([600], [], K, seed=2)
    values, ab = python_graph(b)
    got = assert_fast_equals_python(values, ab, K)
    assert b.n == 600 and got["lens"].tolist() == [600] and got["n_cycles"] == 1 and got["pos"][0] == 0 and not got["reversed"][0]
    assert got["link_offsets"].tolist() == [0, 1, 2] and got["links"].tolist() == [0, 1]
    b = gi.circles_and_paths([600, 40, 200], [1] * 600, K, seed=3)
    values, ab = python_graph(b)
    got = assert_fast_equals_python(values, ab, K)
    assert b.n == 1440 and b.n_unitigs == 603 == len(got["lens"]) and got["n_cycles"] == 3


def test_a_circle_over_c_and_g_stands_behind_seven_sixteenths_of_random_records():
    b = gi.circles_and_paths([], [1] * 2000, K, seed=4, high_circles=[41])
    values, ab = python_graph(b)
    got = assert_fast_equals_python(values, ab, K)
    assert b.n == 2041 and got["n_cycles"] == 1 and len(b.high) == 41 and int(b.high.min()) >= 4 ** K // 4
    at = np.flatnonzero(np.isin(np.array(values, np.uint64), b.high))
    assert len(at) == 41 and at.min() >= (7 / 16 - 0.05) * b.n and (got["unitig"][at] == got["unitig"][at[0]]).all()


STRUCTURES = dict(forks=5, tips=4, bubbles=3, ecs=4)


@pytest.fixture(scope="module")
def structures():
    b = gi.padding_plus_structures(gi.lengths_for(1100, 1050), K, seed=5, **STRUCTURES)
    values, ab = python_graph(b)
    return b, values, ab


def test_padding_plus_structures_counts(structures):
    b, values, ab = structures
    assert b.n == 1100 + gi.structure_records(K, **STRUCTURES) == len(values)
    got = assert_fast_equals_python(values, ab, K)
    assert len(got["lens"]) == b.n_unitigs == 1050 + 15 + 12 + 12 + 20
    assert sorted(set(ab)) == [1, gi.BUBBLE_COV, gi.EC_COV]
    assert [len(b.dies[kind]) for kind in ("tips", "bulges", "ec")] == [4, 3 * K, 4 * K]


def test_the_tips_die_as_claimed(structures):
    b, values, ab = structures
    r = tips_np(values, ab, K, tip_defaults(K, max_len_topo=K, max_len_rc=0))
    assert r["tips_per_round"] == [STRUCTURES["tips"], 0]
    alive = b.alive_after(values, ["tips"])
    assert np.array_equal(r["alive"], alive) and r["records_removed"] == STRUCTURES["tips"]
    assert len(r["u"]["seqs"]) == b.n_unitigs - 3 * STRUCTURES["tips"] + STRUCTURES["tips"]      # branch gone, the two arms one unitig
    assert_fast_equals_python(values, ab, K, alive)


@pytest.mark.parametrize("kinds,over", [(["bulges"], only("bulges", K)), (["ec"], only("ec", K)), (["tips", "bulges", "ec"], simplify_defaults(K, max_len_topo=K, max_len_rc=0))],
                         ids=["bulges", "ec", "simplify"])
def test_bulges_and_ecs_die_as_claimed(structures, kinds, over):
    b, values, ab = structures
    r = simplify_np(values, ab, K, over)
    log, alive = gi.expected_simplify_log(b, values, ab, over)
    assert r["log"] == log
    assert np.array_equal(alive, b.alive_after(values, kinds)) and np.array_equal(r["alive"], alive)
    first = {kind: sum(e[3] for e in r["log"] if e[0] == kind and e[1] <= 1) for kind in ("tips", "bulges", "ec")}
    assert first == dict(tips=STRUCTURES["tips"] * ("tips" in kinds), bulges=STRUCTURES["bubbles"] * ("bulges" in kinds), ec=STRUCTURES["ecs"] * ("ec" in kinds))


def test_a_resumed_call_after_the_tips(structures):
    """what tests/test_gpu_graph_sizes.py expects of simplify(resume=True) after remove_tips: the log of simplify_np from that alive state"""
    b, values, ab = structures
    p = simplify_defaults(K, max_len_topo=K, max_len_rc=0)
    full, alive = gi.expected_simplify_log(b, values, ab, p)
    r = simplify_np(values, ab, K, p, alive=b.alive_after(values, ["tips"]))
    assert full[0][3] == STRUCTURES["tips"] and r["log"] == full[1:] and np.array_equal(r["alive"], alive)


# ------------------------------------------------------------------------------------------------ 3. wide keys
def test_the_k33_closed_form_equals_the_statement():
    k = 33
    bases, offs, exp = gi.wide_isolated_paths(gi.lengths_for(600), seed=4)
    assert len(offs) == 301 and exp["n"] == 600
    values, ab = records_of_reads(exp["reads"], k)
    assert [int(a) | (int(b) << 64) for a, b in zip(exp["lo"].tolist(), exp["hi"].tolist())] == values and set(ab) == {1}
    assert np.array_equal(exp["masks"], graph_masks_np(values, k))
    u = unitigs_np(values, ab, k)
    for name in ("bases", "offsets", "kc", "unitig", "reversed", "pos"):
        assert exp[name].dtype == u[name].dtype and np.array_equal(exp[name], u[name]), name
    assert u["n_cycles"] == 0 and exp["reversed"].any() and not exp["reversed"].all()
    assert unitig_links_np(values, k, u) == [[]] * 600
