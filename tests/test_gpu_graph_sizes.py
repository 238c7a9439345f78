"""The graph kernels past one grid pass (csrc/gkc_graph.hip, csrc/gkc_unitigs.hip, csrc/gkc_unitig_links.hip, csrc/gkc_simplify.hip: "grids are capped and the kernels stride"). The launch geometry: thread-per-element
grids are capped at 2048 workgroups of 256 threads and stride above 524,288 elements (records, unitigs, slots; the ranking runs over 2 n states: n > 262,144); the three
one-workgroup scans take 256 tile sums of 1024 elements per trip and carry a running total above 262,144 records (the link scan: above 131,072 unitigs, two slots each);
the tile kernels stride above 2048 tiles (n > 2,097,152 records, the link tile kernels above 1,048,576 unitigs). The other graph tests stay below 6 * 10^4 records. Here
every size sits on such a border, made exact by the constructions of tests/graph_inputs.py, and every array the API returns — masks, topology, branching records, the
counts of unitigs_build, bases, offsets, KC, the placement of every record, link offsets and links, alive, simplified masks, the per-round logs — is compared byte for
byte with the fast numpy statement of tests/graph_inputs.py, which tests/test_graph_sizes_cpu.py pins to the per-record Python statements.

Not covered: the stride of k_tip_refresh itself, which needs more than 524,288 listed slots on one side, i.e. some 6 * 10^5 real tips over 3 * 10^6 records, for a loop
whose body the tip tests exercise; n >= 2^31.

The whole file: 26 tests in 40 s on an MI355X machine, nearly all of it the numpy statement on the host: 3.7 s for each of the three tile-stride cases (2.1 * 10^6
records), 8.3 s for the tips test, which computes the statement of section 4's input (1.18 * 10^6 records) over its first alive states and shares them with the three
tests after it (1.3 to 2.4 s each); every other case is below 1.1 s. No case needs more than a fraction of a second of device time.
Run with `pytest -m gpu`."""
import numpy as np
import pytest

import __graft_entry__ as ge
from tests import graph_inputs as gi
from tests.test_gpu_graph import branching_raw, counter_for
from tests.test_simplify_cpu import default_params as simplify_defaults, only

pytestmark = pytest.mark.gpu
K, M = 31, 8
TILE, THREADS, GRID_MAX = 1024, 256, 2048                        # GR_TILE, GR_THREADS, QR_GRID_MAX
PASS = GRID_MAX * THREADS                                       # 524,288 elements in one pass of a thread-per-element grid
CARRY = THREADS * TILE                                          # 262,144 elements in one trip of a one-workgroup scan
TILE_PASS = GRID_MAX * TILE                                     # 2,097,152 elements in one pass of a tile grid
DEAD = np.uint64((1 << 64) - 1)


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def counted(gkc, b, n, parts=7, passes=1, m=M):
    """the Counter over a constructed input, and its records in flat order: exactly n of them, the construction's k-mers -> (counter, values, abundances, sizes)"""
    bases, offs = b.pack()
    c = counter_for(gkc, bases, offs, b.k, m, parts, passes)
    values, hi, ab, sizes = gi.records_of_counter(c)
    assert len(values) == n == b.n == c.stats()["kmers_nb_solid"] and not hi.any()
    assert np.array_equal(np.sort(values), np.sort(b.kmers))
    return c, values, ab, sizes


def assert_neighbourhoods(gkc, c, exp):
    """masks, topology, branching records -> the number of branching records"""
    got = c.neighbor_masks()
    bad = np.flatnonzero(got != exp["masks"]) if len(got) == len(exp["masks"]) else None
    assert bad is not None and len(bad) == 0, (len(got), None if bad is None else (len(bad), bad[:10], got[bad[:10]], exp["masks"][bad[:10]]))
    assert np.array_equal(c.graph_topology(), exp["topology"])
    nb = len(exp["branching"])
    rc, got_n, recs, topo = branching_raw(gkc, c, None, nb, nb + 2)
    assert rc == 0 and got_n == nb and np.array_equal(topo, exp["topology"])
    assert np.array_equal(recs[:nb], exp["branching"]) and (recs[nb:] == 0xEE).all()
    return nb


def assert_placement(c, exp, got):
    """got: (bases, offsets, kc, link offsets, links) as the device wrote them, and the placement the context holds, against the fast statement"""
    bases, offs, kc, lo, links = got
    assert bases.dtype == np.uint8 and offs.dtype == np.uint64 and kc.dtype == np.uint64 and lo.dtype == np.uint64 and links.dtype == np.uint64
    assert np.array_equal(offs, exp["offsets"])
    bad = np.flatnonzero(bases != exp["bases"]) if len(bases) == len(exp["bases"]) else None
    assert bad is not None and len(bad) == 0, (len(bases), len(exp["bases"]), None if bad is None else bad[:10])
    assert np.array_equal(kc, exp["kc"])
    un, rev, pos = c.unitig_of_records()
    want = np.where(exp["unitig"] < 0, DEAD, exp["unitig"].astype(np.uint64))
    assert np.array_equal(un, want) and np.array_equal(rev, exp["reversed"]) and np.array_equal(pos.astype(np.int64), exp["pos"])
    assert np.array_equal(lo, exp["link_offsets"]) and np.array_equal(links, exp["links"])


def assert_unitigs_and_links(c, exp):
    counts = c.unitigs_build()
    assert counts == (len(exp["lens"]), len(exp["bases"]), exp["n_cycles"])
    assert_placement(c, exp, c.unitigs() + c.unitig_links())


def assert_whole_graph(gkc, c, values, ab, k=K):
    exp = gi.graph_fast(values, ab, k)
    assert_neighbourhoods(gkc, c, exp)
    assert_unitigs_and_links(c, exp)
    return exp


# ------------------------------------------------------------------------------------------------ 1. the borders of the scans and of the ranking
@pytest.mark.parametrize("n", [CARRY - 1, CARRY, CARRY + 1, PASS - 1, PASS, PASS + 1])
def test_isolated_paths_at_the_scan_and_pass_borders(gkc, n):
    """256 / 257 and 512 / 513 tiles; the last element of the first grid pass and the first of the second. Isolated paths of 1 to 3 records: every record is (0,0), (0,1),
    (1,0) or (1,1), most of them branch, the gather is dense"""
    lens = gi.lengths_for(n)
    b = gi.isolated_paths(lens, K, seed=n)
    c, values, ab, sizes = counted(gkc, b, n)
    exp = assert_whole_graph(gkc, c, values, ab)
    assert len(exp["lens"]) == len(lens) and len(exp["links"]) == 0
    nb = len(exp["branching"])
    assert nb > n // 2 and int(exp["topology"].sum()) == n and exp["topology"][[0, 0, 1, 1], [0, 1, 0, 1]].all()
    if n in (CARRY + 1, PASS + 1):                              # room for one record too few: error 4, the count still reported, nothing written past the capacity
        rc, got_n, recs, _ = branching_raw(gkc, c, None, nb - 1, nb + 2)
        assert rc == 4 and got_n == nb and b"branching" in c.L.gkc_last_error(c.h)
        assert np.array_equal(recs[: nb - 1], exp["branching"][: nb - 1]) and (recs[nb - 1:] == 0xEE).all()
    c.close()


# ------------------------------------------------------------------------------------------------ 2. the borders of the unitigs and of their slots
N_FORKS = 2000


@pytest.mark.parametrize("n_unitigs", [CARRY // 2, CARRY // 2 + 1, PASS // 2, PASS // 2 + 1, PASS, PASS + 1])
def test_unitig_and_slot_borders(gkc, n_unitigs):
    """one record per padding read and 2000 forks: the link scan's carry (131,072 unitigs = 256 tiles of slots), the per-slot pass (262,144 unitigs) and the per-unitig
    pass (524,288 unitigs), with link entries on both sides of every border that lies inside"""
    n_pad = n_unitigs - 3 * N_FORKS
    n = n_pad + 9 * N_FORKS
    b = gi.padding_plus_structures([1] * n_pad, K, seed=n_unitigs, forks=N_FORKS)
    c, values, ab, sizes = counted(gkc, b, n)
    exp = assert_whole_graph(gkc, c, values, ab)
    assert len(exp["lens"]) == n_unitigs == b.n_unitigs and len(exp["links"]) == 4 * N_FORKS
    filled = np.flatnonzero(np.diff(exp["link_offsets"].astype(np.int64)))
    for border in (CARRY, PASS, 2 * PASS):                      # in slots
        if border < 2 * n_unitigs - 2000:
            assert filled.min() < border < filled.max()
    c.close()


# ------------------------------------------------------------------------------------------------ 3. ranking at length
def test_a_path_of_600000_records(gkc):
    n = 600000
    b = gi.long_path(n, K, seed=6)
    c, values, ab, sizes = counted(gkc, b, n, parts=4)
    exp = assert_whole_graph(gkc, c, values, ab)
    rounds = c.timing("graph_rank")[1]
    c.unitigs_build()
    assert c.timing("graph_rank")[1] - rounds >= 20             # 2^19 < n: twenty rounds of pointer jumping, each with three trips over the 2 n states
    assert exp["lens"].tolist() == [n] and exp["n_cycles"] == 0 and sorted(exp["pos"].tolist()) == list(range(n))
    c.close()


def test_a_circle_of_300000_records(gkc):
    n = 300000
    b = gi.circles_and_paths([n], [], K, seed=7)
    c, values, ab, sizes = counted(gkc, b, n, parts=4)
    exp = assert_whole_graph(gkc, c, values, ab)
    assert c.unitigs_build() == (1, n + K - 1, 1)
    un, rev, pos = c.unitig_of_records()
    assert pos[0] == 0 and not rev[0] and not un.any()          # one unitig, cut at the left end of the smallest record, which stands forward
    assert exp["link_offsets"].tolist() == [0, 1, 2] and exp["links"].tolist() == [0, 1]
    c.close()


def test_that_circle_among_padding_and_two_small_circles(gkc):
    n = 300000 + 40 + 200 + 300000
    b = gi.circles_and_paths([300000, 40, 200], [1] * 300000, K, seed=8)
    c, values, ab, sizes = counted(gkc, b, n)
    exp = assert_whole_graph(gkc, c, values, ab)
    assert exp["n_cycles"] == 3 and sorted(exp["lens"].tolist())[-3:] == [40, 200, 300000] and len(exp["lens"]) == 300003
    c.close()


def test_a_circle_whose_states_all_lie_past_the_first_trip(gkc):
    """the vote "some state still walks" of the trips after the first. 700,000 single records, whose walks end at once, and one circle of 41 records over C and G in one
    dataset: the circle's records stand behind the first 7 / 16 of the others, so all its states lie beyond the 524,288 states of the first trip, and from the first
    round on they are the only ones that walk. (41 is prime and not 2^j + 1: a ranking that ended early cannot pass the build's own check of the lengths by accident.)"""
    n_pad, L = 700000, 41
    b = gi.circles_and_paths([], [1] * n_pad, K, seed=13, high_circles=[L])
    c, values, ab, sizes = counted(gkc, b, n_pad + L, parts=1)
    at = np.flatnonzero(np.isin(values, b.high))
    assert len(at) == L and 2 * at.min() >= PASS
    exp = assert_whole_graph(gkc, c, values, ab)
    assert exp["n_cycles"] == 1 and exp["lens"][exp["unitig"][at[0]]] == L and exp["pos"][at[0]] == 0 and not exp["reversed"][at[0]]
    c.close()


# ------------------------------------------------------------------------------------------------ 4. tips, bulges and erroneous connections past one pass
STRUCTURES = dict(forks=1000, tips=2000, bubbles=1500, ecs=1500)
# a bubble's or a connector's branch of k records starts at the smaller of its two end records, whose values cannot both be large (they share a base): its index is
# never among the highest, so there are about twice as many unitigs as one pass holds and the border lies near their middle
N_PAD = 1000000
TOPO = dict(max_len_topo=K, max_len_rc=0)                        # a tip is a dead end of at most k bases: one record


class Simplified:
    """the input of section 4, made once: more than 524,288 records and more than 524,288 unitigs before and after every removal; the fast statement per alive state"""

    def __init__(self):
        self.b = gi.padding_plus_structures([1] * N_PAD, K, seed=9, **STRUCTURES)
        self.n = N_PAD + gi.structure_records(K, **STRUCTURES)
        self.values = None
        self.cache, self.n_unitigs = {}, {}                      # per alive state: the fast statement / its number of unitigs

    def counter(self, gkc):
        c, values, ab, sizes = counted(gkc, self.b, self.n)
        if self.values is None:
            self.values, self.ab = values, ab
        assert np.array_equal(values, self.values)
        return c

    def graph(self, kinds):
        """-> (alive, graph_fast over the survivors of ``kinds``)"""
        if kinds not in self.cache:
            alive = self.b.alive_after(self.values, kinds)
            self.cache[kinds] = (alive, gi.graph_fast(self.values, self.ab, K, alive))
        return self.cache[kinds]

    def hits_on_both_sides(self, before, kind):
        """the unitigs that ``kind`` removes from the graph over the survivors of ``before`` have indices below and above one pass of a per-unitig grid"""
        _, g = self.graph(before)
        u = np.unique(g["unitig"][np.isin(self.values, self.b.dies[kind]) & (g["unitig"] >= 0)])
        assert len(u) == self.b.counts[{"tips": "tips", "bulges": "bubbles", "ec": "ecs"}[kind]] and u.min() < PASS < u.max(), (kind, len(u), u.min(), u.max())

    def assert_state(self, c, got, kinds):
        alive, g = self.graph(kinds)
        assert got["alive"].dtype == bool and np.array_equal(got["alive"], alive)
        assert np.array_equal(c.simplified_masks(), g["masks"])
        assert (got["n_unitigs"], got["n_bases"], got["n_cycles"]) == (len(g["lens"]), len(g["bases"]), 0)
        assert len(g["lens"]) > PASS and int(alive.sum()) > PASS
        assert_placement(c, g, c.simplified_unitigs())


@pytest.fixture(scope="module")
def simplified():
    return Simplified()


def test_tips_past_one_pass_and_a_resumed_simplify(gkc, simplified):
    s = simplified
    c = s.counter(gkc)
    s.hits_on_both_sides((), "tips")
    got = c.remove_tips(**TOPO)
    assert got["tips_per_round"] == [STRUCTURES["tips"], 0] and got["rounds"] == 2 and got["records_removed"] == STRUCTURES["tips"]
    s.assert_state(c, got, ("tips",))
    # the state remove_tips left, resumed (k_alive_count with the masks, over more than one pass): the log of the whole call without its first round
    p = simplify_defaults(K, **TOPO)
    log, alive = gi.expected_simplify_log(s.b, s.values, s.ab, p, s.n_unitigs)
    got = c.simplify(resume=True, **TOPO)
    assert got["log"] == log[1:] and got["rounds"] == len(log) - 1 and got["records_removed"] == sum(e[4] for e in log[1:])
    s.assert_state(c, got, ("tips", "bulges", "ec"))
    c.close()


@pytest.mark.parametrize("kind", ["bulges", "ec"])
def test_one_kind_alone_past_one_pass(gkc, simplified, kind):
    s = simplified
    c = s.counter(gkc)
    s.hits_on_both_sides((), kind)
    p = only(kind, K)
    log, alive = gi.expected_simplify_log(s.b, s.values, s.ab, p, s.n_unitigs)
    got = c.remove_bulges() if kind == "bulges" else c.remove_erroneous_connections()
    n_hits = STRUCTURES["bubbles" if kind == "bulges" else "ecs"]
    assert got["log"] == log and [e[3] for e in log] == [n_hits, 0, 0] and got["records_removed"] == n_hits * K
    s.assert_state(c, got, (kind,))
    c.close()


def test_simplify_past_one_pass(gkc, simplified):
    s = simplified
    c = s.counter(gkc)
    s.hits_on_both_sides(("tips",), "bulges"); s.hits_on_both_sides(("tips", "bulges"), "ec")
    log, alive = gi.expected_simplify_log(s.b, s.values, s.ab, simplify_defaults(K, **TOPO), s.n_unitigs)
    got = c.simplify(**TOPO)
    assert got["log"] == log and got["rounds"] == len(log) and got["records_removed"] == int((~alive).sum())
    assert [(e[0], e[1], e[3]) for e in log if e[3]] == [("tips", 0, STRUCTURES["tips"]), ("bulges", 1, STRUCTURES["bubbles"]), ("ec", 1, STRUCTURES["ecs"])]
    s.assert_state(c, got, ("tips", "bulges", "ec"))
    c.close()


# ------------------------------------------------------------------------------------------------ 5. the tile grids stride
@pytest.mark.parametrize("n", [TILE_PASS, TILE_PASS + 1, TILE_PASS + 3 * TILE + 17], ids=["2048_tiles", "one_more_record", "partial_last_tile"])
def test_the_tile_grids_stride(gkc, n):
    """2048 tiles exactly; one record in tile 2049; a partial last tile in the second pass. 1,200,000 unitigs: the link tile kernels stride too"""
    n_forks, n_unitigs = 3000, 1200000
    assert 2 * n_unitigs > TILE_PASS
    b = gi.padding_plus_structures(gi.lengths_for(n - 9 * n_forks, n_unitigs - 3 * n_forks), K, seed=10, forks=n_forks)
    c, values, ab, sizes = counted(gkc, b, n)
    exp = assert_whole_graph(gkc, c, values, ab)
    assert len(exp["lens"]) == n_unitigs and len(exp["links"]) == 4 * n_forks
    filled = np.flatnonzero(np.diff(exp["link_offsets"].astype(np.int64)))
    assert filled.min() < TILE_PASS < filled.max()
    c.close()


# ------------------------------------------------------------------------------------------------ 6. wide keys, two passes, 512 partitions
def test_wide_keys_past_one_pass(gkc):
    """k = 33: two words per key, one dataset, the closed form of gi.wide_isolated_paths"""
    import torch
    n, k = PASS + 1, 33
    lens = gi.lengths_for(n)
    bases, offs, exp = gi.wide_isolated_paths(lens, seed=11)
    c = counter_for(gkc, bases, offs, k, M, 1)
    lo, hi, ab = c.partition(0, 0)
    assert len(lo) == n == exp["n"] and np.array_equal(lo, exp["lo"]) and np.array_equal(hi, exp["hi"]) and (ab == 1).all()
    masks = c.neighbor_masks()
    assert np.array_equal(masks, exp["masks"]) and np.array_equal(c.graph_topology(), gi.topology_fast(exp["masks"]))
    br = gi.branching_fast(exp["masks"])
    blo, bhi, bab = c.branching_nodes(sort=False)
    assert np.array_equal(blo, exp["lo"][br]) and np.array_equal(bhi, exp["hi"][br]) and (bab == 1).all() and len(blo) > n // 2
    assert c.unitigs_build() == (len(lens), n + (k - 1) * len(lens), 0)
    exp.update(link_offsets=np.zeros(2 * len(lens) + 1, np.uint64), links=np.zeros(0, np.uint64))
    assert_placement(c, exp, c.unitigs() + c.unitig_links())
    c.close()


@pytest.mark.parametrize("parts,passes", [(7, 2), (512, 1)], ids=["two_passes", "512_partitions"])
def test_many_datasets_past_one_pass(gkc, parts, passes):
    """the dataset of a record and its index inside it (gr_dataset_of, i - D.base) beyond the first pass: two passes, and 512 partitions of which a third is empty"""
    n = PASS + 1
    b = gi.isolated_paths(gi.lengths_for(n), K, seed=12)
    c, values, ab, sizes = counted(gkc, b, n, parts=parts, passes=passes)
    assert len(sizes) == parts * passes and (sizes.count(0) > 100 if parts == 512 else min(sizes) > 0)
    assert_whole_graph(gkc, c, values, ab)
    c.close()
