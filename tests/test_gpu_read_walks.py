"""Read walks on the device (csrc/gkc_paths.hip: k_walk_junctions, k_walk_fill; gkc_graph_reads_walks_device; gkc.Counter.read_walks, read_walks_device, write_gfa).
Expected values: the plain Python statement of tests/test_read_walks_cpu.py (pinned there on the reference-run fixtures) over the unitig strings the device wrote and
their (k-1)-overlaps, and, past the sizes a Python loop serves, np.tile of that statement over a tiled input. Every comparison is exact.
Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import graph_inputs as gi
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_read_paths import fixture_counter, unitig_strings
from tests.test_gpu_tips import counter_of_reads
from tests.test_read_paths_cpu import SEGMENT, pack, random_sequence, rc_str
from tests.test_read_walks_cpu import BREAK, COLLINEAR, END, UNLINKED, WALK, fixture_walks, junction_counts, walks_over
from tests.test_reference_run import DIR
from tests.test_simplify_cpu import K as K_SIMPLIFY, branches_of, bubble_reads
from tests.test_unitig_links_cpu import overlap_links
from tests.util import simple_repart

pytestmark = pytest.mark.gpu
WORD = 64                                                       # segments per word of end bits: one wave
TILE = 1024 * WORD                                              # segments per tile of the numbering (GR_TILE words)
PASS = 2048 * 256                                               # segments in one pass of the per-segment kernels' grid (q_grid: 2048 workgroups of 4 waves)
SCAN = 256 * TILE                                               # segments the one-workgroup scan of the tile sums covers before it carries (GR_THREADS tiles)
KEYS = ("seg_offsets", "segments", "junction", "walk_offsets", "walks", "link_offsets", "links", "link_support")


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def assert_walks(got, exp):
    """what Counter.read_walks returned against the statement, entry for entry"""
    assert sorted(got) == sorted(KEYS)
    assert got["segments"].dtype == SEGMENT and got["walks"].dtype == WALK and all(got[n].dtype == np.uint64 for n in KEYS if n not in ("segments", "walks"))
    for n in KEYS:
        assert len(got[n]) == len(exp[n]) and np.array_equal(got[n], exp[n]), (n, len(got[n]), len(exp[n]))


def device_inputs(c, bases, offs):
    """the nodes call and the segments calls for the reads, and the links of the placement c built last, all left on the device -> dict: so (int64[n_reads + 1]),
    seg (bytes), nr, ns, lo, lk, nl"""
    import torch
    to, nr, nb, node, pos = c._read_nodes_tensors(bases, offs)
    ns = c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb)
    so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(max(ns, 1) * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns) == ns
    masks = c._placement_masks
    keep, d_masks = c._masks_once(None if masks is None else masks.data_ptr())
    lo, lk = c._unitig_links_of_placement(c._placement_nu, d_masks)
    return dict(so=so, seg=seg[: ns * 24] if ns else seg, nr=nr, ns=ns, lo=lo, lk=lk, nl=len(lk))


def walks_raw(c, D, room_walks, cap_walks=None, junction=True, support=True, offsets=True, walks=True, canary=0xEE, **over):
    """the export over buffers pre-filled with ``canary`` and 64 bytes longer than needed -> dict(rc, n_walks, junction, walk_offsets, walks, support: the raw bytes).
    over: entries of D replaced for this call"""
    import torch
    D = dict(D, **over)
    nr, ns, nl = D["nr"], D["ns"], D["nl"]
    jn, wo, wk, sup = (torch.full((n + 64,), canary, dtype=torch.uint8, device="cuda") for n in (ns * 8, (nr + 1) * 8, room_walks * 16, nl * 8))
    torch.cuda.synchronize()
    n = C.c_uint64(0xDEAD)
    rc = c.L.gkc_graph_reads_walks_device(c.h, D["so"].data_ptr(), D["seg"].data_ptr(), nr, ns, D["lo"].data_ptr(), D["lk"].data_ptr(), nl, jn.data_ptr() if junction else None,
                                          wo.data_ptr() if offsets else None, wk.data_ptr() if walks else None, room_walks if cap_walks is None else cap_walks, C.byref(n),
                                          sup.data_ptr() if support else None)
    return dict(rc=rc, n_walks=n.value, junction=jn.cpu().numpy(), walk_offsets=wo.cpu().numpy(), walks=wk.cpu().numpy(), support=sup.cpu().numpy())


def untouched(out, *names):
    return all((out[n] == 0xEE).all() for n in (names or ("junction", "walk_offsets", "walks", "support")))


def assert_raw(out, exp, D):
    """a call that wrote everything: the results, and the canary bytes behind every buffer"""
    nr, ns, nl, nw = D["nr"], D["ns"], D["nl"], len(exp["walks"])
    assert out["rc"] == 0 and out["n_walks"] == nw
    assert np.array_equal(out["junction"][: ns * 8].view(np.uint64), exp["junction"]) and (out["junction"][ns * 8:] == 0xEE).all()
    assert np.array_equal(out["walk_offsets"][: (nr + 1) * 8].view(np.uint64), exp["walk_offsets"]) and (out["walk_offsets"][(nr + 1) * 8:] == 0xEE).all()
    assert np.array_equal(out["walks"][: nw * 16].view(WALK), exp["walks"]) and (out["walks"][nw * 16:] == 0xEE).all()
    assert np.array_equal(out["support"][: nl * 8].view(np.uint64), exp["link_support"]) and (out["support"][nl * 8:] == 0xEE).all()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def upload(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------------------------------------ 1. the fixtures' own reads: 8-byte and 16-byte keys
@pytest.mark.parametrize("name", ["k21_freq_4parts", "k31_defaults", "k63_defaults"])
def test_the_fixture_reads_against_the_statement(gkc, name):
    c, k = fixture_counter(gkc, name)
    z = np.load(os.path.join(DIR, name + ".npz"))
    bases, offs, consumed = c.fastx_parse(bytes(z["fasta"]))
    assert consumed == len(z["fasta"])
    seqs = unitig_strings(*c.unitigs()[:2])
    _, fb, fo, fs, slots, exp = fixture_walks(name)
    assert np.array_equal(fb, bases) and np.array_equal(fo, offs) and fs == seqs
    got = c.read_walks(bases, offs)
    assert_walks(got, exp)
    counts = junction_counts(got["junction"])
    print("%s: %d segments, %d walks; link, unlinked, collinear, break, end = %s" % (name, len(got["segments"]), len(got["walks"]), counts))
    assert counts[0] and counts[1] == 0 and counts[2] and counts[3]
    D = device_inputs(c, bases, offs)
    assert np.array_equal(u64(D["lo"]), exp["link_offsets"]) and np.array_equal(u64(D["lk"]), exp["links"])
    assert_raw(walks_raw(c, D, len(exp["walks"])), exp, D)
    c.close()


def test_write_gfa(gkc, tmp_path):
    name = "k31_defaults"
    c, k = fixture_counter(gkc, name)
    _, bases, offs, seqs, slots, exp = fixture_walks(name)
    _, _, kc = c.unitigs()
    paths = []
    for r in range(len(offs) - 1):
        for i, x in enumerate(exp["walks"][int(exp["walk_offsets"][r]): int(exp["walk_offsets"][r + 1])]):
            if x["n_segments"] >= 2:
                paths.append(("r%d_%d" % (r, i), exp["segments"]["node"][int(x["first_segment"]): int(x["first_segment"]) + int(x["n_segments"])].tolist()))
    p = str(tmp_path / "g.gfa")
    assert c.write_gfa(p, reads=(bases, offs)) == (len(seqs), len(exp["links"]), len(paths)) and len(paths) > 0
    assert open(p).read() == gkc.gfa_text(k, seqs, kc, exp["link_offsets"], exp["links"], paths)
    assert c.write_gfa(p) == (len(seqs), len(exp["links"]), 0)
    assert open(p).read() == gkc.gfa_text(k, seqs, kc, exp["link_offsets"], exp["links"])
    c.close()


# ------------------------------------------------------------------------------------------------ 2. the simplified placement
def forked_bubble_reads(k):
    """three parallel branches of k records between two arms (tests/test_simplify_cpu.py: the lesser two are bulges), and behind the right arm a fork of two equally
    covered branches too long to be tips: the simplified graph keeps the links of the fork -> (reads counted, reads asked)"""
    branches = branches_of([k, k, k], [5, 2, 1], seed=7)
    reads, left, right = bubble_reads(branches, seed=7)
    f1, f2 = "A" + random_sequence(71, 299), "C" + random_sequence(72, 299)
    reads = reads + [right[-(k - 1):] + f1] * 3 + [right[-(k - 1):] + f2] * 3
    through_the_removed = left[-60:] + branches[2][0] + right[:60]
    asked = reads + [through_the_removed, rc_str(through_the_removed), right[-60:] + f1[:60], rc_str(right[-60:] + f2[:60]), left + branches[0][0] + right + f2]
    return reads, asked


@pytest.mark.parametrize("name", ["three_branches", "k21_freq_4parts"])
def test_walks_on_the_simplified_graph(gkc, name):
    if name == "three_branches":
        k = K_SIMPLIFY
        reads, asked = forked_bubble_reads(k)
        c = counter_of_reads(gkc, reads, k=k)
        bases, offs = pack(asked)
    else:
        c, k = fixture_counter(gkc, name)
        z = np.load(os.path.join(DIR, name + ".npz"))
        bases, offs, _ = c.fastx_parse(bytes(z["fasta"]))
    vals, _, _ = solid_records(c)
    got = c.simplify()
    assert 0 < got["records_removed"] < len(vals)
    ub, uo, _, lo, lk = c.simplified_unitigs()
    seqs = unitig_strings(ub, uo)
    exp = walks_over(bases, offs, seqs, k, set(vals), overlap_links(seqs, k))
    assert np.array_equal(lo, exp["link_offsets"]) and np.array_equal(lk, exp["links"])
    res = c.read_walks(bases, offs)
    assert_walks(res, exp)
    counts = junction_counts(res["junction"])
    print("%s simplified: %d unitigs, %d links, %d segments, %d walks; link, unlinked, collinear, break, end = %s" % (name, len(seqs), len(lk), len(res["segments"]), len(res["walks"]), counts))
    if name == "three_branches":
        assert len(lk) > 0 and counts[0] >= 3 and counts[1] == 0 and counts[2] >= 2      # links kept and followed; COLLINEAR over the removed same-length bulge, both ways
        assert res["walks"]["n_segments"].max() >= 2 and res["link_support"].sum() == counts[0]
    else:
        assert len(seqs) == 40 and len(lk) == 0 and len(res["link_support"]) == 0
        sg = res["segments"]
        for r in range(len(offs) - 1):                          # no link: no two segments of a read touch
            a = sg[int(res["seg_offsets"][r]): int(res["seg_offsets"][r + 1])]
            assert (a["read_pos"][1:].astype(np.int64) > a["read_pos"][:-1].astype(np.int64) + a["n_kmers"][:-1].astype(np.int64)).all()
        assert counts[0] == 0 and counts[1] == 0 and (res["walks"]["n_segments"] == 1).all() and len(res["walks"]) == len(sg)
        assert np.array_equal(res["walks"]["first_segment"], np.arange(len(sg), dtype=np.uint64)) and np.array_equal(res["walks"]["n_kmers"], sg["n_kmers"])
    D = device_inputs(c, bases, offs)
    assert_raw(walks_raw(c, D, len(exp["walks"])), exp, D)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. exact sizes
K_SNP, M_SNP = 31, 8


@pytest.fixture(scope="module")
def snp_graph(gkc):
    """a random genome of 9000 bases and its twin with another base every 100 bases, both counted: a chain of bubbles. The genome as one read is ONE walk that
    alternates between the shared stretches and its own alleles -> (counter, genome, unitig strings, solid set, overlap slots, segments of that walk)"""
    k = K_SNP
    genome = random_sequence(51, 9000)
    twin = list(genome)
    for at in range(100, 8950, 100):
        twin[at] = "ACGT"[("ACGT".index(genome[at]) + 1 + at // 100 % 3) % 4]
    bases, offs = pack([genome, "".join(twin)])
    c = counter_for(gkc, bases, offs, k, M_SNP, 4)
    vals, _, _ = solid_records(c)
    seqs = unitig_strings(*c.unitigs()[:2])
    slots = overlap_links(seqs, k)
    one = walks_over(*pack([genome]), seqs, k, set(vals), slots)
    W = len(one["segments"])
    assert W > 2 * WORD and one["walks"].tolist() == [(0, W, 9000 - k + 1)] and (one["junction"][:-1] < np.uint64(UNLINKED)).all()
    yield c, genome, seqs, set(vals), slots, W
    c.close()


def short_read(genome):
    return genome[10:60]                                        # inside the first shared stretch: one segment


@pytest.mark.parametrize("p", [0, 1, 62, 63, 64, 65])
def test_a_long_walk_on_every_phase_of_a_word(gkc, snp_graph, p):
    """p one-segment reads in front of the genome: its walk starts on bit p of the end words, the one-segment walks end on every bit up to 63 and start on bit 0"""
    c, genome, seqs, solid, slots, W = snp_graph
    bases, offs = pack([short_read(genome)] * p + [genome])
    exp = walks_over(bases, offs, seqs, K_SNP, solid, slots)
    assert len(exp["segments"]) == p + W and exp["walks"].tolist() == [(i, 1, 50 - K_SNP + 1) for i in range(p)] + [(p, W, 9000 - K_SNP + 1)]
    assert_walks(c.read_walks(bases, offs), exp)
    D = device_inputs(c, bases, offs)
    assert_raw(walks_raw(c, D, p + 1), exp, D)


@pytest.mark.parametrize("border", [TILE, PASS, SCAN], ids=["tile", "grid_pass", "scan_carry"])
def test_a_long_walk_across_the_larger_borders(gkc, snp_graph, border):
    """the segments of (p short reads, the genome) tiled on the device until they pass the border, p chosen so that a copy of the long walk straddles it. Segments
    hold read-relative positions: only seg_offsets and first_segment shift from copy to copy"""
    import torch
    assert (TILE, PASS, SCAN) == (65536, 524288, 16777216)
    c, genome, seqs, solid, slots, W = snp_graph
    p = next(p for p in range(1, 64) if p < border % (p + W) < p + W - 1)
    B = p + W
    bases, offs = pack([short_read(genome)] * p + [genome])
    exp = walks_over(bases, offs, seqs, K_SNP, solid, slots)
    D = device_inputs(c, bases, offs)
    assert D["ns"] == B and np.array_equal(u64(D["so"]), exp["seg_offsets"])
    reps = border // B + 2
    start = (border // B) * B + p
    assert start < border < start + W - 1 and reps * B > border + W      # the walk of copy border // B lies on both sides
    ns, nr = reps * B, reps * (p + 1)
    so = np.concatenate([[0], (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(B) + exp["seg_offsets"][None, 1:]).reshape(-1)]).astype(np.uint64)
    big = dict(D, so=upload(so), seg=D["seg"].repeat(reps), nr=nr, ns=ns)
    jn = torch.zeros(ns, dtype=torch.int64, device="cuda"); wo = torch.zeros(nr + 1, dtype=torch.int64, device="cuda")
    wk = torch.zeros(nr * 16, dtype=torch.uint8, device="cuda"); sup = torch.zeros(max(D["nl"], 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = (big["so"].data_ptr(), big["seg"].data_ptr(), nr, ns, D["lo"].data_ptr(), D["lk"].data_ptr(), D["nl"])
    assert c.read_walks_device(*args) == nr                     # every read is one walk
    assert c.read_walks_device(*args, jn.data_ptr(), wo.data_ptr(), wk.data_ptr(), nr, sup.data_ptr()) == nr
    assert np.array_equal(u64(jn), np.tile(exp["junction"], reps))
    assert np.array_equal(u64(wo), np.arange(nr + 1, dtype=np.uint64))
    want = np.tile(exp["walks"], reps)
    want["first_segment"] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(B), p + 1)
    got = wk.cpu().numpy().view(WALK)
    assert np.array_equal(got, want)
    assert got[(border // B) * (p + 1) + p].tolist() == (start, W, 9000 - K_SNP + 1)
    assert np.array_equal(u64(sup)[: D["nl"]], exp["link_support"] * np.uint64(reps))


# ------------------------------------------------------------------------------------------------ 4. edges
def small_case(snp_graph):
    c, genome, seqs, solid, slots, W = snp_graph
    sub = genome[:450] + ("C" if genome[450] != "C" else "G") + genome[451:700]      # (450 is no allele's position: COLLINEAR inside a shared stretch)
    bases, offs = pack([genome[:500], "", short_read(genome), sub, genome[150:250] + genome[4000:4100], rc_str(genome[300:900])])
    return c, bases, offs, walks_over(bases, offs, seqs, K_SNP, solid, slots)


def test_no_reads_and_no_segments(gkc, snp_graph):
    c, genome, seqs, solid, slots, W = snp_graph
    for reads in ([], ["", "ACGT", "N" * 40, "A" * 40]):
        bases, offs = pack(reads)
        exp = walks_over(bases, offs, seqs, K_SNP, solid, slots)
        assert len(exp["segments"]) == 0 and len(exp["walks"]) == 0 and not exp["link_support"].any()
        assert_walks(c.read_walks(bases, offs), exp)
        D = device_inputs(c, bases, offs)
        assert_raw(walks_raw(c, D, 2), exp, D)                  # every offset 0, the support zeroed, nothing else touched
        size = walks_raw(c, D, 2, offsets=False, walks=False)
        assert size["rc"] == 0 and size["n_walks"] == 0 and untouched(size)


def test_exactly_one_read_and_the_small_case(gkc, snp_graph):
    c, genome, seqs, solid, slots, W = snp_graph
    bases, offs = pack([genome[:500]])
    exp = walks_over(bases, offs, seqs, K_SNP, solid, slots)
    assert len(exp["walks"]) == 1 and exp["walks"]["n_segments"][0] == len(exp["segments"]) > 4
    assert_walks(c.read_walks(bases, offs), exp)
    c, bases, offs, exp = small_case(snp_graph)
    counts = junction_counts(exp["junction"])
    assert counts[0] and counts[2] == 1 and counts[3] == 1 and counts[4] == 5 and exp["walk_offsets"].tolist()[:3] == [0, 1, 1]
    assert_walks(c.read_walks(bases, offs), exp)
    assert c.read_walks(bases, offs, link_support=False)["link_support"] is None


def test_no_links_at_all(gkc):
    k = 31
    b = gi.isolated_paths(gi.lengths_for(120), k, seed=9)
    rb, ro = b.pack()
    c = counter_for(gkc, rb, ro, k, 8, 4)
    ub, uo, _ = c.unitigs()
    seqs = unitig_strings(ub, uo)
    assert len(seqs) == 60
    reads = seqs[:20] + [seqs[i] + seqs[i + 1] for i in range(20, 40, 2)] + [rc_str(seqs[41]) + seqs[40] + seqs[41]]
    bases, offs = pack(reads)
    vals, _, _ = solid_records(c)
    exp = walks_over(bases, offs, seqs, k, set(vals), overlap_links(seqs, k))
    assert len(exp["links"]) == 0 and junction_counts(exp["junction"]) == [0, 0, 0, 12, 31] and len(exp["walks"]) == 43
    res = c.read_walks(bases, offs)
    assert_walks(res, exp)
    D = device_inputs(c, bases, offs)
    assert D["nl"] == 0
    assert_raw(walks_raw(c, D, 43), exp, D)
    c.close()


def test_capacity_null_outputs_and_sizing(gkc, snp_graph):
    c, bases, offs, exp = small_case(snp_graph)
    D = device_inputs(c, bases, offs)
    nw = len(exp["walks"])
    full = walks_raw(c, D, nw)
    assert_raw(full, exp, D)
    # one walk too few: error 4, the count, nothing written
    small = walks_raw(c, D, nw, cap_walks=nw - 1)
    assert small["rc"] == 4 and small["n_walks"] == nw and b"walks" in c.L.gkc_last_error(c.h) and untouched(small)
    # d_junction == NULL, d_link_support == NULL, both
    for jn, sup in ((False, True), (True, False), (False, False)):
        out = walks_raw(c, D, nw, junction=jn, support=sup)
        assert out["rc"] == 0 and out["n_walks"] == nw
        for n, given in (("junction", jn), ("support", sup), ("walk_offsets", True), ("walks", True)):
            assert np.array_equal(out[n], full[n]) if given else untouched(out, n)
    # the sizing call, twice
    for _ in range(2):
        size = walks_raw(c, D, nw, offsets=False, walks=False)
        assert size["rc"] == 0 and size["n_walks"] == nw and untouched(size)


# ------------------------------------------------------------------------------------------------ 5. errors and state
def test_errors_and_state(gkc):
    k, m, parts = K_SNP, M_SNP, 4
    genome = random_sequence(52, 2000)
    twin = genome[:1000] + ("C" if genome[1000] != "C" else "G") + genome[1001:]
    bases, offs = pack([genome, twin])
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    # a placement, the inputs of the call, the answer
    seqs = unitig_strings(*c.unitigs()[:2])
    vals, _, _ = solid_records(c)
    qb, qo = pack([genome[500:1500], twin[900:1100], "", genome[:100] + genome[1500:1600]])
    exp = walks_over(qb, qo, seqs, k, set(vals), overlap_links(seqs, k))
    D = device_inputs(c, qb, qo)
    nw, ns, nr, nl, nu = len(exp["walks"]), D["ns"], D["nr"], D["nl"], len(seqs)
    assert (nw, ns, nr, nl, nu) == (4, 8, 4, 8, 4) and exp["seg_offsets"].tolist() == [0, 3, 6, 6, 8]
    assert_raw(walks_raw(c, D, nw), exp, D)

    def refused(word, **over):
        out = walks_raw(c, D, nw, **over)
        assert out["rc"] == 1 and word in c.L.gkc_last_error(c.h) and untouched(out), (word, out["rc"], c.L.gkc_last_error(c.h))

    # walks without offsets, offsets without walks
    refused(b"offsets", offsets=False)
    refused(b"offsets", walks=False)
    # segment offsets that are no CSR table of the segments
    so = exp["seg_offsets"]
    for wrong in (so + np.uint64(1), so[::-1].copy(), np.concatenate([so[:-1], [so[-1] + np.uint64(7)]]).astype(np.uint64), np.array([0, 3, 2, 6, 8], np.uint64)):
        refused(b"CSR", so=upload(wrong))
    refused(b"CSR", ns=ns - 1)
    refused(b"CSR", nr=nr - 1)
    # segments of a read that overlap, or descend
    sg = exp["segments"]
    bad = sg.copy(); bad["read_pos"][1] -= 1
    refused(b"overlap", seg=upload(bad))
    bad = sg.copy(); bad[[0, 1]] = bad[[1, 0]]
    refused(b"overlap", seg=upload(bad))
    # a node of no unitig: just beyond, far beyond, a sentinel of the nodes call; in a last segment too
    for at, node in ((0, 2 * nu), (1, 2 * nu + 1), (2, 1 << 50), (7, gkc.NODE_ABSENT), (3, gkc.NODE_REMOVED)):
        bad = sg.copy(); bad["node"][at] = node
        refused(b"unitig", seg=upload(bad))
    # link offsets: beyond n_links, descending; n_links smaller than the offsets say
    lo = exp["link_offsets"]
    bad = lo.copy(); bad[-1] += np.uint64(1)
    refused(b"link offsets", lo=upload(bad))
    bad = lo.copy(); bad[3] = np.uint64(1 << 40)
    refused(b"link offsets", lo=upload(bad))
    bad = lo.copy(); bad[2], bad[3] = lo[3] + np.uint64(1), lo[2]
    refused(b"link offsets", lo=upload(bad))
    refused(b"link offsets", nl=nl - 1)
    # the same calls as sizing calls: the checks are those of the fill
    bad = sg.copy(); bad["node"][0] = 2 * nu
    out = walks_raw(c, D, nw, offsets=False, walks=False, seg=upload(bad))
    assert out["rc"] == 1 and untouched(out)
    # a recount: the placement of the first count must not answer; before any build of the new results neither
    c.begin_pass(0); c.push_reads(bases, offs); c.finish_pass()
    out = walks_raw(c, D, nw)
    assert out["rc"] == 1 and untouched(out) and (b"changed" in c.L.gkc_last_error(c.h) or b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h))
    c.unitigs_build()
    assert_raw(walks_raw(c, D, nw), exp, D)
    c.close()
    # before a build
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    out = walks_raw(c, D, nw)
    assert out["rc"] == 1 and b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h) and untouched(out)
    with pytest.raises(gkc.GkcError):
        c.read_walks(qb, qo)
    c.close()


# ------------------------------------------------------------------------------------------------ 6. timers
def test_timers(gkc, snp_graph):
    c, bases, offs, exp = small_case(snp_graph)
    names = ("graph_read_nodes", "graph_read_segments", "graph_read_walks", "query_reads")
    before = {n: c.timing(n)[1] for n in names}
    c.read_walks(bases, offs)                                   # one nodes call; the sizing call and the fill of the segments and of the walks: one interval per call
    assert [c.timing(n)[1] - before[n] for n in names] == [1, 2, 2, 0]
