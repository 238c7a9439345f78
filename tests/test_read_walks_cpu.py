"""Read walks (include/gkc.h, "read paths": junction, walk, link support; csrc/gkc_paths.hip), the part that needs no GPU: the export is declared and bound, the walk
record is 16 bytes on both sides, gfa_text writes GFA 1, and a plain Python statement of the definitions — read_walks_np — a loop over the segments of every read that
looks the next segment's node up in the slot the segment leaves through. It is pinned on the reference-run fixtures (their own FASTA as reads against their own unitigs
and links), checked from the strings alone (a walk glued from its unitig slices spells its piece of the read), under reverse complement, and on hand-made cases;
tests/test_gpu_read_walks.py imports it."""
import ctypes
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_read_paths_cpu import SEGMENT, fixture_paths, graph_of, pack, random_sequence, rc_str, read_paths_np
from tests.test_unitig_links_cpu import csr, fixture_links, hairpin_reads, overlap_links, slots_of, unitig_links_np
from tests.test_unitigs_cpu import circle, fixture_unitigs, unitigs_np
from tests.util import str2int

NAME = "gkc_graph_reads_walks_device"
WALK = np.dtype([("first_segment", np.uint64), ("n_segments", np.uint32), ("n_kmers", np.uint32)])
END, BREAK, COLLINEAR, UNLINKED = 2 ** 64 - 1, 2 ** 64 - 2, 2 ** 64 - 3, 2 ** 64 - 4


# ------------------------------------------------------------------------------------------------ the statement
def read_walks_np(seg_offsets, segments, unitig_lengths, link_offsets, links):
    """-> (junction uint64[n_segments], walk_offsets uint64[n_reads + 1], walks WALK[], link_support uint64[n_links]), by the rules of the header in their order"""
    so = [int(x) for x in seg_offsets]; lo = [int(x) for x in link_offsets]; lk = [int(x) for x in links]; L = [int(x) for x in unitig_lengths]
    seg = [(int(s["node"]), int(s["read_pos"]), int(s["unitig_pos"]), int(s["n_kmers"])) for s in segments]
    junction = [END] * len(seg); support = [0] * len(lk); walks = []; walk_offsets = [0]
    for r in range(len(so) - 1):
        cur = None                                              # the walk under way: [first segment, segments, k-mers]
        for s in range(so[r], so[r + 1]):
            node_a, rp_a, up_a, nk_a = seg[s]
            if cur is None:
                cur = [s, 0, 0]
            cur[1] += 1; cur[2] += nk_a
            if s + 1 == so[r + 1]:
                j = END
            else:
                node_b, rp_b, up_b, _ = seg[s + 1]
                gap = rp_b - (rp_a + nk_a)
                assert gap >= 0
                u, sa, v, sb = node_a >> 1, node_a & 1, node_b >> 1, node_b & 1
                if gap == 0:
                    last = up_a - (nk_a - 1) if sa else up_a + (nk_a - 1)
                    leaves = last == (0 if sa else L[u] - 1)
                    enters = up_b == (L[v] - 1 if sb else 0)
                    slot = lk[lo[node_a]: lo[node_a + 1]]
                    j = lo[node_a] + slot.index(node_b) if leaves and enters and node_b in slot else UNLINKED
                else:
                    d = nk_a + gap
                    j = COLLINEAR if node_b == node_a and up_b == (up_a - d if sa else up_a + d) else BREAK
            junction[s] = j
            if j < UNLINKED:
                support[j] += 1
            else:
                walks.append(tuple(cur)); cur = None
        assert cur is None
        walk_offsets.append(len(walks))
    w = np.zeros(len(walks), WALK)
    for i, x in enumerate(walks):
        w[i] = x
    return np.array(junction, np.uint64).reshape(-1), np.array(walk_offsets, np.uint64), w, np.array(support, np.uint64).reshape(-1)


def lengths_of(seqs, k):
    return [len(s) - k + 1 for s in seqs]


def walks_over(bases, offs, seqs, k, solid, slots):
    """the reads against the unitig strings and their link slots -> dict: the answer of read_paths_np plus junction, walk_offsets, walks, link_offsets, links, link_support"""
    got = dict(read_paths_np(bases, offs, seqs, k, solid))
    lo, lk = csr(slots)
    j, wo, w, sup = read_walks_np(got["seg_offsets"], got["segments"], lengths_of(seqs, k), lo, lk)
    got.update(junction=j, walk_offsets=wo, walks=w, link_offsets=lo, links=lk, link_support=sup)
    return got


@functools.lru_cache(maxsize=None)
def fixture_walks(name):
    """a reference-run fixture's own FASTA as reads against its own unitigs and links -> (k, bases, offsets, unitig strings, slots, dict as walks_over gives it)"""
    k, bases, offs, seqs, paths = fixture_paths(name)
    _, u, slots = fixture_links(name)
    assert u["seqs"] == seqs
    lo, lk = csr(slots)
    j, wo, w, sup = read_walks_np(paths["seg_offsets"], paths["segments"], lengths_of(seqs, k), lo, lk)
    got = dict(paths)
    got.update(junction=j, walk_offsets=wo, walks=w, link_offsets=lo, links=lk, link_support=sup)
    return k, bases, offs, seqs, slots, got


def junction_counts(j):
    """-> [link, unlinked, collinear, break, end]"""
    return [int((j < np.uint64(UNLINKED)).sum())] + [int((j == np.uint64(x)).sum()) for x in (UNLINKED, COLLINEAR, BREAK, END)]


def mirror(e, lo, lk):
    """the entry that is link entry e taken in the other direction: for e in slot 2u + su with value (v, mv), the entry (u, 1 - su) of slot 2v + (1 - mv)"""
    t = int(np.searchsorted(np.asarray(lo, np.uint64), np.uint64(e), side="right")) - 1
    u, su, v, mv = t >> 1, t & 1, int(lk[e]) >> 1, int(lk[e]) & 1
    tt = 2 * v + (1 - mv)
    slot = [int(x) for x in lk[int(lo[tt]): int(lo[tt + 1])]]
    return int(lo[tt]) + slot.index(u << 1 | (1 - su))


def oriented_slice(seqs, k, s):
    """the bases a segment spells: the slice of its unitig on strand 0, the reverse complement of the corresponding slice on strand 1"""
    node, up, nk = int(s["node"]), int(s["unitig_pos"]), int(s["n_kmers"])
    q = seqs[node >> 1]
    return rc_str(q[up - (nk - 1): up + k]) if node & 1 else q[up: up + nk + k - 1]


def glue(pieces, k):
    out = pieces[0]
    for p in pieces[1:]:
        assert out[-(k - 1):] == p[: k - 1]
        out += p[k - 1:]
    return out


def assert_walks_spell_the_reads(bases, offs, seqs, k, got, slots_by_strings):
    """from the strings alone: every walk glued from its segments' oriented slices is its piece of the read; every link junction's entry is a (k-1)-overlap of the
    sequences; the support sums to the link junctions; walks = segments - link junctions"""
    raw = bases.tobytes().decode()
    sg, j, w = got["segments"], got["junction"], got["walks"]
    n_link = 0
    for r in range(len(offs) - 1):
        read = raw[int(offs[r]): int(offs[r + 1])]
        lo_w, hi_w = int(got["walk_offsets"][r]), int(got["walk_offsets"][r + 1])
        assert (lo_w == hi_w) == (got["seg_offsets"][r] == got["seg_offsets"][r + 1])
        nxt = int(got["seg_offsets"][r])
        for x in w[lo_w: hi_w]:
            s0, ns, nk = int(x["first_segment"]), int(x["n_segments"]), int(x["n_kmers"])
            assert s0 == nxt and ns >= 1                        # ascending, and together the walks of a read are its segments
            nxt = s0 + ns
            rp = int(sg["read_pos"][s0])
            assert glue([oriented_slice(seqs, k, sg[s]) for s in range(s0, s0 + ns)], k).upper() == read[rp: rp + nk + k - 1].upper()
            assert nk == int(sg["n_kmers"][s0: s0 + ns].sum()) and (j[s0: s0 + ns - 1] < np.uint64(UNLINKED)).all() and j[s0 + ns - 1] >= np.uint64(UNLINKED)
            for s in range(s0, s0 + ns - 1):
                assert int(got["links"][int(j[s])]) == int(sg["node"][s + 1]) and int(sg["node"][s + 1]) in slots_by_strings[int(sg["node"][s])]
                n_link += 1
        assert nxt == int(got["seg_offsets"][r + 1])
    assert int(got["link_support"].sum()) == n_link == junction_counts(j)[0] and len(w) == len(sg) - n_link
    assert np.array_equal(got["link_support"], np.bincount(j[j < np.uint64(UNLINKED)].astype(np.int64), minlength=len(got["links"])).astype(np.uint64))


# ------------------------------------------------------------------------------------------------ exports
def test_export_is_declared_mapped_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    assert NAME in gkc.SYMBOLS
    assert ("int %s(gkc_ctx* ctx, const uint64_t* d_seg_offsets, const gkc_read_segment* d_segments, uint64_t n_reads, uint64_t n_segments," % NAME) in hdr
    assert "gkc_*" in vmap or NAME in vmap
    assert "typedef struct gkc_read_walk" in hdr and '"graph_read_walks"' in hdr
    for name, value in (("END", "(~0ull)"), ("BREAK", "(~0ull - 1)"), ("COLLINEAR", "(~0ull - 2)"), ("UNLINKED", "(~0ull - 3)")):
        assert any(line.split()[:3] == ["#define", "GKC_JUNCTION_" + name, value.split()[0]] and value in line for line in hdr.splitlines()), name
    for meth in ("read_walks", "read_walks_device", "write_gfa"):
        assert callable(getattr(gkc.Counter, meth))
    assert callable(gkc.gfa_text)
    assert len(getattr(gkc.lib(), NAME).argtypes) == 14


def test_the_walk_record_is_16_bytes():
    gkc = ge.load().gkc
    assert ctypes.sizeof(gkc.ReadWalk) == 16 == gkc.READ_WALK.itemsize and gkc.READ_WALK == WALK
    assert [(n, getattr(gkc.ReadWalk, n).offset) for n, _ in gkc.ReadWalk._fields_] == [(n, WALK.fields[n][1]) for n in WALK.names]
    assert (gkc.JUNCTION_END, gkc.JUNCTION_BREAK, gkc.JUNCTION_COLLINEAR, gkc.JUNCTION_UNLINKED) == (END, BREAK, COLLINEAR, UNLINKED)


# ------------------------------------------------------------------------------------------------ the fixtures
PINNED = {   # name: reads, segments, walks, [link, unlinked, collinear, break, end]
    "k21_freq_4parts": (6000, 20071, 11780, [8291, 0, 4021, 1759, 6000]),
    "k31_defaults": (600, 1827, 1013, [814, 0, 208, 205, 600]),
    "k63_defaults": (300, 330, 313, [17, 0, 12, 36, 265]),
    "k21_freq": (600, 2464, 1180, [1284, 0, 332, 248, 600]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_statement_on_the_fixtures(name):
    k, bases, offs, seqs, slots, got = fixture_walks(name)
    counts = junction_counts(got["junction"])
    print("%s: %d reads, %d segments, %d walks; link, unlinked, collinear, break, end = %s" % (name, len(offs) - 1, len(got["segments"]), len(got["walks"]), counts))
    assert (len(offs) - 1, len(got["segments"]), len(got["walks"]), counts) == PINNED[name]
    assert k % 2 == 1 and counts[1] == 0
    assert_walks_spell_the_reads(bases, offs, seqs, k, got, overlap_links(seqs, k))


@pytest.mark.parametrize("name", ["k31_defaults", "k21_freq"])
def test_the_reverse_complement_mirrors_walks_and_support(name):
    k, bases, offs, seqs, slots, got = fixture_walks(name)
    raw = bases.tobytes().decode()
    reads = [raw[int(offs[r]): int(offs[r + 1])] for r in range(len(offs) - 1)]
    _, values, _, _ = fixture_unitigs(name)
    rb, ro = pack([rc_str(r) for r in reads])
    rv = walks_over(rb, ro, seqs, k, set(values), slots)
    assert np.array_equal(rv["walk_offsets"], got["walk_offsets"]) and np.array_equal(rv["seg_offsets"], got["seg_offsets"])
    for r in range(len(reads)):
        a, b = int(got["walk_offsets"][r]), int(got["walk_offsets"][r + 1])
        for x, y in zip(got["walks"][a:b], rv["walks"][a:b][::-1]):
            assert x["n_segments"] == y["n_segments"] and x["n_kmers"] == y["n_kmers"]
            fw = got["segments"][int(x["first_segment"]): int(x["first_segment"]) + int(x["n_segments"])]
            bw = rv["segments"][int(y["first_segment"]): int(y["first_segment"]) + int(y["n_segments"])][::-1]
            assert np.array_equal(fw["node"] ^ np.uint64(1), bw["node"]) and np.array_equal(fw["n_kmers"], bw["n_kmers"])
    lo, lk = got["link_offsets"], got["links"]
    assert got["link_support"].sum() > 0
    for e in range(len(lk)):
        m = mirror(e, lo, lk)
        assert mirror(m, lo, lk) == e and rv["link_support"][m] == got["link_support"][e]


# ------------------------------------------------------------------------------------------------ hand cases
def odd_k_case(graph_reads, reads, k):
    seqs, solid = graph_of(graph_reads, k)
    slots = overlap_links(seqs, k)
    bases, offs = pack(reads)
    return seqs, slots, walks_over(bases, offs, seqs, k, solid, slots)


def test_a_read_across_a_fork():
    k = 11
    stem, left, right = random_sequence(2, 40), random_sequence(102, 30), random_sequence(202, 30)
    a, b = stem + left, stem + right
    seqs, slots, got = odd_k_case([a, b], [a, b], k)
    sg, j = got["segments"], got["junction"]
    assert len(seqs) == 3 and got["seg_offsets"].tolist() == [0, 2, 4] and got["walk_offsets"].tolist() == [0, 1, 2]
    assert got["walks"].tolist() == [(0, 2, 70 - k + 1), (2, 2, 70 - k + 1)]
    assert j[1] == END and j[3] == END and j[0] != j[2] and sg["node"][0] == sg["node"][2]
    t = int(sg["node"][0])
    lo, lk = got["link_offsets"], got["links"]
    assert int(lo[t + 1]) - int(lo[t]) == 2 and sorted(j[[0, 2]].tolist()) == [int(lo[t]), int(lo[t]) + 1]      # the slot holds both branches; each read takes its own
    assert int(lk[int(j[0])]) == int(sg["node"][1]) and int(lk[int(j[2])]) == int(sg["node"][3])
    assert got["link_support"].sum() == 2 and got["link_support"][int(j[0])] == 1 and got["link_support"][int(j[2])] == 1


def test_a_substitution_is_collinear_with_a_gap_of_k():
    k, at = 11, 40
    genome = random_sequence(1, 80)
    read = genome[:at] + ("C" if genome[at] != "C" else "G") + genome[at + 1:]
    seqs, slots, got = odd_k_case([genome], [read], k)
    sg = got["segments"]
    assert len(sg) == 2 and got["junction"].tolist() == [COLLINEAR, END] and int(sg["read_pos"][1]) - int(sg["read_pos"][0]) - int(sg["n_kmers"][0]) == k
    assert got["walks"].tolist() == [(0, 1, at - k + 1), (1, 1, 80 - k - at)] and got["walk_offsets"].tolist() == [0, 2] and len(got["link_support"]) == 0


def test_a_jump_inside_one_unitig_is_a_break():
    k = 11
    genome = random_sequence(1, 80)
    to = next(t for t in range(50, 60) if genome[t] != genome[30] and genome[t - 1] != genome[29])      # (no window over the joint spells a k-mer of the genome)
    seqs, slots, got = odd_k_case([genome], [genome[:30] + genome[to:]], k)
    sg = got["segments"]
    assert len(sg) == 2 and sg["node"][0] == sg["node"][1] and got["junction"].tolist() == [BREAK, END]
    assert sg["read_pos"].tolist() == [0, 30] and sg["n_kmers"].tolist() == [30 - k + 1, 80 - to - k + 1]      # the k - 1 k-mers over the joint are in no unitig
    assert got["walks"].tolist() == [(0, 1, 20), (1, 1, 80 - to - k + 1)]


@pytest.mark.parametrize("k,L", [(7, 40), (21, 40)])
def test_twice_round_a_circle_joins_across_the_cut(k, L):
    seq, vals = circle(k, L)
    seqs = unitigs_np(vals, [1] * L, k)["seqs"]
    slots = overlap_links(seqs, k)
    assert len(seqs) == 1 and slots == [[0], [1]]               # L:+:0:+ and L:-:0:-
    once = seqs[0][:L]
    read = once + once + once[: k - 1]                         # starts at the cut
    for rd, strand in ((read, 0), (rc_str(read), 1)):
        bases, offs = pack([rd])
        got = walks_over(bases, offs, seqs, k, set(vals), slots)
        sg = got["segments"]
        assert sg["node"].tolist() == [strand, strand] and sg["n_kmers"].tolist() == [L, L] and sg["unitig_pos"].tolist() == [L - 1 if strand else 0] * 2
        assert got["junction"].tolist() == [strand, END]        # entry 0 is the self-link of the '+' side, entry 1 that of the '-' side
        assert got["walks"].tolist() == [(0, 2, 2 * L)] and got["link_support"].tolist() == ([0, 1] if strand else [1, 0])


def test_a_hairpin_leaves_and_arrives_through_the_same_end():
    k = 21
    seqs, slots, _ = odd_k_case(hairpin_reads(k), [], k)
    assert len(seqs) == 1 and slots == [[1], []]                # L:+:0:-
    U = seqs[0]
    L = len(U) - k + 1
    seqs, slots, got = odd_k_case(hairpin_reads(k), [U + rc_str(U)[k - 1:]], k)
    sg = got["segments"]
    assert sg["node"].tolist() == [0, 1] and sg["unitig_pos"].tolist() == [0, L - 1] and sg["n_kmers"].tolist() == [L, L] and sg["read_pos"].tolist() == [0, L]
    assert got["junction"].tolist() == [0, END] and int(got["links"][0]) == 0 << 1 | 1
    assert got["walks"].tolist() == [(0, 2, 2 * L)] and got["link_support"].tolist() == [1]


def test_an_N_is_collinear_or_a_break_by_the_positions():
    k = 11
    genome = random_sequence(1, 80)
    seqs, slots, got = odd_k_case([genome], [genome[:40] + "N" + genome[41:], genome[:40] + "N" + genome[45:]], k)
    assert got["seg_offsets"].tolist() == [0, 2, 4] and got["junction"].tolist() == [COLLINEAR, END, BREAK, END]
    assert got["walk_offsets"].tolist() == [0, 2, 4] and got["walks"]["n_segments"].tolist() == [1, 1, 1, 1]


def test_empty_reads_and_reads_of_one_segment():
    k = 11
    stem, left, right = random_sequence(2, 40), random_sequence(102, 30), random_sequence(202, 30)
    a, b = stem + left, stem + right
    seqs, slots, got = odd_k_case([a, b], ["", a, "", "", stem, "A" * 5, b[20:], ""], k)
    assert got["seg_offsets"].tolist() == [0, 0, 2, 2, 2, 3, 3, 5, 5] and got["walk_offsets"].tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3]
    j = got["junction"]
    assert j[1] == END and j[2] == END and j[4] == END and j[0] < UNLINKED and j[3] < UNLINKED and j[0] != j[3]
    assert got["walks"].tolist() == [(0, 2, 70 - k + 1), (2, 1, 40 - k + 1), (3, 2, 50 - k + 1)]


def test_an_even_k_palindrome():
    """k = 6: the palindrome ACGCGT is a unitig of its own between two others. The links are those of the DEFINITION (unitig_links_np: the neighbour masks), which is what
    the device writes. Both reads cross the palindrome on strand 0 (a palindrome takes the strand of its record); the answer below is pinned as the defined one."""
    k = 6
    genome = "TTGACA" + "ACGCGT" + "GGATCA"
    seqs, solid = graph_of([genome], k)
    vals = sorted(solid)
    u = unitigs_np(vals, [1] * len(vals), k)
    assert u["seqs"] == seqs
    slots = unitig_links_np(vals, k, u)
    out = []
    for read in (genome, rc_str(genome)):
        bases, offs = pack([read])
        got = walks_over(bases, offs, seqs, k, solid, slots)
        assert len(got["segments"]) == 3 and int(got["segments"]["n_kmers"].sum()) == len(genome) - k + 1
        out.append((got["segments"]["node"].tolist(), got["junction"].tolist(), got["walks"].tolist()))
    assert seqs == ["CGCGTTGTCAA", "ACGCGT", "CGCGTGGATCA"] and slots == [[], [3], [0, 4], [0, 4], [], [3]]
    # Into the palindrome: the link arrives at its END (entry 3 = unitig 1, mv 1) whichever neighbour one comes from, the segment on it stands forward (node 2): no entry
    # equals node_B, the junction is UNLINKED. Out of it: the slot of its '+' side holds both neighbours, and the read's own is found there.
    assert out == [([1, 2, 4], [UNLINKED, 2, END], [(0, 1, 6), (1, 2, 7)]), ([5, 2, 0], [UNLINKED, 1, END], [(0, 1, 6), (1, 2, 7)])]


# ------------------------------------------------------------------------------------------------ GFA
def test_gfa_text_on_the_reference_unitigs():
    gkc = ge.load().gkc
    name = "k21_freq_4parts"
    k, bases, offs, seqs, slots, got = fixture_walks(name)
    _, values, ab, u = fixture_unitigs(name)
    lo, lk = csr(slots)
    raw = bases.tobytes().decode()
    sg = got["segments"]
    paths, pieces = [], {}
    for r in range(len(offs) - 1):
        for i, x in enumerate(got["walks"][int(got["walk_offsets"][r]): int(got["walk_offsets"][r + 1])]):
            if x["n_segments"] >= 2:
                s0 = int(x["first_segment"])
                paths.append(("r%d_%d" % (r, i), sg["node"][s0: s0 + int(x["n_segments"])].tolist()))
                rp = int(offs[r]) + int(sg["read_pos"][s0])
                up, st, Lu = int(sg["unitig_pos"][s0]), int(sg["node"][s0]) & 1, len(seqs[int(sg["node"][s0]) >> 1]) - k + 1
                pieces[paths[-1][0]] = (raw[rp: rp + int(x["n_kmers"]) + k - 1], Lu - 1 - up if st else up)
    text = gkc.gfa_text(k, seqs, u["kc"], lo, lk, paths)
    assert isinstance(text, str) and text.endswith("\n")
    lines = text.split("\n")[:-1]
    assert lines[0] == "H\tVN:Z:1.0" and all(ln[0] in "SLP" for ln in lines[1:])
    S = [ln.split("\t") for ln in lines if ln[0] == "S"]; Ls = [ln.split("\t") for ln in lines if ln[0] == "L"]; P = [ln.split("\t") for ln in lines if ln[0] == "P"]
    assert len(S) == 711 and len(Ls) == 1528 and len(P) == len(paths) > 1000
    abundance = {int(v): int(a) for v, a in zip(values, ab)}
    for u_, f in enumerate(S):
        assert f[1] == "%d" % u_ and f[2] == seqs[u_] and len(f) == 4
        want = sum(abundance[min(x, y)] for x, y in ((str2int(f[2][i: i + k]), str2int(rc_str(f[2][i: i + k]))) for i in range(len(f[2]) - k + 1)))
        assert f[3] == "KC:i:%d" % want
    back = [[] for _ in range(2 * len(seqs))]
    orient = lambda v, sign: seqs[int(v)] if sign == "+" else rc_str(seqs[int(v)])
    for f in Ls:
        assert len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5] == "%dM" % (k - 1)
        assert orient(f[1], f[2])[-(k - 1):] == orient(f[3], f[4])[: k - 1]
        back[2 * int(f[1]) + (f[2] == "-")].append(int(f[3]) << 1 | (f[4] == "-"))
    assert back == slots
    for f in P:
        assert len(f) == 4 and f[3] == "*"
        piece, at = pieces[f[1]]
        spelled = glue([orient(x[:-1], x[-1]) for x in f[2].split(",")], k)
        assert spelled[at: at + len(piece)] == piece.upper()
    assert gkc.gfa_text(k, seqs, u["kc"], lo, lk) == "\n".join(lines[: 1 + 711 + 1528]) + "\n"
