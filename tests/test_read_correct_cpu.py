"""Correction of the reads (include/gkc.h, "read paths": region, correction; csrc/gkc_correct.hip), the part that needs no GPU: the export is declared, mapped and
bound, the two structs have the layout of their ctypes twins, and a plain Python statement of the rule — correct_reads_np — over the reads, their segments and the
unitig STRINGS: per read the regions (gap, head, tail), per region the targets from one segment's base-to-base map, the changes counted, the region rewritten whole or
not at all. It is pinned on the reference-run fixtures, checked from the strings alone (threading the corrected reads again, correcting them again, the reverse
complement), against a ground truth (a planted substitution at every position of a read comes out as the genome's base) and on hand-made cases;
tests/test_gpu_read_correct.py imports it."""
import ctypes
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_read_paths_cpu import fixture_paths, graph_of, pack, random_sequence, rc_str, read_paths_np
from tests.test_read_walks_cpu import BREAK, END, UNLINKED, junction_counts, lengths_of, read_walks_np
from tests.test_unitig_links_cpu import csr, overlap_links
from tests.test_unitigs_cpu import circle, fixture_unitigs, unitigs_np

NAME = "gkc_graph_reads_correct_device"
STATS = ("gaps_fixed", "gaps_skipped", "heads_fixed", "tails_fixed", "ends_skipped", "ends_no_room", "bases_changed")
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ------------------------------------------------------------------------------------------------ the statement
def regions_np(length, segs, lengths, k, ends):
    """the regions of one read of ``length`` bases with segments ``segs`` [(node, read_pos, unitig_pos, n_kmers)], lengths[u] = L_u -> a list of
    (kind, first, behind, segment whose map gives the targets, room): kind "gap" / "head" / "tail", read positions [first, behind)"""
    out = []
    if not segs:
        return out
    node, rp, up, nk = F = segs[0]
    if ends and rp > 0:
        out.append(("head", 0, rp, F, up + rp <= lengths[node >> 1] - 1 if node & 1 else up >= rp))
    for A, B in zip(segs[:-1], segs[1:]):
        gap = B[1] - (A[1] + A[3])
        assert gap >= 0
        d = A[3] + gap
        if gap > 0 and B[0] == A[0] and B[2] == (A[2] - d if A[0] & 1 else A[2] + d) and gap >= k:
            out.append(("gap", A[1] + A[3] + k - 1, B[1], A, True))
    node, rp, up, nk = Z = segs[-1]
    t = length - (rp + nk + k - 1)
    assert t >= 0
    if ends and t > 0:
        out.append(("tail", length - t, length, Z, up - (nk - 1) >= t if node & 1 else up + nk - 1 + t <= lengths[node >> 1] - 1))
    return out


def target_np(seqs, k, seg, x):
    """the base the map of segment ``seg`` gives read position x"""
    node, rp, up, _ = seg
    q = seqs[node >> 1]
    if node & 1:
        i = up + k - 1 - (x - rp)
        assert 0 <= i < len(q)
        return _COMPLEMENT[q[i]]
    i = up + (x - rp)
    assert 0 <= i < len(q)
    return q[i]


def correct_reads_np(bases, offsets, seg_offsets, segments, seqs, k, max_subst=2, ends=1):
    """-> dict: bases uint8[n_bases], n_changed uint32[n_reads], changed bool[n_bases], stats (a dict over STATS), regions: per read a list of
    (kind, first, behind, room, changes, rewritten)"""
    seqs = [s if isinstance(s, str) else bytes(s).decode() for s in seqs]
    L = lengths_of(seqs, k)
    raw = np.asarray(bases, np.uint8).tobytes().decode("latin-1")
    offs = [int(x) for x in offsets]; so = [int(x) for x in seg_offsets]
    out = list(raw[: offs[-1]])
    st = dict.fromkeys(STATS, 0)
    n_changed = np.zeros(len(offs) - 1, np.uint32); changed = np.zeros(offs[-1], bool); regions = []
    for r in range(len(offs) - 1):
        b = offs[r]
        segs = [(int(s["node"]), int(s["read_pos"]), int(s["unitig_pos"]), int(s["n_kmers"])) for s in segments[so[r]: so[r + 1]]]
        mine = []
        for kind, x0, x1, seg, room in regions_np(offs[r + 1] - b, segs, L, k, ends):
            if not room:
                st["ends_no_room"] += 1
                mine.append((kind, x0, x1, False, None, False))
                continue
            targets = [target_np(seqs, k, seg, x) for x in range(x0, x1)]
            diff = [x for x, t in zip(range(x0, x1), targets) if raw[b + x] != t]
            fix = len(diff) <= max_subst
            if fix:
                st["gaps_fixed" if kind == "gap" else "heads_fixed" if kind == "head" else "tails_fixed"] += 1
                st["bases_changed"] += len(diff)
                n_changed[r] += len(diff)
                for x, t in zip(range(x0, x1), targets):
                    out[b + x] = t
                for x in diff:
                    changed[b + x] = True
            else:
                st["gaps_skipped" if kind == "gap" else "ends_skipped"] += 1
            mine.append((kind, x0, x1, True, len(diff), fix))
        regions.append(mine)
    return dict(bases=np.frombuffer("".join(out).encode("latin-1"), np.uint8).copy(), n_changed=n_changed, changed=changed, stats=st, regions=regions)


def stats_tuple(st):
    return tuple(int(st[n]) for n in STATS)


@functools.lru_cache(maxsize=None)
def fixture_corrected(name, max_subst=2, ends=1):
    """the statement over a reference-run fixture (fixture_paths): -> (k, bases, offsets, unitig strings, the paths, correct_reads_np(...))"""
    k, bases, offs, seqs, paths = fixture_paths(name)
    return k, bases, offs, seqs, paths, correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, k, max_subst, ends)


def corrected_over(reads, seqs, solid, k, max_subst=2, ends=1):
    """reads (strings) threaded and corrected against the unitig strings -> (bases, offsets, paths, corrected, the corrected reads as strings)"""
    bases, offs = pack(reads)
    paths = read_paths_np(bases, offs, seqs, k, solid)
    got = correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, k, max_subst, ends)
    text = got["bases"].tobytes().decode("latin-1")
    return bases, offs, paths, got, [text[int(offs[r]): int(offs[r + 1])] for r in range(len(reads))]


def substitute(s, at, step=1):
    """s with the base at ``at`` replaced by another one"""
    return s[:at] + "ACGT"[("ACGT".index(s[at].upper()) + step) % 4] + s[at + 1:]


# ------------------------------------------------------------------------------------------------ exports
def test_export_is_declared_mapped_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    assert gkc.SYMBOLS.count(NAME) == 1
    assert ("int %s(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases," % NAME) in hdr
    assert "gkc_*" in vmap or NAME in vmap
    assert "typedef struct gkc_correct_params" in hdr and "typedef struct gkc_correct_stats" in hdr and '"graph_read_correct"' in hdr
    for meth in ("correct_reads", "correct_reads_device"):
        assert callable(getattr(gkc.Counter, meth))
    assert callable(gkc.write_corrected_fasta)
    assert len(getattr(gkc.lib(), NAME).argtypes) == 15


def test_the_structs_have_the_layout_of_their_twins():
    gkc = ge.load().gkc
    assert ctypes.sizeof(gkc.CorrectParams) == 16 and ctypes.sizeof(gkc.CorrectStats) == 56
    assert [(n, getattr(gkc.CorrectParams, n).offset) for n, _ in gkc.CorrectParams._fields_] == [("max_subst", 0), ("ends", 4), ("pad", 8)]
    assert [(n, getattr(gkc.CorrectStats, n).offset) for n, _ in gkc.CorrectStats._fields_] == [(n, 8 * i) for i, n in enumerate(STATS)]
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    assert "typedef struct gkc_correct_params { uint32_t max_subst; uint32_t ends; uint32_t pad[2]; } gkc_correct_params;" in hdr
    assert "typedef struct gkc_correct_stats  { uint64_t " + ", ".join(STATS) + "; } gkc_correct_stats;" in hdr


def test_write_corrected_fasta(tmp_path):
    gkc = ge.load().gkc
    bases, offs = pack(["ACGT", "", "NNacgtTT"])
    p = str(tmp_path / "reads.fa")
    assert gkc.write_corrected_fasta(p, bases, offs) == 3
    assert open(p).read() == ">0\nACGT\n>1\n\n>2\nNNacgtTT\n"
    assert gkc.write_corrected_fasta(p, bases, offs, names=["a b", b"c", 7]) == 3
    assert open(p).read() == ">a b\nACGT\n>c\n\n>7\nNNacgtTT\n"
    with pytest.raises(gkc.GkcError):
        gkc.write_corrected_fasta(p, bases, offs, names=["a"])


# ------------------------------------------------------------------------------------------------ the fixtures
PINNED = {   # (name, max_subst): gaps_fixed, gaps_skipped, heads_fixed, tails_fixed, ends_skipped, ends_no_room, bases_changed at ends = 1
    ("k21_freq_4parts", 2): (3907, 114, 1018, 1031, 84, 430, 6850), ("k21_freq_4parts", 1): (3334, 687, 868, 860, 405, 430, 5062),
    ("k31_defaults", 2): (192, 16, 111, 132, 14, 90, 518), ("k31_defaults", 1): (159, 49, 86, 107, 64, 90, 352),
    ("k63_defaults", 2): (12, 0, 75, 78, 21, 67, 229),
    ("k21_freq", 2): (323, 9, 95, 98, 2, 52, 602),
}
FIXTURES = sorted({n for n, _ in PINNED})


@pytest.mark.parametrize("name,max_subst", sorted(PINNED))
def test_statement_on_the_fixtures(name, max_subst):
    k, bases, offs, seqs, paths, got = fixture_corrected(name, max_subst)
    print("%s, max_subst %d: %s" % (name, max_subst, dict(got["stats"])))
    assert stats_tuple(got["stats"]) == PINNED[name, max_subst]
    # the gaps evaluated are the collinear junctions of the walks statement (no links needed: rule 4 asks for none)
    lo, lk = csr(overlap_links(seqs, k))
    j = read_walks_np(paths["seg_offsets"], paths["segments"], lengths_of(seqs, k), lo, lk)[0]
    assert got["stats"]["gaps_fixed"] + got["stats"]["gaps_skipped"] == junction_counts(j)[2]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_corrected_reads_thread_with_fewer_segments_and_correct_to_themselves(name):
    k, bases, offs, seqs, paths, got = fixture_corrected(name)
    _, values, _, _ = fixture_unitigs(name)
    again = read_paths_np(got["bases"], offs, seqs, k, set(values))
    assert len(again["segments"]) == len(paths["segments"]) - got["stats"]["gaps_fixed"]
    twice = correct_reads_np(got["bases"], offs, again["seg_offsets"], again["segments"], seqs, k)
    assert np.array_equal(twice["bases"], got["bases"]) and not twice["changed"].any() and not twice["n_changed"].any()
    a, b = twice["stats"], got["stats"]
    assert a["gaps_fixed"] == a["heads_fixed"] == a["tails_fixed"] == a["bases_changed"] == 0
    assert (a["gaps_skipped"], a["ends_skipped"], a["ends_no_room"]) == (b["gaps_skipped"], b["ends_skipped"], b["ends_no_room"])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("max_subst", [1, 2])
def test_changes_lie_in_regions_and_regions_left_alone_have_a_reason(name, max_subst):
    k, bases, offs, seqs, paths, got = fixture_corrected(name, max_subst)
    L = lengths_of(seqs, k)
    raw, new = bases.tobytes().decode("latin-1"), got["bases"].tobytes().decode("latin-1")
    inside = np.zeros(len(bases), bool)
    n_fixed = 0
    for r, mine in enumerate(got["regions"]):
        b = int(offs[r])
        segs = [(int(s["node"]), int(s["read_pos"]), int(s["unitig_pos"]), int(s["n_kmers"])) for s in paths["segments"][int(paths["seg_offsets"][r]): int(paths["seg_offsets"][r + 1])]]
        for (kind, x0, x1, room, changes, fix), (_, _, _, seg, _) in zip(mine, regions_np(int(offs[r + 1]) - b, segs, L, k, 1)):
            assert x0 < x1 and not inside[b + x0: b + x1].any()          # never empty, and disjoint
            inside[b + x0: b + x1] = True
            if not room:
                assert kind != "gap" and new[b + x0: b + x1] == raw[b + x0: b + x1]
                continue
            want = "".join(target_np(seqs, k, seg, x) for x in range(x0, x1))
            differ = sum(a != t for a, t in zip(raw[b + x0: b + x1], want))
            assert differ == changes and fix == (differ <= max_subst)
            assert new[b + x0: b + x1] == (want if fix else raw[b + x0: b + x1])
            n_fixed += fix
    st = got["stats"]
    assert n_fixed == st["gaps_fixed"] + st["heads_fixed"] + st["tails_fixed"]
    differs = np.frombuffer(raw.encode("latin-1"), np.uint8) != got["bases"]
    assert np.array_equal(differs, got["changed"]) and not (differs & ~inside).any()
    assert int(got["n_changed"].sum()) == st["bases_changed"] == int(got["changed"].sum())
    assert got["n_changed"].tolist() == [int(got["changed"][int(offs[r]): int(offs[r + 1])].sum()) for r in range(len(offs) - 1)]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reverse_complement_gives_the_reverse_complemented_output(name):
    k, bases, offs, seqs, paths, got = fixture_corrected(name)
    _, values, _, _ = fixture_unitigs(name)
    raw, new = bases.tobytes().decode(), got["bases"].tobytes().decode()
    cut = lambda text: [text[int(offs[r]): int(offs[r + 1])] for r in range(len(offs) - 1)]
    _, ro, _, rv, rv_reads = corrected_over([rc_str(r) for r in cut(raw)], seqs, set(values), k)
    assert np.array_equal(ro, offs)
    # an N has no complement: rc_str leaves it, and a corrected N became a base; upper case throughout the fixtures
    assert rv_reads == [rc_str(r) for r in cut(new)]
    a, b = rv["stats"], got["stats"]
    assert (a["gaps_fixed"], a["gaps_skipped"], a["ends_skipped"], a["ends_no_room"], a["bases_changed"]) == (b["gaps_fixed"], b["gaps_skipped"], b["ends_skipped"], b["ends_no_room"], b["bases_changed"])
    assert (a["heads_fixed"], a["tails_fixed"]) == (b["tails_fixed"], b["heads_fixed"])
    assert np.array_equal(rv["n_changed"], got["n_changed"])


# ------------------------------------------------------------------------------------------------ ground truth
GENOME_LEN, READ_LEN = 3000, 150


@functools.lru_cache(maxsize=None)
def ground_truth(k):
    """a random genome, the unitigs of its error-free tiling reads, and the solid set -> (genome, unitig strings, solid)"""
    genome = random_sequence(7, GENOME_LEN)
    tiles = [genome[a: a + READ_LEN] for a in range(0, GENOME_LEN - READ_LEN + 1, 50)]
    seqs, solid = graph_of(tiles, k)
    return genome, seqs, solid


@pytest.mark.parametrize("k", [21, 31])
def test_one_substitution_at_every_position_comes_out_as_the_genome(k):
    genome, seqs, solid = ground_truth(k)
    assert len(seqs) == 1                                       # a random genome of this length repeats no (k-1)-mer: one unitig, room at both ends of every slice
    truth, reads = [], []
    for at in range(READ_LEN):
        a = 200 + 13 * at
        for piece in (genome[a: a + READ_LEN], rc_str(genome[a: a + READ_LEN])):
            truth.append(piece); reads.append(substitute(piece, at, 1 + at % 3))
    _, offs, paths, got, out = corrected_over(reads, seqs, solid, k)
    assert out == truth
    st = got["stats"]
    # positions [0, k) are a head, [150 - k, 150) a tail, the others a gap of exactly k
    assert (st["heads_fixed"], st["tails_fixed"], st["gaps_fixed"]) == (2 * k, 2 * k, 2 * (READ_LEN - 2 * k))
    assert st["bases_changed"] == 2 * READ_LEN and (got["n_changed"] == 1).all() and stats_tuple(st)[1] == 0 and stats_tuple(st)[4:6] == (0, 0)


@pytest.mark.parametrize("k", [21, 31])
def test_two_close_substitutions_need_a_limit_of_two_and_three_are_left(k):
    genome, seqs, solid = ground_truth(k)
    piece = genome[500: 500 + READ_LEN]
    for d in (1, k // 2, k - 1):
        two = substitute(substitute(piece, 70), 70 + d)
        for rd, want in ((two, piece), (rc_str(two), rc_str(piece))):
            assert corrected_over([rd], seqs, solid, k, max_subst=2)[4] == [want]
            left = corrected_over([rd], seqs, solid, k, max_subst=1)
            assert left[4] == [rd] and stats_tuple(left[3]["stats"]) == (0, 1, 0, 0, 0, 0, 0)
    three = substitute(substitute(substitute(piece, 70), 75), 80)
    left = corrected_over([three], seqs, solid, k, max_subst=2)
    assert left[4] == [three] and stats_tuple(left[3]["stats"]) == (0, 1, 0, 0, 0, 0, 0)
    assert corrected_over([three], seqs, solid, k, max_subst=3)[4] == [piece]
    far = substitute(substitute(piece, 40), 40 + k + 5)        # two regions, one change each
    got = corrected_over([far], seqs, solid, k, max_subst=1)
    assert got[4] == [piece] and stats_tuple(got[3]["stats"]) == (2, 0, 0, 0, 0, 0, 2)


# ------------------------------------------------------------------------------------------------ hand cases
def test_an_N_and_a_lower_case_base_are_changes():
    k = 21
    genome, seqs, solid = ground_truth(k)
    piece = genome[900: 900 + READ_LEN]
    for ch in ("N", piece[60].lower(), "n"):
        rd = piece[:60] + ch + piece[61:]
        _, _, paths, got, out = corrected_over([rd], seqs, solid, k)
        if ch == piece[60].lower():                            # a lower-case base is a base to the k-mers: the read threads whole, no region holds it, it stays
            assert len(paths["segments"]) == 1 and out == [rd] and stats_tuple(got["stats"]) == (0,) * 7
            sub = substitute(substitute(rd, 55), 65)           # between two substitutions it lies in their region, [55, 66), and counts
            left = corrected_over([sub], seqs, solid, k, max_subst=2)
            assert left[4] == [sub] and stats_tuple(left[3]["stats"]) == (0, 1, 0, 0, 0, 0, 0)
            got3 = corrected_over([sub], seqs, solid, k, max_subst=3)
            assert got3[4] == [piece] and stats_tuple(got3[3]["stats"]) == (1, 0, 0, 0, 0, 0, 3) and got3[3]["changed"].nonzero()[0].tolist() == [55, 60, 65]
        else:
            assert out == [piece] and stats_tuple(got["stats"]) == (1, 0, 0, 0, 0, 0, 1) and got["changed"].nonzero()[0].tolist() == [60]


def test_a_break_and_a_link_junction_are_left_alone():
    k = 11
    stem, left, right = random_sequence(2, 40), random_sequence(102, 30), random_sequence(202, 30)
    a, b = stem + left, stem + right
    seqs, solid = graph_of([a, b], k)
    lo, lk = csr(overlap_links(seqs, k))
    genome1 = random_sequence(1, 80)
    seqs1, solid1 = graph_of([genome1], k)
    to = next(t for t in range(50, 60) if genome1[t] != genome1[30] and genome1[t - 1] != genome1[29])
    jump = genome1[:30] + genome1[to:]                          # test_a_jump_inside_one_unitig_is_a_break
    for reads, sq, sol, want in (([a, b], seqs, solid, [0, END, 0, END]), ([jump], seqs1, solid1, [BREAK, END])):
        bases, offs, paths, got, out = corrected_over(reads, sq, sol, k)
        l2, k2 = csr(overlap_links(sq, k))
        j = read_walks_np(paths["seg_offsets"], paths["segments"], lengths_of(sq, k), l2, k2)[0]
        assert [x if x >= UNLINKED else 0 for x in j.tolist()] == want
        assert out == reads and stats_tuple(got["stats"]) == (0,) * 7


def test_reads_without_a_segment_and_reads_shorter_than_k():
    k = 21
    genome, seqs, solid = ground_truth(k)
    reads = ["", "ACGT", "A" * 60, "N" * 30, genome[100:250], "acgtn" * 3, genome[10: 10 + k - 1]]
    _, offs, paths, got, out = corrected_over(reads, seqs, solid, k)
    assert paths["seg_offsets"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and out == reads and stats_tuple(got["stats"]) == (0,) * 7
    assert got["n_changed"].tolist() == [0] * 7


def test_a_head_with_no_room_at_a_unitigs_first_base():
    k = 21
    genome, seqs, solid = ground_truth(k)
    U = seqs[0]
    # three bases in front of the unitig's first base: the head has no room on strand 0; its reverse complement: the tail has none on strand 1
    rd = "ACG" + U[:100]
    for read, stat in ((rd, (0, 0, 0, 0, 0, 1, 0)), (rc_str(rd), (0, 0, 0, 0, 0, 1, 0))):
        _, _, paths, got, out = corrected_over([read], seqs, solid, k)
        assert len(paths["segments"]) == 1 and out == [read] and stats_tuple(got["stats"]) == stat
        assert [(x[0], x[3]) for x in got["regions"][0]] == [("head" if read is rd else "tail", False)]
    # behind the unitig's last base the same; and one base of room is not three
    rd = U[-100:] + "ACG"
    for read in (rd, rc_str(rd)):
        _, _, _, got, out = corrected_over([read], seqs, solid, k)
        assert out == [read] and stats_tuple(got["stats"]) == (0, 0, 0, 0, 0, 1, 0)
    rd = "AC" + U[1:100]
    _, _, _, got, out = corrected_over([rd], seqs, solid, k)
    assert out == [rd] and got["stats"]["ends_no_room"] == 1
    # with room the same head is rewritten (one base in front of U[1:])
    rd = substitute(U[0], 0) + U[1:100]
    _, _, _, got, out = corrected_over([rd], seqs, solid, k)
    assert out == [U[:100]] and stats_tuple(got["stats"]) == (0, 0, 1, 0, 0, 0, 1)


def test_ends_off_and_a_limit_of_zero():
    k = 21
    genome, seqs, solid = ground_truth(k)
    piece = genome[1200: 1200 + READ_LEN]
    rd = substitute(substitute(substitute(piece, 5), 75), 140)  # a head, a gap, a tail
    _, _, _, got, out = corrected_over([rd], seqs, solid, k)
    assert out == [piece] and stats_tuple(got["stats"]) == (1, 0, 1, 1, 0, 0, 3)
    _, _, _, got, out = corrected_over([rd], seqs, solid, k, ends=0)
    assert out == [substitute(substitute(piece, 5), 140)] and stats_tuple(got["stats"]) == (1, 0, 0, 0, 0, 0, 1)
    _, _, _, got, out = corrected_over([rd], seqs, solid, k, max_subst=0)
    assert out == [rd] and stats_tuple(got["stats"]) == (0, 1, 0, 0, 2, 0, 0)


@pytest.mark.parametrize("k,L", [(7, 40), (21, 40)])
def test_twice_round_a_circle_the_gap_at_the_cut_is_empty(k, L):
    """a read that starts in the middle of the cycle's unitig and runs on round it: the k-mers over the cut are in no unitig position (there is no wrap), the next segment
    starts at the cut — same node, but not collinear (the unitig position falls back), so nothing is evaluated; and where the placement makes a collinear gap shorter
    than k (none here) the region would be empty: either way nothing is counted"""
    seq, vals = circle(k, L)
    seqs = unitigs_np(vals, [1] * L, k)["seqs"]
    once = seqs[0][:L]
    for start in (0, 5):
        read = (once + once + once)[start: start + 2 * L + k - 1]
        for rd in (read, rc_str(read)):
            _, _, paths, got, out = corrected_over([rd], seqs, set(vals), k)
            assert len(paths["segments"]) >= 2 and out == [rd] and stats_tuple(got["stats"]) == (0,) * 7
    # an empty region by construction: two segments of one node, collinear with a gap below k
    SEG = paths["segments"].dtype
    sg = np.zeros(2, SEG)
    sg[0] = (0, 0, 0, 5, 0); sg[1] = (0, 5 + k - 1, 5 + k - 1, 5, 0)
    rd = seqs[0][: 10 + 2 * k - 2]
    if len(rd) == 10 + 2 * k - 2:
        bases, offs = pack([rd])
        got = correct_reads_np(bases, offs, np.array([0, 2], np.uint64), sg, seqs, k)
        assert stats_tuple(got["stats"]) == (0,) * 7 and got["regions"] == [[]]
