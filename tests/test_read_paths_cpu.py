"""Read paths (include/gkc.h, "read paths"; csrc/gkc_paths.hip and the third mode of k_q_reads), the part that needs no GPU: the two exports are declared and bound, the
segment record is 24 bytes on both sides, and a plain Python statement of the definition — read_paths_np — built from the unitig SEQUENCES only: a dictionary from
canonical k-mer to (unitig, position, spelled forward?) made by slicing every unitig string, and the set of solid values to tell a removed k-mer from an absent one. It
knows nothing of the record order or of the placement arrays the device gathers from. It is pinned here on the reference's own unitigs of one input (the fixture of
tests/test_unitigs_cpu.py, which carries the reference's sha256) and on hand-made cases; tests/test_gpu_read_paths.py imports it."""
import ctypes
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_reference_run import DIR, load
from tests.test_unitigs_cpu import circle, fixture_unitigs, unitigs_np
from tests.util import CODE, str2int

NAMES = ["gkc_graph_reads_nodes_device", "gkc_graph_reads_segments_device"]
SEGMENT = np.dtype([("node", np.uint64), ("read_pos", np.uint32), ("unitig_pos", np.uint32), ("n_kmers", np.uint32), ("pad", np.uint32)])
MAPPED, REMOVED, ABSENT, NO_KMER = 0, 1, 2, 3
NONE64 = np.uint64((1 << 64) - 1)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------------------------------------ the statement
def kmers_per_position(read, k):
    """read: bytes -> per position (forward k-mer, its reverse complement) as Python ints, or None where no k-mer starts: fewer than k bases left, or a character
    outside ACGTacgt in the window"""
    out = [None] * len(read)
    mask = (1 << (2 * k)) - 1
    f = rc = good = 0
    for i, ch in enumerate(read):
        code = CODE.get(ch)
        if code is None:
            f = rc = good = 0
            continue
        f = ((f << 2) | code) & mask
        rc = (rc >> 2) | ((code ^ 2) << (2 * (k - 1)))
        good += 1
        if good >= k:
            out[i - k + 1] = (f, rc)
    return out


def unitig_index(seqs, k):
    """canonical k-mer -> (unitig, position, the unitig spells the canonical form there), by slicing every unitig string; a k-mer in two places is an error"""
    index = {}
    for u, s in enumerate(seqs):
        s = s if isinstance(s, str) else bytes(s).decode()
        for p, pair in enumerate(kmers_per_position(s.encode(), k)[: len(s) - k + 1]):
            f, rc = pair
            c = min(f, rc)
            assert c not in index, "k-mer %x lies in two places of the unitigs" % c
            index[c] = (u, p, f == c)
    return index


def read_paths_np(bases, offsets, seqs, k, solid):
    """bases, offsets: the flat read buffer; seqs: the unitigs as strings; solid: the canonical values of the results (a set) -> dict:
    unitig uint64[n] (2^64 - 1 unless mapped), strand bool[n], pos uint32[n], status uint8[n] (0 mapped, 1 removed, 2 absent, 3 no k-mer), seg_offsets uint64[n_reads + 1],
    segments SEGMENT[], support uint64[n_unitigs]"""
    index = unitig_index(seqs, k)
    raw = np.asarray(bases, np.uint8).tobytes()
    offs = [int(x) for x in offsets]
    n = offs[-1]
    unitig = np.full(n, NONE64, np.uint64); strand = np.zeros(n, bool); pos = np.zeros(n, np.uint32); status = np.full(n, NO_KMER, np.uint8)
    seg_offsets = np.zeros(len(offs), np.uint64); segs = []; support = np.zeros(len(seqs), np.uint64)
    for r in range(len(offs) - 1):
        b = offs[r]
        prev = None                                             # (unitig, strand, pos) of the position before, inside this read
        for j, pair in enumerate(kmers_per_position(raw[b: offs[r + 1]], k)):
            cur = None
            if pair is not None:
                f, rc = pair
                c = min(f, rc)
                hit = index.get(c)
                if hit is None:
                    status[b + j] = REMOVED if c in solid else ABSENT
                else:
                    u, p, fwd = hit
                    s = (f == c) != fwd                         # the read spells the slice itself, or its reverse complement
                    unitig[b + j], strand[b + j], pos[b + j], status[b + j] = u, s, p, MAPPED
                    cur = (u, s, p)
            if cur is not None:
                if prev is not None and prev[:2] == cur[:2] and cur[2] == prev[2] + (-1 if cur[1] else 1):
                    segs[-1][3] += 1
                else:
                    segs.append([(cur[0] << 1) | int(cur[1]), j, cur[2], 1])
                support[cur[0]] += np.uint64(1)
            prev = cur
        seg_offsets[r + 1] = len(segs)
    segments = np.zeros(len(segs), SEGMENT)
    for i, (node, rp, up, nk) in enumerate(segs):
        segments[i] = (node, rp, up, nk, 0)
    return dict(unitig=unitig, strand=strand, pos=pos, status=status, seg_offsets=seg_offsets, segments=segments, support=support)


def expand_segments(seg_offsets, segments, offsets):
    """the per-position arrays the segments stand for -> (unitig, strand, pos, mapped)"""
    n = int(offsets[-1])
    unitig = np.full(n, NONE64, np.uint64); strand = np.zeros(n, bool); pos = np.zeros(n, np.uint32); mapped = np.zeros(n, bool)
    for r in range(len(offsets) - 1):
        last_end = 0
        for s in segments[int(seg_offsets[r]): int(seg_offsets[r + 1])]:
            g, nk, st = int(offsets[r]) + int(s["read_pos"]), int(s["n_kmers"]), bool(int(s["node"]) & 1)
            assert nk > 0 and int(s["read_pos"]) >= last_end and g + nk <= int(offsets[r + 1]) and not mapped[g: g + nk].any() and s["pad"] == 0
            last_end = int(s["read_pos"]) + nk
            unitig[g: g + nk] = int(s["node"]) >> 1; strand[g: g + nk] = st; mapped[g: g + nk] = True
            pos[g: g + nk] = int(s["unitig_pos"]) + (-1 if st else 1) * np.arange(nk)
    return unitig, strand, pos, mapped


def assert_consistent(got, offsets):
    """what every answer satisfies: the segments are maximal, expand to the per-position arrays, and the support counts the mapped positions per unitig"""
    u, s, p, m = expand_segments(got["seg_offsets"], got["segments"], offsets)
    assert np.array_equal(m, got["status"] == MAPPED)
    assert np.array_equal(u, got["unitig"]) and np.array_equal(s, got["strand"]) and np.array_equal(p, got["pos"])
    assert (got["unitig"][~m] == NONE64).all() and not got["strand"][~m].any() and not got["pos"][~m].any()
    assert int(got["support"].sum()) == int(m.sum())
    assert np.array_equal(got["support"], np.bincount(got["unitig"][m].astype(np.int64), minlength=len(got["support"])).astype(np.uint64))
    sg = got["segments"]
    for r in range(len(offsets) - 1):                           # maximal: two neighbours in a read never continue each other
        a = sg[int(got["seg_offsets"][r]): int(got["seg_offsets"][r + 1])]
        for x, y in zip(a[:-1], a[1:]):
            st = -1 if int(x["node"]) & 1 else 1
            assert not (x["node"] == y["node"] and int(x["read_pos"]) + int(x["n_kmers"]) == int(y["read_pos"])
                        and int(y["unitig_pos"]) == int(x["unitig_pos"]) + st * int(x["n_kmers"]))


def pack(reads):
    rs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offs = np.zeros(len(rs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rs], dtype=np.uint64)
    return np.frombuffer(b"".join(rs), np.uint8).copy(), offs


def rc_str(s):
    return s.encode().translate(_COMP)[::-1].decode()


def parse_fasta(text):
    """one sequence per header line, lines joined: the reads of a fixture's FASTA as the device parser gives them"""
    reads, cur = [], None
    for line in bytes(text).split(b"\n"):
        line = line.rstrip(b"\r")
        if line[:1] in (b">", b"@"):
            if cur is not None:
                reads.append(b"".join(cur))
            cur = []
        elif line and cur is not None:
            cur.append(line)
    if cur is not None:
        reads.append(b"".join(cur))
    return reads


@functools.lru_cache(maxsize=None)
def fixture_paths(name):
    """the statement over a reference-run fixture: its own FASTA as reads against the unitigs of its solid set -> (k, bases, offsets, unitig strings, read_paths_np(...))"""
    z = np.load(os.path.join(DIR, name + ".npz"))
    k, values, ab, u = fixture_unitigs(name)
    bases, offs = pack(parse_fasta(z["fasta"]))
    return k, bases, offs, u["seqs"], read_paths_np(bases, offs, u["seqs"], k, set(values))


def graph_of(reads, k):
    """the unitigs (strings) and the solid set of every k-mer of ``reads``"""
    solid = set()
    for r in reads:
        solid |= {min(p) for p in kmers_per_position(r.encode(), k) if p is not None}
    vals = sorted(solid)
    return unitigs_np(vals, [1] * len(vals), k)["seqs"], solid


def random_sequence(seed, n):
    return "".join("ACGT"[b] for b in np.random.default_rng(seed).integers(0, 4, n))


# ------------------------------------------------------------------------------------------------ tests
def test_exports_are_declared_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    for n in NAMES:
        assert n in gkc.SYMBOLS, n
        assert ("int %s(gkc_ctx* ctx, " % n) in hdr, n
        assert "gkc_*" in vmap or n in vmap
    assert "typedef struct gkc_read_segment" in hdr and '"graph_read_nodes"' in hdr and '"graph_read_segments"' in hdr
    for name in ("GKC_NODE_REMOVED", "GKC_NODE_ABSENT", "GKC_NODE_NO_KMER"):
        assert "#define %s " % name in hdr
    for meth in ("read_nodes", "read_nodes_device", "read_segments", "read_segments_device"):
        assert callable(getattr(gkc.Counter, meth))


def test_the_segment_record_is_24_bytes():
    gkc = ge.load().gkc
    assert ctypes.sizeof(gkc.ReadSegment) == 24 == gkc.READ_SEGMENT.itemsize
    assert gkc.READ_SEGMENT == SEGMENT
    assert [(n, getattr(gkc.ReadSegment, n).offset) for n, _ in gkc.ReadSegment._fields_] == [(n, SEGMENT.fields[n][1]) for n in SEGMENT.names]
    assert (gkc.NODE_REMOVED, gkc.NODE_ABSENT, gkc.NODE_NO_KMER) == (2 ** 64 - 1, 2 ** 64 - 2, 2 ** 64 - 3)


def test_statement_on_the_reference_unitigs():
    """k21_freq_4parts: the reads of the fixture's FASTA against the reference's own unitigs of them (abundance-min 2). Of the 900,000 positions (6000 reads of 150 bases) 613,958 are mapped,
    134,449 absent (k-mers seen once) and 151,593 carry no k-mer (the last 20 positions of every read, and 31,593 windows with an N); none is removed: every solid k-mer
    lies in a unitig"""
    k, bases, offs, seqs, got = fixture_paths("k21_freq_4parts")
    _, values, _, _ = fixture_unitigs("k21_freq_4parts")
    solid = set(values)
    raw = bases.tobytes()
    counts = np.bincount(got["status"], minlength=4).tolist()
    print("k21_freq_4parts: %d positions: mapped, removed, absent, no k-mer = %s; %d segments" % (len(bases), counts, len(got["segments"])))
    assert counts == [613958, 0, 134449, 151593] and len(bases) == 900000 and counts[3] > 6000 * (k - 1)
    n_valid = 0
    for r in range(len(offs) - 1):
        b, e = int(offs[r]), int(offs[r + 1])
        for j, pair in enumerate(kmers_per_position(raw[b:e], k)):
            g = b + j
            if pair is None:
                assert got["status"][g] == NO_KMER
                continue
            n_valid += 1
            assert (got["status"][g] == MAPPED) == (min(pair) in solid)      # mapped if and only if the canonical value is among the fixture's solid values
            if got["status"][g] == MAPPED:
                p = int(got["pos"][g])
                w = seqs[int(got["unitig"][g])][p: p + k]
                assert (rc_str(w) if got["strand"][g] else w) == raw[g: g + k].decode()
    assert n_valid == counts[0] + counts[2]
    assert_consistent(got, offs)
    assert int(got["support"].sum()) == counts[0] and (got["support"] > 0).all()      # the reads are the input the unitigs were made from


def test_a_substitution_splits_a_read_in_two():
    k = 11
    genome = random_sequence(1, 80)
    seqs, solid = graph_of([genome], k)
    assert seqs in ([genome], [rc_str(genome)])
    at = 40
    read = genome[:at] + ("C" if genome[at] != "C" else "G") + genome[at + 1:]
    bases, offs = pack([read])
    got = read_paths_np(bases, offs, seqs, k, solid)
    assert_consistent(got, offs)
    assert got["status"].tolist() == [MAPPED] * (at - k + 1) + [ABSENT] * k + [MAPPED] * (80 - k + 1 - (at + 1)) + [NO_KMER] * (k - 1)
    s = got["segments"]
    assert len(s) == 2 and s["node"][0] == s["node"][1] and s["read_pos"].tolist() == [0, at + 1] and s["n_kmers"].tolist() == [at - k + 1, 80 - k - at]
    fwd = seqs[0] == genome
    assert s["unitig_pos"].tolist() == ([0, at + 1] if fwd else [80 - k, 80 - k - at - 1]) and int(s["node"][0]) & 1 == (0 if fwd else 1)
    assert got["support"].tolist() == [80 - k + 1 - k]


def test_a_read_across_a_branching_node():
    k = 11
    stem, left, right = random_sequence(2, 40), random_sequence(102, 30), random_sequence(202, 30)
    assert left[0] != right[0]
    a, b = stem + left, stem + right
    seqs, solid = graph_of([a, b], k)
    assert len(seqs) == 3                                       # the stem and the two branches
    bases, offs = pack([a, b])
    got = read_paths_np(bases, offs, seqs, k, solid)
    assert_consistent(got, offs)
    assert (got["status"] == MAPPED).sum() == 2 * (70 - k + 1) and got["seg_offsets"].tolist() == [0, 2, 4]
    s = got["segments"]
    assert s["read_pos"].tolist() == [0, 40 - k + 1, 0, 40 - k + 1] and s["n_kmers"].tolist() == [40 - k + 1, 30, 40 - k + 1, 30]
    assert s["node"][0] == s["node"][2] and len({int(x) >> 1 for x in s["node"][[0, 1, 3]]}) == 3
    assert sorted(got["support"].tolist()) == [30, 30, 2 * (40 - k + 1)]


def test_the_reverse_complement_mirrors_the_segments():
    k = 11
    stem, left, right = random_sequence(2, 40), random_sequence(102, 30), random_sequence(202, 30)
    a, b = stem + left, stem + right
    seqs, solid = graph_of([a, b], k)
    read = a[:55] + ("C" if a[55] != "C" else "G") + a[56:]     # three segments: stem, branch, (k absent), branch
    bases, offs = pack([read, rc_str(read)])
    got = read_paths_np(bases, offs, seqs, k, solid)
    assert_consistent(got, offs)
    assert got["seg_offsets"].tolist() == [0, 3, 6]
    n_pos = len(read) - k + 1
    fw, rv = got["segments"][:3], got["segments"][3:][::-1]
    for x, y in zip(fw, rv):
        st = -1 if int(x["node"]) & 1 else 1
        assert int(y["node"]) == int(x["node"]) ^ 1 and y["n_kmers"] == x["n_kmers"]
        assert int(y["read_pos"]) == n_pos - (int(x["read_pos"]) + int(x["n_kmers"]))
        assert int(y["unitig_pos"]) == int(x["unitig_pos"]) + st * (int(x["n_kmers"]) - 1)


@pytest.mark.parametrize("k,L", [(7, 40), (21, 40)])
def test_a_cycle_read_twice_round_breaks_at_the_cut(k, L):
    seq, vals = circle(k, L)
    seqs = unitigs_np(vals, [1] * L, k)["seqs"]
    assert len(seqs) == 1 and len(seqs[0]) == L + k - 1
    for read in (seq + seq + seq[: k - 1], rc_str(seq + seq + seq[: k - 1])):
        bases, offs = pack([read])
        got = read_paths_np(bases, offs, seqs, k, set(vals))
        assert_consistent(got, offs)
        s = got["segments"]
        assert (got["status"][: 2 * L] == MAPPED).all() and int(s["n_kmers"].sum()) == 2 * L and got["support"].tolist() == [2 * L]
        assert len(set(s["node"].tolist())) == 1 and len(s) in (2, 3) and L in s["n_kmers"].tolist()
        st = int(s["node"][0]) & 1
        for x in s[1:]:                                         # every segment after the first starts at the cut: there is no wrap
            assert int(x["unitig_pos"]) == (L - 1 if st else 0)
        for x in s[:-1]:
            assert int(x["unitig_pos"]) + (-1 if st else 1) * (int(x["n_kmers"]) - 1) == (0 if st else L - 1)


def test_an_even_k_palindrome_stands_forward():
    k = 6
    pal = "ACGCGT"
    assert rc_str(pal) == pal
    genome = "TTGACA" + pal + "GGATCA"
    seqs, solid = graph_of([genome], k)
    x = str2int(pal)
    own = [u for u, s in enumerate(seqs) if pal in s or pal in rc_str(s)]
    assert len(own) == 1 and len(seqs[own[0]]) == k              # a unitig of its own
    for read in (genome, rc_str(genome)):
        bases, offs = pack([read])
        got = read_paths_np(bases, offs, seqs, k, solid)
        assert_consistent(got, offs)
        at = read.index(pal)
        assert got["status"][at] == MAPPED and got["unitig"][at] == own[0] and not got["strand"][at] and got["pos"][at] == 0
        assert (got["status"][: len(read) - k + 1] == MAPPED).all() and x in solid


def test_removed_and_absent_are_told_apart():
    k = 11
    genome = random_sequence(5, 60)
    seqs, solid = graph_of([genome], k)
    more = solid | {min(p) for p in kmers_per_position(("A" * k).encode(), k) if p is not None}      # in the results, in no unitig
    bases, offs = pack(["A" * (k + 2), "C" * k, "ACGTN" * 4, "acgt" * 5, ""])
    got = read_paths_np(bases, offs, seqs, k, more)
    assert_consistent(got, offs)
    assert got["status"][: k + 2].tolist() == [REMOVED] * 3 + [NO_KMER] * (k - 1) and got["status"][k + 2] == ABSENT
    assert (got["status"][int(offs[2]): int(offs[3])] == NO_KMER).all()                              # k = 11 > 4 bases between two N
    assert (got["status"][int(offs[3]): int(offs[3]) + 10] == ABSENT).all() and len(got["segments"]) == 0
