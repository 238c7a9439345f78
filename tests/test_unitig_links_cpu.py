"""Links between the unitigs (include/gkc.h, "unitigs": side, slot, entry; gkc_graph_unitigs_links), the part that needs no GPU. Two plain Python statements:
A, the definition, over the neighbour masks and the placement of tests/test_unitigs_cpu.py; B, from the unitig SEQUENCES alone, the rule of the reference's LinkTigs.cpp:
every (k-1)-overlap between unitig extremities. At odd k they must agree; the reference's own links of one input (tests/golden/reference_run/
k21_freq_4parts_unitig_links.json, written by tools/make_unitig_links_vector.py from the reference's .unitigs.fa) pin statement A. tests/test_gpu_unitig_links.py
imports the statements."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_graph_cpu import graph_masks_np, neighbours, revcomp
from tests.test_reference_run import DIR
from tests.test_unitigs_cpu import CYCLES, NOT_ISOLATED, circle, fixture_unitigs, unitigs_np
from tests.util import str2int

NAME = "gkc_graph_unitigs_links"
_COMP = str.maketrans("ACGT", "TGCA")


def rc_str(s):
    return s.translate(_COMP)[::-1]


# ------------------------------------------------------------------------------------------------ statement A: the definition
def unitig_links_np(values, k, u, masks=None):
    """values: the solid k-mers in flat order, u: unitigs_np(values, ...) -> the 2 n_unitigs slots, each the ascending list of its entries v << 1 | (0: one arrives at
    the begin of v, 1: at its end). Asserts on the way that the record one arrives at lies at pos 0 / pos L_v - 1 of its unitig."""
    vals = [int(v) for v in values]
    index = {v: i for i, v in enumerate(vals)}
    masks = graph_masks_np(vals, k) if masks is None else masks
    lens = [len(s) - k + 1 for s in u["seqs"]]
    slots = [[] for _ in range(2 * len(lens))]
    for i, x in enumerate(vals):
        un, rev, p = int(u["unitig"][i]), bool(u["reversed"][i]), int(u["pos"][i])
        ends = []                                                   # (side, end of the record that is this side)
        if p == lens[un] - 1:
            ends.append((0, 1 if rev else 0))
        if p == 0:
            ends.append((1, 0 if rev else 1))
        for side, s in ends:
            nib = (int(masks[i]) >> (4 * s)) & 15
            for nt in range(4):
                if not (nib >> nt) & 1:
                    continue
                y = neighbours(x, k)[4 * s + nt]
                ry = revcomp(y, k)
                j = index[min(y, ry)]
                a = (1 - s) if y < ry else s
                v, rev_j = int(u["unitig"][j]), bool(u["reversed"][j])
                begin = a == (0 if rev_j else 1)
                assert int(u["pos"][j]) == (0 if begin else lens[v] - 1), "one arrives at an extremity of the neighbour's unitig"
                slots[2 * un + side].append(v << 1 | (0 if begin else 1))
    return [sorted(s) for s in slots]


# ------------------------------------------------------------------------------------------------ statement B: the (k-1)-overlaps of the sequences (LinkTigs.cpp)
def overlap_links(seqs, k):
    """(u, +) -> (v, +) iff the last k - 1 bases of u are the first k - 1 of v; the three other combinations through reverse complements. A palindromic (k-1)-mer
    matches begins and ends alike: the reference's "nevermind orientation" case falls out of the string comparison."""
    seqs = [s if isinstance(s, str) else bytes(s).decode() for s in seqs]
    starts = {}                                                      # (k-1)-mer -> entries one arrives at reading it
    for v, s in enumerate(seqs):
        starts.setdefault(s[: k - 1], []).append(v << 1 | 0)
        starts.setdefault(rc_str(s)[: k - 1], []).append(v << 1 | 1)
    slots = []
    for s in seqs:
        slots.append(sorted(starts.get(s[-(k - 1):], [])))
        slots.append(sorted(starts.get(rc_str(s)[-(k - 1):], [])))
    return slots


def csr(slots):
    offs = np.zeros(len(slots) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in slots], dtype=np.uint64)
    return offs, np.array([e for s in slots for e in s], np.uint64).reshape(-1)


def slots_of(offsets, links):
    o = [int(x) for x in offsets]
    return [[int(e) for e in links[o[t]: o[t + 1]]] for t in range(len(o) - 1)]


def assert_symmetric(slots):
    """slot 2u + su holds (v, mv) <=> slot 2v + (1 - mv) holds (u, 1 - su); the entries of a slot are distinct"""
    for t, s in enumerate(slots):
        assert len(set(s)) == len(s)
        u, su = t >> 1, t & 1
        for e in s:
            v, mv = e >> 1, e & 1
            assert (u << 1 | (1 - su)) in slots[2 * v + (1 - mv)], (t, e)


def links_digest(seqs, slots):
    """[unitigs, links, sha256]: each link one line "ru su rv sv", ru / rv the ranks of the two unitigs' canonical sequences among all sorted canonical sequences,
    su / sv the side left through and the sign arrived with, relative to the canonical orientation (a unitig stored as the reverse complement of its canonical
    form has its side and its sign flipped); the lines sorted, joined by newlines"""
    seqs = [s if isinstance(s, str) else bytes(s).decode() for s in seqs]
    can = [min(s, rc_str(s)) for s in seqs]
    rank = {c: r for r, c in enumerate(sorted(can))}
    assert len(rank) == len(seqs)
    flip = [c != s for c, s in zip(can, seqs)]
    lines = []
    for t, s in enumerate(slots):
        u, su = t >> 1, t & 1
        for e in s:
            v, mv = e >> 1, e & 1
            lines.append("%d %s %d %s" % (rank[can[u]], "+-"[su ^ flip[u]], rank[can[v]], "+-"[mv ^ flip[v]]))
    lines.sort()
    return [len(seqs), len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()]


def reference_links_digest():
    want = json.load(open(os.path.join(DIR, "k21_freq_4parts_unitig_links.json")))
    assert want["k"] == 21
    return [want["unitigs"], want["links"], want["sha256_sorted_links"]]


def parse_unitigs_fasta(path):
    """a .unitigs.fa in the layout of bcalm2, the header fields as GraphUnitigs.cpp:304-359 (parse_unitig_header) reads them: tokens separated by white space, a token
    shorter than 3 characters is the id, "L:<+|->:<unitig>:<+|->" a link, "km:f:<x>" the mean abundance -> (ids, fields dict per unitig, sequences, slots)"""
    ids, fields, seqs, slots = [], [], [], []
    for line in open(path):
        line = line.rstrip("\n")
        if not line.startswith(">"):
            seqs.append(line)
            continue
        toks = line[1:].split()
        ids.append(int(toks[0]))
        f = {}
        plus, minus = [], []
        for tok in toks[1:]:
            if tok[:2] == "L:":
                _, side, v, sign = tok.split(":")
                assert side in "+-" and sign in "+-"
                (minus if side == "-" else plus).append(int(v) << 1 | (sign == "-"))
            else:
                name, typ, val = tok.split(":")
                f[name] = int(val) if typ == "i" else val
        fields.append(f); slots.append(plus); slots.append(minus)
    assert len(seqs) == len(ids)
    return ids, fields, seqs, slots


@functools.lru_cache(maxsize=None)
def fixture_links(name):
    k, values, ab, u = fixture_unitigs(name)
    return k, u, unitig_links_np(values, k, u)


def histogram(slots):
    return [sum(len(s) == d for s in slots) for d in range(5)]


# ------------------------------------------------------------------------------------------------ tests
def test_export_is_declared_mapped_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    assert NAME in gkc.SYMBOLS
    assert ("int %s(gkc_ctx* ctx, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs," % NAME) in hdr
    assert '"graph_unitig_links"' in hdr
    vmap = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc.map")).read()
    assert "gkc_*" in vmap or NAME in vmap
    for meth in ("unitig_links", "unitig_links_device", "write_unitigs_fasta"):
        assert callable(getattr(gkc.Counter, meth))
    L = gkc.lib()
    assert len(getattr(L, NAME).argtypes) == 7


@pytest.mark.parametrize("name,n_links", [("k21_freq_4parts", 1528), ("k21_defaults_parts", 1528), ("k31_defaults", 168), ("k63_defaults", 8)])
def test_definition_equals_the_overlaps_on_the_fixtures(name, n_links):
    k, u, slots = fixture_links(name)
    assert slots == overlap_links(u["seqs"], k)
    assert_symmetric(slots)
    assert sum(len(s) for s in slots) == n_links
    if name.startswith("k21"):
        assert len(u["seqs"]) == 711 and histogram(slots) == [280, 756, 386, 0, 0]
        assert all((e >> 1) != (t >> 1) for t, s in enumerate(slots) for e in s)      # no self-links in this input


def test_definition_reproduces_the_reference_links():
    k, u, slots = fixture_links("k21_freq_4parts")
    assert links_digest(u["seqs"], slots) == reference_links_digest()


@pytest.mark.parametrize("k", [3, 5, 7])
def test_fuzz_over_random_subsets_odd_k(k):
    rng = np.random.default_rng(100 + k)                            # the subsets of test_fuzz_over_random_subsets
    every = sorted({min(x, revcomp(x, k)) for x in range(4 ** k)})
    top = 0
    for density in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9):
        vals = [x for x in every if rng.random() < density]
        u = unitigs_np(vals, rng.integers(1, 50, len(vals)).tolist(), k)
        slots = unitig_links_np(vals, k, u)
        assert slots == overlap_links(u["seqs"], k)
        assert_symmetric(slots)
        top = max(top, max(len(s) for s in slots))
    assert top == 4                                                 # over the densities together: a sparse subset of the 32 canonical 3-mers cannot hold a side of degree 4


@pytest.mark.parametrize("k", [4, 6])
def test_fuzz_over_random_subsets_even_k(k):
    """the structural fact of the definition (arrival at pos 0 / pos L - 1, asserted inside the statement) holds at even k, and every link of the definition is a
    (k-1)-overlap of the sequences (a neighbour shares k - 1 bases) with no entry twice in a slot; the overlaps hold MORE where palindromes stand, so equality is not
    asserted there, and that they do differ is"""
    rng = np.random.default_rng(100 + k)
    every = sorted({min(x, revcomp(x, k)) for x in range(4 ** k)})
    differs = False
    for density in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9):
        vals = [x for x in every if rng.random() < density]
        u = unitigs_np(vals, rng.integers(1, 50, len(vals)).tolist(), k)
        slots = unitig_links_np(vals, k, u)
        over = overlap_links(u["seqs"], k)
        assert len(slots) == len(over)
        for a, b in zip(slots, over):
            assert len(set(a)) == len(a) and set(a) <= set(b)
        differs = differs or slots != over
    assert differs


@pytest.mark.parametrize("k,L", [c for c in CYCLES if c not in NOT_ISOLATED])
def test_an_isolated_circle_links_to_itself(k, L):
    seq, vals = circle(k, L)
    u = unitigs_np(vals, [1] * L, k)
    slots = unitig_links_np(vals, k, u)
    assert slots == [[0 << 1 | 0], [0 << 1 | 1]]                    # L:+:0:+ and L:-:0:-
    assert slots == overlap_links(u["seqs"], k)
    assert_symmetric(slots)


def statement_of_reads(reads, k):
    """every k-mer of the reads is solid, one dataset: flat order = ascending -> (values, unitigs_np, slots)"""
    vals = sorted({min(x, revcomp(x, k)) for r in reads for x in (str2int(r[i: i + k]) for i in range(len(r) - k + 1))})
    u = unitigs_np(vals, [1] * len(vals), k)
    slots = unitig_links_np(vals, k, u)
    assert slots == overlap_links(u["seqs"], k)
    assert_symmetric(slots)
    return vals, u, slots


def random_sequence(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def hairpin_reads(k=21):
    rng = np.random.default_rng(3)
    half = random_sequence(rng, (k - 1) // 2)
    lead = random_sequence(rng, 30)
    return [lead + "A" + half + rc_str(half) + "T"]


def poly_a_reads():
    rng = np.random.default_rng(1)                                  # (the seeds: the flanks' unitigs are numbered and oriented as in the lists asserted below)
    return [random_sequence(rng, 30) + "A" * 30 + random_sequence(rng, 30)]


def fork_reads():
    rng = np.random.default_rng(7)
    lead, x, y, z = (random_sequence(rng, 30) for _ in range(4))
    return [lead + x, lead + y, z + lead]


def star_reads():
    rng = np.random.default_rng(6)
    lead = random_sequence(rng, 30)
    return [lead + X + random_sequence(rng, 30) for X in "ACGT"]


def test_a_hairpin_links_its_end_to_its_own_end():
    vals, u, slots = statement_of_reads(hairpin_reads(), 21)
    assert len(u["seqs"]) == 1 and slots == [[1], []]               # L:+:0:-


def test_a_poly_a_record_links_to_itself_on_both_sides():
    vals, u, slots = statement_of_reads(poly_a_reads(), 21)
    assert len(u["seqs"]) == 3
    assert slots == [[0, 2], [1, 5], [], [1, 5], [0, 2], []]


def test_a_fork():
    vals, u, slots = statement_of_reads(fork_reads(), 21)
    assert len(u["seqs"]) == 3
    assert slots == [[3, 4], [], [1], [], [], [1]]


def test_a_star_has_one_side_of_degree_four():
    vals, u, slots = statement_of_reads(star_reads(), 21)
    assert len(u["seqs"]) == 5 and histogram(slots) == [5, 4, 0, 0, 1]
    four = [s for s in slots if len(s) == 4][0]
    assert four == sorted(four) and len({e >> 1 for e in four}) == 4


def test_fasta_header_parser(tmp_path):
    p = tmp_path / "x.unitigs.fa"
    p.write_text(">0 LN:i:25 KC:i:10 km:f:2.0  L:+:1:- L:+:2:+ L:-:0:- \nACGTACGTACGTACGTACGTACGTA\n>1 LN:i:21 KC:i:3 km:f:3.0 \nACGTACGTACGTACGTACGTT\n")
    ids, fields, seqs, slots = parse_unitigs_fasta(str(p))
    assert ids == [0, 1] and [f["LN"] for f in fields] == [25, 21] and [f["KC"] for f in fields] == [10, 3] and [f["km"] for f in fields] == ["2.0", "3.0"]
    assert slots == [[3, 4], [1], [], []] and [len(s) for s in seqs] == [25, 21]
