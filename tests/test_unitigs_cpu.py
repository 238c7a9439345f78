"""Unitigs of the solid k-mers (include/gkc.h, "unitigs"; csrc/gkc_unitigs.hip), the part that needs no GPU: the three exports are declared and bound, and a plain
Python statement of the definition — links between the ends of the records, unitigs as the components of the link graph, their sequences — built on the neighbours
of tests/test_graph_cpu.py and pinned by the reference's OWN unitigs of one input (tests/golden/reference_run/k21_freq_4parts_unitigs.json: count, total length, sha256
of the sorted canonical sequences), not by the code under test. The statement walks the links record by record; the device ranks them by pointer jumping.
tests/test_gpu_unitigs.py imports the statement."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_graph_cpu import graph_masks_np, neighbours, revcomp
from tests.test_reference_run import DIR, load

NAMES = ["gkc_graph_unitigs_build", "gkc_graph_unitigs_write", "gkc_graph_unitigs_nodes"]
NONE = -1
_POP4 = [bin(i).count("1") for i in range(16)]
_LETTERS = "ACTG"                                              # nucleotide codes 0..3
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ------------------------------------------------------------------------------------------------ the statement
def links_np(values, k, masks=None):
    """values: the solid k-mers (canonical Python ints) in flat order -> int64[2n]: link[2i + s] = 2j + a or NONE. End s = 0 of record i is its right end (mask bits
    0-3), s = 1 its left end (bits 4-7); one arrives at end a of record j."""
    vals = [int(v) for v in values]
    index = {v: i for i, v in enumerate(vals)}
    masks = graph_masks_np(vals, k) if masks is None else masks
    link = np.full(2 * len(vals), NONE, np.int64)
    for i, x in enumerate(vals):
        for s in (0, 1):
            nib = (int(masks[i]) >> (4 * s)) & 15
            if _POP4[nib] != 1:
                continue
            y = neighbours(x, k)[4 * s + nib.bit_length() - 1]
            ry = revcomp(y, k)
            if x == revcomp(x, k) or y == ry:                   # a palindrome is a unitig of its own and nothing links to it
                continue
            c = min(y, ry)
            j = index[c]
            a = (1 - s) if c == y else s                        # leaving right one arrives at a left end when the neighbour is canonical as it stands, and so on
            if j == i or _POP4[(int(masks[j]) >> (4 * a)) & 15] != 1:
                continue
            link[2 * i + s] = 2 * j + a
    return link


def _walk(link, i, s, stop=None):
    """the records met leaving record i through end s, as (record, reversed), record i first; stops at an end without a link, or on coming back to ``stop``"""
    path = [(i, s == 1)]                                        # leaving through the left end: the record stands reverse-complemented
    cur = i
    while True:
        t = int(link[2 * cur + s])
        if t == NONE:
            return path
        j, a = t >> 1, t & 1
        if j == stop:
            return path
        path.append((j, a == 0))                                # entered through its right end: reverse-complemented
        cur, s = j, 1 - a


def unitig_paths(link):
    """-> (paths, n_cycles): every unitig as a list of (record, reversed), numbered by ascending start record"""
    n = len(link) // 2
    seen = np.zeros(n, bool)
    paths, n_cycles = [], 0
    for i in range(n):                                          # paths: met first at the end record with the smaller index
        if seen[i] or (link[2 * i] != NONE and link[2 * i + 1] != NONE):
            continue
        p = _walk(link, i, 0 if link[2 * i] != NONE else (1 if link[2 * i + 1] != NONE else 0))
        if len(p) == 1:
            p = [(i, False)]                                    # a single record stands forward
        for r, _ in p:
            assert not seen[r]
            seen[r] = True
        paths.append(p)
    for i in range(n):                                          # what is left lies on cycles: cut at the left end of the smallest record, which stands forward
        if seen[i]:
            continue
        p = _walk(link, i, 0, stop=i)
        for r, _ in p:
            assert not seen[r]
            seen[r] = True
        paths.append(p); n_cycles += 1
    paths.sort(key=lambda p: p[0][0])
    return paths, n_cycles


def kmer_str(x, k):
    return "".join(_LETTERS[(x >> (2 * (k - 1 - t))) & 3] for t in range(k))


def unitigs_np(values, abundances, k, masks=None):
    """-> dict: bases uint8[n_bases] (ASCII), offsets uint64[n_unitigs + 1], kc uint64[n_unitigs], unitig int64[n], reversed bool[n], pos int64[n], n_cycles, link"""
    vals = [int(v) for v in values]
    link = links_np(vals, k, masks)
    paths, n_cycles = unitig_paths(link)
    n = len(vals)
    unitig = np.full(n, -1, np.int64); rev = np.zeros(n, bool); pos = np.zeros(n, np.int64)
    seqs, kc = [], []
    for u, p in enumerate(paths):
        s = None
        for q, (r, rv) in enumerate(p):
            unitig[r], rev[r], pos[r] = u, rv, q
            w = kmer_str(revcomp(vals[r], k) if rv else vals[r], k)
            if s is None:
                s = [w]
            else:
                assert w[:-1] == prev[1:], "consecutive records overlap by k - 1 bases"
                s.append(w[-1])
            prev = w
        seqs.append("".join(s)); kc.append(sum(int(abundances[r]) for r, _ in p))
    assert (unitig >= 0).all()
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    bases = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
    return dict(bases=bases, offsets=offsets, kc=np.array(kc, np.uint64).reshape(-1), unitig=unitig, reversed=rev, pos=pos, n_cycles=n_cycles, link=link, seqs=seqs)


def unitig_sequences(values, k, masks=None):
    """the unitigs as ASCII strings, numbered by ascending start record"""
    return unitigs_np(values, [0] * len(values), k, masks)["seqs"]


def canonical_digest(seqs):
    """[count, total length, sha256 of the sorted canonical sequences joined by newlines]: what the fixture of the reference's unitigs holds"""
    can = sorted(min(b, b.translate(_COMP)[::-1]) for b in (s.encode() if isinstance(s, str) else bytes(s) for s in seqs))
    return [len(can), sum(len(x) for x in can), hashlib.sha256(b"\n".join(can)).hexdigest()]


def split_sequences(bases, offsets):
    b = np.asarray(bases, np.uint8).tobytes()
    o = [int(x) for x in offsets]
    return [b[o[i]: o[i + 1]] for i in range(len(o) - 1)]


def reference_digest():
    want = json.load(open(os.path.join(DIR, "k21_freq_4parts_unitigs.json")))
    return [want["unitigs"], want["total_length"], want["sha256_sorted_canonical"]]


@functools.lru_cache(maxsize=None)
def fixture_unitigs(name):
    """the statement over the solid set of a reference-run fixture, flat order = dataset order -> (k, values, abundances, unitigs_np(...)); computed once per run"""
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    values = [v for p in parts for v, _ in p]; ab = [a for p in parts for _, a in p]
    return k, values, ab, unitigs_np(values, ab, k)


# ------------------------------------------------------------------------------------------------ inputs with a known shape
def circular_sequence(k, L, seed, isolated=True, budget=60000):
    """a circular sequence of L bases (string) whose L k-mers are L distinct canonical k-mers, none a palindrome, and, with ``isolated``, form ONE isolated cycle of the
    graph: no k-mer of the cycle is a neighbour of another one except along the cycle, or of itself. Grown base by base, depth first (at small k a sequence drawn blindly
    almost never is one); the last k - 1 k-mers wrap around into the first bases and have no choice. None found within the budget: AssertionError."""
    rng = np.random.default_rng(seed)
    mask = (1 << (2 * k)) - 1

    def canon(x):
        return min(x, revcomp(x, k))

    def clean(x, used, allowed):
        c = canon(x)
        if c in used or x == revcomp(x, k):
            return False
        if not isolated:
            return True
        return all(cn in allowed or (cn not in used and cn != c) for cn in (canon(nb) for nb in neighbours(x, k)))

    for attempt in range(40):
        seq = [int(b) for b in rng.integers(0, 4, k)]
        x = 0
        for b in seq:
            x = (x << 2) | b
        if not clean(x, set(), set()):
            continue
        kmers = [x]; used = {canon(x)}; choices = []
        steps = 0
        while steps < budget and len(kmers) < L:
            t = len(kmers)                                     # k-mer t ends with the base at position t + k - 1 (mod L)
            if len(choices) < t:
                choices.append([seq[(t + k - 1) % L]] if t + k - 1 >= L else [int(b) for b in rng.permutation(4)])
            placed = False
            while choices[t - 1] and not placed:
                b = choices[t - 1].pop(); steps += 1
                y = ((kmers[-1] << 2) | b) & mask
                if clean(y, used, {canon(kmers[-1])} | ({canon(kmers[0])} if t == L - 1 else set())):
                    if t + k - 1 < L:
                        seq.append(b)
                    kmers.append(y); used.add(canon(y)); placed = True
            if placed:
                continue
            choices.pop()                                      # dead end: take k-mer t - 1 back
            if t == 1:
                break
            used.discard(canon(kmers.pop()))
            if t + k - 2 < L:
                seq.pop()
        if len(kmers) == L:
            assert len(seq) == L
            return "".join(_LETTERS[b] for b in seq)
    raise AssertionError("no such circle of %d %d-mers found" % (L, k))


def circular_kmers(seq, k):
    """the canonical k-mers of a circular sequence, ascending (= the flat order of a single dataset)"""
    from tests.util import str2int
    ext = seq + seq[: k - 1]
    return sorted(min(x, revcomp(x, k)) for x in (str2int(ext[i: i + k]) for i in range(len(seq))))


# ------------------------------------------------------------------------------------------------ tests
def test_exports_are_declared_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    for n in NAMES:
        assert n in gkc.SYMBOLS, n
        assert ("int %s(gkc_ctx* ctx" % n) in hdr, n
    for name in ("graph_links", "graph_rank", "graph_emit"):
        assert '"%s"' % name in hdr
    for meth in ("unitigs", "unitigs_device", "unitig_of_records"):
        assert callable(getattr(gkc.Counter, meth))


def test_statement_on_a_tiny_graph():
    """k = 3, the set {AAC, ACG} of tests/test_graph_cpu.py: AAC -> ACG is a link (one successor, one predecessor); the right end of ACG has one neighbour too, CGT,
    but that is ACG itself, so the unitig ends there: AACG"""
    from tests.util import str2int
    u = unitigs_np([str2int("AAC"), str2int("ACG")], [3, 4], 3)
    assert u["link"].tolist() == [2 * 1 + 1, NONE, NONE, 2 * 0 + 0]
    assert u["seqs"] == ["AACG"] and u["kc"].tolist() == [7] and u["offsets"].tolist() == [0, 4]
    assert u["unitig"].tolist() == [0, 0] and u["pos"].tolist() == [0, 1] and not u["reversed"].any() and u["n_cycles"] == 0


@pytest.mark.parametrize("name", ["k21_freq_4parts", "k21_defaults_parts"])
def test_statement_reproduces_the_reference_unitigs(name):
    k, values, ab, u = fixture_unitigs(name)
    assert k == 21 and u["n_cycles"] == 0
    assert canonical_digest(u["seqs"]) == reference_digest()
    assert len(u["bases"]) == 47975 and len(u["kc"]) == 711 and int(u["kc"].sum()) == sum(ab)


@pytest.mark.parametrize("name,n_unitigs,n_bases", [("k31_defaults", 90, 6320), ("k63_defaults", 28, 4588)])
def test_statement_regression_values(name, n_unitigs, n_bases):
    """the statement's own values for two more fixtures (no unitigs of the reference are recorded for them)"""
    k, values, ab, u = fixture_unitigs(name)
    assert (len(u["seqs"]), len(u["bases"]), u["n_cycles"]) == (n_unitigs, n_bases, 0)
    assert n_bases == len(values) + (k - 1) * n_unitigs


def check_properties(vals, k, u):
    link = u["link"]
    n = len(vals)
    for t in range(2 * n):                                      # the links are symmetric
        if link[t] != NONE:
            assert link[link[t]] == t and (link[t] >> 1) != (t >> 1)
    assert sorted(zip(u["unitig"].tolist(), u["pos"].tolist())) == [(a, b) for a in range(len(u["seqs"])) for b in range(len(u["seqs"][a]) - k + 1)]      # every record in exactly one place
    assert len(u["bases"]) == n + (k - 1) * len(u["seqs"])
    starts = [int(np.flatnonzero((u["unitig"] == a) & (u["pos"] == 0))[0]) for a in range(len(u["seqs"]))]
    assert starts == sorted(starts)
    from tests.util import str2int
    for a, s in enumerate(u["seqs"]):                           # the sequence spells its records, each in the orientation it was given
        members = np.flatnonzero(u["unitig"] == a)
        for r in members:
            w = str2int(s[u["pos"][r]: u["pos"][r] + k])
            assert w == (revcomp(vals[r], k) if u["reversed"][r] else vals[r])
        if len(members) == 1:
            assert not u["reversed"][members[0]]


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_fuzz_over_random_subsets(k):
    rng = np.random.default_rng(100 + k)
    every = sorted({min(x, revcomp(x, k)) for x in range(4 ** k)})
    for density in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9):
        vals = [x for x in every if rng.random() < density]
        u = unitigs_np(vals, rng.integers(1, 50, len(vals)).tolist(), k)
        check_properties(vals, k, u)


CYCLES = [(k, L) for k in (5, 7, 21) for L in (k + 3, 40, 200)]
# 200 of the 512 canonical 5-mers cannot be told apart from their neighbourhoods: every k-mer of such a circle has some of its six other neighbours on the circle (a
# depth-first search of 2.4 million steps finds no isolated cycle), so that circle is a graph with branching nodes and is checked as one
NOT_ISOLATED = {(5, 200)}


@functools.lru_cache(maxsize=None)
def circle(k, L):
    """-> (sequence, its canonical k-mers ascending = the flat order of one dataset)"""
    seq = circular_sequence(k, L, seed=1000 * k + L, isolated=(k, L) not in NOT_ISOLATED)
    return seq, circular_kmers(seq, k)


@pytest.mark.parametrize("k,L", CYCLES)
def test_a_circular_sequence_is_one_unitig_cut_at_its_smallest_record(k, L):
    seq, vals = circle(k, L)
    assert len(set(vals)) == L and all(v != revcomp(v, k) for v in vals)
    u = unitigs_np(vals, [1] * L, k)
    check_properties(vals, k, u)
    if (k, L) in NOT_ISOLATED:
        assert len(u["seqs"]) > 1 and (u["link"] == NONE).any()
        return
    assert (u["link"] != NONE).all() and u["n_cycles"] == 1 and len(u["seqs"]) == 1 and len(u["seqs"][0]) == L + k - 1
    assert u["pos"][0] == 0 and not u["reversed"][0] and sorted(u["pos"].tolist()) == list(range(L))
    assert u["seqs"][0][:k] == kmer_str(vals[0], k)
    # the unitig is the circle opened at record 0, read in that record's forward direction
    both = (seq + seq + seq[: k - 1]).encode()
    assert u["seqs"][0].encode() in both or u["seqs"][0].encode().translate(_COMP)[::-1] in both
