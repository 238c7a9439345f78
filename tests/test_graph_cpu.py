"""Graph neighbourhoods of the solid k-mers (include/gkc.h, "graph neighbourhoods"; csrc/gkc_graph.hip), the part that needs no GPU: the three exports are declared and
bound, and a plain numpy / Python statement of the masks, of "branching" and of the topology table — pinned by the reference's OWN /branching/nodes in the reference-run
fixtures, not by the code under test. tests/test_gpu_graph.py imports the statement."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_reference_run import DIR, load

NAMES = ["gkc_graph_neighbors_solid", "gkc_graph_neighbors_partition", "gkc_graph_branching_solid"]

# reverse-complement of a k-mer held as 16 little-endian bytes: every byte's four nucleotides reversed and complemented (A, C, T, G = 0..3: the complement is ^ 2), the
# bytes read backwards, the 64 - k unused nucleotides shifted out
_RC_BYTE = bytes((((b & 3) << 6) | ((b & 12) << 2) | ((b & 48) >> 2) | ((b & 192) >> 6)) ^ 0xAA for b in range(256))


def revcomp(x, k):
    return int.from_bytes(x.to_bytes(16, "little").translate(_RC_BYTE), "big") >> (2 * (64 - k))


def neighbours(x, k):
    """the eight neighbours of x taken as the forward strand, in the bit order of the mask: right extensions by A, C, T, G, then left extensions by A, C, T, G"""
    mask = (1 << (2 * k)) - 1
    return [((x << 2) | j) & mask for j in range(4)] + [(x >> 2) | (j << (2 * (k - 1))) for j in range(4)]


def graph_masks_np(values, k, solid=None):
    """values: the solid k-mers (canonical, Python ints or a uint64 array), any order -> uint8[n]: bit e set <=> the canonical form of neighbour e is one of them
    (or, with ``solid``, a member of that set instead)"""
    vals = [int(v) for v in values]
    solid = set(vals) if solid is None else set(solid)
    out = np.zeros(len(vals), np.uint8)
    for i, x in enumerate(vals):
        b = 0
        for e, n in enumerate(neighbours(x, k)):
            if min(n, revcomp(n, k)) in solid:
                b |= 1 << e
        out[i] = b
    return out


_POP4 = np.array([bin(i).count("1") for i in range(16)], np.uint8)


def degrees(masks):
    """-> (in, out) = solid predecessors / successors per k-mer"""
    masks = np.asarray(masks, np.uint8)
    return _POP4[masks >> 4], _POP4[masks & 15]


def branching_from_masks(masks):
    """bool[n]: not (exactly one predecessor and exactly one successor)"""
    i, o = degrees(masks)
    return ~((i == 1) & (o == 1))


def topology_from_masks(masks):
    i, o = degrees(masks)
    t = np.zeros((5, 5), np.uint64)
    np.add.at(t, (i.astype(np.intp), o.astype(np.intp)), 1)
    return t


def pack_branching(values, abundances, k):
    """ascending by value, {value little-endian 8 / 16 bytes, abundance u32}: the records of the reference's /branching/nodes"""
    nb = 8 if k <= 31 else 16
    return b"".join(int(v).to_bytes(nb, "little") + int(a).to_bytes(4, "little") for v, a in sorted(zip(values, abundances)))


def test_exports_are_declared_and_bound():
    gkc = ge.load().gkc
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    for n in NAMES:
        assert n in gkc.SYMBOLS, n
        assert ("int %s(gkc_ctx* ctx" % n) in hdr, n
    for meth in ("neighbor_masks", "neighbor_masks_partition", "branching_nodes", "graph_topology"):
        assert callable(getattr(gkc.Counter, meth))


def test_revcomp_statement():
    from tests.util import revcomp_int
    rng = np.random.default_rng(5)
    for k in (5, 21, 31, 32, 33, 63):
        for _ in range(50):
            x = int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * k)) - 1)
            assert revcomp(x, k) == revcomp_int(x, k)


def test_masks_statement_on_a_tiny_graph():
    """k = 3, the set {AAC, ACG}, worked by hand"""
    from tests.util import str2int
    k = 3
    vals = [str2int("AAC"), str2int("ACG")]
    assert all(v == min(v, revcomp(v, k)) for v in vals)          # both canonical (A < C < T < G)
    m = graph_masks_np(vals, k)
    # AAC: its right extension by G (bit 3) is ACG. Nothing else of the set: GTT = revcomp(AAC) is reached from AAC only by a step the forward strand does not take
    assert m[0] == 1 << 3
    # ACG: its left extension by A (bit 4) is AAC; its right extension by T (bit 2) is CGT, whose canonical form is ACG itself — a self-loop, no special case
    assert m[1] == (1 << 4) | (1 << 2)
    assert branching_from_masks(m).tolist() == [True, False]      # AAC has no predecessor; ACG has one of each
    t = topology_from_masks(m)
    assert int(t.sum()) == 2 and t[0, 1] == 1 and t[1, 1] == 1


@pytest.mark.parametrize("name,n_parts,n_solid,n_branching", [("k31_defaults", 1, 3620, 93), ("k63_defaults", 1, 2852, 51), ("k21_defaults_parts", 4, 33755, 661)])
def test_statement_reproduces_the_reference_branching_nodes(name, n_parts, n_solid, n_branching):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    assert nbpart == n_parts
    values = [v for p in parts for v, _ in p]; ab = [a for p in parts for _, a in p]
    assert len(values) == n_solid
    masks = graph_masks_np(values, k)
    br = branching_from_masks(masks)
    assert int(br.sum()) == n_branching
    got = pack_branching([v for v, b in zip(values, br) if b], [a for a, b in zip(ab, br) if b], k)
    assert got == bytes(z["branching_nodes"])
    t = topology_from_masks(masks)
    assert int(t.sum()) == n_solid and int(t.sum() - t[1, 1]) == n_branching
