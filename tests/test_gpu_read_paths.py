"""Read paths on the device (csrc/gkc_paths.hip and the third mode of k_q_reads: gkc_graph_reads_nodes_device / _segments_device; gkc.Counter.read_nodes, read_segments and
their _device forms). Expected values: the plain Python statement of tests/test_read_paths_cpu.py over the unitig SEQUENCES the device wrote (a dictionary of their
k-mers, pinned there on the reference's own unitigs), and, where the reads are the unitigs themselves, arithmetic on the offsets. Every comparison is exact.
Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import graph_inputs as gi
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_tips import counter_of_reads
from tests.test_gpu_unitigs import CASES, GENOME, N_READS, READ_LEN, SUB_PPM, case_id, fixture_counter, palindrome_reads
from tests.test_query_cpu import freq_order_of
from tests.test_read_paths_cpu import (ABSENT, MAPPED, NO_KMER, NONE64, REMOVED, SEGMENT, assert_consistent, fixture_paths, pack, random_sequence, rc_str, read_paths_np)
from tests.test_reference_run import DIR
from tests.test_simplify_cpu import K as K_SIMPLIFY, branches_of, bubble_reads
from tests.test_unitigs_cpu import fixture_unitigs, split_sequences
from tests.util import simple_repart

pytestmark = pytest.mark.gpu
QR_TILE = 4096
TILE_PASS = 2048 * QR_TILE                                      # positions in one pass of the reads kernel's grid
PASS = 2048 * 256                                               # elements in one pass of a thread-per-element grid (and positions in one pass of the word kernels)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def unitig_strings(bases, offs):
    return [s.decode() for s in split_sequences(bases, offs)]


def assert_nodes(got, exp):
    u, s, p, st = got
    assert u.dtype == np.uint64 and s.dtype == bool and p.dtype == np.uint32 and st.dtype == np.uint8
    bad = np.flatnonzero(st != exp["status"])
    assert len(st) == len(exp["status"]) and len(bad) == 0, (len(st), len(exp["status"]), bad[:10], st[bad[:10]], exp["status"][bad[:10]])
    assert np.array_equal(u, exp["unitig"]) and np.array_equal(s, exp["strand"]) and np.array_equal(p, exp["pos"])


def assert_segments(got, exp):
    so, seg, sup = got
    assert so.dtype == np.uint64 and seg.dtype == SEGMENT and sup.dtype == np.uint64
    assert np.array_equal(so, exp["seg_offsets"])
    assert len(seg) == len(exp["segments"]) and np.array_equal(seg, exp["segments"]), (len(seg), len(exp["segments"]))
    assert np.array_equal(sup, exp["support"])


def assert_equals_statement(c, bases, offs, seqs, k, solid, exp=None):
    """read_nodes and read_segments of the reads against the statement over the unitig strings; the status against query_reads -> the statement's result"""
    if exp is None:
        exp = read_paths_np(bases, offs, seqs, k, solid)
    assert_nodes(c.read_nodes(bases, offs), exp)
    assert_segments(c.read_segments(bases, offs), exp)
    ab = c.query_reads(bases, offs)
    st = exp["status"]
    assert np.array_equal(st == NO_KMER, ab == -1) and np.array_equal((st == MAPPED) | (st == REMOVED), ab > 0) and np.array_equal(st == ABSENT, ab == 0)
    return exp


def identity_expectation(offs, k, reverse=None):
    """the unitigs fed back as reads (offs: their offsets): position j < L_u of unitig u lies at (u, strand 0, j), the last k - 1 positions carry no k-mer, one segment
    per unitig; ``reverse``: bool[n_unitigs], the unitigs' reverse complements were fed instead and spell another string: strand 1, positions descending"""
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    nu = len(offs) - 1
    L = np.diff(offs) - (k - 1)
    n = int(offs[-1])
    rev = np.zeros(nu, bool) if reverse is None else reverse
    u_of = np.repeat(np.arange(nu), np.diff(offs))
    j = np.arange(n) - offs[:-1][u_of]
    mapped = j < L[u_of]
    pos = np.where(rev[u_of], L[u_of] - 1 - j, j)
    segments = np.zeros(nu, SEGMENT)
    segments["node"] = (np.arange(nu, dtype=np.uint64) << np.uint64(1)) | rev.astype(np.uint64)
    segments["unitig_pos"] = np.where(rev, L - 1, 0); segments["n_kmers"] = L
    return dict(unitig=np.where(mapped, u_of.astype(np.uint64), NONE64), strand=rev[u_of] & mapped, pos=np.where(mapped, pos, 0).astype(np.uint32),
                status=np.where(mapped, MAPPED, NO_KMER).astype(np.uint8), seg_offsets=np.arange(nu + 1, dtype=np.uint64), segments=segments, support=L.astype(np.uint64))


def reverse_complements(bases, offs):
    """-> (bases of the reverse complement of every unitig, bool[n]: it differs from the unitig — all but a palindrome that is a unitig of its own, at even k)"""
    seqs = split_sequences(bases, offs)
    rcs = [s.translate(_COMP)[::-1] for s in seqs]
    return np.frombuffer(b"".join(rcs), np.uint8).copy(), np.array([a != b for a, b in zip(seqs, rcs)], bool)


def assert_identity(c, k, bases, offs):
    """the unitigs and their reverse complements as reads; bases, offs: what the device wrote for the placement the context holds"""
    exp = identity_expectation(offs, k)
    assert_nodes(c.read_nodes(bases, offs), exp)
    assert_segments(c.read_segments(bases, offs), exp)
    rb, differs = reverse_complements(bases, offs)
    L = np.diff(offs.astype(np.int64)) - (k - 1)
    assert (L[~differs] == 1).all() and (k % 2 == 0 or differs.all())
    exp = identity_expectation(offs, k, differs)
    assert_nodes(c.read_nodes(rb, offs), exp)
    assert_segments(c.read_segments(rb, offs), exp)
    return differs


def device_call(c, bases, offs, room_segments=None, cap_segments=None, support=True, with_pos=True, canary=0xEE, misalign=(0, 0)):
    """the two exports over buffers pre-filled with ``canary`` and 64 bytes longer than needed -> dict(rc_nodes, rc_segments, n_segments, node, pos, seg_offsets,
    segments, support: the raw bytes). misalign: bytes added to (d_bases, d_node)"""
    import torch
    nb, nr = int(offs[-1]), len(offs) - 1
    tb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    if nb:
        tb[misalign[0]: misalign[0] + nb] = torch.from_numpy(np.ascontiguousarray(bases[:nb])).cuda()
    to = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64).copy()).cuda()
    node = torch.full((nb * 8 + 64,), canary, dtype=torch.uint8, device="cuda"); pos = torch.full((nb * 4 + 64,), canary, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = dict(rc_nodes=c.L.gkc_graph_reads_nodes_device(c.h, tb.data_ptr() + misalign[0], to.data_ptr(), nr, nb, node.data_ptr() + misalign[1], pos.data_ptr() if with_pos else None))
    out.update(node=node.cpu().numpy(), pos=pos.cpu().numpy())
    if out["rc_nodes"] != 0 or room_segments is None:
        return out
    so = torch.full(((nr + 1) * 8 + 64,), canary, dtype=torch.uint8, device="cuda"); seg = torch.full((room_segments * 24 + 64,), canary, dtype=torch.uint8, device="cuda")
    nu = c._placement_nu                                          # (set by unitigs_build / remove_tips / simplify: the segments part needs a placement built through c)
    sup = torch.full((nu * 8 + 64,), canary, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64(0xDEAD)
    out["rc_segments"] = c.L.gkc_graph_reads_segments_device(c.h, node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(),
                                                             room_segments if cap_segments is None else cap_segments, C.byref(n), sup.data_ptr() if support else None)
    out.update(n_segments=n.value, seg_offsets=so.cpu().numpy(), segments=seg.cpu().numpy(), support=sup.cpu().numpy())
    return out


# ------------------------------------------------------------------------------------------------ 1. the fixtures' own reads against the unitigs of their solid sets
@pytest.mark.parametrize("name", ["k21_freq_4parts", "k31_defaults", "k63_defaults"])
def test_the_fixture_reads_against_the_statement(gkc, name):
    c, k = fixture_counter(gkc, name)
    z = np.load(os.path.join(DIR, name + ".npz"))
    bases, offs, consumed = c.fastx_parse(bytes(z["fasta"]))
    assert consumed == len(z["fasta"])
    seqs = unitig_strings(*c.unitigs()[:2])
    _, values, _, u = fixture_unitigs(name)
    assert seqs == u["seqs"]
    exp = None
    if name == "k21_freq_4parts":                               # the statement over these reads and unitigs was computed for tests/test_read_paths_cpu.py
        _, fb, fo, fs, exp = fixture_paths(name)
        assert np.array_equal(fb, bases) and np.array_equal(fo, offs) and fs == seqs
    exp = assert_equals_statement(c, bases, offs, seqs, k, set(values), exp)
    counts = np.bincount(exp["status"], minlength=4)
    print("%s: %d positions: mapped, removed, absent, no k-mer = %s; %d segments" % (name, len(bases), counts.tolist(), len(exp["segments"])))
    assert counts[MAPPED] and counts[ABSENT] and counts[NO_KMER] and not counts[REMOVED]
    c.close()


# ------------------------------------------------------------------------------------------------ 2. the unitigs as reads: every record where the placement says
def case_counter(gkc, case):
    """the input of tests/test_gpu_unitigs.py::test_unitigs_against_the_statement"""
    k, m, parts, passes, order, (amin, amax) = case
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes() for i in range(N_READS)]
    if k == 5:
        reads = reads[:1]
    if k % 2 == 0:
        reads += palindrome_reads(np.random.default_rng(k), k)
    if k == 5 or k % 2 == 0:
        bases, offs = pack(reads)
    freq = freq_order_of(reads, m) if order == "freq" else None
    return counter_for(gkc, bases, offs, k, m, parts, passes, freq, amin, amax)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_unitigs_as_reads(gkc, case):
    k = case[0]
    c = case_counter(gkc, case)
    d_bases, d_offs, _ = c.unitigs_device()
    bases, offs = d_bases.cpu().numpy(), d_offs.cpu().numpy().view(np.uint64)
    nu, nb = len(offs) - 1, len(bases)
    assert nu > 0 and nb == int(offs[-1])
    # where they lie: the tensors unitigs_device returned are the arguments
    import torch
    node = torch.zeros(nb, dtype=torch.int64, device="cuda"); pos = torch.zeros(nb, dtype=torch.int32, device="cuda")
    so = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(nu * 24, dtype=torch.uint8, device="cuda"); sup = torch.zeros(nu, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.read_nodes_device(d_bases.data_ptr(), d_offs.data_ptr(), nu, nb, node.data_ptr(), pos.data_ptr())
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), d_offs.data_ptr(), nu, nb) == nu
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), d_offs.data_ptr(), nu, nb, so.data_ptr(), seg.data_ptr(), nu, sup.data_ptr()) == nu
    exp = identity_expectation(offs, k)
    v = node.cpu().numpy().view(np.uint64)
    want = np.where(exp["status"] == MAPPED, exp["unitig"] << np.uint64(1), np.uint64(gkc.NODE_NO_KMER))
    assert np.array_equal(v, want) and np.array_equal(pos.cpu().numpy().view(np.uint32), exp["pos"])
    assert_segments((so.cpu().numpy().view(np.uint64), seg.cpu().numpy().view(SEGMENT), sup.cpu().numpy().view(np.uint64)), exp)
    # through the host, and reverse-complemented
    differs = assert_identity(c, k, bases, offs)
    if k == 32:
        assert not differs.all()                                # the palindrome: a unitig of its own, strand 0 whichever way it is read
    c.close()


# ------------------------------------------------------------------------------------------------ 3. after simplify: removed k-mers, and the unitigs of what is left
@pytest.mark.parametrize("name", ["three_branches", "k21_freq_4parts"])
def test_reads_against_the_simplified_graph(gkc, name):
    if name == "three_branches":
        k = K_SIMPLIFY
        reads = bubble_reads(branches_of([k, k, k], [5, 2, 1], seed=7), seed=7)[0]
        c = counter_of_reads(gkc, reads, k=k)
        bases, offs = pack(reads)
    else:
        c, k = fixture_counter(gkc, name)
        z = np.load(os.path.join(DIR, name + ".npz"))
        bases, offs, _ = c.fastx_parse(bytes(z["fasta"]))
    vals, _, _ = solid_records(c)
    got = c.simplify()
    assert 0 < got["records_removed"] < len(vals)
    ub, uo = c.simplified_unitigs()[:2]
    exp = assert_equals_statement(c, bases, offs, unitig_strings(ub, uo), k, set(vals))
    counts = np.bincount(exp["status"], minlength=4)
    print("%s simplified: mapped, removed, absent, no k-mer = %s; %d segments" % (name, counts.tolist(), len(exp["segments"])))
    assert counts[MAPPED] and counts[REMOVED]
    ab = c.query_reads(bases, offs)
    assert (ab[exp["status"] == REMOVED] > 0).all()              # removed from the graph, still in the results
    assert_identity(c, k, ub, uo)
    c.close()


# ------------------------------------------------------------------------------------------------ 4. edges of the read buffer
K_EDGE, M_EDGE = 31, 8


@pytest.fixture(scope="module")
def edge_graph(gkc):
    """one error-free genome of 9000 bases counted as one read: a single path -> (counter, genome, unitig strings, solid set)"""
    genome = random_sequence(41, 9000)
    bases, offs = pack([genome])
    c = counter_for(gkc, bases, offs, K_EDGE, M_EDGE, 4)
    vals, _, _ = solid_records(c)
    seqs = unitig_strings(*c.unitigs()[:2])
    assert len(seqs) == 1 and len(vals) == 9000 - K_EDGE + 1
    yield c, genome, seqs, set(vals)
    c.close()


def substitute(s, at):
    return s[:at] + ("C" if s[at] != "C" else "G") + s[at + 1:]


def cut(s, borders):
    return [s[a:b] for a, b in zip([0] + borders, borders + [len(s)])]


def test_no_reads_at_all(gkc, edge_graph):
    c, genome, seqs, solid = edge_graph
    bases, offs = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    u, s, p, st = c.read_nodes(bases, offs)
    assert len(u) == len(s) == len(p) == len(st) == 0
    so, seg, sup = c.read_segments(bases, offs)
    assert so.tolist() == [0] and len(seg) == 0 and sup.tolist() == [0]
    got = device_call(c, bases, offs, room_segments=2)
    assert got["rc_nodes"] == 0 and got["rc_segments"] == 0 and got["n_segments"] == 0
    assert got["seg_offsets"][:8].view(np.uint64).tolist() == [0] and (got["seg_offsets"][8:] == 0xEE).all() and (got["segments"] == 0xEE).all() and (got["node"] == 0xEE).all()


EDGE_READS = {
    "empty_reads_between_others": lambda g: ["", g[:100], "", "", g[200:300], ""],
    "k_minus_1_and_k_bases": lambda g: [g[:K_EDGE - 1], g[50:50 + K_EDGE], g[100:100 + K_EDGE + 1]],
    "an_N_inside": lambda g: [g[:100] + "N" + g[101:200]],
    "lower_case": lambda g: [g[:150].lower(), rc_str(g[300:450]).lower()],
    # around QR_TILE = 4096; none of 4095, 4097, 8197 is a multiple of 16
    "4095_bases": lambda g: [g[:4095]],
    "4096_bases_a_read_of_one_base_at_the_last_position": lambda g: cut(g[:4096], [4095]),
    "4097_bases_substitution_on_the_border": lambda g: [substitute(g[:4097], 4096)],
    "4200_bases_a_read_starts_at_the_last_position_of_the_tile": lambda g: cut(g[:4200], [4095]),
    "8197_bases_one_segment_across_the_border_substitution_on_the_next": lambda g: cut(substitute(g[:8197], 8192), [4095]),
    "8197_bases_substitution_on_the_first_border": lambda g: [substitute(g[:8197], 4096)],
}


@pytest.mark.parametrize("shape", sorted(EDGE_READS))
def test_edges_of_the_read_buffer(gkc, edge_graph, shape):
    c, genome, seqs, solid = edge_graph
    k = K_EDGE
    bases, offs = pack(EDGE_READS[shape](genome))
    exp = assert_equals_statement(c, bases, offs, seqs, k, solid)
    assert_consistent(exp, offs)
    st, sg = exp["status"], exp["segments"]
    first = offs[:-1][np.diff(offs.astype(np.int64)) > 0]
    if shape == "empty_reads_between_others":
        assert exp["seg_offsets"].tolist() == [0, 0, 1, 1, 1, 2, 2]
    if shape == "k_minus_1_and_k_bases":
        assert (st == MAPPED).sum() == 0 + 1 + 2 and exp["seg_offsets"].tolist() == [0, 0, 1, 2] and sg["n_kmers"].tolist() == [1, 2]
    if shape == "an_N_inside":
        assert (st[100 - k + 1: 101] == NO_KMER).all() and (st[: 100 - k + 1] == MAPPED).all() and (st[101: 200 - k + 1] == MAPPED).all()      # exactly k windows are lost
        assert sg["read_pos"].tolist() == [0, 101]
    if shape == "lower_case":
        assert (st == MAPPED).sum() == 2 * (150 - k + 1) and len(sg) == 2 and int(sg["node"][0]) ^ int(sg["node"][1]) == 1
    if shape.startswith("4095"):
        assert len(bases) == QR_TILE - 1 and len(sg) == 1 and sg["n_kmers"][0] == 4095 - k + 1
    if shape.startswith("4096"):
        assert int(first[-1]) == QR_TILE - 1 and len(sg) == 1
    if shape.startswith("4097"):
        assert st[4097 - k] == ABSENT and st[4096 - k] == MAPPED and len(sg) == 1
    if shape.startswith("4200") or shape.startswith("8197_bases_one"):
        assert int(first[-1]) == QR_TILE - 1 and len(sg) == 2 and sg["read_pos"].tolist() == [0, 0]
        s = sg[1]
        assert QR_TILE - 1 + int(s["n_kmers"]) > QR_TILE + 1    # ONE segment from the last position of the first tile into the second
    if shape.startswith("8197_bases_one"):
        # (the windows over base 8192 that still fit into the read: the buffer ends five bases behind it)
        assert (st[8192 - k + 1: 8197 - k + 1] == ABSENT).all() and (st[8197 - k + 1:] == NO_KMER).all() and st[8192 - k] == MAPPED and sg["n_kmers"][1] == 8192 - k + 1 - 4095
    if shape.startswith("8197_bases_substitution"):
        assert (st[4096 - k + 1: 4097] == ABSENT).all() and sg["read_pos"].tolist() == [0, 4097] and sg["n_kmers"].tolist() == [4096 - k + 1, 8197 - k + 1 - 4097]


# ------------------------------------------------------------------------------------------------ 5. past one grid pass
def test_past_one_grid_pass(gkc):
    """The tile grid of the reads kernel strides above 2048 x 4096 = 8,388,608 positions, the word kernels of the segments above 524,288 positions, the thread-per-read
    kernels above 524,288 reads, and the one-workgroup scan carries above 256 x 1024 words = 16,777,216 positions. The graph: isolated paths of 1 to 3 records (the
    input of tests/test_gpu_graph_sizes.py), so reads are short and many; its unitigs as reads, nine times over, behind one read of N that puts a read start exactly
    on position 8,388,608. A read's last k - 1 positions carry no k-mer, so the last MAPPED position of the first pass is that of the read in front of the border, and
    the first position of the second pass is a mapped position of the next read: that is asserted."""
    import torch
    k = 31
    lens = gi.lengths_for(120000)
    b = gi.isolated_paths(lens, k, seed=5)
    rb, ro = b.pack()
    c = counter_for(gkc, rb, ro, k, 8, 7)
    d_bases, d_offs, _ = c.unitigs_device()
    offs1 = d_offs.cpu().numpy().view(np.uint64).astype(np.int64)
    nu, T = len(offs1) - 1, int(offs1[-1])
    assert nu == len(lens)
    reps = 9
    pad = TILE_PASS % T
    assert pad > 0 and nu * reps > PASS and pad + T * reps > 2 * TILE_PASS + 64 * 1024 and 2 * TILE_PASS == 256 * 1024 * 64
    tb = torch.cat([torch.full((pad,), ord("N"), dtype=torch.uint8, device="cuda"), d_bases.repeat(reps)])
    offs = np.concatenate([[0], pad + (np.arange(reps)[:, None] * T + offs1[None, :-1]).reshape(-1), [pad + T * reps]]).astype(np.uint64)
    nr, nb = len(offs) - 1, int(offs[-1])
    assert nr == 1 + nu * reps and nb == len(tb) and TILE_PASS in offs.tolist()
    to = torch.from_numpy(offs.view(np.int64)).cuda()
    node = torch.zeros(nb, dtype=torch.int64, device="cuda"); pos = torch.zeros(nb, dtype=torch.int32, device="cuda")
    so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(nu * reps * 24, dtype=torch.uint8, device="cuda"); sup = torch.zeros(nu, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.read_nodes_device(tb.data_ptr(), to.data_ptr(), nr, nb, node.data_ptr(), pos.data_ptr())
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb) == nu * reps
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), nu * reps, sup.data_ptr()) == nu * reps
    one = identity_expectation(offs1, k)
    want_node = np.where(one["status"] == MAPPED, one["unitig"] << np.uint64(1), np.uint64(gkc.NODE_NO_KMER))
    want_node = np.concatenate([np.full(pad, gkc.NODE_NO_KMER, np.uint64), np.tile(want_node, reps)])
    want_pos = np.concatenate([np.zeros(pad, np.uint32), np.tile(one["pos"], reps)])
    got_node = node.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_node, want_node) and np.array_equal(pos.cpu().numpy().view(np.uint32), want_pos)
    borders = list(range(PASS * (pad // PASS + 1), nb - 64, PASS))
    assert TILE_PASS in borders and 2 * TILE_PASS in borders
    for border in borders:                                      # mapped positions on both sides of every border behind the read of N
        assert (want_node[border - 64: border] < np.uint64(gkc.NODE_NO_KMER)).any() and (want_node[border: border + 64] < np.uint64(gkc.NODE_NO_KMER)).any()
    r = int(np.searchsorted(offs, TILE_PASS))                   # the read that starts on the border, the read in front of it
    assert offs[r] == TILE_PASS and want_node[TILE_PASS] >> np.uint64(1) == (r - 1) % nu
    last = int(np.flatnonzero(want_node[:TILE_PASS] < np.uint64(gkc.NODE_NO_KMER))[-1])
    assert int(offs[r - 1]) <= last == TILE_PASS - k and want_node[last] >> np.uint64(1) == (r - 2) % nu
    assert np.array_equal(so.cpu().numpy().view(np.uint64), np.concatenate([[0], np.arange(nu * reps + 1)]).astype(np.uint64))
    assert np.array_equal(seg.cpu().numpy().view(SEGMENT), np.tile(one["segments"], reps))
    assert np.array_equal(sup.cpu().numpy().view(np.uint64), one["support"] * np.uint64(reps))
    c.close()


# ------------------------------------------------------------------------------------------------ 6. errors and state
def test_errors_and_state(gkc):
    k, m, parts = 31, 8, 4
    genome = random_sequence(43, 3000)
    bases, offs = pack([genome])
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    reads = cut(substitute(genome[:1000], 500), [300, 300, 700])
    qb, qo = pack(reads)
    # before any build
    got = device_call(c, qb, qo)
    assert got["rc_nodes"] == 1 and b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h) and (got["node"] == 0xEE).all() and (got["pos"] == 0xEE).all()
    seqs = unitig_strings(*c.unitigs()[:2])
    vals, _, _ = solid_records(c)
    exp = read_paths_np(qb, qo, seqs, k, set(vals))
    ns, nb, nr = len(exp["segments"]), len(qb), len(qo) - 1
    assert ns == 4
    # exact room; nothing is written outside; both sizing forms
    got = device_call(c, qb, qo, room_segments=ns)
    assert got["rc_nodes"] == 0 and got["rc_segments"] == 0 and got["n_segments"] == ns
    assert (got["node"][nb * 8:] == 0xEE).all() and (got["pos"][nb * 4:] == 0xEE).all() and (got["seg_offsets"][(nr + 1) * 8:] == 0xEE).all()
    assert (got["segments"][ns * 24:] == 0xEE).all() and (got["support"][len(seqs) * 8:] == 0xEE).all()
    assert np.array_equal(got["segments"][: ns * 24].view(SEGMENT), exp["segments"]) and np.array_equal(got["seg_offsets"][: (nr + 1) * 8].view(np.uint64), exp["seg_offsets"])
    assert np.array_equal(got["support"][: len(seqs) * 8].view(np.uint64), exp["support"])
    # d_pos == NULL, d_support == NULL
    alone = device_call(c, qb, qo, with_pos=False)
    assert alone["rc_nodes"] == 0 and np.array_equal(alone["node"], got["node"]) and (alone["pos"] == 0xEE).all()
    nosup = device_call(c, qb, qo, room_segments=ns, support=False)
    assert nosup["rc_segments"] == 0 and np.array_equal(nosup["segments"], got["segments"]) and (nosup["support"] == 0xEE).all()
    # one segment too few: error 4, the count, nothing written
    small = device_call(c, qb, qo, room_segments=ns, cap_segments=ns - 1)
    assert small["rc_segments"] == 4 and small["n_segments"] == ns and b"segments" in c.L.gkc_last_error(c.h)
    assert (small["segments"] == 0xEE).all() and (small["seg_offsets"] == 0xEE).all() and (small["support"] == 0xEE).all()
    # misaligned d_bases, misaligned d_node
    for mis in ((4, 0), (0, 8)):
        bad = device_call(c, qb, qo, misalign=mis)
        assert bad["rc_nodes"] == 1 and b"aligned" in c.L.gkc_last_error(c.h) and (bad["node"] == 0xEE).all() and (bad["pos"] == 0xEE).all()
    # offsets that are no CSR table of the bases
    for wrong in (qo + np.uint64(1), qo[::-1].copy(), np.concatenate([qo[:-1], [qo[-1] + np.uint64(7)]]).astype(np.uint64)):
        o = wrong.copy(); o_last = int(qo[-1])
        import torch
        tb = torch.from_numpy(qb).cuda(); to = torch.from_numpy(o.view(np.int64).copy()).cuda()
        node = torch.full((nb * 8 + 64,), 0xEE, dtype=torch.uint8, device="cuda"); pos = torch.full((nb * 4 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert c.L.gkc_graph_reads_nodes_device(c.h, tb.data_ptr(), to.data_ptr(), nr, o_last, node.data_ptr(), pos.data_ptr()) == 1 and b"CSR" in c.L.gkc_last_error(c.h)
        assert (node.cpu().numpy() == 0xEE).all() and (pos.cpu().numpy() == 0xEE).all()
        so = torch.full(((nr + 1) * 8 + 64,), 0xEE, dtype=torch.uint8, device="cuda"); seg = torch.full((ns * 24 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        good_node = torch.from_numpy(got["node"].copy()).cuda(); good_pos = torch.from_numpy(got["pos"].copy()).cuda()
        torch.cuda.synchronize()
        n = C.c_uint64()
        assert c.L.gkc_graph_reads_segments_device(c.h, good_node.data_ptr(), good_pos.data_ptr(), to.data_ptr(), nr, o_last, so.data_ptr(), seg.data_ptr(), ns, C.byref(n), None) == 1
        assert b"CSR" in c.L.gkc_last_error(c.h) and (so.cpu().numpy() == 0xEE).all() and (seg.cpu().numpy() == 0xEE).all()
    # a recount: the placement of the first count must not answer
    c.begin_pass(0); c.push_reads(bases, offs); c.finish_pass()
    got = device_call(c, qb, qo)
    assert got["rc_nodes"] == 1 and (b"changed" in c.L.gkc_last_error(c.h) or b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h)) and (got["node"] == 0xEE).all()
    c.unitigs_build()
    assert_nodes(c.read_nodes(qb, qo), exp)
    c.close()


# ------------------------------------------------------------------------------------------------ 7. timers
def test_timers(gkc):
    k, m, parts = 31, 8, 4
    genome = random_sequence(44, 2000)
    bases, offs = pack([genome])
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    c.unitigs_build()
    c.query_reads(bases, offs)
    before = {n: c.timing(n)[1] for n in ("graph_read_nodes", "graph_read_segments", "query_reads")}
    c.read_nodes(bases, offs)
    assert c.timing("graph_read_nodes")[1] == before["graph_read_nodes"] + 1 and c.timing("graph_read_segments")[1] == before["graph_read_segments"]
    c.read_segments(bases, offs)                                # the nodes call, the sizing call, the fill
    assert c.timing("graph_read_nodes")[1] == before["graph_read_nodes"] + 2 and c.timing("graph_read_segments")[1] == before["graph_read_segments"] + 2
    assert c.timing("query_reads")[1] == before["query_reads"]
    c.close()
