"""Unitigs of the solid k-mers on the device (csrc/gkc_unitigs.hip: gkc_graph_unitigs_build / _write / _nodes; gkc.Counter.unitigs, unitigs_device, unitig_of_records).
Expected values: the reference's own unitigs of one input (tests/golden/reference_run/k21_freq_4parts_unitigs.json) and the plain Python statement of the definition in
tests/test_unitigs_cpu.py (pinned there by that fixture), which walks the links record by record where the device ranks them by pointer jumping. Every comparison is
exact. Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_graph_cpu import graph_masks_np, neighbours, revcomp
from tests.test_query_cpu import INF, freq_order_of
from tests.test_reference_run import DIR, load
from tests.test_reference_run import freq_order_of as fixture_freq_order
from tests.test_unitigs_cpu import (CYCLES, NONE, NOT_ISOLATED, canonical_digest, circle, fixture_unitigs, kmer_str, reference_digest, split_sequences, unitigs_np)
from tests.util import simple_repart

pytestmark = pytest.mark.gpu
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def pack(reads):
    """reads: ASCII strings / bytes -> (bases uint8[], offsets uint64[n + 1])"""
    rs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offs = np.zeros(len(rs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rs], dtype=np.uint64)
    return np.frombuffer(b"".join(rs), np.uint8).copy(), offs


def random_sequence(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, n))


def rc_str(s):
    return s.encode().translate(_COMP)[::-1].decode()


def assert_equals_statement(c, k, exp=None):
    """the device's unitigs of the results c holds against the statement over the same records: bases, offsets, KC and the placement of every record, byte for byte
    -> (the statement's result, n_cycles the device reported)"""
    if exp is None:
        vals, abund, _ = solid_records(c)
        exp = unitigs_np(vals, abund, k)
    nu, nb, nc = c.unitigs_build()
    assert (nu, nb, nc) == (len(exp["seqs"]), len(exp["bases"]), exp["n_cycles"])
    bases, offs, kc = c.unitigs()
    assert bases.dtype == np.uint8 and offs.dtype == np.uint64 and kc.dtype == np.uint64
    assert np.array_equal(offs, exp["offsets"])
    bad = np.flatnonzero(bases != exp["bases"]) if len(bases) == len(exp["bases"]) else None
    assert bad is not None and len(bad) == 0, (len(bases), len(exp["bases"]), None if bad is None else bad[:10])
    assert np.array_equal(kc, exp["kc"])
    u, rev, pos = c.unitig_of_records()
    assert np.array_equal(u.astype(np.int64), exp["unitig"]) and np.array_equal(rev, exp["reversed"]) and np.array_equal(pos.astype(np.int64), exp["pos"])
    return exp, nc


# ------------------------------------------------------------------------------------------------ 1. the reference's own unitigs, and two more fixtures
def fixture_counter(gkc, name):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    c = gkc.Counter(0); c.set_solidity(2, INF, 10000); c.configure(k, m, nbpart, table, freq_order=fixture_freq_order(z, m))
    c.begin_pass(0)
    assert c.push_fastx(bytes(z["fasta"])) == len(z["fasta"])
    c.finish_pass()
    assert c.stats()["kmers_nb_solid"] == int(z["nb_solid_kmers"])
    return c, k


def test_unitigs_equal_the_reference_run(gkc):
    c, k = fixture_counter(gkc, "k21_freq_4parts")
    bases, offs, kc = c.unitigs()
    got = canonical_digest(split_sequences(bases, offs))
    print("k21_freq_4parts: %d unitigs, %d bases" % (got[0], got[1]))
    assert got == reference_digest()
    _, values, ab, exp = fixture_unitigs("k21_freq_4parts")
    assert_equals_statement(c, k, exp)
    assert int(kc.sum()) == sum(ab)
    c.close()


@pytest.mark.parametrize("name", ["k31_defaults", "k63_defaults"])
def test_unitigs_equal_the_statement_on_the_fixtures(gkc, name):
    c, k = fixture_counter(gkc, name)
    _, values, ab, exp = fixture_unitigs(name)
    vals, abund, _ = solid_records(c)
    assert vals == values and abund == ab
    assert_equals_statement(c, k, exp)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. small synthetic inputs against the statement
CASES = [
    # k, m, partitions, passes, order, abundance window
    (5, 3, 3, 1, "lexi", (1, INF)),            # one read only: a dense graph, few and short unitigs, self-loops
    (21, 7, 7, 1, "lexi", (1, INF)),
    (31, 8, 7, 1, "lexi", (1, INF)),
    (32, 8, 7, 1, "lexi", (1, INF)),           # 16-byte keys; even k: a palindrome with one neighbour on either side
    (33, 8, 7, 1, "lexi", (1, INF)),
    (63, 10, 7, 1, "lexi", (1, INF)),
    (21, 6, 7, 1, "freq", (1, INF)),           # frequency-order minimizers
    (31, 8, 1, 1, "lexi", (1, INF)),
    (31, 8, 4, 1, "lexi", (1, INF)),
    (31, 8, 512, 1, "lexi", (1, INF)),         # empty datasets: a neighbour's record index counts across them
    (31, 8, 7, 2, "lexi", (1, INF)),           # links into the other passes' datasets
    (33, 8, 5, 3, "lexi", (1, INF)),
    (31, 8, 7, 1, "lexi", (2, INF)),           # a neighbour counted outside the window is no neighbour
]
N_READS, READ_LEN, GENOME, SUB_PPM = 1000, 100, 3000, 5000


def case_id(c):
    return "k%d-m%d-P%d-p%d-%s-a%d" % (c[0], c[1], c[2], c[3], c[4], c[5][0])


def palindrome_reads(rng, k):
    """two copies of flank + (a reverse-complement palindrome of k bases) + flank: at even k a record that is its own reverse complement, with one neighbour on either side"""
    half = random_sequence(rng, k // 2)
    r = random_sequence(rng, 40) + half + rc_str(half) + random_sequence(rng, 40)
    return [r, r]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_unitigs_against_the_statement(gkc, case):
    k, m, parts, passes, order, (amin, amax) = case
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes() for i in range(N_READS)]
    if k == 5:
        reads = reads[:1]                                       # a fifth of the 5-mers: with all of them present nothing links
    if k % 2 == 0:
        reads += palindrome_reads(np.random.default_rng(k), k)
    if k == 5 or k % 2 == 0:
        bases, offs = pack(reads)
    freq = freq_order_of(reads, m) if order == "freq" else None
    c = counter_for(gkc, bases, offs, k, m, parts, passes, freq, amin, amax)
    vals, abund, sizes = solid_records(c)
    assert len(vals) == c.stats()["kmers_nb_solid"] > 0
    exp, _ = assert_equals_statement(c, k)
    lens = np.diff(exp["offsets"].astype(np.int64)) - (k - 1)
    print("%s: %d solid k-mers in %d datasets (%d empty) -> %d unitigs, longest %d records, %d reversed records" % (case_id(case), len(vals), len(sizes), sizes.count(0), len(lens), lens.max(), exp["reversed"].sum()))
    assert lens.max() > 1 and exp["reversed"].any() and not exp["reversed"].all()
    if k >= 21 and amin == 1:
        assert (lens == 1).any()
    if parts == 512:
        assert 0 in sizes
    if k % 2 == 0:
        pal = [i for i, v in enumerate(vals) if v == revcomp(v, k)]
        masks = graph_masks_np(vals, k)
        assert pal and all(masks[i] != 0 for i in pal) and all(lens[exp["unitig"][i]] == 1 for i in pal)      # it has neighbours and stands alone
    if (amin, amax) != (1, INF):
        full = counter_for(gkc, bases, offs, k, m, parts, passes, freq)
        every, every_ab, _ = solid_records(full); full.close()
        assert len(every) > len(vals)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. cycles
def circle_read(seq, k):
    return seq + seq[: k - 1]                                   # every k-mer of the circle once


@pytest.mark.parametrize("k,L", CYCLES)
def test_a_circle_alone(gkc, k, L):
    seq, want = circle(k, L)
    bases, offs = pack([circle_read(seq, k)])
    m = 3 if k == 5 else (4 if k == 7 else 7)
    c = counter_for(gkc, bases, offs, k, m, 4)
    vals, abund, _ = solid_records(c)
    assert sorted(vals) == want and set(abund) == {1}
    exp, nc = assert_equals_statement(c, k)
    if (k, L) not in NOT_ISOLATED:
        assert nc == 1 and len(exp["seqs"]) == 1
        u, rev, pos = c.unitig_of_records()
        first = int(np.flatnonzero(pos == 0)[0])
        assert first == 0 and not rev[0]                        # cut at the left end of the smallest record, which stands forward
        b1 = c.unitigs()
        b2 = c.unitigs()                                        # a second build gives identical output
        assert all(np.array_equal(x, y) for x, y in zip(b1, b2))
        assert bytes(b1[0][:k]).decode() == kmer_str(vals[0], k)
    c.close()


def test_circles_mixed_with_ordinary_reads(gkc):
    k, m, parts = 21, 7, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    reads = [bases[i * READ_LEN:(i + 1) * READ_LEN].tobytes().decode() for i in range(N_READS)]
    reads += [circle_read(circle(k, L)[0], k) for L in (k + 3, 40, 200)]
    bases, offs = pack(reads)
    for passes in (1, 2):
        c = counter_for(gkc, bases, offs, k, m, parts, passes)
        exp, nc = assert_equals_statement(c, k)
        assert nc == 3
        u, rev, pos = c.unitig_of_records()
        lens = np.diff(exp["offsets"].astype(np.int64)) - (k - 1)
        for L in (k + 3, 40, 200):                              # each circle is one unitig that starts, forward, at its smallest record
            want = set(circle(k, L)[1])
            vals, _, _ = solid_records(c)
            idx = [i for i, v in enumerate(vals) if v in want]
            assert len(idx) == L and len(set(u[idx].tolist())) == 1 and lens[int(u[idx[0]])] == L
            assert pos[min(idx)] == 0 and not rev[min(idx)]
        first = c.unitigs()
        again = c.unitigs()
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        c.close()


# ------------------------------------------------------------------------------------------------ 4. shapes where the ranking can go wrong
def one_path(gkc, n_records, k, m, seed, parts=4):
    """one error-free read over a random sequence: a path of n_records records -> the read; checked against the statement and against the read itself"""
    read = random_sequence(np.random.default_rng(seed), n_records + k - 1)
    bases, offs = pack([read])
    c = counter_for(gkc, bases, offs, k, m, parts)
    vals, _, _ = solid_records(c)
    assert len(vals) == n_records
    exp, nc = assert_equals_statement(c, k)
    assert nc == 0 and len(exp["seqs"]) == 1 and exp["seqs"][0] in (read, rc_str(read))
    c.close()
    return exp


def test_a_single_record_and_two_linked_records(gkc):
    exp = one_path(gkc, 1, 21, 7, 1)
    assert exp["pos"].tolist() == [0] and not exp["reversed"][0]
    exp = one_path(gkc, 2, 21, 7, 2)
    assert sorted(exp["pos"].tolist()) == [0, 1] and (exp["link"] != NONE).sum() == 2


@pytest.mark.parametrize("r", range(1, 11))
def test_paths_of_a_power_of_two_records(gkc, r):
    for n in (2 ** r - 1, 2 ** r, 2 ** r + 1):
        exp = one_path(gkc, n, 31, 8, 100 * r + n)
        assert sorted(exp["pos"].tolist()) == list(range(n))


def test_a_path_longer_than_a_tile_has_rounds(gkc):
    exp = one_path(gkc, 5000, 31, 8, 7, parts=7)
    assert 5000 % 1024 != 0 and sorted(exp["pos"].tolist()) == list(range(5000))


def test_a_hairpin(gkc):
    """x = a + P with P a reverse-complement palindrome of k - 1 bases: the right extension of x by comp(a) is revcomp(x), the record's only right neighbour is itself"""
    k, m = 21, 7
    rng = np.random.default_rng(3)
    half = random_sequence(rng, (k - 1) // 2)
    lead = random_sequence(rng, 30)
    read = lead + "A" + half + rc_str(half) + "T"
    bases, offs = pack([read])
    c = counter_for(gkc, bases, offs, k, m, 4)
    vals, abund, _ = solid_records(c)
    self_nb = [i for i, v in enumerate(vals) if any(min(nn, revcomp(nn, k)) == v for nn in neighbours(v, k))]
    assert len(self_nb) == 1 and abund[self_nb[0]] == 2         # the hairpin k-mer was seen on both strands
    exp, nc = assert_equals_statement(c, k)
    assert nc == 0 and len(exp["seqs"]) == 1 and len(exp["seqs"][0]) == len(read) - 1
    i = self_nb[0]
    assert (exp["link"][2 * i: 2 * i + 2] == NONE).sum() == 1   # one end of it is linked into the path, the other one meets itself and ends the unitig
    c.close()


# ------------------------------------------------------------------------------------------------ 5. closure: the unitigs hold exactly the solid k-mers, each once
@pytest.mark.parametrize("k,m", [(31, 8), (63, 10)])
def test_the_unitigs_counted_again_give_the_solid_set(gkc, k, m):
    import torch
    parts = 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts, amin=2)
    vals, _, _ = solid_records(c)
    d_bases, d_offs, d_kc = c.unitigs_device()
    assert d_bases.is_cuda and d_bases.dtype == torch.uint8 and d_offs.dtype == torch.int64 and len(d_kc) == len(d_offs) - 1
    c2 = gkc.Counter(0); c2.configure(k, m, parts, simple_repart(m, parts))
    c2.begin_pass(0)
    c2.push_reads_device(d_bases.data_ptr(), d_offs.data_ptr(), len(d_offs) - 1, len(d_bases))
    c2.finish_pass()
    vals2, abund2, _ = solid_records(c2)
    assert sorted(vals2) == sorted(vals) and set(abund2) == {1}
    c.close(); c2.close()


# ------------------------------------------------------------------------------------------------ 6. interface
def write_raw(c, cap_bases, cap_unitigs, room_bases, room_unitigs, kc=True):
    """gkc_graph_unitigs_write into buffers pre-filled with 0xEE -> (rc, bases uint8[room_bases], offsets bytes, kc bytes)"""
    import torch
    tb = torch.full((max(16, room_bases),), 0xEE, dtype=torch.uint8, device="cuda")
    to = torch.full(((room_unitigs + 1) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    tk = torch.full((max(1, room_unitigs) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = c.L.gkc_graph_unitigs_write(c.h, tb.data_ptr(), cap_bases, to.data_ptr(), cap_unitigs, tk.data_ptr() if kc else None)
    return rc, tb.cpu().numpy()[:room_bases], to.cpu().numpy(), tk.cpu().numpy()[: room_unitigs * 8]


def test_masks_given_or_computed_and_capacities(gkc):
    import torch
    k, m, parts = 31, 8, 7
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = counter_for(gkc, bases, offs, k, m, parts)
    vals, abund, _ = solid_records(c)
    exp = unitigs_np(vals, abund, k)
    nu, nb = len(exp["seqs"]), len(exp["bases"])
    # the masks where they lie, at an unaligned address
    t = torch.zeros(len(vals) + 9, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    assert c.neighbor_masks(d_out=t.data_ptr() + 1) == len(vals)
    assert c.unitigs_build(d_masks=t.data_ptr() + 1) == (nu, nb, 0)
    given = c.unitigs(d_masks=t.data_ptr() + 1)
    computed = c.unitigs()
    assert all(np.array_equal(x, y) for x, y in zip(given, computed))
    assert np.array_equal(given[0], exp["bases"]) and np.array_equal(given[1], exp["offsets"]) and np.array_equal(given[2], exp["kc"])
    # exact room, with and without KC; nothing beyond n_bases / n_unitigs + 1 / n_unitigs is touched
    rc, b, o, kc = write_raw(c, nb, nu, nb + 5, nu + 2)
    assert rc == 0 and np.array_equal(b[:nb], exp["bases"]) and (b[nb:] == 0xEE).all()
    assert np.array_equal(o[: (nu + 1) * 8].view(np.uint64), exp["offsets"]) and (o[(nu + 1) * 8:] == 0xEE).all()
    assert np.array_equal(kc[: nu * 8].view(np.uint64), exp["kc"]) and (kc[nu * 8:] == 0xEE).all()
    rc, b, o, kc = write_raw(c, nb, nu, nb, nu, kc=False)
    assert rc == 0 and np.array_equal(b, exp["bases"]) and (kc == 0xEE).all()
    # one base / one unitig too few
    for cap_b, cap_u in ((nb - 1, nu), (nb, nu - 1), (0, 0)):
        rc, b, o, kc = write_raw(c, cap_b, cap_u, nb + 5, nu + 2)
        assert rc == 4 and b"unitigs" in c.L.gkc_last_error(c.h)
        assert (b == 0xEE).all() and (o == 0xEE).all() and (kc == 0xEE).all()
    c.close()


def test_state_errors_recount_and_empty_results(gkc):
    k, m, parts = 31, 8, 8
    bases, offs = gkc.synth_reads_np(11, N_READS, READ_LEN, GENOME, SUB_PPM)
    c = gkc.Counter(0)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*gkc_configure"):
        c.unitigs_build()
    c.configure(k, m, parts, simple_repart(m, parts))
    c.begin_pass(0); c.push_reads(bases, offs)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*still open"):
        c.unitigs()
    c.finish_pass()
    # before a build
    rc, _, _, _ = write_raw(c, 1 << 20, 1 << 10, 16, 1)
    assert rc == 1 and b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*gkc_graph_unitigs_build"):
        c.unitig_of_records()
    first, _ = assert_equals_statement(c, k)
    # a recount with another abundance-min: the placement of the first count must not answer
    c.set_solidity(3, INF)
    c.count(bases, offs)
    rc, _, _, _ = write_raw(c, 1 << 22, 1 << 16, 16, 1)
    assert rc == 1 and b"changed" in c.L.gkc_last_error(c.h)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*(changed|gkc_graph_unitigs_build)"):
        c.unitig_of_records()
    second, _ = assert_equals_statement(c, k)
    assert len(second["seqs"]) != len(first["seqs"])
    # a count without any solid k-mer
    c.set_solidity(1000000, INF)
    c.count(bases, offs)
    assert c.stats()["kmers_nb_solid"] == 0
    assert c.unitigs_build() == (0, 0, 0)
    b, o, kc = c.unitigs()
    assert b.shape == (0,) and o.tolist() == [0] and kc.shape == (0,)
    u, rev, pos = c.unitig_of_records()
    assert len(u) == len(rev) == len(pos) == 0
    # a released pass
    c.set_solidity(1, INF)
    c.count(bases, offs)
    assert_equals_statement(c, k)
    c.release_pass(0)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*released"):
        c.unitigs()
    c.close()
