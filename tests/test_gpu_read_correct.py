"""Correction of the reads on the device (csrc/gkc_correct.hip: k_correct_copy, k_correct_unitig_offsets, k_correct_check, k_correct_apply;
gkc_graph_reads_correct_device; gkc.Counter.correct_reads, correct_reads_device). Expected values: the plain Python statement of tests/test_read_correct_cpu.py (pinned
there on the reference-run fixtures) over the unitig strings the device wrote, and, past the sizes a Python loop serves, np.tile of that statement over a tiled input.
Every comparison is exact. Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.test_gpu_graph import counter_for, solid_records
from tests.test_gpu_read_paths import unitig_strings
from tests.test_gpu_read_walks import forked_bubble_reads, upload
from tests.test_gpu_tips import counter_of_reads
from tests.test_read_correct_cpu import PINNED, STATS, correct_reads_np, fixture_corrected, ground_truth, stats_tuple, substitute
from tests.test_read_paths_cpu import SEGMENT, fixture_paths, pack, rc_str, read_paths_np
from tests.test_reference_run import DIR, load
from tests.test_reference_run import freq_order_of as fixture_freq_order
from tests.test_simplify_cpu import K as K_SIMPLIFY
from tests.test_unitigs_cpu import fixture_unitigs
from tests.util import simple_repart

pytestmark = pytest.mark.gpu
VEC = 16                                                        # bytes a lane of the copy moves per trip
WORD = 64                                                       # positions per word of d_changed_bits
WAVE = 64                                                       # reads per wave of the per-read kernels (check, apply): one lane per read
PASS = 2048 * 256                                               # reads in one pass of the per-read kernels' grid (q_grid: 2048 workgroups of 256 lanes)
COPY_PASS = PASS * VEC                                          # bytes in one pass of the copy's grid
K_GT, M_GT = 21, 8
INF = 2147483647
CANARY = 0xEE


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def counter_of_fixture(gkc, name):
    z, k, m, nbpart, table, parts = load(os.path.join(DIR, name + ".npz"))
    freq = fixture_freq_order(z, m)
    if name == "k21_freq":                                      # one partition, no stored order: any valid frequency order gives the same dataset
        freq = np.arange(4 ** m, dtype=np.uint32)
    c = gkc.Counter(0); c.set_solidity(2, INF, 10000); c.configure(k, m, nbpart, table, freq_order=freq)
    c.begin_pass(0)
    assert c.push_fastx(bytes(z["fasta"])) == len(z["fasta"])
    c.finish_pass()
    assert c.stats()["kmers_nb_solid"] == int(z["nb_solid_kmers"])
    return c, k


def device_inputs(c, bases, offs):
    """the reads, their segments and the unitig strings of the placement c built last, all left on the device -> dict: tb (uint8, exactly n_bases or 16), to, nr, nb,
    so, seg (bytes), ns, ub, uo"""
    import torch
    tb, to, nr, nb = c._reads_to_device(bases, offs)
    node = torch.zeros(max(nb, 2), dtype=torch.int64, device="cuda"); pos = torch.zeros(max(nb, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.read_nodes_device(tb.data_ptr(), to.data_ptr(), nr, nb, node.data_ptr(), pos.data_ptr())
    ns = c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb)
    so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(max(ns, 1) * 24, dtype=torch.uint8, device="cuda")
    nu, nub = c._placement_nu, c._placement_nb
    ub = torch.zeros(max(nub, 16), dtype=torch.uint8, device="cuda"); uo = torch.zeros(nu + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert c.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns) == ns
    assert c.L.gkc_graph_unitigs_write(c.h, ub.data_ptr(), nub, uo.data_ptr(), nu, None) == 0
    return dict(tb=tb, to=to, nr=nr, nb=nb, so=so, seg=seg[: ns * 24] if ns else seg, ns=ns, ub=ub, uo=uo)


def correct_raw(c, D, params=(2, 1), in_place=False, n_changed=True, bits=True, stats=True, out_shift=None, **over):
    """the export over buffers pre-filled with CANARY and 64 bytes longer than needed -> dict(rc, out, n_changed, bits: the raw bytes, stats: a tuple or None).
    params: (max_subst, ends) or None for NULL; in_place: d_out == d_bases (a copy of the reads with canary bytes behind it serves as both); out_shift: d_out =
    d_bases + out_shift inside one buffer; over: entries of D replaced for this call"""
    import torch
    D = dict(D, **over)
    nr, nb, ns = D["nr"], D["nb"], D["ns"]
    out, nch, bt = (torch.full((n + 64,), CANARY, dtype=torch.uint8, device="cuda") for n in (nb if out_shift is None else 2 * nb + 64, nr * 4, (nb + 63) // 64 * 8))
    d_bases = D["tb"].data_ptr()
    if in_place or out_shift is not None:
        out[:nb] = D["tb"][:nb]
        d_bases = out.data_ptr()
    torch.cuda.synchronize()
    prm = None if params is None else ge.load().gkc.CorrectParams(params[0], params[1])
    st = ge.load().gkc.CorrectStats(*([0xDEAD] * 7))
    rc = c.L.gkc_graph_reads_correct_device(c.h, d_bases, D["to"].data_ptr(), nr, nb, D["so"].data_ptr(), D["seg"].data_ptr(), ns, D["ub"].data_ptr(), D["uo"].data_ptr(),
                                            None if prm is None else C.byref(prm), out.data_ptr() + (out_shift or 0), nch.data_ptr() if n_changed else None,
                                            bt.data_ptr() if bits else None, C.byref(st) if stats else None)
    return dict(rc=rc, out=out.cpu().numpy(), n_changed=nch.cpu().numpy(), bits=bt.cpu().numpy(), stats=tuple(int(getattr(st, n)) for n in STATS), nb=nb,
                input=D["tb"][:nb].cpu().numpy())


def untouched(res, in_place=False):
    """no output written: the canaries everywhere, the reads themselves where the output is the input, the stats as they were"""
    nb = res["nb"]
    body = np.array_equal(res["out"][:nb], res["input"]) and (res["out"][nb:] == CANARY).all() if in_place else (res["out"] == CANARY).all()
    return body and (res["n_changed"] == CANARY).all() and (res["bits"] == CANARY).all() and res["stats"] == (0xDEAD,) * 7


def bits_of(changed):
    return np.packbits(np.concatenate([changed, np.zeros(-len(changed) % 64, bool)]), bitorder="little")


def assert_raw(res, exp, D):
    """a call that wrote everything: the results, and the canary bytes behind every buffer"""
    nr, nb = D["nr"], D["nb"]
    assert res["rc"] == 0 and res["stats"] == stats_tuple(exp["stats"])
    bad = np.flatnonzero(res["out"][:nb] != exp["bases"])
    assert len(bad) == 0, (len(bad), bad[:10])
    assert (res["out"][nb:] == CANARY).all()
    assert np.array_equal(res["n_changed"][: nr * 4].view(np.uint32), exp["n_changed"]) and (res["n_changed"][nr * 4:] == CANARY).all()
    nw = (nb + 63) // 64 * 8
    assert np.array_equal(res["bits"][:nw], bits_of(exp["changed"])) and (res["bits"][nw:] == CANARY).all()


def assert_corrected(got, exp, paths):
    """what Counter.correct_reads returned against the statement"""
    assert sorted(got) == ["bases", "changed", "n_changed", "seg_offsets", "segments", "stats"]
    assert got["bases"].dtype == np.uint8 and got["n_changed"].dtype == np.uint32 and got["changed"].dtype == bool and got["segments"].dtype == SEGMENT
    assert np.array_equal(got["seg_offsets"], paths["seg_offsets"]) and np.array_equal(got["segments"], paths["segments"])
    assert got["stats"] == {n: int(exp["stats"][n]) for n in STATS}
    assert np.array_equal(got["bases"], exp["bases"]) and np.array_equal(got["n_changed"], exp["n_changed"]) and np.array_equal(got["changed"], exp["changed"])


# ------------------------------------------------------------------------------------------------ 1. the fixtures' own reads: 8-byte and 16-byte keys
@pytest.mark.parametrize("name", ["k21_freq_4parts", "k31_defaults", "k63_defaults", "k21_freq"])
def test_the_fixture_reads_against_the_statement(gkc, name):
    c, k = counter_of_fixture(gkc, name)
    _, bases, offs, fseqs, paths = fixture_paths(name)
    c.unitigs_build()
    D = device_inputs(c, bases, offs)
    seqs = unitig_strings(D["ub"][: c._placement_nb].cpu().numpy(), D["uo"].cpu().numpy().view(np.uint64))
    if seqs != fseqs:                                           # (the device numbers the unitigs by its own record order)
        _, values, _, _ = fixture_unitigs(name)
        paths = read_paths_np(bases, offs, seqs, k, set(values))
    for max_subst in (2, 1):
        for ends in (1, 0):
            exp = fixture_corrected(name, max_subst, ends)[5] if seqs == fseqs else correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, k, max_subst, ends)
            if ends and (name, max_subst) in PINNED:
                assert stats_tuple(exp["stats"]) == PINNED[name, max_subst]
            assert_raw(correct_raw(c, D, (max_subst, ends)), exp, D)
            print("%s, max_subst %d, ends %d: %s" % (name, max_subst, ends, stats_tuple(exp["stats"])))
    exp = fixture_corrected(name)[5] if seqs == fseqs else correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, k)
    assert_corrected(c.correct_reads(bases, offs), exp, paths)
    assert_raw(correct_raw(c, D, (2, 1), in_place=True), exp, D)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. the simplified placement
def test_correction_on_the_simplified_graph(gkc):
    k = K_SIMPLIFY
    reads, asked = forked_bubble_reads(k)
    c = counter_of_reads(gkc, reads, k=k)
    bases, offs = pack(asked)
    vals, _, _ = solid_records(c)
    got = c.simplify()
    assert 0 < got["records_removed"] < len(vals)
    ub, uo, _, _, _ = c.simplified_unitigs()
    seqs = unitig_strings(ub, uo)
    paths = read_paths_np(bases, offs, seqs, k, set(vals))
    seen = []
    for max_subst in (2, 1000):
        exp = correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, k, max_subst, 1)
        assert_corrected(c.correct_reads(bases, offs, max_subst=max_subst), exp, paths)
        seen.append(exp["stats"])
        print("three_branches simplified, max_subst %d: %s" % (max_subst, stats_tuple(exp["stats"])))
    # the read through the removed same-length bulge, both ways: a collinear gap, evaluated at either limit and rewritten to the branch that stayed at the loose one
    assert seen[0]["gaps_fixed"] + seen[0]["gaps_skipped"] >= 2 and seen[1]["gaps_skipped"] == 0 and seen[1]["gaps_fixed"] == seen[0]["gaps_fixed"] + seen[0]["gaps_skipped"]
    c.close()


# ------------------------------------------------------------------------------------------------ 3. exact sizes
@pytest.fixture(scope="module")
def truth_graph(gkc):
    """the ground-truth genome of tests/test_read_correct_cpu.py counted as one read -> (counter, genome, unitig strings, solid set)"""
    genome, seqs, solid = ground_truth(K_GT)
    bases, offs = pack([genome])
    c = counter_for(gkc, bases, offs, K_GT, M_GT, 4)
    vals, _, _ = solid_records(c)
    dev = unitig_strings(*c.unitigs()[:2])
    assert len(dev) == 1 and dev[0] in (seqs[0], rc_str(seqs[0])) and set(vals) == solid
    yield c, genome, dev, solid
    c.close()


def small_reads(genome):
    """short reads with one substitution each: heads, gaps, tails, both strands, one read too short to keep a segment, an empty one, one without an error. 19 reads
    (odd), an odd number of bases: every copy of a tiled input stands one phase further in a vector, a word and a wave"""
    reads = []
    for i in range(16):
        n = 44 + 3 * (i % 5)
        piece = genome[300 + 97 * i: 300 + 97 * i + n]
        piece = substitute(piece, (3, n // 2, n - 4, 21, n - 22)[i % 5], 1 + i % 3)
        reads.append(rc_str(piece) if i % 2 else piece)
    reads += [substitute(genome[100:130], 15), "", genome[2000:2051]]
    return reads


def tiled(D, exp, reps):
    """the inputs of the small case repeated ``reps`` times on the device, and the statement's answer tiled by arithmetic. Segments hold read-relative positions: only
    the two offset tables shift from copy to copy"""
    nr, nb, ns = D["nr"], D["nb"], D["ns"]
    offs = D["to"].cpu().numpy().view(np.uint64); so = D["so"].cpu().numpy().view(np.uint64)
    shift = lambda t, step: np.concatenate([[0], (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(step) + t[None, 1:]).reshape(-1)]).astype(np.uint64)
    big = dict(D, tb=D["tb"][:nb].repeat(reps), to=upload(shift(offs, nb)), so=upload(shift(so, ns)), seg=D["seg"].repeat(reps),
               nr=nr * reps, nb=nb * reps, ns=ns * reps)
    want = dict(bases=np.tile(exp["bases"], reps), n_changed=np.tile(exp["n_changed"], reps), changed=np.tile(exp["changed"], reps),
                stats={n: int(exp["stats"][n]) * reps for n in STATS})
    return big, want, shift(offs, nb)


@pytest.mark.parametrize("reps", [129, PASS // 19 + 3], ids=["every_phase", "grid_pass"])
def test_regions_and_read_borders_on_every_phase_and_past_one_grid_pass(gkc, truth_graph, reps):
    assert (VEC, WORD, WAVE, PASS, COPY_PASS) == (16, 64, 64, 524288, 8388608)
    c, genome, seqs, solid = truth_graph
    bases, offs = pack(small_reads(genome))
    paths = read_paths_np(bases, offs, seqs, K_GT, solid)
    exp = correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, K_GT)
    st = exp["stats"]
    assert len(offs) - 1 == 19 and len(bases) % 2 == 1 and st["gaps_fixed"] >= 3 and st["heads_fixed"] >= 3 and st["tails_fixed"] >= 3 and st["bases_changed"] == 16
    D = device_inputs(c, bases, offs)
    assert D["ns"] == len(paths["segments"]) and np.array_equal(D["so"].cpu().numpy().view(np.uint64), paths["seg_offsets"])
    assert_raw(correct_raw(c, D), exp, D)
    big, want, big_offs = tiled(D, exp, reps)
    at = np.flatnonzero(want["changed"])
    for unit in (VEC, WORD):                                    # a changed byte, a read's first base and the base behind its last one on every phase of a vector and a word
        assert len(set((at % unit).tolist())) == unit and len(set((big_offs % np.uint64(unit)).tolist())) == unit
    starts = np.arange(reps) * 19                               # the first read of a copy on every lane of a wave
    assert len(set((starts % WAVE).tolist())) == WAVE
    if reps > 129:
        assert big["nr"] > PASS + 19 and big["nb"] > COPY_PASS + len(bases) and (PASS // 19) * 19 < PASS < (PASS // 19 + 1) * 19      # a copy of the reads straddles the pass
    assert big["nb"] % VEC != 0                                 # the bytes behind the last whole vector
    assert_raw(correct_raw(c, big), want, big)
    assert_raw(correct_raw(c, big, in_place=True), want, big)


# ------------------------------------------------------------------------------------------------ 4. edges
def small_case(truth_graph):
    c, genome, seqs, solid = truth_graph
    bases, offs = pack(small_reads(genome))
    paths = read_paths_np(bases, offs, seqs, K_GT, solid)
    return c, bases, offs, paths, correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, K_GT)


def test_no_reads_no_segments_and_exactly_one_read(gkc, truth_graph):
    c, genome, seqs, solid = truth_graph
    c.unitigs_build()
    for reads in ([], [""], ["", "ACGT", "N" * 40, "A" * 40], [substitute(genome[500:650], 70)], [genome[500:650]]):
        bases, offs = pack(reads)
        paths = read_paths_np(bases, offs, seqs, K_GT, solid)
        exp = correct_reads_np(bases, offs, paths["seg_offsets"], paths["segments"], seqs, K_GT)
        assert len(paths["segments"]) == (0 if len(reads) != 1 or not reads[0] else 2 if reads[0] != genome[500:650] else 1)
        assert_corrected(c.correct_reads(bases, offs), exp, paths)
        D = device_inputs(c, bases, offs)
        assert_raw(correct_raw(c, D), exp, D)                   # a copy, the counts and the bits zeroed, nothing else touched
        assert_raw(correct_raw(c, D, in_place=True), exp, D)
    assert exp["stats"]["bases_changed"] == 0 and np.array_equal(exp["bases"], bases)


def test_null_outputs_null_params_and_in_place(gkc, truth_graph):
    c, bases, offs, paths, exp = small_case(truth_graph)
    c.unitigs_build()
    D = device_inputs(c, bases, offs)
    full = correct_raw(c, D, (2, 1))
    assert_raw(full, exp, D)
    same = correct_raw(c, D, None)                              # params == NULL: {2, 1}
    assert all(np.array_equal(same[n], full[n]) for n in ("out", "n_changed", "bits")) and same["stats"] == full["stats"] and same["rc"] == 0
    assert correct_raw(c, D, (1, 0))["stats"] != full["stats"]
    for nch, bits, stats in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        res = correct_raw(c, D, (2, 1), n_changed=nch, bits=bits, stats=stats)
        assert res["rc"] == 0 and np.array_equal(res["out"], full["out"])
        assert np.array_equal(res["n_changed"], full["n_changed"]) if nch else (res["n_changed"] == CANARY).all()
        assert np.array_equal(res["bits"], full["bits"]) if bits else (res["bits"] == CANARY).all()
        assert res["stats"] == (full["stats"] if stats else (0xDEAD,) * 7)
    there = correct_raw(c, D, (2, 1), in_place=True)
    assert all(np.array_equal(there[n], full[n]) for n in ("out", "n_changed", "bits")) and there["stats"] == full["stats"]
    got = c.correct_reads_device(D["tb"].data_ptr(), D["to"].data_ptr(), D["nr"], D["nb"], D["so"].data_ptr(), D["seg"].data_ptr(), D["ns"], D["ub"].data_ptr(), D["uo"].data_ptr(),
                                 D["tb"].data_ptr())
    assert got == {n: int(exp["stats"][n]) for n in STATS} and np.array_equal(D["tb"][: D["nb"]].cpu().numpy(), exp["bases"])


# ------------------------------------------------------------------------------------------------ 5. errors and state
def test_errors_and_state(gkc, tmp_path):
    k, m, parts = K_GT, M_GT, 4
    genome, _, solid = ground_truth(k)
    twin = substitute(genome, 1500)
    bases, offs = pack([genome, twin])                          # a bubble: four unitigs
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    seqs = unitig_strings(*c.unitigs()[:2])
    vals, _, _ = solid_records(c)
    nu = len(seqs)
    assert nu == 4
    qb, qo = pack([substitute(substitute(genome[200:350], 60), 120), "", substitute(twin[1400:1600], 30), genome[2500:2560]])
    paths = read_paths_np(qb, qo, seqs, k, set(vals))
    exp = correct_reads_np(qb, qo, paths["seg_offsets"], paths["segments"], seqs, k)
    so, sg = paths["seg_offsets"], paths["segments"]
    assert so.tolist()[:3] == [0, 3, 3] and len(sg) == so[-1] >= 7 and exp["stats"]["gaps_fixed"] == 3
    D = device_inputs(c, qb, qo)
    assert_raw(correct_raw(c, D), exp, D)
    assert gkc.write_corrected_fasta(str(tmp_path / "r.fa"), exp["bases"], qo, names=["a", "b", "c", "d"]) == 4
    text = exp["bases"].tobytes().decode()
    assert open(str(tmp_path / "r.fa")).read() == "".join(">%s\n%s\n" % (n, text[int(qo[r]): int(qo[r + 1])]) for r, n in enumerate("abcd"))

    def refused(word, in_place=False, **over):
        res = correct_raw(c, D, in_place=in_place, **over)
        assert res["rc"] == 1 and word in c.L.gkc_last_error(c.h) and untouched(res, in_place or "out_shift" in over), (word, res["rc"], c.L.gkc_last_error(c.h))

    one = lambda a, i, v: np.concatenate([a[:i], np.array([v], a.dtype), a[i + 1:]])      # a with one value replaced

    def seg_with(i, field, v):
        bad = sg.copy(); bad[field][i] = v
        return upload(bad)

    L = [len(s) - k + 1 for s in seqs]
    last = len(sg) - 1
    for in_place in (False, True):
        # read offsets / segment offsets that are no CSR table
        for wrong in (one(qo, 0, 1), one(qo, 2, int(qo[3]) + 1), one(qo, 4, int(qo[4]) + 7), one(qo, 4, int(qo[4]) - 1)):
            refused(b"read offsets", in_place, to=upload(wrong))
        for wrong in (one(so, 0, 1), one(so, 1, int(so[3]) + 1), one(so, 4, int(so[4]) + 1), one(so, 3, 1 << 50)):
            refused(b"segment offsets", in_place, so=upload(wrong))
        refused(b"segment offsets", in_place, ns=D["ns"] - 1)
        # a segment that overlaps its predecessor, one that descends against it
        refused(b"overlap", in_place, seg=seg_with(1, "read_pos", int(sg["read_pos"][0]) + int(sg["n_kmers"][0]) - 1))
        refused(b"overlap", in_place, seg=seg_with(2, "read_pos", 0))
        # a segment that runs past its read: by one k-mer, and far
        refused(b"past the end", in_place, seg=seg_with(2, "read_pos", 150 - (k - 1) - int(sg["n_kmers"][2]) + 1))
        refused(b"past the end", in_place, seg=seg_with(last, "read_pos", (1 << 32) - 1))
        # a node of no unitig: just beyond, far beyond, a sentinel of the nodes call
        for at, node in ((0, 2 * nu), (1, 2 * nu + 1), (2, 1 << 50), (last, gkc.NODE_ABSENT)):
            refused(b"unitig", in_place, seg=seg_with(at, "node", node))
        # a unitig range that leaves [0, L_u): at either end, on the segment's own strand; and a segment of no k-mer
        u0, rev0 = int(sg["node"][0]) >> 1, int(sg["node"][0]) & 1
        refused(b"range", in_place, seg=seg_with(0, "unitig_pos", int(sg["n_kmers"][0]) - 2 if rev0 else L[u0] - int(sg["n_kmers"][0]) + 1))
        refused(b"range", in_place, seg=seg_with(0, "unitig_pos", L[u0] if rev0 else (1 << 32) - 1))
        refused(b"range", in_place, seg=seg_with(last, "n_kmers", 0))
        # unitig offsets of another placement
        uo = D["uo"].cpu().numpy().view(np.uint64)
        for wrong in (one(uo, 0, 1), one(uo, nu, int(uo[nu]) + 1), one(uo, 1, int(uo[1]) - 1), one(uo, 2, 1 << 60)):
            refused(b"unitig offsets", in_place, uo=upload(wrong))
    # an output that overlaps the input without being it, and one that is not aligned
    refused(b"overlaps", out_shift=16)
    refused(b"overlaps", out_shift=D["nb"] - 16 - D["nb"] % 16)
    refused(b"aligned", out_shift=D["nb"] + 1 + (-D["nb"]) % 16)
    assert correct_raw(c, D, out_shift=D["nb"] + (-D["nb"]) % 16)["rc"] == 0      # (disjoint inside one buffer: served)
    # a recount: the placement of the first count must not answer; before any build of the new results neither
    c.begin_pass(0); c.push_reads(bases, offs); c.finish_pass()
    res = correct_raw(c, D)
    assert res["rc"] == 1 and untouched(res) and (b"changed" in c.L.gkc_last_error(c.h) or b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h))
    with pytest.raises(gkc.GkcError):
        c.correct_reads(qb, qo)
    c.unitigs_build()
    assert_raw(correct_raw(c, D), exp, D)
    c.close()
    # before a build
    c = gkc.Counter(0); c.configure(k, m, parts, simple_repart(m, parts))
    c.count(bases, offs)
    res = correct_raw(c, D)
    assert res["rc"] == 1 and b"gkc_graph_unitigs_build" in c.L.gkc_last_error(c.h) and untouched(res)
    with pytest.raises(gkc.GkcError):
        c.correct_reads(qb, qo)
    c.close()


# ------------------------------------------------------------------------------------------------ 6. timers
def test_timers(gkc, truth_graph):
    c, bases, offs, paths, exp = small_case(truth_graph)
    c.unitigs_build()
    names = ("graph_read_nodes", "graph_read_segments", "graph_emit", "graph_read_correct", "graph_read_walks")
    before = {n: c.timing(n)[1] for n in names}
    c.correct_reads(bases, offs)                                # one nodes call, the sizing call and the fill of the segments, the unitig strings, one correction
    assert [c.timing(n)[1] - before[n] for n in names] == [1, 2, 1, 1, 0]
    D = device_inputs(c, bases, offs)
    mid = c.timing("graph_read_correct")[1]
    for i in range(3):
        correct_raw(c, D)
        assert c.timing("graph_read_correct")[1] == mid + i + 1
