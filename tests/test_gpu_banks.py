"""Multi-bank counting on the device (gkc.Banks: csrc/gkc_banks.hip) against the CPU oracle. Expected values everywhere: oracle.gko.Dsk once per bank with the
window [1, 2^31 - 1] and the same repartition table, the per-dataset union of the banks' k-mers taken in numpy (an int32 matrix, one column per bank), then
tests/test_banks_cpu.py:solid_mask — itself checked against the reference's recorded answers. Every comparison is exact. Run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests.test_banks_cpu import KINDS, fixture_cases, solid_mask
from tests.util import simple_repart, synth_reads

pytestmark = pytest.mark.gpu

INF = 2 ** 31 - 1


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ expected values
def oracle_bank(reads, k, m, parts, rep, passes=1):
    """-> [(lo, hi, abundance) per dataset] of one bank"""
    bases, offs = gko.pack_reads(reads)
    d = gko.Dsk(bases, offs, k, m, parts, rep, nb_passes=passes, abundance_min=1, abundance_max=INF)
    out = [d.part(i) for i in range(parts * passes)]
    d.close()
    return out


def union_of(per_bank, nb_banks=None, columns=None):
    """per_bank: oracle_bank results -> [(lo, hi, int32[n][nb_banks]) per dataset]: the ascending union of the banks' k-mers and their counts; columns[i]: the
    bank index per_bank[i] stands for (default i); a bank nobody stands for is a column of zeros"""
    nb_banks = nb_banks or len(per_bank)
    columns = list(range(len(per_bank))) if columns is None else columns
    out = []
    for d in range(len(per_bank[0])):
        if all(not p[d][1].any() for p in per_bank):                                   # 8-byte keys
            lo = np.unique(np.concatenate([p[d][0] for p in per_bank]))
            mat = np.zeros((len(lo), nb_banks), np.int32)
            for col, p in zip(columns, per_bank):
                mat[np.searchsorted(lo, p[d][0]), col] = p[d][2]
            out.append((lo, np.zeros(len(lo), np.uint64), mat))
        else:                                                                          # 16-byte keys: (hi, lo) order
            ints = [[(h << 64) | l for l, h in zip(p[d][0].tolist(), p[d][1].tolist())] for p in per_bank]
            keys = sorted(set().union(*ints))
            at = {x: i for i, x in enumerate(keys)}
            mat = np.zeros((len(keys), nb_banks), np.int32)
            for col, p, xs in zip(columns, per_bank, ints):
                mat[[at[x] for x in xs], col] = p[d][2]
            out.append((np.array([x & (2 ** 64 - 1) for x in keys], np.uint64), np.array([x >> 64 for x in keys], np.uint64), mat))
    return out


def records_of(lo, hi, ab, wide):
    """the Count{value, abundance} memory layout: 16 bytes (k <= 31) or 32 (k <= 63), pad bytes zero"""
    r = np.zeros((len(lo), 4 if wide else 2), np.uint64)
    r[:, 0] = lo
    if wide:
        r[:, 1] = hi
    r[:, 2 if wide else 1] = ab.astype(np.uint64)
    return r.tobytes()


def check_evaluation(B, exp, kind, amin, amax, solid_vec=None, histo_max=50):
    """evaluates and compares every dataset's records, vectors and sizes and the histogram -> number of solid k-mers"""
    B.evaluate(kind, amin, amax, solid_vec, histo_max)
    wide = B.rec_bytes == 32
    total = 0; sums = []
    for d, (lo, hi, mat) in enumerate(exp):
        mask = solid_mask(mat, kind, amin, amax, solid_vec)
        s = mat.sum(axis=1, dtype=np.int64)
        sums.append(s)
        tag = (kind, amin, amax, "dataset", d)
        assert B.partition_info(d) == (int(mask.sum()), len(lo)), tag
        assert B.partition_records(d).tobytes() == records_of(lo[mask], hi[mask], s[mask], wide), tag
        assert np.array_equal(B.vectors(d), mat[mask]), tag
        total += int(mask.sum())
    s = np.concatenate(sums) if sums else np.zeros(0, np.int64)
    assert np.array_equal(B.histogram(), np.bincount(np.minimum(s, histo_max), minlength=histo_max + 1).astype(np.uint64)), (kind, amin, amax)
    return total


def count_and_add(c, B, bank, reads):
    bases, offs = gko.pack_reads(reads)
    c.count(bases, offs)
    B.add(bank)


def merged(gkc, banks_reads, k, m, parts, rep=None, passes=1):
    """-> (Counter, Banks with every bank added in order, expected union)"""
    rep = simple_repart(m, parts) if rep is None else rep
    c = gkc.Counter(0); c.configure(k, m, parts, rep, nb_passes=passes)
    B = gkc.Banks(c, len(banks_reads))
    for i, reads in enumerate(banks_reads):
        count_and_add(c, B, i, reads)
    exp = union_of([oracle_bank(r, k, m, parts, rep, passes) for r in banks_reads])
    return c, B, exp


# ------------------------------------------------------------------------------------------------ 1. the reference's known answers
@pytest.mark.parametrize("table,m", [("perbank1", 8), ("perbank2", 4)])
def test_reference_known_answers(gkc, golden_dir, table, m):
    """TestDSK.cpp:482-612: one bank per sequence; all rows of a table on ONE merged state by repeated evaluation"""
    name, seqs, k, cases = [t for t in fixture_cases(golden_dir) if t[0] == table][0]
    c, B, exp = merged(gkc, [[s] for s in seqs], k, m, 1, rep=np.zeros(4 ** m, np.uint16))
    assert len(cases) in (9, 45)
    for kind, amin, amax, recorded in cases:
        assert check_evaluation(B, exp, kind, amin, amax) == recorded, (table, kind, amin, amax)
    B.close(); c.close()


# ------------------------------------------------------------------------------------------------ 2. / 3. bit-exact merge
WINDOWS = ((1, INF), (2, INF), (2, 3))


def test_merge_bit_exact_8_byte_keys(gkc):
    k, m, parts = 31, 10, 16
    rep = simple_repart(m, parts)
    # one genome for all four, the seeds of the reads and the substitution rates differ
    banks = [synth_reads_same_genome(6000, 200000, 100, genome_seed=1, seed=10 + i, sub_rate=sr) for i, sr in enumerate((0.0, 0.005, 0.01, 0.03))]
    c, B, exp = merged(gkc, banks, k, m, parts, rep)
    shared = sum(int((mat > 0).all(axis=1).sum()) for _, _, mat in exp); everything = sum(len(lo) for lo, _, _ in exp)
    assert 0 < shared < everything                                   # the banks overlap partly
    for kind in KINDS:
        for amin, amax in WINDOWS:
            check_evaluation(B, exp, kind, amin, amax, [1, 0, 1, 0] if kind == "custom" else None)
    # kind sum is the single-bank count of the concatenated reads
    whole = oracle_bank([r for b in banks for r in b], k, m, parts, rep)
    B.evaluate("sum", 1, INF, None, 50)
    for d in range(parts):
        assert B.partition_records(d).tobytes() == records_of(*whole[d], False), d
        lo, hi, ab = B.partition(d)
        assert np.array_equal(lo, whole[d][0]) and np.array_equal(hi, whole[d][1]) and np.array_equal(ab, whole[d][2])
    B.close(); c.close()


def synth_reads_same_genome(n_reads, genome_len, read_len, genome_seed, seed, sub_rate):
    """tests/util.py:synth_reads draws genome and reads from one seed; banks that overlap need one genome and different reads: the reads of
    synth_reads(genome_seed) with sub_rate 0 are error-free windows of the genome, so a bank = a seeded choice among many of them + its own substitutions"""
    pool = _genome_windows(genome_seed, genome_len, read_len)
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACTG", dtype=np.uint8); code = np.zeros(256, np.uint8); code[alpha] = np.arange(4, dtype=np.uint8)
    out = []
    for i in rng.integers(0, len(pool), n_reads):
        r = code[np.frombuffer(pool[int(i)], dtype=np.uint8)]
        hit = rng.random(read_len) < sub_rate
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
        out.append(alpha[r].tobytes())
    return out


@functools.lru_cache(maxsize=None)
def _genome_windows(genome_seed, genome_len, read_len):
    return tuple(synth_reads(20000, genome_len, read_len, seed=genome_seed, sub_rate=0.0))


def test_merge_bit_exact_16_byte_keys(gkc):
    k, m, parts = 63, 11, 16
    rep = simple_repart(m, parts)
    banks = [synth_reads_same_genome(3000, 200000, 100, genome_seed=2, seed=20 + i, sub_rate=sr) for i, sr in enumerate((0.0, 0.01, 0.02))]
    # keys that share their top word: 200 copies of one 150 bp read and its one-substitution variants
    rng = np.random.default_rng(5)
    read = "".join(rng.choice(list("ACGT"), 150))
    variants = [read[:p] + ("A" if read[p] != "A" else "C") + read[p + 1:] for p in range(0, 150, 3)]
    banks.append([read] * 200 + variants)
    c, B, exp = merged(gkc, banks, k, m, parts, rep)
    hi = np.concatenate([h for _, h, _ in exp])
    assert len(hi) > len(np.unique(hi))                              # some keys differ in the low word only
    for kind in ("sum", "min", "one"):
        for amin, amax in WINDOWS:
            check_evaluation(B, exp, kind, amin, amax)
    whole = oracle_bank([r for b in banks for r in b], k, m, parts, rep)
    B.evaluate("sum", 1, INF, None, 50)
    for d in range(parts):
        assert B.partition_records(d).tobytes() == records_of(*whole[d], True), d
    B.close(); c.close()


# ------------------------------------------------------------------------------------------------ 4. tile and scan boundaries
def kmer_reads(values, k=31):
    """k-mer-long reads whose canonical k-mers are exactly `values`: the forward k-mer starts with A and does not end with T, so its reverse complement is larger"""
    v = np.asarray(values, dtype=np.uint64)
    assert ((v >> np.uint64(2 * k - 2)) == 0).all() and ((v & np.uint64(3)) != 2).all()
    shifts = np.arange(2 * (k - 1), -1, -2, dtype=np.uint64)
    codes = ((v[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8)
    flat = np.frombuffer(b"ACTG", dtype=np.uint8)[codes]
    return [row.tobytes() for row in flat]


def boundary_sizes(gkc):
    T, S = gkc.Banks.TILE, gkc.Banks.SCAN_BLOCK
    big = S * T + 1 if S * T + 1 <= 2000000 else 2000000             # (with the kernels' constants: 256 * 1024 + 1, one element past a full block of the scan of tile sums)
    return [1, T - 1, T, T + 1, 3 * T + 7, big]


BASE_A = 1 << 40


def bank_b_values(case, n):
    i = np.arange(n, dtype=np.uint64) * np.uint64(4)
    return {"equal": np.uint64(BASE_A) + i,                          # everything is a duplicate
            "interleaved": np.uint64(BASE_A) + i + np.uint64(1),     # disjoint: A even, B odd, alternating
            "below": np.uint64(1 << 38) + i,
            "above": np.uint64(1 << 42) + i}[case]


@functools.lru_cache(maxsize=None)
def boundary_bank(case, n):
    """-> (reads, oracle result) of bank A (case "a") or of bank B of a case"""
    v = np.uint64(BASE_A) + np.arange(n, dtype=np.uint64) * np.uint64(4) if case == "a" else bank_b_values(case, n)
    reads = kmer_reads(v)
    return reads, oracle_bank(reads, 31, 10, 1, np.zeros(4 ** 10, np.uint16))


@pytest.mark.parametrize("case", ["equal", "interleaved", "below", "above"])
@pytest.mark.parametrize("which", range(6))
def test_tile_and_scan_boundaries(gkc, which, case):
    n = boundary_sizes(gkc)[which]
    (ra, oa), (rb, ob) = boundary_bank("a", n), boundary_bank(case, n)
    assert len(oa[0][0]) == n and len(ob[0][0]) == n                # the sizes are exact
    c = gkc.Counter(0); c.configure(31, 10, 1, np.zeros(4 ** 10, np.uint16))
    B = gkc.Banks(c, 2)
    count_and_add(c, B, 0, ra); count_and_add(c, B, 1, rb)
    exp = union_of([oa, ob])
    assert len(exp[0][0]) == (n if case == "equal" else 2 * n)
    assert check_evaluation(B, exp, "sum", 1, INF) == len(exp[0][0])
    assert check_evaluation(B, exp, "all", 1, INF) == (n if case == "equal" else 0)
    check_evaluation(B, exp, "custom", 1, INF, [0, 1])               # every other k-mer solid when interleaved: the gather's scan across tiles
    B.close(); c.close()


# ------------------------------------------------------------------------------------------------ 5. shapes
def small_banks(n_banks, n_reads=300, seed0=30):
    return [synth_reads_same_genome(n_reads, 200000, 100, genome_seed=1, seed=seed0 + i, sub_rate=0.01) for i in range(n_banks)]


def test_two_passes_added_pass_by_pass_or_at_once(gkc):
    k, m, parts, passes = 31, 10, 4, 2
    rep = simple_repart(m, parts)
    banks = small_banks(3)
    exp = union_of([oracle_bank(r, k, m, parts, rep, passes) for r in banks])
    assert sum(len(lo) for lo, _, _ in exp[:parts]) and sum(len(lo) for lo, _, _ in exp[parts:])        # both passes hold k-mers
    c = gkc.Counter(0); c.configure(k, m, parts, rep, nb_passes=passes)
    one_by_one = gkc.Banks(c, 3); at_once = gkc.Banks(c, 3)
    for i, reads in enumerate(banks):
        bases, offs = gko.pack_reads(reads)
        for ps in range(passes):
            c.begin_pass(ps); c.push_reads(bases, offs); c.finish_pass()
            one_by_one.add(i)                                        # the pass just counted; the other pass still holds the previous bank's (merged) results
        at_once.add(i)                                               # both passes of the bank, into another object
    for B in (one_by_one, at_once):
        assert B.nb_datasets == parts * passes
        for kind in ("sum", "min", "one"):
            check_evaluation(B, exp, kind, 2, INF)
        B.close()
    c.close()


def test_empty_bank_missing_bank_any_order_and_context_reuse(gkc):
    k, m, parts = 31, 10, 4
    rep = simple_repart(m, parts)
    banks = small_banks(3)
    per = [oracle_bank(r, k, m, parts, rep) for r in banks]
    c = gkc.Counter(0); c.configure(k, m, parts, rep)
    # banks 2, 0, 1 of 5: bank 3 is counted from zero reads, bank 4 is never added
    B = gkc.Banks(c, 5)
    for i in (2, 0, 1):
        count_and_add(c, B, i, banks[i])
    count_and_add(c, B, 3, [])
    exp = union_of(per, nb_banks=5)
    for kind, sv in (("sum", None), ("min", None), ("max", None), ("one", None), ("all", None), ("custom", [1, 1, 0, 0, 0])):
        check_evaluation(B, exp, kind, 1, INF, sv)
    assert check_evaluation(B, exp, "min", 1, INF) == 0 and check_evaluation(B, exp, "all", 0, INF) == sum(len(lo) for lo, _, _ in exp)
    # the context goes on to other work: the merged state owns its copies
    c.begin_pass(0); c.push_reads(*gko.pack_reads(banks[0][:50])); c.finish_pass()
    check_evaluation(B, exp, "sum", 2, 3)
    assert B.all_counts() == {(int(h) << 64) | int(l): tuple(r) for lo, hi, mat in exp
                              for l, h, r, ok in zip(lo.tolist(), hi.tolist(), mat.tolist(), solid_mask(mat, "sum", 2, 3).tolist()) if ok}
    # an evaluation of nothing at all
    E = gkc.Banks(c, 2)
    assert check_evaluation(E, [(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 2), np.int32))] * parts, "sum", 1, INF) == 0
    E.close(); B.close(); c.close()


def test_many_partitions_mostly_empty_datasets(gkc):
    k, m, parts = 31, 10, 64
    rep = simple_repart(m, parts)
    banks = [b[:n] for b, n in zip(small_banks(3, 300, seed0=40), (300, 40, 3))]
    c, B, exp = merged(gkc, banks, k, m, parts, rep)
    per = [oracle_bank(r, k, m, parts, rep) for r in banks]
    assert any(len(per[2][d][0]) == 0 and len(per[0][d][0]) > 0 for d in range(parts))                  # datasets empty in some banks only
    for kind in KINDS:
        check_evaluation(B, exp, kind, 1, 2, [1, 0, 0] if kind == "custom" else None)
    # the histogram's three homes: privatised in LDS (50 bins above, the largest that fits here), or too large for it and added to in HBM
    for hm in (15999, 16000, 20000):
        check_evaluation(B, exp, "sum", 1, INF, histo_max=hm)
    B2 = c.count_banks([gko.pack_reads(r) for r in banks], kind="max", amin=2, amax=INF, histo_max=50)    # the convenience loop
    mask_total = sum(int(solid_mask(mat, "max", 2, INF).sum()) for _, _, mat in exp)
    assert sum(B2.partition_info(d)[0] for d in range(parts)) == mask_total
    assert check_evaluation(B2, exp, "max", 2, INF) == mask_total
    B2.close(); B.close(); c.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_name_their_cause(gkc):
    k, m, parts = 31, 10, 4
    rep = simple_repart(m, parts)
    reads = small_banks(1, 100)[0]
    bases, offs = gko.pack_reads(reads)
    c = gkc.Counter(0); c.configure(k, m, parts, rep)
    with pytest.raises(gkc.GkcError, match="nb_banks"):
        gkc.Banks(c, 0)
    with pytest.raises(gkc.GkcError, match="nb_banks"):
        gkc.Banks(c, 65)
    B = gkc.Banks(c, 2)
    with pytest.raises(gkc.GkcError, match="no finished dataset"):
        B.add(0)
    c.count(bases, offs)
    for read in (lambda: B.partition_info(0), lambda: B.partition(0), lambda: B.vectors(0), lambda: B.histogram(), lambda: B.partition_device(0)):
        with pytest.raises(gkc.GkcError, match="gkc_banks_evaluate first"):
            read()
    with pytest.raises(gkc.GkcError, match="bank 2 >= nb_banks 2"):
        B.add(2)
    B.add(0)
    with pytest.raises(gkc.GkcError, match="added already"):
        B.add(0)                                                     # the same (bank, dataset) pairs again
    with pytest.raises(gkc.GkcError, match="added already"):
        B.add(1)                                                     # the same results as another bank: count the bank first
    c.count(bases, offs)
    with pytest.raises(gkc.GkcError, match="added already"):
        B.add(0)                                                     # a recount into a bank that holds the datasets
    # another model
    other = gkc.Counter(0); other.configure(k, m, parts, simple_repart(m, parts, seed=8)); other.count(bases, offs)
    with pytest.raises(gkc.GkcError, match="model"):
        B.add(1, other)
    other.close()
    # the same model in another context is fine — unless its window cuts counts away
    twin = gkc.Counter(0); twin.set_solidity(2, INF); twin.configure(k, m, parts, rep); twin.count(bases, offs)
    with pytest.raises(gkc.GkcError, match="solidity window"):
        B.add(1, twin)
    twin.set_solidity(1, INF); twin.count(bases, offs)
    twin.release_pass(0)
    with pytest.raises(gkc.GkcError, match="released"):
        B.add(1, twin)
    twin.count(bases, offs)
    B.add(1, twin)
    twin.close()
    B.evaluate("sum", 1, INF, None, 50)
    with pytest.raises(gkc.GkcError, match="kind"):
        B.evaluate(9, 1, INF)
    with pytest.raises(gkc.GkcError, match="solid_vec"):
        B.evaluate("custom", 1, INF)
    with pytest.raises(gkc.GkcError, match="dataset 4 >= 4"):
        B.partition_info(parts)
    # an evaluation is gone once a bank is added
    B3 = gkc.Banks(c, 2)
    c.count(bases, offs); B3.add(0); B3.evaluate("sum", 1, INF); assert B3.partition_info(0)[0] > 0
    c.count(bases, offs); B3.add(1)
    with pytest.raises(gkc.GkcError, match="gkc_banks_evaluate first"):
        B3.partition_info(0)
    B3.close()
    # the object outlives its context
    exp = union_of([oracle_bank(reads, k, m, parts, rep)] * 2)
    c.close()
    check_evaluation(B, exp, "all", 1, INF)
    with pytest.raises(gkc.GkcError, match="dataset 4 >= 4"):       # ... and still finds its error text
        B.partition_info(parts)
    B.close()
