"""Abundance queries on the device (gkc.Counter.query_* / gkc.Banks.query_reads: csrc/gkc_query.hip) against the CPU oracle. Expected values: the dict over
oracle.gko.Dsk(...).part(d) of all datasets looked up per position with oracle.gko.kmers (tests/test_query_cpu.py, checked there against a naive counter).
Every comparison is exact. Run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests.test_gpu_banks import oracle_bank, synth_reads_same_genome, union_of
from tests.test_query_cpu import EXTRA_READS, INF, canonical_per_position, expected_abundance, freq_order_of, oracle_table
from tests.util import naive_counts, revcomp_int, simple_repart, synth_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


# ------------------------------------------------------------------------------------------------ helpers
def counter_for(gkc, counted, k, m, parts, passes=1, rep=None, freq=None, amin=1, amax=INF):
    rep = simple_repart(m, parts) if rep is None else rep
    c = gkc.Counter(0); c.configure(k, m, parts, rep, nb_passes=passes, freq_order=freq)
    if (amin, amax) != (1, INF):
        c.set_solidity(amin, amax)
    c.count(*gko.pack_reads(counted))
    return c


def to_device(a, pad=64):
    """numpy array -> torch uint8 tensor on the device with `pad` spare bytes behind it (torch allocations are 16-byte aligned)"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(len(raw) + pad, dtype=torch.uint8, device="cuda")
    if len(raw):
        t[: len(raw)] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    return t


def query_reads_on_device(c, bases, offs, n_bases=None):
    """Counter.query_reads_device with torch buffers -> int32[n_bases]"""
    import torch
    n_bases = len(bases) if n_bases is None else n_bases
    tb = to_device(bases); to = to_device(offs)
    out = torch.full((len(bases) + 16,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.query_reads_device(tb.data_ptr(), to.data_ptr(), len(offs) - 1, n_bases, out.data_ptr())
    res = out.cpu().numpy()
    assert (res[n_bases:] == -7).all()                        # nothing written behind the array
    return res[:n_bases].copy()


# ------------------------------------------------------------------------------------------------ 1. the per-position array
CASES = [
    # k, m, parts, passes, order, abundance-min, n_rate, ragged
    (31, 8, 16, 1, "lexi", 1, 0.0, False),
    (31, 8, 16, 3, "lexi", 2, 0.01, True),
    (21, 6, 7, 2, "freq", 1, 0.0, True),
    (63, 10, 16, 2, "lexi", 1, 0.005, False),
    (47, 9, 5, 1, "freq", 3, 0.0, False),
    (5, 2, 3, 2, "lexi", 1, 0.0, False),
    (32, 8, 4, 1, "lexi", 1, 0.0, False),
    (33, 8, 4, 1, "lexi", 1, 0.0, False),
]


@functools.lru_cache(maxsize=None)
def case_data(case):
    k, m, parts, passes, order, amin, n_rate, ragged = case
    if k == 5:
        counted = synth_reads(50, 300, read_len=100, seed=3, sub_rate=0.02, n_rate=n_rate, ragged=ragged)
    else:
        counted = synth_reads(150 if k >= 47 else 200, 3000, read_len=100, seed=3, sub_rate=0.02, n_rate=n_rate, ragged=ragged)
    counted = counted + EXTRA_READS
    queried = counted + synth_reads(20, 3000, read_len=100, seed=99, sub_rate=0)       # ... and reads of a foreign genome
    rep = simple_repart(m, parts)
    freq = freq_order_of(counted, m) if order == "freq" else None
    _, table = oracle_table(counted, k, m, parts, passes, rep, freq=freq, amin=amin)
    bases, offs, exp = expected_abundance(queried, k, table)
    assert (exp > 0).any() and (exp == 0).any() and (exp == -1).any()
    return counted, rep, freq, bases, offs, exp


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d-m%d-P%d-p%d-%s-a%d" % c[:6])
def test_per_position_abundance(gkc, case, entry):
    k, m, parts, passes, order, amin = case[:6]
    counted, rep, freq, bases, offs, exp = case_data(case)
    c = counter_for(gkc, counted, k, m, parts, passes, rep, freq, amin=amin)
    got = c.query_reads(bases, offs) if entry == "host" else query_reads_on_device(c, bases, offs)
    print("k=%d: %d hits, %d zeros, %d without k-mer" % (k, (exp > 0).sum(), (exp == 0).sum(), (exp == -1).sum()))
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])
    c.close()


# ------------------------------------------------------------------------------------------------ 2. tile borders
@pytest.mark.parametrize("k,m", [(31, 8), (63, 10)])
def test_tile_borders(gkc, k, m):
    """one read of 40 000 bases, then 300 reads of lengths 1..400 cut from the same genome: for any tile size <= 16 384 read starts, read ends and invalid
    characters fall at every phase of a tile border"""
    rng = np.random.default_rng(11)
    alpha = np.frombuffer(b"ACTG", dtype=np.uint8)
    genome = alpha[rng.integers(0, 4, 45000)]
    counted = [genome[s:s + 150].tobytes() for s in rng.integers(0, 45000 - 150, 400)]
    long_read = genome[:40000].copy()
    long_read[rng.integers(0, 40000, 60)] = ord("N")
    long_read[[4095, 4096, 8191, 8192, 16383, 16384]] = ord("n")
    queried = [long_read.tobytes()]
    for i in range(300):
        L = 1 + (i * 131) % 400
        s = int(rng.integers(0, 45000 - L))
        r = genome[s:s + L].copy()
        if i % 7 == 0:
            r[int(rng.integers(0, L))] = ord("N")
        queried.append(r.tobytes())
    parts = 16
    rep = simple_repart(m, parts)
    _, table = oracle_table(counted, k, m, parts, 1, rep)
    bases, offs, exp = expected_abundance(queried, k, table)
    assert (exp > 0).any() and (exp == 0).any() and (exp == -1).any()
    c = counter_for(gkc, counted, k, m, parts, 1, rep)
    for got in (c.query_reads(bases, offs), query_reads_on_device(c, bases, offs)):
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])
    c.close()


# ------------------------------------------------------------------------------------------------ 3. keys
@pytest.mark.parametrize("k,m", [(31, 8), (63, 10)])
def test_keys(gkc, k, m):
    import torch
    parts, passes = 16, 2
    counted = synth_reads(150, 3000, read_len=100, seed=3, sub_rate=0.02) + EXTRA_READS
    rep = simple_repart(m, parts)
    ds, table = oracle_table(counted, k, m, parts, passes, rep)
    c = counter_for(gkc, counted, k, m, parts, passes, rep)
    keys = sorted(table)
    # the key, its reverse complement, and the neighbours key - 1 / key + 1 (mostly absent; answered from the dict through their canonical form)
    probes = keys + [revcomp_int(x, k) for x in keys] + [x - 1 for x in keys if x > 0] + [x + 1 for x in keys if x + 1 < 4 ** k]
    exp = np.array([table.get(min(x, revcomp_int(x, k)), 0) for x in probes], np.int32)
    assert (exp[: 2 * len(keys)] > 0).all() and (exp[2 * len(keys):] == 0).any()
    assert np.array_equal(c.query_kmers(probes), exp)                                  # host, bare keys (stride 8 / 16)
    a, n, stride = c._query_keys(probes)
    assert stride == (8 if k <= 31 else 16)
    tk = to_device(a); out = torch.zeros(n + 4, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    c.query_kmers_device(tk.data_ptr(), n, stride, out.data_ptr())                     # device, bare keys
    assert np.array_equal(out.cpu().numpy()[:n], exp)
    # Count arrays as they come out of the library (stride 16 / 32)
    raw = np.concatenate([c.partition_records(ps, pt) for ps in range(passes) for pt in range(parts)])
    exp_rec = np.concatenate([ab for _, _, ab in ds])
    assert len(raw) == len(exp_rec) * c.rec_bytes
    assert np.array_equal(c.query_kmers(raw), exp_rec)
    tr = to_device(raw); out = torch.zeros(len(exp_rec) + 4, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    c.query_kmers_device(tr.data_ptr(), len(exp_rec), c.rec_bytes, out.data_ptr())
    assert np.array_equal(out.cpu().numpy()[: len(exp_rec)], exp_rec)
    # a value that is no k-mer
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*4\\^%d" % k):
        c.query_kmers(keys[:5] + [4 ** k] + keys[5:9])
    assert np.array_equal(c.query_kmers(keys[:9]), exp[:9])                            # ... and the context still answers
    c.close()


# ------------------------------------------------------------------------------------------------ 4. index stride
@pytest.mark.parametrize("parts", [1, 64])
def test_index_stride(gkc, monkeypatch, parts):
    """window borders everywhere: one large dataset (parts = 1) and many tiny or empty ones (parts = 64), strides 1, 2, 3, 64 and the default"""
    k, m = 31, 8
    counted = synth_reads(200, 3000, read_len=100, seed=3, sub_rate=0.02) + EXTRA_READS
    queried = counted + synth_reads(20, 3000, read_len=100, seed=99, sub_rate=0)
    rep = simple_repart(m, parts)
    ds, table = oracle_table(counted, k, m, parts, 1, rep)
    if parts == 1:
        assert 8000 < len(ds[0][0]) < 11000
    else:
        assert any(len(lo) == 0 for lo, _, _ in ds) or min(len(lo) for lo, _, _ in ds) < 64
    bases, offs, exp = expected_abundance(queried, k, table)
    c = counter_for(gkc, counted, k, m, parts, 1, rep)              # ONE context: a stride that changes rebuilds the index
    keys = sorted(table)
    for stride in ("1", "2", "3", "64", None):
        if stride is None:
            monkeypatch.delenv("GKC_QUERY_INDEX_STRIDE", raising=False)
        else:
            monkeypatch.setenv("GKC_QUERY_INDEX_STRIDE", stride)
        got = c.query_reads(bases, offs)
        assert np.array_equal(got, exp), (stride, np.flatnonzero(got != exp)[:10])
        assert np.array_equal(c.query_kmers(keys), np.array([table[x] for x in keys], np.int32)), stride
        c2 = counter_for(gkc, counted, k, m, parts, 1, rep)         # ... and a fresh context at this stride
        assert np.array_equal(query_reads_on_device(c2, bases, offs), exp), stride
        c2.close()
    c.close()


# ------------------------------------------------------------------------------------------------ 5. solidity window
def test_solidity_window(gkc):
    """counted with [2, 5]: a k-mer seen once, or more than five times, is not in the results and reads 0"""
    k, m, parts = 31, 8, 16
    counted = synth_reads(200, 3000, read_len=100, seed=3, sub_rate=0.02) + EXTRA_READS
    rep = simple_repart(m, parts)
    _, table = oracle_table(counted, k, m, parts, 1, rep, amin=2, amax=5)
    bases, offs, exp = expected_abundance(counted, k, table)
    seen = naive_counts(counted, k)
    _, _, can = canonical_per_position(counted, k)
    times = np.array([-1 if x is None else seen[x] for x in can])
    assert (times == 1).any() and (times > 5).any() and ((times >= 2) & (times <= 5)).any()
    c = counter_for(gkc, counted, k, m, parts, 1, rep, amin=2, amax=5)
    got = c.query_reads(bases, offs)
    assert np.array_equal(got, exp)
    assert (got[(times == 1) | (times > 5)] == 0).all()
    inside = (times >= 2) & (times <= 5)
    assert np.array_equal(got[inside], times[inside])
    c.close()


# ------------------------------------------------------------------------------------------------ 6. state
def test_state_errors_and_recount(gkc):
    k, m, parts = 31, 8, 8
    rep = simple_repart(m, parts)
    reads_a = synth_reads(100, 3000, read_len=100, seed=3, sub_rate=0.02)
    reads_b = synth_reads(100, 3000, read_len=100, seed=4, sub_rate=0.02)
    bases, offs = gko.pack_reads(reads_a + reads_b)
    c = gkc.Counter(0)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*gkc_configure"):
        c.query_reads(bases, offs)
    c.configure(k, m, parts, rep)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*not counted"):             # before any count
        c.query_reads(bases, offs)
    c.begin_pass(0); c.push_reads(*gko.pack_reads(reads_a))
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*still open"):              # a pass is open
        c.query_reads(bases, offs)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*still open"):
        c.query_kmers([1, 2, 3])
    c.finish_pass()
    _, table_a = oracle_table(reads_a, k, m, parts, 1, rep)
    _, _, exp_a = expected_abundance(reads_a + reads_b, k, table_a)
    assert np.array_equal(c.query_reads(bases, offs), exp_a)
    # a recount of DIFFERENT reads in the same context: the index of the first count must not answer
    c.count(*gko.pack_reads(reads_b))
    _, table_b = oracle_table(reads_b, k, m, parts, 1, rep)
    _, _, exp_b = expected_abundance(reads_a + reads_b, k, table_b)
    assert not np.array_equal(exp_a, exp_b)
    assert np.array_equal(c.query_reads(bases, offs), exp_b)
    assert np.array_equal(query_reads_on_device(c, bases, offs), exp_b)
    # offsets that are no CSR table of the bases
    down = offs.copy(); down[5] = down[4] - 1
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*offsets"):
        query_reads_on_device(c, bases, down)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*offsets"):
        c.query_reads(bases, down)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*offsets"):                 # the table ends beyond n_bases
        query_reads_on_device(c, bases, offs, n_bases=len(bases) - 100)
    far = offs.copy(); far[7] = np.uint64(1) << np.uint64(50)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*offsets"):
        query_reads_on_device(c, bases, far)
    assert np.array_equal(c.query_reads(bases, offs), exp_b)                           # ... and the context still answers
    c.release_pass(0)
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*released"):
        c.query_reads(bases, offs)
    c.close()
    # two passes configured, only pass 0 finished
    c = gkc.Counter(0); c.configure(k, m, parts, rep, nb_passes=2)
    c.begin_pass(0); c.push_reads(*gko.pack_reads(reads_a)); c.finish_pass()
    with pytest.raises(gkc.GkcError, match="gkc error 1: .*pass 1 is not counted"):
        c.query_reads(bases, offs)
    c.begin_pass(1); c.push_reads(*gko.pack_reads(reads_a)); c.finish_pass()
    _, table_2 = oracle_table(reads_a, k, m, parts, 2, rep)
    assert table_2 == table_a
    assert np.array_equal(c.query_reads(bases, offs), exp_a)
    c.close()


# ------------------------------------------------------------------------------------------------ 7. per-read summary
def test_read_summary(gkc):
    case = CASES[1]
    k, m, parts, passes, order, amin = case[:6]
    counted, rep, freq, bases, offs, exp = case_data(case)
    c = counter_for(gkc, counted, k, m, parts, passes, rep, freq, amin=amin)
    got = c.query_reads(bases, offs)
    assert np.array_equal(got, exp)
    s = c.query_read_summary(got, offs)
    assert len(s) == len(offs) - 1
    none_valid = 0
    for r in range(len(offs) - 1):
        a = got[int(offs[r]):int(offs[r + 1])]
        v = a[a >= 0]
        want = (len(v), int((v > 0).sum()), int(v.min()) if len(v) else 0, int(v.max()) if len(v) else 0, int(v.sum()))
        assert tuple(int(x) for x in s[r].tolist()) == want, (r, s[r], want)
        none_valid += len(v) == 0
    assert none_valid >= 3                                           # reads without a valid k-mer: "ACG", "", "ACGTN" * 10
    c.close()


# ------------------------------------------------------------------------------------------------ 8. banks
def expected_banks(queried, k, exp_union, nb_banks):
    """-> (bases, offsets, int32[n_bases] sums, int32[n_bases][nb_banks] rows) from the union of tests/test_gpu_banks.py"""
    rows = {}
    for lo, hi, mat in exp_union:
        for a, b, v in zip(lo.tolist(), hi.tolist(), mat):
            rows[(b << 64) | a] = v
    bases, offs, can = canonical_per_position(queried, k)
    sums = np.zeros(len(bases), np.int32); vec = np.zeros((len(bases), nb_banks), np.int32)
    for g, x in enumerate(can):
        if x is None:
            sums[g] = -1
        elif x in rows:
            vec[g] = rows[x]; sums[g] = int(rows[x].sum())
    return bases, offs, sums, vec


@pytest.mark.parametrize("k,m", [(31, 10), (63, 11)])
def test_banks(gkc, k, m):
    parts, nb_banks = 16, 5
    rep = simple_repart(m, parts)
    banks = [synth_reads_same_genome(300, 20000, 100, genome_seed=1, seed=10 + i, sub_rate=sr) for i, sr in enumerate((0.0, 0.005, 0.02, 0.01))]
    queried = banks[0][:40] + banks[2][:40] + banks[3][:40] + [b"ACGTN" * 30, b"AC", b""] + synth_reads(10, 3000, read_len=100, seed=99, sub_rate=0)
    c = gkc.Counter(0); c.configure(k, m, parts, rep)
    B = gkc.Banks(c, nb_banks)                                       # banks 0..2 now, bank 3 later, bank 4 never
    for i in range(3):
        c.count(*gko.pack_reads(banks[i])); B.add(i)
    per_bank = [oracle_bank(r, k, m, parts, rep) for r in banks]
    bases, offs, sums, vec = expected_banks(queried, k, union_of(per_bank[:3], nb_banks), nb_banks)
    assert (sums > 0).any() and (sums == 0).any() and (sums == -1).any() and (vec[:, :3] > 0).all(axis=1).any() and not vec[:, 3:].any()

    def check(sums_, vec_):
        s, v = B.query_reads(bases, offs)
        assert np.array_equal(s, sums_), np.flatnonzero(s != sums_)[:10]
        assert np.array_equal(v, vec_)
        s2, v2 = B.query_reads(bases, offs, vectors=False)            # d_vectors = NULL
        assert v2 is None and np.array_equal(s2, sums_)

    check(sums, vec)                                                  # before any evaluation
    B.evaluate("min", 1, INF, None, 50)
    check(sums, vec)                                                  # an evaluation changes nothing
    assert B.partition_info(0)[1] > 0
    c.count(*gko.pack_reads(banks[3])); B.add(3)                      # another bank: the index of the old key array is gone
    bases, offs, sums4, vec4 = expected_banks(queried, k, union_of(per_bank, nb_banks), nb_banks)
    assert not np.array_equal(sums, sums4) and vec4[:, 3].any() and not vec4[:, 4].any()
    check(sums4, vec4)
    c.close()                                                         # the object keeps what it needs
    check(sums4, vec4)
    B.close()


# ------------------------------------------------------------------------------------------------ 9. several workgroups per dataset
def test_many_reads_vectorised(gkc):
    """5 000 reads x 150 bases, 64 partitions: hundreds of tiles, every dataset searched from many workgroups; the expectation by np.searchsorted into the
    concatenated oracle results"""
    k, m, parts = 31, 8, 64
    bases, offs = gkc.synth_reads_np(7, 5000, 150, 100000, 10000)
    rep = simple_repart(m, parts)
    d = gko.Dsk(bases, offs, k, m, parts, rep)
    ds = [d.part(i) for i in range(parts)]
    d.close()
    lo = np.concatenate([x[0] for x in ds]); ab = np.concatenate([x[2] for x in ds])
    order = np.argsort(lo, kind="stable"); lo = lo[order]; ab = ab[order]
    assert len(np.unique(lo)) == len(lo)
    # query the counted reads and as many reads of another genome
    b2, _ = gkc.synth_reads_np(8, 5000, 150, 100000, 0)
    qb = np.concatenate([bases, b2]); qo = np.arange(10001, dtype=np.uint64) * np.uint64(150)
    exp = np.full(len(qb), -1, np.int32)
    for r in range(10000):
        can = gko.kmers(qb[r * 150:(r + 1) * 150].tobytes(), k)["can_lo"]
        at = np.minimum(np.searchsorted(lo, can), len(lo) - 1)
        exp[r * 150: r * 150 + len(can)] = np.where(lo[at] == can, ab[at], 0)
    assert (exp[: len(bases)] != 0).all() and (exp[len(bases):] == 0).any()
    c = gkc.Counter(0); c.configure(k, m, parts, rep)
    c.count(bases, offs)
    got = query_reads_on_device(c, qb, qo)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])
    c.close()
