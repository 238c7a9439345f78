"""Stage B (csrc/gkc_count.hip) at exact sub-bucket sizes: tier borders, run ends, count edges. GKC_MAX_SUB_BITS=0 makes a partition one sub-bucket and
GKC_DEDUPE=0 a k-mer-long read one key of weight 1, so tests/stageb_inputs.py decides the number of keys of every sub-bucket and the sorted rank of every key:
every power of two from 64 to 8192 with its neighbours, 32768 and 32769, as distinct k-mers, as one k-mer, and as runs that end on / next to the last rank of a
lane and of a wave with the abundances around 64 and 255. Expected records, totals and histograms come from tests/util.naive_counts and a plain sort
(tests/test_stageb_cpu.py pins the inputs against the oracle); every comparison is exact, and a failure names the partition's pattern, size and tier.
k = 27 / 31: 8-byte keys on the f64-tagged / the integer network; k = 47 / 63: 16-byte keys. The switches are re-read at every pass. Run with `pytest -m gpu`."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests import stageb_inputs as sb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


def exact_sizes(monkeypatch, **switches):
    """one sub-bucket per partition, one key per read, and a test's own switches"""
    monkeypatch.setenv("GKC_MAX_SUB_BITS", "0"); monkeypatch.setenv("GKC_DEDUPE", "0")
    for name, value in switches.items():
        monkeypatch.setenv(name, str(value))


def count(gkc, k, specs, seed, amin=1, amax=sb.INF, histo_max=10000):
    """one Counter, every partition in one pass -> (expected, records per partition, partition_info per partition, histogram, stats)"""
    reads, repart, expected = sb.exact_partitions(k, sb.M, specs, seed)
    bases, offs = gko.pack_reads(reads)
    c = gkc.Counter(0)
    try:
        c.set_solidity(amin, amax, histo_max)
        c.configure(k, sb.M, len(specs), repart)
        c.count(bases, offs)
        records = [c.partition_records(0, p).tobytes() for p in range(len(specs))]
        infos = [c.partition_info(0, p) for p in range(len(specs))]
        return expected, records, infos, c.histogram(), c.stats()
    finally:
        c.close()


def first_difference(got, want, rec):
    """where two record arrays part, as text (a failed comparison of 10^5 bytes says nothing)"""
    g = np.frombuffer(got, np.uint64).reshape(-1, rec // 8); w = np.frombuffer(want, np.uint64).reshape(-1, rec // 8)
    n = min(len(g), len(w))
    bad = np.flatnonzero((g[:n] != w[:n]).any(axis=1))
    i = int(bad[0]) if len(bad) else n
    return "%d records, expected %d; %d differ, the first at index %d: got %s, expected %s" % (
        len(g), len(w), len(bad), i, g[i].tolist() if i < len(g) else None, w[i].tolist() if i < len(w) else None)


def check(gkc, k, specs, labels, seed=None, amin=1, amax=sb.INF, histo_max=10000, wg_max=None):
    """records, (solid, distinct, k-mers), histogram, distinct total and the number of roots of the split levels, against the expectation"""
    expected, records, infos, histogram, stats = count(gkc, k, specs, k if seed is None else seed, amin, amax, histo_max)
    rec = 32 if sb.is_wide(k) else 16
    for p, (label, exp) in enumerate(zip(labels, expected)):
        tag = sb.describe(label, k, wg_max)
        want = exp.solid_records(amin, amax)
        same = records[p] == want
        assert same, "%s: %s" % (tag, first_difference(records[p], want, rec))
        assert infos[p] == (len(want) // rec, exp.distinct, exp.kmers), tag
    want = sb.total_histogram(expected, histo_max)
    bad = np.flatnonzero(histogram != want)
    assert len(bad) == 0, [(int(b), int(histogram[b]), int(want[b])) for b in bad[:10]]
    assert stats["kmers_nb_distinct"] == sum(e.distinct for e in expected)
    assert stats["kmers_nb_solid"] == sum(int(e.solid(amin, amax).sum()) for e in expected)
    if labels[0][0] != "weighted":
        assert stats["oversize_buckets"] == sb.roots(labels, sb.is_wide(k), wg_max)
    return records, stats


def patterns_of(pattern):
    return ("runs", "ends") if pattern == "runs" else (pattern,)


@pytest.mark.parametrize("pattern", ["distinct", "one", "runs"])
@pytest.mark.parametrize("k", sb.K_CASES)
def test_every_size_and_pattern(gkc, monkeypatch, k, pattern):
    """every size as distinct k-mers / as one k-mer (abundance n: the escape to cnt32 from 255 on, the left == 0 branch of the split above the workgroup tier,
    at 32769 a giant of equal keys) / the runs patterns; the roots of the split levels are the partitions beyond 4096 keys (2048 with 16-byte keys)"""
    exact_sizes(monkeypatch)
    specs, labels = sb.case(k, patterns_of(pattern))
    check(gkc, k, specs, labels)


@pytest.mark.parametrize("pattern", ["distinct", "one", "runs"])
@pytest.mark.parametrize("k", sb.K_CASES)
def test_every_size_and_pattern_without_the_workgroup_tier(gkc, monkeypatch, k, pattern):
    """GKC_WG_MAX=1024: the workgroup tier is empty, its sizes go through the split levels: roots are the partitions beyond 2048 / 1024 keys"""
    exact_sizes(monkeypatch, GKC_WG_MAX=1024)
    specs, labels = sb.case(k, patterns_of(pattern))
    assert sb.roots(labels, sb.is_wide(k), 1024) > sb.roots(labels, sb.is_wide(k))
    check(gkc, k, specs, labels, wg_max=1024)


@pytest.mark.parametrize("k", sb.K_CASES)
def test_solidity_and_histogram_edges(gkc, monkeypatch, k):
    """the window [3, 256] is closed (2 and 257 out, 3 and 256 in), bins are clamped at histo_max = 300 (299 apart, 300 and 301 together), and bins below 64
    are counted in LDS, the others in global memory: the runs patterns, and a copy of each extended by k-mers seen 2, 3, 299, 300 and 301 times"""
    exact_sizes(monkeypatch)
    extend = (2, 3, 299, 300, 301)
    specs, labels = sb.case(k, ("runs", "ends"), extend=extend)
    expected = sb.exact_partitions(k, sb.M, specs, k)[2]
    h = sb.total_histogram(expected, 300)
    n_ext = sum(1 for pat, _ in labels if pat.endswith("+"))
    assert n_ext == 18 and h[299] == n_ext and h[300] == 2 * n_ext and all(h[b] > 0 for b in (62, 63, 64, 65, 254, 255, 256, 257))
    solid = sum(int(e.solid(3, 256).sum()) for e in expected)
    assert 0 < solid < sum(e.distinct for e in expected)
    check(gkc, k, specs, labels, amin=3, amax=256, histo_max=300)


@pytest.mark.parametrize("k", sb.K_CASES)
def test_split_levels_forced_deep(gkc, monkeypatch, k):
    """GKC_DEEP_BITS=2: two bits per split level make more levels than the four fixed launches; 4097, 8193 and 32769 keys in every pattern are all roots"""
    exact_sizes(monkeypatch, GKC_DEEP_BITS=2)
    specs, labels = sb.case(k, ("distinct", "one", "runs", "ends"), ns=sb.DEEP_SIZES)
    assert sb.roots(labels, sb.is_wide(k)) == len(labels) == 12
    check(gkc, k, specs, labels)


@pytest.mark.parametrize("k", [27, 47])
def test_integer_network_on_the_tagged_input(gkc, monkeypatch, k):
    """the two k whose keys the f64-tagged network orders, with GKC_NO_F64 on the integer network: the same records"""
    exact_sizes(monkeypatch)
    for pattern in ("distinct", "one", "runs"):
        specs, labels = sb.case(k, patterns_of(pattern))
        monkeypatch.delenv("GKC_NO_F64", raising=False)
        tagged, _ = check(gkc, k, specs, labels)
        monkeypatch.setenv("GKC_NO_F64", "1")
        integer, _ = check(gkc, k, specs, labels)
        assert integer == tagged, pattern


@pytest.mark.parametrize("k", [27, 30, 31])
@pytest.mark.parametrize("wb", [2, 3, 4])
def test_weighted_runs(gkc, monkeypatch, k, wb):
    """identical reads merged into weighted keys before the sort (GKC_DEDUPE=1): runs whose copies are just below, at and beyond what one merged record stands
    for with 2 / 3 / 4 weight bits. The sizes are not exact here (the partitions have sub-bucket bits): this is about the weighted sums."""
    monkeypatch.setenv("GKC_DEDUPE", "1"); monkeypatch.setenv("GKC_WEIGHT_BITS", str(wb)); monkeypatch.delenv("GKC_MAX_SUB_BITS", raising=False)
    specs = sb.weighted_specs(wb)
    _, stats = check(gkc, k, specs, [("weighted", sum(s)) for s in specs], seed=100 + wb)
    assert stats["dedupe_kmers_in"] > stats["dedupe_keys_out"] > 0, stats                 # the merge ran
