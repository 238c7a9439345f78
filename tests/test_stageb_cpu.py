"""tests/stageb_inputs.py pinned on the CPU: the inputs of tests/test_gpu_stageb_sizes.py put exactly the intended number of k-mers into every partition, the
oracle counts them to the records the generator expects (which it computes without the oracle), and the runs patterns hold the rank positions and abundances
they are there for. A change to the generator that empties the GPU tests of their edges fails here."""
import numpy as np
import pytest

from oracle import gko
from tests import stageb_inputs as sb


def oracle_agrees(k, specs, labels, amin=1, amax=sb.INF, histo_max=10000, seed=None):
    reads, repart, expected = sb.exact_partitions(k, sb.M, specs, seed if seed is not None else k)
    assert len(reads) == sum(sum(s) for s in specs)
    assert all(len(r) == k for r in reads)
    bases, offs = gko.pack_reads(reads)
    ref = gko.Dsk(bases, offs, k, sb.M, len(specs), repart, abundance_min=amin, abundance_max=amax, histo_max=histo_max)
    for p, (spec, label, exp) in enumerate(zip(specs, labels, expected)):
        tag = sb.describe(label, k)
        assert (exp.distinct, exp.kmers) == (len(spec), sum(spec)), tag
        assert ref.part_stats(p)[0] == sum(spec), tag                      # exactly the intended k-mer total
        assert ref.part_records(p).tobytes() == exp.solid_records(amin, amax), tag
    assert np.array_equal(ref.histogram(), sb.total_histogram(expected, histo_max))
    assert ref.stats["kmers_nb_distinct"] == sum(e.distinct for e in expected)
    assert ref.stats["kmers_nb_solid"] == sum(int(e.solid(amin, amax).sum()) for e in expected)
    ref.close()
    return reads, expected


def test_size_list():
    s = sb.sizes()
    assert len(s) == 31 and len(set(s)) == 31 and sum(s) == 114512
    for wide in (False, True):
        cap1, cap2, cap3 = sb.caps(wide)
        for border in (64, 128, 256, 512, cap1, cap2, cap3, sb.caps(wide, 1024)[2], 8192, 32768):
            assert border in s and border + 1 in s, border
        assert set(sb.runs_sizes(wide)) >= {cap1, cap1 + 1, cap2, cap2 + 1, cap3, cap3 + 1}
    assert sb.runs_sizes(True) == [32, 33, 512, 513, 1024, 1025, 2048, 2049, 4097]


@pytest.mark.parametrize("wide", [False, True])
def test_runs_patterns_hold_their_edges(wide):
    """from the specs alone: rank positions and abundances of the runs patterns (check_runs_spec), and what the checks mean for the kernels' coordinates"""
    wave = 512 if wide else 1024
    every = set()
    for ends in (False, True):
        for n in sb.runs_sizes(wide) + list(sb.DEEP_SIZES):
            spec = sb.spec_runs(n, wide, ends)
            every |= sb.check_runs_spec(spec, n, wide, ends)
            runs = sb.run_layout(spec)
            assert all(a[1] < b[0] for a, b in zip(runs, runs[1:]))        # runs are disjoint and in rank order
            if n > 2 * wave + 2:                                           # the workgroup tier or beyond: every wave border below n - 2 is an edge
                for border in (wave, 2 * wave, 3 * wave):
                    if border <= n - 3:
                        assert any((l == border - 1) if ends else (f < border <= l) for f, l, _ in runs), (n, border)
    assert every >= set(sb.ABUNDANCES)
    # a run of 255 copies that ends on the last rank of the first wave of a workgroup sort
    n = sb.caps(wide)[2]
    assert (wave - 255, wave - 1, 255) in sb.run_layout(sb.spec_runs(n, wide, ends=True)) and sb.tier(n, wide) == "workgroup tier"


def test_tier_names():
    assert sb.tier(1024, False).startswith("first tier, 16") and sb.tier(1025, False) == "double-size wave network"
    assert sb.tier(2049, False) == "workgroup tier" and sb.tier(4097, False).startswith("split levels, small")
    assert sb.tier(2049, False, wg_max=1024).startswith("split levels") and sb.tier(2048, False, wg_max=1024) == "double-size wave network"
    assert sb.tier(512, True).startswith("first tier, 8") and sb.tier(1025, True) == "workgroup tier" and sb.tier(2049, True).startswith("split levels")
    assert sb.tier(8193, True).endswith("large launch") and sb.tier(32769, False).endswith("giant") and sb.tier(32768, False).endswith("large launch")
    assert sb.roots([("one", n) for n in sb.sizes()], False) == 6 and sb.roots([("one", n) for n in sb.sizes()], True) == 9
    assert sb.roots([("one", n) for n in sb.sizes()], False, 1024) == 9 and sb.roots([("one", n) for n in sb.sizes()], True, 1024) == 12


@pytest.mark.parametrize("pattern", ["distinct", "one", "runs"])
@pytest.mark.parametrize("k", sb.K_CASES)
def test_every_size_and_pattern_inputs(k, pattern):
    patterns = ("runs", "ends") if pattern == "runs" else (pattern,)
    specs, labels = sb.case(k, patterns)
    reads, expected = oracle_agrees(k, specs, labels)
    assert len(specs) == (18 if pattern == "runs" else 31)
    if pattern == "distinct":
        assert len(set(reads)) == len(reads) == 114512
    if pattern == "one":
        assert [e.distinct for e in expected] == [1] * 31 and [int(e.ab[0]) for e in expected] == sb.sizes()


@pytest.mark.parametrize("k", sb.K_CASES)
def test_solidity_and_deep_inputs(k):
    specs, labels = sb.case(k, ("runs", "ends"), extend=(2, 3, 299, 300, 301))
    oracle_agrees(k, specs, labels, amin=3, amax=256, histo_max=300)
    specs, labels = sb.case(k, ("distinct", "one", "runs", "ends"), ns=sb.DEEP_SIZES)
    oracle_agrees(k, specs, labels)


@pytest.mark.parametrize("k", [27, 30, 31])
@pytest.mark.parametrize("wb", [2, 3, 4])
def test_weighted_inputs(k, wb):
    specs = sb.weighted_specs(wb)
    oracle_agrees(k, specs, [("weighted", sum(s)) for s in specs], seed=100 + wb)


def test_results_are_cached_and_deterministic():
    specs, _ = sb.case(27, ("one",))
    a = sb.exact_partitions(27, sb.M, specs, 27); b = sb.exact_partitions(27, sb.M, [list(s) for s in specs], 27)
    assert a is b
    sb._exact_partitions.cache_clear()
    c = sb.exact_partitions(27, sb.M, specs, 27)
    assert c[0] == a[0] and np.array_equal(c[1], a[1]) and [e.records for e in c[2]] == [e.records for e in a[2]]
    d = sb.exact_partitions(27, sb.M, specs, 28)
    assert d[0] != a[0]
