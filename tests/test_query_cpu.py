"""Expected values of the abundance queries (gkc.Counter.query_reads / query_kmers, gkc.Banks.query_reads), and their own check on the CPU.

The helper the GPU tests use (tests/test_gpu_query.py) builds ONE dict over oracle.gko.Dsk(...).part(d) of all datasets and looks every position of the queried reads
up with oracle.gko.kmers. Here that helper is checked against tests.util.naive_counts plus the solidity window — a statement of the semantics that shares nothing
with the oracle — and it asserts on the way that no k-mer occurs in two datasets (the routing k-mer -> minimizer -> dataset is a function)."""
import numpy as np
import pytest

from oracle import gko
from tests.util import CODE, naive_counts, revcomp_int, simple_repart, synth_reads

INF = 2 ** 31 - 1
EXTRA_READS = [b"A" * 60, b"ACAC" * 20, b"ACGTN" * 10, b"ACG", b""]


def freq_order_of(reads, m):
    """frequency order of the m-mers of the reads (RepartitionAlgorithm.cpp:311-492), as tests/test_gpu_parity.py makes it"""
    L = gko.lib()
    counts = np.zeros(4 ** m, np.uint32)
    for r in reads:
        L.gko_count_mmers(r, len(r), m, counts)
    freq = np.zeros(4 ** m, np.uint32)
    L.gko_freq_order_from_counts(m, counts, freq)
    return freq


def oracle_table(counted, k, m, parts, passes, rep, freq=None, amin=1, amax=INF):
    """-> ([(lo, hi, abundance) per dataset], {k-mer int: abundance} over all datasets); a k-mer in two datasets is an error"""
    bases, offs = gko.pack_reads(counted)
    d = gko.Dsk(bases, offs, k, m, parts, rep, nb_passes=passes, freq_order=freq, abundance_min=amin, abundance_max=amax)
    ds = [d.part(i) for i in range(parts * passes)]
    d.close()
    table = {}
    for i, (lo, hi, ab) in enumerate(ds):
        for a, b, c in zip(lo.tolist(), hi.tolist(), ab.tolist()):
            key = (b << 64) | a
            assert key not in table, "k-mer %x is in two datasets (the second: %d)" % (key, i)
            table[key] = c
    return ds, table


def canonical_per_position(queried, k):
    """-> (bases, offsets, [canonical k-mer int or None per base]): None where no k-mer starts (read too short there, or a character outside ACGTacgt in the window)"""
    bases, offs = gko.pack_reads(queried)
    can = [None] * len(bases)
    for r, o in zip(queried, offs[:-1].tolist()):
        km = gko.kmers(r, k)
        for i, (lo, hi, v) in enumerate(zip(km["can_lo"].tolist(), km["can_hi"].tolist(), km["valid"].tolist())):
            if v:
                can[o + i] = (hi << 64) | lo
    return bases, offs, can


def expected_abundance(queried, k, table):
    """-> (bases, offsets, int32[n_bases]): > 0 abundance, 0 valid k-mer not in the table, -1 no k-mer"""
    bases, offs, can = canonical_per_position(queried, k)
    exp = np.array([-1 if x is None else table.get(x, 0) for x in can], np.int32).reshape(-1)
    return bases, offs, exp


def naive_abundance(counted, queried, k, amin, amax):
    """the same array from the dictionary counter of tests/util.py: nothing of the oracle"""
    cnt = naive_counts(counted, k)
    out = []
    for r in queried:
        b = bytes(r)
        for i in range(len(b)):
            w = b[i:i + k]
            if len(w) < k or any(ch not in CODE for ch in w):
                out.append(-1); continue
            f = 0
            for ch in w:
                f = (f << 2) | CODE[ch]
            rc = revcomp_int(f, k)
            a = cnt.get(min(f, rc), 0)
            out.append(a if amin <= a <= amax else 0)
    return np.array(out, np.int32).reshape(-1)


@pytest.mark.parametrize("k,m,parts,passes,amin,amax", [(31, 8, 16, 3, 1, INF), (31, 8, 16, 1, 2, 5), (63, 10, 16, 2, 1, INF), (63, 10, 5, 1, 2, INF)])
def test_expected_value_helper_against_naive_counts(k, m, parts, passes, amin, amax):
    counted = synth_reads(60, 1500, read_len=100, seed=3, sub_rate=0.02, n_rate=0.01, ragged=True) + EXTRA_READS
    queried = counted[:30] + EXTRA_READS + synth_reads(10, 1500, read_len=100, seed=99, sub_rate=0)
    rep = simple_repart(m, parts)
    ds, table = oracle_table(counted, k, m, parts, passes, rep, amin=amin, amax=amax)
    assert len(ds) == parts * passes and sum(len(lo) for lo, _, _ in ds) == len(table) > 0
    bases, offs, exp = expected_abundance(queried, k, table)
    assert len(exp) == len(bases) == int(offs[-1])
    assert np.array_equal(exp, naive_abundance(counted, queried, k, amin, amax))
    assert (exp > 0).any() and (exp == 0).any() and (exp == -1).any()


def test_expected_value_helper_frequency_order():
    """the dataset a k-mer lies in changes with the minimizer order, the answer does not"""
    k, m, parts, passes = 21, 6, 7, 2
    counted = synth_reads(60, 1500, read_len=100, seed=3, sub_rate=0.02, ragged=True) + EXTRA_READS
    rep = simple_repart(m, parts)
    _, t_lexi = oracle_table(counted, k, m, parts, passes, rep)
    ds, t_freq = oracle_table(counted, k, m, parts, passes, rep, freq=freq_order_of(counted, m))
    assert t_lexi == t_freq
    assert np.array_equal(expected_abundance(counted, k, t_freq)[2], naive_abundance(counted, counted, k, 1, INF))
