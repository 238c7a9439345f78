"""Deterministic inputs that put an exact number of keys into a Stage-B sub-bucket (csrc/gkc_count.hip), with the sorted rank of every key known in advance.

With GKC_MAX_SUB_BITS=0 a partition is one sub-bucket, with GKC_DEDUPE=0 a read of exactly k nucleotides is one key of weight 1: a partition that receives n such
reads is a sub-bucket of n keys. exact_partitions() routes k-mer-long reads to partitions through a repartition table built from the minimizers of the reads
themselves and gives the i-th smallest canonical k-mer of a partition the i-th multiplicity of its spec, so a spec states which ranks a run of equal keys covers.

The routing uses the oracle's minimizers (a wrong minimizer would send a read to another partition: tests/test_stageb_cpu.py pins that against oracle.gko.Dsk);
the expected records, totals and histograms are computed from the emitted reads with tests/util.naive_counts and a plain sort, independent of oracle and device.
A plain helper module: no fixtures, no test."""
import collections
import functools
import heapq

import numpy as np

from oracle import gko
from tests.util import naive_counts

INF = 2 ** 31 - 1
M = 8                                           # minimizer length of every case: 65536 table entries to hand out
K_CASES = (27, 31, 47, 63)                      # 8-byte keys f64-tagged / integer network, 16-byte keys f64-tagged / integer network (no sub-bucket bits)

_CODES = bytes.maketrans(b"ACTG", b"0123")      # the nucleotide code of tests/util.CODE as base-4 digits
_COMPLEMENT = bytes.maketrans(b"ACTG", b"TGAC")


def is_wide(k):
    return k > 31


# ------------------------------------------------------------------------------------------------ sizes and tiers
def sizes():
    """every power of two from 64 to 8192 with its two neighbours (the tier borders are among them whichever power of two a constant moves to), the smallest
    sizes, and the giant border"""
    return [1, 2, 3, 4, 5] + [2 ** j + d for j in range(6, 14) for d in (-1, 0, 1)] + [32768, 32769]


RUNS_SIZES = (64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 8193)
DEEP_SIZES = (4097, 8193, 32769)


def runs_sizes(wide):
    """the sizes of the runs patterns: both sides of every tier border (16-byte keys: half of each, rounded up, which are their borders)"""
    return [(n + 1) // 2 for n in RUNS_SIZES] if wide else list(RUNS_SIZES)


def caps(wide, wg_max=None):
    """(first tier, double-size wave network, workgroup tier) capacities in keys; wg_max: GKC_WG_MAX"""
    cap1, cap2, c1 = (512, 1024, 2048) if wide else (1024, 2048, 4096)
    return cap1, cap2, max(cap2, min(wg_max, c1) if wg_max else c1)


def tier(n, wide, wg_max=None):
    """the name of the tier a sub-bucket of n keys takes (for messages)"""
    cap1, cap2, cap3 = caps(wide, wg_max)
    if n <= cap1:
        return "first tier, %d keys per lane" % keys_per_lane(n, wide)
    if n <= cap2:
        return "double-size wave network"
    if n <= cap3:
        return "workgroup tier"
    return "split levels" + (", giant" if n > 32768 else ", small launch" if n <= 8192 else ", large launch")


def keys_per_lane(n, wide):
    """keys per lane of the network that sorts a sub-bucket of n keys which is not split (wave_sort_dispatch, k_wave_sort_big, k_wg_sort)"""
    cap1, cap2, _ = caps(wide)
    if n <= cap1:
        return next(kpl for kpl in (1, 2, 4, 8, 16) if n <= 64 * kpl)
    return (16 if wide else 32) if n <= cap2 else (8 if wide else 16)


def roots(labels, wide, wg_max=None):
    """partitions that go to the split levels: what gkc_stats.oversize_buckets counts"""
    return sum(1 for _, n in labels if n > caps(wide, wg_max)[2])


# ------------------------------------------------------------------------------------------------ patterns
ABUNDANCES = (62, 63, 64, 65, 254, 255, 256, 257)          # around HIST_LDS = 64 and around the one-byte escape at 255
LANE_KEYS = (1, 2, 4, 8, 16, 32)


def spec_distinct(n):
    return (1,) * n


def spec_one(n):
    return (n,)


def spec_runs(n, wide, ends=False):
    """multiplicities, in ascending order of the k-mers, that total n and make runs of equal keys which cover ranks 0-1 and n-2 .. n-1, end on / one before /
    one after a lane's last rank for 1 .. 32 keys per lane, straddle every wave border of the workgroup tier (ends: END on the last rank of the wave, with 255,
    256 and 254 copies) and have the abundances around 64 and 255 as far as n has room for them; every other rank is a k-mer seen once"""
    wave = 512 if wide else 1024
    taken = np.zeros(n, bool); runs = {}

    def place(first, length):
        if first < 0 or first + length > n or taken[first:first + length].any():
            return False
        taken[first:first + length] = True; runs[first] = length
        return True

    def place_ending(kpl, residue, length, lo):
        """the first free place at or after rank lo whose last rank is residue modulo kpl -> the rank behind it, or lo"""
        for last in range(lo + length - 1, n):
            if last % kpl == residue % kpl and place(last - length + 1, length):
                return last + 1
        return lo

    assert n >= 8 and place(0, 2) and place(n - 2, 2)
    for i, border in enumerate((wave, 2 * wave, 3 * wave)):
        if border <= n - 3:
            assert place(border - (255, 256, 254)[i], (255, 256, 254)[i]) if ends else place(border - 1, 2)
    lo = 2
    for kpl in LANE_KEYS:
        for j, residue in enumerate((kpl - 1, kpl - 2, 0)):                # on, one before, one after the lane's last rank
            lo = place_ending(kpl, residue, 2 + (j + kpl) % 2, lo)
    for a in (255, 64, 63, 254, 256, 65, 62, 257):
        if a not in runs.values():
            place_ending(1, 0, a, 0)
    spec = []; r = 0
    while r < n:
        spec.append(runs.get(r, 1)); r += runs.get(r, 1)
    assert sum(spec) == n
    return tuple(spec)


def run_layout(spec):
    """-> [(first rank, last rank, multiplicity)] of the k-mers seen more than once, with one key of weight 1 per read"""
    out = []; r = 0
    for c in spec:
        if c > 1:
            out.append((r, r + c - 1, c))
        r += c
    return out


def check_runs_spec(spec, n, wide, ends=False):
    """the rank positions and abundances the runs patterns promise, from the spec alone"""
    runs = run_layout(spec); lasts = {l for _, l, _ in runs}; mult = {c for _, _, c in runs}
    tag = ("runs", n, "ends" if ends else "straddles")
    assert sum(spec) == n, tag
    assert runs[0][:2] == (0, 1) and runs[-1][:2] == (n - 2, n - 1), tag
    wave = 512 if wide else 1024
    for i, border in enumerate((wave, 2 * wave, 3 * wave)):
        if border <= n - 3:
            if ends:
                assert (border - (255, 256, 254)[i], border - 1, (255, 256, 254)[i]) in runs, tag + (border,)
            else:
                assert any(f < border <= l for f, l, _ in runs), tag + (border,)
    if ends and n > 2 * wave:
        assert (wave - 255, wave - 1, 255) in runs, tag                    # 255 copies that end on the last rank of the workgroup tier's first wave
    for kpl in (LANE_KEYS if n >= 512 else (keys_per_lane(n, wide),)):
        for residue in (kpl - 1, kpl - 2, 0):
            assert any(l % kpl == residue % kpl for l in lasts), tag + (kpl, residue)
    if n >= 512:
        assert 255 in mult, tag
    if n >= 2048:
        assert mult >= set(ABUNDANCES), tag
    return mult


def case(k, patterns, ns=None, extend=()):
    """-> (specs, labels): one partition per pattern and size; labels[p] = (pattern, n) with n the keys of the partition. `extend`: multiplicities appended
    to a copy of every runs pattern ("runs+", "ends+": n grows by their sum)"""
    wide = is_wide(k)
    specs = []; labels = []
    for pat in patterns:
        for n in (ns or (runs_sizes(wide) if pat in ("runs", "ends") else sizes())):
            if pat in ("runs", "ends"):
                s = spec_runs(n, wide, ends=pat == "ends")
                check_runs_spec(s, n, wide, ends=pat == "ends")
            else:
                s = {"distinct": spec_distinct, "one": spec_one}[pat](n)
            specs.append(s); labels.append((pat, n))
            if extend and pat in ("runs", "ends"):
                specs.append(s + tuple(extend)); labels.append((pat + "+", n + sum(extend)))
    if any(p in ("runs", "ends") for p in patterns) and ns is None:
        seen = set().union(*[{c for c in s if c > 1} for s, (pat, _) in zip(specs, labels) if pat in ("runs", "ends")])
        assert seen >= set(ABUNDANCES), sorted(seen)
    return tuple(specs), tuple(labels)


def weighted_specs(wb):
    """partitions for the record deduplication: k-mers seen as often as one merged record can stand for with wb weight bits (2^wb, or 2^wb - 1 when two top bits
    of the key are dropped), once less and once more, twice that, beyond one byte and far beyond, between k-mers seen once; in every order"""
    w = 1 << wb
    mults = (w - 1, w, w + 1, 2 * w - 1, 2 * w + 1, 255, 256, 600)
    apart = tuple(c for x in mults for c in (x, 1, 1))
    return (apart + (1,) * 300, tuple(reversed(mults)), (1,) * 40 + (600,), (1,) * 3000 + mults + (1,) * 500 + tuple(reversed(mults)))


def describe(label, k, wg_max=None):
    return "k=%d %s n=%d (%s)" % (k, label[0], label[1], tier(label[1], is_wide(k), wg_max))


# ------------------------------------------------------------------------------------------------ the generator
class Expected:
    """what one partition must hold: keys (ascending canonical k-mers, Python ints), ab (their abundances), distinct, kmers"""

    def __init__(self, keys, ab, wide):
        self.keys = keys; self.ab = np.asarray(ab, dtype=np.int64); self.wide = wide
        self.distinct = len(keys); self.kmers = int(self.ab.sum())
        self.records = self.solid_records(1, INF)

    def solid(self, amin, amax):
        return (self.ab >= amin) & (self.ab <= amax)                       # a closed interval

    def solid_records(self, amin, amax):
        """the Count{value, abundance} memory layout of the solid k-mers: 16 bytes (k <= 31) or 32 (k <= 63), pad bytes zero"""
        keep = self.solid(amin, amax)
        r = np.zeros((int(keep.sum()), 4 if self.wide else 2), np.uint64)
        keys = [x for x, ok in zip(self.keys, keep.tolist()) if ok]
        r[:, 0] = np.array([x & (2 ** 64 - 1) for x in keys], np.uint64)
        if self.wide:
            r[:, 1] = np.array([x >> 64 for x in keys], np.uint64)
        r[:, 2 if self.wide else 1] = self.ab[keep].astype(np.uint64)
        return r.tobytes()

    def histogram(self, histo_max=10000):
        """the partition's contribution: bin min(abundance, histo_max) per distinct k-mer"""
        return np.bincount(np.minimum(self.ab, histo_max), minlength=histo_max + 1).astype(np.uint64)


def canonical(read):
    """canonical k-mer of a k-mer-long read as an integer (the smaller of the two strands in the code A C T G = 0 1 2 3)"""
    return min(int(read.translate(_CODES), 4), int(read[::-1].translate(_COMPLEMENT).translate(_CODES), 4))


def exact_partitions(k, m, specs, seed):
    """-> (reads, repart, expected): k-mer-long reads in a seeded shuffle, half of them reverse complements, whose canonical k-mers are all distinct across
    partitions; partition p receives len(specs[p]) distinct k-mers, the i-th smallest of them specs[p][i] times. Cached per argument set: do not modify."""
    return _exact_partitions(k, m, tuple(tuple(int(c) for c in s) for s in specs), seed)


@functools.lru_cache(maxsize=None)
def _exact_partitions(k, m, specs, seed):
    rng = np.random.default_rng(seed)
    quota = [len(s) for s in specs]
    assert all(q > 0 and min(s) > 0 for q, s in zip(quota, specs)) and len(specs) < 65536
    n_pool = max(6 * sum(quota), 40000)
    pool = np.frombuffer(b"ACTG", np.uint8)[rng.integers(0, 4, n_pool + k - 1)].tobytes()
    mins, valid = gko.minimizers(pool, k, m)
    assert len(mins) == n_pool and valid.all()
    # the table, from the pool's own minimizer histogram: the most frequent value goes to the partition that still lacks the most k-mers, until none lacks any
    freq = np.bincount(mins, minlength=4 ** m)
    lacking = [(-q, p) for p, q in enumerate(quota)]
    heapq.heapify(lacking)
    repart = np.zeros(4 ** m, np.uint16)
    for value in np.argsort(-freq, kind="stable").tolist():
        need, p = lacking[0]
        if need >= 0 or freq[value] == 0:
            break
        repart[value] = p
        heapq.heapreplace(lacking, (need + int(freq[value]), p))
    assert lacking[0][0] >= 0, "the pool is short of k-mers for partition %d (k = %d)" % (lacking[0][1], k)
    part_of = repart[mins]
    order = np.argsort(part_of, kind="stable")
    first = np.searchsorted(part_of[order], np.arange(len(specs) + 1))
    fwd = []; rev = []; copies = []; where = {}
    for p, spec in enumerate(specs):
        at = order[first[p]: first[p] + quota[p]].tolist()
        assert len(at) == quota[p] and first[p] + quota[p] <= first[p + 1], (p, quota[p])          # every quota is met exactly
        mers = sorted((canonical(pool[i:i + k]), pool[i:i + k]) for i in at)
        for (value, read), c in zip(mers, spec):
            assert value not in where, "a k-mer twice in the pool"
            where[value] = p
            fwd.append(read); rev.append(read[::-1].translate(_COMPLEMENT)); copies.append(c)
    which = np.repeat(np.arange(len(fwd)), copies)
    which = which[rng.permutation(len(which))]
    flip = rng.random(len(which)) < 0.5
    reads = [rev[i] if f else fwd[i] for i, f in zip(which.tolist(), flip.tolist())]
    # the expectation, from the reads alone: the naive counter on every distinct read, times its copies
    counts = {}
    for read, c in collections.Counter(reads).items():
        (value, one), = naive_counts([read], k).items()
        assert one == 1
        counts[value] = counts.get(value, 0) + c
    assert counts.keys() == where.keys()
    per_part = [[] for _ in specs]
    for value, c in counts.items():
        per_part[where[value]].append((value, c))
    expected = []
    for p, spec in enumerate(specs):
        pairs = sorted(per_part[p])
        assert tuple(c for _, c in pairs) == spec, p                       # the i-th smallest k-mer has the i-th multiplicity: ranks are as the spec says
        expected.append(Expected([v for v, _ in pairs], [c for _, c in pairs], is_wide(k)))
    return reads, repart, tuple(expected)


def total_histogram(expected, histo_max=10000):
    h = np.zeros(histo_max + 1, np.uint64)
    for e in expected:
        h += e.histogram(histo_max)
    return h
