"""Inputs for Stage A (csrc/gkc_scan.hip) with a read start, an N, a short read or the end of the push at a stated offset from a tile border, on the descriptor
budget of a tile, and beyond one trip of the read-start kernel and of the persistent grid. Bases are one random ACGT array and reads are offsets into it, both built
with numpy. tests/test_input_sizes_cpu.py asserts every claimed position, tests/test_gpu_input_sizes.py compares the device with the oracle."""
import functools
from collections import namedtuple

import numpy as np

SCAN_TILE = 8192                 # csrc/gkc_common.hpp SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD: k-mer start positions per workgroup and trip
SCAN_PER_THREAD = 16             # csrc/gkc_common.hpp SCAN_PER_THREAD
SCAN_HALO = 64                   # csrc/gkc_common.hpp SCAN_HALO_WORDS = 4 words of 16 bases read beyond the tile
DESC_PER_TILE = 1280             # csrc/gkc_scan.hip gkc_scan_push: desc_cap_wg = tiles_per_wg * (SCAN_TILE * 5 / 32) record descriptors; one more and the emit pass re-scans
MARK_ONE_TRIP = 4096 * 256       # csrc/gkc_scan.hip gkc_scan_push: k_mark_read_starts runs at most 4096 workgroups of 256 threads; more read offsets take its grid-stride loop
SCAN_GRID_MAX = 256 * 2          # csrc/gkc_scan.hip gkc_scan_push: 160 KB / 64 KB of LDS = 2 persistent workgroups on each of 256 compute units; more tiles take the tile loop with prefetch

# (k, m, frequency order?): one- and two-word records, k on both sides of 32, the smallest k, the widest window
KM_CASES = ((5, 3, False), (31, 10, False), (32, 10, False), (33, 9, False), (63, 10, False), (31, 8, True))
PARTS = 4
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# bases, offsets: the whole pass as the oracle sees it; pushes: (first read, last read + 1) of every push; claims: (d, position) per phase
Construction = namedtuple("Construction", "bases offsets pushes claims")


def phases(k):
    return tuple(range(-(k + 1), k + 2))


def _random_bases(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)]


def _borders(k):
    """-> (n_bases, positions, claims): position SCAN_TILE * (i + 1) + d for the i-th d of phases(k), one border per phase"""
    ph = np.array(phases(k), dtype=np.int64)
    pos = SCAN_TILE * (np.arange(len(ph), dtype=np.int64) + 1) + ph
    return SCAN_TILE * (len(ph) + 1), pos, list(zip(ph.tolist(), pos.tolist()))


def _offsets(cuts, n):
    return np.concatenate([[0], np.asarray(cuts, dtype=np.int64), [n]]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def read_boundary_at(k):
    """a. a read ends and the next one starts at every claimed position; one push"""
    n, pos, claims = _borders(k)
    offs = _offsets(pos, n)
    return Construction(_random_bases(100 + k, n), offs, ((0, len(offs) - 1),), claims)


@functools.lru_cache(maxsize=None)
def letter_at(k, what):
    """b. one long read with an 'N' (what = "N") or a lower-case base (what = "lower") at every claimed position; one push"""
    n, pos, claims = _borders(k)
    bases = _random_bases(200 + k, n)
    bases[pos] = ord("N") if what == "N" else bases[pos] | 0x20
    return Construction(bases, _offsets([], n), ((0, 1),), claims)


@functools.lru_cache(maxsize=None)
def short_read_at(k, length):
    """c. a read of `length` bases starts at every claimed position (the reads between are long); one push"""
    n, pos, claims = _borders(k)
    offs = _offsets(np.stack([pos, pos + length], axis=1).reshape(-1), n)
    return Construction(_random_bases(300 + k + length, n), offs, ((0, len(offs) - 1),), claims)


@functools.lru_cache(maxsize=None)
def push_end_at(k):
    """d. successive pushes of one pass, one read each, of SCAN_TILE * t + d bases for t = 1, 2 and every d: the claims are (d, bases of the push)"""
    lens = np.array([SCAN_TILE * t + d for t in (1, 2) for d in phases(k)], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    claims = [(d, SCAN_TILE * t + d) for t in (1, 2) for d in phases(k)]
    return Construction(_random_bases(400 + k, int(lens.sum())), offs, tuple((i, i + 1) for i in range(len(lens))), claims)


CONSTRUCTIONS = ("boundary", "N", "lower", "short-1", "short+0", "short+1", "push_end")


def build(name, k):
    if name == "boundary":
        return read_boundary_at(k)
    if name in ("N", "lower"):
        return letter_at(k, name)
    if name.startswith("short"):
        return short_read_at(k, k + int(name[5:]))
    assert name == "push_end"
    return push_end_at(k)


BUDGET_K, BUDGET_M = 5, 3
BUDGET_READS = (DESC_PER_TILE - 1, DESC_PER_TILE, DESC_PER_TILE + 1)


@functools.lru_cache(maxsize=None)
def descriptor_budget(n_reads):
    """e. one push of exactly one tile: n_reads reads of exactly k = 5 bases (one k-mer, so one record, each), then one read of N's to the end of the tile"""
    bases = _random_bases(500 + n_reads, SCAN_TILE)
    bases[BUDGET_K * n_reads:] = ord("N")
    offs = _offsets(BUDGET_K * np.arange(1, n_reads + 1), SCAN_TILE)
    return Construction(bases, offs, ((0, n_reads + 1),), [])


MANY_K, MANY_M, MANY_READS, MANY_LEN = 21, 8, (1 << 20) + 5, 24


@functools.lru_cache(maxsize=None)
def many_reads():
    """f. more read offsets than one trip of k_mark_read_starts marks and more tiles (3073) than the persistent grid holds; one push"""
    n = MANY_READS * MANY_LEN
    offs = (np.arange(MANY_READS + 1, dtype=np.uint64) * np.uint64(MANY_LEN))
    return Construction(_random_bases(600, n), offs, ((0, MANY_READS),), [])


def push_slices(con):
    """-> [(bases of the push, its offsets from 0)]"""
    out = []
    for r0, r1 in con.pushes:
        b0, b1 = int(con.offsets[r0]), int(con.offsets[r1])
        out.append((con.bases[b0:b1], con.offsets[r0:r1 + 1] - con.offsets[r0]))
    return out
