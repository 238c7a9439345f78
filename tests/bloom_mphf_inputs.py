"""Inputs that put the Bloom filter (csrc/gkc_bloom.hip) and the MPHF (csrc/gkc_mphf.hip) on the borders of their own constants, with the oracle's answer to each.

Bloom: array sizes on both sides of a 2^20-bit region border (a last region that holds no item and receives its neighbour's spill only, one that owns 1 / 100 positions,
an array that ends on the border, the sizes whose total is a power of two), 1 and 10 hash functions, the smallest k and the first 16-byte keys. MPHF: key counts whose
level-0 array is 448 / 512 bits (one / two rank samples) and 2^19 / 2^19 + 64 bits (one region / a second region of one word), and 8191 / 8192 / 8193 keys (the chunk of
the flag scan). Abundances on every border of the discretisation table of MapMPHF. Results that lie in 1, 2-16 or >= 17 device arrays.

Expected values are the oracle's (oracle/gko.py), computed once per case and shared by tests/test_bloom_mphf_cpu.py (which pins that every input reaches its edge)
and tests/test_gpu_bloom_mphf_sizes.py: the arrays are read-only. A plain helper module: no fixtures, no test."""
import functools
import struct
import types

import numpy as np

from oracle import gko
from tests.util import revcomp_int, simple_repart, synth_reads

INF = 2 ** 31 - 1
R = 1 << 20                                     # BR_BITS: bits of a Bloom region
COHERENT = 2 * 4096                             # what the block-coherent kinds add to the size asked for (Bloom.hpp:437-441)
REACH = 12 + 4095 + 1                           # bits from a root position that an item of a coherent kind can set: cano2 <= 13 stays below it, offsets <= 4095
MR = 1 << 19                                    # MR_BITS: bits of an MPHF region
KINDS = ("basic", "cache", "neighbor")


# ------------------------------------------------------------------------------------------------ keys
def random_keys(k, n, seed):
    """n distinct random k-mers (Python ints, in drawing order)"""
    rng = np.random.default_rng(seed)
    out = []; seen = set()
    while len(out) < n:
        raw = np.frombuffer(rng.bytes(16 * (n - len(out) + 16)), dtype=np.uint64).reshape(-1, 2)
        for a, b in raw.tolist():
            x = (a | (b << 64)) & (4 ** k - 1)
            if x not in seen and len(out) < n:
                seen.add(x); out.append(x)
    return out


def with_neighbours(keys, k, n, seed):
    """replaces the last n keys by right neighbours of the first n (the key shifted by one nucleotide, a random one appended): contains8 of either has a bit to find"""
    nt = np.random.default_rng(seed).integers(0, 4, n).tolist()
    out = list(keys[: len(keys) - n]) + [((x << 2) | c) & (4 ** k - 1) for x, c in zip(keys[:n], nt)]
    assert len(set(out)) == len(out) == len(keys)
    return out


def near_palindrome_core(k):
    """a k-mer whose (k-2)-mer core is its own reverse complement (k even); with k odd no such core exists (its middle nucleotide would be its own complement):
    the core then differs from its reverse complement in the middle nucleotide alone"""
    half = (k - 2) // 2
    left = int(np.random.default_rng(k).integers(0, 4 ** half))
    if (k - 2) % 2 == 0:
        core = (left << (2 * half)) | revcomp_int(left, half)
        assert revcomp_int(core, k - 2) == core
    else:
        core = (left << (2 * half + 2)) | (1 << (2 * half)) | revcomp_int(left, half)
        assert revcomp_int(core, k - 2) ^ core == 2 << (2 * half)
    return (3 << (2 * (k - 1))) | (core << 2) | 1


def _frozen(a):
    a = np.ascontiguousarray(a); a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ A. Bloom array sizes on region borders
A_KEYS, A_OTHERS, A_HASH, A_SPLIT = 30000, 2000, 7, 12345          # (the two insert calls part at an odd index)
A_K = (31, 33)
A_COHERENT_SIZES = (R - 8192, R - 8192 + 1, R - 100, R, R + 1, R + 100, 2 * R - 8192, 2 * R - 8192 - 1)
A_BASIC_SIZES = (R - 100, R, R + 100, 2 * R - 1, 2 * R)
A_CASES = [(kind, t) for kind in ("cache", "neighbor") for t in A_COHERENT_SIZES] + [("basic", t) for t in A_BASIC_SIZES]
A_GATHER_SIZE = R + 100                                            # the neighbor size whose contains8 is repeated with GKC_BLOOM_GATHER


def geometry(kind, tai_bits):
    """(tai, reduced_tai, pow2, nchar, n_regions) as BloomContainer / BloomCacheCoherent size an array (Bloom.hpp:185-198, 437-441) and as the region build cuts it"""
    tai = tai_bits + (COHERENT if kind != "basic" else 0)
    nchar = 1 + tai // 8
    pow2 = tai & (tai - 1) == 0
    if pow2:
        tai -= 1
    reduced = tai - COHERENT if kind != "basic" else tai
    return tai, reduced, pow2, nchar, (tai + 1 + R - 1) // R


def last_region_reachable(kind, tai_bits):
    """can an item set a bit in the last region? (R - 8192 + 1: the array is two bits longer than a region, and no item reaches beyond R - 4085)"""
    tai, reduced, _, _, n_regions = geometry(kind, tai_bits)
    top = reduced - 1 + (REACH - 1 if kind != "basic" else 0)
    return top >= (n_regions - 1) * R


@functools.lru_cache(maxsize=None)
def a_keys(k):
    """-> (keys, others): 30000 random k-mers, the last 1000 of them right neighbours of the first 1000, and 2000 k-mers that are no keys"""
    keys = random_keys(k, A_KEYS + A_OTHERS, 1000 + k)
    return tuple(with_neighbours(keys[:A_KEYS], k, A_OTHERS // 2, k)), tuple(keys[A_KEYS:])


def a_queried8(k):
    """the first 1000 keys (a right neighbour of each is a key), the last 1000 (a left neighbour is) and the 2000 others"""
    keys, others = a_keys(k)
    return keys[: A_OTHERS // 2] + keys[-(A_OTHERS // 2):] + others


def set_bits(array, first, last):
    """number of set bits of a Bloom byte array in the bit range [first, last)"""
    last = min(last, 8 * len(array))
    if first >= last:
        return 0
    bits = np.unpackbits(array[first // 8: (last + 7) // 8], bitorder="little")
    return int(bits[first - first // 8 * 8: last - first // 8 * 8].sum())


def _bloom_expectation(kind, tai_bits, nb_hash, k, inserted, queried, queried8):
    ob = gko.Bloom(kind, tai_bits, nb_hash, k)
    ob.insert(inserted)
    e = types.SimpleNamespace(kind=kind, tai_bits=tai_bits, nb_hash=nb_hash, k=k, nbytes=int(ob.nbytes), bitsize=int(ob.bitsize), array=_frozen(ob.array()),
                              contains=_frozen(ob.contains(queried)), contains8=_frozen(ob.contains8(queried8)) if kind == "neighbor" else None)
    return e


@functools.lru_cache(maxsize=None)
def a_expected(kind, tai_bits, k):
    """the oracle's filter of the 30000 keys: nbytes, bitsize, array, contains over keys + others, contains8 (neighbor) over a_queried8"""
    keys, others = a_keys(k)
    return _bloom_expectation(kind, tai_bits, A_HASH, k, keys, keys + others, a_queried8(k))


# ------------------------------------------------------------------------------------------------ B. nb_hash and k edges
B_HASHES, B_HASH_K, B_HASH_KEYS = (1, 10), (31, 63), 5000
B_SMALL_K, B_WIDE_K, B_EDGE_HASH = (3, 4, 5), (32, 33), 4


@functools.lru_cache(maxsize=None)
def b_hash_expected(kind, nb_hash, k):
    keys = random_keys(k, B_HASH_KEYS + 2000, 2000 + k)
    inserted, others = tuple(with_neighbours(keys[:B_HASH_KEYS], k, 1000, k)), tuple(keys[B_HASH_KEYS:])
    queried8 = inserted[:1000] + inserted[-1000:] + others
    e = _bloom_expectation(kind, B_HASH_KEYS * 11, nb_hash, k, inserted, inserted + others, queried8)
    e.inserted, e.queried, e.queried8 = inserted, inserted + others, queried8
    return e


def hand_made_keys(k):
    """all zero, all one, the two values around the 64-bit word border, and the key of near_palindrome_core"""
    return [0, 4 ** k - 1, 1 << 64, (1 << 64) - 1, near_palindrome_core(k)]


@functools.lru_cache(maxsize=None)
def b_k_expected(kind, k):
    """k in 3 .. 5: every value of 4^k queried, every second one inserted (a 1- to 3-mer core). k = 32, 33: 3000 random keys and the hand-made ones inserted, these and
    1000 others queried. 11 bits per inserted key, 4 hash functions."""
    if k in B_SMALL_K:
        queried = tuple(range(4 ** k)); inserted = queried[::2]
    else:
        keys = random_keys(k, 4000, 3000 + k)
        hand = sorted({x for x in hand_made_keys(k) if x < 4 ** k})           # (k = 32: 2^64 is no 32-mer, and 2^64 - 1 is the all-one key)
        rest = [x for x in keys if x not in hand]
        inserted = tuple(with_neighbours(rest[:3000], k, 500, k) + hand); queried = inserted + tuple(rest[3000:])
    e = _bloom_expectation(kind, 11 * len(inserted), B_EDGE_HASH, k, inserted, queried, queried)
    e.inserted, e.queried, e.queried8 = inserted, queried, queried
    return e


# ------------------------------------------------------------------------------------------------ C. results spread over several device arrays
C_M, C_PARTS = 10, 4
C_CLASSES = {"one": (1, 1), "few": (2, 16), "many": (17, None)}     # arrays the solid records lie in: the class a configuration is meant for
C_PASSES = {"one": 1, "few": 4, "many": 24}                         # a pass is a Stage-B batch of its own, its records an array of their own
C_CASES = [(31, "one"), (31, "few"), (31, "many"), (63, "many")]


@functools.lru_cache(maxsize=None)
def c_input(k):
    """-> (bases, offsets, repart, keys, abundances): reads of a 3000-nt genome at 20x, and the solid k-mers (abundance >= 2) of a one-pass oracle count, ascending"""
    reads = synth_reads(600, 3000, 100, seed=40 + k, n_rate=0.001)
    bases, offs = gko.pack_reads(reads)
    rep = simple_repart(C_M, C_PARTS)
    ref = gko.Dsk(bases, offs, k, C_M, C_PARTS, rep, abundance_min=2)
    solid = ref.all_counts(); ref.close()
    keys = tuple(sorted(solid))
    return _frozen(bases), _frozen(offs), _frozen(rep), keys, tuple(solid[x] for x in keys)


def count_arrays(datasets, rec_bytes):
    """datasets: (device pointer, n_solid) in dataset order -> number of device arrays: a dataset joins the one before when it starts where that one ends"""
    n = 0; end = None
    for p, ns in datasets:
        if not ns:
            continue
        if end is None or p != end:
            n += 1
        end = p + ns * rec_bytes
    return n


def abundance_map_of(keys, abundances, k):
    """-> (oracle MPHF of the keys in this order, the map MPHFAlgorithm::populate fills, abundances at or above the table's last entry)"""
    om = gko.Mphf(list(keys), k)
    want = np.zeros(len(keys), np.uint8)
    want[om.lookup(keys).astype(np.int64)] = [gko.abundance_index(a) for a in abundances]
    return om, want, sum(1 for a in abundances if a >= ABUNDANCE_TABLE[-2])


# ------------------------------------------------------------------------------------------------ D. MPHF exact sizes
D_SIZES = (149, 150, 8191, 8192, 8193, 174762, 174763)
D_CASES = [(31, n) for n in D_SIZES] + [(63, n) for n in (150, 8193, 174763)]
D_LEVEL0 = {149: 448, 150: 512, 174762: MR, 174763: MR + 64}        # bits of the level-0 array the size is there for
D_BUILDS = ({"GKC_MPHF_REGIONS_MIN": "1"}, {"GKC_MPHF_REGIONS": "0"}, {"GKC_MPHF_ORDERED": "1"})


def d_sample(n):
    """indices of the keys whose codes are compared: all of them up to 8193 keys, else every 8th and the first and last 600"""
    if n <= 8193:
        return list(range(n))
    return sorted(set(range(0, n, 8)) | set(range(600)) | set(range(n - 600, n)))


@functools.lru_cache(maxsize=None)
def d_expected(k, n):
    """n distinct random k-mers, ascending, 500 others, and the oracle's BooPHF of the keys: its save() stream, the codes of the sample and of the others"""
    drawn = random_keys(k, n + 500, 5000 + k * 7 + n)
    keys = sorted(drawn[:n]); others = drawn[n:]
    om = gko.Mphf(keys, k)
    sample = [keys[i] for i in d_sample(n)]
    return types.SimpleNamespace(k=k, n=n, keys=keys, others=others, sample=sample, stream=_frozen(om.save()),
                                 codes=_frozen(om.lookup(sample)), other_codes=_frozen(om.lookup(others)))


def mphf_levels(stream):
    """the stream of mphf::save (layout: gkc_mphf_save) -> (gamma, nelem, lastbitsetrank, [(domain, nchar, nranks) per level], n_final)"""
    gamma, nb_levels, last, nelem = struct.unpack_from("<diQQ", stream, 0)
    pos = 28; levels = []
    for _ in range(nb_levels):
        domain, nchar = struct.unpack_from("<QQ", stream, pos); pos += 16 + 8 * nchar
        nranks, = struct.unpack_from("<Q", stream, pos); pos += 8 + 8 * nranks
        levels.append((domain, nchar, nranks))
    n_final, = struct.unpack_from("<Q", stream, pos)
    return gamma, nelem, last, levels, n_final


# ------------------------------------------------------------------------------------------------ E. abundance table borders
ABUNDANCES = (1, 2, 69, 70, 71, 72, 73, 99, 100, 101, 102, 109, 110, 111, 499, 500, 501, 519, 520, 999, 1000, 1001, 1099, 1100, 4999, 5000, 5199, 5200,
              9999, 10000, 10999, 11000, 48999, 49000, 49999, 50000, 50001, 60000)
E_K, E_M, E_PARTS = (21, 33), 8, 4


def _abundance_table():
    """MapMPHF::initDiscretizationScheme (MapMPHF.hpp:96-145), restated: 70 steps of 1, 15 of 2, 40 of 10, 25 of 20, 40 of 100, 25 of 200, 40 of 1000; the last
    entry twice"""
    t = [0]
    for count, step in ((70, 1), (15, 2), (40, 10), (25, 20), (40, 100), (25, 200), (40, 1000)):
        for _ in range(count):
            t.append(t[-1] + step)
    return tuple(t + [t[-1]])


ABUNDANCE_TABLE = _abundance_table()


def table_index(a):
    """the cell of an abundance by a plain search of ABUNDANCE_TABLE (MPHFAlgorithm.cpp:253-266): the last entry <= a, and 255 from the table's last value on"""
    if a >= ABUNDANCE_TABLE[-2]:
        return len(ABUNDANCE_TABLE) - 2
    return max(i for i, v in enumerate(ABUNDANCE_TABLE) if v <= a)


_CODES = np.frombuffer(b"ACTG", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def e_input(k):
    """-> (bases, offsets, repart, values): k-mer-long reads in a seeded shuffle, a third of them reverse complements, whose canonical k-mers are `values`, the i-th
    of them ABUNDANCES[i] times. The forward k-mer starts with A and does not end with T, so its reverse complement is the larger strand (the generator of
    tests/test_gpu_banks.py:kmer_reads, for any k)."""
    rng = np.random.default_rng(900 + k)
    values = []
    for x in random_keys(k, 4 * len(ABUNDANCES), 900 + k):
        x &= 4 ** (k - 1) - 1
        if x & 3 != 2 and x not in values and len(values) < len(ABUNDANCES):
            values.append(x)
    assert len(values) == len(ABUNDANCES) and all(revcomp_int(x, k) > x for x in values)
    fwd = np.array([[(x >> (2 * (k - 1 - i))) & 3 for i in range(k)] for x in values], dtype=np.uint8)
    rev = (fwd[:, ::-1] ^ 2).astype(np.uint8)
    which = np.repeat(np.arange(len(values)), ABUNDANCES)
    which = which[rng.permutation(len(which))]
    flip = rng.random(len(which)) < 1 / 3
    rows = np.where(flip[:, None], rev[which], fwd[which])
    bases = _CODES[rows].reshape(-1)
    offs = np.arange(len(which) + 1, dtype=np.uint64) * np.uint64(k)
    return _frozen(bases), _frozen(offs), _frozen(simple_repart(E_M, E_PARTS)), tuple(values)
