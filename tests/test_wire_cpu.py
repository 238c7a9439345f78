"""The host decoders of the packed result batches (gatb-core_amd/csrc/gkc_wire.hpp) on their own: tests/wire_driver.cpp is compiled with plain g++ against the header,
packs the records of a case with a plain scalar encoder of its own into a buffer of exactly the size the header's layout function gives, decodes every block with
unpack_block and compares the sink with the records byte for byte. The cases are the smallest shapes at which a decoder can go wrong. No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

CSRC = os.path.join(ge.ROOT, "gatb-core_amd", "csrc")
FIXED7, FIXED8, PKV, PKV_TWO, FIXED16, FIXED17, PKV16 = range(7)          # WireFormat
SUB, BLOCK = 128, 8192
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire") / "wire_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ge.ROOT, "tests", "wire_driver.cpp"), "-lpthread"], check=True)
    return exe


def have_avx512():
    try:
        flags = next(line for line in open("/proc/cpuinfo") if line.startswith("flags")).split()
    except (OSError, StopIteration):
        return False
    return "avx512f" in flags and "popcnt" in flags


def run(driver, fmt, keys, ab, short=-1, avx512=False, dest_offset=0, parts=None):
    """one batch through the driver; returns the words of its "ok" line as a dict"""
    assert len(keys) == len(ab)
    text = "format %d\navx512 %d\nshort %d\ndest_offset %d\n" % (fmt, int(avx512), short, dest_offset)
    if parts:
        text += "parts %d %s\n" % (len(parts), " ".join(str(p) for p in parts))
    text += "records %d\n" % len(keys) + "".join("%x %x %d\n" % (k >> 64, k & M64, a) for k, a in zip(keys, ab))
    r = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0] == "ok"
    out = {w[i]: w[i + 1] for i in range(1, len(w) - 1, 2)}
    assert int(out["records"]) == len(keys)
    return out


def keys_of_gaps(gaps, first=4 * 12345, mod=M64):
    """the first key and the running sums of the gaps (modulo the key width: a delta is a difference modulo it)"""
    keys, k = [first], first
    for g in gaps:
        k = (k + int(g)) & mod
        keys.append(k)
    return keys


def gaps_of_length(rng, bits, n):
    """n gaps of exactly `bits` bits"""
    return [(1 << (bits - 1)) | int(rng.integers(0, 1 << 62)) % (1 << (bits - 1)) for _ in range(n)]


def gaps_of_length128(rng, bits, n):
    return [(1 << (bits - 1)) | ((int(rng.integers(0, 1 << 62)) << 62 | int(rng.integers(0, 1 << 62))) % (1 << (bits - 1))) for _ in range(n)]


def abundances(n, flagged=True):
    """1 everywhere but: 2 / 254 / 255 / 700 at positions 7, 8, 63 and 64 of every sub-block (the ends of a group of 8 and of a bitmap word), rotating, and 700
    (an escape) on the last record — of a partial sub-block where n is no multiple of 128"""
    ab = [1] * n
    if flagged:
        vals = (2, 254, 255, 700)
        for j, i in enumerate(i for s in range(0, n, SUB) for i in (s + 7, s + 8, s + 63, s + 64) if i < n):
            ab[i] = vals[(j + j // 4) % 4]
        ab[n - 1] = 700
    return ab


def both_emitters(driver, keys, ab, short, **kw):
    """the two-width format through the scalar emitter and (where the CPU has it) the AVX-512 one, to a 64-byte-aligned sink and to one that is not"""
    sinks = set()
    for avx in ((False, True) if have_avx512() else (False,)):
        for off in (0, 16):
            sinks.add(run(driver, PKV_TWO, keys, ab, short=short, avx512=avx, dest_offset=off, **kw)["sink"])
    assert len(sinks) == 1
    return sinks.pop()


def pkv8(driver, keys, ab, short, **kw):
    """8-byte keys through PKV with one width and with two: the same sink"""
    one = run(driver, PKV, keys, ab, **kw)
    assert both_emitters(driver, keys, ab, short, **kw) == one["sink"]
    return one


@pytest.mark.skipif(not have_avx512(), reason="this CPU has no AVX-512: the scalar emitter is what the other tests run")
def test_avx512_emitter_runs(driver):
    rng = np.random.default_rng(1)
    gaps = gaps_of_length(rng, 44, 200)
    run(driver, PKV_TWO, keys_of_gaps(gaps), abundances(201), short=8, avx512=True)


def test_one_record(driver):
    for flagged in (False, True):
        out = pkv8(driver, [0x123456789], abundances(1, flagged), short=8)
        assert int(out["blocks"]) == 1 and int(out["abundance_bytes"]) == int(flagged)


def test_partial_sub_block(driver):
    """99 records: once nothing to split (99 large gaps... 98 and the base key), once 60 long gaps and 39 short ones"""
    rng = np.random.default_rng(4)
    large = gaps_of_length(rng, 47, 98)
    pkv8(driver, keys_of_gaps(large), abundances(99), short=-1)
    mixed = gaps_of_length(rng, 47, 60) + gaps_of_length(rng, 8, 38)      # (+ the block's first record, whose delta of 0 is short: 39)
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    pkv8(driver, keys_of_gaps(mixed), abundances(99), short=8)


@pytest.mark.parametrize("n", [128, 129, 8193])
def test_sub_block_and_block_boundaries(driver, n):
    """a full sub-block, one record beyond it, one record beyond a block (a second block of one record); without any flagged record too (an empty abundance stream)"""
    rng = np.random.default_rng(n)
    gaps = [gaps_of_length(rng, 8 if rng.random() < 0.3 else 45, 1)[0] for _ in range(n - 1)]
    out = pkv8(driver, keys_of_gaps(gaps), abundances(n), short=8)
    assert int(out["blocks"]) == (n + BLOCK - 1) // BLOCK
    out = pkv8(driver, keys_of_gaps(gaps), abundances(n, False), short=8)
    assert int(out["abundance_bytes"]) == 0


def test_two_partitions(driver):
    """blocks never straddle partitions: 130 + 1 + 300 records are three blocks"""
    rng = np.random.default_rng(9)
    gaps = gaps_of_length(rng, 40, 430)
    out = pkv8(driver, keys_of_gaps(gaps), abundances(431), short=12, parts=[130, 1, 300])
    assert int(out["blocks"]) == 3


def pattern_small():
    """the gap pattern of pattern_reads() in tests/test_gpu_sink_two_widths.py: 14 sub-blocks + 77 records; single short / long gaps at positions 0, 63, 64 and
    127 of a sub-block, runs that end on the boundaries of 8 / 16 / 64 records"""
    n = 14 * SUB + 77
    small = np.zeros(n, bool)
    for s, pos in zip(range(1, 5), (0, 63, 64, 127)):
        small[s * SUB + pos] = True
    for s, pos in zip(range(5, 9), (0, 63, 64, 127)):
        small[s * SUB:(s + 1) * SUB] = True; small[s * SUB + pos] = False
    small[9 * SUB:9 * SUB + 16] = True
    small[10 * SUB + 60:10 * SUB + 68] = True; small[10 * SUB + 100:10 * SUB + 111] = True
    small[11 * SUB + 112:12 * SUB] = True
    small[12 * SUB:13 * SUB:2] = True
    for a, b in ((7, 9), (63, 65), (119, 128)):
        small[13 * SUB + a:13 * SUB + b] = True
    small[14 * SUB::2] = True
    return small


def test_single_gaps_and_runs_at_the_boundaries(driver):
    rng = np.random.default_rng(3)
    small = pattern_small()
    gaps = [gaps_of_length(rng, int(rng.integers(1, 9)) if s else int(rng.integers(47, 49)), 1)[0] for s in small[1:]]
    pkv8(driver, keys_of_gaps(gaps), abundances(len(small)), short=8)


@pytest.mark.parametrize("long_bits,short_bits", [(1, -1), (56, 8), (57, 8), (64, 8), (64, 56), (40, 1), (56, 55)])
def test_widths(driver, long_bits, short_bits):
    """long widths of 1, 56, 57 (travels as 64) and 64; short widths of 1 (a gap of 0 does not occur) and 56: two sub-blocks and a partial one"""
    rng = np.random.default_rng(100 * long_bits + short_bits + 1)
    n = 2 * SUB + 50
    gaps = []
    for i in range(n - 1):
        if short_bits < 0 or rng.random() < 0.6:
            gaps += gaps_of_length(rng, long_bits, 1)
        else:
            gaps += gaps_of_length(rng, int(rng.integers(1, short_bits + 1)), 1)
    gaps[5] = gaps_of_length(rng, long_bits, 1)[0]                        # (every sub-block has a gap of the long width)
    gaps[SUB + 5] = gaps_of_length(rng, long_bits, 1)[0]
    gaps[2 * SUB + 5] = gaps_of_length(rng, long_bits, 1)[0]
    if short_bits > 0:
        gaps[SUB] = gaps_of_length(rng, short_bits, 1)[0]
    pkv8(driver, keys_of_gaps(gaps), abundances(n), short=short_bits)


def test_pkv_16_byte_keys(driver):
    """sub-block widths of 1, 63, 64, 65 and 128 bits and a partial last sub-block, the same abundances"""
    rng = np.random.default_rng(16)
    widths = (1, 63, 64, 65, 128, 100)
    n = 5 * SUB + 50
    gaps = []
    for i in range(1, n):
        w = widths[i // SUB]
        gaps += gaps_of_length128(rng, w if i % SUB == 5 or rng.random() < 0.5 else int(rng.integers(1, w + 1)), 1)
    keys = keys_of_gaps(gaps, first=(0x1234 << 64) | 0x5678, mod=M128)
    sinks = {run(driver, PKV16, keys, abundances(n), dest_offset=off)["sink"] for off in (0, 16)}
    assert len(sinks) == 1
    run(driver, PKV16, keys[:1], abundances(1))
    run(driver, PKV16, keys, abundances(n, False))


@pytest.mark.parametrize("fmt,escapes", [(FIXED7, 2), (FIXED8, 0)])
def test_fixed_entries(driver, fmt, escapes):
    """deltas of 2^48 - 2, 2^48 - 1 and 2^48: the last two escape at width 7; an abundance of 255 or more on the record of a key escape"""
    rng = np.random.default_rng(7)
    n = 300
    gaps = gaps_of_length(rng, 40, n - 1)
    gaps[9], gaps[19], gaps[29] = (1 << 48) - 2, (1 << 48) - 1, 1 << 48
    ab = abundances(n)
    ab[10], ab[20], ab[30] = 254, 255, 700                               # (record i carries gap i - 1)
    out = run(driver, fmt, keys_of_gaps(gaps), ab)
    n_ab = sum(a >= 255 for a in ab)
    assert int(out["exceptions"]) == escapes + n_ab
    out = run(driver, fmt, keys_of_gaps(gaps), ab, dest_offset=16, parts=[1, 299])
    assert int(out["blocks"]) == 2


def test_fixed_8_escape(driver):
    """width 8: a delta of 2^56 - 1 and above escapes"""
    gaps = [5, (1 << 56) - 2, (1 << 56) - 1, 1 << 56, 7]
    out = run(driver, FIXED8, keys_of_gaps(gaps), [1, 1, 255, 1, 300, 1])
    assert int(out["exceptions"]) == 2 + 2


@pytest.mark.parametrize("fmt,escapes", [(FIXED16, 3), (FIXED17, 0)])
def test_fixed_entries_16_byte_keys(driver, fmt, escapes):
    """a delta of 2^120 - 2, of exactly 2^120 - 1 and above: the last ones escape at width 16, through two entries each"""
    rng = np.random.default_rng(8)
    n = 300
    gaps = gaps_of_length128(rng, 107, n - 1)
    gaps[9], gaps[19], gaps[29], gaps[39] = (1 << 120) - 2, (1 << 120) - 1, (1 << 120) + 5, 1 << 127
    ab = abundances(n)
    ab[10], ab[20], ab[30], ab[40] = 254, 255, 700, 1
    keys = keys_of_gaps(gaps, first=(0x1234 << 64) | 0x5678, mod=M128)
    out = run(driver, fmt, keys, ab)
    assert int(out["exceptions"]) == 2 * escapes + sum(a >= 255 for a in ab)
    run(driver, fmt, keys, ab, dest_offset=16, parts=[299, 1])
