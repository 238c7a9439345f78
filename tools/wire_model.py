#!/usr/bin/env python3
"""CPU model of the packed result stream (csrc/gkc_sink.hip): bytes per record of the KEY part of one partition under several wire formats. numpy only, nothing
from the library: a random genome, reads with substitutions, canonical k-mers, partition = mix64(lexicographic canonical minimizer) % parts (no m-mer exclusions),
the sorted distinct keys of partition 0 and their gaps. The abundance bitmap and bytes (0.15-0.28 B per record) come on top in every format.

    python tools/wire_model.py [--genome 1000000] [--reads 200000] [--sub 0.01] [--k 31] [--m 10] [--parts 8]

The table says where the bytes are, not the third digit; the next format decision starts from it."""
import argparse

import numpy as np

SUB = 128                                                        # records per sub-block
CHUNK = 16                                                       # sub-blocks per pack iteration (padded to 16 bytes together in the two-width format)


def mix64(x):
    x = x.copy()
    x ^= x >> np.uint64(33); x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33); x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return x


def words(code, w):
    """forward and reverse-complement values of every w-mer of every row of `code` (A C T G = 0 1 2 3, complement = code ^ 2)"""
    n = code.shape[1] - w + 1
    f = np.zeros((code.shape[0], n), np.uint64); r = np.zeros_like(f)
    for j in range(w):
        c = code[:, j:j + n].astype(np.uint64)
        f |= c << np.uint64(2 * (w - 1 - j))
        r |= (c ^ np.uint64(2)) << np.uint64(2 * j)
    return f, r


def partition_keys(a):
    rng = np.random.default_rng(a.seed)
    genome = rng.integers(0, 4, a.genome, dtype=np.uint8)
    start = rng.integers(0, a.genome - a.len + 1, a.reads)
    code = genome[start[:, None] + np.arange(a.len)[None, :]]
    flip = rng.random(a.reads) < 0.5
    code[flip] = code[flip, ::-1] ^ 2
    err = rng.random(code.shape) < a.sub
    code[err] = (code[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
    keys = []
    for r0 in range(0, a.reads, 20000):                          # (slices of reads: the k-mer matrices of all of them at once would take 10 GB)
        c = code[r0:r0 + 20000]
        f, r = words(c, a.k); kmer = np.minimum(f, r)
        f, r = words(c, a.m); mm = np.minimum(f, r)
        nk, win = kmer.shape[1], a.k - a.m + 1
        mini = mm[:, :nk].copy()
        for j in range(1, win):
            np.minimum(mini, mm[:, j:j + nk], out=mini)
        keys.append(kmer[mix64(mini) % np.uint64(a.parts) == 0])
    return np.unique(np.concatenate(keys), return_counts=True)


def bit_length(d):
    out = np.zeros(d.shape, np.int64); x = d.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = x >= (np.uint64(1) << np.uint64(s)); out[big] += s; x[big] >>= np.uint64(s)
    return out + (x > 0)


def sub_blocks(length):
    n = len(length) // SUB * SUB
    return length[:n].reshape(-1, SUB)


def one_width(L):
    return (L.max(axis=1) * (SUB // 8) + 1).sum()


def k_widths(L, k, gain_min=0, pad=False):
    """best split of every sub-block into k widths (exact, from its histogram of bit lengths), log2(k) selector bits per record, k width bytes; k = 2 is the format
    of the library: `gain_min` = a split must gain that many bytes, `pad` = 16 sub-blocks are padded to 16 bytes together"""
    total = 0; run = 0
    for i, row in enumerate(L):
        wl = int(row.max()); srt = np.sort(row)
        best = wl * SUB // 8
        if k == 2:
            for ws in range(wl):
                ns = int(np.searchsorted(srt, ws, side="right"))
                cost = SUB // 8 + (ns * ws + 7) // 8 + ((SUB - ns) * wl + 7) // 8
                if cost + gain_min <= wl * SUB // 8 and cost < best:
                    best = cost
        else:                                                    # three widths: two thresholds
            cum = np.searchsorted(srt, np.arange(wl + 1), side="right")
            for w1 in range(wl):
                for w2 in range(w1 + 1, wl):
                    cost = 2 * SUB // 8 + (cum[w1] * w1 + (cum[w2] - cum[w1]) * w2 + (SUB - cum[w2]) * wl + 7) // 8
                    best = min(best, cost)
        run += best
        if pad and i % CHUNK == CHUNK - 1:
            run = (run + 15) // 16 * 16
        total += k
    return run + total


def fixed_classes(length, widths, sel_bits):
    w = np.asarray(widths); idx = np.searchsorted(w, length)
    if (idx >= len(w)).any():
        return float("inf")
    return (w[idx].sum() + sel_bits * len(length)) / 8.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genome", type=int, default=1000000); ap.add_argument("--reads", type=int, default=200000); ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--sub", type=float, default=0.01); ap.add_argument("--k", type=int, default=31); ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--parts", type=int, default=8); ap.add_argument("--seed", type=int, default=1); ap.add_argument("--three", action="store_true", help="also price three widths per sub-block (slow)")
    a = ap.parse_args()
    keys, counts = partition_keys(a)
    gaps = np.diff(keys); length = bit_length(gaps); n = len(gaps)
    print("partition 0 of %d: %d distinct keys, %.1f %% singletons, mean gap 2^%.1f" % (a.parts, len(keys), 100.0 * (counts == 1).mean(), np.log2(gaps.astype(np.float64).mean())))
    hist = np.bincount(length, minlength=65)
    print("bit lengths of the gaps (length: records):")
    print("  " + "  ".join("%d:%d" % (b, hist[b]) for b in range(65) if hist[b]))
    print("  1-35 bits: %.1f %% of the gaps" % (100.0 * hist[1:36].sum() / n))
    L = sub_blocks(length); nl = L.size
    p = hist[hist > 0] / n
    rows = [("independent exponential gaps of this mean: their entropy", np.log2(np.e * gaps.astype(np.float64).mean()) / 8.0),
            ("one width per sub-block of 128 + width byte (GKC_SINK_TWO_WIDTHS=0)", one_width(L) / nl),
            ("two widths per sub-block, best split, 1 selector bit, 2 width bytes", k_widths(L, 2) / nl),
            ("  the same as the library sends it: a split gains >= 16 bytes, 16 sub-blocks padded to 16 bytes", k_widths(L, 2, 16, True) / nl),
            ("2-bit selector, four bit widths per batch (14/30/44/largest)", fixed_classes(length, (14, 30, 44, max(45, int(length.max()))), 2) / n),
            ("2-bit selector, four byte lengths per batch (2/5/6/7 bytes)", fixed_classes(length, (16, 40, 48, 56), 2) / n),
            ("4-bit nibble count + nibbles", ((((length + 3) // 4) * 4 + 4).sum() / 8.0) / n),
            ("order-0 entropy of (bit length, mantissa)", (-(p * np.log2(p)).sum() + (np.maximum(length - 1, 0)).mean()) / 8.0)]
    if a.three:
        rows.insert(4, ("three widths per sub-block, 2 selector bits, 3 width bytes", k_widths(L, 3) / nl))
    print("bytes per record, keys only:")
    for name, v in rows:
        print("  %-100s %.2f" % (name, v))


if __name__ == "__main__":
    main()
