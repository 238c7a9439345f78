"""The packed result batches with TWO delta widths per sub-block of 128 records (csrc/gkc_sink.hip k_pack_pkv_two_widths / csrc/gkc_wire.hpp unpack_pkv_two_widths): 8-byte keys at abundance-min 1,
dense partitions. A sub-block travels as [selector bitmap][short deltas][long deltas] where that is at least 16 bytes shorter than its deltas at one width, and as
those otherwise; GKC_SINK_TWO_WIDTHS=0 keeps one width everywhere. Every case: for every partition, what gkc_wait_partition hands out is byte for byte
gkc_partition_counts, and that the oracle's records; two passes with one context (the staging buffer and the unpack threads are reused). GKC_SINK_DENSE=1 makes
partitions of any size take the dense format. Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests.util import simple_repart, synth_reads

pytestmark = pytest.mark.gpu

K = 31
SUB, BLOCK = 128, 8192
ALPHA = "ACTG"                                                   # codes 0 1 2 3


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


def kmer_of(key):
    """the 31-mer whose forward value is `key`"""
    return "".join(ALPHA[(key >> (2 * (K - 1 - i))) & 3] for i in range(K)).encode()


def reads_of_gaps(gaps, first=4 * 12345):
    """One read of exactly k nucleotides per key; the keys are `first` and the running sums of `gaps` (multiples of 4). Every key starts with A (below 2^60) and ends
    with A, so its reverse complement starts with T and the forward value is the canonical one: the partition holds exactly these keys, with exactly these gaps."""
    keys = np.uint64(first) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(gaps, dtype=np.uint64), dtype=np.uint64)])
    assert int(keys[-1]) < 1 << 60 and all(int(g) % 4 == 0 and int(g) > 0 for g in gaps)
    return [kmer_of(int(x)) for x in keys]


_cache = {}


def case(name, make_reads, m, parts, rep=None):
    """(bases, offs, rep, oracle) of a named input, computed once for the module and never changed"""
    key = (name, m, parts)
    if key not in _cache:
        bases, offs = gko.pack_reads(make_reads())
        rep_ = simple_repart(m, parts) if rep is None else rep
        _cache[key] = (bases, offs, rep_, gko.Dsk(bases, offs, K, m, parts, rep_, abundance_min=1))
    return _cache[key]


def gaps_by_sub_block(rec):
    """the gaps of a partition's device records, per sub-block of 128 (a block's first record has no gap: it travels as the block's base key)"""
    keys = rec.view(np.uint64).reshape(-1, 2)[:, 0]
    out = []
    for b0 in range(0, len(keys), BLOCK):
        kb = keys[b0:b0 + BLOCK]
        d = np.diff(kb)
        for s0 in range(0, len(kb), SUB):
            out.append(d[max(s0 - 1, 0):min(s0 + SUB, len(kb)) - 1] if s0 else d[:SUB - 1])
    return out


def run_case(gkc, inp, parts, passes=2, sink_mb=256, batch_keys=0):
    """two passes over one context; returns (the partitions' device records, the wire bytes of the last pass, what the sink handed out)"""
    bases, offs, rep, ref = inp
    m = int(round(np.log(len(rep)) / np.log(4)))
    c = gkc.Counter(0); c.configure(K, m, parts, rep); c.set_solidity(1, 2147483647, 10000)
    if batch_keys:
        c.set_batch_keys(batch_keys)
    sink = gkc.HostBuffer(sink_mb << 20)
    c.set_host_sink(sink)
    recs, landed = [], []
    for rnd in range(passes):
        c.begin_pass(0); c.push_reads(bases, offs); c.finish_pass()
        recs, landed = [], []
        for p in range(parts):
            view, n = c.wait_partition(0, p)
            dev = c.partition_records(0, p)
            assert n * 16 == len(dev), (rnd, p)
            if n:
                assert view is not None and np.array_equal(view, dev), (rnd, p, n)
            assert np.array_equal(dev, ref.part_records(p)), (rnd, p)
            recs.append(dev); landed.append(bytes(view) if n else b"")
    wire = c.stats()["sink_wire_bytes"]
    c.set_host_sink(None)
    return recs, wire, landed


# ------------------------------------------------------------------------------------------------ inputs
def clustered_reads():
    """30x over 100 kb with 1 % substitutions: about 6e5 distinct k-mers, a third of their gaps small (an error k-mer beside its parent). A sub-block of 128 such gaps
    without a small one does not happen by chance (0.7^128), so 1200 keys below 2^42 (ten leading A's: the random genome puts less than one k-mer there) with gaps
    of 2^31 .. 2^32 are added: the first sub-blocks of the partitions they fall into have no small gap."""
    rng = np.random.default_rng(11)
    g = (np.uint64(1) << np.uint64(31)) + rng.integers(0, 1 << 29, 1199).astype(np.uint64) * np.uint64(4)
    return synth_reads(20000, 100000, 150, sub_rate=0.01) + reads_of_gaps(g)


def clustered_with_copies():
    reads = synth_reads(20000, 100000, 150, sub_rate=0.01)
    return reads + [reads[0]] * 700


def sparse_reads():
    return synth_reads(3000, 20000, 150, seed=62, n_rate=0.001)


SMALL = lambda rng, n: rng.integers(1, 64, n).astype(np.uint64) * np.uint64(4)                         # gaps of at most 8 bits
LARGE = lambda rng, n: rng.integers(1 << 44, 1 << 46, n).astype(np.uint64) * np.uint64(4)             # gaps of 47 or 48 bits


def pattern_reads():
    """Case (c): sub-blocks built gap by gap. Record r of the partition sits at position r % 128 of sub-block r // 128 and carries gap[r - 1].
      sub-block 0        large gaps only
      sub-blocks 1-4     ONE small gap, at position 0 / 63 / 64 / 127, among large ones
      sub-blocks 5-8     the mirror: ONE large gap at position 0 / 63 / 64 / 127 among small ones
      sub-blocks 9-13    runs of small gaps among large ones whose ends fall on the boundaries of the pack kernel's prefix (8 records per thread, 16 threads, 64 lanes):
                         positions 0-15, 60-67 and 100-110, 112-127, every other record, 7-8 and 63-64 and 119-127
      sub-block 14       partial (77 records), half small
    """
    rng = np.random.default_rng(3)
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
    gap = np.where(small, SMALL(rng, n), LARGE(rng, n))[1:]                                            # (record 0 is the block's base key)
    return reads_of_gaps(gap), small


def one_partition(m=8):
    return np.zeros(4 ** m, np.uint16)


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("parts", [1, 3])
def test_clustered_dense_partitions(gkc, monkeypatch, parts):
    """The flagship's gap density: ~70 blocks, a partial last block and a partial last sub-block per partition. Both kinds of sub-block occur: a gap below 2^30
    beside one above 2^40, and a sub-block without a small gap. The two-width format puts fewer bytes on the link than one width per sub-block."""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    inp = case("clustered", clustered_reads, 8, parts)
    recs, wire_two, landed = run_case(gkc, inp, parts)
    mixed = pure = 0
    for r in recs:
        assert len(r) // 16 > BLOCK and (len(r) // 16) % SUB                                           # several blocks, a partial last sub-block
        for d in gaps_by_sub_block(r):
            if len(d) == 0:
                continue
            lo, hi = bool((d < np.uint64(1 << 30)).any()), bool((d > np.uint64(1 << 40)).any())
            mixed += lo and hi; pure += not lo
    print("clustered, %d partition(s): %d records, %d sub-blocks with a gap < 2^30 beside one > 2^40, %d without a small gap, %d wire bytes"
          % (parts, sum(len(r) for r in recs) // 16, mixed, pure, wire_two))
    assert mixed > 0 and pure > 0
    monkeypatch.setenv("GKC_SINK_TWO_WIDTHS", "0")
    recs1, wire_one, landed1 = run_case(gkc, inp, parts, passes=1)
    print("one width per sub-block: %d wire bytes (%.3f -> %.3f bytes per record)" % (wire_one, wire_one * 16.0 / sum(len(r) for r in recs), wire_two * 16.0 / sum(len(r) for r in recs)))
    assert landed1 == landed
    assert 0 < wire_two < wire_one


def test_all_short_one_width(gkc, monkeypatch):
    """(a) 256 keys that differ in their last four nucleotides only: consecutive integers, every delta is 1, one small width and no bitmap"""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    # (forward canonical: it begins with 13 A's, the reverse complement has the complement of the A at nucleotide 27 as its fifth)
    inp = case("consecutive", lambda: [kmer_of((0x1234567 << 10) + v) for v in range(256)], 8, 1, one_partition())
    recs, wire, _ = run_case(gkc, inp, 1)
    d = np.diff(recs[0].view(np.uint64).reshape(-1, 2)[:, 0])
    assert len(d) == 255 and (d == 1).all()
    assert wire < 256 * 16


def test_partial_sub_block(gkc, monkeypatch):
    """(b) fewer than 128 records in the partition: one partial sub-block, once split (60 large gaps, 39 small ones) and once not (99 large gaps)"""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    rng = np.random.default_rng(4)
    for name, nsmall in (("partial split", 39), ("partial whole", 0)):
        gap = np.concatenate([LARGE(rng, 60), SMALL(rng, nsmall)]) if nsmall else LARGE(rng, 99)
        gap = gap[rng.permutation(len(gap))]
        inp = case(name, lambda: reads_of_gaps(gap), 8, 1, one_partition())
        recs, wire, _ = run_case(gkc, inp, 1)
        d = gaps_by_sub_block(recs[0])
        assert len(d) == 1 and np.array_equal(d[0], gap)


def test_single_gaps_and_runs_at_the_prefix_boundaries(gkc, monkeypatch):
    """(c) one small gap among large ones and the mirror at positions 0, 63, 64 and 127 of a sub-block, runs of small gaps that end on the boundaries of the pack
    kernel's selector prefix, a partial last sub-block (pattern_reads)"""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    reads, small = pattern_reads()
    inp = case("pattern", lambda: reads, 8, 1, one_partition())
    recs, wire_two, landed = run_case(gkc, inp, 1)
    keys = recs[0].view(np.uint64).reshape(-1, 2)[:, 0]
    assert len(keys) == len(small)
    assert np.array_equal(np.diff(keys) < np.uint64(1 << 8), small[1:]) and (np.diff(keys)[~small[1:]] > np.uint64(1 << 40)).all()
    monkeypatch.setenv("GKC_SINK_TWO_WIDTHS", "0")
    recs1, wire_one, landed1 = run_case(gkc, inp, 1, passes=1)
    assert landed1 == landed and wire_two < wire_one                                                   # (sub-blocks 5-14 are several times shorter with two widths)


def test_wide_gaps_w64_beside_split_sub_blocks(gkc, monkeypatch):
    """(d) 40 partitions on 3000 reads: gaps of 2^56 and more (a long width of 64) in sub-blocks that also hold the small gaps of error k-mers. Hardly anything pays
    here: the bytes on the link are at most those of one width per sub-block plus the second width byte of every sub-block."""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    parts = 40
    inp = case("sparse", sparse_reads, 8, parts)
    recs, wire_two, landed = run_case(gkc, inp, parts)
    wide = wide_and_small = nblk = 0
    for r in recs:
        nblk += (len(r) // 16 + BLOCK - 1) // BLOCK
        for d in gaps_by_sub_block(r):
            w = bool(len(d)) and bool((d >= np.uint64(1 << 56)).any())
            wide += w; wide_and_small += w and bool((d < np.uint64(1 << 30)).any())
    assert wide > 0 and wide_and_small > 0
    monkeypatch.setenv("GKC_SINK_TWO_WIDTHS", "0")
    recs1, wire_one, landed1 = run_case(gkc, inp, parts, passes=1)
    print("sparse: %d blocks, %d wire bytes with two widths, %d with one" % (nblk, wire_two, wire_one))
    assert landed1 == landed
    assert wire_two <= wire_one + nblk * (BLOCK // SUB) + 64                                          # (+ the header's padding to 64 bytes)


def test_abundance_stream_beside_the_selector_bitmap(gkc, monkeypatch):
    """One read copied 700 times inside a clustered partition: abundances of 255 and more escape, the abundance stream's offsets and the selector bitmaps are
    independent of each other"""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    inp = case("copies", clustered_with_copies, 8, 1)
    recs, wire, _ = run_case(gkc, inp, 1)
    ab = recs[0].view(np.uint64).reshape(-1, 2)[:, 1]
    assert int((ab >= 255).sum()) >= 100 and int((ab == 1).sum()) > len(ab) // 2 and int(((ab > 1) & (ab < 255)).sum()) > 0


@pytest.mark.parametrize("switch", ["GKC_SINK_ADAPTIVE=2", "GKC_STAGEB_LANES=1"])
def test_mode_rules_with_two_widths(gkc, monkeypatch, switch):
    """Every other batch raw (GKC_SINK_ADAPTIVE=2; three batches of one partition each: packed, raw, packed) and one Stage-B lane: the same bytes in the sink"""
    monkeypatch.setenv("GKC_SINK_DENSE", "1")
    inp = case("clustered", clustered_reads, 8, 3)
    recs, wire_packed, landed0 = run_case(gkc, inp, 3, passes=1, batch_keys=1 << 20)
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    recs, wire, landed = run_case(gkc, inp, 3, batch_keys=1 << 20)
    assert landed == landed0
    nbytes = sum(len(r) for r in recs)
    if name == "GKC_SINK_ADAPTIVE":
        assert wire_packed < wire < nbytes                                                              # some batches packed, some raw
    else:
        assert wire == wire_packed
