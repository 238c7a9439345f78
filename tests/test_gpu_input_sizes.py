"""The input side at exact positions: the device FASTA / FASTQ parser (csrc/gkc_fastx.hip) and the Stage A scan (csrc/gkc_scan.hip) on the constructions of
tests/fastx_inputs.py and tests/scan_inputs.py, which tests/test_input_sizes_cpu.py pins without a GPU. Parser: one feature at every phase of a 4096-byte tile
border, tiles without a newline, text ends, every prefix and every cut of small texts, line and tile counts on both sides of the prefix scan's chunk of 8192 —
bases, offsets and `consumed` byte for byte against the oracle's reader. Stage A: a read start, an N, a lower-case base, a short read and the end of the push
at every offset from -(k+1) to k+1 around an 8192-position tile border, 1279 / 1280 / 1281 records in one tile, 2^20 + 5 reads in 3073 tiles — every partition,
the statistics and the histogram against the oracle, as tests/test_gpu_parity.py device_vs_oracle compares them. Run with `pytest -m gpu`."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import gko
from tests import fastx_inputs as fx
from tests import scan_inputs as si
from tests.util import simple_repart

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gkc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ge.load().gkc


@pytest.fixture(scope="module")
def parser(gkc):
    c = gkc.Counter(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """the shared references, the cached inputs (a text of 33 MB among them) and the device blocks torch keeps for the texts go when the module is done: the tests after
    this file find the host and the device memory as they would without it"""
    yield
    import torch
    _refs.clear()
    for mod in (fx, si):
        for f in vars(mod).values():
            if hasattr(f, "cache_clear"):
                f.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ parser
def check(parser, text, what=None):
    """a final text: bases, offsets and consumed, byte for byte"""
    b, o, cons = parser.fastx_parse(text)
    rb, ro = gko.fastx_parse(text)
    assert np.array_equal(o, ro), (what, len(o), len(ro), first_difference(o, ro))
    assert np.array_equal(b, rb), (what, first_difference(b, rb))
    assert cons == len(text), what
    return b, o


def first_difference(a, b):
    n = min(len(a), len(b))
    bad = np.flatnonzero(a[:n] != b[:n])
    return "lengths %d / %d, first difference at %s" % (len(a), len(b), int(bad[0]) if len(bad) else None)


def check_chunk(parser, text, fastq, c):
    """the non-final chunk text[:c]: the records of text[:consumed], consumed as the text alone says, and the rest parsed as the final chunk"""
    want = fx.expected_consumed(text[:c], fastq)
    b, o, cons = parser.fastx_parse(text[:c], final=False)
    assert cons == want, (c, cons, want)
    rb, ro = gko.fastx_parse(text[:cons])
    assert np.array_equal(o, ro) and np.array_equal(b, rb), (c, cons, first_difference(o, ro), first_difference(b, rb))
    check(parser, text[cons:], ("rest", c, cons))


@pytest.mark.parametrize("name", sorted(fx.FEATURES))
def test_feature_at_every_phase_of_a_tile_border(parser, name):
    text, claims = fx.feature_at_every_phase(name)
    b, o = check(parser, text, name)
    assert len(o) - 1 > 10 * len(claims)


def test_tiles_without_a_newline(parser):
    for build in (fx.long_sequence_line, fx.long_header_line, fx.long_fastq_record, fx.lines_from_a_border):
        check(parser, build()[0], build.__name__)


@pytest.mark.parametrize("fastq", [False, True])
def test_text_ends_at_every_residue(parser, fastq):
    for t in fx.END_TILES:
        for r in fx.END_RESIDUES:
            for final_newline in (True, False):
                check(parser, fx.text_of_length(fx.FX_TILE * t + r, fastq, final_newline), (t, r, final_newline))


@pytest.mark.parametrize("name", ["fasta_lf", "fasta_crlf"])
def test_every_prefix_as_a_final_text(parser, name):
    """among the CRLF prefixes: a lone '\\r' as the unterminated last line after bases of its record, which the reference keeps (terminated, it is dropped)"""
    text = fx.SMALL_TEXTS[name][0]
    for c in range(len(text) + 1):
        check(parser, text[:c], (name, c))
    for t in fx.LONE_CR_ENDINGS:
        b, o = check(parser, t)
        assert bytes(b) == b"AC\r"
    b, o = check(parser, fx.LONE_CR_TERMINATED)
    assert bytes(b) == b"AC"


@pytest.mark.parametrize("name", sorted(fx.SMALL_TEXTS))
def test_chunk_contract_at_every_cut(parser, name):
    text, fastq = fx.SMALL_TEXTS[name]
    for c in range(len(text) + 1):
        check_chunk(parser, text, fastq, c)


@pytest.mark.parametrize("fastq", [False, True])
def test_chunk_contract_around_tile_borders(parser, fastq):
    text, cuts = fx.three_tile_text(fastq)
    for c in cuts:
        check_chunk(parser, text, fastq, c)


@pytest.mark.parametrize("n_lines", fx.SCAN_LINE_COUNTS)
def test_line_counts_around_the_scan_chunk(parser, n_lines):
    """the record-id scan runs over the lines: 8191, 8192 and 8193 of them, two chunks and one line, a header on the last line of the first chunk / the first of the second"""
    for parity in (0, 1):
        b, o = check(parser, fx.many_short_lines(n_lines, parity), (n_lines, parity))
        assert len(o) - 1 == (n_lines - parity + 1) // 2


def test_more_tiles_than_one_scan_chunk(parser):
    """8196 tiles: tile_line0 and tile_keep of tiles 8192 .. 8195 are sums carried by k_fx_scan_totals / k_fx_scan_add"""
    b, o = check(parser, fx.many_tiles_text())
    assert len(o) - 1 == fx.MANY_TILES_RECORDS and len(b) == 140 * fx.MANY_TILES_RECORDS


# ------------------------------------------------------------------------------------------------ Stage A
_refs = {}


def frequency_order(con, m):
    """frequency order of the m-mers of the first 100 000 bases (RepartitionAlgorithm.cpp:311-492), as tests/test_gpu_parity.py builds it"""
    L = gko.lib()
    counts = np.zeros(4 ** m, np.uint32)
    sample = bytes(con.bases[:100000])
    L.gko_count_mmers(sample, len(sample), m, counts)
    freq = np.zeros(4 ** m, np.uint32)
    L.gko_freq_order_from_counts(m, counts, freq)
    return freq


def reference(key, con, k, m, parts, freq):
    """the oracle's run of a construction, computed once and shared by the tests of the default and the alternative paths"""
    if key not in _refs:
        fo = frequency_order(con, m) if freq else None
        rep = simple_repart(m, parts)
        _refs[key] = (gko.Dsk(con.bases, con.offsets, k, m, parts, rep, freq_order=fo, threads=4), rep, fo)
    return _refs[key]


def device_vs_oracle(gkc, key, con, k, m, parts=si.PARTS, freq=False):
    """the comparisons of tests/test_gpu_parity.py device_vs_oracle, for bases and offsets given as arrays and pushes at stated reads"""
    ref, rep, fo = reference((key, k, m, parts, freq), con, k, m, parts, freq)
    c = gkc.Counter(0)
    try:
        c.set_solidity(1, 2147483647, 10000)
        c.configure(k, m, parts, rep, freq_order=fo)
        c.begin_pass(0)
        for bases, offs in si.push_slices(con):
            c.push_reads(bases, offs)
        c.finish_pass()
        for p in range(parts):
            lo, hi, ab = c.partition(0, p)
            rlo, rhi, rab = ref.part(p)
            assert np.array_equal(lo, rlo), (key, k, m, "partition", p, len(lo), len(rlo))
            assert np.array_equal(hi, rhi) and np.array_equal(ab, rab), (key, k, m, "partition", p)
            assert np.array_equal(c.partition_records(0, p), ref.part_records(p)), (key, k, m, "partition", p)
            assert c.partition_info(0, p)[2] == ref.part_stats(p)[0], (key, k, m, "partition", p)
        st = c.stats()
        for name in ("kmers_nb_valid", "kmers_nb_invalid", "kmers_nb_distinct", "kmers_nb_solid", "nb_sequences"):
            assert st[name] == ref.stats[name], (key, k, m, name, st[name], ref.stats[name])
        assert np.array_equal(c.histogram(), ref.histogram()), (key, k, m)
        lens = np.diff(con.offsets.astype(np.int64))
        assert st["kmers_nb_valid"] + st["kmers_nb_invalid"] == int(np.maximum(lens - k + 1, 0).sum()) and st["nb_sequences"] == len(lens)      # from the offsets alone
        return st, ref
    finally:
        c.close()


@pytest.mark.parametrize("name", si.CONSTRUCTIONS)
@pytest.mark.parametrize("k,m,freq", si.KM_CASES)
def test_stage_a_around_tile_borders(gkc, k, m, freq, name):
    """a read boundary / an N / a lower-case base / a read of k-1, k, k+1 bases / the end of the push at every offset -(k+1) .. k+1 from a tile border"""
    st, ref = device_vs_oracle(gkc, name, si.build(name, k), k, m, freq=freq)
    assert st["nb_superkmers"] >= ref.stats["nb_superkmers"] > 0                  # tile borders may add cuts, nothing removes one


@pytest.mark.parametrize("n_reads", si.BUDGET_READS)
def test_descriptor_budget_of_a_tile(gkc, n_reads):
    """1279 / 1280 / 1281 records in one tile: the last fills the descriptor range of the workgroup, one more makes the emit pass scan again"""
    st, ref = device_vs_oracle(gkc, "budget%d" % n_reads, si.descriptor_budget(n_reads), si.BUDGET_K, si.BUDGET_M)
    assert ref.stats["nb_superkmers"] == n_reads and st["nb_superkmers"] == n_reads


def test_many_reads_and_many_tiles(gkc):
    """2^20 + 5 reads: k_mark_read_starts strides; 3073 tiles: the persistent workgroups loop over tiles with the next one prefetched"""
    st, ref = device_vs_oracle(gkc, "many", si.many_reads(), si.MANY_K, si.MANY_M)
    assert st["kmers_nb_valid"] == si.MANY_READS * (si.MANY_LEN - si.MANY_K + 1) and st["kmers_nb_distinct"] > 4000000


@pytest.mark.parametrize("name", si.CONSTRUCTIONS)
@pytest.mark.parametrize("k,m", [(31, 10), (63, 10)])
@pytest.mark.parametrize("switch,parts", [("GKC_SCAN_NO_DESC=1", si.PARTS), ("GKC_SCAN_GLOBAL_ATOMICS=1", si.PARTS), ("GKC_SCAN_COARSE_MAX=4", 64)])
def test_stage_a_alternative_paths_around_tile_borders(gkc, monkeypatch, switch, parts, k, m, name):
    """the emit pass that scans again instead of reading descriptors, global-atomic cursors, and the two-level scan (64 partitions in 4 groups), on the same inputs"""
    var, _, value = switch.partition("=")
    monkeypatch.setenv(var, value)
    device_vs_oracle(gkc, name, si.build(name, k), k, m, parts=parts)
