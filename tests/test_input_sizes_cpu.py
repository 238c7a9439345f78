"""The constructions of tests/fastx_inputs.py and tests/scan_inputs.py, pinned without a GPU: every claimed feature sits at its claimed byte, every phase of a border
occurs exactly once, the offsets are CSR tables, the oracle reads every text, and the expected `consumed` of the chunk contract depends on the cut and never splits
a record. tests/test_gpu_input_sizes.py runs the same inputs through the device."""
import numpy as np
import pytest

from oracle import gko
from tests import fastx_inputs as fx
from tests import scan_inputs as si


def seqs(data, offs):
    return [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]


def parse(text):
    return seqs(*gko.fastx_parse(text))


# ------------------------------------------------------------------------------------------------ parser
def test_fills_have_the_length_asked_for():
    rng = np.random.default_rng(0)
    for eol in (b"\n", b"\r\n"):
        for n in list(range(3 + 2 * len(eol), 300)) + [4079, 4096, 4113]:
            t = fx.fasta_fill(rng, n, eol)
            assert len(t) == n and t.endswith(eol) and t[:1] == b">"
        for n in list(range(3 + 4 * len(eol), 300)) + [4079, 4096, 4113]:
            t = fx.fastq_fill(rng, n, eol)
            assert len(t) == n and t.endswith(eol) and t.count(b"\n") % 4 == 0
            assert all(len(s) == len(q) for s, q in zip(t.split(b"\n")[1::4], t.split(b"\n")[3::4]))


@pytest.mark.parametrize("name", sorted(fx.FEATURES))
def test_feature_sits_at_every_phase_of_a_border(name):
    text, claims = fx.feature_at_every_phase(name)
    assert sorted(d for d, _ in claims) == list(fx.PHASES) == list(range(-17, 18))              # every phase exactly once
    borders = [(P - d) // fx.FX_TILE for d, P in claims]
    assert all((P - d) % fx.FX_TILE == 0 for d, P in claims) and len(set(borders)) == len(borders) and min(borders) == 1
    assert len(text) > max(P for _, P in claims) + 100
    for d, P in claims:
        if name == "seq_newline":
            assert text[P] == 10 and text[P - 1] in b"ACGT" and text[P + 1] in b"ACGT"
        elif name == "crlf_cr":
            assert text[P] == 13 and text[P + 1] == 10 and text[P - 1] in b"ACGT" and text[P + 2] in b"ACGT"
        elif name == "header_gt":
            assert text[P] == ord(">") and text[P - 1] == 10
        elif name == "blank_line":
            assert text[P] == 10 and text[P - 1] == 10 and text[P - 2] in b"ACGT" and text[P + 1] in b"ACGT"
        elif name == "lone_cr_first":
            assert text[P - 1:P + 2] == b"\n\r\n" and text[text.rfind(b"\n", 0, P - 1) + 1] == ord(">")        # the line before is the header
        elif name == "lone_cr_later":
            assert text[P - 1:P + 2] == b"\n\r\n" and text[P - 2] in b"ACGT"
        elif name == "fastq_plus":
            assert text[P] == ord("+") and text[P - 1] == 10 and text[:P].count(b"\n") % 4 == 2
        elif name == "fastq_qual_at":
            assert text[P] == ord("@") and text[P - 1] == 10 and text[:P].count(b"\n") % 4 == 3
        else:
            assert name == "fastq_crlf_qual" and text[P] == 13 and text[P + 1] == 10 and text[:P].count(b"\n") % 4 == 3
            lines = text[:P].split(b"\n")
            assert len(lines[-1]) == len(lines[-3]) - 1 and lines[-3].endswith(b"\r")           # quality without its '\r' as long as the sequence without its own
    got = parse(text)
    fastq = fx.FEATURES[name][0]
    assert len(got) == (text.count(b"\n") // 4 if fastq else sum(1 for ln in text.split(b"\n") if ln[:1] == b">"))
    if name == "lone_cr_first":
        assert sum(1 for s in got if s == b"\rACGT") == len(claims)                             # kept ...
    if name == "lone_cr_later":
        assert sum(1 for s in got if s == b"ACGTTT") == len(claims) and not any(b"\r" in s for s in got)     # ... dropped
    if name in ("crlf_cr", "fastq_crlf_qual"):
        assert not any(b"\r" in s for s in got)


def test_tiles_without_a_newline():
    text, start, L = fx.long_sequence_line()
    assert L == 3 * 4096 + 5 and text[start - 1] == 10 and text[start + L] == 10 and b"\n" not in text[start:start + L]
    assert (start + L) // fx.FX_TILE - start // fx.FX_TILE >= 3 and max(map(len, parse(text))) == L
    text, start, L = fx.long_header_line()
    assert L == 4096 + 100 and text[start] == ord(">") and text[start - 1] == 10 and text[start + L] == 10 and b"\n" not in text[start:start + L]
    assert b"ACGTTGCAGGA" in parse(text)
    text, start, L = fx.long_fastq_record()
    q0 = start + L + 3
    assert L == 2 * 4096 + 1 and text[start - 1] == 10 and text[start + L:q0] == b"\n+\n" and text[q0 + L] == 10
    assert set(text[q0:q0 + L]) == set(b"@>+I") and b"\n" not in text[start:start + L] and max(map(len, parse(text))) == L
    text, claims = fx.lines_from_a_border()
    assert [L for _, L in claims] == [4095, 4096, 4097]
    for start, L in claims:
        assert start % fx.FX_TILE == 0 and text[start - 1] == 10 and text[start + L] == 10 and b"\n" not in text[start:start + L]
    assert [len(s) for s in parse(text) if len(s) > 4000] == [4095, 4096, 4097]


def test_text_ends():
    assert fx.END_TILES == (1, 2) and fx.END_RESIDUES == (0, 1, 15, 16, 17, 4095)
    for fastq in (False, True):
        for t in fx.END_TILES:
            for r in fx.END_RESIDUES:
                a, b = fx.text_of_length(fx.FX_TILE * t + r, fastq, True), fx.text_of_length(fx.FX_TILE * t + r, fastq, False)
                assert len(a) == len(b) == 4096 * t + r and a[-1] == 10 and b[-1] != 10
                assert len(parse(a)) > 10 and len(parse(b)) > 10


def test_small_texts_and_the_lone_cr_ending():
    for name, (text, fastq) in fx.SMALL_TEXTS.items():
        assert 140 <= len(text) <= 200, (name, len(text))
        assert (b"\r\n" in text) == name.endswith("crlf") and len(parse(text)) >= 6
    assert b"\n\n" in fx.SMALL_FASTA_LF and b"\r\n\r\n" in fx.SMALL_FASTA_CRLF and not fx.SMALL_FASTA_LF.startswith(b">") and not fx.SMALL_FASTA_CRLF.startswith(b">")
    assert b"\n@" in fx.SMALL_FASTQ_LF.replace(b"\n@q", b"") and b"@q3\n\n+\n\n" in fx.SMALL_FASTQ_LF              # qualities that start with '@', an empty record
    # the CRLF prefixes include the ending the device used to strip: the oracle keeps the '\r' there and nowhere else
    cuts = fx.lone_cr_prefixes(fx.SMALL_FASTA_CRLF)
    assert len(cuts) >= 3
    for c in range(len(fx.SMALL_FASTA_CRLF) + 1):
        got = parse(fx.SMALL_FASTA_CRLF[:c])
        assert (len(got) > 0 and got[-1].endswith(b"\r") and len(got[-1]) > 1) == (c in cuts), c
    assert fx.lone_cr_prefixes(fx.SMALL_FASTA_LF) == []
    for t in fx.LONE_CR_ENDINGS:
        assert parse(t) == [b"AC\r"]
    assert parse(fx.LONE_CR_TERMINATED) == [b"AC"]


def chunk_contract_on_the_oracle(text, fastq, cuts):
    whole = parse(text)
    starts = fx.record_starts(text, fastq) | {0, len(text)}
    cons = [fx.expected_consumed(text[:c], fastq) for c in cuts]
    for c, k in zip(cuts, cons):
        assert 0 <= k <= c and k in starts, (c, k)                                               # never splits a record
        assert parse(text[:k]) + parse(text[k:]) == whole, (c, k)
    return cons


@pytest.mark.parametrize("name", sorted(fx.SMALL_TEXTS))
def test_chunk_contract_expectation_at_every_cut(name):
    text, fastq = fx.SMALL_TEXTS[name]
    cons = chunk_contract_on_the_oracle(text, fastq, range(len(text) + 1))
    assert any(a != b for a, b in zip(cons, cons[1:])) and len(set(cons)) >= 6                   # the result depends on the cut
    assert cons[0] == 0 and cons[-1] == (len(text) if fastq else text.rfind(b">"))


@pytest.mark.parametrize("fastq", [False, True])
def test_chunk_contract_expectation_on_three_tiles(fastq):
    text, cuts = fx.three_tile_text(fastq)
    assert 2 * fx.FX_TILE < len(text) <= 3 * fx.FX_TILE and sorted(cuts) == [4096 * t + d for t in (1, 2) for d in range(-17, 18)]
    cons = chunk_contract_on_the_oracle(text, fastq, cuts)
    assert any(a != b for a, b in zip(cons[:35], cons[1:35])) and any(a != b for a, b in zip(cons[35:], cons[36:]))      # ... at both borders


def test_scan_chunk_borders():
    assert fx.SCAN_LINE_COUNTS == (8191, 8192, 8193, 16385) and fx.FXS_CHUNK == 8192
    for n_lines in fx.SCAN_LINE_COUNTS:
        for parity in (0, 1):
            text = fx.many_short_lines(n_lines, parity)
            lines = text.split(b"\n")
            assert text[-1] == 10 and len(lines) - 1 == n_lines and max(map(len, lines)) <= 8
            for j in (8191, 8192):
                if j < n_lines:
                    assert (lines[j][:1] == b">") == (j % 2 == parity), (n_lines, parity, j)     # a header on line 8192 (parity 0) and on line 8191 (parity 1)
            assert len(parse(text)) == sum(1 for ln in lines if ln[:1] == b">")
    text = fx.many_tiles_text()
    n_tiles = (len(text) + fx.FX_TILE - 1) // fx.FX_TILE
    assert len(text) == 150 * fx.MANY_TILES_RECORDS and n_tiles > fx.FXS_CHUNK + 2
    a = np.frombuffer(text, dtype=np.uint8).reshape(-1, 150)
    assert (a[:, 0] == ord(">")).all() and (a[:, [7, 78, 149]] == 10).all() and np.isin(np.delete(a, [7, 78, 149], axis=1)[:, 7:], fx.ACGT).all()
    assert (np.delete(a, [7, 78, 149], axis=1) != 10).all()
    second_chunk = text[fx.FXS_CHUNK * fx.FX_TILE:]
    assert second_chunk.count(b">") >= 20                                                        # headers and kept bases in the tiles of the second scan chunk
    data, offs = gko.fastx_parse(text)
    assert len(offs) - 1 == fx.MANY_TILES_RECORDS and (np.diff(offs) == 140).all() and np.isin(data, fx.ACGT).all()


# ------------------------------------------------------------------------------------------------ Stage A
def csr(con):
    o = con.offsets.astype(np.int64)
    return con.offsets.dtype == np.uint64 and o[0] == 0 and o[-1] == len(con.bases) and (np.diff(o) >= 0).all()


def phases_once(con, k, tiles=None):
    """every phase -(k+1) .. k+1 exactly once per multiple of the tile, every claim next to its own border"""
    want = list(range(-(k + 1), k + 2))
    by_border = {}
    for d, p in con.claims:
        assert (p - d) % si.SCAN_TILE == 0 and (p - d) > 0 and abs(d) <= k + 1
        by_border.setdefault((p - d) // si.SCAN_TILE, []).append(d)
    if tiles is None:
        assert sorted(d for d, _ in con.claims) == want and all(len(v) == 1 for v in by_border.values())       # one border per phase
    else:
        assert sorted(by_border) == list(tiles) and all(sorted(v) == want for v in by_border.values())


@pytest.mark.parametrize("k,m,freq", si.KM_CASES)
def test_stage_a_constructions(k, m, freq):
    assert si.phases(k) == tuple(range(-(k + 1), k + 2)) and si.SCAN_TILE == 8192 and k <= si.SCAN_HALO
    for name in si.CONSTRUCTIONS:
        con = si.build(name, k)
        assert csr(con), name
        assert con.bases.dtype == np.uint8 and np.isin(con.bases, np.frombuffer(b"ACGTNacgt", dtype=np.uint8)).all()
        assert [r0 for r0, _ in con.pushes] == [0] + [r1 for _, r1 in con.pushes][:-1] and con.pushes[-1][1] == len(con.offsets) - 1
        o = set(con.offsets.tolist())
        pos = [p for _, p in con.claims]
        if name == "push_end":
            phases_once(con, k, tiles=(1, 2))
            assert [len(b) for b, _ in si.push_slices(con)] == pos and si.SCAN_TILE in pos and 2 * si.SCAN_TILE in pos
            assert all(len(of) == 2 and of[0] == 0 and of[1] == len(b) for b, of in si.push_slices(con))
            continue
        phases_once(con, k)
        assert len(con.pushes) == 1 and len(con.bases) == si.SCAN_TILE * (2 * k + 4)
        if name == "boundary":
            assert o == set(pos) | {0, len(con.bases)}
        elif name == "N":
            assert list(np.flatnonzero(con.bases == ord("N"))) == pos and len(con.offsets) == 2
        elif name == "lower":
            assert list(np.flatnonzero(con.bases >= ord("a"))) == pos and len(con.offsets) == 2 and not (con.bases == ord("N")).any()
        else:
            L = k + int(name[5:])
            assert L in (k - 1, k, k + 1) and o == set(pos) | {p + L for p in pos} | {0, len(con.bases)}
            starts = con.offsets[:-1].astype(np.int64); lens = np.diff(con.offsets.astype(np.int64))
            assert (lens[np.isin(starts, pos)] == L).all() and (lens[~np.isin(starts, pos)] > 1000).all()


@pytest.mark.parametrize("n_reads", si.BUDGET_READS)
def test_descriptor_budget_construction(n_reads):
    assert si.DESC_PER_TILE == si.SCAN_TILE * 5 // 32 == 1280 and si.BUDGET_READS == (1279, 1280, 1281)
    con = si.descriptor_budget(n_reads)
    k, m = si.BUDGET_K, si.BUDGET_M
    lens = np.diff(con.offsets.astype(np.int64))
    assert csr(con) and len(con.bases) == si.SCAN_TILE and len(lens) == n_reads + 1 and (lens[:-1] == k).all()
    assert (con.bases[k * n_reads:] == ord("N")).all() and np.isin(con.bases[:k * n_reads], si.ACGT).all()
    from tests.util import simple_repart
    ref = gko.Dsk(con.bases, con.offsets, k, m, si.PARTS, simple_repart(m, si.PARTS))
    assert ref.stats["nb_superkmers"] == n_reads and ref.stats["kmers_nb_valid"] == n_reads


def test_many_reads_construction():
    con = si.many_reads()
    n_tiles = (len(con.bases) + si.SCAN_TILE - 1) // si.SCAN_TILE
    assert csr(con) and len(con.offsets) - 1 == (1 << 20) + 5 and (np.diff(con.offsets.astype(np.int64)) == 24).all()
    assert len(con.offsets) > si.MARK_ONE_TRIP == 1 << 20 and n_tiles == 3073 > si.SCAN_GRID_MAX and si.MANY_LEN >= si.MANY_K
