"""FASTA / FASTQ texts for the device parser (csrc/gkc_fastx.hip) with one feature at a stated byte position: at every phase of a tile border, tiles without a
newline, text ends at every residue of a thread's 16 bytes, every prefix and every cut of small texts, and line / tile counts on both sides of the prefix scan's
chunk. numpy only; every builder returns the text and the positions it claims, tests/test_input_sizes_cpu.py asserts each claim byte by byte and that the oracle
reads the text, tests/test_gpu_input_sizes.py compares the device with the oracle."""
import functools

import numpy as np

FX_TILE = 4096          # csrc/gkc_fastx.hip FX_TILE = FX_THREADS * FX_PER: bytes of text per workgroup
FX_PER = 16             # csrc/gkc_fastx.hip FX_PER: bytes per thread (one 16-byte load)
FX_WAVE = 1024          # 64 lanes * FX_PER: bytes per wave, the unit of fx_wg_excl's shuffle scan
FXS_CHUNK = 8192        # csrc/gkc_fastx.hip FXS_CHUNK = 1024 * FXS_ITEMS: entries per workgroup of fx_scan; beyond it k_fx_scan_totals / k_fx_scan_add carry

PHASES = tuple(range(-17, 18))          # one thread's 16 bytes and one more on either side of a tile border
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NL, CR = 10, 13


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def fasta_fill(rng, n, eol=b"\n"):
    """exactly n bytes of whole, ordinary FASTA records: a two-byte header and two lines of 60 bases; the last record takes what is left in lines of at most 60"""
    e = len(eol)
    assert n >= 3 + 2 * e, n
    out, left = [], n
    while left >= 2 + e + 2 * (60 + e) + 3 + 2 * e:
        out += [b">p", eol, _bases(rng, 60), eol, _bases(rng, 60), eol]; left -= 2 + e + 2 * (60 + e)
    out += [b">p", eol]
    left -= 2 + e
    while left > 60 + e + 1 + e:
        out += [_bases(rng, 60), eol]; left -= 60 + e
    out += [_bases(rng, left - e), eol]
    return b"".join(out)


def fastq_fill(rng, n, eol=b"\n"):
    """exactly n bytes of whole four-line FASTQ records of about 50 bases; qualities from '@>+I'"""
    e = len(eol)
    qual = np.frombuffer(b"@>+I", dtype=np.uint8)

    def rec(name, nb):
        return b"".join([b"@", name, eol, _bases(rng, nb), eol, b"+", eol, qual[rng.integers(0, 4, nb)].tobytes(), eol])
    small = 3 + 4 * e                   # "@q" + '+' + four line ends: a record of nb bases has small + 2 nb bytes, with "@qq" one more
    assert n >= small, n
    out, left = [], n
    while left > 2 * (small + 100) + 1:
        out.append(rec(b"q", 50)); left -= small + 100
    if (left - small) % 2 == 0:
        out.append(rec(b"q", (left - small) // 2))
    else:
        out.append(rec(b"qq", (left - small - 1) // 2))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ a. one feature at every phase of a tile border
# name -> (FASTQ?, line end, bytes of the feature's record before the feature, the feature's byte, the rest of the record)
FEATURES = {
    "seq_newline":     (False, b"\n",   b">s\nACGTTGCAAGGCTATTCAGA", b"\n", b"GATTACA\n"),                         # the '\n' of a sequence line
    "crlf_cr":         (False, b"\r\n", b">s\r\nACGTTGCAAGGCTATTCAGA", b"\r", b"\nGATTACA\r\n"),                   # the '\r' of a "\r\n"; at d = -1 the '\r' ends a tile
    "header_gt":       (False, b"\n",   b"", b">", b"h 1\nACGTTGCA\nGG\n"),                                         # the '>' of a header line
    "blank_line":      (False, b"\n",   b">s\nACGTTGCA\n", b"\n", b"TTGA\n"),                                       # a blank line between two sequence lines
    "lone_cr_first":   (False, b"\n",   b">s\n", b"\r", b"\nACGT\n"),                                               # a line that is exactly "\r", first non-empty line: kept
    "lone_cr_later":   (False, b"\n",   b">s\nACGT\n", b"\r", b"\nTT\n"),                                           # ... as a later line: dropped
    "fastq_plus":      (True,  b"\n",   b"@r\nACGTTGCAAG\n", b"+", b"r\n@I+>@I+>@I\n"),                             # the '+' line
    "fastq_qual_at":   (True,  b"\n",   b"@r\nACGTTGCAAG\n+\n", b"@", b"I+>@I+>@I\n"),                              # a quality line whose first byte is '@'
    "fastq_crlf_qual": (True,  b"\r\n", b"@r\r\nACGTTG\r\n+\r\nI@+>II", b"\r", b"\n"),                              # CRLF, stripped quality as long as the sequence: its '\r'
}


@functools.lru_cache(maxsize=None)
def feature_at_every_phase(name):
    """-> (text, [(d, P)]): the feature's byte at P = FX_TILE * (i + 1) + d for the i-th d of PHASES, one border per phase, ordinary records between"""
    fastq, eol, pre, feat, post = FEATURES[name]
    rng = np.random.default_rng(sorted(FEATURES).index(name))
    fill = fastq_fill if fastq else fasta_fill
    out, n, claims = [], 0, []
    for i, d in enumerate(PHASES):
        P = FX_TILE * (i + 1) + d
        gap = P - len(pre) - n
        out += [fill(rng, gap, eol), pre, feat, post]
        n = P + 1 + len(post)
        claims.append((d, P))
    out.append(fill(rng, 200, eol))
    return b"".join(out), claims


# ------------------------------------------------------------------------------------------------ b. tiles without a newline
@functools.lru_cache(maxsize=None)
def long_sequence_line():
    """-> (text, start, length): one sequence line of 3 * FX_TILE + 5 bases"""
    rng = np.random.default_rng(11)
    head = fasta_fill(rng, 777) + b">genome\n"
    L = 3 * FX_TILE + 5
    return head + _bases(rng, L) + b"\n" + fasta_fill(rng, 300), len(head), L


@functools.lru_cache(maxsize=None)
def long_header_line():
    """-> (text, start, length): a header line of FX_TILE + 100 bytes ('>' included, with blanks, '>' and '@' inside)"""
    rng = np.random.default_rng(12)
    head = fasta_fill(rng, 1500)
    L = FX_TILE + 100
    words = np.frombuffer(b"abc XYZ_0123|:>@+ \t", dtype=np.uint8)
    return head + b">" + words[rng.integers(0, len(words), L - 1)].tobytes() + b"\nACGTTGCA\nGGA\n" + fasta_fill(rng, 300), len(head), L


@functools.lru_cache(maxsize=None)
def long_fastq_record():
    """-> (text, start of the sequence line, length): a FASTQ record of 2 * FX_TILE + 1 bases, quality from '@>+I'"""
    rng = np.random.default_rng(13)
    head = fastq_fill(rng, 1000) + b"@long\n"
    L = 2 * FX_TILE + 1
    q = np.frombuffer(b"@>+I", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
    return head + _bases(rng, L) + b"\n+\n" + q + b"\n" + fastq_fill(rng, 400), len(head), L


@functools.lru_cache(maxsize=None)
def lines_from_a_border():
    """-> (text, [(start, length)]): sequence lines that start on a tile border, with FX_TILE - 1, FX_TILE and FX_TILE + 1 bytes of content"""
    rng = np.random.default_rng(14)
    out, n, claims = [], 0, []
    for L in (FX_TILE - 1, FX_TILE, FX_TILE + 1):
        start = (n // FX_TILE + 2) * FX_TILE
        out += [fasta_fill(rng, start - 3 - n), b">x\n", _bases(rng, L), b"\n"]
        claims.append((start, L)); n = start + L + 1
    out.append(fasta_fill(rng, 100))
    return b"".join(out), claims


# ------------------------------------------------------------------------------------------------ c. text ends
END_TILES = (1, 2)
END_RESIDUES = (0, 1, 15, 16, 17, 4095)


@functools.lru_cache(maxsize=None)
def text_of_length(n, fastq, final_newline):
    """a text of exactly n bytes; without the final newline its last line is unterminated"""
    rng = np.random.default_rng(n + 2 * fastq)
    fill = fastq_fill if fastq else fasta_fill
    return fill(rng, n) if final_newline else fill(rng, n + 1)[:-1]


# about 150 bytes each: junk before the first header, blank lines, multi-line records, an empty record, a header with a comment
SMALL_FASTA_LF = (b"junk line\n\n>r1 first\nACGTACGTAC\nGGTTA\n\nCCA\n>r2\n\n\nTTGACA\n>r3\n>r4 empty before\nA\nC\n\nGGGTACCATG\nAC\n"
                  b">r5\tx\nNNACGTNN\nacgtac\n\n\n>r6\nGATTACAGATTACA\nTT\n>r7\nAC\n")
SMALL_FASTA_CRLF = (b"junk line\r\n\r\n>r1 first\r\nACGTACGTAC\r\nGGTTA\r\n\r\nCCA\r\n>r2\r\n\r\n\r\nTTGACA\r\n>r3\r\n>r4 x\r\nA\r\nC\r\n\r\nGGGTAC\r\n"
                    b">r5\tx\r\nNNACGTNN\r\nacgtac\r\n\r\n\r\n>r6\r\nGATTACAGA\r\nTT\r\n")
SMALL_FASTQ_LF = (b"@q1 first\nACGTACGTAC\n+\n@III>+@III\n@q2\nGGTTAACC\n+q2\n@@@@@@@@\n@q3\n\n+\n\n@q4\nTTGACATTGACATT\n+\n>>>>++++IIII@@\n"
                  b"@q5\nA\n+\n@\n@q6\nACGTNNAC\n+\n+I+I+I+I\n@q7\nGATT\n+\nI@I@\n")
SMALL_FASTQ_CRLF = (b"@q1 first\r\nACGTACGTAC\r\n+\r\n@III>+@III\r\n@q2\r\nGGTTAACC\r\n+q2\r\n@@@@@@@@\r\n@q3\r\nTTGACATTGAC\r\n+\r\n>>>>++++III\r\n"
                    b"@q4\r\nAC\r\n+\r\n@I\r\n@q5\r\nACGTNNAC\r\n+\r\n+I+I+I+I\r\n@q6\r\nGATT\r\n+\r\nI@I@\r\n")
SMALL_TEXTS = {"fasta_lf": (SMALL_FASTA_LF, False), "fasta_crlf": (SMALL_FASTA_CRLF, False), "fastq_lf": (SMALL_FASTQ_LF, True), "fastq_crlf": (SMALL_FASTQ_CRLF, True)}

# the ending the oracle and the device used to disagree on: a lone '\r' as the unterminated last line, after bases of the same record (kept, like the reference)
LONE_CR_ENDINGS = (b">a\nAC\n\r", b">a\nAC\r\n\r")
LONE_CR_TERMINATED = b">a\nAC\n\r\n"


def lone_cr_prefixes(text):
    """the prefix lengths of a FASTA text that end in a lone '\\r' line which follows a non-empty line of the same record (bases, or a first "\\r" line that was
    kept): terminated, that '\\r' would be dropped"""
    out = []
    for c in range(2, len(text) + 1):
        if text[c - 1] == CR and text[c - 2] == NL and b">" in text[:c]:
            rec = text[:c - 1].rsplit(b">", 1)[-1]
            if any(len(ln) > 0 for ln in rec.split(b"\n")[1:]):
                out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ d. the chunk contract
def line_starts(chunk):
    """start of every line of the chunk, an unterminated last line included"""
    a = np.frombuffer(chunk, dtype=np.uint8)
    s = np.concatenate([[0], np.flatnonzero(a == NL) + 1])
    return s[s < len(chunk)] if len(chunk) else s[:0]


def expected_consumed(chunk, fastq):
    """bytes a non-final chunk hands on, from the text alone. FASTA: the start of the last line that begins with '>' or '@' (the record it opens may go on in
    the next chunk), 0 without one. FASTQ: the start of line 4 * (complete lines // 4)."""
    s = line_starts(chunk)
    if fastq:
        j = 4 * (chunk.count(b"\n") // 4)
        return int(s[j]) if j < len(s) else len(chunk)
    heads = [int(p) for p in s if chunk[p] in b">@"]
    return heads[-1] if heads else 0


def record_starts(text, fastq):
    """where a record of the whole text starts: every fourth line (FASTQ), every line that begins with '>' (FASTA)"""
    s = line_starts(text)
    return {int(p) for p in s[::4]} if fastq else {int(p) for p in s if text[p] in b">@"}


@functools.lru_cache(maxsize=None)
def three_tile_text(fastq):
    """-> (text, cuts): a text of three tiles and the cuts FX_TILE * t + d, t = 1, 2, d in PHASES"""
    rng = np.random.default_rng(21 + fastq)
    out, n = [], 0
    while n < 3 * FX_TILE - 40:                         # records of 6 .. 21 bytes: several record starts among the 35 cuts of a border
        nb = int(rng.integers(1, 6))
        q = np.frombuffer(b"@>+I", dtype=np.uint8)[rng.integers(0, 4, nb)].tobytes()
        out.append(b"@r\n" + _bases(rng, nb) + b"\n+\n" + q + b"\n" if fastq else b">r\n" + _bases(rng, nb) + b"\n" + (_bases(rng, nb) + b"\n") * int(rng.integers(0, 2)))
        n += len(out[-1])
    return b"".join(out), [FX_TILE * t + d for t in (1, 2) for d in PHASES]


# ------------------------------------------------------------------------------------------------ e. the prefix scan's chunk
SCAN_LINE_COUNTS = (FXS_CHUNK - 1, FXS_CHUNK, FXS_CHUNK + 1, 2 * FXS_CHUNK + 1)


@functools.lru_cache(maxsize=None)
def many_short_lines(n_lines, header_parity):
    """-> text of n_lines lines in records of two lines of a few bytes; header_parity 0: headers on the even lines (line 8192 is one), 1: one line of junk first, headers
    on the odd lines (line 8191 is one). Lines count from 0. The record-id scan runs over the lines, so it crosses its chunk between lines 8191 and 8192."""
    rng = np.random.default_rng(n_lines + header_parity)
    lines = [b"junk"] if header_parity else []
    i = 0
    while len(lines) < n_lines:
        lines.append(b">%x" % i if (len(lines) - header_parity) % 2 == 0 else _bases(rng, 1 + i % 5)); i += 1
    return b"\n".join(lines) + b"\n"


MANY_TILES_RECORDS = 223797           # 150-byte records: 33 569 550 bytes = 8195 whole tiles and one started: tiles 8192 .. 8195 lie in the second chunk of the tile scans


@functools.lru_cache(maxsize=None)
def many_tiles_text():
    """70-column FASTA of more than FXS_CHUNK tiles: records of an 8-byte header line and two lines of 70 bases, built as one (records, 150) array"""
    rng = np.random.default_rng(31)
    R = MANY_TILES_RECORDS
    a = np.empty((R, 150), dtype=np.uint8)
    a[:, 0] = ord(">")
    idx = np.arange(R)
    for j in range(6):                                   # six hexadecimal digits of the record's number
        a[:, 1 + j] = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)[(idx >> (4 * (5 - j))) & 15]
    a[:, 7] = NL
    a[:, 8:] = ACGT[rng.integers(0, 4, (R, 142), dtype=np.uint8)]
    a[:, 78] = NL; a[:, 149] = NL
    return a.tobytes()
