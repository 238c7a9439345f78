"""Golden vector of the reference's OWN links between unitigs: repeats the run of run_unitigs in tools/make_reference_run_vectors.py (the same reads, k = 21,
abundance-min 2, the reference's dbgh5 in the mode GraphUnitigs forces, then oracle/_ref/ref/unitigs_check: GraphUnitigs -> bcalm2 -> LinkTigs), checks that the
.unitigs.fa it reads reproduces the committed digest of the unitig set (k21_freq_4parts_unitigs.json), and writes the L: fields of its headers, made independent of the
numbering and of the stored orientation, to tests/golden/reference_run/k21_freq_4parts_unitig_links.json. It rewrites no other fixture.

    python tools/make_unitig_links_vector.py [directory with dbgh5 and unitigs_check] [--out FILE]

The digest: each link one line "ru su rv sv" — ru / rv the ranks of the two unitigs' canonical sequences among all sorted canonical sequences, su the side left
through ('+': the end, '-': the begin), sv the sign arrived with, both relative to the canonical orientation (a unitig stored as the reverse complement of its
canonical form has its side and its sign flipped) — the lines sorted, joined by newlines, sha256."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import synth_reads  # noqa: E402

_args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--out"]
BIN = _args[0] if _args else os.path.join(ROOT, "oracle", "_ref", "ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_run")
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(GOLDEN, "k21_freq_4parts_unitig_links.json")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def read_unitigs(fa):
    """-> (ids, sequences, links): links as (unitig id, side '+' / '-', unitig id, sign '+' / '-'), from the L:<side>:<unitig>:<sign> fields of the headers"""
    ids, seqs, links = [], [], []
    for line in open(fa, "rb"):
        line = line.strip()
        if not line.startswith(b">"):
            seqs.append(line)
            continue
        toks = line[1:].decode().split()
        ids.append(int(toks[0]))
        for tok in toks[1:]:
            if tok[:2] == "L:":
                _, side, v, sign = tok.split(":")
                links.append((ids[-1], side, int(v), sign))
    assert len(ids) == len(seqs) == len(set(ids))
    return ids, seqs, links


def digests(ids, seqs, links):
    can = [min(s, s.translate(_COMP)[::-1]) for s in seqs]
    order = sorted(can)
    unitigs = [len(order), sum(len(x) for x in order), hashlib.sha256(b"\n".join(order)).hexdigest()]
    rank = {c: r for r, c in enumerate(order)}
    assert len(rank) == len(seqs)
    at = {u: i for i, u in enumerate(ids)}
    flip = [c != s for c, s in zip(can, seqs)]
    other = {"+": "-", "-": "+"}
    lines = []
    for u, su, v, sv in links:
        iu, iv = at[u], at[v]
        lines.append("%d %s %d %s" % (rank[can[iu]], other[su] if flip[iu] else su, rank[can[iv]], other[sv] if flip[iv] else sv))
    lines.sort()
    return unitigs, [len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()]


def main():
    k = 21
    exe = os.path.join(BIN, "unitigs_check")
    for need in (exe, os.path.join(BIN, "dbgh5")):
        if not os.path.exists(need):
            sys.exit("no %s: the reference binaries are not built" % need)
    reads = synth_reads(6000, 30000, 150, seed=43, n_rate=0.002)
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "in.fa")
        open(fa, "w").write("".join(">r%d\n%s\n" % (i, r.decode()) for i, r in enumerate(reads)))
        subprocess.run([os.path.join(BIN, "dbgh5"), "-in", fa, "-kmer-size", str(k), "-abundance-min", "2", "-out", os.path.join(td, "ref"), "-out-tmp", td, "-nb-cores", "1",
                        "-max-memory", "1", "-verbose", "0", "-bloom", "none", "-debloom", "none", "-branching-nodes", "none", "-no-mphf", "-minimizer-type", "1", "-repartition-type", "1"],
                       check=True, capture_output=True)
        subprocess.run([exe, os.path.join(td, "ref.h5"), os.path.join(td, "from_h5"), "1"], check=True, capture_output=True, cwd=td)
        ids, seqs, links = read_unitigs(os.path.join(td, "from_h5.unitigs.fa"))
    unitigs, (n_links, sha) = digests(ids, seqs, links)
    want = json.load(open(os.path.join(GOLDEN, "k21_freq_4parts_unitigs.json")))
    assert unitigs == [want["unitigs"], want["total_length"], want["sha256_sorted_canonical"]], ("the unitigs read are not those of the committed fixture", unitigs)
    json.dump({"k": k, "unitigs": unitigs[0], "links": n_links, "sha256_sorted_links": sha}, open(OUT, "w"))
    degree = {}
    for u, su, _, _ in links:
        degree[(u, su)] = degree.get((u, su), 0) + 1
    hist = [2 * len(ids) - len(degree)] + [sum(d == n for d in degree.values()) for n in range(1, 5)]
    print("k21_freq_4parts_unitig_links: %d links over %d unitigs, %d self-links, sides with 0..4 links: %s, sha256 %s" % (n_links, unitigs[0], sum(u == v for u, _, v, _ in links), hist, sha))


if __name__ == "__main__":
    main()
