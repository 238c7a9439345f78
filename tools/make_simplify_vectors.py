"""Collects the known-answer DATA of the reference's unit tests debruijn_simplunitigs_bubble, _bubble_snp and _ec (test/unit/src/debruijn/TestSimplificationsUnitigs.cpp)
into tests/golden/reference_simplify_vectors.json: per test k, the input sequences, the node counts the reference asserts before and after graph.simplify(), and the
sequences it expects to traverse afterwards. Only data is extracted (nucleotide strings and integers), the way tools/make_tip_vector.py does. No reference code is copied.

usage: make_simplify_vectors.py <root of the reference's gatb-core> [output json]"""
import json
import re
import sys

src = open(sys.argv[1].rstrip("/") + "/test/unit/src/debruijn/TestSimplificationsUnitigs.cpp").read()


def block(name, end):
    i = src.index("void %s" % name)
    return src[i: src.index(end, i + 1)]


def strings(text):
    return re.findall(r'"([ACGT]+)"', text)


def nodes(text):
    return [int(x) for x in re.findall(r"CPPUNIT_ASSERT \(r\.nbNodes == (\d+)\);", text)]


aux = block("debruijn_simplunitigs_bubble_aux", "void debruijn_simplunitigs_bubble ()")
k = int(re.search(r"size_t kmerSize = (\d+);", aux).group(1))
aux_nodes = nodes(aux[: aux.index("if (0)")])                      # (the block after it is switched off in the reference)
assert aux_nodes == [8, 6], aux_nodes
out = {}
for name, end in (("debruijn_simplunitigs_bubble ()", "void debruijn_simplunitigs_bubble_snp"), ("debruijn_simplunitigs_bubble_snp()", "void debruijn_simplunitigs_ec")):
    blk = block(name, end)
    j = blk.index("const char* sequences[] =")
    e = blk.index("};", j)
    seqs, sols = strings(blk[j: e]), strings(blk[e:])
    key = "bubble_snp" if "snp" in name else "bubble"
    assert len(seqs) == (9 if key == "bubble_snp" else 6) and len(sols) == (2 if key == "bubble_snp" else 1), (len(seqs), len(sols))
    out[key] = dict(k=k, sequences=seqs, nodes_before=aux_nodes[0], nodes_after=aux_nodes[1], traversals=sols)
blk = block("debruijn_simplunitigs_ec ()", "CPPUNIT_TEST_SUITE_REGISTRATION")
j = blk.index("const char* sequences[] =")
e = blk.index("};", j)
seqs, sols = strings(blk[j: e]), strings(blk[e:])
ec_nodes = nodes(blk)
assert len(seqs) == 16 and len(sols) == 2 and ec_nodes == [10, 8], (len(seqs), len(sols), ec_nodes)
out["ec"] = dict(k=int(re.search(r"size_t kmerSize = (\d+);", blk).group(1)), sequences=seqs, nodes_before=ec_nodes[0], nodes_after=ec_nodes[1], traversals=sols,
                 traversal_starts=[0, 3])                          # (the indices of the sequences the reference starts its two traversals from)
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "tests/golden/reference_simplify_vectors.json", "w"), indent=1)
for key, v in out.items():
    print(key, v["k"], [len(s) for s in v["sequences"]], v["nodes_before"], v["nodes_after"], [len(s) for s in v["traversals"]])
