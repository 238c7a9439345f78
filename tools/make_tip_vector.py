"""Collects the known-answer DATA of the reference's unit test debruijn_simplunitigs_tip (test/unit/src/debruijn/TestSimplificationsUnitigs.cpp) into
tests/golden/reference_tip_vector.json: the three input sequences, k, and the sequence the reference expects to traverse after graph.simplify(). Only data is
extracted (nucleotide strings and one integer), the way tools/make_reference_test_vectors.py makes reference_unit_vectors.json. No reference code is copied.

usage: make_tip_vector.py <root of the reference's gatb-core> [output json]"""
import json
import re
import sys

src = open(sys.argv[1].rstrip("/") + "/test/unit/src/debruijn/TestSimplificationsUnitigs.cpp").read()
i = src.index("void debruijn_simplunitigs_tip ()")
blk = src[i: src.index("void debruijn_simplunitigs_bubble_aux", i)]
k = int(re.search(r"size_t kmerSize = (\d+);", blk).group(1))
j = blk.index("const char* sequences[] =")
seqs = re.findall(r'"([ACGT]+)"', blk[j: blk.index("};", j)])
assert len(seqs) == 3, len(seqs)
nodes = [int(x) for x in re.findall(r"CPPUNIT_ASSERT \(r\.nbNodes == (\d+)\);", blk)]
assert nodes == [6, 4], nodes
rest = blk[blk.index("graph.simplify"):]
want = max(re.findall(r'"([ACGT]+)"', rest), key=len)                # the one string after simplify(): the traversal the reference asserts
assert len(want) > len(seqs[0])
out = dict(k=k, sequences=seqs, extremity_nodes_before=nodes[0], extremity_nodes_after=nodes[1], traversal=want)
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "tests/golden/reference_tip_vector.json", "w"), indent=1)
print(k, [len(s) for s in seqs], nodes, len(want))
