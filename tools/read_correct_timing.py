"""Developer probe: what rewriting the reads to what the graph says costs on the device (not part of the product). Same input as tools/read_walks_timing.py. In one
process, after a warm-up, every round times
  (a) gkc_query_reads_device            : the yardstick of the chain — the same search, answering with the abundance;
  (b) gkc_graph_reads_nodes_device      : on the placement the context holds;
  (c) gkc_graph_reads_segments_device   : the sizing call and the fill, on the nodes of (b);
  (d) gkc_graph_reads_correct_device    : out of place (every output given), on the segments of (c) and the unitig strings of the placement;
  (e) gkc_graph_reads_correct_device    : in place, on a fresh copy of the reads made before the timed span (the same call without segments: a copy),
first on the placement of the plain build, then on the one gkc_graph_simplify leaves. Every timed span is wall time around a call that ends in a stream synchronise; the
index and the unitig strings are built before the first timed call. Prints per round and the median / min / max.
Condition checked at the end, per placement: median (d) <= median (c) sizing + fill, the existing call on the same reads and the same placement in the same process.
usage: read_correct_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]      (the output is kept in profiles/read_correct_timing.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as ge
import bench

gkc = ge.load().gkc
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
parts = int(sys.argv[2]) if len(sys.argv) > 2 else 512
k = int(sys.argv[3]) if len(sys.argv) > 3 else 31
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
L, m = 150, 10
os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
db, do = c.synth_reads_device(2, n, L, n * 5, 10000)
nb = n * L
c.begin_pass(0); c.push_reads_device(db, do, n, nb); c.finish_pass()
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d positions per call, %d solid k-mers" % (n, L, k, m, parts, nb, c.stats()["kmers_nb_solid"]))
out = torch.empty(nb + 16, dtype=torch.int32, device="cuda")
node = torch.empty(nb + 16, dtype=torch.int64, device="cuda"); pos = torch.empty(nb + 16, dtype=torch.int32, device="cuda")
seg_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
corrected = torch.empty(nb + 16, dtype=torch.uint8, device="cuda"); there = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
no_segments = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
n_changed = torch.empty(n, dtype=torch.int32, device="cuda"); bits = torch.empty((nb + 63) // 64, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def wall(f):
    t0 = time.perf_counter(); r = f(); return (time.perf_counter() - t0) * 1e3, r


def line(label, v):
    v = np.array(v)
    print("%-72s median %8.2f ms   min %8.2f   max %8.2f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))


def measure(label, nu, nub):
    ub = torch.empty(max(nub, 16), dtype=torch.uint8, device="cuda"); uo = torch.empty(nu + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c._chk(c.L.gkc_graph_unitigs_write(c.h, ub.data_ptr(), nub, uo.data_ptr(), nu, None))
    res = {name: [] for name in ("query", "nodes", "seg_sizing", "seg_fill", "correct", "in_place")}
    segments = first = None
    for rnd in range(-1, rounds):
        q, _ = wall(lambda: c.query_reads_device(db, do, n, nb, out.data_ptr()))
        a, _ = wall(lambda: c.read_nodes_device(db, do, n, nb, node.data_ptr(), pos.data_ptr()))
        s, n_seg = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb))
        if segments is None:
            segments = torch.empty(max(n_seg, 1) * 24, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        f, got = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb, seg_offsets.data_ptr(), segments.data_ptr(), n_seg))
        assert got == n_seg
        args = (do, n, nb, seg_offsets.data_ptr(), segments.data_ptr(), n_seg, ub.data_ptr(), uo.data_ptr())
        w, st = wall(lambda: c.correct_reads_device(db, *args, corrected.data_ptr(), 2, True, n_changed.data_ptr(), bits.data_ptr()))
        # the reads once more for the in-place call, outside the timed span: without segments the call is a copy
        c.correct_reads_device(db, do, n, nb, no_segments.data_ptr(), None, 0, ub.data_ptr(), uo.data_ptr(), there.data_ptr())
        wi, sti = wall(lambda: c.correct_reads_device(there.data_ptr(), *args, there.data_ptr(), 2, True, n_changed.data_ptr(), bits.data_ptr()))
        if first is None:
            first = st
        assert st == first == sti and torch.equal(there[:nb], corrected[:nb]) and int(n_changed.sum()) == st["bases_changed"]
        print("%s, %s: query %.1f ms   nodes %.1f ms   segments: sizing %.1f ms, fill %.1f ms (%d)   correct: out of place %.1f ms, in place %.1f ms"
              % (label, "warm-up" if rnd < 0 else "round %d" % rnd, q, a, s, f, n_seg, w, wi))
        if rnd >= 0:
            for name, v in (("query", q), ("nodes", a), ("seg_sizing", s), ("seg_fill", f), ("correct", w), ("in_place", wi)):
                res[name].append(v)
    print("%s: %d unitigs of %d bases; %d segments; out of place: %s" % (label, nu, nub, n_seg, first))
    line(label + ": (a) gkc_query_reads_device", res["query"])
    line(label + ": (b) gkc_graph_reads_nodes_device", res["nodes"])
    line(label + ": (c) gkc_graph_reads_segments_device, sizing call", res["seg_sizing"])
    line(label + ": (c) gkc_graph_reads_segments_device, fill", res["seg_fill"])
    line(label + ": (d) gkc_graph_reads_correct_device, out of place", res["correct"])
    line(label + ": (e) gkc_graph_reads_correct_device, in place", res["in_place"])
    med = {name: float(np.median(v)) for name, v in res.items()}
    seg = med["seg_sizing"] + med["seg_fill"]
    chain = med["nodes"] + seg + med["correct"]
    print("%s: correct %.2f ms = %.3f ns per base, %.3f ns per segment; in place %.2f ms; chain nodes + segments + correct %.1f ms, %.2f x the query (%.1f ms)"
          % (label, med["correct"], med["correct"] * 1e6 / nb, med["correct"] * 1e6 / max(n_seg, 1), med["in_place"], chain, chain / med["query"], med["query"]))
    print("%s: condition correct out of place <= segments sizing + fill: %.2f ms against %.2f ms: %s" % (label, med["correct"], seg, "held" if med["correct"] <= seg else "MISSED"))


keep, d_masks = c._masks_once(None)
nu, nub, _ = c.unitigs_build(d_masks)
measure("plain placement", nu, nub)
w, got = wall(lambda: c.simplify())
print("simplify: %.1f ms, %d rounds, %d records removed, %d unitigs left" % (w, got["rounds"], got["records_removed"], got["n_unitigs"]))
measure("simplified placement", got["n_unitigs"], got["n_bases"])
for name in ("query_reads", "graph_read_nodes", "graph_read_segments", "graph_read_correct"):
    ms, launches = c.timing(name)
    print("gkc_get_timing %-20s %10.1f ms over %d intervals" % (name, ms, launches))
c.device_free(db); c.device_free(do)
c.close()
