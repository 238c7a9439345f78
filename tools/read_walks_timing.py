"""Developer probe: what joining a read's segments across the unitig links costs on the device (not part of the product). Same input as tools/read_paths_timing.py. In one
process, after a warm-up, every round times
  (a) gkc_query_reads_device            : the yardstick — the same search, answering with the abundance;
  (b) gkc_graph_reads_nodes_device      : on the placement the context holds;
  (c) gkc_graph_reads_segments_device   : the sizing call and the fill, on the nodes of (b);
  (d) gkc_graph_reads_walks_device      : the sizing call and the fill (junctions, walks and link support), on the segments of (c) and the links of the placement,
first on the placement of the plain build, then on the one gkc_graph_simplify leaves. Every timed span is wall time around a call that ends in a stream synchronise; the
index and the links are built before the first timed call. Prints per round and the median / min / max.
Condition checked at the end, per placement: the chain a user runs, median (b) + (c) + (d), <= 1.5 x median (a).
usage: read_walks_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]      (the output is kept in profiles/read_walks_timing.txt)"""
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
seg_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda"); walk_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def wall(f):
    t0 = time.perf_counter(); r = f(); return (time.perf_counter() - t0) * 1e3, r


def line(label, v):
    v = np.array(v)
    print("%-64s median %8.2f ms   min %8.2f   max %8.2f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))


def measure(label, nu, d_masks):
    lo, lk = c._unitig_links_of_placement(nu, d_masks)
    nl = len(lk)
    res = {name: [] for name in ("query", "nodes", "seg_sizing", "seg_fill", "walk_sizing", "walk_fill")}
    segments = walks = junction = None
    support = torch.empty(nl + 1, dtype=torch.int64, device="cuda")
    for rnd in range(-1, rounds):
        q, _ = wall(lambda: c.query_reads_device(db, do, n, nb, out.data_ptr()))
        a, _ = wall(lambda: c.read_nodes_device(db, do, n, nb, node.data_ptr(), pos.data_ptr()))
        s, n_seg = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb))
        if segments is None:
            segments = torch.empty(max(n_seg, 1) * 24, dtype=torch.uint8, device="cuda"); junction = torch.empty(max(n_seg, 1), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
        f, got = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb, seg_offsets.data_ptr(), segments.data_ptr(), n_seg))
        assert got == n_seg
        args = (seg_offsets.data_ptr(), segments.data_ptr(), n, n_seg, lo.data_ptr(), lk.data_ptr(), nl)
        ws, n_walks = wall(lambda: c.read_walks_device(*args))
        if walks is None:
            walks = torch.empty(max(n_walks, 1) * 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        wf, got = wall(lambda: c.read_walks_device(*args, junction.data_ptr(), walk_offsets.data_ptr(), walks.data_ptr(), n_walks, support.data_ptr()))
        assert got == n_walks
        print("%s, %s: query %.1f ms   nodes %.1f ms   segments: sizing %.1f ms, fill %.1f ms (%d)   walks: sizing %.1f ms, fill %.1f ms (%d)"
              % (label, "warm-up" if rnd < 0 else "round %d" % rnd, q, a, s, f, n_seg, ws, wf, n_walks))
        if rnd >= 0:
            for name, v in (("query", q), ("nodes", a), ("seg_sizing", s), ("seg_fill", f), ("walk_sizing", ws), ("walk_fill", wf)):
                res[name].append(v)
    j = junction[:n_seg]
    n_link = int((j >= 0).sum()); ends = [int((j == -x).sum()) for x in (1, 2, 3, 4)]      # (the values that are no link index, as signed 64-bit values)
    assert n_link + sum(ends) == n_seg and n_walks == n_seg - n_link and int(support[:nl].sum()) == n_link and int(walk_offsets[n]) == n_walks
    print("%s: %d unitigs, %d links; %d segments, %d walks (%.2f per read); junctions: %d link, %d unlinked, %d collinear, %d break, %d end"
          % (label, nu, nl, n_seg, n_walks, n_walks / n, n_link, ends[3], ends[2], ends[1], ends[0]))
    line(label + ": (a) gkc_query_reads_device", res["query"])
    line(label + ": (b) gkc_graph_reads_nodes_device", res["nodes"])
    line(label + ": (c) gkc_graph_reads_segments_device, sizing call", res["seg_sizing"])
    line(label + ": (c) gkc_graph_reads_segments_device, fill", res["seg_fill"])
    line(label + ": (d) gkc_graph_reads_walks_device, sizing call", res["walk_sizing"])
    line(label + ": (d) gkc_graph_reads_walks_device, fill", res["walk_fill"])
    med = {name: float(np.median(v)) for name, v in res.items()}
    chain = med["nodes"] + med["seg_sizing"] + med["seg_fill"] + med["walk_sizing"] + med["walk_fill"]
    print("%s: walks %.2f ms = %.3f ns per segment; chain nodes + segments + walks %.1f ms, %.2f x the query; condition chain <= 1.5 x median query %.1f ms = %.1f ms: %s"
          % (label, med["walk_sizing"] + med["walk_fill"], (med["walk_sizing"] + med["walk_fill"]) * 1e6 / max(n_seg, 1), chain, chain / med["query"], med["query"], 1.5 * med["query"],
             "met" if chain <= 1.5 * med["query"] else "MISSED"))


keep, d_masks = c._masks_once(None)
nu, _, _ = c.unitigs_build(d_masks)
measure("plain placement", nu, d_masks)
w, got = wall(lambda: c.simplify())
print("simplify: %.1f ms, %d rounds, %d records removed, %d unitigs left" % (w, got["rounds"], got["records_removed"], got["n_unitigs"]))
measure("simplified placement", got["n_unitigs"], c._placement_masks.data_ptr())
for name in ("query_reads", "graph_read_nodes", "graph_read_segments", "graph_read_walks"):
    ms, launches = c.timing(name)
    print("gkc_get_timing %-20s %10.1f ms over %d intervals" % (name, ms, launches))
c.device_free(db); c.device_free(do)
c.close()
