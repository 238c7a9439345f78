"""Developer probe: what threading reads through the compacted graph costs on the device (not part of the product). Same input as tools/query_timing.py. In one process,
after a warm-up, every round times
  (a) gkc_query_reads_device            : the yardstick — the same search, answering with the abundance;
  (b) gkc_graph_reads_nodes_device      : on the placement of the plain build (rounds 0 .. n - 1 first), and
  (c) the same on the placement gkc_graph_simplify leaves (a second set of rounds, with (a) timed again beside it);
  (d) gkc_graph_reads_segments_device   : the sizing call and the fill, on the nodes of (b) / (c).
Every timed span is wall time around a call that ends in a stream synchronise; the index is built before the first timed call. Prints per round and the median / min / max.
Condition checked at the end: median (b) <= 1.5 x median (a), and the same for (c) against the (a) of its rounds.
usage: read_paths_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]"""
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
ns = c.stats()["kmers_nb_solid"]
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d positions per call, %d solid k-mers" % (n, L, k, m, parts, nb, ns))
out = torch.empty(nb + 16, dtype=torch.int32, device="cuda")
node = torch.empty(nb + 16, dtype=torch.int64, device="cuda"); pos = torch.empty(nb + 16, dtype=torch.int32, device="cuda")
seg_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def wall(f):
    t0 = time.perf_counter(); r = f(); return (time.perf_counter() - t0) * 1e3, r


def line(label, v):
    v = np.array(v)
    print("%-56s median %8.2f ms   min %8.2f   max %8.2f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))


def measure(label, nu):
    """rounds of (a), (b) / (c), (d) on the placement the context holds -> (median query, median nodes)"""
    support = torch.empty(nu + 1, dtype=torch.int64, device="cuda")
    res = {"query": [], "nodes": [], "nodes_no_pos": [], "sizing": [], "fill": []}
    segments = None
    for rnd in range(-1, rounds):
        q, _ = wall(lambda: c.query_reads_device(db, do, n, nb, out.data_ptr()))
        a, _ = wall(lambda: c.read_nodes_device(db, do, n, nb, node.data_ptr(), pos.data_ptr()))
        s, n_seg = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb))
        if segments is None:
            segments = torch.empty(max(n_seg, 1) * 24, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        f, got = wall(lambda: c.read_segments_device(node.data_ptr(), pos.data_ptr(), do, n, nb, seg_offsets.data_ptr(), segments.data_ptr(), n_seg, support.data_ptr()))
        assert got == n_seg
        a0, _ = wall(lambda: c.read_nodes_device(db, do, n, nb, node.data_ptr(), None))
        print("%s, %s: query %.1f ms   nodes %.1f ms   nodes without positions %.1f ms   segments: sizing %.1f ms, fill %.1f ms (%d segments)"
              % (label, "warm-up" if rnd < 0 else "round %d" % rnd, q, a, a0, s, f, n_seg))
        if rnd >= 0:
            for name, v in (("query", q), ("nodes", a), ("nodes_no_pos", a0), ("sizing", s), ("fill", f)):
                res[name].append(v)
    found = int((out[:nb] > 0).sum()); valid = int((out[:nb] >= 0).sum())
    v = node[:nb]
    mapped = int(((v >= 0) | (v < -3)).sum()); removed = int((v == -1).sum()); absent = int((v == -2).sum()); no_kmer = int((v == -3).sum())      # (the sentinels as signed 64-bit values)
    assert mapped + removed == found and mapped + removed + absent == valid and no_kmer == nb - valid
    assert int(support[:nu].sum()) == mapped
    print("%s: %d unitigs; %d positions mapped, %d removed, %d absent, %d without a k-mer; %d segments (%.1f k-mers per segment, %.2f segments per read)"
          % (label, nu, mapped, removed, absent, no_kmer, n_seg, mapped / max(n_seg, 1), n_seg / n))
    line(label + ": (a) gkc_query_reads_device", res["query"])
    line(label + ": gkc_graph_reads_nodes_device", res["nodes"])
    line(label + ": gkc_graph_reads_nodes_device, d_pos == NULL", res["nodes_no_pos"])
    line(label + ": gkc_graph_reads_segments_device, sizing call", res["sizing"])
    line(label + ": gkc_graph_reads_segments_device, fill", res["fill"])
    qm, am = float(np.median(res["query"])), float(np.median(res["nodes"]))
    print("%s: nodes / query = %.2f; %.2f ns per position; condition median nodes %.1f ms <= 1.5 x median query %.1f ms: %s" % (label, am / qm, am * 1e6 / nb, am, qm, "met" if am <= 1.5 * qm else "MISSED"))
    return qm, am


nu, _, _ = c.unitigs_build()
measure("(b) plain placement", nu)
w, got = wall(lambda: c.simplify())
print("simplify: %.1f ms, %d rounds, %d records removed, %d unitigs left" % (w, got["rounds"], got["records_removed"], got["n_unitigs"]))
measure("(c) simplified placement", got["n_unitigs"])
for name in ("query_index", "query_reads", "graph_read_nodes", "graph_read_segments"):
    ms, launches = c.timing(name)
    print("gkc_get_timing %-20s %10.1f ms over %d intervals" % (name, ms, launches))
c.device_free(db); c.device_free(do)
c.close()
