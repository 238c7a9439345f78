"""Developer probe: what the simplification of the compacted graph costs on the device (not part of the product). Same input as tools/tip_timing.py. In one process, after
a warm-up, every call computes the masks again and runs gkc_graph_simplify with the default parameters, then reads the gkc_get_timing split: "graph_bulges" and "graph_ec"
(KC when the round is the first on its graph, flags, mark, kill and refresh of that kind's rounds; launch count: the rounds) and, beside them, "graph_tips" of the tip
rounds of the same call: the same kernels around another flag kernel, on the same graph, in the same process. Prints per call and the median / min / max.
Condition checked at the end: a median bulge round and a median EC round each cost at most 2 x the median tip round.
usage: simplify_timing.py [reads = 10^7] [partitions = 512] [k = 31] [calls = 5] [max_sweeps = 10]"""
import ctypes
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
calls = int(sys.argv[4]) if len(sys.argv) > 4 else 5
max_sweeps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
L, m = 150, 10
os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
db, do = c.synth_reads_device(2, n, L, n * 5, 10000)
c.begin_pass(0); c.push_reads_device(db, do, n, n * L); c.finish_pass()
c.device_free(db); c.device_free(do)
ns = c.stats()["kmers_nb_solid"]
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d solid k-mers" % (n, L, k, m, parts, ns), flush=True)

masks = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda"); alive = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
prm = c.simplify_params(max_sweeps=max_sweeps)
log = (gkc.SimplifyRound * gkc.SIMPLIFY_LOG_CAP)()
NAMES = ("graph_tips", "graph_bulges", "graph_ec", "graph_links", "graph_rank", "graph_unitig_links")
KIND_NAME = dict(tips="graph_tips", bulges="graph_bulges", ec="graph_ec")


def split():
    return {name: c.timing(name) for name in NAMES}


res = {name: [] for name in NAMES}
res["wall"] = []; res["logs"] = []
for call in range(-1, calls):
    c.neighbor_masks(d_out=masks.data_ptr())
    out = [ctypes.c_uint64() for _ in range(5)]
    t0 = split()
    w0 = time.perf_counter()
    c._chk(c.L.gkc_graph_simplify(c.h, masks.data_ptr(), alive.data_ptr(), ctypes.byref(prm), log, gkc.SIMPLIFY_LOG_CAP, *[ctypes.byref(x) for x in out]))
    w1 = time.perf_counter()
    t1 = split()
    n_rounds, removed, nu, nb, nc = (x.value for x in out)
    entries = [(gkc.SIMPLIFY_KINDS[e.kind], e.sweep, e.n_unitigs, e.n_hits, e.n_records_removed) for e in log[:n_rounds]]
    per_round = {}
    for kind, name in KIND_NAME.items():
        rounds = t1[name][1] - t0[name][1]
        assert rounds == sum(1 for e in entries if e[0] == kind and e[2])
        per_round[name] = (t1[name][0] - t0[name][0]) / rounds if rounds else float("nan")
    builds = t1["graph_links"][1] - t0["graph_links"][1]
    assert builds == sum(1 for e in entries if e[3]) + 1
    label = "warm-up" if call < 0 else "call %d" % call
    print("%s: %d rounds, %d builds (%d rounds removed nothing and built nothing), wall %.1f ms; per round: graph_tips %.2f  graph_bulges %.2f  graph_ec %.2f ms; inside the call "
          "links %.1f  rank %.1f  unitig links %.1f ms; %d records removed; after: %d unitigs, %d bases"
          % (label, n_rounds, builds, n_rounds - (builds - 1), (w1 - w0) * 1e3, per_round["graph_tips"], per_round["graph_bulges"], per_round["graph_ec"],
             t1["graph_links"][0] - t0["graph_links"][0], t1["graph_rank"][0] - t0["graph_rank"][0], t1["graph_unitig_links"][0] - t0["graph_unitig_links"][0], removed, nu, nb), flush=True)
    if call < 0:
        phase = None
        for kind, sweep, n_unitigs, hits, gone in entries:      # hits per round and kind, once: every call gives the same
            if (kind, sweep) != phase:
                phase = (kind, sweep)
                print("\n  sweep %d %-6s:" % (sweep, kind), end="")
            print(" %d" % hits, end="")
        print(flush=True)
    else:
        for name in KIND_NAME.values():
            res[name].append(per_round[name])
        res["wall"].append((w1 - w0) * 1e3); res["logs"].append(entries)


def line(label, v):
    v = np.array(v)
    print("%-44s median %8.2f ms   min %8.2f   max %8.2f   (%d calls)" % (label, np.median(v), v.min(), v.max(), len(v)))


line("simplify call, wall", res["wall"])
for name in KIND_NAME.values():
    line("per round of the call: " + name, res[name])
assert all(e == res["logs"][0] for e in res["logs"])
tips = float(np.median(res["graph_tips"]))
for name in ("graph_bulges", "graph_ec"):
    a = float(np.median(res[name]))
    print("condition: %s per round %.2f ms <= 2 x graph_tips per round %.2f ms: %s" % (name, a, tips, "met" if a <= 2 * tips else "MISSED"))
c.close()
