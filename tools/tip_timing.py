"""Developer probe: what the tip removal costs on the device (not part of the product). Same input as tools/unitig_timing.py. In one process, after a warm-up, every
round computes the masks, runs a plain gkc_graph_unitigs_build / _write / _links on them (for comparison: "graph_links", "graph_rank", "graph_emit",
"graph_unitig_links"), then gkc_graph_tips_remove with the default parameters, and reads the gkc_get_timing split: "graph_tips" (flags, kill and refresh of every round
of the call; its launch count: the rounds) and what the builds and links inside the call added to the other names. Prints per round and the median / min / max.
Condition checked at the end: median graph_tips PER ROUND OF THE CALL <= 2 x median graph_unitig_links of the plain build.
usage: tip_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]"""
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
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
L, m = 150, 10
os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
db, do = c.synth_reads_device(2, n, L, n * 5, 10000)
c.begin_pass(0); c.push_reads_device(db, do, n, n * L); c.finish_pass()
c.device_free(db); c.device_free(do)
ns = c.stats()["kmers_nb_solid"]
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d solid k-mers" % (n, L, k, m, parts, ns))

masks = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda"); alive = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
c.neighbor_masks(d_out=masks.data_ptr())                           # builds the index
nu, nb, nc = c.unitigs_build(d_masks=masks.data_ptr())
nl = ctypes.c_uint64()
c._chk(c.L.gkc_graph_unitigs_links(c.h, masks.data_ptr(), None, 0, None, 0, ctypes.byref(nl)))
nl = nl.value
bases = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
offsets = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); kc = torch.zeros(nu + 1, dtype=torch.int64, device="cuda")
link_offsets = torch.zeros(2 * nu + 1, dtype=torch.int64, device="cuda"); links = torch.zeros(nl + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
print("before: %d unitigs, %d bases (%.1f records per unitig), %d links" % (nu, nb, ns / max(nu, 1), nl))
prm = gkc.TipParams((5 * k) // 2, 10 * k, 2, 1, 20)
prm_one = gkc.TipParams((5 * k) // 2, 10 * k, 2, 1, 1)             # the first round alone: the one with the most tips
per_round = np.zeros(64, np.uint64)

NAMES = ("graph_links", "graph_rank", "graph_emit", "graph_unitig_links", "graph_tips")


def split():
    return {name: c.timing(name) for name in NAMES}


def delta(a, b):
    return {name: b[name][0] - a[name][0] for name in NAMES}


res = {("plain", name): [] for name in NAMES}
res.update({("call", name): [] for name in NAMES})
res["tips_per_round"] = []; res["wall_call"] = []; res["first_round"] = []
for rnd in range(-1, rounds):
    c.neighbor_masks(d_out=masks.data_ptr())
    t0 = split()
    assert c.unitigs_build(d_masks=masks.data_ptr()) == (nu, nb, nc)
    c._chk(c.L.gkc_graph_unitigs_write(c.h, bases.data_ptr(), nb, offsets.data_ptr(), nu, kc.data_ptr()))
    got = ctypes.c_uint64()
    c._chk(c.L.gkc_graph_unitigs_links(c.h, masks.data_ptr(), link_offsets.data_ptr(), nu, links.data_ptr(), nl, ctypes.byref(got)))
    t1 = split()
    out = [ctypes.c_uint64() for _ in range(6)]
    w0 = time.perf_counter()
    c._chk(c.L.gkc_graph_tips_remove(c.h, masks.data_ptr(), alive.data_ptr(), ctypes.byref(prm), ctypes.byref(out[0]), per_round.ctypes.data_as(ctypes.c_void_p),
                                     *[ctypes.byref(x) for x in out[1:5]]))
    w1 = time.perf_counter()
    t2 = split()
    n_rounds, removed, nu2, nb2, nc2 = (x.value for x in out[:5])
    assert t2["graph_tips"][1] - t1["graph_tips"][1] == n_rounds - (1 if nu2 == 0 else 0)
    plain, call = delta(t0, t1), delta(t1, t2)
    tips = [int(x) for x in per_round[:n_rounds]]
    print("%s: plain build: links %.1f  rank %.1f  emit %.1f  unitig links %.1f ms | tips call: %d rounds, graph_tips %.1f ms (%.2f per round), inside it links %.1f  rank %.1f  "
          "unitig links %.1f ms, wall %.1f ms; tips per round %s; %d records removed; after: %d unitigs, %d bases"
          % ("warm-up" if rnd < 0 else "round %d" % rnd, plain["graph_links"], plain["graph_rank"], plain["graph_emit"], plain["graph_unitig_links"], n_rounds, call["graph_tips"],
             call["graph_tips"] / max(n_rounds, 1), call["graph_links"], call["graph_rank"], call["graph_unitig_links"], (w1 - w0) * 1e3, tips, removed, nu2, nb2))
    c.neighbor_masks(d_out=masks.data_ptr())
    one = [ctypes.c_uint64() for _ in range(5)]
    c._chk(c.L.gkc_graph_tips_remove(c.h, masks.data_ptr(), alive.data_ptr(), ctypes.byref(prm_one), ctypes.byref(one[0]), None, *[ctypes.byref(x) for x in one[1:]]))
    t3 = split()
    first = delta(t2, t3)["graph_tips"]
    print("         the first round alone (max_rounds = 1): graph_tips %.1f ms, %d records removed" % (first, one[1].value))
    if rnd >= 0:
        res["first_round"].append(first)
        for name in NAMES:
            res[("plain", name)].append(plain[name]); res[("call", name)].append(call[name] / max(n_rounds, 1))
        res["wall_call"].append((w1 - w0) * 1e3); res["tips_per_round"].append(tips)


def line(label, v):
    v = np.array(v)
    print("%-44s median %8.2f ms   min %8.2f   max %8.2f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))


for name in NAMES[:4]:
    line("plain build: " + name, res[("plain", name)])
for name in NAMES:
    line("tips call, per round of the call: " + name, res[("call", name)])
line("tips call, wall", res["wall_call"])
line("graph_tips of the first round alone", res["first_round"])
assert all(t == res["tips_per_round"][0] for t in res["tips_per_round"])
a, b = float(np.median(res[("call", "graph_tips")])), float(np.median(res[("plain", "graph_unitig_links")]))
print("condition: graph_tips per round %.2f ms <= 2 x graph_unitig_links %.2f ms: %s" % (a, b, "met" if a <= 2 * b else "MISSED"))
a = float(np.median(res["first_round"]))
print("the same for the first round alone: %.2f ms <= 2 x %.2f ms: %s" % (a, b, "met" if a <= 2 * b else "MISSED"))
c.close()
