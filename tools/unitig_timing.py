"""Developer probe: what the unitigs of the solid k-mers cost on the device (not part of the product). Same input as tools/graph_timing.py. In one process, after a
warm-up round, every round runs gkc_graph_neighbors_solid (the masks, for comparison), gkc_graph_unitigs_build on those masks, gkc_graph_unitigs_write and
gkc_graph_unitigs_links, and reads the gkc_get_timing split of the round: "graph_links" (one kernel), "graph_rank" (pointer jumping, placement, numbering; its launch
count is the number of rounds of pointer jumping), "graph_emit" and "graph_unitig_links" (the edges between the unitigs: count, scan, fill). Prints per round and the
median / min / max over the rounds.
usage: unitig_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]"""
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
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d solid k-mers, %d states" % (n, L, k, m, parts, ns, 2 * ns))

masks = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
c.neighbor_masks(d_out=masks.data_ptr())                           # builds the index
nu, nb, nc = c.unitigs_build(d_masks=masks.data_ptr())
bases = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
offsets = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); kc = torch.zeros(nu + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
print("%d unitigs, %d bases (%.1f records per unitig), %d cycles" % (nu, nb, ns / max(nu, 1), nc))
import ctypes
nl = ctypes.c_uint64()
c._chk(c.L.gkc_graph_unitigs_links(c.h, masks.data_ptr(), None, 0, None, 0, ctypes.byref(nl)))
nl = nl.value
link_offsets = torch.zeros(2 * nu + 1, dtype=torch.int64, device="cuda"); links = torch.zeros(nl + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
print("%d links over %d sides (%.2f per side)" % (nl, 2 * nu, nl / max(2 * nu, 1)))

NAMES = ("graph_neighbors", "graph_links", "graph_rank", "graph_emit", "graph_unitig_links")


def split():
    return {name: c.timing(name) for name in NAMES}


res = {name: [] for name in NAMES}
res["wall_build"] = []; res["wall_write"] = []; res["wall_links"] = []
n_rounds = []
for rnd in range(-1, rounds):
    t0 = split()
    c.neighbor_masks(d_out=masks.data_ptr())
    w0 = time.perf_counter()
    assert c.unitigs_build(d_masks=masks.data_ptr()) == (nu, nb, nc)
    w1 = time.perf_counter()
    c._chk(c.L.gkc_graph_unitigs_write(c.h, bases.data_ptr(), nb, offsets.data_ptr(), nu, kc.data_ptr()))
    w2 = time.perf_counter()
    got = ctypes.c_uint64()
    c._chk(c.L.gkc_graph_unitigs_links(c.h, masks.data_ptr(), link_offsets.data_ptr(), nu, links.data_ptr(), nl, ctypes.byref(got)))
    w3 = time.perf_counter()
    assert got.value == nl
    t1 = split()
    ms = {name: t1[name][0] - t0[name][0] for name in NAMES}
    jumps = t1["graph_rank"][1] - t0["graph_rank"][1]
    print("%s: neighbors %.1f ms   links %.1f ms   rank %.1f ms in %d rounds   emit %.1f ms   unitig links %.1f ms   (wall: build %.1f ms, write %.1f ms, unitig links %.1f ms)"
          % ("warm-up" if rnd < 0 else "round %d" % rnd, ms["graph_neighbors"], ms["graph_links"], ms["graph_rank"], jumps, ms["graph_emit"], ms["graph_unitig_links"],
             (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3))
    if rnd >= 0:
        for name in NAMES:
            res[name].append(ms[name])
        res["wall_build"].append((w1 - w0) * 1e3); res["wall_write"].append((w2 - w1) * 1e3); res["wall_links"].append((w3 - w2) * 1e3); n_rounds.append(jumps)
assert int(offsets[-1]) == nb and int(kc[:nu].sum()) > 0 and int(link_offsets[-1]) == nl
for name, label in (("graph_neighbors", "gkc_graph_neighbors_solid"), ("graph_links", "links"), ("graph_rank", "rank"), ("graph_emit", "emit"), ("graph_unitig_links", "unitig links"),
                    ("wall_build", "build, wall"), ("wall_write", "write, wall"), ("wall_links", "unitig links, wall")):
    v = np.array(res[name])
    print("%-28s median %.1f ms   min %.1f   max %.1f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))
print("rounds of pointer jumping: %s; %.2f ns per state and round; scratch 84 bytes per record, of them 2 x 16 per state in the ranking" % (sorted(set(n_rounds)), np.median(res["graph_rank"]) * 1e6 / (2 * ns * max(n_rounds[0], 1))))
c.close()
