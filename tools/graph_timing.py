"""Developer probe: what the exact neighbourhoods of the solid k-mers cost on the device (not part of the product). Same input as tools/query_timing.py. In one process,
after a warm-up round, every round runs
  (a) the composed path       : the eight neighbour keys of every solid record built on the device (torch), gkc_query_kmers_device over them, (answer > 0) folded to
                                one byte per record — what a user of the abundance queries had to do before gkc_graph_* existed, and the yardstick;
  (b) gkc_graph_neighbors_solid : the same bytes from one kernel;
  (c) gkc_graph_branching_solid : topology table + branching records from the masks of (b);
  (d) gkc_bloom_query_solid(contains8) on the same set, for information: the filter's answer, false positives included (neighbor kind, 11 bits per k-mer, 7 hashes).
Every timed span is wall time and ends in a stream synchronise; the index is built before the first span. (a) and (b) are compared byte for byte in every round. Prints per
round and the median / min / max over the rounds, then the gkc_get_timing split.
usage: graph_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5]"""
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
if k > 31:
    sys.exit("the composed path of this probe builds 8-byte keys: k <= 31")
L, m = 150, 10
os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
db, do = c.synth_reads_device(2, n, L, n * 5, 10000)
c.begin_pass(0); c.push_reads_device(db, do, n, n * L); c.finish_pass()
c.device_free(db); c.device_free(do)
ns = c.stats()["kmers_nb_solid"]
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d solid k-mers, %d lookups per round" % (n, L, k, m, parts, ns, 8 * ns))

# the values of the solid records, dataset order, as a torch tensor (through the host, outside the timed spans)
vals = torch.empty(ns, dtype=torch.int64, device="cuda")
at = 0
for p in range(parts):
    lo, _, _ = c.partition(0, p)
    vals[at: at + len(lo)] = torch.from_numpy(lo.view(np.int64)).cuda(); at += len(lo)
assert at == ns
torch.cuda.synchronize()
j4 = torch.arange(4, dtype=torch.int64, device="cuda")[None, :]
w8 = (1 << torch.arange(8, dtype=torch.int32, device="cuda"))[None, :]
KMASK, M62 = (1 << (2 * k)) - 1, (1 << 62) - 1
keys = torch.empty((ns, 8), dtype=torch.int64, device="cuda")
ans = torch.empty(8 * ns + 4, dtype=torch.int32, device="cuda")
composed = torch.empty(ns, dtype=torch.uint8, device="cuda")
fused = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def path_a():
    x = vals[:, None]
    keys[:, :4] = ((x << 2) | j4) & KMASK
    keys[:, 4:] = ((x >> 2) & M62) | (j4 << (2 * (k - 1)))
    torch.cuda.synchronize()
    c.query_kmers_device(keys.data_ptr(), 8 * ns, 8, ans.data_ptr())
    composed.copy_(((ans[: 8 * ns].view(ns, 8) > 0).to(torch.int32) * w8).sum(1))
    torch.cuda.synchronize()


def path_a_parts():
    """(a) again, its three pieces timed one by one -> (keys, query, fold) ms"""
    def keys_():
        x = vals[:, None]
        keys[:, :4] = ((x << 2) | j4) & KMASK
        keys[:, 4:] = ((x >> 2) & M62) | (j4 << (2 * (k - 1)))
        torch.cuda.synchronize()

    def fold_():
        composed.copy_(((ans[: 8 * ns].view(ns, 8) > 0).to(torch.int32) * w8).sum(1))
        torch.cuda.synchronize()
    return wall(keys_), wall(lambda: c.query_kmers_device(keys.data_ptr(), 8 * ns, 8, ans.data_ptr())), wall(fold_)


def path_b():
    assert c.neighbor_masks(d_out=fused.data_ptr()) == ns


c.neighbor_masks(d_out=fused.data_ptr())                          # builds the index
nbr = gkc.C.c_uint64()
c._chk(c.L.gkc_graph_branching_solid(c.h, fused.data_ptr(), None, 0, gkc.C.byref(nbr), None))
n_br = nbr.value
recs = torch.empty(max(1, n_br) * c.rec_bytes, dtype=torch.uint8, device="cuda")
topo = np.zeros(25, np.uint64)
torch.cuda.synchronize()


def path_c():
    c._chk(c.L.gkc_graph_branching_solid(c.h, fused.data_ptr(), recs.data_ptr(), n_br, gkc.C.byref(nbr), topo.ctypes.data_as(gkc.C.c_void_p)))


bloom = gkc.Bloom(c, "neighbor", 11 * ns, 7, k)
bloom.insert_solid()
d8 = torch.zeros(ns + 16, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
bloom_bits = [0]


def path_d():
    bloom_bits[0] = bloom.query_solid(True, d8.data_ptr())[1]


res = {"a": [], "b": [], "c": [], "d": [], "a_keys": [], "a_query": [], "a_fold": []}
for rnd in range(-1, rounds):
    a = wall(path_a); b = wall(path_b); cc = wall(path_c); d = wall(path_d)
    ak, aq, af = path_a_parts()
    same = bool(torch.equal(composed, fused[:ns]))
    print("%s: (a) composed %.1f ms (keys %.1f + query %.1f + fold %.1f)   (b) graph_neighbors %.1f ms   (c) graph_branching %.1f ms   (d) bloom contains8 %.1f ms   (a) == (b): %s"
          % ("warm-up" if rnd < 0 else "round %d" % rnd, a, ak, aq, af, b, cc, d, same))
    assert same
    if rnd >= 0:
        for name, v in (("a", a), ("b", b), ("c", cc), ("d", d), ("a_keys", ak), ("a_query", aq), ("a_fold", af)):
            res[name].append(v)
exact_bits = int(torch.sum(torch.bitwise_and(fused[:ns, None].to(torch.int32) >> torch.arange(8, dtype=torch.int32, device="cuda")[None, :], 1)))
t = topo.reshape(5, 5)
print("answers: %d neighbour bits set of %d (%.3f per k-mer); the Bloom filter sets %d (%d false positives); %d branching nodes (%.2f %%); topology[1][1] = %d"
      % (exact_bits, 8 * ns, exact_bits / ns, bloom_bits[0], bloom_bits[0] - exact_bits, n_br, 100.0 * n_br / ns, int(t[1, 1])))
assert int(t.sum()) == ns and int(t.sum() - t[1, 1]) == n_br
for name, label in (("a", "(a) composed path"), ("a_keys", "    keys (torch)"), ("a_query", "    query_kmers_device"), ("a_fold", "    fold (torch)"), ("b", "(b) graph_neighbors_solid"),
                    ("c", "(c) graph_branching_solid"), ("d", "(d) bloom contains8")):
    v = np.array(res[name])
    print("%-28s median %.1f ms   min %.1f   max %.1f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))
mb, ma = np.median(res["b"]), np.median(res["a"])
print("(b) / (a) = %.2f   (b) <= (a): %s   %.3f ns per lookup at (b), %.3f at the query of (a)" % (mb / ma, mb <= ma, mb * 1e6 / (8 * ns), np.median(res["a_query"]) * 1e6 / (8 * ns)))
for name in ("query_index", "query_kmers", "graph_neighbors", "graph_branching", "bloom_contains8"):
    ms, launches = c.timing(name)
    print("gkc_get_timing %-16s %10.1f ms over %d intervals" % (name, ms, launches))
bloom.close()
c.close()
