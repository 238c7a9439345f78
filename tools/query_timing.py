"""Developer probe: what an abundance query costs on the device next to counting the same reads (not part of the product). In one process, after a warm-up
round, every round runs
  (a) count()            : gkc_begin_pass + gkc_push_reads_device + gkc_finish_pass of the reads — the yardstick: without queries, the abundances of a second
                           look at the reads cost at least a recount (plus a 16-byte-per-record transfer);
  (b) query_reads_device : the same reads against those results at the default index stride;
  (c) the same with the index disabled (GKC_QUERY_INDEX_STRIDE beyond any dataset: one sample per dataset, a plain binary search over the records).
Every timed span is wall time around a call that ends in a stream synchronise; the index is (re)built before each timed query by a one-read query and reported
on its own. Prints per round and the median / min / max over the rounds, then the gkc_get_timing split.
usage: query_timing.py [reads = 10^7] [partitions = 512] [k = 31] [rounds = 5] [stride of (b) = the library's default]"""
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
stride_b = sys.argv[5] if len(sys.argv) > 5 else None
L, m = 150, 10
NO_INDEX = str(1 << 40)
os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
db, do = c.synth_reads_device(2, n, L, n * 5, 10000)
nb = n * L
out = torch.empty(nb + 16, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
print("%d reads of %d bp, k=%d, m=%d, %d partitions: %d positions per query" % (n, L, k, m, parts, nb))


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def count():
    c.begin_pass(0); c.push_reads_device(db, do, n, nb); c.finish_pass()


def query():
    c.query_reads_device(db, do, n, nb, out.data_ptr())


def build_index(stride):
    """one-read query: (re)builds the index at `stride` outside the timed spans -> ms of the library's query_index timer"""
    if stride is None:
        os.environ.pop("GKC_QUERY_INDEX_STRIDE", None)
    else:
        os.environ["GKC_QUERY_INDEX_STRIDE"] = stride
    t0 = c.timing("query_index")[0]
    c.query_reads_device(db, do, 1, L, out.data_ptr())
    return c.timing("query_index")[0] - t0


res = {"a": [], "b": [], "c": [], "index": []}
answers = None
for rnd in range(-1, rounds):
    a = wall(count)
    ix = build_index(stride_b)
    b = wall(query)
    got_b = (int((out[:nb] > 0).sum()), int((out[:nb] == 0).sum()), int((out[:nb] < 0).sum()))
    build_index(NO_INDEX)
    cc = wall(query)
    got_c = (int((out[:nb] > 0).sum()), int((out[:nb] == 0).sum()), int((out[:nb] < 0).sum()))
    assert got_b == got_c, (got_b, got_c)
    answers = got_b
    print("%s: (a) count %.1f ms   index build %.1f ms   (b) query %.1f ms   (c) query without index %.1f ms" % ("warm-up" if rnd < 0 else "round %d" % rnd, a, ix, b, cc))
    if rnd >= 0:
        res["a"].append(a); res["b"].append(b); res["c"].append(cc); res["index"].append(ix)
print("answers: %d found, %d valid k-mers not in the results, %d positions without a k-mer" % answers)
st = c.stats()
S = int(stride_b or 256)
print("results: %d solid k-mers in %d datasets (%.2f GB of Count records); index at stride %d: %.1f MB"
      % (st["kmers_nb_solid"], parts, st["kmers_nb_solid"] * c.rec_bytes / 1e9, S, (st["kmers_nb_solid"] / S + parts) * (c.rec_bytes // 2) / 1e6))
for name, label in (("a", "(a) count"), ("index", "    index build"), ("b", "(b) query, stride %d" % S), ("c", "(c) query, no index")):
    v = np.array(res[name])
    print("%-24s median %.1f ms   min %.1f   max %.1f   (%d rounds)" % (label, np.median(v), v.min(), v.max(), len(v)))
print("(b) / (a) = %.2f   (c) / (b) = %.2f   %.2f ns per queried position at (b)" % (np.median(res["b"]) / np.median(res["a"]), np.median(res["c"]) / np.median(res["b"]),
                                                                                  np.median(res["b"]) * 1e6 / nb))
for name in ("total_stage_a", "total_stage_b", "query_index", "query_reads", "query_kmers"):
    ms, launches = c.timing(name)
    print("gkc_get_timing %-14s %10.1f ms over %d intervals" % (name, ms, launches))
c.device_free(db); c.device_free(do)
c.close()
