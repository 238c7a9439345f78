"""Developer probe: what multi-bank counting costs on the device (not part of the product). N banks of synthetic reads over one genome are counted one
after another; prints, per bank, the bank's own Stage B next to the gkc_banks_add that merges it, then gkc_banks_evaluate per solidity kind and the HBM
bytes of the merged state. The sequence runs twice: the second round finds its buffers in the context's allocator.
usage: banks_timing.py [reads per bank = 10^7] [banks = 4] [partitions = 512] [k = 31]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as ge
import bench

gkc = ge.load().gkc
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 4
parts = int(sys.argv[3]) if len(sys.argv) > 3 else 512
k = int(sys.argv[4]) if len(sys.argv) > 4 else 31
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 2
L, m = 150, 10
c = gkc.Counter(0)
c.configure(k, m, parts, bench.repart_for_bench(m, parts))
# one genome (the seed), disjoint slices of one read stream: the banks share most error-free k-mers and none of the erroneous ones
reads = [c.synth_reads_device(2, n, L, n * 5, 10000, first_read=i * n) for i in range(nb)]
print("banks %d x %d reads of %d bp, k=%d, m=%d, %d partitions" % (nb, n, L, k, m, parts))


def delta(name, before):
    return c.timing(name)[0] - before


for rnd in range(rounds):
    B = gkc.Banks(c, nb)
    for i, (db, do) in enumerate(reads):
        a0, b0, m0 = c.timing("total_stage_a")[0], c.timing("total_stage_b")[0], c.timing("banks_add")[0]
        c.begin_pass(0); c.push_reads_device(db, do, n, n * L); c.finish_pass()
        t0 = time.perf_counter(); B.add(i); wall = (time.perf_counter() - t0) * 1e3
        st = c.stats()
        print("round %d bank %d: stage_a %.1f ms  total_stage_b %.1f ms  banks_add %.1f ms (wall %.1f ms)  distinct k-mers of the bank %d"
              % (rnd, i, delta("total_stage_a", a0), delta("total_stage_b", b0), delta("banks_add", m0), wall, st["kmers_nb_distinct"]))
    for kind, lo, hi in (("sum", 1, 2 ** 31 - 1), ("sum", 3, 2 ** 31 - 1), ("min", 1, 2 ** 31 - 1), ("one", 3, 2 ** 31 - 1), ("all", 2, 2 ** 31 - 1)):
        e0 = c.timing("banks_evaluate")[0]
        B.evaluate(kind, lo, hi, None, 10000)
        info = [B.partition_info(d) for d in range(parts)]
        solid, distinct = sum(x[0] for x in info), sum(x[1] for x in info)
        assert int(B.histogram().sum()) == distinct
        print("round %d evaluate %-3s [%d, %s]: %.1f ms  solid %d of %d distinct" % (rnd, kind, lo, "inf" if hi == 2 ** 31 - 1 else hi, delta("banks_evaluate", e0), solid, distinct))
    rb = 16 if k <= 31 else 32
    print("round %d merged state: %d distinct k-mers x (%d B key + %d planes x 4 B) = %.2f GB of HBM; last evaluation's output %.2f GB"
          % (rnd, distinct, rb // 2, nb, distinct * (rb // 2 + 4 * nb) / 1e9, solid * (rb + 4 * nb) / 1e9))
    B.close()
for db, do in reads:
    c.device_free(db); c.device_free(do)
c.close()
