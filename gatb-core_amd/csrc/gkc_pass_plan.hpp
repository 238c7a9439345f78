// gkc_pass_plan.hpp — the memory plan of one Stage-B pass: how many lanes, how many keys per batch, which partitions form the next batch.
// Pure host arithmetic (no HIP, no context): gkc_count_pass builds one PassPlan per pass and its lanes carve their batches from it; tests/pass_plan_driver.cpp
// exercises it on its own.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <math.h>
#include <algorithm>
#include <functional>
#include <mutex>
#include <vector>

// what a plan is computed from: the pass (keys per partition, memory), the context's settings, the tunables snapshot of the pass
struct PassPlanInputs {
    double avail_bytes = 0;          // free device memory + blocks parked in the caching allocator
    double reserve_bytes = 0;        // overlapped passes: what Stage A of the next pass will allocate beside this Stage B
    uint32_t key_words = 1;          // 1: 8-byte keys, 16-byte records; 2: 16-byte keys, 32-byte records
    uint32_t nb_passes = 1;
    bool sink = false;               // streamed results (gkc_set_host_sink)
    size_t key_budget = 0;           // max keys per batch, forced (tests); 0 = planned
    size_t batch_cap = 0;            // gkc_set_batch_keys: upper bound of the planned batch size; 0 = the library's own
    double d_hint = 0;               // solid records per key of the last pass of the context; 0 = none yet
    size_t last_plan_budget = 0;     // batch budget the last pass of the context planned; 0 = none yet
    int lanes = 2; uint64_t batch_keys = 0; uint32_t sink_first_div = 4; bool pool_debug = false;      // tunables: GKC_STAGEB_LANES, GKC_BATCH_KEYS, GKC_SINK_FIRST_DIV, GKC_POOL_DEBUG
    uint32_t max_sub_bits = 13, part_align = 256;                                                       // MAX_SUB_BITS, PART_ALIGN of the batch layout
};

// Batches of consecutive partitions, each bounded by a key budget that stays the SAME through the pass: equal batches ask the caching
// allocator for the same block sizes again and again, so after the first batches no hipMalloc / hipFree happens at all (hipMalloc
// costs ~22 ms per GB here; re-deriving the budget from the shrinking free memory made every batch a new size and a k=63 pass, where
// the results take half the HBM, spent seconds in the allocator). Per key slot a batch needs the key twice (a split level uses
// the ping-pong buffer) and 5 B of abundance planes — its working set, returned to the pool afterwards — and leaves one Count
// record per SOLID distinct key resident, so the peak is at the END of the pass: all results + the last working sets.
//  * the budget is what the working sets may take beside the results the whole pass will leave:
//    (0.95 free - keys * rec * 1.05 d) / (lanes * work), d = solid records per key; capped, and cut into equal shares;
//  * d comes from a small probe batch the first time the memory may bind (see probe_wanted) and is kept by the context;
//  * safety net: before every batch the commitments (finished results, the other lanes' running batches) are checked, and if the
//    batch does not fit the extra lanes retire and the main lane halves its batches (slow: blocks change size; never seen when
//    the plan holds).
// Two LANES: Stage B's kernels are bound by different things (expand: store atoms and LDS, sorts: VALU, compaction: HBM), and a single
// in-order stream leaves most of the chip waiting on whichever bound the current kernel has. Two host threads therefore take batches
// from one queue, each on its own stream (thread-local stream override, cur_stream()): measured 264 -> 229 ms for the same work.
struct PassPlan {
    const std::vector<uint64_t>& part_keys;
    const PassPlanInputs in;
    // the two effects planning has on the context: give the parked blocks back (they have the wrong sizes), publish an empty partition as a finished dataset
    const std::function<void()> trim;
    const std::function<void(uint32_t)> mark_empty;
    const size_t key_bytes, rec_bytes, work_per_key;
    uint64_t total_keys = 0, max_part = 0;
    double avail0 = 0, avail_q = 0;              // memory this pass may use; the same rounded down to GB
    size_t cap = 0, probe_keys = 0;
    int lanes = 1;                               // lanes that run (the caller lowers it when a lane's stream cannot be created, before the lanes start)
    int plan_lanes = 1;                          // lanes the budget is computed for: one lane gets the same batches as two would (same blocks whichever way a pass runs)
    double d_hint = 0; size_t last_plan_budget = 0;     // in: the context's; out: what it keeps for its next pass
    size_t fixed_budget = 0;
    // everything below is guarded by mu once the lanes run
    std::mutex mu;
    bool tight = false;                          // memory is running out: the extra lanes retire, one lane finishes the pass
    bool probe_pending = false;
    uint64_t done_keys = 0, done_solid = 0;      // this pass: finished batches (keys, resident records)
    double inflight[4] = { 0, 0, 0, 0 };         // bytes each lane's running batch may still claim (working set + its results)
    size_t last_b[4] = { 0, 0, 0, 0 };
    uint32_t lane_batches[4] = { 0, 0, 0, 0 }; uint64_t keys_left = 0;
    uint32_t next_p = 0; int first_rc = 0;
    uint64_t slots_hint_ = 0;

    PassPlan(const std::vector<uint64_t>& part_keys_, const PassPlanInputs& in_, std::function<void()> trim_, std::function<void(uint32_t)> mark_empty_)
        : part_keys(part_keys_), in(in_), trim(std::move(trim_)), mark_empty(std::move(mark_empty_)),
          key_bytes(in_.key_words == 1 ? 8 : 16), rec_bytes(in_.key_words == 1 ? 16 : 32), work_per_key(2 * key_bytes + 5), d_hint(in_.d_hint), last_plan_budget(in_.last_plan_budget)
    {
        for (uint64_t v : part_keys) { total_keys += v; max_part = std::max(max_part, v); }
        keys_left = total_keys;
        lanes = in.lanes;
        if (lanes < 1) lanes = 1;
        if (lanes > 4) lanes = 4;
        if (total_keys < 50000000ULL || in.key_budget) lanes = 1;               // small inputs (and the tests' tiny forced budgets): one lane
        avail0 = std::max(0.0, in.avail_bytes - in.reserve_bytes);
        const size_t cap_env = (size_t)in.batch_keys;
        // Few, large batches: every batch ends with the drain of ~12 kernels (the expand kernels run one 6 ms workgroup per partition) and
        // eight host round trips; 8 -> 4 batches per 1.2e10 keys: 320 -> 304 ms. Equal shares, a whole number of batches per lane.
        // With a host sink (streamed results) the batches are three times smaller: the first records start over PCIe sooner and the copy that is left
        // when the last batch has been counted is shorter (1e8 reads, abundance-min 2: 431 -> ms per step with everything landed; profiles/r02_*)
        const size_t cap_default = in.key_words == 1 ? (size_t)3200000000ULL : (size_t)1600000000ULL;
        const size_t cap_mode = in.sink ? cap_default / 3 : cap_default;       // (a host sink: three batches per lane keep the link busy)
        // gkc_set_batch_keys is an UPPER bound: never above the library's plan for the mode; GKC_BATCH_KEYS (developer switch) replaces the plan outright
        cap = cap_env ? cap_env : in.batch_cap ? std::min(cap_mode, std::max<size_t>(in.batch_cap, (size_t)1 << 24)) : cap_mode;   // the same with one lane or two
        // budget for a given solid-per-key ratio d. Deterministic in (free memory rounded to GB, total keys, d rounded up to 0.05): every
        // pass of a context plans the same sizes, so from the second pass on all blocks are parked already.
        avail_q = floor(avail0 / 1e9) * 1e9;
        plan_lanes = (in.key_budget || total_keys < 50000000ULL) ? 1 : std::max(2, lanes);                 // (more than two lanes: planned for what will really run)
        probe_keys = (size_t)std::max<uint64_t>(total_keys / 256, 16000000ULL);
        // d not known yet and the memory may bind: count a small PROBE batch first (the first partitions holding ~0.4 % of the keys) and take
        // its ratio. The context keeps that first estimate (until the configuration changes), so every later pass plans the same sizes.
        // In later passes the same small batch is simply the first one in the queue (it runs beside the other lane's first batch).
        probe_pending = !in.key_budget && plan_budget(1.0) < plan_budget(1e-9);
    }

    size_t plan_budget(double d) const {
        const double work = (double)plan_lanes * (double)work_per_key;
        const double dq = std::min(1.0, ceil(1.05 * d / 0.05) * 0.05);
        const double mem = (0.95 * avail_q - (double)total_keys * (double)rec_bytes * dq) / work;
        const uint64_t bmem = mem > (double)((size_t)1 << 20) ? (uint64_t)mem : ((uint64_t)1 << 20);
        if (in.nb_passes > 1) {
            // several passes: every pass plans the SAME batch size — half the cap plus a rounded partition — whatever its share of the k-mers (minimizer % nb_passes
            // does not cut them evenly: 5.2e9 and 6.8e9 keys for the two passes of 1e8 reads). Equal shares per pass gave every pass its own block sizes: the allocator was
            // trimmed and refilled at every pass, 4 s of hipMalloc for 0.15 s of counting (tools/twopass_probe.py).
            // (a small pass — the tests' — is one batch of its own size, rounded up to a power of two so that passes of similar size still plan alike)
            uint64_t mp = 1; while (mp < max_part) mp <<= 1;
            uint64_t tk = 1; while (tk < total_keys) tk <<= 1;
            return (size_t)(std::min<uint64_t>(std::min<uint64_t>(bmem, cap / 2), tk) + mp);
        }
        const uint64_t b = std::min<uint64_t>(bmem, cap);
        const uint64_t per_round = b * (uint64_t)plan_lanes;
        const uint64_t rounds = std::max<uint64_t>((total_keys + per_round - 1) / per_round, 1);
        const uint64_t share = total_keys / (rounds * (uint64_t)plan_lanes);
        return (size_t)std::min<uint64_t>(b + max_part, share + share / 64 + max_part);           // a little over the share: no small last batch
    }

    // the pass begins with a probe batch counted on its own (lane 0, before the lanes start): carve_probe, then probe_finished
    bool probe_wanted() const { return probe_pending && d_hint <= 0; }
    bool carve_probe(std::vector<uint32_t>& batch) { fixed_budget = probe_keys; slots_hint_ = 0; return carve(batch, 0); }
    void probe_finished(uint64_t keys, uint64_t solid) {
        inflight[0] = 0; last_b[0] = 0;
        done_keys += keys; done_solid += solid;
        if (done_keys) d_hint = std::max(1e-6, (double)done_solid / (double)done_keys);
    }
    // the budget of the pass, once d is known (or not needed); called once, before the lanes start
    void settle() {
        fixed_budget = d_hint > 0 ? plan_budget(d_hint) : plan_budget(1.0);   // without a ratio the memory does not bind even at d = 1
        if (in.pool_debug) fprintf(stderr, "[gkc plan] avail %.1f GB, keys %.3e, d_hint %.4f, lanes %d, budget %.3e\n", avail0 / 1e9, (double)total_keys, d_hint, lanes, (double)fixed_budget);
        // another batch size than the last pass planned (another input, a host sink set or dropped, another solidity ratio): the blocks parked in the allocator have the
        // wrong sizes — keeping them would make every new block a failed hipMalloc followed by frees, one parked block at a time (seen: 1.5 s for a 0.26 s pass)
        if (last_plan_budget && (fixed_budget > last_plan_budget + last_plan_budget / 10 || fixed_budget + fixed_budget / 10 < last_plan_budget)) trim();      // (the allocator reuses a block up to 25 % larger than asked)
        last_plan_budget = fixed_budget;
        if (!in.key_budget && fixed_budget < 250000000ULL) {                       // ... unless there is little room: one lane, larger batches
            lanes = 1; plan_lanes = 1; fixed_budget = d_hint > 0 ? plan_budget(d_hint) : plan_budget(1.0);
        }
        uint64_t nonempty = 0; for (uint64_t v : part_keys) nonempty += v != 0;
        const uint64_t avg_part = std::max<uint64_t>(total_keys / std::max<uint64_t>(nonempty, 1), 1);
        const uint64_t hint = (uint64_t)fixed_budget + ((uint64_t)fixed_budget / avg_part + 2) * ((3ull << in.max_sub_bits) + in.part_align);
        slots_hint_ = in.key_budget ? 0 : (hint + in.part_align - 1) / in.part_align * in.part_align;
    }
    // key slots the big working buffers of a batch are sized for (the pass's batch budget; 0: exact sizes)
    uint64_t slots_hint() { std::lock_guard<std::mutex> lk(mu); return slots_hint_; }

    double per_key_now() const {
        const double d_est = done_keys ? std::min(1.0, 1.05 * (double)done_solid / (double)done_keys) : (d_hint > 0 ? std::min(1.0, 1.05 * d_hint) : 1.0);
        return (double)work_per_key + (double)rec_bytes * d_est;
    }
    size_t budget_now(int lane) {                                            // keys of the next batch of one lane (called under mu)
        if (in.key_budget) return in.key_budget;
        double committed = 0; for (int l = 0; l < 4; l++) if (l != lane) committed += inflight[l];
        const double left = 0.98 * avail0 - (double)done_solid * (double)rec_bytes - committed;      // (the plan keeps 0.95: headroom between plan and net)
        const size_t fits = left > 0 ? (size_t)(left / per_key_now()) : 0;
        size_t b = fixed_budget;
        if (b > fits) {
            if (in.pool_debug) fprintf(stderr, "[gkc plan] lane %d: budget %.3e does not fit (%.3e): done_solid %.3e committed %.1f GB\n", lane, (double)b, (double)fits, (double)done_solid, committed / 1e9);
            if (lanes > 1) tight = true;                                     // first the extra lanes retire ...
            if (lane != 0) return b;
            while (b > fits && b > ((size_t)1 << 20)) b /= 2;                // ... then the main lane's batches shrink
            slots_hint_ = 0;                                                 // (exact buffer sizes from here on)
        }
        if (b != last_b[lane]) {                                             // another batch size: the parked blocks have the wrong sizes, and
            if (last_b[lane]) trim();                                        // reusing larger ones would keep exactly the memory that ran out
            last_b[lane] = b;
        }
        return b;
    }
    // next batch of consecutive partitions for one lane; false when nothing is left (or a batch has failed, or the lane retires)
    bool carve(std::vector<uint32_t>& batch, int lane) {
        std::lock_guard<std::mutex> lk(mu);
        const uint32_t Pn = (uint32_t)part_keys.size();
        batch.clear();
        if (first_rc != 0) return false;
        inflight[lane] = 0;
        size_t budget = budget_now(lane);
        if (tight && lane != 0) return false;
        if (probe_pending) { probe_pending = false; budget = probe_keys; }      // the pass's first batch is the small probe batch, every pass (same batches, same blocks)
        // streamed results: the link idles until the first batch has been counted and packed — the first batch of every lane is a quarter of the others (same
        // working buffers: they are sized for the budget), the copies start ~25 ms sooner
        // — and the last one as well: what is left when the last copy has landed is the expansion of the last batch on the host
        // Round 6: a RAMP instead of one small batch — 1/4, 1/2 of the budget, then whole ones. Stage B makes packed records ~2.6x faster than the link takes
        // them, so a batch twice the one before is ready before the link has drained; with one quarter batch per lane followed by whole ones (round 5) the link
        // sat idle between the end of the two small copies and the arrival of the first whole batches (GKC_SINK_DEBUG timeline: 13 ms at 5e7 reads).
        else if (in.sink && in.sink_first_div > 1 && !in.key_budget) {
            const size_t sink_first_div = in.sink_first_div;
            const size_t small = std::max<size_t>(budget / 4, (size_t)1 << 20), tail = small * (size_t)lanes;      // keys kept back for the small last batches
            const size_t ramp = sink_first_div >> std::min<uint32_t>(lane_batches[lane], 31u);                     // 4, 2, 1 (GKC_SINK_FIRST_DIV: the first divisor; measured 1/4: 483.8 ms per step, 1/8: 490.4, 1/16: 491.8; no ramp: 498.3)
            if (ramp > 1) budget = std::max<size_t>(budget / ramp, (size_t)1 << 20);
            else if (keys_left <= tail + small / 2) budget = small;
            else if (keys_left < budget + tail) budget = std::max<size_t>(small, (size_t)(keys_left - tail));
        }
        lane_batches[lane]++;
        uint64_t acc = 0;
        while (next_p < Pn) {
            const uint32_t p = next_p;
            if (part_keys[p] == 0) { mark_empty(p); next_p++; continue; }      // nothing to count (e.g. a partition another rank owns): an empty, finished dataset
            if (!batch.empty() && acc + part_keys[p] > budget) break;
            batch.push_back(p); acc += part_keys[p]; next_p++;
        }
        inflight[lane] = (double)acc * per_key_now();
        keys_left -= std::min<uint64_t>(keys_left, acc);
        return !batch.empty();
    }
    // a lane's batch is through: what it counted (keys, resident records) ...
    void finished(int lane, uint64_t keys, uint64_t solid) { std::lock_guard<std::mutex> lk(mu); inflight[lane] = 0; done_keys += keys; done_solid += solid; }
    // ... or the error it ended with: the pass carves no further batch
    void failed(int lane, int rc) { std::lock_guard<std::mutex> lk(mu); inflight[lane] = 0; if (first_rc == 0) first_rc = rc; }
    int rc() { std::lock_guard<std::mutex> lk(mu); return first_rc; }
};
