// gkc_simplify.hip — the compacted graph simplified on the device: tips, bulges and erroneous connections removed in rounds to a fixed point (include/gkc.h, "tips":
// candidate, tip, competitor, round; "simplify": names, bulge, erroneous connection, schedule). gkc_graph_tips_remove is the first phase of gkc_graph_simplify's schedule
// run alone.
//
// A round works on the placement (ut_build, gkc_unitigs.hip) and the link CSR (ut_links, gkc_unitig_links.hip) of the alive records:
//   k_tip_kc      : one thread per record: the abundance sums KC of the unitigs (64-bit vector atomics; the emit kernel's sum without the bases).
//   k_tip_flags   : one thread per unitig: the degrees of its two slots from the link offsets, its length from first[], the topological rule; for the coverage rule the
//                   entries of its linked slot and of the arrival slot of each (at most five slots), every comparison in 128-bit integers. One flag byte per unitig.
//   k_tip_mark    : one thread per slot of a SURVIVING unitig: a slot with an entry whose unitig is flagged goes on a work list (side-0 slots from the front of the list,
//                   side-1 slots from its back: a single-record unitig has both sides in one mask byte, and each list is refreshed by a launch of its own).
//   k_tip_kill    : one thread per record: the records of flagged unitigs die, alive[i] = 0, masks[i] = 0.
//   k_tip_refresh : one thread per listed slot, so that nearly every lane searches (extremities are few among the records). For each bit of the
//                   outward nibble of the slot's record the neighbour is built and searched (gr_end_search, as in k_unitig_link_fill); the bit of a neighbour that has died is cleared.
//                   Only extremities name records of other unitigs, so no other mask changes. A neighbour that is no record raises *bad.
#include "gkc_unitigs.hpp"

struct TipRule { uint32_t k, max_len_topo, max_len_rc, rc_num, rc_den; };
struct TipCounters { unsigned long long n_tips, n_removed; uint32_t n_work[2], bad, pad; };      // one device word block per round

template <int KW>
__global__ __launch_bounds__(256) void k_tip_kc(const QDs* __restrict__ ds, uint32_t n_ds, uint64_t n, const uint64_t* __restrict__ unitig, unsigned long long* __restrict__ kc)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t U = unitig[i];
        if (U == ~0ull) continue;
        const QDs D = ds[gr_dataset_of(ds, n_ds, i)];
        atomicAdd(&kc[U >> 1], (unsigned long long)*reinterpret_cast<const uint32_t*>(D.recs + (i - D.base) * (uint64_t)RB + sizeof(key_t)));
    }
}
// "c is that much better covered than u": KC_c L_u rc_den > rc_num KC_u L_c, exactly (KC < 2^63, L < 2^31, the ratio's terms < 2^32: the products stay below 2^126)
__device__ __forceinline__ bool ut_better_covered(const TipRule& R, uint64_t kc_c, uint64_t len_c, uint64_t kc_u, uint64_t len_u)
{
    return (unsigned __int128)kc_c * (unsigned __int128)(len_u * R.rc_den) > (unsigned __int128)kc_u * (unsigned __int128)(len_c * R.rc_num);
}
__device__ __forceinline__ void ut_count_hits(bool hit, unsigned long long* __restrict__ counter)      // one atomic per wave
{
    const unsigned long long vote = __ballot(hit);
    if (hit && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)vote) - 1u) atomicAdd(counter, (unsigned long long)__popcll(vote));
}
__global__ __launch_bounds__(256) void k_tip_flags(TipRule R, uint64_t n_unitigs, uint64_t n_alive, const uint64_t* __restrict__ first, const uint64_t* __restrict__ loff,
                                                    const uint64_t* __restrict__ links, const unsigned long long* __restrict__ kc, uint8_t* __restrict__ flag, TipCounters* __restrict__ cnt)
{
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_unitigs; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = loff[2 * u], o1 = loff[2 * u + 1], o2 = loff[2 * u + 2];
        bool tip = false;
        if ((o1 == o0) != (o2 == o1)) {                        // a candidate: exactly one side without a link
            const uint32_t su = o1 != o0 ? 0u : 1u;
            const uint64_t len_u = ut_length(first, n_alive, n_unitigs, u), bases = len_u + R.k - 1;
            tip = bases <= R.max_len_topo;
            if (!tip && bases <= R.max_len_rc) {
                const uint64_t kc_u = kc[u], back = (u << 1) | (1u - su);
                const uint64_t b = su ? o1 : o0, e = su ? o2 : o1;
                for (uint64_t q = b; q < e && !tip; q++) {     // the entries (v, m) of the linked slot: at most four
                    const uint64_t ent = links[q], v = ent >> 1;
                    tip = ut_better_covered(R, kc[v], ut_length(first, n_alive, n_unitigs, v), kc_u, len_u);
                    const uint64_t t2 = 2 * v + (1u - (uint32_t)(ent & 1));      // the slot one arrives through: its other entries are u's siblings
                    bool skipped = false;
                    for (uint64_t p = loff[t2], pe = loff[t2 + 1]; p < pe && !tip; p++) {
                        const uint64_t w = links[p];
                        if (!skipped && w == back) { skipped = true; continue; }      // the one entry that is u coming back
                        tip = ut_better_covered(R, kc[w >> 1], ut_length(first, n_alive, n_unitigs, w >> 1), kc_u, len_u);
                    }
                }
            }
        }
        flag[u] = tip ? 1 : 0;
        ut_count_hits(tip, &cnt->n_tips);
    }
}
__global__ __launch_bounds__(256) void k_tip_mark(uint64_t n_slots, const uint64_t* __restrict__ loff, const uint64_t* __restrict__ links, const uint8_t* __restrict__ flag,
                                                   uint32_t* __restrict__ work, TipCounters* __restrict__ cnt)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_slots; t += (uint64_t)gridDim.x * blockDim.x) {
        if (flag[t >> 1]) continue;
        bool any = false;
        for (uint64_t p = loff[t], pe = loff[t + 1]; p < pe; p++) any = any || flag[links[p] >> 1];
        if (!any) continue;
        const uint32_t at = atomicAdd(&cnt->n_work[t & 1], 1u);      // (few: the neighbours of the round's tips; n_work[0] + n_work[1] <= n_slots < 2^32)
        work[(t & 1) ? n_slots - 1 - at : at] = (uint32_t)t;
    }
}
__global__ __launch_bounds__(256) void k_tip_kill(uint64_t n, const uint64_t* __restrict__ unitig, const uint8_t* __restrict__ flag, uint8_t* __restrict__ alive, uint8_t* __restrict__ masks,
                                                   TipCounters* __restrict__ cnt)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t U = unitig[i];
        const bool dies = U != ~0ull && flag[U >> 1];
        if (dies) { alive[i] = 0; masks[i] = 0; }
        ut_count_hits(dies, &cnt->n_removed);
    }
}
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_tip_refresh(QParams P, uint32_t n_ds, uint64_t n, const uint32_t* __restrict__ work, uint64_t n_work, const uint32_t* __restrict__ slot_rec,
                                                             const uint8_t* __restrict__ alive, uint8_t* __restrict__ masks, TipCounters* __restrict__ cnt)
{
    GrNode<KW> N(P);
    for (uint64_t w = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; w < n_work; w += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t sr = slot_rec[work[w]], s = sr & 1u;    // the record whose end s is this side; no other thread of this launch has the same record (one side per launch)
        const uint64_t i = sr >> 1;
        const uint32_t mk = masks[i], nib = (mk >> (4u * s)) & 15u;
        if (!nib) continue;
        N.load(P, n_ds, i);
        uint32_t gone = 0;
        gr_end_search(P, N, s, nib, [&](uint32_t nt, bool named, bool found, uint64_t j, uint32_t) {
            if (!named) return;
            if (found && j < n) { if (!alive[j]) gone |= 1u << nt; }
            else cnt->bad = 1u;                                // the host answers GKC_ERR_ARG
        });
        if (gone) masks[i] = (uint8_t)(mk & ~(gone << (4u * s)));
    }
}

// ------------------------------------------------------------------------------------------------ bulges, erroneous connections
// Two more flag kernels in the shape of k_tip_flags, over the same placement, link CSR and KC; k_tip_mark, k_tip_kill and k_tip_refresh only read the flag bytes and serve
// every kind. An entry e of slot t says that t NAMES slot e ^ 1 (e = v << 1 | m names (v, 1 - m)), so a whole rule is a walk over the CSR: no search, no record is read.
//   k_bulge_flags : one thread per unitig u: for every X that (u, 0) names and every (c, o) that X names (at most 16), c parallel to u between X and some Y that (u, 1)
//                   and (c, 1 - o) both name (at most 4 x 4 comparisons), c not too long and better covered (128-bit products; the tie goes to the lower index).
//   k_ec_flags    : one thread per unitig u: a sibling at both ends (some slot it names has two entries or more), then the competitors of the tips rule on both sides.
struct BulgeRule { uint32_t k, max_len, alt_num, alt_den, alt_add; };
struct EcRule { uint32_t k, max_len, num, den; };

// "c beats u": KC_u L_c < KC_c L_u, or the two products are equal and c < u (a strict total order; KC < 2^63, L < 2^31)
__device__ __forceinline__ bool ut_beats(uint64_t c, uint64_t kc_c, uint64_t len_c, uint64_t u, uint64_t kc_u, uint64_t len_u)
{
    const unsigned __int128 a = (unsigned __int128)kc_u * (unsigned __int128)len_c, b = (unsigned __int128)kc_c * (unsigned __int128)len_u;
    return a < b || (a == b && c < u);
}
__device__ __forceinline__ bool ut_slot_has(const uint64_t* __restrict__ loff, const uint64_t* __restrict__ links, uint64_t t, uint64_t entry)
{
    bool has = false;
    for (uint64_t p = loff[t], pe = loff[t + 1]; p < pe; p++) has = has || links[p] == entry;
    return has;
}
__global__ __launch_bounds__(256) void k_bulge_flags(BulgeRule R, uint64_t n_unitigs, uint64_t n_alive, const uint64_t* __restrict__ first, const uint64_t* __restrict__ loff,
                                                      const uint64_t* __restrict__ links, const unsigned long long* __restrict__ kc, uint8_t* __restrict__ flag, TipCounters* __restrict__ cnt)
{
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_unitigs; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = loff[2 * u], o1 = loff[2 * u + 1], o2 = loff[2 * u + 2];
        const uint64_t len_u = ut_length(first, n_alive, n_unitigs, u);
        bool hit = false;
        if (o1 != o0 && o2 != o1 && len_u + R.k - 1 <= R.max_len) {
            const uint64_t kc_u = kc[u];
            const uint64_t by_ratio = len_u * R.alt_num / R.alt_den, by_sum = len_u + R.alt_add, max_len_c = by_ratio > by_sum ? by_ratio : by_sum;
            for (uint64_t p = o0; p < o1 && !hit; p++) {           // X: a slot (u, 0) names
                const uint64_t X = links[p] ^ 1ull;
                if ((X >> 1) == u) continue;
                for (uint64_t q = loff[X], qe = loff[X + 1]; q < qe && !hit; q++) {      // (c, o): a slot X names
                    const uint64_t C = links[q] ^ 1ull, c = C >> 1;
                    if (c == u || c == (X >> 1)) continue;
                    const uint64_t len_c = ut_length(first, n_alive, n_unitigs, c);
                    if (len_c > max_len_c || !ut_beats(c, kc[c], len_c, u, kc_u, len_u)) continue;
                    if (!ut_slot_has(loff, links, C, X ^ 1ull)) continue;      // (c, o) names X
                    for (uint64_t y = o1; y < o2 && !hit; y++) {   // Y: a slot (u, 1) names and (c, 1 - o) names
                        const uint64_t ent = links[y], yv = ent >> 1;
                        if (yv == u || yv == c) continue;
                        hit = ut_slot_has(loff, links, C ^ 1ull, ent);
                    }
                }
            }
        }
        flag[u] = hit ? 1 : 0;
        ut_count_hits(hit, &cnt->n_tips);
    }
}
__global__ __launch_bounds__(256) void k_ec_flags(EcRule R, uint64_t n_unitigs, uint64_t n_alive, const uint64_t* __restrict__ first, const uint64_t* __restrict__ loff,
                                                   const uint64_t* __restrict__ links, const unsigned long long* __restrict__ kc, uint8_t* __restrict__ flag, TipCounters* __restrict__ cnt)
{
    const TipRule T{R.k, 0u, 0u, R.num, R.den};                    // the comparison of the tips rule: KC_c L_u den > num KC_u L_c
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_unitigs; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = loff[2 * u], o1 = loff[2 * u + 1], o2 = loff[2 * u + 2];
        const uint64_t len_u = ut_length(first, n_alive, n_unitigs, u);
        bool hit = false;
        if (o1 != o0 && o2 != o1 && len_u + R.k - 1 <= R.max_len) {
            bool sib0 = false, sib1 = false;
            for (uint64_t p = o0; p < o1; p++) { const uint64_t t2 = links[p] ^ 1ull; sib0 = sib0 || loff[t2 + 1] - loff[t2] >= 2; }
            for (uint64_t p = o1; p < o2; p++) { const uint64_t t2 = links[p] ^ 1ull; sib1 = sib1 || loff[t2 + 1] - loff[t2] >= 2; }
            if (sib0 && sib1) {
                const uint64_t kc_u = kc[u];
                for (uint64_t q = o0; q < o2 && !hit; q++) {       // the entries (v, m) of both slots
                    const uint64_t ent = links[q], v = ent >> 1, back = (u << 1) | (q < o1 ? 1u : 0u);
                    if (v != u) hit = ut_better_covered(T, kc[v], ut_length(first, n_alive, n_unitigs, v), kc_u, len_u);
                    bool skipped = false;
                    for (uint64_t p = loff[ent ^ 1ull], pe = loff[(ent ^ 1ull) + 1]; p < pe && !hit; p++) {
                        const uint64_t w = links[p];
                        if (!skipped && w == back) { skipped = true; continue; }      // the one entry that is u coming back
                        if ((w >> 1) != u) hit = ut_better_covered(T, kc[w >> 1], ut_length(first, n_alive, n_unitigs, w >> 1), kc_u, len_u);
                    }
                }
            }
        }
        flag[u] = hit ? 1 : 0;
        ut_count_hits(hit, &cnt->n_tips);
    }
}
// ------------------------------------------------------------------------------------------------ the round all kinds share
enum : uint32_t { UT_KIND_TIPS = 0, UT_KIND_BULGES = 1, UT_KIND_EC = 2 };
static const char* const UT_KIND_TIMING[3] = {"graph_tips", "graph_bulges", "graph_ec"};
struct SimplifyRules { TipRule tips; BulgeRule bulges; EcRule ec; };
// The graph the rounds of a call work on: the placement in the context, its link CSR, the record of every slot and KC. A round that removes nothing leaves all of it
// valid, and the next round of whatever kind starts on it; a round that removes something clears ``fresh`` and the next one builds again.
struct RoundGraph {
    DevBuf loff, lnk, slot, kc;
    uint64_t n_alive = 0, removed = 0;
    bool subset = false;                                       // build over d_alive (something was removed, or the call resumed an earlier state)
    bool fresh = false, kc_done = false;
};
static int ut_round_graph(gkc_ctx* c, const char* who, const uint8_t* d_masks, const uint8_t* d_alive, RoundGraph& G)
{
    UnitigPlacement& U = c->unitigs;
    GKC_TRY(ut_build(c, who, d_masks, G.subset ? d_alive : nullptr, G.n_alive, nullptr, nullptr, nullptr));
    G.kc_done = false;
    const uint64_t nu = U.n_unitigs, n_slots = 2 * nu;
    if (nu) {
        uint64_t nl = 0;
        int rc = ut_links(c, d_masks, nullptr, 0, nullptr, 0, &nl, nullptr);
        if (rc == GKC_OK) rc = c->ensure(G.loff, (size_t)(n_slots + 1) * 8);
        if (rc == GKC_OK) rc = c->ensure(G.lnk, (size_t)(nl ? nl : 1) * 8);
        if (rc == GKC_OK) rc = c->ensure(G.slot, (size_t)n_slots * 4);
        if (rc == GKC_OK) rc = c->ensure(G.kc, (size_t)nu * 8);
        if (rc == GKC_OK) rc = ut_links(c, d_masks, (uint64_t*)G.loff.p, nu, (uint64_t*)G.lnk.p, nl, &nl, (uint32_t*)G.slot.p);
        if (rc != GKC_OK) { U.drop(); return rc; }
    }
    G.fresh = true;
    return GKC_OK;
}
// One round of ``kind``: build, links (when the graph is not fresh), KC (once per graph), flags(kind), mark, kill, one read-back, then the refresh per side.
// *n_unitigs: of the graph the round was decided on; *n_hits, *n_removed: what it removed. Timing: the kind's name, one launch per round on a graph that has unitigs.
static int ut_round(gkc_ctx* c, const char* who, uint8_t* d_masks, uint8_t* d_alive, RoundGraph& G, uint32_t kind, const SimplifyRules& R, uint64_t* n_unitigs, uint64_t* n_hits,
                    uint64_t* n_removed)
{
    UnitigPlacement& U = c->unitigs;
    *n_unitigs = *n_hits = *n_removed = 0;
    if (!G.fresh) GKC_TRY(ut_round_graph(c, who, d_masks, d_alive, G));
    const uint64_t n = U.n, nu = U.n_unitigs, n_slots = 2 * nu;
    *n_unitigs = nu;
    if (!nu) return GKC_OK;                                    // nothing alive: an empty round
    const uint32_t n_ds = (uint32_t)c->datasets.size();
    DevBuf d_flag, d_work, d_cnt;
    int rc = c->ensure(d_flag, (size_t)nu);
    if (rc == GKC_OK) rc = c->ensure(d_work, (size_t)n_slots * 4);
    if (rc == GKC_OK) rc = c->ensure(d_cnt, sizeof(TipCounters));
    if (rc != GKC_OK) { U.drop(); return rc; }
    TipCounters h{};
    hipError_t e;
    {
        ScopedTimer tm(c, UT_KIND_TIMING[kind]);               // its launch count: the rounds of the kind
        const dim3 block(256), per_rec(q_grid((n + 255) / 256)), per_unitig(q_grid((nu + 255) / 256)), per_slot(q_grid((n_slots + 255) / 256));
        const QDs* ds = (const QDs*)c->qidx.table.p;
        const uint64_t* unitig = (const uint64_t*)U.unitig.p; const uint64_t* first = (const uint64_t*)U.first.p;
        const uint64_t* loff = (const uint64_t*)G.loff.p; const uint64_t* lnk = (const uint64_t*)G.lnk.p; const unsigned long long* kc = (const unsigned long long*)G.kc.p;
        uint8_t* flag = (uint8_t*)d_flag.p;
        TipCounters* cnt = (TipCounters*)d_cnt.p;
        e = hipMemsetAsync(cnt, 0, sizeof(TipCounters), c->stream);
        if (e == hipSuccess && !G.kc_done) e = hipMemsetAsync(G.kc.p, 0, (size_t)nu * 8, c->stream);
        if (e == hipSuccess) {
            if (!G.kc_done) GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_tip_kc<KW>), per_rec, block, 0, c->stream, ds, n_ds, n, unitig, (unsigned long long*)G.kc.p));
            if (kind == UT_KIND_TIPS)        hipLaunchKernelGGL(k_tip_flags, per_unitig, block, 0, c->stream, R.tips, nu, G.n_alive, first, loff, lnk, kc, flag, cnt);
            else if (kind == UT_KIND_BULGES) hipLaunchKernelGGL(k_bulge_flags, per_unitig, block, 0, c->stream, R.bulges, nu, G.n_alive, first, loff, lnk, kc, flag, cnt);
            else                             hipLaunchKernelGGL(k_ec_flags, per_unitig, block, 0, c->stream, R.ec, nu, G.n_alive, first, loff, lnk, kc, flag, cnt);
            hipLaunchKernelGGL(k_tip_mark, per_slot, block, 0, c->stream, n_slots, loff, lnk, (const uint8_t*)flag, (uint32_t*)d_work.p, cnt);
            hipLaunchKernelGGL(k_tip_kill, per_rec, block, 0, c->stream, n, unitig, (const uint8_t*)flag, d_alive, d_masks, cnt);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&h, cnt, sizeof(TipCounters), hipMemcpyDeviceToHost, c->stream);
        hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess) G.kc_done = true;
        if (e == hipSuccess && (uint64_t)h.n_work[0] + h.n_work[1] > n_slots) e = hipErrorUnknown;      // (cannot be: a slot is listed once)
        if (e == hipSuccess && h.n_tips && (h.n_work[0] || h.n_work[1])) {
            QParams P{}; q_fill_params(P, q_model_of(c), c->qidx);
            for (uint32_t side = 0; side < 2; side++) {        // one launch per side: a record is at most one slot of a side
                const uint64_t nw = h.n_work[side];
                if (!nw) continue;
                const uint32_t* work = (const uint32_t*)d_work.p + (side ? n_slots - nw : 0);
                const dim3 grid(q_grid((nw + GR_THREADS - 1) / GR_THREADS)), blk(GR_THREADS);
                GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_tip_refresh<KW>), grid, blk, 0, c->stream, P, n_ds, n, work, nw, (const uint32_t*)G.slot.p, (const uint8_t*)d_alive, d_masks, cnt));
            }
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&h.bad, &cnt->bad, 4, hipMemcpyDeviceToHost, c->stream);
        }
        es = hipStreamSynchronize(c->stream);                  // (also after a failure: the scratch goes back to the pool)
        if (e == hipSuccess) e = es;
    }
    if (e != hipSuccess) { U.drop(); GKC_HIP(c, e); }
    *n_hits = h.n_tips;
    if (!h.n_tips) return GKC_OK;
    G.fresh = false;                                           // the masks and the alive array have changed: the placement is no longer theirs
    if (h.bad || h.n_removed > G.n_alive) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: d_masks name a neighbour that is no record of these results (the masks of other results?); d_masks and d_alive are not to be used", who); }
    *n_removed = h.n_removed;
    G.removed += h.n_removed; G.n_alive -= h.n_removed; G.subset = true;
    return GKC_OK;
}
// the placement of the final graph, when the last round changed it (or none ran)
static int ut_rounds_finish(gkc_ctx* c, const char* who, const uint8_t* d_masks, const uint8_t* d_alive, RoundGraph& G)
{
    if (G.fresh) return GKC_OK;
    GKC_TRY(ut_build(c, who, d_masks, G.subset ? d_alive : nullptr, G.n_alive, nullptr, nullptr, nullptr));
    G.fresh = true;
    return GKC_OK;
}

// What a call runs: a tips phase (sweep 0), then up to max_sweeps sweeps of a bulge, an erroneous-connection and a tips phase, until a sweep removes nothing. A phase:
// rounds of its kind until one removes nothing or max_rounds[kind] have run. gkc_graph_tips_remove is max_sweeps == 0.
struct UtSchedule { SimplifyRules R; uint32_t max_rounds[3], max_sweeps; bool resume; };
// Both entry points behind their NULL-context guard. check(S): the caller's own argument checks (after q_prepare), which fill S; a failure drops the placement.
// tips_per_round (gkc_graph_tips_remove) / log (gkc_graph_simplify): where the rounds are written down, or NULL.
template <typename Check>
static int ut_simplify_run(gkc_ctx* c, const char* who, uint8_t* d_masks, uint8_t* d_alive, Check&& check, uint64_t* tips_per_round, gkc_simplify_round* log, uint64_t cap_log,
                           uint64_t* n_rounds, uint64_t* n_records_removed, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    if (n_rounds) *n_rounds = 0;
    if (n_records_removed) *n_records_removed = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (n_cycles) *n_cycles = 0;
    GKC_TRY(q_prepare(c, who));
    UnitigPlacement& U = c->unitigs;
    UtSchedule S{};
    { const int rc = check(S); if (rc != GKC_OK) { U.drop(); return rc; } }
    if (!d_masks || !d_alive) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the masks (in, out) and the alive array (%s) are required", who, S.resume ? "in, out" : "out"); }
    if (tips_per_round) for (uint32_t r = 0; r < S.max_rounds[UT_KIND_TIPS]; r++) tips_per_round[r] = 0;
    const uint64_t n = gr_total(c);
    RoundGraph G; G.n_alive = n;
    if (n && !S.resume) { GKC_HIP(c, hipMemsetAsync(d_alive, 1, (size_t)n, c->stream)); GKC_HIP(c, hipStreamSynchronize(c->stream)); }
    else if (n) {                                              // the state an earlier call left: count it, and see that no dead record has a mask
        DevBuf d_cnt; bool bad = false;
        GKC_TRY(c->ensure(d_cnt, 16));
        const int rc = ut_alive_count(c, d_cnt.p, d_alive, d_masks, n, &G.n_alive, &bad);
        if (rc != GKC_OK) { U.drop(); return rc; }
        if (bad) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: resume: a dead record of d_alive has a mask in d_masks (not a state an earlier call left)", who); }
        G.subset = true;
    }
    uint64_t rounds = 0;
    auto phase = [&](uint32_t kind, uint32_t sweep, uint64_t* gone_phase) -> int {
        for (uint32_t r = 0; r < S.max_rounds[kind]; r++) {
            uint64_t nu = 0, hits = 0, gone = 0;
            GKC_TRY(ut_round(c, who, d_masks, d_alive, G, kind, S.R, &nu, &hits, &gone));
            if (tips_per_round) tips_per_round[rounds] = hits;
            if (log && rounds < cap_log) log[rounds] = gkc_simplify_round{kind, sweep, nu, hits, gone};
            rounds++;
            *gone_phase += gone;
            if (!hits) break;
        }
        return GKC_OK;
    };
    uint64_t gone = 0;
    GKC_TRY(phase(UT_KIND_TIPS, 0, &gone));
    for (uint32_t sweep = 1; sweep <= S.max_sweeps; sweep++) {
        gone = 0;
        GKC_TRY(phase(UT_KIND_BULGES, sweep, &gone));
        GKC_TRY(phase(UT_KIND_EC, sweep, &gone));
        GKC_TRY(phase(UT_KIND_TIPS, sweep, &gone));
        if (!gone) break;
    }
    GKC_TRY(ut_rounds_finish(c, who, d_masks, d_alive, G));
    if (n_rounds) *n_rounds = rounds;
    if (n_records_removed) *n_records_removed = G.removed;
    if (n_unitigs) *n_unitigs = U.n_unitigs;
    if (n_bases) *n_bases = U.n_bases;
    if (n_cycles) *n_cycles = U.n_cycles;
    return GKC_OK;
}

extern "C" {

int gkc_graph_tips_remove(gkc_ctx* c, uint8_t* d_masks, uint8_t* d_alive, const gkc_tip_params* params, uint64_t* n_rounds, uint64_t* tips_per_round, uint64_t* n_records_removed,
                          uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    static const char* who = "gkc_graph_tips_remove";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    auto check = [&](UtSchedule& S) -> int {
        if (!params || params->rc_den == 0 || params->max_rounds > 64) GKC_FAIL(c, GKC_ERR_ARG, "%s: the parameters are required, rc_den != 0, max_rounds <= 64", who);
        S.R.tips = TipRule{c->k, params->max_len_topo, params->max_len_rc, params->rc_num, params->rc_den};
        S.max_rounds[UT_KIND_TIPS] = params->max_rounds;
        return GKC_OK;
    };
    return ut_simplify_run(c, who, d_masks, d_alive, check, tips_per_round, nullptr, 0, n_rounds, n_records_removed, n_unitigs, n_bases, n_cycles);
}

int gkc_graph_simplify(gkc_ctx* c, uint8_t* d_masks, uint8_t* d_alive, const gkc_simplify_params* params, gkc_simplify_round* log, uint64_t cap_log, uint64_t* n_rounds,
                       uint64_t* n_records_removed, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    static const char* who = "gkc_graph_simplify";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    auto check = [&](UtSchedule& S) -> int {
        if (!params || params->tips.rc_den == 0 || params->bulge_alt_den == 0 || params->ec_den == 0)
            GKC_FAIL(c, GKC_ERR_ARG, "%s: the parameters are required, tips.rc_den != 0, bulge_alt_den != 0, ec_den != 0", who);
        if (params->tips.max_rounds > 64 || params->bulge_max_rounds > 64 || params->ec_max_rounds > 64 || params->max_sweeps > 16)
            GKC_FAIL(c, GKC_ERR_ARG, "%s: max_rounds <= 64 for every kind, max_sweeps <= 16", who);
        S.R.tips = TipRule{c->k, params->tips.max_len_topo, params->tips.max_len_rc, params->tips.rc_num, params->tips.rc_den};
        S.R.bulges = BulgeRule{c->k, params->bulge_max_len, params->bulge_alt_num, params->bulge_alt_den, params->bulge_alt_add};
        S.R.ec = EcRule{c->k, params->ec_max_len, params->ec_num, params->ec_den};
        S.max_rounds[UT_KIND_TIPS] = params->tips.max_rounds; S.max_rounds[UT_KIND_BULGES] = params->bulge_max_rounds; S.max_rounds[UT_KIND_EC] = params->ec_max_rounds;
        S.max_sweeps = params->max_sweeps; S.resume = params->resume != 0;
        return GKC_OK;
    };
    return ut_simplify_run(c, who, d_masks, d_alive, check, nullptr, log, cap_log, n_rounds, n_records_removed, n_unitigs, n_bases, n_cycles);
}

}  // extern "C"
