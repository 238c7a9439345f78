// gkc_unitig_links.hip — links between the unitigs: the edges of the compacted graph (include/gkc.h, "unitigs": side, slot, entry; the L: fields of bcalm2), over the
// placement kept by gkc_graph_unitigs_build (gkc_unitigs.hip).
//
//   k_unitig_link_count   : one thread per record. The record at position 0 of unitig u writes the degree of its outward end to cnt[2 u + 1], the one at position L_u - 1
//                           to cnt[2 u]; a single-record unitig writes both. Every slot is written exactly once, with its record and end beside the count.
//   k_graph_tile_sums, gr_scan_tiles, k_graph_tile_offsets<true> (gkc_graph.hpp) over cnt[]: the prefix sum -> offsets[2 n_unitigs + 1];
//   k_unitig_link_fill    : one thread per SLOT, from the record << 1 | end the count kernel left per slot, so that every lane of a wave searches (extremities are
//                           few among the records). A side searches its four neighbours (gr_end_search), reads the placement of the records found,
//                           forms the entries, sorts the four of the slot in registers (empty ones last) and stores the first deg of them at offsets[slot]. A neighbour
//                           the masks name that is no record (masks of other results) raises *bad.
#include "gkc_unitigs.hpp"

constexpr uint32_t UT_INNER = 2u;                              // ut_sides: this end of the record lies inside its path
// which side of its unitig (0: '+', 1: '-') each end of record i is
// (n_alive: the records placed, all of them unless the placement was built over an alive array; a dead record, unitig ~0, has no side)
__device__ __forceinline__ void ut_sides(const uint64_t* __restrict__ unitig, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ first, uint64_t n_alive, uint64_t n_unitigs,
                                         uint64_t i, uint64_t& u, uint32_t& side_r, uint32_t& side_l)
{
    const uint64_t U = unitig[i];
    side_r = UT_INNER; side_l = UT_INNER;
    if (U == ~0ull) { u = 0; return; }
    u = U >> 1;
    const bool rev = U & 1;
    const uint32_t p = pos[i];
    if (p == 0) { if (rev) side_r = 1u; else side_l = 1u; }
    if ((uint64_t)p + 1 == ut_length(first, n_alive, n_unitigs, u)) { if (rev) side_l = 0u; else side_r = 0u; }
}
__global__ __launch_bounds__(256) void k_unitig_link_count(const uint8_t* __restrict__ masks, const uint64_t* __restrict__ unitig, const uint32_t* __restrict__ pos,
                                                            const uint64_t* __restrict__ first, uint64_t n, uint64_t n_alive, uint64_t n_unitigs, uint32_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ slot_rec)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t u; uint32_t side_r, side_l;
        ut_sides(unitig, pos, first, n_alive, n_unitigs, i, u, side_r, side_l);
        if (side_r == UT_INNER && side_l == UT_INNER) continue;
        const uint32_t mk = masks[i];
        if (side_r != UT_INNER) { cnt[2 * u + side_r] = (uint32_t)__popc(mk & 15u); slot_rec[2 * u + side_r] = (uint32_t)i << 1; }      // (i < 2^31: the build's guard)
        if (side_l != UT_INNER) { cnt[2 * u + side_l] = (uint32_t)__popc((mk >> 4) & 15u); slot_rec[2 * u + side_l] = ((uint32_t)i << 1) | 1u; }
    }
}
struct UtSlotCount { const uint32_t* cnt; __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return cnt[i]; } };      // the value of a slot in the prefix sum
__device__ __forceinline__ void ut_order(uint64_t& a, uint64_t& b) { const uint64_t lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_unitig_link_fill(QParams P, uint32_t n_ds, uint64_t n, uint64_t n_slots, const uint8_t* __restrict__ masks,
                                                                  const uint64_t* __restrict__ unitig, const uint32_t* __restrict__ slot_rec,
                                                                  const uint64_t* __restrict__ offsets, uint64_t* __restrict__ links, uint32_t* __restrict__ bad)
{
    GrNode<KW> N(P);
    for (uint64_t t = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; t < n_slots; t += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t sr = slot_rec[t], s = sr & 1u;          // the record whose end s is this side
        const uint64_t i = sr >> 1;
        const uint32_t nib = ((uint32_t)masks[i] >> (4u * s)) & 15u;
        if (!nib) continue;
        N.load(P, n_ds, i);
        uint64_t e[4];
        gr_end_search(P, N, s, nib, [&](uint32_t nt, bool named, bool found, uint64_t j, uint32_t a) {
            uint64_t ent = ~0ull;
            if (named && found && j < n && unitig[j] != ~0ull) {       // (found, and alive: always, with the masks of these results and of this alive array)
                const uint64_t V = unitig[j];
                const bool begin = a == ((V & 1) ? 0u : 1u);   // one arrives at the outward end of the record at position 0
                ent = (V & ~1ull) | (begin ? 0ull : 1ull);
            } else if (named) *bad = 1u;                       // the host answers GKC_ERR_ARG
            e[nt] = ent;
        });
        ut_order(e[0], e[1]); ut_order(e[2], e[3]); ut_order(e[0], e[2]); ut_order(e[1], e[3]); ut_order(e[1], e[2]);
        const uint64_t off = offsets[t], deg = offsets[t + 1] - off;      // (= popcount(nib): what k_unitig_link_count saw in the same masks)
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) if (q < deg) links[off + q] = e[q];
    }
}

int ut_links(gkc_ctx* c, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs, uint64_t* d_links, uint64_t cap_links, uint64_t* n_links, uint32_t* d_keep_slots)
{
    UnitigPlacement& U = c->unitigs;
    if (d_links && !d_link_offsets) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_links: links without offsets (both, or neither to count only)");
    if (U.subset && !d_masks) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_links: the placement was built over an alive array, the masks that went with it are required");
    const uint64_t n = U.n, n_slots = 2 * U.n_unitigs;
    if (!n_slots) {                                            // no record, or none alive
        if (d_link_offsets) { GKC_HIP(c, hipMemsetAsync(d_link_offsets, 0, 8, c->stream)); GKC_HIP(c, hipStreamSynchronize(c->stream)); }
        return GKC_OK;
    }
    if (!d_link_offsets && U.links_counted) { if (n_links) *n_links = U.n_links; return GKC_OK; }      // the sizing call after a count of these results
    const uint32_t n_tiles = (uint32_t)((n_slots + GR_TILE - 1) / GR_TILE), n_ds = (uint32_t)c->datasets.size();
    const bool own_masks = !d_masks;
    DevBuf tmp, d_cnt, d_ts, d_slot;
    ScopedTimer tm(c, "graph_unitig_links");
    if (own_masks) GKC_TRY(c->ensure(tmp, (size_t)n));         // every allocation before the first launch: a failure returns with nothing in flight
    GKC_TRY(c->ensure(d_cnt, (size_t)n_slots * 4)); GKC_TRY(c->ensure(d_ts, ((size_t)n_tiles + 2) * 8));
    if (!d_keep_slots) GKC_TRY(c->ensure(d_slot, (size_t)n_slots * 4));
    uint32_t* slot_rec = d_keep_slots ? d_keep_slots : (uint32_t*)d_slot.p;
    if (own_masks) {
        const int rc = gr_masks_run(c, 0, n, (uint8_t*)tmp.p);
        if (rc != GKC_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
        d_masks = (const uint8_t*)tmp.p;
    }
    const uint64_t* unitig = (const uint64_t*)U.unitig.p; const uint32_t* pos = (const uint32_t*)U.pos.p; const uint64_t* first = (const uint64_t*)U.first.p;
    uint32_t* cnt = (uint32_t*)d_cnt.p; uint64_t* ts = (uint64_t*)d_ts.p;
    const dim3 tiles(q_grid(n_tiles)), block(GR_THREADS);
    uint64_t total = 0;
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n_slots * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(slot_rec, 0, (size_t)n_slots * 4, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_unitig_link_count, dim3(q_grid((n + 255) / 256)), dim3(256), 0, c->stream, d_masks, unitig, pos, first, n, U.n_alive, U.n_unitigs, cnt, slot_rec);
        hipLaunchKernelGGL(k_graph_tile_sums<UtSlotCount>, tiles, block, 0, c->stream, UtSlotCount{cnt}, n_slots, n_tiles, ts);
        gr_scan_tiles(c, ts, nullptr, n_tiles);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, ts + n_tiles, 8, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);     // (also after a failure: the scratch goes back to the pool)
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (n_links) *n_links = total;
    if (own_masks) { U.n_links = total; U.links_counted = true; }      // (masks handed in count once they have been searched without a miss)
    if (!d_link_offsets) return GKC_OK;
    if (cap_unitigs < U.n_unitigs || cap_links < total)
        GKC_FAIL(c, GKC_ERR_CAPACITY, "gkc_graph_unitigs_links: %llu links between %llu unitigs, room for %llu and %llu", (unsigned long long)total, (unsigned long long)U.n_unitigs, (unsigned long long)cap_links, (unsigned long long)cap_unitigs);
    if (total && !d_links) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_links: the links are required");
    uint32_t* d_bad = (uint32_t*)(ts + n_tiles + 1); uint32_t bad = 0;
    e = hipMemsetAsync(d_bad, 0, 4, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((k_graph_tile_offsets<true, UtSlotCount>), tiles, block, 0, c->stream, UtSlotCount{cnt}, n_slots, n_tiles, (const uint64_t*)ts, d_link_offsets);
        e = hipGetLastError();
    }
    if (e == hipSuccess && total) {
        QParams P{}; q_fill_params(P, q_model_of(c), c->qidx);
        const dim3 grid(q_grid((n_slots + GR_THREADS - 1) / GR_THREADS));
        GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_unitig_link_fill<KW>), grid, block, 0, c->stream, P, n_ds, n, n_slots, d_masks, unitig, (const uint32_t*)slot_rec, (const uint64_t*)d_link_offsets, d_links, d_bad));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t ef = hipStreamSynchronize(c->stream);
    GKC_HIP(c, e); GKC_HIP(c, ef);
    if (bad) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_links: d_masks name a neighbour that is no record of these results (the masks of other results?); the buffers hold no links");
    U.n_links = total; U.links_counted = true;
    return GKC_OK;
}

extern "C" {

int gkc_graph_unitigs_links(gkc_ctx* c, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs, uint64_t* d_links, uint64_t cap_links, uint64_t* n_links)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_links) *n_links = 0;
    GKC_TRY(ut_require_placement(c, "gkc_graph_unitigs_links"));
    return ut_links(c, d_masks, d_link_offsets, cap_unitigs, d_links, cap_links, n_links, nullptr);
}

}  // extern "C"
