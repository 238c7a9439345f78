// gkc_graph.hip — exact de Bruijn neighbourhoods of the solid k-mers (include/gkc.h, "graph neighbourhoods").
//
// The reference finds the neighbours of a node through a Bloom filter and removes the filter's false positives afterwards (BloomAlgorithm, DebloomMinimizerAlgorithm:
// contains8 of every solid k-mer; BranchingAlgorithm then takes graph.successors / predecessors of every node and keeps the nodes that are not simple). Here the counted
// results lie in HBM as ascending Count[] per dataset and any canonical k-mer can be looked up in them exactly (gkc_query.hpp: minimizer -> dataset -> sampled index ->
// window), so the neighbourhood of a solid k-mer is eight lookups and nothing has to be filtered.
//
//   k_graph_masks    : one thread per solid record of the whole result state (flat index in dataset order -> dataset by its QDs::base). The eight neighbours
//                      (GrNode in gkc_graph.hpp, shared with the unitig, link and simplify kernels) are
//                      made from the record's value x and ONE reverse complement rx: a right extension is ((x << 2) | j) & mask with reverse complement
//                      (rx >> 2) | (comp(j) << 2(k-1)), a left extension the mirror image. A neighbour shares k-1 bases with x, so its minimizer is the minimum over the
//                      k-m m-mers it shares with x and its one new m-mer: the order keys of x's m-mers are computed once (k-m+1 evaluations), the running minimum without
//                      the first / without the last m-mer kept, and each neighbour adds one evaluation (the order key does not depend on the strand: q_mmer_key takes
//                      the canonical m-mer, the frequency table is built over canonical m-mers). GR_LOCKSTEP searches advance together like in k_q_reads.
//   k_graph_topology : from the masks, in = popcount(mask >> 4), out = popcount(mask & 15). <false>: per tile of GR_TILE records the number of branching ones
//                      (!(in == 1 && out == 1)) and the 5 x 5 table topology[in * 5 + out] (LDS table per workgroup, the dominant (1, 1) cell in a register, flushed once);
//   k_graph_scan_tiles: exclusive prefix of the tile sums by one workgroup (the scheme of the flag scan in gkc_banks.hip), in place; behind gr_scan_tiles it serves every
//                      scan of tile sums of the graph kernels (unitig numbering: two arrays in one launch; unitig links; read paths);
//   k_graph_topology<true>: the branching records compacted in flat order (= dataset order, ascending inside a dataset) as Count records.
// Element indices are 64-bit; grids are capped and the kernels stride.
#include "gkc_graph.hpp"

// ------------------------------------------------------------------------------------------------ masks
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_graph_masks(QParams P, uint32_t n_ds, uint64_t g0, uint64_t n, uint8_t* __restrict__ out)
{
    typedef typename KeyT<KW>::type key_t;
    GrNode<KW> N(P);
    for (uint64_t i = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GR_THREADS) {
        N.load(P, n_ds, g0 + i);
        uint32_t res = 0;
#pragma unroll 1
        for (uint32_t e0 = 0; e0 < 8; e0 += GR_LOCKSTEP) {
            bool act[GR_LOCKSTEP], found[GR_LOCKSTEP]; uint32_t d[GR_LOCKSTEP]; key_t key[GR_LOCKSTEP]; uint64_t pos[GR_LOCKSTEP], base[GR_LOCKSTEP];
            const uint8_t* recs[GR_LOCKSTEP];
#pragma unroll
            for (int u = 0; u < GR_LOCKSTEP; u++) {
                key_t fw, rv;
                N.neighbour(P, e0 + (uint32_t)u, fw, rv, d[u]);
                key[u] = fw < rv ? fw : rv;                    // Model.hpp:294
                act[u] = true;
            }
            q_search<key_t, GrNode<KW>::RB, GR_LOCKSTEP>(P, act, d, key, found, pos, recs, base);
#pragma unroll
            for (int u = 0; u < GR_LOCKSTEP; u++) res |= (uint32_t)found[u] << (e0 + (uint32_t)u);
        }
        out[i] = (uint8_t)res;
    }
}

// ------------------------------------------------------------------------------------------------ topology, branching nodes
template <int KW, bool GATHER>
__global__ __launch_bounds__(GR_THREADS) void k_graph_topology(const uint8_t* __restrict__ masks, uint64_t n, uint32_t n_tiles, uint64_t* __restrict__ offs /* <false>: the tile sums out */,
                                                                unsigned long long* __restrict__ topo, const QDs* __restrict__ ds, uint32_t n_ds, uint8_t* __restrict__ records, uint64_t cap)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    __shared__ uint32_t s_w[GR_THREADS / 64];
    __shared__ unsigned long long s_topo[25];
    if (!GATHER) { if (threadIdx.x < 25) s_topo[threadIdx.x] = 0; __syncthreads(); }
    unsigned long long n11 = 0;                                // nodes with one predecessor and one successor: nearly all of them
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint32_t n_valid;
        const uint32_t w = gr_load4_masks(masks, n, i, &n_valid);
        uint32_t flag[GR_PER_THREAD], s = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) {
            const uint32_t mk = (w >> (8 * r)) & 255u, in = (uint32_t)__popc(mk >> 4), ou = (uint32_t)__popc(mk & 15u);
            const bool valid = r < n_valid, simple = in == 1 && ou == 1;
            flag[r] = valid && !simple; s += flag[r];
            if (!GATHER && valid) { if (simple) n11++; else atomicAdd(&s_topo[in * 5 + ou], 1ull); }
        }
        uint32_t tot;
        const uint32_t ex = gr_block_excl(s, s_w, &tot);
        if (!GATHER) { if (threadIdx.x == 0) offs[t] = tot; }
        else {
            uint64_t p = offs[t] + ex;
#pragma unroll
            for (uint32_t r = 0; r < GR_PER_THREAD; r++) {
                if (!flag[r]) continue;
                if (p < cap) {
                    const uint64_t g = i + r;
                    const QDs D = ds[gr_dataset_of(ds, n_ds, g)];
                    const uint8_t* src = D.recs + (g - D.base) * (uint64_t)RB;
                    const key_t x = q_load_key<key_t>(src);
                    const unsigned long long ab = (unsigned long long)*reinterpret_cast<const uint32_t*>(src + sizeof(key_t));
                    uint8_t* dst = records + p * (uint64_t)RB;
                    if constexpr (KW == 1) store16(dst, (unsigned long long)x, ab);
                    else { store16(dst, (unsigned long long)x, (unsigned long long)(x >> 64)); store16(dst + 16, ab, 0ull); }
                }
                p++;
            }
        }
    }
    if (!GATHER) {
#pragma unroll
        for (int dlt = 32; dlt >= 1; dlt >>= 1) n11 += __shfl_xor(n11, dlt, 64);
        if ((threadIdx.x & 63) == 0 && n11) atomicAdd(&s_topo[1 * 5 + 1], n11);
        __syncthreads();
        if (threadIdx.x < 25 && s_topo[threadIdx.x]) atomicAdd(&topo[threadIdx.x], s_topo[threadIdx.x]);
    }
}
// one workgroup: the exclusive prefix of the tile sums a[0, n_tiles) in place, a[n_tiles] = everything, GR_THREADS sums at a time; then the same for b unless it is NULL
__global__ __launch_bounds__(GR_THREADS) void k_graph_scan_tiles(uint64_t* __restrict__ a, uint64_t* __restrict__ b, uint32_t n_tiles)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    for (uint64_t* sums = a; sums; sums = sums == a ? b : nullptr) {
        uint64_t carry = 0;
        for (uint32_t base = 0; base < n_tiles; base += GR_THREADS) {
            const uint32_t t = base + threadIdx.x;
            const uint64_t v = t < n_tiles ? sums[t] : 0ull;
            uint64_t tot;
            const uint64_t ex = gr_block_excl<uint64_t>(v, s_w, &tot);
            if (t < n_tiles) sums[t] = carry + ex;
            carry += tot;
            if (n_tiles - base <= GR_THREADS) break;           // (base + GR_THREADS may wrap at the top of the 32-bit range)
        }
        if (threadIdx.x == 0) sums[n_tiles] = carry;
    }
}

// ------------------------------------------------------------------------------------------------ host side
uint64_t gr_total(const gkc_ctx* c) { uint64_t t = 0; for (const Dataset& D : c->datasets) t += D.n_solid; return t; }
void gr_scan_tiles(gkc_ctx* c, uint64_t* a, uint64_t* b, uint32_t n_tiles) { hipLaunchKernelGGL(k_graph_scan_tiles, dim3(1), dim3(GR_THREADS), 0, c->stream, a, b, n_tiles); }

// masks of the records [g0, g0 + n) of the flat order into d_masks[0, n); q_prepare has run
int gr_masks_run(gkc_ctx* c, uint64_t g0, uint64_t n, uint8_t* d_masks)
{
    ScopedTimer tm(c, "graph_neighbors");
    QParams P{}; q_fill_params(P, q_model_of(c), c->qidx);
    const uint32_t n_ds = (uint32_t)c->datasets.size();
    const dim3 grid(q_grid((n + GR_THREADS - 1) / GR_THREADS)), block(GR_THREADS);
    GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_graph_masks<KW>), grid, block, 0, c->stream, P, n_ds, g0, n, d_masks));
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}

extern "C" {

int gkc_graph_neighbors_solid(gkc_ctx* c, uint8_t* d_masks, uint64_t* n_solid)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_solid) *n_solid = 0;
    GKC_TRY(q_prepare(c, "gkc_graph_neighbors_solid"));
    const uint64_t total = gr_total(c);
    if (n_solid) *n_solid = total;
    if (!total || !d_masks) return GKC_OK;
    return gr_masks_run(c, 0, total, d_masks);
}

int gkc_graph_neighbors_partition(gkc_ctx* c, uint32_t pass, uint32_t part, uint8_t* d_masks, uint64_t* n_solid)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_solid) *n_solid = 0;
    GKC_TRY(q_prepare(c, "gkc_graph_neighbors_partition"));
    if (pass >= c->nb_passes || part >= c->nb_partitions) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_neighbors_partition: pass %u / partition %u out of range (%u passes, %u partitions)", pass, part, c->nb_passes, c->nb_partitions);
    const size_t d = (size_t)part + (size_t)pass * c->nb_partitions;
    uint64_t g0 = 0; for (size_t j = 0; j < d; j++) g0 += c->datasets[j].n_solid;
    const uint64_t n = c->datasets[d].n_solid;
    if (n_solid) *n_solid = n;
    if (!n || !d_masks) return GKC_OK;
    return gr_masks_run(c, g0, n, d_masks);
}

int gkc_graph_branching_solid(gkc_ctx* c, const uint8_t* d_masks, void* d_records, uint64_t cap_records, uint64_t* n_branching, uint64_t* topology)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_branching) *n_branching = 0;
    if (topology) memset(topology, 0, 25 * sizeof(uint64_t));
    GKC_TRY(q_prepare(c, "gkc_graph_branching_solid"));
    const uint64_t total = gr_total(c);
    if (!total) return GKC_OK;
    const uint64_t n_tiles64 = (total + GR_TILE - 1) / GR_TILE;
    if (n_tiles64 >= (1ull << 32)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_branching_solid: more than 2^32 tiles of %d k-mers", GR_TILE);
    const uint32_t n_tiles = (uint32_t)n_tiles64, n_ds = (uint32_t)c->datasets.size();
    DevBuf tmp, d_offs, d_topo;
    if (!d_masks) { GKC_TRY(c->ensure(tmp, (size_t)total)); GKC_TRY(gr_masks_run(c, 0, total, (uint8_t*)tmp.p)); d_masks = (const uint8_t*)tmp.p; }
    GKC_TRY(c->ensure(d_offs, ((size_t)n_tiles + 1) * 8)); GKC_TRY(c->ensure(d_topo, 25 * 8));
    uint64_t n_br = 0, topo[25];
    {
        ScopedTimer tm(c, "graph_branching");
        const QDs* ds = (const QDs*)c->qidx.table.p;
        const dim3 grid(q_grid(n_tiles)), block(GR_THREADS);
        uint64_t* offs = (uint64_t*)d_offs.p;                  // the tile sums, then their exclusive prefix
        GKC_HIP(c, hipMemsetAsync(d_topo.p, 0, 25 * 8, c->stream));
        GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_graph_topology<KW, false>), grid, block, 0, c->stream, d_masks, total, n_tiles, offs, (unsigned long long*)d_topo.p, ds, n_ds, (uint8_t*)nullptr, (uint64_t)0));
        gr_scan_tiles(c, offs, nullptr, n_tiles);
        if (d_records && cap_records)
            GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_graph_topology<KW, true>), grid, block, 0, c->stream, d_masks, total, n_tiles, offs, (unsigned long long*)nullptr, ds, n_ds, (uint8_t*)d_records, cap_records));
        GKC_HIP(c, hipGetLastError());
        GKC_HIP(c, hipMemcpyAsync(&n_br, (const uint64_t*)d_offs.p + n_tiles, 8, hipMemcpyDeviceToHost, c->stream));
        GKC_HIP(c, hipMemcpyAsync(topo, d_topo.p, 25 * 8, hipMemcpyDeviceToHost, c->stream));
        GKC_HIP(c, hipStreamSynchronize(c->stream));           // the scratch goes back to the pool
    }
    if (n_branching) *n_branching = n_br;
    if (topology) memcpy(topology, topo, sizeof topo);
    if (d_records && n_br > cap_records) GKC_FAIL(c, GKC_ERR_CAPACITY, "gkc_graph_branching_solid: %llu branching nodes, room for %llu records", (unsigned long long)n_br, (unsigned long long)cap_records);
    return GKC_OK;
}

}  // extern "C"
