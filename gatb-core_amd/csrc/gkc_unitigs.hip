// gkc_unitigs.hip — unitigs of the solid k-mers: the maximal non-branching paths of the de Bruijn graph glued into sequences (include/gkc.h, "unitigs").
//
// The reference compacts the graph on the host from the result file (bcalm2 inside GraphUnitigs). Here everything the compaction needs lies in HBM: the ascending
// Count[] of every dataset, the sampled index, the exact neighbour masks of gkc_graph.hip, and a search that returns a neighbour's record index (QDs::base + position).
// A record has two ends (0: right, mask bits 0-3; 1: left, bits 4-7); a state 2 i + s is "at record i, about to leave it through end s".
//
//   k_unitig_links     : one thread per record. For each end whose nibble has exactly one bit the one neighbour is built (GrNode of gkc_graph.hpp: the masks kernel's
//                        neighbours and minimizers), both ends searched in lock step, masks[j] of the record found read, the link rule applied:
//                        link[2 i + s] = 2 j + a (a: the end of j one arrives at) or NONE.
//   k_unitig_rank_*    : list ranking over the 2 n states by pointer jumping (Wyllie). The successor of a state is (j, 1 - a): in through end a, out through the other.
//                        A state carries (next, hops, node): node = the last record reached once the walk has ended (next == NONE), until then the smallest record
//                        index of the stretch jumped over. Double-buffered, one launch per round, a device flag "some state still walks" read back per round; after
//                        ceil(log2(2 n)) + 1 rounds whoever still walks is on a cycle and knows its cycle's smallest record.
//   k_unitig_cut       : that record (one thread per record) removes both halves of its left link; the ranking then runs again. Only when there are cycles.
//   k_unitig_place     : per record the last records T0 / T1 reached going right / left. The unitig starts at min(T0, T1); the record stands forward if and only if
//                        going left reaches the start, and its position is that number of hops. Start records count their unitig and its length per tile of GR_TILE;
//   gr_scan_tiles      : exclusive prefix of both tile sums by one workgroup, one launch (gkc_graph.hip);
//   k_unitig_number    : the start records get their unitig's index and the number of records in front of it; k_unitig_assign hands the index to every record.
//   k_unitig_emit      : the record at position 0 writes its k bases, every other record its last base in path orientation at offset + pos + k - 1; the abundances are
//                        summed per unitig with 64-bit vector atomics.
// State ids are 32-bit (n_solid < 2^31), element indices 64-bit; grids are capped and the kernels stride. Scratch comes from the context's pool on c->stream and is
// synchronised before it goes back.
// The edges of the compacted graph (gkc_graph_unitigs_links, the L: fields of bcalm2) are in gkc_unitig_links.hip: count, scan, fill over the placement kept by the build;
// the tip removal (gkc_graph_tips_remove: rounds of build over an alive array, links, flags, kill, mask refresh) and the bulges and erroneous connections that share its
// round (gkc_graph_simplify) in gkc_simplify.hip.
#include "gkc_unitigs.hpp"

constexpr uint32_t UT_NONE = 0xFFFFFFFFu;
constexpr uint32_t UT_REV = 0x80000000u;                      // k_unitig_place -> k_unitig_assign: the record stands reverse-complemented (beside its start record's index)

// ------------------------------------------------------------------------------------------------ links
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_unitig_links(QParams P, uint32_t n_ds, uint64_t n, const uint8_t* __restrict__ masks, uint32_t* __restrict__ link)
{
    typedef typename KeyT<KW>::type key_t;
    GrNode<KW> N(P);
    for (uint64_t i = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t mk = masks[i];
        bool act[2]; uint32_t nt[2], out[2] = {UT_NONE, UT_NONE};
#pragma unroll
        for (int s = 0; s < 2; s++) { const uint32_t nib = (mk >> (4 * s)) & 15u; act[s] = __popc(nib) == 1; nt[s] = nib ? (uint32_t)__ffs(nib) - 1u : 0u; }
        if (act[0] || act[1]) {
            N.load(P, n_ds, i);
            const bool pal = N.x == N.rx;                      // (even k only) a palindrome is a unitig of its own, and nothing links to one
            bool found[2]; uint32_t d[2], a[2]; key_t key[2]; uint64_t pos[2], base[2]; const uint8_t* recs[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                key_t fw, rv;
                N.neighbour(P, 4u * s + nt[s], fw, rv, d[s]);
                key[s] = fw < rv ? fw : rv;
                a[s] = gr_arrival((uint32_t)s, fw, rv);
                act[s] = act[s] && !pal && fw != rv;
            }
            q_search<key_t, GrNode<KW>::RB, 2>(P, act, d, key, found, pos, recs, base);
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const uint64_t j = base[s] + pos[s];
                if (!(act[s] && found[s]) || j == i || j >= n) continue;      // (found: always, with the masks of these results)
                if (__popc(((uint32_t)masks[j] >> (4u * a[s])) & 15u) == 1) out[s] = 2u * (uint32_t)j + a[s];
            }
        }
        reinterpret_cast<uint2*>(link)[i] = make_uint2(out[0], out[1]);
    }
}

// ------------------------------------------------------------------------------------------------ ranking
// state: x = next state or NONE, y = hops so far, z = the last record (x == NONE) / the smallest record of the stretch jumped over (else)
__global__ __launch_bounds__(256) void k_unitig_rank_init(const uint32_t* __restrict__ link, uint64_t n2, uint4* __restrict__ st)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = link[t];
        st[t] = l == UT_NONE ? make_uint4(UT_NONE, 0u, (uint32_t)(t >> 1), 0u) : make_uint4(l ^ 1u, 1u, (uint32_t)(t >> 1), 0u);
    }
}
__global__ __launch_bounds__(256) void k_unitig_rank_round(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t n2, uint32_t* __restrict__ walking)
{
    bool any = false;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += (uint64_t)gridDim.x * blockDim.x) {
        uint4 a = in[t];
        if (a.x != UT_NONE) {
            const uint4 b = in[a.x];
            a.y += b.y;
            if (b.x == UT_NONE) a.z = b.z; else { a.z = b.z < a.z ? b.z : a.z; any = true; }
            a.x = b.x;
        }
        out[t] = a;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *walking = 1u;
}
// after the last round: a record whose left-going state still walks and has seen no smaller record than itself is the smallest of its cycle
__global__ __launch_bounds__(256) void k_unitig_cut(const uint4* __restrict__ st, uint64_t n, uint32_t* __restrict__ link, unsigned long long* __restrict__ n_cycles)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 s = st[2 * i + 1];
        if (s.x == UT_NONE || s.z != (uint32_t)i) continue;
        const uint32_t l = link[2 * i + 1];                    // (no other thread reads or writes these two entries: their records are not the smallest of the cycle)
        link[l] = UT_NONE; link[2 * i + 1] = UT_NONE;
        atomicAdd(n_cycles, 1ull);
    }
}

// ------------------------------------------------------------------------------------------------ placement, numbering
__global__ __launch_bounds__(GR_THREADS) void k_unitig_place(const uint4* __restrict__ st, uint64_t n, uint32_t n_tiles, uint32_t* __restrict__ start_of, uint32_t* __restrict__ pos,
                                                              uint32_t* __restrict__ len, uint64_t* __restrict__ tile_cnt, uint64_t* __restrict__ tile_len,
                                                              const uint8_t* __restrict__ alive)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint64_t cnt = 0, sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) {
            const uint64_t i = i0 + r;
            if (i >= n) break;
            if (alive && !alive[i]) { start_of[i] = UT_NONE; pos[i] = 0u; len[i] = 0u; continue; }      // a dead record: of no unitig (start | UT_REV never is UT_NONE: n < 2^31)
            const uint4 a = st[2 * i], b = st[2 * i + 1];      // going right, going left
            const uint32_t start = a.z < b.z ? a.z : b.z;
            const bool fwd = b.z == start;                     // (a single record: both walks end where they begin, it stands forward)
            start_of[i] = start | (fwd ? 0u : UT_REV);
            pos[i] = fwd ? b.y : a.y;
            const uint32_t L = start == (uint32_t)i ? a.y + b.y + 1u : 0u;
            len[i] = L;
            cnt += L != 0; sum += L;
        }
        uint64_t tot;
        gr_block_excl<uint64_t>(cnt, s_w, &tot);
        if (threadIdx.x == 0) tile_cnt[t] = tot;
        gr_block_excl<uint64_t>(sum, s_w, &tot);
        if (threadIdx.x == 0) tile_len[t] = tot;
    }
}
__global__ __launch_bounds__(GR_THREADS) void k_unitig_number(const uint32_t* __restrict__ len, uint64_t n, uint32_t n_tiles, const uint64_t* __restrict__ offs_cnt,
                                                               const uint64_t* __restrict__ offs_len, uint32_t* __restrict__ index_at, uint64_t* __restrict__ first)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint32_t L[GR_PER_THREAD]; uint64_t cnt = 0, sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) { L[r] = i0 + r < n ? len[i0 + r] : 0u; cnt += L[r] != 0; sum += L[r]; }
        uint64_t tot;
        uint64_t u = offs_cnt[t] + gr_block_excl<uint64_t>(cnt, s_w, &tot);
        uint64_t f = offs_len[t] + gr_block_excl<uint64_t>(sum, s_w, &tot);
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) {
            if (!L[r]) continue;
            index_at[i0 + r] = (uint32_t)u; first[u] = f;
            u++; f += L[r];
        }
    }
}
__global__ __launch_bounds__(256) void k_unitig_assign(const uint32_t* __restrict__ start_of, const uint32_t* __restrict__ index_at, uint64_t n, uint64_t* __restrict__ unitig)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = start_of[i];
        unitig[i] = s == UT_NONE ? ~0ull : ((uint64_t)index_at[s & ~UT_REV] << 1) | (s >> 31);      // (UT_NONE: a dead record, k_unitig_place)
    }
}

// ------------------------------------------------------------------------------------------------ sequences
__device__ __forceinline__ char ut_letter(uint32_t code) { return (char)((0x47544341u >> (8u * code)) & 255u); }      // A, C, T, G = 0..3
template <int KW>
__global__ __launch_bounds__(256) void k_unitig_emit(const QDs* __restrict__ ds, uint32_t n_ds, uint32_t k, uint64_t n, const uint64_t* __restrict__ unitig, const uint32_t* __restrict__ pos,
                                                      const uint64_t* __restrict__ first, uint64_t n_unitigs, uint64_t n_bases, char* __restrict__ bases, uint64_t* __restrict__ offsets,
                                                      unsigned long long* __restrict__ kc)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    const uint32_t top = 2u * (k - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_unitigs] = n_bases;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t U = unitig[i], u = U >> 1;
        if (U == ~0ull) continue;                              // a dead record of a placement over an alive array
        const QDs D = ds[gr_dataset_of(ds, n_ds, i)];
        const uint8_t* src = D.recs + (i - D.base) * (uint64_t)RB;
        const key_t x = q_load_key<key_t>(src);
        const bool rev = U & 1;
        const uint32_t p = pos[i];
        const uint64_t off = first[u] + u * (uint64_t)(k - 1);
        if (p == 0) {
            const key_t seq = rev ? KeyT<KW>::revcomp(x, k) : x;
            for (uint32_t t = 0; t < k; t++) bases[off + t] = ut_letter((uint32_t)(seq >> (2u * (k - 1 - t))) & 3u);
            offsets[u] = off;
        } else bases[off + p + (k - 1)] = ut_letter(rev ? (((uint32_t)(x >> top) & 3u) ^ 2u) : ((uint32_t)x & 3u));      // the last base of the record as it stands in the path
        if (kc) atomicAdd(&kc[u], (unsigned long long)*reinterpret_cast<const uint32_t*>(src + sizeof(key_t)));
    }
}

// ------------------------------------------------------------------------------------------------ host side
static std::vector<std::pair<const void*, uint64_t>> ut_signature(const gkc_ctx* c)
{
    std::vector<std::pair<const void*, uint64_t>> sig(c->datasets.size());
    for (size_t d = 0; d < sig.size(); d++) sig[d] = {c->datasets[d].d_counts, c->datasets[d].n_solid};
    return sig;
}
// the guards of the queries, then: the placement describes the results the context holds now (also gkc_paths.hip)
int ut_require_placement(gkc_ctx* c, const char* who)
{
    GKC_TRY(q_prepare(c, who));
    UnitigPlacement& U = c->unitigs;
    if (!U.valid) GKC_FAIL(c, GKC_ERR_ARG, "%s: gkc_graph_unitigs_build must be called first", who);
    if (U.epoch != c->pass_epoch || U.sig != ut_signature(c)) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the results have changed since gkc_graph_unitigs_build (build again)", who); }
    return GKC_OK;
}

// pointer jumping over the 2 n states from the links; the finished states in *result (st_a or st_b). *walking: some state never reached an end (it lies on a cycle)
static int ut_rank(gkc_ctx* c, const uint32_t* link, uint64_t n, uint4* st_a, uint4* st_b, uint32_t* d_flag, uint4** result, bool* walking, uint32_t* rounds)
{
    const uint64_t n2 = 2 * n;
    const dim3 grid(q_grid((n2 + 255) / 256)), block(256);
    uint32_t max_rounds = 1; while ((1ull << max_rounds) < n2) max_rounds++;      // ceil(log2(2 n)) ...
    max_rounds += 1;
    hipLaunchKernelGGL(k_unitig_rank_init, grid, block, 0, c->stream, link, n2, st_a);
    uint4 *in = st_a, *out = st_b;
    uint32_t flag = 1;
    for (uint32_t r = 0; r < max_rounds && flag; r++) {
        GKC_HIP(c, hipMemsetAsync(d_flag, 0, 4, c->stream));
        hipLaunchKernelGGL(k_unitig_rank_round, grid, block, 0, c->stream, (const uint4*)in, out, n2, d_flag);
        GKC_HIP(c, hipGetLastError());
        GKC_HIP(c, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
        GKC_HIP(c, hipStreamSynchronize(c->stream));
        std::swap(in, out);
        (*rounds)++;
    }
    *result = in; *walking = flag != 0;
    return GKC_OK;
}

// how many records of alive[0, n) are alive: one atomic per wave. With masks, *bad when a dead record has a mask (not a state a call left)
__global__ __launch_bounds__(256) void k_alive_count(const uint8_t* __restrict__ alive, const uint8_t* __restrict__ masks, uint64_t n, unsigned long long* __restrict__ count,
                                                      uint32_t* __restrict__ bad)
{
    uint64_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const bool a = alive[i] != 0;
        mine += a;
        if (masks && !a && masks[i]) *bad = 1u;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
}
int ut_alive_count(gkc_ctx* c, void* d_cnt16, const uint8_t* d_alive, const uint8_t* d_masks, uint64_t n, uint64_t* n_alive, bool* bad)
{
    uint64_t h[2] = {0, 0};
    hipError_t e = hipMemsetAsync(d_cnt16, 0, 16, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_alive_count, dim3(q_grid((n + 255) / 256)), dim3(256), 0, c->stream, d_alive, d_masks, n, (unsigned long long*)d_cnt16, (uint32_t*)((uint64_t*)d_cnt16 + 1)); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_cnt16, 16, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);     // (also after a failure: the scratch goes back to the pool)
    GKC_HIP(c, e); GKC_HIP(c, es);
    *n_alive = h[0]; *bad = h[1] != 0;
    return GKC_OK;
}

// (gkc_unitigs.hpp) a dead record has mask 0 and no mask names it, so it has no link and the ranking leaves it alone; k_unitig_place gives it no unitig
int ut_build(gkc_ctx* c, const char* who, const uint8_t* d_masks, const uint8_t* d_alive, uint64_t n_alive, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    UnitigPlacement& U = c->unitigs;
    U.drop(); U.n = U.n_alive = U.n_unitigs = U.n_bases = U.n_cycles = 0; U.subset = d_alive != nullptr;
    const uint64_t n = gr_total(c);
    if (n >= (1ull << 31)) GKC_FAIL(c, GKC_ERR_CAPACITY, "%s: %llu solid k-mers, the states of the ranking are 32-bit (fewer than 2^31 records)", who, (unsigned long long)n);
    if (!d_alive) n_alive = n;
    if (n && !n_alive) {                                       // every record dead: no unitig; the placement says so per record
        GKC_TRY(c->ensure(U.unitig, (size_t)n * 8)); GKC_TRY(c->ensure(U.pos, (size_t)n * 4));
        GKC_HIP(c, hipMemsetAsync(U.unitig.p, 0xFF, (size_t)n * 8, c->stream)); GKC_HIP(c, hipMemsetAsync(U.pos.p, 0, (size_t)n * 4, c->stream));
        GKC_HIP(c, hipStreamSynchronize(c->stream));
        U.n = n;
    } else if (n) {
        const uint32_t n_tiles = (uint32_t)((n + GR_TILE - 1) / GR_TILE), n_ds = (uint32_t)c->datasets.size();
        DevBuf tmp, d_link, d_st_a, d_st_b, d_small, d_start, d_len, d_index, d_tc, d_tl;
        if (!d_masks) { GKC_TRY(c->ensure(tmp, (size_t)n)); GKC_TRY(gr_masks_run(c, 0, n, (uint8_t*)tmp.p)); d_masks = (const uint8_t*)tmp.p; }
        GKC_TRY(c->ensure(d_link, (size_t)n * 8)); GKC_TRY(c->ensure(d_st_a, (size_t)n * 32)); GKC_TRY(c->ensure(d_st_b, (size_t)n * 32)); GKC_TRY(c->ensure(d_small, 16));
        GKC_TRY(c->ensure(d_start, (size_t)n * 4)); GKC_TRY(c->ensure(d_len, (size_t)n * 4)); GKC_TRY(c->ensure(d_index, (size_t)n * 4));
        GKC_TRY(c->ensure(d_tc, ((size_t)n_tiles + 1) * 8)); GKC_TRY(c->ensure(d_tl, ((size_t)n_tiles + 1) * 8));
        GKC_TRY(c->ensure(U.unitig, (size_t)n * 8)); GKC_TRY(c->ensure(U.pos, (size_t)n * 4));
        uint32_t* link = (uint32_t*)d_link.p;
        uint32_t* d_flag = (uint32_t*)d_small.p; unsigned long long* d_cycles = (unsigned long long*)d_small.p + 1;
        {
            ScopedTimer tm(c, "graph_links");
            QParams P{}; q_fill_params(P, q_model_of(c), c->qidx);
            const dim3 grid(q_grid((n + GR_THREADS - 1) / GR_THREADS)), block(GR_THREADS);
            GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_unitig_links<KW>), grid, block, 0, c->stream, P, n_ds, n, d_masks, link));
            GKC_HIP(c, hipGetLastError());
        }
        uint64_t totals[2] = {0, 0}, cycles = 0; uint32_t rounds = 0;
        int rc = GKC_OK;
        {
            ScopedTimer tm(c, "graph_rank");
            uint4* st = nullptr; bool walking = false;
            rc = ut_rank(c, link, n, (uint4*)d_st_a.p, (uint4*)d_st_b.p, d_flag, &st, &walking, &rounds);
            if (rc == GKC_OK && walking) {                     // cycles: cut each at the left end of its smallest record, rank again
                const dim3 grid(q_grid((n + 255) / 256)), block(256);
                GKC_HIP(c, hipMemsetAsync(d_cycles, 0, 8, c->stream));
                hipLaunchKernelGGL(k_unitig_cut, grid, block, 0, c->stream, (const uint4*)st, n, link, d_cycles);
                GKC_HIP(c, hipGetLastError());
                GKC_HIP(c, hipMemcpyAsync(&cycles, d_cycles, 8, hipMemcpyDeviceToHost, c->stream));
                rc = ut_rank(c, link, n, (uint4*)d_st_a.p, (uint4*)d_st_b.p, d_flag, &st, &walking, &rounds);
                if (rc == GKC_OK && walking) { c->set_error(GKC_ERR_HIP, "%s: the ranking did not end after the cycles were cut", who); rc = GKC_ERR_HIP; }
            }
            if (rc == GKC_OK) {
                const dim3 tiles(q_grid(n_tiles)), block(GR_THREADS);
                hipLaunchKernelGGL(k_unitig_place, tiles, block, 0, c->stream, (const uint4*)st, n, n_tiles, (uint32_t*)d_start.p, (uint32_t*)U.pos.p, (uint32_t*)d_len.p, (uint64_t*)d_tc.p, (uint64_t*)d_tl.p, d_alive);
                gr_scan_tiles(c, (uint64_t*)d_tc.p, (uint64_t*)d_tl.p, n_tiles);
                GKC_HIP(c, hipGetLastError());
                GKC_HIP(c, hipMemcpyAsync(&totals[0], (const uint64_t*)d_tc.p + n_tiles, 8, hipMemcpyDeviceToHost, c->stream));
                GKC_HIP(c, hipMemcpyAsync(&totals[1], (const uint64_t*)d_tl.p + n_tiles, 8, hipMemcpyDeviceToHost, c->stream));
                GKC_HIP(c, hipStreamSynchronize(c->stream));
                if (totals[0] == 0 || totals[0] > n_alive || totals[1] != n_alive) { c->set_error(GKC_ERR_HIP, "%s: %llu unitigs of %llu records over %llu solid k-mers", who, (unsigned long long)totals[0], (unsigned long long)totals[1], (unsigned long long)n_alive); rc = GKC_ERR_HIP; }
            }
            if (rc == GKC_OK) {
                rc = c->ensure(U.first, (size_t)totals[0] * 8);
                if (rc == GKC_OK) {
                    const dim3 tiles(q_grid(n_tiles)), block(GR_THREADS);
                    hipLaunchKernelGGL(k_unitig_number, tiles, block, 0, c->stream, (const uint32_t*)d_len.p, n, n_tiles, (const uint64_t*)d_tc.p, (const uint64_t*)d_tl.p, (uint32_t*)d_index.p, (uint64_t*)U.first.p);
                    hipLaunchKernelGGL(k_unitig_assign, dim3(q_grid((n + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t*)d_start.p, (const uint32_t*)d_index.p, n, (uint64_t*)U.unitig.p);
                    GKC_HIP(c, hipGetLastError());
                }
            }
            (void)hipStreamSynchronize(c->stream);             // the scratch goes back to the pool
            tm.counts = rounds;                                // "graph_rank" counts the rounds of pointer jumping
        }
        if (rc != GKC_OK) { U.drop(); return rc; }
        U.n = n; U.n_alive = n_alive; U.n_unitigs = totals[0]; U.n_bases = n_alive + totals[0] * (uint64_t)(c->k - 1); U.n_cycles = cycles;
    }
    U.epoch = c->pass_epoch; U.sig = ut_signature(c); U.valid = true;
    if (n_unitigs) *n_unitigs = U.n_unitigs;
    if (n_bases) *n_bases = U.n_bases;
    if (n_cycles) *n_cycles = U.n_cycles;
    return GKC_OK;
}

extern "C" {

int gkc_graph_unitigs_build(gkc_ctx* c, const uint8_t* d_masks, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (n_cycles) *n_cycles = 0;
    GKC_TRY(q_prepare(c, "gkc_graph_unitigs_build"));
    return ut_build(c, "gkc_graph_unitigs_build", d_masks, nullptr, 0, n_unitigs, n_bases, n_cycles);
}

int gkc_graph_unitigs_build_alive(gkc_ctx* c, const uint8_t* d_masks, const uint8_t* d_alive, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (n_cycles) *n_cycles = 0;
    GKC_TRY(q_prepare(c, "gkc_graph_unitigs_build_alive"));
    const uint64_t n = gr_total(c);
    if (n && (!d_masks || !d_alive)) { c->unitigs.drop(); GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_build_alive: the masks and the alive array are required"); }
    uint64_t n_alive = 0; bool bad = false;
    if (n) { DevBuf d_cnt; GKC_TRY(c->ensure(d_cnt, 16)); GKC_TRY(ut_alive_count(c, d_cnt.p, d_alive, nullptr, n, &n_alive, &bad)); }
    return ut_build(c, "gkc_graph_unitigs_build_alive", d_masks, d_alive, n_alive, n_unitigs, n_bases, n_cycles);
}

int gkc_graph_unitigs_write(gkc_ctx* c, char* d_bases, uint64_t cap_bases, uint64_t* d_offsets, uint64_t cap_unitigs, uint64_t* d_kc)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    GKC_TRY(ut_require_placement(c, "gkc_graph_unitigs_write"));
    const UnitigPlacement& U = c->unitigs;
    if (cap_bases < U.n_bases || cap_unitigs < U.n_unitigs)
        GKC_FAIL(c, GKC_ERR_CAPACITY, "gkc_graph_unitigs_write: %llu unitigs of %llu bases, room for %llu and %llu", (unsigned long long)U.n_unitigs, (unsigned long long)U.n_bases, (unsigned long long)cap_unitigs, (unsigned long long)cap_bases);
    if (!d_offsets || (U.n_bases && !d_bases)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_graph_unitigs_write: the bases and the offsets are required");
    ScopedTimer tm(c, "graph_emit");
    if (!U.n_unitigs) { GKC_HIP(c, hipMemsetAsync(d_offsets, 0, 8, c->stream)); GKC_HIP(c, hipStreamSynchronize(c->stream)); return GKC_OK; }      // (no record, or none alive)
    if (d_kc) GKC_HIP(c, hipMemsetAsync(d_kc, 0, (size_t)U.n_unitigs * 8, c->stream));
    const QDs* ds = (const QDs*)c->qidx.table.p;
    const uint32_t n_ds = (uint32_t)c->datasets.size();
    const dim3 grid(q_grid((U.n + 255) / 256)), block(256);
    GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_unitig_emit<KW>), grid, block, 0, c->stream, ds, n_ds, c->k, U.n, (const uint64_t*)U.unitig.p, (const uint32_t*)U.pos.p, (const uint64_t*)U.first.p, U.n_unitigs, U.n_bases, d_bases, d_offsets, (unsigned long long*)d_kc));
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}

int gkc_graph_unitigs_nodes(gkc_ctx* c, uint64_t* d_unitig, uint32_t* d_pos)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    GKC_TRY(ut_require_placement(c, "gkc_graph_unitigs_nodes"));
    const UnitigPlacement& U = c->unitigs;
    if (!U.n) return GKC_OK;
    if (d_unitig) GKC_HIP(c, hipMemcpyAsync(d_unitig, U.unitig.p, (size_t)U.n * 8, hipMemcpyDeviceToDevice, c->stream));
    if (d_pos) GKC_HIP(c, hipMemcpyAsync(d_pos, U.pos.p, (size_t)U.n * 4, hipMemcpyDeviceToDevice, c->stream));
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}

}  // extern "C"
