// gkc_unitigs.hip — unitigs of the solid k-mers: the maximal non-branching paths of the de Bruijn graph glued into sequences (include/gkc.h, "unitigs").
//
// The reference compacts the graph on the host from the result file (bcalm2 inside GraphUnitigs). Here everything the compaction needs lies in HBM: the ascending
// Count[] of every dataset, the sampled index, the exact neighbour masks of gkc_graph.hip, and a search that returns a neighbour's record index (QDs::base + position).
// A record has two ends (0: right, mask bits 0-3; 1: left, bits 4-7); a state 2 i + s is "at record i, about to leave it through end s".
//
//   k_unitig_links     : one thread per record. For each end whose nibble has exactly one bit the one neighbour is built (gr_shared_minima / gr_neighbour of gkc_graph.hpp: the
//                        masks kernel's neighbours and minimizers), both ends searched in lock step, masks[j] of the record found read, the link rule applied:
//                        link[2 i + s] = 2 j + a (a: the end of j one arrives at) or NONE.
//   k_unitig_rank_*    : list ranking over the 2 n states by pointer jumping (Wyllie). The successor of a state is (j, 1 - a): in through end a, out through the other.
//                        A state carries (next, hops, node): node = the last record reached once the walk has ended (next == NONE), until then the smallest record
//                        index of the stretch jumped over. Double-buffered, one launch per round, a device flag "some state still walks" read back per round; after
//                        ceil(log2(2 n)) + 1 rounds whoever still walks is on a cycle and knows its cycle's smallest record.
//   k_unitig_cut       : that record (one thread per record) removes both halves of its left link; the ranking then runs again. Only when there are cycles.
//   k_unitig_place     : per record the last records T0 / T1 reached going right / left. The unitig starts at min(T0, T1); the record stands forward if and only if
//                        going left reaches the start, and its position is that number of hops. Start records count their unitig and its length per tile of GR_TILE;
//   k_unitig_scan      : exclusive prefix of both tile sums by one workgroup (the scheme of k_graph_scan_sums);
//   k_unitig_number    : the start records get their unitig's index and the number of records in front of it; k_unitig_assign hands the index to every record.
//   k_unitig_emit      : the record at position 0 writes its k bases, every other record its last base in path orientation at offset + pos + k - 1; the abundances are
//                        summed per unitig with 64-bit vector atomics.
// State ids are 32-bit (n_solid < 2^31), element indices 64-bit; grids are capped and the kernels stride. Scratch comes from the context's pool on c->stream and is
// synchronised before it goes back.
// The edges of the compacted graph (gkc_graph_unitigs_links, the L: fields of bcalm2) follow the unitigs: count, scan, fill over the placement kept by the build; the tip
// removal (gkc_graph_tips_remove: rounds of build over an alive array, links, flags, kill, mask refresh) and the bulges and erroneous connections that share its round
// (gkc_graph_simplify) are at the end of this file.
#include "gkc_graph.hpp"

constexpr uint32_t UT_NONE = 0xFFFFFFFFu;
constexpr uint32_t UT_REV = 0x80000000u;                      // k_unitig_place -> k_unitig_assign: the record stands reverse-complemented (beside its start record's index)

// ------------------------------------------------------------------------------------------------ links
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_unitig_links(QParams P, uint32_t n_ds, uint64_t n, const uint8_t* __restrict__ masks, uint32_t* __restrict__ link)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    const uint32_t k = P.k, m = P.m;
    const key_t kmask = KeyT<KW>::mask(k);
    const uint32_t top = 2u * (k - 1);                         // bit position of a k-mer's first nucleotide
    for (uint64_t i = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t mk = masks[i];
        bool act[2]; uint32_t nt[2], out[2] = {UT_NONE, UT_NONE};
#pragma unroll
        for (int s = 0; s < 2; s++) { const uint32_t nib = (mk >> (4 * s)) & 15u; act[s] = __popc(nib) == 1; nt[s] = nib ? (uint32_t)__ffs(nib) - 1u : 0u; }
        if (act[0] || act[1]) {
            const QDs D = P.ds[gr_dataset_of(P.ds, n_ds, i)];
            const key_t x = q_load_key<key_t>(D.recs + (i - D.base) * (uint64_t)RB), rx = KeyT<KW>::revcomp(x, k);
            uint32_t min_r, min_l;
            gr_shared_minima<key_t>(P, x, min_r, min_l);
            const uint32_t suf = (uint32_t)x & (P.mmask >> 2), pre = (uint32_t)(x >> (2u * (k - m + 1)));      // the last / the first m-1 nucleotides of x
            const bool pal = x == rx;                          // (even k only) a palindrome is a unitig of its own, and nothing links to one
            bool found[2]; uint32_t d[2], a[2]; key_t key[2]; uint64_t pos[2], base[2]; const uint8_t* recs[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                key_t fw, rv;
                gr_neighbour<key_t>(P, x, rx, kmask, top, suf, pre, min_r, min_l, 4u * s + nt[s], fw, rv, d[s]);
                key[s] = fw < rv ? fw : rv;
                a[s] = fw < rv ? 1u - s : (uint32_t)s;         // leaving right one arrives at the left end of a neighbour that is canonical as it stands; leaving left, the mirror image
                act[s] = act[s] && !pal && fw != rv;
            }
            q_search<key_t, RB, 2>(P, act, d, key, found, pos, recs, base);
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
// one workgroup: the exclusive prefixes of both tile sums in place, [n_tiles] = everything
__global__ __launch_bounds__(GR_THREADS) void k_unitig_scan(uint64_t* __restrict__ tile_cnt, uint64_t* __restrict__ tile_len, uint32_t n_tiles)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    uint64_t carry_c = 0, carry_l = 0;
    for (uint32_t base = 0; base < n_tiles; base += GR_THREADS) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t vc = t < n_tiles ? tile_cnt[t] : 0ull, vl = t < n_tiles ? tile_len[t] : 0ull;
        uint64_t tc, tl;
        const uint64_t ec = gr_block_excl<uint64_t>(vc, s_w, &tc), el = gr_block_excl<uint64_t>(vl, s_w, &tl);
        if (t < n_tiles) { tile_cnt[t] = carry_c + ec; tile_len[t] = carry_l + el; }
        carry_c += tc; carry_l += tl;
        if (n_tiles - base <= GR_THREADS) break;               // (base + GR_THREADS may wrap at the top of the 32-bit range)
    }
    if (threadIdx.x == 0) { tile_cnt[n_tiles] = carry_c; tile_len[n_tiles] = carry_l; }
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

// how many records of alive[0, n) are alive: one atomic per wave
__global__ __launch_bounds__(256) void k_alive_count(const uint8_t* __restrict__ alive, uint64_t n, unsigned long long* __restrict__ count)
{
    uint64_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) mine += alive[i] != 0;
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
}

// The build behind gkc_graph_unitigs_build (d_alive == NULL: every record) and gkc_graph_unitigs_build_alive / gkc_graph_tips_remove (the records with alive[i] != 0, n_alive
// of them; d_masks consistent with it: a dead record has mask 0 and no mask names it, so it has no link and the ranking leaves it alone; k_unitig_place gives it no unitig).
// q_prepare has run.
static int ut_build(gkc_ctx* c, const char* who, const uint8_t* d_masks, const uint8_t* d_alive, uint64_t n_alive, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
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
            if (c->key_words == 1) hipLaunchKernelGGL((k_unitig_links<1>), grid, block, 0, c->stream, P, n_ds, n, d_masks, link);
            else                   hipLaunchKernelGGL((k_unitig_links<2>), grid, block, 0, c->stream, P, n_ds, n, d_masks, link);
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
                hipLaunchKernelGGL(k_unitig_scan, dim3(1), block, 0, c->stream, (uint64_t*)d_tc.p, (uint64_t*)d_tl.p, n_tiles);
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
    uint64_t n_alive = 0;
    if (n) {
        DevBuf d_cnt;
        GKC_TRY(c->ensure(d_cnt, 8));
        hipError_t e = hipMemsetAsync(d_cnt.p, 0, 8, c->stream);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_alive_count, dim3(q_grid((n + 255) / 256)), dim3(256), 0, c->stream, d_alive, n, (unsigned long long*)d_cnt.p); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipMemcpyAsync(&n_alive, d_cnt.p, 8, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);  // (also after a failure: the scratch goes back to the pool)
        GKC_HIP(c, e); GKC_HIP(c, es);
    }
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
    if (c->key_words == 1) hipLaunchKernelGGL((k_unitig_emit<1>), grid, block, 0, c->stream, ds, n_ds, c->k, U.n, (const uint64_t*)U.unitig.p, (const uint32_t*)U.pos.p, (const uint64_t*)U.first.p, U.n_unitigs, U.n_bases, d_bases, d_offsets, (unsigned long long*)d_kc);
    else                   hipLaunchKernelGGL((k_unitig_emit<2>), grid, block, 0, c->stream, ds, n_ds, c->k, U.n, (const uint64_t*)U.unitig.p, (const uint32_t*)U.pos.p, (const uint64_t*)U.first.p, U.n_unitigs, U.n_bases, d_bases, d_offsets, (unsigned long long*)d_kc);
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

// ================================================================================================ links between the unitigs (include/gkc.h, "unitigs": side, slot, entry)
//   k_unitig_link_count   : one thread per record. The record at position 0 of unitig u writes the degree of its outward end to cnt[2 u + 1], the one at position L_u - 1
//                           to cnt[2 u]; a single-record unitig writes both. Every slot is written exactly once, with its record and end beside the count.
//   k_unitig_link_tiles   : the sum of every tile of GR_TILE slots; k_unitig_link_scan: exclusive prefix of the tile sums by one workgroup (the scheme of k_unitig_scan);
//   k_unitig_link_offsets : the exclusive prefix inside the tile on top of the tile's offset -> offsets[2 n_unitigs + 1];
//   k_unitig_link_fill    : one thread per SLOT, from the record << 1 | end the count kernel left per slot, so that every lane of a wave searches (extremities are
//                           few among the records). A side builds its four neighbours (gr_shared_minima / gr_neighbour), searches them two at a
//                           time in lock step, reads the placement of the records found, forms the entries, sorts the four of the slot in registers (empty ones last)
//                           and stores the first deg of them at offsets[slot]. A neighbour the masks name that is no record (masks of other results) raises *bad.
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
    const uint64_t L = (u + 1 < n_unitigs ? first[u + 1] : n_alive) - first[u];
    if ((uint64_t)p + 1 == L) { if (rev) side_l = 0u; else side_r = 0u; }
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
__global__ __launch_bounds__(GR_THREADS) void k_unitig_link_tiles(const uint32_t* __restrict__ cnt, uint64_t n_slots, uint32_t n_tiles, uint64_t* __restrict__ tile_sum)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) sum += i0 + r < n_slots ? cnt[i0 + r] : 0u;
        uint64_t tot;
        gr_block_excl<uint64_t>(sum, s_w, &tot);
        if (threadIdx.x == 0) tile_sum[t] = tot;
    }
}
// one workgroup: the exclusive prefix of the tile sums in place, [n_tiles] = everything
__global__ __launch_bounds__(GR_THREADS) void k_unitig_link_scan(uint64_t* __restrict__ tile_sum, uint32_t n_tiles)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += GR_THREADS) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < n_tiles ? tile_sum[t] : 0ull;
        uint64_t tot;
        const uint64_t e = gr_block_excl<uint64_t>(v, s_w, &tot);
        if (t < n_tiles) tile_sum[t] = carry + e;
        carry += tot;
        if (n_tiles - base <= GR_THREADS) break;               // (base + GR_THREADS may wrap at the top of the 32-bit range)
    }
    if (threadIdx.x == 0) tile_sum[n_tiles] = carry;
}
__global__ __launch_bounds__(GR_THREADS) void k_unitig_link_offsets(const uint32_t* __restrict__ cnt, uint64_t n_slots, uint32_t n_tiles, const uint64_t* __restrict__ tile_off,
                                                                     uint64_t* __restrict__ offsets)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_slots] = tile_off[n_tiles];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint32_t v[GR_PER_THREAD]; uint64_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) { v[r] = i0 + r < n_slots ? cnt[i0 + r] : 0u; sum += v[r]; }
        uint64_t tot;
        uint64_t o = tile_off[t] + gr_block_excl<uint64_t>(sum, s_w, &tot);
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) { if (i0 + r < n_slots) offsets[i0 + r] = o; o += v[r]; }
    }
}
__device__ __forceinline__ void ut_order(uint64_t& a, uint64_t& b) { const uint64_t lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_unitig_link_fill(QParams P, uint32_t n_ds, uint64_t n, uint64_t n_slots, const uint8_t* __restrict__ masks,
                                                                  const uint64_t* __restrict__ unitig, const uint32_t* __restrict__ slot_rec,
                                                                  const uint64_t* __restrict__ offsets, uint64_t* __restrict__ links, uint32_t* __restrict__ bad)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    const uint32_t k = P.k, m = P.m;
    const key_t kmask = KeyT<KW>::mask(k);
    const uint32_t top = 2u * (k - 1);
    for (uint64_t t = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; t < n_slots; t += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t sr = slot_rec[t], s = sr & 1u;          // the record whose end s is this side
        const uint64_t i = sr >> 1;
        const uint32_t nib = ((uint32_t)masks[i] >> (4u * s)) & 15u;
        if (!nib) continue;
        const QDs D = P.ds[gr_dataset_of(P.ds, n_ds, i)];
        const key_t x = q_load_key<key_t>(D.recs + (i - D.base) * (uint64_t)RB), rx = KeyT<KW>::revcomp(x, k);
        uint32_t min_r, min_l;
        gr_shared_minima<key_t>(P, x, min_r, min_l);
        const uint32_t suf = (uint32_t)x & (P.mmask >> 2), pre = (uint32_t)(x >> (2u * (k - m + 1)));
        uint64_t e[4];
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {                     // the four neighbours of the end, two searches in lock step at a time
            bool act[2], found[2]; uint32_t d[2], a[2]; key_t key[2]; uint64_t at[2], base[2]; const uint8_t* recs[2];
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                const uint32_t nt = 2u * h + q;
                key_t fw, rv;
                gr_neighbour<key_t>(P, x, rx, kmask, top, suf, pre, min_r, min_l, 4u * s + nt, fw, rv, d[q]);
                key[q] = fw < rv ? fw : rv;
                a[q] = fw < rv ? 1u - s : s;                   // the arrival rule of k_unitig_links
                act[q] = (nib >> nt) & 1u;
            }
            q_search<key_t, RB, 2>(P, act, d, key, found, at, recs, base);
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                uint64_t ent = ~0ull;
                const uint64_t j = base[q] + at[q];
                if (act[q] && found[q] && j < n && unitig[j] != ~0ull) {      // (found, and alive: always, with the masks of these results and of this alive array)
                    const uint64_t V = unitig[j];
                    const bool begin = a[q] == ((V & 1) ? 0u : 1u);      // one arrives at the outward end of the record at position 0
                    ent = (V & ~1ull) | (begin ? 0ull : 1ull);
                } else if (act[q]) *bad = 1u;                  // the host answers GKC_ERR_ARG
                e[2 * h + q] = ent;
            }
        }
        ut_order(e[0], e[1]); ut_order(e[2], e[3]); ut_order(e[0], e[2]); ut_order(e[1], e[3]); ut_order(e[1], e[2]);
        const uint64_t off = offsets[t], deg = offsets[t + 1] - off;      // (= popcount(nib): what k_unitig_link_count saw in the same masks)
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) if (q < deg) links[off + q] = e[q];
    }
}

// gkc_graph_unitigs_links behind its guards. d_keep_slots (gkc_graph_tips_remove; u32[2 n_unitigs] or NULL): where the record << 1 | end of every slot stays for the caller
static int ut_links(gkc_ctx* c, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs, uint64_t* d_links, uint64_t cap_links, uint64_t* n_links, uint32_t* d_keep_slots)
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
        hipLaunchKernelGGL(k_unitig_link_tiles, tiles, block, 0, c->stream, (const uint32_t*)cnt, n_slots, n_tiles, ts);
        hipLaunchKernelGGL(k_unitig_link_scan, dim3(1), block, 0, c->stream, ts, n_tiles);
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
        hipLaunchKernelGGL(k_unitig_link_offsets, tiles, block, 0, c->stream, (const uint32_t*)cnt, n_slots, n_tiles, (const uint64_t*)ts, d_link_offsets);
        e = hipGetLastError();
    }
    if (e == hipSuccess && total) {
        QParams P{}; q_fill_params(P, q_model_of(c), c->qidx);
        const dim3 grid(q_grid((n_slots + GR_THREADS - 1) / GR_THREADS));
        if (c->key_words == 1) hipLaunchKernelGGL((k_unitig_link_fill<1>), grid, block, 0, c->stream, P, n_ds, n, n_slots, d_masks, unitig, (const uint32_t*)slot_rec, (const uint64_t*)d_link_offsets, d_links, d_bad);
        else                   hipLaunchKernelGGL((k_unitig_link_fill<2>), grid, block, 0, c->stream, P, n_ds, n, n_slots, d_masks, unitig, (const uint32_t*)slot_rec, (const uint64_t*)d_link_offsets, d_links, d_bad);
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

// ================================================================================================ tips (include/gkc.h, "tips": candidate, tip, competitor, round)
// A round works on the placement and the link CSR of the alive records:
//   k_tip_kc      : one thread per record: the abundance sums KC of the unitigs (64-bit vector atomics; the emit kernel's sum without the bases).
//   k_tip_flags   : one thread per unitig: the degrees of its two slots from the link offsets, its length from first[], the topological rule; for the coverage rule the
//                   entries of its linked slot and of the arrival slot of each (at most five slots), every comparison in 128-bit integers. One flag byte per unitig.
//   k_tip_mark    : one thread per slot of a SURVIVING unitig: a slot with an entry whose unitig is flagged goes on a work list (side-0 slots from the front of the list,
//                   side-1 slots from its back: a single-record unitig has both sides in one mask byte, and each list is refreshed by a launch of its own).
//   k_tip_kill    : one thread per record: the records of flagged unitigs die, alive[i] = 0, masks[i] = 0.
//   k_tip_refresh : one thread per listed slot, so that nearly every lane searches (extremities are few among the records). For each bit of the
//                   outward nibble of the slot's record the neighbour is built and searched as in k_unitig_link_fill; the bit of a neighbour that has died is cleared.
//                   Only extremities name records of other unitigs, so no other mask changes. A neighbour that is no record raises *bad.
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
__device__ __forceinline__ uint64_t ut_length(const uint64_t* __restrict__ first, uint64_t n_alive, uint64_t n_unitigs, uint64_t u) { return (u + 1 < n_unitigs ? first[u + 1] : n_alive) - first[u]; }
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
        const unsigned long long vote = __ballot(tip);
        if (tip && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)vote) - 1u) atomicAdd(&cnt->n_tips, (unsigned long long)__popcll(vote));
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
        const unsigned long long vote = __ballot(dies);
        if (dies && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)vote) - 1u) atomicAdd(&cnt->n_removed, (unsigned long long)__popcll(vote));
    }
}
template <int KW>
__global__ __launch_bounds__(GR_THREADS) void k_tip_refresh(QParams P, uint32_t n_ds, uint64_t n, const uint32_t* __restrict__ work, uint64_t n_work, const uint32_t* __restrict__ slot_rec,
                                                             const uint8_t* __restrict__ alive, uint8_t* __restrict__ masks, TipCounters* __restrict__ cnt)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr int RB = 2 * (int)sizeof(key_t);
    const uint32_t k = P.k, m = P.m;
    const key_t kmask = KeyT<KW>::mask(k);
    const uint32_t top = 2u * (k - 1);
    for (uint64_t w = (uint64_t)blockIdx.x * GR_THREADS + threadIdx.x; w < n_work; w += (uint64_t)gridDim.x * GR_THREADS) {
        const uint32_t sr = slot_rec[work[w]], s = sr & 1u;    // the record whose end s is this side; no other thread of this launch has the same record (one side per launch)
        const uint64_t i = sr >> 1;
        const uint32_t mk = masks[i], nib = (mk >> (4u * s)) & 15u;
        if (!nib) continue;
        const QDs D = P.ds[gr_dataset_of(P.ds, n_ds, i)];
        const key_t x = q_load_key<key_t>(D.recs + (i - D.base) * (uint64_t)RB), rx = KeyT<KW>::revcomp(x, k);
        uint32_t min_r, min_l;
        gr_shared_minima<key_t>(P, x, min_r, min_l);
        const uint32_t suf = (uint32_t)x & (P.mmask >> 2), pre = (uint32_t)(x >> (2u * (k - m + 1)));
        uint32_t gone = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {                     // the four neighbours of the end, two searches in lock step at a time (k_unitig_link_fill)
            bool act[2], found[2]; uint32_t d[2]; key_t key[2]; uint64_t at[2], base[2]; const uint8_t* recs[2];
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                const uint32_t nt = 2u * h + q;
                key_t fw, rv;
                gr_neighbour<key_t>(P, x, rx, kmask, top, suf, pre, min_r, min_l, 4u * s + nt, fw, rv, d[q]);
                key[q] = fw < rv ? fw : rv;
                act[q] = (nib >> nt) & 1u;
            }
            q_search<key_t, RB, 2>(P, act, d, key, found, at, recs, base);
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                if (!act[q]) continue;
                const uint64_t j = base[q] + at[q];
                if (found[q] && j < n) { if (!alive[j]) gone |= 1u << (2u * h + q); }
                else cnt->bad = 1u;                            // the host answers GKC_ERR_ARG
            }
        }
        if (gone) masks[i] = (uint8_t)(mk & ~(gone << (4u * s)));
    }
}


// ================================================================================================ simplify (include/gkc.h, "simplify": names, bulge, erroneous connection, schedule)
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
__device__ __forceinline__ void ut_count_hits(bool hit, TipCounters* __restrict__ cnt)      // one atomic per wave
{
    const unsigned long long vote = __ballot(hit);
    if (hit && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)vote) - 1u) atomicAdd(&cnt->n_tips, (unsigned long long)__popcll(vote));
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
        ut_count_hits(hit, cnt);
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
        ut_count_hits(hit, cnt);
    }
}
// resume: how many records are alive, and *bad when a dead record has a mask (the state is not one a call left)
__global__ __launch_bounds__(256) void k_alive_check(const uint8_t* __restrict__ alive, const uint8_t* __restrict__ masks, uint64_t n, unsigned long long* __restrict__ count,
                                                      uint32_t* __restrict__ bad)
{
    uint64_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const bool a = alive[i] != 0;
        mine += a;
        if (!a && masks[i]) *bad = 1u;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
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
            if (!G.kc_done) {
                if (c->key_words == 1) hipLaunchKernelGGL((k_tip_kc<1>), per_rec, block, 0, c->stream, ds, n_ds, n, unitig, (unsigned long long*)G.kc.p);
                else                   hipLaunchKernelGGL((k_tip_kc<2>), per_rec, block, 0, c->stream, ds, n_ds, n, unitig, (unsigned long long*)G.kc.p);
            }
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
                if (c->key_words == 1) hipLaunchKernelGGL((k_tip_refresh<1>), grid, blk, 0, c->stream, P, n_ds, n, work, nw, (const uint32_t*)G.slot.p, (const uint8_t*)d_alive, d_masks, cnt);
                else                   hipLaunchKernelGGL((k_tip_refresh<2>), grid, blk, 0, c->stream, P, n_ds, n, work, nw, (const uint32_t*)G.slot.p, (const uint8_t*)d_alive, d_masks, cnt);
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

extern "C" {

int gkc_graph_tips_remove(gkc_ctx* c, uint8_t* d_masks, uint8_t* d_alive, const gkc_tip_params* params, uint64_t* n_rounds, uint64_t* tips_per_round, uint64_t* n_records_removed,
                          uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    static const char* who = "gkc_graph_tips_remove";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_rounds) *n_rounds = 0;
    if (n_records_removed) *n_records_removed = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (n_cycles) *n_cycles = 0;
    GKC_TRY(q_prepare(c, who));
    UnitigPlacement& U = c->unitigs;
    if (!params || params->rc_den == 0 || params->max_rounds > 64) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the parameters are required, rc_den != 0, max_rounds <= 64", who); }
    if (!d_masks || !d_alive) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the masks (in, out) and the alive array (out) are required", who); }
    if (tips_per_round) for (uint32_t r = 0; r < params->max_rounds; r++) tips_per_round[r] = 0;
    const uint64_t n = gr_total(c);
    SimplifyRules R{};
    R.tips = TipRule{c->k, params->max_len_topo, params->max_len_rc, params->rc_num, params->rc_den};
    if (n) { GKC_HIP(c, hipMemsetAsync(d_alive, 1, (size_t)n, c->stream)); GKC_HIP(c, hipStreamSynchronize(c->stream)); }
    RoundGraph G; G.n_alive = n;
    uint64_t rounds = 0;
    for (uint32_t r = 0; r < params->max_rounds; r++) {
        uint64_t nu = 0, hits = 0, gone = 0;
        GKC_TRY(ut_round(c, who, d_masks, d_alive, G, UT_KIND_TIPS, R, &nu, &hits, &gone));
        rounds++;
        if (tips_per_round) tips_per_round[r] = hits;
        if (!hits) break;
    }
    GKC_TRY(ut_rounds_finish(c, who, d_masks, d_alive, G));
    if (n_rounds) *n_rounds = rounds;
    if (n_records_removed) *n_records_removed = G.removed;
    if (n_unitigs) *n_unitigs = U.n_unitigs;
    if (n_bases) *n_bases = U.n_bases;
    if (n_cycles) *n_cycles = U.n_cycles;
    return GKC_OK;
}

int gkc_graph_simplify(gkc_ctx* c, uint8_t* d_masks, uint8_t* d_alive, const gkc_simplify_params* params, gkc_simplify_round* log, uint64_t cap_log, uint64_t* n_rounds,
                       uint64_t* n_records_removed, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles)
{
    static const char* who = "gkc_graph_simplify";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_rounds) *n_rounds = 0;
    if (n_records_removed) *n_records_removed = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (n_cycles) *n_cycles = 0;
    GKC_TRY(q_prepare(c, who));
    UnitigPlacement& U = c->unitigs;
    if (!params || params->tips.rc_den == 0 || params->bulge_alt_den == 0 || params->ec_den == 0)
        { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the parameters are required, tips.rc_den != 0, bulge_alt_den != 0, ec_den != 0", who); }
    if (params->tips.max_rounds > 64 || params->bulge_max_rounds > 64 || params->ec_max_rounds > 64 || params->max_sweeps > 16)
        { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: max_rounds <= 64 for every kind, max_sweeps <= 16", who); }
    if (!d_masks || !d_alive) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: the masks (in, out) and the alive array (%s) are required", who, params->resume ? "in, out" : "out"); }
    const uint64_t n = gr_total(c);
    SimplifyRules R{};
    R.tips = TipRule{c->k, params->tips.max_len_topo, params->tips.max_len_rc, params->tips.rc_num, params->tips.rc_den};
    R.bulges = BulgeRule{c->k, params->bulge_max_len, params->bulge_alt_num, params->bulge_alt_den, params->bulge_alt_add};
    R.ec = EcRule{c->k, params->ec_max_len, params->ec_num, params->ec_den};
    RoundGraph G; G.n_alive = n;
    if (n && !params->resume) { GKC_HIP(c, hipMemsetAsync(d_alive, 1, (size_t)n, c->stream)); GKC_HIP(c, hipStreamSynchronize(c->stream)); }
    else if (n) {                                              // the state an earlier call left: count it, and see that no dead record has a mask
        DevBuf d_cnt;
        GKC_TRY(c->ensure(d_cnt, 16));
        uint64_t h[2] = {0, 0};
        hipError_t e = hipMemsetAsync(d_cnt.p, 0, 16, c->stream);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_alive_check, dim3(q_grid((n + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)d_alive, (const uint8_t*)d_masks, n, (unsigned long long*)d_cnt.p, (uint32_t*)((uint64_t*)d_cnt.p + 1)); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipMemcpyAsync(h, d_cnt.p, 16, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);  // (also after a failure: the scratch goes back to the pool)
        if (e != hipSuccess || es != hipSuccess) U.drop();
        GKC_HIP(c, e); GKC_HIP(c, es);
        if (h[1]) { U.drop(); GKC_FAIL(c, GKC_ERR_ARG, "%s: resume: a dead record of d_alive has a mask in d_masks (not a state an earlier call left)", who); }
        G.n_alive = h[0]; G.subset = true;
    }
    uint64_t rounds = 0;
    // phase(kind): rounds of the kind until one removes nothing or the kind's max_rounds have run -> what it removed
    auto phase = [&](uint32_t kind, uint32_t sweep, uint64_t* gone_phase) -> int {
        const uint32_t max_rounds = kind == UT_KIND_TIPS ? params->tips.max_rounds : kind == UT_KIND_BULGES ? params->bulge_max_rounds : params->ec_max_rounds;
        for (uint32_t r = 0; r < max_rounds; r++) {
            uint64_t nu = 0, hits = 0, gone = 0;
            GKC_TRY(ut_round(c, who, d_masks, d_alive, G, kind, R, &nu, &hits, &gone));
            if (log && rounds < cap_log) log[rounds] = gkc_simplify_round{kind, sweep, nu, hits, gone};
            rounds++;
            *gone_phase += gone;
            if (!hits) break;
        }
        return GKC_OK;
    };
    uint64_t gone = 0;
    GKC_TRY(phase(UT_KIND_TIPS, 0, &gone));
    for (uint32_t sweep = 1; sweep <= params->max_sweeps; sweep++) {
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

}  // extern "C"
