// gkc_graph.hpp — what the kernels over the solid records in flat order share (gkc_graph.hip: neighbour masks, branching nodes; gkc_unitigs.hip, gkc_unitig_links.hip,
// gkc_simplify.hip: the compacted graph; gkc_paths.hip: read paths): the tile geometry, the dataset of a flat record index, a record with what its neighbours are made
// from (GrNode), the search of the four neighbours of one end, the workgroup prefix sum with the tile kernels on top of it, the mask loads and the key-width dispatch.
// Device code + the host entry points of gkc_graph.hip that the other files call.
#pragma once
#include "gkc_common.hpp"
#include "gkc_device.hpp"
#include "gkc_query.hpp"

constexpr int GR_THREADS = 256, GR_PER_THREAD = 4;
constexpr int GR_TILE = GR_THREADS * GR_PER_THREAD;          // records per tile of the topology / numbering kernels
constexpr int GR_LOCKSTEP = 2;                               // searches a thread advances together (two, more was no better)
static_assert(4 % GR_LOCKSTEP == 0, "the four neighbours of an end, and so all eight, are searched in groups of GR_LOCKSTEP");

// the dataset a flat record index lies in: the last d with base <= g (an empty dataset shares its base with the next one; g is below the total)
__device__ __forceinline__ uint32_t gr_dataset_of(const QDs* __restrict__ ds, uint32_t n_ds, uint64_t g)
{
    uint32_t lo = 0, hi = n_ds;          // answer in [lo, hi)
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (ds[mid].base <= g) lo = mid; else hi = mid; }
    return lo;
}

// The eight neighbours of a solid record are made from its value x and ONE reverse complement rx: a right extension is ((x << 2) | nt) & mask with reverse complement
// (rx >> 2) | (comp(nt) << 2(k-1)), a left extension the mirror image. A neighbour shares k-1 bases with x, so its minimizer is the minimum over the k-m m-mers it shares
// with x and its one new m-mer: the order keys of x's m-mers are computed once (k-m+1 evaluations), the running minimum without the first (min_r) / without the last
// (min_l) m-mer kept, and each neighbour adds one evaluation (the order key does not depend on the strand: q_mmer_key takes the canonical m-mer, the frequency table is
// built over canonical m-mers). GrNode is the record with all of that: one load per record, one neighbour() per neighbour.
// (The minima stay a function of their own that takes the key by value: written out inside load() the same loop costs k_graph_masks<2> and k_unitig_links<2> two
// VGPRs and with them a wave of occupancy)
template <typename K>
__device__ __forceinline__ void gr_shared_minima(const QParams& P, K x, uint32_t& min_r, uint32_t& min_l)
{
    const uint32_t k = P.k, m = P.m;
    min_r = P.default_key; min_l = P.default_key;
    for (uint32_t j = 0; j < P.nb_mm; j++) {                   // first to last: a right extension loses the first one, a left extension the last one
        const uint32_t key = q_mmer_key(P, (uint32_t)(x >> (2u * (k - m - j))) & P.mmask);
        if (j != 0) min_r = key < min_r ? key : min_r;
        if (j + 1 != P.nb_mm) min_l = key < min_l ? key : min_l;
    }
}
template <int KW>
struct GrNode {
    typedef typename KeyT<KW>::type key_t;
    static constexpr int RB = 2 * (int)sizeof(key_t);          // bytes from one record's key to the next
    const key_t kmask; const uint32_t top;                     // of P, once per kernel: the 2k low bits, the bit position of a k-mer's first nucleotide
    key_t x, rx; uint32_t min_r, min_l, suf, pre;              // of the record: its two strands, the shared minima, its last / first m-1 nucleotides
    __device__ __forceinline__ explicit GrNode(const QParams& P) : kmask(KeyT<KW>::mask(P.k)), top(2u * (P.k - 1)) {}
    // the record at flat index g
    __device__ __forceinline__ void load(const QParams& P, uint32_t n_ds, uint64_t g)
    {
        const uint32_t k = P.k, m = P.m;
        const QDs D = P.ds[gr_dataset_of(P.ds, n_ds, g)];
        x = q_load_key<key_t>(D.recs + (g - D.base) * (uint64_t)RB);
        rx = KeyT<KW>::revcomp(x, k);
        gr_shared_minima<key_t>(P, x, min_r, min_l);
        suf = (uint32_t)x & (P.mmask >> 2);
        pre = (uint32_t)(x >> (2u * (k - m + 1)));
    }
    // neighbour e (bit order of the mask: 0-3 right extensions, 4-7 left extensions): its two strands and the dataset its canonical form lies in
    __device__ __forceinline__ void neighbour(const QParams& P, uint32_t e, key_t& fw, key_t& rv, uint32_t& d) const
    {
        const uint32_t m = P.m, nt = e & 3u;
        const bool left = e >= 4;
        fw = left ? ((x >> 2) | ((key_t)nt << top)) : (((x << 2) | (key_t)nt) & kmask);
        rv = left ? (((rx << 2) | (key_t)(nt ^ 2u)) & kmask) : ((rx >> 2) | ((key_t)(nt ^ 2u) << top));
        const uint32_t mk = q_mmer_key(P, left ? ((nt << (2u * (m - 1))) | pre) : ((suf << 2) | nt));
        const uint32_t shared = left ? min_l : min_r;
        d = q_dataset_of(P, mk < shared ? mk : shared);
    }
};
// the end of a neighbour one arrives at, having left a record through its end s (0: right, 1: left): leaving right one arrives at the left end of a neighbour that is
// canonical as it stands (fw < rv); leaving left, the mirror image
template <typename K> __device__ __forceinline__ uint32_t gr_arrival(uint32_t s, K fw, K rv) { return fw < rv ? 1u - s : s; }
// The four neighbours of end s of N, two searches in lock step at a time. Per neighbour nt: f(nt, named, found, j, a) with named = the nibble of the end has bit nt, found =
// the search (run only for a named neighbour) hit a record, j = that record's flat index, a = the end of it one arrives at.
template <int KW, typename F>
__device__ __forceinline__ void gr_end_search(const QParams& P, const GrNode<KW>& N, uint32_t s, uint32_t nib, F&& f)
{
    typedef typename GrNode<KW>::key_t key_t;
#pragma unroll
    for (uint32_t h = 0; h < 4 / GR_LOCKSTEP; h++) {
        bool act[GR_LOCKSTEP], found[GR_LOCKSTEP]; uint32_t d[GR_LOCKSTEP], a[GR_LOCKSTEP]; key_t key[GR_LOCKSTEP]; uint64_t at[GR_LOCKSTEP], base[GR_LOCKSTEP];
        const uint8_t* recs[GR_LOCKSTEP];
#pragma unroll
        for (uint32_t q = 0; q < GR_LOCKSTEP; q++) {
            const uint32_t nt = GR_LOCKSTEP * h + q;
            key_t fw, rv;
            N.neighbour(P, 4u * s + nt, fw, rv, d[q]);
            key[q] = fw < rv ? fw : rv;                        // Model.hpp:294
            a[q] = gr_arrival(s, fw, rv);
            act[q] = (nib >> nt) & 1u;
        }
        q_search<key_t, GrNode<KW>::RB, GR_LOCKSTEP>(P, act, d, key, found, at, recs, base);
#pragma unroll
        for (uint32_t q = 0; q < GR_LOCKSTEP; q++) f(GR_LOCKSTEP * h + q, act[q], found[q], base[q] + at[q], a[q]);
    }
}

// exclusive prefix of v over the GR_THREADS threads of the workgroup; *total = sum. s_w: GR_THREADS / 64 elements of LDS, free again on return
template <typename T>
__device__ __forceinline__ T gr_block_excl(T v, T* s_w, T* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < GR_THREADS / 64; w++) { const T s = s_w[w]; if (w < wv) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + x - v;
}
// the masks of records i .. i + 3 (i a multiple of 4) as one word, and how many of them exist; the caller's array need not be readable beyond n
__device__ __forceinline__ uint32_t gr_load4_masks(const uint8_t* __restrict__ f, uint64_t n, uint64_t i, uint32_t* n_valid)
{
    static_assert(GR_PER_THREAD == 4, "one 32-bit load per thread");
    if (i >= n) { *n_valid = 0; return 0u; }
    if (i + 4 <= n && ((uintptr_t)f & 3) == 0) { *n_valid = 4; return *reinterpret_cast<const uint32_t*>(f + i); }
    const uint32_t c = n - i < 4 ? (uint32_t)(n - i) : 4u;
    uint32_t w = 0;
    for (uint32_t r = 0; r < c; r++) w |= (uint32_t)f[i + r] << (8 * r);
    *n_valid = c;
    return w;
}

// A prefix sum over n elements in three launches: k_graph_tile_sums, gr_scan_tiles (below), k_graph_tile_offsets. The value of element i is val(i), val a small struct with
// __device__ uint32_t operator()(uint64_t i) const.
template <typename F>
__global__ __launch_bounds__(GR_THREADS) void k_graph_tile_sums(F val, uint64_t n, uint32_t n_tiles, uint64_t* __restrict__ tile_sum)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) sum += i0 + r < n ? val(i0 + r) : 0u;
        uint64_t tot;
        gr_block_excl<uint64_t>(sum, s_w, &tot);
        if (threadIdx.x == 0) tile_sum[t] = tot;
    }
}
// out[i] = the values in front of element i: the exclusive prefix inside the tile on top of the tile's offset. CLOSE: out[n] = everything (out has n + 1 entries then)
template <bool CLOSE, typename F>
__global__ __launch_bounds__(GR_THREADS) void k_graph_tile_offsets(F val, uint64_t n, uint32_t n_tiles, const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out)
{
    __shared__ uint64_t s_w[GR_THREADS / 64];
    if (CLOSE && blockIdx.x == 0 && threadIdx.x == 0) out[n] = tile_off[n_tiles];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * GR_TILE + (uint64_t)threadIdx.x * GR_PER_THREAD;
        uint32_t v[GR_PER_THREAD]; uint64_t sum = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) { v[r] = i0 + r < n ? val(i0 + r) : 0u; sum += v[r]; }
        uint64_t tot;
        uint64_t o = tile_off[t] + gr_block_excl<uint64_t>(sum, s_w, &tot);
#pragma unroll
        for (uint32_t r = 0; r < GR_PER_THREAD; r++) { if (i0 + r < n) out[i0 + r] = o; o += v[r]; }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// the statement once per key width, KW = 1 or 2 inside it: GR_BY_KEY_WIDTH(c, hipLaunchKernelGGL((k_graph_masks<KW>), grid, block, 0, c->stream, ...));
#define GR_BY_KEY_WIDTH(c, ...) do { if ((c)->key_words == 1) { constexpr int KW = 1; __VA_ARGS__; } else { constexpr int KW = 2; __VA_ARGS__; } } while (0)
// gkc_graph.hip
uint64_t gr_total(const gkc_ctx* c);                          // solid records of all datasets
// masks of the records [g0, g0 + n) of the flat order into d_masks[0, n); q_prepare has run
int gr_masks_run(gkc_ctx* c, uint64_t g0, uint64_t n, uint8_t* d_masks);
// one launch of one workgroup on c->stream: the exclusive prefix of the tile sums a[0, n_tiles) in place, a[n_tiles] = everything; the same for b unless it is NULL
void gr_scan_tiles(gkc_ctx* c, uint64_t* a, uint64_t* b, uint32_t n_tiles);
