// gkc_graph.hpp — what the kernels over the solid records in flat order share (gkc_graph.hip: neighbour masks, branching nodes; gkc_unitigs.hip: unitigs): the tile
// geometry, the dataset of a flat record index, the neighbours of a record with their minimizers, the workgroup prefix sum and the mask loads. Device code + the host
// entry points of gkc_graph.hip that gkc_unitigs.hip calls.
#pragma once
#include "gkc_common.hpp"
#include "gkc_device.hpp"
#include "gkc_query.hpp"

constexpr int GR_THREADS = 256, GR_PER_THREAD = 4;
constexpr int GR_TILE = GR_THREADS * GR_PER_THREAD;          // records per tile of the topology / numbering kernels
constexpr int GR_LOCKSTEP = 2;                               // searches a thread advances together (two, more was no better)
static_assert(8 % GR_LOCKSTEP == 0, "the eight neighbours are searched in groups of GR_LOCKSTEP");

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
// built over canonical m-mers).
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
// neighbour e (bit order of the mask: 0-3 right extensions, 4-7 left extensions) of x: its two strands and the dataset its canonical form lies in. kmask: the 2k low bits,
// top: bit position of a k-mer's first nucleotide, suf / pre: the last / the first m-1 nucleotides of x
template <typename K>
__device__ __forceinline__ void gr_neighbour(const QParams& P, K x, K rx, K kmask, uint32_t top, uint32_t suf, uint32_t pre, uint32_t min_r, uint32_t min_l, uint32_t e,
                                             K& fw, K& rv, uint32_t& d)
{
    const uint32_t m = P.m, nt = e & 3u;
    const bool left = e >= 4;
    fw = left ? ((x >> 2) | ((K)nt << top)) : (((x << 2) | (K)nt) & kmask);
    rv = left ? (((rx << 2) | (K)(nt ^ 2u)) & kmask) : ((rx >> 2) | ((K)(nt ^ 2u) << top));
    const uint32_t mk = q_mmer_key(P, left ? ((nt << (2u * (m - 1))) | pre) : ((suf << 2) | nt));
    const uint32_t shared = left ? min_l : min_r;
    d = q_dataset_of(P, mk < shared ? mk : shared);
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

// ------------------------------------------------------------------------------------------------ host side (gkc_graph.hip)
uint64_t gr_total(const gkc_ctx* c);                          // solid records of all datasets
// masks of the records [g0, g0 + n) of the flat order into d_masks[0, n); q_prepare has run
int gr_masks_run(gkc_ctx* c, uint64_t g0, uint64_t n, uint8_t* d_masks);
// ------------------------------------------------------------------------------------------------ host side (gkc_unitigs.hip)
// q_prepare, then: the context holds a placement and it describes the results the context holds now (GKC_ERR_ARG otherwise)
int ut_require_placement(gkc_ctx* c, const char* who);
