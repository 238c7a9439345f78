// gkc_banks.hip — several banks counted one after another, merged on the device into one abundance per bank and k-mer, and the
// solidity kinds of the reference evaluated on the merged state (include/gkc.h, "multi-bank counting").
//
// The reference counts an album of N banks in one run: every count processor receives a CountVector with one abundance per bank
// (SortingCountAlgorithm.cpp, PartitionsCommand.cpp:insert), CountProcessorSolidity.hpp:176-304 decides solidity from it, CountProcessorDump.hpp:148-152
// writes Count{kmer, sum} and CountProcessorHistogram.hpp:173-184 bins the sum. Here each bank is counted on its own by the unchanged Stage A / Stage B with the
// window [1, INT32_MAX] (every distinct k-mer of the bank comes out), and gkc_banks_add merges the ascending Count[] of every dataset into the state:
//
//   keys   : the distinct k-mers of all datasets, dataset after dataset (d = part + pass * nb_partitions), ascending inside a dataset; 8 B (k <= 31) or 16 B
//   planes : one int32 array per bank that was added, parallel to `keys` (plane-major: adding a bank streams whole planes); a bank never added has no plane = zeros
//
// Merge of a bank's arrays B_d into the state's A_d, all datasets in ONE launch sequence (workgroups take (dataset, tile) pairs from a device table):
//   k_bk_search_b : every element of B finds lower_bound in A and whether its key is already there (a duplicate); the binary search of a tile's elements is bounded
//                   by the searches of the tile's first and last key (both arrays ascend)
//   scan          : exclusive prefix sum of the duplicate flags over all B (k_bk_tile_sums, k_bk_scan_sums, k_bk_scan_apply)
//   (host)        : duplicates per dataset -> union sizes -> fresh key array and planes
//   k_bk_scatter_a: A[i] goes to i + (non-duplicates of B below it: a bounded search again), with its counts of every plane
//   k_bk_scatter_b: B[j] goes to lower_bound + (non-duplicates of B before it): a new key with zeros in the other planes, or — a duplicate — its count alone
// Every position of every new plane is written exactly once, by one thread: nothing is merged in place and nothing needs a memset.
// Element indices are 64-bit everywhere; tiles are counted in 32 bits (2^32 tiles of 1024 elements).
#include "gkc_common.hpp"
#include "gkc_device.hpp"

constexpr int BK_THREADS = 256, BK_PER_THREAD = 4;
constexpr int BK_TILE = BK_THREADS * BK_PER_THREAD;      // elements one workgroup takes at a time            (gkc.py: Banks.TILE)
constexpr int BK_SCAN_BLOCK = 256;                       // tile sums the one-workgroup scan takes at a time  (gkc.py: Banks.SCAN_BLOCK)
constexpr uint32_t BK_MAX_BANKS = 64;
constexpr uint32_t BK_GRID_MAX = 256 * 8;                // memory-bound: 8 workgroups per CU, the rest by grid stride
constexpr uint32_t BK_LDS_BINS = 16000;                  // histograms up to this many bins are privatised in LDS (64 KB of u32), larger ones go to HBM atomics

struct BkDataset {                       // one per dataset + a sentinel (tile firsts, b_first)
    uint64_t a_off, a_n;                 // the dataset in the state's arrays
    const uint8_t* b_recs; uint64_t b_n; // the bank's Count records of the dataset (b_n = 0: nothing to merge)
    uint64_t b_first;                    // ... and their place in the flat order of all B elements of the call
    uint64_t n_off;                      // the dataset in the new arrays (filled in after the scan)
    uint32_t ta_first, tb_first;         // first tile of the dataset among the tiles of all A / all B
};
struct BkPlanes { const int32_t* in[BK_MAX_BANKS]; int32_t* out[BK_MAX_BANKS]; };
struct BkEval { const int32_t* plane[BK_MAX_BANKS]; int32_t amin[BK_MAX_BANKS], amax[BK_MAX_BANKS]; uint8_t solid[BK_MAX_BANKS]; };

// ------------------------------------------------------------------------------------------------ device helpers
// exclusive prefix of v over the BK_THREADS threads of the workgroup; *total = sum. s_w: 4 words of LDS, free again on return
__device__ __forceinline__ uint32_t bk_block_excl(uint32_t v, uint32_t* s_w, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BK_THREADS / 64; w++) { const uint32_t s = s_w[w]; if (w < wv) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + x - v;
}
// which dataset a tile belongs to: the last d with first[d] <= t (first[] ascending, first[n_ds] = number of tiles; datasets without tiles repeat a value)
template <bool B_SIDE> __device__ __forceinline__ uint32_t bk_dataset_of(const BkDataset* __restrict__ ds, uint32_t n_ds, uint32_t t)
{
    uint32_t lo = 0, hi = n_ds;          // answer in [lo, hi)
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; const uint32_t f = B_SIDE ? ds[mid].tb_first : ds[mid].ta_first; if (f <= t) lo = mid; else hi = mid; }
    return lo;
}
template <typename K> __device__ __forceinline__ K bk_rec_key(const uint8_t* recs, uint64_t j) { return *reinterpret_cast<const K*>(recs + j * (2 * sizeof(K))); }
template <typename K> __device__ __forceinline__ int32_t bk_rec_count(const uint8_t* recs, uint64_t j) { return *reinterpret_cast<const int32_t*>(recs + j * (2 * sizeof(K)) + sizeof(K)); }
// first index in [lo, hi) whose key is not below `key` (hi if none); 16-byte keys compare as (hi, lo): the u128 order
template <typename K> __device__ __forceinline__ uint64_t bk_lower_bound_keys(const K* __restrict__ a, uint64_t lo, uint64_t hi, K key)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
template <typename K> __device__ __forceinline__ uint64_t bk_lower_bound_recs(const uint8_t* __restrict__ recs, uint64_t lo, uint64_t hi, K key)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (bk_rec_key<K>(recs, mid) < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// ------------------------------------------------------------------------------------------------ merge
template <int KW>
__global__ __launch_bounds__(BK_THREADS) void k_bk_search_b(const BkDataset* __restrict__ ds, uint32_t n_ds, uint32_t n_tiles, const typename KeyT<KW>::type* __restrict__ a_keys,
                                                            uint64_t* __restrict__ lb_out, uint8_t* __restrict__ dup_out)
{
    typedef typename KeyT<KW>::type key_t;
    __shared__ uint64_t s_bound[2];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t d = bk_dataset_of<true>(ds, n_ds, t);
        const BkDataset D = ds[d];
        const key_t* a = a_keys + D.a_off;
        const uint64_t j0 = (uint64_t)(t - D.tb_first) * BK_TILE;
        // the tile's first and last key bound every search of the tile: a few hundred keys of A (both arrays ascend), not all of them
        if (threadIdx.x < 2) s_bound[threadIdx.x] = bk_lower_bound_keys<key_t>(a, 0, D.a_n, bk_rec_key<key_t>(D.b_recs, threadIdx.x == 0 ? j0 : min(j0 + BK_TILE, D.b_n) - 1));
        __syncthreads();
        const uint64_t b_lo = s_bound[0], b_hi = s_bound[1];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BK_PER_THREAD; r++) {
            const uint64_t j = j0 + (uint64_t)r * BK_THREADS + threadIdx.x;
            if (j >= D.b_n) continue;
            const key_t key = bk_rec_key<key_t>(D.b_recs, j);
            const uint64_t lb = bk_lower_bound_keys<key_t>(a, b_lo, b_hi, key);
            lb_out[D.b_first + j] = lb;
            dup_out[D.b_first + j] = (lb < D.a_n && a[lb] == key) ? 1 : 0;
        }
    }
}
template <int KW>
__global__ __launch_bounds__(BK_THREADS) void k_bk_scatter_a(const BkDataset* __restrict__ ds, uint32_t n_ds, uint32_t n_tiles, const typename KeyT<KW>::type* __restrict__ a_keys,
                                                             const uint64_t* __restrict__ dup_scan, BkPlanes P, uint32_t nb_banks, uint32_t bank,
                                                             typename KeyT<KW>::type* __restrict__ n_keys)
{
    typedef typename KeyT<KW>::type key_t;
    __shared__ uint64_t s_bound[2];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t d = bk_dataset_of<false>(ds, n_ds, t);
        const BkDataset D = ds[d];
        const uint64_t i0 = (uint64_t)(t - D.ta_first) * BK_TILE;
        if (threadIdx.x < 2) s_bound[threadIdx.x] = D.b_n ? bk_lower_bound_recs<key_t>(D.b_recs, 0, D.b_n, a_keys[D.a_off + (threadIdx.x == 0 ? i0 : min(i0 + BK_TILE, D.a_n) - 1)]) : 0;
        __syncthreads();
        const uint64_t b_lo = s_bound[0], b_hi = s_bound[1];          // (as in k_bk_search_b: the searches of the tile end inside this range of B)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BK_PER_THREAD; r++) {
            const uint64_t i = i0 + (uint64_t)r * BK_THREADS + threadIdx.x;
            if (i >= D.a_n) continue;
            const key_t key = a_keys[D.a_off + i];
            uint64_t below = 0; bool dup = false;               // non-duplicate elements of B below the key; the key is in B as well
            if (D.b_n) {
                const uint64_t rk = bk_lower_bound_recs<key_t>(D.b_recs, b_lo, b_hi, key);
                below = rk - (dup_scan[D.b_first + rk] - dup_scan[D.b_first]);
                dup = rk < D.b_n && bk_rec_key<key_t>(D.b_recs, rk) == key;
            }
            const uint64_t pos = D.n_off + i + below;
            n_keys[pos] = key;
            for (uint32_t p = 0; p < nb_banks; p++) {
                if (!P.out[p]) continue;
                if (p == bank && dup) continue;                 // the duplicate in B writes its count there
                P.out[p][pos] = P.in[p] ? P.in[p][D.a_off + i] : 0;
            }
        }
    }
}
template <int KW>
__global__ __launch_bounds__(BK_THREADS) void k_bk_scatter_b(const BkDataset* __restrict__ ds, uint32_t n_ds, uint32_t n_tiles, const uint64_t* __restrict__ lb_in,
                                                             const uint8_t* __restrict__ dup_in, const uint64_t* __restrict__ dup_scan, BkPlanes P, uint32_t nb_banks, uint32_t bank,
                                                             typename KeyT<KW>::type* __restrict__ n_keys)
{
    typedef typename KeyT<KW>::type key_t;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t d = bk_dataset_of<true>(ds, n_ds, t);
        const BkDataset D = ds[d];
        const uint64_t j0 = (uint64_t)(t - D.tb_first) * BK_TILE;
#pragma unroll
        for (int r = 0; r < BK_PER_THREAD; r++) {
            const uint64_t j = j0 + (uint64_t)r * BK_THREADS + threadIdx.x;
            if (j >= D.b_n) continue;
            const uint64_t g = D.b_first + j;
            const uint64_t pos = D.n_off + lb_in[g] + (j - (dup_scan[g] - dup_scan[D.b_first]));
            const int32_t cnt = bk_rec_count<key_t>(D.b_recs, j);
            if (dup_in[g]) { P.out[bank][pos] = cnt; continue; }
            n_keys[pos] = bk_rec_key<key_t>(D.b_recs, j);
            for (uint32_t p = 0; p < nb_banks; p++) if (P.out[p]) P.out[p][pos] = p == bank ? cnt : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ exclusive prefix sum of 0/1 flags (u8[n], readable up to a multiple of 4) -> u64[n + 1]
__device__ __forceinline__ uint32_t bk_load4_flags(const uint8_t* __restrict__ f, uint64_t n, uint64_t i, uint32_t v[BK_PER_THREAD])
{
    static_assert(BK_PER_THREAD == 4, "one 32-bit load per thread");
    const uint32_t w = i < n ? *reinterpret_cast<const uint32_t*>(f + i) : 0u;
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) { v[r] = (i + r < n) ? ((w >> (8 * r)) & 1u) : 0u; s += v[r]; }
    return s;
}
__global__ __launch_bounds__(BK_THREADS) void k_bk_tile_sums(const uint8_t* __restrict__ f, uint64_t n, uint32_t n_tiles, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t s_w[BK_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t v[BK_PER_THREAD], tot;
        const uint32_t s = bk_load4_flags(f, n, (uint64_t)t * BK_TILE + (uint64_t)threadIdx.x * BK_PER_THREAD, v);
        (void)bk_block_excl(s, s_w, &tot);
        if (threadIdx.x == 0) sums[t] = tot;
    }
}
// one workgroup: offs[t] = sums[0] + ... + sums[t - 1], offs[n_tiles] = everything; BK_SCAN_BLOCK sums at a time, the carry in 64 bits
__global__ __launch_bounds__(BK_SCAN_BLOCK) void k_bk_scan_sums(const uint32_t* __restrict__ sums, uint32_t n_tiles, uint64_t* __restrict__ offs)
{
    static_assert(BK_SCAN_BLOCK == BK_THREADS, "bk_block_excl scans BK_THREADS values");
    __shared__ uint32_t s_w[BK_THREADS / 64];
    uint64_t carry = 0;
    uint32_t ahead = threadIdx.x < n_tiles ? sums[threadIdx.x] : 0u;                  // the next block's sums are on their way while this one is scanned
    for (uint32_t base = 0; base < n_tiles; base += BK_SCAN_BLOCK) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = ahead;
        ahead = (uint64_t)t + BK_SCAN_BLOCK < n_tiles ? sums[t + BK_SCAN_BLOCK] : 0u;
        uint32_t tot;
        const uint32_t ex = bk_block_excl(v, s_w, &tot);
        if (t < n_tiles) offs[t] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) offs[n_tiles] = carry;
}
__global__ __launch_bounds__(BK_THREADS) void k_bk_scan_apply(const uint8_t* __restrict__ f, uint64_t n, uint32_t n_tiles, const uint64_t* __restrict__ offs, uint64_t* __restrict__ out)
{
    __shared__ uint32_t s_w[BK_THREADS / 64];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t v[BK_PER_THREAD], tot;
        const uint64_t i = (uint64_t)t * BK_TILE + (uint64_t)threadIdx.x * BK_PER_THREAD;
        const uint32_t s = bk_load4_flags(f, n, i, v);
        uint64_t x = offs[t] + bk_block_excl(s, s_w, &tot);
#pragma unroll
        for (int r = 0; r < BK_PER_THREAD; r++) { if (i + r < n) out[i + r] = x; x += v[r]; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = offs[n_tiles];
}
// out[i] = scan[at[i]] for the n_at boundaries the host wants to see
__global__ void k_bk_pick(const uint64_t* __restrict__ scan, const uint64_t* __restrict__ at, uint32_t n_at, uint64_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_at) out[i] = scan[at[i]];
}

// ------------------------------------------------------------------------------------------------ evaluate
// CountProcessorSolidity.hpp:176-304 restated: CountRange::includes is the closed range [amin, amax]; sum / min / max look at range 0 only (_thresholds[0])
__device__ __forceinline__ bool bk_in(int32_t v, int32_t lo, int32_t hi) { return v >= lo && v <= hi; }
// histogram[bin]++ for the lanes with `valid`, all 64 lanes of the wave calling: lanes with the same bin (most k-mers of real data have a sum of 1 or 2) are
// counted by ballot and added once — an LDS atomic per lane on one address is served one lane at a time
__device__ __forceinline__ void bk_histo_add(uint32_t* s_histo, unsigned long long* __restrict__ histo, bool lds, uint32_t bin, bool valid)
{
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
        const unsigned long long same = __ballot(valid && bin == b) & todo;
        if ((int)(threadIdx.x & 63) == leader) { if (lds) atomicAdd(&s_histo[b], (uint32_t)__popcll(same)); else atomicAdd(&histo[b], (unsigned long long)__popcll(same)); }
        todo &= ~same;
    }
}
typedef int bk_int4 __attribute__((ext_vector_type(4)));
// one thread takes BK_PER_THREAD consecutive k-mers (16-byte loads of every plane: the planes are padded to a multiple of 4 counts); few, long-lived workgroups,
// each with the histogram in LDS (lds_bins != 0) flushed once at the end
__global__ __launch_bounds__(BK_THREADS) void k_bk_eval(BkEval E, uint32_t nb_banks, uint64_t n, int kind, uint8_t* __restrict__ solid, int32_t* __restrict__ sums,
                                                        unsigned long long* __restrict__ histo, uint32_t histo_max, uint32_t lds_bins)
{
    static_assert(BK_PER_THREAD == 4, "16-byte loads of 4 counts");
    extern __shared__ uint32_t s_histo[];
    for (uint32_t b = threadIdx.x; b < lds_bins; b += BK_THREADS) s_histo[b] = 0;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * BK_TILE; base < n; base += (uint64_t)gridDim.x * BK_TILE) {       // (uniform in the workgroup: the ballots see whole waves)
        const uint64_t i = base + (uint64_t)threadIdx.x * BK_PER_THREAD;
        int64_t sum[4] = {0, 0, 0, 0}; int32_t mn[4], mx[4]; bool all[4], one[4], custom[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { mn[r] = 2147483647; mx[r] = -2147483647 - 1; all[r] = true; one[r] = false; custom[r] = true; }
        for (uint32_t p = 0; p < nb_banks; p++) {
            bk_int4 c = {0, 0, 0, 0};
            if (E.plane[p] && i < n) c = *reinterpret_cast<const bk_int4*>(E.plane[p] + i);
            const int32_t lo = E.amin[p], hi = E.amax[p]; const bool want = E.solid[p] != 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int32_t v = c[r];
                sum[r] += v; mn[r] = v < mn[r] ? v : mn[r]; mx[r] = v > mx[r] ? v : mx[r];
                const bool in = bk_in(v, lo, hi);
                all[r] = all[r] && in; one[r] = one[r] || in; custom[r] = custom[r] && (in == want);
            }
        }
        uint32_t flags = 0; bk_int4 s4;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int32_t s32 = (int32_t)sum[r];                // (sums beyond INT32_MAX are outside the contract: CountNumber is 32 bits)
            bool ok;
            switch (kind) {
                case GKC_SOLIDITY_SUM: ok = bk_in(s32, E.amin[0], E.amax[0]); break;
                case GKC_SOLIDITY_MIN: ok = bk_in(mn[r], E.amin[0], E.amax[0]); break;
                case GKC_SOLIDITY_MAX: ok = bk_in(mx[r], E.amin[0], E.amax[0]); break;
                case GKC_SOLIDITY_ONE: ok = one[r]; break;
                case GKC_SOLIDITY_ALL: ok = all[r]; break;
                default:               ok = custom[r]; break;
            }
            flags |= (ok ? 1u : 0u) << (8 * r); s4[r] = s32;
            const uint32_t bin = sum[r] < 0 ? 0u : (sum[r] > (int64_t)histo_max ? histo_max : (uint32_t)sum[r]);      // histogram of ALL distinct k-mers (CountProcessorHistogram.hpp:173-184)
            bk_histo_add(s_histo, histo, lds_bins != 0, bin, i + r < n);
        }
        if (i + 4 <= n) { *reinterpret_cast<uint32_t*>(solid + i) = flags; *reinterpret_cast<bk_int4*>(sums + i) = s4; }
        else for (int r = 0; r < 4 && i + r < n; r++) { solid[i + r] = (uint8_t)((flags >> (8 * r)) & 1u); sums[i + r] = s4[r]; }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < lds_bins; b += BK_THREADS) { const uint32_t c = s_histo[b]; if (c) atomicAdd(&histo[b], (unsigned long long)c); }
}
// solid k-mers -> Count{value, sum} records (16 / 32 bytes, pad bytes zero, like k_gather_counts) and their rows of the count matrix
template <int KW>
__global__ __launch_bounds__(BK_THREADS) void k_bk_gather(const typename KeyT<KW>::type* __restrict__ keys, BkEval E, uint32_t nb_banks, uint64_t n, const uint8_t* __restrict__ solid,
                                                          const int32_t* __restrict__ sums, const uint64_t* __restrict__ scan, uint64_t* __restrict__ out_counts, int32_t* __restrict__ out_vectors)
{
    for (uint64_t i = (uint64_t)blockIdx.x * BK_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BK_THREADS) {
        if (!solid[i]) continue;
        const uint64_t pos = scan[i];
        const uint64_t ab = (uint64_t)(uint32_t)sums[i];
        if (KW == 1) store16(out_counts + pos * 2, (unsigned long long)keys[i], ab);
        else { const u128 key = keys[i]; store16(out_counts + pos * 4, (unsigned long long)key, (unsigned long long)(key >> 64)); store16(out_counts + pos * 4 + 2, ab, 0ull); }
        for (uint32_t p = 0; p < nb_banks; p++) out_vectors[pos * nb_banks + p] = E.plane[p] ? E.plane[p][i] : 0;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct gkc_banks {
    gkc_ctx* ctx = nullptr;                  // allocator, stream and error text; kept alive by the object (children)
    uint32_t nb_banks = 0, key_words = 1, nb_partitions = 0, nb_passes = 1, n_ds = 0;
    uint64_t model_hash = 0;
    // merged state
    DevBuf keys; std::vector<DevBuf> planes;             // planes[bank].p == nullptr: the bank has no k-mer (yet)
    std::vector<uint64_t> off;                           // [n_ds + 1]: the datasets inside keys / planes
    std::vector<uint8_t> added;                          // [bank * n_ds + dataset]
    std::vector<uint64_t> merged_epoch;                  // [pass]: gkc_ctx::pass_epoch of the results merged last for the datasets of the pass
    // last evaluation
    bool evaluated = false; uint32_t histo_max = 0;
    DevBuf out_counts, out_vectors, d_histo;
    std::vector<uint64_t> solid_off;                     // [n_ds + 1]: the datasets inside out_counts / out_vectors
    // abundance queries (gkc_query_banks_reads_device): the routing tables of the model the object remembers — its own copies, the context may be configured again —
    // and the sampled index over `keys`, built by the first query and dropped by gkc_banks_add
    QueryModel qmodel{}; DevBuf q_repart, q_mkey_lut, q_key2val; QueryIndex qidx;
    uint64_t n_total() const { return off.empty() ? 0 : off.back(); }
    size_t key_bytes() const { return key_words == 1 ? 8 : 16; }
};

static unsigned bk_grid(uint64_t n_blocks) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_blocks, BK_GRID_MAX)); }

// d_scan[n + 1] = exclusive prefix sum of d_flags[n] (n >= 1), on c->stream
static int bk_scan(gkc_ctx* c, const uint8_t* d_flags, uint64_t n, uint64_t* d_scan, DevBuf& d_sums, DevBuf& d_offs)
{
    const uint64_t n_tiles64 = (n + BK_TILE - 1) / BK_TILE;
    if (n_tiles64 >= (1ull << 32)) GKC_FAIL(c, GKC_ERR_ARG, "%llu elements are more than the scan's 2^32 tiles", (unsigned long long)n);
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    GKC_TRY(c->ensure(d_sums, (size_t)n_tiles * 4)); GKC_TRY(c->ensure(d_offs, ((size_t)n_tiles + 1) * 8));
    hipLaunchKernelGGL(k_bk_tile_sums, dim3(bk_grid(n_tiles)), dim3(BK_THREADS), 0, c->stream, d_flags, n, n_tiles, (uint32_t*)d_sums.p);
    hipLaunchKernelGGL(k_bk_scan_sums, dim3(1), dim3(BK_SCAN_BLOCK), 0, c->stream, (const uint32_t*)d_sums.p, n_tiles, (uint64_t*)d_offs.p);
    hipLaunchKernelGGL(k_bk_scan_apply, dim3(bk_grid(n_tiles)), dim3(BK_THREADS), 0, c->stream, d_flags, n, n_tiles, (const uint64_t*)d_offs.p, d_scan);
    GKC_HIP(c, hipGetLastError());
    return GKC_OK;
}
// h_out[i] = d_scan[h_at[i]]; synchronizes c->stream
static int bk_pick(gkc_ctx* c, const uint64_t* d_scan, const std::vector<uint64_t>& h_at, std::vector<uint64_t>& h_out)
{
    const uint32_t n = (uint32_t)h_at.size();
    DevBuf d_at, d_out;
    GKC_TRY(c->ensure(d_at, (size_t)n * 8)); GKC_TRY(c->ensure(d_out, (size_t)n * 8));
    h_out.assign(n, 0);
    GKC_HIP(c, hipMemcpyAsync(d_at.p, h_at.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bk_pick, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_scan, (const uint64_t*)d_at.p, n, (uint64_t*)d_out.p);
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipMemcpyAsync(h_out.data(), d_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    GKC_HIP(c, hipStreamSynchronize(c->stream));                   // (h_at was read, h_out is filled, d_at / d_out go back to the pool)
    return GKC_OK;
}

template <int KW>
static int bk_merge(gkc_banks* b, uint32_t bank, std::vector<BkDataset>& ds /* [n_ds + 1], b_* and a_* filled */, uint64_t n_b)
{
    typedef typename KeyT<KW>::type key_t;
    gkc_ctx* c = b->ctx;
    const uint32_t n_ds = b->n_ds;
    uint64_t ta = 0, tb = 0;
    for (uint32_t d = 0; d <= n_ds; d++) {
        ds[d].ta_first = (uint32_t)ta; ds[d].tb_first = (uint32_t)tb;
        if (d < n_ds) { ta += (ds[d].a_n + BK_TILE - 1) / BK_TILE; tb += (ds[d].b_n + BK_TILE - 1) / BK_TILE; }
    }
    if (ta >= (1ull << 32) || tb >= (1ull << 32)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: more than 2^32 tiles of %d k-mers", BK_TILE);
    const uint32_t n_ta = (uint32_t)ta, n_tb = (uint32_t)tb;
    DevBuf d_ds, d_lb, d_dup, d_scan, d_sums, d_offs;
    GKC_TRY(c->ensure(d_ds, ((size_t)n_ds + 1) * sizeof(BkDataset)));
    GKC_TRY(c->ensure(d_lb, (size_t)n_b * 8)); GKC_TRY(c->ensure(d_dup, ((size_t)n_b + 3) / 4 * 4)); GKC_TRY(c->ensure(d_scan, ((size_t)n_b + 1) * 8));
    GKC_HIP(c, hipMemcpyAsync(d_ds.p, ds.data(), ((size_t)n_ds + 1) * sizeof(BkDataset), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL((k_bk_search_b<KW>), dim3(bk_grid(n_tb)), dim3(BK_THREADS), 0, c->stream, (const BkDataset*)d_ds.p, n_ds, n_tb, (const key_t*)b->keys.p, (uint64_t*)d_lb.p, (uint8_t*)d_dup.p);
    GKC_HIP(c, hipGetLastError());
    GKC_TRY(bk_scan(c, (const uint8_t*)d_dup.p, n_b, (uint64_t*)d_scan.p, d_sums, d_offs));
    // duplicates per dataset -> union sizes
    std::vector<uint64_t> at(n_ds + 1), dups;
    for (uint32_t d = 0; d <= n_ds; d++) at[d] = ds[d].b_first;
    GKC_TRY(bk_pick(c, (const uint64_t*)d_scan.p, at, dups));
    std::vector<uint64_t> n_off(n_ds + 1, 0);
    for (uint32_t d = 0; d < n_ds; d++) { ds[d].n_off = n_off[d]; n_off[d + 1] = n_off[d] + ds[d].a_n + ds[d].b_n - (dups[d + 1] - dups[d]); }
    ds[n_ds].n_off = n_off[n_ds];
    const uint64_t n_new = n_off[n_ds];
    // fresh arrays: the keys, a plane for every bank that has one, and the new bank's
    DevBuf nk; std::vector<DevBuf> np(b->nb_banks);
    GKC_TRY(c->ensure(nk, (size_t)n_new * sizeof(key_t)));
    BkPlanes P{};
    for (uint32_t p = 0; p < b->nb_banks; p++) {
        if (!b->planes[p].p && p != bank) continue;
        GKC_TRY(c->ensure(np[p], ((size_t)n_new + 3) / 4 * 16));          // (padded to whole 16-byte loads of k_bk_eval)
        P.in[p] = (const int32_t*)b->planes[p].p; P.out[p] = (int32_t*)np[p].p;
    }
    GKC_HIP(c, hipMemcpyAsync(d_ds.p, ds.data(), ((size_t)n_ds + 1) * sizeof(BkDataset), hipMemcpyHostToDevice, c->stream));
    if (n_ta) hipLaunchKernelGGL((k_bk_scatter_a<KW>), dim3(bk_grid(n_ta)), dim3(BK_THREADS), 0, c->stream, (const BkDataset*)d_ds.p, n_ds, n_ta, (const key_t*)b->keys.p, (const uint64_t*)d_scan.p, P, b->nb_banks, bank, (key_t*)nk.p);
    hipLaunchKernelGGL((k_bk_scatter_b<KW>), dim3(bk_grid(n_tb)), dim3(BK_THREADS), 0, c->stream, (const BkDataset*)d_ds.p, n_ds, n_tb, (const uint64_t*)d_lb.p, (const uint8_t*)d_dup.p, (const uint64_t*)d_scan.p, P, b->nb_banks, bank, (key_t*)nk.p);
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipStreamSynchronize(c->stream));                   // the old arrays and the scratch buffers go back to the pool
    b->keys = std::move(nk);
    for (uint32_t p = 0; p < b->nb_banks; p++) if (np[p].p) b->planes[p] = std::move(np[p]);
    b->off = n_off;
    return GKC_OK;
}

static int bk_fail_from(gkc_banks* b, gkc_ctx* src, int rc) { if (src != b->ctx) b->ctx->set_error(rc, "%s", src->err.msg.c_str()); return rc; }

extern "C" {

int gkc_banks_create(gkc_ctx* c, uint32_t nb_banks, gkc_banks** out)
{
    gkc_tun_refresh();
    if (!c || !out) return GKC_ERR_ARG;
    *out = nullptr;
    if (!c->configured) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_create: gkc_configure must be called first (the object remembers the model)");
    if (nb_banks < 1 || nb_banks > BK_MAX_BANKS) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_create: nb_banks %u not in [1, %u]", nb_banks, BK_MAX_BANKS);
    gkc_banks* b = new gkc_banks();
    b->ctx = c; b->nb_banks = nb_banks; b->key_words = c->key_words; b->nb_partitions = c->nb_partitions; b->nb_passes = c->nb_passes;
    b->n_ds = c->nb_partitions * c->nb_passes; b->model_hash = c->model_hash;
    b->planes.resize(nb_banks); b->off.assign((size_t)b->n_ds + 1, 0); b->added.assign((size_t)nb_banks * b->n_ds, 0); b->merged_epoch.assign(c->nb_passes, 0);
    gkc_ctx_child_add(c);
    {   // the device tables a query routes k-mers with
        const size_t nm = (size_t)1 << (2 * c->m);
        const bool freq = c->minimizer_type == GKC_MINIMIZER_FREQ;
        int rc = c->ensure(b->q_repart, nm * 2);
        if (rc == GKC_OK && freq) rc = c->ensure(b->q_mkey_lut, nm * 4);
        if (rc == GKC_OK && freq) rc = c->ensure(b->q_key2val, nm * 4);
        hipError_t e = hipSuccess;
        if (rc == GKC_OK) e = hipMemcpyAsync(b->q_repart.p, c->d_repart.p, nm * 2, hipMemcpyDeviceToDevice, c->stream);
        if (rc == GKC_OK && freq && e == hipSuccess) e = hipMemcpyAsync(b->q_mkey_lut.p, c->d_mkey_lut.p, nm * 4, hipMemcpyDeviceToDevice, c->stream);
        if (rc == GKC_OK && freq && e == hipSuccess) e = hipMemcpyAsync(b->q_key2val.p, c->d_key2val.p, nm * 4, hipMemcpyDeviceToDevice, c->stream);
        if (rc == GKC_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (rc == GKC_OK && e != hipSuccess) { c->set_error(GKC_ERR_HIP, "gkc_banks_create: copying the model's tables failed: %s", hipGetErrorString(e)); rc = GKC_ERR_HIP; }
        if (rc != GKC_OK) { delete b; gkc_ctx_child_release(c); return rc; }
        QueryModel& M = b->qmodel;
        M.k = c->k; M.m = c->m; M.nb_partitions = c->nb_partitions; M.nb_passes = c->nb_passes; M.key_words = c->key_words; M.freq_mode = freq ? 1 : 0; M.default_key = c->default_key;
        M.repart = (const uint16_t*)b->q_repart.p; M.mkey_lut = (const uint32_t*)b->q_mkey_lut.p; M.key2val = (const uint32_t*)b->q_key2val.p;
    }
    *out = b;
    return GKC_OK;
}
void gkc_banks_destroy(gkc_banks* b) { if (b) { gkc_ctx* c = b->ctx; (void)hipStreamSynchronize(c->stream); delete b; gkc_ctx_child_release(c); } }

int gkc_banks_add(gkc_banks* b, gkc_ctx* src, uint32_t bank)
{
    gkc_tun_refresh();
    if (!b || !src) return GKC_ERR_ARG;
    gkc_ctx* c = b->ctx;
    if (!src->configured || src->model_hash != b->model_hash || src->nb_partitions != b->nb_partitions || src->nb_passes != b->nb_passes || src->key_words != b->key_words)
        GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: the context's model (k, m, partitions, passes, minimizer order, repartition table) differs from the one the object was created with");
    if (src->device != c->device) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: the context counts on device %d, the object lives on device %d", src->device, c->device);
    if (src->amin != 1 || src->amax != 2147483647)
        GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: the context's solidity window is [%d, %d]: per-bank counts must be complete, count with the default [1, 2147483647] (solidity is decided by gkc_banks_evaluate)", src->amin, src->amax);
    if (bank >= b->nb_banks) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: bank %u >= nb_banks %u", bank, b->nb_banks);
    if (src->in_pass || gkc_stage_b_in_flight(src)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: a pass of the context is open or still counting (gkc_finish_pass / gkc_finish_pass_wait first)");
    { const int rc = gkc_require_resident(src, "gkc_banks_add"); if (rc != GKC_OK) return bk_fail_from(b, src, rc); }
    GKC_HIP(c, hipSetDevice(c->device));
    // which passes hold results that are not merged yet
    std::vector<uint8_t> take(b->nb_passes, 0);
    bool any_done = false, any_new = false;
    for (uint32_t ps = 0; ps < b->nb_passes; ps++) {
        bool done = false;
        for (uint32_t pt = 0; pt < b->nb_partitions; pt++) done = done || src->datasets[(size_t)ps * b->nb_partitions + pt].done;
        if (!done) continue;
        any_done = true;
        if (src->pass_epoch[ps] == b->merged_epoch[ps]) continue;       // merged by an earlier call (passes added one by one)
        take[ps] = 1; any_new = true;
    }
    if (!any_done) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: the context has no finished dataset");
    if (!any_new) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: every finished dataset of the context was added already (bank %u: a (bank, dataset) pair is added once — count the next bank first)", bank);
    std::vector<BkDataset> ds((size_t)b->n_ds + 1, BkDataset{});
    uint64_t n_b = 0;
    for (uint32_t d = 0; d < b->n_ds; d++) {
        ds[d].a_off = b->off[d]; ds[d].a_n = b->off[d + 1] - b->off[d]; ds[d].b_first = n_b;
        const Dataset& S = src->datasets[d];
        if (!take[d / b->nb_partitions] || !S.done) continue;
        if (b->added[(size_t)bank * b->n_ds + d]) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: dataset %u of bank %u was added already (a (bank, dataset) pair is added once)", d, bank);
        if (S.n_solid != S.n_distinct) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_add: dataset %u holds %llu of its %llu distinct k-mers: per-bank counts must be complete", d, (unsigned long long)S.n_solid, (unsigned long long)S.n_distinct);
        ds[d].b_recs = (const uint8_t*)S.d_counts; ds[d].b_n = S.n_solid; n_b += S.n_solid;
    }
    ds[b->n_ds].a_off = b->off[b->n_ds]; ds[b->n_ds].b_first = n_b;
    if (src != c) (void)hipStreamSynchronize(src->stream);
    b->qidx.drop();                                                // the merge replaces the key array the index samples
    if (n_b) {
        ScopedTimer tm(c, "banks_add");
        GKC_TRY(b->key_words == 1 ? bk_merge<1>(b, bank, ds, n_b) : bk_merge<2>(b, bank, ds, n_b));
    }
    for (uint32_t d = 0; d < b->n_ds; d++) if (take[d / b->nb_partitions] && src->datasets[d].done) b->added[(size_t)bank * b->n_ds + d] = 1;
    for (uint32_t ps = 0; ps < b->nb_passes; ps++) if (take[ps]) b->merged_epoch[ps] = src->pass_epoch[ps];
    b->evaluated = false;
    return GKC_OK;
}

int gkc_banks_evaluate(gkc_banks* b, int kind, const int32_t* amin, const int32_t* amax, const uint8_t* solid_vec, uint32_t histo_max)
{
    gkc_tun_refresh();
    if (!b) return GKC_ERR_ARG;
    gkc_ctx* c = b->ctx;
    if (kind < GKC_SOLIDITY_SUM || kind > GKC_SOLIDITY_CUSTOM) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_evaluate: solidity kind %d unknown (GKC_SOLIDITY_*)", kind);
    if (!amin || !amax) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_evaluate: amin and amax hold one value per bank");
    if (kind == GKC_SOLIDITY_CUSTOM && !solid_vec) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_evaluate: kind custom needs solid_vec (one value per bank)");
    if (histo_max < 1 || histo_max > (1u << 24)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_evaluate: histo_max out of range");
    GKC_HIP(c, hipSetDevice(c->device));
    ScopedTimer tm(c, "banks_evaluate");
    b->evaluated = false;
    BkEval E{};
    for (uint32_t p = 0; p < b->nb_banks; p++) { E.plane[p] = (const int32_t*)b->planes[p].p; E.amin[p] = amin[p]; E.amax[p] = amax[p]; E.solid[p] = solid_vec ? solid_vec[p] : 0; }
    const size_t bins = (size_t)histo_max + 1;
    GKC_TRY(c->ensure(b->d_histo, bins * 8));
    GKC_HIP(c, hipMemsetAsync(b->d_histo.p, 0, bins * 8, c->stream));
    b->histo_max = histo_max;
    const uint64_t n = b->n_total();
    b->solid_off.assign((size_t)b->n_ds + 1, 0);
    if (n) {
        DevBuf d_solid, d_sum, d_scan, d_sums, d_offs;
        GKC_TRY(c->ensure(d_solid, ((size_t)n + 3) / 4 * 4)); GKC_TRY(c->ensure(d_sum, ((size_t)n + 3) / 4 * 16)); GKC_TRY(c->ensure(d_scan, ((size_t)n + 1) * 8));
        const uint32_t lds_bins = bins <= BK_LDS_BINS ? (uint32_t)bins : 0u;
        // few, long-lived workgroups: each flushes its LDS histogram once (40 KB at the default 10001 bins: four workgroups per CU)
        const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + BK_TILE - 1) / BK_TILE, 256 * 4));
        hipLaunchKernelGGL(k_bk_eval, dim3(grid), dim3(BK_THREADS), (size_t)lds_bins * 4, c->stream, E, b->nb_banks, n, kind, (uint8_t*)d_solid.p, (int32_t*)d_sum.p,
                           (unsigned long long*)b->d_histo.p, histo_max, lds_bins);
        GKC_HIP(c, hipGetLastError());
        GKC_TRY(bk_scan(c, (const uint8_t*)d_solid.p, n, (uint64_t*)d_scan.p, d_sums, d_offs));
        GKC_TRY(bk_pick(c, (const uint64_t*)d_scan.p, b->off, b->solid_off));
        const uint64_t n_solid = b->solid_off[b->n_ds];
        const size_t rb = b->key_words == 1 ? 16 : 32;
        GKC_TRY(c->ensure(b->out_counts, (size_t)n_solid * rb)); GKC_TRY(c->ensure(b->out_vectors, (size_t)n_solid * b->nb_banks * 4));
        const unsigned ggrid = bk_grid((n + BK_THREADS - 1) / BK_THREADS);
        if (b->key_words == 1) hipLaunchKernelGGL((k_bk_gather<1>), dim3(ggrid), dim3(BK_THREADS), 0, c->stream, (const uint64_t*)b->keys.p, E, b->nb_banks, n, (const uint8_t*)d_solid.p, (const int32_t*)d_sum.p,
                                                  (const uint64_t*)d_scan.p, (uint64_t*)b->out_counts.p, (int32_t*)b->out_vectors.p);
        else                   hipLaunchKernelGGL((k_bk_gather<2>), dim3(ggrid), dim3(BK_THREADS), 0, c->stream, (const u128*)b->keys.p, E, b->nb_banks, n, (const uint8_t*)d_solid.p, (const int32_t*)d_sum.p,
                                                  (const uint64_t*)d_scan.p, (uint64_t*)b->out_counts.p, (int32_t*)b->out_vectors.p);
        GKC_HIP(c, hipGetLastError());
    }
    GKC_HIP(c, hipStreamSynchronize(c->stream));                   // the scratch buffers go back to the pool
    b->evaluated = true;
    return GKC_OK;
}

static int bk_readable(gkc_banks* b, uint32_t dataset, const char* who)
{
    gkc_ctx* c = b->ctx;
    if (!b->evaluated) GKC_FAIL(c, GKC_ERR_ARG, "%s: no evaluation to read (gkc_banks_evaluate first; gkc_banks_add invalidates the last one)", who);
    if (dataset >= b->n_ds) GKC_FAIL(c, GKC_ERR_ARG, "%s: dataset %u >= %u", who, dataset, b->n_ds);
    return GKC_OK;
}
int gkc_banks_partition_info(gkc_banks* b, uint32_t dataset, uint64_t* n_solid, uint64_t* n_distinct)
{
    if (!b) return GKC_ERR_ARG;
    GKC_TRY(bk_readable(b, dataset, "gkc_banks_partition_info"));
    if (n_solid) *n_solid = b->solid_off[dataset + 1] - b->solid_off[dataset];
    if (n_distinct) *n_distinct = b->off[dataset + 1] - b->off[dataset];
    return GKC_OK;
}
static int bk_fetch(gkc_banks* b, uint32_t dataset, const DevBuf& from, size_t row_bytes, void* out, uint64_t cap, uint64_t* n_solid, const char* who)
{
    gkc_ctx* c = b->ctx;
    GKC_TRY(bk_readable(b, dataset, who));
    const uint64_t first = b->solid_off[dataset], n = b->solid_off[dataset + 1] - first;
    if (n_solid) *n_solid = n;
    if (cap < n) GKC_FAIL(c, GKC_ERR_CAPACITY, "%s: dataset holds %llu records, buffer %llu", who, (unsigned long long)n, (unsigned long long)cap);
    if (!n) return GKC_OK;
    if (!out) GKC_FAIL(c, GKC_ERR_ARG, "%s: no output buffer", who);
    GKC_HIP(c, hipSetDevice(c->device));
    GKC_HIP(c, hipMemcpyAsync(out, (const uint8_t*)from.p + (size_t)first * row_bytes, (size_t)n * row_bytes, hipMemcpyDeviceToHost, c->stream));
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}
int gkc_banks_partition_counts(gkc_banks* b, uint32_t dataset, void* out_counts, uint64_t cap_records, uint64_t* n_solid)
{
    if (!b) return GKC_ERR_ARG;
    return bk_fetch(b, dataset, b->out_counts, b->key_words == 1 ? 16 : 32, out_counts, cap_records, n_solid, "gkc_banks_partition_counts");
}
int gkc_banks_partition_vectors(gkc_banks* b, uint32_t dataset, int32_t* out, uint64_t cap_records, uint64_t* n_solid)
{
    if (!b) return GKC_ERR_ARG;
    return bk_fetch(b, dataset, b->out_vectors, (size_t)b->nb_banks * 4, out, cap_records, n_solid, "gkc_banks_partition_vectors");
}
int gkc_banks_partition_counts_device(gkc_banks* b, uint32_t dataset, const void** d_counts, const int32_t** d_vectors, uint64_t* n_solid)
{
    if (!b) return GKC_ERR_ARG;
    GKC_TRY(bk_readable(b, dataset, "gkc_banks_partition_counts_device"));
    const uint64_t first = b->solid_off[dataset];
    if (d_counts) *d_counts = (const uint8_t*)b->out_counts.p + (size_t)first * (b->key_words == 1 ? 16 : 32);
    if (d_vectors) *d_vectors = (const int32_t*)b->out_vectors.p + (size_t)first * b->nb_banks;
    if (n_solid) *n_solid = b->solid_off[dataset + 1] - first;
    return GKC_OK;
}
// the k-mers of reads against the merged state: the search of gkc_query_reads_device over the bare key array (gkc_query.hip), then the planes
int gkc_query_banks_reads_device(gkc_banks* b, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, int32_t* d_sum, int32_t* d_vectors)
{
    gkc_tun_refresh();
    if (!b) return GKC_ERR_ARG;
    gkc_ctx* c = b->ctx;
    GKC_HIP(c, hipSetDevice(c->device));
    if (!b->qidx.valid || b->qidx.stride != gkc_tun().query_index_stride) {
        std::vector<QHostDs> ds(b->n_ds);
        for (uint32_t d = 0; d < b->n_ds; d++) ds[d] = QHostDs{(const uint8_t*)b->keys.p + (size_t)b->off[d] * b->key_bytes(), b->off[d + 1] - b->off[d], b->off[d]};
        GKC_TRY(gkc_query_index_build(c, b->qidx, ds, b->key_words, true));
    }
    const int32_t* planes[BK_MAX_BANKS];
    for (uint32_t p = 0; p < b->nb_banks; p++) planes[p] = (const int32_t*)b->planes[p].p;
    return gkc_query_reads_run(c, b->qmodel, b->qidx, planes, b->nb_banks, d_bases, d_offsets, n_reads, n_bases, d_sum, d_vectors, "gkc_query_banks_reads_device");
}
int gkc_banks_histogram(gkc_banks* b, uint64_t* out, uint32_t n_bins)
{
    if (!b) return GKC_ERR_ARG;
    gkc_ctx* c = b->ctx;
    if (!b->evaluated) GKC_FAIL(c, GKC_ERR_ARG, "gkc_banks_histogram: no evaluation to read (gkc_banks_evaluate first; gkc_banks_add invalidates the last one)");
    if (!out || n_bins < b->histo_max + 1) GKC_FAIL(c, GKC_ERR_CAPACITY, "gkc_banks_histogram: the histogram has %u bins", b->histo_max + 1);
    GKC_HIP(c, hipSetDevice(c->device));
    GKC_HIP(c, hipMemcpyAsync(out, b->d_histo.p, ((size_t)b->histo_max + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}

}  // extern "C"
