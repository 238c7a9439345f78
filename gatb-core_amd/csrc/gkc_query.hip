// gkc_query.hip — abundance queries: the k-mers of reads (or bare k-mer values) looked up in the counted results where they lie (include/gkc.h, "abundance queries").
//
// A k-mer's dataset is a pure function of the k-mer: its minimizer -> repart[minimizer] is the partition, minimizer % nb_passes the pass (the routing of Stage A:
// Sequence2SuperKmer.hpp:81-159, SortingCountAlgorithm.cpp:1083), and every dataset d = part + pass * nb_partitions is an ascending Count[] in HBM. So a query is
//   canonical k-mer -> minimizer order key over its k-m+1 m-mers (the default minimizer takes part, Model.hpp:1254-1287) -> dataset -> search.
//
//   k_q_reads  : position-parallel over tiles of QR_TILE k-mer start positions of the flat read buffer, like k_scan_tile: one workgroup per tile, ASCII read once with
//                16-byte loads into 2-bit planes + an invalid mask in LDS, the m-mer order keys computed per position into LDS (lexicographic / KMC2: ALU only; frequency
//                order: one gather from d_mkey_lut), the window minimum by the shared-core + prefix / suffix scheme of Stage A, validity from the read-start and invalid
//                bit planes. Unlike Stage A the k-mer integer IS formed here (from the big-endian plane), canonicalised in registers.
//   k_q_kmers  : one thread per key; the m-mers come out of the key by shifts; the same routing and search.
//                The kernel has three modes (QM_COUNTS, QM_BANKS, QM_NODES of gkc_query.hpp): everything up to the search is shared, the answer step differs. QM_NODES
//                (gkc_graph_reads_nodes_device, gkc_paths.hip) gathers the placement of the record found and stores 8 x 16 B of nodes and 4 x 16 B of positions.
//   search     : a sampled index — the key of every S-th record of every dataset in one compact array (QueryIndex, S = GKC_QUERY_INDEX_STRIDE, default 256) — is searched
//                first (small enough to stay in the Infinity Cache), the remaining <= log2(S) steps stay inside one window of S records. A thread runs the searches of two
//                positions in lock step so that two independent loads are in flight per lane.
//   k_q_index  : builds the sample array (one thread per sample).
//   k_q_summary: per read n_valid / n_found / min / max / sum of an abundance array, one wave per read.
// The merged state of a gkc_banks is searched the same way over its bare key array; the found position then indexes the per-bank planes (sum, optionally the rows).
// Element indices are 64-bit; grids are capped and the kernels stride.
// The dataset table, the routing (q_mmer_key, q_dataset_of) and the search (q_search) live in gkc_query.hpp: gkc_graph.hip searches the same results.
#include "gkc_common.hpp"
#include "gkc_device.hpp"
#include "gkc_query.hpp"

constexpr int QR_THREADS = 256, QR_PER_THREAD = 16;
constexpr int QR_TILE = QR_THREADS * QR_PER_THREAD;          // k-mer start positions per tile
constexpr int QR_HALO_WORDS = 4;                             // 64 bases of look-ahead (k <= 63)
constexpr int QR_WORDS = QR_TILE / 16 + QR_HALO_WORDS;       // 16-base words per tile
constexpr int QR_PAD = 12;                                   // zero words behind the planes: k-mer extraction and the key step read past the halo
constexpr int QR_LOCKSTEP = 2;                               // searches a thread advances together (measured 1 / 2 / 4 / 8: 234 / 222 / 305 / 278 ms)
static_assert(QR_PER_THREAD == 16, "a thread owns one 16-base word of positions");
#define QMKI(p) ((p) + ((p) >> 4))                            // per-position LDS arrays: lane stride 17 words (see MKI in gkc_scan.hip)

// what a found record answers: its abundance (Count records) or the sum of its counts over the banks (+ the row)
template <typename K, bool BANKS>
__device__ __forceinline__ int32_t q_answer(const QParams& P, const QPlanes& PL, bool found, const uint8_t* recs, uint64_t pos, uint64_t base, uint64_t g)
{
    if constexpr (!BANKS) return found ? *reinterpret_cast<const int32_t*>(recs + pos * (2 * sizeof(K)) + sizeof(K)) : 0;
    int32_t sum = 0;
    for (uint32_t p = 0; p < P.nb_banks; p++) {
        const int32_t v = (found && PL.plane[p]) ? PL.plane[p][base + pos] : 0;
        sum += v;
        if (P.vectors) P.vectors[g * P.nb_banks + p] = v;
    }
    return sum;
}

// ------------------------------------------------------------------------------------------------ reads
template <int KW, int MODE>
__global__ __launch_bounds__(QR_THREADS) void k_q_reads(QParams P, typename QExtra<MODE>::type PL)
{
    typedef typename KeyT<KW>::type key_t;
    constexpr bool BANKS = MODE == QM_BANKS, NODES = MODE == QM_NODES;
    constexpr int RB = BANKS ? (int)sizeof(key_t) : 2 * (int)sizeof(key_t);
    __shared__ uint32_t s_be[QR_WORDS + QR_PAD];
    __shared__ uint32_t s_le[QR_WORDS + QR_PAD];
    __shared__ uint16_t s_bad[QR_WORDS + 8];
    __shared__ uint32_t s_rs[QR_TILE / 32 + 8];
    __shared__ uint32_t s_mk[QMKI(QR_TILE + 16 * QR_HALO_WORDS + 16)];
    static_assert(QR_WORDS <= 2 * QR_THREADS && QR_TILE / 32 + 8 <= QR_THREADS, "one or two words and one read-start word per thread");

    const int t = threadIdx.x;
    const uint32_t k = P.k, m = P.m;
    if (t < QR_PAD) { s_be[QR_WORDS + t] = 0; s_le[QR_WORDS + t] = 0; }
    if (t < 8) s_bad[QR_WORDS + t] = 0;

    for (uint64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * QR_TILE;
        __syncthreads();                                       // LDS of the previous tile fully consumed
        // ---- ASCII -> bit planes (A1) ----
        for (int w = t; w < QR_WORDS; w += QR_THREADS) {
            uint32_t dw[4], le, bad;
            load16(P.bases, t0 + 16ull * w, P.n_bases, dw);
            encode16(dw, le, bad);
            s_be[w] = rev2bit(le); s_le[w] = le; s_bad[w] = (uint16_t)bad;
        }
        if (t < QR_TILE / 32 + 8) s_rs[t] = P.rsbits[t0 / 32 + t];
        __syncthreads();

        // ---- order key of the m-mer starting at every position (as step 1 of k_scan_tile) ----
        for (int w = t; w < QR_WORDS; w += QR_THREADS) {
            const uint32_t xh = s_be[w], xl = s_be[w + 1], yl = s_le[w], yh = s_le[w + 1];
            const uint32_t fsh = 32u - 2u * m, rcx = 0xAAAAAAAAu & P.mmask;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t f32 = j ? __builtin_amdgcn_alignbit(xh, xl, 32 - 2 * j) : xh;
                const uint32_t fw = f32 >> fsh;
                uint32_t key;
                if (P.freq_mode) key = P.mkey_lut[fw];
                else {
                    const uint32_t rc = ((j ? __builtin_amdgcn_alignbit(yh, yl, 2 * j) : yl) & P.mmask) ^ rcx;
                    const uint32_t c = fw < rc ? fw : rc;
                    uint32_t a = ~(c | (c >> 2));
                    a = (a >> 1) & a & P.mask_ma1;
                    key = a ? P.mmask : c;
                }
                s_mk[17 * w + j] = key;
            }
        }
        __syncthreads();

        // ---- minimizer = window minimum of nb_mm keys, the default minimizer taking part (as step 2 of k_scan_tile) ----
        const int p0 = 16 * t;
        const uint32_t Wn = P.nb_mm;
        uint32_t mz[16];
        if (Wn >= 16) {
            const uint32_t* mk_t = s_mk + 17 * t;
            uint32_t core = P.default_key;
            for (uint32_t i = 15; i < Wn; i++) { const uint32_t v = mk_t[i + (i >> 4)]; core = v < core ? v : core; }
            uint32_t suf = 0xFFFFFFFFu, sufL[16];
            sufL[15] = suf;
#pragma unroll
            for (int j = 14; j >= 0; j--) { const uint32_t v = mk_t[j]; suf = v < suf ? v : suf; sufL[j] = suf; }
            uint32_t pre = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t r = sufL[j] < core ? sufL[j] : core;
                mz[j] = pre < r ? pre : r;
                const uint32_t i = Wn + (uint32_t)j;
                const uint32_t v = mk_t[i + (i >> 4)]; pre = v < pre ? v : pre;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                uint32_t best = P.default_key;
                for (uint32_t i = 0; i < Wn; i++) { const uint32_t v = s_mk[QMKI(p0 + j + i)]; best = v < best ? v : best; }
                mz[j] = best;
            }
        }

        // ---- which of the thread's 16 positions start a k-mer, and which of those are valid (A2; as step 3 of k_scan_tile) ----
        uint32_t validmask;
        {
            const int q = t >> 1, off = (t & 1) * 16;
            uint64_t rlo = (uint64_t)s_rs[q] | ((uint64_t)s_rs[q + 1] << 32);
            uint64_t rhi = (uint64_t)s_rs[q + 2] | ((uint64_t)s_rs[q + 3] << 32);
            if (off) { rlo = (rlo >> 16) | (rhi << 48); rhi >>= 16; }
            rlo = (rlo >> 1) | (rhi << 63); rhi >>= 1;        // read starts matter inside (g, g+k-1]: shift by one, window k-1
            const uint64_t blo = (uint64_t)s_bad[t] | ((uint64_t)s_bad[t + 1] << 16) | ((uint64_t)s_bad[t + 2] << 32) | ((uint64_t)s_bad[t + 3] << 48);
            const uint64_t bhi = (uint64_t)s_bad[t + 4] | ((uint64_t)s_bad[t + 5] << 16) | ((uint64_t)s_bad[t + 6] << 32) | ((uint64_t)s_bad[t + 7] << 48);
            // bits j = 0..15: OR of input bits j .. j+len-1 (len in [0, 63]); the set bits are sparse (one read start per read, invalid letters are rare)
            auto window_or16 = [](uint64_t lo, uint64_t hi, uint32_t len) -> uint32_t {
                if (len == 0) return 0u;
                uint32_t acc = 0;
                const uint32_t top = 15u + len;
                uint64_t w = top >= 64 ? lo : (lo & ((1ULL << top) - 1));
                while (w) {
                    const uint32_t b = (uint32_t)__builtin_ctzll(w); w &= w - 1;
                    const uint32_t j1 = b < 15u ? b : 15u, j0 = b + 1u > len ? b + 1u - len : 0u;
                    acc |= ((2u << j1) - 1u) & ~((1u << j0) - 1u);
                }
                if (top > 64) {
                    uint64_t v = hi & ((1ULL << (top - 64)) - 1);
                    while (v) {
                        const uint32_t b = 64u + (uint32_t)__builtin_ctzll(v); v &= v - 1;
                        const uint32_t j0 = b + 1u - len;
                        if (j0 <= 15u) acc |= 0xFFFFu & ~((1u << j0) - 1u);
                    }
                }
                return acc & 0xFFFFu;
            };
            const uint32_t rsany = window_or16(rlo, rhi, k - 1);
            const uint32_t badany = window_or16(blo, bhi, k);
            const long long lim = (long long)P.n_bases - (long long)k - (long long)(t0 + p0);      // last j whose k-mer still fits into the buffer
            const uint32_t fits = lim >= 15 ? 0xFFFFu : (lim < 0 ? 0u : ((2u << (uint32_t)lim) - 1u));
            validmask = ~rsany & fits & ~badany;
        }

        // ---- canonical k-mer, dataset, search: QR_LOCKSTEP positions at a time ----
        int32_t res[NODES ? 1 : 16];
        uint64_t node[NODES ? 16 : 1]; uint32_t npos[NODES ? 16 : 1];      // QM_NODES: unitig << 1 | strand or a GKC_NODE_* sentinel, and the position in the unitig
        const uint64_t g0 = t0 + (uint64_t)p0;
#pragma unroll
        for (int j0 = 0; j0 < 16; j0 += QR_LOCKSTEP) {
            bool act[QR_LOCKSTEP], found[QR_LOCKSTEP]; uint32_t d[QR_LOCKSTEP]; key_t key[QR_LOCKSTEP]; uint64_t pos[QR_LOCKSTEP], base[QR_LOCKSTEP];
            const uint8_t* recs[QR_LOCKSTEP];
            bool flip[QR_LOCKSTEP];                            // QM_NODES: the read spells the reverse complement of the record
#pragma unroll
            for (int u = 0; u < QR_LOCKSTEP; u++) {
                const int j = j0 + u;
                act[u] = (validmask >> j) & 1u;
                // 32 (64) nucleotides from position p0 + j of the big-endian plane; the k-mer is their top 2k bits (first nucleotide most significant, Model.hpp:637-657)
                const int sh = 2 * j;
                uint64_t A[KW + 1];
#pragma unroll
                for (int i = 0; i <= KW; i++) A[i] = ((uint64_t)s_be[t + 2 * i] << 32) | s_be[t + 2 * i + 1];
                key_t fw;
                if constexpr (KW == 1) fw = (key_t)((sh ? ((A[0] << sh) | (A[1] >> (64 - sh))) : A[0]) >> (64u - 2u * k));
                else {
                    const uint64_t B0 = sh ? ((A[0] << sh) | (A[1] >> (64 - sh))) : A[0], B1 = sh ? ((A[1] << sh) | (A[KW] >> (64 - sh))) : A[1];
                    fw = (key_t)(((((u128)B0) << 64) | (u128)B1) >> (128u - 2u * k));
                }
                const key_t rv = KeyT<KW>::revcomp(fw, k);
                key[u] = fw < rv ? fw : rv;                    // Model.hpp:294
                if constexpr (NODES) flip[u] = rv < fw;        // (a palindrome stands forward)
                d[u] = q_dataset_of(P, mz[j]);
            }
            q_search<key_t, RB, QR_LOCKSTEP>(P, act, d, key, found, pos, recs, base);
#pragma unroll
            for (int u = 0; u < QR_LOCKSTEP; u++) {
                const uint64_t g = g0 + (uint64_t)(j0 + u);
                if constexpr (NODES) {
                    // the record's placement (unitig << 1 | reversed, ~0: a record of no unitig) with the strand the read spells it on
                    const bool hit = act[u] && found[u];
                    const uint64_t i = base[u] + pos[u], U = hit ? PL.unitig[i] : ~0ull;
                    const bool placed = hit && U != ~0ull;
                    node[j0 + u] = !act[u] ? GKC_NODE_NO_KMER : (!found[u] ? GKC_NODE_ABSENT : (placed ? (U ^ (flip[u] ? 1ull : 0ull)) : GKC_NODE_REMOVED));
                    npos[j0 + u] = (placed && PL.out_pos) ? PL.pos[i] : 0u;
                } else if (BANKS) { if (g < P.n_bases) { const int32_t s = q_answer<key_t, true>(P, PL, act[u] && found[u], recs[u], pos[u], base[u], g); res[j0 + u] = act[u] ? s : -1; } else res[j0 + u] = -1; }
                else res[j0 + u] = act[u] ? q_answer<key_t, false>(P, PL, found[u], recs[u], pos[u], base[u], g) : -1;
            }
        }
        // ---- out[g] for the positions of the buffer ----
        if constexpr (NODES) {
            if (g0 + 16 <= P.n_bases) {                        // (g0 is a multiple of 16 and the arrays start 16-byte aligned)
                ulonglong2* o = reinterpret_cast<ulonglong2*>(PL.out_node + g0);
#pragma unroll
                for (int q = 0; q < 8; q++) o[q] = make_ulonglong2(node[2 * q], node[2 * q + 1]);
                if (PL.out_pos) {
                    uint4* op = reinterpret_cast<uint4*>(PL.out_pos + g0);
#pragma unroll
                    for (int q = 0; q < 4; q++) op[q] = make_uint4(npos[4 * q], npos[4 * q + 1], npos[4 * q + 2], npos[4 * q + 3]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; j++) if (g0 + j < P.n_bases) { PL.out_node[g0 + j] = node[j]; if (PL.out_pos) PL.out_pos[g0 + j] = npos[j]; }
            }
        } else if (g0 + 16 <= P.n_bases) {
            int4* o = reinterpret_cast<int4*>(P.out + g0);     // (g0 is a multiple of 16 and the array starts 16-byte aligned)
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = make_int4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) if (g0 + j < P.n_bases) P.out[g0 + j] = res[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ keys
template <int KW>
__global__ __launch_bounds__(256) void k_q_kmers(QParams P, const uint8_t* __restrict__ keys, uint64_t n, uint32_t stride, unsigned long long* __restrict__ first_bad)
{
    typedef typename KeyT<KW>::type key_t;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t* w = reinterpret_cast<const uint64_t*>(keys + i * stride);
        key_t x = (key_t)w[0];
        if constexpr (KW == 2) x |= (key_t)(((u128)w[1]) << 64);
        if ((x >> (2u * P.k)) != 0) { atomicMin(first_bad, (unsigned long long)i); P.out[i] = 0; continue; }
        const key_t rv = KeyT<KW>::revcomp(x, P.k);
        const key_t cn = x < rv ? x : rv;
        uint32_t best = P.default_key;
        for (uint32_t j = 0; j < P.nb_mm; j++) {
            const uint32_t key = q_mmer_key(P, (uint32_t)(cn >> (2u * (P.k - P.m - j))) & P.mmask);
            best = key < best ? key : best;
        }
        const bool act[1] = {true}; const uint32_t d[1] = {q_dataset_of(P, best)}; const key_t key[1] = {cn};
        bool found[1]; uint64_t pos[1], base[1]; const uint8_t* recs[1];
        q_search<key_t, 2 * (int)sizeof(key_t), 1>(P, act, d, key, found, pos, recs, base);
        P.out[i] = found[0] ? *reinterpret_cast<const int32_t*>(recs[0] + pos[0] * (2 * sizeof(key_t)) + sizeof(key_t)) : 0;
    }
}

// ------------------------------------------------------------------------------------------------ index
// sample s of the index = the key of record (s - idx_off) * stride of the dataset the sample belongs to: the last dataset with idx_off <= s (datasets without
// samples repeat the offset of the next one)
template <typename K, int RB>
__global__ __launch_bounds__(256) void k_q_index(const QDs* __restrict__ ds, uint32_t n_ds, uint64_t n_samples, uint64_t stride, K* __restrict__ samples)
{
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_samples; s += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_ds;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (ds[mid].idx_off <= s) lo = mid; else hi = mid; }
        const QDs D = ds[lo];
        samples[s] = q_load_key<K>(D.recs + (s - D.idx_off) * stride * (uint64_t)RB);
    }
}

// ------------------------------------------------------------------------------------------------ per-read summary
__global__ __launch_bounds__(256) void k_q_summary(const int32_t* __restrict__ abund, const uint64_t* __restrict__ offsets, uint64_t n_reads, gkc_read_abundance* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n_reads; r += n_waves) {
        const uint64_t b = offsets[r], e = offsets[r + 1];
        uint32_t nv = 0, nf = 0; int32_t mn = 2147483647, mx = 0; unsigned long long sum = 0;
        for (uint64_t g = b + lane; g < e; g += 64) {          // (e < b: nothing)
            const int32_t a = abund[g];
            if (a < 0) continue;
            nv++; nf += a > 0; mn = a < mn ? a : mn; mx = a > mx ? a : mx; sum += (unsigned long long)a;
        }
#pragma unroll
        for (int dlt = 32; dlt >= 1; dlt >>= 1) {
            nv += __shfl_xor(nv, dlt, 64); nf += __shfl_xor(nf, dlt, 64); sum += __shfl_xor(sum, dlt, 64);
            const int32_t a = __shfl_xor(mn, dlt, 64), c = __shfl_xor(mx, dlt, 64);
            mn = a < mn ? a : mn; mx = c > mx ? c : mx;
        }
        if (lane == 0) { gkc_read_abundance R; R.n_valid = nv; R.n_found = nf; R.min = nv ? mn : 0; R.max = mx; R.sum = sum; out[r] = R; }
    }
}

// ------------------------------------------------------------------------------------------------ host side
unsigned q_grid(uint64_t n_blocks) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_blocks, QR_GRID_MAX)); }

int gkc_query_index_build(gkc_ctx* c, QueryIndex& ix, const std::vector<QHostDs>& ds, uint32_t key_words, bool bare)
{
    ScopedTimer tm(c, "query_index");
    const uint64_t S = gkc_tun().query_index_stride;
    const uint32_t n_ds = (uint32_t)ds.size();
    const size_t kb = key_words == 1 ? 8 : 16;
    ix.drop();
    std::vector<QDs> h(std::max<size_t>(n_ds, 1), QDs{nullptr, 0, 0, 0, 0});
    uint64_t n_samples = 0;
    for (uint32_t d = 0; d < n_ds; d++) {
        h[d].recs = (const uint8_t*)ds[d].recs; h[d].n = ds[d].n; h[d].base = ds[d].base;
        h[d].idx_off = n_samples; h[d].idx_n = (ds[d].n + S - 1) / S; n_samples += h[d].idx_n;
    }
    GKC_TRY(c->ensure(ix.table, h.size() * sizeof(QDs)));
    GKC_TRY(c->ensure(ix.samples, (size_t)std::max<uint64_t>(n_samples, 1) * kb));      // (never empty: idle search slots load its first element)
    GKC_HIP(c, hipMemcpyAsync(ix.table.p, h.data(), h.size() * sizeof(QDs), hipMemcpyHostToDevice, c->stream));
    GKC_HIP(c, hipMemsetAsync(ix.samples.p, 0, kb, c->stream));
    if (n_samples) {
        const unsigned grid = q_grid((n_samples + 255) / 256);
        const QDs* t = (const QDs*)ix.table.p;
        if (key_words == 1) { if (bare) hipLaunchKernelGGL((k_q_index<uint64_t, 8>), dim3(grid), dim3(256), 0, c->stream, t, n_ds, n_samples, S, (uint64_t*)ix.samples.p);
                              else      hipLaunchKernelGGL((k_q_index<uint64_t, 16>), dim3(grid), dim3(256), 0, c->stream, t, n_ds, n_samples, S, (uint64_t*)ix.samples.p); }
        else                { if (bare) hipLaunchKernelGGL((k_q_index<u128, 16>), dim3(grid), dim3(256), 0, c->stream, t, n_ds, n_samples, S, (u128*)ix.samples.p);
                              else      hipLaunchKernelGGL((k_q_index<u128, 32>), dim3(grid), dim3(256), 0, c->stream, t, n_ds, n_samples, S, (u128*)ix.samples.p); }
        GKC_HIP(c, hipGetLastError());
    }
    GKC_HIP(c, hipStreamSynchronize(c->stream));               // (h was read)
    ix.stride = S; ix.valid = true;
    return GKC_OK;
}

void q_fill_params(QParams& P, const QueryModel& M, const QueryIndex& ix)
{
    P.k = M.k; P.m = M.m; P.nb_mm = M.k - M.m + 1;
    P.mmask = (uint32_t)((1ULL << (2 * M.m)) - 1);
    P.mask_ma1 = (uint32_t)(0x5555555555555555ULL & ((1ULL << ((M.m - 2) * 2)) - 1));
    P.freq_mode = M.freq_mode; P.mkey_lut = M.mkey_lut; P.key2val = M.key2val; P.default_key = M.default_key;
    P.repart = M.repart; P.nb_passes = M.nb_passes; P.nb_partitions = M.nb_partitions;
    P.ds = (const QDs*)ix.table.p; P.samples = ix.samples.p; P.stride = ix.stride;
}

int gkc_query_reads_run(gkc_ctx* c, const QueryModel& M, const QueryIndex& ix, const int32_t* const* planes, uint32_t nb_banks, const char* d_bases, const uint64_t* d_offsets,
                        uint64_t n_reads, uint64_t n_bases, int32_t* d_out, int32_t* d_vectors, const char* who, const QNodes* nodes)
{
    if (nodes) d_out = reinterpret_cast<int32_t*>(nodes->out_node);      // (the checks below are those of the one output every mode has)
    if (!d_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: offsets are required", who);
    if (n_bases && (!d_bases || !d_out)) GKC_FAIL(c, GKC_ERR_ARG, "%s: bases and the output array are required", who);
    if (((uintptr_t)d_bases & 15) != 0 || ((uintptr_t)d_out & 15) != 0 || (nodes && ((uintptr_t)nodes->out_pos & 15) != 0))
        GKC_FAIL(c, GKC_ERR_ARG, "%s: d_bases and the output array%s must be 16-byte aligned", who, nodes ? "s" : "");
    if (n_bases >= (1ULL << 40)) GKC_FAIL(c, GKC_ERR_ARG, "%s: a single query is limited to 2^40 bases", who);
    ScopedTimer tm(c, nodes ? "graph_read_nodes" : "query_reads");
    const uint64_t n_tiles = (n_bases + QR_TILE - 1) / QR_TILE;
    // read-start bitmask (+ slack so every tile can read its halo words); the offsets check of gkc_push_reads_device in its last word
    const size_t rs_words = (size_t)(n_tiles * QR_TILE / 32 + 64);
    DevBuf d_rs;
    GKC_TRY(c->ensure(d_rs, rs_words * 4));
    GKC_HIP(c, hipMemsetAsync(d_rs.p, 0, rs_words * 4, c->stream));
    GKC_TRY(gkc_launch_mark_read_starts(c, d_offsets, n_reads, n_bases, (uint32_t*)d_rs.p, (uint32_t*)d_rs.p + rs_words - 1));
    uint32_t bad_offsets = 0;
    GKC_HIP(c, hipMemcpyAsync(&bad_offsets, (uint32_t*)d_rs.p + rs_words - 1, 4, hipMemcpyDeviceToHost, c->stream));
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    if (bad_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: read offsets are not a CSR table of the bases (need offsets[0] == 0, non-decreasing, offsets[n_reads] == n_bases = %llu)", who, (unsigned long long)n_bases);
    if (!n_tiles) return GKC_OK;
    QParams P{}; q_fill_params(P, M, ix);
    P.bases = (const uint8_t*)d_bases; P.n_bases = n_bases; P.rsbits = (const uint32_t*)d_rs.p; P.n_tiles = n_tiles;
    P.out = d_out; P.vectors = d_vectors; P.nb_banks = nb_banks;
    QPlanes PL{};
    if (planes) for (uint32_t p = 0; p < nb_banks && p < Q_MAX_BANKS; p++) PL.plane[p] = planes[p];
    const dim3 grid(q_grid(n_tiles)), block(QR_THREADS);
    if (nodes)       { if (M.key_words == 1) hipLaunchKernelGGL((k_q_reads<1, QM_NODES>), grid, block, 0, c->stream, P, *nodes); else hipLaunchKernelGGL((k_q_reads<2, QM_NODES>), grid, block, 0, c->stream, P, *nodes); }
    else if (planes) { if (M.key_words == 1) hipLaunchKernelGGL((k_q_reads<1, QM_BANKS>), grid, block, 0, c->stream, P, PL); else hipLaunchKernelGGL((k_q_reads<2, QM_BANKS>), grid, block, 0, c->stream, P, PL); }
    else             { if (M.key_words == 1) hipLaunchKernelGGL((k_q_reads<1, QM_COUNTS>), grid, block, 0, c->stream, P, PL); else hipLaunchKernelGGL((k_q_reads<2, QM_COUNTS>), grid, block, 0, c->stream, P, PL); }
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipStreamSynchronize(c->stream));               // the mask goes back to the pool
    return GKC_OK;
}

// the guards of gkc_release_pass and of the whole-context consumers, then the index over what the context holds NOW
int q_prepare(gkc_ctx* c, const char* who)
{
    if (!c->configured) GKC_FAIL(c, GKC_ERR_ARG, "%s: gkc_configure must be called first", who);
    if (gkc_stage_b_in_flight(c)) GKC_FAIL(c, GKC_ERR_ARG, "%s while gkc_finish_pass_async is in flight (gkc_finish_pass_wait first)", who);
    if (c->in_pass) GKC_FAIL(c, GKC_ERR_ARG, "%s: pass %u is still open (gkc_finish_pass first)", who, c->pass);
    GKC_TRY(gkc_require_resident(c, who));
    for (size_t d = 0; d < c->datasets.size(); d++)
        if (!c->datasets[d].done) GKC_FAIL(c, GKC_ERR_ARG, "%s: partition %zu of pass %zu is not counted — a query needs every dataset of every pass (%u passes) finished", who,
                                           d % c->nb_partitions, d / c->nb_partitions, c->nb_passes);
    GKC_HIP(c, hipSetDevice(c->device));
    QueryIndex& ix = c->qidx;
    std::vector<std::pair<const void*, uint64_t>> sig(c->datasets.size());
    for (size_t d = 0; d < sig.size(); d++) sig[d] = {c->datasets[d].d_counts, c->datasets[d].n_solid};
    if (ix.valid && ix.stride == gkc_tun().query_index_stride && ix.epoch == c->pass_epoch && ix.sig == sig) return GKC_OK;
    std::vector<QHostDs> ds(sig.size());
    uint64_t first = 0;                                        // (the abundance queries do not read base; gkc_graph.hip finds the dataset of a flat record index by it)
    for (size_t d = 0; d < sig.size(); d++) { ds[d] = QHostDs{sig[d].first, sig[d].second, first}; first += sig[d].second; }
    GKC_TRY(gkc_query_index_build(c, ix, ds, c->key_words, false));
    ix.epoch = c->pass_epoch; ix.sig = std::move(sig);
    return GKC_OK;
}
QueryModel q_model_of(const gkc_ctx* c)
{
    QueryModel M{};
    M.k = c->k; M.m = c->m; M.nb_partitions = c->nb_partitions; M.nb_passes = c->nb_passes; M.key_words = c->key_words;
    M.freq_mode = c->minimizer_type == GKC_MINIMIZER_FREQ; M.default_key = c->default_key;
    M.mkey_lut = (const uint32_t*)c->d_mkey_lut.p; M.key2val = (const uint32_t*)c->d_key2val.p; M.repart = (const uint16_t*)c->d_repart.p;
    return M;
}

extern "C" {

int gkc_query_reads_device(gkc_ctx* c, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, int32_t* d_out)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    GKC_TRY(q_prepare(c, "gkc_query_reads_device"));
    return gkc_query_reads_run(c, q_model_of(c), c->qidx, nullptr, 0, d_bases, d_offsets, n_reads, n_bases, d_out, nullptr, "gkc_query_reads_device");
}

int gkc_query_reads(gkc_ctx* c, const char* bases, const uint64_t* offsets, uint64_t n_reads, int32_t* out)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (!offsets || offsets[0] != 0) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_reads: offsets[0] must be 0");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] < offsets[r]) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_reads: read offsets are not a CSR table of the bases (offsets[%llu] decreases)", (unsigned long long)(r + 1));
    const uint64_t n_bases = offsets[n_reads];
    if (n_bases && (!bases || !out)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_reads: bases and the output array are required");
    GKC_TRY(q_prepare(c, "gkc_query_reads"));
    DevBuf d_b, d_o, d_r;
    GKC_TRY(c->ensure(d_b, (size_t)n_bases + 64)); GKC_TRY(c->ensure(d_o, (size_t)(n_reads + 1) * 8)); GKC_TRY(c->ensure(d_r, (size_t)n_bases * 4 + 64));
    if (n_bases) GKC_HIP(c, hipMemcpyAsync(d_b.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, c->stream));
    GKC_HIP(c, hipMemcpyAsync(d_o.p, offsets, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    int rc = gkc_query_reads_run(c, q_model_of(c), c->qidx, nullptr, 0, (const char*)d_b.p, (const uint64_t*)d_o.p, n_reads, n_bases, (int32_t*)d_r.p, nullptr, "gkc_query_reads");
    if (rc == GKC_OK && n_bases) {
        hipError_t e = hipMemcpyAsync(out, d_r.p, (size_t)n_bases * 4, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { c->set_error(GKC_ERR_HIP, "gkc_query_reads: D2H copy failed: %s", hipGetErrorString(e)); rc = GKC_ERR_HIP; }
    }
    (void)hipStreamSynchronize(c->stream);                     // the caller's buffers were read / are filled, the scratch goes back to the pool
    return rc;
}

int gkc_query_kmers_device(gkc_ctx* c, const void* d_keys, uint64_t n, uint32_t stride, int32_t* d_out)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    GKC_TRY(q_prepare(c, "gkc_query_kmers_device"));
    const uint32_t need = c->key_words == 1 ? 8 : 16;
    if (stride < need || (stride % 8) != 0) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_kmers_device: stride %u invalid for k=%u (need a multiple of 8, >= %u)", stride, c->k, need);
    if (!n) return GKC_OK;
    if (!d_keys || !d_out || ((uintptr_t)d_keys & 7) != 0) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_kmers_device: keys (8-byte aligned) and the output array are required");
    unsigned long long first_bad = ~0ull;
    {
        ScopedTimer tm(c, "query_kmers");
        DevBuf d_bad;
        GKC_TRY(c->ensure(d_bad, 8));
        GKC_HIP(c, hipMemsetAsync(d_bad.p, 0xFF, 8, c->stream));
        QParams P{}; q_fill_params(P, q_model_of(c), c->qidx); P.out = d_out;
        const unsigned grid = q_grid((n + 255) / 256);
        if (c->key_words == 1) hipLaunchKernelGGL((k_q_kmers<1>), dim3(grid), dim3(256), 0, c->stream, P, (const uint8_t*)d_keys, n, stride, (unsigned long long*)d_bad.p);
        else                   hipLaunchKernelGGL((k_q_kmers<2>), dim3(grid), dim3(256), 0, c->stream, P, (const uint8_t*)d_keys, n, stride, (unsigned long long*)d_bad.p);
        GKC_HIP(c, hipGetLastError());
        GKC_HIP(c, hipMemcpyAsync(&first_bad, d_bad.p, 8, hipMemcpyDeviceToHost, c->stream));
        GKC_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (first_bad != ~0ull) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_kmers_device: key %llu is not a %u-mer (its value is >= 4^%u)", first_bad, c->k, c->k);
    return GKC_OK;
}

int gkc_query_kmers(gkc_ctx* c, const void* keys, uint64_t n, uint32_t stride, int32_t* out)
{
    if (!c) return GKC_ERR_ARG;
    if (n && (!keys || !out)) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_kmers: keys and the output array are required");
    GKC_HIP(c, hipSetDevice(c->device));
    DevBuf d_k, d_r;
    GKC_TRY(c->ensure(d_k, (size_t)n * stride + 16)); GKC_TRY(c->ensure(d_r, (size_t)n * 4 + 16));
    if (n) GKC_HIP(c, hipMemcpyAsync(d_k.p, keys, (size_t)n * stride, hipMemcpyHostToDevice, c->stream));
    int rc = gkc_query_kmers_device(c, d_k.p, n, stride, (int32_t*)d_r.p);
    if (rc == GKC_OK && n) {
        hipError_t e = hipMemcpyAsync(out, d_r.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { c->set_error(GKC_ERR_HIP, "gkc_query_kmers: D2H copy failed: %s", hipGetErrorString(e)); rc = GKC_ERR_HIP; }
    }
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int gkc_query_read_summary_device(gkc_ctx* c, const int32_t* d_abund, const uint64_t* d_offsets, uint64_t n_reads, gkc_read_abundance* d_out)
{
    if (!c) return GKC_ERR_ARG;
    if (!n_reads) return GKC_OK;
    if (!d_abund || !d_offsets || !d_out) GKC_FAIL(c, GKC_ERR_ARG, "gkc_query_read_summary_device: the abundance array, the offsets and the output array are required");
    GKC_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_q_summary, dim3(q_grid((n_reads + 3) / 4)), dim3(256), 0, c->stream, d_abund, d_offsets, n_reads, d_out);
    GKC_HIP(c, hipGetLastError());
    GKC_HIP(c, hipStreamSynchronize(c->stream));
    return GKC_OK;
}

}  // extern "C"
