// gkc_correct.hip — correction of the reads from the compacted graph they thread (include/gkc.h, "read paths": region, correction).
//
// gkc_graph_reads_correct_device works on what the neighbouring calls left in HBM: the flat read buffer, the segments of gkc_graph_reads_segments_device and the unitig
// strings of gkc_graph_unitigs_write. The bulk of the output is the input; the corrections are a sparse overlay on it.
//   k_correct_copy          : d_out = d_bases, 16 bytes per lane and trip, the bytes behind the last whole vector one by one. Not launched in place.
//   k_correct_unitig_offsets: one lane per unitig: offsets[u + 1] - offsets[u] == L_u + k - 1 against the placement's first[], offsets[0] == 0.
//   k_correct_check         : one lane per READ, looping over the read's segments (below: why a lane per read): everything the overlay relies on, flagged and never
//                             acted on — bad[0] two segments overlap or descend, bad[1] a segment runs past its read (or the read has 2^32 bases or more), bad[2] a node of
//                             no unitig, bad[3] a unitig range that leaves [0, L_u) or holds no k-mer. L_u comes from the unitig offsets (offsets[u + 1] is the neighbour of
//                             the entry the overlay needs anyway); k_correct_unitig_offsets has found them to be the placement's before this kernel starts.
//   k_correct_apply         : one lane per read. Head, the gap behind every segment, tail: a region is evaluated in two steps, the changes counted (the loop leaves at
//                             max_subst + 1), then, only when it is rewritten, the bytes that differ stored and their bits set (64-bit vector atomics on d_changed_bits,
//                             which was zeroed). A skipped region stores nothing. The seven counters stay in registers over all trips of the lane; a wave adds them up
//                             with shuffles at the end and its lane 0 issues one atomic per counter that is not zero.
// A lane per read, not a lane per segment: a lane needs its read's first base and length for every region, and a segment does not name its read. A lane per segment
// would search the segment offsets (log2(n_reads) dependent loads each) or read a table segment -> read that a further kernel has to write first; a lane per read has
// offsets[r], offsets[r + 1], seg_offsets[r], seg_offsets[r + 1] from four coalesced loads and walks its 24-byte segments, which lie next to those of the neighbouring
// lanes. The price is divergence: a wave takes as many trips as its read with the most segments.
// Element indices are 64-bit; grids go through q_grid and the kernels stride. Scratch comes from the context's pool on c->stream, is allocated before the first launch
// and synchronised before it goes back. The input and the output of k_correct_apply may be the same buffer: neither is __restrict__.
#include "gkc_unitigs.hpp"

constexpr int CR_THREADS = 256;                               // reads a workgroup handles per trip
constexpr int CR_VEC = 16;                                    // bytes a lane copies per trip

struct CrStats { unsigned long long v[7]; };                  // the order of gkc_correct_stats
enum { CR_GAPS_FIXED = 0, CR_GAPS_SKIPPED, CR_HEADS_FIXED, CR_TAILS_FIXED, CR_ENDS_SKIPPED, CR_ENDS_NO_ROOM, CR_BASES_CHANGED };

__global__ __launch_bounds__(CR_THREADS) void k_correct_copy(const char* __restrict__ in, char* __restrict__ out, uint64_t n_bases)
{
    const uint64_t n_vec = n_bases / CR_VEC;
    const uint4* __restrict__ vi = reinterpret_cast<const uint4*>(in); uint4* __restrict__ vo = reinterpret_cast<uint4*>(out);
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = t0; v < n_vec; v += step) vo[v] = vi[v];
    for (uint64_t g = n_vec * CR_VEC + t0; g < n_bases; g += step) out[g] = in[g];
}

__global__ __launch_bounds__(256) void k_correct_unitig_offsets(const uint64_t* __restrict__ uoff, const uint64_t* __restrict__ first, uint64_t n_alive, uint64_t n_unitigs, uint32_t k,
                                                                 uint32_t* __restrict__ bad)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && uoff[0] != 0) *bad = 1u;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_unitigs; u += (uint64_t)gridDim.x * blockDim.x)
        if (uoff[u + 1] - uoff[u] != ut_length(first, n_alive, n_unitigs, u) + (k - 1)) *bad = 1u;
}

// both CSR tables were checked: seg_offsets[r] <= seg_offsets[r + 1] <= n_segments, offsets[r] <= offsets[r + 1] <= n_bases
__global__ __launch_bounds__(CR_THREADS) void k_correct_check(const uint64_t* __restrict__ offsets, uint64_t n_reads, const uint64_t* __restrict__ seg_offsets,
                                                               const gkc_read_segment* __restrict__ segments, const uint64_t* __restrict__ uoff, uint64_t n_unitigs, uint32_t k,
                                                               uint32_t* __restrict__ bad)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t len = offsets[r + 1] - offsets[r], hi = seg_offsets[r + 1];
        if (len >= (1ull << 32)) bad[1] = 1u;
        uint64_t prev_end = 0;
        for (uint64_t s = seg_offsets[r]; s < hi; s++) {
            const gkc_read_segment A = segments[s];
            const uint64_t u = A.node >> 1;
            if ((uint64_t)A.read_pos < prev_end) bad[0] = 1u;
            prev_end = (uint64_t)A.read_pos + A.n_kmers;
            if (prev_end + (k - 1) > len) bad[1] = 1u;
            if (u >= n_unitigs) { bad[2] = 1u; continue; }
            const uint64_t L = uoff[u + 1] - uoff[u] - (k - 1);
            const bool inside = A.n_kmers != 0u && ((A.node & 1ull) ? (uint64_t)A.unitig_pos < L && (uint64_t)A.unitig_pos + 1 >= (uint64_t)A.n_kmers
                                                                    : (uint64_t)A.unitig_pos + A.n_kmers <= L);
            if (!inside) bad[3] = 1u;
        }
    }
}

__device__ __forceinline__ char cr_complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// The map of one segment: read position x -> the unitig base that stands there (strand 1: the complement of the mirrored base).
struct CrMap {
    const char* ub; int64_t at; bool rev;                      // strand 0: ub[at + x]; strand 1: complement(ub[at - x])
    __device__ __forceinline__ CrMap(const char* unitig_bases, uint64_t ubase, const gkc_read_segment& S, uint32_t k)
        : ub(unitig_bases + ubase), at((S.node & 1ull) ? (int64_t)S.unitig_pos + (int64_t)(k - 1) + (int64_t)S.read_pos : (int64_t)S.unitig_pos - (int64_t)S.read_pos), rev(S.node & 1ull) {}
    __device__ __forceinline__ char operator()(uint64_t x) const { return rev ? cr_complement(ub[at - (int64_t)x]) : ub[at + (int64_t)x]; }
};

// region [x0, x1) of the read whose first base is in[0] / out[0] (g0: its index in the flat buffer): count, then write -> rewritten?
__device__ __forceinline__ bool cr_region(const char* in, char* out, uint64_t g0, uint64_t x0, uint64_t x1, const CrMap& T, uint32_t max_subst, unsigned long long* changed_bits, uint32_t& n_changed)
{
    uint32_t diff = 0;
    for (uint64_t x = x0; x < x1 && diff <= max_subst; x++) diff += in[x] != T(x);
    if (diff > max_subst) return false;
    for (uint64_t x = x0; x < x1 && diff; x++) {
        const char t = T(x);
        if (in[x] != t) {
            out[x] = t; diff--; n_changed++;
            if (changed_bits) atomicOr(&changed_bits[(g0 + x) >> 6], 1ull << ((g0 + x) & 63u));
        }
    }
    return true;
}

// k_correct_check found nothing: every segment lies inside its read and its unitig, the segments of a read ascend
__global__ __launch_bounds__(CR_THREADS) void k_correct_apply(const char* in, char* out, const uint64_t* __restrict__ offsets, uint64_t n_reads, const uint64_t* __restrict__ seg_offsets,
                                                               const gkc_read_segment* __restrict__ segments, const char* __restrict__ ubases, const uint64_t* __restrict__ uoff,
                                                               uint32_t k, uint32_t max_subst, uint32_t ends, uint32_t* __restrict__ n_changed, unsigned long long* __restrict__ changed_bits,
                                                               CrStats* __restrict__ stats)
{
    unsigned long long st[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g0 = offsets[r], len = offsets[r + 1] - g0, lo = seg_offsets[r], hi = seg_offsets[r + 1];
        const char* rin = in + g0; char* rout = out + g0;
        uint32_t nch = 0;
        if (lo < hi) {
            gkc_read_segment A = segments[lo];
            if (ends && A.read_pos > 0u) {                      // head
                const uint64_t ub = uoff[A.node >> 1], L = uoff[(A.node >> 1) + 1] - ub - (k - 1);
                const bool room = (A.node & 1ull) ? (uint64_t)A.unitig_pos + A.read_pos + 1 <= L : A.unitig_pos >= A.read_pos;
                if (!room) st[CR_ENDS_NO_ROOM]++;
                else st[cr_region(rin, rout, g0, 0, A.read_pos, CrMap(ubases, ub, A, k), max_subst, changed_bits, nch) ? CR_HEADS_FIXED : CR_ENDS_SKIPPED]++;
            }
            for (uint64_t s = lo; s < hi; s++) {
                const uint64_t end_a = (uint64_t)A.read_pos + A.n_kmers;
                if (s + 1 < hi) {                               // the gap behind A, when B goes on along A's unitig where a piece of the gap's length would end
                    const gkc_read_segment B = segments[s + 1];
                    const uint64_t d = (uint64_t)B.read_pos - (uint64_t)A.read_pos;      // n_kmers_A + gap
                    const bool col = (uint64_t)B.read_pos > end_a && B.node == A.node &&
                                     ((A.node & 1ull) ? (uint64_t)B.unitig_pos + d == (uint64_t)A.unitig_pos : (uint64_t)B.unitig_pos == (uint64_t)A.unitig_pos + d);
                    if (col && (uint64_t)B.read_pos >= end_a + k)
                        st[cr_region(rin, rout, g0, end_a + (k - 1), B.read_pos, CrMap(ubases, uoff[A.node >> 1], A, k), max_subst, changed_bits, nch) ? CR_GAPS_FIXED : CR_GAPS_SKIPPED]++;
                    A = B;
                } else if (ends && end_a + (k - 1) < len) {     // tail
                    const uint64_t t = len - (end_a + (k - 1));
                    const uint64_t ub = uoff[A.node >> 1], L = uoff[(A.node >> 1) + 1] - ub - (k - 1);
                    const bool room = (A.node & 1ull) ? (uint64_t)A.unitig_pos + 1 >= (uint64_t)A.n_kmers + t : (uint64_t)A.unitig_pos + A.n_kmers + t <= L;
                    if (!room) st[CR_ENDS_NO_ROOM]++;
                    else st[cr_region(rin, rout, g0, len - t, len, CrMap(ubases, ub, A, k), max_subst, changed_bits, nch) ? CR_TAILS_FIXED : CR_ENDS_SKIPPED]++;
                }
            }
        }
        if (n_changed) n_changed[r] = nch;
        st[CR_BASES_CHANGED] += nch;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        unsigned long long x = st[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
        if ((threadIdx.x & 63u) == 0u && x) atomicAdd(&stats->v[i], x);
    }
}

extern "C" {

int gkc_graph_reads_correct_device(gkc_ctx* c, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                   const uint64_t* d_seg_offsets, const gkc_read_segment* d_segments, uint64_t n_segments,
                                   const char* d_unitig_bases, const uint64_t* d_unitig_offsets,
                                   const gkc_correct_params* params, char* d_out, uint32_t* d_n_changed, uint64_t* d_changed_bits, gkc_correct_stats* stats)
{
    static_assert(sizeof(gkc_correct_params) == 16 && sizeof(gkc_correct_stats) == 56 && sizeof(CrStats) == sizeof(gkc_correct_stats), "the structs of include/gkc.h");
    const char* who = "gkc_graph_reads_correct_device";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    const gkc_correct_params prm = params ? *params : gkc_correct_params{2u, 1u, {0u, 0u}};
    if (!d_offsets || !d_seg_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: the read offsets and the segment offsets are required", who);
    if (n_bases && (!d_bases || !d_out)) GKC_FAIL(c, GKC_ERR_ARG, "%s: the bases and the output are required", who);
    if (n_segments && !d_segments) GKC_FAIL(c, GKC_ERR_ARG, "%s: the segments gkc_graph_reads_segments_device wrote are required", who);
    if (n_bases >= (1ULL << 40)) GKC_FAIL(c, GKC_ERR_ARG, "%s: a single call is limited to 2^40 bases", who);
    if (n_segments >= (1ULL << 40)) GKC_FAIL(c, GKC_ERR_ARG, "%s: a single call is limited to 2^40 segments", who);
    if (n_bases && (((uintptr_t)d_bases | (uintptr_t)d_out) & 15)) GKC_FAIL(c, GKC_ERR_ARG, "%s: d_bases and d_out must be 16-byte aligned", who);
    const bool in_place = d_out == d_bases;
    if (!in_place && n_bases && (uintptr_t)d_out < (uintptr_t)d_bases + n_bases && (uintptr_t)d_bases < (uintptr_t)d_out + n_bases)
        GKC_FAIL(c, GKC_ERR_ARG, "%s: d_out overlaps d_bases (equal: in place; otherwise they must be disjoint)", who);
    if (!d_unitig_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: the unitig offsets gkc_graph_unitigs_write wrote are required", who);
    GKC_TRY(ut_require_placement(c, who));
    const UnitigPlacement& U = c->unitigs;
    const uint64_t n_unitigs = U.n_unitigs;
    if (U.n_bases && !d_unitig_bases) GKC_FAIL(c, GKC_ERR_ARG, "%s: the unitig bases gkc_graph_unitigs_write wrote are required", who);
    const uint32_t k = (uint32_t)c->k;
    ScopedTimer tm(c, "graph_read_correct");
    const size_t rs_words = (size_t)(std::max(n_bases, n_segments) / 32 + 2);      // the masks gkc_launch_mark_read_starts writes beside its verdict: one array takes both
    DevBuf d_rs, d_st;
    GKC_TRY(c->ensure(d_rs, (rs_words + 8) * 4)); GKC_TRY(c->ensure(d_st, sizeof(CrStats)));
    uint32_t* rs = (uint32_t*)d_rs.p; uint32_t* d_flags = rs + rs_words;      // [0] read offsets, [1] segment offsets, [2] unitig offsets, [3..6] bad[] of k_correct_check
    uint32_t flags[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // ---- the three offset tables
    hipError_t e = hipMemsetAsync(rs, 0, (rs_words + 8) * 4, c->stream);
    if (e == hipSuccess) {
        int rc = gkc_launch_mark_read_starts(c, d_offsets, n_reads, n_bases, rs, d_flags);
        if (rc == GKC_OK) rc = gkc_launch_mark_read_starts(c, d_seg_offsets, n_reads, n_segments, rs, d_flags + 1);
        if (rc != GKC_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
        hipLaunchKernelGGL(k_correct_unitig_offsets, dim3(q_grid((n_unitigs + 255) / 256)), dim3(256), 0, c->stream, d_unitig_offsets, (const uint64_t*)U.first.p, U.n_alive, n_unitigs, k,
                           d_flags + 2);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, 12, hipMemcpyDeviceToHost, c->stream);
    hipError_t es = hipStreamSynchronize(c->stream);           // (also after a failure: the scratch goes back to the pool)
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (flags[0]) GKC_FAIL(c, GKC_ERR_ARG, "%s: read offsets are not a CSR table of the bases (need offsets[0] == 0, non-decreasing, offsets[n_reads] == n_bases = %llu)", who, (unsigned long long)n_bases);
    if (flags[1]) GKC_FAIL(c, GKC_ERR_ARG, "%s: segment offsets are not a CSR table of the segments (need offsets[0] == 0, non-decreasing, offsets[n_reads] == n_segments = %llu)", who, (unsigned long long)n_segments);
    if (flags[2]) GKC_FAIL(c, GKC_ERR_ARG, "%s: the unitig offsets are not those of the context's placement (need offsets[0] == 0 and L_u + k - 1 bases per unitig: the strings of another placement?)", who);
    // ---- the segments
    const dim3 block(CR_THREADS), reads(q_grid((n_reads + CR_THREADS - 1) / CR_THREADS));
    if (n_segments) {
        hipLaunchKernelGGL(k_correct_check, reads, block, 0, c->stream, d_offsets, n_reads, d_seg_offsets, d_segments, d_unitig_offsets, n_unitigs, k, d_flags + 3);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(flags + 3, d_flags + 3, 16, hipMemcpyDeviceToHost, c->stream);
        es = hipStreamSynchronize(c->stream);
        GKC_HIP(c, e); GKC_HIP(c, es);
        if (flags[3]) GKC_FAIL(c, GKC_ERR_ARG, "%s: two segments of a read overlap or descend", who);
        if (flags[4]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a segment runs past the end of its read (read_pos + n_kmers + k - 1 > length), or a read has 2^32 bases or more", who);
        if (flags[5]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a segment names a unitig the context's placement does not have (the segments of another placement?)", who);
        if (flags[6]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a segment holds no k-mer or its unitig range leaves [0, L_u)", who);
    }
    // ---- the copy, the overlay
    e = hipMemsetAsync(d_st.p, 0, sizeof(CrStats), c->stream);
    if (e == hipSuccess && d_n_changed && n_reads && !n_segments) e = hipMemsetAsync(d_n_changed, 0, (size_t)n_reads * 4, c->stream);
    if (e == hipSuccess && d_changed_bits && n_bases) e = hipMemsetAsync(d_changed_bits, 0, (size_t)((n_bases + 63) / 64) * 8, c->stream);
    if (e == hipSuccess && !in_place && n_bases) {
        hipLaunchKernelGGL(k_correct_copy, dim3(q_grid((n_bases / CR_VEC + CR_THREADS) / CR_THREADS)), block, 0, c->stream, d_bases, d_out, n_bases);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_segments) {
        hipLaunchKernelGGL(k_correct_apply, reads, block, 0, c->stream, d_bases, d_out, d_offsets, n_reads, d_seg_offsets, d_segments, d_unitig_bases, d_unitig_offsets, k, prm.max_subst,
                           prm.ends, d_n_changed, (unsigned long long*)d_changed_bits, (CrStats*)d_st.p);
        e = hipGetLastError();
    }
    CrStats h{};
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_st.p, sizeof(CrStats), hipMemcpyDeviceToHost, c->stream);
    es = hipStreamSynchronize(c->stream);
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (stats) {
        stats->gaps_fixed = h.v[CR_GAPS_FIXED]; stats->gaps_skipped = h.v[CR_GAPS_SKIPPED]; stats->heads_fixed = h.v[CR_HEADS_FIXED]; stats->tails_fixed = h.v[CR_TAILS_FIXED];
        stats->ends_skipped = h.v[CR_ENDS_SKIPPED]; stats->ends_no_room = h.v[CR_ENDS_NO_ROOM]; stats->bases_changed = h.v[CR_BASES_CHANGED];
    }
    return GKC_OK;
}

}  // extern "C"
