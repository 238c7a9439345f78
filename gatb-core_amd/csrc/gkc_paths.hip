// gkc_paths.hip — read paths: where the k-mers of reads lie in the compacted graph, and the unitigs a read spells (include/gkc.h, "read paths").
//
// gkc_graph_reads_nodes_device is the reads kernel of gkc_query.hip in its third mode (QM_NODES): the search returns base + pos, the flat record index, and the answer
// step gathers UnitigPlacement::unitig / pos at that index instead of the abundance. Nothing of it is here but the guards and the call.
//
// gkc_graph_reads_segments_device works on the two arrays that call wrote, in words of 64 positions (one wave handles one word, one lane one position):
//   k_path_bits    : position g BREAKS when it does not continue g - 1 (no node, the first position of a read — from the read-start bit mask of gkc_launch_mark_read_starts,
//                    never a search of the offsets —, another node, or a position that is not the neighbour's); it STARTS a segment when it breaks and carries a node. Two
//                    ballots per wave: start[w], brk[w]. Positions behind the buffer break and start nothing; one more word behind the last one does the same, so that
//                    every walk below ends inside the arrays.
//   k_graph_tile_sums, gr_scan_tiles, k_graph_tile_offsets<false> (gkc_graph.hpp) over the starts per word: rank[w] = the starts in front of word w. The number of starts in front of position g is rank[g >> 6] + popcount(start[g >> 6] below bit g & 63):
//                    that is the index of a segment among all segments, and at g = offsets[r] it is seg_offsets[r] — the CSR over the reads needs no pass over the reads'
//                    counts, and no scan of its own (k_path_offsets: one thread per entry).
//   k_path_fill    : a lane whose position starts a segment writes it at that index. Its length is the distance to the next break: the rest of brk[w], then whole words
//                    with one count-trailing-zeros each — at most n_kmers / 64 + 2 words, and a segment is no longer than its read. The read's first position is the last
//                    read start at or in front of g: the read-start mask walked backwards a 32-bit word at a time, at most read_pos / 32 + 2 words; bit 0 is always set
//                    (offsets[0] == 0 was checked). d_support takes one 64-bit vector atomic per segment.
// Element indices are 64-bit; grids go through q_grid and the kernels stride. Scratch comes from the context's pool on c->stream, is allocated before the first launch
// and synchronised before it goes back.
#include "gkc_unitigs.hpp"

constexpr int PT_WAVES = GR_THREADS / 64;                     // words of 64 positions a workgroup handles per trip

__device__ __forceinline__ uint64_t pt_rank(const uint64_t* __restrict__ rank, const uint64_t* __restrict__ start, uint64_t g)
{
    const uint32_t b = (uint32_t)g & 63u;
    return rank[g >> 6] + (uint64_t)__popcll(start[g >> 6] & ((1ull << b) - 1ull));
}

// n_words = words that hold positions of the buffer; word n_words is written too (no start, all breaks)
__global__ __launch_bounds__(GR_THREADS) void k_path_bits(const uint64_t* __restrict__ node, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rsbits, uint64_t n_bases,
                                                           uint64_t n_words, uint64_t* __restrict__ start, uint64_t* __restrict__ brk)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * PT_WAVES + (threadIdx.x >> 6); w <= n_words; w += (uint64_t)gridDim.x * PT_WAVES) {      // (uniform per wave)
        const uint64_t g = w * 64 + lane;
        const bool in = g < n_bases;
        const uint64_t nd = in ? node[g] : GKC_NODE_NO_KMER;
        const uint32_t p = in ? pos[g] : 0u;
        uint64_t nd_prev = __shfl_up(nd, 1, 64); uint32_t p_prev = __shfl_up(p, 1, 64);
        if (lane == 0 && in && g > 0) { nd_prev = node[g - 1]; p_prev = pos[g - 1]; }
        const bool mapped = nd < GKC_NODE_NO_KMER;
        const bool read_start = in && ((rsbits[g >> 5] >> ((uint32_t)g & 31u)) & 1u);
        const bool step = (nd & 1ull) ? (uint64_t)p + 1 == (uint64_t)p_prev : (uint64_t)p == (uint64_t)p_prev + 1;
        const bool cont = mapped && g > 0 && !read_start && nd_prev == nd && step;
        const uint64_t sb = __ballot(mapped && !cont), bb = __ballot(!cont);
        if (lane == 0) { start[w] = sb; brk[w] = bb; }
    }
}
struct PtWordStarts { const uint64_t* start; __device__ __forceinline__ uint32_t operator()(uint64_t w) const { return (uint32_t)__popcll(start[w]); } };      // the value of a word in the prefix sum
// offsets[r] <= n_bases was checked: its word is at most word n_words, which both arrays have
__global__ __launch_bounds__(256) void k_path_offsets(const uint64_t* __restrict__ offsets, uint64_t n_entries, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ start,
                                                       uint64_t* __restrict__ seg_offsets)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_entries; r += (uint64_t)gridDim.x * blockDim.x) seg_offsets[r] = pt_rank(rank, start, offsets[r]);
}
// a read of 2^32 bases or more (read_pos and n_kmers are 32-bit)
__global__ __launch_bounds__(256) void k_path_read_lengths(const uint64_t* __restrict__ offsets, uint64_t n_reads, uint32_t* __restrict__ too_long)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x)
        if (offsets[r + 1] - offsets[r] >= (1ull << 32)) *too_long = 1u;
}
__global__ __launch_bounds__(GR_THREADS) void k_path_fill(const uint64_t* __restrict__ node, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rsbits, uint64_t n_words,
                                                           const uint64_t* __restrict__ start, const uint64_t* __restrict__ brk, const uint64_t* __restrict__ rank,
                                                           gkc_read_segment* __restrict__ segments, unsigned long long* __restrict__ support, uint64_t n_unitigs,
                                                           uint32_t* __restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * PT_WAVES + (threadIdx.x >> 6); w < n_words; w += (uint64_t)gridDim.x * PT_WAVES) {
        const uint64_t sb = start[w];
        if (!((sb >> lane) & 1ull)) continue;
        const uint64_t g = w * 64 + lane;
        // the next break behind g: word n_words is all breaks, the walk ends there at the latest
        uint64_t rest = lane == 63u ? 0ull : (brk[w] >> (lane + 1u));
        uint64_t len;
        if (rest) len = (uint64_t)__builtin_ctzll(rest) + 1;
        else {
            uint64_t w2 = w + 1;
            while ((rest = brk[w2]) == 0ull) w2++;
            len = w2 * 64 + (uint64_t)__builtin_ctzll(rest) - g;
        }
        // the read's first position: the last read start at or in front of g (bit 0 of the mask is set)
        uint64_t wi = g >> 5;
        uint32_t x = rsbits[wi] & (0xFFFFFFFFu >> (31u - ((uint32_t)g & 31u)));
        while (!x) x = rsbits[--wi];
        const uint64_t r0 = wi * 32 + (31u - (uint32_t)__builtin_clz(x));
        const uint64_t nd = node[g];
        gkc_read_segment S;
        S.node = nd; S.read_pos = (uint32_t)(g - r0); S.unitig_pos = pos[g]; S.n_kmers = (uint32_t)len; S.pad = 0u;
        segments[rank[w] + (uint64_t)__popcll(sb & ((1ull << lane) - 1ull))] = S;
        if (support) { if ((nd >> 1) < n_unitigs) atomicAdd(&support[nd >> 1], (unsigned long long)len); else *bad = 1u; }
    }
}

extern "C" {

int gkc_graph_reads_nodes_device(gkc_ctx* c, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t* d_node, uint32_t* d_pos)
{
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    GKC_TRY(ut_require_placement(c, "gkc_graph_reads_nodes_device"));
    const UnitigPlacement& U = c->unitigs;
    const QNodes N{(const uint64_t*)U.unitig.p, (const uint32_t*)U.pos.p, d_node, d_pos};
    return gkc_query_reads_run(c, q_model_of(c), c->qidx, nullptr, 0, d_bases, d_offsets, n_reads, n_bases, nullptr, nullptr, "gkc_graph_reads_nodes_device", &N);
}

int gkc_graph_reads_segments_device(gkc_ctx* c, const uint64_t* d_node, const uint32_t* d_pos, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                    uint64_t* d_seg_offsets, gkc_read_segment* d_segments, uint64_t cap_segments, uint64_t* n_segments, uint64_t* d_support)
{
    static_assert(sizeof(gkc_read_segment) == 24, "gkc_read_segment is 24 bytes");
    const char* who = "gkc_graph_reads_segments_device";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_segments) *n_segments = 0;
    const bool sizing = !d_seg_offsets && !d_segments;
    if (!d_seg_offsets && d_segments) GKC_FAIL(c, GKC_ERR_ARG, "%s: segments without offsets (both, or neither to count only)", who);
    if (!d_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: offsets are required", who);
    if (n_bases && (!d_node || !d_pos)) GKC_FAIL(c, GKC_ERR_ARG, "%s: the nodes and the positions gkc_graph_reads_nodes_device wrote are required", who);
    if (n_bases >= (1ULL << 40)) GKC_FAIL(c, GKC_ERR_ARG, "%s: a single call is limited to 2^40 bases", who);
    uint64_t n_unitigs = 0;
    if (d_support && !sizing) { GKC_TRY(ut_require_placement(c, who)); n_unitigs = c->unitigs.n_unitigs; }
    else GKC_HIP(c, hipSetDevice(c->device));
    ScopedTimer tm(c, "graph_read_segments");
    const uint64_t n_words = (n_bases + 63) / 64, n_w = n_words + 1;      // (+ the word of breaks behind the buffer)
    const uint32_t n_tiles = (uint32_t)((n_w + GR_TILE - 1) / GR_TILE);
    const size_t rs_words = (size_t)(n_bases / 32 + 2);        // bit n_bases is marked too
    DevBuf d_rs, d_start, d_brk, d_rank, d_ts;
    GKC_TRY(c->ensure(d_rs, (rs_words + 4) * 4)); GKC_TRY(c->ensure(d_start, (size_t)n_w * 8)); GKC_TRY(c->ensure(d_brk, (size_t)n_w * 8)); GKC_TRY(c->ensure(d_rank, (size_t)n_w * 8));
    GKC_TRY(c->ensure(d_ts, ((size_t)n_tiles + 1) * 8));
    uint32_t* rs = (uint32_t*)d_rs.p; uint32_t* d_flags = rs + rs_words;      // [0] offsets are no CSR table, [1] a read too long, [2] a node of no unitig
    uint64_t* start = (uint64_t*)d_start.p; uint64_t* brk = (uint64_t*)d_brk.p; uint64_t* rank = (uint64_t*)d_rank.p; uint64_t* ts = (uint64_t*)d_ts.p;
    const dim3 block(GR_THREADS), words(q_grid((n_w + PT_WAVES - 1) / PT_WAVES)), tiles(q_grid(n_tiles));
    uint32_t flags[3] = {0, 0, 0}; uint64_t total = 0;
    // ---- the offsets, the mask of the read starts
    hipError_t e = hipMemsetAsync(rs, 0, (rs_words + 4) * 4, c->stream);
    if (e == hipSuccess) {
        const int rc = gkc_launch_mark_read_starts(c, d_offsets, n_reads, n_bases, rs, d_flags);
        if (rc != GKC_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
        if (n_reads) hipLaunchKernelGGL(k_path_read_lengths, dim3(q_grid((n_reads + 255) / 256)), dim3(256), 0, c->stream, d_offsets, n_reads, d_flags + 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t es = hipStreamSynchronize(c->stream);           // (also after a failure: the scratch goes back to the pool)
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (flags[0]) GKC_FAIL(c, GKC_ERR_ARG, "%s: read offsets are not a CSR table of the bases (need offsets[0] == 0, non-decreasing, offsets[n_reads] == n_bases = %llu)", who, (unsigned long long)n_bases);
    if (flags[1]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a read of 2^32 bases or more (read_pos and n_kmers are 32-bit)", who);
    // ---- starts and breaks, the number of segments
    if (n_bases) {
        hipLaunchKernelGGL(k_path_bits, words, block, 0, c->stream, d_node, d_pos, (const uint32_t*)rs, n_bases, n_words, start, brk);
        hipLaunchKernelGGL(k_graph_tile_sums<PtWordStarts>, tiles, block, 0, c->stream, PtWordStarts{start}, n_w, n_tiles, ts);
        gr_scan_tiles(c, ts, nullptr, n_tiles);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, ts + n_tiles, 8, hipMemcpyDeviceToHost, c->stream);
        es = hipStreamSynchronize(c->stream);
        GKC_HIP(c, e); GKC_HIP(c, es);
    }
    if (n_segments) *n_segments = total;
    if (sizing) return GKC_OK;
    if (cap_segments < total) GKC_FAIL(c, GKC_ERR_CAPACITY, "%s: %llu segments, room for %llu", who, (unsigned long long)total, (unsigned long long)cap_segments);
    if (total && !d_segments) GKC_FAIL(c, GKC_ERR_ARG, "%s: the segments are required", who);
    // ---- offsets, segments, support
    e = hipSuccess;
    if (d_support && n_unitigs) e = hipMemsetAsync(d_support, 0, (size_t)n_unitigs * 8, c->stream);
    if (e == hipSuccess && !n_bases) e = hipMemsetAsync(d_seg_offsets, 0, (size_t)(n_reads + 1) * 8, c->stream);
    if (e == hipSuccess && n_bases) {
        hipLaunchKernelGGL((k_graph_tile_offsets<false, PtWordStarts>), tiles, block, 0, c->stream, PtWordStarts{start}, n_w, n_tiles, (const uint64_t*)ts, rank);
        hipLaunchKernelGGL(k_path_offsets, dim3(q_grid((n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, d_offsets, n_reads + 1, (const uint64_t*)rank, (const uint64_t*)start, d_seg_offsets);
        if (total) hipLaunchKernelGGL(k_path_fill, words, block, 0, c->stream, d_node, d_pos, (const uint32_t*)rs, n_words, (const uint64_t*)start, (const uint64_t*)brk, (const uint64_t*)rank,
                                      d_segments, (unsigned long long*)d_support, n_unitigs, d_flags + 2);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&flags[2], d_flags + 2, 4, hipMemcpyDeviceToHost, c->stream);
    }
    es = hipStreamSynchronize(c->stream);
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (flags[2]) GKC_FAIL(c, GKC_ERR_ARG, "%s: d_node names a unitig the context's placement does not have (the nodes of another placement?); d_support holds no result", who);
    return GKC_OK;
}

}  // extern "C"
