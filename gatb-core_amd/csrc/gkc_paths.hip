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
//
// gkc_graph_reads_walks_device joins the segments of a read across the link CSR of gkc_unitig_links.hip (k_walk_junctions, k_walk_fill: below, in front of the entry points).
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

// ------------------------------------------------------------------------------------------------ walks: the segments of a read joined across unitig links
// One lane per segment, one wave per word of 64 segments. The junction of segment s (include/gkc.h, "junction") is evaluated from s and s + 1 and what the rule in
// force needs of the placement and the link CSR, nothing more: the tests that cost no load come first (B's extremity on strand 0, A's on strand 1), L_u / L_v only for
// the strand that needs them, the slot only when both extremities hold. The wave ballots ENDS: bit s of end[w] says that the junction of s is no link index, i.e. that
// a walk ends with s. (A walk starts behind every end — start(s) = end(s - 1) — but that bit crosses the word border and the lane of bit 0 would have to evaluate a
// second junction; the ends number the walks just as well: the walks in front of segment g are the ends in front of g.) The last segment of the array is always an end
// (bit n_segments of the read-start mask is set, the offsets were checked), so every search for the next end stops inside the array; word n_words is written as 0.
// What the kernel finds wrong it flags and steps around: bad[0] two segments of a read overlap or descend, bad[1] a node of no unitig, bad[2] a slot's range.
__global__ __launch_bounds__(GR_THREADS) void k_walk_junctions(const gkc_read_segment* __restrict__ segments, uint64_t n_segments, uint64_t n_words, const uint32_t* __restrict__ rsbits,
                                                                const uint64_t* __restrict__ first, uint64_t n_alive, uint64_t n_unitigs,
                                                                const uint64_t* __restrict__ loff, const uint64_t* __restrict__ links, uint64_t n_links,
                                                                uint64_t* __restrict__ junction, uint64_t* __restrict__ end, uint32_t* __restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * PT_WAVES + (threadIdx.x >> 6); w <= n_words; w += (uint64_t)gridDim.x * PT_WAVES) {      // (uniform per wave)
        const uint64_t s = w * 64 + lane;
        const bool in = s < n_segments;
        gkc_read_segment A; A.node = 0; A.read_pos = A.unitig_pos = A.n_kmers = A.pad = 0;
        if (in) A = segments[s];
        uint64_t node_b = __shfl_down(A.node, 1, 64); uint32_t rp_b = __shfl_down(A.read_pos, 1, 64), up_b = __shfl_down(A.unitig_pos, 1, 64);
        if (lane == 63u && s + 1 < n_segments) { const gkc_read_segment B = segments[s + 1]; node_b = B.node; rp_b = B.read_pos; up_b = B.unitig_pos; }
        const uint64_t u = A.node >> 1, v = node_b >> 1;
        const bool last = in && ((rsbits[(s + 1) >> 5] >> ((uint32_t)(s + 1) & 31u)) & 1u);      // (bit n_segments is set)
        uint64_t j = GKC_JUNCTION_END;
        if (in && u >= n_unitigs) bad[1] = 1u;
        if (in && !last) {
            const uint64_t end_a = (uint64_t)A.read_pos + A.n_kmers;
            if ((uint64_t)rp_b < end_a) bad[0] = 1u;
            else if ((uint64_t)rp_b == end_a) {
                j = GKC_JUNCTION_UNLINKED;
                if (u < n_unitigs && v < n_unitigs) {           // (lane s + 1 flags a v of no unitig)
                    bool ext = (A.node & 1ull) ? (uint64_t)A.unitig_pos + 1 == (uint64_t)A.n_kmers : true;
                    ext = ext && ((node_b & 1ull) ? true : up_b == 0u);
                    if (ext && !(A.node & 1ull)) ext = (uint64_t)A.unitig_pos + A.n_kmers == ut_length(first, n_alive, n_unitigs, u);
                    if (ext && (node_b & 1ull)) ext = (uint64_t)up_b + 1 == ut_length(first, n_alive, n_unitigs, v);
                    if (ext) {
                        const uint64_t lo = loff[A.node], hi = loff[A.node + 1];
                        if (hi > n_links || lo > hi) bad[2] = 1u;
                        else for (uint64_t e = lo; e < hi; e++) if (links[e] == node_b) { j = e; break; }
                    }
                }
            } else {
                const uint64_t len = (uint64_t)rp_b - (uint64_t)A.read_pos;      // n_kmers_A + gap
                const bool col = node_b == A.node && ((A.node & 1ull) ? (uint64_t)up_b + len == (uint64_t)A.unitig_pos : (uint64_t)up_b == (uint64_t)A.unitig_pos + len);
                j = col ? GKC_JUNCTION_COLLINEAR : GKC_JUNCTION_BREAK;
            }
        }
        if (in && junction) junction[s] = j;
        const uint64_t eb = __ballot(in && j >= GKC_JUNCTION_UNLINKED);
        if (lane == 0) end[w] = eb;
    }
}
struct WkWordEnds { const uint64_t* end; __device__ __forceinline__ uint32_t operator()(uint64_t w) const { return (uint32_t)__popcll(end[w]); } };      // the value of a word in the prefix sum
// every range of the link CSR: non-descending and inside [0, n_links] (n_entries = 2 n_unitigs + 1)
__global__ __launch_bounds__(256) void k_walk_link_offsets(const uint64_t* __restrict__ loff, uint64_t n_entries, uint64_t n_links, uint32_t* __restrict__ bad)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_entries; t += (uint64_t)gridDim.x * blockDim.x)
        if (loff[t] > n_links || (t + 1 < n_entries && loff[t + 1] < loff[t])) *bad = 1u;
}
// A lane whose segment follows an end (or is segment 0) starts a walk and writes it at the rank of its start: the ends in front of it. The walk's end is the next end
// bit at or behind the lane: the rest of end[w], then whole words. Every lane hands its junction on (jbuf: what k_walk_junctions kept in scratch until the capacity was
// known) and adds to the support of the link it names.
__global__ __launch_bounds__(GR_THREADS) void k_walk_fill(const gkc_read_segment* __restrict__ segments, uint64_t n_segments, uint64_t n_words, const uint64_t* __restrict__ end,
                                                           const uint64_t* __restrict__ rank, const uint64_t* __restrict__ jbuf, uint64_t* __restrict__ junction,
                                                           unsigned long long* __restrict__ support, gkc_read_walk* __restrict__ walks)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * PT_WAVES + (threadIdx.x >> 6); w < n_words; w += (uint64_t)gridDim.x * PT_WAVES) {
        const uint64_t s = w * 64 + lane;
        if (s >= n_segments) continue;
        if (jbuf) {
            const uint64_t j = jbuf[s];
            if (junction) junction[s] = j;
            if (support && j < GKC_JUNCTION_UNLINKED) atomicAdd(&support[j], 1ull);
        }
        const uint64_t eb = end[w];
        const bool starts = lane ? (eb >> (lane - 1u)) & 1ull : (w ? end[w - 1] >> 63 : 1ull);
        if (!starts) continue;
        uint64_t rest = eb >> lane, last;
        if (rest) last = s + (uint64_t)__builtin_ctzll(rest);
        else {
            uint64_t w2 = w + 1;
            while (w2 < n_words && (rest = end[w2]) == 0ull) w2++;
            last = rest ? w2 * 64 + (uint64_t)__builtin_ctzll(rest) : n_segments - 1;      // (the last segment is an end: rest is never 0 here)
        }
        const gkc_read_segment Z = segments[last];
        gkc_read_walk W;
        W.first_segment = s; W.n_segments = (uint32_t)(last - s + 1); W.n_kmers = Z.read_pos + Z.n_kmers - segments[s].read_pos;
        walks[rank[w] + (uint64_t)__popcll(eb & ((1ull << lane) - 1ull))] = W;
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

int gkc_graph_reads_walks_device(gkc_ctx* c, const uint64_t* d_seg_offsets, const gkc_read_segment* d_segments, uint64_t n_reads, uint64_t n_segments,
                                 const uint64_t* d_link_offsets, const uint64_t* d_links, uint64_t n_links, uint64_t* d_junction,
                                 uint64_t* d_walk_offsets, gkc_read_walk* d_walks, uint64_t cap_walks, uint64_t* n_walks, uint64_t* d_link_support)
{
    static_assert(sizeof(gkc_read_walk) == 16, "gkc_read_walk is 16 bytes");
    const char* who = "gkc_graph_reads_walks_device";
    gkc_tun_refresh();
    if (!c) return GKC_ERR_ARG;
    if (n_walks) *n_walks = 0;
    const bool sizing = !d_walk_offsets && !d_walks;
    if (!sizing && (!d_walk_offsets || !d_walks)) GKC_FAIL(c, GKC_ERR_ARG, "%s: walks without offsets, or offsets without walks (both, or neither to count only)", who);
    if (!d_seg_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: the segment offsets are required", who);
    if (n_segments && !d_segments) GKC_FAIL(c, GKC_ERR_ARG, "%s: the segments gkc_graph_reads_segments_device wrote are required", who);
    if (n_segments >= (1ULL << 40)) GKC_FAIL(c, GKC_ERR_ARG, "%s: a single call is limited to 2^40 segments", who);
    if (n_links && !d_links) GKC_FAIL(c, GKC_ERR_ARG, "%s: the links are required", who);
    GKC_TRY(ut_require_placement(c, who));
    const UnitigPlacement& U = c->unitigs;
    const uint64_t n_unitigs = U.n_unitigs;
    if (!d_link_offsets) GKC_FAIL(c, GKC_ERR_ARG, "%s: the link offsets gkc_graph_unitigs_links wrote are required", who);
    ScopedTimer tm(c, "graph_read_walks");
    const uint64_t n_words = (n_segments + 63) / 64, n_w = n_words + 1;      // (+ the word behind the array: seg_offsets may name segment n_segments)
    const uint32_t n_tiles = (uint32_t)((n_w + GR_TILE - 1) / GR_TILE);
    const size_t rs_words = (size_t)(n_segments / 32 + 2);     // bit n_segments is marked too
    const bool keep = !sizing && (d_junction || d_link_support) && n_segments;
    DevBuf d_rs, d_end, d_rank, d_ts, d_jbuf;
    GKC_TRY(c->ensure(d_rs, (rs_words + 4) * 4)); GKC_TRY(c->ensure(d_end, (size_t)n_w * 8)); GKC_TRY(c->ensure(d_rank, (size_t)n_w * 8));
    GKC_TRY(c->ensure(d_ts, ((size_t)n_tiles + 1) * 8));
    if (keep) GKC_TRY(c->ensure(d_jbuf, (size_t)n_segments * 8));
    uint32_t* rs = (uint32_t*)d_rs.p; uint32_t* d_flags = rs + rs_words;      // [0] offsets are no CSR table, [1] segments overlap, [2] a node of no unitig, [3] a slot's range
    uint64_t* end = (uint64_t*)d_end.p; uint64_t* rank = (uint64_t*)d_rank.p; uint64_t* ts = (uint64_t*)d_ts.p; uint64_t* jbuf = keep ? (uint64_t*)d_jbuf.p : nullptr;
    const dim3 block(GR_THREADS), words(q_grid((n_w + PT_WAVES - 1) / PT_WAVES)), tiles(q_grid(n_tiles));
    uint32_t flags[4] = {0, 0, 0, 0}; uint64_t total = 0;
    // ---- the offsets, the mask of the reads' first segments, the ranges of the link CSR; then the junctions, the ends and their number
    hipError_t e = hipMemsetAsync(rs, 0, (rs_words + 4) * 4, c->stream);
    if (e == hipSuccess) {
        const int rc = gkc_launch_mark_read_starts(c, d_seg_offsets, n_reads, n_segments, rs, d_flags);
        if (rc != GKC_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
        hipLaunchKernelGGL(k_walk_link_offsets, dim3(q_grid((2 * n_unitigs + 1 + 255) / 256)), dim3(256), 0, c->stream, d_link_offsets, 2 * n_unitigs + 1, n_links, d_flags + 3);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, 16, hipMemcpyDeviceToHost, c->stream);
    hipError_t es = hipStreamSynchronize(c->stream);           // (also after a failure: the scratch goes back to the pool)
    GKC_HIP(c, e); GKC_HIP(c, es);
    if (flags[0]) GKC_FAIL(c, GKC_ERR_ARG, "%s: segment offsets are not a CSR table of the segments (need offsets[0] == 0, non-decreasing, offsets[n_reads] == n_segments = %llu)", who, (unsigned long long)n_segments);
    if (flags[3]) GKC_FAIL(c, GKC_ERR_ARG, "%s: the link offsets are descending or end beyond n_links = %llu (the links of another placement?)", who, (unsigned long long)n_links);
    if (n_segments) {
        hipLaunchKernelGGL(k_walk_junctions, words, block, 0, c->stream, d_segments, n_segments, n_words, (const uint32_t*)rs, (const uint64_t*)U.first.p, U.n_alive, n_unitigs,
                           d_link_offsets, d_links, n_links, jbuf, end, d_flags + 1);
        hipLaunchKernelGGL(k_graph_tile_sums<WkWordEnds>, tiles, block, 0, c->stream, WkWordEnds{end}, n_w, n_tiles, ts);
        gr_scan_tiles(c, ts, nullptr, n_tiles);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, ts + n_tiles, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, 16, hipMemcpyDeviceToHost, c->stream);
        es = hipStreamSynchronize(c->stream);
        GKC_HIP(c, e); GKC_HIP(c, es);
        if (flags[1]) GKC_FAIL(c, GKC_ERR_ARG, "%s: two segments of a read overlap or descend", who);
        if (flags[2]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a segment names a unitig the context's placement does not have (the segments of another placement?)", who);
        if (flags[3]) GKC_FAIL(c, GKC_ERR_ARG, "%s: a slot of the link CSR is descending or ends beyond n_links", who);
    }
    if (n_walks) *n_walks = total;
    if (sizing) return GKC_OK;
    if (cap_walks < total) GKC_FAIL(c, GKC_ERR_CAPACITY, "%s: %llu walks, room for %llu", who, (unsigned long long)total, (unsigned long long)cap_walks);
    // ---- offsets, walks, junctions, support
    e = hipSuccess;
    if (d_link_support && n_links) e = hipMemsetAsync(d_link_support, 0, (size_t)n_links * 8, c->stream);
    if (e == hipSuccess && !n_segments) e = hipMemsetAsync(d_walk_offsets, 0, (size_t)(n_reads + 1) * 8, c->stream);
    if (e == hipSuccess && n_segments) {
        hipLaunchKernelGGL((k_graph_tile_offsets<false, WkWordEnds>), tiles, block, 0, c->stream, WkWordEnds{end}, n_w, n_tiles, (const uint64_t*)ts, rank);
        hipLaunchKernelGGL(k_path_offsets, dim3(q_grid((n_reads + 1 + 255) / 256)), dim3(256), 0, c->stream, d_seg_offsets, n_reads + 1, (const uint64_t*)rank, (const uint64_t*)end, d_walk_offsets);
        hipLaunchKernelGGL(k_walk_fill, words, block, 0, c->stream, d_segments, n_segments, n_words, (const uint64_t*)end, (const uint64_t*)rank, (const uint64_t*)jbuf, d_junction,
                           (unsigned long long*)d_link_support, d_walks);
        e = hipGetLastError();
    }
    es = hipStreamSynchronize(c->stream);
    GKC_HIP(c, e); GKC_HIP(c, es);
    return GKC_OK;
}

}  // extern "C"
