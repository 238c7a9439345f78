// gkc_sink.hip — streamed results, PACKED on the wire (gkc_set_host_sink): the pack kernels and the host's unpack threads. The wire format itself — its constants,
// the layout of a batch, the padding a decoder may read into and the host decoders — is gkc_wire.hpp, which also says why the records travel packed.
//   device   k_pack_pkv_two_widths, k_pack_pkv<KW> (one width; KW = key words): one workgroup per block, two passes over its records (widths, then the packing
//            through LDS), ONE atomic reservation each in the batch's payload stream and abundance stream, the payload starts on 16 bytes and leaves LDS as 16-byte words
//            k_pack_fixed<W>, k_pack_fixed16<W>: one workgroup per block (blocks never straddle partitions, each has its own 16-byte-aligned slot), records -> W-byte
//            entries staged through LDS and written as 16-byte words; reads the batch's Count[] once, writes 0.44x of it
//   link     ONE copy per Stage-B batch on the copy stream: [header | payload], the abundance stream, the exception entries, into a page-locked staging buffer of the library
//   host     a pool of unpack threads: the first to reach a batch waits for its copy (HIP event) and sorts the exceptions, then all of them take blocks off an
//            atomic counter (a block is independent of every other: base key + running sum of its deltas) and write the records with non-temporal 16-byte stores;
//            the last one marks the batch landed (gkc_wait_partition / gkc_finish_pass wait for that)
#include "gkc_common.hpp"
#include "gkc_device.hpp"
#include "gkc_wire.hpp"
#include <algorithm>
#include <utility>
#include <atomic>
#include <deque>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace { constexpr uint32_t PK_THREADS = 256; }

struct PackPlan { const uint32_t* blk_first; /* [nb + 1] first block slot of every partition of the batch */ const uint64_t* ptot; /* [2 (nb + 1)] (distinct, solid) prefixes */ uint32_t nb; };
// where a batch's kernel writes: the sections of wire_layout() in the device buffer (the three header rows, the streams and their cursors: PKV formats only)
struct PackOut {
    uint64_t* bases; uint32_t* cb_off; uint32_t* pay_off16; uint8_t* wbits;
    uint8_t* payload; unsigned long long* pay_cursor /* bytes */;
    uint8_t* cb_stream; unsigned long long* cb_cursor;
    uint64_t* exc; unsigned long long* n_exc; uint32_t exc_cap;
};

// ---- the parts every pack kernel is built from
// block slot g: its partition (the largest p with blk_first[p] <= g), first record and records. Ends on a barrier: what a kernel zeroes in LDS before it is visible behind it.
struct PackBlock { uint64_t r0; uint32_t n; };
__device__ __forceinline__ PackBlock pack_block(const PackPlan& P, const uint32_t g)
{
    __shared__ uint32_t s_p;
    if (threadIdx.x == 0) {
        uint32_t lo = 0, hi = P.nb;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.blk_first[mid] <= g) lo = mid; else hi = mid; }
        s_p = lo;
    }
    __syncthreads();
    const uint32_t p = s_p, j = g - P.blk_first[p];
    const uint64_t s1 = P.ptot[2 * (p + 1) + 1], r0 = P.ptot[2 * p + 1] + (uint64_t)j * PK_BLOCK;
    return { r0, (uint32_t)min((uint64_t)PK_BLOCK, s1 - r0) };
}
__device__ __forceinline__ void pack_except(const PackOut& O, const uint64_t tag, const uint64_t value)
{
    const unsigned long long e = atomicAdd(O.n_exc, 1ull);
    if (e < O.exc_cap) { O.exc[2 * e] = tag; O.exc[2 * e + 1] = value; }
}
__device__ __forceinline__ void pack_words16(uint8_t* dst, const void* lds, const uint32_t words)      // a chunk out of LDS as 16-byte words
{
    for (uint32_t w = threadIdx.x; w < words; w += PK_THREADS) reinterpret_cast<uint4*>(dst)[w] = reinterpret_cast<const uint4*>(lds)[w];
}
// the abundance side of a PKV block: the bitmap (abundance != 1), the stream bytes of the flagged records, the block's places in the two streams
struct PkvLds {
    __attribute__((aligned(16))) unsigned long long bits[PK_BLOCK / 64];
    __attribute__((aligned(16))) uint8_t cb[PK_BLOCK];
    uint32_t wcnt[PK_THREADS / 64];
    unsigned long long base, pay;
};
__device__ __forceinline__ void pkv_clear(PkvLds& S) { for (uint32_t i = threadIdx.x; i < PK_BLOCK / 64; i += PK_THREADS) S.bits[i] = 0ull; }
// one round of pass 1 (records i0 .. i0 + 255, this thread's: `rec`, abundance `ab`, if `valid`): escapes an abundance >= 255, flags the round in the bitmap and appends
// the flagged records' bytes; `run` = flagged records of the rounds before (the same in every thread), returns it with this round's. One barrier inside; the caller
// puts one behind the round.
__device__ __forceinline__ uint32_t pkv_abundance_round(const PackOut& O, PkvLds& S, const bool valid, const uint32_t ab, const uint64_t rec, const uint32_t i0, const uint32_t run)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ab8 = valid ? ab : 1u;
    if (ab8 >= 255u) { pack_except(O, rec, ab); ab8 = 255u; }
    const bool flag = ab8 != 1u;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) { S.bits[(i0 >> 6) + wave] = bal; S.wcnt[wave] = (uint32_t)__popcll(bal); }
    __syncthreads();
    uint32_t before = run, total = 0;
#pragma unroll
    for (int w = 0; w < PK_THREADS / 64; w++) { if (w < (int)wave) before += S.wcnt[w]; total += S.wcnt[w]; }
    if (flag) S.cb[before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint8_t)ab8;
    return run + total;
}
// ONE atomic per stream: `bytes` of payload (a multiple of 16, at most wire_block_max) and `run` abundance bytes; returns where the block's payload goes
__device__ __forceinline__ uint8_t* pkv_reserve(const PackOut& O, PkvLds& S, const uint32_t g, const uint32_t bytes, const uint32_t run)
{
    if (threadIdx.x == 0) {
        S.pay = atomicAdd(O.pay_cursor, (unsigned long long)bytes);
        O.pay_off16[g] = (uint32_t)(S.pay >> 4);
        S.base = run ? atomicAdd(O.cb_cursor, (unsigned long long)run) : 0ull; O.cb_off[g] = (uint32_t)S.base;      // (the stream is shorter than 2^32 bytes: one byte per record at most)
    }
    __syncthreads();
    return O.payload + S.pay;
}
__device__ __forceinline__ void pkv_flush_abundances(const PackOut& O, const PkvLds& S, const uint32_t run)
{
    uint8_t* cb = O.cb_stream + S.base;
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < run; i += PK_THREADS) cb[i] = S.cb[i];      // (a few rounds of fire-and-forget byte stores; unrolled, all 32 possible rounds' loads are hoisted: 104 VGPRs and more)
}

// ---- fixed entries, 8-byte keys: recs = 2 words per record (value, abundance); W = 7 or 8
template <int W>
__global__ __launch_bounds__(PK_THREADS) void k_pack_fixed(const uint64_t* __restrict__ recs, PackPlan P, PackOut O)
{
    constexpr uint64_t PK_ESC = pk_esc(W);
    __shared__ __attribute__((aligned(16))) uint8_t s_out[PK_THREADS * W + 16];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const PackBlock B = pack_block(P, g);
    const uint64_t r0 = B.r0; const uint32_t n = B.n;
    if (t == 0) O.bases[g] = recs[2 * r0];
    uint8_t* dstp = O.payload + (uint64_t)g * pk_slot(W);
    for (uint32_t i0 = 0; i0 < n; i0 += PK_THREADS) {
        const uint32_t i = i0 + t;
        uint64_t d = 0; uint32_t ab8 = 0;
        if (i < n) {
            const ulonglong2 me = *reinterpret_cast<const ulonglong2*>(recs + 2 * (r0 + i));
            const uint64_t prev = i ? recs[2 * (r0 + i - 1)] : me.x;
            d = me.x - prev;
            if (d >= PK_ESC) { pack_except(O, PK_KEY_EXC | (r0 + i), me.x); d = PK_ESC; }
            ab8 = (uint32_t)me.y;
            if (ab8 >= 255u) { pack_except(O, r0 + i, ab8); ab8 = 255u; }
        }
        uint8_t* o = s_out + W * t;
#pragma unroll
        for (int b = 0; b < W - 1; b++) o[b] = (uint8_t)(d >> (8 * b));
        o[W - 1] = (uint8_t)ab8;
        __syncthreads();
        pack_words16(dstp + (uint64_t)i0 * W, s_out, PK_THREADS * W / 16);      // 1792 / 2048 bytes = 112 / 128 x 16
        __syncthreads();
    }
}

// ---- fixed entries, 16-byte keys: recs = 4 words per record (value low, value high, abundance, 0); bases = 2 words per block; W = 16 (15-byte deltas) or 17 (16-byte deltas)
template <int W>
__global__ __launch_bounds__(PK_THREADS) void k_pack_fixed16(const uint64_t* __restrict__ recs, PackPlan P, PackOut O)
{
    typedef unsigned __int128 u128;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[PK_THREADS * W + 16];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const PackBlock B = pack_block(P, g);
    const uint64_t r0 = B.r0; const uint32_t n = B.n;
    if (t == 0) { O.bases[2 * (uint64_t)g] = recs[4 * r0]; O.bases[2 * (uint64_t)g + 1] = recs[4 * r0 + 1]; }
    uint8_t* dstp = O.payload + (uint64_t)g * pk_slot(W);
    for (uint32_t i0 = 0; i0 < n; i0 += PK_THREADS) {
        const uint32_t i = i0 + t;
        uint64_t d_lo = 0, d_hi = 0; uint32_t ab8 = 0;
        if (i < n) {
            const ulonglong2 me = *reinterpret_cast<const ulonglong2*>(recs + 4 * (r0 + i));
            ab8 = (uint32_t)recs[4 * (r0 + i) + 2];
            ulonglong2 pv = me;
            if (i) pv = *reinterpret_cast<const ulonglong2*>(recs + 4 * (r0 + i - 1));
            const u128 d = (((u128)me.y << 64) | me.x) - (((u128)pv.y << 64) | pv.x);
            d_lo = (uint64_t)d; d_hi = (uint64_t)(d >> 64);
            if (W == 16 && (d_hi >> 56) != 0) d_hi = ~0ull, d_lo = ~0ull;                        // does not fit 120 bits: escape below
            if (W == 16 && d_lo == ~0ull && (d_hi & 0xFFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFFull) {  // the escape pattern (also a true delta of exactly 2^120 - 1): two entries
                pack_except(O, PK_KEY_EXC | (r0 + i), me.x); pack_except(O, PK_KEY_EXC_HI | (r0 + i), me.y);
            }
            if (ab8 >= 255u) { pack_except(O, r0 + i, ab8); ab8 = 255u; }
        }
        uint8_t* o = s_out + W * t;
#pragma unroll
        for (int b = 0; b < 8; b++) o[b] = (uint8_t)(d_lo >> (8 * b));
#pragma unroll
        for (int b = 0; b < W - 9; b++) o[8 + b] = (uint8_t)(d_hi >> (8 * b));
        o[W - 1] = (uint8_t)ab8;
        __syncthreads();
        pack_words16(dstp + (uint64_t)i0 * W, s_out, PK_THREADS * W / 16);      // 256 / 272 16-byte words per chunk of PK_THREADS entries
        __syncthreads();
    }
}

// ---- PKV, one width per sub-block, keys of KW words: recs = 2 KW words per record (the value's words, the abundance, padding); bases = KW words per block
template <int KW> struct PackKey;
template <> struct PackKey<1> {
    typedef uint64_t key_t;
    static __device__ __forceinline__ key_t key(const uint64_t* __restrict__ recs, const uint64_t r) { return recs[2 * r]; }
    static __device__ __forceinline__ void load(const uint64_t* __restrict__ recs, const uint64_t r, key_t& k, uint32_t& ab)
    {
        const ulonglong2 me = *reinterpret_cast<const ulonglong2*>(recs + 2 * r); k = me.x; ab = (uint32_t)me.y;
    }
    static __device__ __forceinline__ key_t get(const uint64_t (&s)[1][PKV_CHUNK + 1], const uint32_t i) { return s[0][i]; }
    static __device__ __forceinline__ void put(uint64_t (&s)[1][PKV_CHUNK + 1], const uint32_t i, const key_t k) { s[0][i] = k; }
    static __device__ __forceinline__ uint32_t bits(const key_t d) { return d ? 64u - (uint32_t)__clzll((long long)d) : 0u; }
    static __device__ __forceinline__ uint32_t sent(const uint32_t W) { return W > 56u ? 64u : W; }      // (a host extraction reads 8 bytes at any bit offset: 7 + W <= 63)
    static __device__ __forceinline__ void append(unsigned __int128& acc, uint32_t& nbits, uint8_t*& o, const key_t d, const uint32_t W)
    {
        acc |= (unsigned __int128)d << nbits; nbits += W;
        while (nbits >= 8) { *o++ = (uint8_t)acc; acc >>= 8; nbits -= 8; }
    }
};
template <> struct PackKey<2> {
    typedef unsigned __int128 key_t;
    static __device__ __forceinline__ key_t key(const uint64_t* __restrict__ recs, const uint64_t r)
    {
        const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(recs + 4 * r); return ((key_t)q.y << 64) | q.x;
    }
    static __device__ __forceinline__ void load(const uint64_t* __restrict__ recs, const uint64_t r, key_t& k, uint32_t& ab) { k = key(recs, r); ab = (uint32_t)recs[4 * r + 2]; }
    static __device__ __forceinline__ key_t get(const uint64_t (&s)[2][PKV_CHUNK + 1], const uint32_t i) { return ((key_t)s[1][i] << 64) | s[0][i]; }
    static __device__ __forceinline__ void put(uint64_t (&s)[2][PKV_CHUNK + 1], const uint32_t i, const key_t k) { s[0][i] = (uint64_t)k; s[1][i] = (uint64_t)(k >> 64); }
    static __device__ __forceinline__ uint32_t bits(const key_t d)
    {
        const uint64_t dh = (uint64_t)(d >> 64), dl = (uint64_t)d;
        return dh ? 128u - (uint32_t)__clzll((long long)dh) : dl ? 64u - (uint32_t)__clzll((long long)dl) : 0u;
    }
    static __device__ __forceinline__ uint32_t sent(const uint32_t W) { return W; }
    static __device__ __forceinline__ void append(unsigned __int128& acc, uint32_t& nbits, uint8_t*& o, const key_t d, const uint32_t W)
    {
        const uint32_t wl = W < 64u ? W : 64u, wh = W - wl;
        acc |= (key_t)(uint64_t)d << nbits; nbits += wl;                                    // (the delta's low 64 bits hold nothing above wl bits unless W > 64, and then wl = 64)
        while (nbits >= 8) { *o++ = (uint8_t)acc; acc >>= 8; nbits -= 8; }
        if (wh) { acc |= (key_t)(uint64_t)(d >> 64) << nbits; nbits += wh; while (nbits >= 8) { *o++ = (uint8_t)acc; acc >>= 8; nbits -= 8; } }
    }
};
template <int KW>
__global__ __launch_bounds__(PK_THREADS) void k_pack_pkv(const uint64_t* __restrict__ recs, PackPlan P, PackOut O)
{
    typedef PackKey<KW> K; typedef typename K::key_t key_t;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[PK_THREADS * 64 * KW];             // one chunk's entries: 16 sub-blocks of 16 W bytes, W <= 64 KW
    __shared__ uint64_t s_key[KW][PKV_CHUNK + 1];                                             // the chunk's keys word by word, [..][0] = the key before the chunk
    __shared__ PkvLds S;
    __shared__ uint32_t s_w[PKV_NSUB], s_off[PKV_NSUB + 1];                                   // a sub-block's width (bits of its largest delta), the byte offset of its entries in the block's payload
    const uint32_t g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    pkv_clear(S);
    if (t < PKV_NSUB) s_w[t] = 0u;
    const PackBlock B = pack_block(P, g);
    const uint64_t r0 = B.r0; const uint32_t n = B.n;
    if (t < KW) O.bases[KW * (uint64_t)g + t] = recs[2 * KW * r0 + t];
    // ---- pass 1 (coalesced): the longest delta of every sub-block -> its width; the abundance side
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += PK_THREADS) {
        const uint32_t i = i0 + t;
        uint32_t ab = 1, wd = 0;
        if (i < n) {
            key_t me; K::load(recs, r0 + i, me, ab);
            const key_t prev = i ? K::key(recs, r0 + i - 1) : me;
            wd = K::bits(me - prev);
        }
#pragma unroll
        for (int d_ = 32; d_ >= 1; d_ >>= 1) { const uint32_t y = __shfl_xor(wd, d_, 64); wd = y > wd ? y : wd; }      // (a wave's 64 records lie in one sub-block)
        if (lane == 0 && wd) atomicMax(&s_w[(i0 >> 7) + (wave >> 1)], wd);
        run = pkv_abundance_round(O, S, i < n, ab, r0 + i, i0, run);
        __syncthreads();
    }
    if (t < PKV_NSUB) {                                         // (wave 0) widths, and the exclusive prefix of the sub-blocks' 16 W bytes
        uint32_t W = K::sent(s_w[t]);
        if (t * PKV_SUB >= n) W = 0u;
        uint32_t x = 16u * W;
#pragma unroll
        for (int d_ = 1; d_ < 64; d_ <<= 1) { const uint32_t y = __shfl_up(x, d_, 64); if ((int)lane >= d_) x += y; }
        s_w[t] = W; s_off[t] = x - 16u * W;
        if (t == PKV_NSUB - 1) s_off[PKV_NSUB] = x;
        O.wbits[(uint64_t)g * PKV_NSUB + t] = (uint8_t)W;
    }
    __syncthreads();
    uint8_t* dstp = pkv_reserve(O, S, g, s_off[PKV_NSUB] + (uint32_t)PKV_BITMAP, run);      // (a multiple of 16)
    // ---- pass 2 (the block's records again: L2): chunks of 2048 keys through LDS, every thread packs 8 consecutive deltas into the W bytes of its sub-block's width,
    //      the chunk (16 sub-blocks back to back) leaves as 16-byte words
    for (uint32_t c0 = 0; c0 < n; c0 += PKV_CHUNK) {
        for (uint32_t i = t; i < PKV_CHUNK; i += PK_THREADS) K::put(s_key, 1 + i, c0 + i < n ? K::key(recs, r0 + c0 + i) : (key_t)0);
        if (t == 0) K::put(s_key, 0, K::key(recs, c0 ? r0 + c0 - 1 : r0));
        __syncthreads();
        const uint32_t sub0 = c0 / PKV_SUB, sub = sub0 + (t >> 4), W = s_w[sub], cbase = s_off[sub0];
        {
            unsigned __int128 acc = 0; uint32_t nbits = 0;
            uint8_t* o = s_out + (s_off[sub] - cbase) + (size_t)(t & 15u) * W;
            key_t prev = K::get(s_key, 8 * t);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t i = c0 + 8 * t + q;
                const key_t key = K::get(s_key, 1 + 8 * t + q);
                const key_t d = i < n ? key - prev : (key_t)0;                              // (beyond the block's records: zero bits; W = 0: nothing is written)
                prev = key;
                K::append(acc, nbits, o, d, W);
            }
        }
        __syncthreads();
        pack_words16(dstp + cbase, s_out, (s_off[sub0 + PKV_CHUNK / PKV_SUB] - cbase) >> 4);      // (sub0 + 16 <= 64)
        __syncthreads();
    }
    pack_words16(dstp + s_off[PKV_NSUB], S.bits, (uint32_t)PKV_BITMAP / 16);                 // the bitmap: 1024 bytes = 64 x 16
    pkv_flush_abundances(O, S, run);
}

// ---- PKV with two widths per sub-block (8-byte keys): wbits = [nblk][2 PKV_NSUB] (long widths, then short ones). A thread's 8 records go to bit positions
// that depend on the selector bits before them, so the streams are OR-ed into zeroed LDS words (64-bit LDS atomics) instead of written byte by byte.
__global__ __launch_bounds__(PK_THREADS) void k_pack_pkv_two_widths(const uint64_t* __restrict__ recs, PackPlan P, PackOut O)
{
    constexpr uint32_t NCH = PK_BLOCK / PKV_CHUNK, SPC = PKV_CHUNK / PKV_SUB;                // pack iterations per block, sub-blocks per iteration
    constexpr uint32_t OUT_WORDS = (uint32_t)(PKVT_CHUNK_MAX / 8) + 2;
    __shared__ __attribute__((aligned(16))) unsigned long long s_out[OUT_WORDS];              // one chunk's sub-blocks (+ the word a last delta may spill zeros into)
    __shared__ uint64_t s_key[PKV_CHUNK + 1];                                                 // the chunk's keys, [0] = the key before the chunk
    __shared__ PkvLds S;
    __shared__ unsigned long long s_wmax[2];                                                  // per round of pass 1 (2 sub-blocks): the largest delta,
    __shared__ uint32_t s_hist[2][64];                                                        //   records per bit length (57..64 counted as 63: never a short width)
    __shared__ uint32_t s_wl[PKV_NSUB], s_ws[PKV_NSUB], s_ns[PKV_NSUB], s_sz[PKV_NSUB];       // per sub-block: long / short width, short records, bytes
    __shared__ uint32_t s_off[PKV_NSUB], s_choff[NCH + 1];                                    // byte offset of a sub-block / of a chunk behind the block's abundance bitmap
    const uint32_t g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    pkv_clear(S);
    if (t < PKV_NSUB) { s_wl[t] = 0u; s_ws[t] = 0u; s_ns[t] = 0u; s_sz[t] = 0u; }
    if (t < 128) s_hist[t >> 6][t & 63] = 0u;
    if (t < 2) s_wmax[t] = 0ull;
    const PackBlock B = pack_block(P, g);
    const uint64_t r0 = B.r0; const uint32_t n = B.n;
    if (t == 0) O.bases[g] = recs[2 * r0];
    // ---- pass 1 (coalesced), a round = 256 records = 2 sub-blocks (waves 0-1, waves 2-3): the largest delta and the histogram of bit lengths of each -> its two
    //      widths; the abundance side
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += PK_THREADS) {
        const uint32_t i = i0 + t, sb = wave >> 1;
        uint32_t ab = 1; uint64_t d = 0;
        if (i < n) {
            const ulonglong2 me = *reinterpret_cast<const ulonglong2*>(recs + 2 * (r0 + i));
            const uint64_t prev = i ? recs[2 * (r0 + i - 1)] : me.x;
            d = me.x - prev;
            ab = (uint32_t)me.y;
            const uint32_t len = d ? 64u - (uint32_t)__clzll((long long)d) : 0u;
            atomicAdd(&s_hist[sb][len < 63u ? len : 63u], 1u);
        }
#pragma unroll
        for (int d_ = 32; d_ >= 1; d_ >>= 1) { const uint64_t y = (uint64_t)__shfl_xor((unsigned long long)d, d_, 64); d = y > d ? y : d; }
        if (lane == 0 && d) atomicMax(&s_wmax[sb], (unsigned long long)d);
        run = pkv_abundance_round(O, S, i < n, ab, r0 + i, i0, run);
        if ((wave & 1u) == 0u) {                                // one wave per sub-block: lane L prices the short width L
            const uint32_t sub = (i0 >> 7) + sb, first = sub * PKV_SUB, cnt = first < n ? min(PKV_SUB, n - first) : 0u;
            const uint64_t m = s_wmax[sb];
            uint32_t wl = m ? 64u - (uint32_t)__clzll((long long)m) : 0u;
            if (wl > 56u) wl = 64u;
            uint32_t cum = s_hist[sb][lane];                    // records of at most `lane` bits
#pragma unroll
            for (int d_ = 1; d_ < 64; d_ <<= 1) { const uint32_t y = __shfl_up(cum, d_, 64); if ((int)lane >= d_) cum += y; }
            const uint32_t one = (cnt * wl + 7u) >> 3;
            uint32_t best = lane < wl && lane <= 56u ? ((PKV_SEL + ((cum * lane + 7u) >> 3) + (((cnt - cum) * wl + 7u) >> 3)) << 6) | lane : ~0u;      // (bytes, width): at most 2^11 bytes
#pragma unroll
            for (int d_ = 32; d_ >= 1; d_ >>= 1) { const uint32_t y = __shfl_xor(best, d_, 64); best = y < best ? y : best; }
            const bool split = best != ~0u && (best >> 6) + 16u <= one;
            const uint32_t ws = split ? best & 63u : wl, ns = __shfl(cum, (int)(best & 63u), 64);
            if (lane == 0) { s_wl[sub] = wl; s_ws[sub] = ws; s_ns[sub] = split ? ns : 0u; s_sz[sub] = split ? best >> 6 : one; s_wmax[sb] = 0ull; }
            s_hist[sb][lane] = 0u;
        }
        __syncthreads();
    }
    if (t < PKV_NSUB) {                                         // (wave 0) the sub-blocks' offsets: a prefix inside every chunk of 16, the chunks padded to 16 bytes
        const uint32_t sz = s_sz[t];
        uint32_t x = sz;
#pragma unroll
        for (int d_ = 1; d_ < (int)SPC; d_ <<= 1) { const uint32_t y = __shfl_up(x, d_, SPC); if ((int)(lane & (SPC - 1)) >= d_) x += y; }
        const uint32_t ct = (__shfl(x, (int)(lane | (SPC - 1)), 64) + 15u) & ~15u;
        uint32_t base = 0, end = 0;
#pragma unroll
        for (uint32_t c = 0; c < NCH; c++) { const uint32_t v = __shfl(ct, (int)(c * SPC), 64); if (c < lane / SPC) base += v; end += v; }
        s_off[t] = base + x - sz;
        if ((lane & (SPC - 1)) == 0) s_choff[lane / SPC] = base;
        if (t == 0) s_choff[NCH] = end;
        O.wbits[(uint64_t)g * 2 * PKV_NSUB + t] = (uint8_t)s_wl[t];
        O.wbits[(uint64_t)g * 2 * PKV_NSUB + PKV_NSUB + t] = (uint8_t)s_ws[t];
    }
    __syncthreads();
    uint8_t* dstp = pkv_reserve(O, S, g, s_choff[NCH] + (uint32_t)PKV_BITMAP, run);          // (a multiple of 16, at most wire_block_max)
    pack_words16(dstp, S.bits, (uint32_t)PKV_BITMAP / 16);                                   // the abundance bitmap comes FIRST here: 1024 bytes = 64 x 16
    dstp += PKV_BITMAP;
    // ---- pass 2 (the block's records again: L2): chunks of 2048 keys through LDS, every thread sends its 8 consecutive deltas to the short or the long stream of its
    //      sub-block, at the bit its 16-lane prefix of the selector bits says; the chunk (16 sub-blocks back to back, padded to 16 bytes) leaves as 16-byte words
    auto put = [&](const uint32_t bit, const uint64_t v, const uint32_t w) {                  // v < 2^w at bit `bit` of the zeroed s_out
        if (!v) return;
        const uint32_t sh = bit & 63u;
        atomicOr(&s_out[bit >> 6], (unsigned long long)(v << sh));
        if (sh + w > 64u) atomicOr(&s_out[(bit >> 6) + 1], (unsigned long long)(v >> (64u - sh)));
    };
    for (uint32_t c0 = 0, ch = 0; c0 < n; c0 += PKV_CHUNK, ch++) {
        const uint32_t cbase = s_choff[ch], cbytes = s_choff[ch + 1] - cbase;                 // (cbytes <= PKVT_CHUNK_MAX)
        for (uint32_t i = t; i < PKV_CHUNK; i += PK_THREADS) s_key[1 + i] = c0 + i < n ? recs[2 * (r0 + c0 + i)] : 0ull;
        if (t == 0) s_key[0] = c0 ? recs[2 * (r0 + c0 - 1)] : recs[2 * r0];
        for (uint32_t w = t; w < (cbytes >> 3) + 2u; w += PK_THREADS) s_out[w] = 0ull;
        __syncthreads();
        {
            const uint32_t sub = ch * SPC + (t >> 4), wl = s_wl[sub], ws = s_ws[sub], ns = s_ns[sub], sbyte = s_off[sub] - cbase;
            const bool split = ws != wl;
            uint64_t dl[8]; uint32_t valid = 0, sel = 0;
            uint64_t prev = s_key[8 * t];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t i = c0 + 8 * t + q;
                const uint64_t key = s_key[1 + 8 * t + q];
                dl[q] = i < n ? key - prev : 0ull;
                prev = key;
                const uint32_t len = dl[q] ? 64u - (uint32_t)__clzll((long long)dl[q]) : 0u;
                if (i < n) { valid |= 1u << q; if (!split || len > ws) sel |= 1u << q; }
            }
            const uint32_t mine = (uint32_t)__popc(sel) | ((uint32_t)__popc(valid) << 16);
            uint32_t x = mine;                                  // (long, all) records of the sub-block's threads before this one
#pragma unroll
            for (int d_ = 1; d_ < 16; d_ <<= 1) { const uint32_t y = __shfl_up(x, d_, 16); if ((int)(t & 15u) >= d_) x += y; }
            x -= mine;
            const uint32_t pl = x & 0xFFFFu, ps = (x >> 16) - pl;
            uint32_t sbit = 8u * (sbyte + PKV_SEL) + ps * ws;
            uint32_t lbit = 8u * (sbyte + (split ? PKV_SEL + ((ns * ws + 7u) >> 3) : 0u)) + pl * wl;
            if (split) put(8u * (sbyte + (t & 15u)), (uint64_t)sel, 8u);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                if (!((valid >> q) & 1u)) continue;
                if ((sel >> q) & 1u) { put(lbit, dl[q], wl); lbit += wl; } else { put(sbit, dl[q], ws); sbit += ws; }
            }
        }
        __syncthreads();
        pack_words16(dstp + cbase, s_out, cbytes >> 4);
        __syncthreads();
    }
    pkv_flush_abundances(O, S, run);
}

// ------------------------------------------------------------------------------------------------ host side
struct SinkBatch {
    int users = 0;                               // workers between picking this batch and their last access to it (under gkc_unpacker::mu): a batch is deleted only at users == 0
    hipEvent_t copied = nullptr;                 // the batch's packed bytes are in the staging buffer
    hipEvent_t copy_start = nullptr;             // GKC_SINK_DEBUG: when the copy stream got to it
    WireBatch w;                                 // what the decoders read: the staged batch (wire_staged), its blocks, where they land
    uint64_t n_cb = 0;                           // bytes of the abundance stream (GKC_SINK_DEBUG)
    void* d_packed = nullptr;                    // device buffer, given back once copied
    bool ready = false, syncing = false;         // copy completed + exceptions sorted (under the pool's lock)
    std::atomic<uint64_t> next{0}, finished{0};
    std::atomic<bool> done{false};
    std::chrono::steady_clock::time_point t_queued, t_ready;           // GKC_SINK_DEBUG
    double pack_ms = 0;
};

struct gkc_unpacker {
    gkc_ctx* c = nullptr;
    std::vector<std::thread> threads;
    std::mutex mu; std::condition_variable cv, cv_done;
    std::deque<SinkBatch*> queue;                // batches whose blocks are not all taken yet, oldest first
    std::vector<SinkBatch*> all;                 // every batch of the pass (owned)
    bool stop = false;
    bool debug = false;                          // GKC_SINK_DEBUG as it was when the sink was prepared (gkc_sink_prepare): the workers print a line per batch
    uint8_t* staging = nullptr; uint64_t staging_cap = 0, staging_used = 0;
    std::atomic<uint64_t> n_decisions{0}, n_adaptive_raw{0}, max_batch_records{0};     // batches of this context that travelled raw because the host was behind (gkc_sink_host_behind)

    void worker()
    {
        (void)hipSetDevice(c->device);
        for (;;) {
            SinkBatch* B = nullptr;
            {   std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    if (stop) return;
                    if (!queue.empty()) {
                        B = queue.front();
                        if (B->ready) break;
                        if (!B->syncing) { B->syncing = true; break; }       // this thread waits for the copy
                    }
                    cv.wait(lk);
                }
                B->users++;                                                  // (gkc_sink_reset deletes a batch only when nobody is inside it any more)
            }
            if (!B->ready) {
                (void)hipEventSynchronize(B->copied);
                if (B->w.lay.exc_cap) wire_sort_exceptions(B->w);
                if (B->d_packed) { c->dfree(B->d_packed); B->d_packed = nullptr; }
                B->t_ready = std::chrono::steady_clock::now();
                { std::lock_guard<std::mutex> lk(mu); B->ready = true; }
                cv.notify_all();
            }
            for (;;) {
                const uint64_t g = B->next.fetch_add(1);
                if (g >= B->w.nblk) break;
                unpack_block(B->w, g, have_avx512());
                if (B->finished.fetch_add(1) + 1 == B->w.nblk) {
                    _mm_sfence();
                    if (debug) {
                        const auto now = std::chrono::steady_clock::now();
                        float copy_ms = -1; if (B->copy_start) (void)hipEventElapsedTime(&copy_ms, B->copy_start, B->copied);
                        const auto t00 = all.empty() ? B->t_queued : all.front()->t_queued;
                        fprintf(stderr, "[gkc sink] +%.1f ms: batch of %llu blocks (%.2f GB packed, %llu exceptions): pack %.1f ms, queued -> copied %.1f ms (the copy itself %.1f ms), unpack %.1f ms\n",
                                std::chrono::duration<double, std::milli>(B->t_queued - t00).count(), (unsigned long long)B->w.nblk,
                                (double)((wire_pkv(B->w.fmt) ? B->w.lay.pay_cap : B->w.nblk * B->w.lay.block_max) + B->n_cb) / 1e9, (unsigned long long)B->w.lay.exc_cap, B->pack_ms, std::chrono::duration<double, std::milli>(B->t_ready - B->t_queued).count(), copy_ms,
                                std::chrono::duration<double, std::milli>(now - B->t_ready).count());
                    }
                    { std::lock_guard<std::mutex> lk(mu); B->done.store(true); }
                    cv_done.notify_all(); c->cv_done.notify_all();
                }
            }
            {   std::lock_guard<std::mutex> lk(mu);                              // every block of B has been taken: the next batch becomes the front
                if (!queue.empty() && queue.front() == B && B->next.load() >= B->w.nblk) queue.pop_front();
                B->users--;                                                      // the last access of this thread to B
            }
            cv.notify_all(); cv_done.notify_all();
        }
    }
};

// The unpack threads run on the cores of the NUMA node that holds the buffers they stream through (the page-locked staging buffer and the caller's sink are allocated
// by the thread that set the sink up, on its node): measured on the 2-socket host of the MI355X box, the same 16-24 threads expand a batch in 20 ms or in 50-80 ms
// depending on where the scheduler happened to put them. get_mempolicy(MPOL_F_NODE | MPOL_F_ADDR) names the node of a page; /sys lists its cores.
static int numa_node_of(const void* p)
{
    int node = -1;
    if (syscall(SYS_get_mempolicy, &node, nullptr, 0ul, const_cast<void*>(p), 3ul /* MPOL_F_NODE | MPOL_F_ADDR */) != 0) return -1;
    return node;
}
static bool cpus_of_node(int node, cpu_set_t* set)
{
    char path[96]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r"); if (!f) return false;
    char buf[4096]; const bool got = fgets(buf, sizeof buf, f) != nullptr; fclose(f);
    if (!got) return false;
    CPU_ZERO(set); int n = 0;
    for (char* q = buf; *q; ) {
        char* e; const long a = strtol(q, &e, 10); if (e == q) break;
        long b = a; if (*e == '-') { q = e + 1; b = strtol(q, &e, 10); }
        for (long i = a; i <= b && i < CPU_SETSIZE; i++) { CPU_SET((int)i, set); n++; }
        q = *e == ',' ? e + 1 : e; if (*e != ',') break;
    }
    return n > 0;
}
static void pin_unpackers(gkc_unpacker* U);

static gkc_unpacker* unpacker_of(gkc_ctx* c)
{
    if (c->unpacker) return c->unpacker;
    gkc_unpacker* U = new gkc_unpacker(); U->c = c;
    // measured on the 2 x 64-core host of the MI355X box (tools/hostmem_probe/unpack_probe): 16 threads expand 14e9 records/s (100 GB/s read + 230 GB/s of non-temporal
    // writes) with or without a device -> host copy running beside them; 64 threads fall to 6e9/s beside the copy stream, 128 to 4e9/s even alone
    // (round 7: with the AVX-512 emitter a record costs a thread a third of what the scalar loops take, and 16 threads keep ahead of the link with the two-width format
    //  where 24 of them, beside the copy stream and the Stage-B lanes, had steps in which landed batches piled up and the next ones travelled raw: 12 / 16 / 20 / 24
    //  threads = 447 / 443 / 441 / 487 ms per step, profiles/r07_two_widths.txt)
    //  (only where that emitter will run: 8-byte keys at abundance-min 1; the other formats keep their scalar loops and their 24 threads)
    const unsigned n_alone = have_avx512() && gkc_tun().sink_two_widths && c->key_words == 1 && c->amin <= 1 ? 16u : 24u;
    int n = gkc_tun().unpack_threads > 0 ? gkc_tun().unpack_threads : (int)std::min<unsigned>(n_alone, std::max(2u, std::thread::hardware_concurrency() / 2));
    // Several ranks of one job share the host (a communicator of W ranks on this context = W processes, taken to be spread evenly over the host's NUMA nodes): the host
    // expands 1.2-1.4e10 records/s in all however many ranks ask, and FEWER threads reach it — 8 ranks x 24 threads get 5.2e9 records/s, 8 x 3 threads 1.33e10 (round 6,
    // tools/hostmem_probe/unpack_ranks_probe on the 2 x 64-core host: profiles/r06_host_unpack_ceiling.txt) — so every rank takes its share of 12 threads per node.
    if (gkc_tun().unpack_threads <= 0 && c->comm_world > 1) {
        int nodes = 0; cpu_set_t tmp; while (nodes < 64 && cpus_of_node(nodes, &tmp)) nodes++;
        if (nodes < 1) nodes = 1;
        const int per_node = (c->comm_world + nodes - 1) / nodes;
        n = std::max(2, std::min(n, 12) / std::max(1, per_node));             // 12 per node: 2 ranks on 2 nodes 1.11e10 records/s with 12 or 24 each; 8 ranks: 3 each 1.33e10, 6: 1.01e10, 24: 5.2e9
    }
    if (n < 1) n = 1;
    for (int i = 0; i < n; i++) U->threads.emplace_back([U] { U->worker(); });
    c->unpacker = U;
    return U;
}

// whether the sink of this context takes packed batches (8-byte keys; GKC_SINK_PACKED=0 keeps the plain copies)
bool gkc_sink_packed(gkc_ctx* c, const GkcTun& tun)
{
    const bool off = !tun.sink_packed;
    const bool off2 = !tun.sink_packed2;       // (16-byte keys only)
    return c->sink && !c->sink_raw && (c->key_words == 1 || !off2) && !off && ((uintptr_t)c->sink & 15) == 0;
}

int gkc_sink_prepare(gkc_ctx* c)
{
    if (!gkc_sink_packed(c, gkc_tun())) return GKC_OK;
    gkc_unpacker* U = unpacker_of(c);
    U->debug = gkc_tun().sink_debug;
    const uint64_t want = wire_staging_bytes(c->key_words, c->sink_cap, c->nb_partitions);
    if (U->staging_cap < want) {
        if (U->staging) (void)hipHostFree(U->staging);
        U->staging = nullptr; U->staging_cap = 0;
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return GKC_OK; }      // no staging buffer: the batches travel unpacked
        U->staging = (uint8_t*)p; U->staging_cap = want;
    }
    pin_unpackers(U);
    return GKC_OK;
}

static void pin_unpackers(gkc_unpacker* U)
{
    if (!U->staging) return;
    const int node = numa_node_of(U->c->sink ? U->c->sink : (const void*)U->staging);
    cpu_set_t set;
    if (node < 0 || !cpus_of_node(node, &set)) return;
    for (std::thread& t : U->threads) (void)pthread_setaffinity_np(t.native_handle(), sizeof(set), &set);
    if (U->debug) fprintf(stderr, "[gkc sink] %zu unpack threads on the cores of NUMA node %d (where the sink lives)\n", U->threads.size(), node);
}

// start of a pass / a pass counted again: nothing of the previous one is in flight any more
void gkc_sink_reset(gkc_ctx* c)
{
    gkc_unpacker* U = c->unpacker;
    if (!U) return;
    {   std::unique_lock<std::mutex> lk(U->mu);
        U->cv_done.wait(lk, [&] { for (SinkBatch* B : U->all) if (!B->done.load() || B->users != 0) return false; return true; });
        U->queue.clear();
    }
    for (SinkBatch* B : U->all) { if (B->copied) (void)hipEventDestroy(B->copied); if (B->copy_start) (void)hipEventDestroy(B->copy_start); if (B->d_packed) c->dfree(B->d_packed); delete B; }
    U->all.clear(); U->staging_used = 0; c->sink_wire_bytes = 0; U->max_batch_records = 0;
}
void gkc_sink_drain(gkc_ctx* c)
{
    gkc_unpacker* U = c->unpacker;
    if (!U) return;
    std::unique_lock<std::mutex> lk(U->mu);
    U->cv_done.wait(lk, [&] { for (SinkBatch* B : U->all) if (!B->done.load()) return false; return true; });
}
void gkc_sink_shutdown(gkc_ctx* c)
{
    gkc_unpacker* U = c->unpacker;
    if (!U) return;
    gkc_sink_reset(c);
    { std::lock_guard<std::mutex> lk(U->mu); U->stop = true; }
    U->cv.notify_all();
    for (std::thread& t : U->threads) t.join();
    if (U->staging) (void)hipHostFree(U->staging);
    delete U; c->unpacker = nullptr;
}
void gkc_sink_wait_batch(gkc_ctx* c, const void* batch)
{
    gkc_unpacker* U = c->unpacker;
    if (!U || !batch) return;
    const SinkBatch* B = static_cast<const SinkBatch*>(batch);
    std::unique_lock<std::mutex> lk(U->mu);
    U->cv_done.wait(lk, [&] { return B->done.load(); });
}

// Round 6 — several ranks on one host: is the HOST behind? Records whose copy has landed in the staging buffer and that no thread has expanded yet, against what this
// batch holds. One rank alone expands a batch in 2/3 of the time its copy takes (the link is the bound: at most the batch in hand is pending); 2-8 ranks sharing the
// host's memory controllers get 1.0-1.4e10 records/s between them (profiles/r06_host_unpack_ceiling.txt) and their staging buffers fill with landed, unexpanded
// batches. A batch queued then travels RAW instead (16 B per record on this rank's own link, no host work) — the link is busy 2.6x longer with it and the expansion
// threads catch up: every rank balances its link against its share of the host by itself, batch by batch. The sink ends up byte for byte the same either way.
static thread_local const char* g_sink_why = "";                   // why the last batch of this thread did not travel packed (GKC_SINK_DEBUG)
bool gkc_sink_host_behind(gkc_ctx* c, uint64_t n_records, const GkcTun& tun)
{
    gkc_unpacker* U = c->unpacker;
    if (!U || !tun.sink_adaptive) return false;
    uint64_t pending = 0;
    {   std::lock_guard<std::mutex> lk(U->mu);
        for (SinkBatch* B : U->all) {
            if (B->done.load()) continue;
            if (B->ready || hipEventQuery(B->copied) == hipSuccess) pending += B->w.nblk - std::min<uint64_t>(B->finished.load(), B->w.nblk);
        }
    }
    (void)hipGetLastError();                                        // (hipErrorNotReady of the queries)
    // (against the LARGEST batch of the pass so far, not this one: the small batches at the end of a ramp would otherwise see the whole batch in hand of the
    //  expansion threads as "1.5 batches behind" and travel raw — 16 instead of 6 bytes per record on the link at the very end of the step)
    uint64_t ref = U->max_batch_records.load(); if (n_records > ref) { U->max_batch_records = n_records; ref = n_records; }
    const bool behind = tun.sink_adaptive == 2 ? (U->n_decisions++ & 1) != 0                       // (tests: packed and raw batches alternate in one pass)
                                                     : pending * PK_BLOCK > std::max<uint64_t>(ref + ref / 2, (uint64_t)1 << 22);
    if (behind) { g_sink_why = "the host is behind with the expansion (landed, unexpanded records beyond 1.5 batches): this batch travels raw"; U->n_adaptive_raw++; }
    return behind;
}

// One Stage-B batch: d_out = its Count[] (total records, partition i = [solid_prefix[i], solid_prefix[i+1])), d_ptot = the (distinct, solid) prefixes on the device,
// h_dest = where the records belong in the sink. Runs on the calling lane's stream up to the point where the copy can be queued; returns the batch handle
// (nullptr: not packed — no staging room, too many exceptions — the caller sends the plain records).
const char* gkc_sink_last_refusal() { return g_sink_why; }
void* gkc_sink_send_packed(gkc_ctx* c, const void* d_out, const uint64_t* d_ptot, const std::vector<uint64_t>& solid_prefix, uint8_t* h_dest, const GkcTun& tun)
{
    gkc_unpacker* U = c->unpacker;
    g_sink_why = "no staging buffer";
    if (!U || !U->staging) return nullptr;
    const uint32_t nb = (uint32_t)solid_prefix.size() - 1;
    std::vector<uint32_t> blk_first(nb + 1);
    uint64_t nblk = 0;
    for (uint32_t i = 0; i < nb; i++) { blk_first[i] = (uint32_t)nblk; nblk += (solid_prefix[i + 1] - solid_prefix[i] + PK_BLOCK - 1) / PK_BLOCK; }
    blk_first[nb] = (uint32_t)nblk;
    g_sink_why = "no records / too many blocks";
    if (nblk == 0 || nblk >= (1ull << 31)) return nullptr;
    // fixed entries of 8 bytes where the partitions are sparse, of 7 where dense, PKV (per-sub-block delta widths + bitmap + abundance stream) where dense at
    // abundance-min 1 (most abundances are 1: sequencing errors), checked batch by batch: a batch that came out above 7 bytes per record switches the context back to 7
    const uint64_t dense_min = tun.sink_dense ? tun.sink_dense : PK_DENSE;      // (tests: 1 = every batch is "dense")
    const bool wide = c->key_words == 2;
    const uint64_t n_rec = solid_prefix[nb];
    const bool dense = n_rec / std::max<uint32_t>(nb, 1) >= (wide ? std::min<uint64_t>(dense_min, PK2_DENSE) : dense_min);
    const bool pkv_ok = tun.sink_width6 && !c->sink_no6 && n_rec < (1ull << 32);
    const WireFormat fmt = wide ? (pkv_ok ? WireFormat::Pkv16 : dense ? WireFormat::Fixed16 : WireFormat::Fixed17)
                         : !dense ? WireFormat::Fixed8 : !(c->amin <= 1 && pkv_ok) ? WireFormat::Fixed7 : tun.sink_two_widths ? WireFormat::PkvTwoWidths : WireFormat::Pkv;
    const bool pkv = wire_pkv(fmt);
    const WireLayout L = wire_layout(fmt, nblk, n_rec);                          // (PKV: the worst case — every block at full width; what is copied is what was used)
    g_sink_why = "no device memory for the packed copy";
    DevBuf d_first; if (c->ensure(d_first, (size_t)(nb + 1) * 4) != GKC_OK) return nullptr;
    uint8_t* d_packed = (uint8_t*)c->dalloc((size_t)L.total);
    if (!d_packed) return nullptr;
    hipStream_t st = cur_stream(c);
    const auto t_pack0 = std::chrono::steady_clock::now();
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_packed + L.cnt_off);       // [0] exceptions [1] bytes of the abundance stream [2] bytes of the payload stream (PKV)
    unsigned long long h_cnt[3] = {0, 0, 0};
    bool ok = hipMemcpyAsync(d_first.p, blk_first.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st) == hipSuccess
           && hipMemsetAsync(d_cnt, 0, 24, st) == hipSuccess;
    if (ok) {
        const PackPlan P{ (const uint32_t*)d_first.p, d_ptot, nb };
        const PackOut O{ (uint64_t*)d_packed, (uint32_t*)(d_packed + L.cboff_off), (uint32_t*)(d_packed + L.payoff_off), d_packed + L.wbits_off, d_packed + L.pay_off, d_cnt + 2,
                         d_packed + L.cb_off, d_cnt + 1, (uint64_t*)(d_packed + L.exc_off), d_cnt, (uint32_t)L.exc_cap };
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(PK_THREADS), 0, st, (const uint64_t*)d_out, P, O); };
        switch (fmt) {
        case WireFormat::Fixed7: launch(k_pack_fixed<7>); break;
        case WireFormat::Fixed8: launch(k_pack_fixed<8>); break;
        case WireFormat::Pkv: launch(k_pack_pkv<1>); break;
        case WireFormat::PkvTwoWidths: launch(k_pack_pkv_two_widths); break;
        case WireFormat::Fixed16: launch(k_pack_fixed16<16>); break;
        case WireFormat::Fixed17: launch(k_pack_fixed16<17>); break;
        case WireFormat::Pkv16: launch(k_pack_pkv<2>); break;
        }
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h_cnt, d_cnt, 24, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    d_first.release();                                   // handed back early: what follows only stages and sends the packed block
    const unsigned long long h_nexc = h_cnt[0], h_ncb = h_cnt[1], h_pay = h_cnt[2];
    g_sink_why = !ok ? "pack launch failed" : "too many exceptions";
    if (!ok || h_nexc > L.exc_cap || h_ncb > L.cb_cap || (pkv && h_pay > L.pay_cap - WIRE_TAIL)) { (void)hipGetLastError(); c->dfree(d_packed); return nullptr; }
    // (a batch whose per-block widths + abundance stream came out above the 7 bytes per record of the fixed entries — wide gaps AND few abundances of 1 — switches the
    //  context to those; this batch still travels as it was packed)
    if (pkv && (double)(h_pay + h_ncb) > (wide ? 16.0 : 7.0) * (double)n_rec) c->sink_no6 = true;
    const WireLayout S = wire_staged(fmt, L, h_pay, h_ncb, h_nexc);             // what travels and is staged
    SinkBatch* B = new SinkBatch();
    {   std::lock_guard<std::mutex> lk(c->mu);
        if (U->staging_used + S.total > U->staging_cap) { g_sink_why = "staging buffer full"; delete B; c->dfree(d_packed); return nullptr; }
        B->w.stage = U->staging + U->staging_used; U->staging_used += wire_round(S.total);
        c->sink_wire_bytes += S.pay_off + S.pay_cap + h_ncb + h_nexc * 16;
    }
    B->w.lay = S; B->w.fmt = fmt; B->w.nblk = nblk; B->w.dest = h_dest; B->n_cb = h_ncb; B->d_packed = d_packed;
    B->w.blk_rec0.resize(nblk); B->w.blk_n.resize(nblk);
    for (uint32_t i = 0; i < nb; i++) {
        const uint64_t s0 = solid_prefix[i], s1 = solid_prefix[i + 1];
        for (uint64_t r = s0, g = blk_first[i]; r < s1; r += PK_BLOCK, g++) { B->w.blk_rec0[g] = r; B->w.blk_n[g] = (uint32_t)std::min<uint64_t>(PK_BLOCK, s1 - r); }
    }
    if (tun.sink_debug && hipEventCreate(&B->copy_start) == hipSuccess) (void)hipEventRecord(B->copy_start, c->copy_stream);
    bool queued = hipEventCreateWithFlags(&B->copied, tun.sink_debug ? hipEventDefault : hipEventDisableTiming) == hipSuccess
               && hipMemcpyAsync((void*)B->w.stage, d_packed, (size_t)(S.pay_off + S.pay_cap), hipMemcpyDeviceToHost, c->copy_stream) == hipSuccess
               && (h_ncb == 0 || hipMemcpyAsync((void*)(B->w.stage + S.cb_off), d_packed + L.cb_off, (size_t)h_ncb, hipMemcpyDeviceToHost, c->copy_stream) == hipSuccess)
               && (h_nexc == 0 || hipMemcpyAsync((void*)(B->w.stage + S.exc_off), d_packed + L.exc_off, (size_t)h_nexc * 16, hipMemcpyDeviceToHost, c->copy_stream) == hipSuccess)
               && hipEventRecord(B->copied, c->copy_stream) == hipSuccess;
    if (!queued) { g_sink_why = "copy could not be queued"; (void)hipGetLastError(); (void)hipStreamSynchronize(c->copy_stream); if (B->copied) (void)hipEventDestroy(B->copied); delete B; c->dfree(d_packed); return nullptr; }
    B->t_queued = std::chrono::steady_clock::now(); B->pack_ms = std::chrono::duration<double, std::milli>(B->t_queued - t_pack0).count();
    if (tun.sink_debug) { std::lock_guard<std::mutex> lk(U->mu); if (U->all.empty()) fprintf(stderr, "[gkc sink] first batch queued %.1f ms after Stage B began\n", std::chrono::duration<double, std::milli>(B->t_queued - c->t_stage_b0).count()); }
    { std::lock_guard<std::mutex> lk(U->mu); U->all.push_back(B); U->queue.push_back(B); }
    U->cv.notify_all();
    return B;
}
