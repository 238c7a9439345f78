// gkc_wire.hpp — the wire format of the packed result batches (gkc_set_host_sink), in one place: its constants, the layout of a batch and the host decoders. Plain
// C++17: no HIP header, no gkc_ctx — gkc_sink.hip (the pack kernels, the unpack threads) includes it for the host and the device pass, and tests/wire_driver.cpp
// compiles it with g++ alone and runs every decoder without a GPU.
//
// SURVEY §8(d) ends the clock when the last partition's Count[] is in host memory, and at abundance-min 1 that is 16 bytes per distinct k-mer over PCIe — 58 GB per
// 10^8 reads, 1.1 s at the 52 GB/s the link gives, five times the counting itself. The records of a partition are ascending keys with small abundances, so what
// crosses the link is
//     per block of PK_BLOCK records: the first key (8 bytes), then per record 6 bytes of key DELTA + 1 byte of abundance            = 7 bytes instead of 16
//     — and at abundance-min 1, where most records are the singletons of sequencing errors (84 % of the 30x input), the abundance byte travels only for the
//     records whose abundance is NOT 1: 6 bytes of delta + 1 bit in the block's bitmap + a byte in the batch's abundance stream for those = 6.3 bytes (PK6)
//     — and since round 6 the deltas of that format are bit-packed at the width of the largest delta of their sub-block of 128 records, one width byte per sub-block,
//     8- and 16-byte keys alike (PKV below): 5.8 bytes per record at k = 31, 14.5 of 32 at k = 63 (10^8 reads), no key escapes
//     — and with 8-byte keys a sub-block has TWO widths where that pays: a third of the gaps are the small ones between an error k-mer and its parent, they travel at a
//     short width of their own behind a selector bitmap of 16 bytes (PKV with two widths below; GKC_SINK_TWO_WIDTHS=0 keeps one): 5.34 bytes per record at k = 31
// and library threads on the host expand it into the exact in-memory layout of Kmer<span>::Count ({u64 value; i32 abundance; pad}, Abundance.hpp:68-129) at its
// place in the caller's sink: what gkc_wait_partition hands out is byte for byte what the unpacked copy would have been (tests: the sink against
// gkc_partition_counts). Rare values leave through an exception list of (tag, value) pairs, 16 bytes each, sorted by tag on the host: a delta that does not fit a
// fixed entry (tag PK_KEY_EXC | record index, the delta field then holds the escape: all ones), an abundance of 255 or more (tag = record index, escape 255). The
// reference's sink this stands in for is CountProcessorDump -> BagCache -> CollectionHDF5Patch (CountProcessorDump.hpp:148-152): the consumer of whole Count[] blocks.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include <immintrin.h>

#if defined(__clang__)
#define GKC_WIRE_UNROLL _Pragma("unroll")
#else
#define GKC_WIRE_UNROLL _Pragma("GCC unroll 8")
#endif

constexpr uint32_t PK_BLOCK = 8192;                                     // records per block: blocks never straddle partitions, each is independent of every other
// FIXED entries, 8-byte keys: entry = [key delta : W - 1 bytes][abundance : 1 byte], W = 7 where the partitions are dense (10^8 reads at abundance-min 1: 8.9e5 records
// per partition, 0.03 % of the deltas do not fit 48 bits), W = 8 where they are sparse (abundance-min 2: 1.4e5 per partition, 1 % would escape — and every escape is a
// sorted-list lookup on the host). A block has its own slot of PK_BLOCK entries in the payload.
constexpr uint64_t pk_slot(int W) { return (uint64_t)PK_BLOCK * (uint64_t)W; }      // 57344 / 65536 bytes: multiples of 16
constexpr uint64_t pk_esc(int W) { return (1ull << (8 * (W - 1))) - 1ull; }
constexpr uint64_t PK_KEY_EXC = 1ull << 63;
constexpr uint64_t PK_DENSE = 300000;                                   // records per partition from which the dense formats are used
// FIXED entries, 16-byte keys (k >= 32; round 4): the same scheme on 32-byte Count records {u128 value; i32 abundance; 12 bytes of padding} (Abundance.hpp:68-129 with
// LargeInt<2>): per block the first key (16 bytes), per record [key delta : 15 or 16 bytes][abundance : 1 byte] = widths 16 / 17 instead of 32. A partition of 5.6e5
// records in a 126-bit key space has deltas of ~2^107 — but canonical k-mers thin out towards the top of the key space (density 2 (1 - x)), and with 14-byte deltas
// 0.1-0.4 % of them escaped (1e6 exception entries per batch of 2.6e8 records: measured, the batches fell back to plain copies): 15 bytes where the partitions are
// dense (a delta of 2^120 - 1 or more — a few per batch — escapes through TWO exception entries, low and high word), the full 16 bytes where they are sparse.
constexpr uint64_t PK_KEY_EXC_HI = (1ull << 63) | (1ull << 62);
constexpr uint64_t PK2_DENSE = 100000;                                  // records per partition from which 15-byte deltas are used
// PKV (round 6, it replaces the fixed 6-byte deltas of rounds 3-5): the deltas travel bit-packed at the width of the largest delta of their SUB-BLOCK of PKV_SUB = 128
// records (64 sub-blocks per block, one width byte each in the header). Canonical k-mers thin out towards the top of the key space: the gaps of a partition of 8.9e5
// records average 2^42 and range from 2^41 at the bottom to 2^50 in its last blocks, so one width for all either wastes bits at the bottom or escapes at the top
// (48 bits + 0.03 % escapes before); the largest of 128 exponential gaps is 2.3 bits above their mean (of 8192: 3.2 + what the clusters of k-mers that start with
// their minimizer add): ~44.6 bits on average and NO key escapes. 128 W bits = 16 W bytes: every sub-block starts on a byte and is sent whole (a partition's last one
// too). A block's payload = its sub-blocks back to back + a bitmap of PK_BLOCK bits (abundance != 1), at an offset of the batch's payload stream the block's workgroup
// reserves (u32 in 16-byte units in the header); the abundance bytes of the flagged records, in record order, sit in the batch's abundance stream from the block's
// offset on (u32 per block in the header) — both reserved by ONE atomic each: the order of the blocks in the streams is whatever it came out as. With 8-byte keys
// W > 56 is sent as W = 64 (a host extraction reads 8 bytes at any bit offset: 7 + W <= 63).
constexpr uint32_t PKV_CHUNK = 2048, PKV_SUB = 128, PKV_NSUB = PK_BLOCK / PKV_SUB;              // records per pack iteration (256 threads x 8); per width; widths per block
constexpr uint64_t PKV_BITMAP = PK_BLOCK / 8;
// PKV for 16-byte keys (round 6): the same layout with 128-bit deltas — a sub-block's width W is 0..128 bits, a record's W bits are the low min(W, 64) bits of its
// delta followed by the W - 64 high ones; bases are 16 bytes per block. k = 63, 5.6e5 records per partition: gaps of 2^107 on average, 13.7 bytes per record where
// the fixed entries carry 15 or 16 (+ escapes).
// PKV with TWO widths per sub-block (8-byte keys; the default): the gaps of a partition are NOT independent. At 30x with 1 % substitutions 84 % of the distinct k-mers
// are one-nucleotide variants of a genomic k-mer, and a variant that keeps its minimizer and strand lands INSIDE its parent's gap of 2^42: a third of all gaps are
// small, log-uniform over 1..35 bits, and one width per sub-block sends them all at the ~45 bits of the largest. Here a sub-block has a long width wl (its largest
// delta, as above) and a short one ws: the EXACT minimum of 16 + ceil(n_short ws / 8) + ceil(n_long wl / 8) over ws < wl, from a histogram of the sub-block's bit
// lengths. A sub-block that gains 16 bytes or more by it travels as
//     [selector bitmap: 16 bytes, bit i = record i is long][its short deltas at ws bits, in record order, padded to a byte][its long deltas at wl bits, likewise]
// every other one as its deltas at wl bits with ws = wl and NO bitmap (of a sub-block's records only: the last one of a partition is shorter than 16 wl bytes). Two
// width bytes per sub-block in the header ([wl x 64][ws x 64] per block); the 16 sub-blocks of a pack iteration are padded to 16 bytes together, so a block's payload
// [abundance bitmap][sub-blocks] still starts on 16 bytes and leaves LDS as 16-byte words — and since a split gains at least what that padding costs, a block is never
// larger than under one width. ws <= 56 (a host extraction reads 8 bytes at any bit offset).
constexpr uint32_t PKV_SEL = PKV_SUB / 8;                                                         // bytes of a sub-block's selector bitmap
constexpr uint64_t PKVT_CHUNK_MAX = (uint64_t)(PKV_CHUNK / PKV_SUB) * (PKV_SEL + PKV_SUB * 8);    // (an upper bound: a split sub-block is smaller than 128 x 8 bytes)

enum class WireFormat : int { Fixed7, Fixed8, Pkv, PkvTwoWidths, Fixed16, Fixed17, Pkv16 };
constexpr bool wire_pkv(WireFormat f) { return f == WireFormat::Pkv || f == WireFormat::PkvTwoWidths || f == WireFormat::Pkv16; }
constexpr bool wire_key16(WireFormat f) { return f == WireFormat::Fixed16 || f == WireFormat::Fixed17 || f == WireFormat::Pkv16; }
constexpr int wire_entry(WireFormat f) { return f == WireFormat::Fixed7 ? 7 : f == WireFormat::Fixed8 ? 8 : f == WireFormat::Fixed16 ? 16 : f == WireFormat::Fixed17 ? 17 : 0; }
// worst case of a block's payload: every PKV delta at its full 64 / 128 bits (+ every selector bitmap) + the abundance bitmap; a fixed block's slot
constexpr uint64_t wire_block_max(WireFormat f)
{
    return f == WireFormat::Pkv ? (uint64_t)PK_BLOCK * 8 + PKV_BITMAP : f == WireFormat::PkvTwoWidths ? (uint64_t)PK_BLOCK * 8 + (uint64_t)PKV_NSUB * PKV_SEL + PKV_BITMAP
         : f == WireFormat::Pkv16 ? (uint64_t)PK_BLOCK * 16 + PKV_BITMAP : pk_slot(wire_entry(f));
}

// A batch = [bases | abundance-stream offsets | payload offsets | widths | payload | abundance stream | exceptions | counters]; the three middle rows of the header
// exist in the PKV formats only. The decoders read PAST what they decode — 8 bytes at any byte of a fixed entry or a bit-packed stream, 16 with 16-byte keys, 8
// abundance bytes from the cursor — and what they may read into is promised here, once:
//   - every row of the header, the payload and the abundance stream are rounded up to WIRE_ALIGN bytes; a fixed payload carries WIRE_TAIL bytes behind its last slot
//     (they travel: an entry of 7 bytes is read as 8)
//   - WIRE_TAIL bytes follow the exceptions: the device keeps its three counters there, in a staged batch they are the padding behind everything. A stream that
//     fills its rounding exactly is read into the next section, and the last one into these bytes.
constexpr uint64_t WIRE_ALIGN = 64, WIRE_TAIL = 64;
constexpr uint32_t WIRE_EXC_CAP = 1u << 20;                             // exception entries a batch may have (more: it travels unpacked)
constexpr uint64_t wire_round(uint64_t x) { return (x + WIRE_ALIGN - 1) / WIRE_ALIGN * WIRE_ALIGN; }
struct WireLayout {
    uint64_t cboff_off = 0, payoff_off = 0, wbits_off = 0;              // header rows behind the bases (offset 0): u32 per block each, then 64 / 128 width bytes per block
    uint64_t pay_off = 0, pay_cap = 0;                                  // payload: = the header's size; bytes (PKV: of the stream, what a block takes is reserved by its workgroup)
    uint64_t cb_off = 0, cb_cap = 0;                                    // abundance stream
    uint64_t exc_off = 0, exc_cap = 0;                                  // exceptions: entries of 16 bytes
    uint64_t cnt_off = 0;                                               // device: u64 [0] exceptions [1] bytes of the abundance stream [2] bytes of the payload stream
    uint64_t total = 0;
    uint64_t block_max = 0;
};
// the batch as the device packs it: every section at its capacity for nblk blocks of n_rec records in all
constexpr WireLayout wire_layout(WireFormat f, uint64_t nblk, uint64_t n_rec)
{
    WireLayout L;
    const bool pkv = wire_pkv(f);
    L.block_max = wire_block_max(f);
    L.cboff_off = wire_round(nblk * (wire_key16(f) ? 16 : 8));
    L.payoff_off = L.cboff_off + (pkv ? wire_round(nblk * 4) : 0);
    L.wbits_off = L.payoff_off + (pkv ? wire_round(nblk * 4) : 0);
    L.pay_off = L.wbits_off + (pkv ? nblk * PKV_NSUB * (f == WireFormat::PkvTwoWidths ? 2 : 1) : 0);        // (64 or 128 bytes per block: a multiple of WIRE_ALIGN)
    L.pay_cap = nblk * L.block_max + WIRE_TAIL;
    L.cb_off = L.pay_off + L.pay_cap; L.cb_cap = pkv ? wire_round(n_rec) : 0;                              // (one byte per record at most)
    L.exc_off = L.cb_off + L.cb_cap; L.exc_cap = WIRE_EXC_CAP;
    L.cnt_off = L.exc_off + L.exc_cap * 16;
    L.total = L.cnt_off + WIRE_TAIL;
    return L;
}
// the same batch as it travels and is staged: the header as it is, of the PKV payload and the abundance stream what was used (pay_cursor / n_cb bytes), n_exc exceptions
constexpr WireLayout wire_staged(WireFormat f, WireLayout L, uint64_t pay_cursor, uint64_t n_cb, uint64_t n_exc)
{
    if (wire_pkv(f)) L.pay_cap = wire_round(pay_cursor);
    L.cb_off = L.pay_off + L.pay_cap; L.cb_cap = wire_round(n_cb);
    L.exc_off = L.cb_off + L.cb_cap; L.exc_cap = n_exc;
    L.cnt_off = L.exc_off + n_exc * 16;
    L.total = L.cnt_off + WIRE_TAIL;
    return L;
}
// the staging buffer holds the packed stream of ONE pass (like the sink holds one pass of records). 8-byte keys: a record's delta is at most 8 bytes in every
// format, two width bytes per sub-block of the two-width PKV, whole sub-blocks and one worst-case block of slack per partition; 16-byte keys: 17-byte entries
constexpr uint64_t wire_staging_bytes(int key_words, uint64_t sink_bytes, uint64_t nb_partitions)
{
    return key_words == 1 ? sink_bytes / 16 * 8 + (sink_bytes / 16 / PKV_SUB + nb_partitions * PKV_NSUB) * 2 + nb_partitions * (wire_block_max(WireFormat::PkvTwoWidths) + 8) + ((uint64_t)64 << 20)
                          : sink_bytes / 32 * 17 + nb_partitions * (wire_block_max(WireFormat::Fixed17) + 16) + ((uint64_t)64 << 20);
}

// what a decoder needs of a batch
struct WireBatch {
    const uint8_t* stage = nullptr;              // the staged batch (16-byte aligned)
    WireLayout lay; WireFormat fmt = WireFormat::Fixed7;
    uint64_t nblk = 0;
    std::vector<uint64_t> blk_rec0; std::vector<uint32_t> blk_n;       // per block: first record (index in the batch), records
    uint8_t* dest = nullptr;                     // the batch's records in the caller's sink (16-byte aligned)
    std::vector<std::pair<uint64_t, uint64_t>> exc;                    // sorted by (kind | record index)
};
inline void wire_sort_exceptions(WireBatch& B)
{
    const uint64_t* e = reinterpret_cast<const uint64_t*>(B.stage + B.lay.exc_off);
    B.exc.resize(B.lay.exc_cap);
    for (uint64_t i = 0; i < B.lay.exc_cap; i++) B.exc[i] = { e[2 * i], e[2 * i + 1] };
    std::sort(B.exc.begin(), B.exc.end());
}
inline uint64_t wire_lookup(const WireBatch& B, uint64_t tag)
{
    auto it = std::lower_bound(B.exc.begin(), B.exc.end(), std::make_pair(tag, (uint64_t)0));
    return it != B.exc.end() && it->first == tag ? it->second : 0;
}
inline uint32_t wire_escaped(const WireBatch& B, uint32_t ab, uint64_t rec) { return ab == 255u ? (uint32_t)wire_lookup(B, rec) : ab; }
// the abundance of a PKV record: 1, or (flag f) the next byte of the stream. 16 % of the records, at random: no branch on it (the byte under the cursor is read
// either way)
inline uint32_t wire_abundance(const WireBatch& B, const uint32_t f, const uint8_t*& cb, const uint64_t rec)
{
    const uint32_t ab = 1u + f * ((uint32_t)*cb - 1u); cb += f;
    return wire_escaped(B, ab, rec);
}
inline void wire_store(__m128i* out, uint64_t key, uint32_t ab) { _mm_stream_si128(out, _mm_set_epi64x((long long)(uint64_t)ab, (long long)key)); }      // {u64 value; i32 abundance; 4 bytes of padding = 0}
inline void wire_store(__m128i* out, unsigned __int128 key, uint32_t ab)                                                                                   // {u128 value; i32 abundance; 12 bytes of padding = 0}
{
    _mm_stream_si128(out, _mm_set_epi64x((long long)(uint64_t)(key >> 64), (long long)(uint64_t)key));
    _mm_stream_si128(out + 1, _mm_set_epi64x(0ll, (long long)(uint64_t)ab));
}

template <int W> void unpack_fixed(const WireBatch& B, uint64_t g)                       // 8-byte keys, fixed entries
{
    constexpr uint64_t PK_ESC = pk_esc(W);
    const uint8_t* pay = B.stage + B.lay.pay_off + g * pk_slot(W);
    const uint64_t r0 = B.blk_rec0[g]; const uint32_t n = B.blk_n[g];
    uint64_t key = reinterpret_cast<const uint64_t*>(B.stage)[g];
    __m128i* out = reinterpret_cast<__m128i*>(B.dest + r0 * 16);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t w; memcpy(&w, pay + W * (size_t)i, 8);          // (W = 7: one byte beyond the entry)
        const uint64_t d = w & PK_ESC;
        if (i) key = d == PK_ESC ? wire_lookup(B, PK_KEY_EXC | (r0 + i)) : key + d;
        wire_store(out + i, key, wire_escaped(B, (uint32_t)(w >> (8 * (W - 1))) & 255u, r0 + i));
    }
}
template <int W> void unpack_fixed16(const WireBatch& B, uint64_t g)                     // 16-byte keys, fixed entries
{
    typedef unsigned __int128 u128;
    const uint8_t* pay = B.stage + B.lay.pay_off + g * pk_slot(W);
    const uint64_t r0 = B.blk_rec0[g]; const uint32_t n = B.blk_n[g];
    const uint64_t* b2 = reinterpret_cast<const uint64_t*>(B.stage) + 2 * g;
    u128 key = ((u128)b2[1] << 64) | b2[0];
    __m128i* out = reinterpret_cast<__m128i*>(B.dest + r0 * 32);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t lo, hi; memcpy(&lo, pay + W * (size_t)i, 8); memcpy(&hi, pay + W * (size_t)i + 8, 8);      // (W = 16: the 8th byte of `hi` is the abundance)
        if (W == 16) hi &= 0xFFFFFFFFFFFFFFull;
        if (i) {
            if (W == 16 && lo == ~0ull && hi == 0xFFFFFFFFFFFFFFull) key = ((u128)wire_lookup(B, PK_KEY_EXC_HI | (r0 + i)) << 64) | wire_lookup(B, PK_KEY_EXC | (r0 + i));
            else key += ((u128)hi << 64) | lo;
        }
        wire_store(out + 2 * (size_t)i, key, wire_escaped(B, pay[W * (size_t)i + W - 1], r0 + i));
    }
}

// the header of a PKV block, read once for the three PKV decoders
struct PkvBlock {
    uint64_t r0; uint32_t n;
    const uint8_t* wb;                           // its row of widths
    const uint8_t* pay;                          // its sub-blocks
    const uint64_t* bits;                        // its abundance bitmap: behind the sub-blocks, with two widths before them
    const uint8_t* cb;                           // its abundance bytes
    const uint64_t* base;                        // its first key (a block's first delta is 0)
};
inline PkvBlock pkv_block(const WireBatch& B, uint64_t g)
{
    const bool two = B.fmt == WireFormat::PkvTwoWidths;
    PkvBlock K;
    K.r0 = B.blk_rec0[g]; K.n = B.blk_n[g];
    K.wb = B.stage + B.lay.wbits_off + g * PKV_NSUB * (two ? 2 : 1);
    K.pay = B.stage + B.lay.pay_off + ((uint64_t)reinterpret_cast<const uint32_t*>(B.stage + B.lay.payoff_off)[g] << 4);
    uint32_t total = 0;
    if (!two) for (uint32_t s = 0; s < PKV_NSUB; s++) total += 16u * K.wb[s];
    K.bits = reinterpret_cast<const uint64_t*>(K.pay + total);
    if (two) K.pay += PKV_BITMAP;
    K.cb = B.stage + B.lay.cb_off + reinterpret_cast<const uint32_t*>(B.stage + B.lay.cboff_off)[g];
    K.base = reinterpret_cast<const uint64_t*>(B.stage) + (wire_key16(B.fmt) ? 2 : 1) * g;
    return K;
}
// One sub-block of PKV (<= 128 records at width W), W a template constant: 8 records = W bytes, so inside a group every byte offset and shift is a constant
// (the generic loop with a running bit position expanded 1.0e10 records/s on 24 threads — level with the link; this one keeps the margin of the fixed 6-byte format)
template <int W> void pkv_sub(const WireBatch& B, const uint8_t* pay, const uint32_t cnt, const uint64_t rec0, uint64_t& key, const uint64_t* bits /* the sub-block's 2 words */,
                              const uint8_t*& cb, __m128i* out)
{
    constexpr uint64_t mask = W >= 64 ? ~0ull : ((1ull << (W & 63)) - 1ull);
    auto one = [&](const uint32_t i, const uint64_t w, const uint32_t sh, const uint32_t f) { key += (w >> sh) & mask; wire_store(out + i, key, wire_abundance(B, f, cb, rec0 + i)); };
    uint32_t i = 0;
    for (; i + 8 <= cnt; i += 8) {
        const uint8_t* q = pay + (size_t)(i >> 3) * W;
        const uint32_t m = (uint32_t)(bits[i >> 6] >> (i & 63)) & 255u;
GKC_WIRE_UNROLL
        for (int j = 0; j < 8; j++) { uint64_t w; memcpy(&w, q + ((j * W) >> 3), 8); one(i + j, w, (uint32_t)((j * W) & 7), (m >> j) & 1u); }      // (up to 7 bytes beyond the group: the next one / the bitmap)
    }
    for (uint64_t bit = (uint64_t)i * W; i < cnt; i++, bit += W) { uint64_t w; memcpy(&w, pay + (bit >> 3), 8); one(i, w, (uint32_t)(bit & 7), (uint32_t)(bits[i >> 6] >> (i & 63)) & 1u); }
}
typedef void (*pkv_fn)(const WireBatch&, const uint8_t*, uint32_t, uint64_t, uint64_t&, const uint64_t*, const uint8_t*&, __m128i*);
template <size_t... I> const pkv_fn* pkv_table(std::index_sequence<I...>) { static const pkv_fn t[] = { &pkv_sub<(int)I>... }; return t; }
inline void unpack_pkv(const WireBatch& B, uint64_t g)                                    // PKV: one delta width per sub-block of 128 records, no key escapes
{
    static const pkv_fn* const table = pkv_table(std::make_index_sequence<65>());
    PkvBlock K = pkv_block(B, g);
    uint64_t key = K.base[0];
    __m128i* out = reinterpret_cast<__m128i*>(B.dest + K.r0 * 16);
    for (uint32_t s0 = 0; s0 < K.n; s0 += PKV_SUB) {
        const uint32_t W = std::min<uint32_t>(K.wb[s0 / PKV_SUB], 64u);
        table[W](B, K.pay, std::min<uint32_t>(PKV_SUB, K.n - s0), K.r0 + s0, key, K.bits + (s0 >> 6), K.cb, out + s0);
        K.pay += 16u * W;
    }
}
inline void unpack_pkv16(const WireBatch& B, uint64_t g)                                  // PKV, 16-byte keys: 32-byte records {value low, value high, abundance, 0}
{
    typedef unsigned __int128 u128;
    PkvBlock K = pkv_block(B, g);
    u128 key = ((u128)K.base[1] << 64) | K.base[0];
    __m128i* out = reinterpret_cast<__m128i*>(B.dest + K.r0 * 32);
    for (uint32_t s0 = 0; s0 < K.n; s0 += PKV_SUB) {
        const uint32_t W = K.wb[s0 / PKV_SUB], wl = W < 64u ? W : 64u, wh = W - wl;
        const uint64_t ml = wl >= 64 ? ~0ull : (1ull << wl) - 1ull, mh = wh >= 64 ? ~0ull : (1ull << wh) - 1ull;
        uint64_t bit = 0;
        const uint32_t e = std::min<uint32_t>(K.n, s0 + PKV_SUB);
        for (uint32_t i = s0; i < e; i++) {
            u128 x; memcpy(&x, K.pay + (bit >> 3), 16);                      // (16 bytes from any byte: 7 + 64 bits lie inside; up to 15 bytes beyond the entries: the bitmap)
            const uint64_t lo = (uint64_t)(x >> (bit & 7)) & ml; bit += wl;
            uint64_t hi = 0;
            if (wh) { memcpy(&x, K.pay + (bit >> 3), 16); hi = (uint64_t)(x >> (bit & 7)) & mh; bit += wh; }
            key += ((u128)hi << 64) | lo;
            wire_store(out + 2 * (size_t)i, key, wire_abundance(B, (uint32_t)(K.bits[i >> 6] >> (i & 63)) & 1u, K.cb, K.r0 + i));
        }
        K.pay += 16u * W;
    }
}
// PKV with two widths: the deltas of one stream of a sub-block (cnt records at W bits from p) into an array, by the same constant-shift groups of 8
template <int W> void pkv_take(const uint8_t* p, const uint32_t cnt, uint64_t* d)
{
    constexpr uint64_t mask = W >= 64 ? ~0ull : ((1ull << (W & 63)) - 1ull);
    uint32_t i = 0;
    for (; i + 8 <= cnt; i += 8) {
        const uint8_t* q = p + (size_t)(i >> 3) * W;
GKC_WIRE_UNROLL
        for (int j = 0; j < 8; j++) { uint64_t w; memcpy(&w, q + ((j * W) >> 3), 8); d[i + j] = (w >> ((j * W) & 7)) & mask; }      // (up to 7 bytes beyond the group: the next stream / sub-block / what follows the payload)
    }
    for (uint64_t bit = (uint64_t)i * W; i < cnt; i++, bit += W) { uint64_t w; memcpy(&w, p + (bit >> 3), 8); d[i] = (w >> (bit & 7)) & mask; }
}
typedef void (*take_fn)(const uint8_t*, uint32_t, uint64_t*);
template <size_t... I> const take_fn* take_table(std::index_sequence<I...>) { static const take_fn t[] = { &pkv_take<(int)I>... }; return t; }
// a sub-block's two streams merged by the selector bits while the key runs on, from record i on (si short and li long deltas are taken already): the scalar emitter
// (i = 0), and the last records of a partition behind the AVX-512 one
inline void pkv_merge(const WireBatch& B, const uint64_t* sd, const uint64_t* ld, uint32_t si, uint32_t li, const uint64_t* sel, uint32_t i, const uint32_t cnt, const uint64_t rec0,
                      uint64_t& key, const uint64_t* bits, const uint8_t*& cb, __m128i* out)
{
    for (; i < cnt; i++) {
        const uint32_t l = (uint32_t)(sel[i >> 6] >> (i & 63)) & 1u, f = (uint32_t)(bits[i >> 6] >> (i & 63)) & 1u;
        key += l ? ld[li] : sd[si]; li += l; si += 1u - l;                  // (no branch on a bit that is 1 for two records in three)
        wire_store(out + i, key, wire_abundance(B, f, cb, rec0 + i));
    }
}
// The merge and everything behind it, 8 records at a time, where the host has AVX-512 (every host an MI355X sits in does; pkv_merge is what is left without):
// VPEXPANDQ puts the next short and long deltas at the places the selector byte names, three shifted adds and the carried key make the 8 keys, a second expansion
// puts the abundance bytes of the flagged records over the 1s of the others, and two permutes interleave keys and abundances into 8 records. The expansion threads
// cannot be more (24 beside the copy stream: more of them expand LESS), so what a record costs a thread is what decides whether the host keeps up with a link that
// hands over more records per second; measured per batch of 3.1e8 records: profiles/r07_two_widths.txt.
inline bool have_avx512() { static const bool ok = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("popcnt"); return ok; }
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx512f,popcnt")))
inline void pkv_emit512(const WireBatch& B, const uint64_t* sd, const uint64_t* ld, const uint64_t* sel, const uint32_t cnt, const uint64_t rec0, uint64_t& key_io,
                        const uint64_t* bits, const uint8_t*& cb_io, __m128i* out)
{
    const __m512i zero = _mm512_setzero_si512(), one = _mm512_set1_epi64(1), esc255 = _mm512_set1_epi64(255), last = _mm512_set1_epi64(7);
    const __m512i i0 = _mm512_setr_epi64(0, 8, 1, 9, 2, 10, 3, 11), i1 = _mm512_setr_epi64(4, 12, 5, 13, 6, 14, 7, 15);
    const bool aligned = ((uintptr_t)out & 63) == 0;                              // (8 records = 128 bytes: the same for every group of the sub-block)
    __m512i carry = _mm512_set1_epi64((long long)key_io);
    const uint8_t* cb = cb_io;
    uint32_t si = 0, li = 0, i = 0;
    for (; i + 8 <= cnt; i += 8) {
        const __mmask8 m = (__mmask8)(sel[i >> 6] >> (i & 63)), fm = (__mmask8)(bits[i >> 6] >> (i & 63));
        __m512i x = _mm512_mask_expand_epi64(_mm512_maskz_expand_epi64((__mmask8)~m, _mm512_loadu_si512(sd + si)), m, _mm512_loadu_si512(ld + li));
        const uint32_t nl = (uint32_t)__builtin_popcount(m); li += nl; si += 8u - nl;
        x = _mm512_add_epi64(x, _mm512_alignr_epi64(x, zero, 7));
        x = _mm512_add_epi64(x, _mm512_alignr_epi64(x, zero, 6));
        x = _mm512_add_epi64(x, _mm512_alignr_epi64(x, zero, 4));
        x = _mm512_add_epi64(x, carry);
        carry = _mm512_permutexvar_epi64(last, x);
        __m512i ab = _mm512_mask_expand_epi64(one, fm, _mm512_cvtepu8_epi64(_mm_loadl_epi64(reinterpret_cast<const __m128i*>(cb))));      // (8 bytes from the cursor)
        cb += __builtin_popcount(fm);
        const __mmask8 esc = _mm512_cmpeq_epi64_mask(ab, esc255);
        if (esc) {
            alignas(64) uint64_t a8[8]; _mm512_store_si512(a8, ab);
            for (int j = 0; j < 8; j++) if ((esc >> j) & 1) a8[j] = (uint32_t)wire_lookup(B, rec0 + i + j);
            ab = _mm512_load_si512(a8);
        }
        const __m512i lo = _mm512_permutex2var_epi64(x, i0, ab), hi = _mm512_permutex2var_epi64(x, i1, ab);
        if (aligned) { _mm512_stream_si512(reinterpret_cast<__m512i*>(out + i), lo); _mm512_stream_si512(reinterpret_cast<__m512i*>(out + i + 4), hi); }
        else {
            _mm_stream_si128(out + i, _mm512_castsi512_si128(lo)); _mm_stream_si128(out + i + 1, _mm512_extracti32x4_epi32(lo, 1));
            _mm_stream_si128(out + i + 2, _mm512_extracti32x4_epi32(lo, 2)); _mm_stream_si128(out + i + 3, _mm512_extracti32x4_epi32(lo, 3));
            _mm_stream_si128(out + i + 4, _mm512_castsi512_si128(hi)); _mm_stream_si128(out + i + 5, _mm512_extracti32x4_epi32(hi, 1));
            _mm_stream_si128(out + i + 6, _mm512_extracti32x4_epi32(hi, 2)); _mm_stream_si128(out + i + 7, _mm512_extracti32x4_epi32(hi, 3));
        }
    }
    key_io = (uint64_t)_mm_cvtsi128_si64(_mm512_castsi512_si128(carry)); cb_io = cb;
    pkv_merge(B, sd, ld, si, li, sel, i, cnt, rec0, key_io, bits, cb_io, out);     // the last records of a partition
}
#else
void pkv_emit512(const WireBatch&, const uint64_t*, const uint64_t*, const uint64_t*, uint32_t, uint64_t, uint64_t&, const uint64_t*, const uint8_t*&, __m128i*);
#endif
// PKV, a short and a long delta width per sub-block of 128 records: per sub-block the selector and the counts, each stream into an array, one emitter. (An unsplit
// sub-block is one long stream under a selector of ones; the hosts without AVX-512 no longer take the pkv_sub shortcut for it: one path, and every host an MI355X
// sits in takes the AVX-512 emitter either way.)
inline void unpack_pkv_two_widths(const WireBatch& B, uint64_t g, const bool avx512)
{
    static const take_fn* const take = take_table(std::make_index_sequence<65>());
    const PkvBlock K = pkv_block(B, g);
    const uint8_t* cb = K.cb;
    uint64_t key = K.base[0];
    __m128i* out = reinterpret_cast<__m128i*>(B.dest + K.r0 * 16);
    uint32_t off = 0;
    for (uint32_t s0 = 0; s0 < K.n; s0 += PKV_SUB) {
        const uint32_t s = s0 / PKV_SUB, cnt = std::min<uint32_t>(PKV_SUB, K.n - s0);
        const uint32_t wl = std::min<uint32_t>(K.wb[s], 64u), ws = std::min<uint32_t>(K.wb[PKV_NSUB + s], 64u);
        uint64_t sel[2] = { ~0ull, ~0ull }; uint32_t ns = 0, sbytes = 0, skip = 0;
        if (ws != wl) {
            memcpy(sel, K.pay + off, PKV_SEL);
            const uint32_t nl = (uint32_t)(__builtin_popcountll(sel[0]) + __builtin_popcountll(sel[1]));
            ns = cnt - std::min(nl, cnt); sbytes = (ns * ws + 7u) >> 3; skip = PKV_SEL;
        }
        uint64_t d[2][PKV_SUB + 8];                                         // [0] the short deltas, [1] the long ones (+ 8: the AVX-512 emitter loads 8 from any of them)
        if (ns) take[ws](K.pay + off + skip, ns, d[0]);
        take[wl](K.pay + off + skip + sbytes, cnt - ns, d[1]);
        if (avx512) pkv_emit512(B, d[0], d[1], sel, cnt, K.r0 + s0, key, K.bits + (s0 >> 6), cb, out + s0);
        else pkv_merge(B, d[0], d[1], 0, 0, sel, 0, cnt, K.r0 + s0, key, K.bits + (s0 >> 6), cb, out + s0);
        off += skip + sbytes + (((cnt - ns) * wl + 7u) >> 3);
        if ((s & (PKV_CHUNK / PKV_SUB - 1)) == PKV_CHUNK / PKV_SUB - 1) off = (off + 15u) & ~15u;      // a pack iteration's 16 sub-blocks are padded to 16 bytes together
    }
}
inline void unpack_block(const WireBatch& B, uint64_t g, const bool avx512)
{
    switch (B.fmt) {
    case WireFormat::Fixed7: unpack_fixed<7>(B, g); break;
    case WireFormat::Fixed8: unpack_fixed<8>(B, g); break;
    case WireFormat::Pkv: unpack_pkv(B, g); break;
    case WireFormat::PkvTwoWidths: unpack_pkv_two_widths(B, g, avx512); break;
    case WireFormat::Fixed16: unpack_fixed16<16>(B, g); break;
    case WireFormat::Fixed17: unpack_fixed16<17>(B, g); break;
    case WireFormat::Pkv16: unpack_pkv16(B, g); break;
    }
}
