// The host decoders of the packed result batches (csrc/gkc_wire.hpp) without a GPU: a deliberately plain encoder — one record at a time, a bit cursor, written from the
// format's description in the header, NOT the pack kernels' width rule (any valid choice of widths decodes) — lays a batch out with the header's own layout function
// into a heap buffer of exactly the size that function gives (a read beyond the promised padding is a read beyond the allocation), every block is decoded with
// unpack_block and the sink is compared with the records, byte for byte, padding words included.
//   stdin:  format F (WireFormat as a number) | avx512 0/1 | dest_offset BYTES | short WS (two widths: the short width of every sub-block whose long width is above it;
//           -1: none is split) | parts N n_1 .. n_N | records N, then N lines "key_hi key_lo abundance" (hex hex decimal)
//   stdout: "ok records R blocks B payload P abundance_bytes C exceptions E sink HASH"; anything wrong: a message on stderr and exit status 1
#include "gkc_wire.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

typedef unsigned __int128 u128;
struct Rec { u128 key; uint32_t ab; };

static void fail(const char* what, uint64_t a = 0, uint64_t b = 0) { fprintf(stderr, "wire_driver: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b); exit(1); }
static uint32_t bit_length(u128 d) { uint32_t n = 0; while (d) { n++; d >>= 1; } return n; }
// w bits of v at bit `bit` of p, the lowest first
static void put_bits(uint8_t* p, uint64_t& bit, u128 v, uint32_t w)
{
    for (uint32_t b = 0; b < w; b++, bit++) if ((v >> b) & 1) p[bit >> 3] |= (uint8_t)(1u << (bit & 7));
}

struct Encoder {
    WireFormat fmt; int kw; int ws_case;
    std::vector<uint64_t> bases; std::vector<uint32_t> cb_off, pay_off16; std::vector<uint8_t> wbits, payload, cb;
    std::vector<std::pair<uint64_t, uint64_t>> exc;

    uint8_t abundance8(uint64_t rec, uint32_t ab) { if (ab >= 255u) { exc.push_back({ rec, ab }); return 255; } return (uint8_t)ab; }
    void fixed_block(uint64_t g, const Rec* r, uint64_t r0, uint32_t n)
    {
        const int W = wire_entry(fmt);
        uint8_t* p = payload.data() + g * pk_slot(W);
        const u128 esc = W == 17 ? ~(u128)0 : ((u128)1 << (8 * (W - 1))) - 1;    // the delta field's all-ones
        for (uint32_t i = 0; i < n; i++) {
            u128 d = i ? r[i].key - r[i - 1].key : 0;
            if (kw == 1) d = (uint64_t)d;
            if (W != 17 && d >= esc) {                                      // (a 16-byte field holds every delta)
                d = esc;
                exc.push_back({ PK_KEY_EXC | (r0 + i), (uint64_t)r[i].key });
                if (kw == 2) exc.push_back({ PK_KEY_EXC_HI | (r0 + i), (uint64_t)(r[i].key >> 64) });
            }
            uint64_t bit = 8 * (uint64_t)W * i;
            put_bits(p, bit, d, 8 * (W - 1));
            put_bits(p, bit, abundance8(r0 + i, r[i].ab), 8);
        }
    }
    void pkv_block(uint64_t g, const Rec* r, uint64_t r0, uint32_t n)
    {
        const bool two = fmt == WireFormat::PkvTwoWidths;
        const uint32_t nsub = (n + PKV_SUB - 1) / PKV_SUB;
        std::vector<u128> d(n);
        for (uint32_t i = 0; i < n; i++) { d[i] = i ? r[i].key - r[i - 1].key : 0; if (kw == 1) d[i] = (uint64_t)d[i]; }
        uint8_t* wb = wbits.data() + g * PKV_NSUB * (two ? 2 : 1);
        std::vector<uint8_t> subs((size_t)wire_block_max(fmt), 0), bitmap(PKV_BITMAP, 0);
        uint64_t bit = 0;
        for (uint32_t s = 0; s < nsub; s++) {
            const uint32_t i0 = s * PKV_SUB, cnt = std::min(PKV_SUB, n - i0);
            uint32_t wl = 0;
            for (uint32_t i = 0; i < cnt; i++) wl = std::max(wl, bit_length(d[i0 + i]));
            if (kw == 1 && wl > 56) wl = 64;
            wb[s] = (uint8_t)wl;
            if (!two) {                                                     // 16 wl bytes, whole
                const uint64_t start = bit;
                for (uint32_t i = 0; i < cnt; i++) {
                    if (kw == 1) put_bits(subs.data(), bit, d[i0 + i], wl);
                    else { const uint32_t lo = std::min(wl, 64u); put_bits(subs.data(), bit, (uint64_t)d[i0 + i], lo); put_bits(subs.data(), bit, d[i0 + i] >> 64, wl - lo); }
                }
                bit = start + 8 * 16 * (uint64_t)wl;
                continue;
            }
            const bool split = ws_case >= 0 && (uint32_t)ws_case < wl;
            const uint32_t ws = split ? (uint32_t)ws_case : wl;
            wb[PKV_NSUB + s] = (uint8_t)ws;
            if (split) {
                uint64_t sel = bit; bit += 8 * PKV_SEL;
                for (uint32_t i = 0; i < cnt; i++) if (bit_length(d[i0 + i]) > ws) put_bits(subs.data(), sel, 1, 1); else sel++;
                for (uint32_t i = 0; i < cnt; i++) if (bit_length(d[i0 + i]) <= ws) put_bits(subs.data(), bit, d[i0 + i], ws);
                bit = (bit + 7) / 8 * 8;
            }
            for (uint32_t i = 0; i < cnt; i++) if (!split || bit_length(d[i0 + i]) > ws) put_bits(subs.data(), bit, d[i0 + i], wl);
            bit = (bit + 7) / 8 * 8;
            if (s % (PKV_CHUNK / PKV_SUB) == PKV_CHUNK / PKV_SUB - 1) bit = (bit + 127) / 128 * 128;      // the 16 sub-blocks of a pack iteration are padded to 16 bytes together
        }
        bit = (bit + 127) / 128 * 128;                                      // (a block's payload is reserved in 16-byte units)
        cb_off[g] = (uint32_t)cb.size();
        for (uint32_t i = 0; i < n; i++) if (r[i].ab != 1) { bitmap[i >> 3] |= (uint8_t)(1u << (i & 7)); cb.push_back(abundance8(r0 + i, r[i].ab)); }
        if (payload.size() % 16) fail("payload not on 16 bytes");
        pay_off16[g] = (uint32_t)(payload.size() / 16);
        if (two) payload.insert(payload.end(), bitmap.begin(), bitmap.end());
        payload.insert(payload.end(), subs.begin(), subs.begin() + bit / 8);
        if (!two) payload.insert(payload.end(), bitmap.begin(), bitmap.end());
        if (bit / 8 + PKV_BITMAP > wire_block_max(fmt)) fail("block above its worst case", bit / 8);
    }
};

int main()
{
    int format = -1, avx512 = 0, ws_case = -1; unsigned long long dest_offset = 0, n_rec = 0;
    std::vector<uint64_t> parts; std::vector<Rec> recs;
    char word[64];
    while (scanf("%63s", word) == 1) {
        const std::string w = word;
        if (w == "format") { if (scanf("%d", &format) != 1) fail("format"); }
        else if (w == "avx512") { if (scanf("%d", &avx512) != 1) fail("avx512"); }
        else if (w == "short") { if (scanf("%d", &ws_case) != 1) fail("short"); }
        else if (w == "dest_offset") { if (scanf("%llu", &dest_offset) != 1) fail("dest_offset"); }
        else if (w == "parts") { unsigned long long n, v; if (scanf("%llu", &n) != 1) fail("parts"); for (; n; n--) { if (scanf("%llu", &v) != 1) fail("parts"); parts.push_back(v); } }
        else if (w == "records") {
            if (scanf("%llu", &n_rec) != 1) fail("records");
            for (unsigned long long i = 0; i < n_rec; i++) { unsigned long long hi, lo; unsigned ab; if (scanf("%llx %llx %u", &hi, &lo, &ab) != 3) fail("record", i); recs.push_back({ ((u128)hi << 64) | lo, ab }); }
        } else fail("unknown word");
    }
    if (format < 0 || format > 6) fail("no format");
    if (avx512 && !have_avx512()) fail("this CPU has no AVX-512");
    if (parts.empty()) parts.push_back(n_rec);
    Encoder E; E.fmt = (WireFormat)format; E.kw = wire_key16(E.fmt) ? 2 : 1; E.ws_case = ws_case;
    const size_t rec_bytes = 16 * (size_t)E.kw;

    WireBatch B; B.fmt = E.fmt;
    uint64_t r = 0;
    for (uint64_t n : parts) { for (uint64_t i = 0; i < n; i += PK_BLOCK) { B.blk_rec0.push_back(r + i); B.blk_n.push_back((uint32_t)std::min<uint64_t>(PK_BLOCK, n - i)); } r += n; }
    if (r != n_rec) fail("the partitions do not add up", r, n_rec);
    const uint64_t nblk = B.nblk = B.blk_n.size();
    const WireLayout cap = wire_layout(E.fmt, nblk, n_rec);
    E.bases.resize(nblk * E.kw); E.cb_off.resize(nblk); E.pay_off16.resize(nblk);
    if (wire_pkv(E.fmt)) E.wbits.assign(nblk * PKV_NSUB * (E.fmt == WireFormat::PkvTwoWidths ? 2 : 1), 0); else E.payload.assign(nblk * cap.block_max, 0);
    for (uint64_t g = nblk; g-- > 0; ) {                                    // (the last block first: the order of the blocks in the streams is whatever it came out as)
        const Rec* first = recs.data() + B.blk_rec0[g];
        E.bases[E.kw * g] = (uint64_t)first->key; if (E.kw == 2) E.bases[2 * g + 1] = (uint64_t)(first->key >> 64);
        if (wire_pkv(E.fmt)) E.pkv_block(g, first, B.blk_rec0[g], B.blk_n[g]); else E.fixed_block(g, first, B.blk_rec0[g], B.blk_n[g]);
    }
    if (E.payload.size() > cap.pay_cap || E.cb.size() > cap.cb_cap || E.exc.size() > cap.exc_cap) fail("a section above its capacity");

    // the staged batch, exactly as large as the layout says, every byte the encoder does not set is 0xA5
    const WireLayout L = B.lay = wire_staged(E.fmt, cap, E.payload.size(), E.cb.size(), E.exc.size());
    void* mem = nullptr;
    if (posix_memalign(&mem, 64, L.total)) fail("no memory");
    uint8_t* stage = (uint8_t*)mem;
    memset(stage, 0xA5, L.total);
    auto place = [&](uint64_t off, const void* src, size_t bytes, uint64_t end) { if (off + bytes > end) fail("a section above its place", off + bytes, end); if (bytes) memcpy(stage + off, src, bytes); };
    place(0, E.bases.data(), E.bases.size() * 8, L.cboff_off);
    if (wire_pkv(E.fmt)) {
        place(L.cboff_off, E.cb_off.data(), nblk * 4, L.payoff_off);
        place(L.payoff_off, E.pay_off16.data(), nblk * 4, L.wbits_off);
        place(L.wbits_off, E.wbits.data(), E.wbits.size(), L.pay_off);
    }
    place(L.pay_off, E.payload.data(), E.payload.size(), L.cb_off);
    place(L.cb_off, E.cb.data(), E.cb.size(), L.exc_off);
    std::reverse(E.exc.begin(), E.exc.end());                               // (the device appends them in any order)
    place(L.exc_off, E.exc.data(), E.exc.size() * 16, L.cnt_off);
    B.stage = stage;
    wire_sort_exceptions(B);

    void* sink = nullptr;
    if (posix_memalign(&sink, 64, dest_offset + n_rec * rec_bytes + 64)) fail("no memory");
    memset(sink, 0x5A, dest_offset + n_rec * rec_bytes + 64);
    B.dest = (uint8_t*)sink + dest_offset;
    for (uint64_t g = 0; g < nblk; g++) unpack_block(B, g, avx512 != 0);
    _mm_sfence();

    uint64_t hash = 1469598103934665603ull;
    for (uint64_t i = 0; i < n_rec; i++) {
        uint64_t want[4] = { (uint64_t)recs[i].key, E.kw == 2 ? (uint64_t)(recs[i].key >> 64) : recs[i].ab, E.kw == 2 ? recs[i].ab : 0, 0 };
        if (memcmp(B.dest + i * rec_bytes, want, rec_bytes)) fail("the sink differs from the records at record", i, n_rec);
        for (size_t b = 0; b < rec_bytes; b++) hash = (hash ^ B.dest[i * rec_bytes + b]) * 1099511628211ull;
    }
    for (uint64_t b = 0; b < 64; b++) if (B.dest[n_rec * rec_bytes + b] != 0x5A) fail("written beyond the batch's records", b);
    for (uint64_t b = 0; b < dest_offset; b++) if (((uint8_t*)sink)[b] != 0x5A) fail("written before the batch's records", b);
    printf("ok records %llu blocks %llu payload %llu abundance_bytes %llu exceptions %llu sink %016llx\n", n_rec, (unsigned long long)nblk, (unsigned long long)E.payload.size(),
           (unsigned long long)E.cb.size(), (unsigned long long)E.exc.size(), (unsigned long long)hash);
    free(sink); free(mem);
    return 0;
}
