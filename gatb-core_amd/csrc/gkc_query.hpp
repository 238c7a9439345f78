// gkc_query.hpp — what the kernels that search the counted results share: the device table of the datasets, the routing of a k-mer to its dataset and the
// search over the sampled index (gkc_query.hip: abundance queries; gkc_graph.hip: neighbourhoods of the solid k-mers). Device code + the host entry points that
// prepare the index; the description of the search is in gkc_query.hip.
#pragma once
#include "gkc_common.hpp"
#include "gkc_device.hpp"

constexpr uint32_t QR_GRID_MAX = 256 * 8;
constexpr uint32_t Q_MAX_BANKS = 64;

struct QDs { const uint8_t* recs; uint64_t n, idx_off, idx_n, base; };      // device twin of QHostDs + the dataset's samples inside the index
struct QPlanes { const int32_t* plane[Q_MAX_BANKS]; };
struct QParams {
    const uint8_t* bases; uint64_t n_bases; const uint32_t* rsbits; uint64_t n_tiles;
    uint32_t k, m, nb_mm, mmask, mask_ma1; int freq_mode;
    const uint32_t* mkey_lut; const uint32_t* key2val; uint32_t default_key;
    const uint16_t* repart; uint32_t nb_passes, nb_partitions;
    const QDs* ds; const void* samples; uint64_t stride;
    int32_t* out; int32_t* vectors; uint32_t nb_banks;
};

// what k_q_reads answers per position: the abundance of the record found, the sum over the planes of a gkc_banks, or the record's place in the compacted graph
constexpr int QM_COUNTS = 0, QM_BANKS = 1, QM_NODES = 2;
// QM_NODES (gkc_paths.hip): the placement of the flat records (UnitigPlacement::unitig / pos) and the two outputs, u64[n_bases] and u32[n_bases] or NULL
struct QNodes { const uint64_t* unitig; const uint32_t* pos; uint64_t* out_node; uint32_t* out_pos; };
template <int MODE> struct QExtra { typedef QPlanes type; };  // the kernel's second argument
template <> struct QExtra<QM_NODES> { typedef QNodes type; };

template <typename K> __device__ __forceinline__ K q_load_key(const uint8_t* p) { return *reinterpret_cast<const K*>(p); }

// order key of one m-mer given on the forward strand (A3: LUT semantics, restated like k_sample_exact)
__device__ __forceinline__ uint32_t q_mmer_key(const QParams& P, uint32_t mf)
{
    if (P.freq_mode) return P.mkey_lut[mf];
    const uint32_t rc = (uint32_t)revcomp64(mf, P.m);
    const uint32_t cn = mf < rc ? mf : rc;
    uint32_t a = ~(cn | (cn >> 2));
    a = (a >> 1) & a & P.mask_ma1;                            // "AA" anywhere but as prefix (KMC2 rule)
    return a ? P.mmask : cn;
}
__device__ __forceinline__ uint32_t q_dataset_of(const QParams& P, uint32_t min_key)
{
    const uint32_t value = P.freq_mode ? P.key2val[min_key] : min_key;
    return (uint32_t)P.repart[value] + (value % P.nb_passes) * P.nb_partitions;
}

// U searches in lock step. Dataset d[u] is searched for key[u] where act[u]; pos[u] = index of the record inside the dataset when found[u].
// Phase 1 counts the samples <= key (the samples are the records 0, S, 2S ...): none -> the key is below the dataset's first record; else the key can only be in the window
// of S records behind the last such sample. Phase 2 finds the last record <= key of that window. `best` follows the largest value <= key seen, so no load is needed to
// decide found. Lanes / slots that have finished load the first sample of the index (always allocated) and ignore it: the loop body has no divergent branch around a load.
template <typename K, int RB /* bytes from one record's key to the next */, int U>
__device__ __forceinline__ void q_search(const QParams& P, const bool (&act)[U], const uint32_t (&d)[U], const K (&key)[U], bool (&found)[U], uint64_t (&pos)[U],
                                         const uint8_t* (&recs)[U], uint64_t (&base)[U])
{
    const uint8_t* dummy = reinterpret_cast<const uint8_t*>(P.samples);
    const K* ix[U]; uint64_t n[U], lo[U], hi[U]; K best[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const QDs D = P.ds[act[u] ? d[u] : 0u];
        recs[u] = D.recs; n[u] = D.n; base[u] = D.base; ix[u] = reinterpret_cast<const K*>(P.samples) + D.idx_off;
        lo[u] = 0; hi[u] = act[u] ? D.idx_n : 0; best[u] = 0;
    }
    for (;;) {
        bool any = false; K v[U]; uint64_t mid[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool a = lo[u] < hi[u]; any = any || a;
            mid[u] = lo[u] + ((hi[u] - lo[u]) >> 1);
            v[u] = q_load_key<K>(a ? reinterpret_cast<const uint8_t*>(ix[u] + mid[u]) : dummy);
        }
        if (!any) break;
#pragma unroll
        for (int u = 0; u < U; u++) if (lo[u] < hi[u]) { if (v[u] <= key[u]) { lo[u] = mid[u] + 1; best[u] = v[u]; } else hi[u] = mid[u]; }
    }
    // window: records [w0, w1), record w0 = the last sample <= key. Invariant: record lo <= key (its value in best), record hi > key or hi == w1
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        in[u] = lo[u] != 0;                                    // (lo = samples <= key; 0 also for an empty dataset / an idle slot)
        const uint64_t w0 = in[u] ? (lo[u] - 1) * P.stride : 0;
        const uint64_t w1 = in[u] ? (n[u] - w0 < P.stride ? n[u] : w0 + P.stride) : 0;
        lo[u] = w0; hi[u] = w1;
    }
    for (;;) {
        bool any = false; K v[U]; uint64_t mid[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool a = in[u] && hi[u] - lo[u] > 1; any = any || a;
            mid[u] = lo[u] + ((hi[u] - lo[u]) >> 1);
            v[u] = q_load_key<K>(a ? recs[u] + mid[u] * (uint64_t)RB : dummy);
        }
        if (!any) break;
#pragma unroll
        for (int u = 0; u < U; u++) if (in[u] && hi[u] - lo[u] > 1) { if (v[u] <= key[u]) { lo[u] = mid[u]; best[u] = v[u]; } else hi[u] = mid[u]; }
    }
#pragma unroll
    for (int u = 0; u < U; u++) { found[u] = in[u] && best[u] == key[u]; pos[u] = lo[u]; }
}

// ------------------------------------------------------------------------------------------------ host side (gkc_query.hip)
unsigned q_grid(uint64_t n_blocks);
void q_fill_params(QParams& P, const QueryModel& M, const QueryIndex& ix);
// the guards of gkc_release_pass and of the whole-context consumers, then the index over what the context holds NOW (QDs::base = the dataset's first record in dataset order)
int q_prepare(gkc_ctx* c, const char* who);
QueryModel q_model_of(const gkc_ctx* c);
