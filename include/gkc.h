/* gkc.h — C-ABI of libgkc_hip.so: the MI355X (gfx950) implementation of GATB-Core's DSK k-mer-counting hot path.
 *
 * This is the drop-in boundary. Everything crossing it is plain C: pointers, sizes, integers.
 * No C++ exceptions, STL or torch types cross the ABI. Every function returns 0 on success, non-zero on error
 * (then gkc_last_error() describes it). The host-side C++ classes in gatb-core_amd/host/ (mirrors of
 * gatb::core::kmer::impl::SortingCountAlgorithm<span>, ICountProcessor<span>, IBloom<Item>) and the Python binding
 * gatb-core_amd/gkc.py call nothing else.
 *
 * Reference citations are file:line under /root/reference/gatb-core/src/gatb/.
 *
 * Data conventions (identical to the reference):
 *   nucleotide code  (c>>1)&3 : A=0 C=1 T=2 G=3, anything outside ACGTacgt is invalid   (tools/misc/api/Data.hpp:185)
 *   k-mer integer    first nucleotide in the most significant used bits                  (kmer/impl/Model.hpp:637-657)
 *   canonical        min(forward, reverse complement)                                    (kmer/impl/Model.hpp:294)
 *   Count record     k<=31: 16 B {u64 value; i32 abundance; 4 B pad}
 *                    k<=63: 32 B {u128 value (little endian); i32 abundance; 12 B pad}   (tools/misc/api/Abundance.hpp:68-129)
 */
#ifndef GKC_H
#define GKC_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is compiled with -fvisibility=hidden and linked with a version script (csrc/gkc.map): the declarations below are its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define GKC_OK            0
#define GKC_ERR_ARG       1   /* bad argument / bad state                        */
#define GKC_ERR_HIP       2   /* a HIP runtime call failed (message has details) */
#define GKC_ERR_NOMEM     3   /* device or host allocation failed                */
#define GKC_ERR_CAPACITY  4   /* caller buffer too small                         */
#define GKC_ERR_NODEVICE  5   /* no usable gfx950 device                         */
#define GKC_ERR_FORMAT    6   /* input text the device parser refuses (see gkc_fastx_parse_device) */

#define GKC_MINIMIZER_LEXI 0  /* -minimizer-type 0: lexicographic + KMC2 "no inner AA" rule (Model.hpp:1220-1251) */
#define GKC_MINIMIZER_FREQ 1  /* -minimizer-type 1: (freq_order[c], c) order (Model.hpp:957-973)                  */

typedef struct gkc_ctx gkc_ctx;

/* ---------------------------------------------------------------------------------------------------------------
 * Context. Replaces the per-run state of SortingCountAlgorithm<span> (kmer/impl/SortingCountAlgorithm.hpp:65-263):
 * owns the HIP stream, every device buffer and the per-pass results.
 * ------------------------------------------------------------------------------------------------------------- */
int         gkc_create(int device, gkc_ctx** out);
/* Objects built from a context (gkc_bloom, gkc_mphf, gkc_comm) hold device memory of its allocator and keep it alive: gkc_destroy may be
 * called first, the context is then released when the last of them is destroyed. */
void        gkc_destroy(gkc_ctx* ctx);
const char* gkc_last_error(const gkc_ctx* ctx);      /* ctx may be NULL: last error of a failed gkc_create */
const char* gkc_version(void);

/* Model + Repartitor. Replaces `Model model(k, m, cmp, freq_order)` (SortingCountAlgorithm.cpp:1251-1256, LUT built at
 * Model.hpp:1032-1064) and `Repartitor::operator()` (kmer/impl/PartiInfo.hpp:323).
 *   repart      u16[4^m]  minimizer value -> partition  (the table Repartitor::load reads, PartiInfo.cpp:223-262)
 *   freq_order  u32[4^m]  or NULL; required iff minimizer_type==GKC_MINIMIZER_FREQ (RepartitionAlgorithm.cpp:311-384)
 * k in [3,63] (k<=2 refused like SortingCountAlgorithm.cpp:662-666), m in [2,min(k-1,14)], nb_partitions in [1,65535].
 * Sizing: Stage B is planned for partitions of 2e6 .. 4e6 k-mers (what gkc_device_memory-driven callers and the drop-in's DeviceConfiguration choose: ~4000
 * partitions for 1e8 reads of 150 bp). Any count is correct; partitions beyond 8e6 k-mers are expanded by several workgroups each but skip the record
 * deduplication and send their sub-buckets through one split level (256 partitions for 1e8 reads: 375 ms per pass against 203 ms with 4096). */
int gkc_configure(gkc_ctx* ctx, uint32_t k, uint32_t m, uint32_t nb_partitions, uint32_t nb_passes,
                  int minimizer_type, const uint16_t* repart, const uint32_t* freq_order);

/* Solidity window and histogram length. Replaces CountProcessorSoliditySum::check (CountProcessorSolidity.hpp:186-189,
 * closed interval on the sum) and Histogram::inc clamping (tools/misc/impl/Histogram.hpp:92). Defaults: [1, INT32_MAX],
 * histo_max 10000, i.e. every distinct k-mer is returned and the host's own processor chain can do the filtering. */
int gkc_set_solidity(gkc_ctx* ctx, int32_t abundance_min, int32_t abundance_max, uint32_t histo_max);

/* Super-k-mer length cap (Sequence2SuperKmer.hpp:147). 0 = reference default 28 (k<=31) / 60 (k<=63). */
int gkc_set_max_superkmer(gkc_ctx* ctx, uint32_t maxs);

/* Upper bound on the k-mers of one Stage-B batch (0 = the library's plan). Stage B counts a pass in batches of whole partitions; their size sets the working set
 * in HBM (about 22 bytes per k-mer of a batch, two batches in flight) and how often the chip drains between batches. The library's own plan is made for a host
 * that counts pass after pass in one process: few, large batches (3.2e9 k-mers with 8-byte keys: 10^8 reads = 4 batches, 130 GB of working set, every block reused
 * by the next pass). A host that counts ONE pass per process — dbgh5 — asks for less: 2^30 k-mers per batch cost 8 % of Stage B (157 vs 145 ms at 10^8 reads) and
 * take 46 GB, and a machine whose memory is handed out slowly the first time (28 ms per GB beyond ~120 GB on a freshly booted MI355X box: profiles/
 * r05_cold_pass.txt) does not charge the difference to the one pass there is. The reference's counterpart is the memory the partitions of a pass are sized for
 * (-max-memory, ConfigurationAlgorithm.cpp:398-425). Results do not depend on it. */
int gkc_set_batch_keys(gkc_ctx* ctx, uint64_t max_keys);

/* ---------------------------------------------------------------------------------------------------------------
 * Repartitor sampling — device side of RepartitorAlgorithm (kmer/impl/RepartitionAlgorithm.cpp:287-492). The tables
 * themselves (computeDistrib / justGroup / justGroupLexi, kmer/impl/PartiInfo.cpp:48-218, and the frequency ranking,
 * RepartitionAlgorithm.cpp:352-380) are built by the host from these statistics, like the reference does.
 *   gkc_sample_minimizers : per minimizer value, number of super-k-mers and of k-mers of the sample under the CURRENT model
 *                           (PartiInfo::incSuperKmer_per_minimBin); arrays of 4^m u64, ACCUMULATED into.
 *   gkc_count_mmers       : occurrences of every canonical m-mer at valid positions (MmersFrequency functor, :88-120);
 *                           u32[4^m], ACCUMULATED into.
 * ------------------------------------------------------------------------------------------------------------- */
int gkc_sample_minimizers(gkc_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads,
                          uint64_t* superkmers_per_minim, uint64_t* kmers_per_minim);
int gkc_count_mmers(gkc_ctx* ctx, uint32_t m, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t* counts);
/* The EXACT sample of RepartitorAlgorithm::computeRepartition (RepartitionAlgorithm.cpp:395-475): the reads are walked one by one like
 * Sequence2SuperKmer does (no tiles), the sample stops with the read in which the running number of super-k-mers of pass 0 (of the context's
 * nb_passes: the reference's SampleRepart is a ONE-pass Sequence2SuperKmer, :225, so its callers configure 1 pass for the sample) first exceeds
 * max_superkmers (SampleRepart::processSuperkmer :205-212 sets the cancel flag, checked between sequences), and per minimizer value the
 * super-k-mers, k-mers AND kx-mers are counted (:186-203, _kx = 4) — the last being what Repartitor::computeDistrib balances on
 * (PartiInfo.cpp:48-106). Arrays of 4^m u64 (any may be NULL), ACCUMULATED into; *reads_used = reads of the sample. */
int gkc_sample_exact(gkc_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t max_superkmers,
                     uint64_t* superkmers_per_minim, uint64_t* kmers_per_minim, uint64_t* kxmers_per_minim, uint64_t* reads_used);

/* ---------------------------------------------------------------------------------------------------------------
 * Stage A — replaces SortingCountAlgorithm::fillPartitions (SortingCountAlgorithm.cpp:1211-1344): Sequence2SuperKmer
 * (Sequence2SuperKmer.hpp:81-159) + FillPartitions::processSuperkmer (:1081-1151) + the SuperKmerBinFiles disk shuffle
 * (tools/storage/impl/Storage.cpp:360-430). Reads arrive as a flat ASCII buffer + CSR offsets (offsets[n_reads] ==
 * number of bases); any number of pushes per pass. Super-k-mers whose minimizer % nb_passes != pass are dropped (:1083).
 * ------------------------------------------------------------------------------------------------------------- */
int gkc_begin_pass(gkc_ctx* ctx, uint32_t pass);
int gkc_push_reads(gkc_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads);
/* same, inputs already resident in HBM (d_bases 16-byte aligned). The buffers may be released after the call returns.
 * A push is one segment of super-k-mer records with its own per-push buffers (about 0.8 bytes of descriptors per base besides the records): pushes of up to ~10^8 reads
 * (1.5*10^10 bases) are what those are sized for; a larger input is pushed in several calls (any number per pass). */
int gkc_push_reads_device(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases);

/* Stage B — replaces SortingCountAlgorithm::fillSolidKmers (:1384-1602) = PartitionsByVectorCommand read/sort/dump
 * (kmer/impl/PartitionsCommand.cpp:1206-1805) for every partition of the pass, plus the default processor chain
 * histogram -> solidity -> dump (CountProcessorChain.hpp:128-135). Results stay in HBM until fetched. */
int gkc_finish_pass(gkc_ctx* ctx);

/* Streamed results (the wall ends when the last partition's Count[] is in host memory). With a host sink set, every Stage-B
 * batch is copied into it on a copy stream as soon as it is compacted, while the next batches are counted: the reference's sink it stands
 * in for is CountProcessorDump -> BagCache -> CollectionHDF5Patch (CountProcessorDump.hpp:148-152, CollectionHDF5Patch.hpp:262-308), fed per
 * partition by the dump threads. The sink must be page-locked (gkc_host_alloc) and holds ONE pass (gkc_begin_pass rewinds it); what does
 * not fit stays on the device and gkc_finish_pass reports GKC_ERR_CAPACITY in gkc_last_error while still returning 0 records lost.
 * On the link the batches travel PACKED (base key per block of 8192 records + key deltas bit-packed at the width of their sub-block of 128 records + a bitmap and a
 * stream of the abundances that are not 1: 5.8 of the 16 bytes of a record at k = 31, 14.5 of the 32 at k = 63, 10^8 reads; 7 - 8 / 16 - 17 with fixed-width entries
 * where the partitions are sparse) and are expanded into the exact Count[] layout inside the sink by threads of the library; what gkc_wait_partition hands out
 * is byte for byte what gkc_partition_counts gives.
 *   gkc_finish_pass_async : Stage B on a worker thread of the library; returns at once.
 *   gkc_wait_partition    : blocks until dataset (pass, part) is counted and, with a sink, has landed; *host_records points into the sink
 *                           (NULL without a sink / for what did not fit). Partitions complete in ascending order inside a batch, batches in
 *                           ascending order per lane: a consumer walking the partitions in order overlaps its work with Stage B.
 *   gkc_finish_pass_wait  : joins the worker; the pass is finished like after gkc_finish_pass. If Stage B FAILED on the worker (e.g. GKC_ERR_NOMEM) and the
 *                           context has not begun another pass meanwhile, the pass is in progress again — as after a failed gkc_finish_pass — and
 *                           gkc_finish_pass / gkc_finish_pass_async may be called again (the retry of gkc_count_pass). */
int gkc_set_host_sink(gkc_ctx* ctx, void* pinned_host, uint64_t cap_bytes);     /* NULL: no sink */
/* How the batches cross the link, chosen before gkc_set_host_sink (default GKC_SINK_PACKED):
 *   GKC_SINK_PACKED  as described above: 0.4x of the bytes on the link, and per record 6.3 B read + 16 B of non-temporal stores by CPU threads of this host;
 *   GKC_SINK_RAW     the Count[] of every batch lands at its place in the sink by ONE DMA copy: 16 / 32 B per record on the link, NO host core touches a byte.
 * One rank per host: packed (the link is the bound). Several ranks sharing ONE host's DRAM (8 GPUs of a node, each with its own PCIe link): the expansion threads of all
 * ranks meet at the host's memory controllers (104 B of host traffic per record packed against 16 raw) — the launcher measures one step each way and keeps the faster
 * (bench.py does; DESIGN.md section 5 has the numbers). Both modes leave byte for byte the same sink. */
#define GKC_SINK_PACKED 0
#define GKC_SINK_RAW    1
int gkc_set_sink_mode(gkc_ctx* ctx, int mode);
int gkc_finish_pass_async(gkc_ctx* ctx);
int gkc_wait_partition(gkc_ctx* ctx, uint32_t pass, uint32_t part, const void** host_records, uint64_t* n_solid);
int gkc_finish_pass_wait(gkc_ctx* ctx);

/* Result of dataset (part + pass*nb_partitions) (CountProcessorDump.hpp:131): ascending Count records of the SOLID
 * k-mers, in the exact in-memory layout of Kmer<span>::Count so the host can pass whole arrays to
 * Bag<Count>::insert(const Item*, len) (tools/storage/impl/CollectionHDF5Patch.hpp:262). */
int gkc_partition_info(gkc_ctx* ctx, uint32_t pass, uint32_t part,
                       uint64_t* n_solid, uint64_t* n_distinct, uint64_t* n_kmers);
int gkc_partition_counts(gkc_ctx* ctx, uint32_t pass, uint32_t part, void* out_counts, uint64_t cap_records,
                         uint64_t* n_solid);
/* records [first, first + n) of the dataset into `out` — for a consumer that moves a partition through page-locked buffers smaller than the partition
 * (integration/gatb_device/DeviceCounting.hpp: a ring of 4 MiB slots between the link and the .h5 file). Same stream and ordering as gkc_partition_counts. */
int gkc_partition_counts_range(gkc_ctx* ctx, uint32_t pass, uint32_t part, uint64_t first, uint64_t n, void* out_counts);
/* device pointer to the same records (valid until gkc_begin_pass of the same pass index or gkc_destroy) */
int gkc_partition_counts_device(gkc_ctx* ctx, uint32_t pass, uint32_t part, const void** d_counts, uint64_t* n_solid);

/* Histogram of abundances over ALL distinct k-mers (CountProcessorHistogram.hpp:173-184): histo_max+1 bins. */
int gkc_histogram(gkc_ctx* ctx, uint64_t* out, uint32_t n_bins);

/* Counters the reference reports through getInfo() (SortingCountAlgorithm.cpp:728-780, Sequence2SuperKmer.hpp:103,108) */
typedef struct gkc_stats {
    uint64_t kmers_nb_valid;      /* pass 0 only, like the reference                      */
    uint64_t kmers_nb_invalid;
    uint64_t kmers_nb_distinct;   /* summed over finished passes                          */
    uint64_t kmers_nb_solid;
    uint64_t nb_superkmers;       /* device records (tile boundaries may add a few splits) */
    uint64_t nb_sequences;        /* pass 0 only                                          */
    uint64_t nb_bases;            /* pass 0 only                                          */
    uint64_t superkmer_bytes;     /* bytes of the device record buckets                   */
    uint64_t oversize_buckets;    /* sub-buckets that took the global-memory sort path    */
    uint64_t dedupe_kmers_in;     /* k-mers of the record bins that were deduplicated before the expansion (Stage B, k <= 31) ... */
    uint64_t dedupe_keys_out;     /* ... and the weighted keys they became (0 / 0: the step did not run)                          */
    uint64_t seq_len_min;         /* pass 0 only: shortest / longest read and the sum of the squared read lengths — what BankStats::update keeps   */
    uint64_t seq_len_max;         /* (BankKmers.hpp:164-200: seq_size_min / max / deviation of getInfo(), SortingCountAlgorithm.cpp:735-739);       */
    uint64_t seq_len_sq_sum;      /* seq_len_min is 0 when no read was pushed                                                                       */
    uint64_t reserved[2];         /* [0] reads pushed in the CURRENT pass (nb_sequences is pass 0's); [1] bytes the packed result batches of the last counted pass took on
                                     the link to the host sink (gkc_set_host_sink; 0: nothing travelled packed)                                                       */
} gkc_stats;
int gkc_get_stats(gkc_ctx* ctx, gkc_stats* out);

/* Kernel timing of the last gkc_finish_pass / pushes (HIP events on the context's stream), milliseconds.
 * names: "scan_count", "scan_emit", "expand_count", "expand_scatter", "bucket_sort", "compact", "total_stage_a", "total_stage_b";
 * of the abundance queries (accumulated since gkc_configure): "query_index", "query_reads", "query_kmers"; of the graph neighbourhoods: "graph_neighbors",
 * "graph_branching"; of the unitigs: "graph_links", "graph_rank", "graph_emit", "graph_unitig_links"; of the tip removal: "graph_tips";
 * of the bulges and erroneous connections: "graph_bulges", "graph_ec" */
int gkc_get_timing(gkc_ctx* ctx, const char* name, double* ms, uint64_t* launches);

/* ---------------------------------------------------------------------------------------------------------------
 * Parity / exchange surface for the super-k-mer buckets (the device analogue of SuperKmerBinFiles).
 * ------------------------------------------------------------------------------------------------------------- */
/* Partition `part` of the current pass re-encoded in the REFERENCE wire format: concatenated
 * [u8 nbK][ceil((k+nbK-1)/4) bytes] records (Model.hpp:1386-1471, Storage.cpp:567-580). Order of records is unspecified. */
int gkc_partition_superkmers(gkc_ctx* ctx, uint32_t part, uint8_t* out, uint64_t cap_bytes,
                             uint64_t* n_bytes, uint64_t* n_superkmers, uint64_t* n_kmers);

/* Segment surface (parity tests, custom exchanges): records of partition p occupy rec_index in [rec_offsets[p], rec_offsets[p+1]) of the
 * segment's arena; record_bytes is 16 (k<=31) or 32.
 * gkc_segment_export: segment `seg` (one per push) of the current pass. d_records stays owned by the context.
 * gkc_segment_import: adds a foreign segment; the memory stays owned by the caller and must outlive gkc_finish_pass.
 * gkc_segments_clear: forget all segments of the current pass (frees owned arenas). The multi-GPU exchange itself is gkc_exchange below. */
int gkc_segment_count(gkc_ctx* ctx, uint32_t* n_segments);
int gkc_segment_export(gkc_ctx* ctx, uint32_t seg, const void** d_records, uint32_t* record_bytes,
                       uint64_t* rec_offsets /* [nb_partitions+1] */, uint64_t* kmers_per_partition /* [nb_partitions] */);
int gkc_segment_import(gkc_ctx* ctx, const void* d_records, const uint64_t* rec_offsets /* [nb_partitions+1] */,
                       const uint64_t* kmers_per_partition /* [nb_partitions] */);
int gkc_segments_clear(gkc_ctx* ctx);

/* ---------------------------------------------------------------------------------------------------------------
 * Multi-GPU: one process = one context = one GPU; partitions are OWNED by ranks (contiguous ranges), every rank scans
 * its own reads, and one exchange routes each rank's super-k-mer records to the owner of their partition — the device analogue of the
 * reference's disk shuffle (SuperKmerBinFiles, tools/storage/impl/Storage.cpp:360-430; fillPartitions writes, fillSolidKmers reads:
 * SortingCountAlgorithm.cpp:1211-1344, 1384-1602). Same canonical k-mer => same minimizer => same partition, so after the exchange every
 * rank counts the partitions it owns with no further communication.
 *
 * A communicator is either RCCL (grouped ncclSend / ncclRecv over xGMI, librccl linked directly, asynchronous on its own HIP stream so
 * that the exchange of push i overlaps Stage A of push i+1) or a caller-supplied transport (two callbacks; used where RCCL cannot run,
 * e.g. two ranks sharing one GPU in the tests: gloo with host staging, gatb-core_amd/dist.py).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct gkc_comm gkc_comm;
#define GKC_COMM_ID_BYTES 128                      /* sizeof(ncclUniqueId) */
typedef struct gkc_xfer { int32_t peer; int32_t reserved; void* d_ptr; uint64_t n_bytes; } gkc_xfer;   /* d_ptr: DEVICE memory */
typedef struct gkc_transport {
    void* user;
    /* every rank contributes n_bytes of HOST memory; all[r * n_bytes ...] = rank r's contribution. Blocking. */
    int (*allgather_host)(void* user, const void* mine, uint64_t n_bytes, void* all);
    /* one grouped point-to-point exchange (ncclGroupStart ... ncclGroupEnd semantics): every send and receive of the call is posted
     * before any is waited for; messages between one pair of ranks match in list order; returns when all have completed. */
    int (*sendrecv_device)(void* user, const gkc_xfer* sends, uint32_t n_sends, const gkc_xfer* recvs, uint32_t n_recvs);
} gkc_transport;
/* rank 0 makes the id (ncclGetUniqueId) and the launcher hands it to every rank (torch.distributed store, MPI, a file) */
int  gkc_comm_unique_id(uint8_t id[GKC_COMM_ID_BYTES]);
int  gkc_comm_create_rccl(gkc_ctx* ctx, const uint8_t id[GKC_COMM_ID_BYTES], int world, int rank, gkc_comm** out);
int  gkc_comm_create_transport(gkc_ctx* ctx, const gkc_transport* t, int world, int rank, gkc_comm** out);
/* A transport that needs nothing but a directory all ranks can see (a mailbox of files: host all-gather = one file per rank, device send/recv = staged
 * through host memory, one file per message). For ranks RCCL cannot connect — two processes sharing one GPU in the tests (RCCL refuses a duplicate device),
 * hosts without xGMI — and for launchers that have nothing but a shared file system. Development / test transport: bandwidth is that of the file system. */
int  gkc_comm_create_files(gkc_ctx* ctx, const char* directory, int world, int rank, gkc_comm** out);
/* A transport communicator (gkc_comm_create_transport / _files) whose DEVICE messages stay on the devices: every receive buffer is published as an IPC memory handle
 * through the transport's host all-gather and the sender copies device to device (xGMI peer copy between the GPUs of a node). What a launcher falls back to when RCCL
 * refuses the communicator: the host side of the transport is then only used for a few hundred bytes per exchange. Call before the first push on every rank. */
int  gkc_comm_enable_ipc(gkc_comm* comm, int on);
void gkc_comm_destroy(gkc_comm* comm);
/* Owner ranges: rank r owns partitions [first[r], first[r+1]); first[0] = 0, first[world] = nb_partitions. By default the first
 * exchange of a pass balances them by the k-mers per partition all ranks report ("balanced by weight"); gkc_comm_set_owners
 * pins them (e.g. from the Repartitor's sample, PartiInfo.cpp:48-106), NULL goes back to balancing. gkc_balanced_owner_ranges is the
 * pure host function behind it (no context, no GPU). */
int  gkc_comm_set_owners(gkc_comm* comm, const uint32_t* first /* [world+1] or NULL */);
int  gkc_comm_get_owners(gkc_comm* comm, uint32_t* first /* [world+1] */);
int  gkc_balanced_owner_ranges(const uint64_t* weights, uint32_t nb_partitions, int world, uint32_t* first /* [world+1] */);
/* Routes the records of every push since the last gkc_exchange of this pass to their owners and imports what arrives; the rank's own
 * segments keep only the partitions it owns. Collective: every rank calls it the same number of times per pass (a rank without new
 * pushes takes part with nothing to send — pushes per rank may differ). With RCCL the transfers run on the communicator's stream and
 * gkc_finish_pass waits for them. */
int  gkc_exchange(gkc_ctx* ctx, gkc_comm* comm);
/* The message plan of one exchange for one rank — the pure host function gkc_exchange runs after the all-gather of the count tables (no
 * context, no GPU: the CPU tests drive it with gloo). counts: [world][l_max][2][P] = records, k-mers per partition of segment j of rank r
 * (zero rows beyond n_segs[r]); first: owner ranges. sends[i]: n_recs records starting at record rec_begin of this rank's own segment
 * `seg` go to `peer`; recvs[i]: n_recs records of segment `seg` of `peer` arrive at record rec_begin of the receive arena. Messages between
 * two ranks are listed in the same order on both sides. Capacity of sends / recvs: world * l_max entries each. */
typedef struct gkc_plan_msg { int32_t peer; uint32_t seg; uint64_t rec_begin; uint64_t n_recs; } gkc_plan_msg;
int  gkc_exchange_plan(int world, int rank, uint32_t nb_partitions, const uint32_t* first, const uint64_t* n_segs, uint64_t l_max, const uint64_t* counts,
                       gkc_plan_msg* sends, uint32_t* n_sends, gkc_plan_msg* recvs, uint32_t* n_recvs, uint64_t* recv_total_recs);
typedef struct gkc_comm_stats {
    uint64_t n_exchanges, bytes_sent, bytes_received;   /* record bytes that left / reached this rank (not counting what stayed) */
    double   ms_transfer;                                 /* HIP-event time of the grouped send/recv on the communicator's stream (RCCL) or wall time of the callback */
    double   ms_host;                                     /* wall time inside gkc_exchange (tables, allocation, enqueue) */
    uint64_t reserved[4];                                 /* [0]: receive buffers the IPC transport took through a bounce block (their allocation could not be exported) */
} gkc_comm_stats;
int  gkc_comm_get_stats(gkc_comm* comm, gkc_comm_stats* out);
/* Collective, after gkc_finish_pass of the current pass on every rank: the Count[] arrays of all partitions are gathered on `root` (each owner sends the arrays of
 * its partitions, whole Stage-B batches at a time), and so are the abundance histogram and the pass statistics (summed). Afterwards gkc_wait_partition /
 * gkc_partition_counts* / gkc_histogram / gkc_get_stats on `root` serve EVERY partition of the pass — what a single process would hold — so that one process
 * writes the one result file the reference's consumers open (CountProcessorDump.hpp:85-95: all nb_partitions x nb_passes datasets live in one file;
 * GraphUnitigs.cpp:921-931 opens that file). The other ranks keep what they had. The results must fit root's HBM (solid k-mers only travel). */
int  gkc_gather_results(gkc_ctx* ctx, gkc_comm* comm, int root);
/* Diagnostic: this rank sends n_bytes of a pattern to ITSELF through the communicator's own grouped send / receive path (the message is cut into the same
 * 256 MiB chunks as the messages of gkc_exchange) and compares what arrived. With one rank this is the only way to run ncclSend / ncclRecv and the chunking on
 * hardware. mismatches: 8-byte words that differ; ms: wall time of the transfer. */
int  gkc_comm_loopback(gkc_ctx* ctx, gkc_comm* comm, uint64_t n_bytes, uint64_t* mismatches, double* ms);
/* Start-up self-test over the real peers, collective: in ONE grouped exchange every rank sends n_bytes of a pattern keyed by (source, destination) to every other
 * rank and checks what arrives from each — the send / receive path of gkc_exchange (RCCL: grouped ncclSend / ncclRecv over xGMI, cut into the same 256 MiB chunks)
 * between every pair of GPUs before any record travels. A rank that receives anything but the pattern makes the call fail on EVERY rank (gkc_comm_agree).
 * mismatches: 8-byte words that differ on this rank; ms: wall time of the exchange on this rank. One rank: the loopback above. */
int  gkc_comm_selftest(gkc_ctx* ctx, gkc_comm* comm, uint64_t n_bytes, uint64_t* mismatches, double* ms);
/* What went where: bytes this rank has sent to / received from every peer through the communicator's grouped send / receive path since it was created ([world] each,
 * either may be NULL), and the wall time ncclCommInitRank took when the communicator was made (0 for the other transports). */
int  gkc_comm_peer_bytes(gkc_comm* comm, uint64_t* sent /* [world] */, uint64_t* received /* [world] */, double* init_ms);

/* ---------------------------------------------------------------------------------------------------------------
 * Bloom filter of solid k-mers — replaces BloomBuilder::build / IBloom::insert (kmer/impl/BloomBuilder.hpp:102-128,
 * 174-182) and the query side IBloom::contains / contains8 (tools/collections/impl/Bloom.hpp:211-234, 437-490,
 * 555-828). kind: 0 "basic" (BloomSynchronized), 1 "cache" (BloomCacheCoherent), 2 "neighbor" (BloomNeighborCoherent) —
 * the three kinds BloomFactory::createBloom can return for a k-mer item (Bloom.hpp:1254-1266).
 * The bit array is byte-identical to the reference's getArray() for the same inserted set.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct gkc_bloom gkc_bloom;
int      gkc_bloom_create(gkc_ctx* ctx, int kind, uint64_t tai_bits, uint32_t nb_hash, uint32_t k, gkc_bloom** out);
void     gkc_bloom_destroy(gkc_bloom* b);
uint64_t gkc_bloom_nbytes(const gkc_bloom* b);     /* IBloom::getSize()    */
uint64_t gkc_bloom_bitsize(const gkc_bloom* b);    /* IBloom::getBitSize() */
/* keys: n items, `stride` bytes apart, each starting with the k-mer value (8 B for k<=31, 16 B for k<=63): pass Count
 * arrays with stride 16/32 or raw key arrays with stride 8/16. *_device variants take HBM-resident keys. */
int gkc_bloom_insert(gkc_bloom* b, const void* keys, uint64_t n, uint32_t stride);
int gkc_bloom_insert_device(gkc_bloom* b, const void* d_keys, uint64_t n, uint32_t stride);
/* inserts every solid k-mer of every finished dataset of the context (what BloomAlgorithm::execute does, BloomAlgorithm.cpp:155-199) */
int gkc_bloom_insert_solid(gkc_bloom* b, gkc_ctx* ctx);
int gkc_bloom_contains(gkc_bloom* b, const void* keys, uint64_t n, uint32_t stride, uint8_t* out);
int gkc_bloom_contains8(gkc_bloom* b, const void* keys, uint64_t n, uint32_t stride, uint8_t* out);  /* neighbor kind */
/* The query side at the reference's call site (DebloomMinimizerAlgorithm.cpp:201: contains8 of every solid k-mer; Bloom.hpp:645-811), on the device: every solid
 * k-mer of every finished dataset of the context is queried where it lies (HBM), in dataset order. neighbors8 != 0: contains8 (neighbor kind), one result byte per
 * k-mer (bit j: neighbour j is in the filter); else contains, 0/1 per k-mer. d_out: device buffer of *n_queried bytes or NULL (results discarded).
 * n_positive: number of set result bits. */
int gkc_bloom_query_solid(gkc_bloom* b, gkc_ctx* ctx, int neighbors8, uint8_t* d_out, uint64_t* n_queried, uint64_t* n_positive);
int gkc_bloom_get_array(gkc_bloom* b, uint8_t* out, uint64_t cap_bytes);                               /* IBloom::getArray() */
int gkc_bloom_set_array(gkc_bloom* b, const uint8_t* in, uint64_t n_bytes);                            /* StorageTools::loadBloom */
/* the bit array where it lives (device memory, n_bytes = gkc_bloom_nbytes rounded up to 4): multi-GPU runs insert their own
 * partitions' solid k-mers and OR-reduce the arrays in place (all-reduce with bitwise OR over RCCL) */
int gkc_bloom_device_array(gkc_bloom* b, void** d_bits, uint64_t* n_bytes);
/* in-place bitwise-OR all-reduce of the bit array over the communicator: reduce-scatter (every rank ORs one slice of everybody's array)
 * + all-gather, 2 (world-1)/world of the array per rank instead of (world-1) arrays */
int gkc_bloom_allreduce_or(gkc_bloom* b, gkc_comm* comm);

/* ---------------------------------------------------------------------------------------------------------------
 * Synthetic reads generated in HBM (bench / parity at full size; SURVEY §8d generator): genome of genome_len uniform
 * bases from a counter-based hash of (seed, position); read i (global index first_read+i, so ranks can draw disjoint
 * slices of one read stream over the same genome) starts at hash(seed,index) % (genome_len-read_len+1), is
 * reverse-complemented with probability 1/2 and each base is substituted with probability sub_rate_ppm/1e6.
 * Bit-identical to gatb-core_amd/gkc.py:synth_reads_np (numpy). Outputs are device pointers owned by the caller of
 * gkc_device_free.
 * ------------------------------------------------------------------------------------------------------------- */
int gkc_synth_reads_device(gkc_ctx* ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                           uint64_t genome_len, uint32_t sub_rate_ppm, char** d_bases, uint64_t** d_offsets);
/* The same generator over a REPEAT-RICH genome with low-complexity reads (full-size parity and bench of the paths the reference answers skew with:
 * PartitionsCommand.cpp:505-545, TempCountFileMerger :217-360). GKC_SYNTH_SKEWED: the genome is cut into slots of 8192 bases; a quarter of them start with a copy
 * of one of 50 family sequences of 1000..5000 bases (about genome_len / 1.6e6 copies per family, ~9 % of the bases; every copy 0.5 % diverged), the rest is
 * uniform; 1 % of the reads are a unit of 1..3 bases repeated (poly-A, (AC)n, (ACG)n ...) before the substitutions. Twin: gkc.py synth_reads_np(profile=1). */
#define GKC_SYNTH_UNIFORM 0u
#define GKC_SYNTH_SKEWED  1u
int gkc_synth_reads_profile_device(gkc_ctx* ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                                   uint64_t genome_len, uint32_t sub_rate_ppm, uint32_t profile, char** d_bases, uint64_t** d_offsets);
/* ---- MPHF + abundance map ------------------------------------------------------------------------------
 * Replaces MPHFAlgorithm::execute / populate (kmer/impl/MPHFAlgorithm.cpp:150-275) and the BooPHF build behind it
 * (thirdparty/BooPHF/BooPHF.h:734-1108 as instantiated by tools/collections/impl/BooPHF.hpp:236-300: jenkins64 hasher seeded by
 * std::mt19937_64(37), gamma 3, 25 levels). The level bit arrays and rank samples are the ones BooPHF builds for the same keys, so
 * gkc_mphf_save writes the byte stream of boomphf::mphf::save (what MPHF<>::save puts into the "dsk/mphf" collection, loadable by
 * BooPHF::load) and gkc_mphf_lookup returns BooPHF::lookup's codes. Keys: `stride` bytes per item, the k-mer in the first 8 (k <= 31)
 * or 16 (k <= 63) bytes — a Count array works as it is. */
typedef struct gkc_mphf gkc_mphf;
int      gkc_mphf_build(gkc_ctx* ctx, const void* keys /* host */, uint64_t n, uint32_t stride, uint32_t k, gkc_mphf** out);
int      gkc_mphf_build_solid(gkc_ctx* ctx, gkc_mphf** out);          /* keys = the solid k-mers of every finished dataset (getSolidKmers() order) */
/* Multi-GPU build over the solid k-mers of ALL ranks (each rank holds the partitions it owns): BooPHF's level arrays do not depend on the
 * order keys are processed in, so every level is built from per-rank partial arrays combined with seen = OR, collided = OR | (seen by two
 * ranks) — reduce-scatter + all-gather like the Bloom. Every rank ends up with the complete function: gkc_mphf_save / lookup give the
 * bytes / codes of a single-GPU build over the same key set (rank order = partition order = getSolidKmers() order). Collective. */
int      gkc_mphf_build_solid_dist(gkc_ctx* ctx, gkc_comm* comm, gkc_mphf** out);
/* populate() across ranks: every rank fills the cells of its own solid k-mers, the maps are OR-combined; out (host, gkc_mphf_size bytes) is
 * complete on every rank */
int      gkc_mphf_abundance_map_dist(gkc_mphf* m, gkc_ctx* ctx, gkc_comm* comm, uint8_t* out, uint64_t cap, uint64_t* nb_above_precision);
void     gkc_mphf_destroy(gkc_mphf* m);
uint64_t gkc_mphf_size(const gkc_mphf* m);                             /* number of keys (BooPHF::size) */
int      gkc_mphf_lookup(gkc_mphf* m, const void* keys /* host */, uint64_t n, uint32_t stride, uint64_t* codes);   /* ~0: not a key (final level miss) */
uint64_t gkc_mphf_save_size(const gkc_mphf* m);
int      gkc_mphf_save(gkc_mphf* m, uint8_t* out, uint64_t cap);
/* MPHFAlgorithm::populate: out[code(kmer)] = index of the k-mer's abundance in MapMPHF's discretization table (MapMPHF.hpp:96-145),
 * for every solid k-mer of the context; *nb_above_precision = abundances beyond the table (MPHFAlgorithm.cpp:254-258) */
int      gkc_mphf_abundance_map(gkc_mphf* m, gkc_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* nb_above_precision);

/* ---- multi-bank counting: one abundance per bank and k-mer, solidity kinds ------------------------------------------------------
 * Given an album of N banks the reference hands every count processor a CountVector with one abundance per bank, decides solidity with
 * -solidity-kind sum|min|max|one|all|custom (kmer/impl/CountProcessorSolidity.hpp:176-304), dumps Count{kmer, sum}
 * (CountProcessorDump.hpp:148-152) and histograms the sum (CountProcessorHistogram.hpp:173-184); known answers: test/unit/src/kmer/TestDSK.cpp:482-612.
 * Here the banks are counted one after another by an ordinary context (window [1, INT32_MAX]: every distinct k-mer of the bank comes out) and a
 * gkc_banks object merges their sorted Count[] arrays on the device: per dataset (part + pass * nb_partitions) the ascending distinct k-mers of all
 * banks and nb_banks planes of int32 counts (0 where a bank does not have the k-mer). The object is built from a configured context, remembers its
 * model (k, m, partitions, passes, minimizer order, repartition table) and keeps the context's allocator alive: it may outlive gkc_destroy of the
 * context. Messages of every gkc_banks_* failure are read with gkc_last_error(the context the object was created from).
 *   gkc_banks_add      : every finished dataset of `ctx` that the object has not merged yet becomes bank `bank`'s column (a multi-pass count may add
 *                        after every pass or once after all of them: a pass's results are told apart from a recount by gkc_begin_pass). On return the
 *                        context's results are no longer needed — gkc_begin_pass(ctx, 0) may start the next bank; the merged state owns its copies.
 *                        Banks may be added in any order; a bank never added is a column of zeros. GKC_ERR_ARG when: the context's model differs from
 *                        the object's; its solidity window is not the default [1, INT32_MAX] (per-bank counts must be complete); bank >= nb_banks; a
 *                        (bank, dataset) pair is added twice (the same results again, or a recount into a bank that holds the dataset); a pass is open
 *                        or was released (gkc_release_pass). Allowed after gkc_banks_evaluate: the evaluation is gone then.
 *   gkc_banks_evaluate : one pass over the merged state: sum, min and max of every k-mer's counts, solid or not by `kind` with the closed ranges
 *                        [amin[i], amax[i]] of bank i — sum / min / max look at range 0 only (_thresholds[0]); one: some bank's count in its range; all:
 *                        every bank's; custom: bank i's count is in its range exactly when solid_vec[i] != 0 (CountProcessorSolidity.hpp:291-300) — and
 *                        histogram[min(sum, histo_max)]++ over ALL distinct k-mers. May be repeated with other kinds and ranges without merging again.
 *   reading (GKC_ERR_ARG before an evaluation): the solid k-mers of a dataset as Count{value, sum} records in the layout of gkc_partition_counts
 *                        (16 / 32 bytes, ascending, pad bytes zero) and their count vectors int32[n_solid][nb_banks], on the host or where they lie.
 * Counts and sums are int32 like CountNumber; a sum beyond INT32_MAX is outside the contract (it wraps). */
#define GKC_SOLIDITY_SUM    0
#define GKC_SOLIDITY_MIN    1
#define GKC_SOLIDITY_MAX    2
#define GKC_SOLIDITY_ONE    3
#define GKC_SOLIDITY_ALL    4
#define GKC_SOLIDITY_CUSTOM 5
typedef struct gkc_banks gkc_banks;
int  gkc_banks_create(gkc_ctx* ctx, uint32_t nb_banks /* 1..64 */, gkc_banks** out);
void gkc_banks_destroy(gkc_banks* b);
int  gkc_banks_add(gkc_banks* b, gkc_ctx* ctx, uint32_t bank);
int  gkc_banks_evaluate(gkc_banks* b, int kind, const int32_t* amin /* [nb_banks] */, const int32_t* amax /* [nb_banks] */,
                        const uint8_t* solid_vec /* [nb_banks], GKC_SOLIDITY_CUSTOM only, else NULL */, uint32_t histo_max);
int  gkc_banks_partition_info(gkc_banks* b, uint32_t dataset, uint64_t* n_solid, uint64_t* n_distinct);
int  gkc_banks_partition_counts(gkc_banks* b, uint32_t dataset, void* out_counts, uint64_t cap_records, uint64_t* n_solid);
int  gkc_banks_partition_vectors(gkc_banks* b, uint32_t dataset, int32_t* out /* [n_solid][nb_banks] */, uint64_t cap_records, uint64_t* n_solid);
/* device pointers into the evaluation's buffers: valid until the next gkc_banks_evaluate / gkc_banks_add / gkc_banks_destroy */
int  gkc_banks_partition_counts_device(gkc_banks* b, uint32_t dataset, const void** d_counts, const int32_t** d_vectors, uint64_t* n_solid);
int  gkc_banks_histogram(gkc_banks* b, uint64_t* out, uint32_t n_bins /* >= histo_max + 1 */);

/* ---- abundance queries: the k-mers of reads, or bare k-mer values, looked up in the counted results on the device -----------------------------
 * The reference answers "how often was this k-mer seen" through the MPHF + abundance map (discretised, keys of the set only) or by opening the result file; here the
 * finished datasets are searched where they lie. A k-mer's dataset follows from its minimizer (repart[minimizer], minimizer % nb_passes), each dataset is an ascending
 * Count[]; a sampled index (the key of every GKC_QUERY_INDEX_STRIDE-th record, default 256) is built by the first query, owned by the context and dropped when its
 * results change: a query always answers from the results the context holds NOW (after a recount — gkc_begin_pass(0) ... gkc_finish_pass — the new counts).
 * State (GKC_ERR_ARG otherwise, gkc_last_error names the reason): the context is configured, no pass is open, EVERY dataset of every pass is finished, no pass was
 * released (gkc_release_pass), no gkc_finish_pass_async is in flight. Offsets are checked like gkc_push_reads_device checks them; bad offsets touch no memory outside
 * the buffers. Queries across the ranks of a communicator are not provided: every rank answers from the datasets it holds, and on the root after gkc_gather_results
 * the calls serve every partition like any other call.
 * out[g], g = index of the k-mer's FIRST base in the flat buffer (n_bases entries, 4 bytes per base; device arrays 16-byte aligned like d_bases):
 *   > 0  the Count abundance of the canonical k-mer (it is in the results, i.e. inside the solidity window of the count)
 *     0  a valid k-mer that is not in the results
 *    -1  no k-mer starts here: fewer than k bases left in the read, or the window holds a character outside ACGTacgt
 * Timing names of gkc_get_timing: "query_index", "query_reads", "query_kmers". */
int gkc_query_reads_device(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, int32_t* d_out);
int gkc_query_reads(gkc_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int32_t* out);   /* host in, host out */
/* keys: n items `stride` bytes apart, the k-mer value in the first 8 (k <= 31) / 16 (k <= 63) bytes, like gkc_bloom_insert (a Count array works as it is).
 * The library takes min(key, revcomp(key)). out[i] = abundance or 0. A value >= 4^k: GKC_ERR_ARG. */
int gkc_query_kmers_device(gkc_ctx* ctx, const void* d_keys, uint64_t n, uint32_t stride, int32_t* d_out);
int gkc_query_kmers(gkc_ctx* ctx, const void* keys, uint64_t n, uint32_t stride, int32_t* out);
/* per read, from an abundance array as written above and the offsets it was made with: over the read's valid k-mers (0 counts as a value) */
typedef struct gkc_read_abundance { uint32_t n_valid, n_found; int32_t min, max; uint64_t sum; } gkc_read_abundance;   /* all 0 when n_valid == 0 */
int gkc_query_read_summary_device(gkc_ctx* ctx, const int32_t* d_abund, const uint64_t* d_offsets, uint64_t n_reads, gkc_read_abundance* d_out);
/* the same against a merged multi-bank state (needs no gkc_banks_evaluate, stays valid across evaluations; gkc_banks_add drops the object's index):
 * d_sum[g] as above with the sum over banks; d_vectors (may be NULL): int32[n_bases][nb_banks], row of zeros where d_sum[g] <= 0.
 * Errors are read with gkc_last_error(the context the object was created from). (Named gkc_query_*: the gkc_banks_* exports are a closed list, tests/test_banks_cpu.py.) */
int gkc_query_banks_reads_device(gkc_banks* b, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, int32_t* d_sum, int32_t* d_vectors);

/* ---- graph neighbourhoods: which of the eight de Bruijn neighbours of every solid k-mer are solid too, exactly -----------------------------------
 * What the reference gets from BloomAlgorithm + DebloomMinimizerAlgorithm (contains8 of every solid k-mer, then the false positives filtered out) and what
 * BranchingAlgorithm reads through graph.successors / predecessors: here each neighbour is looked up in the counted results themselves (the search of the
 * abundance queries above, eight lookups per record), so the answer has no false positives and needs neither filter nor debloom.
 * One mask byte per solid record, bit order of gkc_bloom_contains8: bits 0-3 the right extensions ((x << 2) | j) & mask, bits 4-7 the left extensions
 * (x >> 2) | (j << 2(k-1)), j = A, C, T, G = 0..3, x = the record's (canonical) value taken as the forward strand, like the reference's node iterator.
 * A bit is set if and only if min(neighbour, revcomp(neighbour)) is a record of the results the context holds NOW (inside the solidity window of the count). Self-loops
 * and, at even k, palindromes get no special case: the sentence above is the whole definition. Parity with the reference's graph is claimed for odd k.
 * in = popcount(mask >> 4), out = popcount(mask & 15); a node is BRANCHING unless in == 1 and out == 1 (BranchingAlgorithm.cpp: what /branching/nodes holds).
 * State rules, index life cycle and error reporting are those of the abundance queries. No solid k-mer at all is not an error: GKC_OK, counts 0.
 * Every rank of a communicator answers from the datasets it holds; the merged state of a gkc_banks is not served.
 * Timing names of gkc_get_timing: "graph_neighbors", "graph_branching" (the index: "query_index"). */
/* masks of every solid k-mer of every finished dataset, dataset order (the order of gkc_bloom_query_solid / getSolidKmers());
 * d_masks: device buffer of >= kmers_nb_solid bytes, or NULL (only *n_solid is reported) */
int gkc_graph_neighbors_solid(gkc_ctx* ctx, uint8_t* d_masks, uint64_t* n_solid);
/* the same for ONE dataset (a consumer walking the partitions): n = its n_solid */
int gkc_graph_neighbors_partition(gkc_ctx* ctx, uint32_t pass, uint32_t part, uint8_t* d_masks, uint64_t* n_solid);
/* d_masks: what gkc_graph_neighbors_solid wrote, or NULL (computed inside). d_records: device, cap_records Count records in the layout of gkc_partition_counts
 * (value, the k-mer's abundance, pad bytes zero), or NULL: the branching nodes in dataset order, ascending inside a dataset.
 * *n_branching is always reported; cap too small: GKC_ERR_CAPACITY, nothing written beyond cap. topology: host u64[25] or NULL, topology[in * 5 + out] = solid k-mers
 * with that many solid predecessors / successors. */
int gkc_graph_branching_solid(gkc_ctx* ctx, const uint8_t* d_masks, void* d_records, uint64_t cap_records, uint64_t* n_branching, uint64_t* topology);

/* ---- unitigs: the maximal non-branching paths of the solid k-mers glued into sequences, on the device ---------------------------------------------
 * What the reference's GraphUnitigs (bcalm2) computes on the host from the result file, from the exact neighbour masks above. The records are the solid k-mers of all
 * finished datasets, flat index i in dataset order (the order of gkc_graph_neighbors_solid), x_i the canonical value taken as the forward strand. A record has two ends:
 * end 0, the right one (mask bits 0-3), and end 1, the left one (bits 4-7); deg(i, s) = popcount of that nibble.
 *   arrival: y = a neighbour of x_i, c = min(y, revcomp(y)) = record j. Leaving i by its right end one arrives at end 1 of j if c == y, else at end 0; leaving by
 *            the left end at end 0 if c == y, else at end 1.
 *   link   : (i, s) and (j, a) are linked if and only if deg(i, s) == 1, deg(j, a) == 1, j != i, and neither x_i nor y equals its own reverse complement
 *            (palindromes, even k only: a palindrome is a unitig of its own and nothing links to it). The relation is symmetric.
 *   unitig : a connected component of the links: a path, or an isolated cycle. A path starts at whichever of its two end records has the smaller flat index and leaves
 *            it through its linked end; a single record stands forward. A cycle is cut at the left end of its smallest record and starts there, forward. Unitigs are
 *            numbered by ascending start record. A unitig of L records has L + k - 1 bases: record p of the path stands forward or reverse-complemented as it is
 *            traversed, consecutive records overlap by k - 1 bases. KC = the sum of the records' abundances (no parity with the header fields of bcalm2 is claimed).
 * Parity with the reference's unitigs (as a set of canonical sequences) is claimed for odd k, like for the masks.
 * State rules, index life cycle and error reporting are those of the abundance queries. No solid k-mer at all is not an error: GKC_OK, zeros. The ids of the ranking
 * are 32-bit: a context with 2^31 or more solid k-mers returns GKC_ERR_CAPACITY. Every rank of a communicator answers from the datasets it holds; the merged state
 * of a gkc_banks is not served.
 * Timing names of gkc_get_timing: "graph_links", "graph_rank" (its launch count: the rounds of pointer jumping), "graph_emit", "graph_unitig_links".
 *
 * Links between unitigs (the edges of the compacted graph, bcalm2's L: fields). A unitig u of L records has two SIDES: side 0 ('+') is the outward end of the record at
 * pos = L - 1 (its right end if the record stands forward, its left end if reversed), side 1 ('-') the outward end of the record at pos = 0 (its left end if forward, its
 * right end if reversed). A single-record unitig stands forward: side 0 is its right end, side 1 its left end. Slot t = 2 u + side.
 *   link   : for each bit set in the mask nibble of the outward end s of the side's record i: y = that neighbour, c = min(y, revcomp(y)) = record j, a = the arrival end
 *            (a = 1 - s if y < revcomp(y), else a = s: the rule of the links above), (v, rev_j) = the placement of j. One arrives at the BEGIN of v if
 *            a == (rev_j ? 0 : 1): entry v << 1 | 0, "L:+-:v:+"; else at its end: entry v << 1 | 1, "L:+-:v:-". The entries of a slot are in ascending order of that
 *            64-bit value. No special case for j == i, v == u or palindromes: self-links are links (a cut cycle has L:+:u:+ and L:-:u:-, a hairpin end L:+:u:-, a
 *            self-loop record such as poly-A links to itself on both sides).
 * A neighbour reached through a side lies at pos 0 (arriving at a begin) or pos L_v - 1 (arriving at an end) of its unitig. At odd k the entries of a slot are distinct,
 * the relation is symmetric (slot 2u + su holds (v, mv) <=> slot 2v + (1 - mv) holds (u, 1 - su)) and equals the rule of the reference's LinkTigs.cpp: all (k-1)-overlaps
 * between unitig extremities. Parity with the reference is claimed for odd k only; at even k the sentences above are the whole definition. */
/* builds the placement of every solid record and keeps it in the context (dropped when the results change, like the query index).
 * d_masks: what gkc_graph_neighbors_solid wrote, or NULL (computed inside). */
int gkc_graph_unitigs_build(gkc_ctx* ctx, const uint8_t* d_masks, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles);
/* d_bases: ASCII ACGT, cap_bases >= n_bases. d_offsets: u64[n_unitigs + 1] (room for cap_unitigs + 1) — exactly the arguments of gkc_push_reads_device /
 * gkc_query_reads_device. d_kc: u64[n_unitigs] or NULL. Too small: GKC_ERR_CAPACITY, nothing written. GKC_ERR_ARG before a build or after the results changed. */
int gkc_graph_unitigs_write(gkc_ctx* ctx, char* d_bases, uint64_t cap_bases, uint64_t* d_offsets, uint64_t cap_unitigs, uint64_t* d_kc);
/* per solid record, flat order; either may be NULL. d_unitig: u64 = unitig index << 1 | reversed. d_pos: u32 = position in the path. */
int gkc_graph_unitigs_nodes(gkc_ctx* ctx, uint64_t* d_unitig, uint32_t* d_pos);
/* CSR over the 2 n_unitigs sides. d_link_offsets: u64[2 n_unitigs + 1] (room for 2 cap_unitigs + 1), d_links: u64[n_links] (room for cap_links);
 * both NULL: only *n_links is reported (kept with the placement once counted: the sizing call is free after that). d_masks: what gkc_graph_neighbors_solid
 * wrote for THESE results, or NULL (computed inside, on every call that computes). Masks that name a neighbour which is no record of these results: GKC_ERR_ARG
 * after the search, the buffers then hold no links (masks of other results that happen to name only records cannot be told apart and give their own answer).
 * Too small: GKC_ERR_CAPACITY, *n_links reported, nothing written. GKC_ERR_ARG before a build or after the results changed.
 * No solid k-mer: GKC_OK, offsets[0] = 0, *n_links = 0. */
int gkc_graph_unitigs_links(gkc_ctx* ctx, const uint8_t* d_masks, uint64_t* d_link_offsets, uint64_t cap_unitigs,
                            uint64_t* d_links, uint64_t cap_links, uint64_t* n_links);

/* ---- tips: dead-end branches of the compacted graph removed round by round, on the device ----------------------------------------------------------
 * The first step of the reference's Simplifications::simplify() (removeTips), on the unitigs and links above. All terms are those of the unitigs and their links.
 *   alive  : one byte per solid record, flat order; every record starts alive. A dead record is a record of no unitig: its mask is 0 and no alive record's mask names
 *            it. The unitigs of an alive set are the unitigs above over the alive records only, numbered by ascending start record among them.
 *   round  : starts from the masks and alive as they are; takes the unitigs and links of the alive subgraph. Unitig u has L_u records, bases(u) = L_u + k - 1, abundance
 *            sum KC_u. u is a CANDIDATE when exactly one of its two slots has no link and the other, t = 2u + su, has at least one (a slot that links to u's own other
 *            slot counts as linked; no special case for hairpins, self-links or palindromes; an isolated unitig or an isolated cycle never is a candidate).
 *   tip    : a candidate with bases(u) <= max_len_topo (the topological rule), or with bases(u) <= max_len_rc and some competitor c such that
 *            KC_c * L_u * rc_den > rc_num * KC_u * L_c (strict, in exact integers, no floating point). The competitors of u, per entry (v, m) of slot t: the unitig v
 *            itself and every entry (w, .) of v's arrival slot 2v + (1 - m) except the ONE entry (u, 1 - su) that is u coming back.
 *            All tips of a round are decided on the graph at its start and removed together: every record of a tip dies and its mask becomes 0, and every bit of an alive
 *            record's mask that named a dead record is cleared. The next round compacts again: two unitigs a tip kept apart become one.
 * Rounds run until one removes nothing or max_rounds have run.
 * Against the reference: the topological rule is its removeTips pass on a freshly compacted graph, for odd k (k + simplePathLength from a dead-end extremity is the
 * unitig's length in bases, the deletions are deferred to the end of the pass, later passes walk simple paths across joined unitigs). The coverage rule is NOT the
 * reference's (which averages floating-point means of means of the neighbours): it is "some competitor is that much better covered" in integers, and no parity is
 * claimed for it. The stop rule is this library's (the reference's depends on its cutoff events, 20 passes at most). Bulges and erroneous connections are served by
 * gkc_graph_simplify (section "simplify" below); the removal of isolated short unitigs is not served.
 * Timing name of gkc_get_timing: "graph_tips" (flags, kill, refresh of every round; its launch count: the rounds). The builds and links inside the rounds go to the
 * names of the unitigs. */
typedef struct gkc_tip_params {
    uint32_t max_len_topo, max_len_rc;     /* lengths in bases; 0 switches the rule off */
    uint32_t rc_num, rc_den;               /* the ratio of the coverage rule; rc_den == 0: GKC_ERR_ARG */
    uint32_t max_rounds;                   /* 0 does nothing (the placement is the plain build's); more than 64: GKC_ERR_ARG */
} gkc_tip_params;
/* gkc_graph_unitigs_build over the alive records only. d_alive: u8[n_solid]. d_masks: required, and already consistent with d_alive (a dead record has mask 0 and
 * nothing names it). Afterwards gkc_graph_unitigs_nodes reports ~0 / pos 0 for dead records, gkc_graph_unitigs_write emits only alive records
 * (n_bases = n_alive + n_unitigs (k - 1)), gkc_graph_unitigs_links with the same masks gives the links of the subgraph, and with d_masks == NULL GKC_ERR_ARG (the
 * library cannot recompute edited masks). All records dead, or no records: GKC_OK, 0 unitigs, gkc_graph_unitigs_write gives offsets[0] = 0. */
int gkc_graph_unitigs_build_alive(gkc_ctx* ctx, const uint8_t* d_masks, const uint8_t* d_alive, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles);
/* d_masks (in, out): on entry what gkc_graph_neighbors_solid wrote for these results; NULL is GKC_ERR_ARG (the edited masks are part of the result). d_alive (out):
 * n_solid bytes. On return they describe the final subgraph and the placement in the context is that of gkc_graph_unitigs_build_alive on them (of the plain build when
 * nothing was removed). *n_rounds: the rounds run, the last, empty one included. tips_per_round: host u64[max_rounds] or NULL. State rules, error behaviour and the
 * invalidation by a recount are those of gkc_graph_unitigs_build; masks that name a neighbour which is no record: GKC_ERR_ARG, d_masks / d_alive then hold no result. */
int gkc_graph_tips_remove(gkc_ctx* ctx, uint8_t* d_masks, uint8_t* d_alive, const gkc_tip_params* params, uint64_t* n_rounds, uint64_t* tips_per_round,
                          uint64_t* n_records_removed, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles);

/* ---- simplify: tips, bulges and erroneous connections of the compacted graph, on the device ---------------------------------------------------------
 * The three steps of the reference's Simplifications::simplify() (removeTips, removeBulges, removeErroneousConnections) in its order. All terms are those of "unitigs",
 * their links and "tips": slot t = 2u + side, L_u records, bases(u) = L_u + k - 1, abundance sum KC_u.
 *   names  : slot (u, s) NAMES slot (v, 1 - m) when (v, m) is an entry of slot 2u + s: the arrival slot of the tips text. At odd k naming is symmetric; at even k these
 *            sentences are the whole definition and no parity is claimed.
 *   round  : of one kind (0 tips, 1 bulges, 2 erroneous connections), decided on the graph at its start; all hits are removed together exactly as a tip round does it:
 *            the records of a hit die, their masks become 0, every bit of an alive record's mask that named a dead record is cleared, the next round compacts again.
 *   bulge  : (a simple bubble) unitig u is a bulge when all of the following hold.
 *            1. Both of its slots have at least one entry, and bases(u) <= bulge_max_len.
 *            2. There is a unitig c != u, taken in an orientation o in {0, 1}, that runs parallel to it: there is a slot X whose unitig is neither u nor c such that
 *               (u, 0) names X, X names (c, o) and (c, o) names X; and a slot Y whose unitig is neither u nor c such that (u, 1) names Y and (c, 1 - o) names Y.
 *            3. L_c <= max(L_u * bulge_alt_num / bulge_alt_den, L_u + bulge_alt_add), in integer division (the reference's maxlen: 11 / 10 and + 3).
 *            4. c beats u: KC_u * L_c < KC_c * L_u, or the two products are equal and c < u (exact integers). "Beats" is a strict total order: of any set of mutually
 *               parallel unitigs the best covered one is never removed, and two twins never remove each other.
 *            The work per unitig is bounded: at most 4 X of at most 4 entries each give at most 16 (c, o), each checked against at most 4 x 4 slot pairs.
 *   EC     : (erroneous connection) unitig u is an EC when all of the following hold.
 *            1. Both slots have at least one entry, and bases(u) <= ec_max_len.
 *            2. On each of its two sides some slot it names has at least two entries: u has a sibling at both ends (the Z shape of the reference's comment).
 *            3. On at least one side some competitor c != u has KC_c * L_u * ec_den > ec_num * KC_u * L_c (strict, exact integers). The competitors of a side are those
 *               of the tips rule: per entry (v, m) of the slot, v itself and every entry of v's arrival slot except the ONE entry that is u coming back.
 *            A single-record unitig can be an EC.
 *   phase  : phase(kind) runs rounds of that kind until one removes nothing or the kind's max_rounds have run; a kind whose max_rounds is 0 is skipped.
 *   call   : phase(tips) (sweep 0), then sweeps 1, 2, ... of phase(bulges), phase(ec), phase(tips), until a whole sweep removes nothing or max_sweeps have run.
 * Against the reference: the order is that of its simplify() (tips to exhaustion, then bulges and ECs, then a mix); the stop rule is this library's. The bulge rule
 * differs: the reference accepts cov_u <= 1.1 cov_alt and searches alternative paths of several unitigs (heuristic_most_covered_path); here the alternative is ONE unitig
 * and the comparison is strict. The EC rule is in integers; the reference skips pathLen == 0, this library removes nodes of any path length. What is claimed: the
 * reference's three unit tests with known answers (debruijn_simplunitigs_bubble, _bubble_snp, _ec; tests/golden/reference_simplify_vectors.json), nothing more.
 * Not served: alternative paths of several unitigs, the reference's floating-point coverage rules, the removal of isolated short unitigs, the drop-in, communicators,
 * the merged state of a gkc_banks.
 * Timing names of gkc_get_timing: "graph_bulges" and "graph_ec" (KC when the round is the first on its graph, flags, mark, kill and refresh of that kind's rounds; launch
 * count: that kind's rounds on a graph that has unitigs); tip rounds inside keep "graph_tips". A round that removed nothing leaves placement, link CSR and KC valid and
 * the next round starts on them: a call runs (rounds that removed something) + 1 builds, observable as the launch count of "graph_links". */
typedef struct gkc_simplify_params {
    gkc_tip_params tips;                   /* tips.max_rounds: per phase; 0 = no tip phases */
    uint32_t bulge_max_len, bulge_alt_num, bulge_alt_den, bulge_alt_add, bulge_max_rounds;
    uint32_t ec_max_len, ec_num, ec_den, ec_max_rounds;
    uint32_t max_sweeps;                   /* 0: only the leading tip phase; > 16: GKC_ERR_ARG */
    uint32_t resume;                       /* 0: every record starts alive (d_alive is written first); 1: d_masks / d_alive are a consistent state an earlier call left */
} gkc_simplify_params;
typedef struct gkc_simplify_round { uint32_t kind /* 0 tips, 1 bulges, 2 ec */, sweep; uint64_t n_unitigs, n_hits, n_records_removed; } gkc_simplify_round;
/* d_masks, d_alive, the counts on return, state rules, error behaviour and invalidation: those of gkc_graph_tips_remove; the context's placement is the final graph's and
 * gkc_graph_unitigs_write / _nodes / _links answer for it. *n_rounds: every round run, empty ones included; log: host, receives the first cap_log of them (n_unitigs: of
 * the graph the round was decided on), or NULL. Any zero denominator, a max_rounds above 64 or max_sweeps above 16: GKC_ERR_ARG. resume = 1: d_alive is read, a dead
 * record with a mask and masks that name a dead or missing record are GKC_ERR_ARG. No solid k-mer: GKC_OK, zero counts. */
int gkc_graph_simplify(gkc_ctx* ctx, uint8_t* d_masks, uint8_t* d_alive, const gkc_simplify_params* params, gkc_simplify_round* log, uint64_t cap_log,
                       uint64_t* n_rounds, uint64_t* n_records_removed, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* n_cycles);

/* ---- read paths: where the k-mers of reads lie in the compacted graph, and the unitigs a read spells, on the device ---------------------------------
 * The join of "abundance queries" and "unitigs": the k-mers of a flat read buffer are searched in the results exactly as gkc_query_reads_device searches them, and
 * the record found answers with its place in the placement the context holds — the plain build's, gkc_graph_unitigs_build_alive's, or the one gkc_graph_tips_remove /
 * gkc_graph_simplify left. All terms are those of "unitigs": unitig u, L_u records, record i placed at (u, rev_i, p).
 *   node   : g = index of the k-mer's FIRST base in the flat buffer, as in gkc_query_reads_device. f = the k-mer as the read spells it, c = min(f, revcomp(f)) = record i.
 *            d_node[g] = u << 1 | strand, d_pos[g] = p, strand = rev_i XOR (f != c). strand 0: f equals bases [p, p + k) of unitig u as gkc_graph_unitigs_write emits it;
 *            strand 1: f equals their reverse complement. A palindrome (even k) has f == c and takes the strand of its record: no special case.
 *            GKC_NODE_REMOVED : c is a record of the results but of no unitig of this placement (what gkc_graph_unitigs_nodes reports as ~0: a dead record; only on a
 *                               placement built over an alive array);
 *            GKC_NODE_ABSENT  : a valid k-mer that is not in the results (gkc_query_reads_device: 0);
 *            GKC_NODE_NO_KMER : no k-mer starts here (gkc_query_reads_device: -1).
 *            d_pos[g] = 0 under a sentinel. Every value below GKC_NODE_NO_KMER that is no sentinel is a node.
 *   segment: inside one read, position j CONTINUES position j - 1 when both carry a node, the two node values are equal (same unitig, same strand) and
 *            pos_j == pos_{j-1} + 1 on strand 0, pos_j == pos_{j-1} - 1 on strand 1. The match is exact: there is no wrap around the cut of a cycle, a read that runs
 *            round a cycle breaks there. A segment is a maximal run of such positions: node, read_pos = the offset of its first k-mer inside the read, unitig_pos = that
 *            k-mer's position in the unitig, n_kmers = its length. The segments of a read are in ascending read_pos; d_seg_offsets is the CSR over the reads.
 *   support: d_support[u] = the sum of n_kmers over all segments on u, either strand.
 * State: the rules of the abundance queries, and for the nodes call (and for the segments call when d_support is given) a valid placement: GKC_ERR_ARG before a build
 * or after the results changed, as for gkc_graph_unitigs_write. Offsets are checked as gkc_query_reads_device checks them; bad offsets touch no memory outside the
 * buffers.
 *   junction: of segment s, one u64: its relation to segment s + 1 of the SAME read. A = segment s, B = segment s + 1, gap = read_pos_B - (read_pos_A + n_kmers_A) (the
 *            segments of a read are ascending and disjoint: gap >= 0); last_pos(A) = unitig_pos_A + (n_kmers_A - 1) on strand 0, unitig_pos_A - (n_kmers_A - 1) on
 *            strand 1. The slot a segment leaves through is 2u + strand = node_A itself (strand 0 runs to the end of u, side 0; strand 1 to its begin, side 1), and the
 *            entry that names how B is entered is node_B itself (strand 0 enters at the begin of v, mv = 0; strand 1 at its end, mv = 1): the lookup translates nothing.
 *            The rules, in this order:
 *            1. GKC_JUNCTION_END      : s is the last segment of its read.
 *            2. a link entry index e  : gap == 0, A leaves at the extremity of its unitig (last_pos(A) == L_u - 1 on strand 0, == 0 on strand 1), B enters at one
 *                                       (unitig_pos_B == 0 on strand 0, == L_v - 1 on strand 1), and slot node_A holds an entry equal to node_B: the index of that
 *                                       entry in d_links, the lowest one if the slot holds the value twice (even k). Every value below GKC_JUNCTION_UNLINKED is a link index.
 *            3. GKC_JUNCTION_UNLINKED : gap == 0 and rule 2 fails. With segments, links and placement of one graph this never occurs at odd k (two adjacent alive k-mers
 *                                       of a read are neighbours, and neighbours that do not continue each other are extremities joined by a link); at even k a
 *                                       palindromic record can produce it, and it is then the defined answer.
 *            4. GKC_JUNCTION_COLLINEAR: gap > 0, node_B == node_A and unitig_pos_B == unitig_pos_A + (n_kmers_A + gap) on strand 0, - on strand 1: the read runs on along
 *                                       the same unitig behind something of the same length (a substitution in the read, a same-length bulge that simplify removed). A
 *                                       label; nothing is corrected.
 *            5. GKC_JUNCTION_BREAK    : everything else with gap > 0.
 *   walk   : a maximal run of consecutive segments of one read in which every junction is a link index: a path in the compacted graph that spells read bases
 *            [read_pos_first, read_pos_first + n_kmers + k - 1). first_segment indexes d_segments; n_kmers is the sum over its segments (they are contiguous in the
 *            read: read_pos_last + n_kmers_last - read_pos_first). The walks of a read are ascending, d_walk_offsets is the CSR over the reads, a read without
 *            segments has no walk. n_walks = n_segments - (the junctions that are link indices).
 *   link support: d_link_support[e] = the number of junctions whose value is e. Raw and per entry: at odd k the traversals in the other direction are counted on the
 *            MIRROR entry (the mirror of e in slot 2u + su with value (v, mv) is the entry (u, 1 - su) in slot 2v + (1 - mv)); the two counts are not folded.
 *   map    : a segment on node 2u + strand with its first k-mer at (read_pos, unitig_pos) gives read position x of its read a unitig base: on strand 0 base
 *            unitig_pos + (x - read_pos) of unitig u as gkc_graph_unitigs_write emits it, on strand 1 the COMPLEMENT of base unitig_pos + k - 1 - (x - read_pos).
 *   region : a stretch of a read that no k-mer of a segment covers and that one segment's map reaches. Three kinds, each handled on its own:
 *            gap : A, B consecutive in one read and in the COLLINEAR relation of rule 4; read positions [read_pos_A + n_kmers_A + k - 1, read_pos_B), targets from A's
 *                  map (collinearity keeps them inside the unitig). Empty when gap < k (a cycle's cut can give that): nothing is done and nothing counted.
 *            head: (params.ends) the first segment F of the read has read_pos_F > 0: [0, read_pos_F), targets from F's map. ROOM is required: strand 0
 *                  unitig_pos_F >= read_pos_F, strand 1 unitig_pos_F + read_pos_F <= L_u - 1. Without room the region is left alone and counted as ends_no_room.
 *            tail: (params.ends) the last segment Z leaves t = len - (read_pos_Z + n_kmers_Z + k - 1) > 0 bases: the last t bases, targets from Z's map. Room: strand 0
 *                  unitig_pos_Z + n_kmers_Z - 1 + t <= L_u - 1, strand 1 unitig_pos_Z - (n_kmers_Z - 1) >= t.
 *   correction: the CHANGES of a region are the positions whose input byte differs from the target byte (targets are upper-case ACGT: an N or a lower-case letter is a
 *            change). changes <= params.max_subst: the region's bytes become the targets (gaps_fixed / heads_fixed / tails_fixed); otherwise it is left alone
 *            (gaps_skipped / ends_skipped). Whole or not at all. Every other byte of the output equals the input: substitutions only, lengths and offsets never change, a
 *            read without a segment is copied. The regions of a read are disjoint: the result does not depend on the order they are evaluated in.
 * Not served: the ranks of a communicator beyond the datasets a rank holds, and the merged state of a gkc_banks; walks across collinear gaps (a COLLINEAR junction ends
 * a walk), also across corrected ones; the folded (mirror) support of a link; of the correction: gaps whose two sides lie on different unitigs (an error next to a
 * branching node), insertions and deletions, a choice between alternatives by coverage; the drop-in.
 * Timing names of gkc_get_timing: "graph_read_nodes", "graph_read_segments", "graph_read_walks", "graph_read_correct" (the index: "query_index"). */
#define GKC_NODE_REMOVED  (~0ull)        /* in the results, but a record of no unitig in this placement */
#define GKC_NODE_ABSENT   (~0ull - 1)    /* a valid k-mer that is not in the results */
#define GKC_NODE_NO_KMER  (~0ull - 2)    /* no k-mer starts here */
/* d_bases, d_offsets, n_reads, n_bases: the arguments of gkc_query_reads_device, with its limits (d_bases 16-byte aligned, fewer than 2^40 bases). d_node: u64[n_bases],
 * 16-byte aligned. d_pos: u32[n_bases], 16-byte aligned, or NULL (not written, not fetched). */
int gkc_graph_reads_nodes_device(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t* d_node, uint32_t* d_pos);
typedef struct gkc_read_segment { uint64_t node; uint32_t read_pos, unitig_pos, n_kmers, pad /* 0 */; } gkc_read_segment;   /* 24 bytes */
/* d_node, d_pos: what gkc_graph_reads_nodes_device wrote for the same offsets (both required; they are read, never searched again: the call needs no counted results
 * unless d_support is given). d_seg_offsets: u64[n_reads + 1]; d_segments: room for cap_segments; both NULL: only *n_segments is reported. Too small: GKC_ERR_CAPACITY,
 * *n_segments reported, nothing written. A read of 2^32 bases or more: GKC_ERR_ARG. d_support: u64[n_unitigs of the context's placement] or NULL; zeroed and filled by
 * a call that writes segments (not by the sizing call); a node that names no unitig of that placement (nodes of another placement): GKC_ERR_ARG, nothing written outside
 * the array. No reads, or no bases: GKC_OK, every offset 0, *n_segments = 0. */
int gkc_graph_reads_segments_device(gkc_ctx* ctx, const uint64_t* d_node, const uint32_t* d_pos, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                    uint64_t* d_seg_offsets, gkc_read_segment* d_segments, uint64_t cap_segments, uint64_t* n_segments, uint64_t* d_support);
#define GKC_JUNCTION_END       (~0ull)        /* the last segment of its read */
#define GKC_JUNCTION_BREAK     (~0ull - 1)    /* a gap, and not collinear */
#define GKC_JUNCTION_COLLINEAR (~0ull - 2)    /* a gap, behind it the same unitig goes on where a piece of the gap's length would end */
#define GKC_JUNCTION_UNLINKED  (~0ull - 3)    /* no gap, but no link entry joins the two segments; every value below this one is an index into d_links */
typedef struct gkc_read_walk { uint64_t first_segment; uint32_t n_segments, n_kmers; } gkc_read_walk;   /* 16 bytes */
/* d_seg_offsets (u64[n_reads + 1]), d_segments: what gkc_graph_reads_segments_device wrote; d_link_offsets (u64[2 n_unitigs + 1]), d_links (n_links entries): what
 * gkc_graph_unitigs_links wrote for the placement the context holds; n_unitigs and the L_u are the placement's: GKC_ERR_ARG before a build or after the results changed.
 * Fewer than 2^40 segments per call. d_walk_offsets: u64[n_reads + 1]; d_walks: room for cap_walks; both NULL: only *n_walks is reported and nothing is written; one
 * without the other: GKC_ERR_ARG. Too small: GKC_ERR_CAPACITY, *n_walks reported, nothing written. d_junction (u64[n_segments]) and d_link_support (u64[n_links]), each
 * or NULL, are written only by a call that writes walks; the support is zeroed, then filled. Found on the device, never by reading outside a buffer, and answered with
 * GKC_ERR_ARG and no output written: d_seg_offsets is no CSR table over n_segments; two segments of a read overlap or descend; a node names a unitig >= n_unitigs; a
 * slot's range is descending or not inside [0, n_links]. No reads, or no segments: GKC_OK, every offset 0, *n_walks = 0, the support zeroed when given. */
int gkc_graph_reads_walks_device(gkc_ctx* ctx, const uint64_t* d_seg_offsets, const gkc_read_segment* d_segments, uint64_t n_reads, uint64_t n_segments,
                                 const uint64_t* d_link_offsets, const uint64_t* d_links, uint64_t n_links, uint64_t* d_junction,
                                 uint64_t* d_walk_offsets, gkc_read_walk* d_walks, uint64_t cap_walks, uint64_t* n_walks, uint64_t* d_link_support);
typedef struct gkc_correct_params { uint32_t max_subst; uint32_t ends; uint32_t pad[2]; } gkc_correct_params;   /* NULL: {2, 1} */
typedef struct gkc_correct_stats  { uint64_t gaps_fixed, gaps_skipped, heads_fixed, tails_fixed, ends_skipped, ends_no_room, bases_changed; } gkc_correct_stats;
/* The reads rewritten to what the graph says ("region", "correction" above). d_bases, d_offsets, n_reads, n_bases: the reads, as for gkc_graph_reads_nodes_device (16-byte
 * aligned, fewer than 2^40 bases, no read of 2^32 bases or more); d_seg_offsets, d_segments, n_segments (fewer than 2^40): what gkc_graph_reads_segments_device wrote for
 * them; d_unitig_bases, d_unitig_offsets: what gkc_graph_unitigs_write wrote for the placement the context holds; n_unitigs and the L_u are the placement's: GKC_ERR_ARG
 * before a build or after the results changed. d_out: char[n_bases], 16-byte aligned; it may EQUAL d_bases (in place, nothing is copied), any other overlap is GKC_ERR_ARG.
 * d_n_changed (u32[n_reads]: the bases changed per read) and d_changed_bits (u64[(n_bases + 63) / 64]: bit g & 63 of word g >> 6 is set where byte g changed), each or
 * NULL, are fully written by a successful call. stats: host, or NULL. Found on the device before anything is written, never by reading outside a buffer, and answered
 * with GKC_ERR_ARG and no output touched: d_offsets or d_seg_offsets is no CSR table; two segments of a read overlap or descend; a segment runs past its read (read_pos +
 * n_kmers + k - 1 > len); a node names a unitig >= n_unitigs; a segment holds no k-mer or its unitig range leaves [0, L_u); d_unitig_offsets[0] != 0 or
 * d_unitig_offsets[u + 1] - d_unitig_offsets[u] != L_u + k - 1 for some u (the strings of another placement). No reads, or no segments: GKC_OK, the output is a copy, the
 * stats are zero. */
int gkc_graph_reads_correct_device(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                   const uint64_t* d_seg_offsets, const gkc_read_segment* d_segments, uint64_t n_segments,
                                   const char* d_unitig_bases, const uint64_t* d_unitig_offsets,
                                   const gkc_correct_params* params, char* d_out, uint32_t* d_n_changed, uint64_t* d_changed_bits, gkc_correct_stats* stats);

/* ---- input: FASTA / FASTQ text -> flat bases + offsets ON THE DEVICE ------------------------------------
 * Replaces BankFasta::Iterator::get_next_seq_from_file (bank/impl/BankFasta.cpp:488-571, buffered_gets :425-483) and the
 * per-sequence copy into the flat buffer that gkc_push_reads takes. Same result as the reference reader for well-formed text:
 *   FASTA : a line starting with '>' or '@' is a header, all other lines are sequence data (multi-line, CRLF: one trailing '\r' per
 *           line dropped exactly like BankFasta.cpp:479; empty lines ignored);
 *   FASTQ : four lines per record, quality at least as long as the sequence.
 * Anything whose result under the reference's character state machine is NOT expressible per line (multi-line FASTQ, quality shorter
 * than the sequence, a sequence line starting with '+', '>' / '@' before the first header line) returns GKC_ERR_FORMAT — there is no
 * host fallback inside the library.
 * d_text: n_bytes of text in device memory. final_chunk = 0: only complete records are parsed and *consumed tells how many bytes
 * they covered (feed the rest again in front of the next chunk); 1: the text ends here. Outputs are allocated by the library
 * (gkc_device_free): d_bases[n_bases], d_offsets[n_reads + 1] — exactly the arguments of gkc_push_reads_device. */
int gkc_fastx_parse_device(gkc_ctx* ctx, const char* d_text, uint64_t n_bytes, int final_chunk,
                           char** d_bases, uint64_t** d_offsets, uint64_t* n_reads, uint64_t* n_bases, uint64_t* consumed);
/* host text -> H2D -> gkc_fastx_parse_device -> gkc_push_reads_device, inside a pass */
int gkc_push_fastx(gkc_ctx* ctx, const char* text, uint64_t n_bytes, int final_chunk, uint64_t* consumed);

int gkc_device_free(gkc_ctx* ctx, void* d_ptr);
/* Gives the result buffers of a finished pass back (its datasets are gone afterwards: gkc_partition_* on them fail). A host that has drained
 * a pass — the processors have seen every partition — calls it before the next pass, so that a multi-pass count keeps only ONE pass of results
 * in HBM: the point of nb_passes in the reference, which bounds the footprint of a pass and removes the partition files of a pass before the
 * next one (SortingCountAlgorithm.cpp:1219-1241, :705-720; pass count from the available memory / disk: ConfigurationAlgorithm.cpp:398-425). */
int gkc_release_pass(gkc_ctx* ctx, uint32_t pass);
/* HBM the context can use right now (free on the device + blocks parked in its own allocator) and the device total, in bytes: what a host-side
 * configuration step sizes nb_passes / nb_partitions from (the reference reads System::info().getMemoryPhysicalTotal / -max-memory there). */
int gkc_device_memory(gkc_ctx* ctx, uint64_t* usable_bytes, uint64_t* total_bytes);
/* Page-locked host memory for the buffers the host side hands to gkc_push_reads / gkc_push_fastx and receives Count[] records in
 * (gkc_partition_counts): the DMA engines then move them at PCIe rate, pageable memory is staged by the driver at about half of it
 * (measured: DESIGN.md section 6). This is the role of the reference's host-side buffer provider for partition data
 * (tools/misc/impl/Pool.hpp:343-418, MemAllocator, and the BagCache buffers of CountProcessorDump.hpp:134): memory the counting
 * back-end fills and the processors read. No context needed; *p = NULL and GKC_ERR_NOMEM when the allocation fails. */
int gkc_host_alloc(void** p, uint64_t n_bytes);
int gkc_host_free(void* p);
int gkc_device_to_host(gkc_ctx* ctx, void* dst, const void* d_src, uint64_t n_bytes);
int gkc_host_to_device(gkc_ctx* ctx, void* d_dst, const void* src, uint64_t n_bytes);
/* order-independent checksum of the canonical k-mer multiset of device-resident reads, computed by an independent
 * one-thread-per-position kernel (no minimizers, no buckets): sum over valid k-mers of mix(canonical) mod 2^64, and the
 * number of valid k-mers. Used by the full-size parity property "sum_records count*mix(value) == this". */
int gkc_kmer_checksum_device(gkc_ctx* ctx, const char* d_bases, const uint64_t* d_offsets, uint64_t n_reads,
                             uint64_t n_bases, uint64_t* checksum, uint64_t* n_valid);
/* the same checksum over the finished datasets of the context: sum abundance*mix(value), sum abundance */
int gkc_result_checksum(gkc_ctx* ctx, uint64_t* checksum, uint64_t* sum_abundance);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GKC_H */
