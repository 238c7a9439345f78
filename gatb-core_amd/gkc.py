"""ctypes binding over the C-ABI of libgkc_hip.so (include/gkc.h). No torch types cross the boundary.

The extension is REQUIRED: every entry point raises GkcError if the library is missing or a call fails;
there is no CPU fallback anywhere in this module (the CPU oracle lives in oracle/ and is test-only).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO = os.environ.get("GKC_LIB") or os.path.join(CSRC, "libgkc_hip.so")      # GKC_LIB: an experiment build of the same library (tools/build_variant.sh)
_LIB = None

SYMBOLS = [
    "gkc_create", "gkc_destroy", "gkc_last_error", "gkc_version", "gkc_configure", "gkc_set_solidity",
    "gkc_set_max_superkmer", "gkc_set_batch_keys", "gkc_begin_pass", "gkc_push_reads", "gkc_push_reads_device", "gkc_finish_pass",
    "gkc_partition_info", "gkc_partition_counts", "gkc_partition_counts_range", "gkc_partition_counts_device", "gkc_histogram", "gkc_get_stats",
    "gkc_get_timing", "gkc_partition_superkmers", "gkc_segment_count", "gkc_segment_export", "gkc_segment_import",
    "gkc_segments_clear", "gkc_bloom_create", "gkc_bloom_destroy", "gkc_bloom_nbytes", "gkc_bloom_bitsize",
    "gkc_bloom_insert", "gkc_bloom_insert_device", "gkc_bloom_insert_solid", "gkc_bloom_query_solid", "gkc_bloom_contains",
    "gkc_bloom_contains8", "gkc_bloom_get_array", "gkc_bloom_set_array", "gkc_bloom_device_array", "gkc_synth_reads_device", "gkc_synth_reads_profile_device", "gkc_device_free", "gkc_host_alloc", "gkc_host_free", "gkc_release_pass", "gkc_device_memory",
    "gkc_fastx_parse_device", "gkc_push_fastx", "gkc_mphf_build", "gkc_mphf_build_solid", "gkc_mphf_destroy", "gkc_mphf_size",
    "gkc_mphf_lookup", "gkc_mphf_save_size", "gkc_mphf_save", "gkc_mphf_abundance_map",
    "gkc_device_to_host", "gkc_kmer_checksum_device", "gkc_result_checksum", "gkc_sample_minimizers", "gkc_count_mmers",
    "gkc_host_to_device", "gkc_comm_unique_id", "gkc_comm_create_rccl", "gkc_comm_create_transport", "gkc_comm_create_files", "gkc_comm_enable_ipc", "gkc_gather_results", "gkc_comm_loopback", "gkc_comm_selftest", "gkc_comm_peer_bytes", "gkc_comm_destroy", "gkc_comm_set_owners",
    "gkc_comm_get_owners", "gkc_balanced_owner_ranges", "gkc_exchange", "gkc_comm_get_stats", "gkc_bloom_allreduce_or",
    "gkc_mphf_build_solid_dist", "gkc_mphf_abundance_map_dist", "gkc_exchange_plan",
    "gkc_sample_exact", "gkc_set_host_sink", "gkc_set_sink_mode", "gkc_finish_pass_async", "gkc_wait_partition", "gkc_finish_pass_wait",
    "gkc_banks_create", "gkc_banks_destroy", "gkc_banks_add", "gkc_banks_evaluate", "gkc_banks_partition_info", "gkc_banks_partition_counts",
    "gkc_banks_partition_vectors", "gkc_banks_partition_counts_device", "gkc_banks_histogram",
    "gkc_query_reads_device", "gkc_query_reads", "gkc_query_kmers_device", "gkc_query_kmers", "gkc_query_read_summary_device", "gkc_query_banks_reads_device",
    "gkc_graph_neighbors_solid", "gkc_graph_neighbors_partition", "gkc_graph_branching_solid",
    "gkc_graph_unitigs_build", "gkc_graph_unitigs_write", "gkc_graph_unitigs_nodes", "gkc_graph_unitigs_links",
    "gkc_graph_unitigs_build_alive", "gkc_graph_tips_remove", "gkc_graph_simplify",
    "gkc_graph_reads_nodes_device", "gkc_graph_reads_segments_device", "gkc_graph_reads_walks_device",
    "gkc_graph_reads_correct_device",
]

# -solidity-kind of the reference (include/gkc.h GKC_SOLIDITY_*)
GKC_SOLIDITY_SUM, GKC_SOLIDITY_MIN, GKC_SOLIDITY_MAX, GKC_SOLIDITY_ONE, GKC_SOLIDITY_ALL, GKC_SOLIDITY_CUSTOM = range(6)
SOLIDITY_KINDS = {"sum": GKC_SOLIDITY_SUM, "min": GKC_SOLIDITY_MIN, "max": GKC_SOLIDITY_MAX, "one": GKC_SOLIDITY_ONE, "all": GKC_SOLIDITY_ALL,
                  "custom": GKC_SOLIDITY_CUSTOM}


class GkcError(RuntimeError):
    pass


class Xfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("reserved", C.c_int32), ("d_ptr", C.c_void_p), ("n_bytes", C.c_uint64)]


ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
SENDRECV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Xfer), C.c_uint32, C.POINTER(Xfer), C.c_uint32)


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allgather_host", ALLGATHER_CB), ("sendrecv_device", SENDRECV_CB)]


class PlanMsg(C.Structure):
    _fields_ = [("peer", C.c_int32), ("seg", C.c_uint32), ("rec_begin", C.c_uint64), ("n_recs", C.c_uint64)]


class CommStats(C.Structure):
    _fields_ = [("n_exchanges", C.c_uint64), ("bytes_sent", C.c_uint64), ("bytes_received", C.c_uint64), ("ms_transfer", C.c_double),
                ("ms_host", C.c_double), ("reserved", C.c_uint64 * 4)]


class TipParams(C.Structure):
    """gkc_tip_params (include/gkc.h)"""
    _fields_ = [(n, C.c_uint32) for n in ("max_len_topo", "max_len_rc", "rc_num", "rc_den", "max_rounds")]


class SimplifyParams(C.Structure):
    """gkc_simplify_params (include/gkc.h)"""
    _fields_ = [("tips", TipParams)] + [(n, C.c_uint32) for n in (
        "bulge_max_len", "bulge_alt_num", "bulge_alt_den", "bulge_alt_add", "bulge_max_rounds", "ec_max_len", "ec_num", "ec_den", "ec_max_rounds", "max_sweeps", "resume")]


class SimplifyRound(C.Structure):
    """gkc_simplify_round (include/gkc.h)"""
    _fields_ = [("kind", C.c_uint32), ("sweep", C.c_uint32), ("n_unitigs", C.c_uint64), ("n_hits", C.c_uint64), ("n_records_removed", C.c_uint64)]


SIMPLIFY_KINDS = ("tips", "bulges", "ec")
SIMPLIFY_LOG_CAP = 64 + 16 * 3 * 64                             # the most rounds a call can run


class ReadSegment(C.Structure):
    """gkc_read_segment (include/gkc.h): 24 bytes"""
    _fields_ = [("node", C.c_uint64), ("read_pos", C.c_uint32), ("unitig_pos", C.c_uint32), ("n_kmers", C.c_uint32), ("pad", C.c_uint32)]


# gkc_read_segment as a numpy record, and the sentinels of d_node (GKC_NODE_*)
READ_SEGMENT = np.dtype([("node", np.uint64), ("read_pos", np.uint32), ("unitig_pos", np.uint32), ("n_kmers", np.uint32), ("pad", np.uint32)])
NODE_REMOVED, NODE_ABSENT, NODE_NO_KMER = (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 3


class ReadWalk(C.Structure):
    """gkc_read_walk (include/gkc.h): 16 bytes"""
    _fields_ = [("first_segment", C.c_uint64), ("n_segments", C.c_uint32), ("n_kmers", C.c_uint32)]


# gkc_read_walk as a numpy record, and the values of a junction that are no link index (GKC_JUNCTION_*)
READ_WALK = np.dtype([("first_segment", np.uint64), ("n_segments", np.uint32), ("n_kmers", np.uint32)])
JUNCTION_END, JUNCTION_BREAK, JUNCTION_COLLINEAR, JUNCTION_UNLINKED = (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 3, (1 << 64) - 4


class CorrectParams(C.Structure):
    """gkc_correct_params (include/gkc.h): 16 bytes"""
    _fields_ = [("max_subst", C.c_uint32), ("ends", C.c_uint32), ("pad", C.c_uint32 * 2)]


class CorrectStats(C.Structure):
    """gkc_correct_stats (include/gkc.h): 56 bytes"""
    _fields_ = [(n, C.c_uint64) for n in ("gaps_fixed", "gaps_skipped", "heads_fixed", "tails_fixed", "ends_skipped", "ends_no_room", "bases_changed")]


# gkc_read_abundance (include/gkc.h) as a numpy record
READ_ABUNDANCE = np.dtype([("n_valid", np.uint32), ("n_found", np.uint32), ("min", np.int32), ("max", np.int32), ("sum", np.uint64)])


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "kmers_nb_valid", "kmers_nb_invalid", "kmers_nb_distinct", "kmers_nb_solid", "nb_superkmers", "nb_sequences",
        "nb_bases", "superkmer_bytes", "oversize_buckets", "dedupe_kmers_in", "dedupe_keys_out", "seq_len_min", "seq_len_max", "seq_len_sq_sum")] + [("reserved", C.c_uint64 * 2)]


def build(force=False):
    """Compile csrc/*.hip for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))]
    srcs.append(os.path.join(_HERE, "..", "include", "gkc.h"))
    stale = force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return SO


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO):
        raise GkcError("libgkc_hip.so is missing (%s): run __graft_entry__.build(); there is no CPU fallback" % SO)
    L = C.CDLL(SO)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
    P = C.POINTER
    sig = {
        "gkc_create": (C.c_int, [C.c_int, P(vp)]),
        "gkc_destroy": (None, [vp]),
        "gkc_last_error": (C.c_char_p, [vp]),
        "gkc_version": (C.c_char_p, []),
        "gkc_configure": (C.c_int, [vp, u32, u32, u32, u32, C.c_int, vp, vp]),
        "gkc_set_solidity": (C.c_int, [vp, i32, i32, u32]),
        "gkc_set_max_superkmer": (C.c_int, [vp, u32]),
        "gkc_set_batch_keys": (C.c_int, [vp, u64]),
        "gkc_begin_pass": (C.c_int, [vp, u32]),
        "gkc_push_reads": (C.c_int, [vp, vp, vp, u64]),
        "gkc_push_reads_device": (C.c_int, [vp, vp, vp, u64, u64]),
        "gkc_finish_pass": (C.c_int, [vp]),
        "gkc_partition_info": (C.c_int, [vp, u32, u32, P(u64), P(u64), P(u64)]),
        "gkc_partition_counts": (C.c_int, [vp, u32, u32, vp, u64, P(u64)]),
        "gkc_partition_counts_range": (C.c_int, [vp, u32, u32, u64, u64, vp]),
        "gkc_partition_counts_device": (C.c_int, [vp, u32, u32, P(vp), P(u64)]),
        "gkc_histogram": (C.c_int, [vp, vp, u32]),
        "gkc_get_stats": (C.c_int, [vp, P(Stats)]),
        "gkc_get_timing": (C.c_int, [vp, C.c_char_p, P(C.c_double), P(u64)]),
        "gkc_partition_superkmers": (C.c_int, [vp, u32, vp, u64, P(u64), P(u64), P(u64)]),
        "gkc_segment_count": (C.c_int, [vp, P(u32)]),
        "gkc_segment_export": (C.c_int, [vp, u32, P(vp), P(u32), vp, vp]),
        "gkc_segment_import": (C.c_int, [vp, vp, vp, vp]),
        "gkc_segments_clear": (C.c_int, [vp]),
        "gkc_bloom_create": (C.c_int, [vp, C.c_int, u64, u32, u32, P(vp)]),
        "gkc_bloom_destroy": (None, [vp]),
        "gkc_bloom_nbytes": (u64, [vp]),
        "gkc_bloom_bitsize": (u64, [vp]),
        "gkc_bloom_insert": (C.c_int, [vp, vp, u64, u32]),
        "gkc_bloom_insert_device": (C.c_int, [vp, vp, u64, u32]),
        "gkc_bloom_insert_solid": (C.c_int, [vp, vp]),
        "gkc_bloom_query_solid": (C.c_int, [vp, vp, C.c_int, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "gkc_bloom_contains": (C.c_int, [vp, vp, u64, u32, vp]),
        "gkc_bloom_contains8": (C.c_int, [vp, vp, u64, u32, vp]),
        "gkc_bloom_get_array": (C.c_int, [vp, vp, u64]),
        "gkc_bloom_set_array": (C.c_int, [vp, vp, u64]),
        "gkc_bloom_device_array": (C.c_int, [vp, P(vp), P(u64)]),
        "gkc_synth_reads_device": (C.c_int, [vp, u64, u64, u64, u32, u64, u32, P(vp), P(vp)]),
        "gkc_synth_reads_profile_device": (C.c_int, [vp, u64, u64, u64, u32, u64, u32, u32, P(vp), P(vp)]),
        "gkc_device_free": (C.c_int, [vp, vp]),
        "gkc_host_alloc": (C.c_int, [P(vp), u64]),
        "gkc_host_free": (C.c_int, [vp]),
        "gkc_release_pass": (C.c_int, [vp, u32]),
        "gkc_device_memory": (C.c_int, [vp, P(u64), P(u64)]),
        "gkc_device_to_host": (C.c_int, [vp, vp, vp, u64]),
        "gkc_fastx_parse_device": (C.c_int, [vp, vp, u64, C.c_int, P(vp), P(vp), P(u64), P(u64), P(u64)]),
        "gkc_push_fastx": (C.c_int, [vp, vp, u64, C.c_int, P(u64)]),
        "gkc_mphf_build": (C.c_int, [vp, vp, u64, u32, u32, P(vp)]), "gkc_mphf_build_solid": (C.c_int, [vp, P(vp)]),
        "gkc_mphf_destroy": (None, [vp]), "gkc_mphf_size": (u64, [vp]), "gkc_mphf_lookup": (C.c_int, [vp, vp, u64, u32, vp]),
        "gkc_mphf_save_size": (u64, [vp]), "gkc_mphf_save": (C.c_int, [vp, vp, u64]),
        "gkc_mphf_abundance_map": (C.c_int, [vp, vp, vp, u64, P(u64)]),
        "gkc_kmer_checksum_device": (C.c_int, [vp, vp, vp, u64, u64, P(u64), P(u64)]),
        "gkc_result_checksum": (C.c_int, [vp, P(u64), P(u64)]),
        "gkc_sample_minimizers": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "gkc_count_mmers": (C.c_int, [vp, u32, vp, vp, u64, vp]),
        "gkc_host_to_device": (C.c_int, [vp, vp, vp, u64]),
        "gkc_comm_unique_id": (C.c_int, [vp]),
        "gkc_comm_create_rccl": (C.c_int, [vp, vp, C.c_int, C.c_int, P(vp)]),
        "gkc_comm_create_transport": (C.c_int, [vp, P(Transport), C.c_int, C.c_int, P(vp)]),
        "gkc_comm_create_files": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int, P(vp)]),
        "gkc_comm_enable_ipc": (C.c_int, [vp, C.c_int]),
        "gkc_gather_results": (C.c_int, [vp, vp, C.c_int]),
        "gkc_comm_loopback": (C.c_int, [vp, vp, u64, P(u64), P(C.c_double)]),
        "gkc_comm_selftest": (C.c_int, [vp, vp, u64, P(u64), P(C.c_double)]),
        "gkc_comm_peer_bytes": (C.c_int, [vp, vp, vp, P(C.c_double)]),
        "gkc_comm_destroy": (None, [vp]),
        "gkc_comm_set_owners": (C.c_int, [vp, vp]),
        "gkc_comm_get_owners": (C.c_int, [vp, vp]),
        "gkc_balanced_owner_ranges": (C.c_int, [vp, u32, C.c_int, vp]),
        "gkc_exchange": (C.c_int, [vp, vp]),
        "gkc_comm_get_stats": (C.c_int, [vp, P(CommStats)]),
        "gkc_bloom_allreduce_or": (C.c_int, [vp, vp]),
        "gkc_mphf_build_solid_dist": (C.c_int, [vp, vp, P(vp)]),
        "gkc_mphf_abundance_map_dist": (C.c_int, [vp, vp, vp, vp, u64, P(u64)]),
        "gkc_sample_exact": (C.c_int, [vp, vp, vp, u64, u64, vp, vp, vp, P(u64)]),
        "gkc_set_host_sink": (C.c_int, [vp, vp, u64]),
        "gkc_set_sink_mode": (C.c_int, [vp, C.c_int]),
        "gkc_finish_pass_async": (C.c_int, [vp]),
        "gkc_wait_partition": (C.c_int, [vp, u32, u32, P(vp), P(u64)]),
        "gkc_finish_pass_wait": (C.c_int, [vp]),
        "gkc_exchange_plan": (C.c_int, [C.c_int, C.c_int, u32, vp, vp, u64, vp, P(PlanMsg), P(u32), P(PlanMsg), P(u32), P(u64)]),
        "gkc_banks_create": (C.c_int, [vp, u32, P(vp)]),
        "gkc_banks_destroy": (None, [vp]),
        "gkc_banks_add": (C.c_int, [vp, vp, u32]),
        "gkc_banks_evaluate": (C.c_int, [vp, C.c_int, vp, vp, vp, u32]),
        "gkc_banks_partition_info": (C.c_int, [vp, u32, P(u64), P(u64)]),
        "gkc_banks_partition_counts": (C.c_int, [vp, u32, vp, u64, P(u64)]),
        "gkc_banks_partition_vectors": (C.c_int, [vp, u32, vp, u64, P(u64)]),
        "gkc_banks_partition_counts_device": (C.c_int, [vp, u32, P(vp), P(vp), P(u64)]),
        "gkc_banks_histogram": (C.c_int, [vp, vp, u32]),
        "gkc_query_reads_device": (C.c_int, [vp, vp, vp, u64, u64, vp]),
        "gkc_query_reads": (C.c_int, [vp, vp, vp, u64, vp]),
        "gkc_query_kmers_device": (C.c_int, [vp, vp, u64, u32, vp]),
        "gkc_query_kmers": (C.c_int, [vp, vp, u64, u32, vp]),
        "gkc_query_read_summary_device": (C.c_int, [vp, vp, vp, u64, vp]),
        "gkc_query_banks_reads_device": (C.c_int, [vp, vp, vp, u64, u64, vp, vp]),
        "gkc_graph_neighbors_solid": (C.c_int, [vp, vp, P(u64)]),
        "gkc_graph_neighbors_partition": (C.c_int, [vp, u32, u32, vp, P(u64)]),
        "gkc_graph_branching_solid": (C.c_int, [vp, vp, vp, u64, P(u64), vp]),
        "gkc_graph_unitigs_build": (C.c_int, [vp, vp, P(u64), P(u64), P(u64)]),
        "gkc_graph_unitigs_write": (C.c_int, [vp, vp, u64, vp, u64, vp]),
        "gkc_graph_unitigs_nodes": (C.c_int, [vp, vp, vp]),
        "gkc_graph_unitigs_links": (C.c_int, [vp, vp, vp, u64, vp, u64, P(u64)]),
        "gkc_graph_unitigs_build_alive": (C.c_int, [vp, vp, vp, P(u64), P(u64), P(u64)]),
        "gkc_graph_tips_remove": (C.c_int, [vp, vp, vp, P(TipParams), P(u64), vp, P(u64), P(u64), P(u64), P(u64)]),
        "gkc_graph_simplify": (C.c_int, [vp, vp, vp, P(SimplifyParams), P(SimplifyRound), u64, P(u64), P(u64), P(u64), P(u64), P(u64)]),
        "gkc_graph_reads_nodes_device": (C.c_int, [vp, vp, vp, u64, u64, vp, vp]),
        "gkc_graph_reads_segments_device": (C.c_int, [vp, vp, vp, vp, u64, u64, vp, vp, u64, P(u64), vp]),
        "gkc_graph_reads_walks_device": (C.c_int, [vp, vp, vp, u64, u64, vp, vp, u64, vp, vp, vp, u64, P(u64), vp]),
        "gkc_graph_reads_correct_device": (C.c_int, [vp, vp, vp, u64, u64, vp, vp, u64, vp, vp, P(CorrectParams), vp, vp, vp, P(CorrectStats)]),
    }
    for name in SYMBOLS:
        f = getattr(L, name)          # raises AttributeError if the symbol is not exported
        f.restype, f.argtypes = sig[name]
    _LIB = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- host twins of device helpers (full-size parity properties) ----
M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64_np(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def synth_rnd_np(seed, stream, idx):
    with np.errstate(over="ignore"):
        base = mix64_np(np.uint64(seed) ^ (np.uint64(stream) << np.uint64(56)))
        return mix64_np(base + np.asarray(idx, dtype=np.uint64))


def synth_genome_np(seed, pos, profile=0):
    """numpy twin of synth_genome_code (csrc/gkc_api.hip): 2-bit codes of the genome at `pos`"""
    pos = np.asarray(pos, dtype=np.uint64)
    code = (synth_rnd_np(seed, 1, pos) & np.uint64(3)).astype(np.uint32)
    if profile == 1:
        slot = pos >> np.uint64(13); inn = pos & np.uint64(8191)
        h = synth_rnd_np(seed, 4, slot)
        f = (h >> np.uint64(8)) % np.uint64(50)
        ln = np.uint64(1000) + synth_rnd_np(seed, 5, f) % np.uint64(4001)
        rep = ((h & np.uint64(3)) == 0) & (inn < ln)
        fc = (synth_rnd_np(seed, 6, f * np.uint64(8192) + inn) & np.uint64(3)).astype(np.uint32)
        d = synth_rnd_np(seed, 7, pos)
        fc = np.where(d % np.uint64(1000) < np.uint64(5), (fc + 1 + ((d >> np.uint64(32)) % np.uint64(3)).astype(np.uint32)) & 3, fc)
        code = np.where(rep, fc, code)
    return code


def synth_reads_np(seed, n_reads, read_len, genome_len, sub_ppm, first_read=0, profile=0):
    """numpy twin of the k_synth_reads kernel (csrc/gkc_api.hip): -> (bases uint8[n*L], offsets uint64[n+1]); profile 1 = GKC_SYNTH_SKEWED"""
    i = np.repeat(np.arange(first_read, first_read + n_reads, dtype=np.uint64), read_len)
    j = np.tile(np.arange(read_len, dtype=np.uint64), n_reads)
    g = (i - np.uint64(first_read)) * np.uint64(read_len) + j
    u = synth_rnd_np(seed, 2, i)
    start = (u >> np.uint64(1)) % np.uint64(genome_len - read_len + 1)
    rev = (u & np.uint64(1)).astype(bool)
    pos = np.where(rev, start + np.uint64(read_len - 1) - j, start + j)
    code = synth_genome_np(seed, pos, profile)
    code = np.where(rev, code ^ 2, code)
    if profile == 1:
        hl = synth_rnd_np(seed, 8, i)
        ul = np.uint64(1) + (hl >> np.uint64(8)) % np.uint64(3)
        lc = ((hl >> (np.uint64(16) + np.uint64(2) * (j % ul))) & np.uint64(3)).astype(np.uint32)
        code = np.where(hl % np.uint64(100) == 0, lc, code)
    v = synth_rnd_np(seed, 3, np.uint64(first_read) * np.uint64(read_len) + g)
    sub = (v % np.uint64(1000000)) < np.uint64(sub_ppm)
    code = np.where(sub, (code + 1 + ((v >> np.uint64(32)) % np.uint64(3)).astype(np.uint32)) & 3, code)
    bases = np.frombuffer(b"ACTG", dtype=np.uint8)[code]
    return bases.copy(), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)


class HostBuffer:
    """page-locked host memory (gkc_host_alloc) as a numpy uint8 array: ``buf.a``; freed with the object"""

    def __init__(self, nbytes):
        self._p = C.c_void_p()
        rc = lib().gkc_host_alloc(C.byref(self._p), int(nbytes))
        if rc != 0 or not self._p.value:
            raise GkcError("gkc_host_alloc(%d) failed (%d)" % (nbytes, rc))
        self.nbytes = int(nbytes)
        self.a = np.ctypeslib.as_array((C.c_uint8 * max(1, self.nbytes)).from_address(self._p.value))[: self.nbytes]

    def __del__(self):
        try:
            if self._p.value:
                lib().gkc_host_free(self._p); self._p = C.c_void_p()
        except Exception:
            pass


class Counter:
    """Host-side handle over one gkc_ctx (one GPU). Mirrors the call protocol of SortingCountAlgorithm::execute
    (reference kmer/impl/SortingCountAlgorithm.cpp:636-781): configure -> per pass: begin, push reads, finish -> fetch."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.gkc_create(device, C.byref(h))
        if rc != 0:
            raise GkcError("gkc_create failed (%d): %s" % (rc, (self.L.gkc_last_error(None) or b"").decode()))
        self.h = h
        self.k = self.m = self.nb_partitions = self.nb_passes = None
        self._keep = []

    def _chk(self, rc):
        if rc != 0:
            raise GkcError("gkc error %d: %s" % (rc, (self.L.gkc_last_error(self.h) or b"").decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.gkc_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, k, m, nb_partitions, repart, nb_passes=1, freq_order=None):
        repart = np.ascontiguousarray(repart, dtype=np.uint16)
        if repart.size != 4 ** m:
            raise GkcError("repart must have 4^m entries")
        fo = None if freq_order is None else np.ascontiguousarray(freq_order, dtype=np.uint32)
        self._chk(self.L.gkc_configure(self.h, k, m, nb_partitions, nb_passes, 0 if fo is None else 1, _p(repart), _p(fo)))
        self.k, self.m, self.nb_partitions, self.nb_passes = k, m, nb_partitions, nb_passes
        self.rec_bytes = 16 if k <= 31 else 32

    def set_solidity(self, amin=1, amax=2147483647, histo_max=10000):
        self._chk(self.L.gkc_set_solidity(self.h, amin, amax, histo_max)); self.histo_max = histo_max

    def set_max_superkmer(self, maxs):
        self._chk(self.L.gkc_set_max_superkmer(self.h, maxs))

    def set_batch_keys(self, max_keys):
        """upper bound on the k-mers of one Stage-B batch (0: the library's plan)"""
        self._chk(self.L.gkc_set_batch_keys(self.h, max_keys))

    def begin_pass(self, p=0):
        self._tips = None                                       # the masks and the alive array of remove_tips go with the results they describe
        self._chk(self.L.gkc_begin_pass(self.h, p))

    def push_reads(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(self.L.gkc_push_reads(self.h, _p(bases), _p(offsets), len(offsets) - 1))

    def push_reads_device(self, d_bases, d_offsets, n_reads, n_bases):
        self._chk(self.L.gkc_push_reads_device(self.h, d_bases, d_offsets, n_reads, n_bases))

    def finish_pass(self):
        self._chk(self.L.gkc_finish_pass(self.h))

    def set_host_sink(self, host_buffer):
        """stream every Stage-B batch's records into ``host_buffer`` (a HostBuffer: page-locked) while Stage B runs; None switches it off"""
        self._sink = host_buffer
        self._chk(self.L.gkc_set_host_sink(self.h, None if host_buffer is None else host_buffer._p, 0 if host_buffer is None else host_buffer.nbytes))

    def set_sink_mode(self, mode):
        """"packed" (default: 0.4x of the bytes on the link, expanded by host threads) | "raw" (plain Count[] by DMA, no host core touches a byte)"""
        self._chk(self.L.gkc_set_sink_mode(self.h, {"packed": 0, "raw": 1}[mode]))

    def finish_pass_async(self):
        self._chk(self.L.gkc_finish_pass_async(self.h))

    def finish_pass_wait(self):
        self._chk(self.L.gkc_finish_pass_wait(self.h))

    def wait_partition(self, pass_, part):
        """-> (uint8 view of the partition's Count records inside the host sink or None, n_solid) once they have landed"""
        p = C.c_void_p(); n = C.c_uint64()
        self._chk(self.L.gkc_wait_partition(self.h, pass_, part, C.byref(p), C.byref(n)))
        if not p.value or not n.value:
            return None, n.value
        off = p.value - self._sink._p.value
        return self._sink.a[off: off + n.value * self.rec_bytes], n.value

    def release_pass(self, p):
        """gives the result buffers of a finished (and drained) pass back"""
        self._chk(self.L.gkc_release_pass(self.h, p))

    def device_memory(self):
        """(usable, total) bytes of HBM"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.gkc_device_memory(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def count(self, bases, offsets):
        """all passes over one host batch"""
        for p in range(self.nb_passes):
            self.begin_pass(p); self.push_reads(bases, offsets); self.finish_pass()

    def partition_info(self, pass_, part):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.gkc_partition_info(self.h, pass_, part, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def partition_records(self, pass_, part, out=None):
        """raw Count records (uint8 view); ``out``: a uint8 array to receive them (e.g. HostBuffer.a: page-locked, DMA at PCIe rate)"""
        ns, _, _ = self.partition_info(pass_, part)
        if out is None:
            out = np.zeros(max(1, ns * self.rec_bytes), np.uint8)
        elif out.nbytes < ns * self.rec_bytes:
            raise GkcError("output buffer too small")
        n = C.c_uint64()
        self._chk(self.L.gkc_partition_counts(self.h, pass_, part, _p(out), ns, C.byref(n)))
        return out[: ns * self.rec_bytes]

    def partition_records_range(self, pass_, part, first, n):
        """records [first, first + n) of the dataset (gkc_partition_counts_range)"""
        out = np.zeros(max(1, n * self.rec_bytes), np.uint8)
        self._chk(self.L.gkc_partition_counts_range(self.h, pass_, part, first, n, _p(out)))
        return out[: n * self.rec_bytes]

    def partition(self, pass_, part):
        """-> (lo uint64[], hi uint64[], abundance int32[])"""
        raw = self.partition_records(pass_, part)
        if self.rec_bytes == 16:
            r = raw.view(np.uint64).reshape(-1, 2)
            return r[:, 0].copy(), np.zeros(len(r), np.uint64), (r[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        r = raw.view(np.uint64).reshape(-1, 4)
        return r[:, 0].copy(), r[:, 1].copy(), (r[:, 2] & np.uint64(0xFFFFFFFF)).astype(np.int32)

    def partition_device(self, pass_, part):
        p = C.c_void_p(); n = C.c_uint64()
        self._chk(self.L.gkc_partition_counts_device(self.h, pass_, part, C.byref(p), C.byref(n)))
        return p.value, n.value

    def count_banks(self, banks, kind="sum", amin=1, amax=2147483647, solid_vec=None, histo_max=10000):
        """counts every bank of ``banks`` — a list of (bases, offsets) — one after another, merges their counts on the device and evaluates the
        solidity kind (what the reference does with an album of banks) -> the evaluated Banks object (bank i = banks[i])"""
        b = Banks(self, len(banks))
        try:
            for i, (bases, offsets) in enumerate(banks):
                self.count(bases, offsets)
                b.add(i)
            b.evaluate(kind, amin, amax, solid_vec, histo_max)
        except Exception:
            b.close()
            raise
        return b

    def all_counts(self):
        out = {}
        for ps in range(self.nb_passes):
            for pt in range(self.nb_partitions):
                lo, hi, ab = self.partition(ps, pt)
                for a, b, c in zip(lo.tolist(), hi.tolist(), ab.tolist()):
                    out[(b << 64) | a] = c
        return out

    def histogram(self):
        hm = getattr(self, "histo_max", 10000)
        h = np.zeros(hm + 1, np.uint64)
        self._chk(self.L.gkc_histogram(self.h, _p(h), hm + 1))
        return h

    def stats(self):
        s = Stats(); self._chk(self.L.gkc_get_stats(self.h, C.byref(s)))
        d = {n: getattr(s, n) for n, _ in Stats._fields_ if n != "reserved"}
        d["pass_nb_sequences"] = int(s.reserved[0]); d["sink_wire_bytes"] = int(s.reserved[1])
        return d

    def timing(self, name):
        ms = C.c_double(); n = C.c_uint64()
        self._chk(self.L.gkc_get_timing(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def partition_superkmers(self, part, cap_bytes=1 << 26):
        out = np.zeros(cap_bytes, np.uint8)
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.gkc_partition_superkmers(self.h, part, _p(out), cap_bytes, C.byref(a), C.byref(b), C.byref(c)))
        return out[: a.value].copy(), b.value, c.value

    # ---- Repartitor sampling
    def sample_minimizers(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nsk = np.zeros(4 ** self.m, np.uint64); nk = np.zeros(4 ** self.m, np.uint64)
        self._chk(self.L.gkc_sample_minimizers(self.h, _p(bases), _p(offsets), len(offsets) - 1, _p(nsk), _p(nk)))
        return nsk, nk

    def sample_exact(self, bases, offsets, max_superkmers):
        """-> (superkmers, kmers, kxmers per minimizer, reads used): SampleRepart restated read by read on the device"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        a = np.zeros(4 ** self.m, np.uint64); b = np.zeros(4 ** self.m, np.uint64); d = np.zeros(4 ** self.m, np.uint64); used = C.c_uint64()
        self._chk(self.L.gkc_sample_exact(self.h, _p(bases), _p(offsets), len(offsets) - 1, max_superkmers, _p(a), _p(b), _p(d), C.byref(used)))
        return a, b, d, used.value

    def count_mmers(self, m, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        cnt = np.zeros(4 ** m, np.uint32)
        self._chk(self.L.gkc_count_mmers(self.h, m, _p(bases), _p(offsets), len(offsets) - 1, _p(cnt)))
        return cnt

    # ---- segments (multi-GPU exchange surface)
    def segment_count(self):
        n = C.c_uint32(); self._chk(self.L.gkc_segment_count(self.h, C.byref(n))); return n.value

    def segment_export(self, seg):
        p = C.c_void_p(); rb = C.c_uint32()
        off = np.zeros(self.nb_partitions + 1, np.uint64); km = np.zeros(self.nb_partitions, np.uint64)
        self._chk(self.L.gkc_segment_export(self.h, seg, C.byref(p), C.byref(rb), _p(off), _p(km)))
        return p.value, rb.value, off, km

    def segment_import(self, d_records, rec_offsets, kmers):
        ro = np.ascontiguousarray(rec_offsets, dtype=np.uint64); km = np.ascontiguousarray(kmers, dtype=np.uint64)
        self._chk(self.L.gkc_segment_import(self.h, d_records, _p(ro), _p(km)))

    def segments_clear(self):
        self._chk(self.L.gkc_segments_clear(self.h))

    # ---- synthetic input + checksums
    def push_fastx(self, text, final=True):
        """FASTA / FASTQ text (bytes) parsed on the device and pushed; returns the number of bytes consumed"""
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        cons = C.c_uint64(0)
        self._chk(self.L.gkc_push_fastx(self.h, _p(buf) if len(buf) else None, len(buf), 1 if final else 0, C.byref(cons)))
        return cons.value

    def fastx_parse(self, text, final=True):
        """device parse of FASTA / FASTQ text -> (bases uint8[], offsets uint64[n+1], consumed); copies text in and results out (tests)"""
        import torch
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        t = torch.from_numpy(buf.copy()).cuda() if len(buf) else torch.empty(0, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        b = C.c_void_p(); o = C.c_void_p(); nr = C.c_uint64(0); nb = C.c_uint64(0); cons = C.c_uint64(0)
        self._chk(self.L.gkc_fastx_parse_device(self.h, t.data_ptr() if len(buf) else None, len(buf), 1 if final else 0,
                                                C.byref(b), C.byref(o), C.byref(nr), C.byref(nb), C.byref(cons)))
        bases = self.device_to_host(b.value, nb.value) if nb.value else np.zeros(0, np.uint8)
        offs = self.device_to_host(o.value, (nr.value + 1) * 8).view(np.uint64)
        self.device_free(b.value); self.device_free(o.value)
        return bases, offs, cons.value

    def synth_reads_device(self, seed, n_reads, read_len, genome_len, sub_ppm, first_read=0, profile=0):
        """profile 1 = GKC_SYNTH_SKEWED: repeat families in the genome + 1 % low-complexity reads (include/gkc.h)"""
        b = C.c_void_p(); o = C.c_void_p()
        self._chk(self.L.gkc_synth_reads_profile_device(self.h, seed, first_read, n_reads, read_len, genome_len, sub_ppm, profile, C.byref(b), C.byref(o)))
        return b.value, o.value

    def device_free(self, p):
        self._chk(self.L.gkc_device_free(self.h, p))

    def device_to_host(self, d_ptr, nbytes):
        out = np.zeros(nbytes, np.uint8)
        self._chk(self.L.gkc_device_to_host(self.h, _p(out), d_ptr, nbytes))
        return out

    def host_to_device(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.gkc_host_to_device(self.h, d_ptr, _p(arr), arr.nbytes))

    def exchange(self, comm):
        """multi-GPU: route the records pushed since the last exchange of this pass to the owners of their partitions (collective)"""
        self._chk(self.L.gkc_exchange(self.h, comm.h))

    def kmer_checksum_device(self, d_bases, d_offsets, n_reads, n_bases):
        a = C.c_uint64(); b = C.c_uint64()
        self._chk(self.L.gkc_kmer_checksum_device(self.h, d_bases, d_offsets, n_reads, n_bases, C.byref(a), C.byref(b)))
        return a.value, b.value

    def result_checksum(self):
        a = C.c_uint64(); b = C.c_uint64()
        self._chk(self.L.gkc_result_checksum(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- abundance queries against the finished datasets (include/gkc.h, "abundance queries")
    def query_reads(self, bases, offsets):
        """-> int32[n_bases]: per position of the flat buffer the abundance of the k-mer starting there (> 0), 0 = valid k-mer not in the results, -1 = no k-mer"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offsets) < 1 or int(offsets[-1]) > len(bases):
            raise GkcError("the offsets end beyond the bases")
        out = np.zeros(int(offsets[-1]), np.int32)
        self._chk(self.L.gkc_query_reads(self.h, _p(bases), _p(offsets), len(offsets) - 1, _p(out)))
        return out

    def query_reads_device(self, d_bases, d_offsets, n_reads, n_bases, d_out):
        """the same where the reads lie: device pointers, d_bases and d_out 16-byte aligned, d_out int32[n_bases]"""
        self._chk(self.L.gkc_query_reads_device(self.h, d_bases, d_offsets, n_reads, n_bases, d_out))

    def _query_keys(self, keys):
        """keys: ints, a uint64 array (k <= 31), a uint64[n][2] array of (low, high) words (k <= 63), or raw Count records (the uint8 view of
        partition_records) -> (array, n, stride in bytes)"""
        kb = 8 if self.k <= 31 else 16
        if isinstance(keys, np.ndarray) and keys.dtype == np.uint8:
            a = np.ascontiguousarray(keys)
            if a.nbytes % self.rec_bytes:
                raise GkcError("a uint8 key array holds whole Count records of %d bytes" % self.rec_bytes)
            return a, a.nbytes // self.rec_bytes, self.rec_bytes
        if isinstance(keys, np.ndarray) and keys.dtype == np.uint64:
            a = np.ascontiguousarray(keys)
            if a.nbytes % kb:
                raise GkcError("a uint64 key array holds %d words per key" % (kb // 8))
            return a, a.nbytes // kb, kb
        ks = [int(x) for x in keys]
        if kb == 8:
            a = np.array([x & M64 if x >> 64 == 0 else M64 for x in ks], dtype=np.uint64)      # (a value beyond 64 bits is no k-mer for k <= 31: all ones is refused too)
            return a, len(ks), 8
        a = np.zeros((len(ks), 2), np.uint64)
        a[:, 0] = [x & M64 for x in ks]; a[:, 1] = [(x >> 64) & M64 for x in ks]
        return a, len(ks), 16

    def query_kmers(self, keys):
        """-> int32[n]: the abundance of min(key, revcomp(key)) in the results, or 0 (keys: see _query_keys)"""
        a, n, stride = self._query_keys(keys)
        out = np.zeros(n, np.int32)
        self._chk(self.L.gkc_query_kmers(self.h, _p(a) if n else None, n, stride, _p(out) if n else None))
        return out

    def query_kmers_device(self, d_keys, n, stride, d_out):
        self._chk(self.L.gkc_query_kmers_device(self.h, d_keys, n, stride, d_out))

    def query_read_summary_device(self, d_abund, d_offsets, n_reads, d_out):
        """d_out: gkc_read_abundance[n_reads] (24 bytes each) on the device"""
        self._chk(self.L.gkc_query_read_summary_device(self.h, d_abund, d_offsets, n_reads, d_out))

    def query_read_summary(self, abund, offsets):
        """per read of an abundance array made by query_reads with the same offsets -> records of READ_ABUNDANCE (n_valid, n_found, min, max, sum)"""
        import torch
        abund = np.ascontiguousarray(abund, dtype=np.int32); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if n <= 0:
            return np.zeros(0, READ_ABUNDANCE)
        if int(offsets[-1]) > len(abund):
            raise GkcError("the offsets end beyond the abundance array")
        ta = torch.from_numpy(abund.view(np.uint8).copy()).cuda() if len(abund) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        to = torch.from_numpy(offsets.view(np.uint8).copy()).cuda()
        tr = torch.zeros(n * READ_ABUNDANCE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.query_read_summary_device(ta.data_ptr(), to.data_ptr(), n, tr.data_ptr())
        return tr.cpu().numpy().view(READ_ABUNDANCE).copy()

    # ---- graph neighbourhoods of the solid k-mers (include/gkc.h, "graph neighbourhoods")
    def neighbor_masks(self, d_out=None):
        """one byte per solid k-mer, dataset order: bits 0-3 the solid right extensions, bits 4-7 the solid left extensions (A, C, T, G) -> uint8[n_solid] on the
        host, or, with ``d_out`` (a device pointer to >= n_solid bytes), written there and n_solid returned"""
        n = C.c_uint64()
        if d_out is not None:
            self._chk(self.L.gkc_graph_neighbors_solid(self.h, d_out, C.byref(n)))
            return n.value
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
        return self._masks_to_host(n.value, lambda p: self.L.gkc_graph_neighbors_solid(self.h, p, C.byref(n)))

    def neighbor_masks_partition(self, pass_, part):
        """the masks of one dataset -> uint8[n_solid of the dataset]"""
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_neighbors_partition(self.h, pass_, part, None, C.byref(n)))
        return self._masks_to_host(n.value, lambda p: self.L.gkc_graph_neighbors_partition(self.h, pass_, part, p, C.byref(n)))

    def _masks_to_host(self, n, call):
        import torch
        if not n:
            return np.zeros(0, np.uint8)
        t = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self._chk(call(t.data_ptr()))
        return t.cpu().numpy()

    def branching_nodes(self, sort=True, d_masks=None):
        """the solid k-mers that do not have exactly one solid predecessor and one solid successor -> (lo uint64[], hi uint64[], abundance int32[]) like partition().
        sort=True: ascending by value, the order of the reference's /branching/nodes (on the host, as the reference sorts); sort=False: dataset order, ascending inside
        a dataset. d_masks: device pointer to the masks neighbor_masks(d_out) wrote (None: computed here, once)"""
        import torch
        keep = None
        if d_masks is None:
            n = C.c_uint64()
            self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
            if n.value:
                keep = torch.zeros(n.value, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                d_masks = keep.data_ptr()
                self._chk(self.L.gkc_graph_neighbors_solid(self.h, d_masks, C.byref(n)))
        nb = C.c_uint64()
        self._chk(self.L.gkc_graph_branching_solid(self.h, d_masks, None, 0, C.byref(nb), None))
        words = self.rec_bytes // 8
        if not nb.value:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32)
        t = torch.zeros(nb.value * self.rec_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_branching_solid(self.h, d_masks, t.data_ptr(), nb.value, C.byref(nb), None))
        r = t.cpu().numpy().view(np.uint64).reshape(-1, words)
        lo = r[:, 0].copy(); hi = r[:, 1].copy() if words == 4 else np.zeros(len(r), np.uint64)
        ab = (r[:, words // 2] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        if sort:
            o = np.lexsort((lo, hi))
            lo, hi, ab = lo[o], hi[o], ab[o]
        return lo, hi, ab

    def graph_topology(self, d_masks=None):
        """-> uint64[5, 5]: [in, out] = solid k-mers with that many solid predecessors / successors"""
        topo = np.zeros(25, np.uint64); nb = C.c_uint64()
        self._chk(self.L.gkc_graph_branching_solid(self.h, d_masks, None, 0, C.byref(nb), _p(topo)))
        return topo.reshape(5, 5)

    # ---- unitigs of the solid k-mers (include/gkc.h, "unitigs")
    def unitigs_build(self, d_masks=None):
        """ranks the solid records into unitigs and keeps the placement in the context -> (n_unitigs, n_bases, n_cycles). d_masks: device pointer to the masks
        neighbor_masks(d_out) wrote (None: computed inside)"""
        nu, nb, nc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._placement_nu = None; self._placement_masks = None      # (the plain build: its masks are those of the results, read_walks computes them when it needs them)
        self._chk(self.L.gkc_graph_unitigs_build(self.h, d_masks, C.byref(nu), C.byref(nb), C.byref(nc)))
        self._placement_nu = nu.value; self._placement_nb = nb.value
        return nu.value, nb.value, nc.value

    def unitigs_device(self, d_masks=None):
        """-> (bases uint8[n_bases] ASCII, offsets int64[n_unitigs + 1], kc int64[n_unitigs]) as torch tensors on the device (the 64-bit values are unsigned in the
        C-ABI and below 2^63 here); bases.data_ptr() / offsets.data_ptr() are the arguments of push_reads_device / query_reads_device"""
        import torch
        nu, nb, _ = self.unitigs_build(d_masks)
        bases = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
        offsets = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); kc = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_unitigs_write(self.h, bases.data_ptr(), nb, offsets.data_ptr(), nu, kc.data_ptr()))
        return bases[:nb], offsets, kc[:nu]

    def unitigs(self, d_masks=None):
        """-> (bases uint8[n_bases], offsets uint64[n_unitigs + 1], kc uint64[n_unitigs]) as numpy: unitig u is bases[offsets[u]: offsets[u + 1]], kc[u] the sum of
        its k-mers' abundances; numbered by ascending start record"""
        b, o, kc = self.unitigs_device(d_masks)
        return b.cpu().numpy(), o.cpu().numpy().view(np.uint64), kc.cpu().numpy().view(np.uint64)

    def unitig_of_records(self):
        """per solid record, dataset order, from the placement of the last unitigs_build / unitigs / remove_tips -> (unitig index uint64[n], reversed bool[n],
        pos uint32[n]); a dead record of the placement remove_tips left: unitig 2^64 - 1, not reversed, pos 0"""
        import torch
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
        u = torch.zeros(max(n.value, 1), dtype=torch.int64, device="cuda"); p = torch.zeros(max(n.value, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_unitigs_nodes(self.h, u.data_ptr(), p.data_ptr()))
        u = u[: n.value].cpu().numpy().view(np.uint64)
        dead = u == np.uint64(M64)
        return np.where(dead, np.uint64(M64), u >> np.uint64(1)), ((u & np.uint64(1)) != 0) & ~dead, p[: n.value].cpu().numpy().view(np.uint32)

    # ---- read paths (include/gkc.h, "read paths")
    def read_nodes_device(self, d_bases, d_offsets, n_reads, n_bases, d_node, d_pos=None):
        """where the reads lie: device pointers, d_bases, d_node and d_pos 16-byte aligned. d_node uint64[n_bases]: unitig << 1 | strand of the k-mer that starts at
        each position, in the placement the context holds (unitigs_build, remove_tips, simplify), or NODE_REMOVED / NODE_ABSENT / NODE_NO_KMER; d_pos uint32[n_bases]
        (or None): its position in the unitig"""
        self._chk(self.L.gkc_graph_reads_nodes_device(self.h, d_bases, d_offsets, n_reads, n_bases, d_node, d_pos))

    def read_segments_device(self, d_node, d_pos, d_offsets, n_reads, n_bases, d_seg_offsets=None, d_segments=None, cap_segments=0, d_support=None):
        """the maximal runs of consecutive unitig positions inside each read, from what read_nodes_device wrote for the same offsets -> n_segments. d_seg_offsets
        uint64[n_reads + 1] and d_segments READ_SEGMENT[cap_segments] both None: the count only. d_support: uint64[n_unitigs] or None"""
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_reads_segments_device(self.h, d_node, d_pos, d_offsets, n_reads, n_bases, d_seg_offsets, d_segments, cap_segments, C.byref(n), d_support))
        return n.value

    def _reads_to_device(self, bases, offsets):
        """-> (bases tensor, offsets tensor, n_reads, n_bases); the bases padded so that an empty buffer still has an address"""
        import torch
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offsets) < 1 or int(offsets[-1]) > len(bases):
            raise GkcError("the offsets end beyond the bases")
        nb = int(offsets[-1])
        tb = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
        if nb:
            tb[:nb] = torch.from_numpy(bases[:nb].copy()).cuda()
        to = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
        return tb, to, len(offsets) - 1, nb

    def _read_nodes_tensors(self, bases, offsets):
        import torch
        tb, to, nr, nb = self._reads_to_device(bases, offsets)
        node = torch.zeros(max(nb, 2), dtype=torch.int64, device="cuda"); pos = torch.zeros(max(nb, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.read_nodes_device(tb.data_ptr(), to.data_ptr(), nr, nb, node.data_ptr(), pos.data_ptr())
        return to, nr, nb, node, pos

    def read_nodes(self, bases, offsets):
        """per position of the flat buffer, for the k-mer that starts there -> (unitig uint64[n_bases], strand bool[n_bases], pos uint32[n_bases], status uint8[n_bases]).
        status 0: mapped — the k-mer as the read spells it is bases [pos, pos + k) of that unitig (strand False) or their reverse complement (strand True); 1: removed
        (in the results, but of no unitig of the placement remove_tips / simplify left); 2: absent (a valid k-mer that is not in the results); 3: no k-mer starts
        here. unitig is 2^64 - 1, strand False and pos 0 wherever status != 0."""
        _, _, nb, node, pos = self._read_nodes_tensors(bases, offsets)
        v = node[:nb].cpu().numpy().view(np.uint64)
        status = np.zeros(nb, np.uint8)
        status[v == np.uint64(NODE_REMOVED)] = 1; status[v == np.uint64(NODE_ABSENT)] = 2; status[v == np.uint64(NODE_NO_KMER)] = 3
        mapped = status == 0
        return (np.where(mapped, v >> np.uint64(1), np.uint64(M64)), ((v & np.uint64(1)) != 0) & mapped, pos[:nb].cpu().numpy().view(np.uint32), status)

    def read_segments(self, bases, offsets, support=True):
        """the unitigs every read spells -> (seg_offsets uint64[n_reads + 1], segments as a numpy record array of dtype READ_SEGMENT, support uint64[n_unitigs] or
        None). Read r has segments[seg_offsets[r]: seg_offsets[r + 1]], ascending read_pos: node = unitig << 1 | strand, read_pos = the offset of the segment's first
        k-mer inside the read, unitig_pos = that k-mer's position in the unitig, n_kmers consecutive positions (descending on strand 1). support[u] = the k-mers of
        all reads that lie on unitig u. The nodes call, the sizing call and the fill, all on the device."""
        import torch
        to, nr, nb, node, pos = self._read_nodes_tensors(bases, offsets)
        ns = self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb)
        so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(max(ns, 1) * READ_SEGMENT.itemsize, dtype=torch.uint8, device="cuda")
        sup = None
        if support:
            # unitigs of the placement this object built last (unitigs_build, remove_tips, simplify set it). The nodes call above has just answered from the context's
            # placement and fails after a recount, so a count that outlived its results never sizes the array
            nu = getattr(self, "_placement_nu", None)
            if nu is None:
                raise GkcError("the placement in the context was not built through this object (unitigs_build, remove_tips or simplify first)")
            sup = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        got = self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns, sup.data_ptr() if support else None)
        if got != ns:
            raise GkcError("the fill found %d segments, the sizing call %d" % (got, ns))
        return (so.cpu().numpy().view(np.uint64), seg.cpu().numpy()[: ns * READ_SEGMENT.itemsize].view(READ_SEGMENT).copy(),
                sup[:nu].cpu().numpy().view(np.uint64) if support else None)

    def read_walks_device(self, d_seg_offsets, d_segments, n_reads, n_segments, d_link_offsets, d_links, n_links, d_junction=None, d_walk_offsets=None, d_walks=None,
                          cap_walks=0, d_link_support=None):
        """the segments of every read joined across the links of the compacted graph, from what read_segments_device and gkc_graph_unitigs_links wrote for the placement
        the context holds -> n_walks. d_walk_offsets uint64[n_reads + 1] and d_walks READ_WALK[cap_walks] both None: the count only. d_junction: uint64[n_segments] or
        None; d_link_support: uint64[n_links] or None"""
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_reads_walks_device(self.h, d_seg_offsets, d_segments, n_reads, n_segments, d_link_offsets, d_links, n_links, d_junction, d_walk_offsets, d_walks,
                                                      cap_walks, C.byref(n), d_link_support))
        return n.value

    def read_walks(self, bases, offsets, link_support=True):
        """the paths in the compacted graph every read spells -> dict: seg_offsets, segments (as read_segments gives them), junction uint64[n_segments] (per segment its
        relation to the next segment of the same read: the index into links of the link it follows, or JUNCTION_END / BREAK / COLLINEAR / UNLINKED), walk_offsets
        uint64[n_reads + 1], walks (numpy record array of dtype READ_WALK: first_segment, n_segments, n_kmers — a maximal chain of segments joined by links; it spells
        n_kmers + k - 1 bases of the read from its first segment's read_pos), link_offsets, links (as unitig_links gives them, of the placement this object built last:
        unitigs_build, remove_tips or simplify), link_support uint64[n_links] or None: the reads crossing every link entry, raw (the other direction counts on the mirror
        entry). The nodes call, the segments calls, the link calls and the walks calls, all on the device."""
        import torch
        to, nr, nb, node, pos = self._read_nodes_tensors(bases, offsets)
        nu = getattr(self, "_placement_nu", None)
        if nu is None:
            raise GkcError("the placement in the context was not built through this object (unitigs_build, remove_tips or simplify first)")
        ns = self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb)
        so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(max(ns, 1) * READ_SEGMENT.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns) != ns:
            raise GkcError("the fill found another number of segments than the sizing call")
        # the masks the placement was built from: those remove_tips / simplify left, or the plain ones (computed once for the two link calls)
        masks = getattr(self, "_placement_masks", None)
        keep, d_masks = self._masks_once(None if masks is None else masks.data_ptr())
        lo, links = self._unitig_links_of_placement(nu, d_masks)
        nl = len(links)
        args = (so.data_ptr(), seg.data_ptr(), nr, ns, lo.data_ptr(), links.data_ptr(), nl)
        nw = self.read_walks_device(*args)
        jn = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda"); wo = torch.zeros(nr + 1, dtype=torch.int64, device="cuda")
        wk = torch.zeros(max(nw, 1) * READ_WALK.itemsize, dtype=torch.uint8, device="cuda")
        sup = torch.zeros(max(nl, 1), dtype=torch.int64, device="cuda") if link_support else None
        torch.cuda.synchronize()
        if self.read_walks_device(*args, jn.data_ptr(), wo.data_ptr(), wk.data_ptr(), nw, sup.data_ptr() if link_support else None) != nw:
            raise GkcError("the fill found another number of walks than the sizing call")
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        return dict(seg_offsets=u64(so), segments=seg.cpu().numpy()[: ns * READ_SEGMENT.itemsize].view(READ_SEGMENT).copy(), junction=u64(jn[:ns]), walk_offsets=u64(wo),
                    walks=wk.cpu().numpy()[: nw * READ_WALK.itemsize].view(READ_WALK).copy(), link_offsets=u64(lo), links=u64(links),
                    link_support=u64(sup[:nl]) if link_support else None)

    def correct_reads_device(self, d_bases, d_offsets, n_reads, n_bases, d_seg_offsets, d_segments, n_segments, d_unitig_bases, d_unitig_offsets, d_out,
                             max_subst=2, ends=True, d_n_changed=None, d_changed_bits=None, params=None):
        """the reads rewritten to what the graph says (gkc_graph_reads_correct_device): device pointers, the segments read_segments_device wrote for these reads and the
        unitig strings gkc_graph_unitigs_write wrote for the placement the context holds. d_out uint8[n_bases] (d_out == d_bases: in place), d_n_changed uint32[n_reads]
        or None, d_changed_bits uint64[(n_bases + 63) // 64] or None; params: a CorrectParams, None with max_subst = ends = None for the library's default -> the stats
        as a dict"""
        if params is None and max_subst is not None:
            params = CorrectParams(max_subst, 1 if ends else 0)
        st = CorrectStats()
        self._chk(self.L.gkc_graph_reads_correct_device(self.h, d_bases, d_offsets, n_reads, n_bases, d_seg_offsets, d_segments, n_segments, d_unitig_bases, d_unitig_offsets,
                                                        None if params is None else C.byref(params), d_out, d_n_changed, d_changed_bits, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in CorrectStats._fields_}

    def correct_reads(self, bases, offsets, max_subst=2, ends=True):
        """the reads corrected against the placement this object built last (unitigs_build, remove_tips or simplify) -> dict: bases uint8[n_bases] (same offsets: only
        substitutions), n_changed uint32[n_reads], changed bool[n_bases], stats (gaps_fixed, gaps_skipped, heads_fixed, tails_fixed, ends_skipped, ends_no_room,
        bases_changed), seg_offsets and segments of the INPUT reads (as read_segments gives them). A stretch between two segments that continue each other along one
        unitig, and a read's ends in front of its first / behind its last segment, become the unitig's bases when at most max_subst of them differ. The nodes call, the
        segments calls, the unitig strings and the correction, all on the device."""
        import torch
        tb, to, nr, nb = self._reads_to_device(bases, offsets)
        node = torch.zeros(max(nb, 2), dtype=torch.int64, device="cuda"); pos = torch.zeros(max(nb, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.read_nodes_device(tb.data_ptr(), to.data_ptr(), nr, nb, node.data_ptr(), pos.data_ptr())
        nu = getattr(self, "_placement_nu", None)
        if nu is None:
            raise GkcError("the placement in the context was not built through this object (unitigs_build, remove_tips or simplify first)")
        nub = self._placement_nb
        ns = self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb)
        so = torch.zeros(nr + 1, dtype=torch.int64, device="cuda"); seg = torch.zeros(max(ns, 1) * READ_SEGMENT.itemsize, dtype=torch.uint8, device="cuda")
        ub = torch.zeros(max(nub, 16), dtype=torch.uint8, device="cuda"); uo = torch.zeros(nu + 1, dtype=torch.int64, device="cuda")
        out = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda"); nch = torch.zeros(max(nr, 1), dtype=torch.int32, device="cuda")
        bits = torch.zeros((nb + 63) // 64 + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if self.read_segments_device(node.data_ptr(), pos.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns) != ns:
            raise GkcError("the fill found another number of segments than the sizing call")
        self._chk(self.L.gkc_graph_unitigs_write(self.h, ub.data_ptr(), nub, uo.data_ptr(), nu, None))
        stats = self.correct_reads_device(tb.data_ptr(), to.data_ptr(), nr, nb, so.data_ptr(), seg.data_ptr(), ns, ub.data_ptr(), uo.data_ptr(), out.data_ptr(), max_subst, ends,
                                          nch.data_ptr(), bits.data_ptr())
        changed = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nb].astype(bool)
        return dict(bases=out[:nb].cpu().numpy(), n_changed=nch[:nr].cpu().numpy().view(np.uint32), changed=changed, stats=stats,
                    seg_offsets=so.cpu().numpy().view(np.uint64), segments=seg.cpu().numpy()[: ns * READ_SEGMENT.itemsize].view(READ_SEGMENT).copy())

    # ---- links between the unitigs (include/gkc.h, "unitigs": side, slot, entry)
    def unitig_links_device(self, d_masks=None):
        """the edges of the compacted graph as a CSR over the 2 n_unitigs sides -> (link_offsets int64[2 n_unitigs + 1], links int64[n_links]) as torch tensors on
        the device: slot 2 u + side (side 0: '+', the end of unitig u; side 1: '-', its begin) holds links[link_offsets[t]: link_offsets[t + 1]], ascending, each
        v << 1 | (0: one arrives at the begin of v, "v:+"; 1: at its end, "v:-"). Builds the placement first, like unitigs_device."""
        keep, d_masks = self._masks_once(d_masks)
        nu, _, _ = self.unitigs_build(d_masks)
        return self._unitig_links_of_placement(nu, d_masks)

    def _masks_once(self, d_masks):
        """the masks for a build and the link calls behind it, computed once when none are given -> (the tensor that owns them or None, device pointer or None)"""
        import torch
        if d_masks is not None:
            return None, d_masks
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
        if not n.value:
            return None, None
        keep = torch.zeros(n.value, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, keep.data_ptr(), C.byref(n)))
        return keep, keep.data_ptr()

    def _unitig_links_of_placement(self, nu, d_masks):
        import torch
        nl = C.c_uint64()
        self._chk(self.L.gkc_graph_unitigs_links(self.h, d_masks, None, 0, None, 0, C.byref(nl)))
        offsets = torch.zeros(2 * nu + 1, dtype=torch.int64, device="cuda"); links = torch.zeros(max(nl.value, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_unitigs_links(self.h, d_masks, offsets.data_ptr(), nu, links.data_ptr(), nl.value, C.byref(nl)))
        return offsets, links[: nl.value]

    # ---- tips (include/gkc.h, "tips")
    def remove_tips(self, max_len_topo=None, max_len_rc=None, rc_ratio=(2, 1), max_rounds=20):
        """removes the tips of the compacted graph round by round (gkc_graph_tips_remove) and leaves the simplified graph as the context's placement. Defaults: the
        reference's constants, max_len_topo = 5 k // 2 bases, max_len_rc = 10 k bases, ratio 2 / 1; 0 switches a rule off. -> dict: alive bool[n_solid], rounds,
        tips_per_round (list), records_removed, n_unitigs, n_bases, n_cycles. The device masks and alive array stay on the object until the next count
        (simplified_unitigs, write_unitigs_fasta(simplified=True) read them)."""
        import torch
        k = self.k
        prm = TipParams((5 * k) // 2 if max_len_topo is None else max_len_topo, 10 * k if max_len_rc is None else max_len_rc, rc_ratio[0], rc_ratio[1], max_rounds)
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
        masks = torch.zeros(max(n.value, 16), dtype=torch.uint8, device="cuda"); alive = torch.zeros(max(n.value, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if n.value:
            self._chk(self.L.gkc_graph_neighbors_solid(self.h, masks.data_ptr(), C.byref(n)))
        per_round = np.zeros(max(1, min(max_rounds, 64)), np.uint64)
        nr, rem, nu, nb, nc = (C.c_uint64() for _ in range(5))
        self._tips = None; self._placement_nu = None; self._placement_masks = None
        self._chk(self.L.gkc_graph_tips_remove(self.h, masks.data_ptr(), alive.data_ptr(), C.byref(prm), C.byref(nr), _p(per_round), C.byref(rem), C.byref(nu), C.byref(nb), C.byref(nc)))
        self._placement_nu = nu.value; self._placement_nb = nb.value; self._placement_masks = masks
        self._tips = dict(masks=masks, alive=alive, n=n.value, n_unitigs=nu.value, n_bases=nb.value)
        return dict(alive=alive[: n.value].cpu().numpy().astype(bool), rounds=nr.value, tips_per_round=[int(x) for x in per_round[: nr.value]], records_removed=rem.value,
                    n_unitigs=nu.value, n_bases=nb.value, n_cycles=nc.value)

    # ---- simplify (include/gkc.h, "simplify")
    def simplify_params(self, max_len_topo=None, max_len_rc=None, rc_ratio=(2, 1), tip_rounds=20, bulge_max_len=None, bulge_alt=(11, 10, 3), bulge_rounds=20,
                        ec_max_len=None, ec_ratio=(4, 1), ec_rounds=20, max_sweeps=10, resume=False):
        """-> SimplifyParams with the reference's constants where an argument is None: tips as remove_tips, bulge_max_len = max(3 k, k + 100) bases, alternative up to
        max(11 / 10 L, L + 3) records, ec_max_len = 9 k bases, ratio 4 / 1; 20 rounds per phase, 10 sweeps"""
        k = self.k
        tips = TipParams((5 * k) // 2 if max_len_topo is None else max_len_topo, 10 * k if max_len_rc is None else max_len_rc, rc_ratio[0], rc_ratio[1], tip_rounds)
        return SimplifyParams(tips, max(3 * k, k + 100) if bulge_max_len is None else bulge_max_len, bulge_alt[0], bulge_alt[1], bulge_alt[2], bulge_rounds,
                              9 * k if ec_max_len is None else ec_max_len, ec_ratio[0], ec_ratio[1], ec_rounds, max_sweeps, 1 if resume else 0)

    def simplify(self, params=None, **kw):
        """tips, bulges and erroneous connections of the compacted graph removed on the device (gkc_graph_simplify): phase(tips), then sweeps of phase(bulges),
        phase(ec), phase(tips) until a sweep removes nothing, and the simplified graph left as the context's placement. ``params``: a SimplifyParams, or the keyword
        arguments of simplify_params. With resume the state an earlier remove_tips / simplify left on this object is continued, otherwise every record starts alive.
        -> dict: alive bool[n_solid], rounds, records_removed (of this call), n_unitigs, n_bases, n_cycles, log: a list of (kind name, sweep, n_unitigs, n_hits,
        n_records_removed) per round. The device masks and alive array stay on the object until the next count, as after remove_tips."""
        import torch
        prm = params if params is not None else self.simplify_params(**kw)
        n = C.c_uint64()
        self._chk(self.L.gkc_graph_neighbors_solid(self.h, None, C.byref(n)))
        if prm.resume:
            t = self._tips_state()
            masks, alive = t["masks"], t["alive"]
        else:
            masks = torch.zeros(max(n.value, 16), dtype=torch.uint8, device="cuda"); alive = torch.zeros(max(n.value, 16), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if n.value:
                self._chk(self.L.gkc_graph_neighbors_solid(self.h, masks.data_ptr(), C.byref(n)))
        log = (SimplifyRound * SIMPLIFY_LOG_CAP)()
        nr, rem, nu, nb, nc = (C.c_uint64() for _ in range(5))
        self._tips = None; self._placement_nu = None; self._placement_masks = None
        self._chk(self.L.gkc_graph_simplify(self.h, masks.data_ptr(), alive.data_ptr(), C.byref(prm), log, SIMPLIFY_LOG_CAP, C.byref(nr), C.byref(rem), C.byref(nu), C.byref(nb),
                                            C.byref(nc)))
        self._placement_nu = nu.value; self._placement_nb = nb.value; self._placement_masks = masks
        self._tips = dict(masks=masks, alive=alive, n=n.value, n_unitigs=nu.value, n_bases=nb.value)
        return dict(alive=alive[: n.value].cpu().numpy().astype(bool), rounds=nr.value, records_removed=rem.value, n_unitigs=nu.value, n_bases=nb.value, n_cycles=nc.value,
                    log=[(SIMPLIFY_KINDS[e.kind], int(e.sweep), int(e.n_unitigs), int(e.n_hits), int(e.n_records_removed)) for e in log[: min(nr.value, SIMPLIFY_LOG_CAP)]])

    def remove_bulges(self, bulge_max_len=None, bulge_alt=(11, 10, 3), max_rounds=20, resume=False):
        """the bulges alone: simplify with no tip and no EC rounds, i.e. one phase(bulges) and the empty sweep after it"""
        return self.simplify(tip_rounds=0, ec_rounds=0, bulge_max_len=bulge_max_len, bulge_alt=bulge_alt, bulge_rounds=max_rounds, resume=resume)

    def remove_erroneous_connections(self, ec_max_len=None, ec_ratio=(4, 1), max_rounds=20, resume=False):
        """the erroneous connections alone: simplify with no tip and no bulge rounds"""
        return self.simplify(tip_rounds=0, bulge_rounds=0, ec_max_len=ec_max_len, ec_ratio=ec_ratio, ec_rounds=max_rounds, resume=resume)

    def simplified_masks(self):
        """-> uint8[n_solid]: the neighbour masks of the graph remove_tips / simplify left (0 for dead records)"""
        t = self._tips_state()
        return t["masks"][: t["n"]].cpu().numpy()

    def _tips_state(self):
        t = getattr(self, "_tips", None)
        if t is None:
            raise GkcError("remove_tips or simplify must be called first (after the last count)")
        return t

    def simplified_unitigs(self):
        """the graph remove_tips left -> (bases uint8[n_bases], offsets uint64[n_unitigs + 1], kc uint64[n_unitigs], link_offsets uint64[2 n_unitigs + 1],
        links uint64[n_links]) as numpy, in the layouts of unitigs() and unitig_links(). The placement in the context must still be the one remove_tips left
        (unitigs_build and the methods over it replace it: call remove_tips again)."""
        import torch
        t = self._tips_state()
        nu, nb = t["n_unitigs"], t["n_bases"]
        bases = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
        offsets = torch.zeros(nu + 1, dtype=torch.int64, device="cuda"); kc = torch.zeros(max(nu, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self._chk(self.L.gkc_graph_unitigs_write(self.h, bases.data_ptr(), nb, offsets.data_ptr(), nu, kc.data_ptr()))
        lo, links = self._unitig_links_of_placement(nu, t["masks"].data_ptr())
        if int(offsets[-1]) != nb:
            raise GkcError("the placement in the context is not the one remove_tips left (call remove_tips again)")
        return (bases[:nb].cpu().numpy(), offsets.cpu().numpy().view(np.uint64), kc[:nu].cpu().numpy().view(np.uint64), lo.cpu().numpy().view(np.uint64),
                links.cpu().numpy().view(np.uint64))

    def unitig_links(self, d_masks=None):
        """-> (link_offsets uint64[2 n_unitigs + 1], links uint64[n_links]) as numpy, see unitig_links_device"""
        o, l = self.unitig_links_device(d_masks)
        return o.cpu().numpy().view(np.uint64), l.cpu().numpy().view(np.uint64)

    def write_unitigs_fasta(self, path, d_masks=None, simplified=False):
        """the unitigs with their links in the layout of bcalm2 that the reference's GraphUnitigs::load_unitigs parses: per unitig
        ">u LN:i:<bases> KC:i:<kc> km:f:<kc / records, one decimal>  L:+:v:+- ... L:-:v:+- ..." (the '+' side's links first, each side in slot order), the sequence on
        the next line. Host code over unitigs() and unitig_links(), or, with ``simplified``, over simplified_unitigs(): the graph remove_tips left
        -> (n_unitigs, n_links)"""
        if simplified:
            bases, offs, kc, lo, links = self.simplified_unitigs()
        else:
            keep, d_masks = self._masks_once(d_masks)
            bases, offs, kc = self.unitigs(d_masks)
            lo, links = (t.cpu().numpy().view(np.uint64) for t in self._unitig_links_of_placement(len(kc), d_masks))
        k = self.k
        text = bases.tobytes().decode()
        with open(path, "w") as f:
            for u in range(len(kc)):
                b0, b1 = int(offs[u]), int(offs[u + 1])
                fields = ["%d" % u, "LN:i:%d" % (b1 - b0), "KC:i:%d" % int(kc[u]), "km:f:%.1f" % (int(kc[u]) / (b1 - b0 - k + 1))]
                for side, sign in ((0, "+"), (1, "-")):
                    for e in links[int(lo[2 * u + side]): int(lo[2 * u + side + 1])]:
                        fields.append("L:%s:%d:%s" % (sign, int(e) >> 1, "-" if int(e) & 1 else "+"))
                f.write(">" + " ".join(fields) + "\n" + text[b0:b1] + "\n")
        return len(kc), len(links)

    def write_gfa(self, path, simplified=False, reads=None):
        """the compacted graph as GFA 1 (gfa_text): the unitigs and links of unitigs() and unitig_links(), or, with ``simplified``, of simplified_unitigs(). reads =
        (bases, offsets): a P line named r<read>_<walk> for every walk of read_walks that has at least two segments -> (n_unitigs, n_links, n_paths)"""
        if simplified:
            bases, offs, kc, lo, links = self.simplified_unitigs()
        else:
            keep, d_masks = self._masks_once(None)
            bases, offs, kc = self.unitigs(d_masks)
            lo, links = (t.cpu().numpy().view(np.uint64) for t in self._unitig_links_of_placement(len(kc), d_masks))
        text = bases.tobytes().decode()
        seqs = [text[int(offs[u]): int(offs[u + 1])] for u in range(len(kc))]
        paths = None
        if reads is not None:
            w = self.read_walks(reads[0], reads[1], link_support=False)
            paths = []
            for r in range(len(w["walk_offsets"]) - 1):
                for i, x in enumerate(w["walks"][int(w["walk_offsets"][r]): int(w["walk_offsets"][r + 1])]):
                    if x["n_segments"] >= 2:
                        s0 = int(x["first_segment"])
                        paths.append(("r%d_%d" % (r, i), [int(v) for v in w["segments"]["node"][s0: s0 + int(x["n_segments"])]]))
        with open(path, "w") as f:
            f.write(gfa_text(self.k, seqs, kc, lo, links, paths))
        return len(kc), len(links), 0 if paths is None else len(paths)


def write_corrected_fasta(path, bases, offsets, names=None):
    """the reads of a flat buffer (correct_reads(...)["bases"] with the offsets of the input) as FASTA, one record per read: ">" + names[r] (None: the read's number) and
    the sequence on one line. Host code -> the number of reads"""
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    offs = [int(x) for x in offsets]
    if names is not None and len(names) != len(offs) - 1:
        raise GkcError("%d names for %d reads" % (len(names), len(offs) - 1))
    with open(path, "wb") as f:
        for r in range(len(offs) - 1):
            name = ("%d" % r) if names is None else names[r]
            f.write(b">" + (name if isinstance(name, bytes) else str(name).encode()) + b"\n" + raw[offs[r]: offs[r + 1]] + b"\n")
    return len(offs) - 1


def gfa_text(k, seqs, kc, link_offsets, links, walks=None):
    """unitigs, links and read walks as GFA 1 -> str. Pure host code over arrays: seqs the unitig sequences (str or bytes), kc their abundance sums, link_offsets /
    links the CSR of unitig_links() (slot 2 u + side holds entries v << 1 | mv). "H VN:Z:1.0"; per unitig "S <u> <sequence> KC:i:<kc[u]>"; per link entry
    "L <u> <+|-> <v> <+|-> <k-1>M", the from-orientation + for side 0 (one leaves through the end of u) and - for side 1, the to-orientation + for mv = 0 (one arrives at
    the begin of v) and - for mv = 1; walks: an iterable of (name, [node, ...]), node = unitig << 1 | strand, each "P <name> <u+|u-,...> *". Fields are tab-separated."""
    lines = ["H\tVN:Z:1.0"]
    for u, s in enumerate(seqs):
        lines.append("S\t%d\t%s\tKC:i:%d" % (u, s if isinstance(s, str) else bytes(s).decode(), int(kc[u])))
    lo = [int(x) for x in link_offsets]
    for t in range(len(lo) - 1):
        for e in links[lo[t]: lo[t + 1]]:
            lines.append("L\t%d\t%s\t%d\t%s\t%dM" % (t >> 1, "+-"[t & 1], int(e) >> 1, "+-"[int(e) & 1], k - 1))
    for name, nodes in (walks or ()):
        lines.append("P\t%s\t%s\t*" % (name, ",".join("%d%s" % (int(n) >> 1, "+-"[int(n) & 1]) for n in nodes)))
    return "\n".join(lines) + "\n"


def balanced_owner_ranges(weights, world):
    """contiguous partition ranges per rank balanced by weight (pure host function of the library): first[world+1]"""
    w = np.ascontiguousarray(weights, dtype=np.uint64)
    first = np.zeros(world + 1, np.uint32)
    rc = lib().gkc_balanced_owner_ranges(_p(w), len(w), world, _p(first))
    if rc != 0:
        raise GkcError("gkc_balanced_owner_ranges failed (%d)" % rc)
    return first


def exchange_plan(world, rank, first, n_segs, counts):
    """gkc_exchange_plan (pure host): counts uint64[world][l_max][2][P] -> (sends, recvs, recv_total) with (peer, seg, rec_begin, n_recs) tuples"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    l_max, P = counts.shape[1], counts.shape[3]
    first = np.ascontiguousarray(first, dtype=np.uint32); n_segs = np.ascontiguousarray(n_segs, dtype=np.uint64)
    cap = world * max(1, l_max) + 1
    ps = (PlanMsg * cap)(); pr = (PlanMsg * cap)(); a = C.c_uint32(); b = C.c_uint32(); tot = C.c_uint64()
    rc = lib().gkc_exchange_plan(world, rank, P, _p(first), _p(n_segs), l_max, _p(counts), ps, C.byref(a), pr, C.byref(b), C.byref(tot))
    if rc != 0:
        raise GkcError("gkc_exchange_plan failed (%d)" % rc)
    f = lambda arr, n: [(arr[i].peer, arr[i].seg, arr[i].rec_begin, arr[i].n_recs) for i in range(n)]
    return f(ps, a.value), f(pr, b.value), tot.value


class Comm:
    """gkc_comm: one rank of a multi-GPU run. ``Comm.rccl(counter, id_bytes, world, rank)`` or ``Comm.transport(counter, t, world, rank)``
    where ``t`` offers allgather_host(bytes) -> list of bytes and sendrecv_device(sends, recvs) with (peer, device pointer, nbytes) tuples."""

    def __init__(self, counter, h, keep=None):
        self.c = counter; self.L = counter.L; self.h = h; self._keep = keep

    @staticmethod
    def unique_id():
        buf = np.zeros(128, np.uint8)
        if lib().gkc_comm_unique_id(_p(buf)) != 0:
            raise GkcError("ncclGetUniqueId failed")
        return buf.tobytes()

    @classmethod
    def rccl(cls, counter, id_bytes, world, rank):
        h = C.c_void_p(); buf = np.frombuffer(bytes(id_bytes), dtype=np.uint8).copy()
        counter._chk(counter.L.gkc_comm_create_rccl(counter.h, _p(buf), world, rank, C.byref(h)))
        return cls(counter, h)

    @classmethod
    def transport(cls, counter, t, world, rank):
        def _ag(user, mine, n, out):
            try:
                parts = t.allgather_host(C.string_at(mine, n))
                C.memmove(out, b"".join(parts), n * world)
                return 0
            except Exception as e:      # noqa
                import traceback; traceback.print_exc()
                return 1

        def _sr(user, sends, ns, recvs, nr):
            try:
                t.sendrecv_device([(sends[i].peer, sends[i].d_ptr, sends[i].n_bytes) for i in range(ns)],
                                  [(recvs[i].peer, recvs[i].d_ptr, recvs[i].n_bytes) for i in range(nr)])
                return 0
            except Exception as e:      # noqa
                import traceback; traceback.print_exc()
                return 1

        cb1, cb2 = ALLGATHER_CB(_ag), SENDRECV_CB(_sr)
        st = Transport(None, cb1, cb2)
        h = C.c_void_p()
        counter._chk(counter.L.gkc_comm_create_transport(counter.h, C.byref(st), world, rank, C.byref(h)))
        return cls(counter, h, keep=(cb1, cb2, st, t))

    @classmethod
    def files(cls, counter, directory, world, rank):
        """file-mailbox transport inside the library (gkc_comm_create_files): ranks that share nothing but a directory"""
        h = C.c_void_p()
        counter._chk(counter.L.gkc_comm_create_files(counter.h, str(directory).encode(), world, rank, C.byref(h)))
        return cls(counter, h)

    def enable_ipc(self, on=True):
        """device messages of a transport communicator go device to device through IPC memory handles (gkc_comm_enable_ipc)"""
        self.c._chk(self.L.gkc_comm_enable_ipc(self.h, 1 if on else 0))

    def loopback(self, n_bytes):
        """this rank sends n_bytes to itself through the communicator's send / receive path (chunked like gkc_exchange) -> (mismatching words, ms)"""
        bad = C.c_uint64(0); ms = C.c_double(0)
        self.c._chk(self.L.gkc_comm_loopback(self.c.h, self.h, int(n_bytes), C.byref(bad), C.byref(ms)))
        return bad.value, ms.value

    def selftest(self, n_bytes):
        """collective: every rank sends n_bytes of a keyed pattern to every other rank in one grouped exchange and checks what arrives (gkc_comm_selftest);
        raises on every rank when one of them saw garbage -> (mismatching words on this rank, ms)"""
        bad = C.c_uint64(0); ms = C.c_double(0)
        self.c._chk(self.L.gkc_comm_selftest(self.c.h, self.h, int(n_bytes), C.byref(bad), C.byref(ms)))
        return bad.value, ms.value

    def peer_bytes(self, world):
        """-> (bytes sent to every peer, bytes received from every peer, ms ncclCommInitRank took)"""
        a = np.zeros(world, np.uint64); b = np.zeros(world, np.uint64); ms = C.c_double(0)
        self.c._chk(self.L.gkc_comm_peer_bytes(self.h, _p(a), _p(b), C.byref(ms)))
        return a, b, ms.value

    def gather_results(self, root=0):
        """collective after finish_pass: every partition's Count[], the histogram and the statistics on `root` (gkc_gather_results)"""
        self.c._chk(self.L.gkc_gather_results(self.c.h, self.h, root))

    def set_owners(self, first):
        a = None if first is None else np.ascontiguousarray(first, dtype=np.uint32)
        self.c._chk(self.L.gkc_comm_set_owners(self.h, _p(a)))

    def owners(self, world):
        a = np.zeros(world + 1, np.uint32)
        self.c._chk(self.L.gkc_comm_get_owners(self.h, _p(a))); return a

    def stats(self):
        s = CommStats(); self.c._chk(self.L.gkc_comm_get_stats(self.h, C.byref(s)))
        d = {n: getattr(s, n) for n, _ in CommStats._fields_ if n != "reserved"}
        d["ipc_bounced"] = int(s.reserved[0])      # receive buffers of the IPC transport that could not be exported (mapped ranges) and went through a hipMalloc bounce block
        return d

    def close(self):
        if getattr(self, "h", None):
            self.L.gkc_comm_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mphf:
    """BooPHF minimal perfect hash built on the device (include/gkc.h gkc_mphf_*)"""

    def __init__(self, counter, keys=None, k=None, comm=None):
        """keys=None: the solid k-mers of the counter (comm: of all ranks' counters — collective); else a list of ints / uint64 array
        (k <= 31) or list of ints (k <= 63)"""
        self.c = counter; self.L = counter.L; self.comm = comm
        h = C.c_void_p()
        if keys is None and comm is not None:
            counter._chk(self.L.gkc_mphf_build_solid_dist(counter.h, comm.h, C.byref(h))); self.k = counter.k
        elif keys is None:
            counter._chk(self.L.gkc_mphf_build_solid(counter.h, C.byref(h))); self.k = counter.k
        else:
            self.k = k
            a = self._keys(keys)
            counter._chk(self.L.gkc_mphf_build(counter.h, _p(a), len(a), a.strides[0], k, C.byref(h)))
        self.h = h

    def _keys(self, keys):
        if self.k <= 31:
            return np.ascontiguousarray(np.array([int(x) for x in keys], dtype=np.uint64))
        a = np.zeros((len(keys), 2), dtype=np.uint64)
        for i, x in enumerate(keys):
            a[i, 0] = int(x) & 0xFFFFFFFFFFFFFFFF; a[i, 1] = int(x) >> 64
        return a

    @property
    def size(self):
        return self.L.gkc_mphf_size(self.h)

    def lookup(self, keys):
        a = self._keys(keys); out = np.zeros(len(a), np.uint64)
        self.c._chk(self.L.gkc_mphf_lookup(self.h, _p(a), len(a), a.strides[0], _p(out))); return out

    def save(self):
        n = self.L.gkc_mphf_save_size(self.h); out = np.zeros(n, np.uint8)
        self.c._chk(self.L.gkc_mphf_save(self.h, _p(out), n)); return out

    def abundance_map(self):
        out = np.zeros(self.size, np.uint8); above = C.c_uint64(0)
        if self.comm is not None:
            self.c._chk(self.L.gkc_mphf_abundance_map_dist(self.h, self.c.h, self.comm.h, _p(out), len(out), C.byref(above))); return out, above.value
        self.c._chk(self.L.gkc_mphf_abundance_map(self.h, self.c.h, _p(out), len(out), C.byref(above))); return out, above.value

    def close(self):
        if self.h:
            self.L.gkc_mphf_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bloom:
    KINDS = {"basic": 0, "cache": 1, "neighbor": 2}

    def __init__(self, counter, kind, tai_bits, nb_hash, k):
        self.c = counter; self.L = counter.L; self.k = k
        h = C.c_void_p()
        counter._chk(self.L.gkc_bloom_create(counter.h, self.KINDS[kind], tai_bits, nb_hash, k, C.byref(h)))
        self.h = h; self.stride = 8 if k <= 31 else 16

    def _keys(self, keys):
        ks = [int(x) for x in keys]
        if self.stride == 8:
            return np.array(ks, dtype=np.uint64)
        a = np.zeros((len(ks), 2), np.uint64)
        a[:, 0] = [x & M64 for x in ks]; a[:, 1] = [x >> 64 for x in ks]
        return a

    def insert(self, keys):
        a = self._keys(keys); self.c._chk(self.L.gkc_bloom_insert(self.h, _p(a), len(a), self.stride))

    def insert_solid(self):
        self.c._chk(self.L.gkc_bloom_insert_solid(self.h, self.c.h))

    def query_solid(self, neighbors8=True, d_out=None):
        """contains8 (or contains) of every solid k-mer of the counter, on the device (gkc_bloom_query_solid) -> (k-mers queried, set result bits)"""
        nq = C.c_uint64(0); npos = C.c_uint64(0)
        self.c._chk(self.L.gkc_bloom_query_solid(self.h, self.c.h, 1 if neighbors8 else 0, d_out, C.byref(nq), C.byref(npos)))
        return nq.value, npos.value

    def contains(self, keys):
        a = self._keys(keys); out = np.zeros(len(a), np.uint8)
        self.c._chk(self.L.gkc_bloom_contains(self.h, _p(a), len(a), self.stride, _p(out))); return out

    def contains8(self, keys):
        a = self._keys(keys); out = np.zeros(len(a), np.uint8)
        self.c._chk(self.L.gkc_bloom_contains8(self.h, _p(a), len(a), self.stride, _p(out))); return out

    @property
    def nbytes(self):
        return self.L.gkc_bloom_nbytes(self.h)

    @property
    def bitsize(self):
        return self.L.gkc_bloom_bitsize(self.h)

    def allreduce_or(self, comm):
        """OR the partial filters of all ranks in place (collective): gkc_bloom_allreduce_or"""
        self.c._chk(self.L.gkc_bloom_allreduce_or(self.h, comm.h))

    def device_array(self):
        """(device pointer, bytes) of the bit array"""
        p = C.c_void_p(); n = C.c_uint64(0)
        self.c._chk(self.L.gkc_bloom_device_array(self.h, C.byref(p), C.byref(n))); return p.value, n.value

    def array(self):
        out = np.zeros(self.nbytes, np.uint8)
        self.c._chk(self.L.gkc_bloom_get_array(self.h, _p(out), len(out))); return out

    def close(self):
        if getattr(self, "h", None):
            self.L.gkc_bloom_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Banks:
    """gkc_banks: the counts of several banks merged on the device — per dataset the distinct k-mers of all banks with one abundance per bank — and the
    reference's solidity kinds evaluated on them (include/gkc.h, multi-bank counting). Count bank i with ``counter`` (default solidity window), then
    ``add(i)``; ``evaluate`` as often as needed; read with ``partition`` / ``vectors`` / ``histogram``."""
    TILE = 1024          # k-mers one workgroup merges / scans at a time (csrc/gkc_banks.hip BK_TILE)
    SCAN_BLOCK = 256     # tile sums the one-workgroup scan takes at a time (BK_SCAN_BLOCK)

    def __init__(self, counter, nb_banks):
        self.c = counter; self.L = counter.L; self.nb_banks = nb_banks
        self.nb_datasets = counter.nb_partitions * counter.nb_passes
        self.rec_bytes = counter.rec_bytes
        self._ctx = C.c_void_p(counter.h.value)       # error messages live in the context the object was created from (alive as long as the object is)
        h = C.c_void_p()
        counter._chk(self.L.gkc_banks_create(counter.h, nb_banks, C.byref(h)))
        self.h = h; self.histo_max = None

    def _chk(self, rc):
        if rc != 0:
            raise GkcError("gkc error %d: %s" % (rc, (self.L.gkc_last_error(self._ctx) or b"").decode()))

    def add(self, bank, counter=None):
        """every finished dataset of ``counter`` (default: the one the object was created from) becomes the column of ``bank``"""
        self._chk(self.L.gkc_banks_add(self.h, (counter or self.c).h, bank))

    def _per_bank(self, v, dtype):
        a = np.asarray(v, dtype=dtype)
        a = np.full(self.nb_banks, a, dtype=dtype) if a.ndim == 0 else np.ascontiguousarray(a)
        if a.shape != (self.nb_banks,):
            raise GkcError("one value per bank expected")
        return a

    def evaluate(self, kind="sum", amin=1, amax=2147483647, solid_vec=None, histo_max=10000):
        """kind: "sum" | "min" | "max" | "one" | "all" | "custom" (or GKC_SOLIDITY_*); amin / amax: one value for every bank or one per bank"""
        k = SOLIDITY_KINDS[kind] if isinstance(kind, str) else int(kind)
        lo = self._per_bank(amin, np.int32); hi = self._per_bank(amax, np.int32)
        sv = None if solid_vec is None else self._per_bank(solid_vec, np.uint8)
        self._chk(self.L.gkc_banks_evaluate(self.h, k, _p(lo), _p(hi), _p(sv), histo_max))
        self.histo_max = histo_max

    def partition_info(self, dataset):
        """-> (solid, distinct) k-mers of the dataset"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.gkc_banks_partition_info(self.h, dataset, C.byref(a), C.byref(b)))
        return a.value, b.value

    def partition_records(self, dataset):
        """raw Count{value, sum} records of the dataset's solid k-mers (uint8 view)"""
        ns, _ = self.partition_info(dataset)
        out = np.zeros(max(1, ns * self.rec_bytes), np.uint8); n = C.c_uint64()
        self._chk(self.L.gkc_banks_partition_counts(self.h, dataset, _p(out), ns, C.byref(n)))
        return out[: ns * self.rec_bytes]

    def partition(self, dataset):
        """-> (lo uint64[], hi uint64[], abundance int32[]): the structured arrays of Counter.partition, abundance = sum over the banks"""
        raw = self.partition_records(dataset)
        w = self.rec_bytes // 8
        r = raw.view(np.uint64).reshape(-1, w)
        hi = np.zeros(len(r), np.uint64) if w == 2 else r[:, 1].copy()
        return r[:, 0].copy(), hi, (r[:, w // 2] & np.uint64(0xFFFFFFFF)).astype(np.int32)

    def vectors(self, dataset):
        """-> int32[n_solid][nb_banks]: the abundance of every solid k-mer of the dataset in every bank, rows in the order of ``partition``"""
        ns, _ = self.partition_info(dataset)
        out = np.zeros((max(1, ns), self.nb_banks), np.int32); n = C.c_uint64()
        self._chk(self.L.gkc_banks_partition_vectors(self.h, dataset, _p(out), ns, C.byref(n)))
        return out[:ns]

    def partition_device(self, dataset):
        """-> (device pointer of the records, device pointer of the count vectors, n_solid)"""
        p = C.c_void_p(); v = C.c_void_p(); n = C.c_uint64()
        self._chk(self.L.gkc_banks_partition_counts_device(self.h, dataset, C.byref(p), C.byref(v), C.byref(n)))
        return p.value, v.value, n.value

    def query_reads_device(self, d_bases, d_offsets, n_reads, n_bases, d_sum, d_vectors=None):
        self._chk(self.L.gkc_query_banks_reads_device(self.h, d_bases, d_offsets, n_reads, n_bases, d_sum, d_vectors))

    def query_reads(self, bases, offsets, vectors=True):
        """the k-mers of the reads against the merged state (no evaluation needed) -> (int32[n_bases] sum over the banks, > 0 / 0 / -1 like Counter.query_reads,
        int32[n_bases][nb_banks] rows or None)"""
        import torch
        bases = np.ascontiguousarray(bases, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nb = len(bases)
        tb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        if nb:
            tb[:nb] = torch.from_numpy(bases.copy()).cuda()
        to = torch.from_numpy(offsets.view(np.uint8).copy()).cuda()
        ts = torch.zeros(nb + 16, dtype=torch.int32, device="cuda")
        tv = torch.zeros(nb * self.nb_banks + 16, dtype=torch.int32, device="cuda") if vectors else None
        torch.cuda.synchronize()
        self.query_reads_device(tb.data_ptr(), to.data_ptr(), len(offsets) - 1, nb, ts.data_ptr(), tv.data_ptr() if vectors else None)
        sums = ts.cpu().numpy()[:nb].copy()
        return sums, (tv.cpu().numpy()[: nb * self.nb_banks].reshape(nb, self.nb_banks).copy() if vectors else None)

    def histogram(self):
        """histogram[min(sum, histo_max)] over all distinct k-mers of the last evaluation"""
        hm = self.histo_max if self.histo_max is not None else 10000
        h = np.zeros(hm + 1, np.uint64)
        self._chk(self.L.gkc_banks_histogram(self.h, _p(h), hm + 1))
        return h

    def all_counts(self):
        """{k-mer: tuple of its abundance in every bank} over the solid k-mers of all datasets"""
        out = {}
        for d in range(self.nb_datasets):
            lo, hi, _ = self.partition(d)
            for a, b, v in zip(lo.tolist(), hi.tolist(), self.vectors(d).tolist()):
                out[(b << 64) | a] = tuple(v)
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.gkc_banks_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
