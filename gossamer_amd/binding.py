"""ctypes binding of libgossgpu.so (the C ABI declared in include/goss_gpu.h).

This module is plumbing only: it loads the in-tree shared library, declares the entry
points and wraps them in a small context class.  There is no fallback of any kind: if the
library is missing, or no gfx950 device is usable, the calls raise.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOSS_GPU_LIB") or os.path.join(_PKG, "libgossgpu.so")

MODE_KMER_SET = 0
MODE_GRAPH = 1

# every symbol include/goss_gpu.h declares
SYMBOLS = [
    "goss_gpu_strerror", "goss_gpu_last_error", "goss_gpu_abi_version", "goss_gpu_create",
    "goss_gpu_destroy", "goss_gpu_push_bases_host", "goss_gpu_push_bases_device",
    "goss_gpu_finish", "goss_gpu_result", "goss_gpu_result_copy", "goss_gpu_emit",
    "goss_gpu_file_count", "goss_gpu_file_info", "goss_gpu_file_read",
    "goss_gpu_emit_sparse_array", "goss_gpu_timing_get", "goss_gpu_timing_reset",
    "goss_gpu_synth_reads", "goss_synth_reads_host", "goss_gpu_reset", "goss_gpu_push_run_device", "goss_gpu_set_path", "goss_gpu_host_alloc", "goss_gpu_host_free", "goss_gpu_host_register", "goss_gpu_host_unregister", "goss_gpu_push_run_sparse", "goss_gpu_push_run_host", "goss_gpu_emit_estimate",
    "goss_gpu_select_counts", "goss_gpu_select_normal", "goss_gpu_emit_count_bits", "goss_gpu_emit_dump", "goss_gpu_lint", "goss_gpu_stat", "goss_gpu_check_index",
    "goss_gpu_set_budget_limit", "goss_gpu_emit_dump_range", "goss_gpu_prepare", "goss_gpu_emit_part", "goss_gpu_emit_assemble", "goss_gpu_emit_part_ranges", "goss_gpu_emit_last_high",
    "goss_gpu_file_device", "goss_gpu_big_counts", "goss_gpu_push_run_graph",
    "goss_gpu_group_exchange", "goss_gpu_group_emit",
    "goss_gpu_set_deferred", "goss_gpu_stage_room", "goss_gpu_group_route_exchange",
    "goss_gpu_push_keys_host", "goss_gpu_push_keys_device", "goss_gpu_push_packed_device", "goss_gpu_pack_bases_device", "goss_gpu_expect_bases",
    "goss_gpu_route_records_device", "goss_gpu_push_records_device",
    "goss_gpu_push_bases_host_async", "goss_gpu_push_packed_host", "goss_gpu_push_packed_host_async", "goss_gpu_flush",
    "goss_gpu_object_open", "goss_gpu_object_open_emitted", "goss_gpu_object_close", "goss_gpu_object_last_error",
    "goss_gpu_object_info", "goss_gpu_object_rank", "goss_gpu_object_select", "goss_gpu_object_multiplicity",
    "goss_gpu_object_lookup", "goss_gpu_object_node_ranks",
    "goss_gpu_prune_tips", "goss_gpu_trim_paths", "goss_gpu_clip_links", "goss_gpu_paths_timing",
    "goss_gpu_segments_build", "goss_gpu_segments_table", "goss_gpu_segments_text", "goss_gpu_segments_release",
    "goss_gpu_entries_build", "goss_gpu_entries_release", "goss_gpu_entries_length", "goss_gpu_entries_end_rank",
    "goss_gpu_components_mark_host", "goss_gpu_components_mark_device", "goss_gpu_components_build", "goss_gpu_components_table",
    "goss_gpu_components_labels", "goss_gpu_components_keep", "goss_gpu_components_release",
    "goss_gpu_components_grow", "goss_gpu_components_marks", "goss_gpu_components_keep_marked",
    "goss_gpu_pool_begin", "goss_gpu_pool_add_masks", "goss_gpu_pool_sizes", "goss_gpu_pool_intersections",
    "goss_gpu_pool_emit_index", "goss_gpu_pool_release",
]

# every symbol include/goss_gpu_match.h declares (reads against an object)
MATCH_SYMBOLS = ["goss_gpu_object_match_reads", "goss_gpu_object_match_reads_host"]

# every symbol include/goss_gpu_near.h declares (compute-near-kmers on an object)
NEAR_SYMBOLS = ["goss_gpu_object_near_kmers", "goss_gpu_object_near_kmers_host"]
CLASSIFY_SYMBOLS = ["goss_gpu_object_classify_reads", "goss_gpu_object_classify_bits_host", "goss_gpu_object_classify_reads_host"]

# every symbol include/goss_gpu_elect.h declares (reads against up to 64 references: colour words on a KmerSet)
ELECT_SYMBOLS = ["goss_gpu_object_colours_host", "goss_gpu_object_colours_from_index", "goss_gpu_object_colour_reads",
                 "goss_gpu_object_colour_reads_host"]

# every symbol include/goss_gpu_taxo.h declares (annotate-kmers and classify-reads on an object)
TAXO_SYMBOLS = ["goss_gpu_object_taxo_tree_host", "goss_gpu_object_taxo_annotation_host", "goss_gpu_object_taxo_annotation_read",
                "goss_gpu_object_taxo_annotate", "goss_gpu_object_taxo_annotate_host", "goss_gpu_object_taxo_classify_reads",
                "goss_gpu_object_taxo_classify_reads_host", "goss_gpu_object_taxo_pair", "goss_gpu_object_taxo_pair_host",
                "goss_gpu_object_taxo_tally", "goss_gpu_object_taxo_tally_host"]

# every symbol include/goss_gpu_relative.h declares (trim-relative and merge-graph-with-reference on a finished graph)
RELATIVE_SYMBOLS = ["goss_gpu_trim_relative", "goss_gpu_recount_from", "goss_gpu_relative_timing"]

# every symbol include/goss_gpu_links.h declares (read links: reads threaded over the linear segments of a finished graph)
READ_LINKS_SYMBOLS = ["goss_gpu_read_links_begin", "goss_gpu_read_links_segments", "goss_gpu_read_links_windows_host",
                      "goss_gpu_read_links_add_host", "goss_gpu_read_links_finish", "goss_gpu_read_links_table",
                      "goss_gpu_read_links_release"]

RECORD_BYTES = 12          # one-word keys (2 * len <= 62); two-word keys: 20 (record_bytes)


def record_bytes(k, mode=0):
    """bytes of a super-k-mer record of a (k, mode) context: SkRec (12) for one-word keys, SkRec2 (20) for two-word keys"""
    length = k + (1 if mode == 1 else 0)
    return 12 if 2 * length <= 62 else 20


RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p)

# goss_gpu_tips_report, in the order of its fields
TIPS_REPORT_FIELDS = ("edges_before", "edges_after", "candidates", "tips", "zapped", "too_long", "both_joined", "isolated",
                      "outweighed", "joined_at_begin", "joined_at_end")

# goss_gpu_paths_report and goss_gpu_links_report, in the order of their fields
PATHS_REPORT_FIELDS = ("edges_before", "edges_after", "candidates", "paths", "zapped", "too_long", "spared_by_cutoff", "missing_rc")
LINKS_REPORT_FIELDS = ("edges_before", "edges_after", "candidates", "links", "edges", "too_long", "major_out", "major_in", "missing_rc")
PATHS_CUTOFF = 1
PATHS_NO_EDGE = 0xFFFFFFFFFFFFFFFF

# goss_gpu_relative_report and goss_gpu_recount_report, in the order of their fields
RELATIVE_REPORT_FIELDS = ("edges_before", "edges_after", "forks", "below", "mirror_only")
RECOUNT_REPORT_FIELDS = ("edges_before", "edges_after")


# goss_gpu_segments_info and goss_gpu_segment, in the order of their fields
SEGMENTS_INFO_FIELDS = (("segments", C.c_uint64), ("text_bytes", C.c_uint64), ("paths", C.c_uint64), ("taken_paths", C.c_uint64),
                        ("cycle_edges", C.c_uint64), ("longest_path", C.c_uint64), ("rounds", C.c_uint32),
                        ("walk_steps", C.c_uint32), ("ms_link", C.c_float), ("ms_rank", C.c_float),
                        ("ms_figures", C.c_float), ("ms_text", C.c_float))
SEGMENT_DTYPE = [("s", "<u8"), ("s2", "<u8"), ("text_offset", "<u8"), ("text_bytes", "<u8"), ("len", "<u8"),
                 ("first_rank", "<u4"), ("edges", "<u4"), ("min", "<u4"), ("max", "<u4"), ("flags", "<u4"), ("end_rank", "<u4")]
SEGMENTS_NO_LINE_BREAKS = 1
SEGMENT_INCLUDE_FIRST, SEGMENT_INCLUDE_LAST = 1, 2


class SegmentsInfo(C.Structure):
    _fields_ = list(SEGMENTS_INFO_FIELDS)


# goss_gpu_entries_info, in the order of its fields
ENTRIES_INFO_FIELDS = (("entries", C.c_uint64), ("cycle_edges", C.c_uint64), ("longest_path", C.c_uint64),
                       ("hist_size", C.c_uint64), ("rounds", C.c_uint32), ("walk_steps", C.c_uint32),
                       ("ms_link", C.c_float), ("ms_rank", C.c_float), ("ms_paths", C.c_float), ("ms_emit", C.c_float))


class EntriesInfo(C.Structure):
    _fields_ = list(ENTRIES_INFO_FIELDS)


# goss_gpu_mark_info, goss_gpu_components_info and goss_gpu_component, in the order of their fields
MARK_INFO_FIELDS = (("windows", C.c_uint64), ("hits", C.c_uint64), ("marked_total", C.c_uint64), ("ms", C.c_float))
COMPONENTS_INFO_FIELDS = (("components", C.c_uint64), ("marked_edges", C.c_uint64), ("largest", C.c_uint64), ("launches", C.c_uint32),
                          ("ms_link", C.c_float), ("ms_label", C.c_float), ("ms_figures", C.c_float))
COMPONENT_DTYPE = [("s", "<u8"), ("s2", "<u8"), ("edges", "<u8"), ("start", "<u4"), ("min", "<u4"), ("max", "<u4"), ("mirror", "<u4")]
COMPONENTS_MARKED = 1
COMPONENT_NONE = 0xFFFFFFFF


# goss_gpu_grow_info, in the order of its fields
GROW_INFO_FIELDS = (("marked_before", C.c_uint64), ("mirrored", C.c_uint64), ("marked_total", C.c_uint64), ("passes_run", C.c_uint32),
                    ("launches", C.c_uint32), ("ms_link", C.c_float), ("ms_label", C.c_float), ("ms_grow", C.c_float))
GROW_LINEAR_PATHS = 1


# goss_gpu_read_links_info, goss_gpu_read_links_batch, goss_gpu_read_links_table_info and goss_gpu_link_row
READ_LINKS_INFO_FIELDS = (("edges", C.c_uint64), ("entries", C.c_uint64), ("edges_without_segment", C.c_uint64),
                          ("ms_link", C.c_float), ("ms_rank", C.c_float), ("ms_segments", C.c_float), ("reserved", C.c_uint32))
READ_LINKS_BATCH_FIELDS = (("reads", C.c_uint64), ("windows", C.c_uint64), ("misses", C.c_uint64), ("carried", C.c_uint64),
                           ("hits", C.c_uint64), ("records", C.c_uint64), ("ms_windows", C.c_float), ("ms_scans", C.c_float),
                           ("ms_compact", C.c_float), ("reserved", C.c_uint32))
READ_LINKS_TABLE_FIELDS = (("records", C.c_uint64), ("rows", C.c_uint64), ("ms_sort", C.c_float), ("ms_reduce", C.c_float))
LINK_DTYPE = [("a", "<u4"), ("b", "<u4"), ("count", "<u8"), ("gap_sum", "<u8")]
LINKS_CARRY = 1
LINK_NONE = 0xFFFFFFFF                           # Context.segment_of_edges: an edge on a cycle without an entry edge
LINK_MISS = 0xFFFFFFFF                           # Context.thread_windows: a window that was not aligned
LINK_NON_UNIQUE = 0x80000000                     # ... set on the segment of a window whose segment is not unique


class ReadLinksInfo(C.Structure):
    _fields_ = list(READ_LINKS_INFO_FIELDS)


class ReadLinksBatch(C.Structure):
    _fields_ = list(READ_LINKS_BATCH_FIELDS)


class ReadLinksTableInfo(C.Structure):
    _fields_ = list(READ_LINKS_TABLE_FIELDS)


def unique_segments(lengths, multiplicities, k, coverage):
    """SuperGraph::unique (SuperGraph.cc:667-700) for superpaths of one segment each, as they are straight after
    build-supergraph: np.bool_ per entry from the EntryEdgeSet's lengths and multiplicities.  False where
    length + k < 50; else f = ln(2) / 2 + (n / (2 rho)) (rho^2 - c^2 / 2) >= 5.0 with n = length, c = (n * multiplicity)
    / n and rho = coverage, in float64 with the reference's operations in its order, one rounding each.  Pure numpy."""
    import numpy as np
    lengths = np.asarray(lengths, dtype=np.uint64)
    n = lengths.astype(np.float64)
    m = np.asarray(multiplicities, dtype=np.uint32).astype(np.float64)
    rho = np.float64(coverage)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (n * m) / n
        k0 = np.float64(np.log(np.float64(2.0))) / np.float64(2.0)
        f = k0 + (n / (np.float64(2) * rho)) * (rho * rho - (c * c) / np.float64(2.0))
        ok = f >= np.float64(5.0)
    return ok & ~(lengths + np.uint64(k) < np.uint64(50))


def estimate_coverage(hist):
    """EstimateCoverageOnly (EstimateGraphStatistics.cc:306-364) over a multiplicity histogram -- a dict or (x, y) pairs,
    taken in ascending x.  Integer logic over the first 50 rows: the x of the largest y from the first rise on.  Fewer
    than 50 rows, or a gap between two of the first 50 x, raise ValueError with the reference's text.  The reference's
    two errors are kept: rows beyond the fiftieth are never looked at, so a peak there is missed; and a histogram that
    never rises among them answers 0 instead of failing.  Pure Python."""
    rows = sorted(dict(hist).items()) if not isinstance(hist, dict) else sorted(hist.items())
    if len(rows) < 50:
        raise ValueError("Not enough data to estimate coverage.")
    fit, best_x, best_y = False, 0, 0
    prev_x, prev_y = rows[0]
    for x, y in rows[1:50]:
        if prev_x + 1 != x:
            raise ValueError("Coverage histogram appears to be discontinuous. Cannot estimate coverage.")
        if prev_y < y:
            fit = True
        if fit and best_y < y:
            best_x, best_y = x, y
        prev_x, prev_y = x, y
    return int(best_x)


def filter_links(table, min_count):
    """The three filters of GossCmdThreadReads.cc:795-886 over a LINK_DTYPE table, as a new LINK_DTYPE table ascending by
    (a, b).  One: a row of count < min_count goes; a row that stays becomes (a, b, count 1, gap_sum = gap_sum // count) --
    the reference re-adds it with its average gap and the default count.  Two: of the rows of one a the best supported
    stays; three: of the rows of one b likewise.  After the first filter every count is 1, so both choices are ties:
    the reference takes the first of a vector filled in unordered_map order, which depends on the library's hash; here
    the tie goes to the smallest id.  Pure numpy, no device work."""
    import numpy as np
    t = np.sort(np.asarray(table, dtype=LINK_DTYPE), order=["a", "b"])
    t = t[t["count"] >= min_count]
    t["gap_sum"] = t["gap_sum"] // np.maximum(t["count"], 1)
    t["count"] = 1
    if len(t):                                       # (sorted by (a, b): the first row of an a has its smallest b)
        t = t[np.concatenate(([True], t["a"][1:] != t["a"][:-1]))]
        t = np.sort(t, order=["b", "a"])
        t = t[np.concatenate(([True], t["b"][1:] != t["b"][:-1]))]
        t = np.sort(t, order=["a", "b"])
    return t


class MarkInfo(C.Structure):
    _fields_ = list(MARK_INFO_FIELDS)


class GrowInfo(C.Structure):
    _fields_ = list(GROW_INFO_FIELDS)


class ComponentsInfo(C.Structure):
    _fields_ = list(COMPONENTS_INFO_FIELDS)


# pool-samples (csrc/kernels_pool.hpp): rows of the pair tile, words of a row per visit of a workgroup of
# pool_pairs_kernel, words of a row per workgroup of pool_positions_kernel
POOL_TILE = 64
POOL_PAIR_WORDS = 128
POOL_POS_WORDS = 128


def pool_similarity_text(inter, sizes):
    """the <out>.sim text of pool-samples (GossCmdPoolSamples.cc): for every i < j one line "i\tj\tsim\n" with
    sim = double(inter) / double(|i| + |j| - inter) as a C++ ostream prints it; inter[i][j] = common k-mers"""
    out = []
    n = len(sizes)
    for i in range(n):
        for j in range(i + 1, n):
            x = int(inter[i][j])
            u = int(sizes[i]) + int(sizes[j]) - x
            out.append("%d\t%d\t%s\n" % (i, j, format_double(float(x) / float(u)) if u else "-nan"))
    return "".join(out)


def format_double(x):
    """a double as a C++ ostream prints it by default (six significant digits, %g)"""
    return "%g" % x


def segment_stats(row, k):
    """(L, min, max, mean, sd) of one row of the segment table as print-contigs prints them: L = edges + K, the mean
    and the deviation from the 64-bit sums in doubles, in the reference's order of operations"""
    import math
    m = int(row["edges"])
    a = float(int(row["s"])) / m
    rad = float(int(row["s2"])) / m - a * a
    sd = format_double(math.sqrt(rad)) if rad >= 0.0 else "-nan"
    return m + k, int(row["min"]), int(row["max"]), format_double(a), sd


def pack_bases(text):
    """bytes of bases -> (codes u32 per 16 positions, nonbase u16 per 16 positions): the packed form of
    goss_gpu_push_packed_host (numpy restatement of the host parser's packer, for the tests)."""
    import numpy as np
    a = np.frombuffer(text if isinstance(text, (bytes, bytearray)) else text.encode(), dtype=np.uint8)
    n = a.size
    g = (n + 15) // 16
    pad = np.full(g * 16, 10, dtype=np.uint8)
    pad[:n] = a
    low = pad | 0x20
    code = np.zeros(g * 16, dtype=np.uint32)
    code[low == ord("c")] = 1
    code[low == ord("g")] = 2
    code[low == ord("t")] = 3
    bad = ~((low == ord("a")) | (low == ord("c")) | (low == ord("g")) | (low == ord("t")))
    shifts = (2 * np.arange(16, dtype=np.uint32))[None, :]
    codes = np.bitwise_or.reduce(code.reshape(g, 16) << shifts, axis=1).astype(np.uint32)
    bshift = np.arange(16, dtype=np.uint32)[None, :]
    nonbase = np.bitwise_or.reduce(bad.reshape(g, 16).astype(np.uint32) << bshift, axis=1).astype(np.uint16)
    return np.ascontiguousarray(codes), np.ascontiguousarray(nonbase)


class GossGpuError(RuntimeError):
    def __init__(self, status, text, detail=""):
        super().__init__("%s (status %d)%s" % (text, status, (": " + detail) if detail else ""))
        self.status = status


class Counts(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("keys", C.c_uint64), ("distinct", C.c_uint64),
                ("key_words", C.c_uint32), ("reserved", C.c_uint32)]


T_EXTRACT, T_HIST, T_SCAN, T_SCATTER, T_REDUCE, T_EMIT, T_ORDER, T_CLASSES = 0, 1, 2, 3, 4, 5, 6, 8
T_NAMES = ["extract", "hist", "scan", "scatter", "reduce", "emit", "order"]


class Timing(C.Structure):
    _fields_ = [("ms", C.c_float * T_CLASSES), ("launches", C.c_uint32 * T_CLASSES),
                ("units", C.c_uint64 * T_CLASSES)]

    def as_dict(self):
        return {n: {"ms": self.ms[i], "launches": self.launches[i], "units": self.units[i]}
                for i, n in enumerate(T_NAMES)}


_lib = None


def load():
    """Load libgossgpu.so; raises if it has not been built (see __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GossGpuError(-2, "libgossgpu.so is not built", LIB_PATH)
    try:
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7; importing it
        # first makes libgossgpu.so bind to that same runtime (same SONAME) instead of
        # bringing /opt/rocm's copy in beside it, which leaves torch without a GPU.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.goss_gpu_strerror.restype = C.c_char_p
    L.goss_gpu_strerror.argtypes = [C.c_int]
    L.goss_gpu_last_error.restype = C.c_char_p
    L.goss_gpu_last_error.argtypes = [C.c_void_p]
    L.goss_gpu_abi_version.restype = C.c_uint32
    L.goss_gpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p]
    L.goss_gpu_destroy.argtypes = [C.c_void_p]
    L.goss_gpu_destroy.restype = None
    L.goss_gpu_push_bases_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.goss_gpu_push_bases_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.goss_gpu_finish.argtypes = [C.c_void_p, C.POINTER(Counts)]
    L.goss_gpu_result.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.goss_gpu_result_copy.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.goss_gpu_emit.argtypes = [C.c_void_p]
    L.goss_gpu_file_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.goss_gpu_file_info.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.goss_gpu_file_read.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64]
    L.goss_gpu_emit_sparse_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                             C.c_uint64, C.c_uint64, C.c_uint64]
    L.goss_gpu_timing_get.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.goss_gpu_timing_reset.argtypes = [C.c_void_p]
    L.goss_gpu_reset.argtypes = [C.c_void_p]
    L.goss_gpu_set_path.argtypes = [C.c_void_p, C.c_int]
    L.goss_gpu_push_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.goss_gpu_synth_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]
    L.goss_synth_reads_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]
    _lib = L
    return L


def synth_reads_host(nreads, read_len, genome_len, seed=1, first_read=0):
    """The synthetic read generator on the host: bytes of nreads*(read_len+1)."""
    L = load()
    buf = C.create_string_buffer(nreads * (read_len + 1))
    rc = L.goss_synth_reads_host(buf, nreads, read_len, genome_len, seed, first_read)
    if rc:
        raise GossGpuError(rc, L.goss_gpu_strerror(rc).decode())
    return buf.raw


def _torch_ready():
    """The library runs on its own HIP stream.  Device buffers handed to it by pointer usually come
    from torch, whose kernels are asynchronous on torch's stream: wait for them (C callers of the
    ABI order their own streams; this wrapper does it for the Python tests and bench.py)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


def group_exchange(contexts, sample_per_context=0):
    """goss_gpu_group_exchange on several finished Contexts of one process: context j ends up holding range j
    of the union.  Returns the range sizes."""
    L = load()
    n = len(contexts)
    arr = (C.c_void_p * n)(*[c._h for c in contexts])
    sizes = (C.c_uint64 * n)()
    L.goss_gpu_group_exchange.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    _torch_ready()
    contexts[0]._check(L.goss_gpu_group_exchange(arr, n, sample_per_context, sizes))
    return [int(x) for x in sizes]


class GroupXStats(C.Structure):
    _fields_ = [("transport", C.c_uint32), ("rounds", C.c_uint32), ("records", C.c_uint64), ("windows", C.c_uint64),
                ("record_bytes", C.c_uint64), ("route_ms", C.c_double), ("wire_ms", C.c_double), ("count_ms", C.c_double),
                ("count_wait_ms", C.c_double)]


def group_route_exchange(contexts, transport=0):
    """goss_gpu_group_route_exchange: what the (deferred) contexts have staged is cut into super-k-mer records routed by
    minimizer, part p of every context moved to context p and counted there.  Returns the call's statistics as a dict."""
    L = load()
    n = len(contexts)
    arr = (C.c_void_p * n)(*[c._h for c in contexts])
    st = GroupXStats()
    L.goss_gpu_group_route_exchange.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.POINTER(GroupXStats)]
    _torch_ready()
    contexts[0]._check(L.goss_gpu_group_route_exchange(arr, n, transport, C.byref(st)))
    return {f: getattr(st, f) for f, _ in GroupXStats._fields_}


def group_emit(contexts, estimate=0):
    """goss_gpu_group_emit: every context's slices, the index files on contexts[0]"""
    L = load()
    n = len(contexts)
    arr = (C.c_void_p * n)(*[c._h for c in contexts])
    L.goss_gpu_group_emit.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint64]
    contexts[0]._check(L.goss_gpu_group_emit(arr, n, estimate))


class Context:
    """One counting context on one GPU (include/goss_gpu.h)."""

    def __init__(self, k, mode=MODE_KMER_SET, device=0, hbm_budget=0, stream=None):
        self._L = load()
        self._h = C.c_void_p()
        rc = self._L.goss_gpu_create(C.byref(self._h), device, k, mode, hbm_budget, stream)
        if rc:
            self._h = None
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode())
        self.k = k
        self.mode = mode
        self.device = device
        self.key_words = 1 if 2 * (k + (1 if mode == MODE_GRAPH else 0)) <= 62 else 2

    def close(self):
        if getattr(self, "_h", None):
            self._L.goss_gpu_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(),
                               self._L.goss_gpu_last_error(self._h).decode())

    def push_host(self, data):
        if isinstance(data, str):
            data = data.encode()
        self._check(self._L.goss_gpu_push_bases_host(self._h, data, len(data)))

    def push_host_async(self, data, on_release=None):
        """goss_gpu_push_bases_host_async: the bytes object stays referenced until the library hands it back."""
        if isinstance(data, str):
            data = data.encode()
        if not hasattr(self, "_lent"):
            self._lent, self._lent_id = {}, 0
            self._release_cb = RELEASE_FN(self._released)
        self._lent_id += 1
        self._lent[self._lent_id] = (data, on_release)
        self._L.goss_gpu_push_bases_host_async.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, RELEASE_FN, C.c_void_p]
        self._check(self._L.goss_gpu_push_bases_host_async(self._h, data, len(data), self._release_cb, C.c_void_p(self._lent_id)))

    def _released(self, user):
        data, cb = self._lent.pop(int(user or 0))
        if cb:
            cb()

    def push_packed_host(self, text, async_=False):
        """Pack a byte string of bases on the host (2 bits per base + 1 flag bit) and push it
        (goss_gpu_push_packed_host / _async).  Returns (codes, nonbase) numpy arrays."""
        import numpy as np
        codes, bad = pack_bases(text)
        n = len(text)
        if async_:
            if not hasattr(self, "_lent"):
                self._lent, self._lent_id = {}, 0
                self._release_cb = RELEASE_FN(self._released)
            self._lent_id += 1
            self._lent[self._lent_id] = ((codes, bad), None)
            self._L.goss_gpu_push_packed_host_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, RELEASE_FN, C.c_void_p]
            self._check(self._L.goss_gpu_push_packed_host_async(self._h, C.c_void_p(codes.ctypes.data), C.c_void_p(bad.ctypes.data), n,
                                                                self._release_cb, C.c_void_p(self._lent_id)))
        else:
            self._L.goss_gpu_push_packed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
            self._check(self._L.goss_gpu_push_packed_host(self._h, C.c_void_p(codes.ctypes.data), C.c_void_p(bad.ctypes.data), n))
        return codes, bad

    def flush(self):
        """goss_gpu_flush: wait for the queued copies; every lent buffer comes back."""
        self._L.goss_gpu_flush.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_flush(self._h))

    def push_device(self, ptr, nbytes):
        _torch_ready()
        self._check(self._L.goss_gpu_push_bases_device(self._h, C.c_void_p(ptr), nbytes))

    def expect_bases(self, total_bases):
        """goss_gpu_expect_bases: a hint -- how many bases will be pushed in all before finish (0: unknown)."""
        self._L.goss_gpu_expect_bases.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_expect_bases(self._h, total_bases))

    def push_packed_device(self, codes_ptr, nonbase_ptr, nbases):
        """goss_gpu_push_packed_device: packed bases resident in HBM (u32 of codes + u16 of flags per 16 positions)."""
        _torch_ready()
        self._L.goss_gpu_push_packed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_push_packed_device(self._h, C.c_void_p(codes_ptr), C.c_void_p(nonbase_ptr), nbases))

    def pack_bases_device(self, bases_ptr, nbytes, codes_ptr, nonbase_ptr):
        """goss_gpu_pack_bases_device: bytes in HBM -> the packed form in the caller's arrays (ceil(nbytes / 16) each)."""
        _torch_ready()
        self._L.goss_gpu_pack_bases_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        self._check(self._L.goss_gpu_pack_bases_device(self._h, C.c_void_p(bases_ptr), nbytes, C.c_void_p(codes_ptr), C.c_void_p(nonbase_ptr)))

    def push_run(self, keys_ptr, counts_ptr, m):
        _torch_ready()
        self._check(self._L.goss_gpu_push_run_device(self._h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), m))

    def push_run_host(self, keys_ptr, counts_ptr, m):
        """A counted run in host memory (goss_gpu_push_run_host): m keys of key_words u64, m u32 counts."""
        self._L.goss_gpu_push_run_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_push_run_host(self._h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), m))

    def push_keys_host(self, keys):
        """Raw k-mers (unsorted, un-normalised) in host memory: a numpy uint64 array of n * key_words values
        (goss_gpu_push_keys_host)."""
        import numpy as np
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        n = a.size // self.key_words
        self._L.goss_gpu_push_keys_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_push_keys_host(self._h, C.c_void_p(a.ctypes.data), n))

    def push_keys_device(self, ptr, n):
        """Raw k-mers resident in HBM (goss_gpu_push_keys_device)."""
        _torch_ready()
        self._L.goss_gpu_push_keys_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_push_keys_device(self._h, C.c_void_p(ptr), n))

    def route_records(self, bases_ptr, nbytes, nparts, records_ptr, part_first, part_cap, ready=False):
        """goss_gpu_route_records_device: the windows of a device-resident base string as super-k-mer records in
        nparts buffers.  Returns (record slots filled per part -- pads, records of no window, included --, windows per
        part, ok); ok False = some part_cap was too small and `records` holds what every part needs.  ready: the
        caller has waited for whatever wrote the bases (no device-wide synchronisation here)."""
        if not ready:
            _torch_ready()
        U = C.c_uint64 * nparts
        first, cap, recs, wins = U(*part_first), U(*part_cap), U(), U()
        self._L.goss_gpu_route_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                          C.POINTER(C.c_uint64)]
        rc = self._L.goss_gpu_route_records_device(self._h, C.c_void_p(bases_ptr), nbytes, nparts, C.c_void_p(records_ptr),
                                                   first, cap, recs, wins)
        if rc not in (0, -9):
            self._check(rc)
        return [int(x) for x in recs], [int(x) for x in wins], rc == 0

    def push_records(self, records_ptr, nrecords, nwindows=0, ready=False):
        """goss_gpu_push_records_device: count the windows of super-k-mer records resident in HBM.  ready: the caller
        has waited for whatever wrote the records (no device-wide synchronisation here: other streams go on)."""
        if not ready:
            _torch_ready()
        self._L.goss_gpu_push_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
        self._check(self._L.goss_gpu_push_records_device(self._h, C.c_void_p(records_ptr), nrecords, nwindows))

    def prepare(self):
        """Start mapping the HBM arena in the background (goss_gpu_prepare)."""
        self._L.goss_gpu_prepare.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_prepare(self._h))

    def push_run_graph(self, files, key_bits):
        """A graph given as {suffix: bytes} of its files ("-edges.*", "-counts.*") as one run, edges and
        multiplicities decoded on the device (goss_gpu_push_run_graph)."""
        import struct

        class SparseRun(C.Structure):
            _fields_ = [("D", C.c_uint64), ("count", C.c_uint64), ("high_bits", C.c_char_p), ("high_words", C.c_uint64),
                        ("ncols", C.c_uint32), ("weight", C.c_uint32), ("col", C.c_char_p * 4), ("col_bytes", C.c_uint32 * 4),
                        ("col_shift", C.c_uint32 * 4), ("counts", C.c_void_p)]

        class Vba(C.Structure):
            _fields_ = [("ord0", C.c_char_p), ("ord0_bytes", C.c_uint64), ("ord1p", SparseRun), ("ord1", C.c_char_p),
                        ("ord1_bytes", C.c_uint64), ("ord2p", SparseRun), ("ord2", C.c_char_p), ("ord2_bytes", C.c_uint64)]

        def layout(bits, prefix, shift, out):
            split = {24: (8, 16), 40: (8, 32), 48: (16, 32), 56: (8, 48), 72: (8, 64), 80: (16, 64), 88: (8, 80),
                     96: (32, 64), 104: (8, 96), 112: (16, 96), 120: (24, 96), 128: (64, 64)}
            if bits in (8, 16, 32, 64):
                out.append((prefix, bits // 8, shift))
                return
            ub, lb = split[bits]
            layout(ub, prefix + ".upr", shift + lb, out)
            layout(lb, prefix + ".lwr", shift, out)

        keep = []

        def run(base):
            h = struct.unpack("<8Q", files[base + ".header"][:64])
            r = SparseRun()
            r.D, r.count = h[1], h[7]
            hb = files[base + ".high-bits"]
            keep.append(hb)
            r.high_bits, r.high_words = hb, len(hb) // 8
            cols = []
            layout(h[2], "", 0, cols)
            r.ncols = len(cols)
            for i, (suffix, nbytes, shift) in enumerate(cols):
                data = files[base + ".low-bits" + suffix] or b"\0"
                keep.append(data)
                r.col[i], r.col_bytes[i], r.col_shift[i] = data, nbytes, shift
            return r

        edges = run("-edges")
        v = Vba()
        v.ord0, v.ord0_bytes = files["-counts.ord0"] or b"\0", len(files["-counts.ord0"])
        v.ord1p = run("-counts.ord1p")
        v.ord1, v.ord1_bytes = files["-counts.ord1"] or b"\0", len(files["-counts.ord1"])
        v.ord2p = run("-counts.ord2p")
        v.ord2, v.ord2_bytes = files["-counts.ord2"] or b"\0", len(files["-counts.ord2"])
        self._L.goss_gpu_push_run_graph.argtypes = [C.c_void_p, C.POINTER(SparseRun), C.POINTER(Vba)]
        self._check(self._L.goss_gpu_push_run_graph(self._h, C.byref(edges), C.byref(v)))

    def set_path(self, path):
        """0: segment hash path with LSD fallback (default); 1: LSD radix sort only."""
        self._check(self._L.goss_gpu_set_path(self._h, path))

    def reset(self):
        self._check(self._L.goss_gpu_reset(self._h))

    def set_budget_limit(self, max_bytes):
        """Let the arena grow up to max_bytes when a chunk or a merge needs it (goss_gpu_set_budget_limit)."""
        self._L.goss_gpu_set_budget_limit.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_set_budget_limit(self._h, max_bytes))

    def set_deferred(self, on=True):
        """goss_gpu_set_deferred: host pushes only stage; a full staging buffer is reported (GOSS_ERR_BUFFER)."""
        self._L.goss_gpu_set_deferred.argtypes = [C.c_void_p, C.c_int]
        self._check(self._L.goss_gpu_set_deferred(self._h, 1 if on else 0))

    def stage_room(self):
        """goss_gpu_stage_room -> (bytes the staging buffer still takes, its capacity)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._L.goss_gpu_stage_room.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_stage_room(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stat(self, name):
        """A diagnostic counter of the context (goss_gpu_stat)."""
        v = C.c_uint64()
        self._L.goss_gpu_stat.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_stat(self._h, name.encode(), C.byref(v)))
        return v.value

    def finish(self):
        c = Counts()
        self._check(self._L.goss_gpu_finish(self._h, C.byref(c)))
        self.counts = c
        return c

    def result_ptrs(self):
        k, v, m = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self._L.goss_gpu_result(self._h, C.byref(k), C.byref(v), C.byref(m)))
        return k.value, v.value, m.value

    def result(self):
        """(keys as python ints, counts) copied to the host."""
        import numpy as np
        m = self.counts.distinct
        w = self.counts.key_words
        keys = np.zeros(max(1, m * w), dtype=np.uint64)
        cnts = np.zeros(max(1, m), dtype=np.uint32)
        self._check(self._L.goss_gpu_result_copy(self._h, 0, m, keys.ctypes.data_as(C.c_void_p), cnts.ctypes.data_as(C.c_void_p)))
        keys = keys[: m * w]
        cnts = cnts[:m]
        if w == 1:
            ks = keys.tolist()
        else:
            ks = [l | (h << 64) for l, h in zip(keys[0::2].tolist(), keys[1::2].tolist())]
        return ks, cnts

    def big_counts(self):
        """{key: exact count} of the keys that occurred 2^32 - 1 times or more (goss_gpu_big_counts)."""
        self._L.goss_gpu_big_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]
        n = C.c_uint32()
        keys = (C.c_uint64 * 512)()
        counts = (C.c_uint64 * 256)()
        self._check(self._L.goss_gpu_big_counts(self._h, keys, counts, 256, C.byref(n)))
        return {int(keys[2 * i]) | (int(keys[2 * i + 1]) << 64): int(counts[i]) for i in range(min(n.value, 256))}

    def select_counts(self, lo, hi):
        """Between finish and emit: keep the result items whose count lies in [lo, hi]
        (goss_gpu_select_counts: the set algebra of intersect-kmer-sets / subtract-kmer-set)."""
        self._L.goss_gpu_select_counts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        self._check(self._L.goss_gpu_select_counts(self._h, lo, hi))

    def select_normal(self):
        """Between finish and emit: keep the items that are their own canonical form (goss_gpu_select_normal)."""
        self._L.goss_gpu_select_normal.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_select_normal(self._h))

    def emit_device(self):
        """Build the on-disk arrays in HBM without copying them to the host."""
        self._check(self._L.goss_gpu_emit(self._h))

    def emit(self):
        self.emit_device()
        return self.files()

    def emit_estimate(self, m):
        """emit with the SparseArray size estimate M = m instead of the exact count (goss_gpu_emit_estimate: what the
        merges and graph-to-kmer-set build with)."""
        self._L.goss_gpu_emit_estimate.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_emit_estimate(self._h, m))
        return self.files()

    def emit_count_bits(self, mask, suffix):
        """After emit: append the file `suffix`, one bit per result item, set where count & mask != 0
        (goss_gpu_emit_count_bits: the .lhs-bits / .rhs-bits of merge-and-annotate-kmer-sets)."""
        self._L.goss_gpu_emit_count_bits.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
        self._check(self._L.goss_gpu_emit_count_bits(self._h, mask, suffix.encode()))
        return self.files()

    def emit_dump(self, flags=0):
        """After finish: the text form of the object as the one file ".dump" (goss_gpu_emit_dump)."""
        self._L.goss_gpu_emit_dump.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self._L.goss_gpu_emit_dump(self._h, flags))
        return self.files()

    def emit_dump_range(self, flags, first, count):
        """The text of elements [first, first + count) only, the header lines in front of the piece that starts at 0
        (goss_gpu_emit_dump_range)."""
        self._L.goss_gpu_emit_dump_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
        self._check(self._L.goss_gpu_emit_dump_range(self._h, flags, first, count))
        return self.files()

    def emit_part(self, first_index, total, estimate=0, prev_last_high=None):
        """Distributed emission, this range's part (goss_gpu_emit_part; with prev_last_high -- the high part of the last
        key of the ranges below, emit_last_high of their owners -- goss_gpu_emit_part_ranges: "-d0" blocks too)."""
        if prev_last_high is None:
            self._L.goss_gpu_emit_part.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
            self._check(self._L.goss_gpu_emit_part(self._h, first_index, total, estimate))
        else:
            self._L.goss_gpu_emit_part_ranges.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
            self._check(self._L.goss_gpu_emit_part_ranges(self._h, first_index, total, estimate, prev_last_high))

    def emit_last_high(self, total, estimate=0):
        """goss_gpu_emit_last_high -> (high part of this range's last key, range is not empty)"""
        h, ne = C.c_uint64(), C.c_int()
        self._L.goss_gpu_emit_last_high.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        self._check(self._L.goss_gpu_emit_last_high(self._h, total, estimate, C.byref(h), C.byref(ne)))
        return h.value, bool(ne.value)

    def emit_assemble(self, spans_ptr, span_bytes, total, estimate=0, big=b"", hist=b""):
        """Distributed emission, the files that need all ranges (goss_gpu_emit_assemble): spans_ptr =
        device address of the ranges' ".part.span" files back to back (span_bytes in all), big / hist = the
        concatenated records (bytes)."""
        self._L.goss_gpu_emit_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                                   C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
        _torch_ready()
        self._check(self._L.goss_gpu_emit_assemble(self._h, C.c_void_p(spans_ptr), span_bytes, total, estimate,
                                                   big, len(big) // 16, hist, len(hist) // 16))

    def file_list(self):
        """[(suffix, size, device address or None)] of the emitted files"""
        self._L.goss_gpu_file_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        n = C.c_uint32()
        self._check(self._L.goss_gpu_file_count(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            name = C.create_string_buffer(256)
            size = C.c_uint64()
            self._check(self._L.goss_gpu_file_info(self._h, i, name, 256, C.byref(size)))
            p = C.c_void_p()
            self._check(self._L.goss_gpu_file_device(self._h, i, C.byref(p)))
            out.append((name.value.decode(), size.value, p.value))
        return out

    def read_file(self, suffix):
        """bytes of one emitted file"""
        for i, (name, size, _) in enumerate(self.file_list()):
            if name == suffix:
                buf = C.create_string_buffer(max(1, size))
                self._check(self._L.goss_gpu_file_read(self._h, i, 0, buf, size))
                return buf.raw[:size]
        raise KeyError(suffix)

    def emit_sparse_array(self, dev_ptr, key_words, n, N, M, N_end=None):
        if N_end is None:
            N_end = N
        mask = (1 << 64) - 1
        _torch_ready()
        self._check(self._L.goss_gpu_emit_sparse_array(self._h, C.c_void_p(dev_ptr), key_words, n, N & mask, N >> 64, M,
                                                       N_end & mask, N_end >> 64))
        return self.files()

    def lint(self, asymmetric=False, examples=False):
        """goss_gpu_lint on the finished graph: dict of the problem counts of lint-graph's pass 1; with `examples` also
        "nexamples" and "examples", the (index, kind, other) of the offending edges the report holds (32 at the most)."""
        class LintReport(C.Structure):
            _fields_ = [("missing_rc", C.c_uint64), ("count_mismatch", C.c_uint64), ("zero_count", C.c_uint64),
                        ("order_violation", C.c_uint64), ("nexamples", C.c_uint32), ("pad", C.c_uint32),
                        ("ex_index", C.c_uint64 * 32), ("ex_other", C.c_uint64 * 32), ("ex_kind", C.c_uint32 * 32)]
        rep = LintReport()
        self._L.goss_gpu_lint.argtypes = [C.c_void_p, C.c_int, C.POINTER(LintReport)]
        self._check(self._L.goss_gpu_lint(self._h, 1 if asymmetric else 0, C.byref(rep)))
        out = {"missing_rc": rep.missing_rc, "count_mismatch": rep.count_mismatch, "zero_count": rep.zero_count,
               "order_violation": rep.order_violation}
        if examples:
            out["nexamples"] = rep.nexamples
            out["examples"] = [(int(rep.ex_index[i]), int(rep.ex_kind[i]), int(rep.ex_other[i])) for i in range(min(rep.nexamples, 32))]
        return out

    def prune_tips(self, iterations=1):
        """Between finish and emit, graph mode: `iterations` rounds of prune-tips on the device (goss_gpu_prune_tips).
        The context's result becomes the pruned graph; returns one report dict per iteration."""
        class TipsReport(C.Structure):
            _fields_ = [(name, C.c_uint64) for name in TIPS_REPORT_FIELDS]
        reps = (TipsReport * max(1, iterations))()
        self._L.goss_gpu_prune_tips.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(TipsReport)]
        self._check(self._L.goss_gpu_prune_tips(self._h, iterations, reps))
        if iterations and getattr(self, "counts", None) is not None:
            self.counts.distinct = int(reps[iterations - 1].edges_after)       # what result() copies
        return [{name: int(getattr(reps[i], name)) for name in TIPS_REPORT_FIELDS} for i in range(iterations)]

    def _paths_pass(self, fn, fields, *args):
        class Report(C.Structure):
            _fields_ = [(name, C.c_uint64) for name in fields]
        rep = Report()
        fn.argtypes = [C.c_void_p] + [C.c_uint32] * len(args) + [C.POINTER(Report)]
        self._check(fn(self._h, *args, C.byref(rep)))
        if getattr(self, "counts", None) is not None:
            self.counts.distinct = int(rep.edges_after)                        # what result() copies
        return {name: int(getattr(rep, name)) for name in fields}

    def trim_paths(self, cutoff=None):
        """Between finish and emit, graph mode: one pass of trim-paths on the device (goss_gpu_trim_paths): every path
        of at most 2K edges that starts at a node without incoming edges goes.  `cutoff` spares a path that holds an
        edge of that multiplicity or more (GOSS_PATHS_CUTOFF); None leaves the flag clear, as the reference's command
        does whatever -C says.  The context's result becomes the trimmed graph; returns the report dict."""
        if cutoff is None:
            return self._paths_pass(self._L.goss_gpu_trim_paths, PATHS_REPORT_FIELDS, 0, 0)
        return self._paths_pass(self._L.goss_gpu_trim_paths, PATHS_REPORT_FIELDS, PATHS_CUTOFF, cutoff)

    def clip_links(self):
        """Between finish and emit, graph mode: one pass of clip-links on the device (goss_gpu_clip_links): every path
        of at most 2K edges that leaves a fork and enters a join as a minor branch (under a third of the node's
        multiplicity) goes.  The context's result becomes the clipped graph; returns the report dict."""
        return self._paths_pass(self._L.goss_gpu_clip_links, LINKS_REPORT_FIELDS, 0)

    def paths_timing(self):
        """{phase: ms} of the last trim_paths / clip_links pass: link, flag, gather, walk, compact (goss_gpu_paths_timing)"""
        ms = (C.c_float * 5)()
        self._L.goss_gpu_paths_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(self._L.goss_gpu_paths_timing(self._h, ms))
        return dict(zip(("link", "flag", "gather", "walk", "compact"), (float(x) for x in ms)))

    def _relative_pass(self, fn, fields, arg):
        class Report(C.Structure):
            _fields_ = [(name, C.c_uint64) for name in fields]
        rep = Report()
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, type(arg), C.POINTER(Report)]
        self._check(fn(self._h, arg, C.byref(rep)))
        if getattr(self, "counts", None) is not None:
            self.counts.distinct = int(rep.edges_after)                        # what result() copies
        return {name: int(getattr(rep, name)) for name in fields}

    def trim_relative(self, rel=0.02):
        """Between finish and emit, graph mode: trim-relative on the device (goss_gpu_trim_relative): at every node with
        two or more outgoing edges, an edge whose multiplicity is below `rel` times the node's sum goes, and its reverse
        complement with it.  The context's result becomes the trimmed graph; returns the report dict."""
        return self._relative_pass(self._L.goss_gpu_trim_relative, RELATIVE_REPORT_FIELDS, C.c_double(rel))

    def recount_from(self, obj):
        """Between finish and emit, graph mode: merge-graph-with-reference on the device (goss_gpu_recount_from): the
        edges that the open graph `obj` holds too stay, with its multiplicities.  The context's result becomes the
        merged graph; emit_estimate(report["edges_before"]) writes the reference's files.  Returns the report dict."""
        return self._relative_pass(self._L.goss_gpu_recount_from, RECOUNT_REPORT_FIELDS, C.c_void_p(obj._h.value))

    def relative_timing(self):
        """{phase: ms} of the last trim_relative (judge, mirror, compact) or recount_from (judge = the lookup, mirror 0,
        compact) pass (goss_gpu_relative_timing)"""
        ms = (C.c_float * 3)()
        self._L.goss_gpu_relative_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(self._L.goss_gpu_relative_timing(self._h, ms))
        return dict(zip(("judge", "mirror", "compact"), (float(x) for x in ms)))

    def segments_build(self, min_length=0, min_coverage=0, line_breaks=True):
        """Between finish and emit, graph mode: build the linear segments on the device (goss_gpu_segments_build) and
        hold them; returns the info dict.  segments_table / segments_text read them, segments_release gives them back."""
        inf = SegmentsInfo()
        self._L.goss_gpu_segments_build.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(SegmentsInfo)]
        self._check(self._L.goss_gpu_segments_build(self._h, min_length, min_coverage,
                                                    0 if line_breaks else SEGMENTS_NO_LINE_BREAKS, C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in SEGMENTS_INFO_FIELDS}

    def segments_table(self, first, count):
        import numpy as np
        out = np.zeros(count, dtype=SEGMENT_DTYPE)
        self._L.goss_gpu_segments_table.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_segments_table(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def segments_text(self, offset, nbytes):
        buf = C.create_string_buffer(max(1, nbytes))
        self._L.goss_gpu_segments_text.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p]
        self._check(self._L.goss_gpu_segments_text(self._h, offset, nbytes, buf))
        return buf.raw[:nbytes]

    def segments_release(self):
        self._L.goss_gpu_segments_release.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_segments_release(self._h))

    def linear_segments(self, min_length=0, min_coverage=0, line_breaks=True):
        """The linear segments of the graph, as `goss print-contigs` numbers them: (table, text, info).  table is a
        numpy structured array (SEGMENT_DTYPE), one row per segment in printing order; text holds the bodies back to
        back, row["text_offset"] / row["text_bytes"] say where.  The context's result is untouched."""
        info = self.segments_build(min_length, min_coverage, line_breaks)
        try:
            table = self.segments_table(0, info["segments"])
            text = self.segments_text(0, info["text_bytes"])
        finally:
            self.segments_release()
        return table, text, info

    def contigs(self, min_length=0, min_coverage=0, line_breaks=True, verbose_headers=False, sequence=True):
        """Exactly the bytes `goss print-contigs` writes for the graph the context holds."""
        table, text, _ = self.linear_segments(min_length, min_coverage, line_breaks)
        out = []
        if not sequence:
            out.append(b"Number\tLength\tMinCov\tMaxCov\tMeanCov\tStdDevCov\n")
        for no, row in enumerate(table, 1):
            if not sequence:
                out.append(("%d\t%d\t%d\t%d\t%s\t%s\n" % ((no,) + segment_stats(row, self.k))).encode())
                continue
            head = ">%d" % no
            if verbose_headers:
                head += " %d:%d:%d:%s:%s" % segment_stats(row, self.k)
            out.append(head.encode() + b"\n")
            o = int(row["text_offset"])
            out.append(text[o:o + int(row["text_bytes"])])
        return b"".join(out)

    def entries_build(self):
        """Between finish and emit, graph mode: build the graph's EntryEdgeSet on the device (goss_gpu_entries_build)
        and hold its images as the context's file list ("-entries.*"); returns the info dict.  files() / read_file()
        read them, Object.from_context opens them, entries_release gives them back."""
        inf = EntriesInfo()
        self._L.goss_gpu_entries_build.argtypes = [C.c_void_p, C.POINTER(EntriesInfo)]
        self._check(self._L.goss_gpu_entries_build(self._h, C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in ENTRIES_INFO_FIELDS}

    def entries_release(self):
        self._L.goss_gpu_entries_release.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_entries_release(self._h))

    def entry_edge_set(self):
        """The EntryEdgeSet of the graph, as `goss build-entry-edge-set` writes it: ({name: bytes}, info), the names
        as on disk less the graph's name ("-entries.header", "-entries.edges.high-bits", ...).  The context's result
        is untouched."""
        info = self.entries_build()
        try:
            files = self.files()
        finally:
            self.entries_release()
        return files, info

    def mark_reads(self, bases):
        """Between finish and emit, graph mode: mark the edges that the forward (K+1)-windows of the reads in `bases`
        (bytes, '\\n' between reads) touch (goss_gpu_components_mark_host); the marks add up over the calls and are
        held until components_release or any call that gives back a held result.  Returns the info dict."""
        inf = MarkInfo()
        self._L.goss_gpu_components_mark_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(MarkInfo)]
        self._check(self._L.goss_gpu_components_mark_host(self._h, bases, len(bases), C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in MARK_INFO_FIELDS}

    def components(self, marked=False):
        """The connected components of the graph -- of the marked edges with marked=True -- as `goss count-components`
        numbers them: (info dict, numpy structured array of the table, COMPONENT_DTYPE) with the true figures (the
        reference's rows count the start edge twice).  The labels and the table stay held for component_labels."""
        import numpy as np
        inf = ComponentsInfo()
        self._L.goss_gpu_components_build.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ComponentsInfo)]
        self._check(self._L.goss_gpu_components_build(self._h, COMPONENTS_MARKED if marked else 0, C.byref(inf)))
        table = np.zeros(inf.components, dtype=COMPONENT_DTYPE)
        self._L.goss_gpu_components_table.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_components_table(self._h, 0, inf.components, table.ctypes.data_as(C.c_void_p)))
        return {name: getattr(inf, name) for name, _ in COMPONENTS_INFO_FIELDS}, table

    def component_labels(self, first=0, count=None):
        """The component index of every edge after components(): np.uint32[M], COMPONENT_NONE where unmarked."""
        import numpy as np
        if count is None:
            count = self.result_ptrs()[2] - first
        out = np.zeros(count, dtype=np.uint32)
        self._L.goss_gpu_components_labels.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_components_labels(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def keep_component(self, edge_rank):
        """The result becomes the whole-graph component of the edge of that rank and that of its reverse complement
        (goss_gpu_components_keep); returns the number of edges kept."""
        kept = C.c_uint64()
        self._L.goss_gpu_components_keep.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_components_keep(self._h, edge_rank, C.byref(kept)))
        if getattr(self, "counts", None) is not None:
            self.counts.distinct = int(kept.value)       # what result() copies
        return int(kept.value)

    def grow_marks(self, radius=1, linear_paths=False):
        """After mark_reads: the marks take in their mirror image and grow by `radius` passes as `goss build-subgraph`
        grows them -- by nodes, or with linear_paths by linear paths (goss_gpu_components_grow).  Returns (info dict,
        added): added[i] = the edges pass i brought, 0 for the passes that were not run because nothing could follow.
        The marks stay held; components(marked=True), marks() and keep_marked() work on them."""
        inf = GrowInfo()
        added = (C.c_uint64 * max(radius, 1))()
        self._L.goss_gpu_components_grow.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(GrowInfo)]
        self._check(self._L.goss_gpu_components_grow(self._h, radius, GROW_LINEAR_PATHS if linear_paths else 0, added, C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in GROW_INFO_FIELDS}, [int(a) for a in added[:radius]]

    def marks(self, first=0, count=None):
        """The marks as they are now: np.bool_[M], one per edge in rank order (goss_gpu_components_marks)."""
        import numpy as np
        if count is None:
            count = self.result_ptrs()[2] - first
        out = np.zeros(count, dtype=np.uint8)
        self._L.goss_gpu_components_marks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_components_marks(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out.astype(np.bool_)

    def keep_marked(self):
        """The result becomes its marked edges (goss_gpu_components_keep_marked); what was held is given back.
        Returns the number of edges kept; a following emit() writes the subgraph."""
        kept = C.c_uint64()
        self._L.goss_gpu_components_keep_marked.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_components_keep_marked(self._h, C.byref(kept)))
        if getattr(self, "counts", None) is not None:
            self.counts.distinct = int(kept.value)       # what result() copies
        return int(kept.value)

    def components_release(self):
        self._L.goss_gpu_components_release.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_components_release(self._h))

    # ---- read links (include/goss_gpu_links.h) --------------------------------------------------------------------

    def read_links_begin(self, unique=None, carry=True):
        """Between finish and emit, graph mode: build and hold the segment of every edge (goss_gpu_read_links_begin).
        unique: a truth value per entry rank, or None for "every segment is unique".  Returns the info dict."""
        import numpy as np
        inf = ReadLinksInfo()
        bits, nbits = None, 0
        if unique is not None:
            u = np.asarray(unique, dtype=np.bool_)
            nbits = len(u)
            bits = np.packbits(u, bitorder="little").tobytes() + b"\0"
        self._L.goss_gpu_read_links_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(ReadLinksInfo)]
        self._check(self._L.goss_gpu_read_links_begin(self._h, LINKS_CARRY if carry else 0, bits, nbits, C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in READ_LINKS_INFO_FIELDS if name != "reserved"}

    def read_links_release(self):
        self._L.goss_gpu_read_links_release.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_read_links_release(self._h))

    def read_links_segments(self, first=0, count=None):
        """After read_links_begin: np.uint32 per edge of rank [first, first + count), LINK_NONE where it has no segment."""
        import numpy as np
        if count is None:
            count = self.result_ptrs()[2] - first
        out = np.zeros(count, dtype=np.uint32)
        self._L.goss_gpu_read_links_segments.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_read_links_segments(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_links_windows(self, bases):
        """After read_links_begin: (np.uint32 per window of the batch in read order, info dict)
        (goss_gpu_read_links_windows_host)."""
        import numpy as np
        inf = ReadLinksBatch()
        out = np.zeros(max(len(bases), 1), dtype=np.uint32)
        self._L.goss_gpu_read_links_windows_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                             C.POINTER(ReadLinksBatch)]
        self._check(self._L.goss_gpu_read_links_windows_host(self._h, bases, len(bases), out.ctypes.data_as(C.c_void_p), len(out),
                                                             C.byref(inf)))
        return out[:inf.windows].copy(), {name: getattr(inf, name) for name, _ in READ_LINKS_BATCH_FIELDS if name != "reserved"}

    def read_links_add(self, bases):
        """After read_links_begin: the records of one batch of whole reads join those held (goss_gpu_read_links_add_host);
        returns the info dict."""
        inf = ReadLinksBatch()
        self._L.goss_gpu_read_links_add_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(ReadLinksBatch)]
        self._check(self._L.goss_gpu_read_links_add_host(self._h, bases, len(bases), C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in READ_LINKS_BATCH_FIELDS if name != "reserved"}

    def read_links_table(self):
        """After read_links_begin: reduce the records held (goss_gpu_read_links_finish) and return (LINK_DTYPE array
        ascending by (a, b), info dict).  The records stay: more batches may follow, and a second call answers alike."""
        import numpy as np
        inf = ReadLinksTableInfo()
        self._L.goss_gpu_read_links_finish.argtypes = [C.c_void_p, C.POINTER(ReadLinksTableInfo)]
        self._check(self._L.goss_gpu_read_links_finish(self._h, C.byref(inf)))
        table = np.zeros(inf.rows, dtype=LINK_DTYPE)
        self._L.goss_gpu_read_links_table.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self._L.goss_gpu_read_links_table(self._h, 0, inf.rows, table.ctypes.data_as(C.c_void_p)))
        return table, {name: getattr(inf, name) for name, _ in READ_LINKS_TABLE_FIELDS}

    def segment_of_edges(self):
        """The segment of every edge of the graph: np.uint32[M], the entry rank of the linear path that holds the edge,
        LINK_NONE on a cycle without an entry edge.  The context's result is untouched; nothing stays held."""
        self.read_links_begin(carry=False)
        try:
            return self.read_links_segments()
        finally:
            self.read_links_release()

    def thread_windows(self, bases, unique=None, carry=True):
        """The read-to-path primitive: per forward (K+1)-window of the reads in `bases` (bytes, '\\n' between reads), in
        read order, the segment it is aligned to -- | LINK_NON_UNIQUE where `unique` says so -- or LINK_MISS.  carry=True
        is the aligner of the reference's thread-reads, carry=False the exact answer (include/goss_gpu_links.h).  The
        context's result is untouched; nothing stays held."""
        self.read_links_begin(unique, carry)
        try:
            return self.read_links_windows(bases)[0]
        finally:
            self.read_links_release()

    def read_links(self, batches, unique=None, carry=True):
        """The link table of the reads in `batches` (an iterable of bytes, whole reads each): LINK_DTYPE rows
        (a, b, count, gap_sum) ascending by (a, b), 64-bit sums.  The context's result is untouched; nothing stays held."""
        self.read_links_begin(unique, carry)
        try:
            for bases in batches:
                self.read_links_add(bases)
            return self.read_links_table()[0]
        finally:
            self.read_links_release()

    def pool_begin(self, nsets, z):
        """goss_gpu_pool_begin: zeroed bit rows of nsets samples over a union of z k-mers, held by the context"""
        self._L.goss_gpu_pool_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        self._check(self._L.goss_gpu_pool_begin(self._h, nsets, z))
        self._pool_sets = nsets

    def pool_add_masks(self, first_set, nbits, masks_ptr, z):
        """goss_gpu_pool_add_masks: masks_ptr is a device pointer to z u32 (bit i: the k-mer is in sample first_set + i)"""
        self._L.goss_gpu_pool_add_masks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
        _torch_ready()
        self._check(self._L.goss_gpu_pool_add_masks(self._h, first_set, nbits, C.c_void_p(masks_ptr), z))

    def pool_sizes(self):
        """the k-mers of every sample: a list of ints"""
        n = getattr(self, "_pool_sets", 1)          # (without a begin the library refuses before it writes)
        out = (C.c_uint64 * n)()
        self._L.goss_gpu_pool_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_pool_sizes(self._h, out))
        return [int(x) for x in out]

    def pool_intersections(self):
        """the common k-mers of every pair of samples: nsets lists of nsets ints, symmetric, the diagonal the sizes"""
        n = getattr(self, "_pool_sets", 1)          # (without a begin the library refuses before it writes)
        out = (C.c_uint64 * (n * n))()
        self._L.goss_gpu_pool_intersections.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self._L.goss_gpu_pool_intersections(self._h, out))
        return [[int(out[i * n + j]) for j in range(n)] for i in range(n)]

    def pool_emit_index(self):
        """goss_gpu_pool_emit_index: the files of the <out>-index SparseArray as {suffix: bytes}"""
        self._L.goss_gpu_pool_emit_index.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_pool_emit_index(self._h))
        return self.files()

    def pool_release(self):
        self._L.goss_gpu_pool_release.argtypes = [C.c_void_p]
        self._check(self._L.goss_gpu_pool_release(self._h))

    def check_index(self, files, base=""):
        """goss_gpu_check_index on a SparseArray given as {suffix: bytes} (files[base + ".header"]
        ...): the context must hold the array's decoded elements (push_run + finish).  Returns a
        dict of the mismatch counts."""
        import struct

        def layout(bits, prefix, shift, out):
            # IntegerArray::builder column files (IntegerArray.cc:259-357)
            split = {24: (8, 16), 40: (8, 32), 48: (16, 32), 56: (8, 48), 72: (8, 64), 80: (16, 64), 88: (8, 80),
                     96: (32, 64), 104: (8, 96), 112: (16, 96), 120: (24, 96), 128: (64, 64)}
            if bits in (8, 16, 32, 64):
                out.append((prefix, bits // 8, shift))
                return
            ub, lb = split[bits]
            layout(ub, prefix + ".upr", shift + lb, out)
            layout(lb, prefix + ".lwr", shift, out)

        class SparseFiles(C.Structure):
            _fields_ = [("D", C.c_uint64), ("count", C.c_uint64), ("size_lo", C.c_uint64), ("size_hi", C.c_uint64),
                        ("high_bits", C.c_char_p), ("high_words", C.c_uint64),
                        ("d0", C.c_char_p), ("d0_bytes", C.c_uint64), ("d1", C.c_char_p), ("d1_bytes", C.c_uint64),
                        ("ncols", C.c_uint32), ("pad", C.c_uint32),
                        ("col", C.c_char_p * 4), ("col_bytes", C.c_uint32 * 4), ("col_shift", C.c_uint32 * 4)]

        class IndexReport(C.Structure):
            _fields_ = [("select_mismatch", C.c_uint64), ("rank_mismatch", C.c_uint64), ("access_miss", C.c_uint64),
                        ("failures", C.c_uint64), ("nexamples", C.c_uint32), ("pad", C.c_uint32),
                        ("ex_index", C.c_uint64 * 16), ("ex_kind", C.c_uint32 * 16)]

        h = struct.unpack("<8Q", files[base + ".header"][:64])
        f = SparseFiles()
        f.D, qd, f.size_lo, f.size_hi, f.count = h[1], h[2], h[5], h[6], h[7]
        hb = files[base + ".high-bits"]
        f.high_bits, f.high_words = hb, len(hb) // 8
        f.d0, f.d0_bytes = files[base + "-d0"], len(files[base + "-d0"])
        f.d1, f.d1_bytes = files[base + "-d1"], len(files[base + "-d1"])
        cols = []
        layout(qd, "", 0, cols)
        f.ncols = len(cols)
        for i, (suffix, nbytes, shift) in enumerate(cols):
            f.col[i] = files[base + ".low-bits" + suffix] or b"\0"
            f.col_bytes[i] = nbytes
            f.col_shift[i] = shift
        rep = IndexReport()
        self._L.goss_gpu_check_index.argtypes = [C.c_void_p, C.POINTER(SparseFiles), C.POINTER(IndexReport)]
        self._check(self._L.goss_gpu_check_index(self._h, C.byref(f), C.byref(rep)))
        return {"select": rep.select_mismatch, "rank": rep.rank_mismatch, "access": rep.access_miss, "failures": rep.failures,
                "examples": [(rep.ex_index[i], rep.ex_kind[i]) for i in range(rep.nexamples)]}

    def files(self):
        n = C.c_uint32()
        self._check(self._L.goss_gpu_file_count(self._h, C.byref(n)))
        out = {}
        for i in range(n.value):
            name = C.create_string_buffer(256)
            size = C.c_uint64()
            self._check(self._L.goss_gpu_file_info(self._h, i, name, 256, C.byref(size)))
            buf = C.create_string_buffer(max(1, size.value))
            self._check(self._L.goss_gpu_file_read(self._h, i, 0, buf, size.value))
            out[name.value.decode()] = buf.raw[: size.value]
        return out

    def timing(self, reset=False):
        t = Timing()
        self._check(self._L.goss_gpu_timing_get(self._h, C.byref(t)))
        if reset:
            self._check(self._L.goss_gpu_timing_reset(self._h))
        return t

    def synth_reads(self, dev_ptr, nreads, read_len, genome_len, seed=1, first_read=0):
        self._check(self._L.goss_gpu_synth_reads(self._h, C.c_void_p(dev_ptr), nreads, read_len, genome_len, seed, first_read))


# ---- objects opened for queries (goss_gpu_object_*) ------------------------------------------

OBJECT_KMER_SET, OBJECT_GRAPH, OBJECT_SPARSE_ARRAY, OBJECT_ENTRY_EDGE_SET = 0, 1, 2, 3
QUERY_NORMALIZE, QUERY_INCOMING = 1, 2
MATCH_NORMALIZE, MATCH_ANY = 1, 4
NEAR_WHOLE_BASES, NEAR_NORMALIZE = 1, 2          # Object.near_kmers: the two departures from the reference's loop
CLASSIFY_NORMALIZE = 1                           # Object.classify_reads: look up each window's canonical form
ELECT_NORMALIZE = 1                              # Object.colour_reads: look up each window's canonical form
ELECT_MAX_COLOURS = 64                           # Object.colours: the references a colour word can speak of
TAXO_NORMALIZE = 1                               # Object.taxo_annotate / taxo_classify_reads: canonical windows
TAXO_NONE, TAXO_MANY = 0xFFFFFFFF, 0xFFFFFFFE    # Object.taxo_classify_reads: no class / classes on more than one path
ERR_BUFFER = -9


def encode_kmers(strings, k):
    """2-bit codes of k-mer strings (A=0 C=1 G=2 T=3, first base most significant; either case): a numpy uint64
    array of n values when 2k <= 62, else of n {lo, hi} rows -- the key layout of the C ABI."""
    import numpy as np
    strings = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    if any(len(s) != k for s in strings):
        raise ValueError("every k-mer must have %d bases" % k)
    lut = np.full(256, 255, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        lut[ch] = v
    codes = lut[np.frombuffer(b"".join(strings), dtype=np.uint8)].reshape(len(strings), k).astype(np.uint64)
    if (codes == 255).any():
        raise ValueError("a k-mer holds a character other than ACGT")
    shift = 2 * (k - 1 - np.arange(k, dtype=np.uint64))            # bit position of each base

    def word(sel, sub):
        if not sel.any():
            return np.zeros(len(strings), dtype=np.uint64)
        return np.bitwise_or.reduce(codes[:, sel] << (shift[sel] - np.uint64(sub)), axis=1).astype(np.uint64)
    if 2 * k <= 62:
        return word(np.ones(k, dtype=bool), 0)
    lo, hi = word(shift < 64, 0), word(shift >= 64, 64)
    return np.ascontiguousarray(np.stack([lo, hi], axis=1))


class ObjectDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("K", C.c_uint32), ("count", C.c_uint64), ("key_words", C.c_uint32),
                ("asymmetric", C.c_uint32), ("N_lo", C.c_uint64), ("N_hi", C.c_uint64), ("D", C.c_uint64),
                ("resident_bytes", C.c_uint64)]


class NamedFile(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("bytes", C.c_uint64)]


class MatchInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("windows", C.c_uint64), ("hits", C.c_uint64), ("matched_reads", C.c_uint64),
                ("ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ClassifyInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("windows", C.c_uint64), ("counts", C.c_uint64 * 16), ("ms", C.c_float)]

    def as_dict(self):
        return {"reads": self.reads, "windows": self.windows, "counts": list(self.counts), "ms": self.ms}


class ElectInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("windows", C.c_uint64), ("by_count", C.c_uint64 * 65), ("ms", C.c_float)]

    def as_dict(self):
        return {"reads": self.reads, "windows": self.windows, "by_count": list(self.by_count), "ms": self.ms}


def elect(colours, windows, threshold, pairs=False, numeric_second_mate=True):
    """The decision of `electus classify` (KmerFilter, ElectApp.cc:406-451) over what Object.colour_reads gave: a list of
    bools, one per read, or with pairs=True one per pair, the mates being reads 2i and 2i + 1.  A single read matches
    when it has a window and its word has at least `threshold` bits.  A pair matches when the first mate does, or when
    the second mate has a window and the OR of both words reaches the threshold -- as a number, which is what the
    reference compares (ElectApp.cc:443); numeric_second_mate=False counts that word's bits instead."""
    import numpy as np
    def ints(a):                                 # numpy, a torch tensor (int64 with the same bits) or a plain sequence
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        return [int(x) & 0xFFFFFFFFFFFFFFFF for x in (np.asarray(a).reshape(-1).tolist() if hasattr(a, "dtype") else a)]
    c, w = ints(colours), [x & 0xFFFFFFFF for x in ints(windows)]
    if len(c) != len(w):
        raise ValueError("colours and windows differ in length")
    t = int(threshold)

    def bits(x):
        return bin(x).count("1")
    if not pairs:
        return [wi >= 1 and bits(ci) >= t for ci, wi in zip(c, w)]
    if len(c) % 2:
        raise ValueError("pairs need an even number of reads")
    out = []
    for i in range(0, len(c), 2):
        both = c[i] | c[i + 1]
        out.append((w[i] >= 1 and bits(c[i]) >= t) or (w[i + 1] >= 1 and (both if numeric_second_mate else bits(both)) >= t))
    return out


class TaxoInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("windows", C.c_uint64), ("hits", C.c_uint64), ("none", C.c_uint64), ("many", C.c_uint64),
                ("unannotated", C.c_uint64), ("ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def parse_phylogeny(text):
    """A phylogeny file -- a nested token list, "(" key value ... child ... ")" -- as {"anns": {key: value}, "kids": [...]}"""
    toks = text.decode() if isinstance(text, (bytes, bytearray)) else text
    toks = toks.split()
    stack, root, i = [], None, 0
    while i < len(toks):
        tok = toks[i]
        if tok == "(":
            node = {"anns": {}, "kids": []}
            if stack:
                stack[-1]["kids"].append(node)
            elif root is not None:
                raise ValueError("phylogeny: tokens after the root's ')'")
            else:
                root = node
            stack.append(node)
            i += 1
        elif tok == ")":
            if not stack:
                raise ValueError("phylogeny: ')' without '('")
            stack.pop()
            i += 1
        else:
            if not stack or stack[-1]["kids"] or i + 1 >= len(toks) or toks[i + 1] in ("(", ")"):
                raise ValueError("phylogeny: stray token %r" % tok)
            stack[-1]["anns"][tok] = toks[i + 1]
            i += 2
    if root is None or stack:
        raise ValueError("phylogeny: unbalanced")
    return root


def format_phylogeny(root):
    """The text AnnotTree::write makes of a parsed phylogeny: one space per depth, "(" on a line of its own, one
    key TAB value line per annotation in key order, the children in order, ")"."""
    out, todo = [], [(root, 0)]
    while todo:
        node, d = todo.pop()
        if node is None:
            out.append(" " * d + ")\n")
            continue
        out.append(" " * d + "(\n")
        out += [" " * (d + 1) + k + "\t" + node["anns"][k] + "\n" for k in sorted(node["anns"])]
        todo.append((None, d))
        todo += [(c, d + 1) for c in reversed(node["kids"])]
    return "".join(out)


def phylogeny_nodes(root, need=("node", "name")):
    """(nodes in file order, ids, parent_index) of a parsed phylogeny, as Object.taxo_tree takes them; a node without one
    of `need`, or with a node id that is no uint32, raises"""
    nodes, ids, parent, todo = [], [], [], [(root, None)]
    while todo:
        node, p = todo.pop()
        i = len(nodes)
        for k in need:
            if k not in node["anns"]:
                raise ValueError("phylogeny: node %d (in file order) has no '%s'" % (i, k))
        v = node["anns"]["node"]
        if not v.isdigit() or int(v) > 0xFFFFFFFF:
            raise ValueError("phylogeny: node %d (in file order) has the id %r" % (i, v))
        nodes.append(node)
        ids.append(int(v))
        parent.append(i if p is None else p)
        todo += [(c, i) for c in reversed(node["kids"])]
    return nodes, ids, parent


def _declare_object(L):
    if getattr(L, "_object_declared", False):
        return
    P, U64 = C.c_void_p, C.c_uint64
    L.goss_gpu_object_open.argtypes = [C.POINTER(P), C.c_int, P, C.c_int, C.c_char_p, C.POINTER(NamedFile), C.c_uint32]
    L.goss_gpu_object_open_emitted.argtypes = [C.POINTER(P), P]
    L.goss_gpu_object_close.argtypes = [P]
    L.goss_gpu_object_close.restype = None
    L.goss_gpu_object_last_error.argtypes = [P]
    L.goss_gpu_object_last_error.restype = C.c_char_p
    L.goss_gpu_object_info.argtypes = [P, C.POINTER(ObjectDesc)]
    L.goss_gpu_object_rank.argtypes = [P, P, U64, C.c_uint32, P, P]
    L.goss_gpu_object_select.argtypes = [P, P, U64, P]
    L.goss_gpu_object_multiplicity.argtypes = [P, P, U64, P]
    L.goss_gpu_object_lookup.argtypes = [P, P, U64, C.c_uint32, P]
    L.goss_gpu_object_node_ranks.argtypes = [P, P, U64, C.c_uint32, P, P]
    L.goss_gpu_object_match_reads.argtypes = [P, P, U64, C.c_uint32, U64, P, P, P, C.POINTER(MatchInfo)]
    L.goss_gpu_entries_length.argtypes = [P, P, U64, P]
    L.goss_gpu_entries_end_rank.argtypes = [P, P, U64, P]
    L.goss_gpu_object_near_kmers.argtypes = [P, P, P, C.c_uint32, P, P, C.POINTER(U64)]
    L.goss_gpu_object_near_kmers_host.argtypes = [P, P, P, C.c_uint32, P, P, C.POINTER(U64)]
    L.goss_gpu_object_classify_reads.argtypes = [P, P, U64, P, P, C.c_uint32, U64, P, P, P, C.POINTER(ClassifyInfo)]
    L.goss_gpu_object_classify_bits_host.argtypes = [P, P, P]
    L.goss_gpu_object_classify_reads_host.argtypes = [P, P, U64, C.c_uint32, U64, P, P, P, C.POINTER(ClassifyInfo)]
    L.goss_gpu_object_colours_host.argtypes = [P, P, C.c_uint32]
    L.goss_gpu_object_colours_from_index.argtypes = [P, P, C.POINTER(C.c_uint32)]
    L.goss_gpu_object_colour_reads.argtypes = [P, P, U64, C.c_uint32, U64, P, P, P, C.POINTER(ElectInfo)]
    L.goss_gpu_object_colour_reads_host.argtypes = [P, P, U64, C.c_uint32, U64, P, P, P, C.POINTER(ElectInfo)]
    U32 = C.c_uint32
    L.goss_gpu_object_taxo_tree_host.argtypes = [P, U32, P, P]
    L.goss_gpu_object_taxo_annotation_host.argtypes = [P, P]
    L.goss_gpu_object_taxo_annotation_read.argtypes = [P, P, P]
    L.goss_gpu_object_taxo_annotate.argtypes = [P, P, U64, P, U32, U64, P, C.POINTER(TaxoInfo)]
    L.goss_gpu_object_taxo_annotate_host.argtypes = [P, P, U64, P, U32, U64, P, C.POINTER(TaxoInfo)]
    L.goss_gpu_object_taxo_classify_reads.argtypes = [P, P, U64, U32, U64, P, P, P, C.POINTER(TaxoInfo)]
    L.goss_gpu_object_taxo_classify_reads_host.argtypes = [P, P, U64, U32, U64, P, P, P, C.POINTER(TaxoInfo)]
    L.goss_gpu_object_taxo_pair.argtypes = [P, P, P, U64, P]
    L.goss_gpu_object_taxo_pair_host.argtypes = [P, P, P, U64, P]
    L.goss_gpu_object_taxo_tally.argtypes = [P, P, U64, P]
    L.goss_gpu_object_taxo_tally_host.argtypes = [P, P, U64, P]
    L._object_declared = True


class Object:
    """One KmerSet, Graph, bare SparseArray or EntryEdgeSet resident in HBM, with batched queries (goss_gpu_object_*).

    Every query takes device torch tensors (used in place; results come back as torch tensors on the same device)
    or numpy arrays (staged through the device; results come back as numpy).  Keys: uint64 values when
    key_words == 1, else rows of {lo, hi} (torch: int64 with the same bits)."""

    def __init__(self, handle, L, device):
        self._L = L
        self._h = handle
        self.device = device
        d = ObjectDesc()
        self._check(L.goss_gpu_object_info(self._h, C.byref(d)))
        self.kind, self.K, self.count, self.key_words = d.kind, d.K, d.count, d.key_words
        self.asymmetric = bool(d.asymmetric)
        self.N = d.N_lo | (d.N_hi << 64)
        self.D, self.resident_bytes = d.D, d.resident_bytes
        self.node_words = 1 if 2 * self.K <= 62 else 2

    @classmethod
    def open(cls, files, base, kind, device=0, stream=None):
        """files: {name as on disk: bytes} (e.g. "gr.header", "gr-edges.low-bits.lwr", ...); kind OBJECT_*"""
        L = load()
        _declare_object(L)
        names = sorted(files)
        arr = (NamedFile * max(1, len(names)))()
        keep = []
        for i, n in enumerate(names):
            data = bytes(files[n])
            buf = C.create_string_buffer(data, max(1, len(data)))
            keep.append(buf)
            arr[i] = NamedFile(n.encode(), C.cast(buf, C.c_void_p), len(data))
        h = C.c_void_p()
        rc = L.goss_gpu_object_open(C.byref(h), device, stream, kind, base.encode(), arr, len(names))
        if rc:
            raise GossGpuError(rc, L.goss_gpu_strerror(rc).decode(), L.goss_gpu_object_last_error(None).decode())
        return cls(h, L, device)

    @classmethod
    def from_context(cls, ctx):
        """What the context has just emitted -- or built with entries_build --, device to device
        (goss_gpu_object_open_emitted)."""
        L = load()
        _declare_object(L)
        h = C.c_void_p()
        rc = L.goss_gpu_object_open_emitted(C.byref(h), ctx._h)
        if rc:
            raise GossGpuError(rc, L.goss_gpu_strerror(rc).decode(), L.goss_gpu_object_last_error(None).decode())
        return cls(h, L, ctx.device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.goss_gpu_object_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), self._L.goss_gpu_object_last_error(self._h).decode())

    def info(self):
        return {"kind": self.kind, "K": self.K, "count": self.count, "key_words": self.key_words,
                "asymmetric": self.asymmetric, "N": self.N, "D": self.D, "resident_bytes": self.resident_bytes}

    # -- staging: (device pointer, n, torch tensor kept alive, numpy?) --
    def _input(self, a, words):
        import numpy as np
        import torch
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise ValueError("torch inputs must be device tensors")
            t = a.contiguous()
            if t.element_size() != 8:
                raise ValueError("keys and ranks are 64-bit")
            _torch_ready()
            return t, t.numel() // words, False
        arr = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        t = torch.from_numpy(arr.view(np.int64)).to("cuda:%d" % self.device)
        return t, arr.size // words, True

    def _out(self, like, n, dtype, cols=1):
        import torch
        shape = (n,) if cols == 1 else (n, cols)
        return torch.empty(shape, dtype=dtype, device=like.device)

    @staticmethod
    def _back(t, staged, np_dtype):
        if not staged:
            return t
        return t.cpu().numpy().view(np_dtype)

    def rank(self, keys, normalize=False):
        """(rank, present) of every key: SparseArray::accessAndRank"""
        import numpy as np
        import torch
        t, n, staged = self._input(keys, self.key_words)
        r = self._out(t, n, torch.int64)
        p = self._out(t, n, torch.bool)
        self._check(self._L.goss_gpu_object_rank(self._h, t.data_ptr(), n, QUERY_NORMALIZE if normalize else 0, r.data_ptr(), p.data_ptr()))
        return self._back(r, staged, np.uint64), self._back(p, staged, np.bool_)

    def select(self, ranks):
        """the key of every rank: SparseArray::select"""
        import numpy as np
        import torch
        t, n, staged = self._input(ranks, 1)
        k = self._out(t, n, torch.int64, self.key_words)
        self._check(self._L.goss_gpu_object_select(self._h, t.data_ptr(), n, k.data_ptr()))
        return self._back(k, staged, np.uint64)

    def multiplicity(self, ranks):
        """Graph::multiplicity of every edge rank (u32; torch: int32 with the same bits)"""
        import numpy as np
        import torch
        t, n, staged = self._input(ranks, 1)
        c = self._out(t, n, torch.int32)
        self._check(self._L.goss_gpu_object_multiplicity(self._h, t.data_ptr(), n, c.data_ptr()))
        return self._back(c, staged, np.uint32)

    def lookup(self, keys, normalize=False):
        """the count of every key, 0 when absent (1 / 0 in a KmerSet): rank + multiplicity in one kernel"""
        import numpy as np
        import torch
        t, n, staged = self._input(keys, self.key_words)
        c = self._out(t, n, torch.int32)
        self._check(self._L.goss_gpu_object_lookup(self._h, t.data_ptr(), n, QUERY_NORMALIZE if normalize else 0, c.data_ptr()))
        return self._back(c, staged, np.uint32)

    def node_ranks(self, nodes, incoming=False, normalize=False):
        """(begin, end) edge ranks of every node (K-mers): GraphEssentials::beginEndRank; out-degree = end - begin,
        incoming=True: of the node's reverse complement (the in-degree)"""
        import numpy as np
        import torch
        t, n, staged = self._input(nodes, self.node_words)
        b = self._out(t, n, torch.int64)
        e = self._out(t, n, torch.int64)
        flags = (QUERY_INCOMING if incoming else 0) | (QUERY_NORMALIZE if normalize else 0)
        self._check(self._L.goss_gpu_object_node_ranks(self._h, t.data_ptr(), n, flags, b.data_ptr(), e.data_ptr()))
        return self._back(b, staged, np.uint64), self._back(e, staged, np.uint64)

    def length(self, ranks):
        """EntryEdgeSet::length of every entry rank: the edges of the path that starts there (u32; torch: int32)"""
        import numpy as np
        import torch
        t, n, staged = self._input(ranks, 1)
        c = self._out(t, n, torch.int32)
        self._check(self._L.goss_gpu_entries_length(self._h, t.data_ptr(), n, c.data_ptr()))
        return self._back(c, staged, np.uint32)

    def end_rank(self, ranks):
        """EntryEdgeSet::endRank of every entry rank: the entry at which the mirror path starts (u64; torch: int64)"""
        import numpy as np
        import torch
        t, n, staged = self._input(ranks, 1)
        e = self._out(t, n, torch.int64)
        self._check(self._L.goss_gpu_entries_end_rank(self._h, t.data_ptr(), n, e.data_ptr()))
        return self._back(e, staged, np.uint64)

    def near_kmers(self, lhs, rhs, whole_bases=False, normalize=False):
        """(lhs_new, rhs_new, gray): compute-near-kmers over a KmerSet's two membership bitmaps
        (goss_gpu_object_near_kmers).  A k-mer of one side only that has a neighbour of the other side only in the set
        loses both bits; gray is how many did.  lhs, rhs: (count + 63) // 64 words in WordyBitVector layout, as numpy
        uint64 arrays (numpy comes back), as bytes read from the .lhs-bits / .rhs-bits files (bytes come back) or as
        device int64 tensors (tensors come back).  With both flags off the result is the reference's; whole_bases
        flips whole bases instead of the reference's bit-shifted masks, normalize looks every neighbour up in its
        canonical form."""
        import numpy as np
        import torch
        as_bytes = isinstance(lhs, (bytes, bytearray, memoryview))
        if as_bytes:
            lhs, rhs = np.frombuffer(bytes(lhs), dtype=np.uint64).copy(), np.frombuffer(bytes(rhs), dtype=np.uint64).copy()
        tl, nl, staged = self._input(lhs, 1)
        tr, nr, _ = self._input(rhs, 1)
        nwords = (self.count + 63) // 64
        if nl != nr or nl < nwords or (nwords and nl != nwords):
            raise ValueError("the bitmaps must hold %d words each" % nwords)
        ol, orr = torch.zeros_like(tl), torch.zeros_like(tr)
        _torch_ready()
        flags =(NEAR_WHOLE_BASES if whole_bases else 0) | (NEAR_NORMALIZE if normalize else 0)
        gray = C.c_uint64(0)
        self._check(self._L.goss_gpu_object_near_kmers(self._h, tl.data_ptr() if nwords else None, tr.data_ptr() if nwords else None, flags,
                                                       ol.data_ptr() if nwords else None, orr.data_ptr() if nwords else None, C.byref(gray)))
        a, b = self._back(ol, staged, np.uint64), self._back(orr, staged, np.uint64)
        if as_bytes:
            a, b = a.tobytes(), b.tobytes()
        return a, b, gray.value

    # the bases of a batch of reads on the device: (uint8 tensor, staged?)
    def _bases(self, bases):
        import numpy as np
        import torch
        if isinstance(bases, torch.Tensor):
            if not bases.is_cuda or bases.element_size() != 1:
                raise ValueError("torch inputs must be device tensors of bytes")
            _torch_ready()
            return bases.contiguous().reshape(-1), False
        arr = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
        return torch.from_numpy(arr.copy()).to("cuda:%d" % self.device), True

    @staticmethod
    def _count_reads(t):
        n = t.numel()
        return int((t == 10).sum()) + (1 if n and int(t[-1]) != 10 else 0)

    def match_reads(self, bases, normalize=False, any=False, starts=False, flags=0, max_reads=None):
        """(windows, hits[, starts], info) per read of `bases` (reads separated by '\\n'): goss_gpu_object_match_reads.
        windows[r]: valid L-windows of read r; hits[r]: how many are in the object, or with any=True 1 / 0.
        bases: bytes or numpy uint8 (staged; numpy comes back) or a device uint8 tensor (used in place; tensors
        come back).  The outputs are sized by counting the newlines; max_reads overrides that."""
        import numpy as np
        import torch
        t, staged = self._bases(bases)
        n = t.numel()
        flags |= (MATCH_NORMALIZE if normalize else 0) | (MATCH_ANY if any else 0)
        info = MatchInfo()
        call = self._L.goss_gpu_object_match_reads
        ptr = t.data_ptr() if n else None
        if max_reads is None:
            max_reads = self._count_reads(t)
        w = self._out(t, max_reads, torch.int32)
        h = self._out(t, max_reads, torch.int32)
        s = self._out(t, max_reads + 1, torch.int64) if starts else None
        rc = call(self._h, ptr, n, flags, max_reads, w.data_ptr(), h.data_ptr(), s.data_ptr() if starts else None, C.byref(info))
        if rc == ERR_BUFFER:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), "needs max_reads = %d" % info.reads)
        self._check(rc)
        r = info.reads
        out = [self._back(w[:r], staged, np.uint32), self._back(h[:r], staged, np.uint32)]
        if starts:
            out.append(self._back(s[:r + 1], staged, np.uint64))
        return tuple(out) + (info.as_dict(),)

    def classify_bits(self, lhs, rhs):
        """Keeps a KmerSet's two membership bitmaps on the device for later classify_reads calls
        (goss_gpu_object_classify_bits_host); a second call replaces the pair.  lhs, rhs: (count + 63) // 64 words each,
        as numpy uint64 arrays or as the bytes of the .lhs-bits / .rhs-bits files."""
        import numpy as np
        nwords = (self.count + 63) // 64
        arrs = []
        for b in (lhs, rhs):
            a = np.frombuffer(bytes(b), dtype=np.uint64) if isinstance(b, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
            if a.size < nwords or (nwords and a.size != nwords):
                raise ValueError("the bitmaps must hold %d words each" % nwords)
            arrs.append(np.ascontiguousarray(a))
        self._check(self._L.goss_gpu_object_classify_bits_host(self._h, arrs[0].ctypes.data if nwords else None,
                                                               arrs[1].ctypes.data if nwords else None))

    def classify_reads(self, bases, lhs=None, rhs=None, normalize=True, starts=False, flags=0, max_reads=None):
        """(classes, windows[, starts], info) per read of `bases` (reads separated by '\\n'): goss_gpu_object_classify_reads.
        classes[r]: the OR of 1 << (2 * lhs[rank] + rhs[rank]) over the windows of read r that are in the set (bit 0: neither
        side, 1: right only, 2: left only, 3: both); windows[r]: its valid K-windows.  lhs, rhs: the bitmaps as near_kmers
        takes them (numpy, bytes, device int64 tensors), or both None for the pair kept by classify_bits.  bases and
        what comes back: as match_reads.  info: reads, windows, counts (reads per mask, a list of 16) and ms."""
        import numpy as np
        import torch
        t, staged = self._bases(bases)
        n = t.numel()
        nwords = (self.count + 63) // 64
        keep, ptrs = [], []
        for b in (lhs, rhs):                     # (one of the two None: the call itself refuses)
            if b is None:
                ptrs.append(None)
                continue
            if isinstance(b, (bytes, bytearray, memoryview)):
                b = np.frombuffer(bytes(b), dtype=np.uint64).copy()
            tb, nb, _ = self._input(b, 1)
            if nb < nwords or (nwords and nb != nwords):
                raise ValueError("the bitmaps must hold %d words each" % nwords)
            keep.append(tb)
            ptrs.append(tb.data_ptr() if nwords else None)
        pl, pr = ptrs
        flags |= CLASSIFY_NORMALIZE if normalize else 0
        info = ClassifyInfo()
        if max_reads is None:
            max_reads = self._count_reads(t)
        c = self._out(t, max_reads, torch.int32)
        w = self._out(t, max_reads, torch.int32)
        s = self._out(t, max_reads + 1, torch.int64) if starts else None
        rc = self._L.goss_gpu_object_classify_reads(self._h, t.data_ptr() if n else None, n, pl, pr, flags, max_reads, c.data_ptr(), w.data_ptr(),
                                                    s.data_ptr() if starts else None, C.byref(info))
        if rc == ERR_BUFFER:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), "needs max_reads = %d" % info.reads)
        self._check(rc)
        r = info.reads
        out = [self._back(c[:r], staged, np.uint32), self._back(w[:r], staged, np.uint32)]
        if starts:
            out.append(self._back(s[:r + 1], staged, np.uint64))
        return tuple(out) + (info.as_dict(),)

    # -- up to 64 references in one pass (goss_gpu_object_colour*) --
    def colours(self, array, ncolours):
        """Keeps one colour word per k-mer of a KmerSet on the device for later colour_reads calls
        (goss_gpu_object_colours_host): bit i of array[r] says that reference i holds the k-mer at rank r.  array: count
        uint64 values; ncolours: 1 .. 64, and no word may have a bit at or above it.  A second call replaces the words."""
        import numpy as np
        a = np.ascontiguousarray(array, dtype=np.uint64).reshape(-1)
        if a.size != self.count:
            raise ValueError("the colours must hold %d words" % self.count)
        self._check(self._L.goss_gpu_object_colours_host(self._h, a.ctypes.data if a.size else None, ncolours))

    def colours_from_index(self, index_obj):
        """The colour words made on the device from a pool's index (goss_gpu_object_colours_from_index): self is the
        KmerSet opened from <out>-union, index_obj the OBJECT_SPARSE_ARRAY opened from <out>-index.  Returns S, the number
        of samples the index speaks of."""
        s = C.c_uint32(0)
        self._check(self._L.goss_gpu_object_colours_from_index(self._h, getattr(index_obj, "_h", None), C.byref(s)))
        return s.value

    def colour_reads(self, bases, normalize=True, starts=False, max_reads=None):
        """(colours, windows[, starts], info) per read of `bases` (reads separated by '\\n'): goss_gpu_object_colour_reads.
        colours[r]: the OR of the kept colour words over the windows of read r that are in the set (uint64; torch: int64
        with the same bits); windows[r]: its valid K-windows.  bases and what comes back: as match_reads.  info: reads,
        windows, by_count (reads per number of bits in their word, a list of 65) and ms."""
        import numpy as np
        import torch
        t, staged = self._bases(bases)
        n = t.numel()
        info = ElectInfo()
        if max_reads is None:
            max_reads = self._count_reads(t)
        c = self._out(t, max_reads, torch.int64)
        w = self._out(t, max_reads, torch.int32)
        s = self._out(t, max_reads + 1, torch.int64) if starts else None
        rc = self._L.goss_gpu_object_colour_reads(self._h, t.data_ptr() if n else None, n, ELECT_NORMALIZE if normalize else 0, max_reads,
                                                  c.data_ptr(), w.data_ptr(), s.data_ptr() if starts else None, C.byref(info))
        if rc == ERR_BUFFER:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), "needs max_reads = %d" % info.reads)
        self._check(rc)
        r = info.reads
        out = [self._back(c[:r], staged, np.uint64), self._back(w[:r], staged, np.uint32)]
        if starts:
            out.append(self._back(s[:r + 1], staged, np.uint64))
        return tuple(out) + (info.as_dict(),)

    # -- a taxonomy over the set's k-mers (goss_gpu_object_taxo_*) --
    def taxo_tree(self, ids, parent_index):
        """Validates, numbers and uploads a tree: ids[i] the node's id, parent_index[i] the index of its parent, the root
        its own (goss_gpu_object_taxo_tree_host).  A second call replaces the tree and drops the annotation.  Every
        per-node array of the taxo_ calls is in this order."""
        import numpy as np
        a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        p = np.ascontiguousarray(parent_index, dtype=np.uint32).reshape(-1)
        if a.size != p.size:
            raise ValueError("ids and parent_index differ in length")
        self._check(self._L.goss_gpu_object_taxo_tree_host(self._h, a.size, a.ctypes.data if a.size else None, p.ctypes.data if a.size else None))
        self._taxo_n = int(a.size)

    def taxo_annotation(self, ann=None):
        """Starts an all-untouched annotation (None) or loads one: `count` node ids as a numpy uint32 array or as the bytes
        of a .annotation file, TAXO_NONE for an untouched k-mer (goss_gpu_object_taxo_annotation_host)."""
        import numpy as np
        if ann is None:
            return self._check(self._L.goss_gpu_object_taxo_annotation_host(self._h, None))
        a = np.frombuffer(bytes(ann), dtype=np.uint32) if isinstance(ann, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(ann, dtype=np.uint32).reshape(-1)
        if a.size != self.count:
            raise ValueError("the annotation must hold %d node ids" % self.count)
        a = np.ascontiguousarray(a) if a.size else np.zeros(1, dtype=np.uint32)     # (a pointer that is not NULL)
        self._check(self._L.goss_gpu_object_taxo_annotation_host(self._h, a.ctypes.data))

    def _u32(self, a, like=None):
        """a uint32 array on the device: (int32 tensor, staged?)"""
        import numpy as np
        import torch
        if isinstance(a, torch.Tensor):
            if not a.is_cuda or a.element_size() != 4:
                raise ValueError("torch inputs must be device tensors of 32-bit values")
            _torch_ready()
            return a.contiguous().reshape(-1), False
        arr = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        return torch.from_numpy(arr.view(np.int32).copy()).to("cuda:%d" % self.device), True

    def taxo_annotate(self, bases, read_nodes, normalize=True, flags=0, max_reads=None):
        """(windows, info): every window of every read of `bases` that is in the set takes the read's node into its
        k-mer's class by lca (goss_gpu_object_taxo_annotate).  read_nodes: one node id per read (numpy uint32 or a device
        int32 tensor with the same bits), or one id for all.  bases and what comes back: as match_reads.  info: reads,
        windows, hits, ms."""
        import numpy as np
        import torch
        t, staged = self._bases(bases)
        n = t.numel()
        if max_reads is None:
            max_reads = self._count_reads(t)
        if isinstance(read_nodes, int):
            read_nodes = np.full(max_reads, read_nodes, dtype=np.uint32)
        rn, _ = self._u32(read_nodes)
        if rn.numel() != max_reads:
            raise ValueError("read_nodes must hold %d node ids" % max_reads)
        w = self._out(t, max_reads, torch.int32)
        info = TaxoInfo()
        rc = self._L.goss_gpu_object_taxo_annotate(self._h, t.data_ptr() if n else None, n, rn.data_ptr() if max_reads else None,
                                                   flags | (TAXO_NORMALIZE if normalize else 0), max_reads, w.data_ptr(), C.byref(info))
        if rc == ERR_BUFFER:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), "needs max_reads = %d" % info.reads)
        self._check(rc)
        return self._back(w[:info.reads], staged, np.uint32), info.as_dict()

    def taxo_read_annotation(self):
        """(annotation, counts): the node id of every rank (TAXO_NONE where untouched) and, per node, the ranks whose class
        is exactly that node (goss_gpu_object_taxo_annotation_read); numpy uint32 / uint64."""
        import numpy as np
        ann = np.zeros(max(1, self.count), dtype=np.uint32)
        counts = np.zeros(max(1, getattr(self, "_taxo_n", 0)), dtype=np.uint64)
        self._check(self._L.goss_gpu_object_taxo_annotation_read(self._h, ann.ctypes.data, counts.ctypes.data))
        return ann[:self.count], counts[:getattr(self, "_taxo_n", 0)]

    def taxo_classify_reads(self, bases, normalize=True, starts=False, flags=0, max_reads=None):
        """(result, windows[, starts], info) per read of `bases`: goss_gpu_object_taxo_classify_reads.  result[r]: the
        deepest class among the read's windows when those classes lie on one root-to-leaf path, TAXO_MANY when they do
        not, TAXO_NONE without any.  bases and what comes back: as match_reads.  info: reads, windows, none, many,
        unannotated, ms."""
        import numpy as np
        import torch
        t, staged = self._bases(bases)
        n = t.numel()
        info = TaxoInfo()
        if max_reads is None:
            max_reads = self._count_reads(t)
        c = self._out(t, max_reads, torch.int32)
        w = self._out(t, max_reads, torch.int32)
        s = self._out(t, max_reads + 1, torch.int64) if starts else None
        rc = self._L.goss_gpu_object_taxo_classify_reads(self._h, t.data_ptr() if n else None, n, flags | (TAXO_NORMALIZE if normalize else 0),
                                                         max_reads, c.data_ptr(), w.data_ptr(), s.data_ptr() if starts else None, C.byref(info))
        if rc == ERR_BUFFER:
            raise GossGpuError(rc, self._L.goss_gpu_strerror(rc).decode(), "needs max_reads = %d" % info.reads)
        self._check(rc)
        r = info.reads
        out = [self._back(c[:r], staged, np.uint32), self._back(w[:r], staged, np.uint32)]
        if starts:
            out.append(self._back(s[:r + 1], staged, np.uint64))
        return tuple(out) + (info.as_dict(),)

    def taxo_pair(self, a, b):
        """the join of two result arrays, mate by mate (goss_gpu_object_taxo_pair): the deeper node when one is an
        ancestor-or-equal of the other, TAXO_MANY when not, the other where one is TAXO_NONE"""
        import numpy as np
        import torch
        ta, staged = self._u32(a)
        tb, _ = self._u32(b)
        if ta.numel() != tb.numel():
            raise ValueError("the two arrays differ in length")
        out = torch.empty_like(ta)
        n = ta.numel()
        self._check(self._L.goss_gpu_object_taxo_pair(self._h, ta.data_ptr() if n else None, tb.data_ptr() if n else None, n,
                                                      out.data_ptr() if n else None))
        return self._back(out, staged, np.uint32)

    def taxo_tally(self, values):
        """how often each node occurs among `values` (node ids, TAXO_NONE, TAXO_MANY), in the order of the tree, then the
        NONEs and the MANYs: n_nodes + 2 numpy uint64 (goss_gpu_object_taxo_tally)"""
        import numpy as np
        tv, _ = self._u32(values)
        counts = np.zeros(getattr(self, "_taxo_n", 0) + 2, dtype=np.uint64)
        self._check(self._L.goss_gpu_object_taxo_tally(self._h, tv.data_ptr() if tv.numel() else None, tv.numel(), counts.ctypes.data))
        return counts
