"""ctypes binding of libparasuite_hip.so (include/parasuite_hip.h).

The library is the product; this module only marshals arguments.  If the
shared object is missing the import fails loudly -- there is no fallback.

The ABI is declared once: the mirrors of the header's structs (STRUCTS, in the header's order) and the signature of every
function (SIGNATURES), which lib() applies when it loads the library.  tests/test_capi_cpu.py holds both against the header.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("PARASUITE_LIB") or os.path.join(_HERE, "libparasuite_hip.so")   # PARASUITE_LIB: a diagnostic build of the same library


def _fields(ctype, *names):
    return [(k, ctype) for k in names]


# ---- the structs of the header, in its order ----

class SearchOpts(C.Structure):
    """ps_search_opts: the search options of `bwa aln` / `bwa samse` beyond -n / -X, upstream's defaults unless named:
    SearchOpts(max_gap_opens=2, seed_len=20).  Ranges: include/parasuite_hip.h; check() asks the library (host only)."""
    _fields_ = [("struct_size", C.c_uint32)] + _fields(
        C.c_int32, "max_gap_opens", "max_gap_extensions", "indel_end_skip", "max_del_occ", "seed_len", "max_seed_diff", "max_entries",
        "s_mm", "s_gapo", "s_gape", "max_top2", "max_alt_hits")

    def __init__(self, **kw):
        super().__init__()
        lib().ps_search_opts_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_) or k == "struct_size":
                raise TypeError("SearchOpts has no option " + k)
            setattr(self, k, int(v))

    def check(self, profile_mode=False):
        _chk(lib().ps_search_opts_check(C.byref(self), 1 if profile_mode else 0))


class IndexInfo(C.Structure):
    _fields_ = [("seq_len", C.c_uint64), ("l_pac", C.c_uint64), ("primary", C.c_uint64), ("L2", C.c_uint64 * 5),
                ("n_blocks", C.c_uint64), ("n_sa", C.c_uint64), ("device_bytes", C.c_uint64),
                ("n_contigs", C.c_int32), ("n_holes", C.c_int32), ("sa_rounds", C.c_int32), ("sa_intv", C.c_int32),
                ("build_ms", C.c_double), ("jump_levels", C.c_int32), ("pad_", C.c_int32)]


ALN_DTYPE = np.dtype([("k", "<u8"), ("l", "<u8"), ("score", "<u2"), ("units", "<u2"), ("n_mm", "u1"), ("n_gapo", "u1"),
                      ("n_gape", "u1"), ("n_ins", "u1"), ("n_del", "u1"), ("pad", "u1", 7)])
HIT_DTYPE = np.dtype([("pos", "<i8"), ("sa", "<u8"), ("type", "<i4"), ("strand", "<i4"), ("mapq", "<i4"), ("n_mm", "<i4"),
                      ("n_gapo", "<i4"), ("n_gape", "<i4"), ("ref_shift", "<i4"), ("score", "<i4"), ("c1", "<i4"),
                      ("c2", "<i4"), ("n_cigar", "<i4"), ("n_multi", "<i4"), ("cigar", "<u4", 16)], align=True)


class Timing(C.Structure):
    _fields_ = _fields(C.c_double, "ms_width", "ms_backtrack", "ms_compact", "ms_select", "ms_sa2pos", "ms_refine", "ms_host_post",
                       "ms_total") + \
               _fields(C.c_int32, "n_width_launches", "n_backtrack_launches") + _fields(C.c_int64, "n_overflow_tier1", "n_overflow_tier2") + \
               _fields(C.c_double, "ms_classify", "ms_rows", "ms_sel_hard", "ms_sel_easy", "bt_begin_ms", "bt_end_ms")


class KStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "occ_pairs", "occ_same_blk", "nodes", "pushes", "pops", "lf_steps", "iters", "exact_steps")


class CollapseInfo(C.Structure):
    _fields_ = _fields(C.c_int64, "n_reads", "n_searched", "n_groups", "n_multi", "largest", "n_overflow_reads", "n_overflow_searched") + \
               _fields(C.c_int32, "n_bins", "n_bins_collapsed") + [("ms_collapse", C.c_double)]


class BamStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_in", "n_out", "bam_bytes")


class ProfileStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_records", "n_counted", "n_unmapped", "n_duplicate", "n_start_zero", "n_indel_reads", "n_skipped",
                       "n_without_qual", "n_qual_beyond_read")


class ClusterStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_records", "n_unmapped", "n_skipped_indel", "n_kept", "n_clusters", "n_clusters_written",
                       "n_crosslinked", "n_ccr", "n_double_stranded", "n_snp_hits", "n_snv_sites", "n_t2c_beyond_51", "n_ccr_clipped",
                       "n_ccr_past_end", "n_order_unmodelled")


class ExtractStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_records", "n_weak", "n_kept", "bam_bytes")


class NamesStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_records", "out_bytes")


class CombineStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_genome", "n_transcript", "n_unplaced", "n_unlocated", "n_missed_indel_splice", "n_groups",
                       "n_groups_ambiguous", "n_no_contig", "n_mt_unplaced", "n_lifted", "n_spliced", "n_strand_flipped", "bam_bytes")


_ROUTE_PATHS = ("reads_fq", "ref_fa", "out_prefix", "transcripts_fa", "bwa_mm", "parasuite_mm", "error_profile", "indel_profile")
_ROUTE_INTS = ("threads", "refine", "max_read_len", "mapq_genomic", "mapq_transcript")


class RouteOpts(C.Structure):
    _fields_ = _fields(C.c_char_p, *_ROUTE_PATHS) + _fields(C.c_int32, *_ROUTE_INTS)


class RouteStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("first", BamStats), ("refine", BamStats), ("transcript", BamStats),
                ("extract", ExtractStats), ("combine", CombineStats)] + \
               _fields(C.c_double, "s_total", "s_parse", "s_index_genome", "s_index_transcripts", "s_first", "s_profile", "s_refine",
                       "s_transcript", "s_combine") + \
               _fields(C.c_uint32, "n_index_loads_genome", "n_index_loads_transcripts", "n_fastq_parses", "pad_")


class RouteOpts2(C.Structure):
    """ps_route_opts2: ps_route_opts' fields behind a struct_size, then ref_refine, search and keep_unaligned"""
    _fields_ = [("struct_size", C.c_uint32)] + _fields(C.c_int32, *_ROUTE_INTS) + _fields(C.c_char_p, *_ROUTE_PATHS, "ref_refine") + \
               [("search", C.POINTER(SearchOpts)), ("keep_unaligned", C.c_int32), ("pad_", C.c_int32)]


ROUTE_OPTS_OLD_SIZE = RouteOpts2.ref_refine.offset          # a struct_size up to here holds what ps_route_opts holds


class ResidentOpts(C.Structure):
    _fields_ = _fields(C.c_uint32, "struct_size", "max_references")


class ResidentStats(C.Structure):
    _fields_ = _fields(C.c_uint32, "active", "n_references") + \
               _fields(C.c_uint64, "n_calls", "n_index_loads", "n_index_reuses", "n_stale_reloads", "n_evictions", "n_dropped_after_error",
                       "bytes_index_resident")


class BenchmarkStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_lines", "n_reads", "n_positives", "n_negatives", "n_records", "n_processed", "n_tp", "n_tn",
                       "n_unplaced", "n_other_contig", "n_outside", "n_other_bound", "bad_number_record") + \
               _fields(C.c_float, "precision", "recall", "accuracy")


class SimulateOpts(C.Structure):
    _fields_ = _fields(C.c_char_p, "transcripts_fa", "out_prefix", "error_profile", "t2c_profile", "t2c_positions", "quality_dist",
                       "indel_profile") + \
               [("bound_prob", C.c_double), ("seed", C.c_uint64), ("select_read", C.c_double), ("snp_rate", C.c_double),
                ("snp_report", C.c_double), ("allow_indels", C.c_int32), ("pad_", C.c_int32)]


class SimulateStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_reads", "n_bases_simulated", "sum_read_length", "n_clusters", "n_t2c", "n_errors", "most_t2c",
                       "most_errors", "n_indels", "n_snps", "n_transcripts", "n_selected", "n_clusters_skipped", "n_reads_skipped",
                       "n_snps_reported", "n_non_acgt", "n_snps_preselected", "n_snp_positions") + \
               _fields(C.c_double, "avg_read_length", "avg_reads_per_cluster", "s_total", "s_read", "s_plan", "s_snp", "s_snp_kernels",
                       "s_reads", "s_write")


class FetchStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_lines", "n_sites", "n_reverse", "n_bases", "n_hole_bases", "n_inverted", "n_no_contig",
                       "n_past_end", "n_before_start", "n_pieces") + \
               _fields(C.c_double, "s_total", "s_read", "s_index", "s_kernels", "s_write")


class BgzfStats(C.Structure):
    _fields_ = _fields(C.c_uint32, "struct_size", "n_blocks", "n_stored", "n_fixed", "n_dynamic", "pad_") + \
               _fields(C.c_uint64, "in_bytes", "out_bytes") + [("kernel_ms", C.c_double)]


class BamRecordsStats(C.Structure):
    _fields_ = _fields(C.c_uint64, "n_reads", "n_records", "n_device", "n_host", "bytes") + \
               _fields(C.c_double, "ms_upload", "ms_kernels", "ms_host_records", "ms_download")


class BamSortStats(C.Structure):
    _fields_ = _fields(C.c_uint32, "struct_size", "on_device") + \
               _fields(C.c_uint64, "n_records", "bytes", "n_calls_device", "n_calls_host", "n_resident") + \
               _fields(C.c_double, "ms_upload", "ms_sort", "ms_gather", "ms_download")


class BamNameSortStats(C.Structure):
    _fields_ = _fields(C.c_uint32, "struct_size", "on_device") + \
               _fields(C.c_uint64, "n_records", "bytes", "n_calls_device", "n_calls_host", "n_resident") + \
               _fields(C.c_uint32, "key_words", "pad_") + [("n_passes", C.c_uint64)] + \
               _fields(C.c_double, "ms_upload", "ms_keys", "ms_sort", "ms_gather", "ms_download")


# every struct typedef of the header -> its mirror (ps_aln and ps_hit are read as numpy records)
STRUCTS = {"ps_search_opts": SearchOpts, "ps_index_info": IndexInfo, "ps_aln": ALN_DTYPE, "ps_hit": HIT_DTYPE, "ps_timing": Timing,
           "ps_kstats": KStats, "ps_collapse_info": CollapseInfo, "ps_bam_stats": BamStats, "ps_profile_stats": ProfileStats, "ps_cluster_stats": ClusterStats,
           "ps_extract_stats": ExtractStats, "ps_names_stats": NamesStats, "ps_combine_stats": CombineStats,
           "ps_route_opts": RouteOpts, "ps_route_stats": RouteStats, "ps_route_opts2": RouteOpts2, "ps_resident_opts": ResidentOpts,
           "ps_resident_stats": ResidentStats, "ps_benchmark_stats": BenchmarkStats, "ps_simulate_opts": SimulateOpts,
           "ps_simulate_stats": SimulateStats, "ps_fetch_stats": FetchStats, "ps_bgzf_stats": BgzfStats,
           "ps_bam_records_stats": BamRecordsStats, "ps_bam_sort_stats": BamSortStats,
           "ps_bam_name_sort_stats": BamNameSortStats}

# ---- the functions of the header, in its order: name -> (restype, argtypes) ----
# int, int64_t, uint64_t, double, const char *; _PTR: ps_ctx *, ps_batch * and every buffer handed over as an address
_I, _I64, _U64, _D, _S, _PTR, _P = C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_char_p, C.c_void_p, C.POINTER
_MAP = [_I] + [_S] * 6          # threads, mm, error_profile, indel_profile, ref_fa, fastq, out

SIGNATURES = {
    "ps_version": (_S, []),
    "ps_last_error": (_S, []),
    "ps_index": (_I, [_S]),
    "ps_map": (_I, _MAP),
    "ps_search_opts_default": (None, [_P(SearchOpts)]),
    "ps_search_opts_check": (_I, [_P(SearchOpts), _I]),
    "ps_map_opts": (_I, _MAP + [_P(SearchOpts)]),
    "ps_ctx_open": (_PTR, [_S, _I]),
    "ps_ctx_clone": (_PTR, [_PTR, _I]),
    "ps_ctx_build": (_PTR, [_S, _I, _I]),
    "ps_ctx_close": (None, [_PTR]),
    "ps_ctx_set_stock": (_I, [_PTR, _S]),
    "ps_ctx_set_profile": (_I, [_PTR, _S, _S, _S]),
    "ps_ctx_set_profile_matrix": (_I, [_PTR, _P(_D), _D, _D, _I]),
    "ps_ctx_set_search": (_I, [_PTR, _P(SearchOpts)]),
    "ps_ctx_set_tiers": (_I, [_PTR, _P(C.c_uint32), _P(C.c_int32), _I]),
    "ps_ctx_set_stats": (_I, [_PTR, _I]),
    "ps_ctx_set_lanes": (_I, [_PTR, _I]),
    "ps_ctx_set_collapse": (_I, [_PTR, _I]),
    "ps_ctx_info": (_I, [_PTR, _P(IndexInfo)]),
    "ps_ctx_blob": (_I, [_PTR, _I, _P(_PTR), _P(_U64)]),
    "ps_ctx_meta": (_I64, [_PTR, _S, _I64]),
    "ps_ctx_from_blobs": (_PTR, [_S, _I64, _I, _P(_PTR)]),
    "ps_ctx_fetch": (_I, [_PTR, _I, _PTR, _U64]),
    "ps_ctx_export_blob": (_I, [_PTR, _I, _PTR, _U64]),
    "ps_ctx_index_check": (_I, [_PTR, _PTR]),
    "ps_ctx_sa_lookup": (_I, [_PTR, _PTR, _I64, _PTR]),
    "ps_ctx_order_sort": (_I, [_PTR, _PTR, _I64, _PTR]),
    "ps_batch_from_fastq": (_PTR, [_PTR, _S]),
    "ps_batch_from_codes": (_PTR, [_PTR, _I64, _I, _PTR]),
    "ps_batch_free": (None, [_PTR]),
    "ps_batch_n": (_I64, [_PTR]),
    "ps_batch_search": (_I, [_PTR]),
    "ps_batch_select_hard": (_I, [_PTR, _U64, _P(_U64)]),
    "ps_batch_select_easy": (_I, [_PTR, _I]),
    "ps_batch_locate": (_I, [_PTR]),
    "ps_batch_run": (_I, [_PTR, _I]),
    "ps_batch_write_sam": (_I, [_PTR, _S, _I, _I]),
    "ps_batch_n_aln": (_I, [_PTR, _PTR, _I64]),
    "ps_batch_alns": (_I64, [_PTR, _I64, _PTR, _I64]),
    "ps_batch_hits": (_I, [_PTR, _PTR, _I64]),
    "ps_batch_timing": (_I, [_PTR, _P(Timing)]),
    "ps_ctx_read_iters": (_I64, [_PTR, _PTR, _I64]),
    "ps_ctx_launch_order": (_I64, [_PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _I64]),
    "ps_batch_kstats": (_I, [_PTR, _I, _P(KStats)]),
    "ps_batch_collapse_info": (_I, [_PTR, _P(CollapseInfo)]),
    "ps_batch_duplicate_of": (_I, [_PTR, _PTR, _I64]),
    "ps_release_host_cache": (None, []),
    "ps_parse_check": (_I, [_S, _I, _U64, _P(_U64)]),
    "ps_sam_to_bam": (_I, [_S, _S, _I, _I, _I, _I, _P(BamStats)]),
    "ps_map_to_bam": (_I, _MAP + [_I, _I, _I, _P(BamStats)]),
    "ps_bam_view": (_I, [_S, _S, _I, _I, _P(BamStats)]),
    "ps_bam_sort": (_I, [_S, _S, _I, _I, _P(BamStats)]),
    "ps_bam_index": (_I, [_S, _I]),
    "ps_error_profile": (_I, [_S, _S, _I, _S]),
    "ps_error_profile_full": (_I, [_S, _S, _I, _S, _I, _P(ProfileStats)]),
    "ps_pileup_clusters": (_I, [_S, _S, _S, _S, _I, _S, _P(ClusterStats)]),
    "ps_extract_weak_reads": (_I, [_S, _S, _S, _I, _I, _P(ExtractStats)]),
    "ps_extract_read_names": (_I, [_S, _S, _P(NamesStats)]),
    "ps_combine_genome_transcript": (_I, [_S, _S, _S, _I, _I, _I, _P(CombineStats)]),
    "ps_map_profiled": (_I, _MAP + [_I, _I, _S]),
    "ps_map_route": (_I, [_P(RouteOpts), _P(RouteStats)]),
    "ps_map_route_opts": (_I, [_P(RouteOpts2), _P(RouteStats)]),
    "ps_resident_begin": (_I, [_P(ResidentOpts)]),
    "ps_resident_end": (_I, []),
    "ps_resident_info": (_I, [_P(ResidentStats)]),
    "ps_benchmark_reads": (_I, [_S, _S, _S, _P(BenchmarkStats)]),
    "ps_simulate_reads": (_I, [_P(SimulateOpts), _P(SimulateStats)]),
    "ps_fetch_sequences": (_I, [_S, _S, _S, _I, _P(FetchStats)]),
    "ps_bgzf_device": (_I, [_I]),
    "ps_bgzf_compress": (_I, [_PTR, _U64, _I, _PTR, _U64, _P(BgzfStats)]),
    "ps_bam_records_device": (_I, [_I]),
    "ps_bam_records_info": (_I, [_P(BamRecordsStats)]),
    "ps_batch_bam_records": (_I64, [_PTR, _I, _I, _I, _PTR, _U64, _PTR, _P(BamRecordsStats)]),
    "ps_bam_sort_device": (_I, [_I]),
    "ps_bam_sort_info": (_I, [_P(BamSortStats)]),
    "ps_bam_sort_records": (_I64, [_PTR, _U64, _I, _I, _PTR, _U64, _P(BamSortStats)]),
    "ps_bam_name_sort_device": (_I, [_I]),
    "ps_bam_name_sort_info": (_I, [_P(BamNameSortStats)]),
    "ps_bam_name_sort_records": (_I64, [_PTR, _U64, _I, _I, _PTR, _U64, _P(BamNameSortStats)]),
}
EXPORTS = list(SIGNATURES)

_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise ImportError("libparasuite_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


class PsError(RuntimeError):
    pass


def _chk(rc):
    if rc:
        raise PsError(lib().ps_last_error().decode())


def _opt(v):
    """a parameter the header documents as optional: None or "" -> NULL, anything else its text.  Required strings are encoded
    where they are passed, so that None for one of them raises here instead of reaching the library"""
    return None if v is None or v == "" else str(v).encode()


def _search_ptr(search):
    """a SearchOpts, a dict of its fields, or None (the defaults)"""
    if search is None:
        return None
    return C.pointer(search if isinstance(search, SearchOpts) else SearchOpts(**search))


def _struct_dict(st):
    return {f: (_struct_dict(getattr(st, f)) if isinstance(getattr(st, f), C.Structure) else getattr(st, f)) for f, _ in st._fields_}


def _stats(fn, cls, *args):
    """fn(*args, &stats) for a call whose last parameter is its stats struct; returns the struct as a dict (nested for nested structs)"""
    st = cls()
    _chk(fn(*args, C.byref(st)))
    return _struct_dict(st)


class Ctx:
    """Device-resident FM index + alignment options (ps_ctx)."""

    def __init__(self, handle):
        if not handle:
            raise PsError(lib().ps_last_error().decode())
        self.h = handle
        self._keep = None

    @classmethod
    def open(cls, ref_fa, device=0):
        return cls(lib().ps_ctx_open(ref_fa.encode(), device))

    @classmethod
    def build(cls, ref_fa, device=0, save_files=False):
        return cls(lib().ps_ctx_build(ref_fa.encode(), device, 1 if save_files else 0))

    @classmethod
    def from_blobs(cls, meta, device, ptrs, keep=None):
        arr = (C.c_void_p * 3)(*ptrs)
        c = cls(lib().ps_ctx_from_blobs(meta, len(meta), device, arr))
        c._keep = keep
        return c

    def clone(self, device=0):
        """a second context holding a device-to-device copy of this one's index (ps_map's route to every device after the first)"""
        return Ctx(lib().ps_ctx_clone(self.h, int(device)))

    def close(self):
        if self.h:
            lib().ps_ctx_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stock(self, n="0.04"):
        _chk(lib().ps_ctx_set_stock(self.h, str(n).encode()))

    def set_search(self, search=None, **kw):
        """the search options (SearchOpts, a dict, or keywords; None: the defaults): kept when set_stock / set_profile change the costs"""
        _chk(lib().ps_ctx_set_search(self.h, _search_ptr(kw if search is None and kw else search)))

    def set_profile_files(self, ep, ip, x="-1"):
        _chk(lib().ps_ctx_set_profile(self.h, ep.encode(), _opt(ip), str(x).encode()))

    def set_profile(self, P, ins_rate=0.0, del_rate=0.0, x=-1):
        arr = (C.c_double * 16)(*[float(v) for v in np.asarray(P, dtype=np.float64).reshape(16)])
        _chk(lib().ps_ctx_set_profile_matrix(self.h, arr, ins_rate, del_rate, int(x)))

    def set_tiers(self, pool_cap=None, aln_cap=None, bt_blocks=0):
        pc = (C.c_uint32 * 3)(*pool_cap) if pool_cap else None
        ac = (C.c_int32 * 3)(*aln_cap) if aln_cap else None
        _chk(lib().ps_ctx_set_tiers(self.h, pc, ac, bt_blocks))

    def set_stats(self, on=True):
        """search launches that follow count their Occ lookups / pushes / pops (Batch.kstats(1)); off = the timed kernel"""
        _chk(lib().ps_ctx_set_stats(self.h, 1 if on else 0))

    def set_lanes(self, n):
        """batches created afterwards take n (1 or 2) lanes of work in turn; two batches on two lanes may run from two threads"""
        _chk(lib().ps_ctx_set_lanes(self.h, int(n)))

    def set_collapse(self, mode=1):
        """identical reads of a batch are searched once and the result copied to the others; every output stays what it is
        without.  1 on, 0 off, -1 (the default of a context): as PS_COLLAPSE says when the batch is searched"""
        _chk(lib().ps_ctx_set_collapse(self.h, int(mode)))

    def info(self):
        i = IndexInfo()
        _chk(lib().ps_ctx_info(self.h, C.byref(i)))
        return i

    def blob(self, which):
        p, n = C.c_void_p(), C.c_uint64()
        _chk(lib().ps_ctx_blob(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def meta(self):
        n = lib().ps_ctx_meta(self.h, None, 0)
        buf = C.create_string_buffer(n)
        lib().ps_ctx_meta(self.h, buf, n)
        return buf.raw

    def fetch(self, which):
        _, n = self.blob(which)
        out = np.empty(n, dtype=np.uint8)
        _chk(lib().ps_ctx_fetch(self.h, which, out.ctypes.data, n))
        return out

    def sa_samples(self):
        """Sampled suffix array as uint64: blob 1 holds n_sa low words followed by the bit-32 plane; entry 0 means -1."""
        n_sa = int(self.info().n_sa)
        w = self.fetch(1).view("<u4")
        out = w[:n_sa].astype(np.uint64)
        hi = (w[n_sa:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
        out |= hi.reshape(-1)[:n_sa].astype(np.uint64) << np.uint64(32)
        out[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        return out

    def index_check(self):
        """every row of the index against the packed text along the LF cycle -> dict(rows, bad_symbols, bad_samples, longest_arc)"""
        out = np.zeros(4, dtype=np.uint64)
        _chk(lib().ps_ctx_index_check(self.h, out.ctypes.data))
        return dict(rows=int(out[0]), bad_symbols=int(out[1]), bad_samples=int(out[2]), longest_arc=int(out[3]))

    def sa_lookup(self, rows):
        """SA[row] for rows in [1, seq_len] (device LF walk to a sampled row)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty(r.size, dtype=np.uint64)
        _chk(lib().ps_ctx_sa_lookup(self.h, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def order_sort(self, keys):
        """the hand-out order of a search launch from its 8-bit keys: order[queue position] = read (stable, ascending)"""
        k = np.ascontiguousarray(keys, dtype=np.uint8)
        out = np.empty(k.size, dtype=np.int32)
        _chk(lib().ps_ctx_order_sort(self.h, k.ctypes.data, k.size, out.ctypes.data))
        return out

    def export_blob(self, which, dev_ptr, nbytes):
        _chk(lib().ps_ctx_export_blob(self.h, which, dev_ptr, nbytes))

    def bwt_syms_chunked(self, chunk_blocks=1 << 20):
        """BWT symbol string (1 byte/symbol) decoded block-wise; for genomes too big for bwt_syms()."""
        info = self.info()
        blk = self.fetch(0).view("<u4").reshape(-1, 16)
        out = np.empty(blk.shape[0] * 192, dtype=np.uint8)
        sh = np.arange(32, dtype=np.uint32)[None, None, :]
        for a in range(0, blk.shape[0], chunk_blocks):
            lo = (blk[a:a + chunk_blocks, 4:10, None] >> sh) & 1
            hi = (blk[a:a + chunk_blocks, 10:16, None] >> sh) & 1
            out[a * 192:(a + lo.shape[0]) * 192] = (lo | (hi << 1)).astype(np.uint8).reshape(-1)
        return out[:info.seq_len]

    def bwt_syms(self):
        """Decode the Occ blocks (two bit planes per block) back into the BWT symbol string; also the block counts."""
        blk = self.fetch(0).view("<u4").reshape(-1, 16)
        return self.bwt_syms_chunked(), blk[:, :4]

    RI_WORDS = 20          # ps_types.h: PS_RI_WORDS

    def read_iters(self):
        """per-read profile of the last search launch (PS_READ_ITERS=1), RI_WORDS words per read in the launch's own order of the reads:
        iterations | stack slots | D(read), D(seed) << 8, the estimate's two scans << 16 / << 24 | best score, final budget << 8, hits << 16 | 16 words of D bounds"""
        n = lib().ps_ctx_read_iters(self.h, None, 0)
        out = np.zeros(n, dtype=np.uint32)
        lib().ps_ctx_read_iters(self.h, out.ctypes.data, n)
        return out

    def launch_order(self):
        """what the last search launch was prepared with (PS_READ_ITERS=1), by the read index read_iters() rows have: dict(est, key,
        pred, order, ids) -- estimated best score in budget units, the class the hand-out order sorts by, the model's expected node
        count, queue position -> read, read -> input read; arrays of length 0 where the launch made no order"""
        n = lib().ps_ctx_launch_order(self.h, None, None, None, None, None, 0)
        out = dict(est=np.zeros(n, dtype=np.uint8), key=np.zeros(n, dtype=np.uint8), pred=np.zeros(n, dtype=np.float32),
                   order=np.zeros(n, dtype=np.int32), ids=np.zeros(n, dtype=np.int32))
        lib().ps_ctx_launch_order(self.h, *[out[k].ctypes.data for k in ("est", "key", "pred", "order", "ids")], n)
        return out

    def batch_from_fastq(self, path):
        return Batch(lib().ps_batch_from_fastq(self.h, path.encode()), self)

    def batch_from_codes(self, codes):
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        return Batch(lib().ps_batch_from_codes(self.h, c.shape[0], c.shape[1], c.ctypes.data), self)


class Batch:
    def __init__(self, handle, ctx):
        if not handle:
            raise PsError(lib().ps_last_error().decode())
        self.h = handle
        self.ctx = ctx

    def free(self):
        if self.h:
            lib().ps_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def n(self):
        return lib().ps_batch_n(self.h)

    def search(self):
        _chk(lib().ps_batch_search(self.h))

    def select_hard(self, draws_before=0):
        out = C.c_uint64()
        _chk(lib().ps_batch_select_hard(self.h, draws_before, C.byref(out)))
        return out.value

    def select_easy(self, threads=8):
        _chk(lib().ps_batch_select_easy(self.h, threads))

    def locate(self):
        _chk(lib().ps_batch_locate(self.h))

    def run(self, threads=8):
        _chk(lib().ps_batch_run(self.h, threads))

    def write_sam(self, path, header=True, threads=8):
        _chk(lib().ps_batch_write_sam(self.h, path.encode(), 1 if header else 0, threads))

    def n_aln(self):
        out = np.zeros(self.n, dtype=np.int32)
        _chk(lib().ps_batch_n_aln(self.h, out.ctypes.data, out.size))
        return out

    def alns(self, read, cap=256):
        out = np.zeros(cap, dtype=ALN_DTYPE)
        n = lib().ps_batch_alns(self.h, read, out.ctypes.data, cap)
        if n > cap:
            return self.alns(read, n)
        return out[:n]

    def hits(self):
        out = np.zeros(self.n, dtype=HIT_DTYPE)
        _chk(lib().ps_batch_hits(self.h, out.ctypes.data, out.size))
        return out

    def timing(self):
        return _stats(lib().ps_batch_timing, Timing, self.h)

    def kstats(self, which):
        return _stats(lib().ps_batch_kstats, KStats, self.h, which)

    def collapse_info(self):
        """ps_collapse_info of the last search as a dict: reads, reads searched, groups ... (collapse off: n_searched == n_reads)"""
        return _stats(lib().ps_batch_collapse_info, CollapseInfo, self.h)

    def bam_records(self, min_mapq=0, on_device=True, threads=8):
        """after locate(): the batch's BAM records with MAPQ >= min_mapq, in input order -> (the bytes, per record 0 device-built /
        1 host-built as a uint8 array, ps_bam_records_stats as a dict); on_device False: the host route.  The route runs twice, once for
        the size and once for the bytes, and with on_device each run adds to the counters of ps_bam_records_info"""
        st = BamRecordsStats()
        n = lib().ps_batch_bam_records(self.h, int(min_mapq), int(bool(on_device)), int(threads), None, 0, None, C.byref(st))
        if n < 0:
            raise PsError(lib().ps_last_error().decode())
        dst, origin = np.zeros(max(1, n), dtype=np.uint8), np.zeros(max(1, st.n_records), dtype=np.uint8)
        n2 = lib().ps_batch_bam_records(self.h, int(min_mapq), int(bool(on_device)), int(threads), dst.ctypes.data, n, origin.ctypes.data, C.byref(st))
        if n2 < 0:
            raise PsError(lib().ps_last_error().decode())
        return dst[:n2].tobytes(), origin[:st.n_records].copy(), _struct_dict(st)

    def duplicate_of(self):
        """input order: the input index of the representative of every read's group (a representative names itself).  The groups
        are exact -- compared in full, never by hash -- and in one rare case incomplete: identical reads may stand in two groups
        (include/parasuite_hip.h).  An error if the batch was searched with collapse off"""
        out = np.zeros(self.n, dtype=np.int64)
        _chk(lib().ps_batch_duplicate_of(self.h, out.ctypes.data, out.size))
        return out


def ps_parse_check(path, threads=1, chunk_bytes=0):
    """host-only: (reads, bases, hash, pieces) of the read parser -- whole file, or streamed in windows as ps_map does"""
    out = (C.c_uint64 * 4)()
    _chk(lib().ps_parse_check(path.encode(), int(threads), int(chunk_bytes), out))
    return tuple(int(v) for v in out)


def ps_error_profile(mapping, ref_fa, max_read_len=101, out_prefix=None):
    """<out_prefix>.errorprofile / .indelprofile from the records of a SAM or BAM file (counted on the GPU)"""
    _chk(lib().ps_error_profile(mapping.encode(), ref_fa.encode(), int(max_read_len), _opt(out_prefix)))


def ps_error_profile_full(mapping, ref_fa, max_read_len=101, out_prefix=None, infer_qualities=False):
    """all six files of ErrorProfiling.inferErrorProfile(infer_qualities, false): <out_prefix>.errorprofile, .indelprofile,
    .errorprofile.vcf, .qualityPerMismatch, .indels, .qualities (empty without infer_qualities); returns the record counters"""
    return _stats(lib().ps_error_profile_full, ProfileStats, mapping.encode(), ref_fa.encode(), int(max_read_len), _opt(out_prefix),
                  int(bool(infer_qualities)))


def ps_pileup_clusters(mapping, ref_fa, out_file, snp_vcf=None, min_read_coverage=1, site_prefix=None):
    """the six files of PileupClusters.calculateReadPileups: <out_file>, .ccr.fasta, .ccr.tsv, .report and
    <site_prefix or mapping>.sitefrequency.tsv, .sitepositions.tsv (counted on the GPU); returns the counters.
    The library itself refuses a missing mapping, ref_fa or out_file"""
    return _stats(lib().ps_pileup_clusters, ClusterStats, _opt(mapping), _opt(ref_fa), _opt(out_file), _opt(snp_vcf), int(min_read_coverage),
                  _opt(site_prefix))


def ps_extract_weak_reads(mapping, out_bam, out_fastq, mapq_threshold=10, threads=8):
    """ExtractWeakMappingReads.extractReads: records with MAPQ < mapq_threshold -> out_fastq (read orientation restored), the
    others -> out_bam under the input's header (host code, needs no GPU); returns the counters"""
    return _stats(lib().ps_extract_weak_reads, ExtractStats, mapping.encode(), out_bam.encode(), out_fastq.encode(), int(mapq_threshold),
                  int(threads))


def ps_combine_genome_transcript(genome_bam, transcript_bam, out_bam, sort_by_coordinate=False, write_index=False, threads=8):
    """CombineGenomeTranscript.combine: the genomic records, then the transcript hits lifted to genome coordinates (on the GPU),
    optionally coordinate-sorted with <out_bam>.bai; returns the counters"""
    return _stats(lib().ps_combine_genome_transcript, CombineStats, genome_bam.encode(), transcript_bam.encode(), out_bam.encode(),
                  int(bool(sort_by_coordinate)), int(bool(write_index)), int(threads))


def ps_benchmark_reads(mapping, out_statistics, reads_fq):
    """ValidateBenchmarkStatisticsPARCLIP.calculateBenchmarkStatistics: a mapping of simulated reads (SAM or BAM) scored against
    the truth in the read names, the reads file counted for the totals (both on the GPU); writes out_statistics and returns
    the counters"""
    return _stats(lib().ps_benchmark_reads, BenchmarkStats, mapping.encode(), out_statistics.encode(), reads_fq.encode())


def ps_simulate_reads(transcripts_fa, out_prefix, error_profile, t2c_profile, t2c_positions, quality_dist, indel_profile, bound_prob, seed=0,
                      select_read=None, snp_rate=None, snp_report=None, allow_indels=None):
    """bin/createSimulatedPARCLIPDataset.pl, the `simulate` mode: PAR-CLIP reads drawn from transcripts on the GPU; writes
    <out_prefix>.fastq, .clusters, _snps.vsf, .log and .err and returns the counters.  None for one of the last four selects the
    Perl's constant (0.216, 0.01, 0.8, indels allowed)"""
    o = SimulateOpts(*[str(v).encode() for v in (transcripts_fa, out_prefix, error_profile, t2c_profile, t2c_positions, quality_dist, indel_profile)],
                     float(bound_prob), int(seed), -1.0 if select_read is None else float(select_read), -1.0 if snp_rate is None else float(snp_rate),
                     -1.0 if snp_report is None else float(snp_report), -1 if allow_indels is None else int(bool(allow_indels)), 0)
    return _stats(lib().ps_simulate_reads, SimulateStats, C.byref(o))


def ps_fetch_sequences(ref_fa, sites, out_file, bed=False):
    """FetchSequencesForBindingSites / FetchSequencesForBEDFile.fetchSequences, the `fetch` (bed false) and `fetchBed` modes:
    the reference sequence of every site of a table, gathered on the GPU from the index of ref_fa (.ann and .pac; the FASTA is
    not opened); writes out_file and returns the counters"""
    return _stats(lib().ps_fetch_sequences, FetchStats, ref_fa.encode(), sites.encode(), out_file.encode(), int(bool(bed)))


def ps_bgzf_device(device):
    """the BGZF switch: -1 host zlib (the default), device >= 0: every BAM this process writes from now on is compressed on it"""
    _chk(lib().ps_bgzf_device(int(device)))


def ps_bgzf_compress(data, device=0):
    """data cut at 0xff00 bytes -> (the BGZF members without an end-of-file block, the stats dict), compressed on the device;
    device -1: by the library's host path (zlib at PS_BAM_LEVEL, 16 threads)"""
    data = bytes(data)
    n_blocks = (len(data) + 0xff00 - 1) // 0xff00
    dst = C.create_string_buffer(max(1, len(data) + len(data) // 100 + n_blocks * 128))   # the device never exceeds the stored form; zlib may, a little
    st = BgzfStats(struct_size=C.sizeof(BgzfStats))
    _chk(lib().ps_bgzf_compress(data, len(data), int(device), dst, len(dst), C.byref(st)))
    return dst.raw[:st.out_bytes], _struct_dict(st)


def ps_bam_records_device(on):
    """the switch of the BAM records' device route (off by default): ps_map_to_bam and every pass of ps_map_route build their
    records on the device that mapped the piece; setting it, either way, resets the counters of ps_bam_records_info"""
    _chk(lib().ps_bam_records_device(int(bool(on))))


def ps_bam_records_info():
    """ps_bam_records_stats as a dict: what the device route has done since the switch was last set"""
    return _stats(lib().ps_bam_records_info, BamRecordsStats)


def ps_bam_sort_device(device):
    """the switch of the coordinate sort's device route: -1 the host (the default), device >= 0: every sorted BAM this process
    writes from now on is sorted and gathered on it; setting it, either way, resets the counters of ps_bam_sort_info"""
    _chk(lib().ps_bam_sort_device(int(device)))


def ps_bam_sort_info():
    """ps_bam_sort_stats as a dict: what the coordinate sort has done since the switch was last set"""
    return _stats(lib().ps_bam_sort_info, BamSortStats)


def _sort_records(fn, stats_cls, records, device, threads, cap, guard):
    """the staged sort of either order: (the sorted records, the call's stats as a dict[, the guard bytes])"""
    records = bytes(records)
    cap = len(records) if cap is None else int(cap)
    dst = C.create_string_buffer(b"\xee" * (cap + guard), cap + guard) if cap + guard else C.create_string_buffer(1)
    st = stats_cls(struct_size=C.sizeof(stats_cls))
    n = fn(records, len(records), int(device), int(threads), dst, cap, C.byref(st))
    if n < 0:
        raise PsError(lib().ps_last_error().decode())
    out = dst.raw[:n], _struct_dict(st)
    return out + (dst.raw[cap:cap + guard],) if guard else out


def ps_bam_sort_records(records, device=0, threads=16, cap=None, guard=0):
    """BAM records back to back -> (the same records in coordinate order, the call's ps_bam_sort_stats as a dict); device -1: the
    library's host route.  cap: the capacity told to the library (default: what the records take); guard: bytes of 0xee kept
    behind cap, returned as a third value so that a caller can see them untouched"""
    return _sort_records(lib().ps_bam_sort_records, BamSortStats, records, device, threads, cap, guard)


def ps_bam_name_sort_device(device):
    """the switch of the name sort's device route (`samtools sort -n`'s order): -1 the host (the default), device >= 0: every
    name-sorted BAM this process writes from now on is sorted and gathered on it; setting it, either way, resets the counters of
    ps_bam_name_sort_info and leaves the coordinate sort's switch alone"""
    _chk(lib().ps_bam_name_sort_device(int(device)))


def ps_bam_name_sort_info():
    """ps_bam_name_sort_stats as a dict: what the name sort has done since its switch was last set"""
    return _stats(lib().ps_bam_name_sort_info, BamNameSortStats)


def ps_bam_name_sort_records(records, device=0, threads=16, cap=None, guard=0):
    """BAM records back to back -> (the same records in name order, the call's ps_bam_name_sort_stats as a dict); device -1: the
    library's host route.  cap and guard: as ps_bam_sort_records takes them"""
    return _sort_records(lib().ps_bam_name_sort_records, BamNameSortStats, records, device, threads, cap, guard)


def _map_args(threads, mm, error_profile, indel_profile, ref_fa, fastq, out):
    """what ps_map, ps_map_opts, ps_map_to_bam and ps_map_profiled have in common: the two profile files are optional"""
    return int(threads), str(mm).encode(), _opt(error_profile), _opt(indel_profile), ref_fa.encode(), fastq.encode(), out.encode()


def ps_map_profiled(threads, mm, error_profile, indel_profile, ref_fa, reads, out_sam, min_mapq, max_read_len, profile_prefix):
    """ps_map + <profile_prefix>.errorprofile / .indelprofile of its alignments with MAPQ >= min_mapq, counted from memory
    (the library refuses a missing profile_prefix)"""
    _chk(lib().ps_map_profiled(*_map_args(threads, mm, error_profile, indel_profile, ref_fa, reads, out_sam), int(min_mapq), int(max_read_len),
                               _opt(profile_prefix)))


def ps_index(ref_fa):
    _chk(lib().ps_index(ref_fa.encode()))


def ps_map(threads, mm, error_profile, indel_profile, ref_fa, fastq, out_sam, search=None):
    """search: a SearchOpts or a dict of its fields (`ps_map_opts`); None: `ps_map`"""
    args = _map_args(threads, mm, error_profile, indel_profile, ref_fa, fastq, out_sam)
    if search is None:
        _chk(lib().ps_map(*args))
    else:
        _chk(lib().ps_map_opts(*args, _search_ptr(search)))


def ps_sam_to_bam(sam, bam, min_mapq=0, sort_by_coordinate=False, write_index=False, threads=8):
    """SAM text -> BAM; MAPQ filter, coordinate sort and <bam>.bai in the same pass (host code, needs no GPU)."""
    return _stats(lib().ps_sam_to_bam, BamStats, sam.encode(), bam.encode(), int(min_mapq), int(bool(sort_by_coordinate)), int(bool(write_index)),
                  int(threads))


def ps_map_to_bam(threads, mm, error_profile, indel_profile, ref_fa, fastq, out_bam, min_mapq=0, sort_by_coordinate=False, write_index=False):
    """ps_map with the records going straight into a (MAPQ-filtered, optionally sorted + indexed) BAM: no SAM text in between"""
    return _stats(lib().ps_map_to_bam, BamStats, *_map_args(threads, mm, error_profile, indel_profile, ref_fa, fastq, out_bam),
                  int(min_mapq), int(bool(sort_by_coordinate)), int(bool(write_index)))


def ps_bam_view(in_bam, out_bam, min_mapq=0, threads=8):
    return _stats(lib().ps_bam_view, BamStats, in_bam.encode(), out_bam.encode(), int(min_mapq), int(threads))


def ps_bam_sort(in_bam, out_bam, by_name=False, threads=8):
    return _stats(lib().ps_bam_sort, BamStats, in_bam.encode(), out_bam.encode(), int(bool(by_name)), int(threads))


def ps_bam_index(bam, threads=8):
    _chk(lib().ps_bam_index(bam.encode(), int(threads)))


def _route_args(paths, threads, refine, max_read_len, mapq_genomic, mapq_transcript):
    """the fields ps_route_opts and ps_route_opts2 share: (the eight strings, the five integers).  Every string goes through
    _opt: the library itself refuses a missing reads_fq, ref_fa or out_prefix before it touches anything"""
    return [_opt(p) for p in paths], [int(threads), int(bool(refine)), int(max_read_len), int(mapq_genomic), int(mapq_transcript)]


def ps_map_route(reads_fq, ref_fa, out_prefix, transcripts_fa=None, threads=8, refine=False, max_read_len=101, mapq_genomic=10,
                 mapq_transcript=1, bwa_mm=None, parasuite_mm=None, error_profile=None, indel_profile=None):
    """the toolkit's whole `map` mode (Main.java:249-420) in one call: the passes, the error profile, the weak-read extraction, the
    lift and the sorts with the reads parsed once, each index loaded once and everything between the passes handed over in memory;
    leaves the files Main.java names under out_prefix and returns ps_route_stats as nested dicts"""
    paths, ints = _route_args((reads_fq, ref_fa, out_prefix, transcripts_fa, bwa_mm, parasuite_mm, error_profile, indel_profile),
                              threads, refine, max_read_len, mapq_genomic, mapq_transcript)
    o = RouteOpts(*paths, *ints)
    return _stats(lib().ps_map_route, RouteStats, C.byref(o))


def ps_map_route_opts(reads_fq, ref_fa, out_prefix, transcripts_fa=None, threads=8, refine=False, max_read_len=101, mapq_genomic=10,
                      mapq_transcript=1, bwa_mm=None, parasuite_mm=None, error_profile=None, indel_profile=None, ref_refine=None,
                      keep_unaligned=False, search=None, struct_size=None):
    """ps_map_route with Main.java's --ref-refine and --unaligned and the search options of every pass (a SearchOpts, a dict of
    its fields or None); struct_size: the size the struct claims (None: all of it)"""
    paths, ints = _route_args((reads_fq, ref_fa, out_prefix, transcripts_fa, bwa_mm, parasuite_mm, error_profile, indel_profile),
                              threads, refine, max_read_len, mapq_genomic, mapq_transcript)
    o = RouteOpts2(C.sizeof(RouteOpts2) if struct_size is None else int(struct_size), *ints, *paths, _opt(ref_refine),
                   _search_ptr(search), int(bool(keep_unaligned)), 0)
    return _stats(lib().ps_map_route_opts, RouteStats, C.byref(o))


def ps_extract_read_names(mapping, out_file):
    """ExtractNotMappedReads.extractReads, the `extractAligned` mode: "@" + QNAME per record of a SAM or BAM file, in file order
    (host code, needs no GPU)"""
    return _stats(lib().ps_extract_read_names, NamesStats, mapping.encode(), out_file.encode())


def ps_resident_begin(max_references=2):
    o = ResidentOpts(C.sizeof(ResidentOpts), int(max_references))
    _chk(lib().ps_resident_begin(C.byref(o)))


def ps_resident_end():
    _chk(lib().ps_resident_end())


def ps_resident_info():
    """ps_resident_stats as a dict; any time: outside a scope active is 0 and the counters are the last scope's"""
    return _stats(lib().ps_resident_info, ResidentStats)


class resident:
    """with capi.resident(max_references=2): ... -- the mapping calls inside keep their indexes and the device's lanes of work
    in HBM from call to call (include/parasuite_hip.h: the resident scope).  The scope is ended on every way out of the block,
    an exception included; ps_resident_info() afterwards still shows the scope's counters."""

    def __init__(self, max_references=2):
        self.max_references = max_references

    def __enter__(self):
        ps_resident_begin(self.max_references)
        return self

    def __exit__(self, exc_type, exc, tb):
        ps_resident_end()
        return False

    @staticmethod
    def info():
        return ps_resident_info()
