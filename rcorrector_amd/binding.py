"""ctypes binding of include/rcorrector_amd.h.  No algorithm lives here."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")

# every function include/rcorrector_amd.h declares (tests check the .so exports all of them)
ABI_SYMBOLS = [
    "rc_create", "rc_destroy", "rc_last_error", "rc_device_numa_node", "rc_device_memory",
    "rc_table_build", "rc_table_build_device", "rc_table_load_jfdump",
    "rc_table_count_begin", "rc_table_count_add", "rc_table_count_add_device", "rc_table_count_finish",
    "rc_table_count_keep", "rc_table_count_arenas", "rc_table_count_release", "rc_table_count_park", "rc_table_count_finish_sharded", "rc_submit_resident", "rc_wait_resident",
    "rc_table_count_reads_device", "rc_table_write_jfdump", "rc_table_share", "rc_table_replicate", "rc_table_replicate_async", "rc_table_lookup", "rc_table_export", "rc_table_digest", "rc_table_layout", "rc_table_stats",
    "rc_table_count_spectrum", "rc_table_spectrum", "rc_table_compare",
    "rc_recount_begin", "rc_recount_add", "rc_recount_add_device", "rc_recount_follow", "rc_recount_finish",
    "rc_change_report_begin", "rc_change_report_get", "rc_change_report_end",
    "rc_weak_profile_device", "rc_weak_profile_into",
    "rc_read_depth_device", "rc_read_depth_into",
    "rc_read_screen_device", "rc_read_screen_into",
    "rc_norm_select_device",
    "rc_dup_census_begin", "rc_dup_census_get", "rc_dup_census_end", "rc_read_keys_device", "rc_dup_census_merge",
    "rc_recur_census_begin", "rc_recur_census_get", "rc_recur_census_end", "rc_recur_census_merge", "rc_change_keys_device",
    "rc_trust_profile_device", "rc_trust_profile_begin", "rc_trust_profile_get", "rc_trust_profile_end",
    "rc_mate_overlap_device", "rc_mate_overlap_begin", "rc_mate_overlap_get", "rc_mate_overlap_end",
    "rc_read_trim_device",
    "rc_read_merge_device",
    "rc_estimate_error_rate", "rc_bad_quality_from_hist", "rc_set_run_params", "rc_set_quality_bits", "rc_pack_quality_bits",
    "rc_correct_batch", "rc_set_slot_lanes", "rc_runtime_prepare", "rc_submit", "rc_wait", "rc_host_alloc", "rc_host_free", "rc_host_register", "rc_host_unregister", "rc_correct_batch_traced", "rc_correct_device", "rc_strong_threshold_device", "rc_probe_device", "rc_sync",
    "rc_strong_threshold_read", "rc_correct_read", "rc_kmer_info_read",
    "rc_pack_bases", "rc_submit_packed", "rc_wait_packed", "rc_apply_fixes",
    "rc_profile_enable", "rc_profile_get", "rc_profile_reset", "rc_profile_correct_counters", "rc_profile_read_rounds", "rc_selftest_get_bound", "rc_debug_routes", "rc_debug_pipeline", "rc_summary",
    "rc_selftest_transport_packed", "rc_selftest_transport_bytes",
]


class RcorrectorError(RuntimeError):
    pass


def library_path():
    # RC_LIB lets a developer A/B a differently built library; the default is the in-tree build
    return os.environ.get("RC_LIB") or os.path.join(HERE, "librcorrector_amd.so")


def build_library(quiet=True):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", CSRC, "-j4", "all"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)
    return library_path()


class _Config(C.Structure):
    _fields_ = [("device", C.c_int), ("k", C.c_int), ("max_fix_per_k", C.c_int)]


class _Batch(C.Structure):
    _fields_ = [("mode", C.c_int), ("n", C.c_size_t),
                ("seq", C.c_void_p), ("qual", C.c_void_p), ("off", C.c_void_p),
                ("seq2", C.c_void_p), ("qual2", C.c_void_p), ("off2", C.c_void_p),
                ("ret", C.c_void_p), ("l", C.c_void_p), ("m", C.c_void_p), ("h", C.c_void_p)]


class _PackedBatch(C.Structure):
    _fields_ = [("mode", C.c_int), ("n", C.c_size_t), ("nbytes", C.c_uint64),
                ("off", C.c_void_p), ("bases", C.c_void_p), ("qual_bits", C.c_void_p),
                ("exc_pos", C.c_void_p), ("exc_chr", C.c_void_p), ("n_exc", C.c_size_t),
                ("ret", C.c_void_p), ("l", C.c_void_p), ("m", C.c_void_p), ("h", C.c_void_p),
                ("fix_pos", C.c_void_p), ("fix_chr", C.c_void_p), ("fix_cap", C.c_size_t), ("n_fix", C.c_size_t)]


class _ResidentBatch(C.Structure):
    _fields_ = [("mode", C.c_int), ("n", C.c_size_t), ("arena_a", C.c_int), ("arena_b", C.c_int),
                ("begin_a", C.c_uint64), ("bytes_a", C.c_uint64), ("begin_b", C.c_uint64), ("bytes_b", C.c_uint64),
                ("off", C.c_void_p), ("qual_bits", C.c_void_p),
                ("ret", C.c_void_p), ("l", C.c_void_p), ("m", C.c_void_p), ("h", C.c_void_p),
                ("fix_pos", C.c_void_p), ("fix_chr", C.c_void_p), ("fix_cap", C.c_size_t), ("n_fix", C.c_size_t)]


class _SpectrumStats(C.Structure):
    _fields_ = [("distinct", C.c_uint64), ("total", C.c_uint64), ("unique", C.c_uint64), ("max_count", C.c_uint64)]


COMPARE_FIELDS = ("distinct_a", "distinct_b", "shared", "mass_a", "mass_b", "shared_mass_a", "shared_mass_b", "max_count_a", "max_count_b")


class _CompareStats(C.Structure):
    """rc_table_compare_stats: nine counts"""
    _fields_ = [(f, C.c_uint64) for f in COMPARE_FIELDS]


class _RecountStats(C.Structure):
    _fields_ = [("all", _SpectrumStats), ("absent_distinct", C.c_uint64), ("absent_total", C.c_uint64)]


REPORT_MAX_LEN = 1024       # RC_REPORT_MAX_LEN
REPORT_MAX_PER_READ = 64    # RC_REPORT_MAX_PER_READ


class _ChangeReport(C.Structure):
    _fields_ = [("reads", C.c_uint64 * 2), ("reads_changed", C.c_uint64 * 2), ("reads_unfixable", C.c_uint64 * 2), ("changes", C.c_uint64 * 2),
                ("len_hist", C.c_uint64 * REPORT_MAX_LEN * 2), ("by_pos5", C.c_uint64 * REPORT_MAX_LEN * 2), ("by_pos3", C.c_uint64 * REPORT_MAX_LEN * 2),
                ("subst", C.c_uint64 * 4 * 5), ("by_qual", C.c_uint64 * 3), ("per_read", C.c_uint64 * (REPORT_MAX_PER_READ + 1))]


class _ReadWeak(C.Structure):
    """rc_read_weak: 16 bytes per read"""
    _fields_ = [("weak", C.c_int32), ("bad_prefix", C.c_int32), ("bad_suffix", C.c_int32), ("uncovered", C.c_int32)]


class _RecurCensus(C.Structure):
    """rc_recur_census: six counts, the caller's three arrays, n_top"""
    _fields_ = [("changes", C.c_uint64), ("contexted", C.c_uint64), ("clipped", C.c_uint64),
                ("sites", C.c_uint64), ("sites_recurrent", C.c_uint64), ("changes_at_recurrent", C.c_uint64),
                ("recur", C.c_void_p), ("top_key", C.c_void_p), ("top_count", C.c_void_p), ("n_top", C.c_uint32)]


RECUR_FLANK = 14

SELFTEST_CANARY = 0xA5        # RC_SELFTEST_CANARY
SELFTEST_ARENA_SLACK = 64     # RC_SELFTEST_ARENA_SLACK
SELFTEST_FIX_SLACK = 64       # RC_SELFTEST_FIX_SLACK


def recur_key_decode(key):
    """A site key of the recurrence census as (from_letter, to_letter, 29-mer): the canonical window's text, the letter its
    centre was corrected from ('N': anything but upper-case ACGT) and the centre itself."""
    key = int(key)
    f, w = key & 7, key >> 3
    n = 2 * RECUR_FLANK + 1
    text = "".join("ACGT"[(w >> (2 * (n - 1 - i))) & 3] for i in range(n))
    return ("ACGTN"[f] if f <= 4 else "?", text[RECUR_FLANK], text)


class _DupCensus(C.Structure):
    """rc_dup_census: three counts and the caller's two arrays of max_bin + 1 uint64"""
    _fields_ = [("units", C.c_uint64), ("distinct_before", C.c_uint64), ("distinct_after", C.c_uint64),
                ("copies_before", C.c_void_p), ("copies_after", C.c_void_p)]


TRUST_MAX_LEN = 1024
_TrustArray = (C.c_uint64 * TRUST_MAX_LEN) * 2
TRUST_FIELDS = ("windows", "solid5", "weak5", "solid3", "weak3")


class _TrustCounts(C.Structure):
    """rc_trust_counts: five arrays of [2][RC_TRUST_MAX_LEN] uint64, one version of the reads"""
    _fields_ = [(n, _TrustArray) for n in TRUST_FIELDS]


class _TrustProfile(C.Structure):
    """rc_trust_profile"""
    _fields_ = [("k", C.c_int32), ("min_count", C.c_int32), ("reads", C.c_uint64 * 2), ("before", _TrustCounts), ("after", _TrustCounts)]


OVERLAP_MAX_LEN = 1024
OVERLAP_FRAG_LEN = 2048
OVERLAP_SCALARS = ("min_overlap", "max_mismatch_pct", "pairs", "overlapping", "compared_before", "disagree_before", "compared_after", "disagree_after",
                   "resolved", "introduced", "kept", "pairs_improved", "pairs_worsened", "pairs_same")
OVERLAP_ARRAYS = ("frag", "compared5", "disagree5_before", "disagree5_after")
OVERLAP_WORDS = len(OVERLAP_SCALARS) + OVERLAP_FRAG_LEN + 6 * OVERLAP_MAX_LEN


class _MateOverlap(C.Structure):
    """rc_mate_overlap: 64-bit counts throughout"""
    _fields_ = ([(n, C.c_uint64) for n in OVERLAP_SCALARS] + [("frag", C.c_uint64 * OVERLAP_FRAG_LEN)] +
                [(n, (C.c_uint64 * OVERLAP_MAX_LEN) * 2) for n in OVERLAP_ARRAYS[1:]])


def mate_overlap_dict(words):
    """OVERLAP_WORDS 64-bit words laid out as an rc_mate_overlap (a copy of device memory, say) -> the dict Context.mate_overlap returns"""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint64)
    if w.size != OVERLAP_WORDS:
        raise ValueError("an rc_mate_overlap has %d 64-bit words, got %d" % (OVERLAP_WORDS, w.size))
    out = {n: int(w[i]) for i, n in enumerate(OVERLAP_SCALARS)}
    at = len(OVERLAP_SCALARS)
    out["frag"] = w[at:at + OVERLAP_FRAG_LEN].copy()
    at += OVERLAP_FRAG_LEN
    for n in OVERLAP_ARRAYS[1:]:
        out[n] = w[at:at + 2 * OVERLAP_MAX_LEN].reshape(2, OVERLAP_MAX_LEN).copy()
        at += 2 * OVERLAP_MAX_LEN
    return out


TRIM_MAX_LEN = 1023
TRIM_ADAPTER_MAX = 64
TRIM_ADAPTER = b"AGATCGGAAGAGC"      # the Illumina universal stem
READ_TRIM_DTYPE = np.dtype([("keep_len", np.int32), ("cut_qual", np.int32), ("cut_adapter", np.int32), ("cut_pair", np.int32)])     # rc_read_trim
TRIM_TALLY_DTYPE = np.dtype([("reads", np.uint64, (2,)), ("cut_reads", np.uint64, (2, 3)), ("bases_removed", np.uint64, (2,)),
                             ("short_reads", np.uint64, (2,)), ("units", np.uint64), ("units_kept", np.uint64), ("pairs_overlapping", np.uint64),
                             ("keep_hist", np.uint64, (2, 1024))])                                                                  # rc_trim_tally
TRIM_TALLY_WORDS = TRIM_TALLY_DTYPE.itemsize // 8


class _TrimParams(C.Structure):
    """rc_trim_params"""
    _fields_ = [("qual_min", C.c_int32), ("qual_base", C.c_int32), ("adapter_min", C.c_int32), ("adapter_mm_pct", C.c_int32), ("pair_overlap", C.c_int32),
                ("pair_min_overlap", C.c_int32), ("pair_mm_pct", C.c_int32), ("min_len", C.c_int32), ("adapter1", C.c_uint8 * 64), ("adapter2", C.c_uint8 * 64),
                ("adapter1_len", C.c_int32), ("adapter2_len", C.c_int32)]


def trim_params(qual_min=20, qual_base=33, adapter1=TRIM_ADAPTER, adapter2=None, adapter_min=5, adapter_mm_pct=10, pair_overlap=True, pair_min_overlap=30,
                pair_mm_pct=10, min_len=20, adapter1_len=None, adapter2_len=None):
    """an rc_trim_params; adapter2 = None: adapter1's.  Nothing is checked here but what the struct cannot hold (an adapter of
    more than 64 bytes); adapter*_len overrides the length the library is told."""
    a1 = bytes(adapter1)
    a2 = a1 if adapter2 is None else bytes(adapter2)
    if len(a1) > TRIM_ADAPTER_MAX or len(a2) > TRIM_ADAPTER_MAX:
        raise ValueError("an adapter has at most %d bases" % TRIM_ADAPTER_MAX)
    p = _TrimParams(int(qual_min), int(qual_base), int(adapter_min), int(adapter_mm_pct), int(bool(pair_overlap)), int(pair_min_overlap), int(pair_mm_pct),
                    int(min_len))
    C.memmove(p.adapter1, a1, len(a1))
    C.memmove(p.adapter2, a2, len(a2))
    p.adapter1_len = len(a1) if adapter1_len is None else int(adapter1_len)
    p.adapter2_len = len(a2) if adapter2_len is None else int(adapter2_len)
    return p


def trim_tally_dict(words):
    """TRIM_TALLY_WORDS 64-bit words laid out as an rc_trim_tally (a copy of device memory, say) -> a dict named as the struct's
    fields: ints and numpy uint64 arrays"""
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
    if w.size != TRIM_TALLY_WORDS:
        raise ValueError("an rc_trim_tally has %d 64-bit words, got %d" % (TRIM_TALLY_WORDS, w.size))
    t = w.view(TRIM_TALLY_DTYPE)[0]
    return {n: (int(t[n]) if t[n].shape == () else t[n].copy()) for n in TRIM_TALLY_DTYPE.names}


MERGE_MAX_LEN = 1023          # bases of a mate; a merged read has up to 2 * 1023 - min_overlap
MERGE_LEN_BINS = 2048
READ_MERGE_DTYPE = np.dtype([("merged_len", np.int32), ("d", np.int32), ("v", np.int32), ("m", np.int32)])     # rc_read_merge
MERGE_TALLY_DTYPE = np.dtype([("pairs", np.uint64), ("merged", np.uint64), ("unmerged", np.uint64), ("readthrough", np.uint64), ("compared", np.uint64),
                              ("mismatches", np.uint64), ("took_mate1", np.uint64), ("took_mate2", np.uint64), ("ties", np.uint64),
                              ("len_hist", np.uint64, (MERGE_LEN_BINS,))])                                      # rc_merge_tally
MERGE_TALLY_WORDS = MERGE_TALLY_DTYPE.itemsize // 8


class _MergeParams(C.Structure):
    """rc_merge_params"""
    _fields_ = [("min_overlap", C.c_int32), ("max_mismatch_pct", C.c_int32), ("qual_base", C.c_int32), ("qual_cap", C.c_int32)]


def merge_params(min_overlap=30, max_mismatch_pct=10, qual_base=33, qual_cap=41):
    """an rc_merge_params; nothing is checked here: the library says what is out of range"""
    return _MergeParams(int(min_overlap), int(max_mismatch_pct), int(qual_base), int(qual_cap))


def merge_tally_dict(words):
    """MERGE_TALLY_WORDS 64-bit words laid out as an rc_merge_tally (a copy of device memory, say) -> a dict named as the
    struct's fields: ints and a numpy uint64 array"""
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
    if w.size != MERGE_TALLY_WORDS:
        raise ValueError("an rc_merge_tally has %d 64-bit words, got %d" % (MERGE_TALLY_WORDS, w.size))
    t = w.view(MERGE_TALLY_DTYPE)[0]
    return {n: (int(t[n]) if t[n].shape == () else t[n].copy()) for n in MERGE_TALLY_DTYPE.names}


class _DeviceBatch(C.Structure):
    _fields_ = [("mode", C.c_int), ("n_reads", C.c_uint32), ("nbytes", C.c_uint64),
                ("max_read_len", C.c_int32),
                ("d_seq", C.c_void_p), ("d_qual", C.c_void_p), ("d_off", C.c_void_p),
                ("d_ret", C.c_void_p), ("d_l", C.c_void_p), ("d_m", C.c_void_p), ("d_h", C.c_void_p)]


_lib = None


def load_library():
    """Loads librcorrector_amd.so; raises RcorrectorError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RcorrectorError(
            "%s not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C rcorrector_amd/csrc).  There is no CPU fallback." % path)
    # torch wheels bundle their own copy of the HIP runtime (same soname).  If torch is going to be
    # used in this process (bench.py / tests use it for device tensors and torch.distributed) it
    # has to be loaded FIRST so that exactly one HIP runtime is live; a C/C++ host links ROCm's.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the binding
        pass
    try:
        L = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise RcorrectorError("cannot load %s: %s" % (path, e))
    vp, sz = C.c_void_p, C.c_size_t
    L.rc_create.restype = vp
    L.rc_create.argtypes = [C.POINTER(_Config), C.c_char_p, sz]
    L.rc_destroy.argtypes = [vp]
    L.rc_last_error.restype = C.c_char_p
    L.rc_last_error.argtypes = [vp]
    L.rc_table_build.argtypes = [vp, vp, vp, sz]
    L.rc_table_build_device.argtypes = [vp, vp, vp, sz]
    L.rc_table_load_jfdump.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.rc_table_count_reads_device.argtypes = [vp, vp, sz, C.c_int, C.POINTER(C.c_int64)]
    L.rc_table_count_begin.argtypes = [vp]
    L.rc_table_count_add.argtypes = [vp, vp, sz]
    L.rc_table_count_add_device.argtypes = [vp, vp, sz]
    L.rc_table_count_finish.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.rc_table_count_keep.argtypes = [vp, C.c_int]
    L.rc_table_count_arenas.argtypes = [vp, C.POINTER(C.c_size_t), vp, sz]
    L.rc_table_count_release.argtypes = [vp]
    L.rc_table_count_park.argtypes = [vp]
    L.rc_table_count_finish_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.rc_set_slot_lanes.argtypes = [vp, C.c_int]
    if hasattr(L, "rc_runtime_prepare"):   # (RC_LIB may name a library of an earlier round: tools/ab.sh)
        L.rc_runtime_prepare.argtypes = [C.c_int]
    L.rc_submit_resident.argtypes = [vp, C.POINTER(_ResidentBatch), C.c_int]
    L.rc_wait_resident.argtypes = [vp, C.c_int]
    L.rc_table_write_jfdump.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.rc_table_share.argtypes = [vp, vp]
    L.rc_table_replicate.argtypes = [vp, vp]
    L.rc_table_replicate_async.argtypes = [vp, vp]
    L.rc_device_numa_node.argtypes = [vp]
    L.rc_device_memory.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rc_table_lookup.argtypes = [vp, vp, sz, vp]
    L.rc_table_export.argtypes = [vp, vp, vp, sz, C.POINTER(C.c_size_t)]
    L.rc_table_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rc_table_layout.argtypes = [vp]
    L.rc_table_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rc_table_count_spectrum.argtypes = [vp, C.c_uint32]
    L.rc_table_spectrum.argtypes = [vp, C.c_int, vp, C.c_uint32, C.POINTER(_SpectrumStats)]
    L.rc_table_compare.argtypes = [vp, vp, C.c_uint32, vp, C.POINTER(_CompareStats)]
    L.rc_recount_begin.argtypes = [vp, C.c_uint32]
    L.rc_recount_add.argtypes = [vp, vp, C.c_size_t]
    L.rc_recount_add_device.argtypes = [vp, vp, C.c_size_t]
    L.rc_recount_follow.argtypes = [vp, C.c_int]
    L.rc_recount_finish.argtypes = [vp, vp, C.POINTER(_RecountStats)]
    L.rc_change_report_begin.argtypes = [vp]
    L.rc_change_report_get.argtypes = [vp, C.POINTER(_ChangeReport)]
    L.rc_change_report_end.argtypes = [vp]
    L.rc_weak_profile_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, vp]
    L.rc_weak_profile_into.argtypes = [vp, C.c_int, vp, C.c_int32]
    L.rc_read_depth_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, vp]
    L.rc_read_depth_into.argtypes = [vp, C.c_int, vp]
    L.rc_read_screen_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, vp]
    L.rc_read_screen_into.argtypes = [vp, C.c_int, vp, C.c_int32, vp]
    L.rc_norm_select_device.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp]
    L.rc_dup_census_begin.argtypes = [vp]
    L.rc_dup_census_get.argtypes = [vp, C.c_uint32, C.POINTER(_DupCensus)]
    L.rc_dup_census_end.argtypes = [vp]
    L.rc_read_keys_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int, vp]
    L.rc_dup_census_merge.argtypes = [vp, vp]
    L.rc_recur_census_begin.argtypes = [vp]
    L.rc_recur_census_get.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_RecurCensus)]
    L.rc_recur_census_end.argtypes = [vp]
    L.rc_recur_census_merge.argtypes = [vp, vp]
    L.rc_change_keys_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, C.c_uint64, vp]
    L.rc_trust_profile_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rc_trust_profile_begin.argtypes = [vp, C.c_int32]
    L.rc_trust_profile_get.argtypes = [vp, C.POINTER(_TrustProfile)]
    L.rc_trust_profile_end.argtypes = [vp]
    L.rc_mate_overlap_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rc_mate_overlap_begin.argtypes = [vp, C.c_int32, C.c_int32]
    L.rc_read_trim_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(_TrimParams), vp, vp, vp]
    L.rc_read_merge_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(_MergeParams), vp, vp, vp, vp, C.c_uint64, vp]
    L.rc_mate_overlap_get.argtypes = [vp, C.POINTER(_MateOverlap)]
    L.rc_mate_overlap_end.argtypes = [vp]
    L.rc_estimate_error_rate.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
    L.rc_bad_quality_from_hist.restype = C.c_char
    L.rc_bad_quality_from_hist.argtypes = [vp, vp, C.c_int32]
    L.rc_set_run_params.argtypes = [vp, C.c_double, C.c_char]
    L.rc_set_quality_bits.argtypes = [vp, C.c_int]
    L.rc_pack_quality_bits.restype = None
    L.rc_pack_quality_bits.argtypes = [vp, sz, C.c_char, vp]
    L.rc_correct_batch.argtypes = [vp, C.POINTER(_Batch)]
    L.rc_submit.argtypes = [vp, C.POINTER(_Batch), C.c_int]
    L.rc_wait.argtypes = [vp, C.c_int]
    L.rc_host_alloc.argtypes = [vp, sz, C.POINTER(C.c_void_p)]
    L.rc_host_free.argtypes = [vp, vp]
    L.rc_correct_device.argtypes = [vp, C.POINTER(_DeviceBatch)]
    L.rc_probe_device.argtypes = [vp, vp, C.c_uint64, vp]
    L.rc_strong_threshold_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int32, vp]
    L.rc_sync.argtypes = [vp]
    L.rc_strong_threshold_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32)]
    L.rc_correct_read.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    L.rc_kmer_info_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rc_pack_bases.restype = sz
    L.rc_pack_bases.argtypes = [vp, sz, sz, vp, vp, vp, sz]
    L.rc_submit_packed.argtypes = [vp, C.POINTER(_PackedBatch), C.c_int]
    L.rc_wait_packed.argtypes = [vp, C.c_int]
    L.rc_apply_fixes.restype = None
    L.rc_apply_fixes.argtypes = [vp, vp, vp, sz]
    L.rc_profile_enable.argtypes = [vp, C.c_int]
    L.rc_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.rc_profile_reset.argtypes = [vp]
    L.rc_profile_correct_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rc_profile_read_rounds.argtypes = [vp, vp]
    L.rc_selftest_get_bound.argtypes = [vp, vp, sz, C.c_double, vp, vp]
    L.rc_debug_routes.argtypes = [vp, vp, vp, vp, C.c_uint32]
    L.rc_debug_pipeline.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rc_selftest_transport_packed.argtypes = [vp, vp, sz, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp]
    L.rc_selftest_transport_bytes.argtypes = [vp, vp, sz, C.c_uint32, vp, sz, C.c_uint32, vp, vp, C.c_uint32, vp, vp]
    L.rc_summary.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _lib = L
    return L


def runtime_prepare(hw_queues=16):
    """rc_runtime_prepare: ask the HIP runtime for hardware queues for the slot lanes' streams (GPU_MAX_HW_QUEUES unless the process
    has it already).  Before the process first touches HIP -- before torch does; one thread.  1 = set, 0 = was set already."""
    return load_library().rc_runtime_prepare(int(hw_queues))


def pack_reads(seqs):
    """list of bytes -> (uint8 arena with a NUL after every read, uint32 offsets[n+1])."""
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    off = np.zeros(len(seqs) + 1, dtype=np.uint32)
    np.cumsum(lens + 1, out=off[1:])
    if seqs:
        arena = np.frombuffer(b"\0".join(seqs) + b"\0", dtype=np.uint8).copy()
    else:
        arena = np.zeros(0, np.uint8)
    return arena, off


def unpack_reads(arena, off):
    b = arena.tobytes()
    return [b[off[i]:off[i + 1] - 1] for i in range(len(off) - 1)]


def _ptr(x):
    """device/host pointer of a numpy array, a torch tensor or a raw integer address."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        # a torch tensor: whatever produced it ran on torch's stream, the library works on its own --
        # make sure the producer has finished before the address is handed over
        if getattr(x, "is_cuda", False):
            import torch
            torch.cuda.current_stream(x.device).synchronize()
        return x.data_ptr()
    raise TypeError("cannot take a pointer of %r" % type(x))


class Context:
    """One GPU: stream, k-mer table in HBM, scratch.  Mirrors the objects main.cpp sets up
    (KmerCode kcode / Store kmers / globals, main.cpp:17-30,140,270)."""

    def __init__(self, k=23, max_fix_per_k=4, device=0):
        self._L = load_library()
        cfg = _Config(device, k, max_fix_per_k)
        err = C.create_string_buffer(512)
        self._h = self._L.rc_create(C.byref(cfg), err, 512)
        if not self._h:
            raise RcorrectorError(err.value.decode() or "rc_create failed")
        self.k = k

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self._L.rc_host_free(self._h, p)
            self._pinned = []
            self._L.rc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RcorrectorError("rc=%d: %s" % (rc, self._L.rc_last_error(self._h).decode()))

    # ---- table ----
    def table_build(self, codes, counts):
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        self._ck(self._L.rc_table_build(self._h, codes.ctypes.data, counts.ctypes.data, len(codes)))

    def table_build_device(self, d_codes, d_counts, n):
        self._ck(self._L.rc_table_build_device(self._h, _ptr(d_codes), _ptr(d_counts), n))

    def load_jfdump(self, path):
        stored = C.c_int64(0)
        self._ck(self._L.rc_table_load_jfdump(self._h, os.fsencode(path), C.byref(stored)))
        return stored.value

    def count_reads_device(self, d_seq, nbytes, min_count=2):
        n = C.c_int64(0)
        self._ck(self._L.rc_table_count_reads_device(self._h, _ptr(d_seq), nbytes, min_count, C.byref(n)))
        return n.value

    def count_begin(self):
        self._ck(self._L.rc_table_count_begin(self._h))

    def count_add(self, arena):
        """arena: bytes / uint8 array of NUL-separated reads in host memory"""
        a = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else np.ascontiguousarray(arena, dtype=np.uint8)
        self._ck(self._L.rc_table_count_add(self._h, a.ctypes.data, a.size))

    def count_add_device(self, d_seq, nbytes):
        self._ck(self._L.rc_table_count_add_device(self._h, _ptr(d_seq), nbytes))

    def count_finish(self, min_count=2):
        n = C.c_int64(0)
        self._ck(self._L.rc_table_count_finish(self._h, min_count, C.byref(n)))
        return n.value

    def write_jfdump(self, path):
        n = C.c_int64(0)
        self._ck(self._L.rc_table_write_jfdump(self._h, os.fsencode(path), C.byref(n)))
        return n.value

    def share_table_of(self, other):
        """Use `other`'s table (same device) instead of an own copy; keeps `other` alive."""
        self._ck(self._L.rc_table_share(self._h, other._h))
        self._table_owner = other

    def replicate_table_of(self, other):
        """An own copy of `other`'s table, device to device (rc_table_replicate)."""
        self._ck(self._L.rc_table_replicate(self._h, other._h))

    def replicate_table_of_async(self, other):
        """The same with the copy left in flight on this context's stream (sync() waits for it): queue the copies to all
        GPUs of a node first, they travel at the same time (rc_table_replicate_async)."""
        self._ck(self._L.rc_table_replicate_async(self._h, other._h))

    def numa_node(self):
        """NUMA node of the host this context's GPU hangs off, -1 if the system does not say (rc_device_numa_node)."""
        return int(self._L.rc_device_numa_node(self._h))

    def lookup(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        out = np.zeros(len(codes), dtype=np.int32)
        self._ck(self._L.rc_table_lookup(self._h, codes.ctypes.data, len(codes), out.ctypes.data))
        return out

    def table_export(self):
        """All stored (canonical code, count) pairs (unspecified order)."""
        cap = int(self.table_stats()["entries"])
        codes = np.zeros(cap, dtype=np.uint64)
        counts = np.zeros(cap, dtype=np.int32)
        n = C.c_size_t(0)
        self._ck(self._L.rc_table_export(self._h, codes.ctypes.data, counts.ctypes.data, cap, C.byref(n)))
        return codes[:n.value], counts[:n.value]

    def table_digest(self):
        """64-bit digest of the table's content (layout independent)."""
        v = C.c_uint64(0)
        self._ck(self._L.rc_table_digest(self._h, C.byref(v)))
        return v.value

    def table_layout(self):
        """0 = WIDE slots, 1 = PACKED slots (rc_table_layout)."""
        r = self._L.rc_table_layout(self._h)
        if r < 0:
            raise RcorrectorError("no table")
        return r

    def table_stats(self):
        b, n, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.rc_table_stats(self._h, C.byref(b), C.byref(n), C.byref(e)))
        return {"bytes": b.value, "buckets": n.value, "entries": e.value}

    # ---- k-mer count spectrum ----
    def count_spectrum(self, max_bin=10000):
        """Arms the counted spectrum (rc_table_count_spectrum): the next count_finish / count_finish_sharded bins every
        k-mer it sees, those below min_count included, into max_bin + 1 bins (the last one: counts >= max_bin).  0: off."""
        self._ck(self._L.rc_table_count_spectrum(self._h, int(max_bin)))

    def kmer_spectrum(self, source="table", max_bin=10000):
        """rc_table_spectrum: (uint64 array freq[max_bin + 1], {"distinct", "total", "unique", "max_count"}) of the current
        table's live entries (source="table") or of what the last armed count saw (source="counted")."""
        src = {"table": 0, "counted": 1}.get(source)
        if src is None:
            raise ValueError("source must be 'table' or 'counted'")
        freq = np.zeros(int(max_bin) + 1, dtype=np.uint64)
        st = _SpectrumStats()
        self._ck(self._L.rc_table_spectrum(self._h, src, freq.ctypes.data, int(max_bin), C.byref(st)))
        return freq, {"distinct": st.distinct, "total": st.total, "unique": st.unique, "max_count": st.max_count}

    # ---- two tables side by side ----
    def table_compare(self, other, max_bin=255):
        """rc_table_compare: this context's table (a) against `other`'s (b; same k, same device; may be this context) --
        {"cells": uint64 array (max_bin + 1, max_bin + 1), cells[i, j] = distinct canonical k-mers whose count folds to i here
        and to j there (0: not held; the last bin: at least max_bin), and the fields of rc_table_compare_stats as ints}."""
        n = int(max_bin) + 1 if 1 <= int(max_bin) <= 1023 else 1   # (a max_bin out of range: the library refuses it)
        cells = np.zeros((n, n), dtype=np.uint64)
        st = _CompareStats()
        self._ck(self._L.rc_table_compare(self._h, other._h, int(max_bin) & 0xFFFFFFFF, cells.ctypes.data, C.byref(st)))
        out = {f: int(getattr(st, f)) for f in COMPARE_FIELDS}
        out["cells"] = cells
        return out

    # ---- recount session: the spectrum of reads after correction, and the k-mers the table does not hold ----
    def recount_begin(self, max_bin=10000):
        """rc_recount_begin: opens a counting session that builds no table and leaves the table, the kept arenas and a
        counted spectrum alone; recount_finish bins into max_bin + 1 bins (the last one: counts >= max_bin)."""
        self._ck(self._L.rc_recount_begin(self._h, int(max_bin)))
        self._recount_bin = int(max_bin)

    def recount_add(self, arena):
        """arena: bytes / uint8 array of NUL-separated reads in host memory"""
        a = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else np.ascontiguousarray(arena, dtype=np.uint8)
        self._ck(self._L.rc_recount_add(self._h, a.ctypes.data, a.size))

    def recount_add_device(self, d_seq, nbytes):
        """an arena in HBM, e.g. what correct_device has corrected in place"""
        self._ck(self._L.rc_recount_add_device(self._h, _ptr(d_seq), nbytes))

    def recount_follow(self, on=True):
        """rc_recount_follow: while a session is open, every batch that completes on this context (correct_batch, wait,
        wait_packed, wait_resident) leaves its corrected arena with the session, device to device."""
        self._ck(self._L.rc_recount_follow(self._h, 1 if on else 0))

    def recount_finish(self):
        """rc_recount_finish: (uint64 array freq[max_bin + 1], {"distinct", "total", "unique", "max_count", "absent_distinct",
        "absent_total"}) of the k-mers of everything added since recount_begin; absent = not in this context's table."""
        freq = np.zeros(getattr(self, "_recount_bin", 0) + 1, dtype=np.uint64)
        st = _RecountStats()
        self._ck(self._L.rc_recount_finish(self._h, freq.ctypes.data, C.byref(st)))
        a = st.all
        return freq, {"distinct": a.distinct, "total": a.total, "unique": a.unique, "max_count": a.max_count,
                      "absent_distinct": st.absent_distinct, "absent_total": st.absent_total}

    # ---- correction report: what was changed, where in the read, and in which reads ----
    def change_report_begin(self):
        """rc_change_report_begin: from now on every batch that completes on this context (any entry point, slot lanes
        included) is compared on the GPU with its uncorrected arena and counted, each batch once."""
        self._ck(self._L.rc_change_report_begin(self._h))

    def change_report(self):
        """rc_change_report_get: dict of uint64 arrays named and shaped as the fields of rc_change_report -- reads,
        reads_changed, reads_unfixable, changes [2 mates]; len_hist, by_pos5, by_pos3 [2][1024]; subst [5 from: A C G T other]
        [4 to: A C G T]; by_qual [low, high, none]; per_read [65].  The report stays armed and cumulative."""
        r = _ChangeReport()
        self._ck(self._L.rc_change_report_get(self._h, C.byref(r)))
        return {name: np.ctypeslib.as_array(getattr(r, name)).astype(np.uint64) for name, _ in _ChangeReport._fields_}

    def change_report_end(self):
        """rc_change_report_end: disarms the report and frees what it held."""
        self._ck(self._L.rc_change_report_end(self._h))

    # ---- the per-read payloads' one-shot registrations (weak_profile_into, read_depth_into, read_screen_into) ----
    def _payload_into(self, kind, slot, total_reads, out, register, *also_held):
        """The (total_reads, 4) int32 array of a payload registration: `out` checked, or a page-locked one allocated; handed
        to register(address), then held under (kind, slot) with also_held (the library writes / reads them until the batch's
        wait returns)."""
        total_reads = int(total_reads)
        if out is None:
            out = self.host_array(total_reads * 4, dtype=np.int32).reshape(total_reads, 4)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags.c_contiguous and out.shape == (total_reads, 4)):
            raise TypeError("out must be a C-contiguous int32 numpy array of shape (total_reads, 4)")
        self._ck(register(out.ctypes.data))
        self.__dict__.setdefault("_payload_out", {})[(kind, int(slot))] = (out,) + also_held
        return out

    # ---- per-read weak-k-mer profile: weak windows, bad prefix / suffix, uncovered bases ----
    def weak_profile_device(self, d_seq, d_off, n_reads, nbytes, max_read_len, d_out, min_count=1):
        """rc_weak_profile_device: the reads of an arena in HBM as they are; d_out: device memory for n_reads x 4 int32
        (weak, bad_prefix, bad_suffix, uncovered: rc_read_weak).  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_weak_profile_device(self._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, max_read_len, int(min_count), _ptr(d_out)))

    def weak_profile_into(self, slot, total_reads, min_count=1, out=None):
        """rc_weak_profile_into: the next batch submitted into `slot` (correct_batch: slot 0) also profiles its corrected reads.
        Returns a page-locked (total_reads, 4) int32 array -- columns weak, bad_prefix, bad_suffix, uncovered, rows indexed like
        ret / l / m / h -- that the batch's wait fills (out: a C-contiguous int32 array of that shape to fill instead, e.g. a
        pageable one).  One shot: every submit consumes the registration."""
        return self._payload_into("weak", slot, total_reads, out, lambda p: self._L.rc_weak_profile_into(self._h, int(slot), p, int(min_count)))

    def weak_profile_withdraw(self, slot):
        """rc_weak_profile_into(out = NULL): the next batch of `slot` is not profiled after all"""
        self._ck(self._L.rc_weak_profile_into(self._h, int(slot), None, 1))

    # ---- per-read k-mer depth: valid windows and the quartiles of their counts ----
    def read_depth_device(self, d_seq, d_off, n_reads, nbytes, max_read_len, d_out):
        """rc_read_depth_device: the reads of an arena in HBM as they are; d_out: device memory for n_reads x 4 int32
        (valid, q1, median, q3: rc_read_depth).  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_read_depth_device(self._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, int(max_read_len), _ptr(d_out)))

    def read_depth_into(self, slot, total_reads, out=None):
        """rc_read_depth_into: the next batch submitted into `slot` (correct_batch: slot 0) also takes the k-mer depth of its
        corrected reads.  Returns a page-locked (total_reads, 4) int32 array -- columns valid, q1, median, q3, rows indexed like
        ret / l / m / h -- that the batch's wait fills (out: a C-contiguous int32 array of that shape to fill instead, e.g. a
        pageable one).  One shot: every submit consumes the registration."""
        return self._payload_into("depth", slot, total_reads, out, lambda p: self._L.rc_read_depth_into(self._h, int(slot), p))

    def read_depth_withdraw(self, slot):
        """rc_read_depth_into(out = NULL): the next batch of `slot` has its depth not taken after all"""
        self._ck(self._L.rc_read_depth_into(self._h, int(slot), None))

    # ---- normalisation by k-mer depth: one byte per unit from the depths of its mates ----
    def norm_select_device(self, d_depth, n_units, mode, unit_base, target, min_cov, seed, max_bin, d_keep, d_tally):
        """rc_norm_select_device: d_depth: what read_depth_device left in HBM (n_units rows in mode 0, 2 * n_units in modes 1
        and 2); d_keep: device memory for n_units bytes (0 over, 1 kept, 2 low, 3 no valid window: RC_NORM_*); the outcomes and the
        unit depths are ADDED to d_tally: device memory for 4 + 2 * (max_bin + 1) uint64, zeroed by the caller.  unit_base: the
        units of the whole input in front of this batch.  Needs no table.  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_norm_select_device(self._h, _ptr(d_depth), int(n_units), int(mode), int(unit_base), int(target), int(min_cov), int(seed),
                                               int(max_bin), _ptr(d_keep), _ptr(d_tally)))

    # ---- read trimming: per read, how many bases to keep after the quality, adapter and pair cuts ----
    def read_trim_device(self, d_seq, d_qual, d_off, n_reads, nbytes, max_read_len, mode, params, d_out, d_keep=None, d_tally=None):
        """rc_read_trim_device: the reads of an arena in HBM as they are, d_qual (may be None) their quality bytes at the same
        offsets; params: trim_params(...) (None: the defaults); d_out: device memory for n_reads x 4 int32 (keep_len, cut_qual,
        cut_adapter, cut_pair: READ_TRIM_DTYPE); d_keep (may be None): one byte per unit, 1 kept, 0 short; the counts are ADDED to
        d_tally (may be None): device memory for TRIM_TALLY_WORDS uint64, zeroed by the caller (trim_tally_dict reads a copy of
        it).  Needs no table.  Asynchronous: sync() to wait."""
        p = trim_params() if params is None else params
        self._ck(self._L.rc_read_trim_device(self._h, _ptr(d_seq), _ptr(d_qual), _ptr(d_off), int(n_reads), int(nbytes), int(max_read_len), int(mode),
                                             C.byref(p), _ptr(d_out), _ptr(d_keep), _ptr(d_tally)))

    # ---- read merging: overlapping mates into one read each, a new compact arena written on the device ----
    def read_merge_device(self, d_seq, d_qual, d_off, n_reads, nbytes, max_read_len, mode, params, d_rows, d_mseq, d_mqual, d_moff, out_cap, d_tally=None):
        """rc_read_merge_device: the pairs (mode 1: in halves, 2: interleaved) of an arena in HBM as they are, d_qual (may be None)
        their quality bytes at the same offsets; params: merge_params(...) (None: the defaults); d_rows: device memory for
        n_reads / 2 x 4 int32 (merged_len, d, v, m: READ_MERGE_DTYPE); the merged reads go to d_mseq, and their qualities to
        d_mqual (may be None), out_cap >= nbytes bytes each on a 16-byte boundary, at the offsets d_moff (n_reads / 2 + 1 uint32;
        the last is the new arena's size); an unmerged pair becomes an empty read.  The counts are ADDED to d_tally (may be
        None): device memory for MERGE_TALLY_WORDS uint64, zeroed by the caller (merge_tally_dict reads a copy of it).  The new
        arena is one every per-read entry point takes in mode 0.  Needs no table.  Asynchronous: sync() to wait."""
        p = merge_params() if params is None else params
        self._ck(self._L.rc_read_merge_device(self._h, _ptr(d_seq), _ptr(d_qual), _ptr(d_off), int(n_reads), int(nbytes), int(max_read_len), int(mode),
                                              C.byref(p), _ptr(d_rows), _ptr(d_mseq), _ptr(d_mqual), _ptr(d_moff), int(out_cap), _ptr(d_tally)))

    # ---- per-read screen against a second k-mer set: valid and hit windows, covered bases, longest run of hits ----
    def read_screen_device(self, screen, d_seq, d_off, n_reads, nbytes, max_read_len, d_out, min_count=1):
        """rc_read_screen_device: the reads of an arena in HBM as they are against the table of `screen` (a Context of the same
        k on the same device; it may be this one); d_out: device memory for n_reads x 4 int32 (valid, hits, covered, longest:
        rc_read_screen).  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_read_screen_device(self._h, screen._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, int(max_read_len), int(min_count),
                                               _ptr(d_out)))

    def read_screen_into(self, slot, total_reads, screen, min_count=1, out=None):
        """rc_read_screen_into: the next batch submitted into `slot` (correct_batch: slot 0) also has its corrected reads
        screened against the table of `screen`.  Returns a page-locked (total_reads, 4) int32 array -- columns valid, hits,
        covered, longest, rows indexed like ret / l / m / h -- that the batch's wait fills (out: a C-contiguous int32 array of
        that shape to fill instead, e.g. a pageable one).  One shot: every submit consumes the registration.  `screen` must
        keep its table until that wait; this context holds on to it until the next registration of the slot."""
        return self._payload_into("screen", slot, total_reads, out,
                                  lambda p: self._L.rc_read_screen_into(self._h, int(slot), screen._h, int(min_count), p), screen)

    def read_screen_withdraw(self, slot):
        """rc_read_screen_into(out = NULL): the next batch of `slot` is not screened after all"""
        self._ck(self._L.rc_read_screen_into(self._h, int(slot), None, 1, None))

    # ---- duplicate census: exact copies among the reads / pairs, before and after correction ----
    def dup_census_begin(self):
        """rc_dup_census_begin: from now on every batch that completes on this context (any batch entry point, slot lanes
        included) leaves a 128-bit key per unit (a read; a pair in modes 1 and 2) of its bases as uploaded and as corrected."""
        self._ck(self._L.rc_dup_census_begin(self._h))

    def dup_census(self, max_bin=10000):
        """rc_dup_census_get: {"units", "distinct_before", "distinct_after": int; "copies_before", "copies_after": uint64 arrays
        of max_bin + 1 -- entry c: distinct units that occur exactly c times, the last one max_bin times or more}.  The census
        stays open and cumulative; the keys are kept."""
        before = np.zeros(int(max_bin) + 1, dtype=np.uint64)
        after = np.zeros(int(max_bin) + 1, dtype=np.uint64)
        r = _DupCensus(0, 0, 0, before.ctypes.data, after.ctypes.data)
        self._ck(self._L.rc_dup_census_get(self._h, int(max_bin), C.byref(r)))
        return {"units": int(r.units), "distinct_before": int(r.distinct_before), "distinct_after": int(r.distinct_after),
                "copies_before": before, "copies_after": after}

    def dup_census_end(self):
        """rc_dup_census_end: closes the census and frees the keys."""
        self._ck(self._L.rc_dup_census_end(self._h))

    def read_keys_device(self, d_seq, d_off, n_reads, nbytes, mode, d_keys):
        """rc_read_keys_device: the keys of an arena in HBM as it is; d_keys: device memory (16-byte aligned) for two uint64 per
        unit -- n_reads units in mode 0, n_reads / 2 pairs in modes 1 and 2.  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_read_keys_device(self._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, int(mode), _ptr(d_keys)))

    def dup_census_merge(self, other):
        """rc_dup_census_merge: appends the keys `other` (a Context with an open census, on any device) has accumulated to this
        context's; other keeps its own."""
        self._ck(self._L.rc_dup_census_merge(self._h, other._h))

    # ---- recurrent-correction census: the sites where one fix was made in many reads ----
    def recur_census_begin(self):
        """rc_recur_census_begin: from now on every batch that completes on this context (any batch entry point, slot lanes
        included) leaves a 61-bit site key per contexted change; submits block until their kernels have run while it is open."""
        self._ck(self._L.rc_recur_census_begin(self._h))

    def recur_census(self, max_bin, min_count=2, max_sites=1000):
        """rc_recur_census_get: {"changes", "contexted", "clipped", "sites", "sites_recurrent", "changes_at_recurrent", "n_top":
        int; "recur": uint64 array of max_bin + 1 -- entry c: sites with exactly c changes, the last one max_bin or more;
        "top_key", "top_count": uint64 arrays of n_top, the sites with min_count changes or more by count descending, then key
        ascending, at most max_sites; "top_sites": [(count, from_letter, to_letter, 29-mer)] decoded from them}.  The census
        stays open and cumulative; the keys are kept."""
        recur = np.zeros(int(max_bin) + 1, dtype=np.uint64)
        top_key = np.zeros(max(int(max_sites), 1), dtype=np.uint64)
        top_count = np.zeros(max(int(max_sites), 1), dtype=np.uint64)
        r = _RecurCensus(0, 0, 0, 0, 0, 0, recur.ctypes.data, top_key.ctypes.data, top_count.ctypes.data, 0)
        self._ck(self._L.rc_recur_census_get(self._h, int(max_bin), int(min_count), int(max_sites), C.byref(r)))
        n = int(r.n_top)
        top_key, top_count = top_key[:n].copy(), top_count[:n].copy()
        return {"changes": int(r.changes), "contexted": int(r.contexted), "clipped": int(r.clipped), "sites": int(r.sites),
                "sites_recurrent": int(r.sites_recurrent), "changes_at_recurrent": int(r.changes_at_recurrent), "n_top": n,
                "recur": recur, "top_key": top_key, "top_count": top_count,
                "top_sites": [(int(c),) + recur_key_decode(k) for k, c in zip(top_key, top_count)]}

    def recur_census_end(self):
        """rc_recur_census_end: closes the census and frees the keys."""
        self._ck(self._L.rc_recur_census_end(self._h))

    def recur_census_merge(self, other):
        """rc_recur_census_merge: appends the keys and totals `other` (a Context with an open census, on any device) has
        accumulated to this context's; other keeps its own."""
        self._ck(self._L.rc_recur_census_merge(self._h, other._h))

    def change_keys_device(self, d_before, d_after, d_off, n_reads, nbytes, d_keys, cap, d_counts):
        """rc_change_keys_device: the site keys of the contexted changes between two arenas in HBM (same offsets, same alignment
        modulo 16) appended to d_keys (device memory for cap uint64), never past cap; d_counts: device memory for three uint64
        -- changes, contexted, keys found (exact even where cap was too small).  Asynchronous: sync() to wait."""
        self._ck(self._L.rc_change_keys_device(self._h, _ptr(d_before), _ptr(d_after), _ptr(d_off), n_reads, nbytes, _ptr(d_keys), int(cap),
                                               _ptr(d_counts)))

    # ---- k-mer trust profile by read position, before and after correction ----
    def trust_profile_begin(self, min_count=1):
        """rc_trust_profile_begin: from now on every batch that completes on this context (any batch entry point, slot lanes
        included) counts, per mate and window position from either end, its solid and weak k-windows -- of its bases as
        uploaded and as corrected.  A k-mer the table holds fewer than min_count times is weak."""
        self._ck(self._L.rc_trust_profile_begin(self._h, int(min_count)))

    def trust_profile(self):
        """rc_trust_profile_get: {"k", "min_count": int; "reads": uint64[2]; "before", "after": dicts of the uint64 arrays
        "windows", "solid5", "weak5", "solid3", "weak3", each (2, RC_TRUST_MAX_LEN): [mate][position]}.  The profile stays open
        and cumulative."""
        r = _TrustProfile()
        self._ck(self._L.rc_trust_profile_get(self._h, C.byref(r)))
        version = lambda c: {n: np.ctypeslib.as_array(getattr(c, n)).astype(np.uint64) for n in TRUST_FIELDS}   # noqa: E731
        return {"k": int(r.k), "min_count": int(r.min_count), "reads": np.array(list(r.reads), dtype=np.uint64),
                "before": version(r.before), "after": version(r.after)}

    def trust_profile_end(self):
        """rc_trust_profile_end: closes the profile and frees its counts and scratch."""
        self._ck(self._L.rc_trust_profile_end(self._h))

    # ---- mate-overlap report: where the mates of a pair disagree, before and after correction ----
    def mate_overlap_begin(self, min_overlap=30, max_mismatch_pct=10):
        """rc_mate_overlap_begin: from now on every batch of pairs that completes on this context (any batch entry point, slot
        lanes included) is counted once: mate 1 against the reverse complement of mate 2 at the offset chosen on the bases as
        they arrived, before and after correction.  Needs no table."""
        self._ck(self._L.rc_mate_overlap_begin(self._h, int(min_overlap), int(max_mismatch_pct)))

    def mate_overlap(self):
        """rc_mate_overlap_get: a dict named as the struct's fields -- ints ("min_overlap", "max_mismatch_pct", "pairs",
        "overlapping", "compared_before", ...) and uint64 arrays: "frag" (RC_OVERLAP_FRAG_LEN), "compared5", "disagree5_before",
        "disagree5_after" (2, RC_OVERLAP_MAX_LEN): [mate][position].  The session stays open."""
        r = _MateOverlap()
        self._ck(self._L.rc_mate_overlap_get(self._h, C.byref(r)))
        return mate_overlap_dict(np.frombuffer(bytes(r), np.uint64))

    def mate_overlap_end(self):
        """rc_mate_overlap_end: closes the session and frees its counts."""
        self._ck(self._L.rc_mate_overlap_end(self._h))

    def mate_overlap_device(self, d_before, d_after, d_off, n_reads, nbytes, max_read_len, mode, d_counts, min_overlap=30, max_mismatch_pct=10):
        """rc_mate_overlap_device: the pairs of two arenas in HBM that share d_off, the bases as read and as corrected (may be
        one and the same), ADDED to d_counts: device memory for one rc_mate_overlap (OVERLAP_WORDS uint64, zeroed by the caller;
        mate_overlap_dict reads a copy of it).  Asynchronous on the context's stream."""
        self._ck(self._L.rc_mate_overlap_device(self._h, _ptr(d_before), _ptr(d_after), _ptr(d_off), n_reads, nbytes, int(max_read_len), int(mode),
                                                int(min_overlap), int(max_mismatch_pct), _ptr(d_counts)))

    def trust_profile_device(self, d_seq, d_off, n_reads, nbytes, max_read_len, mode, d_counts, min_count=1):
        """rc_trust_profile_device: the reads of an arena in HBM as they are, ADDED to d_counts: device memory for one
        rc_trust_counts (5 x 2 x RC_TRUST_MAX_LEN uint64: windows, solid5, weak5, solid3, weak3), zeroed by the caller.
        Asynchronous: sync() to wait."""
        self._ck(self._L.rc_trust_profile_device(self._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, int(max_read_len), int(mode), int(min_count),
                                                 _ptr(d_counts)))

    # ---- run parameters ----
    def estimate_error_rate(self, wk=0.95):
        r = C.c_double(0)
        self._ck(self._L.rc_estimate_error_rate(self._h, wk, C.byref(r)))
        return r.value

    def bad_quality_from_hist(self, first_hist, last_hist, total):
        fh = np.ascontiguousarray(first_hist, dtype=np.int32)
        lh = np.ascontiguousarray(last_hist, dtype=np.int32)
        return self._L.rc_bad_quality_from_hist(fh.ctypes.data, lh.ctypes.data, int(total))

    def set_run_params(self, error_rate, bad_quality):
        if isinstance(bad_quality, int):
            bad_quality = bytes([bad_quality & 0xFF])
        self._ck(self._L.rc_set_run_params(self._h, error_rate, bad_quality))

    def set_quality_bits(self, on=True):
        """Quality arenas handed to this context are bit arrays (rc_set_quality_bits)."""
        self._ck(self._L.rc_set_quality_bits(self._h, 1 if on else 0))

    def pack_quality_bits(self, qual, bad_quality, out=None):
        """uint8 quality arena -> bit array (bit p = qual[p] > bad_quality), rc_pack_quality_bits."""
        qual = self._arena(qual, "qual")
        if isinstance(bad_quality, int):
            bad_quality = bytes([bad_quality & 0xFF])
        if out is None:
            out = np.zeros((qual.size + 7) // 8, dtype=np.uint8)
        self._L.rc_pack_quality_bits(qual.ctypes.data, qual.size, bad_quality, out.ctypes.data)
        return out

    # ---- correction ----
    @staticmethod
    def _arena(a, what):
        # the library reads and (for seq) rewrites these buffers through raw pointers: a wrong dtype or a
        # strided view would silently be garbage, so refuse instead of converting (seq is corrected in place)
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
            raise TypeError("%s must be a C-contiguous uint8 numpy array" % what)
        return a

    def _batch(self, mode, seq, qual, off, seq2, qual2, off2, res=None):
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        total = 2 * n if mode == 1 else n
        if res is None:
            res = [np.zeros(total, dtype=np.int32) for _ in range(4)]
        b = _Batch()
        b.mode, b.n = mode, n
        keep = [off, res]
        b.seq, b.qual, b.off = self._arena(seq, "seq").ctypes.data, self._arena(qual, "qual").ctypes.data, off.ctypes.data
        if mode == 1:
            off2 = np.ascontiguousarray(off2, dtype=np.uint32)
            keep.append(off2)
            b.seq2, b.qual2, b.off2 = self._arena(seq2, "seq2").ctypes.data, self._arena(qual2, "qual2").ctypes.data, off2.ctypes.data
        b.ret, b.l, b.m, b.h = (r.ctypes.data for r in res)
        return b, res, keep

    def correct_batch(self, mode, seq, qual, off, seq2=None, qual2=None, off2=None):
        """Host-buffer batch (rc_correct_batch).  seq arenas are corrected IN PLACE.
        Returns (ret, l, m, h)."""
        b, res, _keep = self._batch(mode, seq, qual, off, seq2, qual2, off2)
        self._ck(self._L.rc_correct_batch(self._h, C.byref(b)))
        return tuple(res)

    def submit(self, slot, mode, seq, qual, off, seq2=None, qual2=None, off2=None, res=None):
        """rc_submit: starts a batch in `slot`; wait(slot) returns (ret, l, m, h).  The arrays must not
        be touched until then.  res: optional list of four int32 arrays to receive the results
        (e.g. pinned ones from host_array)."""
        b, res, keep = self._batch(mode, seq, qual, off, seq2, qual2, off2, res)
        self._ck(self._L.rc_submit(self._h, C.byref(b), slot))
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[slot] = (res, keep, (seq, qual, seq2, qual2))

    def wait(self, slot):
        self._ck(self._L.rc_wait(self._h, slot))
        res, _keep, _arr = self._inflight.pop(slot)
        return tuple(res)

    # ---- the packed boundary (rc_packed_batch) ----
    def pack_bases(self, arena, bases=None, exc_pos=None, exc_chr=None):
        """2-bit codes + the letters outside ACGT of a byte arena (rc_pack_bases).  Returns (bases, exc_pos, exc_chr):
        the given arrays (e.g. page-locked ones) or new ones, the exception arrays cut to their length."""
        arena = self._arena(arena, "arena")
        nw = (arena.size + 15) // 16
        if bases is None:
            bases = np.zeros(nw, dtype=np.uint32)
        cap = 0 if exc_pos is None else len(exc_pos)
        n = self._L.rc_pack_bases(arena.ctypes.data, 0, arena.size, bases.ctypes.data, exc_pos.ctypes.data if cap else None,
                                  exc_chr.ctypes.data if cap else None, cap)
        if n > cap:   # (first call without room, or too little of it)
            exc_pos, exc_chr = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
            self._L.rc_pack_bases(arena.ctypes.data, 0, arena.size, bases.ctypes.data, exc_pos.ctypes.data, exc_chr.ctypes.data, n)
        if exc_pos is None:
            exc_pos, exc_chr = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
        return bases, exc_pos[:n], exc_chr[:n]

    def submit_packed(self, slot, mode, nbytes, off, bases, qual_bits, exc_pos, exc_chr, res=None, fix_pos=None, fix_chr=None, fix_cap=None):
        """rc_submit_packed: off over the whole arena (mode 1: first mates then second mates, 2 n + 1 entries).
        wait_packed(slot) returns (ret, l, m, h, fix_pos, fix_chr)."""
        off = np.ascontiguousarray(off, dtype=np.uint32)
        total = len(off) - 1
        if res is None:
            res = [np.zeros(total, dtype=np.int32) for _ in range(4)]
        if fix_pos is None:
            fix_cap = int(nbytes) if fix_cap is None else fix_cap
            fix_pos, fix_chr = np.zeros(fix_cap, dtype=np.uint32), np.zeros(fix_cap, dtype=np.uint8)
        b = _PackedBatch()
        b.mode, b.n, b.nbytes = mode, (total // 2 if mode == 1 else total), int(nbytes)
        b.off, b.bases = off.ctypes.data, bases.ctypes.data
        b.qual_bits = None if qual_bits is None else qual_bits.ctypes.data
        b.n_exc = len(exc_pos)
        b.exc_pos, b.exc_chr = (exc_pos.ctypes.data, exc_chr.ctypes.data) if len(exc_pos) else (None, None)
        b.ret, b.l, b.m, b.h = (r.ctypes.data for r in res)
        b.fix_pos, b.fix_chr, b.fix_cap = fix_pos.ctypes.data, fix_chr.ctypes.data, len(fix_pos)
        self._ck(self._L.rc_submit_packed(self._h, C.byref(b), slot))
        if not hasattr(self, "_inflight_packed"):
            self._inflight_packed = {}
        self._inflight_packed[slot] = (b, res, fix_pos, fix_chr, (off, bases, qual_bits, exc_pos, exc_chr))

    def wait_packed(self, slot):
        self._ck(self._L.rc_wait_packed(self._h, slot))
        b, res, fix_pos, fix_chr, _keep = self._inflight_packed.pop(slot)
        return tuple(res) + (fix_pos[:b.n_fix], fix_chr[:b.n_fix])

    def set_slot_lanes(self, on=True):
        """slots > 0 of the asynchronous entry points in contexts of their own (kernels of batches in flight overlap) or not"""
        self._ck(self._L.rc_set_slot_lanes(self._h, 1 if on else 0))

    def device_memory(self):
        """(free, total) bytes of the context's GPU memory right now"""
        f, t = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.rc_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    # ---- reads the k-mer counter kept in HBM (rc_resident_batch) ----
    def count_keep(self, on=True):
        self._ck(self._L.rc_table_count_keep(self._h, 1 if on else 0))

    def count_arenas(self):
        """bytes of the arenas the counter kept, in the order they were added"""
        n = C.c_size_t(0)
        self._ck(self._L.rc_table_count_arenas(self._h, C.byref(n), None, 0))
        b = np.zeros(max(1, n.value), dtype=np.uint64)
        self._ck(self._L.rc_table_count_arenas(self._h, C.byref(n), b.ctypes.data, len(b)))
        return b[:n.value]

    def count_park(self):
        """rc_table_count_park: the arenas added since count_begin become kept arenas; nothing is counted, no table built"""
        self._ck(self._L.rc_table_count_park(self._h))

    def count_finish_sharded(self, others, min_count=2):
        """rc_table_count_finish_sharded over [self] + others (contexts with open counting sessions, one per GPU): the
        table is built in this context; returns the number of entries kept"""
        hs = (C.c_void_p * (1 + len(others)))(self._h, *[o._h for o in others])
        n = C.c_int64(0)
        self._ck(self._L.rc_table_count_finish_sharded(hs, 1 + len(others), min_count, C.byref(n)))
        return n.value

    def count_release(self):
        self._ck(self._L.rc_table_count_release(self._h))

    def submit_resident(self, slot, mode, off, qual_bits, arena_a, begin_a, bytes_a, arena_b=0, begin_b=0, bytes_b=0, res=None, fix_pos=None,
                        fix_chr=None, fix_cap=None):
        """rc_submit_resident: the batch is a byte range of kept arena `arena_a` (mode 1: + one of `arena_b`); off over the
        batch's own arena (bytes_a + bytes_b bytes).  wait_resident(slot) returns (ret, l, m, h, fix_pos, fix_chr)."""
        off = np.ascontiguousarray(off, dtype=np.uint32)
        total = len(off) - 1
        if res is None:
            res = [np.zeros(total, dtype=np.int32) for _ in range(4)]
        if fix_pos is None:
            fix_cap = int(bytes_a + bytes_b) if fix_cap is None else fix_cap
            fix_pos, fix_chr = np.zeros(fix_cap, dtype=np.uint32), np.zeros(fix_cap, dtype=np.uint8)
        b = _ResidentBatch()
        b.mode, b.n = mode, (total // 2 if mode == 1 else total)
        b.arena_a, b.begin_a, b.bytes_a = int(arena_a), int(begin_a), int(bytes_a)
        b.arena_b, b.begin_b, b.bytes_b = int(arena_b), int(begin_b), int(bytes_b)
        b.off = off.ctypes.data
        b.qual_bits = None if qual_bits is None else qual_bits.ctypes.data
        b.ret, b.l, b.m, b.h = (r.ctypes.data for r in res)
        b.fix_pos, b.fix_chr, b.fix_cap = fix_pos.ctypes.data, fix_chr.ctypes.data, len(fix_pos)
        self._ck(self._L.rc_submit_resident(self._h, C.byref(b), slot))
        if not hasattr(self, "_inflight_resident"):
            self._inflight_resident = {}
        self._inflight_resident[slot] = (b, res, fix_pos, fix_chr, (off, qual_bits))

    def wait_resident(self, slot):
        self._ck(self._L.rc_wait_resident(self._h, slot))
        b, res, fix_pos, fix_chr, _keep = self._inflight_resident.pop(slot)
        return tuple(res) + (fix_pos[:b.n_fix], fix_chr[:b.n_fix])

    def apply_fixes(self, arena, fix_pos, fix_chr):
        arena = self._arena(arena, "arena")
        fp, fc = np.ascontiguousarray(fix_pos, dtype=np.uint32), np.ascontiguousarray(fix_chr, dtype=np.uint8)
        self._L.rc_apply_fixes(arena.ctypes.data, fp.ctypes.data, fc.ctypes.data, len(fp))

    def host_array(self, n, dtype=np.uint8):
        """A page-locked numpy array (rc_host_alloc): rc_submit DMAs straight from / into it.
        Freed with the context."""
        dt = np.dtype(dtype)
        p = C.c_void_p(0)
        self._ck(self._L.rc_host_alloc(self._h, max(1, n * dt.itemsize), C.byref(p)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p.value)
        buf = (C.c_uint8 * (n * dt.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt, count=n)


    def correct_device(self, mode, n_reads, nbytes, max_read_len, d_seq, d_qual, d_off, d_ret, d_l, d_m, d_h):
        b = _DeviceBatch(mode, n_reads, nbytes, max_read_len, _ptr(d_seq), _ptr(d_qual), _ptr(d_off),
                         _ptr(d_ret), _ptr(d_l), _ptr(d_m), _ptr(d_h))
        self._ck(self._L.rc_correct_device(self._h, C.byref(b)))

    def strong_threshold_device(self, d_seq, d_off, n_reads, nbytes, max_read_len, d_strong):
        self._ck(self._L.rc_strong_threshold_device(self._h, _ptr(d_seq), _ptr(d_off), n_reads, nbytes, max_read_len, _ptr(d_strong)))

    # ---- one read per call (ErrorCorrection.h:26-28) ----
    def strong_threshold_read(self, seq):
        """GetStrongTrustedThreshold of one read (bytes)."""
        out = C.c_int32(0)
        self._ck(self._L.rc_strong_threshold_read(self._h, bytes(seq), C.byref(out)))
        return out.value

    def correct_read(self, seq, qual, pair_strong_threshold=-1):
        """ErrorCorrection of one read: returns (return value, corrected read as bytes)."""
        buf = C.create_string_buffer(bytes(seq))
        out = C.c_int32(0)
        self._ck(self._L.rc_correct_read(self._h, buf, None if qual is None else bytes(qual), int(pair_strong_threshold), C.byref(out)))
        return out.value, buf.value

    def kmer_info_read(self, seq):
        """GetKmerInformation of one read: (l, m, h)."""
        l, m, h = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self._L.rc_kmer_info_read(self._h, bytes(seq), C.byref(l), C.byref(m), C.byref(h)))
        return l.value, m.value, h.value

    def probe_device(self, d_seq, nbytes, d_counts):
        self._ck(self._L.rc_probe_device(self._h, _ptr(d_seq), nbytes, _ptr(d_counts)))

    def sync(self):
        self._ck(self._L.rc_sync(self._h))

    # ---- measurement ----
    def profile(self, on=True):
        """on: False/0 off, True/1 kernel timers, 2 also the instrumented correction kernel."""
        self._ck(self._L.rc_profile_enable(self._h, int(on)))

    def profile_correct_counters(self):
        """(reads handed to the correction kernel, their gather rounds, table buckets read) since the last reset."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.rc_profile_correct_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def profile_read_rounds(self, d_rounds=None):
        """int32 device tensor (one entry per read, zeroed) that the instrumented correction kernel fills with every read's
        gather rounds; None switches it off."""
        self._ck(self._L.rc_profile_read_rounds(self._h, None if d_rounds is None else d_rounds.data_ptr()))

    def profile_reset(self):
        self._ck(self._L.rc_profile_reset(self._h))

    def profile_get(self, kernel):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._ck(self._L.rc_profile_get(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def selftest_get_bound(self, c, error_rate):
        """GetBound(c) as the kernels evaluate it: (int32 array, float64 array)."""
        c = np.ascontiguousarray(c, dtype=np.int32)
        oi = np.zeros(len(c), dtype=np.int32)
        od = np.zeros(len(c), dtype=np.float64)
        self._ck(self._L.rc_selftest_get_bound(self._h, c.ctypes.data, len(c), error_rate, oi.ctypes.data, od.ctypes.data))
        return oi, od

    def debug_routes(self, n):
        """Test support (rc_debug_routes): (cls uint8[n], cand uint8[n], runs uint64[n]) of the last batch correct_batch /
        correct_device ran -- which kernel finished each read.  Raises where the arrays do not describe the whole batch."""
        cls, cand, runs = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        self._ck(self._L.rc_debug_routes(self._h, cls.ctypes.data, cand.ctypes.data, runs.ctypes.data, n))
        return cls, cand, runs

    def debug_pipeline(self):
        """Test support (rc_debug_pipeline): (batches, chunks) -- the batches this context and its slot lanes ran as a chunked
        pipeline (RC_PIPELINE_CHUNKS) and the non-empty chunks those launched, since the context was made."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.rc_debug_pipeline(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def selftest_transport_packed(self, packed, nbytes, off, exc_pos, exc_chr, after, cap):
        """Test support (rc_selftest_transport_packed): the packed boundary's kernels alone.  Returns (unpacked, n_fix, fix_pos,
        fix_chr): the whole device arena after the expansion (round16(nbytes) + SELFTEST_ARENA_SLACK bytes, SELFTEST_CANARY where
        nothing was written), the number of fixes between the packed codes and `after`, and the fix arrays of cap +
        SELFTEST_FIX_SLACK entries (canary bytes where nothing was written)."""
        packed, off = np.ascontiguousarray(packed, dtype=np.uint32), np.ascontiguousarray(off, dtype=np.uint32)
        exc_pos, exc_chr = np.ascontiguousarray(exc_pos, dtype=np.uint32), np.ascontiguousarray(exc_chr, dtype=np.uint8)
        after = np.ascontiguousarray(after, dtype=np.uint8)
        nbytes, cap = int(nbytes), int(cap)
        if len(packed) != (nbytes + 15) // 16 or len(after) != nbytes or len(exc_pos) != len(exc_chr) or len(off) < 1:
            raise ValueError("selftest_transport_packed: the arrays do not describe an arena of %d bytes" % nbytes)
        unpacked = np.zeros((nbytes + 15) // 16 * 16 + SELFTEST_ARENA_SLACK, np.uint8)
        n_fix = np.zeros(1, np.uint32)
        fix_pos, fix_chr = np.zeros(cap + SELFTEST_FIX_SLACK, np.uint32), np.zeros(cap + SELFTEST_FIX_SLACK, np.uint8)
        self._ck(self._L.rc_selftest_transport_packed(self._h, packed.ctypes.data, nbytes, off.ctypes.data, len(off) - 1, exc_pos.ctypes.data,
                                                      exc_chr.ctypes.data, len(exc_pos), after.ctypes.data, unpacked.ctypes.data,
                                                      n_fix.ctypes.data, cap, fix_pos.ctypes.data, fix_chr.ctypes.data))
        return unpacked, int(n_fix[0]), fix_pos, fix_chr

    def selftest_transport_bytes(self, orig_a, na, shift_a, orig_b, nb, shift_b, after, cap):
        """Test support (rc_selftest_transport_bytes): the resident boundary's fix list alone.  orig_a / orig_b: shift + n +
        SELFTEST_ARENA_SLACK bytes each (what lies in front of a range down to the 16-byte boundary, the range, the slack behind
        it; orig_b None where nb == 0), after: the na + nb corrected bytes.  Returns (n_fix, fix_pos, fix_chr) as above."""
        na, nb, shift_a, shift_b, cap = int(na), int(nb), int(shift_a), int(shift_b), int(cap)
        orig_a = np.ascontiguousarray(orig_a, dtype=np.uint8)
        orig_b = None if orig_b is None else np.ascontiguousarray(orig_b, dtype=np.uint8)
        after = np.ascontiguousarray(after, dtype=np.uint8)
        if len(orig_a) != shift_a + na + SELFTEST_ARENA_SLACK or len(after) != na + nb or (orig_b is None) != (nb == 0) or \
                (orig_b is not None and len(orig_b) != shift_b + nb + SELFTEST_ARENA_SLACK):
            raise ValueError("selftest_transport_bytes: the arrays do not describe ranges of %d and %d bytes" % (na, nb))
        n_fix = np.zeros(1, np.uint32)
        fix_pos, fix_chr = np.zeros(cap + SELFTEST_FIX_SLACK, np.uint32), np.zeros(cap + SELFTEST_FIX_SLACK, np.uint8)
        self._ck(self._L.rc_selftest_transport_bytes(self._h, orig_a.ctypes.data, na, shift_a, None if orig_b is None else orig_b.ctypes.data, nb,
                                                     shift_b, after.ctypes.data, n_fix.ctypes.data, cap, fix_pos.ctypes.data, fix_chr.ctypes.data))
        return int(n_fix[0]), fix_pos, fix_chr

    def summary(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.rc_summary(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
