"""ctypes binding of include/tdoa_mi355x.h.  No CPU fallback: loading fails loudly if the
HIP library is missing, and every compute call raises TdoaError on a non-zero status."""
import collections
import ctypes as C
import os

import numpy as np

from . import build as _build

OK = 0
KERNELS = ["STATS", "FWD_COL", "FWD_ROW", "INV_ROW", "INV_COL", "PEAK", "TRACK_STEP", "TRACK_FINISH"]


class TdoaError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("tdoa_mi355x status %d: %s" % (status, msg))
        self.status = status


class Params(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("max_lag", C.c_int32), ("corr_block", C.c_int32),
                ("weak_threshold", C.c_double), ("window_len", C.c_int64),
                ("device", C.c_int32), ("windows_per_batch", C.c_int32),
                ("k1_smooth", C.c_int32), ("k1_gate", C.c_int32), ("lag_mode", C.c_int32), ("reserved", C.c_int32)]


LAGS_SIGNED, LAGS_GO = 0, 1


class Peak(C.Structure):
    _fields_ = [("lag", C.c_int32), ("abs_corr", C.c_float), ("corr", C.c_double)]


PEAK_DTYPE = np.dtype([("lag", np.int32), ("abs_corr", np.float32), ("corr", np.float64)])


QUALITY_DTYPE = np.dtype([("n_samples", np.int64), ("i_avg", np.float64), ("q_avg", np.float64), ("i_std", np.float64),
                          ("q_std", np.float64), ("power_level", np.float64), ("mean_power", np.float64),
                          ("i_min", np.int32), ("i_max", np.int32), ("q_min", np.int32), ("q_max", np.int32),
                          ("has_clipping", np.int32), ("has_overload", np.int32)])


class FinePeak(C.Structure):
    _fields_ = [("delay", C.c_double), ("frac", C.c_float), ("y", C.c_float * 3), ("plausible", C.c_int32),
                ("reserved", C.c_int32)]


CLOSURE_DTYPE = np.dtype([("lag_ij", np.int32), ("lag_ik", np.int32), ("lag_jk", np.int32), ("residual", np.int32),
                          ("score_q", np.int64), ("own_q", np.int64), ("runner_q", np.int64),
                          ("corr_ij", np.float64), ("corr_ik", np.float64), ("corr_jk", np.float64),
                          ("score", np.float64), ("runner_up", np.float64)])      # tdoa_closure
LOCATION_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("pairs_in", np.int32), ("reserved", np.int32),
                           ("score_q", np.int64), ("runner_q", np.int64),
                           ("score", np.float64), ("runner_up", np.float64)])      # tdoa_location
ZOOM_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("pairs_in", np.int32), ("n_best", np.int32),
                       ("row_lo", np.int32), ("row_hi", np.int32), ("col_lo", np.int32), ("col_hi", np.int32),
                       ("score_q", np.int64), ("runner_q", np.int64),
                       ("score", np.float64), ("runner_up", np.float64)])      # tdoa_zoom
SYNC_DTYPE = np.dtype([("moved", np.int32), ("pairs_in", np.int32), ("score_q", np.int64), ("start_q", np.int64),
                       ("score", np.float64)])      # tdoa_sync
SYNC_LINE_DTYPE = np.dtype([("moved", np.int32), ("terms_in", np.int32), ("positions", np.int32), ("reserved", np.int32),
                            ("score_q", np.int64), ("start_q", np.int64), ("score", np.float64)])      # tdoa_sync_line
CELL_TRACK_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("positions", np.int32), ("steps", np.int32),
                             ("score_q", np.int64), ("runner_q", np.int64),
                             ("score", np.float64), ("runner_up", np.float64)])      # tdoa_cell_track
MAP_STATS_MAX_RANKS = 8
MAP_STATS_DTYPE = np.dtype([("quantile_q", np.int64, (MAP_STATS_MAX_RANKS,)), ("quantile", np.float64, (MAP_STATS_MAX_RANKS,)),
                            ("level_q", np.int64), ("n_live", np.int32), ("foot_cells", np.int32), ("foot_near", np.int32),
                            ("row_lo", np.int32), ("row_hi", np.int32), ("col_lo", np.int32), ("col_hi", np.int32),
                            ("reserved", np.int32)])      # tdoa_map_stats
FINE_DTYPE = np.dtype([("delay", np.float64), ("frac", np.float32), ("y", np.float32, (3,)), ("plausible", np.int32),
                       ("reserved", np.int32)])


# tdoa_debug_last_route: the names of include/tdoa_mi355x.h's TDOA_INV_*, TDOA_STEP_*, TDOA_COL_*, TDOA_ROW_* in number order
ROUTE_INVERSE = ["none", "segments", "decimated", "short_lag", "full"]
ROUTE_PAIR_STEP = ["tiles", "columns", "staged"]
ROUTE_COL_PASS = ["none", "k1_256", "k1_512", "k1_two_sweep", "c256", "two_sweep", "short16x", "colx", "generic"]
ROUTE_ROW_PASS = ["none", "unpack_blocks", "unpack_in_place", "unpack_tiles", "hot", "generic"]
ROUTE_FLAGS = ["seg_quads", "seg_pack3", "fused_k1", "once", "small_fused", "pruned", "xcd_pairs", "dec_gp", "stg_folded",
               "stg_blocked"]
# the last slot is a bit field (TDOA_ROUTE_STG_BLOCKED_BIT, TDOA_ROUTE_STG_MERGED_BIT, TDOA_ROUTE_K1_SPLIT_BIT,
# TDOA_ROUTE_STG_PAIRED_BIT, TDOA_ROUTE_STG_NT_BIT): last_route() reports each bit as a bool -- ROUTE_FLAGS' last name, then
# ROUTE_BIT_FLAGS
ROUTE_STG_BLOCKED_BIT, ROUTE_STG_MERGED_BIT, ROUTE_K1_SPLIT_BIT, ROUTE_STG_PAIRED_BIT, ROUTE_STG_NT_BIT = 1, 2, 4, 8, 16
ROUTE_BIT_FLAGS = {"stg_blocked": ROUTE_STG_BLOCKED_BIT, "stg_merged": ROUTE_STG_MERGED_BIT, "k1_split": ROUTE_K1_SPLIT_BIT,
                   "stg_paired": ROUTE_STG_PAIRED_BIT, "stg_nt": ROUTE_STG_NT_BIT}


class FastAnalysis(C.Structure):
    _fields_ = [("total_samples", C.c_int32), ("has_clipping", C.c_int32), ("has_overload", C.c_int32),
                ("reserved", C.c_int32), ("i_avg", C.c_double), ("q_avg", C.c_double), ("i_std", C.c_double),
                ("q_std", C.c_double), ("snr_estimate", C.c_double), ("power_level", C.c_double)]


class FmStats(C.Structure):
    _fields_ = [("s1", C.c_int64), ("s2_lo", C.c_uint64), ("s2_hi", C.c_uint64),
                ("mean", C.c_float), ("scale", C.c_float)]


# every symbol include/tdoa_mi355x.h declares
SYMBOLS = [
    "tdoa_default_params", "tdoa_create", "tdoa_destroy", "tdoa_strerror", "tdoa_last_error",
    "tdoa_abi_version", "tdoa_device_count",
    "tdoa_load_iq_u8", "tdoa_preprocess_c64", "tdoa_time_domain_correlation_c64",
    "tdoa_cross_correlate_c64", "tdoa_simple_correlate_c64", "tdoa_fast_snr_u8",
    "tdoa_fast_analyze_u8", "tdoa_fast_analyze_capture_u8",
    "tdoa_capture_upload", "tdoa_capture_upload_file", "tdoa_capture_attach_device", "tdoa_capture_clear",
    "tdoa_synth_capture", "tdoa_synth_weak_capture", "tdoa_capture_download", "tdoa_capture_upload_range",
    "tdoa_num_windows", "tdoa_num_pairs", "tdoa_process", "tdoa_process_u8",
    "tdoa_process_fine", "tdoa_fm_xcorr_fine_u8", "tdoa_window_quality_all", "tdoa_window_quality_u8",
    "tdoa_fm_xcorr_u8", "tdoa_fm_preprocess_u8", "tdoa_fm_xcorr_lags_u8", "tdoa_debug_force_generic",
    "tdoa_debug_flags", "tdoa_debug_last_k1", "tdoa_debug_graph_info", "tdoa_debug_poison_workspace", "tdoa_debug_last_route", "tdoa_debug_segment_quads", "tdoa_debug_staged_groups", "tdoa_debug_step_layout", "tdoa_debug_k1_split_table", "tdoa_debug_stg_paired_index", "tdoa_cross_correlate_batch_c64",
    "tdoa_latlon_to_ecef", "tdoa_ecef_to_latlon", "tdoa_solve_3station", "tdoa_solve_nstation", "tdoa_solve_surface",
    "tdoa_profile_enable", "tdoa_profile_select", "tdoa_profile_reset", "tdoa_profile_get", "tdoa_kernel_name",
    "tdoa_plan_info", "tdoa_process_lags", "tdoa_process_peaks", "tdoa_fm_xcorr_peaks_u8", "tdoa_debug_select_peaks",
    "tdoa_group_create", "tdoa_group_destroy", "tdoa_group_last_error", "tdoa_group_member",
    "tdoa_group_capture_upload_files", "tdoa_group_process", "tdoa_debug_owned_runs",
    "tdoa_num_stacks", "tdoa_process_stacked", "tdoa_group_process_stacked", "tdoa_process_stacked_drift",
    "tdoa_process_track",
    "tdoa_num_triples", "tdoa_process_closure", "tdoa_group_process_closure", "tdoa_debug_closure_from_q",
    "tdoa_locate_set_table", "tdoa_process_locate", "tdoa_debug_locate_from_q", "tdoa_locate_grid_table",
    "tdoa_group_locate_set_table", "tdoa_group_process_locate",
    "tdoa_locate_set_clock", "tdoa_group_locate_set_clock", "tdoa_process_sync", "tdoa_debug_sync_from_q",
    "tdoa_process_locate_track", "tdoa_debug_locate_track_from_q", "tdoa_group_process_locate_track",
    "tdoa_group_process_sync",
    "tdoa_process_locate_multi", "tdoa_debug_locate_multi_from_q", "tdoa_group_process_locate_multi",
    "tdoa_process_locate_track_multi", "tdoa_debug_locate_track_multi_from_q", "tdoa_group_process_locate_track_multi",
    "tdoa_locate_set_stats", "tdoa_locate_last_stats", "tdoa_group_locate_set_stats", "tdoa_group_locate_last_stats",
    "tdoa_process_sync_drift", "tdoa_debug_sync_drift_from_q", "tdoa_group_process_sync_drift", "tdoa_sync_line_clock",
    "tdoa_locate_set_upsample", "tdoa_group_locate_set_upsample", "tdoa_locate_upsample_taps", "tdoa_debug_upsample_q",
    "tdoa_process_sync_fine", "tdoa_group_process_sync_fine", "tdoa_debug_sync_fine_from_q",
    "tdoa_locate_set_fine_table", "tdoa_group_locate_set_fine_table", "tdoa_process_locate_zoom", "tdoa_group_process_locate_zoom",
    "tdoa_debug_locate_zoom_from_q",
    "tdoa_process_sync_drift_fine", "tdoa_group_process_sync_drift_fine", "tdoa_debug_sync_drift_fine_from_q",
    "tdoa_sync_line_clock16",
    "tdoa_process_locate_track_zoom", "tdoa_group_process_locate_track_zoom", "tdoa_debug_locate_track_zoom_from_q",
    "tdoa_process_sync_locate", "tdoa_group_process_sync_locate", "tdoa_debug_sync_locate_from_q", "tdoa_clock_mix_rows",
    "tdoa_debug_clock_mix",
    "tdoa_process_sync_drift_locate", "tdoa_group_process_sync_drift_locate", "tdoa_debug_sync_drift_locate_from_q",
    "tdoa_line_mix_rows", "tdoa_debug_line_mix",
    "tdoa_process_locate_multi_zoom", "tdoa_group_process_locate_multi_zoom", "tdoa_debug_locate_multi_zoom_from_q",
]


# ---- the stack searches (csrc/stack_search.inc), each stated once ---------------------------------------------------------
# The header gives every search three entries of one shape: a handle; windows_per_stack (own, group) or q, n_sets, [track_len,]
# n_stations, n_w (the caller's Q); the search's ints; ref_delay, centre; the outputs, <key>_host or <key>.  _run_search and
# load() read the order from here, and tests/test_capi_bindings_cpu.py holds it to the header.
_POINTER = {np.dtype(np.int32): C.POINTER(C.c_int32), np.dtype(np.float64): C.POINTER(C.c_double),
            np.dtype(np.int64): C.POINTER(C.c_int64)}      # a record goes as void *
_Output = collections.namedtuple("_Output", "key dtype shape want poison ctype")


def _Out(key, dtype, shape, want=None, poison=False):
    """an output: its key in the result, its dtype, its shape (names of _shape_numbers, or plain ints), the want_* flag that
    selects it when it is optional, whether it starts as 0xA5 bytes and not as zeros; ctype is its pointer's argtype"""
    return _Output(key, dtype, shape, want, poison, _POINTER.get(np.dtype(dtype), C.c_void_p))


class _Search:
    def __init__(self, name, ints, outputs, inputs=(), track_len=False, stats=None, bare=False, late_ints=(), mix_width=4):
        self.name, self.ints, self.outputs, self.inputs = name, ints, outputs, inputs
        self.late_ints = late_ints           # ints the header states behind the inputs
        self.mix_width = mix_width           # the ints of an entry of the input "mix": 4 tdoa_clock_mix, 6 tdoa_line_mix
        self.entries = {"own": "tdoa_process_" + name, "group": "tdoa_group_process_" + name,
                        "q": "tdoa_debug_%s_from_q" % name}
        self.track_len = track_len           # the from-Q entry takes track_len
        self.stats = stats                   # the key "stats" is shaped like, for the delay-table family
        self.bare = bare                     # the result is the one array, not a dict


def _rounds(outputs):
    """the outputs with a leading axis of K rounds"""
    return tuple(o._replace(shape=("K",) + o.shape) for o in outputs)


_LOCATE_OUT = (_Out("loc", LOCATION_DTYPE, ("n_sets",)), _Out("lags", np.int32, ("n_sets", "P")),
               _Out("corr", np.float64, ("n_sets", "P")), _Out("map", np.int64, ("n_sets", "n_cells"), "want_map"))
_ZOOM_OUT = (_Out("zoom", ZOOM_DTYPE, ("n_sets",), poison=True), _Out("zlags", np.int32, ("n_sets", "P"), poison=True),
             _Out("zcorr", np.float64, ("n_sets", "P"), poison=True),
             _Out("zmap", np.int64, ("n_sets", "window"), "want_zmap", poison=True))
_TRACK_OUT = (_Out("track", CELL_TRACK_DTYPE, ("n_tracks",)), _Out("cells", np.int32, ("n_tracks", "L")),
              _Out("own", np.int64, ("n_tracks", "L")), _Out("lags", np.int32, ("n_sets", "P")),
              _Out("corr", np.float64, ("n_sets", "P")), _Out("total", np.int64, ("n_tracks", "n_cells"), "want_total"))
_SYNC_OUT = (_Out("sync", SYNC_DTYPE, ("n_sets",)), _Out("clock", np.int32, ("n_sets", "S")),
             _Out("lags", np.int32, ("n_sets", "P")), _Out("corr", np.float64, ("n_sets", "P")))
_CLOCKS = ("ref_delay", "centre")
SEARCHES = {s.name: s for s in (
    _Search("closure", ("gate", "min_separation"), (_Out("closure", CLOSURE_DTYPE, ("n_sets", "T")),), ("centre",), bare=True),
    _Search("locate", ("min_separation",), _LOCATE_OUT, stats="loc"),
    _Search("locate_multi", ("n_emitters", "guard", "min_separation"), _rounds(_LOCATE_OUT), stats="loc"),
    _Search("locate_track", ("max_step", "min_separation"), _TRACK_OUT, track_len=True, stats="track"),
    _Search("locate_track_multi", ("max_step", "n_emitters", "guard", "min_separation"),
            _rounds(_TRACK_OUT[:3] + (_Out("pairs", np.int32, ("n_sets", 2)),) + _TRACK_OUT[3:]), track_len=True, stats="track"),
    _Search("locate_zoom", ("min_separation", "Z", "H", "fine_separation"), _LOCATE_OUT + _ZOOM_OUT, stats="loc"),
    _Search("sync", ("gate", "rounds"), _SYNC_OUT, _CLOCKS),
    _Search("sync_fine", ("gate", "rounds", "U", "fine_rounds"),
            _SYNC_OUT + (_Out("fine", SYNC_DTYPE, ("n_sets",)), _Out("clock16", np.int32, ("n_sets", "S")),
                         _Out("fine_lags", np.int32, ("n_sets", "P")), _Out("fine_corr", np.float64, ("n_sets", "P"))), _CLOCKS),
    _Search("sync_drift", ("gate", "max_drift", "drift_den", "rounds"),
            (_Out("line", SYNC_LINE_DTYPE, ("n_tracks",)), _Out("clock", np.int32, ("n_tracks", "S")),
             _Out("rate", np.int32, ("n_tracks", "S")), _Out("rows", np.int32, ("n_sets", "S")),
             _Out("lags", np.int32, ("n_sets", "P")), _Out("corr", np.float64, ("n_sets", "P"))), _CLOCKS, track_len=True),
)}
# searches added after the nine: the same records, resolved through _search (tests pin SEARCHES to its nine names)
LATER_SEARCHES = {s.name: s for s in (
    _Search("sync_drift_fine", ("gate", "max_drift", "drift_den", "rounds", "U", "fine_rounds"),
            SEARCHES["sync_drift"].outputs +
            (_Out("fine", SYNC_LINE_DTYPE, ("n_tracks",)), _Out("clock16", np.int32, ("n_tracks", "S")),
             _Out("fine_rate", np.int32, ("n_tracks", "S")), _Out("fine_rows", np.int32, ("n_sets", "S")),
             _Out("fine_lags", np.int32, ("n_sets", "P")), _Out("fine_corr", np.float64, ("n_sets", "P"))), _CLOCKS, track_len=True),
)}


# ... and after that one (tests pin LATER_SEARCHES to its one name as they pin SEARCHES): the zoomed cell tracks, whose z outputs
# are written over a poison pattern like the zoom's
_TRACK_ZOOM_OUT = (_Out("ztrack", CELL_TRACK_DTYPE, ("n_tracks",), poison=True), _Out("zcells", np.int32, ("n_tracks", "L"), poison=True),
                   _Out("zown", np.int64, ("n_tracks", "L"), poison=True), _Out("zlags", np.int32, ("n_sets", "P"), poison=True),
                   _Out("zcorr", np.float64, ("n_sets", "P"), poison=True),
                   _Out("zmap", np.int64, ("n_sets", "window"), "want_zmap", poison=True),
                   _Out("ztotal", np.int64, ("n_tracks", "window"), "want_ztotal", poison=True))
TRACK_ZOOM_SEARCHES = {s.name: s for s in (
    _Search("locate_track_zoom", ("max_step", "min_separation", "Z", "H", "fine_step", "fine_separation"),
            _TRACK_OUT + _TRACK_ZOOM_OUT, track_len=True, stats="track"),
    # clocks to fix in one call: the fine clock search's arguments, the mix, the zoom locate's ints, the sixteen outputs of the two
    # with the rows between them (the locate's lags and corr under loc_ names: the clock search's have theirs)
    _Search("sync_locate", SEARCHES["sync_fine"].ints,
            SEARCHES["sync_fine"].outputs + (_Out("rows", np.int32, ("n_sets", "S")),) +
            tuple(o._replace(key="loc_" + o.key) if o.key in ("lags", "corr") else o for o in SEARCHES["locate_zoom"].outputs),
            _CLOCKS + ("mix",), stats="loc", late_ints=SEARCHES["locate_zoom"].ints),
)}
# free-running clocks to fix in one call: the fine clock lines' arguments, the line mix, the zoomed tracks' ints, the twenty-six
# outputs of the two with the mix's rows between them (the tracks' lags and corr under loc_ names: the lines have theirs)
TRACK_ZOOM_SEARCHES["sync_drift_locate"] = _Search(
    "sync_drift_locate", LATER_SEARCHES["sync_drift_fine"].ints,
    LATER_SEARCHES["sync_drift_fine"].outputs + (_Out("mix_rows", np.int32, ("n_sets", "S")),) +
    tuple(o._replace(key="loc_" + o.key) if o.key in ("lags", "corr") else o for o in TRACK_ZOOM_SEARCHES["locate_track_zoom"].outputs),
    _CLOCKS + ("mix",), track_len=True, stats="track", late_ints=TRACK_ZOOM_SEARCHES["locate_track_zoom"].ints, mix_width=6)

# the zoomed rounds (tests pin TRACK_ZOOM_SEARCHES to its three names too): the rounds' four outputs and, [round][stack][...], the
# zoom's with the counts behind the records
MULTI_ZOOM_SEARCHES = {s.name: s for s in (
    _Search("locate_multi_zoom", ("n_emitters", "guard", "min_separation", "Z", "H", "fine_separation"),
            _rounds(_LOCATE_OUT + _ZOOM_OUT[:1] + (_Out("zpairs", np.int32, ("n_sets", 2), poison=True),) + _ZOOM_OUT[1:]), stats="loc"),
)}


def _search(name):
    """the record of search `name`, from any of the tables"""
    for table in (SEARCHES, LATER_SEARCHES, TRACK_ZOOM_SEARCHES, MULTI_ZOOM_SEARCHES):
        if name in table:
            return table[name]
    raise KeyError(name)


def _search_argtypes(s, route):
    """the argtypes of search s's entry `route`"""
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    shape = [i64p] + [C.c_int] * (3 + s.track_len) if route == "q" else [C.c_int]
    return ([C.c_void_p] + shape + [C.c_int] * len(s.ints) + [i32p] * len(s.inputs) + [C.c_int] * len(s.late_ints) +
            [o.ctype for o in s.outputs])


_lib = None


def library_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load the shared library (building it with hipcc if absent).  Raises if impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and _build.needs_build():
        _build.build()
    if not os.path.exists(_build.LIB):
        raise RuntimeError("libtdoa_mi355x.so is missing; run tdoa_amd.build.build() (needs hipcc)")
    L = C.CDLL(_build.LIB)
    vp, sz = C.c_void_p, C.c_size_t
    fp, u8p, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    L.tdoa_default_params.argtypes = [C.POINTER(Params)]
    L.tdoa_default_params.restype = None
    L.tdoa_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.tdoa_destroy.argtypes = [vp]
    L.tdoa_destroy.restype = None
    L.tdoa_strerror.argtypes = [C.c_int]
    L.tdoa_strerror.restype = C.c_char_p
    L.tdoa_last_error.argtypes = [vp]
    L.tdoa_last_error.restype = C.c_char_p
    L.tdoa_kernel_name.argtypes = [C.c_int]
    L.tdoa_kernel_name.restype = C.c_char_p
    L.tdoa_load_iq_u8.argtypes = [vp, u8p, sz, fp]
    L.tdoa_preprocess_c64.argtypes = [vp, fp, sz, fp, C.POINTER(C.c_int)]
    L.tdoa_time_domain_correlation_c64.argtypes = [vp, fp, sz, fp, sz, C.c_int, i32p, dp]
    L.tdoa_cross_correlate_c64.argtypes = [vp, fp, sz, fp, sz, i32p, dp]
    L.tdoa_cross_correlate_batch_c64.argtypes = [vp, C.POINTER(fp), C.POINTER(sz), C.c_int, i32p, dp]
    L.tdoa_simple_correlate_c64.argtypes = [vp, fp, sz, fp, sz, i32p, fp]
    L.tdoa_fast_snr_u8.argtypes = [vp, u8p, C.c_int, dp]
    L.tdoa_fast_analyze_u8.argtypes = [vp, u8p, C.c_int, C.POINTER(FastAnalysis)]
    L.tdoa_fast_analyze_capture_u8.argtypes = [vp, u8p, sz, C.POINTER(FastAnalysis), C.POINTER(FastAnalysis)]
    L.tdoa_capture_upload.argtypes = [vp, C.c_int, u8p, sz]
    L.tdoa_capture_upload_file.argtypes = [vp, C.c_int, C.c_char_p, C.POINTER(sz)]
    L.tdoa_capture_attach_device.argtypes = [vp, C.c_int, vp, sz]
    L.tdoa_capture_clear.argtypes = [vp]
    L.tdoa_synth_capture.argtypes = [vp, C.c_int, sz, C.c_double, C.c_double, C.c_double, dp, dp, C.c_double,
                                     C.c_uint64]
    L.tdoa_synth_weak_capture.argtypes = [vp, C.c_int, sz, C.c_double, C.c_double, dp, dp, C.c_double, C.c_double,
                                          C.c_uint64]
    L.tdoa_capture_upload_range.argtypes = [vp, C.c_int, sz, sz, u8p, sz]
    L.tdoa_capture_download.argtypes = [vp, C.c_int, sz, sz, u8p]
    L.tdoa_num_windows.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tdoa_num_pairs.argtypes = [vp]
    L.tdoa_process.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.tdoa_process_u8.argtypes = [vp, C.POINTER(u8p), C.POINTER(sz), C.c_int, vp]
    L.tdoa_fm_xcorr_u8.argtypes = [vp, u8p, sz, u8p, sz, C.c_int, C.POINTER(Peak)]
    L.tdoa_window_quality_all.argtypes = [vp, C.c_int, C.c_int, vp]
    L.tdoa_window_quality_u8.argtypes = [vp, u8p, sz, vp]
    L.tdoa_process_fine.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp, vp]
    L.tdoa_fm_xcorr_fine_u8.argtypes = [vp, u8p, sz, u8p, sz, C.c_int, C.c_double, C.POINTER(Peak),
                                        C.POINTER(FinePeak)]
    L.tdoa_fm_preprocess_u8.argtypes = [vp, u8p, sz, fp, C.POINTER(FmStats)]
    L.tdoa_fm_xcorr_lags_u8.argtypes = [vp, u8p, sz, u8p, sz, C.c_int, dp]
    L.tdoa_debug_force_generic.argtypes = [vp, C.c_int]
    L.tdoa_debug_flags.argtypes = [vp, C.c_uint]
    L.tdoa_debug_last_k1.argtypes = [vp, C.c_int, C.POINTER(FmStats), C.POINTER(C.c_int32)]
    L.tdoa_debug_graph_info.argtypes = [vp, C.POINTER(C.c_int32), C.c_char_p]
    L.tdoa_debug_poison_workspace.argtypes = [vp]
    L.tdoa_debug_last_route.argtypes = [vp, C.POINTER(C.c_int32)]
    L.tdoa_debug_segment_quads.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.tdoa_debug_staged_groups.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int]
    L.tdoa_debug_k1_split_table.argtypes = [C.POINTER(C.c_uint16), u8p]
    L.tdoa_debug_stg_paired_index.argtypes = [C.c_int, C.c_int, C.c_int]
    L.tdoa_debug_stg_paired_index.restype = C.c_int64
    L.tdoa_debug_step_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.tdoa_latlon_to_ecef.argtypes = [C.c_double, C.c_double, C.c_double, dp]
    L.tdoa_latlon_to_ecef.restype = None
    L.tdoa_ecef_to_latlon.argtypes = [C.c_double, C.c_double, C.c_double, dp]
    L.tdoa_ecef_to_latlon.restype = None
    L.tdoa_solve_3station.argtypes = [dp, dp, dp, C.POINTER(C.c_int)]
    L.tdoa_solve_nstation.argtypes = [dp, C.c_int, dp, dp, C.c_int, dp, C.POINTER(C.c_int)]
    L.tdoa_solve_surface.argtypes = [dp, C.c_int, dp, dp, C.c_double, dp, C.POINTER(C.c_int)]
    L.tdoa_profile_enable.argtypes = [vp, C.c_int]
    L.tdoa_profile_select.argtypes = [vp, C.c_uint]
    L.tdoa_profile_reset.argtypes = [vp]
    L.tdoa_profile_get.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int64), dp]
    L.tdoa_plan_info.argtypes = [vp, C.POINTER(C.c_int64), i32p, i32p]
    L.tdoa_process_lags.argtypes = [vp, C.c_int, C.c_int, fp, vp]
    L.tdoa_process_peaks.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, i32p]
    L.tdoa_fm_xcorr_peaks_u8.argtypes = [vp, u8p, sz, u8p, sz, C.c_int, C.c_int, C.c_int, vp, i32p]
    L.tdoa_debug_select_peaks.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, vp, i32p]
    L.tdoa_group_create.argtypes = [C.POINTER(Params), i32p, C.c_int, C.POINTER(vp)]
    L.tdoa_group_destroy.argtypes = [vp]
    L.tdoa_group_destroy.restype = None
    L.tdoa_group_last_error.argtypes = [vp]
    L.tdoa_group_last_error.restype = C.c_char_p
    L.tdoa_group_member.argtypes = [vp, C.c_int]
    L.tdoa_group_member.restype = vp
    L.tdoa_group_capture_upload_files.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(sz)]
    L.tdoa_group_process.argtypes = [vp, vp]
    L.tdoa_num_stacks.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tdoa_process_stacked.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, i32p, vp, fp,
                                       C.POINTER(C.c_int64)]
    L.tdoa_group_process_stacked.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, i32p, vp, fp]
    L.tdoa_process_stacked_drift.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, i32p, vp, fp,
                                             C.POINTER(C.c_int64), i32p, vp]
    L.tdoa_process_track.argtypes = [vp, C.c_int, C.c_int, vp, i32p, dp, fp, C.POINTER(C.c_int64)]
    L.tdoa_num_triples.argtypes = [vp]
    i64p = C.POINTER(C.c_int64)
    L.tdoa_locate_set_table.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int]
    L.tdoa_group_locate_set_table.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int]
    L.tdoa_locate_grid_table.argtypes = [dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                         C.c_double, C.c_double, i32p]
    L.tdoa_locate_set_clock.argtypes = [vp, i32p, C.c_int, C.c_int]
    L.tdoa_group_locate_set_clock.argtypes = [vp, i32p, C.c_int, C.c_int]
    L.tdoa_sync_line_clock.argtypes = [i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    L.tdoa_sync_line_clock16.argtypes = [i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    L.tdoa_locate_set_stats.argtypes = [vp, C.POINTER(C.c_uint16), C.c_int, C.c_int]
    L.tdoa_group_locate_set_stats.argtypes = [vp, C.POINTER(C.c_uint16), C.c_int, C.c_int]
    L.tdoa_locate_last_stats.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.tdoa_group_locate_last_stats.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.tdoa_locate_set_upsample.argtypes = [vp, C.c_int]
    L.tdoa_locate_set_fine_table.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int]
    L.tdoa_group_locate_set_fine_table.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int]
    L.tdoa_group_locate_set_upsample.argtypes = [vp, C.c_int]
    L.tdoa_locate_upsample_taps.argtypes = [C.c_int, i32p]
    L.tdoa_debug_upsample_q.argtypes = [vp, i64p, C.c_int, C.c_int, i64p]
    L.tdoa_clock_mix_rows.argtypes = [i32p, C.c_int, C.c_int, i32p, C.c_int, i32p]
    L.tdoa_debug_clock_mix.argtypes = [vp, i32p, C.c_int, C.c_int, i32p, C.c_int, C.c_int, i32p, i64p, i64p]
    L.tdoa_line_mix_rows.argtypes = [i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, i32p]
    L.tdoa_debug_line_mix.argtypes = [vp, i32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int, i32p, i64p, i64p]
    L.tdoa_debug_owned_runs.argtypes = [sz, sz, C.c_int64, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz), C.c_int,
                                        C.POINTER(C.c_int)]
    for s in list(SEARCHES.values()) + list(LATER_SEARCHES.values()) + list(TRACK_ZOOM_SEARCHES.values()) + list(MULTI_ZOOM_SEARCHES.values()):
        for route, entry in s.entries.items():
            getattr(L, entry).argtypes = _search_argtypes(s, route)
    _lib = L
    return L


def default_params():
    p = Params()
    load().tdoa_default_params(C.byref(p))
    return p


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _c64(x):
    a = np.ascontiguousarray(x, dtype=np.complex64)
    return a, a.view(np.float32)


def _params(kw):
    p = default_params()
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


# The methods of searches added after the nine live in base classes of Context and Group, as their records live in
# LATER_SEARCHES: tests pin the functions Context and Group define themselves to the parent commit's.
class _LaterContextSearches:
    def process_sync_drift_fine(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, U=16, fine_rounds=2,
                                centre=None):
        """tdoa_process_sync_drift_fine -> process_sync_drift's outputs (the coarse stage's bytes) and {"fine": [3]
        SYNC_LINE_DTYPE, "clock16": [3][S] int32 (kappa_s in 1/16 sample), "fine_rate": [3][S] int32 (eta_s, 1/(U drift_den) lag
        per stack), "fine_rows": [n_stacks][S] int32 (1/16 sample: tdoa_locate_set_clock's unit), "fine_lags": [n_stacks][P]
        int32 (1/U sample), "fine_corr": [n_stacks][P] float64}: the coarse lines' offsets and rates moved by |y_s|, |g_s| <= U
        in `fine_rounds` sweeps on the words of the surfaces upsampled to 1/U sample"""
        return _process_search(self, self, "sync_drift_fine", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre), n_tracks=3)

    def sync_drift_fine_from_q(self, q, ref_delay, track_len, n_w=1, gate=0, max_drift=0, drift_den=1, rounds=0, U=16, fine_rounds=2,
                               centre=None):
        """tdoa_debug_sync_drift_fine_from_q: the clock-line search's and the refinement's kernels on the caller's words q
        [n_sets][P][2 max_lag - 1] int64, set t track_len + j position j of line t -> what process_sync_drift_fine returns,
        n_sets / track_len lines and n_sets stacks"""
        return self._from_q("sync_drift_fine", q, np.size(ref_delay), dict(
            track_len=track_len, n_w=n_w, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre))

    def process_locate_track_zoom(self, Z, H, windows_per_stack=0, max_step=0, min_separation=1, fine_step=0, fine_separation=1,
                                  want_total=False, want_zmap=True, want_ztotal=True):
        """tdoa_process_locate_track_zoom -> process_locate_track's dict (the coarse stage's bytes) and {"ztrack": [n_tracks]
        CELL_TRACK_DTYPE (its cells are fine cells), "zcells": [n_tracks][L] int32, "zown": [n_tracks][L] int64, "zlags":
        [n_stacks][P] int32 (1/U sample), "zcorr": [n_stacks][P] float64, with want_zmap "zmap": [n_stacks][(2H+1)^2] int64 and
        with want_ztotal "ztotal": [n_tracks][(2H+1)^2] int64}: per block the track through the (2H+1)^2-cell windows of the fine
        table around Z x the coarse track's cells, consecutive fine cells at most fine_step rows and columns apart, with the
        largest summed score.  The z arrays are written over a poison pattern"""
        return _process_search(self, self, "locate_track_zoom", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, min_separation=min_separation, Z=Z, H=H, fine_step=fine_step,
            fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap, want_ztotal=want_ztotal))

    def locate_track_zoom_from_q(self, q, n_stations, track_len, Z, H, n_w=1, max_step=0, min_separation=1, fine_step=0,
                                 fine_separation=1, want_total=True, want_zmap=True, want_ztotal=True):
        """tdoa_debug_locate_track_zoom_from_q: the tracks' and the zoomed tracks' kernels on the caller's words q
        [n_sets][P][2 max_lag - 1] int64, set t track_len + j position j of track t, with the context's table, fine table and
        clocks -> what process_locate_track_zoom returns, n_sets for n_stacks"""
        return self._from_q("locate_track_zoom", q, n_stations, dict(
            track_len=track_len, n_w=n_w, max_step=max_step, min_separation=min_separation, Z=Z, H=H, fine_step=fine_step,
            fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap, want_ztotal=want_ztotal))


    def process_sync_locate(self, ref_delay, Z, H, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None, mix=None,
                            min_separation=1, fine_separation=1, want_map=False, want_zmap=True):
        """tdoa_process_sync_locate -> process_sync_fine's eight outputs (that call's bytes), "rows": [n_stacks][S] int32 (1/16
        sample), and process_locate_zoom's eight as after locate_set_clock(rows), the locate's lags and corr under "loc_lags"
        and "loc_corr": the fine clock search, a clock row per stack mixed on the device from its clock16 by mix [n_stacks][4]
        (a, b, wa, wb; None: every stack its own clock; clock_mix.midpoint_mix for [reference | target | reference]), and the
        zoom locate under those rows, in one step.  The context's clock table is neither read nor changed"""
        return _process_search(self, self, "sync_locate", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay,
            centre=centre, mix=mix, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation, want_map=want_map,
            want_zmap=want_zmap))

    def sync_locate_from_q(self, q, ref_delay, Z, H, n_w=1, gate=0, rounds=0, U=16, fine_rounds=2, centre=None, mix=None,
                           min_separation=1, fine_separation=1, want_map=True, want_zmap=True):
        """tdoa_debug_sync_locate_from_q: the same kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64 with the
        context's table, fine table and settings -> what process_sync_locate returns, n_sets for n_stacks; mix names sets"""
        return self._from_q("sync_locate", q, np.size(ref_delay), dict(
            n_w=n_w, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre, mix=mix,
            min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation, want_map=want_map, want_zmap=want_zmap))

    def debug_clock_mix(self, clock16, mix, U_loc=1):
        """tdoa_debug_clock_mix: the mix kernel alone on clock16 [n][S] int32 and mix [m][4] -> (rows [m][S] int32, cdiff [m][P]
        int64 = row[j] - row[i] in locate_set_clock's pair order, cdiff_up = U_loc x cdiff), written over poisoned arrays"""
        c = np.ascontiguousarray(clock16, dtype=np.int32)
        if c.ndim != 2:
            raise ValueError("clock16 must be [n][S]")
        m, (n, S) = np.shape(mix)[0], c.shape
        rows, cdiff, up = (_poisoned((m, S), np.int32), _poisoned((m, S * (S - 1) // 2), np.int64),
                           _poisoned((m, S * (S - 1) // 2), np.int64))
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._chk(self._L.tdoa_debug_clock_mix(self._h, c.ctypes.data_as(i32p), n, S, _mix(mix), m, int(U_loc), rows.ctypes.data_as(i32p),
                                               cdiff.ctypes.data_as(i64p), up.ctypes.data_as(i64p)))
        return rows, cdiff, up


    def process_sync_drift_locate(self, ref_delay, Z, H, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, U=16,
                                  fine_rounds=2, centre=None, mix=None, max_step=0, min_separation=1, fine_step=0, fine_separation=1,
                                  want_total=False, want_zmap=True, want_ztotal=True):
        """tdoa_process_sync_drift_locate -> process_sync_drift_fine's twelve outputs (that call's bytes), "mix_rows":
        [n_stacks][S] int32 (1/16 sample), and process_locate_track_zoom's thirteen as after locate_set_clock(mix_rows), the
        coarse tracks' lags and corr under "loc_lags" and "loc_corr": the fine clock lines, a clock row per stack made on the
        device from their clock16 and fine_rate by mix [n_stacks][6] (a, xa, b, xb, wa, wb; None: every stack its own line at its
        own position; line_mix.forward_mix or bridge_mix for [reference | target | reference]), and the zoomed cell tracks under
        those rows, in one step.  The context's clock table is neither read nor changed"""
        return _process_search(self, self, "sync_drift_locate", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre, mix=mix, max_step=max_step, min_separation=min_separation, Z=Z,
            H=H, fine_step=fine_step, fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap,
            want_ztotal=want_ztotal))

    def sync_drift_locate_from_q(self, q, ref_delay, track_len, Z, H, n_w=1, gate=0, max_drift=0, drift_den=1, rounds=0, U=16,
                                 fine_rounds=2, centre=None, mix=None, max_step=0, min_separation=1, fine_step=0, fine_separation=1,
                                 want_total=True, want_zmap=True, want_ztotal=True):
        """tdoa_debug_sync_drift_locate_from_q: the same kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64, set
        t track_len + j position j of line and track t, with the context's table, fine table and settings -> what
        process_sync_drift_locate returns, n_sets for n_stacks; mix names the n_sets / track_len lines"""
        return self._from_q("sync_drift_locate", q, np.size(ref_delay), dict(
            track_len=track_len, n_w=n_w, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre, mix=mix, max_step=max_step, min_separation=min_separation, Z=Z,
            H=H, fine_step=fine_step, fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap,
            want_ztotal=want_ztotal))

    def debug_line_mix(self, clock16, fine_rate, U, drift_den, mix, U_loc=1):
        """tdoa_debug_line_mix: the line mix kernel alone on clock16, fine_rate [n_lines][S] int32 and mix [m][6] -> (rows [m][S]
        int32, cdiff [m][P] int64 = row[j] - row[i] in locate_set_clock's pair order, cdiff_up = U_loc x cdiff), written over
        poisoned arrays"""
        c, h = _line_words(clock16, fine_rate)
        m, (n, S) = np.shape(mix)[0], c.shape
        rows, cdiff, up = (_poisoned((m, S), np.int32), _poisoned((m, S * (S - 1) // 2), np.int64),
                           _poisoned((m, S * (S - 1) // 2), np.int64))
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._chk(self._L.tdoa_debug_line_mix(self._h, c.ctypes.data_as(i32p), h.ctypes.data_as(i32p), n, S, int(U), int(drift_den),
                                              _mix(mix, width=6), m, int(U_loc), rows.ctypes.data_as(i32p), cdiff.ctypes.data_as(i64p),
                                              up.ctypes.data_as(i64p)))
        return rows, cdiff, up

    def process_locate_multi_zoom(self, Z, H, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
                                  want_map=False, want_zmap=True):
        """tdoa_process_locate_multi_zoom -> process_locate_multi's dict (the rounds' bytes) and, all [n_emitters][n_stacks][...],
        {"zoom": ZOOM_DTYPE, "zpairs": [2] int32 (pairs_in, reserved), "zlags": [P] int32 (1/U sample), "zcorr": [P] float64, with
        want_zmap "zmap": [(2H+1)^2] int64}: every round's coarse cell searched again on the (2H+1)^2-cell window of the fine
        table around Z x that cell, under the mask the round ran under.  The z arrays are written over a poison pattern"""
        return _process_search(self, self, "locate_multi_zoom", dict(
            windows_per_stack=windows_per_stack, n_emitters=n_emitters, guard=guard, min_separation=min_separation, Z=Z, H=H,
            fine_separation=fine_separation, want_map=want_map, want_zmap=want_zmap))

    def locate_multi_zoom_from_q(self, q, n_stations, Z, H, n_w=1, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
                                 want_map=True, want_zmap=True):
        """tdoa_debug_locate_multi_zoom_from_q: the rounds' and the zoomed rounds' kernels on the caller's words q
        [n_sets][P][2 max_lag - 1] int64 (or one set) with the context's table, fine table and clocks -> what
        process_locate_multi_zoom returns, n_sets for n_stacks"""
        return self._from_q("locate_multi_zoom", q, n_stations, dict(
            n_w=n_w, n_emitters=n_emitters, guard=guard, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation,
            want_map=want_map, want_zmap=want_zmap))


class _LaterGroupSearches:
    def process_locate_multi_zoom(self, Z, H, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
                                  want_map=False, want_zmap=True):
        """tdoa_group_process_locate_multi_zoom -> Context.process_locate_multi_zoom's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate_multi_zoom", dict(
            windows_per_stack=windows_per_stack, n_emitters=n_emitters, guard=guard, min_separation=min_separation, Z=Z, H=H,
            fine_separation=fine_separation, want_map=want_map, want_zmap=want_zmap))

    def process_sync_drift_fine(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, U=16, fine_rounds=2,
                                centre=None):
        """tdoa_group_process_sync_drift_fine -> Context.process_sync_drift_fine's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "sync_drift_fine", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre), n_tracks=3)

    def process_locate_track_zoom(self, Z, H, windows_per_stack=0, max_step=0, min_separation=1, fine_step=0, fine_separation=1,
                                  want_total=False, want_zmap=True, want_ztotal=True):
        """tdoa_group_process_locate_track_zoom -> Context.process_locate_track_zoom's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate_track_zoom", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, min_separation=min_separation, Z=Z, H=H, fine_step=fine_step,
            fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap, want_ztotal=want_ztotal))


    def process_sync_locate(self, ref_delay, Z, H, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None, mix=None,
                            min_separation=1, fine_separation=1, want_map=False, want_zmap=True):
        """tdoa_group_process_sync_locate -> Context.process_sync_locate's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "sync_locate", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay,
            centre=centre, mix=mix, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation, want_map=want_map,
            want_zmap=want_zmap))


    def process_sync_drift_locate(self, ref_delay, Z, H, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, U=16,
                                  fine_rounds=2, centre=None, mix=None, max_step=0, min_separation=1, fine_step=0, fine_separation=1,
                                  want_total=False, want_zmap=True, want_ztotal=True):
        """tdoa_group_process_sync_drift_locate -> Context.process_sync_drift_locate's outputs, byte-identical to a single
        context's"""
        return _process_search(self, self.member(0), "sync_drift_locate", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds, U=U,
            fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre, mix=mix, max_step=max_step, min_separation=min_separation, Z=Z,
            H=H, fine_step=fine_step, fine_separation=fine_separation, want_total=want_total, want_zmap=want_zmap,
            want_ztotal=want_ztotal))


class Context(_LaterContextSearches):
    """One tdoa_ctx (one GPU, single caller)."""

    def __init__(self, **kw):
        self._L = load()
        p = _params(kw)
        self.params = p
        h = C.c_void_p()
        rc = self._L.tdoa_create(C.byref(p), C.byref(h))
        if rc != OK:
            raise TdoaError(rc, self._L.tdoa_strerror(rc).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.tdoa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            detail = self._L.tdoa_last_error(self._h).decode()
            raise TdoaError(rc, "%s (%s)" % (self._L.tdoa_strerror(rc).decode(), detail))

    # ---- mode A ------------------------------------------------------------
    def load_iq_u8(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        n = raw.size // 2
        out = np.empty(n, dtype=np.complex64)
        self._chk(self._L.tdoa_load_iq_u8(self._h, _u8(raw), n, _f(out.view(np.float32))))
        return out

    def preprocess(self, sig):
        a, v = _c64(sig)
        out = np.empty_like(a)
        weak = C.c_int()
        self._chk(self._L.tdoa_preprocess_c64(self._h, _f(v), a.size, _f(out.view(np.float32)), C.byref(weak)))
        return out, bool(weak.value)

    def time_domain_correlation(self, s1, s2, max_lag):
        a, va = _c64(s1)
        b, vb = _c64(s2)
        d, c = C.c_int32(), C.c_double()
        self._chk(self._L.tdoa_time_domain_correlation_c64(self._h, _f(va), a.size, _f(vb), b.size, int(max_lag),
                                                           C.byref(d), C.byref(c)))
        return d.value, c.value

    def cross_correlate(self, s1, s2):
        a, va = _c64(s1)
        b, vb = _c64(s2)
        d, c = C.c_int32(), C.c_double()
        self._chk(self._L.tdoa_cross_correlate_c64(self._h, _f(va), a.size, _f(vb), b.size, C.byref(d), C.byref(c)))
        return d.value, c.value

    def cross_correlate_batch(self, signals):
        """every signal preprocessed once, every pair i < j correlated (processor.go:816-850): [(delay, corr)] in pair order"""
        arrs = [_c64(x) for x in signals]
        k = len(arrs)
        ptrs = (C.POINTER(C.c_float) * k)(*[_f(v) for _, v in arrs])
        sizes = (C.c_size_t * k)(*[a.size for a, _ in arrs])
        npair = k * (k - 1) // 2
        d = (C.c_int32 * npair)()
        c = (C.c_double * npair)()
        self._chk(self._L.tdoa_cross_correlate_batch_c64(self._h, ptrs, sizes, k, d, c))
        return [(d[p], c[p]) for p in range(npair)]

    def simple_correlate(self, s1, s2):
        a, va = _c64(s1)
        b, vb = _c64(s2)
        d, c = C.c_int32(), C.c_float()
        self._chk(self._L.tdoa_simple_correlate_c64(self._h, _f(va), a.size, _f(vb), b.size, C.byref(d), C.byref(c)))
        return d.value, c.value

    def fast_snr(self, samples_u8, total_samples):
        s = np.ascontiguousarray(samples_u8, dtype=np.uint8)
        out = C.c_double()
        self._chk(self._L.tdoa_fast_snr_u8(self._h, _u8(s), int(total_samples), C.byref(out)))
        return out.value

    def fast_analyze(self, samples_u8, total_samples):
        s = np.ascontiguousarray(samples_u8, dtype=np.uint8)
        fa = FastAnalysis()
        self._chk(self._L.tdoa_fast_analyze_u8(self._h, _u8(s), int(total_samples), C.byref(fa)))
        return fa

    def fast_analyze_capture(self, raw_u8):
        """fast_analyzer's two output lines: (ref, tgt) analyses of one .dat capture."""
        s = np.ascontiguousarray(raw_u8, dtype=np.uint8)
        ref, tgt = FastAnalysis(), FastAnalysis()
        self._chk(self._L.tdoa_fast_analyze_capture_u8(self._h, _u8(s), s.size, C.byref(ref), C.byref(tgt)))
        return ref, tgt

    # ---- mode B ------------------------------------------------------------
    def capture_upload(self, station, iq_u8):
        s = np.ascontiguousarray(iq_u8, dtype=np.uint8)
        self._chk(self._L.tdoa_capture_upload(self._h, int(station), _u8(s), s.size // 2))

    def capture_upload_range(self, station, total_samples, first_sample, iq_u8):
        """upload only samples [first_sample, first_sample + len) of a capture of total_samples (sharded ingest)"""
        s = np.ascontiguousarray(iq_u8, dtype=np.uint8)
        self._chk(self._L.tdoa_capture_upload_range(self._h, int(station), int(total_samples), int(first_sample),
                                                    _u8(s), s.size // 2))

    def capture_upload_owned(self, station, iq_u8, rank, world, window_len):
        """upload the sample runs of `iq_u8` that tdoa_process(rank, world) reads; returns the bytes sent"""
        from . import sharding
        s = np.ascontiguousarray(iq_u8, dtype=np.uint8)
        sent = 0
        for first, count in sharding.owned_sample_runs(rank, world, s.size // 2, window_len):
            self.capture_upload_range(station, s.size // 2, first, s[2 * first:2 * (first + count)])
            sent += 2 * count
        return sent

    def capture_upload_file(self, station, path):
        n = C.c_size_t()
        self._chk(self._L.tdoa_capture_upload_file(self._h, int(station), os.fsencode(path), C.byref(n)))
        return n.value

    def capture_attach_device(self, station, dev_ptr, n_samples):
        self._chk(self._L.tdoa_capture_attach_device(self._h, int(station), C.c_void_p(int(dev_ptr)), int(n_samples)))

    def synth_capture(self, station, block_samples, station_lle, tx_lle, seed, ref_freq=162.4e6,
                      tgt_freq=101.7e6, noise=0.01, tx_power=1000.0):
        st = np.ascontiguousarray(station_lle, dtype=np.float64)
        tx = np.ascontiguousarray(tx_lle, dtype=np.float64)
        self._chk(self._L.tdoa_synth_capture(self._h, int(station), int(block_samples), ref_freq, tgt_freq, noise,
                                             _d(st), _d(tx), tx_power, int(seed)))

    def synth_weak_capture(self, station, block_samples, station_lle, tx_lle, seed, ref_freq=162.4e6,
                           tgt_freq=92.3e6, ref_power=10.0, tgt_power=1000.0):
        """weak_signal_simulator.go capture (weak reference blocks, strong target block) generated in HBM"""
        st = np.ascontiguousarray(station_lle, dtype=np.float64)
        tx = np.ascontiguousarray(tx_lle, dtype=np.float64)
        self._chk(self._L.tdoa_synth_weak_capture(self._h, int(station), int(block_samples), ref_freq, tgt_freq,
                                                  _d(st), _d(tx), ref_power, tgt_power, int(seed)))

    def capture_download(self, station, first_sample, n_samples):
        out = np.empty(2 * int(n_samples), dtype=np.uint8)
        self._chk(self._L.tdoa_capture_download(self._h, int(station), int(first_sample), int(n_samples), _u8(out)))
        return out

    def capture_clear(self):
        self._chk(self._L.tdoa_capture_clear(self._h))

    def num_windows(self):
        a, b = C.c_int(), C.c_int()
        self._chk(self._L.tdoa_num_windows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def num_pairs(self):
        return self._L.tdoa_num_pairs(self._h)

    def num_stations(self):
        p = self.num_pairs()
        return (1 + int(round((1 + 8 * p) ** 0.5))) // 2

    def process(self, rank=0, world=1, out_dev_ptr=None, want_host=True):
        wpb, w = self.num_windows()
        p = self.num_pairs()
        out = np.zeros((w, p), dtype=PEAK_DTYPE) if want_host else None
        self._chk(self._L.tdoa_process(self._h, int(rank), int(world),
                                       out.ctypes.data_as(C.c_void_p) if want_host else None,
                                       C.c_void_p(int(out_dev_ptr)) if out_dev_ptr else None))
        return out

    def window_quality_all(self, rank=0, world=1):
        """tdoa_window_quality_all -> [W][S] QUALITY_DTYPE"""
        wpb, w = self.num_windows()
        out = np.zeros((w, self.num_stations()), dtype=QUALITY_DTYPE)
        self._chk(self._L.tdoa_window_quality_all(self._h, int(rank), int(world), out.ctypes.data_as(C.c_void_p)))
        return out

    def window_quality(self, iq_u8):
        s = np.ascontiguousarray(iq_u8, dtype=np.uint8)
        out = np.zeros(1, dtype=QUALITY_DTYPE)
        self._chk(self._L.tdoa_window_quality_u8(self._h, _u8(s), s.size // 2, out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def process_fine(self, gate_samples, rank=0, world=1):
        """tdoa_process_fine -> (peaks [W][P], fine [W][P])"""
        wpb, w = self.num_windows()
        p = self.num_pairs()
        out = np.zeros((w, p), dtype=PEAK_DTYPE)
        fine = np.zeros((w, p), dtype=FINE_DTYPE)
        self._chk(self._L.tdoa_process_fine(self._h, int(rank), int(world), float(gate_samples),
                                            out.ctypes.data_as(C.c_void_p), fine.ctypes.data_as(C.c_void_p)))
        return out, fine

    def fm_xcorr_fine(self, iq1, iq2, max_lag, gate_samples):
        a = np.ascontiguousarray(iq1, dtype=np.uint8)
        b = np.ascontiguousarray(iq2, dtype=np.uint8)
        pk, fk = Peak(), FinePeak()
        self._chk(self._L.tdoa_fm_xcorr_fine_u8(self._h, _u8(a), a.size // 2, _u8(b), b.size // 2, int(max_lag),
                                                float(gate_samples), C.byref(pk), C.byref(fk)))
        return (pk.lag, pk.corr), dict(delay=fk.delay, frac=fk.frac, y=np.array(list(fk.y)),
                                       plausible=bool(fk.plausible))

    def process_u8(self, captures):
        caps = [np.ascontiguousarray(c, dtype=np.uint8) for c in captures]
        n = len(caps)
        ptrs = (C.POINTER(C.c_uint8) * n)(*[_u8(c) for c in caps])
        sizes = (C.c_size_t * n)(*[c.size // 2 for c in caps])
        blk = min(c.size // 2 for c in caps) // 3
        wl = min(self.params.window_len, blk)
        w = 3 * max(1, blk // wl) if blk >= 2 else 0
        out = np.zeros((w, n * (n - 1) // 2), dtype=PEAK_DTYPE)
        self._chk(self._L.tdoa_process_u8(self._h, ptrs, sizes, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def fm_xcorr(self, iq1, iq2, max_lag):
        a = np.ascontiguousarray(iq1, dtype=np.uint8)
        b = np.ascontiguousarray(iq2, dtype=np.uint8)
        pk = Peak()
        self._chk(self._L.tdoa_fm_xcorr_u8(self._h, _u8(a), a.size // 2, _u8(b), b.size // 2, int(max_lag), C.byref(pk)))
        return pk.lag, pk.corr

    def fm_xcorr_lags(self, iq1, iq2, max_lag):
        a = np.ascontiguousarray(iq1, dtype=np.uint8)
        b = np.ascontiguousarray(iq2, dtype=np.uint8)
        out = np.zeros(2 * max_lag - 1, dtype=np.float64)
        self._chk(self._L.tdoa_fm_xcorr_lags_u8(self._h, _u8(a), a.size // 2, _u8(b), b.size // 2, int(max_lag), _d(out)))
        return out

    def process_lags(self, rank=0, world=1, out_dev_ptr=None, want_host=True):
        """tdoa_process_lags -> [W][P][2 max_lag - 1] float32 correlation surfaces, reference scale (lag d at d + max_lag - 1);
        windows of other ranks are zero"""
        wpb, w = self.num_windows()
        out = np.zeros((w, self.num_pairs(), 2 * self.params.max_lag - 1), dtype=np.float32) if want_host else None
        self._chk(self._L.tdoa_process_lags(self._h, int(rank), int(world), _f(out) if want_host else None,
                                            C.c_void_p(int(out_dev_ptr)) if out_dev_ptr else None))
        return out

    def process_peaks(self, k, min_separation, rank=0, world=1):
        """tdoa_process_peaks -> (peaks [W][P][k] PEAK_DTYPE, count [W][P] int32): the k strongest separate peaks of every
        pair-window (include/tdoa_mi355x.h states the rule); peak 1 is process()'s"""
        wpb, w = self.num_windows()
        p = self.num_pairs()
        out = np.zeros((w, p, max(int(k), 1)), dtype=PEAK_DTYPE)
        count = np.zeros((w, p), dtype=np.int32)
        self._chk(self._L.tdoa_process_peaks(self._h, int(rank), int(world), int(k), int(min_separation),
                                             out.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, count

    def num_stacks(self, windows_per_stack=0):
        """tdoa_num_stacks -> (stacks_per_block, n_stacks_total)"""
        a, b = C.c_int(), C.c_int()
        self._chk(self._L.tdoa_num_stacks(self._h, int(windows_per_stack), C.byref(a), C.byref(b)))
        return a.value, b.value

    def process_stacked(self, windows_per_stack=0, k=1, min_separation=1, gate=None, rank=0, world=1, want_surface=False,
                        want_partial=False):
        """tdoa_process_stacked -> dict: peaks [n_stacks][P][k] PEAK_DTYPE, count [n_stacks][P] int32, fine [n_stacks][P]
        FINE_DTYPE (peak 1 refined; gate None: max_lag), and on request surface [n_stacks][P][2 max_lag - 1] float32 and
        partial (same shape, int64: the rank's fixed-point sums Q).  With world > 1 only `partial` means anything alone."""
        _, n = self.num_stacks(windows_per_stack)
        out = _stacked_outputs(n, self.num_pairs(), 2 * self.params.max_lag - 1, k, want_surface, want_partial)
        self._chk(self._L.tdoa_process_stacked(
            self._h, int(rank), int(world), int(windows_per_stack), int(k), int(min_separation),
            float(self.params.max_lag if gate is None else gate), out["peaks"].ctypes.data_as(C.c_void_p),
            out["count"].ctypes.data_as(C.POINTER(C.c_int32)), out["fine"].ctypes.data_as(C.c_void_p),
            _f(out["surface"]) if want_surface else None,
            out["partial"].ctypes.data_as(C.POINTER(C.c_int64)) if want_partial else None))
        return out

    def process_stacked_drift(self, windows_per_stack=0, max_drift=0, drift_den=1, k=1, min_separation=1, gate=None,
                              want_surface=False, want_partial=False, want_profile=True):
        """tdoa_process_stacked_drift -> the dict of process_stacked computed along the best of the 2 max_drift + 1 lag
        slopes h / drift_den lags per window, plus drift [n_stacks][P] int32 (h*) and, unless want_profile is False,
        profile [n_stacks][P][2 max_drift + 1] PEAK_DTYPE (the peak of every slope); partial is Q of h*"""
        _, n = self.num_stacks(windows_per_stack)
        p = self.num_pairs()
        out = _stacked_outputs(n, p, 2 * self.params.max_lag - 1, k, want_surface, want_partial)
        out["drift"] = np.zeros((n, p), dtype=np.int32)
        if want_profile:
            out["profile"] = np.zeros((n, p, 2 * max(int(max_drift), 0) + 1), dtype=PEAK_DTYPE)
        self._chk(self._L.tdoa_process_stacked_drift(
            self._h, int(windows_per_stack), int(k), int(min_separation),
            float(self.params.max_lag if gate is None else gate), int(max_drift), int(drift_den),
            out["peaks"].ctypes.data_as(C.c_void_p), out["count"].ctypes.data_as(C.POINTER(C.c_int32)),
            out["fine"].ctypes.data_as(C.c_void_p), _f(out["surface"]) if want_surface else None,
            out["partial"].ctypes.data_as(C.POINTER(C.c_int64)) if want_partial else None,
            out["drift"].ctypes.data_as(C.POINTER(C.c_int32)),
            out["profile"].ctypes.data_as(C.c_void_p) if want_profile else None))
        return out

    def process_track(self, windows_per_stack=0, max_step=1, want_surface=False, want_total=False):
        """tdoa_process_track -> dict: score [n_stacks][P] PEAK_DTYPE (lag: the track's lag at the stack's first window,
        corr: the signed sum along the track on C's scale), lags [n_stacks][P][mm] int32 and values [n_stacks][P][mm]
        float64 (each window's lag and its own correlation there; mm the stack length, positions past a shorter stack's
        end 0), and on request surface [n_stacks][P][2 max_lag - 1] float32 and total (same shape, int64): the best sum
        over the tracks that start at every lag"""
        _, n = self.num_stacks(windows_per_stack)
        p = self.num_pairs()
        wpb, _ = self.num_windows()
        mm = wpb if int(windows_per_stack) <= 0 else min(int(windows_per_stack), wpb)
        n_lags = 2 * self.params.max_lag - 1
        out = {"score": np.zeros((n, p), dtype=PEAK_DTYPE), "lags": np.zeros((n, p, mm), dtype=np.int32),
               "values": np.zeros((n, p, mm), dtype=np.float64)}
        if want_surface:
            out["surface"] = np.zeros((n, p, n_lags), dtype=np.float32)
        if want_total:
            out["total"] = np.zeros((n, p, n_lags), dtype=np.int64)
        self._chk(self._L.tdoa_process_track(
            self._h, int(windows_per_stack), int(max_step), out["score"].ctypes.data_as(C.c_void_p),
            out["lags"].ctypes.data_as(C.POINTER(C.c_int32)), _d(out["values"]),
            _f(out["surface"]) if want_surface else None,
            out["total"].ctypes.data_as(C.POINTER(C.c_int64)) if want_total else None))
        return out

    def num_triples(self):
        """tdoa_num_triples: S (S-1) (S-2) / 6 station triples (0 with fewer than three stations)"""
        return self._L.tdoa_num_triples(self._h)

    def process_closure(self, windows_per_stack=0, gate=0, min_separation=1, centre=None):
        """tdoa_process_closure -> [n_stacks][T] CLOSURE_DTYPE: per stack and station triple i < j < k the three lags that
        close (lag_ij + lag_jk = lag_ik) with the largest summed magnitude within `gate` lags of the pairs' centres
        (centre: one int per station, None: all 0), next to what the three independent argmaxes give (own_q, residual)
        and the runner-up"""
        return _process_search(self, self, "closure", dict(
            windows_per_stack=windows_per_stack, gate=gate, min_separation=min_separation, centre=centre), T=self.num_triples())

    def closure_from_q(self, q, n_stations, n_w=1, gate=0, min_separation=1, centre=None):
        """tdoa_debug_closure_from_q: the closure kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64 (or one
        set [P][2 max_lag - 1]) -> [n_sets][T] CLOSURE_DTYPE"""
        return self._from_q("closure", q, n_stations, dict(n_w=n_w, gate=gate, min_separation=min_separation, centre=centre))

    def locate_set_table(self, table, n_cols=None):
        """tdoa_locate_set_table: table [n_cells][n_stations] int32 delays in units of 1/16 sample; n_cols gives cells their
        rows and columns (None: a plain list).  table None: forget it.  Kept on the device until replaced"""
        ptr, n_cells, n_cols, S = _table(table, n_cols)
        self._chk(self._L.tdoa_locate_set_table(self._h, ptr, n_cells, n_cols, S))
        self._locate_cells = n_cells

    def process_locate(self, windows_per_stack=0, min_separation=1, want_map=False):
        """tdoa_process_locate -> {"loc": [n_stacks] LOCATION_DTYPE, "lags": [n_stacks][P] int32, "corr": [n_stacks][P]
        float64, and with want_map "map": [n_stacks][n_cells] int64}: per stack the table's cell with the largest summed
        magnitude of all pairs' stacks at the cell's lags, the runner-up, and the lags and signed correlations there"""
        return _process_search(self, self, "locate", dict(
            windows_per_stack=windows_per_stack, min_separation=min_separation, want_map=want_map))

    def locate_from_q(self, q, n_stations, n_w=1, min_separation=1, want_map=True):
        """tdoa_debug_locate_from_q: the search's kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64 (or one
        set [P][2 max_lag - 1]) with the context's table -> what process_locate returns, n_sets for n_stacks"""
        return self._from_q("locate", q, n_stations, dict(n_w=n_w, min_separation=min_separation, want_map=want_map))

    def locate_set_clock(self, clock):
        """tdoa_locate_set_clock: clock [n_stacks][n_stations] int32 station clocks in units of 1/16 sample, one row per stack
        of the searches that follow.  clock None: forget them.  Kept on the device until replaced"""
        self._chk(self._L.tdoa_locate_set_clock(self._h, *_clock(clock)))

    def locate_set_stats(self, ranks, foot=0):
        """tdoa_locate_set_stats: while set, every process_locate*, locate*_from_q call also computes MAP_STATS_DTYPE
        statistics of every judged plane (its dict gains "stats", shaped like "loc" or "track"): the live words' exact order
        statistics at `ranks` (up to 8 values 0 .. 65535; 32768: the median) and, with foot > 0, the cells that reach
        foot / 65536 of the way from the first rank's word to the best.  ranks None: off"""
        self._chk(self._L.tdoa_locate_set_stats(self._h, *_ranks(ranks), int(foot)))
        self._stats_on = ranks is not None and np.size(ranks) > 0

    def locate_last_stats(self):
        """tdoa_locate_last_stats -> [n_planes] MAP_STATS_DTYPE of the last call of the delay-table family, in its records'
        order"""
        return _last_stats(self, self._L.tdoa_locate_last_stats)

    def locate_set_upsample(self, U):
        """tdoa_locate_set_upsample: while U in {2, 4, 8, 16} is set, every process_locate*, locate*_from_q call scores its
        cells on the surfaces upsampled to 1/U sample (tdoa_amd.upsample states it); "lags" are then in units of 1/U sample.
        U = 1: off"""
        self._chk(self._L.tdoa_locate_set_upsample(self._h, int(U)))

    def locate_set_fine_table(self, table, n_cols=None):
        """tdoa_locate_set_fine_table: the zoom locate's second table [n_cells_f][n_stations] int32, in n_cols columns, Z fine
        cells per cell of the table.  table None: forget it.  Kept on the device until replaced"""
        ptr, n_cells, n_cols, S = _table(table, n_cols)
        self._chk(self._L.tdoa_locate_set_fine_table(self._h, ptr, n_cells, n_cols, S))

    def process_locate_zoom(self, Z, H, windows_per_stack=0, min_separation=1, fine_separation=1, want_map=False, want_zmap=True):
        """tdoa_process_locate_zoom -> process_locate's dict (the coarse stage's bytes) and {"zoom": [n_stacks] ZOOM_DTYPE,
        "zlags": [n_stacks][P] int32 (1/U sample), "zcorr": [n_stacks][P] float64, and with want_zmap "zmap":
        [n_stacks][(2H+1)^2] int64}: per stack the best of the (2H+1)^2 cells of the fine table around Z x its best cell.  The
        zoom's arrays are written over a poison pattern"""
        return _process_search(self, self, "locate_zoom", dict(
            windows_per_stack=windows_per_stack, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation,
            want_map=want_map, want_zmap=want_zmap))

    def locate_zoom_from_q(self, q, n_stations, Z, H, n_w=1, min_separation=1, fine_separation=1, want_map=True, want_zmap=True):
        """tdoa_debug_locate_zoom_from_q: the locate's and the zoom's kernels on the caller's words q [n_sets][P][2 max_lag - 1]
        int64 (or one set) with the context's table, fine table and clocks -> what process_locate_zoom returns, n_sets for
        n_stacks"""
        return self._from_q("locate_zoom", q, n_stations, dict(
            n_w=n_w, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation, want_map=want_map,
            want_zmap=want_zmap))

    def upsample_q(self, q, U):
        """tdoa_debug_upsample_q: the upsampler on the caller's rows q [n_rows][2 max_lag - 1] int64 (or one row) ->
        [n_rows][(2 max_lag - 2) U + 1] int64, written over a poisoned array"""
        q = np.ascontiguousarray(q, dtype=np.int64)
        one = q.ndim == 1
        if one:
            q = q[None]
        n = 2 * self.params.max_lag - 1
        if q.ndim != 2 or q.shape[1] != n:
            raise ValueError("q must be [n_rows][2 max_lag - 1]")
        out = np.full((q.shape[0], (n - 1) * int(U) + 1 if int(U) > 0 else 1), -0x0123456789ABCDEF, dtype=np.int64)
        self._chk(self._L.tdoa_debug_upsample_q(self._h, q.ctypes.data_as(C.POINTER(C.c_int64)), q.shape[0], int(U),
                                                out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out[0] if one else out

    def _from_q(self, name, q, n_stations, values):
        """search `name` on the caller's words q"""
        s, S = _search(name), int(n_stations)
        q = _q_sets(q, S, self.params.max_lag)
        n = _shape_numbers(values, q.shape[0], S, getattr(self, "_locate_cells", 0), values.get("track_len", 1))
        out = _run_search(s, "q", getattr(self._L, s.entries["q"]), self._h, self._chk, n, values, q)
        return self._with_stats(out, s.stats) if s.stats else out

    def _with_stats(self, out, like):
        """out with "stats" shaped like out[like] while the setting is on"""
        if getattr(self, "_stats_on", False):
            out["stats"] = self.locate_last_stats().reshape(out[like].shape)
        return out

    def process_sync(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, centre=None):
        """tdoa_process_sync -> {"sync": [n_stacks] SYNC_DTYPE, "clock": [n_stacks][S] int32 (samples), "lags": [n_stacks][P]
        int32, "corr": [n_stacks][P] float64}: per stack the station clocks k_s = centre[s] + x_s, |x_s| <= gate, k_0 =
        centre[0], that make all pairs' stacks largest at the lags the known emitter's delays ref_delay [S] (units of 1/16
        sample) predict; a joint start, the placing and `rounds` sweeps"""
        return _process_search(self, self, "sync", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, ref_delay=ref_delay, centre=centre))

    def sync_from_q(self, q, ref_delay, n_w=1, gate=0, rounds=0, centre=None):
        """tdoa_debug_sync_from_q: the clock search's kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64 (or
        one set [P][2 max_lag - 1]) -> what process_sync returns, n_sets for n_stacks"""
        return self._from_q("sync", q, np.size(ref_delay), dict(
            n_w=n_w, gate=gate, rounds=rounds, ref_delay=ref_delay, centre=centre))

    def process_sync_fine(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None):
        """tdoa_process_sync_fine -> process_sync's outputs (the coarse stage's bytes) and {"fine": [n_stacks] SYNC_DTYPE,
        "clock16": [n_stacks][S] int32 (1/16 sample: tdoa_locate_set_clock's unit), "fine_lags": [n_stacks][P] int32 (1/U
        sample), "fine_corr": [n_stacks][P] float64}: the coarse clocks moved by |y_s| <= U fine lags in `fine_rounds` sweeps
        on the words of the surfaces upsampled to 1/U sample"""
        return _process_search(self, self, "sync_fine", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay,
            centre=centre))

    def sync_fine_from_q(self, q, ref_delay, n_w=1, gate=0, rounds=0, U=16, fine_rounds=2, centre=None):
        """tdoa_debug_sync_fine_from_q: the clock search's and the refinement's kernels on the caller's words q
        [n_sets][P][2 max_lag - 1] int64 (or one set [P][2 max_lag - 1]) -> what process_sync_fine returns, n_sets for n_stacks"""
        return self._from_q("sync_fine", q, np.size(ref_delay), dict(
            n_w=n_w, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay, centre=centre))

    def process_sync_drift(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None):
        """tdoa_process_sync_drift -> {"line": [3] SYNC_LINE_DTYPE, "clock": [3][S] int32 (samples), "rate": [3][S] int32,
        "rows": [n_stacks][S] int32 (1/16 sample: tdoa_locate_set_clock's unit), "lags": [n_stacks][P] int32, "corr":
        [n_stacks][P] float64}: per block the station clocks k_s(j) = k_s + shift(h_s, j), |k_s - centre[s]| <= gate, |h_s| <=
        max_drift in units of 1 / drift_den lag per stack, that make all pairs' signed sums along the block's stacks largest
        at the lags the known emitter's delays ref_delay [S] predict; the placing and `rounds` sweeps"""
        return _process_search(self, self, "sync_drift", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds,
            ref_delay=ref_delay, centre=centre), n_tracks=3)

    def sync_drift_from_q(self, q, ref_delay, track_len, n_w=1, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None):
        """tdoa_debug_sync_drift_from_q: the clock-line search's kernels on the caller's words q [n_sets][P][2 max_lag - 1]
        int64, set t track_len + j position j of line t -> what process_sync_drift returns, n_sets / track_len lines and
        n_sets stacks"""
        return self._from_q("sync_drift", q, np.size(ref_delay), dict(
            track_len=track_len, n_w=n_w, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds,
            ref_delay=ref_delay, centre=centre))

    def process_locate_track(self, windows_per_stack=0, max_step=0, min_separation=1, want_total=False):
        """tdoa_process_locate_track -> {"track": [n_tracks] CELL_TRACK_DTYPE, "cells": [n_tracks][L] int32, "own":
        [n_tracks][L] int64, "lags": [n_stacks][P] int32, "corr": [n_stacks][P] float64, and with want_total "total":
        [n_tracks][n_cells] int64}: per block the track of cells through its stacks' maps, consecutive cells at most max_step
        rows and columns apart, with the largest summed score; the runner-up; per stack the lags and signed correlations at
        the track's cell"""
        return _process_search(self, self, "locate_track", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, min_separation=min_separation, want_total=want_total))

    def locate_track_from_q(self, q, n_stations, track_len, n_w=1, max_step=0, min_separation=1, want_total=True):
        """tdoa_debug_locate_track_from_q: the search's and the recurrence's kernels on the caller's words q
        [n_sets][P][2 max_lag - 1] int64, set t track_len + j position j of track t, with the context's table and clocks ->
        what process_locate_track returns, n_sets for n_stacks"""
        return self._from_q("locate_track", q, n_stations, dict(
            track_len=track_len, n_w=n_w, max_step=max_step, min_separation=min_separation, want_total=want_total))

    def process_locate_multi(self, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, want_map=False):
        """tdoa_process_locate_multi -> process_locate's dict with a leading axis of n_emitters rounds: "loc" [K][n_stacks],
        "lags" and "corr" [K][n_stacks][P], with want_map "map" [K][n_stacks][n_cells].  Round r searches with the lags within
        `guard` of the earlier rounds' cells' lags counting 0 in every pair"""
        return _process_search(self, self, "locate_multi", dict(
            windows_per_stack=windows_per_stack, n_emitters=n_emitters, guard=guard, min_separation=min_separation,
            want_map=want_map))

    def locate_multi_from_q(self, q, n_stations, n_w=1, n_emitters=1, guard=0, min_separation=1, want_map=True):
        """tdoa_debug_locate_multi_from_q: the rounds' kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64 (or one
        set [P][2 max_lag - 1]) with the context's table and clocks -> what process_locate_multi returns, n_sets for n_stacks"""
        return self._from_q("locate_multi", q, n_stations, dict(
            n_w=n_w, n_emitters=n_emitters, guard=guard, min_separation=min_separation, want_map=want_map))

    def process_locate_track_multi(self, windows_per_stack=0, max_step=0, n_emitters=1, guard=0, min_separation=1, want_total=False):
        """tdoa_process_locate_track_multi -> process_locate_track's dict with a leading axis of n_emitters rounds: "track"
        [K][n_tracks], "cells" and "own" [K][n_tracks][L], "lags" and "corr" [K][n_stacks][P], "pairs" [K][n_stacks][2] int32
        (pairs_in, reserved), with want_total "total" [K][n_tracks][n_cells].  Round r tracks with the lags within `guard` of
        the earlier rounds' tracks' lags counting 0 in every stack's pairs"""
        return _process_search(self, self, "locate_track_multi", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, n_emitters=n_emitters, guard=guard,
            min_separation=min_separation, want_total=want_total))

    def locate_track_multi_from_q(self, q, n_stations, track_len, n_w=1, max_step=0, n_emitters=1, guard=0, min_separation=1,
                                  want_total=True):
        """tdoa_debug_locate_track_multi_from_q: the rounds' kernels on the caller's words q [n_sets][P][2 max_lag - 1] int64, set
        t track_len + j position j of track t, with the context's table and clocks -> what process_locate_track_multi returns,
        n_sets for n_stacks"""
        return self._from_q("locate_track_multi", q, n_stations, dict(
            track_len=track_len, n_w=n_w, max_step=max_step, n_emitters=n_emitters, guard=guard, min_separation=min_separation,
            want_total=want_total))

    def fm_xcorr_peaks(self, iq1, iq2, max_lag, k, min_separation):
        """tdoa_fm_xcorr_peaks_u8 -> (peaks [k] PEAK_DTYPE, count) of one pair of windows"""
        a = np.ascontiguousarray(iq1, dtype=np.uint8)
        b = np.ascontiguousarray(iq2, dtype=np.uint8)
        out = np.zeros(max(int(k), 1), dtype=PEAK_DTYPE)
        count = C.c_int32()
        self._chk(self._L.tdoa_fm_xcorr_peaks_u8(self._h, _u8(a), a.size // 2, _u8(b), b.size // 2, int(max_lag), int(k),
                                                 int(min_separation), out.ctypes.data_as(C.c_void_p), C.byref(count)))
        return out, count.value

    def debug_select_peaks(self, surface, lag_lo, k, min_separation):
        """tdoa_debug_select_peaks: the selection kernel on a raw surface (lags lag_lo, lag_lo + 1, ...) at scale 1 ->
        (peaks [k] PEAK_DTYPE, count)"""
        c = np.ascontiguousarray(surface, dtype=np.float32)
        out = np.zeros(max(int(k), 1), dtype=PEAK_DTYPE)
        count = C.c_int32()
        self._chk(self._L.tdoa_debug_select_peaks(self._h, _f(c), c.size, int(lag_lo), int(k), int(min_separation),
                                                  out.ctypes.data_as(C.c_void_p), C.byref(count)))
        return out, count.value

    def fm_preprocess(self, iq):
        a = np.ascontiguousarray(iq, dtype=np.uint8)
        out = np.empty(a.size // 2, dtype=np.float32)
        st = FmStats()
        self._chk(self._L.tdoa_fm_preprocess_u8(self._h, _u8(a), a.size // 2, _f(out), C.byref(st)))
        return out, st

    def graph_info(self, dot_path=None):
        """{nodes, edges, roots, memsets} of the step graph the last process() captured (tdoa_debug_graph_info)"""
        info = (C.c_int32 * 4)()
        self._chk(self._L.tdoa_debug_graph_info(self._h, info, dot_path.encode() if dot_path else None))
        return dict(nodes=info[0], edges=info[1], roots=info[2], memsets=info[3])

    def poison_workspace(self):
        """fill the float workspaces with NaN (tdoa_debug_poison_workspace): a later call that reads what it did not write
        then shows NaN instead of an earlier call's values"""
        self._chk(self._L.tdoa_debug_poison_workspace(self._h))

    def last_route(self):
        """the kernel forms of the last batch planned, or of the batch the replayed step graph captured
        (tdoa_debug_last_route): {"inverse", "pair_step", "col_pass", "row_pass": names; "fk", "seg_pq": numbers; the
        ROUTE_FLAGS, "stg_merged" (the staged walk settles the neighbour shares inside a 64-column block), "k1_split" (the
        fused column kernel reads the split half-plane angle table), "stg_paired" (the staged walk's spectra lie in paired
        lines, one KB per LDS-DMA) and "stg_nt" (its loader wave's loads are non-temporal): bools}"""
        info = (C.c_int32 * 16)()
        self._chk(self._L.tdoa_debug_last_route(self._h, info))
        out = dict(inverse=ROUTE_INVERSE[info[0]], pair_step=ROUTE_PAIR_STEP[info[1]], col_pass=ROUTE_COL_PASS[info[2]],
                   row_pass=ROUTE_ROW_PASS[info[3]], fk=info[4], seg_pq=info[5])
        out.update((name, bool(info[6 + k])) for k, name in enumerate(ROUTE_FLAGS))
        out.update((name, bool(info[15] & bit)) for name, bit in ROUTE_BIT_FLAGS.items())
        return out

    def fm_stats(self, iq):
        """window statistics from the reduce-only pass of the fused path (tdoa_fm_preprocess_u8 with out_f32 = NULL)"""
        a = np.ascontiguousarray(iq, dtype=np.uint8)
        st = FmStats()
        self._chk(self._L.tdoa_fm_preprocess_u8(self._h, _u8(a), a.size // 2, None, C.byref(st)))
        return st

    def force_generic(self, on=True):
        self._chk(self._L.tdoa_debug_force_generic(self._h, 1 if on else 0))

    def debug_flags(self, generic=False, no_short_lag=False, no_fused_k1=False, no_segment_form=False, no_xcd_rows=False,
                    no_segment_quads=False, no_decimate=False, no_k1_once=False, no_seg_pack3=False, no_dec_cols=False, dec_cols_always=False, pow2_only=False, no_dec_staged=False, no_small_fused=False, small_fused_always=False):
        """pick kernel variants by hand (tests / measurements): include/tdoa_mi355x.h TDOA_DEBUG_*; no argument = the
        library's default path, every argument switches one specialised form off"""
        self._chk(self._L.tdoa_debug_flags(self._h, (1 if generic else 0) | (2 if no_short_lag else 0) |
                                           (4 if no_fused_k1 else 0) | (8 if no_segment_form else 0) |
                                           (16 if no_xcd_rows else 0) | (64 if no_segment_quads else 0) |
                                           (256 if no_decimate else 0) | (512 if no_k1_once else 0) |
                                           (1024 if no_seg_pack3 else 0) | (2048 if no_dec_cols else 0) |
                                           (4096 if dec_cols_always else 0) | (8192 if pow2_only else 0) | (16384 if no_dec_staged else 0) | (32768 if no_small_fused else 0) | (65536 if small_fused_always else 0)))

    def last_k1(self, sw_index=0):
        """(statistics of station-window `sw_index` of the last batch, True if that batch read every capture byte once:
        the single-look K1 of csrc/k1_single_look.hpp) -- tdoa_debug_last_k1"""
        st = FmStats()
        once = C.c_int32(0)
        self._chk(self._L.tdoa_debug_last_k1(self._h, int(sw_index), C.byref(st), C.byref(once)))
        return st, bool(once.value)

    # ---- measurement -------------------------------------------------------
    def profile_enable(self, on=True):
        """True / 1: launch by launch with events; 2: events as nodes of the replayed step graph; False / 0: off"""
        self._chk(self._L.tdoa_profile_enable(self._h, int(on)))

    def profile_select(self, names=None):
        """record events only for the named scopes (tdoa_kernel_name); None = all"""
        if names is None:
            mask = 0xffffffff
        else:
            all_names = [self._L.tdoa_kernel_name(k).decode() for k in range(len(KERNELS))]
            mask = 0
            for n in names:
                mask |= 1 << all_names.index(n)
        self._chk(self._L.tdoa_profile_select(self._h, mask))

    def profile_reset(self):
        self._chk(self._L.tdoa_profile_reset(self._h))

    def profile(self):
        out = {}
        for k, name in enumerate(KERNELS):
            ms, n, b = C.c_double(), C.c_int64(), C.c_double()
            self._chk(self._L.tdoa_profile_get(self._h, k, C.byref(ms), C.byref(n), C.byref(b)))
            out[self._L.tdoa_kernel_name(k).decode()] = {"ms": ms.value, "launches": n.value, "bytes": b.value}
        return out

    def plan_info(self):
        n, n1, n2 = C.c_int64(), C.c_int32(), C.c_int32()
        self._chk(self._L.tdoa_plan_info(self._h, C.byref(n), C.byref(n1), C.byref(n2)))
        return n.value, n1.value, n2.value


def _centre(centre, n_stations):
    """the centres as the C ABI takes them: None, or n_stations int32"""
    if centre is None:
        return None
    c = np.ascontiguousarray(centre, dtype=np.int32)
    if c.shape != (int(n_stations),):
        raise ValueError("centre must hold one integer per station")
    return c.ctypes.data_as(C.POINTER(C.c_int32))


def _table(table, n_cols):
    """(pointer, n_cells, n_cols, n_stations) of a delay table as the C ABI takes it; None: (NULL, 0, 1, 0)"""
    if table is None:
        return None, 0, 1, 0
    t = np.ascontiguousarray(table, dtype=np.int32)
    if t.ndim != 2:
        raise ValueError("table must be [n_cells][n_stations]")
    return t.ctypes.data_as(C.POINTER(C.c_int32)), t.shape[0], int(t.shape[0] if n_cols is None else n_cols), t.shape[1]


def _clock(clock):
    """(pointer, n_stacks, n_stations) of a clock table as the C ABI takes it; None: (NULL, 0, 0)"""
    if clock is None:
        return None, 0, 0
    k = np.ascontiguousarray(clock, dtype=np.int32)
    if k.ndim != 2:
        raise ValueError("clock must be [n_stacks][n_stations]")
    return k.ctypes.data_as(C.POINTER(C.c_int32)), k.shape[0], k.shape[1]


def _ref_delay(ref_delay, n_stations):
    """the known emitter's delays as the C ABI takes them: n_stations int32"""
    r = np.ascontiguousarray(ref_delay, dtype=np.int32).reshape(-1)
    if r.shape != (int(n_stations),):
        raise ValueError("ref_delay must hold one delay per station")
    return r.ctypes.data_as(C.POINTER(C.c_int32))


def _q_sets(q, n_stations, max_lag):
    """the caller's words as the from-Q entries take them: [n_sets][P][2 max_lag - 1] int64, one set promoted"""
    q = np.ascontiguousarray(q, dtype=np.int64)
    if q.ndim == 2:
        q = q[None]
    if q.ndim != 3 or q.shape[1:] != (n_stations * (n_stations - 1) // 2, 2 * max_lag - 1):
        raise ValueError("q must be [n_sets][S (S-1) / 2][2 max_lag - 1]")
    return q


def _poisoned(shape, dtype):
    """an output array the library has to write every byte of"""
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = 0xA5
    return a


def _shape_numbers(values, n_sets, S, n_cells=0, track_len=1, **given):
    """the numbers the outputs' shapes name.  A count the library refuses is clamped: the arrays only have to exist.  `given`
    states P, T or n_tracks where the caller knows them better"""
    n = {"n_sets": n_sets, "S": S, "n_cells": n_cells, "P": S * (S - 1) // 2, "T": max(S * (S - 1) * (S - 2) // 6, 1),
         "L": max(int(track_len), 1), "K": min(max(int(values.get("n_emitters", 1)), 1), 8),
         "window": (2 * min(max(int(values.get("H", 0)), 0), 64) + 1) ** 2}
    n["n_tracks"] = max(n_sets // n["L"], 1)             # (the library refuses a call without a whole track or line)
    n.update(given)
    return n


def _search_outputs(s, n, values):
    """{key: array} of search s's outputs; an optional one only where values[its flag] asks for it"""
    return {o.key: (_poisoned if o.poison else np.zeros)([n.get(d, d) for d in o.shape], o.dtype)
            for o in s.outputs if o.want is None or values[o.want]}


def _search_ptrs(s, out):
    """the outputs' pointers in the header's order, None for one that is absent"""
    return [out[o.key].ctypes.data_as(o.ctype) if o.key in out else None for o in s.outputs]


def _mix(mix, n_stations=None, width=4):
    """a mix as the C ABI takes it: None, or [m][width] int32: (a, b, wa, wb), tdoa_clock_mix's layout, or with width 6
    (a, xa, b, xb, wa, wb), tdoa_line_mix's"""
    if mix is None:
        return None
    names = ("a", "b", "wa", "wb") if width == 4 else ("a", "xa", "b", "xb", "wa", "wb")
    m = np.asarray(mix)
    if m.dtype.names:
        m = np.stack([m[k] for k in names], axis=-1)
    m = np.ascontiguousarray(m, dtype=np.int32)
    if m.ndim != 2 or m.shape[1] != width:
        raise ValueError("mix must be [m][%d]: %s" % (width, ", ".join(names)))
    return m.ctypes.data_as(C.POINTER(C.c_int32))


def _line_words(clock16, fine_rate):
    """the fine lines' clocks and rates as the C ABI takes them: two [n_lines][S] int32"""
    c, h = np.ascontiguousarray(clock16, dtype=np.int32), np.ascontiguousarray(fine_rate, dtype=np.int32)
    if c.ndim != 2 or c.shape != h.shape:
        raise ValueError("clock16 and fine_rate must be [n_lines][S]")
    return c, h


_INPUT = {"ref_delay": _ref_delay, "centre": _centre, "mix": _mix}


def _run_search(s, route, fn, handle, chk, n, values, q=None):
    """One call of search s (a SEARCHES record) through `route`: "own", "group", or "q" with the caller's words q (_q_sets').
    fn is that entry's C function and chk raises on its status; n are the _shape_numbers; values holds what the caller gave,
    by the header's parameter names: windows_per_stack or (track_len,) n_w, s.ints, s.inputs and the want_* flags"""
    out = _search_outputs(s, n, values)
    if route == "q":
        shape = ([q.ctypes.data_as(C.POINTER(C.c_int64)), n["n_sets"]] + ([int(values["track_len"])] if s.track_len else []) +
                 [n["S"], int(values["n_w"])])
    else:
        shape = [int(values["windows_per_stack"])]
    if values.get("mix") is not None and np.shape(values["mix"])[0] != n["n_sets"]:
        raise ValueError("mix must hold one entry per stack")
    chk(fn(handle, *shape, *[int(values[k]) for k in s.ints],
           *[_mix(values[k], width=s.mix_width) if k == "mix" else _INPUT[k](values[k], n["S"]) for k in s.inputs],
           *[int(values[k]) for k in s.late_ints], *_search_ptrs(s, out)))
    return out[s.outputs[0].key] if s.bare else out


def _process_search(owner, counts, name, values, **given):
    """search `name` on owner's own sum (a Context: counts is owner) or merged sum (a Group: counts is its member 0)"""
    s = _search(name)
    route = "own" if counts is owner else "group"
    per_block, n_sets = counts.num_stacks(values["windows_per_stack"])
    n = _shape_numbers(values, n_sets, counts.num_stations(), getattr(owner, "_locate_cells", 0), per_block, **given)
    out = _run_search(s, route, getattr(owner._L, s.entries[route]), owner._h, owner._chk, n, values)
    return owner._with_stats(out, s.stats) if s.stats else out


def _zoom_outputs(n_sets, p, n_cells, H, want_map, want_zmap):
    return _search_outputs(SEARCHES["locate_zoom"], _shape_numbers({"H": H}, n_sets, 0, n_cells, P=p),
                           {"want_map": want_map, "want_zmap": want_zmap})


def _zoom_ptrs(out):
    return tuple(_search_ptrs(SEARCHES["locate_zoom"], out))


def _stacked_outputs(n_stacks, p, n_lags, k, want_surface, want_partial):
    out = {"peaks": np.zeros((n_stacks, p, max(int(k), 1)), dtype=PEAK_DTYPE), "count": np.zeros((n_stacks, p), dtype=np.int32),
           "fine": np.zeros((n_stacks, p), dtype=FINE_DTYPE)}
    if want_surface:
        out["surface"] = np.zeros((n_stacks, p, n_lags), dtype=np.float32)
    if want_partial:
        out["partial"] = np.zeros((n_stacks, p, n_lags), dtype=np.int64)
    return out


def _ranks(ranks):
    """(pointer, n_ranks) of the statistics' ranks as the C ABI takes them; None: (NULL, 0)"""
    if ranks is None:
        return None, 0
    r = np.ascontiguousarray(ranks).reshape(-1)
    if r.size and (r.min() < 0 or r.max() > 65535):
        raise ValueError("ranks are 0 .. 65535")
    r = r.astype(np.uint16)
    return r.ctypes.data_as(C.POINTER(C.c_uint16)), r.size


def _last_stats(owner, call):
    n = C.c_int(0)
    rc = call(owner._h, None, 0, C.byref(n))             # the count first (a state error when there are none)
    if n.value == 0:
        owner._chk(rc)
    out = np.zeros(max(n.value, 1), dtype=MAP_STATS_DTYPE)
    owner._chk(call(owner._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return out[:n.value]


class _Member(Context):
    """A group member's tdoa_ctx, borrowed (tdoa_group_member): every Context call; close() leaves it to the group."""

    def __init__(self, group, handle):
        self._L = group._L
        self.params = group.params
        self._group = group                  # the group outlives its views
        self._h = C.c_void_p(handle)

    def close(self):
        self._h = None


class Group(_LaterGroupSearches):
    """A multi-device group (tdoa_group): one tdoa_ctx per member, member k = rank k of len(devices) in tdoa_process's
    sharding; devices may repeat (several members on one GPU).  Keyword arguments are tdoa_params fields, as for Context."""

    def __init__(self, devices, **kw):
        self._L = load()
        self.params = _params(kw)
        self.devices = [int(d) for d in devices]
        n = len(self.devices)
        devs = (C.c_int32 * n)(*self.devices)
        h = C.c_void_p()
        rc = self._L.tdoa_group_create(C.byref(self.params), devs if n else None, n, C.byref(h))
        if rc != OK:
            raise TdoaError(rc, "%s (%s)" % (self._L.tdoa_strerror(rc).decode(), self._L.tdoa_group_last_error(None).decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.tdoa_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            detail = self._L.tdoa_group_last_error(self._h).decode()
            raise TdoaError(rc, "%s (%s)" % (self._L.tdoa_strerror(rc).decode(), detail))

    def member(self, k):
        """member k's context, borrowed: synth / download / debug calls on that member alone"""
        h = self._L.tdoa_group_member(self._h, int(k))
        if not h:
            raise IndexError("no member %r in a group of %d" % (k, len(self.devices)))
        return _Member(self, h)

    def capture_upload_files(self, paths):
        """station s = paths[s] (.dat, raw u8 I,Q); every member reads only the sample runs its windows need.
        Returns size/2 per file."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        ns = (C.c_size_t * n)()
        self._chk(self._L.tdoa_group_capture_upload_files(self._h, n, arr, ns))
        return list(ns)

    def process(self, out=None):
        """tdoa_group_process -> [W][P] PEAK_DTYPE, byte-identical to a single context's process(); `out` (optional): a
        C-contiguous [W][P] PEAK_DTYPE array to write into (left as it was if the call fails)"""
        m = self.member(0)
        _, w = m.num_windows()
        p = m.num_pairs()
        if out is None:
            out = np.zeros((w, p), dtype=PEAK_DTYPE)
        elif out.dtype != PEAK_DTYPE or out.shape != (w, p) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (%d, %d) PEAK_DTYPE array" % (w, p))
        self._chk(self._L.tdoa_group_process(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def process_stacked(self, windows_per_stack=0, k=1, min_separation=1, gate=None, want_surface=False):
        """tdoa_group_process_stacked -> the dict of Context.process_stacked (no partial), byte-identical to a single
        context's"""
        m = self.member(0)
        _, n = m.num_stacks(windows_per_stack)
        out = _stacked_outputs(n, m.num_pairs(), 2 * self.params.max_lag - 1, k, want_surface, False)
        self._chk(self._L.tdoa_group_process_stacked(
            self._h, int(windows_per_stack), int(k), int(min_separation),
            float(self.params.max_lag if gate is None else gate), out["peaks"].ctypes.data_as(C.c_void_p),
            out["count"].ctypes.data_as(C.POINTER(C.c_int32)), out["fine"].ctypes.data_as(C.c_void_p),
            _f(out["surface"]) if want_surface else None))
        return out

    def process_closure(self, windows_per_stack=0, gate=0, min_separation=1, centre=None):
        """tdoa_group_process_closure -> [n_stacks][T] CLOSURE_DTYPE, byte-identical to a single context's"""
        m = self.member(0)
        return _process_search(self, m, "closure", dict(
            windows_per_stack=windows_per_stack, gate=gate, min_separation=min_separation, centre=centre), T=m.num_triples())

    def locate_set_table(self, table, n_cols=None):
        """tdoa_group_locate_set_table: the table to every member"""
        ptr, n_cells, n_cols, S = _table(table, n_cols)
        self._chk(self._L.tdoa_group_locate_set_table(self._h, ptr, n_cells, n_cols, S))
        self._locate_cells = n_cells

    def process_locate(self, windows_per_stack=0, min_separation=1, want_map=False):
        """tdoa_group_process_locate -> Context.process_locate's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate", dict(
            windows_per_stack=windows_per_stack, min_separation=min_separation, want_map=want_map))

    def locate_set_clock(self, clock):
        """tdoa_group_locate_set_clock: the station clocks to every member"""
        self._chk(self._L.tdoa_group_locate_set_clock(self._h, *_clock(clock)))

    def locate_set_stats(self, ranks, foot=0):
        """tdoa_group_locate_set_stats: Context.locate_set_stats on every member"""
        self._chk(self._L.tdoa_group_locate_set_stats(self._h, *_ranks(ranks), int(foot)))
        self._stats_on = ranks is not None and np.size(ranks) > 0

    def locate_last_stats(self):
        """tdoa_group_locate_last_stats -> Context.locate_last_stats' array, byte-identical to a single context's"""
        return _last_stats(self, self._L.tdoa_group_locate_last_stats)

    def locate_set_upsample(self, U):
        """tdoa_group_locate_set_upsample: Context.locate_set_upsample on every member"""
        self._chk(self._L.tdoa_group_locate_set_upsample(self._h, int(U)))

    def locate_set_fine_table(self, table, n_cols=None):
        """tdoa_group_locate_set_fine_table: the zoom locate's fine table to every member"""
        ptr, n_cells, n_cols, S = _table(table, n_cols)
        self._chk(self._L.tdoa_group_locate_set_fine_table(self._h, ptr, n_cells, n_cols, S))

    def process_locate_zoom(self, Z, H, windows_per_stack=0, min_separation=1, fine_separation=1, want_map=False, want_zmap=True):
        """tdoa_group_process_locate_zoom -> Context.process_locate_zoom's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate_zoom", dict(
            windows_per_stack=windows_per_stack, min_separation=min_separation, Z=Z, H=H, fine_separation=fine_separation,
            want_map=want_map, want_zmap=want_zmap))

    _with_stats = Context._with_stats

    def process_locate_track(self, windows_per_stack=0, max_step=0, min_separation=1, want_total=False):
        """tdoa_group_process_locate_track -> Context.process_locate_track's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate_track", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, min_separation=min_separation, want_total=want_total))

    def process_locate_multi(self, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, want_map=False):
        """tdoa_group_process_locate_multi -> Context.process_locate_multi's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "locate_multi", dict(
            windows_per_stack=windows_per_stack, n_emitters=n_emitters, guard=guard, min_separation=min_separation,
            want_map=want_map))

    def process_locate_track_multi(self, windows_per_stack=0, max_step=0, n_emitters=1, guard=0, min_separation=1, want_total=False):
        """tdoa_group_process_locate_track_multi -> Context.process_locate_track_multi's outputs, byte-identical to a single
        context's"""
        return _process_search(self, self.member(0), "locate_track_multi", dict(
            windows_per_stack=windows_per_stack, max_step=max_step, n_emitters=n_emitters, guard=guard,
            min_separation=min_separation, want_total=want_total))

    def process_sync(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, centre=None):
        """tdoa_group_process_sync -> Context.process_sync's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "sync", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, ref_delay=ref_delay, centre=centre))

    def process_sync_fine(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None):
        """tdoa_group_process_sync_fine -> Context.process_sync_fine's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "sync_fine", dict(
            windows_per_stack=windows_per_stack, gate=gate, rounds=rounds, U=U, fine_rounds=fine_rounds, ref_delay=ref_delay,
            centre=centre))

    def process_sync_drift(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None):
        """tdoa_group_process_sync_drift -> Context.process_sync_drift's outputs, byte-identical to a single context's"""
        return _process_search(self, self.member(0), "sync_drift", dict(
            windows_per_stack=windows_per_stack, gate=gate, max_drift=max_drift, drift_den=drift_den, rounds=rounds,
            ref_delay=ref_delay, centre=centre), n_tracks=3)


def clock_mix_rows(clock16, mix):
    """tdoa_clock_mix_rows (host only): clock16 [n][S] int32 and mix [m][4] (a, b, wa, wb) -> rows [m][S] int32, the nearest
    integer to (wa clock16[a] + wb clock16[b]) / (wa + wb), halves away from zero: tdoa_process_sync_locate's clock rows"""
    c = np.ascontiguousarray(clock16, dtype=np.int32)
    if c.ndim != 2:
        raise ValueError("clock16 must be [n][S]")
    m = np.shape(mix)[0]
    rows = _poisoned((m, c.shape[1]), np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = load().tdoa_clock_mix_rows(c.ctypes.data_as(i32p), c.shape[0], c.shape[1], _mix(mix), m, rows.ctypes.data_as(i32p))
    if rc != 0:
        raise TdoaError(rc, "tdoa_clock_mix_rows")
    return rows


def line_mix_rows(clock16, fine_rate, U, drift_den, mix):
    """tdoa_line_mix_rows (host only): clock16, fine_rate [n_lines][S] int32 and mix [m][6] (a, xa, b, xb, wa, wb) -> rows [m][S]
    int32: line a continued to xa and line b to xb by tdoa_sync_line_clock16's rule (x of either sign), then tdoa_clock_mix_rows'
    mean by wa, wb: tdoa_process_sync_drift_locate's clock rows"""
    c, h = _line_words(clock16, fine_rate)
    m = np.shape(mix)[0]
    rows = _poisoned((m, c.shape[1]), np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = load().tdoa_line_mix_rows(c.ctypes.data_as(i32p), h.ctypes.data_as(i32p), c.shape[0], c.shape[1], int(U), int(drift_den),
                                   _mix(mix, width=6), m, rows.ctypes.data_as(i32p))
    if rc != 0:
        raise TdoaError(rc, "tdoa_line_mix_rows")
    return rows


def sync_line_clock16(clock16, fine_rate, U, drift_den, first_position, n_positions):
    """tdoa_sync_line_clock16 (host only): a fine line's clocks [S] (1/16 sample) and fine rates [S] continued over positions
    first_position .. first_position + n_positions - 1 -> [n_positions][S] int32 in 1/16 sample, what locate_set_clock takes"""
    k = np.ascontiguousarray(clock16, dtype=np.int32).reshape(-1)
    h = np.ascontiguousarray(fine_rate, dtype=np.int32).reshape(-1)
    if k.shape != h.shape:
        raise ValueError("clock16 and fine_rate must hold one integer per station")
    out = np.zeros((max(int(n_positions), 1), k.shape[0]), dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = load().tdoa_sync_line_clock16(k.ctypes.data_as(i32p), h.ctypes.data_as(i32p), k.shape[0], int(U), int(drift_den),
                                       int(first_position), int(n_positions), out.ctypes.data_as(i32p))
    if rc:
        raise TdoaError(rc, "tdoa_sync_line_clock16")
    return out


def sync_line_clock(clock, rate, drift_den, first_position, n_positions):
    """tdoa_sync_line_clock (host only): a line's clocks [S] (samples) and rates [S] continued over positions first_position
    .. first_position + n_positions - 1 -> [n_positions][S] int32 in units of 1/16 sample, what locate_set_clock takes"""
    k = np.ascontiguousarray(clock, dtype=np.int32).reshape(-1)
    h = np.ascontiguousarray(rate, dtype=np.int32).reshape(-1)
    if k.shape != h.shape:
        raise ValueError("clock and rate must hold one integer per station")
    out = np.zeros((max(int(n_positions), 1), k.shape[0]), dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = load().tdoa_sync_line_clock(k.ctypes.data_as(i32p), h.ctypes.data_as(i32p), k.shape[0], int(drift_den), int(first_position),
                                     int(n_positions), out.ctypes.data_as(i32p))
    if rc != 0:
        raise TdoaError(rc, "tdoa_sync_line_clock")
    return out


def locate_upsample_taps(U):
    """tdoa_locate_upsample_taps (host only) -> [U][16] int32: the taps of the U phases at scale 2^15"""
    taps = np.zeros((max(int(U), 1), 16), dtype=np.int32)
    rc = load().tdoa_locate_upsample_taps(int(U), taps.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        raise TdoaError(rc, "tdoa_locate_upsample_taps")
    return taps


def locate_grid_table(stations_lle, lat0, lon0, dlat, dlon, rows, cols, height_m, sample_rate):
    """tdoa_locate_grid_table (host only): the delay table [rows cols][n_stations] int32 of a latitude / longitude grid"""
    st = np.ascontiguousarray(stations_lle, dtype=np.float64).reshape(-1, 3)
    rows, cols = int(rows), int(cols)
    n_cells = rows * cols if rows >= 1 and cols >= 1 and rows * cols <= 2 ** 22 else 1      # (the library refuses the rest)
    out = np.zeros((n_cells, st.shape[0]), dtype=np.int32)
    rc = load().tdoa_locate_grid_table(_d(st.reshape(-1)), st.shape[0], float(lat0), float(lon0), float(dlat), float(dlon), rows,
                                       cols, float(height_m), float(sample_rate), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != OK:
        raise TdoaError(rc, "tdoa_locate_grid_table")
    return out


def latlon_to_ecef(lat, lon, elev):
    out = np.zeros(3)
    load().tdoa_latlon_to_ecef(lat, lon, elev, _d(out))
    return out


def ecef_to_latlon(x, y, z):
    out = np.zeros(3)
    load().tdoa_ecef_to_latlon(x, y, z, _d(out))
    return out


def solve_3station(stations_lle, range_diff):
    st = np.ascontiguousarray(stations_lle, dtype=np.float64).reshape(9)
    rd = np.ascontiguousarray(range_diff, dtype=np.float64)
    out = np.zeros(3)
    it = C.c_int()
    rc = load().tdoa_solve_3station(_d(st), _d(rd), _d(out), C.byref(it))
    return rc, out, it.value


def segment_quads(n_stations, pairs):
    """host only: the quad cover the segment form uses for a window's (template, signal) station pairs;
    returns rows [a, b, c, d, pair(a,c), pair(a,d), pair(b,c), pair(b,d)] (-1 = empty / not wanted)"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = np.full((max(len(pr), 1), 8), -2, dtype=np.int32)
    n = load().tdoa_debug_segment_quads(int(n_stations), pr.ctypes.data_as(C.POINTER(C.c_int32)), len(pr),
                                        out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    if n < 0:
        raise ValueError("tdoa_debug_segment_quads: error %d" % -n)
    return out[:n]


def staged_groups(n_stations, max_pairs=15):
    """host only: the staged column walk's share-out of a window's pairs to workgroups: a list of (station mask, [pair numbers])"""
    masks = np.zeros(128, dtype=np.uint32)
    counts = np.zeros(128, dtype=np.int32)
    pairs = np.zeros((128, 16), dtype=np.uint8)
    n = load().tdoa_debug_staged_groups(int(n_stations), int(max_pairs), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        counts.ctypes.data_as(C.POINTER(C.c_int32)), pairs.ctypes.data_as(C.POINTER(C.c_uint8)), 128)
    if n < 0:
        raise ValueError("tdoa_debug_staged_groups: error %d" % -n)
    return [(int(masks[g]), [int(x) for x in pairs[g, :counts[g]]]) for g in range(n)]


def stg_paired_index(n2, row, col):
    """host only: the element index of (row, col) in the staged walk's paired block layout of a 4096 x n2 spectrum"""
    i = load().tdoa_debug_stg_paired_index(int(n2), int(row), int(col))
    if i < 0:
        raise ValueError("tdoa_debug_stg_paired_index: n2 is 256 or 512, row in [0, n2), col in [0, 4096)")
    return int(i)


def k1_split_table():
    """host only: the fused column kernels' split half-plane angle table, (hi uint16[32768], lo uint8[32768])"""
    hi = np.zeros(32768, dtype=np.uint16)
    lo = np.zeros(32768, dtype=np.uint8)
    rc = load().tdoa_debug_k1_split_table(hi.ctypes.data_as(C.POINTER(C.c_uint16)), _u8(lo))
    if rc:
        raise ValueError("tdoa_debug_k1_split_table: error %d" % rc)
    return hi, lo


def solve_nstation(stations_lle, range_diff, weights=None, solve_z=False):
    st = np.ascontiguousarray(stations_lle, dtype=np.float64)
    n = st.size // 3
    rd = np.ascontiguousarray(range_diff, dtype=np.float64)
    wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    out = np.zeros(3)
    it = C.c_int()
    rc = load().tdoa_solve_nstation(_d(st.reshape(-1)), n, _d(rd), _d(wt) if wt is not None else None,
                                    1 if solve_z else 0, _d(out), C.byref(it))
    return rc, out, it.value


def solve_surface(stations_lle, range_diff, weights=None, height_m=0.0):
    """tdoa_solve_surface: least-squares fix on the ellipsoid at `height_m` -> (status, lle, iterations)"""
    st = np.ascontiguousarray(stations_lle, dtype=np.float64)
    n = st.size // 3
    rd = np.ascontiguousarray(range_diff, dtype=np.float64)
    wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    out = np.zeros(3)
    it = C.c_int()
    rc = load().tdoa_solve_surface(_d(st.reshape(-1)), n, _d(rd), _d(wt) if wt is not None else None, float(height_m),
                                   _d(out), C.byref(it))
    return rc, out, it.value


def owned_runs(total_samples, n_min, window_len, rank, world):
    """host only: [(first_sample, n_samples)] a group member `rank` of `world` uploads of a capture of total_samples
    (tdoa_debug_owned_runs; the C++ form of sharding.owned_sample_runs)"""
    L = load()
    args = (int(total_samples), int(n_min), int(window_len), int(rank), int(world))
    n = C.c_int(0)
    rc = L.tdoa_debug_owned_runs(*args, None, None, 0, C.byref(n))          # the count first
    first, count = (C.c_size_t * max(n.value, 1))(), (C.c_size_t * max(n.value, 1))()
    if rc == OK:
        rc = L.tdoa_debug_owned_runs(*args, first, count, n.value, C.byref(n))
    if rc != OK:
        raise ValueError("tdoa_debug_owned_runs: error %d" % rc)
    return [(first[i], count[i]) for i in range(n.value)]


def step_layout(n_stations, n_windows, rank, world, max_per_batch=2**31 - 1):
    """host only: what tdoa_process(rank, world) runs, as tdoa_debug_step_layout lays it out -- (pair-windows, quads):
    rows [unit, group, slot a, slot b, station of slot a, station of slot b] in launch order, and
    rows [group, slot a, slot b, slot c, slot d, pw(a,c), pw(a,d), pw(b,c), pw(b,d)] with group-relative indices"""
    n_pairs = n_stations * (n_stations - 1) // 2
    cap = max(n_windows * n_pairs, 1)
    pw = np.zeros((cap, 6), dtype=np.int32)
    quads = np.zeros((cap, 9), dtype=np.int32)
    nq = C.c_int32(0)
    n = load().tdoa_debug_step_layout(int(n_stations), int(n_windows), int(rank), int(world), int(max_per_batch),
                                      pw.ctypes.data_as(C.POINTER(C.c_int32)), cap,
                                      quads.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nq))
    if n < 0:
        raise ValueError("tdoa_debug_step_layout: error %d" % -n)
    return pw[:n], quads[:nq.value]
