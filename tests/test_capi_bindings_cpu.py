"""The ctypes binding against include/tdoa_mi355x.h, without a device: every argtypes list has the prototype's length; the
stack searches' table (capi.SEARCHES) states the header's parameter order and types for all 27 entries; the public methods put
every value into its slot and every output behind its pointer (a recording stand-in takes the library's place); and no public
signature of Context or Group has changed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def _prototypes():
    """{function: [(C type, parameter name)]} of every prototype in the header"""
    text = open(os.path.join(ROOT, "include", "tdoa_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for name, params in re.findall(r"\b(tdoa_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in (x.strip() for x in params.split(",")):
            if p in ("", "void"):
                continue
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[\w*\])?", p, flags=re.S)          # (an array parameter is a pointer)
            ctype = " ".join((m.group(1) + ("*" if m.group(3) else "")).replace("const", " ").replace("*", " * ").split())
            plist.append((ctype, m.group(2)))
        assert name not in out, name
        out[name] = plist
    return out


# ---- 1. arity ---------------------------------------------------------------------------------------------------------------
def test_every_argtypes_list_has_the_prototypes_length(capi):
    lib, protos = capi.load(), _prototypes()
    assert sorted(protos) == sorted(capi.SYMBOLS)
    checked = 0
    for name, params in protos.items():
        argtypes = getattr(lib, name).argtypes
        if argtypes is None:
            assert name in ("tdoa_abi_version", "tdoa_device_count") and not params, name
            continue
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        checked += 1
    assert checked >= 115


# ---- 2. the searches' order and types -----------------------------------------------------------------------------------------
C_TYPES = {"int": C.c_int, "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double), "int64_t *": C.POINTER(C.c_int64)}
SCALARS = {"int32_t *": np.int32, "double *": np.float64, "int64_t *": np.int64}


def test_the_search_table_states_the_headers_order_and_types(capi):
    lib, protos = capi.load(), _prototypes()
    records = {"tdoa_closure *": capi.CLOSURE_DTYPE, "tdoa_location *": capi.LOCATION_DTYPE, "tdoa_zoom *": capi.ZOOM_DTYPE,
               "tdoa_sync *": capi.SYNC_DTYPE, "tdoa_sync_line *": capi.SYNC_LINE_DTYPE, "tdoa_cell_track *": capi.CELL_TRACK_DTYPE}
    assert sorted(capi.SEARCHES) == ["closure", "locate", "locate_multi", "locate_track", "locate_track_multi", "locate_zoom",
                                     "sync", "sync_drift", "sync_fine"]
    checked = 0
    for s in capi.SEARCHES.values():
        assert s.entries == {"own": "tdoa_process_" + s.name, "group": "tdoa_group_process_" + s.name,
                             "q": "tdoa_debug_%s_from_q" % s.name}
        for route, entry in s.entries.items():
            if route == "q":
                names = ["ctx", "q", "n_sets"] + (["track_len"] if s.track_len else []) + ["n_stations", "n_w"]
            else:
                names = ["ctx" if route == "own" else "g", "windows_per_stack"]
            names += list(s.ints) + list(s.inputs)
            names += [("out" if s.name == "closure" else o.key) if route == "q" else o.key + "_host" for o in s.outputs]
            assert [n for _, n in protos[entry]] == names, entry
            argtypes = getattr(lib, entry).argtypes
            assert len(argtypes) == len(names), entry
            first_out = len(names) - len(s.outputs)
            for k, ((ctype, name), argtype) in enumerate(zip(protos[entry], argtypes)):
                if k == 0:
                    assert ctype == ("tdoa_group *" if route == "group" else "tdoa_ctx *") and argtype is C.c_void_p, entry
                elif ctype in C_TYPES:
                    assert argtype is C_TYPES[ctype], (entry, name)
                else:
                    assert ctype in records and argtype is C.c_void_p, (entry, name, ctype)
                if k >= first_out:                       # the array behind the pointer has the pointee's type
                    dtype = np.dtype(s.outputs[k - first_out].dtype)
                    assert dtype == (records[ctype] if ctype in records else np.dtype(SCALARS[ctype])), (entry, name)
                elif k >= first_out - len(s.inputs):
                    assert ctype == "int32_t *", (entry, name)
                elif name != "q" and k > 0:
                    assert ctype == "int", (entry, name)
            checked += 1
    assert checked == 27


# ---- 3. the values reach their slots ------------------------------------------------------------------------------------------
N, S, P, CELLS, K, L, H, MAX_LAG = 15, 4, 6, 7, 2, 3, 1, 8    # sets or stacks, stations, pairs, table cells, rounds, track length
TRIPLES_OWN = 11                                             # what the stand-in's tdoa_num_triples answers (from-Q: S C 3 = 4)
HANDLE, GROUP_HANDLE, MEMBER_HANDLE = 0x1110, 0x2220, 0x3330
INTS = {"gate": 21, "min_separation": 22, "rounds": 23, "U": 24, "fine_rounds": 25, "max_drift": 26, "drift_den": 27,
        "max_step": 28, "guard": 29, "Z": 30, "fine_separation": 31, "n_emitters": K, "H": H}
WPS, N_W = 33, 34
REF_DELAY, CENTRE = [160, -32, 48, 7], [3, -4, 5, -6]


class StandIn:
    """takes the library's place: answers the counts, records every other call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            if name == "tdoa_num_stacks":
                args[2]._obj.value, args[3]._obj.value = L, N
            elif name == "tdoa_num_pairs":
                return P
            elif name == "tdoa_num_triples":
                return TRIPLES_OWN
            elif name == "tdoa_group_member":
                return MEMBER_HANDLE
            elif name not in ("tdoa_destroy", "tdoa_group_destroy"):
                self.calls.append((name, args))
            return 0
        return fn


def _owner(capi, cls, handle):
    o = object.__new__(cls)
    o._L, o._h, o._locate_cells = StandIn(), C.c_void_p(handle), CELLS
    o.params = capi.Params(max_lag=MAX_LAG)
    return o


def _stated(capi, name, route, k=K, h=H, track_len=L):
    """{key: (dtype, shape)} as the methods' docstrings state them"""
    i32, f64, i64 = np.int32, np.float64, np.int64
    tracks = max(N // track_len, 1)
    lines = tracks if route == "q" else 3
    loc = {"loc": (capi.LOCATION_DTYPE, (N,)), "lags": (i32, (N, P)), "corr": (f64, (N, P)), "map": (i64, (N, CELLS))}
    track = {"track": (capi.CELL_TRACK_DTYPE, (tracks,)), "cells": (i32, (tracks, track_len)), "own": (i64, (tracks, track_len)),
             "lags": (i32, (N, P)), "corr": (f64, (N, P)), "total": (i64, (tracks, CELLS))}
    sync = {"sync": (capi.SYNC_DTYPE, (N,)), "clock": (i32, (N, S)), "lags": (i32, (N, P)), "corr": (f64, (N, P))}
    if name == "closure":
        return {"closure": (capi.CLOSURE_DTYPE, (N, 4 if route == "q" else TRIPLES_OWN))}
    if name == "locate":
        return loc
    if name == "locate_multi":
        return {key: (d, (k,) + shape) for key, (d, shape) in loc.items()}
    if name == "locate_track":
        return track
    if name == "locate_track_multi":
        track = dict(list(track.items())[:3] + [("pairs", (i32, (N, 2)))] + list(track.items())[3:])
        return {key: (d, (k,) + shape) for key, (d, shape) in track.items()}
    if name == "locate_zoom":
        return dict(loc, zoom=(capi.ZOOM_DTYPE, (N,)), zlags=(i32, (N, P)), zcorr=(f64, (N, P)), zmap=(i64, (N, (2 * h + 1) ** 2)))
    if name == "sync":
        return sync
    if name == "sync_fine":
        return dict(sync, fine=(capi.SYNC_DTYPE, (N,)), clock16=(i32, (N, S)), fine_lags=(i32, (N, P)), fine_corr=(f64, (N, P)))
    assert name == "sync_drift"
    return {"line": (capi.SYNC_LINE_DTYPE, (lines,)), "clock": (i32, (lines, S)), "rate": (i32, (lines, S)), "rows": (i32, (N, S)),
            "lags": (i32, (N, P)), "corr": (f64, (N, P))}


HEADER_INTS = {"closure": ["gate", "min_separation"], "locate": ["min_separation"],
               "locate_multi": ["n_emitters", "guard", "min_separation"], "locate_track": ["max_step", "min_separation"],
               "locate_track_multi": ["max_step", "n_emitters", "guard", "min_separation"],
               "locate_zoom": ["min_separation", "Z", "H", "fine_separation"], "sync": ["gate", "rounds"],
               "sync_fine": ["gate", "rounds", "U", "fine_rounds"], "sync_drift": ["gate", "max_drift", "drift_den", "rounds"]}
TRACKED = ("locate_track", "locate_track_multi", "sync_drift")
CLOCKED = ("sync", "sync_fine", "sync_drift")
OPTIONAL = {"map": "want_map", "zmap": "want_zmap", "total": "want_total"}
POISONED = ("zoom", "zlags", "zcorr", "zmap")


def _address(p):
    return p.value if isinstance(p, C.c_void_p) else C.cast(p, C.c_void_p).value


def _call(capi, name, route, ints=INTS, track_len=L, centre=CENTRE, **wants):
    """search `name` through `route` on a stand-in -> (the method's result, the recorded call's arguments, the q it was given)"""
    owner = _owner(capi, capi.Group if route == "group" else capi.Context, GROUP_HANDLE if route == "group" else HANDLE)
    kw = {k: ints[k] for k in HEADER_INTS[name]}
    kw.update(wants)
    if name == "closure" or name in CLOCKED:
        kw["centre"] = centre
    q = None
    if route == "q":
        q = np.arange(N * P * (2 * MAX_LAG - 1), dtype=np.int64).reshape(N, P, 2 * MAX_LAG - 1)
        args = (q, REF_DELAY if name in CLOCKED else S) + ((track_len,) if name in TRACKED else ())
        result = getattr(owner, name + "_from_q")(*args, n_w=N_W, **kw)
    else:
        args = (REF_DELAY,) if name in CLOCKED else ()
        result = getattr(owner, "process_" + name)(*args, windows_per_stack=WPS, **kw)
    (entry, recorded), = owner._L.calls
    assert entry == {"own": "tdoa_process_", "group": "tdoa_group_process_", "q": "tdoa_debug_"}[route] + name + ("_from_q" if route == "q" else "")
    return result, list(recorded), q


def _check(capi, name, route, result, recorded, q, stated, ints=INTS, track_len=L, centre=CENTRE, absent=()):
    handle = recorded.pop(0)
    assert handle.value == (GROUP_HANDLE if route == "group" else HANDLE)
    if route == "q":
        assert _address(recorded.pop(0)) == q.ctypes.data
        head = [N] + ([track_len] if name in TRACKED else []) + [S, N_W]
    else:
        head = [WPS]
    head += [ints[k] for k in HEADER_INTS[name]]
    assert recorded[:len(head)] == head, (name, route)
    del recorded[:len(head)]
    if name in CLOCKED:
        assert np.ctypeslib.as_array(recorded.pop(0), shape=(S,)).tolist() == REF_DELAY
    if name == "closure" or name in CLOCKED:
        c = recorded.pop(0)
        assert c is None if centre is None else np.ctypeslib.as_array(c, shape=(S,)).tolist() == centre
    arrays = {"closure": result} if name == "closure" else result
    assert isinstance(arrays, dict) and "stats" not in arrays
    assert list(arrays) == [key for key in stated if key not in absent]
    assert len(recorded) == len(stated), (name, route)
    for (key, (dtype, shape)), pointer in zip(stated.items(), recorded):
        if key in absent:
            assert pointer is None, key
            continue
        a = arrays[key]
        assert a.dtype == dtype and a.shape == shape and a.flags.c_contiguous, (name, route, key, a.shape, shape)
        assert _address(pointer) == a.ctypes.data, key
        assert set(a.tobytes()) <= {0xA5 if key in POISONED else 0}, key          # the stand-in wrote nothing


@pytest.mark.parametrize("route", ["own", "group", "q"])
@pytest.mark.parametrize("name", sorted(HEADER_INTS))
def test_values_and_outputs_reach_their_slots(capi, name, route):
    assert len(set(INTS.values()) | {WPS, N_W, N, S, L}) == len(INTS) + 5                # no two slots can be confused
    stated = _stated(capi, name, route)
    wants = {flag: True for key, flag in OPTIONAL.items() if key in stated}
    result, recorded, q = _call(capi, name, route, **wants)
    _check(capi, name, route, result, recorded, q, stated)
    if wants or name == "closure" or name in CLOCKED:         # every optional output off, and no centre
        off = {flag: False for flag in wants}
        result, recorded, q = _call(capi, name, route, centre=None, **off)
        _check(capi, name, route, result, recorded, q, stated, centre=None, absent=[k for k, f in OPTIONAL.items() if f in off])


def test_the_flags_defaults(capi):
    """want_map and want_total: off on the own and group routes, on from Q; want_zmap: on everywhere"""
    for name, key in (("locate", "map"), ("locate_multi", "map"), ("locate_zoom", "map"), ("locate_track", "total"),
                      ("locate_track_multi", "total")):
        for route in ("own", "group", "q"):
            result, recorded, _ = _call(capi, name, route)
            assert (key in result) == (route == "q"), (name, route)
            assert ("zmap" in result) == (name == "locate_zoom")
            assert (recorded[-1] is None) == (route != "q" and name != "locate_zoom")


@pytest.mark.parametrize("route", ["own", "group", "q"])
def test_a_refused_count_is_passed_on_and_the_arrays_still_exist(capi, route):
    for n_emitters, k in ((0, 1), (9, 8)):
        ints = dict(INTS, n_emitters=n_emitters)
        for name in ("locate_multi", "locate_track_multi"):
            want = {"locate_multi": "want_map", "locate_track_multi": "want_total"}[name]
            result, recorded, q = _call(capi, name, route, ints=ints, **{want: True})
            _check(capi, name, route, result, recorded, q, _stated(capi, name, route, k=k), ints=ints)
    for h, clamped in ((-1, 0), (65, 64)):
        ints = dict(INTS, H=h)
        result, recorded, q = _call(capi, "locate_zoom", route, ints=ints, want_map=True)
        _check(capi, "locate_zoom", route, result, recorded, q, _stated(capi, "locate_zoom", route, h=clamped), ints=ints)
    if route == "q":
        for name in TRACKED:
            want = {} if name == "sync_drift" else {"want_total": True}
            result, recorded, q = _call(capi, name, route, track_len=0, **want)
            _check(capi, name, route, result, recorded, q, _stated(capi, name, route, track_len=1), track_len=0)


def test_the_driver_needs_no_library_and_q_is_normalised_once(capi):
    s = capi.SEARCHES["sync"]
    seen, status = [], []
    values = dict(n_w=1, gate=2, rounds=3, ref_delay=[0, 16, 32], centre=None)
    q = capi._q_sets(np.zeros((3, 5), dtype=np.int32), 3, 3)                      # one set, promoted and converted
    assert q.shape == (1, 3, 5) and q.dtype == np.int64 and q.flags.c_contiguous
    out = capi._run_search(s, "q", lambda *a: seen.append(a) or 17, None, status.append, capi._shape_numbers(values, 1, 3), values, q)
    assert status == [17] and seen[0][1:6] == (seen[0][1], 1, 3, 1, 2) and sorted(out) == ["clock", "corr", "lags", "sync"]
    for bad, n_stations in ((np.zeros((1, 3, 4)), 3), (np.zeros((1, 2, 5)), 3), (np.zeros(5), 3), (np.zeros((1, 1, 3, 5)), 3)):
        with pytest.raises(ValueError, match=re.escape("q must be [n_sets][S (S-1) / 2][2 max_lag - 1]")):
            capi._q_sets(bad, n_stations, 3)
    owner = _owner(capi, capi.Context, HANDLE)
    for method, args in ((owner.locate_from_q, (np.zeros((1, 3, 4)), 3)), (owner.sync_from_q, (np.zeros((1, 6, 15)), [0, 1, 2]))):
        with pytest.raises(ValueError, match="q must be"):
            method(*args)
    good = np.zeros((1, 6, 15), dtype=np.int64)
    with pytest.raises(ValueError, match="centre must hold one integer per station"):
        owner.closure_from_q(good, 4, centre=[1, 2, 3])
    with pytest.raises(ValueError, match="centre must hold one integer per station"):
        owner.process_sync(REF_DELAY, centre=[1, 2, 3])
    with pytest.raises(ValueError, match="ref_delay must hold one delay per station"):
        owner.process_sync_fine([1, 2, 3])
    assert owner._L.calls == []                              # nothing reached the library


# ---- 4. the public signatures, as the parent commit had them --------------------------------------------------------------------
CONTEXT_SIGNATURES = [
    ("capture_attach_device", "(self, station, dev_ptr, n_samples)"),
    ("capture_clear", "(self)"),
    ("capture_download", "(self, station, first_sample, n_samples)"),
    ("capture_upload", "(self, station, iq_u8)"),
    ("capture_upload_file", "(self, station, path)"),
    ("capture_upload_owned", "(self, station, iq_u8, rank, world, window_len)"),
    ("capture_upload_range", "(self, station, total_samples, first_sample, iq_u8)"),
    ("close", "(self)"),
    ("closure_from_q", "(self, q, n_stations, n_w=1, gate=0, min_separation=1, centre=None)"),
    ("cross_correlate", "(self, s1, s2)"),
    ("cross_correlate_batch", "(self, signals)"),
    ("debug_flags", "(self, generic=False, no_short_lag=False, no_fused_k1=False, no_segment_form=False, no_xcd_rows=False, no_segment_quads=False, no_decimate=False, no_k1_once=False, no_seg_pack3=False, no_dec_cols=False, dec_cols_always=False, pow2_only=False, no_dec_staged=False, no_small_fused=False, small_fused_always=False)"),
    ("debug_select_peaks", "(self, surface, lag_lo, k, min_separation)"),
    ("fast_analyze", "(self, samples_u8, total_samples)"),
    ("fast_analyze_capture", "(self, raw_u8)"),
    ("fast_snr", "(self, samples_u8, total_samples)"),
    ("fm_preprocess", "(self, iq)"),
    ("fm_stats", "(self, iq)"),
    ("fm_xcorr", "(self, iq1, iq2, max_lag)"),
    ("fm_xcorr_fine", "(self, iq1, iq2, max_lag, gate_samples)"),
    ("fm_xcorr_lags", "(self, iq1, iq2, max_lag)"),
    ("fm_xcorr_peaks", "(self, iq1, iq2, max_lag, k, min_separation)"),
    ("force_generic", "(self, on=True)"),
    ("graph_info", "(self, dot_path=None)"),
    ("last_k1", "(self, sw_index=0)"),
    ("last_route", "(self)"),
    ("load_iq_u8", "(self, raw)"),
    ("locate_from_q", "(self, q, n_stations, n_w=1, min_separation=1, want_map=True)"),
    ("locate_last_stats", "(self)"),
    ("locate_multi_from_q", "(self, q, n_stations, n_w=1, n_emitters=1, guard=0, min_separation=1, want_map=True)"),
    ("locate_set_clock", "(self, clock)"),
    ("locate_set_fine_table", "(self, table, n_cols=None)"),
    ("locate_set_stats", "(self, ranks, foot=0)"),
    ("locate_set_table", "(self, table, n_cols=None)"),
    ("locate_set_upsample", "(self, U)"),
    ("locate_track_from_q", "(self, q, n_stations, track_len, n_w=1, max_step=0, min_separation=1, want_total=True)"),
    ("locate_track_multi_from_q", "(self, q, n_stations, track_len, n_w=1, max_step=0, n_emitters=1, guard=0, min_separation=1, want_total=True)"),
    ("locate_zoom_from_q", "(self, q, n_stations, Z, H, n_w=1, min_separation=1, fine_separation=1, want_map=True, want_zmap=True)"),
    ("num_pairs", "(self)"),
    ("num_stacks", "(self, windows_per_stack=0)"),
    ("num_stations", "(self)"),
    ("num_triples", "(self)"),
    ("num_windows", "(self)"),
    ("plan_info", "(self)"),
    ("poison_workspace", "(self)"),
    ("preprocess", "(self, sig)"),
    ("process", "(self, rank=0, world=1, out_dev_ptr=None, want_host=True)"),
    ("process_closure", "(self, windows_per_stack=0, gate=0, min_separation=1, centre=None)"),
    ("process_fine", "(self, gate_samples, rank=0, world=1)"),
    ("process_lags", "(self, rank=0, world=1, out_dev_ptr=None, want_host=True)"),
    ("process_locate", "(self, windows_per_stack=0, min_separation=1, want_map=False)"),
    ("process_locate_multi", "(self, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, want_map=False)"),
    ("process_locate_track", "(self, windows_per_stack=0, max_step=0, min_separation=1, want_total=False)"),
    ("process_locate_track_multi", "(self, windows_per_stack=0, max_step=0, n_emitters=1, guard=0, min_separation=1, want_total=False)"),
    ("process_locate_zoom", "(self, Z, H, windows_per_stack=0, min_separation=1, fine_separation=1, want_map=False, want_zmap=True)"),
    ("process_peaks", "(self, k, min_separation, rank=0, world=1)"),
    ("process_stacked", "(self, windows_per_stack=0, k=1, min_separation=1, gate=None, rank=0, world=1, want_surface=False, want_partial=False)"),
    ("process_stacked_drift", "(self, windows_per_stack=0, max_drift=0, drift_den=1, k=1, min_separation=1, gate=None, want_surface=False, want_partial=False, want_profile=True)"),
    ("process_sync", "(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, centre=None)"),
    ("process_sync_drift", "(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None)"),
    ("process_sync_fine", "(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None)"),
    ("process_track", "(self, windows_per_stack=0, max_step=1, want_surface=False, want_total=False)"),
    ("process_u8", "(self, captures)"),
    ("profile", "(self)"),
    ("profile_enable", "(self, on=True)"),
    ("profile_reset", "(self)"),
    ("profile_select", "(self, names=None)"),
    ("simple_correlate", "(self, s1, s2)"),
    ("sync_drift_from_q", "(self, q, ref_delay, track_len, n_w=1, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None)"),
    ("sync_fine_from_q", "(self, q, ref_delay, n_w=1, gate=0, rounds=0, U=16, fine_rounds=2, centre=None)"),
    ("sync_from_q", "(self, q, ref_delay, n_w=1, gate=0, rounds=0, centre=None)"),
    ("synth_capture", "(self, station, block_samples, station_lle, tx_lle, seed, ref_freq=162400000.0, tgt_freq=101700000.0, noise=0.01, tx_power=1000.0)"),
    ("synth_weak_capture", "(self, station, block_samples, station_lle, tx_lle, seed, ref_freq=162400000.0, tgt_freq=92300000.0, ref_power=10.0, tgt_power=1000.0)"),
    ("time_domain_correlation", "(self, s1, s2, max_lag)"),
    ("upsample_q", "(self, q, U)"),
    ("window_quality", "(self, iq_u8)"),
    ("window_quality_all", "(self, rank=0, world=1)"),
]
GROUP_SIGNATURES = [
    ("capture_upload_files", "(self, paths)"),
    ("close", "(self)"),
    ("locate_last_stats", "(self)"),
    ("locate_set_clock", "(self, clock)"),
    ("locate_set_fine_table", "(self, table, n_cols=None)"),
    ("locate_set_stats", "(self, ranks, foot=0)"),
    ("locate_set_table", "(self, table, n_cols=None)"),
    ("locate_set_upsample", "(self, U)"),
    ("member", "(self, k)"),
    ("process", "(self, out=None)"),
    ("process_closure", "(self, windows_per_stack=0, gate=0, min_separation=1, centre=None)"),
    ("process_locate", "(self, windows_per_stack=0, min_separation=1, want_map=False)"),
    ("process_locate_multi", "(self, windows_per_stack=0, n_emitters=1, guard=0, min_separation=1, want_map=False)"),
    ("process_locate_track", "(self, windows_per_stack=0, max_step=0, min_separation=1, want_total=False)"),
    ("process_locate_track_multi", "(self, windows_per_stack=0, max_step=0, n_emitters=1, guard=0, min_separation=1, want_total=False)"),
    ("process_locate_zoom", "(self, Z, H, windows_per_stack=0, min_separation=1, fine_separation=1, want_map=False, want_zmap=True)"),
    ("process_stacked", "(self, windows_per_stack=0, k=1, min_separation=1, gate=None, want_surface=False)"),
    ("process_sync", "(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, centre=None)"),
    ("process_sync_drift", "(self, ref_delay, windows_per_stack=0, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None)"),
    ("process_sync_fine", "(self, ref_delay, windows_per_stack=0, gate=0, rounds=0, U=16, fine_rounds=2, centre=None)"),
]


def test_no_public_signature_changed(capi):
    for cls, stated in ((capi.Context, CONTEXT_SIGNATURES), (capi.Group, GROUP_SIGNATURES)):
        found = [(name, str(inspect.signature(f))) for name, f in sorted(vars(cls).items())
                 if not name.startswith("_") and inspect.isfunction(f)]
        assert found == stated
        for s in capi.SEARCHES:                              # explicit defs, each with its docstring
            for name in ["process_" + s] + ([s + "_from_q"] if cls is capi.Context else []):
                f = vars(cls)[name]
                assert inspect.isfunction(f) and f.__doc__ and f.__qualname__ == "%s.%s" % (cls.__name__, name), name
