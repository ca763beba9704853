"""Bindings of the in-tree HIP library ``libwgrt.so`` (C ABI: ``include/wgrt.h``).

The scene, ray-setup and diagnostic entry points are bound with ctypes; the trace launch goes
through the PyTorch-ROCm operator ``torch.ops.wgrt.trace`` (``_wgrt_torch.so``, built from
csrc/wgrt_torch.cpp: ``ops()``), which forwards device tensors to ``wgrt_trace_opts`` of the same
loaded library.  There is no CPU fallback: if either library is missing or cannot be loaded,
every entry point raises ``WgrtError``.
"""
from __future__ import annotations

import ctypes
import os
import types

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libwgrt.so")   # the in-tree build, the only one the product binds
OPS_PATH = os.path.join(PKG, "_wgrt_torch.so")   # the torch operator library (csrc/wgrt_torch.cpp)

ABI_VERSION = 9
# include/wgrt.h (the drop-in boundary) and include/wgrt_debug.h (test / profiling hooks)
EXPORTED = ("wgrt_scene_create", "wgrt_scene_create_ex", "wgrt_scene_destroy", "wgrt_scene_get_info",
            "wgrt_trace_fullcolor", "wgrt_trace_fullcolor_ex", "wgrt_trace_single", "wgrt_trace_single_ex",
            "wgrt_trace_opts", "wgrt_scene_reserve", "wgrt_rays_init", "wgrt_scene_classify",
            "wgrt_locator_classify_host", "wgrt_locator_palette_host", "wgrt_selftest_math", "wgrt_status_string", "wgrt_last_error",
            "wgrt_abi_version", "wgrt_eyebox_payload_floats", "wgrt_eyebox_pack", "wgrt_eyebox_assemble",
            "wgrt_eyebox_window_sums", "wgrt_eyebox_evaluate_workspace_bytes", "wgrt_eyebox_evaluate",
            "wgrt_eyebox_evaluate_host", "wgrt_window_plan_create", "wgrt_window_plan_destroy",
            "wgrt_window_plan_width", "wgrt_trace_windows", "wgrt_window_plan_validate", "wgrt_window_table_host",
            "wgrt_chain_begin", "wgrt_chain_step", "wgrt_chain_end", "wgrt_chain_gather", "wgrt_trace_fate", "wgrt_fate_census",
            "wgrt_fate_census_host", "wgrt_fate_col", "wgrt_fate_cols", "wgrt_fate_reason_name", "wgrt_trace_replicas",
            "wgrt_window_replicas_fold", "wgrt_window_replicas_fold_host", "wgrt_trace_expected",
            "wgrt_expected_weight_host", "wgrt_trace_footprint", "wgrt_footprint_plan_validate",
            "wgrt_footprint_bin_host", "wgrt_footprint_channel_name", "wgrt_trace_hits", "wgrt_hit_bytes",
            "wgrt_hits_grid", "wgrt_hits_grid_host", "wgrt_trace_paths", "wgrt_path_vertex_bytes",
            "wgrt_paths_footprint", "wgrt_paths_footprint_host", "wgrt_trace_visits", "wgrt_visit_channels",
            "wgrt_visits_sensitivity", "wgrt_visits_reweight", "wgrt_visits_sensitivity_host",
            "wgrt_visits_reweight_host", "wgrt_visit_channel_host", "wgrt_visit_channel_count_host",
            "wgrt_trace_stokes", "wgrt_stokes_quanta_host", "wgrt_visits_reweight_many",
            "wgrt_visits_reweight_many_host", "wgrt_visit_wavelengths", "wgrt_hits_source_counts",
            "wgrt_hits_source_counts_host", "wgrt_hits_reweight_sources", "wgrt_hits_reweight_sources_host")
EXPORTED_DEBUG = ("wgrt_debug_shadow", "wgrt_debug_scene_copy", "wgrt_debug_set_auto_order",
                  "wgrt_debug_get_auto_order", "wgrt_debug_get_tile_tail", "wgrt_debug_order_host",
                  "wgrt_debug_chain_plan", "wgrt_debug_chain_set_serial", "wgrt_debug_set_byte_locator",
                  "wgrt_debug_set_palette_cap", "wgrt_debug_scene_palette", "wgrt_debug_expected_replays",
                  "wgrt_debug_chain_report", "wgrt_debug_set_fused_run", "wgrt_debug_fused_run",
                  "wgrt_debug_fused_items_host", "wgrt_debug_set_fused_taper", "wgrt_debug_fused_taper",
                  "wgrt_debug_fused_partition_host", "wgrt_debug_set_footprint_aggregate",
                  "wgrt_debug_set_reweight_layout", "wgrt_debug_trace_kernels", "wgrt_debug_last_trace_kernel")


class WgrtError(RuntimeError):
    pass


_d = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.POINTER(ctypes.c_int64)
_f = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p


class SceneDesc(ctypes.Structure):
    _fields_ = [
        ("IC", _d), ("n_ic", ctypes.c_int64),
        ("FC", _d), ("FC_offset", _i64), ("n_fc_slices", ctypes.c_int64),
        ("OC", _d), ("OC_offset", _i64), ("n_oc_slices", ctypes.c_int64),
        ("n_g", ctypes.c_double),
        ("eff_reg1", _d), ("n_eff_reg1", ctypes.c_int64),
        ("eff_reg2", _d), ("n_eff_reg2", ctypes.c_int64),
        ("eff_reg_FOV", _d), ("eff_reg_FOV_range", _d),
        ("lut_ic1", _d), ("lut_ic2", _d), ("lut_ic3", _d),
        ("lut_fc1", _d), ("lut_fc2", _d), ("lut_oc1", _d), ("lut_oc2", _d),
        ("ch5", ctypes.c_int32), ("ch3", ctypes.c_int32),
        ("lut_TIR", _d), ("lut_gap", _d),
        ("num_lmd", ctypes.c_int32), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32),
    ]


class Rays(ctypes.Structure):
    _fields_ = [(k, _vp) for k in ("x", "y", "gap_x", "gap_y", "pol", "azi", "m", "n", "lmd_num", "te",
                                   "tm", "delta_phase")]


class TraceStats(ctypes.Structure):
    _fields_ = [("bounces", ctypes.c_uint64), ("bad_rays", ctypes.c_uint64),
                ("eyebox_hits", ctypes.c_uint64), ("replayed", ctypes.c_uint64),
                ("handoff_giveups", ctypes.c_uint64), ("interactions", ctypes.c_uint64),
                ("libm_rays", ctypes.c_uint64)]


STATS_LEN = len(TraceStats._fields_)   # int64 words of a wgrt_trace_stats (torch stats tensors)
# ... and their indices by name: STAT.bounces, STAT.eyebox_hits, ... (tests/test_capi.py pins the layout to the header)
STAT = types.SimpleNamespace(**{name: i for i, (name, _) in enumerate(TraceStats._fields_)})


class DebugOpts(ctypes.Structure):
    """wgrt_debug_opts (include/wgrt_debug.h): per-call test / profiling overrides."""
    _fields_ = [("cert_tol", ctypes.c_double), ("cert_tol32", ctypes.c_double), ("chunk_rays", ctypes.c_int),
                ("timeline", ctypes.c_void_p), ("timeline_waves", ctypes.c_int64),
                ("fail_after_trace", ctypes.c_int), ("handoff_wait_ticks", ctypes.c_uint64)]


class LaunchOpts(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_int), ("variant", ctypes.c_int), ("workgroups", ctypes.c_int),
                ("chunk_order", ctypes.c_void_p), ("n_chunk_order", ctypes.c_int64),
                ("num_iter", ctypes.c_int), ("gid_blocks", ctypes.c_void_p), ("gid_block_rays", ctypes.c_int64),
                ("debug", ctypes.POINTER(DebugOpts)), ("grid_sqrt_k", ctypes.c_double)]


class FootprintPlanC(ctypes.Structure):
    """wgrt_footprint_plan (include/wgrt.h): the footprint maps' rectangle of the plate and its cells."""
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("cell_x", ctypes.c_double),
                ("cell_y", ctypes.c_double), ("nx_cells", ctypes.c_int32), ("ny_cells", ctypes.c_int32)]


LUT_ORDER = ("lut_ic1", "lut_ic2", "lut_ic3", "lut_fc1", "lut_fc2", "lut_oc1", "lut_oc2")   # lut_f32_angles bits


class SceneOpts(ctypes.Structure):
    _fields_ = [("cell_mm", ctypes.c_double), ("host_build", ctypes.c_int), ("lut_f32_angles", ctypes.c_int)]


class ShadowStats(ctypes.Structure):
    _fields_ = [("decisions", ctypes.c_uint64), ("uncertain", ctypes.c_uint64), ("silent_flips", ctypes.c_uint64),
                ("bounces", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64), ("max_ratio", ctypes.c_double),
                ("max_ratio32", ctypes.c_double),
                ("max_ratio_by_depth", ctypes.c_double * 6), ("decisions_by_depth", ctypes.c_uint64 * 6),
                ("ratio_hist", ctypes.c_uint64 * 20), ("max_ener_ratio", ctypes.c_double), ("max_amp", ctypes.c_double)]


class ChainPlan(ctypes.Structure):
    """``wgrt_chain_plan`` (include/wgrt_debug.h): where a chain's next step goes."""
    _fields_ = [("chained", ctypes.c_int), ("side", ctypes.c_int), ("join", ctypes.c_int), ("seed", ctypes.c_int),
                ("clear", ctypes.c_int), ("wait_serial", ctypes.c_uint32), ("publish_serial", ctypes.c_uint32),
                ("serial_after", ctypes.c_uint32), ("in_segment_after", ctypes.c_int64)]


# wgrt_debug_chain_plan's flags and the largest tag serial (include/wgrt_debug.h)
CHAIN_LEARNS, CHAIN_VARIANT1, CHAIN_SINGLE, CHAIN_FUSED, CHAIN_DEBUG, CHAIN_CAPTURE, CHAIN_FULL = 1, 2, 4, 8, 16, 32, 64
CHAIN_SERIAL_MAX = 0x7ffffffe


def chain_plan(in_segment: int, serial: int, flags: int = 0) -> dict:
    """``wgrt_debug_chain_plan``: the host logic of ``wgrt_chain_step`` (no GPU needed)."""
    p = ChainPlan()
    check(load().wgrt_debug_chain_plan(int(in_segment), int(serial), int(flags), ctypes.byref(p)),
          "wgrt_debug_chain_plan")
    return {f: int(getattr(p, f)) for f, _ in ChainPlan._fields_}


class ChainReport(ctypes.Structure):
    """``wgrt_chain_report`` (include/wgrt_debug.h): what an open chain has done so far."""
    _fields_ = [("gathering", ctypes.c_int), ("cap", ctypes.c_int), ("steps", ctypes.c_int64),
                ("launches", ctypes.c_int64), ("fused_launches", ctypes.c_int64), ("largest_launch", ctypes.c_int64),
                ("plain_steps", ctypes.c_int64), ("pending", ctypes.c_int64)]


def chain_report(chain: int) -> dict:
    """``wgrt_debug_chain_report`` of an open chain's handle (host counters; no GPU work)."""
    r = ChainReport()
    check(load().wgrt_debug_chain_report(ctypes.c_void_p(int(chain)), ctypes.byref(r)), "wgrt_debug_chain_report")
    return {f: int(getattr(r, f)) for f, _ in ChainReport._fields_}


class SceneInfo(ctypes.Structure):
    _fields_ = [("tile_bytes", ctypes.c_int64), ("tiles", ctypes.c_int64),
                ("grid_cells_x", ctypes.c_int64), ("grid_cells_y", ctypes.c_int64),
                ("grid_cell_mm", ctypes.c_double), ("grid_edge_cells", ctypes.c_int64),
                ("n_polygons", ctypes.c_int32), ("device", ctypes.c_int32),
                ("jtile_bytes", ctypes.c_int64), ("nonunitary_blocks", ctypes.c_int64)]


_lib = None
_lib_path = LIB_PATH
_accept_abi = (ABI_VERSION,)


def use_library(path: str, accept_abi=(ABI_VERSION,)) -> None:
    """Tools only (tools/with_lib.py: A/B timing of build variants, tools/ab.py): bind another build of
    the library, optionally of an earlier ABI whose structs are prefixes of this one's, instead of the
    in-tree one.  Must run before anything loads the library; the product never calls it."""
    global _lib_path, _accept_abi
    if _lib is not None:
        raise WgrtError(f"libwgrt is already loaded from {_lib_path}")
    _lib_path, _accept_abi = os.path.abspath(path), tuple(accept_abi)


def loaded_path() -> str:
    """The library file load() binds (the in-tree build unless a tool chose another)."""
    return _lib_path


def load():
    """Load libwgrt.so (never builds implicitly: build with ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _lib_path
    if not os.path.exists(path):
        raise WgrtError(f"{path} not found: the HIP library is not built "
                        "(run `python -c 'import __graft_entry__ as g; g.build()'`)")
    try:
        # RTLD_GLOBAL: the torch operator library (ops()) resolves the C ABI against this copy
        L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:
        raise WgrtError(f"cannot load {path}: {e}") from e
    # the ABI first: an accepted earlier build (tools only, use_library) may lack later entry points
    L.wgrt_abi_version.restype = ctypes.c_int
    L.wgrt_abi_version.argtypes = []
    abi = L.wgrt_abi_version()
    if abi not in _accept_abi:
        raise WgrtError(f"libwgrt ABI {abi} not in the accepted {_accept_abi}")
    st = ctypes.c_int
    L.wgrt_scene_create.restype = st
    L.wgrt_scene_create.argtypes = [ctypes.POINTER(SceneDesc), ctypes.c_int, ctypes.POINTER(_vp)]
    L.wgrt_scene_create_ex.restype = st
    L.wgrt_scene_create_ex.argtypes = [ctypes.POINTER(SceneDesc), ctypes.c_int, ctypes.POINTER(SceneOpts),
                                       ctypes.POINTER(_vp)]
    L.wgrt_scene_destroy.restype = st
    L.wgrt_scene_destroy.argtypes = [_vp]
    L.wgrt_scene_get_info.restype = st
    L.wgrt_scene_get_info.argtypes = [_vp, ctypes.POINTER(SceneInfo)]
    L.wgrt_trace_fullcolor.restype = st
    L.wgrt_trace_fullcolor.argtypes = [_vp, ctypes.POINTER(Rays), ctypes.c_int64, ctypes.c_int64, _vp, _vp,
                                       _vp, _vp, _vp]
    L.wgrt_trace_fullcolor_ex.restype = st
    L.wgrt_trace_fullcolor_ex.argtypes = [_vp, ctypes.POINTER(Rays), ctypes.c_int64, ctypes.c_int64, _vp,
                                          _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int]
    L.wgrt_trace_single.restype = st
    L.wgrt_trace_single.argtypes = L.wgrt_trace_fullcolor.argtypes
    L.wgrt_trace_single_ex.restype = st
    L.wgrt_trace_single_ex.argtypes = L.wgrt_trace_fullcolor_ex.argtypes
    L.wgrt_trace_opts.restype = st
    L.wgrt_trace_opts.argtypes = [_vp, ctypes.POINTER(Rays), ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp,
                                  _vp, ctypes.POINTER(LaunchOpts)]
    L.wgrt_rays_init.restype = st
    L.wgrt_rays_init.argtypes = [_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32,
                                 ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(Rays), _vp, _vp]
    L.wgrt_scene_classify.restype = st
    L.wgrt_scene_classify.argtypes = [_vp, _vp, ctypes.c_int64, _vp, _vp]
    L.wgrt_locator_classify_host.restype = st
    L.wgrt_locator_classify_host.argtypes = [ctypes.POINTER(SceneDesc), ctypes.c_double, _vp, ctypes.c_int64, _vp]
    L.wgrt_selftest_math.restype = st
    L.wgrt_selftest_math.argtypes = [_vp, _vp, ctypes.c_int64, _vp, _vp]
    L.wgrt_scene_reserve.restype = st
    L.wgrt_scene_reserve.argtypes = [_vp, ctypes.c_int64, ctypes.c_int, _vp]
    if abi >= 6:   # the strong-scaling gather's row-copy kernels (ABI 6)
        L.wgrt_eyebox_payload_floats.restype = ctypes.c_int64
        L.wgrt_eyebox_payload_floats.argtypes = [ctypes.c_int64]
        L.wgrt_eyebox_pack.restype = st
        L.wgrt_eyebox_pack.argtypes = [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp]
        L.wgrt_eyebox_assemble.restype = st
        L.wgrt_eyebox_assemble.argtypes = [_vp, ctypes.c_int64, _vp, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp]
    if abi >= 8:   # the per-slab eyebox reduction (ABI 8)
        L.wgrt_eyebox_window_sums.restype = st
        L.wgrt_eyebox_window_sums.argtypes = [_vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, _vp, _vp]
    if abi >= 9:   # the evaluation of the window-sum table (ABI 9)
        L.wgrt_eyebox_evaluate_workspace_bytes.restype = ctypes.c_int64
        L.wgrt_eyebox_evaluate_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
        ev = [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp]
        L.wgrt_eyebox_evaluate.restype = st
        L.wgrt_eyebox_evaluate.argtypes = ev + [_vp]
        L.wgrt_eyebox_evaluate_host.restype = st
        L.wgrt_eyebox_evaluate_host.argtypes = ev
    if hasattr(L, "wgrt_trace_windows"):   # the window-table sink: new symbols within ABI 9, bound by name
        L.wgrt_window_plan_create.restype = st
        L.wgrt_window_plan_create.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int,
                                              ctypes.POINTER(_vp)]
        L.wgrt_window_plan_destroy.restype = st
        L.wgrt_window_plan_destroy.argtypes = [_vp]
        L.wgrt_window_plan_width.restype = ctypes.c_int64
        L.wgrt_window_plan_width.argtypes = [_vp]
        L.wgrt_trace_windows.restype = st
        L.wgrt_trace_windows.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp]
        L.wgrt_window_plan_validate.restype = st
        L.wgrt_window_plan_validate.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
        L.wgrt_window_table_host.restype = st
        L.wgrt_window_table_host.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int64,
                                             ctypes.c_int64, _vp]
    # test / profiling hooks (include/wgrt_debug.h)
    L.wgrt_debug_shadow.restype = st
    L.wgrt_debug_shadow.argtypes = [_vp, ctypes.POINTER(Rays), ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _vp,
                                    _vp, _vp, _vp]
    L.wgrt_debug_scene_copy.restype = st
    L.wgrt_debug_scene_copy.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_int64]
    if hasattr(L, "wgrt_debug_set_auto_order"):   # the automatic issue order's hooks (absent from earlier builds)
        L.wgrt_debug_set_auto_order.restype = st
        L.wgrt_debug_set_auto_order.argtypes = [ctypes.c_int]
        L.wgrt_debug_get_auto_order.restype = st
        L.wgrt_debug_get_auto_order.argtypes = [_vp, _vp, _vp, ctypes.c_int64]
        L.wgrt_debug_get_tile_tail.restype = st
        L.wgrt_debug_get_tile_tail.argtypes = [_vp, _vp, ctypes.c_int64]
        L.wgrt_debug_order_host.restype = st
        L.wgrt_debug_order_host.argtypes = [_vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp]
    if hasattr(L, "wgrt_chain_begin"):   # chained single launches: new symbols within ABI 9, bound by name
        L.wgrt_chain_begin.restype = st
        L.wgrt_chain_begin.argtypes = [_vp, ctypes.POINTER(Rays), ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, ctypes.POINTER(_vp)]
        L.wgrt_chain_step.restype = st
        L.wgrt_chain_step.argtypes = [_vp]
        L.wgrt_chain_end.restype = st
        L.wgrt_chain_end.argtypes = [_vp]
        L.wgrt_debug_chain_plan.restype = st
        L.wgrt_debug_chain_plan.argtypes = [ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ChainPlan)]
        L.wgrt_debug_chain_set_serial.restype = st
        L.wgrt_debug_chain_set_serial.argtypes = [_vp, _vp, ctypes.c_uint32]
    if hasattr(L, "wgrt_chain_gather"):   # the opt-in gathering chain: new within ABI 9, bound by name
        L.wgrt_chain_gather.restype = st
        L.wgrt_chain_gather.argtypes = [_vp, ctypes.c_int, ctypes.c_int]
    if hasattr(L, "wgrt_debug_chain_report"):   # a chain's readout: new within ABI 9, bound by name
        L.wgrt_debug_chain_report.restype = st
        L.wgrt_debug_chain_report.argtypes = [_vp, ctypes.POINTER(ChainReport)]
    if hasattr(L, "wgrt_trace_fate"):   # per-ray fates and their census: new symbols within ABI 9, bound by name
        L.wgrt_trace_fate.restype = st
        L.wgrt_trace_fate.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, _vp]
        cen = [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp]
        L.wgrt_fate_census.restype = st
        L.wgrt_fate_census.argtypes = cen + [_vp]
        L.wgrt_fate_census_host.restype = st
        L.wgrt_fate_census_host.argtypes = cen
        L.wgrt_fate_col.restype = ctypes.c_int32
        L.wgrt_fate_col.argtypes = [ctypes.c_int]
        L.wgrt_fate_cols.restype = ctypes.c_int32
        L.wgrt_fate_cols.argtypes = []
        L.wgrt_fate_reason_name.restype = ctypes.c_char_p
        L.wgrt_fate_reason_name.argtypes = [ctypes.c_int]
    if hasattr(L, "wgrt_trace_replicas"):   # replica window tables and their fold: new symbols within ABI 9, by name
        L.wgrt_trace_replicas.restype = st
        L.wgrt_trace_replicas.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, ctypes.c_int]
        L.wgrt_window_replicas_fold.restype = st
        L.wgrt_window_replicas_fold.argtypes = [_vp, ctypes.c_int32, ctypes.c_int64, _vp, _vp]
        L.wgrt_window_replicas_fold_host.restype = st
        L.wgrt_window_replicas_fold_host.argtypes = [_vp, ctypes.c_int32, ctypes.c_int64, _vp]
    if hasattr(L, "wgrt_trace_expected"):   # the expected-value estimator: new symbols within ABI 9, by name
        a = L.wgrt_trace_opts.argtypes   # (wgrt_trace_opts' arguments without matrix_EB, then plan, table, replicas)
        L.wgrt_trace_expected.restype = st
        L.wgrt_trace_expected.argtypes = a[:5] + a[6:] + [_vp, _vp, ctypes.c_int]
        L.wgrt_expected_weight_host.restype = ctypes.c_double
        L.wgrt_expected_weight_host.argtypes = [ctypes.c_double] * 7
        L.wgrt_debug_expected_replays.restype = st
        L.wgrt_debug_expected_replays.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64]
    if hasattr(L, "wgrt_trace_footprint"):   # the footprint maps: new symbols within ABI 9, by name
        L.wgrt_trace_footprint.restype = st
        L.wgrt_trace_footprint.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, ctypes.POINTER(FootprintPlanC), _vp]
        L.wgrt_footprint_plan_validate.restype = st
        L.wgrt_footprint_plan_validate.argtypes = [ctypes.POINTER(FootprintPlanC)]
        L.wgrt_footprint_bin_host.restype = st
        L.wgrt_footprint_bin_host.argtypes = [ctypes.POINTER(FootprintPlanC), _vp, _vp, _vp, _vp, ctypes.c_int64,
                                              ctypes.c_int32, _vp]
        L.wgrt_footprint_channel_name.restype = ctypes.c_char_p
        L.wgrt_footprint_channel_name.argtypes = [ctypes.c_int]
        L.wgrt_debug_set_footprint_aggregate.restype = st
        L.wgrt_debug_set_footprint_aggregate.argtypes = [ctypes.c_int]
    if hasattr(L, "wgrt_trace_hits"):   # the hit list and its re-binning: new symbols within ABI 9, by name
        L.wgrt_trace_hits.restype = st
        L.wgrt_trace_hits.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_uint32]
        L.wgrt_hit_bytes.restype = ctypes.c_int32
        L.wgrt_hit_bytes.argtypes = []
        L.wgrt_hits_grid.restype = st
        L.wgrt_hits_grid.argtypes = [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp]
        L.wgrt_hits_grid_host.restype = st
        L.wgrt_hits_grid_host.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, ctypes.c_int64, _vp,
                                          ctypes.c_int32, ctypes.c_int32, _vp]
    if hasattr(L, "wgrt_trace_paths"):   # ray paths and their reduction: new symbols within ABI 9, by name
        L.wgrt_trace_paths.restype = st
        L.wgrt_trace_paths.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_uint32, _vp]
        L.wgrt_path_vertex_bytes.restype = ctypes.c_int32
        L.wgrt_path_vertex_bytes.argtypes = []
        L.wgrt_paths_footprint.restype = st
        L.wgrt_paths_footprint.argtypes = [_vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp]
        L.wgrt_paths_footprint_host.restype = st
        L.wgrt_paths_footprint_host.argtypes = [_vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp]
    if hasattr(L, "wgrt_trace_visits"):   # branch visit counts and their reductions: new symbols within ABI 9, by name
        i32 = ctypes.c_int32
        L.wgrt_trace_visits.restype = st
        L.wgrt_trace_visits.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, _vp, ctypes.c_int64, _vp, _vp]
        L.wgrt_visit_channels.restype = i32
        L.wgrt_visit_channels.argtypes = [_vp]
        L.wgrt_visits_sensitivity.restype = st
        L.wgrt_visits_sensitivity.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp]
        L.wgrt_visits_reweight.restype = st
        L.wgrt_visits_reweight.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp]
        L.wgrt_visits_sensitivity_host.restype = st
        L.wgrt_visits_sensitivity_host.argtypes = [i32, i32, i32, i32, _vp, _vp, i32, i32, i32, _vp, _vp, ctypes.c_int64, _vp]
        L.wgrt_visits_reweight_host.restype = st
        L.wgrt_visits_reweight_host.argtypes = [i32, i32, i32, i32, _vp, _vp, i32, i32, i32, _vp, _vp, ctypes.c_int64, _vp,
                                                _vp]
        L.wgrt_visit_channel_host.restype = i32
        L.wgrt_visit_channel_host.argtypes = [i32, i32, i32, i32, i32]
        L.wgrt_visit_channel_count_host.restype = i32
        L.wgrt_visit_channel_count_host.argtypes = [i32, i32]
    if hasattr(L, "wgrt_visits_reweight_many"):   # design ensembles: new symbols within ABI 9, by name
        i32 = ctypes.c_int32
        L.wgrt_visits_reweight_many.restype = st
        L.wgrt_visits_reweight_many.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, i32, _vp, _vp, _vp]
        L.wgrt_visits_reweight_many_host.restype = st
        L.wgrt_visits_reweight_many_host.argtypes = [i32, i32, i32, i32, _vp, _vp, i32, i32, i32, _vp, _vp, ctypes.c_int64,
                                                     _vp, i32, _vp, _vp]
        L.wgrt_visit_wavelengths.restype = i32
        L.wgrt_visit_wavelengths.argtypes = [_vp]
        L.wgrt_debug_set_reweight_layout.restype = st
        L.wgrt_debug_set_reweight_layout.argtypes = [ctypes.c_int]
    if hasattr(L, "wgrt_hits_reweight_sources"):   # source what-ifs: new symbols within ABI 9, by name
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        L.wgrt_hits_source_counts.restype = st
        L.wgrt_hits_source_counts.argtypes = [_vp, _vp, i64, i64, _vp, _vp]
        L.wgrt_hits_source_counts_host.restype = st
        L.wgrt_hits_source_counts_host.argtypes = [i32, i32, i32, _vp, i64, i64, _vp]
        L.wgrt_hits_reweight_sources.restype = st
        L.wgrt_hits_reweight_sources.argtypes = [_vp, _vp, _vp, i64, _vp, i64, i32, _vp, _vp, _vp]
        L.wgrt_hits_reweight_sources_host.restype = st
        L.wgrt_hits_reweight_sources_host.argtypes = [i32, i32, i32, _vp, _vp, i32, i32, i32, _vp, i64, _vp, i64, i32, _vp,
                                                      _vp]
    if hasattr(L, "wgrt_trace_stokes"):   # the Stokes window tables: new symbols within ABI 9, by name
        L.wgrt_trace_stokes.restype = st
        L.wgrt_trace_stokes.argtypes = L.wgrt_trace_opts.argtypes + [_vp, _vp, _vp]
        L.wgrt_stokes_quanta_host.restype = None
        L.wgrt_stokes_quanta_host.argtypes = [ctypes.c_double] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    if hasattr(L, "wgrt_locator_palette_host"):   # the byte locator's hooks: new symbols within ABI 9, bound by name
        L.wgrt_locator_palette_host.restype = st
        L.wgrt_locator_palette_host.argtypes = [ctypes.POINTER(SceneDesc), ctypes.c_double, _i64, _i64, _d,
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), _vp, _vp, _vp,
                                                ctypes.c_int64]
        L.wgrt_debug_set_byte_locator.restype = st
        L.wgrt_debug_set_byte_locator.argtypes = [ctypes.c_int]
        L.wgrt_debug_set_palette_cap.restype = st
        L.wgrt_debug_set_palette_cap.argtypes = [ctypes.c_int]
        L.wgrt_debug_scene_palette.restype = st
        L.wgrt_debug_scene_palette.argtypes = [_vp] + [ctypes.POINTER(ctypes.c_int)] * 3
    if hasattr(L, "wgrt_debug_set_fused_run"):   # fused launches' runs: new symbols within ABI 9, bound by name
        L.wgrt_debug_set_fused_run.restype = st
        L.wgrt_debug_set_fused_run.argtypes = [ctypes.c_int]
        L.wgrt_debug_fused_run.restype = st
        L.wgrt_debug_fused_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.wgrt_debug_fused_items_host.restype = st
        L.wgrt_debug_fused_items_host.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                  ctypes.c_int64, _vp, _vp, _vp, _i64]
    if hasattr(L, "wgrt_debug_set_fused_taper"):   # fused launches' taper: new symbols within ABI 9, bound by name
        L.wgrt_debug_set_fused_taper.restype = st
        L.wgrt_debug_set_fused_taper.argtypes = [ctypes.c_int]
        L.wgrt_debug_fused_taper.restype = st
        L.wgrt_debug_fused_taper.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.wgrt_debug_fused_partition_host.restype = st
        L.wgrt_debug_fused_partition_host.argtypes = [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_int64] * 2 + \
            [ctypes.POINTER(ctypes.c_int)] + [_vp] * 6 + [_i64]
    if hasattr(L, "wgrt_debug_trace_kernels"):   # the kernel table's readouts: new symbols within ABI 9, bound by name
        L.wgrt_debug_trace_kernels.restype = st
        L.wgrt_debug_trace_kernels.argtypes = [_vp, ctypes.c_int64]
        L.wgrt_debug_last_trace_kernel.restype = st
        L.wgrt_debug_last_trace_kernel.argtypes = [_vp, _vp]
    L.wgrt_status_string.restype = ctypes.c_char_p
    L.wgrt_status_string.argtypes = [ctypes.c_int]
    L.wgrt_last_error.restype = ctypes.c_char_p
    L.wgrt_last_error.argtypes = []
    _lib = L
    return L


_ops = None


def ops():
    """``torch.ops.wgrt``: the trace operator (``_wgrt_torch.so``), loaded after ``libwgrt.so``,
    whose C ABI it calls (never builds implicitly)."""
    global _ops
    if _ops is not None:
        return _ops
    load()
    if not os.path.exists(OPS_PATH):
        raise WgrtError(f"{OPS_PATH} not found: the torch operator library is not built "
                        "(run `python -c 'import __graft_entry__ as g; g.build()'`)")
    import torch
    try:
        torch.ops.load_library(OPS_PATH)
    except OSError as e:
        raise WgrtError(f"cannot load {OPS_PATH}: {e}") from e
    _ops = torch.ops.wgrt
    return _ops


def check(status: int, what: str):
    if status != 0:
        L = load()
        raise WgrtError(f"{what}: {L.wgrt_status_string(status).decode()} -- {L.wgrt_last_error().decode()}")


def _ptr(a: np.ndarray, t=_d):
    return a.ctypes.data_as(t)


def make_desc(IC, FC, FC_offset, OC, OC_offset, n_g, eff_reg1, eff_reg2, eff_reg_FOV, eff_reg_FOV_range,
          lut_ic1, lut_ic2, lut_ic3, lut_fc1, lut_fc2, lut_oc1, lut_oc2, lut_TIR, lut_gap):
    """Validate the reference's scene arrays and pack them into a ``wgrt_scene_desc``.

    Returns ``(desc, keepalive, (num_lmd, nx, ny, n_fc_slices, n_oc_slices))``; keep the
    second item alive while the descriptor is in use.  Single-wavelength LUTs (the
    ``process_rays_kernel_pro`` shapes: lut_TIR [NX, NY, 4], lut_fc1 [nFC, NX, NY, C], ...)
    are accepted and described as num_lmd = 1 (the same memory layout).  Raises ValueError on any shape
    mismatch (the reference would index out of bounds instead).
    """
    if np.ndim(lut_TIR) == 3:   # single-wavelength LUTs (GRTF:419-427): add a lambda axis of 1
        lut_ic1, lut_ic2, lut_ic3, lut_TIR, lut_gap = (np.asarray(a)[None] for a in
                                                       (lut_ic1, lut_ic2, lut_ic3, lut_TIR, lut_gap))
        lut_fc1, lut_fc2, lut_oc1, lut_oc2 = (np.asarray(a)[:, None] for a in (lut_fc1, lut_fc2, lut_oc1, lut_oc2))
    f64 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    c128 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.complex128)
    i64 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.int64)
    k = dict(IC=f64(IC), FC=f64(FC), FC_offset=i64(FC_offset), OC=f64(OC), OC_offset=i64(OC_offset),
             eff1=f64(eff_reg1), eff2=f64(eff_reg2), fov=f64(eff_reg_FOV), fovr=f64(eff_reg_FOV_range),
             ic1=c128(lut_ic1), ic2=c128(lut_ic2), ic3=c128(lut_ic3), fc1=c128(lut_fc1),
             fc2=c128(lut_fc2), oc1=c128(lut_oc1), oc2=c128(lut_oc2), tir=f64(lut_TIR), gap=f64(lut_gap))
    for name in ("IC", "FC", "OC", "eff1", "eff2"):
        a = k[name]
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"{name} must have shape (V, 2), got {a.shape}")
    if k["tir"].ndim != 4 or k["tir"].shape[-1] != 4:
        raise ValueError(f"lut_TIR must have shape (L, NX, NY, 4), got {k['tir'].shape}")
    nl, nx, ny = k["tir"].shape[:3]
    nfc, noc = k["FC_offset"].shape[0] - 1, k["OC_offset"].shape[0] - 1
    want = {"gap": (nl, nx, ny, 8), "fov": (nx, ny, 4, 2), "fovr": (nx, ny, 4)}
    for name, shp in want.items():
        if k[name].shape != shp:
            raise ValueError(f"{name}: shape {k[name].shape} != {shp}")
    for name in ("ic1", "ic2", "ic3"):
        if k[name].shape[:3] != (nl, nx, ny):
            raise ValueError(f"lut_{name}: shape {k[name].shape} does not match grid {(nl, nx, ny)}")
    for name, ns in (("fc1", nfc), ("fc2", nfc), ("oc1", noc), ("oc2", noc)):
        if k[name].shape[:4] != (ns, nl, nx, ny):
            raise ValueError(f"lut_{name}: shape {k[name].shape} does not match {(ns, nl, nx, ny)}")
    if k["FC_offset"][-1] > k["FC"].shape[0] or k["OC_offset"][-1] > k["OC"].shape[0]:
        raise ValueError("FC_offset / OC_offset point past the vertex arrays")
    ch5 = k["ic1"].shape[-1]
    if not (k["ic2"].shape[-1] == k["ic3"].shape[-1] == k["oc1"].shape[-1] == k["oc2"].shape[-1] == ch5):
        raise ValueError("ic*/oc* LUTs must share one channel count")
    ch3 = k["fc1"].shape[-1]
    if k["fc2"].shape[-1] != ch3:
        raise ValueError("fc1/fc2 LUTs must share one channel count")
    desc = SceneDesc(
        _ptr(k["IC"]), k["IC"].shape[0], _ptr(k["FC"]), _ptr(k["FC_offset"], _i64), nfc,
        _ptr(k["OC"]), _ptr(k["OC_offset"], _i64), noc, float(n_g),
        _ptr(k["eff1"]), k["eff1"].shape[0], _ptr(k["eff2"]), k["eff2"].shape[0],
        _ptr(k["fov"]), _ptr(k["fovr"]),
        _ptr(k["ic1"]), _ptr(k["ic2"]), _ptr(k["ic3"]), _ptr(k["fc1"]), _ptr(k["fc2"]),
        _ptr(k["oc1"]), _ptr(k["oc2"]), ch5, ch3, _ptr(k["tir"]), _ptr(k["gap"]), nl, nx, ny)
    return desc, k, (nl, nx, ny, nfc, noc)


class Scene:
    """Device-resident geometry + packed LUT tiles (``wgrt_scene_create``).

    Arguments are the reference's scene arrays (couplers_coor.py:740-750 and the
    seven LUTs of gpu_ray_tracing_pro_fullColor.py:28-34), as host numpy arrays.
    """

    def __init__(self, IC, FC, FC_offset, OC, OC_offset, n_g, eff_reg1, eff_reg2, eff_reg_FOV,
                 eff_reg_FOV_range, lut_ic1, lut_ic2, lut_ic3, lut_fc1, lut_fc2, lut_oc1, lut_oc2,
                 lut_TIR, lut_gap, device: int = 0, cell_mm: float = 0.0, host_build: bool = False,
                 lut_f32_angles: int | None = None):
        """``cell_mm`` / ``host_build`` / ``lut_f32_angles``: wgrt_scene_opts (0 / False: the defaults;
        ``lut_f32_angles=None``: bit k set for each LUT given in single precision, luts.lut_f32_mask)."""
        L = load()
        desc, _keep, (nl, nx, ny, nfc, noc) = make_desc(
            IC, FC, FC_offset, OC, OC_offset, n_g, eff_reg1, eff_reg2, eff_reg_FOV, eff_reg_FOV_range,
            lut_ic1, lut_ic2, lut_ic3, lut_fc1, lut_fc2, lut_oc1, lut_oc2, lut_TIR, lut_gap)
        h = _vp()
        if lut_f32_angles is None:
            from .luts import lut_f32_mask
            lut_f32_angles = lut_f32_mask(dict(zip(LUT_ORDER, (lut_ic1, lut_ic2, lut_ic3, lut_fc1, lut_fc2,
                                                               lut_oc1, lut_oc2))))
        opts = SceneOpts(float(cell_mm), 1 if host_build else 0, int(lut_f32_angles))
        self.lut_f32_angles = int(lut_f32_angles)
        check(L.wgrt_scene_create_ex(ctypes.byref(desc), int(device), ctypes.byref(opts), ctypes.byref(h)),
              "wgrt_scene_create")
        self._h = h
        self.single_lambda = np.ndim(lut_TIR) == 3
        self.device = int(device)
        self.num_lmd, self.nx, self.ny = nl, nx, ny
        self.n_fc_slices, self.n_oc_slices = nfc, noc
        self.n_g = float(n_g)

    @classmethod
    def from_geometry(cls, geom, luts: dict, device: int = 0, wavelength: int | None = None, **opts):
        """Scene of a geometry + LUT set.  ``wavelength=l`` builds the single-wavelength scene
        of wavelength l (the arrays process_rays_kernel_pro takes, luts.single_wavelength);
        ``opts``: ``cell_mm`` / ``host_build`` (wgrt_scene_opts)."""
        tir, gap = geom.lut_TIR, geom.lut_gap
        if wavelength is not None:
            from .luts import single_wavelength
            luts, tir, gap = single_wavelength(luts, tir, gap, wavelength)
        return cls(geom.IC, geom.FC, geom.FC_offset, geom.OC, geom.OC_offset, geom.n_g, geom.eff_reg1,
                   geom.eff_reg2, geom.eff_reg_FOV, geom.eff_reg_FOV_range, luts["lut_ic1"], luts["lut_ic2"],
                   luts["lut_ic3"], luts["lut_fc1"], luts["lut_fc2"], luts["lut_oc1"], luts["lut_oc2"],
                   tir, gap, device=device, **opts)

    @property
    def handle(self):
        if self._h is None:
            raise WgrtError("scene destroyed")
        return self._h

    def info(self) -> dict:
        inf = SceneInfo()
        check(load().wgrt_scene_get_info(self.handle, ctypes.byref(inf)), "wgrt_scene_get_info")
        return {f: getattr(inf, f) for f, _ in SceneInfo._fields_}

    def debug_copy(self, which: str) -> np.ndarray:
        """Host copy of a device structure (wgrt_debug_scene_copy): "cells" (uint64 [ncy, ncx]),
        "tiles" / "jtiles" (float64 [tiles, doubles per tile]), "cells8" / "palette" (the byte locator's byte grid,
        uint8 [ncy, ncx], and its 256 palette words; a scene without a byte grid raises)."""
        inf = self.info()
        if which == "cells":
            out = np.empty((inf["grid_cells_y"], inf["grid_cells_x"]), np.uint64)
        elif which == "cells8":
            out = np.empty((inf["grid_cells_y"], inf["grid_cells_x"]), np.uint8)
        elif which == "palette":
            out = np.empty(256, np.uint64)
        else:
            per = inf["tile_bytes" if which == "tiles" else "jtile_bytes"] // 8
            out = np.empty((inf["tiles"], per), np.float64)
        k = {"cells": 0, "tiles": 1, "jtiles": 2, "cells8": 3, "palette": 4}[which]
        check(load().wgrt_debug_scene_copy(self.handle, k, out.ctypes.data, out.nbytes), "wgrt_debug_scene_copy")
        return out

    def palette_info(self) -> dict:
        """``wgrt_debug_scene_palette``: the grid's distinct cell words, whether the scene has a byte grid, and
        whether its Jones-vector launches run the byte locator now."""
        n, g, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(load().wgrt_debug_scene_palette(self.handle, ctypes.byref(n), ctypes.byref(g), ctypes.byref(a)),
              "wgrt_debug_scene_palette")
        return {"distinct_words": n.value, "byte_grid": bool(g.value), "active": bool(a.value)}

    def last_trace_kernel(self) -> tuple:
        """``wgrt_debug_last_trace_kernel``: the kernel table entry ``(mode, byte, wide, fused, single, amp)`` the scene's
        last launch looked up (``trace_kernels``' order); all -1 after a variant 1 launch, or before any."""
        idx = np.empty(6, np.int32)
        check(load().wgrt_debug_last_trace_kernel(self.handle, idx.ctypes.data), "wgrt_debug_last_trace_kernel")
        return tuple(int(v) for v in idx)

    def eb_shape(self):
        if self.single_lambda:   # process_rays_kernel_pro's matrix_EB [NY, NX, 80, 120]
            return (self.ny, self.nx, 80, 120)
        return (self.num_lmd, self.ny, self.nx, 80, 120)

    def close(self):
        if getattr(self, "_h", None) is not None:
            load().wgrt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def locator_classify_host(geom, luts, xy: np.ndarray, cell_mm: float = 0.125) -> np.ndarray:
    """Host replica of the kernels' polygon locator (``wgrt_locator_classify_host``): bit k of
    the result is is_inside_or_on_edge(point, polygon k) (0 eff_reg1, 1 eff_reg2, 2 IC,
    3.. FC slices, then OC slices).  Needs no GPU."""
    L = load()
    desc, keep, _ = make_desc(geom.IC, geom.FC, geom.FC_offset, geom.OC, geom.OC_offset, geom.n_g,
                              geom.eff_reg1, geom.eff_reg2, geom.eff_reg_FOV, geom.eff_reg_FOV_range,
                              luts["lut_ic1"], luts["lut_ic2"], luts["lut_ic3"], luts["lut_fc1"],
                              luts["lut_fc2"], luts["lut_oc1"], luts["lut_oc2"], geom.lut_TIR, geom.lut_gap)
    pts = np.ascontiguousarray(xy, dtype=np.float64)
    out = np.zeros(pts.shape[0], dtype=np.uint64)
    check(L.wgrt_locator_classify_host(ctypes.byref(desc), float(cell_mm), pts.ctypes.data_as(_vp), pts.shape[0],
                                       out.ctypes.data_as(_vp)),
          "wgrt_locator_classify_host")
    return out



def trace_kernels(modes: int) -> np.ndarray:
    """``wgrt_debug_trace_kernels``: which entries of the Jones kernel table are built, as a uint8 array
    ``[modes, 2, 2, 2, 2, 2]`` over (mode, byte locator, 64-bit cells, fused, single wavelength, AMP); needs no GPU.
    ``modes`` must be the library's count of trace modes (any other is refused)."""
    out = np.full(int(modes) * 32, 255, np.uint8)
    check(load().wgrt_debug_trace_kernels(out.ctypes.data, out.size), "wgrt_debug_trace_kernels")
    return out.reshape(int(modes), 2, 2, 2, 2, 2)


def set_byte_locator(on: bool) -> None:
    """``wgrt_debug_set_byte_locator``: the Jones-vector lane's byte locator on / off, process-wide (A/B, tests)."""
    check(load().wgrt_debug_set_byte_locator(1 if on else 0), "wgrt_debug_set_byte_locator")


def set_reweight_layout(interleaved: bool) -> None:
    """``wgrt_debug_set_reweight_layout``: the form of ``wgrt_visits_reweight_many``'s deposits, process-wide (A/B, tests):
    through a scratch interleaved over a chunk's designs (the default) or straight into the tables; both give the same
    bits."""
    check(load().wgrt_debug_set_reweight_layout(1 if interleaved else 0), "wgrt_debug_set_reweight_layout")


def set_footprint_aggregate(on: bool) -> None:
    """``wgrt_debug_set_footprint_aggregate``: the footprint sink's on-chip summing on / off, process-wide (A/B, tests);
    both forms give the same map."""
    check(load().wgrt_debug_set_footprint_aggregate(1 if on else 0), "wgrt_debug_set_footprint_aggregate")


def set_fused_run(run: int = 0) -> None:
    """``wgrt_debug_set_fused_run``: the run length of fused launches, process-wide (A/B, tests): 0 automatic, 1 a
    hand-off after every trace, n (a power of two up to 64) runs of n traces on one lane."""
    check(load().wgrt_debug_set_fused_run(int(run)), "wgrt_debug_set_fused_run")


def fused_run(num_iter: int, handoff_bound: bool = False) -> int:
    """``wgrt_debug_fused_run``: the run length a fused launch of ``num_iter`` traces runs with now (no GPU needed)."""
    run = ctypes.c_int()
    check(load().wgrt_debug_fused_run(int(num_iter), 1 if handoff_bound else 0, ctypes.byref(run)), "wgrt_debug_fused_run")
    return run.value


def fused_items_host(n_chunks: int, num_iter: int, run: int, head: int):
    """``wgrt_debug_fused_items_host``: every work item of ``head``'s queue, in order, from the code the kernels compile
    (no GPU needed): ``(chunk, first_trace, end_trace)`` arrays, one entry per item."""
    cap = (int(n_chunks) + 1) * ((int(num_iter) + int(run) - 1) // int(run)) + 1
    chunk, k0, k1 = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n = ctypes.c_int64()
    check(load().wgrt_debug_fused_items_host(int(n_chunks), int(num_iter), int(run), int(head), 0, cap, chunk.ctypes.data,
                                             k0.ctypes.data, k1.ctypes.data, ctypes.byref(n)),
          "wgrt_debug_fused_items_host")
    assert n.value < cap, "the head's queue ends before the buffer does"
    return chunk[:n.value], k0[:n.value], k1[:n.value]


def set_fused_taper(t0: int = -1) -> None:
    """``wgrt_debug_set_fused_taper``: the taper of fused launches, process-wide (A/B, tests): -1 the library's rule,
    0 never, a power of two that first tail length (the launch's last runs are t0, t0 / 2, ..., 2, 1 traces)."""
    check(load().wgrt_debug_set_fused_taper(int(t0)), "wgrt_debug_set_fused_taper")


def fused_taper(num_iter: int, n_rays: int, handoff_bound: bool = False) -> int:
    """``wgrt_debug_fused_taper``: the first tail length a fused launch of ``num_iter`` traces of ``n_rays`` rays runs
    with now (0: none)."""
    t0 = ctypes.c_int()
    check(load().wgrt_debug_fused_taper(int(num_iter), int(n_rays), 1 if handoff_bound else 0, ctypes.byref(t0)),
          "wgrt_debug_fused_taper")
    return t0.value


def fused_partition_host(n_chunks: int, num_iter: int, run: int, t0: int, head: int = 0, items: bool = True) -> dict:
    """``wgrt_debug_fused_partition_host``: the run partition of a fused launch and ``head``'s work items under it, from
    the code the kernels compile (no GPU needed): ``run_first`` (per run), ``trace_first``, ``trace_end`` (per
    trace) and, with ``items``, the ``chunk``, ``first_trace``, ``end_trace`` arrays of every item, in order."""
    n_it = int(num_iter)
    cap = (int(n_chunks) + 1) * n_it + 1 if items else 0
    n_runs = ctypes.c_int()
    rf, tf, te = (np.zeros(n_it, np.int32) for _ in range(3))
    chunk, k0, k1 = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n = ctypes.c_int64()
    check(load().wgrt_debug_fused_partition_host(int(n_chunks), n_it, int(run), int(t0), int(head), 0, cap,
                                                 ctypes.byref(n_runs), rf.ctypes.data, tf.ctypes.data, te.ctypes.data,
                                                 chunk.ctypes.data, k0.ctypes.data, k1.ctypes.data,
                                                 ctypes.byref(n)), "wgrt_debug_fused_partition_host")
    assert not items or n.value < cap, "the head's queue ends before the buffer does"
    return {"run_first": rf[:n_runs.value], "trace_first": tf, "trace_end": te,
            "chunk": chunk[:n.value], "first_trace": k0[:n.value], "end_trace": k1[:n.value]}


def set_palette_cap(cap: int = 256) -> None:
    """``wgrt_debug_set_palette_cap``: scenes created from now on get a byte grid only with at most ``cap``
    distinct cell words (tests force the word-form fallback with a small cap)."""
    check(load().wgrt_debug_set_palette_cap(int(cap)), "wgrt_debug_set_palette_cap")


def locator_palette_host(geom, luts, cell_mm: float = 0.125, tables: bool = True) -> dict:
    """Host build of the byte locator's tables (``wgrt_locator_palette_host``; needs no GPU): ``count`` distinct
    cell words, ``cells`` (uint64 [ncy, ncx]) and, when the descriptor gets a byte grid, ``palette`` (uint64
    [256]) and ``cells8`` (uint8 [ncy, ncx]); else both None; ``x0, y0, h``: the grid's origin and cell size.  ``tables=False``: the count and grid size only."""
    L = load()
    desc, keep, _ = make_desc(geom.IC, geom.FC, geom.FC_offset, geom.OC, geom.OC_offset, geom.n_g,
                              geom.eff_reg1, geom.eff_reg2, geom.eff_reg_FOV, geom.eff_reg_FOV_range,
                              luts["lut_ic1"], luts["lut_ic2"], luts["lut_ic3"], luts["lut_fc1"],
                              luts["lut_fc2"], luts["lut_oc1"], luts["lut_oc2"], geom.lut_TIR, geom.lut_gap)
    ncx, ncy, cnt, has = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    grid = (ctypes.c_double * 3)()
    call = lambda *bufs: check(L.wgrt_locator_palette_host(ctypes.byref(desc), float(cell_mm), ctypes.byref(ncx),
                                                           ctypes.byref(ncy), grid, ctypes.byref(cnt), ctypes.byref(has), *bufs),
                               "wgrt_locator_palette_host")
    call(None, None, None, 0)
    out = {"count": cnt.value, "byte_grid": bool(has.value), "ncx": ncx.value, "ncy": ncy.value, "x0": grid[0],
           "y0": grid[1], "h": grid[2], "cells": None,
           "palette": None, "cells8": None}
    if not tables:
        return out
    shape = (ncy.value, ncx.value)
    pal, c8, cells = np.zeros(256, np.uint64), np.zeros(shape, np.uint8), np.zeros(shape, np.uint64)
    call(pal.ctypes.data_as(_vp), c8.ctypes.data_as(_vp), cells.ctypes.data_as(_vp), cells.size)
    out["cells"] = cells
    if has.value:
        out["palette"], out["cells8"] = pal, c8
    return out
