"""Device-side entry points over torch ROCm tensors (PyTorch is the memory/stream plumbing).

``trace_fullcolor`` is one launch of the bounce kernel (the reference's
``process_rays_kernel_pro_fullColor[blocks, 256](...)``, GRTF:833-1246) through the
PyTorch-ROCm operator ``torch.ops.wgrt.trace`` (csrc/wgrt_torch.cpp), which forwards to the
C ABI ``wgrt_trace_opts``; it validates every buffer and raises on misuse instead of
corrupting memory.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import STAT, STATS_LEN, DebugOpts, Rays, Scene, TraceStats, WgrtError, check, load, ops

RAY_COLUMNS = ("x", "y", "gap_x", "gap_y", "pol", "azi", "m", "n", "lmd_num", "te", "tm", "delta_phase")
READ_COLUMNS = ("x", "y", "m", "n", "lmd_num", "te", "tm", "delta_phase")

VARIANT_AUTO, VARIANT_GRID, VARIANT_JONES32, VARIANT_JONES64 = 0, 1, 7, 9   # include/wgrt.h
CHUNK = 64   # rays per work-queue chunk of the persistent kernels (wgrt_launch_opts.chunk_order)


def _stream_handle(device: torch.device, stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return int(s.cuda_stream)


def _as_dev(t, dtype, name, device, n=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if n is not None and t.numel() != n:
        raise ValueError(f"{name} has {t.numel()} elements, expected {n}")
    return t


def rays_to_device(rays: dict, device="cuda") -> dict:
    """Copy the twelve float32 host columns (rays.build_rays) to device tensors."""
    return {k: torch.from_numpy(np.ascontiguousarray(rays[k], dtype=np.float32)).to(device)
            for k in RAY_COLUMNS if k in rays}


def trace_fullcolor(scene: Scene, rays: dict, rng_states: torch.Tensor, matrix_EB: torch.Tensor | None,
                    gid_offset: int = 0, n_rays: int | None = None, stats: torch.Tensor | None = None,
                    per_ray_bounces: torch.Tensor | None = None, stream=None, variant: int = VARIANT_AUTO,
                    workgroups: int = 0, chunk_order: torch.Tensor | None = None, num_iter: int = 1,
                    gid_blocks: torch.Tensor | None = None, gid_block_rays: int = 0, debug: dict | None = None,
                    grid_sqrt_k: float = 0.0, windows=None, fate: torch.Tensor | None = None, replicas: int = 0,
                    expected: bool = False, footprint=None, hits=None, paths=None, select=None, visits=None,
                 stokes=None) -> None:
    """Asynchronous launch on ``stream`` (default: torch's current stream).

    rays: dict of device float32 tensors keyed like the reference columns
    (``x, y, m, n, lmd_num, te, tm, delta_phase`` required; the four columns the
    kernel never reads may be absent).  rng_states uint32 -> torch.int32 view is
    accepted too.  stats: optional int64[STATS_LEN] device tensor that is added to
    (bounces, bad_rays, eyebox_hits, replayed, handoff_giveups, interactions, libm_rays; ``check_stats`` raises
    on a hand-off give-up).  chunk_order: optional int32 device permutation of the 64-ray chunks
    (``schedule_by_lifetime``); results do not depend on it.  num_iter: chained traces of every
    ray (the reference's ``num_iter`` loop of launches, MAIN:169-177) in one call -- results
    identical to ``num_iter`` calls; the Jones-vector variants run them in one persistent launch
    (``wgrt_launch_opts.num_iter``).  gid_blocks / gid_block_rays: global ray ids of a shard made of
    several block ranges (int64 device tensor, first global id of each local block of
    ``gid_block_rays`` rays; ``gid_offset`` must then be 0).  debug: ``wgrt_debug_opts`` fields
    (cert_tol, cert_tol32, chunk_rays, timeline (uint64 device tensor), fail_after_trace,
    handoff_wait_ticks) -- test / profiling hooks.  grid_sqrt_k: the single-trace grid rule
    (``wgrt_launch_opts.grid_sqrt_k``; 0 the default, < 0 the resident grid).  windows: ``(plan, table)``, a
    ``WindowPlan`` and a float64 ``[n_slabs, plan.W]`` device tensor (``plan.new_table(scene)``) that every
    out-coupling is also counted into (``wgrt_trace_windows``: the table equals ``eyebox_window_sums`` of the grid
    the same trace leaves); ``matrix_EB`` may then be None, and no grid is written.  fate: a uint8 device tensor
    of one byte per ray of the batch that takes every traced ray's fate code (``wgrt_trace_fate``; ``FATE_CODES``,
    0 for a ray that was skipped); single launches only (``num_iter > 1`` raises), and nothing else the launch
    leaves changes.  replicas: ``B``, with ``windows=(plan, table)`` and ``table`` the float64 ``[B, n_slabs, plan.W]``
    tensor of ``plan.new_table(scene, replicas=B)``: an out-coupling of the ray with global id ``g`` counts into
    ``table[g % B]`` (``wgrt_trace_replicas``; 2 <= B <= 64), so ``table.sum(0)`` is the table a plain windows trace
    leaves, bit for bit, and ``fold_replicas`` / ``evaluation_error_bars`` turn the copies into jackknife error
    bars; single launches only, not together with ``fate``; 0 or 1: no replicas.  expected: the expected-value
    estimator (``wgrt_trace_expected``): needs ``windows=(plan, table)`` and ``matrix_EB=None``; the walk --
    ``rng_states``, ``per_ray_bounces``, ``stats`` -- is the plain launch's bit for bit, but every out-coupler
    interaction inside the FoV's eyebox rectangle adds its out-coupling probability (a multiple of 2^-32) to the
    table instead of 1.0 per out-coupled ray: the same expectation with a fraction of the variance.  Works with
    ``replicas=B``; a grid, ``fate``, ``num_iter > 1`` and a ``TraceChain`` raise ``ValueError``.  footprint:
    ``(fp, map)``, a ``FootprintPlan`` and the int64 ``[num_lmd, 9, ny_cells, nx_cells]`` device tensor of
    ``fp.new_map(scene)`` (``wgrt_trace_footprint``): every Monte-Carlo draw of the bounce loop adds 1 to the map at
    the plate cell where the ray stood, in the channel of its state R0..R5, and the draw that loses the ray or
    out-couples it inside / beside its eyebox rectangle also in channel 6 / 7 / 8 (``FOOTPRINT_CHANNELS``); nothing
    else the launch leaves changes.  Single launches only; ``fate``, ``replicas``, ``expected``, ``num_iter > 1`` and a
    ``TraceChain`` raise ``ValueError``.  hits: ``(hit_list, tag)``, a ``HitList`` on the scene's device and a tag
    0 .. 65535 (``wgrt_trace_hits``): every out-coupling of the launch, inside its eyebox rectangle or beside it, is
    appended to the list as one record tagged ``tag``; nothing else the launch leaves changes.  Single launches only;
    ``fate``, ``replicas``, ``expected``, ``footprint``, ``num_iter > 1`` and a ``TraceChain`` raise ``ValueError``.
    paths: ``(path_list, tag)``, a ``PathList`` on the scene's device and a tag 0 .. 65535 (``wgrt_trace_paths``): every
    draw of the bounce loop of the rays ``select`` names -- a uint8 / bool device tensor ``[n_rays]``, nonzero: record
    the ray; None: every ray (``select_by_fate`` builds one from a fate launch of the same RNG states) -- is appended
    as one record, and the end of a trace that leaves the plate or misses in R5 as one more; nothing else the launch
    leaves changes.  Single launches only; ``fate``, ``replicas``, ``expected``, ``footprint``, ``hits``,
    ``num_iter > 1`` and a ``TraceChain`` raise ``ValueError``.
    visits: ``(visit_table, slot)``, a ``VisitTable`` on the scene's device and an int32 device tensor ``[n_rays]`` or
    None (``wgrt_trace_visits``): ray i is counted into row ``slot[i]`` (negative: not counted; None: row i) -- every
    Monte-Carlo draw that takes a branch adds 1 to its channel (``visit_channels``) in the row, and a ray that
    out-couples leaves its row's end record; nothing else the launch leaves changes.  Raises ``ValueError`` if
    ``slot.max() >= n_rows`` (the device does not validate slots; the check synchronises).  Single launches only;
    ``fate``, ``replicas``, ``expected``, ``footprint``, ``hits``, ``paths``, ``num_iter > 1`` and a ``TraceChain``
    raise ``ValueError``.
    stokes: a ``StokesTable`` of the scene and the window plan (``wgrt_trace_stokes``; needs ``windows=(plan, table)``):
    every out-coupling the window table counts also adds the three fixed-point normalised Stokes parameters of the
    out-coupled field (``q_k = rint(s_k * 2^30)``, in the TE / TM basis of that FoV's out-coupled order) to the same
    entries of the int64 ``[3, n_slabs, W]`` tables; nothing else the launch leaves changes.  Single launches only; any
    other sink, ``replicas``, ``num_iter > 1`` and a ``TraceChain`` raise ``ValueError``.
    """
    if scene.single_lambda:
        raise ValueError("trace_fullcolor needs a full-colour scene; use trace_single for a single-wavelength one")
    _trace(scene, rays, rng_states, matrix_EB, gid_offset, n_rays, stats, per_ray_bounces, stream, variant,
           workgroups, single=False, chunk_order=chunk_order, num_iter=num_iter, gid_blocks=gid_blocks,
           gid_block_rays=gid_block_rays, debug=debug, grid_sqrt_k=grid_sqrt_k, windows=windows, fate=fate,
           replicas=replicas, expected=expected, footprint=footprint, hits=hits, paths=paths, select=select,
           visits=visits, stokes=stokes)


def new_stats(device) -> torch.Tensor:
    """A zeroed int64 device tensor laid out as ``wgrt_trace_stats``."""
    return torch.zeros(STATS_LEN, dtype=torch.int64, device=device)


def check_stats(stats: torch.Tensor) -> None:
    """Raise if a fused launch gave up a hand-off (``wgrt_trace_stats.handoff_giveups``): the
    eyebox grid and RNG states of that call are then wrong.  Warn (``luts.EnerUnderflowWarning``, a
    ``LUTPrecisionWarning``) if traces were decided in the ener-underflow regime
    (``wgrt_trace_stats.libm_rays``, ABI 7): their paths depend on the libm's last bits, so they may
    differ from a CPU run of the reference.  Synchronises on ``stats``."""
    st = stats.cpu()
    g = int(st[STAT.handoff_giveups])
    if g:
        raise WgrtError(f"{g} fused-launch traces gave up waiting for their ray's previous trace "
                        "(hand-off failure; results of this call are invalid)")
    lm = int(st[STAT.libm_rays]) if st.numel() > STAT.libm_rays else 0
    if lm:
        import warnings
        from .luts import EnerUnderflowWarning
        warnings.warn(f"{lm} traces reached the ener-underflow regime (a guard product ener * e below 2^-1000, "
                      "GRTF:1020): their decisions hang on the last bits of cos / sin / atan2, so they may differ "
                      "from the reference run on another libm (wgrt_trace_stats.libm_rays)",
                      EnerUnderflowWarning, stacklevel=2)


def reserve(scene: Scene, n_rays: int, num_iter: int = 1, stream=None) -> None:
    """Pre-allocate the Jones-vector variants' launch scratch for up to ``n_rays`` rays x
    ``num_iter`` chained traces on ``stream`` (``wgrt_scene_reserve``): later launches within
    those sizes neither allocate nor synchronise."""
    device = torch.device("cuda", scene.device)
    check(load().wgrt_scene_reserve(scene.handle, int(n_rays), int(num_iter),
                                    ctypes.c_void_p(_stream_handle(device, stream))), "wgrt_scene_reserve")


def trace_single(scene: Scene, rays: dict, rng_states: torch.Tensor, matrix_EB: torch.Tensor | None,
                 gid_offset: int = 0, n_rays: int | None = None, stats: torch.Tensor | None = None,
                 per_ray_bounces: torch.Tensor | None = None, stream=None, variant: int = VARIANT_AUTO,
                 workgroups: int = 0, chunk_order: torch.Tensor | None = None, num_iter: int = 1,
                 gid_blocks: torch.Tensor | None = None, gid_block_rays: int = 0, debug: dict | None = None,
                 grid_sqrt_k: float = 0.0, windows=None, fate: torch.Tensor | None = None, replicas: int = 0,
                 expected: bool = False, footprint=None, hits=None, paths=None, select=None, visits=None,
                 stokes=None) -> None:
    """One launch of the single-wavelength kernel (``process_rays_kernel_pro``, GRTF:419-831)
    through ``wgrt_trace_single_ex``: no ``lmd_num`` column (ignored if present),
    matrix_EB [NY, NX, 80, 120], branch guard ener * efficiency > 1e-15.  The scene must be
    a single-wavelength one (``Scene.from_geometry(..., wavelength=l)`` or 3-D LUTs).  ``windows``, ``fate``,
    ``replicas``, ``expected``, ``footprint``, ``hits``, ``paths``, ``select``, ``visits``, ``stokes``: as ``trace_fullcolor``."""
    if not scene.single_lambda:
        raise ValueError("trace_single needs a single-wavelength scene (Scene.from_geometry(..., wavelength=l))")
    _trace(scene, rays, rng_states, matrix_EB, gid_offset, n_rays, stats, per_ray_bounces, stream, variant,
           workgroups, single=True, chunk_order=chunk_order, num_iter=num_iter, gid_blocks=gid_blocks,
           gid_block_rays=gid_block_rays, debug=debug, grid_sqrt_k=grid_sqrt_k, windows=windows, fate=fate,
           replicas=replicas, expected=expected, footprint=footprint, hits=hits, paths=paths, select=select,
           visits=visits, stokes=stokes)


MAX_REPLICAS = 64   # WGRT_MAX_REPLICAS (include/wgrt.h)


def _replica_count(replicas) -> int:
    """``replicas`` as the count of replica tables: 0 for none (0, 1 or None), else 2 .. MAX_REPLICAS."""
    B = int(replicas or 0)
    if B in (0, 1):
        return 0
    if not 2 <= B <= MAX_REPLICAS:
        raise ValueError(f"replicas must be 0, 1 or 2 .. {MAX_REPLICAS}, got {B}")
    return B


class WindowPlan:
    """The plan of the trace's window-table sink (``wgrt_window_plan``): a binary pupil ``mask`` (default
    ``pupil_mask()``) and the eye-position steps (8 / 12), uploaded to ``device`` once.  ``W = 1 + npy * npx``
    is the table's width (57 by default); ``new_table(scene)`` a zeroed float64 ``[n_slabs, W]`` table on the
    scene's device, in the layout of ``eyebox_window_sums``; ``new_table(scene, replicas=B)`` the zeroed
    ``[B, n_slabs, W]`` replica tables of ``trace_*(replicas=B)``.  A mask with a tap other than 0 or 1 raises
    (``eyebox_window_sums`` serves it from a grid)."""

    def __init__(self, mask=None, step_y: int = 8, step_x: int = 12, device: int = 0):
        from .AR_system_evaluation_functions import _square_mask
        self.mask = _square_mask(mask)
        self.ms, self.step_y, self.step_x, self.device = int(self.mask.shape[0]), int(step_y), int(step_x), int(device)
        self._h = None
        L = load()
        h = ctypes.c_void_p()
        check(L.wgrt_window_plan_create(self.mask.ctypes.data, self.ms, self.step_y, self.step_x, self.device,
                                        ctypes.byref(h)), "wgrt_window_plan_create")
        self._h = h
        self.W = int(L.wgrt_window_plan_width(h))

    @property
    def handle(self):
        if self._h is None:
            raise WgrtError("window plan destroyed")
        return self._h

    def new_table(self, scene: Scene, replicas: int = 0) -> torch.Tensor:
        if scene.device != self.device:
            raise ValueError(f"the plan is on device {self.device}, the scene on device {scene.device}")
        n_slabs = scene.num_lmd * scene.ny * scene.nx
        B = _replica_count(replicas)
        return torch.zeros(((B,) if B else ()) + (n_slabs, self.W), dtype=torch.float64,
                           device=torch.device("cuda", scene.device))

    def close(self):
        if getattr(self, "_h", None) is not None:
            load().wgrt_window_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FOOTPRINT_CHANNELS = ("R0", "R1", "R2", "R3", "R4", "R5", "lost", "eyebox", "beside_eyebox")   # wgrt_footprint_channel_name


class FootprintPlan:
    """The plan of the footprint maps (``wgrt_footprint_plan``; ``trace_*(footprint=(fp, map))``): a rectangle of the
    plate from ``(x0, y0)`` in ``nx_cells`` x ``ny_cells`` cells of ``cell_x`` x ``cell_y`` mm.  A point counts into
    cell ``ix = floor((x - x0) / cell_x)``, ``iy = floor((y - y0) / cell_y)`` and is dropped outside the rectangle.
    Cell sizes must be > 0 and finite, the origin finite, the cell counts 1 .. 4096 (``ValueError`` otherwise; the
    check is the library's, ``wgrt_footprint_plan_validate``).  ``new_map(scene)``: a zeroed int64
    ``[num_lmd, 9, ny_cells, nx_cells]`` map on the scene's device."""

    def __init__(self, x0: float, y0: float, cell_x: float, cell_y: float, nx_cells: int, ny_cells: int):
        self.x0, self.y0, self.cell_x, self.cell_y = float(x0), float(y0), float(cell_x), float(cell_y)
        self.nx_cells, self.ny_cells = int(nx_cells), int(ny_cells)
        if not (-2 ** 31 <= self.nx_cells < 2 ** 31 and -2 ** 31 <= self.ny_cells < 2 ** 31):
            raise ValueError("nx_cells / ny_cells must be 1 .. 4096")
        L = load()
        if L.wgrt_footprint_plan_validate(ctypes.byref(self.c_plan())) != 0:
            raise ValueError(L.wgrt_last_error().decode())

    def c_plan(self):
        return _lib.FootprintPlanC(self.x0, self.y0, self.cell_x, self.cell_y, self.nx_cells, self.ny_cells)

    @classmethod
    def for_scene(cls, geom, cells=(256, 256)):
        """The plan of ``cells = (H, W)`` cells over the bounding box of ``geom.eff_reg1`` grown by one cell on every
        side: every counted draw lies inside ``eff_reg1`` or its 1e-12 edge band, so nothing is dropped."""
        H, W = int(cells[0]), int(cells[1])
        if H < 3 or W < 3:
            raise ValueError("for_scene needs at least 3 x 3 cells (one on every side of the plate's box)")
        box = np.asarray(geom.eff_reg1, dtype=np.float64)
        (xmin, ymin), (xmax, ymax) = box.min(axis=0), box.max(axis=0)
        cx, cy = (xmax - xmin) / (W - 2), (ymax - ymin) / (H - 2)
        return cls(xmin - cx, ymin - cy, cx, cy, W, H)

    def map_shape(self, scene) -> tuple:
        return (int(scene.num_lmd), len(FOOTPRINT_CHANNELS), self.ny_cells, self.nx_cells)

    def new_map(self, scene: Scene) -> torch.Tensor:
        return torch.zeros(self.map_shape(scene), dtype=torch.int64, device=torch.device("cuda", scene.device))

    def as_dict(self) -> dict:
        return {"x0": self.x0, "y0": self.y0, "cell_x": self.cell_x, "cell_y": self.cell_y,
                "nx_cells": self.nx_cells, "ny_cells": self.ny_cells}


def footprint_bin(fp: FootprintPlan, x, y, l, channel, num_lmd: int, out=None) -> np.ndarray:
    """The footprint sink on the host (``wgrt_footprint_bin_host``; numpy arrays, no GPU needed) through the kernels'
    binning rule: point i adds 1 to ``out[l[i], channel[i], iy, ix]``; a point outside the plan, with a non-finite
    coordinate, or with ``l`` / ``channel`` out of range is dropped.  Adds into ``out`` (C-contiguous int64
    ``[num_lmd, 9, ny_cells, nx_cells]``) when given."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    l = np.ascontiguousarray(np.broadcast_to(np.asarray(l, dtype=np.int32), x.shape))
    channel = np.ascontiguousarray(np.broadcast_to(np.asarray(channel, dtype=np.int32), x.shape))
    if x.ndim != 1 or y.shape != x.shape:
        raise ValueError("x, y must be 1-D arrays of one length")
    shape = (int(num_lmd), len(FOOTPRINT_CHANNELS), fp.ny_cells, fp.nx_cells)
    if out is None:
        out = np.zeros(shape, dtype=np.int64)
    elif out.dtype != np.int64 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous int64 array of shape {shape}")
    check(load().wgrt_footprint_bin_host(ctypes.byref(fp.c_plan()), x.ctypes.data, y.ctypes.data, l.ctypes.data,
                                         channel.ctypes.data, x.shape[0], int(num_lmd), out.ctypes.data),
          "wgrt_footprint_bin_host")
    return out


HIT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("gid", "<i8"), ("tile", "<u4"), ("flags", "<u4")])   # wgrt_hit
HIT_MAX_TAG = 65535


class HitListOverflow(WgrtError):
    """A hit list counted more out-couplings than it has room for (``check_hits``)."""


def hit_inside(records) -> np.ndarray:
    """Per record: inside its FoV's eyebox rectangle (flag bit 0; fate reason 3, else reason 4)."""
    return (records["flags"] & 1).astype(bool)


def hit_tag(records) -> np.ndarray:
    """Per record: the tag of the call that appended it (flag bits 16..31)."""
    return (records["flags"] >> 16).astype(np.int64)


def hit_lmn(records, nx: int, ny: int):
    """Per record: ``(l, m, n)`` of its tile index ``(l * nx + m) * ny + n``."""
    t = records["tile"].astype(np.int64)
    return t // (int(nx) * int(ny)), t // int(ny) % int(nx), t % int(ny)


def sort_hits(records) -> np.ndarray:
    """The records sorted by ``(tag, gid)``, which is unique per record."""
    return records[np.lexsort((records["gid"], hit_tag(records)))]


class _RecordList:
    """What ``HitList`` and ``PathList`` share: the record buffer, a uint8 ``[capacity, 32]`` device tensor, the device
    counter the launches add to, and the reading of both.  A subclass names its records: their numpy dtype, the
    library's struct (whose size ``<struct>_bytes()`` gives), the noun and unit of its overflow message and that
    message's exception class."""
    _dtype = _struct = _noun = _unit = _overflow = None

    def __init__(self, capacity: int, device=0):
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise ValueError("capacity must be >= 0")
        if int(getattr(load(), self._struct + "_bytes")()) != self._dtype.itemsize:
            raise WgrtError(f"the library's {self._struct} is not 32 bytes")
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.buffer = torch.zeros((self.capacity, self._dtype.itemsize), dtype=torch.uint8, device=self.device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    def clear(self) -> None:
        self.counter.zero_()

    def count(self) -> int:
        return int(self.counter.cpu()[0])

    def stored(self) -> int:
        return min(self.count(), self.capacity)

    def raw(self) -> np.ndarray:
        """The stored records in the buffer's order."""
        n = self.stored()
        return self.buffer[:n].cpu().numpy().reshape(-1).view(self._dtype).copy()

    def check_overflow(self) -> None:
        """Raise the list's overflow exception if it counted more records than it stores.  Synchronises."""
        n = self.count()
        if n > self.capacity:
            raise self._overflow(f"the {self._noun} counted {n} {self._unit} but has room for {self.capacity}: "
                                 f"a capacity of {n} would have sufficed")


class HitList(_RecordList):
    """A hit list (``wgrt_hit`` records; ``trace_*(hits=(hit_list, tag))``): the record buffer, a uint8
    ``[capacity, 32]`` device tensor, and the device counter the launches add to.  ``count()`` is the number of
    out-couplings so far (stored or not), ``stored()`` is ``min(count, capacity)``; both synchronise.  ``records()``
    is the stored records as a numpy structured array (``HIT_DTYPE``: ``x, y, gid, tile, flags``) sorted by
    ``(tag, gid)``; ``hit_inside``, ``hit_tag`` and ``hit_lmn`` decode them.  ``grid(scene, H, W, ranges=None)`` bins
    the stored records on the device into a float32 ``[num_lmd, ny, nx, H, W]`` grid (``wgrt_hits_grid``): over the
    scene's eyebox ranges the records inside their rectangle, over ``ranges`` (``[nx, ny, 4]``: xmin, xmax, ymin, ymax
    per FoV) those inside the caller's -- at ``(80, 120)`` over the scene's, ``matrix_EB`` of the same launches bit for
    bit.  ``clear()`` zeroes the counter."""
    _dtype, _struct, _noun, _unit, _overflow = HIT_DTYPE, "wgrt_hit", "hit list", "out-couplings", HitListOverflow

    def records(self) -> np.ndarray:
        return sort_hits(self.raw())

    def grid(self, scene: Scene, H: int, W: int, ranges=None, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if torch.device("cuda", scene.device) != self.device:
            raise ValueError(f"the hit list is on {self.device}, the scene on device {scene.device}")
        H, W = int(H), int(W)
        if not (1 <= H <= 4096 and 1 <= W <= 4096):
            raise ValueError("H and W must be 1 .. 4096")
        shape = tuple(scene.eb_shape()[:-2]) + (H, W)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=self.device)
        else:
            _as_dev(out, torch.float32, "grid", self.device)
            if tuple(out.shape) != shape:
                raise ValueError(f"grid shape {tuple(out.shape)} != {shape}")
        r = None
        if ranges is not None:
            r = torch.as_tensor(np.ascontiguousarray(ranges, dtype=np.float64)).to(self.device) \
                if not isinstance(ranges, torch.Tensor) else ranges
            _as_dev(r, torch.float64, "ranges", self.device, scene.nx * scene.ny * 4)
        check(load().wgrt_hits_grid(scene.handle, self.buffer.data_ptr(), self.stored(), r.data_ptr() if r is not None else None,
                                    H, W, out.data_ptr(), ctypes.c_void_p(_stream_handle(self.device, stream))),
              "wgrt_hits_grid")
        return out

    def _for_scene(self, scene: Scene) -> int:
        """The stored record count for a reduction that needs the whole list: raises ``HitListOverflow`` for a list that
        counted more than it stores (a re-weighted table of a truncated list is silently wrong).  Synchronises."""
        if torch.device("cuda", scene.device) != self.device:
            raise ValueError(f"the hit list is on {self.device}, the scene on device {scene.device}")
        self.check_overflow()
        return self.stored()

    def source_counts(self, scene: Scene, R: int, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The stored records counted per entry class on the device (``wgrt_hits_source_counts``): int64
        ``[num_lmd, 2, R]``, ``[l, 0, r]`` the out-couplings at wavelength ``l`` of the rays with block index
        ``r = gid mod R`` inside their FoV's eyebox rectangle, ``[l, 1, r]`` those beside it.  ``R``: rays per FoV x
        wavelength block.  Adds into ``out`` when given.  Raises ``HitListOverflow`` for a list that overflowed."""
        R = int(R)
        if R < 1:
            raise ValueError("R must be >= 1 rays per block")
        n = self._for_scene(scene)
        shape = (scene.num_lmd, 2, R)
        if out is None:
            out = torch.zeros(shape, dtype=torch.int64, device=self.device)
        else:
            _as_dev(out, torch.int64, "out", self.device)
            if tuple(out.shape) != shape:
                raise ValueError(f"out shape {tuple(out.shape)} != {shape}")
        check(load().wgrt_hits_source_counts(scene.handle, self.buffer.data_ptr(), n, R, out.data_ptr(),
                                             ctypes.c_void_p(_stream_handle(self.device, stream))),
              "wgrt_hits_source_counts")
        return out

    def reweight_sources(self, scene: Scene, plan: WindowPlan, weights, out: torch.Tensor | None = None,
                         sums: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The window tables of K projector pupils from the stored records, without a re-trace
        (``wgrt_hits_reweight_sources``): ``weights`` float64 ``[K, R]`` (an array or a tensor; ``source_weights`` makes
        them), ``weights[k, r]`` the relative radiance of entry class ``r = gid mod R`` in source k, finite and in
        ``[0, 1024]``.  Returns float64 ``[K, n_slabs, W]``: table k is the table the launches would have left had every
        ray of class r carried ``weights[k, r]``; a row of ones gives their window table bit for bit.  ``sums``: int64
        ``[K, 2, num_lmd]``, the weights' sum and sum of squares over the depositing records in quanta of 2^-32
        (``ess_of_quanta``).  ``out`` and ``sums`` are added to when given.  Raises ``HitListOverflow`` for a list
        that overflowed."""
        if plan.device != scene.device:
            raise ValueError(f"the plan is on device {plan.device}, the scene on device {scene.device}")
        n = self._for_scene(scene)
        w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64))
        if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1 or w.dtype != torch.float64:
            raise ValueError("weights must be float64 [K >= 1, R >= 1]: one value per source and entry class")
        w = w.to(self.device).contiguous()
        if not bool((torch.isfinite(w) & (w >= 0) & (w <= SOURCE_MAX_WEIGHT)).all()):
            raise ValueError(f"weights must be finite and in [0, {SOURCE_MAX_WEIGHT:g}]")
        K, R = int(w.shape[0]), int(w.shape[1])
        n_slabs = scene.num_lmd * scene.ny * scene.nx
        for name, t, dtype, shape in (("out", out, torch.float64, (K, n_slabs, plan.W)),
                                      ("sums", sums, torch.int64, (K, 2, scene.num_lmd))):
            if t is not None:
                _as_dev(t, dtype, name, self.device)
                if tuple(t.shape) != shape:
                    raise ValueError(f"{name} shape {tuple(t.shape)} != {shape}")
        if out is None:
            out = torch.zeros((K, n_slabs, plan.W), dtype=torch.float64, device=self.device)
        check(load().wgrt_hits_reweight_sources(scene.handle, plan.handle, self.buffer.data_ptr(), n, w.data_ptr(), R, K,
                                                out.data_ptr(), sums.data_ptr() if sums is not None else None,
                                                ctypes.c_void_p(_stream_handle(self.device, stream))),
              "wgrt_hits_reweight_sources")
        return out


SOURCE_MAX_WEIGHT = 1024.0   # csrc/wgrt_sources.h


def hits_source_counts_host(records, nx: int, ny: int, num_lmd: int, R: int, out=None) -> np.ndarray:
    """``HitList.source_counts`` on the host (``wgrt_hits_source_counts_host``; numpy arrays, no GPU needed): int64
    ``[num_lmd, 2, R]``.  Adds into ``out`` when given."""
    rec = np.ascontiguousarray(records, dtype=HIT_DTYPE)
    shape = (int(num_lmd), 2, int(R))
    if int(R) < 1:
        raise ValueError("R must be >= 1 rays per block")
    if out is None:
        out = np.zeros(shape, dtype=np.int64)
    elif out.dtype != np.int64 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous int64 array of shape {shape}")
    check(load().wgrt_hits_source_counts_host(int(nx), int(ny), int(num_lmd), rec.ctypes.data, rec.shape[0], int(R),
                                              out.ctypes.data), "wgrt_hits_source_counts_host")
    return out


def hits_reweight_sources_host(records, weights, nx: int, ny: int, num_lmd: int, scene_ranges, mask=None, step_y: int = 8,
                               step_x: int = 12, out=None, sums=None):
    """``HitList.reweight_sources`` on the host (``wgrt_hits_reweight_sources_host``; numpy arrays, no GPU needed)
    through the same rule and with the same bits: ``records`` a ``HIT_DTYPE`` array, ``weights`` float64 ``[K, R]``,
    ``scene_ranges`` the scene's ``eff_reg_FOV_range`` ``[nx, ny, 4]``, ``mask`` the plan's binary pupil mask (default
    ``pupil_mask()``).  Returns ``(tables, sums)``, float64 ``[K, num_lmd * ny * nx, W]`` and int64
    ``[K, 2, num_lmd]``; both are added to when given."""
    from .AR_system_evaluation_functions import _square_mask
    rec = np.ascontiguousarray(records, dtype=HIT_DTYPE)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError("weights must be [K >= 1, R >= 1]: one value per source and entry class")
    rg = np.ascontiguousarray(scene_ranges, dtype=np.float64)
    if rg.shape != (int(nx), int(ny), 4):
        raise ValueError(f"scene_ranges must have shape {(int(nx), int(ny), 4)}")
    m = _square_mask(mask)
    K, R = w.shape
    shape = (K, int(num_lmd) * int(ny) * int(nx), _window_width(m, step_y, step_x))
    if out is None:
        out = np.zeros(shape, dtype=np.float64)
    elif out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous float64 array of shape {shape}")
    if sums is None:
        sums = np.zeros((K, 2, int(num_lmd)), dtype=np.int64)
    elif sums.dtype != np.int64 or not sums.flags.c_contiguous or sums.shape != (K, 2, int(num_lmd)):
        raise ValueError(f"sums must be a C-contiguous int64 array of shape {(K, 2, int(num_lmd))}")
    check(load().wgrt_hits_reweight_sources_host(int(nx), int(ny), int(num_lmd), rg.ctypes.data, m.ctypes.data, m.shape[0],
                                                 int(step_y), int(step_x), rec.ctypes.data, rec.shape[0], w.ctypes.data,
                                                 R, K, out.ctypes.data, sums.ctypes.data),
          "wgrt_hits_reweight_sources_host")
    return out, sums


SOURCE_KEYS = ("centre", "diameter", "sigma", "te", "tm", "weights")


def check_sources(sources, R: int) -> list:
    """What ``source_weights`` can check without the entry points: ``sources`` as a list of dicts (a ``[K, R]`` array
    becomes K dicts of explicit ``weights``), or ``ValueError`` naming the source -- an unknown key, ``weights`` beside
    another key or of another length than R, a weight, ``te`` or ``tm`` that is negative or not finite, a ``diameter``
    or ``sigma`` that is not positive and finite, a ``centre`` that is not a finite ``[x, y]``."""
    R = int(R)
    if R < 2 or R % 2:
        raise ValueError(f"sources need an even number R >= 2 of rays per block (half TE, half TM), got {R}")
    if isinstance(sources, (dict, str)) or not hasattr(sources, "__len__") or len(sources) == 0:
        raise ValueError(f"sources must be a non-empty list of dicts or a [K, R] array, got {sources!r}")
    if not all(isinstance(s, dict) for s in sources):
        try:
            arr = np.asarray(sources, dtype=np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.ndim != 2 or arr.shape[1] != R:
            raise ValueError(f"sources must be a list of dicts or a [K, {R}] array of weights")
        sources = [{"weights": row} for row in arr]
    out = []
    for k, s in enumerate(sources):
        unknown = sorted(str(key) for key in set(s) - set(SOURCE_KEYS))
        if unknown:
            raise ValueError(f"source {k}: unknown key(s) {unknown}; the keys are {list(SOURCE_KEYS)}")
        try:
            if "weights" in s:
                if len(s) > 1:
                    raise ValueError(f"source {k}: 'weights' excludes the other keys")
                w = np.array(s["weights"], dtype=np.float64)
                if w.shape != (R,):
                    raise ValueError(f"source {k}: weights must hold {R} values, got shape {w.shape}")
                if not (np.isfinite(w).all() and (w >= 0).all()):
                    raise ValueError(f"source {k}: a weight is negative or not finite")
                out.append({"weights": w})
                continue
            d = {}
            if "centre" in s:
                c = np.asarray(s["centre"], dtype=np.float64)
                if c.shape != (2,) or not np.isfinite(c).all():
                    raise ValueError(f"source {k}: centre must be a finite [x, y], got {s['centre']!r}")
                d["centre"] = [float(c[0]), float(c[1])]
            for key in ("diameter", "sigma"):
                if key in s:
                    if isinstance(s[key], bool) or not (np.isfinite(float(s[key])) and float(s[key]) > 0):
                        raise ValueError(f"source {k}: {key} must be positive and finite, got {s[key]!r}")
                    d[key] = float(s[key])
            for key in ("te", "tm"):
                if key in s:
                    if isinstance(s[key], bool) or not (np.isfinite(float(s[key])) and float(s[key]) >= 0):
                        raise ValueError(f"source {k}: the factor {key} must be non-negative and finite, got {s[key]!r}")
                    d[key] = float(s[key])
            out.append(d)
        except TypeError as e:
            raise ValueError(f"source {k}: {e}") from e
    return out


def source_weights(points, R: int, sources) -> np.ndarray:
    """The weights of K projector pupils for ``HitList.reweight_sources``: float64 ``[K, R]``.  ``points``: the entry
    points ``[R / 2, 2]`` the rays were built from (entry class r starts at ``points[r mod (R / 2)]`` and is TE for
    ``r < R / 2``, TM otherwise).  ``sources``: a list of dicts, or a ``[K, R]`` array of explicit weights.  ``{}`` is the
    nominal source, the uniformly filled in-coupler with half the rays TE and half TM.  Keys: ``centre`` ``[x, y]``
    (default: the centroid of ``points``); ``diameter``, a hard circular stop about the centre (weight 0 outside);
    ``sigma``, a Gaussian apodisation ``exp(-d^2 / (2 sigma^2))`` of the distance d from the centre; ``te`` / ``tm``,
    non-negative factors on the two halves (default 1 and 1); ``weights``, an explicit ``[R]`` array, which excludes
    the other keys.  Every row is scaled to mean 1 over its R classes, so the tables' divisor stays ``R * num_iter`` and
    efficiencies are per unit of projector power.  An unknown key, a negative or non-finite value, a source of zero total
    weight or a weight above 1024 after scaling raises ``ValueError`` naming the source."""
    R = int(R)
    sources = check_sources(sources, R)
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape != (R // 2, 2) or not np.isfinite(pts).all():
        raise ValueError(f"points must be a finite [R / 2, 2] array, got shape {pts.shape} for R = {R}")
    out = np.empty((len(sources), R), dtype=np.float64)
    for k, s in enumerate(sources):
        if "weights" in s:
            w = np.array(s["weights"], dtype=np.float64)
        else:
            centre = np.asarray(s.get("centre", pts.mean(axis=0)), dtype=np.float64)
            d2 = ((pts - centre) ** 2).sum(axis=1)
            w = np.ones(R // 2, dtype=np.float64)
            if "diameter" in s:
                w = np.where(d2 <= (float(s["diameter"]) / 2) ** 2, w, 0.0)
            if "sigma" in s:
                w = w * np.exp(-d2 / (2 * float(s["sigma"]) ** 2))
            w = np.concatenate([float(s.get("te", 1.0)) * w, float(s.get("tm", 1.0)) * w])
        total = w.sum()
        if not total > 0:
            raise ValueError(f"source {k}: the source has zero total weight (nothing is emitted)")
        w = w * (R / total)
        if w.max() > SOURCE_MAX_WEIGHT:
            raise ValueError(f"source {k}: a weight is {w.max():g} after scaling to mean 1, above {SOURCE_MAX_WEIGHT:g}: "
                             f"the source keeps too small a part of the {R} entry classes")
        out[k] = w
    return out


def source_map(points, counts, H: int, W: int):
    """The entrance-pupil map on the host: ``(delivered, launched)``.  ``delivered`` int64 ``[num_lmd, 2, H, W]``: per
    wavelength and input polarisation (0 TE, 1 TM), the out-couplings inside the eyebox (``counts[:, 0]`` of
    ``HitList.source_counts``, int64 ``[num_lmd, 2, R]``) of the rays that entered in each cell; ``launched`` int64
    ``[H, W]``: the entry points per cell (each launches one ray per FoV, wavelength, polarisation and iteration).  The
    cells cover the bounding box of ``points`` ``[R / 2, 2]``, ``FootprintPlan``'s rule ``ix = floor((x - x0) / cell_x)``,
    ``iy = floor((y - y0) / cell_y)``, with the box's upper edges counted into the last cell, so that nothing is dropped."""
    pts = np.asarray(points, dtype=np.float64)
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    H, W = int(H), int(W)
    if not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError("H and W must be 1 .. 4096")
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1 or not np.isfinite(pts).all():
        raise ValueError("points must be a finite [R / 2, 2] array")
    P = pts.shape[0]
    if c.ndim != 3 or c.shape[1] != 2 or c.shape[2] != 2 * P:
        raise ValueError(f"counts must be [num_lmd, 2, {2 * P}], got shape {c.shape}")
    (x0, y0), (x1, y1) = pts.min(axis=0), pts.max(axis=0)
    cx, cy = (x1 - x0) / W or 1.0, (y1 - y0) / H or 1.0
    ix = np.minimum(np.floor((pts[:, 0] - x0) / cx).astype(np.int64), W - 1)
    iy = np.minimum(np.floor((pts[:, 1] - y0) / cy).astype(np.int64), H - 1)
    cell = iy * W + ix
    launched = np.bincount(cell, minlength=H * W).astype(np.int64).reshape(H, W)
    inside = c[:, 0].astype(np.int64).reshape(c.shape[0], 2, P)          # [l, TE / TM, point]
    delivered = np.zeros((c.shape[0], 2, H * W), dtype=np.int64)
    for l in range(c.shape[0]):
        for p in range(2):
            np.add.at(delivered[l, p], cell, inside[l, p])
    return delivered.reshape(c.shape[0], 2, H, W), launched


def check_hits(hit_list: HitList) -> None:
    """Raise ``HitListOverflow`` if the list counted more out-couplings than it stores.  Synchronises."""
    hit_list.check_overflow()


def hits_grid_host(records, nx: int, ny: int, num_lmd: int, scene_ranges, H: int, W: int, ranges=None,
                   out=None) -> np.ndarray:
    """``HitList.grid`` on the host (``wgrt_hits_grid_host``; numpy arrays, no GPU needed) through the same rule:
    ``records`` a ``HIT_DTYPE`` array, ``scene_ranges`` the scene's ``eff_reg_FOV_range`` ``[nx, ny, 4]``.  Adds into
    ``out`` (C-contiguous float32 ``[num_lmd, ny, nx, H, W]``) when given."""
    rec = np.ascontiguousarray(records, dtype=HIT_DTYPE)
    sr = np.ascontiguousarray(scene_ranges, dtype=np.float64)
    if sr.size != int(nx) * int(ny) * 4:
        raise ValueError("scene_ranges must be [nx, ny, 4]")
    cr = None
    if ranges is not None:
        cr = np.ascontiguousarray(ranges, dtype=np.float64)
        if cr.size != int(nx) * int(ny) * 4:
            raise ValueError("ranges must be [nx, ny, 4]")
    shape = (int(num_lmd), int(ny), int(nx), int(H), int(W))
    if out is None:
        if not all(1 <= v <= 4096 for v in shape[3:]):
            raise ValueError("H and W must be 1 .. 4096")
        out = np.zeros(shape, dtype=np.float32)
    elif out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
    # (records are 16-B aligned in the library's eyes: numpy allocations are)
    check(load().wgrt_hits_grid_host(int(nx), int(ny), int(num_lmd), sr.ctypes.data, rec.ctypes.data, rec.shape[0],
                                     cr.ctypes.data if cr is not None else None, int(H), int(W), out.ctypes.data),
          "wgrt_hits_grid_host")
    return out


PATH_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("gid", "<i8"), ("step", "<u4"), ("flags", "<u4")])   # wgrt_path_vertex
PATH_MAX_TAG = 65535
PATH_KINDS = {0: "draw", 1: "end_left_plate", 2: "draw_lost", 3: "draw_eyebox", 4: "draw_beside_eyebox", 5: "end_oc_miss"}


class PathListOverflow(WgrtError):
    """A path list counted more records than it has room for (``check_paths``)."""


def path_state(records) -> np.ndarray:
    """Per record: the state R0..R5 the ray is in (flag bits 0..2; 4 after the R3 -> R4 switch)."""
    return (records["flags"] & 7).astype(np.int64)


def path_kind(records) -> np.ndarray:
    """Per record: its kind (flag bits 4..7; ``PATH_KINDS``): 0 / 2 / 3 / 4 a draw, 1 / 5 an end record."""
    return (records["flags"] >> 4 & 15).astype(np.int64)


def path_lmd(records) -> np.ndarray:
    """Per record: the wavelength index of its ray (flag bits 8..15)."""
    return (records["flags"] >> 8 & 255).astype(np.int64)


def path_tag(records) -> np.ndarray:
    """Per record: the tag of the call that appended it (flag bits 16..31)."""
    return (records["flags"] >> 16).astype(np.int64)


def sort_paths(records) -> np.ndarray:
    """The records sorted by ``(tag, gid, step)``, which is unique per record."""
    return records[np.lexsort((records["step"], records["gid"], path_tag(records)))]


def path_polylines(records) -> dict:
    """``{tag: {gid: float64 [k, 2]}}``: every ray's records in step order as the points of its polyline after the
    start point (the draws' positions, then the end record's if the trace has one)."""
    rec = sort_paths(np.asarray(records, dtype=PATH_DTYPE))
    out: dict = {}
    if not len(rec):
        return out
    tag = path_tag(rec)
    first = np.flatnonzero(np.r_[True, (tag[1:] != tag[:-1]) | (rec["gid"][1:] != rec["gid"][:-1])])
    xy = np.stack([rec["x"], rec["y"]], axis=1)
    for a, b in zip(first, np.r_[first[1:], len(rec)]):
        out.setdefault(int(tag[a]), {})[int(rec["gid"][a])] = xy[a:b].copy()
    return out


class PathList(_RecordList):
    """A path list (``wgrt_path_vertex`` records; ``trace_*(paths=(path_list, tag), select=mask)``), the twin of
    ``HitList``: the record buffer, a uint8 ``[capacity, 32]`` device tensor, and the device counter the launches add
    to.  ``count()`` is the number of records so far (stored or not), ``stored()`` is ``min(count, capacity)``; both
    synchronise.  ``records()`` is the stored records as a numpy structured array (``PATH_DTYPE``: ``x, y, gid, step,
    flags``) sorted by ``(tag, gid, step)``; ``path_state``, ``path_kind``, ``path_lmd`` and ``path_tag`` decode them.
    ``footprint(scene, fp, out=None)`` adds the stored records on the device into an int64 footprint map of plan
    ``fp`` (``wgrt_paths_footprint``): of launches with ``select=None``, ``trace_*(footprint=...)``'s map of the same
    launches bit for bit; of a fate-selected list, the footprint of those rays alone.  ``polylines()``:
    ``path_polylines`` of the stored records.  ``clear()`` zeroes the counter; ``reserve(capacity)`` grows the buffer,
    keeping the stored records (a ray leaves at most its bounces + 1 records: a first pass's ``per_ray_bounces`` bound
    the room a selection needs)."""

    _dtype, _struct, _noun, _unit, _overflow = PATH_DTYPE, "wgrt_path_vertex", "path list", "records", PathListOverflow

    def reserve(self, capacity: int) -> None:
        """Room for at least ``capacity`` records: a larger buffer takes the stored records' place, in their order (the
        counter is the same tensor as before).  Nothing happens when the list is large enough.  Synchronises."""
        capacity = int(capacity)
        if capacity <= self.capacity:
            return
        n = self.stored()
        buffer = torch.zeros((capacity, PATH_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        buffer[:n] = self.buffer[:n]
        self.buffer, self.capacity = buffer, capacity

    def records(self) -> np.ndarray:
        return sort_paths(self.raw())

    def polylines(self) -> dict:
        return path_polylines(self.raw())

    def footprint(self, scene: Scene, fp: FootprintPlan, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if torch.device("cuda", scene.device) != self.device:
            raise ValueError(f"the path list is on {self.device}, the scene on device {scene.device}")
        if not isinstance(fp, FootprintPlan):
            raise TypeError("footprint(scene, FootprintPlan)")
        if out is None:
            out = fp.new_map(scene)
        else:
            _as_dev(out, torch.int64, "map", self.device)
            if tuple(out.shape) != fp.map_shape(scene):
                raise ValueError(f"map shape {tuple(out.shape)} != {fp.map_shape(scene)}")
        check(ops().paths_footprint(self.buffer, self.stored(), int(scene.num_lmd), fp.x0, fp.y0, fp.cell_x, fp.cell_y,
                                    fp.nx_cells, fp.ny_cells, out, _stream_handle(self.device, stream)),
              "wgrt_paths_footprint")
        return out


def check_paths(path_list: PathList) -> None:
    """Raise ``PathListOverflow`` if the list counted more records than it stores.  Synchronises."""
    path_list.check_overflow()


def paths_footprint_host(records, fp: FootprintPlan, num_lmd: int, out=None) -> np.ndarray:
    """``PathList.footprint`` on the host (``wgrt_paths_footprint_host``; numpy arrays, no GPU needed) through the same
    rule: ``records`` a ``PATH_DTYPE`` array.  Adds into ``out`` (C-contiguous int64 ``[num_lmd, 9, ny_cells,
    nx_cells]``) when given."""
    rec = np.ascontiguousarray(records, dtype=PATH_DTYPE)
    if rec.ndim != 1:
        raise ValueError("records must be a 1-D PATH_DTYPE array")
    if not 1 <= int(num_lmd) <= 256:
        raise ValueError("num_lmd must be 1 .. 256")
    shape = (int(num_lmd), len(FOOTPRINT_CHANNELS), fp.ny_cells, fp.nx_cells)
    if out is None:
        out = np.zeros(shape, dtype=np.int64)
    elif out.dtype != np.int64 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous int64 array of shape {shape}")
    check(load().wgrt_paths_footprint_host(rec.ctypes.data, rec.shape[0], int(num_lmd), ctypes.byref(fp.c_plan()),
                                           out.ctypes.data), "wgrt_paths_footprint_host")
    return out


VISIT_END_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("gid", "<i8"), ("tile", "<u4"), ("flags", "<u4")])   # wgrt_visit_end
VISIT_INSIDE, VISIT_OUT = 1, 2   # wgrt_visit_end.flags: bit 0 inside the FoV's eyebox rectangle, bit 1 out-coupled


def visit_channels(scene) -> list:
    """The names of a scene's visit channels in index order (csrc/wgrt_visits.h; ``scene``: anything with
    ``n_fc_slices`` and ``n_oc_slices``, or the pair itself): ``ic.b1, ic.b2`` the in-coupling event's two branches,
    ``r0.b1 .. r1.b2`` the in-coupler states', ``r2[i].b1/.b2`` and ``r3[i].b1/.b2`` in fold-coupler slice i,
    ``r4[i].b1/.b2/.b3`` and ``r5[i].b1/.b2/.b3`` in out-coupler slice i (``b3``: the out-coupling) --
    ``6 + 4 n_fc_slices + 6 n_oc_slices`` of them."""
    nfc, noc = (scene if isinstance(scene, (tuple, list)) else (scene.n_fc_slices, scene.n_oc_slices))
    names = ["ic.b1", "ic.b2", "r0.b1", "r0.b2", "r1.b1", "r1.b2"]
    for i in range(int(nfc)):
        names += [f"r{r}[{i}].b{b}" for r in (2, 3) for b in (1, 2)]
    for i in range(int(noc)):
        names += [f"r{r}[{i}].b{b}" for r in (4, 5) for b in (1, 2, 3)]
    return names


def _lnscale(names, scales, device=None):
    """``scales`` -- ``{channel name: s}`` or a length-C array / tensor of s -- as float64 ``log s`` per channel."""
    if isinstance(scales, dict):
        ln = np.zeros(len(names), dtype=np.float64)
        for k, v in scales.items():
            if k not in names:
                raise ValueError(f"{k!r} is not a visit channel of this scene")
            if not (float(v) > 0.0 and np.isfinite(float(v))):
                raise ValueError(f"the scale of {k!r} must be positive and finite, got {v!r}")
            ln[names.index(k)] = np.log(float(v))
        out = torch.from_numpy(ln)
    else:
        out = torch.as_tensor(scales, dtype=torch.float64).detach().cpu().reshape(-1)
        if out.numel() != len(names):
            raise ValueError(f"scales must name channels or hold {len(names)} values, got {out.numel()}")
        if not bool((out > 0).all()) or not bool(torch.isfinite(out).all()):
            raise ValueError("every scale must be positive and finite")
        out = out.log()
    return out if device is None else out.to(device)


def _lnscale_many(names, scales) -> torch.Tensor:
    """K designs -- a list of ``{channel name: s}`` dicts (an empty dict: every scale 1) or a ``[K, C]`` array / tensor of
    s -- as a float64 ``[K, C]`` host tensor of ``log s``, each row through ``_lnscale`` (the same refusals)."""
    if isinstance(scales, dict):
        raise ValueError("scales must be a list of {channel: s} dicts or a [K, C] array, not one dict")
    if isinstance(scales, (list, tuple)) and all(isinstance(d, dict) for d in scales):
        rows = list(scales)
    else:
        a = torch.as_tensor(scales, dtype=torch.float64).detach().cpu()
        if a.dim() != 2 or a.shape[1] != len(names):
            raise ValueError(f"scales must be a list of dicts or have shape [K, {len(names)}], got {tuple(a.shape)}")
        rows = list(a)
    if not rows:
        raise ValueError("scales must hold at least one design")
    return torch.stack([_lnscale(names, r) for r in rows]).contiguous()


def tolerance_scales(channels, sigma: float, n_designs: int, seed: int = 0, select=None) -> np.ndarray:
    """The scales of a tolerance ensemble, float64 ``[n_designs, C]``: row 0 all ones (the nominal design); in the other
    rows ``ln s_c ~ N(0, sigma^2)`` independently for every selected channel, drawn from ``np.random.default_rng(seed)``,
    and exactly 1 for the others.  ``channels``: the names (``visit_channels``); ``select``: ``fnmatch`` patterns over them
    (e.g. ``["r4[*].b3", "r5[*].b3"]``; None: every channel)."""
    import fnmatch
    channels = list(channels)
    if not (float(sigma) > 0.0 and np.isfinite(float(sigma))):
        raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
    if isinstance(n_designs, bool) or int(n_designs) != n_designs or int(n_designs) < 2:
        raise ValueError(f"n_designs must be >= 2 (the nominal design and one drawn), got {n_designs!r}")
    on = np.ones(len(channels), dtype=bool)
    if select is not None:
        on[:] = False
        for pat in ([select] if isinstance(select, str) else list(select)):
            # (brackets name a slice here, not a character class: only * and ? are wildcards)
            hit = np.array([fnmatch.fnmatchcase(n, pat.replace("[", "[[]")) for n in channels], dtype=bool)
            if not hit.any():
                raise ValueError(f"the pattern {pat!r} matches no channel")
            on |= hit
    out = np.ones((int(n_designs), len(channels)), dtype=np.float64)
    draws = np.random.default_rng(seed).normal(0.0, float(sigma), size=(int(n_designs) - 1, int(on.sum())))
    out[1:, on] = np.exp(draws)
    return out


class VisitTable:
    """The rows of visits launches (``trace_*(visits=(visit_table, slot))``; ``wgrt_trace_visits``): ``counts``, an int32
    ``[n_rows, C]`` device tensor (the library's uint32 words) that the launches add to, and ``ends``, a uint8
    ``[n_rows, 32]`` device tensor of ``wgrt_visit_end`` records (``VISIT_END_DTYPE``: ``x, y, gid, tile, flags``) that
    a counted ray writes when it out-couples.  ``clear()`` zeroes both (the launches never do).  ``channels``: the
    names.  ``sensitivity(plan, out=None)`` adds, for every delivered row, its counts into float64
    ``[C, n_slabs, W]`` tables (``wgrt_visits_sensitivity``): ``d table / d log s_c``, binned as the window table.
    ``reweight(plan, scales, out=None)`` adds the rows re-weighted by ``prod_c s_c^N_c`` into a float64
    ``[n_slabs, W]`` table (``wgrt_visits_reweight``; ``scales``: ``{channel name: s}`` or C values): the window table
    of the design whose channels are scaled so, without a re-trace; with every scale 1, the launches' own table bit for
    bit.  ``reweight_many(plan, scales, out=None, sums=None)`` does that for K designs in one pass over the rows
    (``wgrt_visits_reweight_many``): float64 ``[K, n_slabs, W]`` tables, table k the bytes of ``reweight``'s for design
    k, and the weights' sums as int64 quanta of 2^-32 ``[K, 2, num_lmd]`` (``ess_of_quanta``).  ``ess(scales)``: the
    effective sample size ``(sum w)^2 / sum w^2`` of those weights per wavelength (a float64
    device tensor ``[num_lmd]``; 0 where nothing was delivered).  ``host()``: ``(counts uint32, ends)`` as numpy."""

    def __init__(self, scene: Scene, n_rows: int, device=None):
        self.n_rows = int(n_rows)
        if self.n_rows < 0:
            raise ValueError("n_rows must be >= 0")
        self.scene = scene
        self.channels = visit_channels(scene)
        self.n_channels = len(self.channels)
        if int(load().wgrt_visit_channels(scene.handle)) != self.n_channels:
            raise WgrtError("the library's channel count differs from engine.visit_channels")
        device = scene.device if device is None else device
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        if self.device.type == "cuda" and self.device.index is None:   # "cuda": the current device, named
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device != torch.device("cuda", scene.device):
            raise ValueError(f"the visit table is on {self.device}, the scene on device {scene.device}")
        self.counts = torch.zeros((self.n_rows, self.n_channels), dtype=torch.int32, device=self.device)
        self.ends = torch.zeros((self.n_rows, VISIT_END_DTYPE.itemsize), dtype=torch.uint8, device=self.device)

    def clear(self) -> None:
        self.counts.zero_()
        self.ends.zero_()

    def host(self):
        return (self.counts.cpu().numpy().view(np.uint32).copy(),
                self.ends.cpu().numpy().reshape(-1).view(VISIT_END_DTYPE).copy())

    def _reduce(self, plan, lnscale, out, shape, stream):
        if plan.device != self.scene.device:
            raise ValueError(f"the plan is on device {plan.device}, the scene on device {self.scene.device}")
        if out is None:
            out = torch.zeros(shape, dtype=torch.float64, device=self.device)
        else:
            _as_dev(out, torch.float64, "out", self.device)
            if tuple(out.shape) != shape:
                raise ValueError(f"out shape {tuple(out.shape)} != {shape}")
        check(ops().visits_reduce(self.scene.handle.value, plan.handle.value, self.counts, self.ends, self.n_rows,
                                  lnscale, out, _stream_handle(self.device, stream)),
              "wgrt_visits_sensitivity" if lnscale is None else "wgrt_visits_reweight")
        return out

    def sensitivity(self, plan: WindowPlan, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        n_slabs = self.scene.num_lmd * self.scene.ny * self.scene.nx
        return self._reduce(plan, None, out, (self.n_channels, n_slabs, plan.W), stream)

    def reweight(self, plan: WindowPlan, scales, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        n_slabs = self.scene.num_lmd * self.scene.ny * self.scene.nx
        return self._reduce(plan, _lnscale(self.channels, scales, self.device), out, (n_slabs, plan.W), stream)

    def reweight_many(self, plan: WindowPlan, scales, out: torch.Tensor | None = None, sums: torch.Tensor | None = None,
                      stream=None):
        """``(tables, sums)`` for K designs from one pass over the rows (``wgrt_visits_reweight_many``): ``scales`` is a
        list of ``{channel name: s}`` dicts (an empty dict: the nominal design) or a ``[K, C]`` array or tensor of s;
        ``tables`` float64 ``[K, n_slabs, W]``, ``tables[k]`` the bytes of ``reweight(plan, scales[k])``; ``sums`` int64
        ``[K, 2, num_lmd]``, the weights' sum and sum of squares in quanta of 2^-32 (``ess_of_quanta``).  Both are added
        to when given."""
        if plan.device != self.scene.device:
            raise ValueError(f"the plan is on device {plan.device}, the scene on device {self.scene.device}")
        ln = _lnscale_many(self.channels, scales).to(self.device)
        K = ln.shape[0]
        n_slabs = self.scene.num_lmd * self.scene.ny * self.scene.nx
        for name, t, dtype, shape in (("out", out, torch.float64, (K, n_slabs, plan.W)),
                                      ("sums", sums, torch.int64, (K, 2, self.scene.num_lmd))):
            if t is not None:
                _as_dev(t, dtype, name, self.device)
                if tuple(t.shape) != shape:
                    raise ValueError(f"{name} shape {tuple(t.shape)} != {shape}")
        if out is None:
            out = torch.zeros((K, n_slabs, plan.W), dtype=torch.float64, device=self.device)
        if sums is None:
            sums = torch.zeros((K, 2, self.scene.num_lmd), dtype=torch.int64, device=self.device)
        check(ops().visits_reweight_many(self.scene.handle.value, plan.handle.value, self.counts, self.ends, self.n_rows,
                                         ln, out, sums, _stream_handle(self.device, stream)),
              "wgrt_visits_reweight_many")
        return out, sums

    def weight_sums(self, scales) -> torch.Tensor:
        """Float64 ``[2, num_lmd]``: per wavelength, the sum and the sum of squares of the delivered rows' weights
        ``prod_c s_c^N_c`` (torch, from the same rows; sums of several tables add)."""
        ln = _lnscale(self.channels, scales, self.device)
        ends = self.ends[:self.n_rows].view(torch.int32)   # [n_rows, 8]: x, y, gid (two words each), tile, flags
        on = (ends[:, 7] & VISIT_INSIDE) != 0
        w = torch.exp(self.counts[:self.n_rows][on].double() @ ln)
        l = (ends[on, 6].long() // (self.scene.nx * self.scene.ny)).clamp_(0, self.scene.num_lmd - 1)
        out = torch.zeros((2, self.scene.num_lmd), dtype=torch.float64, device=self.device)
        out[0].index_add_(0, l, w)
        out[1].index_add_(0, l, w * w)
        return out

    def ess(self, scales) -> torch.Tensor:
        return ess_of(self.weight_sums(scales))


def ess_of(sums) -> torch.Tensor:
    """The effective sample size ``(sum w)^2 / sum w^2`` per wavelength of ``VisitTable.weight_sums`` (0 where nothing
    was delivered)."""
    s1, s2 = sums[0], sums[1]
    return torch.where(s2 > 0, s1 * s1 / s2.clamp_min(1e-300), torch.zeros_like(s1))


def ess_of_quanta(sums):
    """The effective sample size ``s1^2 / s2`` per design and wavelength, float64 ``[K, num_lmd]``, of
    ``VisitTable.reweight_many``'s int64 ``[K, 2, num_lmd]`` sums (quanta of 2^-32; a tensor or an array, returned in
    kind; 0 where nothing was delivered)."""
    if isinstance(sums, torch.Tensor):
        s1, s2 = sums[:, 0].double() * 2.0 ** -32, sums[:, 1].double() * 2.0 ** -32
        return torch.where(s2 > 0, s1 * s1 / s2.clamp_min(1e-300), torch.zeros_like(s1))
    s = np.asarray(sums).astype(np.float64) * 2.0 ** -32
    return np.where(s[:, 1] > 0, s[:, 0] * s[:, 0] / np.maximum(s[:, 1], 1e-300), 0.0)


def _visits_host(fn, name, counts, ends, nx, ny, num_lmd, scene_ranges, plan_mask, step_y, step_x, shape, out, *more,
                 tail=()):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    ends = np.ascontiguousarray(ends, dtype=VISIT_END_DTYPE)
    if counts.ndim != 2 or ends.shape != (counts.shape[0],):
        raise ValueError("counts must be [n_rows, C] and ends [n_rows]")
    rg = np.ascontiguousarray(scene_ranges, dtype=np.float64)
    if rg.shape != (int(nx), int(ny), 4):
        raise ValueError(f"scene_ranges must have shape {(int(nx), int(ny), 4)}")
    mask = np.ascontiguousarray(plan_mask, dtype=np.float32)
    if out is None:
        out = np.zeros(shape, dtype=np.float64)
    elif out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError(f"out must be a C-contiguous float64 array of shape {shape}")
    check(fn(int(nx), int(ny), int(num_lmd), counts.shape[1], rg.ctypes.data, mask.ctypes.data, mask.shape[0],
             int(step_y), int(step_x), counts.ctypes.data, ends.ctypes.data, counts.shape[0], *more, out.ctypes.data, *tail), name)
    return out


def _window_width(mask, step_y, step_x):
    ms = np.asarray(mask).shape[0]
    return 1 + ((80 - ms) // int(step_y) + 1) * ((120 - ms) // int(step_x) + 1)


def visits_sensitivity_host(counts, ends, nx: int, ny: int, num_lmd: int, scene_ranges, mask, step_y: int = 8,
                            step_x: int = 12, out=None) -> np.ndarray:
    """``VisitTable.sensitivity`` on the host (``wgrt_visits_sensitivity_host``; numpy arrays, no GPU needed) through the
    same rule: ``counts`` uint32 ``[n_rows, C]``, ``ends`` a ``VISIT_END_DTYPE`` array, ``scene_ranges`` the scene's
    ``eff_reg_FOV_range`` ``[nx, ny, 4]``, ``mask`` the plan's binary pupil mask.  Adds into ``out`` (float64
    ``[C, num_lmd * ny * nx, W]``) when given."""
    C = np.asarray(counts).shape[1]
    shape = (C, int(num_lmd) * int(ny) * int(nx), _window_width(mask, step_y, step_x))
    return _visits_host(load().wgrt_visits_sensitivity_host, "wgrt_visits_sensitivity_host", counts, ends, nx, ny, num_lmd,
                        scene_ranges, mask, step_y, step_x, shape, out)


def visits_reweight_host(counts, ends, lnscale, nx: int, ny: int, num_lmd: int, scene_ranges, mask, step_y: int = 8,
                         step_x: int = 12, out=None) -> np.ndarray:
    """``VisitTable.reweight`` on the host (``wgrt_visits_reweight_host``): ``lnscale`` float64 ``[C]``, ``log s`` per
    channel.  Adds into ``out`` (float64 ``[num_lmd * ny * nx, W]``) when given."""
    ln = np.ascontiguousarray(lnscale, dtype=np.float64)
    if ln.shape != (np.asarray(counts).shape[1],):
        raise ValueError("lnscale must hold one value per channel")
    shape = (int(num_lmd) * int(ny) * int(nx), _window_width(mask, step_y, step_x))
    return _visits_host(load().wgrt_visits_reweight_host, "wgrt_visits_reweight_host", counts, ends, nx, ny, num_lmd,
                        scene_ranges, mask, step_y, step_x, shape, out, ln.ctypes.data)


def visits_reweight_many_host(counts, ends, lnscale, nx: int, ny: int, num_lmd: int, scene_ranges, mask, step_y: int = 8,
                              step_x: int = 12, out=None, sums=None):
    """``VisitTable.reweight_many`` on the host (``wgrt_visits_reweight_many_host``): ``lnscale`` float64 ``[K, C]``,
    ``log s`` per design and channel.  Returns ``(tables, sums)``, float64 ``[K, num_lmd * ny * nx, W]`` and int64
    ``[K, 2, num_lmd]``; both are added to when given."""
    ln = np.ascontiguousarray(lnscale, dtype=np.float64)
    if ln.ndim != 2 or ln.shape[0] < 1 or ln.shape[1] != np.asarray(counts).shape[1]:
        raise ValueError("lnscale must be [K >= 1, C]: one value per design and channel")
    K = ln.shape[0]
    if sums is None:
        sums = np.zeros((K, 2, int(num_lmd)), dtype=np.int64)
    elif sums.dtype != np.int64 or not sums.flags.c_contiguous or sums.shape != (K, 2, int(num_lmd)):
        raise ValueError(f"sums must be a C-contiguous int64 array of shape {(K, 2, int(num_lmd))}")
    shape = (K, int(num_lmd) * int(ny) * int(nx), _window_width(mask, step_y, step_x))
    out = _visits_host(load().wgrt_visits_reweight_many_host, "wgrt_visits_reweight_many_host", counts, ends, nx, ny,
                       num_lmd, scene_ranges, mask, step_y, step_x, shape, out, ln.ctypes.data, K,
                       tail=(sums.ctypes.data,))
    return out, sums


STOKES_SCALE = 2.0 ** 30   # quanta per unit of a normalised Stokes parameter (csrc/wgrt_stokes.h)


class StokesTable:
    """The Stokes window tables of ``trace_*(stokes=table)`` (``wgrt_trace_stokes``; csrc/wgrt_stokes.h): ``tables``, an
    int64 ``[3, n_slabs, plan.W]`` device tensor that the launches add to -- table k holds, entry by entry beside the
    window table ``N`` of the same launches, the sum of ``q_k = rint(s_k * 2^30)`` over the out-couplings ``N`` counts,
    ``s_1 .. s_3`` the normalised Stokes parameters of the out-coupled field in the TE / TM basis of that FoV's
    out-coupled order.  ``clear()`` zeroes them (the launches never do); ``raw()`` is the tensor; ``host()`` a numpy
    copy.  ``AR_system_evaluation_functions.polarisation_from_stokes(N, S)`` turns them into mean Stokes vectors."""

    def __init__(self, scene: Scene, plan: WindowPlan, device=None):
        self.scene, self.plan = scene, plan
        device = scene.device if device is None else device
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        if self.device.type == "cuda" and self.device.index is None:   # "cuda": the current device, named
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device != torch.device("cuda", scene.device):
            raise ValueError(f"the Stokes tables are on {self.device}, the scene on device {scene.device}")
        if plan.device != scene.device:
            raise ValueError(f"the plan is on device {plan.device}, the scene on device {scene.device}")
        self.tables = torch.zeros((3, scene.num_lmd * scene.ny * scene.nx, plan.W), dtype=torch.int64, device=self.device)

    def clear(self) -> None:
        self.tables.zero_()

    def raw(self) -> torch.Tensor:
        return self.tables

    def host(self) -> np.ndarray:
        return self.tables.cpu().numpy().copy()


def stokes_quanta(a: complex, b: complex) -> tuple:
    """The three quanta ``(q1, q2, q3)`` of the field with complex TE amplitude ``a`` and TM amplitude ``b``, through the
    code the kernels run (``wgrt_stokes_quanta_host``; no GPU needed)."""
    q = (ctypes.c_int32 * 3)()
    a, b = complex(a), complex(b)
    load().wgrt_stokes_quanta_host(a.real, a.imag, b.real, b.imag, q)
    return int(q[0]), int(q[1]), int(q[2])


def _debug_opts(debug: dict | None):
    if not debug:
        return None
    unknown = set(debug) - {f for f, _ in DebugOpts._fields_} - {"timeline"}
    if unknown:
        raise ValueError(f"unknown debug options {sorted(unknown)}")
    d = DebugOpts()
    for k, v in debug.items():
        if k == "timeline":
            if v is not None:
                if v.dtype != torch.int64 or not v.is_contiguous() or v.numel() % 8:
                    raise ValueError("timeline must be a contiguous int64 tensor of 8 words per wave")
                d.timeline = ctypes.c_void_p(v.data_ptr())
                d.timeline_waves = v.numel() // 8
        elif k != "timeline_waves":
            setattr(d, k, v)
    return d


def _read_columns(rays, rng_states, n_rays, single, device):
    """The columns a launch reads (READ_COLUMNS, no ``lmd_num`` for a single-wavelength scene), validated
    together with ``rng_states`` and the ray count: ``(cols, N)``.  ``_trace`` and ``shadow`` share it."""
    x = rays["x"]
    N = x.numel() if n_rays is None else int(n_rays)
    if N < 0 or N > x.numel():
        raise ValueError(f"n_rays={N} out of range for {x.numel()} rays")
    cols = {}
    for k in READ_COLUMNS:
        if single and k == "lmd_num":
            continue
        if k not in rays:
            raise ValueError(f"missing ray column {k!r}")
        cols[k] = _as_dev(rays[k], torch.float32, k, device, x.numel())
    if rng_states.dtype not in (torch.int32, torch.uint32):
        raise TypeError(f"rng_states must be uint32 (or an int32 view), got {rng_states.dtype}")
    _as_dev(rng_states, rng_states.dtype, "rng_states", device, x.numel())
    return cols, N


_SINKS = ("fate", "replicas", "expected", "footprint", "hits", "paths", "visits", "stokes")   # the keywords, as they arrived


def _launch_sink(fate, replicas, expected, footprint, hits, paths, select, visits, num_iter, chain, stokes=None):
    """The one rule of what a launch may be asked to leave besides the grid and the window table, checked before any
    payload is looked at: a launch has at most one sink -- ``fate``, ``expected``, ``footprint``, ``hits``, ``paths``
    (with its ``select``), ``visits`` or ``stokes``; ``replicas`` describe the window table and go alone or with ``expected``; and
    a launch with a sink or with replicas is a single one (``num_iter == 1``), not a chain's.  Returns ``(kind,
    payload, B)``: the sink's keyword and its value (``"replicas"`` and ``B`` for replica tables alone, ``None, None``
    for none) and the replica count (0: the one table).  Raises ``ValueError`` otherwise."""
    B = _replica_count(replicas)
    values = (fate, B or None, expected or None, footprint, hits, paths, visits, stokes)
    given = [k for k, v in zip(_SINKS, values) if v is not None]
    if len(given) > 1 and given != ["replicas", "expected"]:
        raise ValueError(f"a launch has at most one sink: {given[-1]}= takes no {' or '.join(given[:-1])}")
    if select is not None and paths is None:
        raise ValueError("select= chooses the rays of a paths launch: it needs paths=(PathList, tag)")
    if not given:
        return None, None, 0
    kind = given[-1]
    if int(num_iter) > 1:
        raise ValueError(f"{kind}= needs num_iter == 1: a sink and replica tables are filled by single launches")
    if chain:
        raise ValueError(f"a chain takes no {kind} launches: trace them with single launches")
    return kind, values[_SINKS.index(kind)], B


# kind -> the operator and, from the sink's validated payload, the arguments it adds to trace_windows'
_SINK_OPS = {
    None: ("trace_windows", lambda _: ()),
    "fate": ("trace_fate", lambda fate: (fate,)),
    "replicas": ("trace_replicas", lambda B: (B,)),
    "footprint": ("trace_footprint", lambda p: (p[0].x0, p[0].y0, p[0].cell_x, p[0].cell_y, p[0].nx_cells, p[0].ny_cells,
                                                p[1])),
    "hits": ("trace_hits", lambda p: (p[0].buffer, p[0].capacity, p[0].counter, int(p[1]))),
    "paths": ("trace_paths", lambda p: (p[0].buffer, p[0].capacity, p[0].counter, int(p[1]), p[2])),   # (list, tag, select)
    "visits": ("trace_visits", lambda p: (p[1], p[0].n_rows, p[0].counts, p[0].ends)),
    "stokes": ("trace_stokes", lambda t: (t.tables,)),
}


def _trace(scene, rays, rng_states, matrix_EB, gid_offset, n_rays, stats, per_ray_bounces, stream, variant,
           workgroups, single, chunk_order=None, num_iter=1, gid_blocks=None, gid_block_rays=0, debug=None,
           grid_sqrt_k=0.0, windows=None, chain=False, fate=None, replicas=0, expected=False, footprint=None,
           hits=None, paths=None, select=None, visits=None, stokes=None):
    kind, payload, B = _launch_sink(fate, replicas, expected, footprint, hits, paths, select, visits, num_iter, chain,
                                    stokes)
    device = torch.device("cuda", scene.device)
    # the sink's own payload (before anything is read or launched)
    if kind == "visits":
        visit_table, visit_slot = payload
        if not isinstance(visit_table, VisitTable):
            raise TypeError("visits=(VisitTable, slot)")
        if visit_table.device != device:
            raise ValueError(f"the visit table is on {visit_table.device}, expected {device}")
        if visit_table.n_channels != len(visit_channels(scene)):
            raise ValueError(f"the visit table has {visit_table.n_channels} channels, the scene "
                             f"{len(visit_channels(scene))}")
    elif kind in ("hits", "paths"):
        record_list, _ = payload
        if not isinstance(record_list, PathList if kind == "paths" else HitList):
            raise TypeError("paths=(PathList, tag)" if kind == "paths" else "hits=(HitList, tag)")
        if record_list.device != device:
            raise ValueError(f"the {record_list._noun} is on {record_list.device}, expected {device}")
        if kind == "paths" and int(scene.num_lmd) > 256:
            raise ValueError("a path record names at most 256 wavelengths: the scene has more")
    elif kind == "footprint":
        fp, fp_map = payload
        if not isinstance(fp, FootprintPlan):
            raise TypeError("footprint=(FootprintPlan, map)")
        _as_dev(fp_map, torch.int64, "footprint map", device)
        if tuple(fp_map.shape) != fp.map_shape(scene):
            raise ValueError(f"footprint map shape {tuple(fp_map.shape)} != {fp.map_shape(scene)}")
    elif kind == "stokes":
        if not isinstance(payload, StokesTable):
            raise TypeError("stokes=StokesTable")
        if payload.device != device:
            raise ValueError(f"the Stokes tables are on {payload.device}, expected {device}")
        if windows is None:
            raise ValueError("stokes= lies beside a window table: it needs windows=(plan, table)")
        if tuple(payload.tables.shape) != (3, scene.num_lmd * scene.ny * scene.nx, windows[0].W):
            raise ValueError(f"the Stokes tables' shape {tuple(payload.tables.shape)} != "
                             f"{(3, scene.num_lmd * scene.ny * scene.nx, windows[0].W)}")
    elif kind == "expected":
        if matrix_EB is not None:
            raise ValueError("expected=True takes no grid (matrix_EB=None): a float32 cell cannot hold the 2^-32 sums")
        if windows is None:
            raise ValueError("expected=True needs windows=(plan, table)")
    cols, N = _read_columns(rays, rng_states, n_rays, single, device)
    x = cols["x"]
    if matrix_EB is None and windows is None:
        raise ValueError("matrix_EB=None needs windows=(plan, table)")
    if matrix_EB is not None:
        _as_dev(matrix_EB, torch.float32, "matrix_EB", device)
        if tuple(matrix_EB.shape) != scene.eb_shape():
            raise ValueError(f"matrix_EB shape {tuple(matrix_EB.shape)} != {scene.eb_shape()}")
    if windows is not None:
        plan, table = windows
        _as_dev(table, torch.float64, "windows table", device)
        want = ((B,) if B else ()) + (scene.num_lmd * scene.ny * scene.nx, plan.W)
        if tuple(table.shape) != want:
            raise ValueError(f"windows table shape {tuple(table.shape)} != {want}")
    if stats is not None:
        _as_dev(stats, torch.int64, "stats", device, STATS_LEN)
    if per_ray_bounces is not None:
        if per_ray_bounces.dtype not in (torch.int32, torch.uint32):
            raise TypeError("per_ray_bounces must be uint32 / int32")
        _as_dev(per_ray_bounces, per_ray_bounces.dtype, "per_ray_bounces", device, x.numel())
    if kind == "fate":
        _as_dev(fate, torch.uint8, "fate", device, x.numel())
    if B and windows is None:
        raise ValueError("replicas need windows=(plan, table): a grid has no replicas")
    n_chunks = (N + CHUNK - 1) // CHUNK
    if chunk_order is not None:
        _as_dev(chunk_order, torch.int32, "chunk_order", device, n_chunks)
    if gid_blocks is not None:
        if gid_block_rays < 1:
            raise ValueError("gid_blocks needs gid_block_rays >= 1")
        _as_dev(gid_blocks, torch.int64, "gid_blocks", device, (N + gid_block_rays - 1) // gid_block_rays if N else None)
    if select is not None:
        if select.dtype == torch.bool:
            select = select.view(torch.uint8)
        _as_dev(select, torch.uint8, "select", device, N if N else None)
    if kind == "visits":
        if visit_slot is None:
            if N > visit_table.n_rows:
                raise ValueError(f"without slots ray i is counted into row i: {N} rays need {N} rows, the table has "
                                 f"{visit_table.n_rows}")
        else:
            _as_dev(visit_slot, torch.int32, "slot", device, x.numel())
            top = int(visit_slot[:N].max()) if N else -1   # (the device does not validate slots; synchronises)
            if top >= visit_table.n_rows:
                raise ValueError(f"slot.max() = {top} is not below the table's "
                                 f"{visit_table.n_rows} rows")
    dbg = _debug_opts(debug)
    # the launch: torch.ops.wgrt.trace (csrc/wgrt_torch.cpp) -> wgrt_trace_opts on the caller's stream; with a
    # window table torch.ops.wgrt.trace_windows -> wgrt_trace_windows
    args = (scene.handle.value, cols["x"], cols["y"], cols["m"], cols["n"], cols.get("lmd_num"),
            cols["te"], cols["tm"], cols["delta_phase"], rng_states, matrix_EB, stats, per_ray_bounces,
            N, int(gid_offset), _stream_handle(device, stream), 1 if single else 0, int(variant),
            int(workgroups), chunk_order, int(num_iter), gid_blocks,
            int(gid_block_rays) if gid_blocks is not None else 0,
            ctypes.addressof(dbg) if dbg is not None else 0, float(grid_sqrt_k))
    if chain:
        # torch.ops.wgrt.chain_begin -> wgrt_chain_begin: nothing is launched; the handle, and everything the
        # chain's launches will read or write (the side stream uses memory torch's allocator accounts to the
        # caller's stream, so the tensors must outlive the chain: TraceChain holds them until end)
        h = ops().chain_begin(*args, plan.handle.value if windows is not None else 0,
                              table if windows is not None else None)
        if h <= 0:   # the negated wgrt_status of the failure
            check(-h, "wgrt_chain_begin")
        return h, (args, dbg, windows)
    if kind is None and windows is None:
        status = ops().trace(*args)
    elif kind == "expected":   # no grid among its arguments
        status = ops().trace_expected(*args[:10], *args[11:], plan.handle.value, table, B)
    else:   # torch.ops.wgrt.trace_<kind> -> wgrt_trace_<kind>: trace_windows' arguments (plan 0, no table: the grid alone)
        if kind == "paths":
            payload = (*payload, select)
        op, own = _SINK_OPS[kind]
        status = getattr(ops(), op)(*args, plan.handle.value if windows is not None else 0,
                                    table if windows is not None else None, *own(payload))
    check(status, "wgrt_trace_single" if single else "wgrt_trace_fullcolor")


class TraceChain:
    """A chain of single traces of one batch (``wgrt_chain_begin`` / ``_step`` / ``_end``): each ``step()`` is one
    trace (``num_iter = 1``) and the chain leaves exactly what as many ``trace_fullcolor`` calls leave --
    ``rng_states``, ``matrix_EB`` / window table and ``stats``, bit for bit -- but consecutive launches run on two
    hardware queues, so one launch's drain is covered by the next one's bulk.  A context manager::

        with TraceChain(scene, rays, rng, eb, stats=stats) as ch:
            for _ in range(k):
                ch.step()

    Takes ``trace_fullcolor``'s arguments (no ``per_ray_bounces``).  Between ``__enter__`` and ``__exit__`` nothing
    else may touch ``rng_states``, ``matrix_EB``, the window table or ``stats`` on the stream; after ``__exit__``
    the stream is ordered after every step.

    ``gather=True`` (or a cap of 2 .. 64 steps) opts into ``wgrt_chain_gather``, for a caller that calls its steps back
    to back and reads nothing before the end: a step called while the stream is still busy with the chain's earlier
    launches is not enqueued but counted, and the count goes out as one fused launch when a later step finds the
    stream idle, at the cap, and at the end (``hold=True``: only at the cap and at the end).  Such a step's work
    starts no earlier than a later ``step()`` or the end, the stream's launch scratch grows to the cap (24 bytes per
    ray and step; 1 GiB by default) and stays, and ``stats``' ``replayed`` is the fused launches' count (a ray a launch
    abandons counts once in it): at most the plain launches'.  Everything else stays bit for bit.  ``report()`` says
    what an open chain has launched.

    The chain holds references to every tensor until it ends, and
    ``__exit__`` always ends it, also on an exception.  Steps that cannot be chained (the scene's learning
    launches, variant 1, ``chunk_order``, a debug timeline, a stream under capture) run as plain launches."""

    def __init__(self, scene: Scene, rays: dict, rng_states: torch.Tensor, matrix_EB: torch.Tensor | None,
                 gid_offset: int = 0, n_rays: int | None = None, stats: torch.Tensor | None = None, stream=None,
                 variant: int = VARIANT_AUTO, workgroups: int = 0, chunk_order: torch.Tensor | None = None,
                 gid_blocks: torch.Tensor | None = None, gid_block_rays: int = 0, debug: dict | None = None,
                 grid_sqrt_k: float = 0.0, windows=None, replicas: int = 0, expected: bool = False,
                 gather: bool | int = False, hold: bool = False, footprint=None, hits=None, paths=None, select=None,
                 visits=None, stokes=None):
        if scene.single_lambda:
            raise ValueError("TraceChain needs a full-colour scene")
        _launch_sink(None, replicas, expected, footprint, hits, paths, select, visits, 1, chain=True, stokes=stokes)
        self._h = 0
        self._step = ops().chain_step
        self._h, self._keep = _trace(scene, rays, rng_states, matrix_EB, gid_offset, n_rays, stats, None, stream,
                                     variant, workgroups, single=False, chunk_order=chunk_order, gid_blocks=gid_blocks,
                                     gid_block_rays=gid_block_rays, debug=debug, grid_sqrt_k=grid_sqrt_k,
                                     windows=windows, chain=True)
        self.steps = 0
        if gather:
            try:
                check(load().wgrt_chain_gather(ctypes.c_void_p(self._h), 0 if gather is True else int(gather),
                                               int(bool(hold))), "wgrt_chain_gather")
            except Exception:
                self.end()
                raise

    def step(self) -> None:
        if not self._h:
            raise WgrtError("the chain has ended")
        status = self._step(self._h)
        if status:
            check(status, "wgrt_chain_step")
        self.steps += 1

    def report(self) -> dict:
        """``wgrt_debug_chain_report``: steps, launches, fused launches, the largest launch, steps still pending."""
        if not self._h:
            raise WgrtError("the chain has ended")
        from ._lib import chain_report
        return chain_report(self._h)

    def end(self) -> None:
        h, self._h = self._h, 0
        if h:
            try:
                check(ops().chain_end(h), "wgrt_chain_end")
            finally:
                self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.end()
        return False

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def fold_replicas(table, stream=None):
    """The fold of replica window tables ``[B, n_slabs, W]`` (``trace_*(replicas=B)``): ``[1 + B, n_slabs, W]`` whose row
    0 is the sum of the replicas in ascending order -- the table a plain windows trace leaves -- and whose row
    ``1 + b`` is row 0 less replica ``b``, the leave-one-out tables of the jackknife.  A device tensor is folded on
    the device (``wgrt_window_replicas_fold``, asynchronous on ``stream``), a numpy array on the host
    (``wgrt_window_replicas_fold_host``, no GPU needed); both give the same bits."""
    L = load()
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.float64 or table.dim() != 3 or not table.is_contiguous():
            raise ValueError("replica tables must be a contiguous float64 [B, n_slabs, W] tensor")
        B = _replica_count(table.shape[0])
        if not B:
            raise ValueError(f"need 2 .. {MAX_REPLICAS} replicas, got {table.shape[0]}")
        out = torch.empty((1 + B,) + tuple(table.shape[1:]), dtype=torch.float64, device=table.device)
        with torch.cuda.device(table.device):
            check(L.wgrt_window_replicas_fold(ctypes.c_void_p(table.data_ptr()), B, table[0].numel(),
                                              ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(_stream_handle(table.device, stream))),
                  "wgrt_window_replicas_fold")
        return out
    t = np.ascontiguousarray(table, dtype=np.float64)
    if t.ndim != 3:
        raise ValueError("replica tables must have shape [B, n_slabs, W]")
    out = np.empty((1 + t.shape[0],) + t.shape[1:], dtype=np.float64)
    check(L.wgrt_window_replicas_fold_host(t.ctypes.data, t.shape[0], t[0].size, out.ctypes.data),
          "wgrt_window_replicas_fold_host")
    return out


# ---- where every ray ends: fate codes, their census and the loss budget (csrc/wgrt_fate.h states the code) ----
# The classes of ``loss_budget``: every fate code belongs to exactly one (reason, regions; the entry is region 9).
FATE_CLASSES = (("in_coupling_loss", 2, (9,)), ("left_in_coupler", 6, (9, 0, 1)), ("left_plate", 1, (0, 1, 2, 3, 4, 5)),
                ("lost_ic", 2, (0, 1)), ("lost_fc", 2, (2, 3)), ("lost_oc", 2, (4, 5)), ("eyebox", 3, (4, 5)),
                ("beside_eyebox", 4, (4, 5)), ("oc_miss", 5, (5,)), ("bounce_cap", 7, (0, 1, 2, 3, 4, 5)))


def fate_col(code: int) -> int:
    """Column of fate code ``code`` in a census row (``wgrt_fate_col``); raises for a code no trace can end with."""
    c = int(load().wgrt_fate_col(int(code)))
    if c < 0:
        raise ValueError(f"{code} is not a fate code")
    return c


def _fate_constant(name: str):
    L = load()
    if name == "FATE_COLS":
        return int(L.wgrt_fate_cols())
    if name == "FATE_REASONS":
        return {r: L.wgrt_fate_reason_name(r).decode() for r in range(1, 8)}
    return tuple(c for c in range(256) if L.wgrt_fate_col(c) >= 0)   # FATE_CODES


def __getattr__(name: str):
    # FATE_COLS, FATE_REASONS ({reason: name}) and FATE_CODES (the codes a trace can end with) come from the
    # library, so they are read when first used (importing this module needs no built library)
    if name in ("FATE_COLS", "FATE_REASONS", "FATE_CODES"):
        v = _fate_constant(name)
        globals()[name] = v
        return v
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def fate_census(scene: Scene, rays: dict, fate: torch.Tensor, table: torch.Tensor | None = None,
                stream=None) -> torch.Tensor:
    """Count the fate codes a trace left (``trace_*(fate=...)``) per tile (``wgrt_fate_census``): ray i with code c
    adds 1 to ``table[(l * ny + n) * nx + m, fate_col(c)]``, an int64 ``[n_slabs, FATE_COLS]`` device tensor in
    ``matrix_EB``'s slab order that is accumulated into when given (a zeroed one is made otherwise) and returned.
    ``rays``: the batch's ``m``, ``n`` (and, full colour, ``lmd_num``) columns.  Asynchronous on ``stream``."""
    device = torch.device("cuda", scene.device)
    fate = _as_dev(fate, torch.uint8, "fate", device)
    n = fate.numel()
    cols = {k: _as_dev(rays[k], torch.float32, k, device) for k in ("m", "n") + (() if scene.single_lambda else ("lmd_num",))}
    for k, v in cols.items():
        if v.numel() < n:
            raise ValueError(f"ray column {k!r} has {v.numel()} rays, fate has {n}")
    L = load()
    shape = (scene.num_lmd * scene.ny * scene.nx, int(L.wgrt_fate_cols()))
    if table is None:
        table = torch.zeros(shape, dtype=torch.int64, device=device)
    else:
        _as_dev(table, torch.int64, "table", device)
        if tuple(table.shape) != shape:
            raise ValueError(f"table shape {tuple(table.shape)} != {shape}")
    lmd = cols.get("lmd_num")
    check(L.wgrt_fate_census(ctypes.c_void_p(fate.data_ptr()), ctypes.c_void_p(cols["m"].data_ptr()),
                             ctypes.c_void_p(cols["n"].data_ptr()),
                             ctypes.c_void_p(lmd.data_ptr()) if lmd is not None else None, n, scene.nx, scene.ny,
                             scene.num_lmd, ctypes.c_void_p(table.data_ptr()),
                             ctypes.c_void_p(_stream_handle(device, stream))), "wgrt_fate_census")
    return table


def fate_census_host(fate, m, n, lmd_num, nx: int, ny: int, num_lmd: int, table=None) -> np.ndarray:
    """The census on the host (``wgrt_fate_census_host``; numpy arrays, no GPU needed): the same validity rule,
    tile index and column function as the device's.  ``lmd_num=None``: wavelength 0.  Adds into ``table`` (int64
    ``[num_lmd * ny * nx, FATE_COLS]``, C-contiguous) when given."""
    L = load()
    fate = np.ascontiguousarray(fate, dtype=np.uint8)
    cols = [np.ascontiguousarray(c, dtype=np.float32) if c is not None else None for c in (m, n, lmd_num)]
    if any(c is not None and c.shape[0] < fate.shape[0] for c in cols):
        raise ValueError("a tile index column is shorter than fate")
    if table is None:
        table = np.zeros((num_lmd * ny * nx, int(L.wgrt_fate_cols())), dtype=np.int64)
    elif table.dtype != np.int64 or not table.flags.c_contiguous:
        raise ValueError("table must be a C-contiguous int64 array")
    check(L.wgrt_fate_census_host(fate.ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data,
                                  cols[2].ctypes.data if cols[2] is not None else None, fate.shape[0], int(nx), int(ny),
                                  int(num_lmd), table.ctypes.data), "wgrt_fate_census_host")
    return table


def select_by_fate(fate: torch.Tensor, classes) -> torch.Tensor:
    """The ``select`` mask of a paths launch from the fate codes of a fate launch of the same batch and RNG states
    (``trace_*(fate=...)`` on a clone of the states): a uint8 device tensor, 1 where the ray's fate belongs to one of
    ``classes`` -- a class name of ``FATE_CLASSES`` (``"eyebox"``, ``"left_plate"``, ``"lost_fc"``, ...), a raw fate code
    (int), or a list / tuple of either.  The classes are ``loss_budget``'s, from the one table."""
    if isinstance(classes, (str, int, np.integer)):
        classes = [classes]
    by_name = {name: [10 * region + reason for region in regions] for name, reason, regions in FATE_CLASSES}
    lut = torch.zeros(256, dtype=torch.uint8)
    for c in classes:
        if isinstance(c, str):
            if c not in by_name:
                raise ValueError(f"{c!r} is not a fate class (one of {', '.join(by_name)})")
            codes = by_name[c]
        else:
            fate_col(int(c))   # (raises for a code no trace can end with)
            codes = [int(c)]
        lut[codes] = 1
    if fate.dtype != torch.uint8:
        raise TypeError("fate must be a uint8 tensor of fate codes")
    return lut.to(fate.device)[fate.long()]


def loss_budget(census, scene) -> dict:
    """The loss budget of a fate census (``fate_census``; a device tensor or a numpy array ``[n_slabs, FATE_COLS]``;
    ``scene``: anything with ``num_lmd``, ``nx``, ``ny``): where the traced rays ended, per wavelength and in total,
    in the classes of ``FATE_CLASSES`` -- ``in_coupling_loss`` (code 92: lost at the in-coupler's first diffraction),
    ``left_in_coupler`` (96, 06, 16: the second order walked out of the in-coupler), ``left_plate`` (reason 1),
    ``lost_ic`` / ``lost_fc`` / ``lost_oc`` (reason 2 in the in-coupler, fold-grating and out-coupler states),
    ``eyebox`` (reason 3), ``beside_eyebox`` (reason 4), ``oc_miss`` (55) and ``bounce_cap`` (reason 7).  Returns
    ``{"per_wavelength": [{"rays", "counts", "fractions"}, ...], "total": {...}, "eyebox": int64 [num_lmd, ny, nx]}``:
    ``counts`` are the integer class counts (they sum to ``rays``, the rays counted), ``fractions`` their shares of
    ``rays`` (summing to 1 up to the rounding of ten float64 quotients; all 0 when no ray was counted), and ``eyebox``
    the reason-3 count of every tile: the rays of that FoV and wavelength that reached its eyebox."""
    c = census.cpu().numpy() if isinstance(census, torch.Tensor) else np.asarray(census)
    nl, ny, nx = int(scene.num_lmd), int(scene.ny), int(scene.nx)
    c = c.reshape(nl, ny, nx, -1).astype(np.int64)
    cols = {name: [fate_col(10 * region + reason) for region in regions] for name, reason, regions in FATE_CLASSES}

    def entry(rows):   # rows: [..., FATE_COLS] -> one budget record
        tot = rows.reshape(-1, rows.shape[-1]).sum(axis=0)
        counts = {name: int(tot[k].sum()) for name, k in cols.items()}
        rays = int(tot.sum())
        assert rays == sum(counts.values()), "a census column outside every class"
        return {"rays": rays, "counts": counts,
                "fractions": {name: (v / rays if rays else 0.0) for name, v in counts.items()}}
    return {"per_wavelength": [entry(c[l]) for l in range(nl)], "total": entry(c),
            "eyebox": c[..., cols["eyebox"]].sum(axis=-1)}


def timeline_summary(buf, percentiles: bool = True) -> dict:
    """Summary of one launch's wave timeline (``debug=dict(timeline=buf)``: 8 int64 words per wave --
    start, queue exhausted, end (s_memrealtime, 100 MHz), passes, lane-passes, XCD, passes and
    lane-passes up to the queue running dry): when the work queue ran dry, when the waves ended,
    and the pass durations and lane occupancy before (bulk) and after (drain) -- where a single
    launch's time goes."""
    t = buf.cpu().numpy().reshape(-1, 8)
    t = t[t[:, 0] > 0]
    start, exh, end, passes, lanes, xcc, p_exh, l_exh = (t[:, k].astype(np.float64) for k in range(8))
    t0 = start.min()
    us = lambda v: (v - t0) / 100.0   # 100 MHz ticks -> us
    drain_passes = passes - p_exh
    last = us(end) >= np.percentile(us(end), 99)
    pc = lambda v, qs: [round(float(np.percentile(v, q)), 3) for q in qs]
    return {"waves": int(len(t)),
            "exhausted_us": pc(us(exh), (0, 50, 100)),
            "end_us": pc(us(end), (0, 50, 99, 100)),
            "drain_frac": round(float((us(end).max() - np.median(us(exh))) / max(us(end).max(), 1e-9)), 4),
            "bulk_us_per_pass": round(float(np.median(us(exh) / np.maximum(p_exh, 1))), 3),
            "drain_us_per_pass": round(float(np.median((end - exh) / 100.0 / np.maximum(drain_passes, 1))), 3),
            "bulk_lanes_per_pass": round(float(l_exh.sum() / max(p_exh.sum(), 1)), 2),
            "drain_lanes_per_pass": round(float((lanes - l_exh).sum() / max(drain_passes.sum(), 1)), 2),
            "last1pct_drain_passes": round(float(np.median(drain_passes[last])), 1),
            "last1pct_drain_us_per_pass": round(float(np.median(((end - exh) / 100.0 /
                                                                   np.maximum(drain_passes, 1))[last])), 3)}


def schedule_by_lifetime(per_ray_bounces, tile_of_ray, n_tiles: int | None = None):
    """Issue order of the 64-ray chunks for ``chunk_order``: the chunks whose rays belong to the
    (wavelength, FoV) tiles with the longest mean lifetime in a previous launch go first, so the
    rays that outlive the work queue come from short-lived tiles.  The kernel's work queue hands
    out chunk positions in stripes of 16 (stripe s on head s % 8, each head's stripes in
    increasing order, wgrt_trace.hip), so a global longest-first order is also longest-first on
    every head.  ``per_ray_bounces`` from an earlier launch of the same batch
    (``trace_*(per_ray_bounces=...)``), ``tile_of_ray`` any integer tile key per ray (e.g.
    ``(lmd_num * NX + m) * NY + n``).  Device tensors in, int32 device permutation out (a few
    small torch ops, no host sync).  A pure scheduling hint: results are unchanged (DESIGN.md
    §5.4: it measured within noise on C3)."""
    b = per_ray_bounces.to(torch.float32)
    key = tile_of_ray.to(torch.int64)
    nt = int(n_tiles) if n_tiles is not None else int(key.max().item()) + 1
    tot = torch.zeros(nt, dtype=torch.float32, device=b.device).index_add_(0, key, b)
    cnt = torch.zeros(nt, dtype=torch.float32, device=b.device).index_add_(0, key, torch.ones_like(b))
    mean = tot / cnt.clamp_min(1.0)
    N = b.numel()
    first = torch.arange(0, N, CHUNK, device=b.device)
    chunk_key = mean[key[first]]
    return torch.argsort(-chunk_key.to(torch.float64), stable=True).to(torch.int32)


def block_runs(block_list) -> list[tuple[int, int, int]]:
    """Runs of consecutive global block ids: ``(local_block_lo, global_block_lo, count)``."""
    ids = [int(v) for v in block_list]
    runs, i = [], 0
    while i < len(ids):
        j = i + 1
        while j < len(ids) and ids[j] == ids[j - 1] + 1:
            j += 1
        runs.append((i, ids[i], j - i))
        i = j
    return runs


def init_rays(points, num_fov_x: int, num_fov_y: int, lambdas, rays_per_fov: int, blocks=None,
              device="cuda", all_columns: bool = True, stream=None, block_list=None):
    """Build a ray batch on the device (``wgrt_rays_init``; replaces MAIN:59-115 and the RNG
    seeding at MAIN:158, bit-identical to ``rays.build_rays`` + ``rays.rng_seeds``).

    ``points``: the R/2 origins (numpy or torch float64 [R/2, 2]); ``blocks=(lo, hi)``
    builds FoV x wavelength blocks [lo, hi) only (one rank's shard, global ids from lo * R);
    ``block_list`` (any sequence of global block ids) builds those blocks back to back (an
    interleaved shard: local block j is global block block_list[j], RNG seeded with its global
    ids).  ``all_columns=False`` allocates only the eight columns the kernel reads.
    Returns ``(rays, rng_states)``: a dict of float32 tensors and an int32 view of the
    uint32 RNG states."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    R = int(rays_per_fov)
    lam = np.ascontiguousarray(list(lambdas), dtype=np.int32)
    nblk = num_fov_x * num_fov_y * len(lam)
    if block_list is not None:
        if blocks is not None:
            raise ValueError("give blocks or block_list, not both")
        ids = [int(v) for v in block_list]
        if any(not 0 <= v < nblk for v in ids):
            raise ValueError(f"block_list has ids outside [0, {nblk})")
        runs = block_runs(ids)
        nb = len(ids)
    else:
        lo, hi = (0, nblk) if blocks is None else (int(blocks[0]), int(blocks[1]))
        if not 0 <= lo <= hi <= nblk:
            raise ValueError(f"block range {blocks} outside [0, {nblk}]")
        runs, nb = [(0, lo, hi - lo)], hi - lo
    pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points, dtype=np.float64))
    pts = pts.to(device=device, dtype=torch.float64).contiguous()
    if tuple(pts.shape) != (R // 2, 2):
        raise ValueError(f"points must have shape ({R // 2}, 2), got {tuple(pts.shape)}")
    N = nb * R
    names = RAY_COLUMNS if all_columns else READ_COLUMNS
    rays = {k: torch.empty(N, dtype=torch.float32, device=device) for k in names}
    rng = torch.empty(N, dtype=torch.int32, device=device)
    for loc, glo, cnt in runs:
        off = loc * R * 4   # bytes into every 4-byte column
        cols = Rays(**{k: ctypes.c_void_p(v.data_ptr() + off) for k, v in rays.items()})
        check(load().wgrt_rays_init(ctypes.c_void_p(pts.data_ptr()), R, int(num_fov_x), int(num_fov_y),
                                    lam.ctypes.data_as(ctypes.c_void_p), len(lam), glo, glo + cnt,
                                    ctypes.byref(cols), ctypes.c_void_p(rng.data_ptr() + off),
                                    ctypes.c_void_p(_stream_handle(device, stream))),
              "wgrt_rays_init")
    return rays, rng


def classify_points(scene: Scene, xy: torch.Tensor, stream=None) -> torch.Tensor:
    """Per-point polygon membership bitmask through the scene's exact locator."""
    device = torch.device("cuda", scene.device)
    xy = _as_dev(xy, torch.float64, "xy", device)
    n = xy.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=device)
    check(load().wgrt_scene_classify(scene.handle, ctypes.c_void_p(xy.data_ptr()), n,
                                     ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(_stream_handle(device, stream))), "wgrt_scene_classify")
    return out


SHADOW_DEPTHS = ("[1,10)", "[10,30)", "[30,100)", "[100,300)", "[300,1000)", "[1000,inf)")


def shadow(scene: Scene, rays: dict, rng_states: torch.Tensor, gid_offset: int = 0, n_rays: int | None = None,
           per_ray_bounces: torch.Tensor | None = None, stream=None) -> dict:
    """Certification shadow of the Jones-vector lane (``wgrt_debug_shadow``): traces the rays with
    the reference's own arithmetic and measures, at every Monte-Carlo decision, how far the
    product lane's thresholds stray from the reference's relative to its certification bound.
    ``rng_states`` / ``per_ray_bounces`` are updated as one exact launch would.  Synchronous;
    returns the statistics as a dict (``max_ratio``, ``silent_flips``, ``uncertain``, ...)."""
    device = torch.device("cuda", scene.device)
    single = scene.single_lambda
    cols, N = _read_columns(rays, rng_states, n_rays, single, device)
    r = Rays(**{k: ctypes.c_void_p(v.data_ptr()) for k, v in cols.items()})
    nbytes = ctypes.sizeof(_lib.ShadowStats)
    buf = torch.zeros(nbytes // 8, dtype=torch.int64, device=device)
    check(load().wgrt_debug_shadow(scene.handle, ctypes.byref(r), N, int(gid_offset), int(single),
                                   ctypes.c_void_p(rng_states.data_ptr()),
                                   ctypes.c_void_p(per_ray_bounces.data_ptr()) if per_ray_bounces is not None else None,
                                   ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(_stream_handle(device, stream))),
          "wgrt_debug_shadow")
    host = buf.cpu().numpy()
    st = _lib.ShadowStats.from_buffer_copy(host.tobytes())
    return {"decisions": st.decisions, "uncertain": st.uncertain, "silent_flips": st.silent_flips,
            "bounces": st.bounces, "fallbacks": st.fallbacks, "max_ratio": st.max_ratio,
            "max_ratio32": st.max_ratio32,
            "max_ratio32_by_depth": dict(zip(SHADOW_DEPTHS, list(st.max_ratio_by_depth))),
            "decisions_by_depth": dict(zip(SHADOW_DEPTHS, [int(v) for v in st.decisions_by_depth])),
            "ratio32_hist_log10": {f"1e{b - 18}": int(v) for b, v in enumerate(st.ratio_hist) if v},
            "max_ener_ratio": st.max_ener_ratio, "max_amp": st.max_amp}


def selftest_math(a: torch.Tensor, b: torch.Tensor, stream=None) -> torch.Tensor:
    """Device sqrt, div, hypot_cr, atan2, sin, cos, wrap on (a, b) -> [7, n] float64."""
    n = a.numel()
    out = torch.empty((7, n), dtype=torch.float64, device=a.device)
    check(load().wgrt_selftest_math(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), n,
                                    ctypes.c_void_p(out.data_ptr()),
                                    ctypes.c_void_p(_stream_handle(a.device, stream))), "wgrt_selftest_math")
    return out


def expected_weight(e1: float, e2: float, e3: float, en1: float, en2: float, en3: float, threshold: float = 0.0) -> float:
    """The deposit ``q`` of one out-coupler interaction under the expected-value estimator (``trace_*(expected=True)``)
    through the code the kernels run (``wgrt_expected_weight_host``; no GPU needed): the out-coupling probability of
    the reference's branch chain for efficiencies ``e1, e2, e3`` and guard products ``en_k = ener * e_k`` against
    ``threshold``, rounded to a multiple of 2^-32."""
    return float(load().wgrt_expected_weight_host(e1, e2, e3, en1, en2, en3, threshold))


__all__ = ["StokesTable", "stokes_quanta", "STOKES_SCALE", "VisitTable", "visit_channels", "ess_of", "ess_of_quanta", "tolerance_scales", "visits_sensitivity_host", "visits_reweight_host", "visits_reweight_many_host", "VISIT_END_DTYPE", "Scene", "WindowPlan", "FootprintPlan", "footprint_bin", "FOOTPRINT_CHANNELS", "PathList", "PathListOverflow", "check_paths", "paths_footprint_host", "sort_paths", "path_polylines", "path_state", "path_kind", "path_lmd", "path_tag", "PATH_DTYPE", "PATH_KINDS", "select_by_fate", "HitList", "HitListOverflow", "check_hits", "hits_grid_host", "sort_hits", "hit_inside", "hit_tag", "hit_lmn", "HIT_DTYPE", "TraceChain", "fold_replicas", "expected_weight", "MAX_REPLICAS", "fate_census", "fate_census_host", "fate_col", "loss_budget", "FATE_CLASSES", "WgrtError", "TraceStats", "STAT", "STATS_LEN", "new_stats", "check_stats", "block_runs",
           "trace_fullcolor", "trace_single", "init_rays", "schedule_by_lifetime",
           "rays_to_device", "classify_points", "shadow", "selftest_math", "RAY_COLUMNS", "_lib"]
