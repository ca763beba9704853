"""Full-colour driver (reference ``gpu_ray_tracing_pro_fullColor.py``, MAIN:1-210).

Same flow as the reference script, on the MI355X kernel:

1. coupler geometry (``couplers_coor_full_color``, MAIN:19-25);
2. the seven RCWA LUTs -- the reference's ``.npy`` files when ``lut_dir`` is given
   (MAIN:28-34), otherwise the seeded synthetic set (the files are not available offline);
3. ray batch: ``num_rays_per_FoV / 2`` in-coupler origins shared by every FoV x wavelength
   block, TE then TM halves (MAIN:59-115), RNG seeds ``0x9E3779B9 * (gid + 1)`` (MAIN:158),
   laid out on the device by ``wgrt_rays_init``;
4. ``num_iter`` chained launches of the bounce kernel (MAIN:169-177), as one fused call
   (``num_iter`` traces per ray in one persistent launch; identical results) when a GPU traces
   at most ``FUSE_MAX_RAYS`` rays, else as separate launches (``fuse`` overrides), timed with HIP
   events (no JIT in the timed region, unlike the reference's wall clock);
5. efficiencies ``A = sum(EB) / N / num_iter``, ``eff_c = 3 * sum(A[lambda])`` (MAIN:186-192)
   and ``evaluation(EB / R / num_iter)`` (MAIN:197-198) -- on the host from the copied-back grid as the
   reference does, or (``eyebox="device"``, ``--eyebox device``) from the per-slab window sums one device pass
   leaves (``eyebox_window_sums``), without the grid leaving the GPU; with ``evaluate_on="device"``
   (``--evaluate device``) the table stays there too and the colour math runs in ``wgrt_eyebox_evaluate``; or
   (``eyebox="windows"``, ``--eyebox windows``) from the same table counted by the trace itself
   (``wgrt_trace_windows``), with no grid allocated at all;
   with ``budget=True`` (``--budget``) every launch also stores each ray's fate code, a census counts them per
   tile, and the loss budget -- where the rays that did not reach the eyebox went -- is printed per wavelength;
   with ``error_bars=B`` (``--error-bars B``, windows mode) the trace counts into ``B`` replica tables by ray id and
   every printed figure carries a jackknife standard error;
   with ``footprint=(H, W)`` (``--footprint HxW``) every launch also counts each interaction into a per-wavelength
   plate map -- where the light interacts, is lost and leaves (``wgrt_trace_footprint``);
   with ``paths="eyebox"`` (``--paths eyebox``; any fate class, or ``all``) the draws of the selected rays are kept as
   records -- which way that light went (``wgrt_trace_paths``) -- and reduced to a conditional footprint on request;
   with ``sensitivity=True`` (``--sensitivity``) the branches the delivered rays took are counted per channel
   (``wgrt_trace_visits``): which grating to change; with ``what_if={channel: scale}`` (``--what-if``) the same rays,
   re-weighted, give the figures of the scaled design without a re-trace; with ``designs=[...]`` (``--designs``) or
   ``tolerance=sigma`` (``--tolerance``) the same for K listed or randomly drawn designs in one pass
   (``wgrt_visits_reweight_many``): candidates side by side, or the band every figure lands in; with
   ``sources=[...]`` (``--sources``) the hit list, re-weighted by each ray's entry class, gives the figures of K
   projector pupils -- smaller, decentred, apodised, TE or TM -- from the one trace (``wgrt_hits_reweight_sources``);
6. the "Eyebox Center View.png" export (MAIN:199-203): the evaluated image at the first eye row,
   last eye column, as 8-bit RGB, rows flipped (``eyebox_center_view``, written without OpenCV).

The matplotlib plots (MAIN:213-237) are visual-only and not reproduced.
Multi-GPU: run under ``torch.distributed.run``; each rank traces an interleaved set of FoV x
wavelength blocks and the eyebox slabs are gathered to rank 0 (``distributed.py``); in device mode the ranks'
window sums are sum-reduced instead (``distributed.EyeboxReduce``; in windows mode the ranks' tables as they are).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import time
from types import SimpleNamespace

import numpy as np


# Fusing the num_iter chained traces into one persistent launch overlaps each trace's tail with
# the next one's bulk: 1.5x faster at 1.35M rays per GPU (C3), even at 5.4M (C4), and 13 % slower
# at 82.6M (C5, where the tail is a small part of a launch and the fused kernel runs one wave per
# SIMD fewer).  fuse=None picks by the rays per GPU.
FUSE_MAX_RAYS = 4_000_000


def run(num_FOV_x: int = 100, num_FOV_y: int = 75, num_rays_per_FoV: int = 5000, num_iter: int = 4,
        lambdas=(0, 1, 2), lut_dir: str | None = None, lut_seed: int = 0, lut_profile: str = "default",
        point_seed: int | None = None, evaluate: bool = True, verbose: bool = True, variant: int = 0,
        fuse: bool | None = None, points: np.ndarray | None = None, png: str | None = None,
        eyebox: str = "host", keep_grid: bool = False, evaluate_on: str = "host",
        keep_image: bool = False, budget: bool = False, error_bars: int = 0, estimator: str = "analog",
        footprint=None, hits=None, paths=None, paths_capacity=None, paths_footprint=None, sensitivity=None,
        what_if=None, polarisation: bool = False, analyser=None, analyser_frame: str = "fov", designs=None,
        tolerance=None, tolerance_designs: int = 64, tolerance_seed: int = 0, tolerance_channels=None,
        sources=None, source_counts: bool = False, source_map=None) -> dict:
    """The reference script's job on this engine; returns its printed quantities and arrays.
    ``points``: the R/2 in-coupler origins to use (default: sampled, GRTF:12-23, seeded by
    ``point_seed``); ``png``: where to write the "Eyebox Center View" image (needs ``evaluate``).

    ``eyebox``: where the grid is reduced after the trace.  ``"host"`` (the reference's flow, MAIN:186-198):
    the whole grid is copied to the host (864 MB at the default job), summed, scaled and evaluated there, and
    returned as ``matrix_EB``.  ``"device"``: one device pass reduces every 80 x 120 slab to its total and its
    7 x 8 pupil sums (``eyebox_window_sums``); ``A``, ``efficiency`` and the evaluation come from that
    ``[n_slabs, 57]`` table, several GPUs sum-reduce it (``distributed.EyeboxReduce``) instead of gathering
    slabs, and the grid stays on the device -- ``matrix_EB`` is returned only with ``keep_grid=True``.
    ``A`` and ``efficiency`` are bit-identical to the host mode's while a slab's count stays below 2^24 (then
    its float32 sum is the exact integer, as is the float64 one), which always holds for
    ``num_rays_per_FoV * num_iter < 2^24``; the evaluation divides the exact float64 window sums once where
    the host mode divides and sums in float32 (at most 902 * 2^-24 relative per eye position).

    ``"windows"``: the trace counts every out-coupling straight into that table (``engine.WindowPlan``,
    ``wgrt_trace_windows``): no grid is allocated, zeroed, scattered into or read back (864 MB at the default job
    against the table's 10 MB), several GPUs sum-reduce their tables as they are, and everything after the trace
    is device mode's, fed the same table bit for bit.  There is no grid to keep: ``keep_grid=True`` raises.

    ``evaluate_on``: where the colour math of the evaluation runs.  ``"host"``: ``evaluation_from_perceive`` in
    numpy.  ``"device"`` (needs ``eyebox="device"`` or ``"windows"``): the window-sum table (rank 0's, after the
    reduce, on several GPUs) is evaluated where it lives (``evaluation_from_window_sums``); only the three figures and
    the centre image come back, ``center_view`` and the PNG are built from that image, and ``output_image``
    (every eye position's image) is returned only with ``keep_image=True``.

    ``budget``: also report where every ray ended.  The ``num_iter`` traces then go as plain single launches
    (neither fused nor chained: only a single launch stores fates), each storing the rays' fate codes in one
    reused buffer of a byte per ray (``engine.trace_fullcolor(fate=...)``) and followed by ``engine.fate_census``
    into one ``[n_slabs, 56]`` table; several GPUs census their shards and sum-reduce the tables to rank 0.  Returned
    as ``fate_census`` (the int64 table) and ``loss_budget`` (``engine.loss_budget``) and printed per wavelength
    after the efficiencies.  Works with every ``eyebox`` mode; everything else returned is bit-identical to
    ``budget=False`` (separate launches give the fused call's results).

    ``error_bars``: ``B`` (2 .. 64; 0: none): Monte-Carlo standard errors of everything printed, from one job.  The
    trace counts the out-couplings of the ray with global id ``g`` into copy ``g % B`` of the window table
    (``engine.trace_fullcolor(replicas=B)``), the copies are folded into their sum and the ``B`` leave-one-out tables
    (``engine.fold_replicas``), and the metrics are jackknifed over them (``evaluation_error_bars``,
    ``efficiency_error_bars``).  A grid has no replicas, so it needs ``eyebox="windows"``; and it needs ``B | R / 2``:
    the TE ray and the TM ray of one origin then fall into the same replica, and every tile gives every replica the
    same number of rays, drawn from disjoint subsets of the ``R / 2`` origins all tiles share -- rays are not
    independent across tiles, and replicas by origin carry that dependence into the error bar.  Anything else raises
    ``ValueError`` before any GPU work, as does ``budget=True`` with it.  The traces go as plain single launches (only
    a single launch fills replica tables).  The result gains ``efficiency_se`` (per colour), ``A_se``, ``delta_e_se``,
    ``U_fov_se``, ``U_EB_se`` and ``jackknife`` (the leave-one-out figures ``[B, 3]``), and ``+-`` is printed beside each
    figure; everything returned before is bit-identical with and without it.  ``U_fov`` and ``U_EB`` are min / max
    ratios, for which the jackknife is an indication only.  Memory: 10.3 MB per replica at the default job (22,500
    slabs x 57 x 8 B), 205 MB at ``B = 20``, against the grid's 864 MB.

    ``estimator``: ``"analog"`` (the reference's: a ray counts 1 where its last draw out-couples it) or ``"expected"``
    (``engine.trace_fullcolor(expected=True)``): the same walk -- ``rng_states``, ``bounces`` and ``eyebox_hits`` are the
    analog job's -- but every out-coupler interaction inside the eyebox rectangle adds its out-coupling probability to
    the window table, so ``A``, the efficiencies, the three figures and their ``_se`` come from a table with the same
    expectation and a fraction of the variance.  It needs ``eyebox="windows"`` (a grid cannot hold the sums), goes as
    plain single launches, combines with ``error_bars``, both ``evaluate_on`` and several GPUs, and excludes
    ``budget=True``; anything else raises ``ValueError`` before any GPU work.  The result says which in ``estimator``.

    ``footprint``: ``(H, W)`` (None: none): also report where on the plate the light interacts, is lost and leaves.
    Every launch counts each Monte-Carlo draw of the bounce loop into an int64 map ``[num_lmd, 9, H, W]`` over the
    bounding box of ``eff_reg1`` (``engine.FootprintPlan.for_scene``, ``engine.trace_fullcolor(footprint=...)``):
    channels 0..5 the draws in state R0..R5, 6 the draws that lost the ray, 7 / 8 those that out-coupled it inside /
    beside its eyebox rectangle.  The traces go as plain single launches; several GPUs sum-reduce their maps to rank
    0.  Returned as ``footprint`` (the numpy map) and ``footprint_plan`` (the plan's fields) and printed per
    wavelength as totals.  Works with every ``eyebox`` mode; everything else returned is bit-identical to the run
    without it.  ``budget=True``, ``error_bars`` and ``estimator="expected"`` with it raise ``ValueError`` before any GPU
    work.

    ``hits``: ``True`` or a capacity in records (None / False: none): also keep every out-coupling -- inside its FoV's
    eyebox rectangle or beside it -- as a record ``(x, y, gid, tile, flags)`` (``engine.HitList``,
    ``engine.trace_fullcolor(hits=...)``).  The traces go as plain single launches, tagged with their iteration
    number.  ``True`` sizes the list to ``ceil(0.125 * rays of the shard * num_iter)`` records, about twice the 6 % of
    rays that the default LUT profile out-couples on the small jobs of the test suite; a list that is too small raises
    ``engine.HitListOverflow`` after the trace, naming the capacity that would have sufficed.  Several GPUs send their
    stored records to rank 0 (the counts all-gathered first, then the buffers padded to the largest); the ids are
    global, so the sorted concatenation is the single-process list.  Returned as ``hits`` (the structured array, sorted
    by tag and global id) and ``hit_count``, and printed per wavelength: out-couplings inside and beside the eyebox, and
    the beside share.  Works with every ``eyebox`` mode; everything else returned is bit-identical to the run without
    it.  ``budget=True``, ``error_bars``, ``estimator="expected"`` and ``footprint`` with it raise ``ValueError`` before
    any GPU work.

    ``paths``: ``"all"``, a fate class name of ``engine.FATE_CLASSES`` (``"eyebox"``, ``"left_plate"``, ``"lost_fc"``,
    ...) or a list of them (None: none): also record which way the selected rays went -- one record ``(x, y, gid, step,
    flags)`` per Monte-Carlo draw of the bounce loop, and one more where a trace leaves the plate or misses in R5
    (``engine.PathList``, ``engine.trace_fullcolor(paths=..., select=...)``).  The traces go as plain single launches,
    tagged with their iteration number.  For a class selection each iteration clones the RNG states, runs a fate launch
    with no grid on the clone, builds the mask from its fates (``engine.select_by_fate``) and runs the paths launch from
    the original states; ``"all"`` skips the first pass.  ``paths_capacity``: the list's room in records.  By default a
    selection's list is sized from its first pass and cannot overflow: a draw is made in a loop iteration and every
    iteration counts a bounce, so before each paths launch the list is grown to hold ``bounces + 1`` records of every
    selected ray (the first pass's per-ray bounces; one more for the end record).  ``"all"`` has no first pass and gets 8
    records per ray of the shard and iteration (measured: 3.7 per ray on BASELINE config 3, 3.9 on the 5 x 4 x 3 test
    job).  A list that is too small -- a given capacity, or ``"all"``'s default -- raises
    ``engine.PathListOverflow`` after the trace, naming the capacity that would have sufficed.  Several GPUs send their
    stored records to rank 0; the ids are global, so the sorted concatenation is the single-process list.  Returned as
    ``paths`` (the structured array, sorted by tag, global id and step) and ``paths_selected`` (rays recorded per
    wavelength, over all iterations), and printed per wavelength: rays selected, records kept, mean draws per selected
    ray.  ``paths_footprint=(H, W)``: also the list reduced on the device into a footprint map over the plate's
    bounding box (``PathList.footprint``: the conditional footprint of the selected rays), returned as
    ``paths_footprint`` / ``paths_footprint_plan``.  Works with every ``eyebox`` mode; everything else returned is
    bit-identical to the run without it.  ``budget=True``, ``error_bars``, ``estimator="expected"``, ``footprint`` and
    ``hits`` with it raise ``ValueError`` before any GPU work.

    ``sensitivity``: ``True`` or K (None: off; needs ``eyebox="windows"``): also the design sensitivities.  A ray reaches
    the eyebox with probability ``prod e_taken``, so for a delivered ray ``d log p / d log s_c = N_c``, the times it
    took channel c -- a (state, coupler slice, branch) triple, ``engine.visit_channels``.  The traces go as plain single
    launches.  Each iteration clones the RNG states, runs a fate launch with no grid on the clone, gives the rays of the
    ``eyebox`` class one row each, runs the visits launch from the original states (``engine.VisitTable``,
    ``engine.trace_fullcolor(visits=...)``) and reduces its rows on the device into one float64 ``[C, n_slabs, 57]``
    table (``VisitTable.sensitivity``): ``d table / d log s_c``, binned exactly as the window table; several GPUs sum
    theirs.  Returned as ``sensitivity`` and ``sensitivity_channels`` (the names), and printed per wavelength: the K
    (default 8) channels of largest elasticity ``sum_slabs sens[c, s, 0] / sum_slabs table[s, 0]`` -- the mean visits per
    delivered ray: the % change of that wavelength's efficiency per % change of the channel's efficiency.

    ``what_if``: ``{channel name: scale}`` (None: off; needs ``eyebox="windows"``): each iteration also re-weights its
    delivered rays by ``prod_c s_c^N_c`` into a second window table (``VisitTable.reweight``) -- the table of the design
    whose channels' efficiencies are scaled so, unbiased while every ``e1 + e2 + e3`` stays <= 1.  After
    the baseline's figures the same efficiencies and evaluation are printed for that table, with the weights' effective
    sample size per wavelength.  Returned as ``what_if``: ``scales``, ``table``, ``A``, ``efficiency``, ``ess`` and, with
    ``evaluate``, ``delta_e``, ``U_fov``, ``U_EB``.

    Both work together and leave everything else returned bit-identical to the run without them.  ``budget=True``,
    ``error_bars``, ``estimator="expected"``, ``footprint``, ``hits`` and ``paths`` with either raise ``ValueError``
    before any GPU work.

    ``designs``: a list of ``{channel name: scale}`` dicts (``{}``: the nominal design) or a ``[K, C]`` array of scales
    (None: off): the what-if for K designs at once.  Each iteration re-weights its delivered rays for every design in one
    pass (``VisitTable.reweight_many``, ``wgrt_visits_reweight_many``) into one float64 ``[K, n_slabs, 57]`` tensor and
    one int64 ``[K, 2, num_lmd]`` tensor of weight sums; several GPUs sum-reduce both to rank 0.  Table k is, bit for
    bit, the ``what_if`` table of ``designs[k]``; the designs share the sample, so their differences carry far less noise
    than two runs'.  ``tolerance``: sigma (None: off): the same for ``tolerance_designs`` designs of
    ``engine.tolerance_scales`` -- design 0 nominal, in the others ``ln s_c ~ N(0, sigma^2)`` per channel matching
    ``tolerance_channels`` (``fnmatch`` patterns such as ``"r4[*].b3"``; None: every channel), from
    ``tolerance_seed``.  The two exclude each other, need ``eyebox="windows"``, ride the visits launch of ``sensitivity``
    and ``what_if`` (all three combine) and carry their exclusions.  The tables' bytes are computed up front and
    printed; more than the device has free raises ``ValueError`` naming the largest K that fits.  Returned as
    ``ensemble``: ``scales`` ``[K, C]``, ``channels``, ``table``, ``A`` ``[K, L, NY, NX]``, ``efficiency`` ``[K, L]``,
    ``ess`` ``[K, L]`` and, with ``evaluate``, ``delta_e``, ``U_fov``, ``U_EB`` ``[K]`` (``evaluation_ensemble``); for
    ``tolerance`` also ``summary``: per figure (``efficiency`` per wavelength, ``delta_e``, ``U_fov``, ``U_EB``) its
    ``nominal`` value, and ``mean``, ``std``, ``p5``, ``p50``, ``p95`` over designs 1 .. K-1, and ``min_ess`` over all
    designs.  The estimator is the what-if's, and so is its limit: an up-scaled channel is over-credited wherever a
    state's branch efficiencies already sum to 1, so the upper tail of a tolerance band is optimistic.

    ``polarisation``: also the polarisation state of the delivered light (needs ``eyebox="windows"``).  The traces go as
    plain single launches that add, for every out-coupling the window table counts, the three fixed-point normalised
    Stokes parameters of the out-coupled field to int64 tables ``[3, n_slabs, 57]`` beside it (``engine.StokesTable``,
    ``engine.trace_fullcolor(stokes=...)``); several GPUs sum-reduce theirs to rank 0.  The basis is each FoV's own
    TE / TM basis of its out-coupled order, as the LUTs define it (``analyser_frame="fov"``); ``"lab"`` turns each FoV's
    table by its out-coupled azimuth plus 90 degrees (``geom.angles["phi_in_ic"]``, ``couplers_coor._field_angles``'
    ``ph``; ``stokes_rotate``) into the plate's x / y axes -- the paraxial form: it neglects ``cos(theta_polar)``, under
    2 % at this field of view.  Printed per wavelength: the mean Stokes vector and the degree of polarisation of all
    delivered light, and the spread of the per-FoV degree of polarisation.  ``analyser``: degrees (None: none): also the
    efficiencies and the evaluation of the table seen through an ideal linear polariser at that angle from the frame's
    first axis (``analyser_table``), with no re-trace.  Returned as ``stokes`` (the int64 tables, always in the FoVs' own
    bases), ``polarisation`` (``frame``, ``mean`` ``[L, 3]``, ``dop`` ``[L]``, ``dop_fov`` ``[L, NY, NX]``) and, with an
    analyser, ``analysed`` (``theta_deg``, ``frame``, ``table``, ``A``, ``efficiency`` and, with ``evaluate``,
    ``delta_e``, ``U_fov``, ``U_EB``).  Everything returned before is bit-identical with and without it.  ``budget=True``,
    ``error_bars``, ``estimator="expected"``, ``footprint``, ``hits``, ``paths``, ``sensitivity`` and ``what_if`` with it
    raise ``ValueError`` before any GPU work.

    ``sources``: a list of source dicts (``engine.source_weights``: ``{}`` the nominal source; ``centre``, ``diameter``,
    ``sigma``, ``te``, ``tm`` or explicit ``weights``) or a ``[K, R]`` array of weights (None: off): the figures of K
    projector pupils from the one trace.  A ray's entry point and input polarisation are a function of its global id, so
    each rank re-weights its own hit list on the device after the traces (``HitList.reweight_sources``,
    ``wgrt_hits_reweight_sources``): every out-coupling deposits its entry class's weight instead of 1.  This is exact,
    not an approximation, and the sources share the rays, so their differences carry far less noise than two runs'.  It
    implies ``hits=True`` when ``hits`` is not given, needs ``eyebox="windows"`` and combines and excludes exactly as
    ``hits`` does.  The tables' bytes are computed up front and printed; more than the device has free raises
    ``ValueError`` naming the largest K that fits.  The tables and the integer weight sums of several GPUs are
    sum-reduced to rank 0.  Printed: one line per source with the efficiencies, the three figures and the smallest
    effective sample size.  Returned as ``sources``: ``weights`` ``[K, R]``, ``table`` ``[K, n_slabs, 57]``, ``A``,
    ``efficiency`` ``[K, L]``, ``sums``, ``ess`` ``[K, L]`` and, with ``evaluate``, ``delta_e``, ``U_fov``, ``U_EB``
    ``[K]``; source ``{}`` has the job's own table and figures bit for bit.  Every row of weights has mean 1, so the
    efficiencies are per unit of projector power.  A stop that keeps a fraction of the entry points keeps that fraction
    of the rays: judge a source with its effective sample size beside it.

    ``source_counts=True`` (needs ``hits``): also the hit list counted per entry class on the device
    (``HitList.source_counts``), returned as ``source_counts`` (int64 ``[num_lmd, 2, R]``: inside / beside the eyebox),
    and printed per wavelength: the delivered efficiency of the TE half and of the TM half of the input.
    ``source_map=(H, W)``: also the entrance-pupil map ``engine.source_map`` of those counts, returned as
    ``source_map`` (``delivered`` ``[num_lmd, 2, H, W]``, ``launched`` ``[H, W]``)."""
    if sources is not None:
        from .engine import check_sources
        sources = check_sources(sources, int(num_rays_per_FoV))
        if eyebox != "windows":
            raise ValueError("sources re-weights the hit list into window tables: it needs eyebox='windows'")
        if hits is None or hits is False:
            hits = True
    if source_map is not None:
        if len(tuple(source_map)) != 2 or not all(1 <= int(v) <= 4096 for v in source_map):
            raise ValueError(f"source_map must be (H, W) cells, each 1 .. 4096, got {source_map!r}")
        source_map = (int(source_map[0]), int(source_map[1]))
        if not source_counts:
            raise ValueError("source_map is a map of the source counts: it needs source_counts=True")
    if source_counts:
        if hits is None or hits is False:
            raise ValueError("source_counts counts the hit list per entry class: it needs hits")
        if int(num_rays_per_FoV) % 2:
            raise ValueError("source_counts needs an even num_rays_per_FoV: half the entry classes are TE, half TM")
    if sources is not None and points is not None:   # the whole check before any GPU work where the origins are given
        from .engine import source_weights
        source_weights(points, int(num_rays_per_FoV), sources)
    if analyser_frame not in ("fov", "lab"):
        raise ValueError(f"analyser_frame must be 'fov' or 'lab', got {analyser_frame!r}")
    if analyser is not None:
        if isinstance(analyser, bool) or not isinstance(analyser, (int, float, np.integer, np.floating)) \
                or not np.isfinite(float(analyser)):
            raise ValueError(f"analyser must be an angle in degrees, got {analyser!r}")
        if not polarisation:
            raise ValueError("analyser needs polarisation=True: the analysed table comes from the Stokes tables")
        analyser = float(analyser)
    if polarisation:
        if budget or error_bars or estimator == "expected" or footprint is not None or \
                not (hits is None or hits is False) or not (paths is None or paths is False) or \
                not (sensitivity is None or sensitivity is False) or what_if is not None or designs is not None or \
                tolerance is not None:
            raise ValueError("polarisation is not combined with budget=True, error_bars, estimator='expected', footprint, "
                             "hits, paths, sensitivity, what_if, designs or tolerance: a launch fills Stokes tables or "
                             "does one of those")
        if eyebox != "windows":
            raise ValueError("polarisation fills tables beside the window table: it needs eyebox='windows'")
    top_k = 0
    if sensitivity is None or sensitivity is False:
        sensitivity = None
    else:
        top_k = 8 if sensitivity is True else sensitivity
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or int(top_k) < 1:
            raise ValueError(f"sensitivity must be True or the number K >= 1 of channels to print, got {sensitivity!r}")
        top_k = int(top_k)
    if what_if is not None:
        if not isinstance(what_if, dict) or not what_if:
            raise ValueError(f"what_if must be a dict {{channel name: scale}}, got {what_if!r}")
        from .luts import channel_quad
        for name, sc_ in what_if.items():
            try:
                channel_quad(name)
                ok = float(sc_) > 0.0 and np.isfinite(float(sc_))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"what_if: {name!r}={sc_!r} is not a visit channel with a positive finite scale")
        what_if = {str(k): float(v) for k, v in what_if.items()}
    if designs is not None and tolerance is not None:
        raise ValueError("designs and tolerance exclude each other: an ensemble is listed or drawn, not both")
    if designs is not None:
        if isinstance(designs, dict) or not hasattr(designs, "__len__") or len(designs) == 0:
            raise ValueError(f"designs must be a non-empty list of {{channel name: scale}} dicts or a [K, C] array, "
                             f"got {designs!r}")
        if all(isinstance(d, dict) for d in designs):
            from .luts import channel_quad
            for d in designs:
                for name, sc_ in d.items():
                    try:
                        channel_quad(name)
                        ok = float(sc_) > 0.0 and np.isfinite(float(sc_))
                    except (TypeError, ValueError):
                        ok = False
                    if not ok:
                        raise ValueError(f"designs: {name!r}={sc_!r} is not a visit channel with a positive finite scale")
            designs = [{str(k): float(v) for k, v in d.items()} for d in designs]
        else:
            try:
                designs = np.ascontiguousarray(designs, dtype=np.float64)
            except (TypeError, ValueError):
                designs = None
            if designs is None or designs.ndim != 2 or not (np.isfinite(designs).all() and (designs > 0).all()):
                raise ValueError("designs must be a list of {channel name: scale} dicts or a [K, C] array of positive "
                                 "finite scales")
    if tolerance is not None:
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or \
                not (float(tolerance) > 0.0 and np.isfinite(float(tolerance))):
            raise ValueError(f"tolerance must be a positive finite sigma of ln(scale), got {tolerance!r}")
        if isinstance(tolerance_designs, bool) or not isinstance(tolerance_designs, (int, np.integer)) or \
                int(tolerance_designs) < 2:
            raise ValueError(f"tolerance_designs must be >= 2 (the nominal design and one drawn), got "
                             f"{tolerance_designs!r}")
        tolerance, tolerance_designs = float(tolerance), int(tolerance_designs)
        if tolerance_channels is not None:
            tolerance_channels = [tolerance_channels] if isinstance(tolerance_channels, str) else list(tolerance_channels)
            if not tolerance_channels or not all(isinstance(p, str) and p for p in tolerance_channels):
                raise ValueError(f"tolerance_channels must be a list of channel patterns, got {tolerance_channels!r}")
    ensemble = designs is not None or tolerance is not None
    if sensitivity is not None or what_if is not None or ensemble:
        if budget or error_bars or estimator == "expected" or footprint is not None or \
                not (hits is None or hits is False) or not (paths is None or paths is False):
            raise ValueError("sensitivity / what_if / designs / tolerance are not combined with budget=True, error_bars, "
                             "estimator='expected', footprint, hits or paths: a launch counts branch visits or does one "
                             "of those")
        if eyebox != "windows":
            raise ValueError("sensitivity / what_if / designs / tolerance reduce into window tables: they need "
                             "eyebox='windows'")
    path_classes = None   # the fate classes of a selection (None: none, or every ray)
    if paths is None or paths is False:
        paths = None
        if paths_capacity is not None or paths_footprint is not None:
            raise ValueError("paths_capacity / paths_footprint need paths")
    else:
        if budget or error_bars or estimator == "expected" or footprint is not None or not (hits is None or hits is False):
            raise ValueError("paths is not combined with budget=True, error_bars, estimator='expected', footprint or "
                             "hits: a launch keeps a path list or does one of those")
        from .engine import FATE_CLASSES
        names = [paths] if isinstance(paths, str) else list(paths)
        known = [c[0] for c in FATE_CLASSES]
        if not names or not all(isinstance(n, str) and (n in known or (n == "all" and len(names) == 1)) for n in names):
            raise ValueError(f"paths must be 'all', a fate class or a list of fate classes ({', '.join(known)}), "
                             f"got {paths!r}")
        path_classes = None if names == ["all"] else names
        if paths_capacity is not None and (isinstance(paths_capacity, bool) or int(paths_capacity) != paths_capacity
                                           or int(paths_capacity) < 0):
            raise ValueError(f"paths_capacity must be a capacity >= 0 in records, got {paths_capacity!r}")
        if paths_footprint is not None:
            if len(tuple(paths_footprint)) != 2 or not all(3 <= int(v) <= 4096 for v in paths_footprint):
                raise ValueError(f"paths_footprint must be (H, W) cells, each 3 .. 4096, got {paths_footprint!r}")
            paths_footprint = (int(paths_footprint[0]), int(paths_footprint[1]))
    if hits is None or hits is False:
        hits = None
    else:
        if budget or error_bars or estimator == "expected" or footprint is not None:
            raise ValueError("hits is not combined with budget=True, error_bars, estimator='expected' or footprint: a "
                             "launch keeps a hit list or does one of those")
        if hits is not True and (isinstance(hits, bool) or int(hits) != hits or int(hits) < 0):
            raise ValueError(f"hits must be True or a capacity >= 0 in records, got {hits!r}")
    if footprint is not None:
        if budget or error_bars or estimator == "expected":
            raise ValueError("footprint is not combined with budget=True, error_bars or estimator='expected': a launch "
                             "counts footprints or does one of those")
        if len(tuple(footprint)) != 2 or not all(3 <= int(v) <= 4096 for v in footprint):
            raise ValueError(f"footprint must be (H, W) cells, each 3 .. 4096, got {footprint!r}")
        footprint = (int(footprint[0]), int(footprint[1]))
    if estimator not in ("analog", "expected"):
        raise ValueError(f"estimator must be 'analog' or 'expected', got {estimator!r}")
    expected = estimator == "expected"
    if expected:
        if eyebox != "windows":
            raise ValueError("estimator='expected' scores into the window table: it needs eyebox='windows' (a float32 "
                             "grid cannot hold the sums)")
        if budget:
            raise ValueError("estimator='expected' and budget=True exclude each other: no launch both scores every "
                             "visit and stores fates")
    error_bars = int(error_bars or 0)
    if error_bars:
        if not 2 <= error_bars <= 64:
            raise ValueError(f"error_bars must be 0 or 2 .. 64 replicas, got {error_bars}")
        if eyebox != "windows":
            raise ValueError("error_bars counts into replica window tables: it needs eyebox='windows' (a grid has no "
                             "replicas)")
        if budget:
            raise ValueError("error_bars and budget=True exclude each other: a launch stores fates or fills replica "
                             "tables, not both")
        if int(num_rays_per_FoV) % 2 or (int(num_rays_per_FoV) // 2) % error_bars:
            raise ValueError(f"error_bars={error_bars} must divide num_rays_per_FoV / 2 = {int(num_rays_per_FoV) / 2:g}: the "
                             "replicas are then disjoint subsets of the origins every tile shares")
    if eyebox not in ("host", "device", "windows"):
        raise ValueError(f"eyebox must be 'host', 'device' or 'windows', got {eyebox!r}")
    if evaluate_on not in ("host", "device"):
        raise ValueError(f"evaluate_on must be 'host' or 'device', got {evaluate_on!r}")
    if evaluate_on == "device" and eyebox == "host":
        raise ValueError("evaluate_on='device' evaluates the on-device window sums: it needs eyebox='device' "
                         "or 'windows'")
    if eyebox == "windows" and keep_grid:
        raise ValueError("eyebox='windows' traces without a grid: there is none to keep (keep_grid=True)")
    from .engine import STAT
    with _set_up(num_FOV_x, num_FOV_y, int(num_rays_per_FoV), num_iter, lambdas, lut_dir, lut_seed, lut_profile,
                 point_seed, points, verbose, eyebox == "windows", budget, error_bars) as job:   # closes the scene on every way out
        job.expected = expected
        job.footprint = None
        if footprint is not None:
            from .engine import FootprintPlan
            fp = FootprintPlan.for_scene(job.geom, cells=footprint)
            job.footprint = (fp, fp.new_map(job.scene))
        job.hits = None
        if hits is not None:
            from .engine import HitList
            cap = -(-job.shard.n_rays * int(num_iter) // 8) if hits is True else int(hits)
            job.hits = HitList(cap, job.dev)
        src = _sources_set_up(job, sources) if sources is not None else None
        job.paths = None
        if paths is not None:
            import torch

            from .engine import PathList, WindowPlan
            # the default room: "all" has no first pass to size the list from, and gets 8 records per ray and iteration;
            # a selection starts empty and is grown from each first pass's mask and bounces (hip_tracer)
            auto = paths_capacity is None and path_classes is not None
            cap = int(paths_capacity) if paths_capacity is not None else \
                (0 if auto else job.shard.n_rays * int(num_iter) * 8)
            job.paths = SimpleNamespace(list=PathList(cap, job.dev), classes=path_classes, fate=None, windows=None,
                                        selected=torch.zeros(job.scene.num_lmd, dtype=torch.int64, device=job.dev))
            if path_classes is not None:   # a selection's first pass: its fates, and a table for its out-couplings
                job.paths.fate = torch.zeros(job.shard.n_rays, dtype=torch.uint8, device=job.dev)
                scratch = WindowPlan(device=job.dev.index)
                job.paths.windows = (scratch, scratch.new_table(job.scene))
                if auto:
                    job.paths.bounces = torch.zeros(job.shard.n_rays, dtype=torch.int32, device=job.dev)
        job.stokes = None
        if polarisation:
            from .engine import StokesTable
            job.stokes = StokesTable(job.scene, job.windows[0], job.dev)
        job.visits = None
        if sensitivity is not None or what_if is not None or ensemble:
            import torch

            from .engine import WindowPlan, visit_channels
            names = visit_channels(job.scene)
            if what_if is not None and not set(what_if) <= set(names):
                raise ValueError(f"what_if names no visit channel of this scene: {sorted(set(what_if) - set(names))}")
            n_slabs, W = job.windows[1].shape
            ens = None
            if ensemble:
                ens = _ensemble_set_up(job, names, n_slabs, W, designs, tolerance, tolerance_designs, tolerance_seed,
                                       tolerance_channels)
            scratch = WindowPlan(device=job.dev.index)
            job.visits = SimpleNamespace(
                plan=job.windows[0], fate=torch.zeros(job.shard.n_rays, dtype=torch.uint8, device=job.dev),
                windows=(scratch, scratch.new_table(job.scene)), channels=names,
                sens=(torch.zeros((len(names), n_slabs, W), dtype=torch.float64, device=job.dev)
                      if sensitivity is not None else None), scales=what_if,
                table=torch.zeros((n_slabs, W), dtype=torch.float64, device=job.dev) if what_if is not None else None,
                sums=torch.zeros((2, job.scene.num_lmd), dtype=torch.float64, device=job.dev), ensemble=ens)
        try:
            kern_s = _trace(job, variant, fuse)
        finally:
            if job.paths is not None and job.paths.windows is not None:
                job.paths.windows[0].close()
            if job.visits is not None:
                job.visits.windows[0].close()
        t_post = time.perf_counter()   # everything below is post-processing of the traced grid
        grid, table, stats = _collect(job, eyebox != "host", keep_grid)
        reps = None
        if job.replicas and job.rank == 0:   # the replica tables -> their sum (the one table, bit for bit) + leave-one-outs
            from .engine import fold_replicas
            reps, table = table, fold_replicas(table)[0]
        out = dict(num_rays=job.num_rays, num_iter=num_iter, gpu_seconds=kern_s, bounces=int(stats[STAT.bounces]),
                   eyebox_hits=int(stats[STAT.eyebox_hits]), rng_states=job.rng.cpu().numpy().view(np.uint32),
                   estimator=estimator)
        census = _census(job)
        fmap = None
        if job.footprint is not None:   # integer counts: the ranks' maps add exactly
            from .distributed import reduce_eyebox
            fmap = reduce_eyebox(job.footprint[1])
        records = _gather_hits(job) if job.hits is not None else None
        stables = ssums = scounts = None
        if src is not None:   # every rank re-weights its own list; grid-valued doubles and integers: both add exactly
            from .distributed import reduce_eyebox
            job.hits.reweight_sources(job.scene, job.windows[0], src.weights_dev, out=src.tables, sums=src.sums)
            stables, ssums = reduce_eyebox(src.tables), reduce_eyebox(src.sums)
        if source_counts:     # integer counts: the ranks' add exactly
            from .distributed import reduce_eyebox
            scounts = reduce_eyebox(job.hits.source_counts(job.scene, job.R))
        path_records = path_map = path_sel = None
        if job.paths is not None:
            from .distributed import reduce_eyebox
            path_records = _gather_paths(job)
            path_sel = reduce_eyebox(job.paths.selected)
            if paths_footprint is not None:   # every rank reduces its own list; integer counts: the maps add exactly
                from .engine import FootprintPlan
                pfp = FootprintPlan.for_scene(job.geom, cells=paths_footprint)
                path_map = reduce_eyebox(job.paths.list.footprint(job.scene, pfp))
        sens = wtable = wsums = etables = esums = None
        if job.visits is not None:   # sums over rays: the ranks' tables add
            from .distributed import reduce_eyebox
            sens = reduce_eyebox(job.visits.sens) if job.visits.sens is not None else None
            if what_if is not None:
                wtable, wsums = reduce_eyebox(job.visits.table), reduce_eyebox(job.visits.sums)
            if ensemble:   # grid-valued doubles and integers: both add exactly
                etables = reduce_eyebox(job.visits.ensemble.tables)
                esums = reduce_eyebox(job.visits.ensemble.sums)
        stokes = None
        if job.stokes is not None:   # integer sums: the ranks' tables add exactly
            from .distributed import reduce_eyebox
            stokes = reduce_eyebox(job.stokes.raw())
        if job.rank != 0:
            return out
        _report(job, out, grid, table, reps)
        if census is not None:
            _report_budget(job, out, census)
        if fmap is not None:
            _report_footprint(job, out, fmap)
        if records is not None:
            _report_hits(job, out, records)
        if path_records is not None:
            _report_paths(job, out, path_records, path_sel, path_map, pfp if path_map is not None else None)
        if evaluate:
            _evaluate(job, out, grid, table, evaluate_on, keep_image, png, reps)
        if sens is not None and sensitivity is not None:
            _report_sensitivity(job, out, sens, table, top_k)
        if wtable is not None:
            _report_what_if(job, out, what_if, wtable, wsums, evaluate, evaluate_on)
        if ensemble:
            _report_ensemble(job, out, job.visits.ensemble, etables, esums, evaluate, evaluate_on)
        if stokes is not None:
            _report_polarisation(job, out, table, stokes, analyser, analyser_frame, evaluate, evaluate_on)
        if scounts is not None:
            _report_source_counts(job, out, scounts, source_map)
        if stables is not None:
            _report_sources(job, out, src, stables, ssums, evaluate, evaluate_on)
        out["post_seconds"] = time.perf_counter() - t_post
        job.say(f"Post-processing time  : {out['post_seconds']:.4f} s  (eyebox reduced "
                f"{'by the trace' if eyebox == 'windows' else 'on the ' + eyebox})")
        return out


@contextlib.contextmanager
def _set_up(nx, ny, R, num_iter, lambdas, lut_dir, lut_seed, lut_profile, point_seed, points, verbose,
            windows: bool = False, budget: bool = False, replicas: int = 0):
    """Steps 1-3: geometry, LUTs, the scene, the origins (rank 0's on every rank), every rank's shard and this
    rank's rays, as the record the later stages read; the scene is closed when the ``with`` block ends.
    ``windows``: a zeroed window table (``job.windows = (plan, table)``) instead of the grid (``job.eb`` None).
    ``budget``: a fate buffer of a byte per ray of the shard and a zeroed census table (``job.fate``, ``job.census``).
    ``replicas``: the table is the zeroed ``[replicas, n_slabs, W]`` replica tables (``job.replicas``)."""
    import torch
    import torch.distributed as dist

    from .couplers_coor import design_geometry
    from .distributed import hip_shard_builder, make_shard
    from .engine import Scene, WindowPlan, new_stats
    if budget:
        from .engine import FATE_COLS
    from .luts import load_luts, lut_f32_mask, synthetic_luts, validate_luts
    from .rays import generate_points_in_polygon

    world, rank = (dist.get_world_size(), dist.get_rank()) if dist.is_initialized() else (1, 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    say = (lambda *a: print(*a, flush=True)) if (verbose and rank == 0) else (lambda *a: None)

    say("=" * 60 + "\nInitializing system components ...\n" + "=" * 60)
    geom = design_geometry(nx, ny)
    f32_angles = 0
    if lut_dir:
        raw = load_luts(lut_dir)
        f32_angles = lut_f32_mask(raw)   # complex64 files: float32 cosines, as the compiled reference
        luts = validate_luts(raw, len(geom.lmd), nx, ny, geom.num_fc_slices, geom.num_oc_slices)
    else:
        luts = synthetic_luts(geom, seed=lut_seed, profile=lut_profile)
    with contextlib.closing(Scene.from_geometry(geom, luts, device=dev.index, lut_f32_angles=f32_angles)) as scene:
        if points is None:
            points = generate_points_in_polygon(geom.IC, R // 2,
                                                rng=None if point_seed is None else np.random.default_rng(point_seed))
        points = np.ascontiguousarray(points, dtype=np.float64)
        if world > 1:  # every rank must use the same origins
            t = torch.from_numpy(points).to(dev)
            dist.broadcast(t, src=0)
            points = t.cpu().numpy()
        shards = [make_shard(nx, ny, len(lambdas), R, world, r) for r in range(world)]
        # ray columns and RNG seeds built on the device (MAIN:59-158 without the host arrays:
        # 48 B x N of host memory and its upload at the reference's 100 x 75 x 3 x 5000 default)
        rays, rng = hip_shard_builder(points, nx, ny, lambdas, R, dev)(shards[rank])
        eb = None if windows else torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
        plan = WindowPlan(device=dev.index) if windows else None
        num_rays = nx * ny * len(lambdas) * R
        fate = torch.zeros(rng.numel(), dtype=torch.uint8, device=dev) if budget else None
        census = (torch.zeros((scene.num_lmd * ny * nx, FATE_COLS), dtype=torch.int64, device=dev) if budget else None)
        say(f"Initialization complete: {num_rays:,} rays, {world} GPU(s)\n" + "=" * 60 + "\nSTART GPU RAY TRACING\n" + "=" * 60)
        try:
            yield SimpleNamespace(nx=nx, ny=ny, R=R, num_iter=num_iter, lambdas=lambdas, world=world, rank=rank,
                                  dev=dev, say=say, scene=scene, shards=shards, shard=shards[rank], rays=rays, rng=rng,
                                  eb=eb, windows=(plan, plan.new_table(scene, replicas=replicas)) if windows else None,
                                  stats=new_stats(dev), num_rays=num_rays, fate=fate, census=census,
                                  replicas=replicas, geom=geom, points=points)
        finally:
            if plan is not None:
                plan.close()


def _trace(job, variant, fuse) -> float:
    """Step 4, the num_iter chained launches of MAIN:169-177; fuse: as one call (wgrt_launch_opts.num_iter, one
    persistent launch for the Jones-vector variants), with identical results.  With the job's fate buffer
    (``budget``): plain single launches, each followed by its census; with replica tables (``error_bars``): plain
    single launches too.  Returns their seconds by HIP events."""
    import torch

    from .distributed import hip_tracer, run_steps, split_calls
    from .engine import check_stats, fate_census, reserve
    n_rays = job.shard.n_rays
    per_call = 0 if (n_rays <= FUSE_MAX_RAYS if fuse is None else fuse) else 1
    hook = None
    if job.fate is not None:   # the budget: a launch's fates are counted before the next launch overwrites them
        per_call = 1
        hook = lambda j, when: when == "end" and fate_census(job.scene, job.rays, job.fate, table=job.census)
    if job.replicas or getattr(job, "expected", False):   # only a single launch fills replica tables or scores the
        per_call = 1                                      # expected-value estimator; the tracer offers no chain
    if getattr(job, "footprint", None) is not None:       # ... or counts footprints
        per_call = 1
    if getattr(job, "hits", None) is not None:            # ... or keeps a hit list
        per_call = 1
    if getattr(job, "paths", None) is not None:           # ... or a path list
        per_call = 1
    if getattr(job, "visits", None) is not None:          # ... or counts branch visits
        per_call = 1
    if getattr(job, "stokes", None) is not None:          # ... or fills Stokes tables
        per_call = 1
    calls = split_calls(job.num_iter, per_call)
    if n_rays and calls:
        reserve(job.scene, n_rays, max(calls))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    if n_rays:
        run_steps(hip_tracer(job.scene, variant, job.stats, job.windows, fate=job.fate, replicas=job.replicas,
                             expected=getattr(job, "expected", False), footprint=getattr(job, "footprint", None),
                             hits=getattr(job, "hits", None), paths=getattr(job, "paths", None),
                             visits=getattr(job, "visits", None), stokes=getattr(job, "stokes", None)),
                  job.rays, job.rng, job.eb,
                  job.shard.gid, job.num_iter, per_call, hook=hook)
    t1.record()
    torch.cuda.synchronize()
    check_stats(job.stats)
    return t0.elapsed_time(t1) / 1e3


def _collect(job, on_device: bool, keep_grid: bool):
    """The ranks' results brought together, ``(grid, table, stats)``: the whole job's eyebox grid on the host
    (rank 0, in host mode or with ``keep_grid``; else None), device mode's ``[n_slabs, 57]`` window sums of that
    grid as a device tensor (rank 0's is the job's; else None), and the job's counters on the host.  With replica
    tables the table is all of them, ``[B, n_slabs, 57]``: replicas are by global ray id, so the ranks' tables add."""
    import torch.distributed as dist

    from .AR_system_evaluation_functions import eyebox_window_sums
    from .distributed import EyeboxGather, EyeboxReduce, reduce_eyebox
    if job.windows is not None:
        table = reduce_eyebox(job.windows[1])
        if job.world > 1:
            dist.all_reduce(job.stats)
        return None, table, job.stats.cpu().numpy()
    want_grid = not on_device or keep_grid
    table = None
    if job.world > 1:
        plan = ([s.blocks for s in job.shards], job.nx, job.ny, job.lambdas, job.scene.num_lmd)
        if on_device:
            table = EyeboxReduce(*plan)(job.eb)
        if want_grid:
            EyeboxGather(*plan, device=job.dev)(job.eb)
        dist.all_reduce(job.stats)
    elif on_device:
        table = eyebox_window_sums(job.eb)
    return job.eb.cpu().numpy() if want_grid and job.rank == 0 else None, table, job.stats.cpu().numpy()


def _census(job):
    """The job's fate census on rank 0 (``budget``; else None): every rank's table of its shard, sum-reduced -- one
    reduce of an int64 table through ``distributed._operands``, as the window tables go."""
    if job.census is None:
        return None
    from .distributed import reduce_eyebox
    return reduce_eyebox(job.census)


def _report_budget(job, out: dict, census) -> None:
    """The loss budget into ``out`` and printed per wavelength (``engine.loss_budget``)."""
    from .engine import FATE_CLASSES, loss_budget
    out["fate_census"] = census.cpu().numpy()
    out["loss_budget"] = b = loss_budget(out["fate_census"], job.scene)
    names = {0: "Blue", 1: "Green", 2: "Red"}
    job.say("Loss budget (share of the traced rays)")
    job.say("  " + " " * 18 + "".join(f"{names.get(k, str(k)):>10s}" for k in range(len(b["per_wavelength"]))) + f"{'all':>10s}")
    for name, _, _ in FATE_CLASSES:
        row = [w["fractions"][name] for w in b["per_wavelength"]] + [b["total"]["fractions"][name]]
        job.say(f"  {name:18s}" + "".join(f"{v * 100:9.3f}%" for v in row))


def _report_sensitivity(job, out: dict, sens, table, top_k: int) -> None:
    """The sensitivity tables into ``out`` and, per wavelength, the ``top_k`` channels of largest elasticity printed: the
    visits of channel c per delivered ray, ``sum_slabs sens[c, s, 0] / sum_slabs table[s, 0]``."""
    out["sensitivity"] = s = sens.cpu().numpy()
    out["sensitivity_channels"] = list(job.visits.channels)
    nl = job.scene.num_lmd
    per = s[:, :, 0].reshape(s.shape[0], nl, -1).sum(axis=2)                 # [C, num_lmd]
    tot = table[:, 0].cpu().numpy().reshape(nl, -1).sum(axis=1)              # [num_lmd]
    names = {0: "Blue", 1: "Green", 2: "Red"}
    job.say(f"Design sensitivities: the {top_k} channels of largest elasticity (% efficiency per % of the channel)")
    for l in range(nl):
        el = per[:, l] / tot[l] if tot[l] else np.zeros(s.shape[0])
        order = np.argsort(-el, kind="stable")[:top_k]
        job.say(f"  {names.get(l, str(l)):6s}" + "".join(f"  {job.visits.channels[c]}={el[c]:.3f}" for c in order))


def _report_what_if(job, out: dict, scales: dict, wtable, wsums, evaluate: bool, evaluate_on: str) -> None:
    """The what-if table's figures into ``out["what_if"]`` and printed: the efficiencies and the evaluation ``_report``
    and ``_evaluate`` give for the baseline's table, and the weights' effective sample size."""
    from .AR_system_evaluation_functions import (evaluation_from_perceive, evaluation_from_window_sums,
                                                 perceive_from_window_sums)
    from .engine import ess_of
    shape = job.scene.eb_shape()
    A = wtable[:, 0].cpu().numpy().reshape(shape[:-2]).astype(np.float32) / job.num_rays / job.num_iter
    names = {0: "Blue", 1: "Green", 2: "Red"}
    eff = {names.get(k, str(k)): float(np.sum(A[k] * 3)) for k in range(A.shape[0])}
    ess = ess_of(wsums).cpu().numpy()
    w = dict(scales=dict(scales), table=wtable.cpu().numpy(), A=A, efficiency=eff, ess=ess)
    job.say("What if " + ", ".join(f"{k} x {v:g}" for k, v in scales.items()) + " (the same rays, re-weighted)")
    if any(v > 1.0 for v in scales.values()):
        # (a scale above 1 can push a state's e1 + e2 + e3 past 1, where the scaled design gains less than the weights
        # say: the figures below are then too high; DESIGN.md 4.10 has the size of it on the synthetic LUTs)
        job.say("  note: scaled up -- unbiased only where the state's branch efficiencies still sum to <= 1; "
                "check the scaled LUTs (luts.scale_channel) or confirm with a direct run")
    for c in ("Red", "Green", "Blue"):
        if c in eff:
            k = {v: i for i, v in names.items()}[c]
            job.say(f"Efficiency ({c:5s})    : {eff[c] * 100:8.3f} %  (effective sample size {ess[k]:,.0f})")
    if evaluate:
        divisor = job.R * job.num_iter
        if evaluate_on == "device":
            *figures, _ = evaluation_from_window_sums(wtable, shape, divisor, image="center")
        else:
            *figures, _ = evaluation_from_perceive(perceive_from_window_sums(w["table"], shape, divisor))
        w["delta_e"], w["U_fov"], w["U_EB"] = (float(v) for v in figures)
        job.say(f"Color dispersion      : {w['delta_e']:8.2f}")
        job.say(f"FoV uniformity        : {w['U_fov'] * 100:8.2f} %")
        job.say(f"Eyebox uniformity     : {w['U_EB'] * 100:8.2f} %")
    out["what_if"] = w


ENSEMBLE_CHUNK = 64   # designs per chunk of wgrt_visits_reweight_many: its scratch is [n_slabs * W, 64] float64


def _ensemble_set_up(job, names, n_slabs: int, W: int, designs, tolerance, n_designs, seed, patterns):
    """The ensemble's record for ``hip_tracer`` (``visits.ensemble``): ``scales`` (what ``reweight_many`` takes),
    ``scales_array`` ``[K, C]``, ``tolerance`` (sigma or None) and the two device tensors every iteration adds to.  The
    tables' bytes are printed and checked against the device's free memory first."""
    import torch

    from .engine import tolerance_scales
    C = len(names)
    if tolerance is not None:
        scales = array = tolerance_scales(names, tolerance, n_designs, seed, patterns)
    elif isinstance(designs, np.ndarray):
        if designs.shape[1] != C:
            raise ValueError(f"designs has {designs.shape[1]} scales per design, the scene {C} visit channels")
        scales = array = designs
    else:
        bad = sorted(set().union(*designs) - set(names))
        if bad:
            raise ValueError(f"designs names no visit channel of this scene: {bad}")
        scales, array = designs, np.ones((len(designs), C), dtype=np.float64)
        for k, d in enumerate(designs):
            for name, s in d.items():
                array[k, names.index(name)] = s
    K = array.shape[0]
    per_design, fixed = n_slabs * W * 8, n_slabs * W * ENSEMBLE_CHUNK * 8   # a table; the reduction's scratch
    free = int(torch.cuda.mem_get_info(job.dev)[0])
    job.say(f"Design ensemble       : {K} designs, tables {K * per_design / 1e6:,.1f} MB "
            f"(+ {fixed / 1e6:,.1f} MB while reducing; {free / 1e6:,.0f} MB free)")
    if K * per_design + fixed > free:
        fits = max((free - fixed) // per_design, 0)
        raise ValueError(f"designs / tolerance: {K} tables of {per_design / 1e6:,.1f} MB exceed the device's free memory "
                         f"({free / 1e6:,.0f} MB); the largest K that fits is {fits}")
    return SimpleNamespace(scales=scales, scales_array=array, tolerance=tolerance,
                           tables=torch.zeros((K, n_slabs, W), dtype=torch.float64, device=job.dev),
                           sums=torch.zeros((K, 2, job.scene.num_lmd), dtype=torch.int64, device=job.dev))


def _report_ensemble(job, out: dict, ens, tables, sums, evaluate: bool, evaluate_on: str) -> None:
    """The ensemble's figures into ``out["ensemble"]`` and printed: one line per listed design, or, for a tolerance
    ensemble, the band of every figure over the drawn designs."""
    from .AR_system_evaluation_functions import evaluation_ensemble
    from .engine import ess_of_quanta
    shape = job.scene.eb_shape()
    t = tables.cpu().numpy()
    K = t.shape[0]
    A = t[:, :, 0].reshape((K,) + tuple(shape[:-2])).astype(np.float32) / job.num_rays / job.num_iter
    eff = np.array([[float(np.sum(A[k, l] * 3)) for l in range(A.shape[1])] for k in range(K)], dtype=np.float64)
    ess = ess_of_quanta(sums.cpu().numpy())
    e = dict(scales=ens.scales_array, channels=list(job.visits.channels), table=t, A=A, efficiency=eff, ess=ess,
             sums=sums.cpu().numpy())
    figures = {}
    if evaluate:
        figures = evaluation_ensemble(tables if evaluate_on == "device" else t, shape, job.R * job.num_iter, evaluate_on)
        e.update(figures)
    names = {0: "Blue", 1: "Green", 2: "Red"}
    lam = [names.get(l, str(l)) for l in range(eff.shape[1])]
    if ens.tolerance is None:
        job.say(f"Design ensemble: {K} designs (the same rays, re-weighted)")
        for k in range(K):
            line = f"  design {k:3d}: " + "  ".join(f"{n} {eff[k, l] * 100:7.3f} %" for l, n in enumerate(lam))
            if figures:
                line += (f"  dE {figures['delta_e'][k]:6.2f}  U_fov {figures['U_fov'][k] * 100:6.2f} %"
                         f"  U_EB {figures['U_EB'][k] * 100:6.2f} %")
            job.say(line + f"  min ESS {ess[k].min():,.0f}")
    else:
        band = lambda v: dict(nominal=v[0], mean=v[1:].mean(axis=0), std=v[1:].std(axis=0),
                              **{f"p{p}": np.percentile(v[1:], p, axis=0) for p in (5, 50, 95)})
        s = dict(efficiency=band(eff), **{k: band(v) for k, v in figures.items()}, min_ess=float(ess.min()))
        e["summary"] = s
        job.say(f"Tolerance band: sigma(ln s) = {ens.tolerance:g}, {K - 1} designs drawn "
                f"(nominal | mean +- std | 5 % / 50 % / 95 %)")
        row = lambda name, b, f, i=(): job.say(
            f"  {name:18s}: {b['nominal'][i] * f:8.3f} | {b['mean'][i] * f:8.3f} +- {b['std'][i] * f:7.3f} | "
            f"{b['p5'][i] * f:8.3f} / {b['p50'][i] * f:8.3f} / {b['p95'][i] * f:8.3f}")
        for l, n in enumerate(lam):
            row(f"Efficiency {n} %", s["efficiency"], 100.0, l)
        for key, name, f in (("delta_e", "Color dispersion", 1.0), ("U_fov", "FoV uniformity %", 100.0),
                             ("U_EB", "Eyebox uniform. %", 100.0)):
            if key in s:
                row(name, s[key], f)
        job.say(f"  smallest effective sample size: {s['min_ess']:,.0f}")
    if (ens.scales_array > 1.0).any():
        # (the what-if's limit, _report_what_if: an up-scaled channel is over-credited where a state's branch
        # efficiencies already sum to 1, so the figures of such designs -- a band's upper tail -- are too high)
        job.say("  note: scaled up -- unbiased only where the state's branch efficiencies still sum to <= 1; "
                "check the scaled LUTs (luts.scale_channel) or confirm with a direct run")
    out["ensemble"] = e


def _sources_set_up(job, sources):
    """The sources' record: ``weights`` float64 ``[K, R]`` (``engine.source_weights`` over the job's origins), their
    device copy, and the two device tensors the re-weighting adds to.  The tables' bytes are printed and checked against
    the device's free memory first."""
    import torch

    from .engine import source_weights
    weights = source_weights(job.points, job.R, sources)
    K = weights.shape[0]
    n_slabs, W = job.windows[1].shape
    # a table; the re-weighting's chunk scratch, the weights [K, R] and their transposed copy [R, 64 * chunks]
    per_source = n_slabs * W * 8
    fixed = lambda k: n_slabs * W * ENSEMBLE_CHUNK * 8 + job.R * (k + -(-k // ENSEMBLE_CHUNK) * ENSEMBLE_CHUNK) * 8
    free = int(torch.cuda.mem_get_info(job.dev)[0])
    job.say(f"Source what-ifs       : {K} sources, tables {K * per_source / 1e6:,.1f} MB "
            f"(+ {fixed(K) / 1e6:,.1f} MB while re-weighting; {free / 1e6:,.0f} MB free)")
    if K * per_source + fixed(K) > free:
        fits = K
        while fits > 0 and fits * per_source + fixed(fits) > free:
            fits -= 1
        raise ValueError(f"sources: {K} tables of {per_source / 1e6:,.1f} MB exceed the device's free memory "
                         f"({free / 1e6:,.0f} MB); the largest K that fits is {fits}")
    return SimpleNamespace(weights=weights, weights_dev=torch.from_numpy(weights).to(job.dev),
                           tables=torch.zeros((K, n_slabs, W), dtype=torch.float64, device=job.dev),
                           sums=torch.zeros((K, 2, job.scene.num_lmd), dtype=torch.int64, device=job.dev))


def _report_sources(job, out: dict, src, tables, sums, evaluate: bool, evaluate_on: str) -> None:
    """The sources' figures into ``out["sources"]`` and printed, one line per source (as ``_report_ensemble``'s)."""
    from .AR_system_evaluation_functions import evaluation_ensemble
    from .engine import ess_of_quanta
    shape = job.scene.eb_shape()
    t = tables.cpu().numpy()
    K = t.shape[0]
    A = t[:, :, 0].reshape((K,) + tuple(shape[:-2])).astype(np.float32) / job.num_rays / job.num_iter
    eff = np.array([[float(np.sum(A[k, l] * 3)) for l in range(A.shape[1])] for k in range(K)], dtype=np.float64)
    ess = ess_of_quanta(sums.cpu().numpy())
    s = dict(weights=src.weights, table=t, A=A, efficiency=eff, ess=ess, sums=sums.cpu().numpy())
    figures = {}
    if evaluate:
        figures = evaluation_ensemble(tables if evaluate_on == "device" else t, shape, job.R * job.num_iter, evaluate_on)
        s.update(figures)
    names = {0: "Blue", 1: "Green", 2: "Red"}
    lam = [names.get(l, str(l)) for l in range(eff.shape[1])]
    job.say(f"Source what-ifs: {K} sources (the same rays, re-weighted by entry class; per unit of projector power)")
    for k in range(K):
        line = f"  source {k:3d}: " + "  ".join(f"{n} {eff[k, l] * 100:7.3f} %" for l, n in enumerate(lam))
        if figures:
            line += (f"  dE {figures['delta_e'][k]:6.2f}  U_fov {figures['U_fov'][k] * 100:6.2f} %"
                     f"  U_EB {figures['U_EB'][k] * 100:6.2f} %")
        job.say(line + f"  min ESS {ess[k].min():,.0f}")
    out["sources"] = s


def _report_source_counts(job, out: dict, counts, cells) -> None:
    """The per-class counts into ``out["source_counts"]``, per wavelength the delivered efficiency of the TE half and of
    the TM half of the input printed, and, with ``cells = (H, W)``, the entrance-pupil map into ``out["source_map"]``."""
    c = counts.cpu().numpy()
    out["source_counts"] = c
    half = job.R // 2
    launched = job.nx * job.ny * half * job.num_iter                   # rays of one polarisation at one wavelength
    names = {0: "Blue", 1: "Green", 2: "Red"}
    used = int((c[:, 0, :half].sum(axis=0) + c[:, 0, half:].sum(axis=0) > 0).sum())
    job.say(f"Delivered light by input polarisation ({used:,} of {half:,} entry points delivered any)")
    job.say(f"  {'':10s}{'TE half':>12s}{'TM half':>12s}")
    for l in range(c.shape[0]):
        te, tm = int(c[l, 0, :half].sum()), int(c[l, 0, half:].sum())
        job.say(f"  {names.get(l, str(l)):10s}{te / launched * 100:11.3f}%{tm / launched * 100:11.3f}%")
    if cells is not None:
        from .engine import source_map
        delivered, per_cell = source_map(job.points, c, *cells)
        out["source_map"] = dict(delivered=delivered, launched=per_cell)


def _report_polarisation(job, out: dict, table, stokes, analyser, frame: str, evaluate: bool, evaluate_on: str) -> None:
    """The Stokes tables into ``out["stokes"]``, the polarisation of the delivered light into ``out["polarisation"]`` and
    printed per wavelength, and, with an analyser, the analysed table's efficiencies and evaluation into
    ``out["analysed"]`` (as ``_report`` and ``_evaluate`` give them for the job's own table)."""
    from .AR_system_evaluation_functions import (analyser_table, evaluation_from_perceive, evaluation_from_window_sums,
                                                 perceive_from_window_sums, polarisation_from_stokes, stokes_rotate)
    shape = job.scene.eb_shape()
    nl, ny, nx = (int(v) for v in shape[:3])
    out["stokes"] = stokes.cpu().numpy()
    S = stokes
    if frame == "lab":
        # slab (l, n, m) of FoV (m, n): its TE axis lies at the out-coupled azimuth + 90 degrees (paraxial)
        import torch
        ph = np.asarray(job.geom.angles["phi_in_ic"], dtype=np.float64)[0]   # [nx, ny]
        psi = np.broadcast_to(ph.T[None] + np.pi / 2, (nl, ny, nx)).reshape(-1)
        S = stokes_rotate(stokes, torch.from_numpy(np.ascontiguousarray(psi)).to(stokes.device))
    N0 = table[:, 0].cpu().numpy().astype(np.float64)                      # the slabs' totals
    S0 = (S[:, :, 0].cpu().numpy()).astype(np.float64)                     # [3, n_slabs]
    per_fov = polarisation_from_stokes(N0[:, None], S0[:, :, None])
    dop_fov = per_fov["dop"][:, 0].reshape(nl, ny, nx)
    whole = polarisation_from_stokes(N0.reshape(nl, -1).sum(axis=1)[:, None],
                                     S0.reshape(3, nl, -1).sum(axis=2)[:, :, None])
    mean, dop = whole["mean"][:, :, 0].T, whole["dop"][:, 0]               # [L, 3], [L]
    out["polarisation"] = dict(frame=frame, mean=mean, dop=dop, dop_fov=dop_fov)
    names = {0: "Blue", 1: "Green", 2: "Red"}
    basis = "each FoV's own TE / TM basis" if frame == "fov" else "the plate's axes, paraxial"
    job.say(f"Polarisation of the delivered light ({basis})")
    job.say(f"  {'':10s}{'s1':>9s}{'s2':>9s}{'s3':>9s}{'DoP':>9s}{'DoP over the FoVs: min / mean / max':>40s}")
    for k in range(nl):
        d = dop_fov[k][np.isfinite(dop_fov[k])]
        spread = f"{d.min():.3f} / {d.mean():.3f} / {d.max():.3f}" if d.size else "-"
        job.say(f"  {names.get(k, str(k)):10s}{mean[k, 0]:9.4f}{mean[k, 1]:9.4f}{mean[k, 2]:9.4f}{dop[k]:9.4f}{spread:>40s}")
    if analyser is None:
        return
    atab = analyser_table(table, S, np.deg2rad(analyser))
    A = atab[:, 0].cpu().numpy().reshape(shape[:-2]).astype(np.float32) / job.num_rays / job.num_iter
    eff = {names.get(k, str(k)): float(np.sum(A[k] * 3)) for k in range(A.shape[0])}
    a = dict(theta_deg=analyser, frame=frame, table=atab.cpu().numpy(), A=A, efficiency=eff)
    job.say(f"Through a linear polariser at {analyser:g} degrees ({frame} frame)")
    for c in ("Red", "Green", "Blue"):
        if c in eff:
            job.say(f"Efficiency ({c:5s})    : {eff[c] * 100:8.3f} %")
    if evaluate:
        divisor = job.R * job.num_iter
        if evaluate_on == "device":
            *figures, _ = evaluation_from_window_sums(atab.contiguous(), shape, divisor, image="center")
        else:
            *figures, _ = evaluation_from_perceive(perceive_from_window_sums(a["table"], shape, divisor))
        a["delta_e"], a["U_fov"], a["U_EB"] = (float(v) for v in figures)
        job.say(f"Color dispersion      : {a['delta_e']:8.2f}")
        job.say(f"FoV uniformity        : {a['U_fov'] * 100:8.2f} %")
        job.say(f"Eyebox uniformity     : {a['U_EB'] * 100:8.2f} %")
    out["analysed"] = a


def _gather_paths(job):
    """The job's path list on rank 0 (None elsewhere), sorted by (tag, global id, step) (``_gather_list``)."""
    from .engine import PATH_DTYPE, PathListOverflow, sort_paths
    return _gather_list(job, job.paths.list, PATH_DTYPE, sort_paths, PathListOverflow, "path", "records")


def _report_paths(job, out: dict, records, selected, fmap, fp) -> None:
    """The path list into ``out`` and, per wavelength, the rays selected, the records kept and the mean draws per
    selected ray printed."""
    from .engine import path_kind, path_lmd
    out["paths"] = records
    out["paths_selected"] = selected.cpu().numpy() if hasattr(selected, "cpu") else np.asarray(selected)
    if fmap is not None:
        out["paths_footprint"] = fmap.cpu().numpy()
        out["paths_footprint_plan"] = fp.as_dict()
    names = {0: "Blue", 1: "Green", 2: "Red"}
    l, draw = path_lmd(records), ~np.isin(path_kind(records), (1, 5))
    what = "every ray" if job.paths.classes is None else ", ".join(job.paths.classes)
    job.say(f"Ray paths kept ({what}): {len(records):,} records")
    job.say(f"  {'':10s}{'rays selected':>15s}{'records':>15s}{'draws per ray':>15s}")
    for k in range(job.scene.num_lmd):
        n, r, d = int(out["paths_selected"][k]), int((l == k).sum()), int((draw & (l == k)).sum())
        job.say(f"  {names.get(k, str(k)):10s}{n:15,d}{r:15,d}{(d / n if n else 0.0):15.2f}")


def _gather_hits(job):
    """The job's hit list on rank 0 (None elsewhere), sorted by (tag, global id) (``_gather_list``)."""
    from .engine import HIT_DTYPE, HitListOverflow, sort_hits
    return _gather_list(job, job.hits, HIT_DTYPE, sort_hits, HitListOverflow, "hit", "out-couplings")


def _gather_list(job, hl, dtype, sort, overflow, what, counted):
    """A record list of the job (``engine.HitList``, ``engine.PathList``) on rank 0 (None elsewhere), sorted: every rank
    checks its own list for overflow (together: a rank whose list overflowed raises on every rank), the counts are
    all-gathered, and the stored records gathered as buffers padded to the largest."""
    import torch
    import torch.distributed as dist
    n, cap = hl.count(), hl.capacity
    counts = torch.tensor([n, min(n, cap), cap], dtype=torch.int64, device=job.dev)
    every = [counts]
    if job.world > 1:
        every = [torch.zeros_like(counts) for _ in range(job.world)]
        dist.all_gather(every, counts)
    every = [tuple(int(v) for v in t.cpu()) for t in every]
    over = [(r, c) for r, c in enumerate(every) if c[0] > c[2]]
    if over:
        raise overflow("; ".join(f"rank {r}: the {what} list counted {c[0]} {counted} but has room for {c[2]} "
                                 f"(a capacity of {c[0]} would have sufficed)" for r, c in over))
    if job.world == 1:
        return hl.records()
    width = max(c[1] for c in every)
    mine = torch.zeros((width, dtype.itemsize), dtype=torch.uint8, device=job.dev)
    mine[:every[job.rank][1]] = hl.buffer[:every[job.rank][1]]
    parts = [torch.zeros_like(mine) for _ in range(job.world)] if job.rank == 0 else None
    dist.gather(mine, parts, dst=0)
    if job.rank != 0:
        return None
    rec = np.concatenate([p[:c[1]].cpu().numpy().reshape(-1).view(dtype) for p, c in zip(parts, every)])
    return sort(rec)


def _report_hits(job, out: dict, records) -> None:
    """The hit list into ``out`` and, per wavelength, its out-couplings inside and beside the eyebox printed."""
    from .engine import hit_inside, hit_lmn
    out["hits"] = records
    out["hit_count"] = int(len(records))
    names = {0: "Blue", 1: "Green", 2: "Red"}
    l = hit_lmn(records, job.nx, job.ny)[0]
    inside = hit_inside(records)
    job.say(f"Out-couplings kept: {len(records):,} records")
    job.say(f"  {'':10s}{'inside eyebox':>15s}{'beside eyebox':>15s}{'beside share':>15s}")
    for k in range(job.scene.num_lmd):
        a, b = int((inside & (l == k)).sum()), int((~inside & (l == k)).sum())
        job.say(f"  {names.get(k, str(k)):10s}{a:15,d}{b:15,d}{(b / (a + b) if a + b else 0.0) * 100:14.2f}%")


def _report_footprint(job, out: dict, fmap) -> None:
    """The footprint map into ``out`` and its totals printed per wavelength (``engine.FOOTPRINT_CHANNELS``)."""
    from .engine import FOOTPRINT_CHANNELS
    out["footprint"] = m = fmap.cpu().numpy()
    out["footprint_plan"] = job.footprint[0].as_dict()
    names = {0: "Blue", 1: "Green", 2: "Red"}
    tot = m.sum(axis=(2, 3))   # [num_lmd, 9]
    job.say(f"Footprint ({m.shape[2]} x {m.shape[3]} cells): interactions per state, and where the light is lost / leaves")
    job.say("  " + " " * 10 + "".join(f"{c:>15s}" for c in FOOTPRINT_CHANNELS))
    for l in range(m.shape[0]):
        job.say(f"  {names.get(l, str(l)):10s}" + "".join(f"{int(v):15,d}" for v in tot[l]))


def _report(job, out: dict, grid, table, reps=None) -> None:
    """Step 5's efficiencies, into ``out`` and printed: ``A`` from the host grid, or from the table's slab totals
    -- integer counts: below 2^24 the float32 cast is the value np.sum gives on the host.  ``reps``: the replica
    tables ``table`` is the sum of: their standard errors (``efficiency_error_bars``) too."""
    num_rays, num_iter, kern_s = job.num_rays, job.num_iter, out["gpu_seconds"]
    if table is not None:
        A = table[:, 0].cpu().numpy().reshape(job.scene.eb_shape()[:-2]).astype(np.float32) / num_rays / num_iter
    else:
        A = np.sum(grid, axis=(-2, -1)) / num_rays / num_iter
    names = {0: "Blue", 1: "Green", 2: "Red"}
    eff = {names.get(k, str(k)): float(np.sum(A[k] * 3)) for k in range(A.shape[0])}
    eff_se = None
    if reps is not None:
        from .AR_system_evaluation_functions import efficiency_error_bars
        bars = efficiency_error_bars(reps, job.scene.eb_shape(), num_rays, num_iter)
        eff_se = {names.get(k, str(k)): float(v) for k, v in enumerate(bars["efficiency_se"])}
        out.update(A_se=bars["A_se"], efficiency_se=eff_se)
    job.say("Simulation finished.")
    job.say(f"Number of rays traced : {num_rays * num_iter:,}")
    job.say(f"GPU calculation time  : {kern_s:.4f} s  ({out['bounces'] / max(kern_s, 1e-12):.3e} ray-bounces/s)")
    for c in ("Red", "Green", "Blue"):
        if c in eff:
            job.say(f"Efficiency ({c:5s})    : {eff[c] * 100:8.3f} %" +
                    (f"  +- {eff_se[c] * 100:.3f}" if eff_se is not None else ""))
    out.update(A=A, efficiency=eff)
    if grid is not None:
        out["matrix_EB"] = grid


def _evaluate(job, out: dict, grid, table, evaluate_on: str, keep_image: bool, png, reps=None) -> None:
    """Steps 5-6, into ``out`` and printed: the evaluation -- of the table where it lives, of the table's host
    copy, or of the host grid (MAIN:197-198) -- then the centre view and its PNG.  ``reps``: the replica tables
    ``table`` is the sum of: the leave-one-out tables are evaluated as well and jackknifed (``evaluation_error_bars``)."""
    from .AR_system_evaluation_functions import (evaluation, evaluation_error_bars, evaluation_from_perceive,
                                                 evaluation_from_window_sums, perceive_from_window_sums)
    shape, divisor = job.scene.eb_shape(), job.R * job.num_iter
    whole = evaluate_on == "host" or keep_image   # ``image``: every eye position's, else the centre one alone
    se = None
    if reps is not None:   # the figures themselves come from ``table`` below, exactly as without error bars
        se = evaluation_error_bars(reps, shape, divisor, evaluate_on, image=None)
        out.update(delta_e_se=se["delta_e_se"], U_fov_se=se["U_fov_se"], U_EB_se=se["U_EB_se"], jackknife=se["jackknife"])
    if evaluate_on == "device":
        *figures, image = evaluation_from_window_sums(table, shape, divisor, image="all" if whole else "center")
    elif table is not None:
        *figures, image = evaluation_from_perceive(perceive_from_window_sums(table.cpu().numpy(), shape, divisor))
    else:
        *figures, image = evaluation(grid / job.R / job.num_iter)
    delta_e, U_fov, U_EB = (float(v) for v in figures)
    out.update(delta_e=delta_e, U_fov=U_fov, U_EB=U_EB)
    if whole:
        out["output_image"] = image
    out["center_view"] = eyebox_center_view(image) if whole else center_view_u8(image)
    if png:
        write_png(png, out["center_view"])
        job.say(f"Wrote {png}")
    pm = (lambda k, scale: f"  +- {se[k] * scale:.2f}") if se is not None else (lambda k, scale: "")
    job.say(f"Color dispersion      : {delta_e:8.2f}" + pm("delta_e_se", 1))
    job.say(f"FoV uniformity        : {U_fov * 100:8.2f} %" + pm("U_fov_se", 100))
    job.say(f"Eyebox uniformity     : {U_EB * 100:8.2f} %" + pm("U_EB_se", 100))


def eyebox_center_view(output_image: np.ndarray) -> np.ndarray:
    """The image MAIN:199-203 exports: ``output_image[:, :, :, 0, n_epx - 1]`` (first eye row, last eye
    column) as uint8 (``* 255`` then truncation), rows flipped -- uint8 RGB [n_FOVy, n_FOVx, 3].  (The
    reference converts it to BGR for cv2.imwrite, which stores the RGB image in the PNG.)"""
    n_epx = output_image.shape[4]
    return center_view_u8(output_image[:, :, :, 0, n_epx - 1])


def center_view_u8(center: np.ndarray) -> np.ndarray:
    """One eye position's image ``[n_FOVy, n_FOVx, 3]`` as ``eyebox_center_view`` exports it."""
    return np.ascontiguousarray(np.flipud((center * 255).astype(np.uint8)))


def write_png(path: str, rgb: np.ndarray) -> None:
    """8-bit RGB PNG (filter 0 on every row, zlib), without OpenCV / PIL."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected an [H, W, 3] uint8 image")
    h, w = a.shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    raw = b"".join(b"\x00" + a[r].tobytes() for r in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """Decoder of write_png's files (8-bit RGB, filter 0), for the tests."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3).copy()


def main(argv=None):
    ap = argparse.ArgumentParser(description="MI355X full-colour waveguide ray tracing (reference MAIN flow)")
    ap.add_argument("--num-fov-x", type=int, default=100)
    ap.add_argument("--num-fov-y", type=int, default=75)
    ap.add_argument("--rays-per-fov", type=int, default=5000)
    ap.add_argument("--num-iter", type=int, default=4)
    ap.add_argument("--lut-dir", default=None, help="directory with lut_*_fullColor.npy (default: synthetic)")
    ap.add_argument("--lut-seed", type=int, default=0)
    ap.add_argument("--lut-profile", default="default")
    ap.add_argument("--point-seed", type=int, default=None)
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--fuse", choices=["auto", "yes", "no"], default="auto",
                    help="num_iter chained traces as one fused launch (auto: when a GPU traces <= 4M rays)")
    ap.add_argument("--no-fuse", action="store_true", help="same as --fuse no")
    ap.add_argument("--eyebox", choices=["host", "device", "windows"], default="host",
                    help="where the eyebox grid is reduced after the trace: host (the reference's flow: the whole "
                         "grid is copied back), device (per-slab pupil sums on the GPU; the grid stays there) or "
                         "windows (the trace counts into the pupil-sum table itself; no grid is allocated)")
    ap.add_argument("--evaluate", choices=["host", "device"], default="host",
                    help="where the evaluation's colour math runs: host (numpy) or device (wgrt_eyebox_evaluate on "
                         "the window-sum table; needs --eyebox device or windows)")
    ap.add_argument("--footprint", default="", metavar="HxW",
                    help="also count every interaction into a per-wavelength plate map of H x W cells (interactions per "
                         "state, where light is lost and where it out-couples); not with --budget, --error-bars or "
                         "--estimator expected")
    ap.add_argument("--footprint-out", default="", metavar="FILE.npy", help="save the footprint map there (numpy)")
    ap.add_argument("--hits", nargs="?", const=-1, default=None, type=int, metavar="N",
                    help="also keep every out-coupling, inside the eyebox or beside it, as a record (x, y, global ray id, "
                         "tile, flags): N records of room (default: an eighth of the traces)")
    ap.add_argument("--hits-out", default="", metavar="FILE.npy", help="save the records there (numpy structured array)")
    ap.add_argument("--paths", default="", metavar="CLASS[,CLASS...]",
                    help="also record which way the selected rays went, one record per Monte-Carlo draw: 'all', or fate "
                         "classes such as eyebox, left_plate, lost_fc (a fate launch per iteration then chooses the rays); "
                         "not with --budget, --error-bars, --estimator expected, --footprint or --hits")
    ap.add_argument("--paths-capacity", type=int, default=None, metavar="N", help="records of room in the path list")
    ap.add_argument("--paths-out", default="", metavar="FILE.npy", help="save the path records there (numpy structured array)")
    ap.add_argument("--paths-footprint", default="", metavar="HxW",
                    help="also reduce the path list into a footprint map of H x W cells: the conditional footprint")
    ap.add_argument("--sensitivity", nargs="?", const=8, default=None, type=int, metavar="K",
                    help="also count the branches the delivered rays took per channel (state, coupler slice, branch) and "
                         "print, per wavelength, the K (default 8) channels whose efficiency the result is most sensitive "
                         "to; needs --eyebox windows; not with --budget, --error-bars, --estimator expected, --footprint, "
                         "--hits or --paths")
    ap.add_argument("--sensitivity-out", default="", metavar="FILE.npy", help="save the sensitivity tables there (numpy)")
    ap.add_argument("--what-if", default="", metavar="CHANNEL=SCALE[,...]",
                    help="also the figures of the design whose channels' efficiencies are scaled so, from the same rays "
                         "re-weighted, e.g. 'r4[2].b3=1.2,r2[0].b2=0.9'; needs --eyebox windows")
    ap.add_argument("--designs", default="", metavar="FILE.json",
                    help="also the figures of every design of a list, from the same rays re-weighted in one pass: a JSON "
                         "list of {CHANNEL: SCALE} objects ({}: the nominal design); needs --eyebox windows; not with "
                         "--tolerance")
    ap.add_argument("--tolerance", type=float, default=None, metavar="SIGMA",
                    help="also a tolerance band: the figures of random designs whose channel efficiencies are off by "
                         "ln s ~ N(0, SIGMA^2), from the same rays; needs --eyebox windows")
    ap.add_argument("--tolerance-designs", type=int, default=64, metavar="K", help="designs of the band, the nominal included")
    ap.add_argument("--tolerance-seed", type=int, default=0, metavar="S", help="seed of the band's draws")
    ap.add_argument("--tolerance-channels", default="", metavar="PAT[,PAT...]",
                    help="the channels that vary, as patterns over their names, e.g. 'r4[*].b3,r5[*].b3' (default: all)")
    ap.add_argument("--ensemble-out", default="", metavar="FILE.npz",
                    help="save the ensemble's scales, tables, weight sums and figures there (numpy)")
    ap.add_argument("--sources", default="", metavar="FILE.json",
                    help="also the figures of every projector pupil of a list, from the one trace's hit list re-weighted "
                         "by entry class: a JSON list of objects with the keys centre [x, y], diameter, sigma, te, tm or "
                         "weights ({}: the nominal source); needs --eyebox windows; implies --hits")
    ap.add_argument("--sources-out", default="", metavar="FILE.npz",
                    help="save the sources' weights, tables, weight sums and figures there (numpy)")
    ap.add_argument("--source-counts", action="store_true",
                    help="with --hits: also count the out-couplings per entry class and print, per wavelength, the "
                         "delivered efficiency of the TE half and of the TM half of the input")
    ap.add_argument("--source-map", default="", metavar="HxW",
                    help="with --source-counts: also the entrance-pupil map of H x W cells, delivered and launched")
    ap.add_argument("--source-map-out", default="", metavar="FILE.npz", help="save the entrance-pupil map there (numpy)")
    ap.add_argument("--polarisation", action="store_true",
                    help="also the polarisation of the delivered light: Stokes tables beside the window table, the mean "
                         "Stokes vector and degree of polarisation per wavelength; needs --eyebox windows; not with "
                         "--budget, --error-bars, --estimator expected, --footprint, --hits, --paths, --sensitivity or "
                         "--what-if")
    ap.add_argument("--analyser", type=float, default=None, metavar="DEG",
                    help="with --polarisation: also the efficiencies and the evaluation through an ideal linear polariser "
                         "at DEG degrees, from the same trace")
    ap.add_argument("--analyser-frame", choices=["fov", "lab"], default="fov",
                    help="the frame of the Stokes vectors and the analyser: each FoV's own TE / TM basis, or the plate's "
                         "axes (each FoV's table turned by its out-coupled azimuth + 90 degrees; paraxial)")
    ap.add_argument("--polarisation-out", default="", metavar="FILE.npy", help="save the Stokes tables there (numpy int64)")
    ap.add_argument("--budget", action="store_true",
                    help="also report where every ray ended: per-ray fates, their per-tile census and the loss budget "
                         "per wavelength (the traces then run as plain single launches)")
    ap.add_argument("--error-bars", type=int, default=0, metavar="B",
                    help="Monte-Carlo standard errors of every printed figure from B replica window tables filled by ray "
                         "id and jackknifed (needs --eyebox windows and B dividing rays-per-fov / 2)")
    ap.add_argument("--estimator", choices=["analog", "expected"], default="analog",
                    help="expected: score every out-coupler visit with its out-coupling probability (needs --eyebox "
                         "windows): the same expectation, less variance")
    ap.add_argument("--json", default=None, help="write scalar results here")
    ap.add_argument("--png", default="Eyebox Center View.png",
                    help="the eyebox-center image (MAIN:199-203); empty string: do not write it")
    a = ap.parse_args(argv)
    import torch
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    def cells(flag, text):   # "HxW" -> (H, W); None for a flag not given
        if not text:
            return None
        try:
            hw = tuple(int(v) for v in text.lower().split("x"))
        except ValueError:
            hw = ()
        if len(hw) != 2:
            ap.error(f"{flag} takes HxW, got {text!r}")
        return hw
    what_if = None
    if a.what_if:
        what_if = {}
        for item in a.what_if.split(","):
            name, eq, value = item.partition("=")
            try:
                what_if[name.strip()] = float(value)
            except ValueError:
                eq = ""
            if not eq or not name.strip():
                ap.error(f"--what-if takes CHANNEL=SCALE[,CHANNEL=SCALE...], got {a.what_if!r}")
    if a.sensitivity is not None and a.sensitivity < 1:
        ap.error(f"--sensitivity takes the number K >= 1 of channels to print, got {a.sensitivity}")
    designs = None
    if a.designs:
        try:
            with open(a.designs) as f:
                designs = json.load(f)
        except (OSError, ValueError) as e:
            ap.error(f"--designs: cannot read {a.designs!r}: {e}")
        if not isinstance(designs, list) or not designs or not all(isinstance(d, dict) for d in designs):
            ap.error(f"--designs takes a JSON file holding a non-empty list of {{CHANNEL: SCALE}} objects, got {a.designs!r}")
    if a.tolerance is not None and not (a.tolerance > 0 and np.isfinite(a.tolerance)):
        ap.error(f"--tolerance takes a sigma > 0, got {a.tolerance}")
    if a.tolerance_designs < 2:
        ap.error(f"--tolerance-designs takes K >= 2 (the nominal design and one drawn), got {a.tolerance_designs}")
    if designs is not None and a.tolerance is not None:
        ap.error("--designs and --tolerance exclude each other")
    sources = None
    if a.sources:
        try:
            with open(a.sources) as f:
                sources = json.load(f)
        except (OSError, ValueError) as e:
            ap.error(f"--sources: cannot read {a.sources!r}: {e}")
        if not isinstance(sources, list) or not sources or not all(isinstance(d, dict) for d in sources):
            ap.error(f"--sources takes a JSON file holding a non-empty list of source objects, got {a.sources!r}")
    if a.source_map and not a.source_counts:
        ap.error("--source-map needs --source-counts")
    if a.source_counts and a.hits is None and sources is None:
        ap.error("--source-counts needs --hits")
    footprint = cells("--footprint", a.footprint)
    paths_footprint = cells("--paths-footprint", a.paths_footprint)
    res = run(a.num_fov_x, a.num_fov_y, a.rays_per_fov, a.num_iter, lut_dir=a.lut_dir, lut_seed=a.lut_seed,
              lut_profile=a.lut_profile, point_seed=a.point_seed, evaluate=not a.no_eval,
              fuse=False if a.no_fuse else {"auto": None, "yes": True, "no": False}[a.fuse],
              png=a.png or None, eyebox=a.eyebox, evaluate_on=a.evaluate, budget=a.budget, error_bars=a.error_bars, estimator=a.estimator,
              footprint=footprint, hits=None if a.hits is None else (True if a.hits < 0 else a.hits),
              paths=None if not a.paths else (a.paths.split(",") if "," in a.paths else a.paths),
              paths_capacity=a.paths_capacity, paths_footprint=paths_footprint, sensitivity=a.sensitivity,
              what_if=what_if, polarisation=a.polarisation, analyser=a.analyser, analyser_frame=a.analyser_frame,
              designs=designs, tolerance=a.tolerance, tolerance_designs=a.tolerance_designs,
              tolerance_seed=a.tolerance_seed,
              tolerance_channels=[p for p in a.tolerance_channels.split(",") if p] or None,
              sources=sources, source_counts=a.source_counts, source_map=cells("--source-map", a.source_map))
    if a.sources_out and "sources" in res:   # (rank 0 has the tables)
        np.savez(a.sources_out, **{k: v for k, v in res["sources"].items() if isinstance(v, np.ndarray)})
    if a.source_map_out and "source_map" in res:
        np.savez(a.source_map_out, counts=res["source_counts"], **res["source_map"])
    if a.ensemble_out and "ensemble" in res:   # (rank 0 has the tables)
        e = res["ensemble"]
        np.savez(a.ensemble_out, channels=np.array(e["channels"]),
                 **{k: v for k, v in e.items() if isinstance(v, np.ndarray)})
    if a.polarisation_out and "stokes" in res:   # (rank 0 has the tables)
        np.save(a.polarisation_out, res["stokes"])
    if a.sensitivity_out and "sensitivity" in res:   # (rank 0 has the tables)
        np.save(a.sensitivity_out, res["sensitivity"])
    if a.footprint_out and "footprint" in res:   # (rank 0 has the map)
        np.save(a.footprint_out, res["footprint"])
    if a.hits_out and "hits" in res:   # (rank 0 has the list)
        np.save(a.hits_out, res["hits"])
    if a.paths_out and "paths" in res:   # (rank 0 has the list)
        np.save(a.paths_out, res["paths"])
    if a.json and (not dist.is_initialized() or dist.get_rank() == 0):
        keep = {k: v for k, v in res.items() if isinstance(v, (int, float, dict, str))}
        if "what_if" in keep:   # (its arrays stay out, as the top level's do; the ESS goes as a list)
            keep["what_if"] = {k: (v.tolist() if k == "ess" else v) for k, v in keep["what_if"].items()
                               if k == "ess" or isinstance(v, (int, float, dict, str))}
        if "ensemble" in keep:   # (the per-design figures and the summary go as lists; the tables stay out)
            lists = lambda d: {k: (lists(v) if isinstance(v, dict) else np.asarray(v).tolist()) for k, v in d.items()}
            keep["ensemble"] = lists({k: v for k, v in keep["ensemble"].items()
                                      if k in ("efficiency", "ess", "delta_e", "U_fov", "U_EB", "summary", "channels")})
        if "sources" in keep:   # (the per-source figures go as lists; the weights and the tables stay out)
            keep["sources"] = {k: np.asarray(v).tolist() for k, v in keep["sources"].items()
                               if k in ("efficiency", "ess", "delta_e", "U_fov", "U_EB")}
        keep.pop("source_map", None)
        with open(a.json, "w") as f:
            json.dump(keep, f, indent=1)
    if dist.is_initialized():
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
