"""The Jones-vector trace's kernel table, stated for the tests: which instantiations of ``jones_body`` the library builds
(``csrc/wgrt_trace.hip`` ``JonesKernels``), which test launches each of them, the four scenes that select the
single-wavelength and AMP axes, and one adapter per mode that launches an entry and checks what it leaves.

An entry is ``(mode, byte, wide, fused, single, amp)``: the index of the C++ table ``k[mode][byte locator][64-bit
cells][fused][single wavelength][AMP]``, the mode in ``TraceMode``'s order.  ``tests/test_kernel_table.py`` (no GPU) holds
this statement against the library's own (``wgrt_debug_trace_kernels``); ``tests/test_gpu_kernel_table.py`` launches
every entry of ``SWEPT`` and asserts, through ``wgrt_debug_last_trace_kernel``, that the launch ran that entry.

The four cases exist on every waveguide design of ``tests/_designs.py`` (``case(name, design)``, or the name
``kt_rgb@D32``; a bare name is the default design's): ``tests/test_gpu_designs.py`` runs the adapters on 32 polygons.

The checkers and comparators are the sink tests' own, imported from their modules: the case names below are known to
each module's ``_case``, so ``checked`` and ``_trace`` of that module work on them as on its own cases."""
from types import SimpleNamespace

import numpy as np

# -- the table ---------------------------------------------------------------------------------------------------------

MODES = ("plain", "timeline", "learn", "chain", "fate", "replicas", "expected", "footprint", "hits", "paths", "visits",
         "stokes")                                          # TraceMode's order (csrc/wgrt_trace_mode.h)
SINKS = MODES[4:]


def _add(mode, fused, single, amp, wide=True):
    """``JonesKernels::add``: one instantiation in both locator forms and (``wide``) both cell widths."""
    return {(MODES.index(mode), byte, w, int(fused), int(single), int(amp)) for byte in (0, 1)
            for w in ((0, 1) if wide else (0,))}


def _add_amp(mode, fused, single):
    return _add(mode, fused, single, False) | _add(mode, fused, single, True)


def _add_single_amp(mode, fused):
    return _add_amp(mode, fused, False) | _add_amp(mode, fused, True)


# JonesKernels' constructor, line for line
RULES = [
    _add_single_amp("plain", False),                        # every combination: 32
    _add_single_amp("plain", True),
    _add("timeline", False, False, False, wide=False),      # 32-bit cells, full colour, no AMP: 4
    _add("timeline", True, False, False, wide=False),
    _add("learn", False, False, False),                     # full colour, no AMP: 4
    _add_amp("chain", False, False),                        # full colour: 8
    *[_add_single_amp(sink, False) for sink in SINKS],      # the sinks: single launches, 16 each
]
BUILT = frozenset().union(*RULES)


def mask():
    """``BUILT`` in the shape of ``_lib.trace_kernels``: uint8 ``[modes, 2, 2, 2, 2, 2]``."""
    m = np.zeros((len(MODES), 2, 2, 2, 2, 2), np.uint8)
    for e in BUILT:
        m[e] = 1
    return m


def entry_id(e):
    """``stokes-word-64-single-amp``: mode, locator form, cell width, then the axes that are on."""
    mode, byte, wide, fused, single, amp = e
    return "-".join([MODES[mode], "byte" if byte else "word", "64" if wide else "32"] +
                    [n for n, on in (("fused", fused), ("single", single), ("amp", amp)) if on])


# -- who launches what -------------------------------------------------------------------------------------------------

# Entries that faulted or hung on the GPU when the sweep first launched them and whose cause is not found: entry ->
# reason.  Empty unless that happens; never longer than the entries that faulted.
EXCLUDED = {}

# Entries another test owns (it asserts ``last_trace_kernel`` itself): the debug timeline needs its own buffer and the
# learning launch a scene that still learns, so neither fits the sweep's adapters.
OWNED = {
    **{e: "tests/test_gpu_byte_locator.py::test_timeline_kernels_in_both_forms"
       for e in BUILT if MODES[e[0]] == "timeline"},
    **{e: "tests/test_gpu_auto_order.py::test_learn_then_ordered_launch_is_exact"
       for e in BUILT if MODES[e[0]] == "learn" and e[1] == 1},
    **{e: "tests/test_gpu_auto_order.py::test_learning_launch_over_the_word_locator"
       for e in BUILT if MODES[e[0]] == "learn" and e[1] == 0},
}
SWEPT = sorted(e for e in BUILT if e not in OWNED and e not in EXCLUDED)

# -- the four cases ------------------------------------------------------------------------------------------------------

NX = NY = 7
R = 64
CASE_OF = {(0, 0): "kt_rgb", (1, 0): "kt_s2", (0, 1): "kt_rgb_amp", (1, 1): "kt_s2_amp"}   # (single, amp) -> name
CASES = {name: key for key, name in CASE_OF.items()}
# the CPU oracle's eyebox hits in one launch (tests/test_kernel_table.py asserts them)
ORACLE_HITS = {"kt_rgb": 176, "kt_s2": 73, "kt_rgb_amp": 71, "kt_s2_amp": 29}
_cases = {}


def on_design(name, design=None):
    """The name of case ``name`` on the waveguide design ``design`` (``tests/_designs.py``): ``kt_rgb@D32``; the default
    design's cases keep their bare names.  The sink modules' ``_case`` and ``checked`` take these names as they take
    the bare ones, so every adapter below runs on any design."""
    from tests import _designs as D
    base, _, d = name.partition("@")
    design = design or d or D.DEFAULT
    assert base in CASES and design in D.DESIGNS and (not d or d == design), (name, design)
    return base if design == D.DEFAULT else f"{base}@{design}"


def split(name):
    """``(bare case name, design)`` of a case name."""
    from tests import _designs as D
    base, _, d = name.partition("@")
    return base, d or D.DEFAULT


def is_case(name):
    """Whether ``name`` names one of the four cases, on any design."""
    from tests import _designs as D
    base, d = split(name) if isinstance(name, str) else (None, None)
    return base in CASES and d in D.DESIGNS and name == on_design(base, d)


def oracle_hits(name):
    from tests import _designs as D
    base, d = split(name)
    return ORACLE_HITS[base] if d == D.DEFAULT else D.ORACLE_HITS[d][base]


def case(name, design=None):
    """One of the four cases, built once and shared: 7 x 7 FoVs, 64 rays per block, full colour (9,408 rays) or
    wavelength 2 alone (3,136), on the default synthetic LUTs (seed 0) or, for AMP, the same with ``lut_fc2`` taken from
    ``synthetic_luts(geom, seed=3, profile="adversarial_polarizing")``: that table has non-unitary blocks, so every launch
    on the scene runs the AMP kernels, while the rest of the walk is the default profile's and still delivers.
    ``design`` (or a name ``kt_rgb@D32``): the same case on another waveguide design, with ``tests/_designs.CASE_R`` rays
    per block (64 wherever that delivers)."""
    name = on_design(name, design)
    if name not in _cases:
        from gpu_ray_tracing_for_waveguide_based_ar_display_amd.luts import synthetic_luts
        from tests import _designs as D
        base, d = split(name)
        single, amp = CASES[base]
        c = D.config(d, NX, NY, [2] if single else [0, 1, 2], R if d == D.DEFAULT else D.CASE_R[d][base])
        if amp:
            c.luts = dict(c.luts, lut_fc2=synthetic_luts(c.geom, seed=3, profile="adversarial_polarizing")["lut_fc2"])
        if single:
            c.wavelength = 2
            c.eb_shape = lambda: (NY, NX, 80, 120)
        _cases[name] = c
    return _cases[name]


_walks = {}


def walk(name, launches=1, design=None):
    """The plain CPU oracle's chained launches of case ``name`` (on ``design``), once per key and shared, read-only: per launch
    ``SimpleNamespace(rng, eb, table, per, fate, bounces, interactions)`` -- the RNG states, grid and window table after
    it, its per-ray bounces and fates, and the running totals of bounces and interactions."""
    name = on_design(name, design)
    key = (name, launches)
    if key not in _walks:
        from gpu_ray_tracing_for_waveguide_based_ar_display_amd import AR_system_evaluation_functions as E
        from oracle import OracleScene
        c = case(name)
        sc = OracleScene.from_geometry(c.geom, c.luts, wavelength=c.wavelength)
        rng, eb, total, inter, out = c.fresh_rng(), np.zeros(c.eb_shape(), np.float32), 0, 0, []
        for _ in range(launches):
            tot, per, fate, n_int = sc.trace(c.rays, rng, eb, per_ray_bounces=True, fate=True, interactions=True)
            total += tot
            inter += n_int
            w = SimpleNamespace(rng=rng.copy(), eb=eb.copy(), table=E.eyebox_window_sums(eb), per=per, fate=fate,
                                bounces=total, interactions=inter)
            for a in (w.rng, w.eb, w.table, w.per, w.fate):
                a.setflags(write=False)
            out.append(w)
        _walks[key] = out
    return _walks[key]


def same_walk(want, rng, stats, per=None, eb=None, table=None):
    """What a launch leaves beside its sink against ``want`` (an element of ``walk``), bit for bit; ``stats`` by the
    counters the oracle has: bounces, interactions, eyebox hits, and no bad ray and no hand-off given up."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import STAT
    np.testing.assert_array_equal(rng, want.rng)
    if per is not None:
        np.testing.assert_array_equal(per, want.per)
    if eb is not None:
        assert eb.tobytes() == want.eb.tobytes()
    if table is not None:
        assert table.tobytes() == want.table.tobytes()
    assert int(stats[STAT.bounces]) == want.bounces
    assert int(stats[STAT.interactions]) == want.interactions
    assert int(stats[STAT.eyebox_hits]) == int(round(float(want.eb.sum())))
    assert int(stats[STAT.bad_rays]) == 0 and int(stats[STAT.handoff_giveups]) == 0


# -- the adapters: launch one entry's mode through its public entry, compare with the mode's checker ------------------
# Each takes (name, scene, dev, variant, fused, debug) and returns the launch's stats.  ``scene`` is the caller's, so
# that it can ask the scene which kernel ran; the chain's adapter makes its own (``test_gpu_chain._Run``) and returns it.

REPLICAS = 4
CHAIN_STEPS = 3


def _plain(name, scene, dev, variant, fused, debug):
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import engine
    c = case(name)
    num_iter = 2 if fused else 1
    want = walk(name, 2)[num_iter - 1]
    plan = engine.WindowPlan()
    table = plan.new_table(scene)
    rng = torch.from_numpy(c.fresh_rng().view(np.int32)).to(dev)
    eb = torch.zeros(c.eb_shape(), dtype=torch.float32, device=dev)
    per = None if fused else torch.zeros(c.N, dtype=torch.int32, device=dev)   # (a fused launch takes none)
    stats = engine.new_stats(dev)
    trace = engine.trace_single if c.wavelength is not None else engine.trace_fullcolor
    trace(scene, engine.rays_to_device(c.rays, dev), rng, eb, stats=stats, per_ray_bounces=per, variant=variant,
          num_iter=num_iter, windows=(plan, table), debug=debug)
    torch.cuda.synchronize()
    stats = stats.cpu().numpy()
    same_walk(want, rng.cpu().numpy().view(np.uint32), stats, None if fused else per.cpu().numpy().view(np.uint32),
              eb.cpu().numpy(), table.cpu().numpy())
    plan.close()
    return stats


def _chain(name, scene, dev, variant, fused, debug):
    """Three chained steps on two workgroups (the chain tests' shape: a launch that fills the chip alone is not
    chained).  Makes its own scene; returns ``(stats, scene's last kernel, nonunitary blocks)``."""
    from tests import test_gpu_chain as M
    assert scene is None and not fused
    r = M._Run(case(name), dev, variant=variant, workgroups=2, debug=debug, windows=True)
    try:
        got = r.chain(CHAIN_STEPS).out()
        want = walk(name, CHAIN_STEPS)[-1]
        M._assert_oracle(got, dict(rng=want.rng, eb=want.eb, bounces=want.bounces, interactions=want.interactions))
        same_walk(want, got["rng"], got["stats"], eb=got["eb"], table=got["table"])
        return got["stats"], r.scene.last_trace_kernel(), r.scene.info()["nonunitary_blocks"]
    finally:
        r.close()


def _fate(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_fate as M
    want = walk(name)[0]
    got = M._launches(case(name), dev, 1, variant, True, per_ray=True, windows=True, scene=scene, debug=debug)[0]
    assert not (got["fate"] == 0xFF).any(), "a fate was not written"
    np.testing.assert_array_equal(got["fate"], want.fate)
    same_walk(want, got["rng"], got["stats"], got["bounces"], got["eb"], got["table"])
    return got["stats"]


def _replicas(name, scene, dev, variant, fused, debug):
    import torch
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import engine
    from tests import test_gpu_replicas as M
    c = M._case(name)
    want, rng_want, total = M.oracle_replicas(name, REPLICAS, 1)
    assert sum(int(want[b, :, 0].sum() > 0) for b in range(REPLICAS)) >= 2   # the replicas differ, and deliver
    plan = engine.WindowPlan()
    per = torch.zeros(c.N, dtype=torch.int32, device=dev)
    table, eb, rng, stats = M._trace(c, dev, REPLICAS, variant=variant, grid=True, scene=scene, plan=plan,
                                     per_ray_bounces=per, debug=debug)
    plan.close()
    assert table.tobytes() == want.tobytes()
    w = walk(name)[0]
    np.testing.assert_array_equal(rng_want, w.rng)
    assert total.tobytes() == w.eb.tobytes()
    same_walk(w, rng, stats, per.cpu().numpy().view(np.uint32), eb, table.sum(0))
    return stats


def _expected(name, scene, dev, variant, fused, debug):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd import engine
    from tests import test_gpu_expected as M
    chk = M.checked(name)
    assert chk["hits"] > 0 and chk["D"][:, 0].sum() > chk["hits"]
    plan = engine.WindowPlan()
    table, rng, stats, per = M._trace(M._case(name), dev, variant=variant, scene=scene, plan=plan, debug=debug)
    plan.close()
    M._in_bound(table, chk, name)
    np.testing.assert_array_equal(rng, chk["rng"])
    np.testing.assert_array_equal(per, chk["bounces"])
    same_walk(walk(name)[0], rng, stats, per)              # (an expected-value launch fills no grid)
    return stats


def _footprint(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_footprint as M
    chk = M.checked(name)
    got = M._trace(M._case(name), dev, variant=variant, scene=scene, debug=debug)
    assert got.map.dtype == np.int64 and got.map.shape == chk["map"].shape
    np.testing.assert_array_equal(got.map, chk["map"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    same_walk(walk(name)[0], got.rng, got.stats, got.per, got.eb, got.table)
    return got.stats


def _hits(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_hits as M
    chk = M.checked(name)
    got = M._trace(M._case(name), dev, variant=variant, scene=scene, debug=debug)
    M._same_list(got.rec, chk["rec"])
    assert got.count == len(chk["rec"]) == sum(chk["counts"]) > 0
    np.testing.assert_array_equal(got.rng, chk["rng"])
    same_walk(walk(name)[0], got.rng, got.stats, got.per, got.eb, got.table)
    return got.stats


def _paths(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_paths as M
    chk = M.checked(name)
    got = M._trace(M._case(name), dev, variant=variant, scene=scene, debug=debug)
    M._same_list(got.rec, chk["rec"])
    assert got.count == len(chk["rec"]) > 0 and M._unique(got.rec)
    np.testing.assert_array_equal(got.rng, chk["rng"])
    same_walk(walk(name)[0], got.rng, got.stats, got.per, got.eb, got.table)
    return got.stats


def _visits(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_visits as M
    chk = M.checked(name)
    got = M._trace(M._case(name), dev, variant=variant, scene=scene, debug=debug)
    M._same_rows(got.counts, got.ends, chk["counts"], chk["ends"])
    np.testing.assert_array_equal(got.rng, chk["rng"])
    same_walk(walk(name)[0], got.rng, got.stats, got.per, got.eb, got.table)
    return got.stats


def _stokes(name, scene, dev, variant, fused, debug):
    from tests import test_gpu_stokes as M
    chk = M.checked(name)
    got = M._trace(M._case(name), dev, variant=variant, scene=scene, debug=debug)
    M._within(got, chk, f"{name} variant {variant}")
    np.testing.assert_array_equal(got.rng, chk["rng"])
    same_walk(walk(name)[0], got.rng, got.stats, got.per, got.eb, got.table)
    return got.stats


ADAPTERS = {"plain": _plain, "chain": _chain, "fate": _fate, "replicas": _replicas, "expected": _expected,
            "footprint": _footprint, "hits": _hits, "paths": _paths, "visits": _visits, "stokes": _stokes}
