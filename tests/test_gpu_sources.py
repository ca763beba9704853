"""Source what-ifs on the GPU (``wgrt_hits_reweight_sources`` and ``wgrt_hits_source_counts`` through ``engine.HitList``):
the tables, the integer weight sums and the class counts of traced hit lists against the numpy checker
(``tests/_sources.py``) and the host twins, bytes against bytes; the chunk boundaries; empty and short lists;
``wgrt_visits_reweight_many`` after its fold kernel moved to the header both share; the driver's ``sources``."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib  # noqa: E402
from tests import _sources as S  # noqa: E402
from tests.test_gpu_hits import _trace  # noqa: E402
from tests.test_gpu_parity import _config  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5A
CASES = {"small": S.SMALL, "c2s": S.C2S}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _switches():
    yield
    _lib.set_byte_locator(True)
    _lib.set_reweight_layout(True)


_traced = {}


def traced(name, dev):
    """Two launches of case ``name`` tagged 0 and 1 into one list, once per module and read-only: the namespace of
    ``tests.test_gpu_hits._trace`` (``hl`` and ``scene`` left open) with ``c``, ``nl``, ``ranges`` and a ``plan``."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import WindowPlan
    if name not in _traced:
        c = _config(**CASES[name])
        got = _trace(c, dev, launches=2, keep=True)
        got.c, got.plan = c, WindowPlan()
        got.nl = 1 if c.wavelength is not None else 3
        got.ranges = np.ascontiguousarray(c.geom.eff_reg_FOV_range, dtype=np.float64)
        _traced[name] = got
    return _traced[name]


def _with_canary(shape, dtype, dev):
    """A zeroed tensor of ``shape`` at the front of a buffer whose last 64 elements are canaries."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 64, dtype=dtype, device=dev)
    buf[n:] = CANARY
    return buf, buf[:n].view(shape)


def _check(got, w, dev):
    """``reweight_sources`` of ``got``'s list under ``w`` against the checker and the host twin: ``(tables, sums)``."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import hits_reweight_sources_host
    c, K = got.c, w.shape[0]
    sums = torch.zeros((K, 2, got.nl), dtype=torch.int64, device=dev)
    tables = got.hl.reweight_sources(got.scene, got.plan, w, sums=sums)
    torch.cuda.synchronize()
    assert tables.dtype == torch.float64 and tuple(tables.shape) == (K, got.nl * c.ny * c.nx, got.plan.W)
    t, s = tables.cpu().numpy(), sums.cpu().numpy()
    want_t, want_s = S.reweighted(got.rec, w, c.nx, c.ny, got.nl, got.ranges)
    assert t.tobytes() == want_t.tobytes() and s.tobytes() == want_s.tobytes()
    twin_t, twin_s = hits_reweight_sources_host(got.hl.raw(), w, c.nx, c.ny, got.nl, got.ranges)
    assert t.tobytes() == twin_t.tobytes() and s.tobytes() == twin_s.tobytes()
    return t, s


def test_small_three_sources(dev):
    """Ones, TE only and weights on the 2^-8 grid: the checker's and the twin's bytes; row 0 is the launches' table."""
    from tests.test_hits import checked
    got = traced("small", dev)
    assert got.rec.tobytes() == checked("small", 2)["rec"].tobytes() and len(got.rec) == S.SMALL_COUNTS["records"]
    t, s = _check(got, S.three_sources(got.c.R), dev)
    assert t[0].tobytes() == got.table.tobytes() and got.table.sum() > 0
    assert t[1].sum() > 0 and t[2].sum() > 0 and t[1].tobytes() != t[0].tobytes()
    np.testing.assert_array_equal(s[0, 0], s[0, 1])
    assert int(s[0, 0].sum()) >> 32 == int(got.table[:, 0].sum())


@pytest.mark.parametrize("K", [1, 64, 70])
def test_chunk_boundaries(dev, K):
    """K below a chunk of 64 sources, exactly one, and a second chunk of 6 live lanes; weights with zeros; nothing
    written beyond either output; a second call doubles both."""
    got = traced("small", dev)
    c = got.c
    w = S.grid_weights(70, c.R, seed=70, zeros=0.2)[:K]
    assert (w == 0).any() or K == 1
    want_t, want_s = S.reweighted(got.rec, w, c.nx, c.ny, got.nl, got.ranges)
    obuf, out = _with_canary((K, got.nl * c.ny * c.nx, got.plan.W), torch.float64, dev)
    sbuf, sums = _with_canary((K, 2, got.nl), torch.int64, dev)
    for times in (1, 2):
        t = got.hl.reweight_sources(got.scene, got.plan, torch.from_numpy(w).to(dev), out=out, sums=sums)
        assert t is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == (times * want_t).tobytes(), (K, times)
        assert sums.cpu().numpy().tobytes() == (times * want_s).tobytes(), (K, times)
        assert (obuf[out.numel():] == CANARY).all() and (sbuf[sums.numel():] == CANARY).all()
    assert want_t[K - 1].sum() > 0


def test_single_wavelength(dev):
    """7,744 rays through ``trace_single``: more than one workgroup of records, one wavelength."""
    got = traced("c2s", dev)
    c = got.c
    rec = got.rec
    inside = (rec["flags"] & 1) == 1
    r = rec["gid"] % c.R
    assert dict(inside=int(inside.sum()), te=int((inside & (r < c.R // 2)).sum()),
                tm=int((inside & (r >= c.R // 2)).sum())) == S.C2S_COUNTS
    assert len(rec) > 256 and rec["tile"].max() < c.nx * c.ny and got.nl == 1
    w = np.concatenate([S.three_sources(c.R), S.grid_weights(2, c.R, seed=9, zeros=0.3)])
    t, _ = _check(got, w, dev)
    assert t[0].tobytes() == got.table.tobytes() and got.table.sum() > 0


@pytest.mark.parametrize("name", ["small", "c2s"])
def test_source_counts(dev, name):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import hits_source_counts_host
    got = traced(name, dev)
    c = got.c
    want = S.class_counts(got.rec, c.nx, c.ny, got.nl, c.R)
    cbuf, out = _with_canary((got.nl, 2, c.R), torch.int64, dev)
    for times in (1, 2):
        t = got.hl.source_counts(got.scene, c.R, out=out)
        assert t is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == (times * want).tobytes()
        assert (cbuf[out.numel():] == CANARY).all()
    fresh = got.hl.source_counts(got.scene, c.R)
    assert fresh.dtype == torch.int64 and fresh.cpu().numpy().tobytes() == want.tobytes()
    assert want.tobytes() == hits_source_counts_host(got.hl.raw(), c.nx, c.ny, got.nl, c.R).tobytes()
    assert int(want.sum()) == len(got.rec) and int(want[:, 0].sum()) == int(((got.rec["flags"] & 1) == 1).sum())
    # another R is another partition of the same records
    other = got.hl.source_counts(got.scene, 7).cpu().numpy()
    assert other.tobytes() == S.class_counts(got.rec, c.nx, c.ny, got.nl, 7).tobytes()


def test_empty_and_short_lists(dev):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import HitList, HitListOverflow
    got = traced("small", dev)
    c, scene, plan = got.c, got.scene, got.plan
    w = S.three_sources(c.R)
    # n == 0: no launch, nothing touched
    empty = HitList(16, dev)
    sums = torch.zeros((3, 2, 3), dtype=torch.int64, device=dev)
    t = empty.reweight_sources(scene, plan, w, sums=sums)
    cnt = empty.source_counts(scene, c.R)
    torch.cuda.synchronize()
    assert not t.any() and not sums.any() and not cnt.any()
    L = _lib.load()
    assert L.wgrt_hits_reweight_sources(scene.handle, plan.handle, None, 0, torch.from_numpy(w).to(dev).data_ptr(), c.R, 3,
                                        None, None, None) == 0
    assert L.wgrt_hits_source_counts(scene.handle, None, 0, c.R, None, None) == 0
    # a list that counted more than it stores
    short = HitList(len(got.rec), dev)
    short.buffer.copy_(got.hl.buffer[:len(got.rec)])
    short.counter.fill_(len(got.rec))
    assert short.reweight_sources(scene, plan, w[:1]).cpu().numpy()[0].tobytes() == got.table.tobytes()
    short.counter.fill_(len(got.rec) + 1)
    with pytest.raises(HitListOverflow, match=str(len(got.rec) + 1)):
        short.reweight_sources(scene, plan, w)
    with pytest.raises(HitListOverflow, match=str(len(got.rec) + 1)):
        short.source_counts(scene, c.R)


def test_refusals(dev):
    got = traced("small", dev)
    c, scene, plan, hl = got.c, got.scene, got.plan, got.hl
    w = S.three_sources(c.R)
    n_slabs = 3 * c.nx * c.ny
    for bad in (np.ones(c.R), np.ones((0, c.R)), -w, w * 1000, np.where(w == 1, np.nan, w), np.where(w == 1, np.inf, w)):
        with pytest.raises(ValueError, match="weights"):
            hl.reweight_sources(scene, plan, bad)
    with pytest.raises(ValueError, match="out"):
        hl.reweight_sources(scene, plan, w, out=torch.zeros((2, n_slabs, plan.W), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="sums"):
        hl.reweight_sources(scene, plan, w, sums=torch.zeros((3, 2, 2), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="out"):
        hl.source_counts(scene, c.R, out=torch.zeros((3, 2, c.R + 1), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="R"):
        hl.source_counts(scene, 0)
    L = _lib.load()
    wd = torch.from_numpy(w).to(dev)
    out = torch.zeros((3, n_slabs, plan.W), dtype=torch.float64, device=dev)
    sums = torch.zeros((3, 2, 3), dtype=torch.int64, device=dev)
    cnt = torch.zeros((3, 2, c.R), dtype=torch.int64, device=dev)
    n = len(got.rec)

    def rw(s=scene.handle, p=plan.handle, hits=hl.buffer.data_ptr(), n_=n, wp=wd.data_ptr(), R=c.R, K=3, o=out.data_ptr(),
           ws=sums.data_ptr()):
        return L.wgrt_hits_reweight_sources(s, p, hits, n_, wp, R, K, o, ws, None)
    for bad in (dict(s=None), dict(p=None), dict(hits=None), dict(hits=hl.buffer.data_ptr() + 8), dict(n_=-1), dict(wp=None),
                dict(wp=wd.data_ptr() + 4), dict(R=0), dict(K=0), dict(o=None), dict(o=out.data_ptr() + 4),
                dict(ws=sums.data_ptr() + 4), dict(K=65536 * 64)):
        assert rw(**bad) == 1, bad                                   # WGRT_ERR_INVALID_ARGUMENT

    def sc(s=scene.handle, hits=hl.buffer.data_ptr(), n_=n, R=c.R, cp=cnt.data_ptr()):
        return L.wgrt_hits_source_counts(s, hits, n_, R, cp, None)
    for bad in (dict(s=None), dict(hits=None), dict(hits=hl.buffer.data_ptr() + 8), dict(n_=-1), dict(R=0), dict(cp=None),
                dict(cp=cnt.data_ptr() + 4)):
        assert sc(**bad) == 1, bad
    torch.cuda.synchronize()
    assert not out.any() and not sums.any() and not cnt.any()
    assert rw(ws=None) == 0                                          # the sums are optional
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == got.table.tobytes() and not sums.any()


def test_visits_reweight_many_after_the_fold_kernels_move(dev):
    """``wgrt_visits_reweight_many`` folds its chunk scratch with the kernel of wgrt_many_fold.h, as the sources do: one
    call on ``small`` (crafted rows, two chunks) gives the bytes of ``wgrt_visits_reweight_many_host``."""
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.AR_system_evaluation_functions import pupil_mask
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import VisitTable, visits_reweight_many_host
    from tests import _reweight_many as M
    got = traced("small", dev)
    c = got.c
    counts, ends, deposits = M.crafted_rows(c, 257, seed=257)
    vt = VisitTable(got.scene, len(ends), dev)
    vt.counts.copy_(torch.from_numpy(counts.view(np.int32)))
    vt.ends.copy_(torch.from_numpy(ends.view(np.uint8).reshape(len(ends), 32)))
    ln = M.designs(70, vt.n_channels)
    tables, sums = vt.reweight_many(got.plan, np.exp(ln))
    torch.cuda.synchronize()
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import _lnscale_many
    lnk = _lnscale_many(vt.channels, np.exp(ln)).numpy()                        # (the log-scales the device was given)
    twin, tsums = visits_reweight_many_host(counts, ends, lnk, c.nx, c.ny, 3, got.ranges, pupil_mask())
    t = tables.cpu().numpy()
    assert float(t[0][:, 0].sum()) == deposits.sum() > 0
    print(f"{int((t != twin).sum())} of {int((twin != 0).sum())} entries differ from the host twin")
    assert t.tobytes() == twin.tobytes()
    assert sums.cpu().numpy().tobytes() == tsums.tobytes()


# the driver ----------------------------------------------------------------------------------------------------------

NX, NY, R, STEPS = 5, 4, 100, 2
_runs = {}


def _points():
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.couplers_coor import design_geometry
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import generate_points_in_polygon
    return generate_points_in_polygon(design_geometry(NX, NY).IC, R // 2, rng=np.random.default_rng(1))


def _diameter(pts):
    return 2 * float(np.median(np.sqrt(((pts - pts.mean(axis=0)) ** 2).sum(axis=1))))


def _run(key, **kw):
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
    if key not in _runs:
        _runs[key] = run(NX, NY, R, STEPS, points=_points(), verbose=False, eyebox="windows", **kw)
    return _runs[key]


def _sources():
    return [{}, {"te": 1, "tm": 0}, {"te": 0, "tm": 1}, {"diameter": _diameter(_points())}]


def _same(a, b, k):
    if isinstance(a, np.ndarray):
        assert a.tobytes() == b.tobytes(), k
    elif isinstance(a, dict):
        assert set(a) == set(b), k
        for j in a:
            _same(a[j], b[j], (k, j))
    else:
        assert a == b or (isinstance(a, float) and float(a).hex() == float(b).hex()), k


def test_driver_sources(dev):
    plain = _run("plain")
    got = _run("sources", sources=_sources(), source_counts=True, source_map=(6, 8))
    assert set(got) - set(plain) == {"sources", "hits", "hit_count", "source_counts", "source_map"}
    for k in plain:   # the figures of the run without sources, unchanged (the timings aside)
        if k not in ("gpu_seconds", "post_seconds"):
            _same(got[k], plain[k], k)
    s = got["sources"]
    n_slabs = 3 * NX * NY
    assert s["weights"].shape == (4, R) and s["table"].shape == (4, n_slabs, 57) and s["sums"].shape == (4, 2, 3)
    # source 0 is the job's own: its table gives the job's A and efficiencies, its figures are the job's
    A0 = s["table"][0][:, 0].reshape(3, NY, NX).astype(np.float32) / (NX * NY * 3 * R) / STEPS
    assert A0.tobytes() == plain["A"].tobytes() == s["A"][0].tobytes() and plain["A"].sum() > 0
    for l, n in enumerate(("Blue", "Green", "Red")):
        assert float(s["efficiency"][0, l]).hex() == float(plain["efficiency"][n]).hex()
    assert [float(s[n][0]).hex() for n in ("delta_e", "U_fov", "U_EB")] == \
        [float(plain[n]).hex() for n in ("delta_e", "U_fov", "U_EB")]
    # ... and the table of the records the run kept, by the checker
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.couplers_coor import design_geometry
    ranges = np.ascontiguousarray(design_geometry(NX, NY).eff_reg_FOV_range, dtype=np.float64)
    want_t, want_s = S.reweighted(got["hits"], s["weights"], NX, NY, 3, ranges)
    assert s["table"].tobytes() == want_t.tobytes() and s["sums"].tobytes() == want_s.tobytes()
    # the two halves add up to twice the nominal source
    assert (s["table"][1] + s["table"][2]).tobytes() == (2 * s["table"][0]).tobytes()
    assert s["table"][1].sum() > 0 and s["table"][2].sum() > 0
    # a stop keeps a part of the rays: a smaller effective sample
    assert (s["ess"][3] < s["ess"][0]).all() and (s["ess"][3] > 0).all()
    np.testing.assert_array_equal(s["ess"][0], s["table"][0][:, 0].reshape(3, -1).sum(axis=1))
    # the counts and the map
    assert got["source_counts"].tobytes() == S.class_counts(got["hits"], NX, NY, 3, R).tobytes()
    m = got["source_map"]
    assert m["delivered"].shape == (3, 2, 6, 8) and int(m["launched"].sum()) == R // 2
    np.testing.assert_array_equal(m["delivered"].sum(axis=(1, 2, 3)), got["source_counts"][:, 0].sum(axis=1))
    # an array of weights is taken as it is given (scaled to mean 1)
    arr = _run("array", sources=s["weights"][[1, 0]] * 3.0)["sources"]
    assert arr["table"].tobytes() == s["table"][[1, 0]].tobytes()


def _driver_worker(rank, world, outdir):
    torch.cuda.set_device(torch.device("cuda", 0))
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.gpu_ray_tracing_pro_fullColor import run
    res = run(NX, NY, R, STEPS, points=_points(), verbose=False, eyebox="windows", sources=_sources(), source_counts=True)
    if rank != 0:
        assert "sources" not in res and "source_counts" not in res
        return
    np.save(f"{outdir}/tables.npy", res["sources"]["table"])
    np.save(f"{outdir}/sums.npy", res["sources"]["sums"])
    np.save(f"{outdir}/counts.npy", res["source_counts"])


def test_driver_in_two_ranks(dev, tmp_path):
    """Two ranks on the one GPU over gloo: each re-weights its own list; grid-valued doubles and integers add exactly."""
    from tests import _dist
    _dist.spawn(_driver_worker, 2, str(tmp_path))
    one = _run("sources", sources=_sources(), source_counts=True, source_map=(6, 8))
    assert np.load(tmp_path / "tables.npy").tobytes() == one["sources"]["table"].tobytes()
    assert np.load(tmp_path / "sums.npy").tobytes() == one["sources"]["sums"].tobytes()
    assert np.load(tmp_path / "counts.npy").tobytes() == one["source_counts"].tobytes()
