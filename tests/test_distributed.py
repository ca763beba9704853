"""Multi-process (gloo, world size 2 and 3) sharding of the bounce path on CPU.

Each rank traces its FoV x wavelength blocks (interleaved r, r + N, ... by default, or a
contiguous range) with the CPU oracle (the kernel stand-in for a GPU-less host) through
distributed.trace_job / timed_run, and the eyebox grid is collected on rank 0 -- by the gather of
each rank's own slabs (plus the H6 spill into the next slab) or by the sum-reduce.  The result
must equal a single-process trace bit for bit, and every rank's final RNG states must equal its
blocks of the single-process ones.
"""
import os

import numpy as np
import pytest
import torch

from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import STAT
from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import (EB_SLAB, SPILL, EyeboxGather, GidMap,
                                                                            block_range, make_shard, rank_blocks,
                                                                            replica_shard, shard_rays_host, slab_ids,
                                                                            timed_run, trace_job)
from tests import _dist

NX, NY, LAMBDAS, R, NUM_ITER = 4, 3, [0, 1, 2], 32, 2


def _inputs():
    return _dist.small_job(NX, NY, R, lut_seed=2, point_seed=4)


def _oracle_tracer(geom, luts, stats=None):
    """trace_fn of distributed.run_steps on the CPU oracle (one call per run of consecutive blocks
    of the shard's GidMap); adds its bounces to stats[STAT.bounces] like the HIP tracer's device counter."""
    from oracle import OracleScene
    sc = OracleScene.from_geometry(geom, luts)

    def fn(rays, rng_t, eb_t, gid: GidMap, num_iter=1):
        rng = rng_t.numpy().view(np.uint32)
        eb = eb_t.numpy()
        for _ in range(num_iter):
            for lo, hi, g in gid.runs():
                part = {k: v[lo:hi] for k, v in rays.items()}
                r = np.ascontiguousarray(rng[lo:hi])
                b, _ = sc.trace(part, r, eb, gid_offset=g, threads=1)
                rng[lo:hi] = r
                if stats is not None:
                    stats[STAT.bounces] += b
    return fn


def _host_builder(pts):
    def build(shard):
        rays, rng = shard_rays_host(pts, NX, NY, LAMBDAS, R, shard.blocks)
        return rays, torch.from_numpy(rng.view(np.int32))
    return build


def _collector(world, assign, collect):
    if collect == "reduce":
        return None
    blocks = [rank_blocks(NX * NY * len(LAMBDAS), world, r, assign, len(LAMBDAS)) for r in range(world)]
    return EyeboxGather(blocks, NX, NY, LAMBDAS, 3)


def _worker(rank, world, outdir, assign, collect):
    geom, luts, pts = _inputs()
    shard = make_shard(NX, NY, len(LAMBDAS), R, world, rank, assign)
    eb, rng = trace_job(shard, _host_builder(pts), _oracle_tracer(geom, luts),
                        lambda: torch.zeros((3, NY, NX, 80, 120), dtype=torch.float32), num_iter=NUM_ITER,
                        collect=_collector(world, assign, collect))
    np.save(os.path.join(outdir, f"rng{rank}.npy"), rng.numpy())
    np.save(os.path.join(outdir, f"blocks{rank}.npy"), shard.blocks)
    if rank == 0:
        np.save(os.path.join(outdir, "eb.npy"), eb.numpy())


def _bench_worker(rank, world, outdir, assign, collect):
    """bench.py's multi-GPU timed region (distributed.timed_run), gloo + the oracle tracer."""
    geom, luts, pts = _inputs()
    shard = make_shard(NX, NY, len(LAMBDAS), R, world, rank, assign)
    rays, rng_t = _host_builder(pts)(shard)
    eb = torch.zeros((3, NY, NX, 80, 120), dtype=torch.float32)
    stats = torch.zeros(6, dtype=torch.int64)
    calls = []
    hook = lambda j, what: calls.append((j, what))
    el, tot, loc = timed_run(_oracle_tracer(geom, luts, stats), rays, rng_t, eb, shard.gid, NUM_ITER, 1, stats,
                             hook=hook, collect=_collector(world, assign, collect))
    np.save(os.path.join(outdir, f"rng{rank}.npy"), rng_t.numpy())
    np.save(os.path.join(outdir, f"blocks{rank}.npy"), shard.blocks)
    np.save(os.path.join(outdir, f"res{rank}.npy"), np.array([el, tot, loc, len(calls)], dtype=np.float64))
    if rank == 0:
        np.save(os.path.join(outdir, "eb.npy"), eb.numpy())


def _replica_worker(rank, world, outdir):
    """bench.py --gpus N's ``weak`` record (and --scaling weak): rank r traces the whole batch as replica r
    (global ids r * N + i) through timed_run, and the eyebox grids are sum-reduced to rank 0."""
    geom, luts, pts = _inputs()
    shard = replica_shard(NX, NY, len(LAMBDAS), R, world, rank)
    rays, rng = shard_rays_host(pts, NX, NY, LAMBDAS, R, shard.blocks, gid_base=shard.gid_base)
    rng_t = torch.from_numpy(rng.view(np.int32))
    eb = torch.zeros((3, NY, NX, 80, 120), dtype=torch.float32)
    stats = torch.zeros(6, dtype=torch.int64)
    el, tot, loc = timed_run(_oracle_tracer(geom, luts, stats), rays, rng_t, eb, shard.gid, NUM_ITER, 1, stats)
    np.save(os.path.join(outdir, f"rng{rank}.npy"), rng_t.numpy())
    np.save(os.path.join(outdir, f"res{rank}.npy"), np.array([el, tot, loc], dtype=np.float64))
    if rank == 0:
        np.save(os.path.join(outdir, "eb.npy"), eb.numpy())


def _single_process(num_iter=NUM_ITER):
    geom, luts, pts = _inputs()
    rays, rng = shard_rays_host(pts, NX, NY, LAMBDAS, R, np.arange(NX * NY * len(LAMBDAS)))
    eb = np.zeros((3, NY, NX, 80, 120), np.float32)
    from oracle import OracleScene
    sc = OracleScene.from_geometry(geom, luts)
    tot = sum(sc.trace(rays, rng, eb)[0] for _ in range(num_iter))
    return rng, eb, tot


def _check_rng(tmp_path, world, rng):
    for r in range(world):
        blocks = np.load(tmp_path / f"blocks{r}.npy")
        got = np.load(tmp_path / f"rng{r}.npy").view(np.uint32)
        want = rng.reshape(-1, R)[blocks].reshape(-1)
        np.testing.assert_array_equal(got, want, err_msg=f"rank {r}")


@pytest.mark.parametrize("world,assign,collect", [(2, "interleaved", "gather"), (3, "interleaved", "gather"),
                                                  (2, "contiguous", "reduce")])
def test_bench_timed_region_sharded(tmp_path, world, assign, collect):
    """bench.py --gpus N's default (--scaling strong: the metric's one batch split over the ranks as
    interleaved FoV x wavelength blocks, eyebox slabs gathered to rank 0): shard, chained calls
    bracketed by the event hook, eyebox collective, MAX time / SUM bounces all-reduces -- gives the
    single-process job's bounces, grid and RNG states."""
    _dist.spawn(_bench_worker, world, str(tmp_path), assign, collect)
    rng, eb, tot = _single_process()
    res = [np.load(tmp_path / f"res{r}.npy") for r in range(world)]
    assert all(int(r[1]) == tot for r in res)                 # SUM over ranks, on every rank
    assert sum(int(r[2]) for r in res) == tot and all(r[2] > 0 for r in res)
    assert all(r[0] == res[0][0] for r in res) and res[0][0] > 0   # MAX over ranks
    assert all(int(r[3]) == 2 * NUM_ITER for r in res)        # start + end hook per call
    np.testing.assert_array_equal(np.load(tmp_path / "eb.npy"), eb)
    _check_rng(tmp_path, world, rng)


@pytest.mark.parametrize("world,assign,collect", [(2, "interleaved", "gather"), (3, "interleaved", "gather"),
                                                  (3, "contiguous", "gather"), (2, "interleaved", "reduce")])
def test_sharded_job_equals_single_process(tmp_path, world, assign, collect):
    _dist.spawn(_worker, world, str(tmp_path), assign, collect)
    rng, eb, _ = _single_process()
    np.testing.assert_array_equal(np.load(tmp_path / "eb.npy"), eb)
    assert eb.sum() > 0
    _check_rng(tmp_path, world, rng)


def test_replicas_equal_tiled_single_process(tmp_path):
    """Weak scaling (bench.py's ``weak`` record at N > 1): N replicas of the batch with global ids offset
    per rank give exactly the single-process trace of the batch's columns tiled N times (RNG seeded
    by global index, MAIN:158): every rank's RNG states, the SUM of bounces and the reduced grid."""
    world = 2
    _dist.spawn(_replica_worker, world, str(tmp_path))
    geom, luts, pts = _inputs()
    nb = NX * NY * len(LAMBDAS)
    one, _ = shard_rays_host(pts, NX, NY, LAMBDAS, R, np.arange(nb))
    rays = {k: np.concatenate([v] * world) for k, v in one.items()}
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.rays import rng_seeds
    rng = rng_seeds(world * nb * R, 0)
    eb = np.zeros((3, NY, NX, 80, 120), np.float32)
    from oracle import OracleScene
    sc = OracleScene.from_geometry(geom, luts)
    tot = sum(sc.trace(rays, rng, eb)[0] for _ in range(NUM_ITER))
    res = [np.load(tmp_path / f"res{r}.npy") for r in range(world)]
    assert all(int(r[1]) == tot for r in res) and sum(int(r[2]) for r in res) == tot
    assert res[0][2] != res[1][2]   # the replicas draw their own random streams
    np.testing.assert_array_equal(np.load(tmp_path / "eb.npy"), eb)
    for r in range(world):
        np.testing.assert_array_equal(np.load(tmp_path / f"rng{r}.npy").view(np.uint32),
                                      rng[r * nb * R:(r + 1) * nb * R], err_msg=f"rank {r}")


def test_replica_shard_ids():
    s = replica_shard(21, 21, 3, 1024, 8, 5)
    assert s.n_rays == 1323 * 1024 and s.gid.offset == 5 * 1323 * 1024
    assert np.array_equal(s.blocks, np.arange(1323))
    with pytest.raises(ValueError):
        replica_shard(3, 3, 3, 8, 2, 2)


def test_block_ranges_partition():
    for n in (1, 7, 1323, 5043):
        for w in (1, 2, 3, 8):
            rs = [block_range(n, w, r) for r in range(w)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
            assert max(h - l for l, h in rs) - min(h - l for l, h in rs) <= 1
            for assign in ("interleaved", "contiguous"):
                L = 3 if n % 3 == 0 else 1
                bl = [rank_blocks(n, w, r, assign, L) for r in range(w)]
                assert np.array_equal(np.sort(np.concatenate(bl)), np.arange(n))
                assert max(map(len, bl)) - min(map(len, bl)) <= L
    with pytest.raises(ValueError):
        block_range(10, 2, 2)
    with pytest.raises(ValueError):
        rank_blocks(10, 2, 0, "random")


def test_gid_map_runs():
    g = GidMap(np.array([0, 2, 3, 4, 9], dtype=np.int64) * 16, 16)
    assert g.offset is None
    assert list(g.runs()) == [(0, 16, 0), (16, 64, 32), (64, 80, 144)]
    assert GidMap(np.array([5, 6, 7], dtype=np.int64) * 16, 16).offset == 80
    s = make_shard(21, 21, 3, 1024, 8, 3)
    assert s.n_rays == len(s.blocks) * 1024
    fov, k = np.divmod(s.blocks, 3)
    assert np.all((fov + k) % 8 == 3) and set(k.tolist()) == {0, 1, 2}   # every wavelength on every rank


def test_eyebox_gather_assembles_spill():
    """The H6 aliasing (GRTF:154-165): an out-coupling on the eyebox's top edge lands in the first
    SPILL floats of the NEXT slab, which may belong to another rank (or to no rank).  The gather's
    assembly must give exactly the sum of the ranks' grids."""
    rng = np.random.default_rng(0)
    world, nb = 3, NX * NY * len(LAMBDAS)
    blocks = [rank_blocks(nb, world, r, "interleaved", len(LAMBDAS)) for r in range(world)]
    G = EyeboxGather(blocks, NX, NY, LAMBDAS, 3)
    parts, total = [], np.zeros((3, NY, NX, 80, 120), np.float32)
    for r in range(world):
        eb = np.zeros_like(total)
        flat = eb.reshape(-1, EB_SLAB)
        s = slab_ids(blocks[r], NX, NY, LAMBDAS)
        flat[s] = rng.integers(0, 3, size=(len(s), EB_SLAB))
        nxt = s[s + 1 < flat.shape[0]] + 1
        flat[nxt, :SPILL] += rng.integers(0, 2, size=(len(nxt), SPILL))
        total += eb
        parts.append(G.pack(torch.from_numpy(eb), r))
    out = torch.zeros(total.shape, dtype=torch.float32)
    G.assemble(out, parts)
    np.testing.assert_array_equal(out.numpy(), total)


def test_slab_ids_match_block_layout():
    """Block b = ((m * NY + n) * L + k) (MAIN:82-115) writes EB[lambdas[k], n, m] (GRTF:1168)."""
    lam = [1]
    b = np.arange(NX * NY)
    s = slab_ids(b, NX, NY, lam)
    m, n = np.divmod(b, NY)
    np.testing.assert_array_equal(s, (1 * NY + n) * NX + m)
