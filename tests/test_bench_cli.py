"""bench.py's command line: a plain run measures the headline alone, ``--full`` everything else,
``--dump-outputs DIR`` writes what the timed steps left within DUMP_BYTES, the same from run to run."""
import json
import os

import numpy as np
import pytest

import bench


def test_full_and_dump_are_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_budget_and_sample(tmp_path, monkeypatch):
    """Arrays within their share are written whole; a larger one as a sorted seeded sample of its
    elements; the files together stay within DUMP_BYTES; a second dump gives the same bytes."""
    # 1 KiB per header + 8000 B: small (56 B) and mid (2400 B) fit their even shares of what is left,
    # big (8000 B) gets the remaining 5544 B = 1386 of its 2000 elements
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 1024 + 8000)
    rng = np.random.default_rng(5)
    arrays = {"big": rng.random((50, 40)).astype(np.float32), "small": np.arange(7, dtype=np.float64),
              "mid": rng.random(300)}
    n = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "mid.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    np.testing.assert_array_equal(got["small"], arrays["small"])
    np.testing.assert_array_equal(got["mid"], arrays["mid"])
    assert n["small"] == 7 and got["small"].dtype == np.float64
    assert got["big"].dtype == np.float32 and got["big"].ndim == 1 and n["big"] == got["big"].size == 1386
    assert set(got["big"].tolist()) <= set(arrays["big"].reshape(-1).tolist())
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_repeat(tmp_path, capsys):
    """A plain run of the smallest workload: the line holds the headline figures of exactly
    --steps timed steps and none of --full's records, and two runs dump identical outputs, equal
    to steps + warmup chained traces of the same batch."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    lines = []
    for d in ("a", "b"):
        bench.main(["--gpus", "1", "--config", "C2", "--steps", "3", "--warmup", "2", "--dump-outputs",
                    str(tmp_path / d)])
        lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "ray-bounces/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"roofline", "main_job", "fused", "region", "long_region", "emulated_strong", "cpu_baseline"} & set(line)
    out = {n: [np.load(tmp_path / d / (n + ".npy")) for d in ("a", "b")] for n in ("matrix_EB", "rng_states", "stats")}
    for n, (x, y) in out.items():
        assert x.dtype == (np.float32 if n == "matrix_EB" else np.float64), n
        assert x.tobytes() == y.tobytes(), n
    # the same 5 chained traces through the engine
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.configs import CONFIGS, build_inputs
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.distributed import (hip_shard_builder, hip_tracer,
                                                                                make_shard, run_steps)
    from gpu_ray_tracing_for_waveguide_based_ar_display_amd.engine import Scene, new_stats
    w = CONFIGS["C2"]
    dev = torch.device("cuda", 0)
    geom, luts, points = build_inputs(w, lut_seed=0)
    scene = Scene.from_geometry(geom, luts, device=0)
    shard = make_shard(w.nx, w.ny, len(w.lambdas), w.R, 1, 0, "interleaved")
    rays, rng = hip_shard_builder(points, w.nx, w.ny, list(w.lambdas), w.R, dev)(shard)
    eb = torch.zeros(scene.eb_shape(), dtype=torch.float32, device=dev)
    stats = new_stats(dev)
    tracer = hip_tracer(scene, 0, stats)
    run_steps(tracer, rays, rng, eb, shard.gid, 2, 1)
    stats.zero_()
    run_steps(tracer, rays, rng, eb, shard.gid, 3, 1)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out["matrix_EB"][0], eb.cpu().numpy())
    np.testing.assert_array_equal(out["rng_states"][0], rng.cpu().numpy().view(np.uint32).astype(np.float64))
    np.testing.assert_array_equal(out["stats"][0], stats.cpu().numpy().astype(np.float64))
    # value = the timed steps' bounces over their time; ms_per_step is printed to 4 decimals
    assert line["value"] == pytest.approx(out["stats"][0][0] / (line["ms_per_step"] * 3e-3),
                                          rel=1e-4 / line["ms_per_step"] + 1e-6)
    scene.close()
