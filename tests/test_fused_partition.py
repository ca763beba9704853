"""The run partition of a fused launch (csrc/wgrt_items.h), through the host build of the functions the kernels
compile (``wgrt_debug_fused_partition_host``; no GPU).

A launch of ``n`` chained traces in runs of ``S`` with first tail length ``t0`` cuts [0, n) into consecutive runs:
without a taper (``t0 = 0``) runs of ``S`` from 0, the short one last; with one, the last ``2 t0 - 1`` traces are runs
of ``t0, t0 / 2, ..., 2, 1`` and the traces before them runs of ``S`` aligned backwards from there, the short one
first.  Checked for every ``n`` in 1..255, every ``S`` in 1..64 and every admissible ``t0`` against a partition built
here run by run:

* the runs tile [0, n) without gap or overlap;
* what a lane derives from the trace it is at -- its run's first and end trace -- agrees with the run starts;
* ``t0 = 0`` is what ``wgrt_debug_fused_items_host`` returns for the same arguments;
* the tail is ``t0, ..., 2, 1`` wherever ``n`` is long enough, and the last run is one trace.

And for the work items under a partition, on all eight heads: every (run, chunk) pair appears exactly once, and the
item of run r - 1 of a chunk precedes the item of run r of that chunk on the same head -- the premise of the
hand-off's forward-progress argument (a run's last trace publishes what the next run's first trace waits for)."""
import numpy as np
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib

HEADS = 8
RUNS = [1, 2, 4, 8, 16, 32, 64]
N_CHUNKS = [1, 15, 16, 17, 129, 21168]
PARTITIONS = [(39, 8, 4), (39, 8, 2), (39, 8, 0), (9, 4, 2), (8, 8, 4), (5, 4, 2), (3, 4, 2), (2, 2, 1), (9, 2, 1),
              (200, 16, 8), (255, 64, 32), (1, 4, 2)]


@pytest.fixture(autouse=True)
def _switches():
    """The process-wide run and taper switches at their defaults before and after every test."""
    _lib.set_fused_run(0)
    _lib.set_fused_taper(-1)
    yield
    _lib.set_fused_run(0)
    _lib.set_fused_taper(-1)


def _tapers(run):
    return [0] + [t for t in RUNS if t < run]


def _reference(n, run, t0):
    """The runs [(first, end)] built one by one from the end of the launch, as the partition is described."""
    if t0 == 0:
        return [(a, min(a + run, n)) for a in range(0, n, run)]
    back, e, length = [], n, 1
    while length <= t0 and e > 0:   # the tail: 1, 2, ..., t0 from the end, the first of them clipped at 0
        back.append((max(e - length, 0), e))
        e, length = max(e - length, 0), 2 * length
    while e > 0:                    # the head: runs of S backwards from the tail, the short one first
        back.append((max(e - run, 0), e))
        e = max(e - run, 0)
    return back[::-1]


@pytest.mark.parametrize("run", RUNS)
def test_partition_tiles_the_launch(run):
    for t0 in _tapers(run):
        for n in range(1, 256):
            p = _lib.fused_partition_host(1, n, run, t0, items=False)
            want = _reference(n, run, t0)
            first = np.array([a for a, _ in want], np.int32)
            end = np.array([b for _, b in want], np.int32)
            msg = f"n {n} S {run} t0 {t0}"
            # the reference itself tiles [0, n): consecutive, non-empty runs of at most S traces
            assert first[0] == 0 and end[-1] == n and (first[1:] == end[:-1]).all() and (end > first).all(), msg
            assert (end - first <= run).all(), msg
            np.testing.assert_array_equal(p["run_first"], first, err_msg=msg)
            # per trace: the run that holds it
            r = np.searchsorted(first, np.arange(n), side="right") - 1
            np.testing.assert_array_equal(p["trace_first"], first[r], err_msg=msg)
            np.testing.assert_array_equal(p["trace_end"], end[r], err_msg=msg)
            # the last run is one trace under a taper, and the tail is t0, ..., 2, 1 where the launch is long enough
            if t0:
                assert end[-1] - first[-1] == 1, msg
                if n >= 2 * t0 - 1:
                    k = int(np.log2(t0)) + 1
                    assert list(end[-k:] - first[-k:]) == [t0 >> j for j in range(k)], msg
                    # ... and the head's runs are whole but the first
                    assert (end[1:-k] - first[1:-k] == run).all(), msg


@pytest.mark.parametrize("run", RUNS)
def test_no_taper_is_the_uniform_partition(run):
    """t0 = 0 reproduces the runs and the items ``wgrt_debug_fused_items_host`` returns."""
    for n in list(range(1, 70)) + [127, 128, 200, 255]:
        for x in (0, 3, 7):
            chunk, k0, k1 = _lib.fused_items_host(129, n, run, x)
            p = _lib.fused_partition_host(129, n, run, 0, head=x)
            np.testing.assert_array_equal(p["chunk"], chunk)
            np.testing.assert_array_equal(p["first_trace"], k0)
            np.testing.assert_array_equal(p["end_trace"], k1)
        np.testing.assert_array_equal(p["run_first"], np.arange(0, n, run))
        np.testing.assert_array_equal(p["trace_first"], np.arange(n) // run * run)
        np.testing.assert_array_equal(p["trace_end"], np.minimum(np.arange(n) // run * run + run, n))


@pytest.mark.parametrize("n_chunks", N_CHUNKS)
@pytest.mark.parametrize("part", PARTITIONS)
def test_items_are_run_major_over_the_partition(part, n_chunks):
    n, run, t0 = part
    want = _reference(n, run, t0)
    first = np.array([a for a, _ in want], np.int64)
    end = np.array([b for _, b in want], np.int64)
    pos = np.full((len(want), n_chunks), -1, np.int64)    # where on its head's queue the item (run, chunk) stands
    head = np.full((len(want), n_chunks), -1, np.int64)
    count = 0
    for x in range(HEADS):
        p = _lib.fused_partition_host(n_chunks, n, run, t0, head=x)
        chunk, k0, k1 = p["chunk"], p["first_trace"].astype(np.int64), p["end_trace"].astype(np.int64)
        assert ((chunk >= 0) & (chunk < n_chunks)).all()
        r = np.searchsorted(first, k0)
        assert (r < len(want)).all()
        np.testing.assert_array_equal(first[r], k0)       # an item begins where a run begins ...
        np.testing.assert_array_equal(end[r], k1)         # ... and ends where that run ends
        assert (np.diff(r) >= 0).all()                    # run-major
        assert (pos[r, chunk] == -1).all()                # no pair twice (on another head before)
        pos[r, chunk] = np.arange(chunk.size)
        head[r, chunk] = x
        count += chunk.size
    assert count == len(want) * n_chunks and (pos >= 0).all()   # every pair once
    # the publisher of run r's first trace -- the item of run r - 1 -- was dequeued from the same head before
    assert (head == head[0]).all()
    assert (np.diff(pos, axis=0) > 0).all()


C3_RAYS = 21 * 21 * 3 * 1024   # the headline's batch: 21,168 chunks of 64 rays


def test_the_rule_and_the_switch():
    """A launch whose run length is automatic tapers from half its run where the sweep measured a gain:
    runs of 8 or more, batches of 7,500 to 42,000 chunks.  An explicit run length means uniform runs; a debug hand-off
    bound still gives runs of one; an explicit taper wins, cut to below the run."""
    for n in range(2, 256):
        s = _lib.fused_run(n)
        assert _lib.fused_taper(n, C3_RAYS) == (s // 2 if s >= 8 else 0)
        assert _lib.fused_taper(n, C3_RAYS, handoff_bound=True) == 0
    assert [_lib.fused_taper(n, C3_RAYS) for n in (1, 4, 7, 8, 20, 31, 32, 39, 64, 200)] == [0, 0, 0, 0, 0, 0, 4, 4, 8, 8]
    # the batch: the eighth C3 shard and C2 (2,646 chunks) and C4 (84,672) stay untapered
    assert [_lib.fused_taper(39, 64 * c) for c in (1, 2646, 7499, 7500, 21168, 42000, 42001, 84672)] == \
        [0, 0, 0, 4, 4, 4, 0, 0]
    assert _lib.fused_taper(39, 64 * 7499 + 1) == 4   # (chunks round up)
    _lib.set_fused_run(8)
    assert _lib.fused_taper(39, C3_RAYS) == 0
    _lib.set_fused_taper(2)
    assert _lib.fused_taper(39, C3_RAYS) == 2 and _lib.fused_taper(39, 64) == 2
    _lib.set_fused_run(2)
    assert _lib.fused_taper(39, C3_RAYS) == 1
    _lib.set_fused_run(0)
    assert _lib.fused_taper(39, 6000) == 2 and _lib.fused_taper(8, 6000) == 1 and _lib.fused_taper(4, 6000) == 0
    _lib.set_fused_taper(0)
    assert _lib.fused_taper(39, C3_RAYS) == 0 and _lib.fused_taper(200, C3_RAYS) == 0
    assert [_lib.fused_run(n) for n in (2, 4, 7, 8, 20, 39, 64, 200)] == [1, 1, 1, 2, 4, 8, 16, 16]


@pytest.mark.parametrize("bad", [-2, 3, 6, 48, 64, 128])
def test_switch_refuses_other_values(bad):
    with pytest.raises(_lib.WgrtError):
        _lib.set_fused_taper(bad)
    assert _lib.fused_taper(39, C3_RAYS) == 4   # unchanged: still the rule


@pytest.mark.parametrize("args", [(1, 0, 4, 2), (1, 256, 4, 2), (1, 9, 3, 0), (1, 9, 4, 4), (1, 9, 4, 3), (0, 9, 4, 2)])
def test_hook_refuses_what_is_no_partition(args):
    with pytest.raises(_lib.WgrtError):
        _lib.fused_partition_host(*args, items=False)
