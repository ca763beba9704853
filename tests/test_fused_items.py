"""The work items of a fused launch (csrc/wgrt_items.h), through the host build of the code the kernels decode every
dequeue with (``wgrt_debug_fused_items_host``; no GPU): head x's queue position q -> (chunk, run of traces).

A fused launch of ``num_iter`` chained traces hands out, per head, its stripes' chunks once per run of ``S``
consecutive traces, run-major.  The properties the wave loop and the hand-off's forward-progress argument rest on:

* the eight heads' items cover every (trace, chunk) exactly once;
* a run never crosses ``num_iter`` and starts at a multiple of ``S``;
* on every head, all items of run r precede those of run r + 1;
* ``S = 1`` is the mapping of one item per (trace, chunk): stripe s of 16 chunks on head s % 8, trace-major.

The automatic run length and the switch's argument check are host functions too, and are pinned here."""
import numpy as np
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _lib

HEADS, STRIPE = 8, 16
N_CHUNKS = [1, 15, 16, 17, 129, 21168]
NUM_ITER = [1, 2, 5, 8, 9, 39, 64]
RUNS = [1, 2, 4, 8, 64]


def _items(n_chunks, num_iter, run):
    return [_lib.fused_items_host(n_chunks, num_iter, run, x) for x in range(HEADS)]


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("num_iter", NUM_ITER)
@pytest.mark.parametrize("n_chunks", N_CHUNKS)
def test_items_cover_every_trace_of_every_chunk_once(n_chunks, num_iter, run):
    edge = np.zeros((num_iter + 1) * n_chunks, np.int32)   # +1 where an item's run begins, -1 where it ends
    for chunk, k0, k1 in _items(n_chunks, num_iter, run):
        assert ((chunk >= 0) & (chunk < n_chunks)).all()
        # a run starts at a multiple of S and ends at the next one, or at num_iter
        assert (k0 % run == 0).all() and (k0 < num_iter).all()
        np.testing.assert_array_equal(k1, np.minimum(k0 + run, num_iter))
        # all items of run r precede those of run r + 1 on the head
        assert (np.diff(k0) >= 0).all()
        edge += np.bincount(k0.astype(np.int64) * n_chunks + chunk, minlength=edge.size).astype(np.int32)
        edge -= np.bincount(k1.astype(np.int64) * n_chunks + chunk, minlength=edge.size).astype(np.int32)
    seen = np.cumsum(edge.reshape(num_iter + 1, n_chunks), axis=0)[:num_iter]
    assert (seen == 1).all()


@pytest.mark.parametrize("num_iter", NUM_ITER)
@pytest.mark.parametrize("n_chunks", N_CHUNKS)
def test_run_of_one_is_an_item_per_trace(n_chunks, num_iter):
    """S = 1: head x's chunks are its stripes x, x + 8, ... in ascending order, repeated once per trace."""
    for x, (chunk, k0, k1) in enumerate(_items(n_chunks, num_iter, 1)):
        every = np.arange(n_chunks, dtype=np.int64)
        mine = every[(every // STRIPE) % HEADS == x]
        np.testing.assert_array_equal(chunk, np.tile(mine, num_iter))
        np.testing.assert_array_equal(k0, np.repeat(np.arange(num_iter, dtype=np.int32), mine.size))
        np.testing.assert_array_equal(k1, k0 + 1)


@pytest.mark.parametrize("run", [2, 8])
def test_a_run_repeats_the_heads_chunk_list(run):
    """Whatever the run length, a head hands its chunks out in the order a single trace does."""
    for (chunk, k0, _k1), (one, _a, _b) in zip(_items(129, 9, run), _items(129, 1, 1)):
        for r0 in np.unique(k0):
            np.testing.assert_array_equal(chunk[k0 == r0], one)


def test_automatic_run_length():
    """At least four runs per launch, runs of at most 16; a debug hand-off bound asks for hand-offs; the switch wins."""
    try:
        _lib.set_fused_run(0)
        for n in range(2, 65):
            s = _lib.fused_run(n)
            assert s in (1, 2, 4, 8, 16) and (s == 1 or n >= 4 * s) and (s == 16 or n < 8 * s)
            assert _lib.fused_run(n, handoff_bound=True) == 1
        assert [_lib.fused_run(n) for n in (2, 4, 7, 8, 20, 39, 64, 200)] == [1, 1, 1, 2, 4, 8, 16, 16]
        _lib.set_fused_run(2)
        assert _lib.fused_run(39) == 2 and _lib.fused_run(6, handoff_bound=True) == 2
    finally:
        _lib.set_fused_run(0)


@pytest.mark.parametrize("bad", [-1, 3, 6, 48, 65, 128])
def test_switch_refuses_other_values(bad):
    with pytest.raises(_lib.WgrtError):
        _lib.set_fused_run(bad)
    assert _lib.fused_run(39) == 8   # unchanged: still automatic
