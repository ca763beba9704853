"""The automatic issue order's arithmetic (csrc/wgrt_order.h) through its host entry point
wgrt_debug_order_host, which runs the device kernel's code on the CPU: count -> class, then the stable
two-pass sort.  Reference: numpy's stable argsort of the same class keys.  No GPU."""
import numpy as np
import pytest

from gpu_ray_tracing_for_waveguide_based_ar_display_amd._lib import load

CLASSES = 256   # csrc/wgrt_order.h kOrderClasses


def _order(tail, tiles):
    tail = np.ascontiguousarray(tail, np.uint32)
    tiles = np.ascontiguousarray(tiles, np.int32)
    out = np.full(tiles.size, -1, np.int32)
    st = load().wgrt_debug_order_host(tail.ctypes.data, tail.size, tiles.ctypes.data, tiles.size, out.ctypes.data)
    assert st == 0
    return out


def _keys(tail, tiles):
    tail = np.asarray(tail, np.int64)
    tiles = np.asarray(tiles, np.int64)
    mx = int(tail.max()) if tail.size else 0
    ok = (tiles >= 0) & (tiles < tail.size)
    cnt = np.where(ok, tail[np.clip(tiles, 0, max(tail.size - 1, 0))] if tail.size else 0, 0)
    if mx == 0:
        return np.full(tiles.shape, CLASSES - 1, np.int64)
    return CLASSES - 1 - np.minimum(cnt * (CLASSES - 1) // mx, CLASSES - 1)


def _check(tail, tiles):
    got = _order(tail, tiles)
    np.testing.assert_array_equal(np.sort(got), np.arange(len(tiles)))
    np.testing.assert_array_equal(got, np.argsort(_keys(tail, tiles), kind="stable"))
    return got


TILE_MAJOR = np.repeat(np.arange(1323), 16)   # the C3 layout: 16 chunks per tile


@pytest.mark.parametrize("tail", [np.full(1323, 7), np.zeros(1323)], ids=["all_equal", "all_zero"])
def test_flat_table_keeps_the_natural_order(tail):
    np.testing.assert_array_equal(_check(tail, TILE_MAJOR), np.arange(TILE_MAJOR.size))


def test_one_hot_tile_goes_first_and_stays_together():
    tail = np.zeros(1323)
    tail[700] = 40
    got = _check(tail, TILE_MAJOR)
    np.testing.assert_array_equal(got[:16], np.arange(700 * 16, 701 * 16))
    np.testing.assert_array_equal(got[16:], np.delete(np.arange(TILE_MAJOR.size), np.arange(700 * 16, 701 * 16)))


def test_more_tiles_than_classes():
    rng = np.random.default_rng(3)
    tail = rng.integers(0, 5000, 1323)            # counts beyond the 256 classes: several tiles share one
    got = _check(tail, TILE_MAJOR)
    # a tile's 16 chunks stay adjacent and in order
    np.testing.assert_array_equal(got.reshape(-1, 16) - got.reshape(-1, 16)[:, :1], np.tile(np.arange(16), (1323, 1)))


@pytest.mark.parametrize("n", [0, 1, 5, 255, 256, 257, 4097])
def test_sizes_around_the_worker_count(n):
    rng = np.random.default_rng(n)
    tail = rng.integers(0, 300, 50)
    _check(tail, rng.integers(0, 50, n))


def test_chunks_of_no_tile_go_last():
    tail = np.array([3, 0, 9, 1])
    tiles = np.array([0, -1, 2, 7, 3, 1, 2])      # -1 and 7: no such tile
    got = _check(tail, tiles)
    assert list(got) == [2, 6, 0, 4, 1, 3, 5]


def test_empty_table():
    np.testing.assert_array_equal(_check(np.zeros(0), np.array([0, 1, -1])), np.arange(3))
