"""Indexed cached forms without a GPU: the argument checks of ccvpe_*_cached_indexed (all made before the handle is used), the
tile_index keyword of the model methods, and aerial.oxford_tiles against oxford_window."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models

EINVAL = -1


def _indexed_calls(lib):
    """(name, call(h, grd, cache, n_tiles, tile_index, batch, result, k, radius)) of the three entry points"""
    return [
        ("forward", lambda h, g, c, n, t, b, r, k, rad: lib.ccvpe_forward_cached_indexed(h, g, 154, 231, c, n, t, b, r, None)),
        ("localize", lambda h, g, c, n, t, b, r, k, rad: lib.ccvpe_localize_cached_indexed(h, g, 154, 231, c, n, t, b, r, None)),
        ("topk", lambda h, g, c, n, t, b, r, k, rad: lib.ccvpe_localize_topk_cached_indexed(h, g, 154, 231, c, n, t, b, k, rad, r, None)),
    ]


def test_indexed_entry_points_check_their_arguments(built_library):
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    out = C.cast(C.pointer(_lib.Outputs()), C.c_void_p)
    good = (C.c_int32 * 5)(2, 0, 2, 1, 0)
    for name, fn in _indexed_calls(lib):
        res = C.cast(out, C.POINTER(_lib.Outputs)) if name == "forward" else p

        def call(h=p, g=p, c=p, n=3, t=good, b=5, r=res, k=8, rad=16):
            rc = fn(h, g, c, n, t, b, r, k, rad)
            return rc, (lib.ccvpe_last_error() or b"").decode()

        # a bogus handle is never read: every refusal below happens before the handle is used
        rc, msg = call(g=None)
        assert rc == EINVAL and "grd" in msg, (name, msg)
        rc, msg = call(c=None)
        assert rc == EINVAL and "cache" in msg, (name, msg)
        rc, msg = call(t=None)
        assert rc == EINVAL and "tile_index" in msg, (name, msg)
        rc, msg = call(r=None)
        assert rc == EINVAL and "output" in msg, (name, msg)
        for n in (0, -1):
            rc, msg = call(n=n)
            assert rc == EINVAL and "n_tiles" in msg, (name, n, msg)
        rc, msg = call(b=0)
        assert rc == EINVAL and "batch" in msg, (name, msg)
        neg = (C.c_int32 * 5)(2, 0, -1, 1, 0)
        rc, msg = call(t=neg)
        assert rc == EINVAL and "tile_index[2] = -1" in msg, (name, msg)
        at_n = (C.c_int32 * 5)(2, 0, 2, 3, 3)
        rc, msg = call(t=at_n)
        assert rc == EINVAL and "tile_index[3] = 3" in msg and "n_tiles 3" in msg, (name, msg)
        rc, msg = call(n=2)   # the same indices against a smaller cache: position 0 holds 2
        assert rc == EINVAL and "tile_index[0] = 2" in msg, (name, msg)
        if name == "topk":
            for k, rad in ((0, 16), (65, 16), (8, -1), (8, 33)):
                rc, msg = call(k=k, rad=rad)
                assert rc == EINVAL and ("k must" if not 1 <= k <= 64 else "radius") in msg, (k, rad, msg)
        # valid arguments all the way: the null handle is the first thing refused
        rc, msg = call(h=None)
        assert rc == EINVAL and "null" in msg, (name, msg)


# ---- model methods ----------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def _methods(m):
    return [lambda g, c, t: m.forward_cached(g, c, tile_index=t),
            lambda g, c, t: m.localize_cached(g, c, tile_index=t),
            lambda g, c, t: m.localize_topk_cached(g, c, 8, 16, tile_index=t)]


def test_model_methods_refuse_a_device_tile_index():
    m = _model()
    g = torch.zeros(5, 3, 154, 231)
    dev = torch.zeros(5, dtype=torch.int32, device="meta")   # any non-CPU tensor; tests/test_indexed_cache_gpu.py passes a cuda one
    for f in _methods(m):
        with pytest.raises(ValueError, match="host data"):
            f(g, torch.zeros(16), dev)


def test_model_methods_refuse_a_tile_index_of_the_wrong_length_or_type():
    m = _model()
    g = torch.zeros(5, 3, 154, 231)
    for f in _methods(m):
        for bad in ([0, 1, 0, 1], np.zeros(6, np.int64), torch.zeros(2, 5, dtype=torch.int32), 3):
            with pytest.raises(ValueError, match="one tile per query"):
                f(g, torch.zeros(16), bad)
        with pytest.raises(ValueError, match="integers"):
            f(g, torch.zeros(16), np.zeros(5, np.float32))
        with pytest.raises(ValueError, match="int32"):
            f(g, torch.zeros(16), np.array([0, 1, 2 ** 32, 0, 1], np.int64))
        # a well-formed host index gets past the keyword's checks: the CPU ground tensor is what is refused next
        for ok in ([2, 0, 2, 1, 0], np.array([2, 0, 2, 1, 0], np.int64), torch.tensor([2, 0, 2, 1, 0])):
            with pytest.raises(ValueError, match="cuda"):
                f(g, torch.zeros(16), ok)


def test_model_methods_keep_eval_check_first():
    m = _model().train()
    g = torch.zeros(5, 3, 154, 231)
    for f in _methods(m):
        with pytest.raises(RuntimeError, match="eval"):
            f(g, torch.zeros(16), [0, 0, 0, 0, 0])


# ---- aerial.oxford_tiles ----------------------------------------------------------------------------------------------

def _check_tiles(coords):
    win = aerial.oxford_window(coords)["origin"]
    t = aerial.oxford_tiles(coords)
    origin, index = t["origin"], t["tile_index"]
    assert origin.dtype == np.int32 and index.dtype == np.int32
    assert origin.ndim == 2 and origin.shape[1] == 2 and index.shape == (win.shape[0],)
    np.testing.assert_array_equal(origin[index], win)
    assert len({tuple(o) for o in origin}) == origin.shape[0], "origins are distinct"
    # first-appearance order: tile j first shows up before tile j + 1, and a query opens a new tile exactly when its window is new
    first = [int(np.argmax(index == j)) for j in range(origin.shape[0])]
    assert first == sorted(first) and first[0] == 0
    seen = set()
    for b, o in enumerate(map(tuple, win)):
        assert (o in seen) == (b not in first)
        seen.add(o)
    return t


def test_oxford_tiles_agree_with_oxford_window_on_random_drives():
    rng = np.random.default_rng(11)
    for _ in range(20):
        B = int(rng.integers(1, 40))
        start = rng.uniform(400, 9000, size=2)
        steps = rng.normal(0, 30, size=(B, 2))
        _check_tiles(start + np.cumsum(steps, axis=0))
    for _ in range(5):   # scattered queries: mostly one tile each
        _check_tiles(rng.uniform(0, 12000, size=(16, 2)))


def test_oxford_tiles_at_grid_boundaries_and_revisits():
    # coordinates on and around the 400-px grid and the 200-px switch inside a cell (oxford_window rounds there)
    edges = []
    for base in (400.0, 800.0, 1200.0):
        for d in (-200.5, -200.0, -199.5, -0.5, 0.0, 0.5, 199.4, 199.5, 200.0):
            edges.append((base + d, base + 1.5 * d))
    t = _check_tiles(np.array(edges))
    assert t["origin"].shape[0] > 1
    # a drive that leaves a tile and comes back: the revisit maps to the first tile, not a new one
    there = [(1000.0 + 10 * i, 1000.0) for i in range(8)]
    away = [(2300.0 + 10 * i, 1000.0) for i in range(4)]
    t = _check_tiles(np.array(there + away + there[::-1]))
    assert t["origin"].shape[0] == 2
    np.testing.assert_array_equal(t["tile_index"], [0] * 8 + [1] * 4 + [0] * 8)
    one = aerial.oxford_tiles(np.array([[1000.0, 1000.0]]))
    np.testing.assert_array_equal(one["tile_index"], [0])
    assert one["origin"].shape == (1, 2)
