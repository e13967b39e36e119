"""Localize over several tiles per query without a GPU: the numpy restatement of the cross-tile reduction on crafted statistics,
the argument checks of ccvpe_localize_region (all made before the handle is used) and of model.localize_region, and the Oxford
region helpers against oxford_window."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import region_ref

EINVAL = -1


def _rows(probs, first_index=100):
    pr = np.zeros((len(probs), 5), np.float32)
    pr[:, 0] = np.arange(len(probs)) + first_index
    pr[:, 1] = probs
    pr[:, 2], pr[:, 3], pr[:, 4] = 0.6, 0.8, 53.0
    return pr


# ---- region_ref -------------------------------------------------------------------------------------------------------

def test_single_pair_keeps_its_row_exactly():
    stats = np.array([[3.25, 1.0 / 4096.5]], np.float32)
    pr = _rows([0.0123456789])
    r = region_ref.region_reduce([0, 1], stats, pr)
    assert r["tile_prob"][0] == np.float32(1.0)
    assert r["rows"][0, 1] == pr[0, 1]
    np.testing.assert_array_equal(r["rows"][0], pr[0])
    assert r["best_pair"][0] == 0


def test_joint_probability_is_the_softmax_over_the_union_of_tiles():
    rng = np.random.default_rng(0)
    logits = [rng.normal(0, 3, size=1000) for _ in range(3)]
    stats = np.array([[l.max(), 1.0 / np.exp(l - l.max()).sum()] for l in logits], np.float32)
    pr = _rows([np.exp(l.max() - l.max()) * s for l, s in zip(logits, stats[:, 1])])
    r = region_ref.region_reduce([0, 3], stats, pr)
    allv = np.concatenate(logits)
    lse = allv.max() + np.log(np.exp(allv - allv.max()).sum())
    joint = np.array([np.exp(l.max() - lse) for l in logits])
    np.testing.assert_allclose(r["joint"], joint, rtol=1e-6)
    b = int(np.argmax(joint))
    assert r["best_pair"][0] == b
    np.testing.assert_allclose(r["tile_prob"], [np.exp(l - lse).sum() for l in logits], rtol=1e-6)


def test_ties_across_pairs_go_to_the_first():
    stats = np.array([[1.0, 0.5], [1.0, 0.5], [1.0, 0.5], [0.0, 0.5]], np.float32)
    pr = _rows([0.2, 0.3, 0.3, 0.5])
    r = region_ref.region_reduce([0, 1, 4], stats, pr)
    assert list(r["best_pair"]) == [0, 1]   # query 1: pairs 1 and 2 tie, pair 3 is lighter (mass e^-1)
    assert r["rows"][1, 0] == pr[1, 0]


def test_duplicate_tiles_split_the_mass_evenly():
    stats = np.array([[2.0, 0.25], [2.0, 0.25]], np.float32)   # the same tile twice: identical statistics
    pr = _rows([0.4, 0.4])
    r = region_ref.region_reduce([0, 2], stats, pr)
    assert r["tile_prob"][0] == np.float32(0.5) and r["tile_prob"][1] == np.float32(0.5)
    assert r["best_pair"][0] == 0
    assert r["rows"][0, 1] == np.float32(0.2)


def test_non_finite_statistics_never_win():
    pr = _rows([0.9, 0.5, 0.5, 0.1])
    for bad in (np.inf, -np.inf, np.nan):
        stats = np.array([[bad, 0.5], [1.0, 0.5], [1.0, np.nan], [0.5, 0.5]], np.float32)
        r = region_ref.region_reduce([0, 4], stats, pr)
        assert r["best_pair"][0] == 1, bad
        assert r["tile_prob"][0] == 0 and r["tile_prob"][2] == 0
        assert np.isfinite(r["rows"][0]).all()
        np.testing.assert_allclose(r["tile_prob"][[1, 3]].sum(), 1.0, rtol=1e-6)
    # no finite pair at all: the first pair, NaN probabilities
    stats = np.array([[np.nan, 0.5], [np.inf, 0.5]], np.float32)
    r = region_ref.region_reduce([0, 2], stats, pr[:2])
    assert r["best_pair"][0] == 0 and np.isnan(r["rows"][0, 1]) and np.isnan(r["tile_prob"]).all()
    assert r["rows"][0, 0] == pr[0, 0]


# ---- C entry point: argument checks -------------------------------------------------------------------------------------

def test_region_entry_points_are_exported(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_encode_ground", "ccvpe_ground_cache_bytes", "ccvpe_localize_region"):
        assert hasattr(lib, n)
    assert {"ccvpe_encode_ground", "ccvpe_ground_cache_bytes", "ccvpe_localize_region"} <= {n for n, _, _ in _lib.SYMBOLS}


def test_localize_region_checks_its_arguments_before_the_handle(built_library):
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    good_off = (C.c_int32 * 4)(0, 1, 5, 7)
    good_tiles = (C.c_int32 * 7)(0, 2, 1, 0, 2, 1, 1)

    def call(h=p, gc=p, nq=3, sc=p, nt=3, off=good_off, tiles=good_tiles, rows=p, best=p, prow=p, pst=p, tp=p):
        rc = lib.ccvpe_localize_region(h, gc, nq, 154, 231, sc, nt, off, tiles, rows, best, prow, pst, tp, None)
        return rc, (lib.ccvpe_last_error() or b"").decode()

    # a bogus handle is never read: every refusal below happens before the handle is used
    for kw, word in (("gc", "grd_cache"), ("sc", "sat_cache"), ("off", "offsets"), ("tiles", "tiles")):
        rc, msg = call(**{kw: None})
        assert rc == EINVAL and word in msg, (kw, msg)
    for kw in ("rows", "best", "prow", "pst", "tp"):
        rc, msg = call(**{kw: None})
        assert rc == EINVAL and "output" in msg, (kw, msg)
    for n in (0, -2):
        rc, msg = call(nq=n)
        assert rc == EINVAL and "n_queries" in msg
        rc, msg = call(nt=n)
        assert rc == EINVAL and "n_tiles" in msg
    rc, msg = call(off=(C.c_int32 * 4)(1, 2, 5, 7))
    assert rc == EINVAL and "offsets[0] = 1" in msg, msg
    rc, msg = call(off=(C.c_int32 * 4)(0, 1, 1, 7))
    assert rc == EINVAL and "offsets[2] = 1" in msg, msg
    rc, msg = call(off=(C.c_int32 * 4)(0, 3, 2, 7))
    assert rc == EINVAL and "offsets[2] = 2" in msg, msg
    rc, msg = call(tiles=(C.c_int32 * 7)(0, 2, 1, -1, 2, 1, 1))
    assert rc == EINVAL and "tiles[3] = -1" in msg, msg
    rc, msg = call(tiles=(C.c_int32 * 7)(0, 2, 1, 0, 2, 1, 3))
    assert rc == EINVAL and "tiles[6] = 3" in msg and "n_tiles 3" in msg, msg
    rc, msg = call(nt=2)   # the same list against a smaller cache: position 1 holds 2
    assert rc == EINVAL and "tiles[1] = 2" in msg, msg
    # valid arguments all the way: the null handle is the first thing refused
    rc, msg = call(h=None)
    assert rc == EINVAL and "handle" in msg, msg


def test_ground_cache_bytes_refuses_bad_arguments(built_library):
    lib = _lib.load()
    assert lib.ccvpe_ground_cache_bytes(None, 1, 154, 231) == 0
    assert lib.ccvpe_encode_ground(None, None, 154, 231, 1, None, None) == EINVAL


# ---- model methods ----------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_localize_region_refuses_bad_tile_lists():
    m = _model()
    gc, sc = torch.zeros(16), torch.zeros(16)
    for bad, word in (([], "at least one query"), ([[0], []], "empty"), ([[0, -1]], "negative"), ([[0, 1.5]], "integers"),
                      ([[0], [2 ** 33]], "int32"), ([[[0, 1]]], "1-D"), (5, "sequence"), ([np.array([True])], "integers")):
        with pytest.raises(ValueError, match=word):
            m.localize_region(gc, sc, bad)
    dev = torch.zeros(2, dtype=torch.int32, device="meta")   # any non-CPU tensor; the GPU test passes a cuda one
    for bad in (dev, [dev], [torch.tensor([0]), dev]):
        with pytest.raises(ValueError, match="host data"):
            m.localize_region(gc, sc, bad)
    # well-formed host lists (ragged, repeated ids, numpy / CPU tensors) get past the checks: the CPU caches are refused next
    for ok in ([[0], [1, 1, 0]], [np.array([2, 0], np.int64)], [torch.tensor([0, 3])], np.array([[0, 1], [1, 0]])):
        with pytest.raises(ValueError, match="cuda"):
            m.localize_region(gc, sc, ok)
    with pytest.raises(RuntimeError, match="eval"):
        _model().train().localize_region(gc, sc, [[0]])


def test_encode_ground_needs_a_cuda_batch():
    with pytest.raises(ValueError, match="cuda"):
        _model().encode_ground(torch.zeros(1, 3, 154, 231))


# ---- aerial.oxford_region ---------------------------------------------------------------------------------------------

def test_oxford_region_radius_zero_is_oxford_tiles():
    rng = np.random.default_rng(3)
    for coords in (rng.uniform(400, 9000, size=(30, 2)), 1000.0 + np.cumsum(rng.normal(0, 40, size=(25, 2)), axis=0),
                   np.array([[599.5, 1000.0], [599.49, 1000.0], [999.5, 999.5], [1399.5, 200.5], [200.0, 199.5]])):
        r = aerial.oxford_region(coords, 0)
        t = aerial.oxford_tiles(coords)
        np.testing.assert_array_equal(r["origin"], t["origin"])
        assert all(len(l) == 1 for l in r["tiles"])
        np.testing.assert_array_equal([l[0] for l in r["tiles"]], t["tile_index"])


def test_oxford_region_hand_checked_priors():
    # the cell of window x0 is [x0+199.5, x0+599.5): 1000 lies in window 800's (1000 - 400 = 600 is past window 400's)
    r = aerial.oxford_region([[1000.0, 1000.0]], 0)
    np.testing.assert_array_equal(r["origin"], [[800, 800]])
    # radius 1: the cell edges at 999.5 are 0.5 away on both axes, the corner (999.5, 999.5) sqrt(0.5) away: all four windows
    r = aerial.oxford_region([[1000.0, 1000.0]], 1.0)
    assert {tuple(o) for o in r["origin"]} == {(400, 400), (800, 400), (400, 800), (800, 800)}
    # radius 0.6: the corner is 0.707 away - only the two edge neighbours join
    r = aerial.oxford_region([[1000.0, 1000.0]], 0.6)
    assert {tuple(o) for o in r["origin"]} == {(800, 800), (400, 800), (800, 400)}
    # around the centre of window 800's cell the neighbours' cells are 200 px away, their corners 200 * sqrt 2 = 282.8 px
    block = {(x, y) for x in (400, 800, 1200) for y in (400, 800, 1200)}
    corners = {(400, 400), (1200, 400), (400, 1200), (1200, 1200)}
    assert {tuple(o) for o in aerial.oxford_region([[1199.5, 1199.5]], 282.0)["origin"]} == block - corners
    assert {tuple(o) for o in aerial.oxford_region([[1199.5, 1199.5]], 283.0)["origin"]} == block
    # radius exactly 200: the disc reaches the included lower edges of the cells above (1399.5) but not the excluded upper ones below
    assert {tuple(o) for o in aerial.oxford_region([[1199.5, 1199.5]], 200.0)["origin"]} == {(800, 800), (1200, 800), (800, 1200)}
    assert {tuple(o) for o in aerial.oxford_region([[1199.5, 1199.5]], 199.9)["origin"]} == {(800, 800)}
    # first-appearance order across queries, each query row-major, shared windows keep their first id
    r = aerial.oxford_region([[1000.0, 1000.0], [1000.0, 1000.0], [1700.0, 1000.0]], 0.6)
    assert r["tiles"][0] == r["tiles"][1]
    assert [tuple(r["origin"][i]) for i in r["tiles"][0]] == [(800, 400), (400, 800), (800, 800)]
    assert [tuple(r["origin"][i]) for i in r["tiles"][2]] == [(1200, 400), (1200, 800)]
    with pytest.raises(ValueError, match="radius"):
        aerial.oxford_region([[0.0, 0.0]], -1)


def test_oxford_region_holds_the_window_of_every_point_of_the_disc():
    rng = np.random.default_rng(5)
    for _ in range(12):
        p = rng.uniform(1000, 6000, size=2)
        rad = float(rng.choice([0.5, 37.0, 200.0, 399.5, 400.0, 650.0]))
        r = aerial.oxford_region(p[None], rad)
        have = {tuple(r["origin"][i]) for i in r["tiles"][0]}
        ang = rng.uniform(0, 2 * np.pi, 4000)
        d = rad * np.sqrt(rng.uniform(0, 1, 4000))
        d[:500] = rad                                           # the rim too
        q = p + np.stack([d * np.cos(ang), d * np.sin(ang)], axis=1)
        seen = {tuple(o) for o in aerial.oxford_window(q)["origin"]}
        assert seen <= have, (p, rad, seen - have)
        assert len(have) == len(r["tiles"][0]), "a query's windows are distinct"
        # and nothing far away: every window's cell is within the radius (plus the rounding half-pixel) of the prior
        for x0, y0 in have:
            gx = max(x0 + 199.5 - p[0], 0, p[0] - (x0 + 599.5))
            gy = max(y0 + 199.5 - p[1], 0, p[1] - (y0 + 599.5))
            assert np.hypot(gx, gy) <= rad + 1e-9


def test_oxford_region_to_map_round_trip():
    rng = np.random.default_rng(7)
    c = rng.uniform(1000, 8000, size=(5000, 2))
    c = np.concatenate([c, np.stack([np.arange(1000, 1800, 0.25), np.full(3200, 2345.6)], axis=1)])
    w = aerial.oxford_window(c)
    idx = np.array([aerial.gt_argmax(*o) for o in w["offset"]])
    back = aerial.oxford_region_to_map(w["origin"], idx)
    err = np.abs(back - c)
    # the window's centre column / row 255 is shared by two ground-truth offsets (gt_argmax's tie at offset 0): 2.5 px there
    centre = np.stack([idx % 512 == 255, idx // 512 == 255], axis=1)
    assert err[~centre].max() <= 800 / 512, err[~centre].max()
    assert err[centre].max() <= 2.5
    one = aerial.oxford_region_to_map((800, 400), int(idx[0]))
    assert one.shape == (2,)
    with pytest.raises(ValueError, match="index"):
        aerial.oxford_region_to_map((0, 0), 512 * 512)
