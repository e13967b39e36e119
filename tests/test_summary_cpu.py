"""The posterior summary without a GPU: the four C entry points and their argument checks (all made before the handle
is used), the model methods' checks, the numpy restatement tests/summary_ref.py pinned to closed forms, and aerial.summary_to_metres
against a row computed on scaled coordinates."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import summary_ref as sr

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_localize_summary", "ccvpe_localize_summary_cached_indexed", "ccvpe_postprocess_summary", "ccvpe_belief_summary")
RADII = (0, 1, 8, 32)


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_summary_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    for name in ("localize_summary", "localize_summary_cached", "postprocess_summary", "belief_summary"):
        assert callable(getattr(models.CVM_OxfordRobotCar, name))
    assert len(aerial.SUMMARY_FIELDS) == 16 and len(set(aerial.SUMMARY_FIELDS)) == 16


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def _callers(lib):
    bufs = [(C.c_float * 16)() for _ in range(4)]
    p, q, s, t = (C.cast(b, C.c_void_p) for b in bufs)
    tidx = (C.c_int32 * 2)(0, 1)

    def full(prior=p, stride=0, radius=8, rows=q, summ=s, post=t, grd=p, sat=p):
        return lib.ccvpe_localize_summary(None, grd, 154, 231, sat, 2, prior, stride, radius, rows, summ, post, None)

    def cached(prior=p, stride=0, radius=8, rows=q, summ=s, post=t, grd=p, cache=p, index=tidx, n_tiles=2):
        return lib.ccvpe_localize_summary_cached_indexed(None, grd, 154, 231, cache, n_tiles, index, 2, prior, stride, radius, rows, summ,
                                                         post, None)

    def logits(prior=p, stride=0, radius=8, rows=q, summ=s, post=t, logits=p, ori=p, batch=2):
        return lib.ccvpe_postprocess_summary(None, logits, ori, batch, prior, stride, radius, rows, summ, post, None)

    return {"full": full, "cached": cached, "logits": logits}, (p, q, s, t)


def test_pose_form_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    callers, (p, q, s, t) = _callers(lib)
    for name, call in callers.items():
        for bad in (1, N - 1, N + 1, -N, 2 * N):
            assert call(stride=bad) == EINVAL and "prior_stride" in _msg(lib), (name, bad, _msg(lib))
        for bad in (-1, 33, 1000):
            assert call(radius=bad) == EINVAL and "radius" in _msg(lib), (name, bad, _msg(lib))
        assert call(rows=None) == EINVAL and "handle" not in _msg(lib), name
        assert call(summ=None) == EINVAL and "summary" in _msg(lib), (name, _msg(lib))
        assert call(summ=q) == EINVAL and "alias" in _msg(lib), (name, _msg(lib))         # summary == rows
        assert call(post=p) == EINVAL and "alias" in _msg(lib), (name, _msg(lib))         # posterior == log_prior
        assert call(post=q) == EINVAL and "alias" in _msg(lib), (name, _msg(lib))         # posterior == rows
        assert call(post=s) == EINVAL and "alias" in _msg(lib), (name, _msg(lib))         # posterior == summary
        # valid arguments all the way, with and without prior and map: the null handle is the first thing refused
        for stride in (0, N):
            for radius in (0, 32):
                assert call(stride=stride, radius=radius) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        assert call(post=None) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        for stride in (0, 7):                                                             # no prior: the stride is ignored
            assert call(prior=None, stride=stride) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        assert call(prior=None, post=None) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
    for kw in ("grd", "sat"):
        assert callers["full"](**{kw: None}) == EINVAL and kw in _msg(lib)
    for kw in ("logits", "ori"):
        assert callers["logits"](**{kw: None}) == EINVAL and kw in _msg(lib)
    assert callers["logits"](prior=None, logits=t) == EINVAL and "alias" in _msg(lib)     # posterior == logits
    for batch in (0, 4097):
        assert callers["logits"](batch=batch) == EINVAL and "batch" in _msg(lib)
    assert callers["cached"](cache=None) == EINVAL and "cache" in _msg(lib)
    assert callers["cached"](index=(C.c_int32 * 2)(0, 2)) == EINVAL and "tile_index[1] = 2" in _msg(lib)
    assert callers["cached"](index=None) == EINVAL and "handle" in _msg(lib)
    assert callers["cached"](index=None, n_tiles=3) == EINVAL and "n_tiles 3 != batch 2" in _msg(lib)


def test_belief_form_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    a, b = (C.c_float * 16)(), (C.c_float * 16)()
    p, q = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)

    def call(belief=p, batch=2, radius=8, out=q):
        return lib.ccvpe_belief_summary(None, belief, batch, radius, out, None)

    assert call(belief=None) == EINVAL and "belief" in _msg(lib)
    assert call(out=None) == EINVAL and "summary" in _msg(lib)
    assert call(out=p) == EINVAL and "alias" in _msg(lib)
    assert call(belief=C.c_void_p(p.value + 2)) == EINVAL and "aligned" in _msg(lib)
    for r in (-1, 33, 1000):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for batch in (0, -1, 4097):
        assert call(batch=batch) == EINVAL and "batch" in _msg(lib), (batch, _msg(lib))
    for r in (0, 8, 32):
        for batch in (1, 4096):
            assert call(radius=r, batch=batch) == EINVAL and "handle" in _msg(lib), (r, batch, _msg(lib))
    assert call(belief=C.c_void_p(p.value + 4)) == EINVAL and "handle" in _msg(lib)        # 4-byte alignment is enough


# ---- model methods ---------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_model_methods_refuse_bad_arguments():
    m = _model()
    g, s = torch.zeros(3, 3, 154, 231), torch.zeros(3, 3, 512, 512)
    lg, ori = torch.zeros(3, N), torch.zeros(3, 2, 512, 512)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="radius"):
            m.localize_summary(g, s, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            m.postprocess_summary(lg, ori, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            m.belief_summary(torch.zeros(3, 512, 512), radius=bad)
    for shape in ((512, 511), (2, 512, 512), (3, 2, 512, 512), (N,)):
        with pytest.raises(ValueError, match="log_prior must be"):
            m.localize_summary(g, s, torch.zeros(shape))
        with pytest.raises(ValueError, match="log_prior must be"):
            m.postprocess_summary(lg, ori, torch.zeros(shape))
    with pytest.raises(ValueError, match="cuda"):
        m.localize_summary(g, s, torch.zeros(3, 512, 512))
    with pytest.raises(RuntimeError, match="cuda"):      # no prior: the inputs are refused as forward refuses them
        m.localize_summary(g, s)
    with pytest.raises(ValueError, match="cuda"):
        m.localize_summary_cached(g, torch.zeros(16))
    with pytest.raises(ValueError, match="tile_index"):
        m.localize_summary_cached(g, torch.zeros(16), None, tile_index=[0, 1])
    with pytest.raises(ValueError, match="logits"):
        m.postprocess_summary(torch.zeros(3, 100), ori)
    with pytest.raises(RuntimeError, match="cuda"):
        m.postprocess_summary(lg, ori)
    for bad in (torch.zeros(512, 512), torch.zeros(3, 512, 511), torch.zeros(3, 2, 512, 512), torch.zeros(3, N), np.zeros((3, 512, 512))):
        with pytest.raises(ValueError, match="belief must be"):
            m.belief_summary(bad)
    with pytest.raises(ValueError, match="belief must be float32"):
        m.belief_summary(torch.zeros(3, 512, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="belief must be contiguous"):
        m.belief_summary(torch.zeros(3, 512, 512).transpose(1, 2))
    for ok in (torch.zeros(3, 512, 512), torch.zeros(2, 1, 512, 512)):
        with pytest.raises(ValueError, match="belief must be a cuda tensor"):
            m.belief_summary(ok, radius=32)
    tr = _model().train()
    for call in (lambda: tr.localize_summary(g, s), lambda: tr.localize_summary_cached(g, s), lambda: tr.postprocess_summary(lg, ori),
                 lambda: tr.belief_summary(torch.zeros(1, 512, 512))):
        with pytest.raises(RuntimeError, match="eval"):
            call()


# ---- the restatement against closed forms ----------------------------------------------------------------------------------
MAPS = sr.crafted_maps()


def _cells(x, y, r):
    return (min(x + r, 511) - max(x - r, 0) + 1) * (min(y + r, 511) - max(y - r, 0) + 1)


@pytest.mark.parametrize("r", RADII)
def test_a_delta_is_a_point(r):
    for name, (x, y) in (("delta_origin", (0, 0)), ("delta_corner", (511, 511)), ("delta_inside", (200, 300))):
        row = sr.summary(MAPS[name], r)
        assert row[0] == y * 512 + x and row[1] == 1.0 and row[2] == 1.0 and row[3] == 0.0
        assert (row[4], row[5]) == (x, y) and (row[10], row[11]) == (x, y)
        assert (row[6:9] == 0).all() and (row[12:15] == 0).all() and row[9] == 1.0
        want = (r + 1) ** 2 if name != "delta_inside" else (2 * r + 1) ** 2
        assert row[15] == want == _cells(x, y, r)


@pytest.mark.parametrize("r", RADII)
def test_uniform_map(r):
    row = sr.summary(MAPS["uniform"], r)
    assert row[0] == 0 and row[1] == np.float32(1.0 / N)                  # the first index is the corner
    assert row[2] == pytest.approx(1.0, rel=1e-12) and row[3] == pytest.approx(math.log(N), rel=1e-12)
    assert row[4] == pytest.approx(255.5, rel=1e-12) and row[5] == pytest.approx(255.5, rel=1e-12)
    assert row[6] == pytest.approx((512 ** 2 - 1) / 12, rel=1e-12) and row[6] == pytest.approx(21845.25, rel=1e-12)
    assert row[8] == pytest.approx(21845.25, rel=1e-12) and abs(row[7]) <= 1e-9
    assert row[9] == pytest.approx((r + 1) ** 2 / N, rel=1e-12) and row[15] == (r + 1) ** 2
    assert row[10] == pytest.approx(r / 2, abs=1e-12) and row[12] == pytest.approx(((r + 1) ** 2 - 1) / 12, abs=1e-9)


@pytest.mark.parametrize("r", RADII)
def test_two_equal_deltas_and_a_scaled_copy(r):
    row = sr.summary(MAPS["two_deltas"], r)
    assert row[0] == 77 * 512 + 150 and row[1] == 0.5                     # the raster-first of the two
    assert row[2] == 1.0 and row[3] == pytest.approx(math.log(2), rel=1e-15)
    assert (row[4], row[5]) == (200.0, 77.0) and (row[6], row[7], row[8]) == (2500.0, 0.0, 0.0)
    assert row[9] == 0.5 and (row[10], row[11]) == (150.0, 77.0) and (row[12:15] == 0).all()       # r < 100: one delta in the window
    big = sr.summary(MAPS["two_deltas_scaled"], r)
    assert big[1] == 1.75 and big[2] == 3.5
    keep = [c for c in range(16) if c not in (1, 2)]
    np.testing.assert_allclose(big[keep], row[keep], rtol=1e-15, atol=0)


def test_special_maps_of_the_restatement():
    z = sr.summary(np.zeros((512, 512), np.float32), 8)
    assert (z[:3] == 0).all() and np.isnan(z[3:]).all()
    m = MAPS["random"].copy()
    m[10, 20] = np.nan
    m[400, 17] = 2.0
    row = sr.summary(m, 8)
    assert row[0] == 400 * 512 + 17 and row[1] == 2.0 and np.isnan(row[2:10]).all() and row[15] == 17 * 17
    tie = sr.delta((300, 40), (30, 41), (31, 41), value=0.25)
    row = sr.summary(tie, 1)
    assert row[0] == 40 * 512 + 300 and row[9] == pytest.approx(1 / 3) and (row[10], row[11]) == (300.0, 40.0)


def test_clipped_window_and_random_map():
    g = sr.summary(MAPS["gauss_border"], 8)
    assert g[0] == 2 * 512 + 509 and g[15] == (8 + 3) * (8 + 3)           # x in 501..511, y in 0..10
    assert g[9] > 0.99 and g[12] < 9.0 and g[14] < 9.0                    # the border cuts the tails off
    rnd = sr.summary(MAPS["random"], 32)
    assert rnd[2] == pytest.approx(0.525 * N, rel=5e-3) and rnd[6] == pytest.approx(21845.25, rel=2e-2)


# ---- summary_to_metres -----------------------------------------------------------------------------------------------------

def test_summary_to_metres_is_the_summary_on_scaled_coordinates():
    assert aerial.SUMMARY_FIELDS[0] == "index" and aerial.SUMMARY_FIELDS[3] == "entropy" and aerial.SUMMARY_FIELDS[9] == "peak_mass"
    f = 0.1171875
    h = MAPS["gauss_centre"].astype(np.float64)
    row = sr.summary(MAPS["gauss_centre"], 8)
    got = aerial.summary_to_metres(row, f)
    assert got.dtype == np.float64 and got.shape == (16,)
    # the same moments with the cell coordinates in metres
    x = np.arange(512)[None, :] * f
    y = np.arange(512)[:, None] * f
    s0, mx, my, vxx, vxy, vyy = sr._moments(h, x, y)
    np.testing.assert_allclose(got[4:9], [mx, my, vxx, vxy, vyy], rtol=1e-9, atol=1e-12)   # (cov_xy is a rounding residue of ~5e-10)
    ys, xs = divmod(int(row[0]), 512)
    w = sr._moments(h[ys - 8:ys + 9, xs - 8:xs + 9], x[:, xs - 8:xs + 9], y[ys - 8:ys + 9, :])
    np.testing.assert_allclose(got[10:15], w[1:], rtol=1e-9, atol=1e-12)
    keep = [0, 1, 2, 3, 9, 15]
    np.testing.assert_array_equal(got[keep], row[keep])
    # one factor per row, tensors, float32
    rows = torch.from_numpy(np.stack([row, row]).astype(np.float32))
    two = aerial.summary_to_metres(rows, [1.0, 2.0])
    assert isinstance(two, torch.Tensor) and two.dtype == torch.float32
    assert torch.equal(two[0], rows[0])
    np.testing.assert_allclose(two[1, [4, 5, 10, 11]].numpy(), 2 * rows[1, [4, 5, 10, 11]].numpy(), rtol=1e-7)
    np.testing.assert_allclose(two[1, [6, 7, 8, 12, 13, 14]].numpy(), 4 * rows[1, [6, 7, 8, 12, 13, 14]].numpy(), rtol=1e-7)
    assert torch.equal(two[1, keep], rows[1, keep])
    with pytest.raises(ValueError, match="summary must be"):
        aerial.summary_to_metres(np.zeros(15), 1.0)


def test_tracker_step_takes_a_summary_radius():
    t = aerial.Tracker()
    with pytest.raises(ValueError, match="origins"):
        t.step(_model(), torch.zeros(2, 3, 154, 231), torch.zeros(16), None, [[800, 400]], [0, 0], [1.0], 0.0, summary_radius=8)
