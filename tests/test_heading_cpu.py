"""The heading posterior without a GPU: the three C entry points and their argument checks (all made before the
handle is used), the model methods' checks, the numpy restatement tests/heading_ref.py pinned to closed forms, and the two helpers of
ccvpe_amd.aerial."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import heading_ref as hr

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_localize_heading", "ccvpe_localize_heading_cached_indexed", "ccvpe_postprocess_heading")
UNIFORM = np.full((512, 512), 1.0 / N, np.float32)


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_heading_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    for name in ("localize_heading", "localize_heading_cached", "postprocess_heading"):
        assert callable(getattr(models.CVM_OxfordRobotCar, name))
    assert len(aerial.HEADING_FIELDS) == 12 and len(set(aerial.HEADING_FIELDS)) == 12


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def _callers(lib):
    bufs = [(C.c_float * 16)() for _ in range(7)]
    p, q, hd, hs, s, t, x = (C.cast(b, C.c_void_p) for b in bufs)
    tidx = (C.c_int32 * 2)(0, 1)

    def full(prior=p, stride=0, radius=8, bins=72, rows=q, head=hd, hist=hs, summ=s, post=t, grd=x, sat=x):
        return lib.ccvpe_localize_heading(None, grd, 154, 231, sat, 2, prior, stride, radius, bins, rows, head, hist, summ, post, None)

    def cached(prior=p, stride=0, radius=8, bins=72, rows=q, head=hd, hist=hs, summ=s, post=t, grd=x, cache=x, index=tidx, n_tiles=2):
        return lib.ccvpe_localize_heading_cached_indexed(None, grd, 154, 231, cache, n_tiles, index, 2, prior, stride, radius, bins, rows,
                                                         head, hist, summ, post, None)

    def logits(prior=p, stride=0, radius=8, bins=72, rows=q, head=hd, hist=hs, summ=s, post=t, logits=x, ori=x, batch=2):
        return lib.ccvpe_postprocess_heading(None, logits, ori, batch, prior, stride, radius, bins, rows, head, hist, summ, post, None)

    return {"full": full, "cached": cached, "logits": logits}, (p, q, hd, hs, s, t, x)


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    callers, (p, q, hd, hs, s, t, x) = _callers(lib)
    for name, call in callers.items():
        for bad in (1, N - 1, N + 1, -N, 2 * N):
            assert call(stride=bad) == EINVAL and "prior_stride" in _msg(lib), (name, bad, _msg(lib))
        for bad in (-1, 33, 1000):
            assert call(radius=bad) == EINVAL and "radius" in _msg(lib), (name, bad, _msg(lib))
        for bad in (-1, 0, 3, 361, 100000):
            assert call(bins=bad) == EINVAL and "nbins" in _msg(lib), (name, bad, _msg(lib))
        assert call(rows=None) == EINVAL and "handle" not in _msg(lib), name
        assert call(head=None) == EINVAL and "heading" in _msg(lib), (name, _msg(lib))
        assert call(hist=None) == EINVAL and "hist" in _msg(lib), (name, _msg(lib))
        # heading and hist alias nothing: each other, rows, the prior, the summary, the posterior
        for kw in (dict(head=hs), dict(head=q), dict(hist=q), dict(head=p), dict(hist=p), dict(summ=hd), dict(summ=hs), dict(post=hd),
                   dict(post=hs)):
            assert call(**kw) == EINVAL and "alias" in _msg(lib), (name, kw, _msg(lib))
        # ... and the rules of the summary forms hold for the rest
        for kw in (dict(summ=q), dict(post=p), dict(post=q), dict(post=s)):
            assert call(**kw) == EINVAL and "alias" in _msg(lib), (name, kw, _msg(lib))
        # valid arguments all the way, with and without prior, summary and map: the null handle is the first thing refused
        for stride in (0, N):
            for radius in (0, 32):
                for bins in (4, 72, 360):
                    assert call(stride=stride, radius=radius, bins=bins) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        for kw in (dict(post=None), dict(summ=None), dict(summ=None, post=None), dict(prior=None, stride=7), dict(prior=None, summ=None, post=None)):
            assert call(**kw) == EINVAL and "handle" in _msg(lib), (name, kw, _msg(lib))
    for kw in ("grd", "sat"):
        assert callers["full"](**{kw: None}) == EINVAL and kw in _msg(lib)
    for kw in ("logits", "ori"):
        assert callers["logits"](**{kw: None}) == EINVAL and kw in _msg(lib)
    assert callers["logits"](prior=None, logits=t) == EINVAL and "alias" in _msg(lib)     # posterior == logits
    for kw in (dict(logits=hd), dict(ori=hd), dict(logits=hs), dict(ori=hs)):
        assert callers["logits"](**kw) == EINVAL and "alias" in _msg(lib), kw
    for batch in (0, 4097):
        assert callers["logits"](batch=batch) == EINVAL and "batch" in _msg(lib)
    assert callers["cached"](cache=None) == EINVAL and "cache" in _msg(lib)
    assert callers["cached"](index=(C.c_int32 * 2)(0, 2)) == EINVAL and "tile_index[1] = 2" in _msg(lib)
    assert callers["cached"](index=None) == EINVAL and "handle" in _msg(lib)
    assert callers["cached"](index=None, n_tiles=3) == EINVAL and "n_tiles 3 != batch 2" in _msg(lib)


# ---- model methods ---------------------------------------------------------------------------------------------------------

def test_model_methods_refuse_bad_arguments():
    m = models.CVM_OxfordRobotCar("cpu").eval()
    g, s = torch.zeros(3, 3, 154, 231), torch.zeros(3, 3, 512, 512)
    lg, ori = torch.zeros(3, N), torch.zeros(3, 2, 512, 512)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="radius"):
            m.localize_heading(g, s, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            m.localize_heading_cached(g, torch.zeros(16), radius=bad)
        with pytest.raises(ValueError, match="radius"):
            m.postprocess_heading(lg, ori, radius=bad)
    for bad in (0, 3, 361, -72):
        with pytest.raises(ValueError, match="bins"):
            m.localize_heading(g, s, bins=bad)
        with pytest.raises(ValueError, match="bins"):
            m.localize_heading_cached(g, torch.zeros(16), bins=bad)
        with pytest.raises(ValueError, match="bins"):
            m.postprocess_heading(lg, ori, bins=bad)
    for shape in ((512, 511), (2, 512, 512), (3, 2, 512, 512), (N,)):
        with pytest.raises(ValueError, match="log_prior must be"):
            m.localize_heading(g, s, torch.zeros(shape))
        with pytest.raises(ValueError, match="log_prior must be"):
            m.postprocess_heading(lg, ori, torch.zeros(shape))
    with pytest.raises(ValueError, match="cuda"):
        m.localize_heading(g, s, torch.zeros(3, 512, 512))
    with pytest.raises(RuntimeError, match="cuda"):      # no prior: the inputs are refused as forward refuses them
        m.localize_heading(g, s)
    with pytest.raises(ValueError, match="cuda"):
        m.localize_heading_cached(g, torch.zeros(16))
    with pytest.raises(ValueError, match="tile_index"):
        m.localize_heading_cached(g, torch.zeros(16), None, tile_index=[0, 1])
    with pytest.raises(ValueError, match="logits"):
        m.postprocess_heading(torch.zeros(3, 100), ori)
    with pytest.raises(RuntimeError, match="cuda"):
        m.postprocess_heading(lg, ori)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.localize_heading(g, s)
    with pytest.raises(RuntimeError, match="eval"):
        m.postprocess_heading(lg, ori)


# ---- the restatement against closed forms -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", (4, 20, 72, 360))
def test_constant_field_is_one_bin(nbins):
    for angle in (0.5, 123.5, 359.5):
        row, hist, E = hr.heading(UNIFORM, hr.Field(hr.unit_field(angle)), nbins, 8)
        b = int(angle // (360.0 / nbins))
        assert hist[b] == pytest.approx(1.0, abs=1e-12) and np.count_nonzero(hist) == 1
        assert row[0] == pytest.approx(1.0, abs=1e-12) and row[4] == pytest.approx(1.0, abs=1e-7) and row[5] == b and row[6] == 1.0
        assert hr.circ_diff(row[3], angle) < 1e-5 and hr.circ_diff(row[10], angle) < 1e-5
        assert row[7] == pytest.approx(81.0 / N, rel=1e-12)       # the argmax of a uniform map is cell 0: a 9 x 9 window cut to 9 x 9 at the corner
        assert row[11] == pytest.approx(1.0, abs=1e-7) and E.sum() == 0.0


def test_two_opposite_headings_of_equal_mass_have_no_mean():
    yy, xx = np.mgrid[0:512, 0:512]
    f = hr.unit_field(np.where((xx + yy) % 2 == 0, 0.0, 180.0))
    f[1] = 0.0                                                    # exactly (1, 0) and (-1, 0)
    row, hist, _ = hr.heading(UNIFORM, hr.Field(f), 72, 0)
    assert row[0] == pytest.approx(1.0, abs=1e-12) and row[1] == 0.0 and row[2] == 0.0 and row[4] == 0.0 and math.isnan(row[3])
    assert hist[0] == pytest.approx(0.5, abs=1e-12) and hist[36] == pytest.approx(0.5, abs=1e-12) and row[5] == 0 and row[6] == pytest.approx(0.5)
    assert row[11] == 1.0 and row[10] == 0.0                      # the window of radius 0 is one cell: heading 0


@pytest.mark.parametrize("nbins", (4, 20, 72, 360))
def test_angle_linear_in_the_index_gives_a_flat_histogram(nbins):
    a = (np.arange(N, dtype=np.float64) + 0.5) * (360.0 / N)      # every bin holds N / nbins cells, none within 1e-3 degree of an edge?
    row, hist, E = hr.heading(UNIFORM, hr.Field(hr.unit_field(a.reshape(512, 512))), nbins, 8)
    hr.assert_edge_cap(row, E)
    np.testing.assert_allclose(hist, 1.0 / nbins, atol=E.max() + 1e-12)
    assert row[0] == pytest.approx(1.0, abs=1e-12) and row[4] < 1e-6 and row[6] == pytest.approx(1.0 / nbins, abs=E.max() + 1e-12)
    assert hist.sum() == pytest.approx(row[0], abs=1e-12)


def test_invalid_cells_reduce_the_mass():
    f = hr.unit_field(45.5)
    f[:, 0, :] = np.nan              # 512 cells
    f[0, 1, :] = np.inf              # 512
    f[1, 2, :] = -np.inf             # 512
    f[:, 3, :] = 0.0                 # 512: the zero vector
    f[1, 4, :] = 0.0                 # (c, 0): valid, heading 0
    f[0, 4, :] = 1.0
    row, hist, _ = hr.heading(UNIFORM, hr.Field(f), 72, 0)
    assert row[0] == pytest.approx(1.0 - 4 * 512 / N, abs=1e-12) and hist.sum() == pytest.approx(row[0], abs=1e-12)
    assert hist[0] == pytest.approx(512 / N, abs=1e-12) and hist[9] == pytest.approx(1.0 - 5 * 512 / N, abs=1e-12)
    assert row[7] == 0.0 and np.isnan(row[8:12]).all()            # the argmax cell (0, 0) is invalid: an empty window
    allbad = np.zeros((2, 512, 512), np.float32)
    row, hist, _ = hr.heading(UNIFORM, hr.Field(allbad), 72, 8)
    assert row[0] == 0.0 and row[7] == 0.0 and (hist == 0).all() and row[5] == 0 and np.isnan(row[[1, 2, 3, 4, 6, 8, 9, 10, 11]]).all()
    row, hist, _ = hr.heading(UNIFORM, hr.Field(hr.unit_field(10.5)), 72, 8, ok=False)
    assert row[5] == -1 and np.isnan(np.delete(row, 5)).all() and (hist == 0).all()


def test_wrap_and_negative_zero_rules():
    f = hr.unit_field(0.0)
    f[0], f[1] = 1.0, -0.0                                        # angle -0.0: bin 0
    assert hr.heading(UNIFORM, hr.Field(f), 72, 0)[0][5] == 0
    f[1] = -1e-30                                                 # s < 0 with acos(1) = 0: 360 - 0 = 360 wraps to bin 0
    row, hist, _ = hr.heading(UNIFORM, hr.Field(f), 72, 0)
    assert row[5] == 0 and hist[0] == pytest.approx(1.0, abs=1e-12) and hist[71] == 0.0
    row, hist, E = hr.heading(UNIFORM, hr.Field(hr.unit_field(89.9995)), 4, 0)        # within 1e-3 of the edge at 90: an edge cell of bins 0 and 1
    assert row[5] == 0 and E[0] == pytest.approx(1.0) and E[1] == pytest.approx(1.0) and E[2:].sum() == 0.0
    with pytest.raises(AssertionError, match="edge cells"):
        hr.assert_edge_cap(row, E)
    row, hist, _ = hr.heading(UNIFORM, hr.Field(hr.unit_field(-90.0)), 4, 0)          # s = -1: 360 - 90 = 270, bin 3 of 4
    assert row[5] == 3 and hr.circ_diff(row[3], 270.0) < 1e-5


@pytest.mark.parametrize("radius,cells", ((0, 1), (1, 4), (8, 81), (32, 33 * 33)))
def test_window_in_a_corner(radius, cells):
    h = np.full((512, 512), 1e-9, np.float32)
    h[511, 511] = 0.5                                             # argmax in the last cell: the window is clipped on two sides
    yy, xx = np.mgrid[0:512, 0:512]
    f = hr.unit_field(np.where((xx >= 511 - 1) & (yy >= 511 - 1), 90.5, 200.5))
    row, _, _ = hr.heading(h, hr.Field(f), 72, radius)
    inner = min(cells, 4)
    assert row[7] == pytest.approx(0.5 + (cells - 1) * float(np.float32(1e-9)), rel=1e-9)
    c = (np.cos(np.radians(90.5)) * (0.5 + (inner - 1) * 1e-9) + np.cos(np.radians(200.5)) * (cells - inner) * 1e-9) / row[7]
    assert row[8] == pytest.approx(c, abs=1e-7)
    assert hr.circ_diff(row[10], 90.5) < 1e-3 and row[11] == pytest.approx(1.0, abs=1e-5)


def test_assert_close_holds_the_bounds():
    fld = hr.Field(hr.crafted_fields()["two_mode"])
    ref = hr.heading(UNIFORM, fld, 72, 8)
    row, hist, _ = ref
    hr.assert_close(row.astype(np.float32), hist.astype(np.float32), ref)
    bad = hist.astype(np.float32).copy()
    bad[8] += np.float32(3e-7)                                    # more than 2^-23 * 1/3 + 2^-33
    with pytest.raises(AssertionError, match="hist"):
        hr.assert_close(row.astype(np.float32), bad, ref)
    for col, d in ((0, 2e-6), (4, 2e-6), (3, 2e-3), (5, 1), (10, 2e-3)):
        r = row.astype(np.float32).copy()
        r[col] += d
        with pytest.raises(AssertionError):
            hr.assert_close(r, hist.astype(np.float32), ref)
    for name, f in hr.crafted_fields().items():                   # every crafted field keeps its edge cells under the cap at every bin count
        for nbins in (4, 20, 72, 360):
            r, _, E = hr.heading(UNIFORM, hr.Field(f), nbins, 8)
            hr.assert_edge_cap(r, E, f"{name} {nbins}")


# ---- aerial helpers ----------------------------------------------------------------------------------------------------------

def test_bin_centres_and_sigma():
    np.testing.assert_allclose(aerial.heading_bin_centres(72), np.arange(72) * 5.0 + 2.5)
    np.testing.assert_allclose(aerial.heading_bin_centres(4), [45.0, 135.0, 225.0, 315.0])
    assert aerial.heading_bin_centres(360).shape == (360,)
    for bad in (3, 361, 0):
        with pytest.raises(ValueError, match="bins"):
            aerial.heading_bin_centres(bad)
    R = np.array([1.0, 0.9, 0.5, 1e-3])
    np.testing.assert_allclose(aerial.heading_sigma_deg(R), np.degrees(np.sqrt(-2.0 * np.log(R))))
    assert aerial.heading_sigma_deg(1.0) == 0.0 and np.isinf(aerial.heading_sigma_deg(0.0))
    assert np.isnan(aerial.heading_sigma_deg(np.array([1.5, -0.1, np.nan]))).all()
    np.testing.assert_allclose(aerial.heading_sigma_deg(torch.tensor([0.9, 0.5])), np.degrees(np.sqrt(-2.0 * np.log([0.9, 0.5]))), rtol=1e-6)
    # a von Mises-like concentrated distribution: sigma of a wrapped normal with standard deviation 10 degrees is 10 degrees
    assert aerial.heading_sigma_deg(math.exp(-0.5 * math.radians(10.0) ** 2)) == pytest.approx(10.0)
