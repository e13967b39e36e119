"""Localize with a position prior without a GPU: the argument checks of the four C entry points (all made before the handle is used)
and of the model methods, the numpy restatement tests/prior_ref.py on crafted maps, and the two log-prior helpers against their
closed forms."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import prior_ref, topk_ref

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_localize_prior", "ccvpe_localize_prior_cached_indexed", "ccvpe_postprocess_prior", "ccvpe_localize_region_prior")


# ---- C entry points: argument checks -------------------------------------------------------------------------------------

def test_prior_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}


def _callers(lib):
    """one call per entry point with a null handle; keyword overrides replace single arguments"""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    tidx = (C.c_int32 * 2)(0, 1)
    off = (C.c_int32 * 3)(0, 1, 3)
    tiles = (C.c_int32 * 3)(0, 1, 0)

    def loc(prior=p, stride=0, k=0, r=0, rows=p, grd=p, sat=p):
        return lib.ccvpe_localize_prior(None, grd, 154, 231, sat, 2, prior, stride, k, r, rows, None)

    def cached(prior=p, stride=0, k=0, r=0, rows=p, grd=p, cache=p, index=tidx):
        return lib.ccvpe_localize_prior_cached_indexed(None, grd, 154, 231, cache, 2, index, 2, prior, stride, k, r, rows, None)

    def post(prior=p, stride=0, k=0, r=0, rows=p, logits=p, ori=p):
        return lib.ccvpe_postprocess_prior(None, logits, ori, 2, prior, stride, k, r, rows, None)

    def region(prior=p, stride=0, k=0, r=0, rows=p):
        assert k == 0 and r == 0   # the region form has no k / radius
        return lib.ccvpe_localize_region_prior(None, p, 2, 154, 231, p, 2, off, tiles, prior, stride, rows, p, p, p, p, None)

    return {"localize": loc, "cached": cached, "post": post, "region": region}


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def test_prior_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    for name, call in _callers(lib).items():
        assert call(prior=None) == EINVAL and "log_prior" in _msg(lib), (name, _msg(lib))
        for bad in (1, N - 1, N + 1, -N, 2 * N):
            assert call(stride=bad) == EINVAL and "prior_stride" in _msg(lib), (name, bad, _msg(lib))
        assert call(rows=None) == EINVAL, name
        # valid arguments all the way: the null handle is the first thing refused
        for stride in (0, N):
            assert call(stride=stride) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        if name == "region":
            continue
        for k in (-1, 65):
            assert call(k=k) == EINVAL and "k must" in _msg(lib), (name, k, _msg(lib))
        for r in (-1, 33):
            assert call(k=4, r=r) == EINVAL and "radius" in _msg(lib), (name, r, _msg(lib))
        assert call(k=0, r=3) == EINVAL and "radius" in _msg(lib) and "k" in _msg(lib), (name, _msg(lib))
        for k, r in ((1, 0), (64, 32), (8, 16)):
            assert call(k=k, r=r) == EINVAL and "handle" in _msg(lib), (name, k, r, _msg(lib))


def test_input_pointers_and_the_cached_tile_index_are_checked(built_library):
    lib = _lib.load()
    c = _callers(lib)
    for kw, word in (("grd", "grd"), ("sat", "sat")):
        assert c["localize"](**{kw: None}) == EINVAL and word in _msg(lib)
    for kw, word in (("logits", "logits"), ("ori", "ori")):
        assert c["post"](**{kw: None}) == EINVAL and word in _msg(lib)
    assert c["cached"](cache=None) == EINVAL and "cache" in _msg(lib)
    assert c["cached"](index=(C.c_int32 * 2)(0, 2)) == EINVAL and "tile_index[1] = 2" in _msg(lib)
    # no tile_index: query b reads tile b, so the cache holds one tile per query
    assert c["cached"](index=None) == EINVAL and "handle" in _msg(lib)
    p = C.cast((C.c_float * 4)(), C.c_void_p)
    rc = lib.ccvpe_localize_prior_cached_indexed(None, p, 154, 231, p, 3, None, 2, p, 0, 0, 0, p, None)
    assert rc == EINVAL and "n_tiles 3 != batch 2" in _msg(lib)
    for batch in (0, 4097):
        assert lib.ccvpe_postprocess_prior(None, p, p, batch, p, 0, 0, 0, p, None) == EINVAL and "batch" in _msg(lib)
    # the region form checks its pair list first, as ccvpe_localize_region
    rc = lib.ccvpe_localize_region_prior(None, p, 2, 154, 231, p, 2, (C.c_int32 * 3)(0, 1, 3), (C.c_int32 * 3)(0, 2, 0), p, 0, p, p, p,
                                         p, p, None)
    assert rc == EINVAL and "tiles[1] = 2" in _msg(lib)


# ---- model methods ----------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_model_methods_refuse_bad_priors():
    m = _model()
    g, s = torch.zeros(3, 3, 154, 231), torch.zeros(3, 3, 512, 512)
    bad_shapes = [(512, 511), (2, 512, 512), (3, 2, 512, 512), (3, 1, 1, 512, 512), (N,), (3, N)]
    for shape in bad_shapes:
        with pytest.raises(ValueError, match="log_prior must be"):
            m.localize_prior(g, s, torch.zeros(shape))
        with pytest.raises(ValueError, match="log_prior must be"):
            m.postprocess_prior(torch.zeros(3, N), torch.zeros(3, 2, 512, 512), torch.zeros(shape))
    with pytest.raises(ValueError, match="float32"):
        m.localize_prior(g, s, torch.zeros(3, 512, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        m.localize_prior(g, s, torch.zeros(512, 512).t())
    for shape in ((512, 512), (1, 512, 512), (3, 512, 512), (1, 1, 512, 512), (3, 1, 512, 512)):   # accepted shapes: CPU refused next
        with pytest.raises(ValueError, match="cuda"):
            m.localize_prior(g, s, torch.zeros(shape))
    for k, r, word in ((-1, 0, "k must"), (65, 0, "k must"), (4, 33, "radius"), (0, 2, "radius")):
        with pytest.raises(ValueError, match=word):
            m.localize_prior(g, s, torch.zeros(512, 512), k=k, radius=r)
    with pytest.raises(ValueError, match="cuda"):
        m.localize_prior_cached(g, torch.zeros(16), torch.zeros(512, 512))
    with pytest.raises(ValueError, match="cuda"):
        m.postprocess_prior(torch.zeros(3, N), torch.zeros(3, 2, 512, 512), torch.zeros(3, 512, 512))
    with pytest.raises(ValueError, match="logits"):
        m.postprocess_prior(torch.zeros(3, 100), torch.zeros(3, 2, 512, 512), torch.zeros(3, 512, 512))
    # the region form: one map or one per pair (P = 3 here)
    with pytest.raises(ValueError, match="log_prior must be"):
        m.localize_region_prior(torch.zeros(16), torch.zeros(16), [[0], [1, 0]], torch.zeros(2, 512, 512))
    with pytest.raises(ValueError, match="cuda"):
        m.localize_region_prior(torch.zeros(16), torch.zeros(16), [[0], [1, 0]], torch.zeros(3, 512, 512))
    with pytest.raises(ValueError, match="empty"):
        m.localize_region_prior(torch.zeros(16), torch.zeros(16), [[0], []], torch.zeros(512, 512))
    tr = _model().train()
    for call in (lambda: tr.localize_prior(g, s, torch.zeros(512, 512)), lambda: tr.localize_prior_cached(g, s, torch.zeros(512, 512)),
                 lambda: tr.postprocess_prior(torch.zeros(3, N), torch.zeros(3, 2, 512, 512), torch.zeros(512, 512)),
                 lambda: tr.localize_region_prior(torch.zeros(16), torch.zeros(16), [[0]], torch.zeros(512, 512))):
        with pytest.raises(RuntimeError, match="eval"):
            call()


# ---- prior_ref on crafted maps ------------------------------------------------------------------------------------------------

def _ori(B, n):
    rng = np.random.default_rng(1)
    a = rng.uniform(-np.pi, np.pi, size=(B, n))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def test_zero_prior_is_the_plain_softmax_and_ties_go_to_the_first_index():
    rng = np.random.default_rng(0)
    lg = rng.normal(0, 2, size=(2, N)).astype(np.float32)
    lg[1, [7, 3000, 99]] = lg[1].max() + 1.0   # three-way tie
    ori = _ori(2, N)
    post = prior_ref.posterior(lg, np.zeros(N, np.float32))
    e = np.exp(lg.astype(np.float64) - lg.max(axis=1, keepdims=True))
    np.testing.assert_allclose(post["h"], e / e.sum(axis=1, keepdims=True), rtol=1e-12)
    rows, margin = prior_ref.argmax_rows(lg, ori, np.zeros(N, np.float32))
    assert rows[0, 0] == np.argmax(lg[0]) and rows[1, 0] == 7 and margin[1] == 0
    np.testing.assert_array_equal(rows[1, 2:4], ori[1, :, 7])
    # a prior that favours the last of the tied pixels moves the argmax there
    lp = np.zeros(N, np.float32)
    lp[99] = 0.5
    rows, _ = prior_ref.argmax_rows(lg, ori, lp)
    assert rows[1, 0] == 99


def test_minus_inf_window_and_all_minus_inf():
    rng = np.random.default_rng(2)
    lg = rng.normal(0, 2, size=(3, N)).astype(np.float32)
    ori = _ori(3, N)
    lp = np.full((3, 512, 512), -np.inf, np.float32)
    lp[0, 100:140, 300:330] = 0.0            # a box
    lp[1] = 0.0
    lp[1, 0, 5] = np.nan                     # a NaN anywhere: no finite posterior
    # query 2: -inf everywhere
    post = prior_ref.posterior(lg, lp.reshape(3, N))
    assert post["finite"].tolist() == [True, False, False]
    h0 = post["h"][0].reshape(512, 512)
    assert (h0[100:140, 300:330] > 0).all() and h0.sum() == pytest.approx(1.0)
    assert (np.delete(h0.reshape(-1), (np.arange(100, 140)[:, None] * 512 + np.arange(300, 330)).reshape(-1)) == 0).all()
    rows, _ = prior_ref.argmax_rows(lg, ori, lp.reshape(3, N))
    y, x = divmod(int(rows[0, 0]), 512)
    assert 100 <= y < 140 and 300 <= x < 330
    assert rows[1, 0] == -1 and np.isnan(rows[1, 1]) and rows[2, 0] == -1 and np.isnan(rows[2, 1])
    tk = prior_ref.topk_rows(lg, ori, lp.reshape(3, N), 8, 4)
    yy, xx = np.divmod(tk[0, :, 0].astype(np.int64), 512)
    assert (tk[0, :, 0] >= 0).all() and ((yy >= 100) & (yy < 140) & (xx >= 300) & (xx < 330)).all()
    assert tk[0, 0, 0] == rows[0, 0] and tk[0, 0, 1] == np.float32(rows[0, 1])
    for b in (1, 2):
        np.testing.assert_array_equal(tk[b], np.tile(np.float32([-1, 0, 0, 0, 0]), (8, 1)))
    # +inf anywhere: no finite posterior either
    lp2 = np.zeros(N, np.float32)
    lp2[12345] = np.inf
    assert not prior_ref.posterior(lg[:1], lp2)["finite"][0]


def test_topk_on_the_posterior_is_topk_ref_on_its_heatmap():
    rng = np.random.default_rng(4)
    lg = rng.normal(0, 1, size=(1, N)).astype(np.float32)
    ori = _ori(1, N)
    lp = aerial.gaussian_log_prior([[200.0, 310.0]], 40.0, "cpu").numpy()
    tk = prior_ref.topk_rows(lg, ori, lp.reshape(1, N), 6, 8)
    h = prior_ref.posterior(lg, lp.reshape(1, N))["h"].astype(np.float32)
    np.testing.assert_array_equal(tk[0, :, 0], topk_ref.peak_indices(h.reshape(512, 512), 8, 6))


# ---- helpers -------------------------------------------------------------------------------------------------------------

def test_gaussian_log_prior_closed_form():
    lp = aerial.gaussian_log_prior([[10.0, 500.0], [255.5, 0.25]], [3.0, 100.0], "cpu")
    assert lp.shape == (2, 512, 512) and lp.dtype == torch.float32 and lp.is_contiguous()
    y, x = np.mgrid[0:512, 0:512].astype(np.float64)
    for b, (cx, cy, s) in enumerate(((10.0, 500.0, 3.0), (255.5, 0.25, 100.0))):
        want = (-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / s ** 2).astype(np.float32)
        np.testing.assert_array_equal(lp[b].numpy(), want)
    assert lp[0, 500, 10] == 0.0
    one = aerial.gaussian_log_prior((5.0, 6.0), 2.0, "cpu")
    assert one.shape == (1, 512, 512)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="sigma"):
            aerial.gaussian_log_prior([[1.0, 1.0]], bad, "cpu")


def test_oxford_log_prior_is_the_gaussian_at_each_pixels_map_position():
    origin = np.array([[800, 400], [1200, 400], [800, 800]])
    prior = np.array([1180.0, 705.5])   # inside window (800, 400) only
    sigma = 60.0
    lp = aerial.oxford_log_prior(origin, prior, sigma, "cpu")
    assert lp.shape == (3, 512, 512) and lp.dtype == torch.float32
    rng = np.random.default_rng(9)
    idx = np.concatenate([rng.integers(0, N, 3000), [0, N - 1, 255 * 512 + 255]])
    for p in range(3):
        pos = aerial.oxford_region_to_map(origin[p], idx)
        want = (-0.5 * ((pos[:, 0] - prior[0]) ** 2 + (pos[:, 1] - prior[1]) ** 2) / sigma ** 2).astype(np.float32)
        np.testing.assert_array_equal(lp[p].reshape(-1).numpy()[idx], want)
    # one scale across windows: the best pixel of every window sits near the prior, and the window that holds the prior wins
    best = [aerial.oxford_region_to_map(origin[p], int(lp[p].argmax())) for p in range(3)]
    assert np.abs(best[0] - prior).max() <= 2.5
    assert lp[0].max() > lp[1].max() and lp[0].max() > lp[2].max()
    # per-pair priors of different queries
    two = aerial.oxford_log_prior(origin[:2], [[1000.0, 600.0], [1500.0, 700.0]], [30.0, 90.0], "cpu")
    pos = aerial.oxford_region_to_map(origin[1], 4242)
    assert two[1].reshape(-1)[4242].item() == np.float32(-0.5 * ((pos[0] - 1500) ** 2 + (pos[1] - 700) ** 2) / 90.0 ** 2)
