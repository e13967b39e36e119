"""Tracking a frame stream without a GPU: the four new C entry points and their argument checks (all made before the handle is used),
the model methods' checks, the numpy restatement tests/track_ref.py on crafted maps, the host helpers against closed forms, and the
crafted stream of the GPU filter test (it must have the property that test then asserts on the device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import track_ref

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_track_update", "ccvpe_track_update_cached_indexed", "ccvpe_track_update_logits", "ccvpe_track_predict")


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_track_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def _update_callers(lib):
    a, b = (C.c_float * 16)(), (C.c_float * 16)()
    p, q = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    tidx = (C.c_int32 * 2)(0, 1)

    def full(prior=p, stride=0, rows=p, post=q, grd=p, sat=p):
        return lib.ccvpe_track_update(None, grd, 154, 231, sat, 2, prior, stride, rows, post, None)

    def cached(prior=p, stride=0, rows=p, post=q, grd=p, cache=p, index=tidx, n_tiles=2):
        return lib.ccvpe_track_update_cached_indexed(None, grd, 154, 231, cache, n_tiles, index, 2, prior, stride, rows, post, None)

    def logits(prior=p, stride=0, rows=p, post=q, logits=p, ori=p, batch=2):
        return lib.ccvpe_track_update_logits(None, logits, ori, batch, prior, stride, rows, post, None)

    return {"full": full, "cached": cached, "logits": logits}, p, q


def test_update_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    callers, p, q = _update_callers(lib)
    for name, call in callers.items():
        for bad in (1, N - 1, N + 1, -N, 2 * N):
            assert call(stride=bad) == EINVAL and "prior_stride" in _msg(lib), (name, bad, _msg(lib))
        assert call(rows=None) == EINVAL and "handle" not in _msg(lib), name
        assert call(post=None) == EINVAL and "posterior" in _msg(lib), (name, _msg(lib))
        assert call(post=p) == EINVAL and "alias" in _msg(lib), (name, _msg(lib))     # posterior == log_prior
        # valid arguments all the way: the null handle is the first thing refused
        for stride in (0, N):
            assert call(stride=stride) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        # no prior: the stride is ignored
        for stride in (0, 7):
            assert call(prior=None, stride=stride) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
    for kw in ("grd", "sat"):
        assert callers["full"](**{kw: None}) == EINVAL and kw in _msg(lib)
    for kw in ("logits", "ori"):
        assert callers["logits"](**{kw: None}) == EINVAL and kw in _msg(lib)
    assert callers["logits"](prior=None, logits=q) == EINVAL and "alias" in _msg(lib)    # posterior == logits
    for batch in (0, 4097):
        assert callers["logits"](batch=batch) == EINVAL and "batch" in _msg(lib)
    assert callers["cached"](cache=None) == EINVAL and "cache" in _msg(lib)
    assert callers["cached"](index=(C.c_int32 * 2)(0, 2)) == EINVAL and "tile_index[1] = 2" in _msg(lib)
    assert callers["cached"](index=None) == EINVAL and "handle" in _msg(lib)
    assert callers["cached"](index=None, n_tiles=3) == EINVAL and "n_tiles 3 != batch 2" in _msg(lib)


def test_predict_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    a, b = (C.c_float * 16)(), (C.c_float * 16)()
    p, q = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)

    def call(belief=p, batch=2, shift=p, taps=p, stride=0, radius=3, floor=p, out=q):
        return lib.ccvpe_track_predict(None, belief, batch, shift, taps, stride, radius, floor, out, None)

    for kw, word in (("belief", "belief"), ("shift", "shift"), ("taps", "taps"), ("floor", "floor"), ("out", "log_prior")):
        assert call(**{kw: None}) == EINVAL and word in _msg(lib), (kw, _msg(lib))
    for r in (-1, 33, 1000):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for s in (1, 3, 5, -4):
        assert call(stride=s) == EINVAL and "taps_stride" in _msg(lib), (s, _msg(lib))
    for batch in (0, -1, 4097):
        assert call(batch=batch) == EINVAL and "batch" in _msg(lib), (batch, _msg(lib))
    assert call(out=p) == EINVAL and "alias" in _msg(lib)
    for r, s in ((0, 0), (0, 1), (3, 4), (32, 0), (32, 33)):
        assert call(radius=r, stride=s) == EINVAL and "handle" in _msg(lib), (r, s, _msg(lib))
    assert call(batch=4096) == EINVAL and "handle" in _msg(lib)


# ---- model methods ---------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_update_methods_refuse_bad_arguments():
    m = _model()
    g, s = torch.zeros(3, 3, 154, 231), torch.zeros(3, 3, 512, 512)
    lg, ori = torch.zeros(3, N), torch.zeros(3, 2, 512, 512)
    for shape in ((512, 511), (2, 512, 512), (3, 2, 512, 512), (N,), (3, N)):
        with pytest.raises(ValueError, match="log_prior must be"):
            m.track_update(g, s, torch.zeros(shape))
        with pytest.raises(ValueError, match="log_prior must be"):
            m.track_update_logits(lg, ori, torch.zeros(shape))
    with pytest.raises(ValueError, match="float32"):
        m.track_update(g, s, torch.zeros(3, 512, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        m.track_update(g, s, torch.zeros(512, 512).t())
    with pytest.raises(ValueError, match="cuda"):
        m.track_update(g, s, torch.zeros(3, 512, 512))
    with pytest.raises(RuntimeError, match="cuda"):      # no prior: the inputs are refused as forward refuses them
        m.track_update(g, s)
    with pytest.raises(ValueError, match="cuda"):
        m.track_update_cached(g, torch.zeros(16))
    with pytest.raises(ValueError, match="tile_index"):
        m.track_update_cached(g, torch.zeros(16), None, tile_index=[0, 1])
    with pytest.raises(ValueError, match="logits"):
        m.track_update_logits(torch.zeros(3, 100), ori)
    with pytest.raises(RuntimeError, match="cuda"):
        m.track_update_logits(lg, ori)
    with pytest.raises(ValueError, match="cuda"):
        m.track_update_logits(lg, ori, torch.zeros(512, 512))
    tr = _model().train()
    for call in (lambda: tr.track_update(g, s), lambda: tr.track_update_cached(g, s), lambda: tr.track_update_logits(lg, ori),
                 lambda: tr.track_predict(torch.zeros(1, 512, 512), [[0, 0]], [1.0], 0.0)):
        with pytest.raises(RuntimeError, match="eval"):
            call()


def test_predict_method_refuses_bad_arguments():
    m = _model()
    bel = torch.zeros(3, 512, 512)
    sh = np.zeros((3, 2))
    for bad in (torch.zeros(512, 512), torch.zeros(3, 512, 511), torch.zeros(3, 2, 512, 512), torch.zeros(3, N), np.zeros((3, 512, 512))):
        with pytest.raises(ValueError, match="belief must be"):
            m.track_predict(bad, sh, [1.0], 0.0)
    with pytest.raises(ValueError, match="belief must be float32"):
        m.track_predict(bel.double(), sh, [1.0], 0.0)
    with pytest.raises(ValueError, match="belief must be contiguous"):
        m.track_predict(bel.transpose(1, 2), sh, [1.0], 0.0)
    for bad in (np.zeros((2, 2)), np.zeros((3, 3)), np.zeros(6), [0.0, 0.0]):
        with pytest.raises(ValueError, match="shift_px"):
            m.track_predict(bel, bad, [1.0], 0.0)
    for bad in (np.zeros((2, 4)), np.zeros((3, 2, 2)), np.zeros(0), np.zeros(34), 1.0):
        with pytest.raises(ValueError, match="taps"):
            m.track_predict(bel, sh, bad, 0.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            m.track_predict(bel, sh, [1.0], bad)
    with pytest.raises(ValueError, match="floor"):
        m.track_predict(bel, sh, [1.0], np.zeros(2))
    # accepted shapes: the CPU belief is refused next
    for taps in ([1.0], np.ones((3, 5), np.float32) / 9, torch.ones(33) / 65):
        for floor in (0.0, 1e-9, np.full(3, 1e-6), torch.zeros(3)):
            with pytest.raises(ValueError, match="belief must be a cuda tensor"):
                m.track_predict(bel, sh, taps, floor)
    with pytest.raises(ValueError, match="belief must be a cuda tensor"):
        m.track_predict(bel.view(3, 1, 512, 512), torch.zeros(3, 2), [1.0], 0.0)


# ---- track_ref on crafted maps -------------------------------------------------------------------------------------------------
HW = 96   # the restatement takes the grid side as an argument; small maps keep these tests quick


def _delta(x, y, hw=HW):
    b = np.zeros((1, hw, hw), np.float32)
    b[0, y, x] = 1.0
    return b


def test_a_delta_moves_by_an_integer_shift_and_splits_on_a_half_pixel():
    c = track_ref.predict_c(_delta(40, 50), [[7.0, -3.0]], [1.0], HW)
    assert c[0, 47, 47] == 1.0 and c.sum() == 1.0                       # content moves by (+dx, +dy): x 40 -> 47, y 50 -> 47
    c = track_ref.predict_c(_delta(40, 50), [[0.5, 0.0]], [1.0], HW)
    assert c[0, 50, 40] == 0.5 and c[0, 50, 41] == 0.5 and c.sum() == 1.0
    c = track_ref.predict_c(_delta(40, 50), [[-2.25, 1.5]], [1.0], HW)    # x 37.75, y 51.5
    want = {(51, 37): 0.5 * 0.25, (51, 38): 0.5 * 0.75, (52, 37): 0.5 * 0.25, (52, 38): 0.5 * 0.75}
    for (y, x), v in want.items():
        assert c[0, y, x] == pytest.approx(v, rel=1e-15)
    assert np.count_nonzero(c) == 4
    # a fractional part of exactly 0 weighs the one source pixel with exactly 1, whatever the value
    b = np.random.default_rng(0).uniform(0, 1, size=(1, HW, HW)).astype(np.float32)
    c = track_ref.predict_c(b, [[3.0, 2.0]], [1.0], HW)
    np.testing.assert_array_equal(c[0, 2:, 3:], b[0, :-2, :-3].astype(np.float64))
    assert (c[0, :2] == 0).all() and (c[0, :, :3] == 0).all()


def test_blur_keeps_the_mass_of_a_centred_delta_and_loses_it_at_the_border():
    for sigma, r in ((2.0, 6), (0.7, 1), (10.0, 32)):
        t = aerial.gaussian_taps(sigma, r)
        c = track_ref.predict_c(_delta(48, 48), [[0.3, -0.6]], t, HW)
        z = float(t[0]) + 2.0 * float(t[1:].astype(np.float64).sum())
        assert c.sum() == pytest.approx(z * z, rel=1e-12) and abs(z - 1.0) < 1e-6
        assert c[0, 48, 48] == c.max() or c[0, 47, 48] == c.max()
    # a delta in the corner keeps a quarter plus the axes' share; one shifted out of the window leaves nothing
    t = aerial.gaussian_taps(2.0, 6).astype(np.float64)
    c = track_ref.predict_c(_delta(0, 0), [[0.0, 0.0]], t.astype(np.float32), HW)
    assert c.sum() == pytest.approx(t.sum() ** 2, rel=1e-12) and c.sum() < 0.5
    for shift in ([HW + 7.0, 0.0], [0.0, -(HW + 7.0)], [600.0, 600.0]):
        assert track_ref.predict_c(_delta(40, 50), [shift], t.astype(np.float32), HW).sum() == 0.0
    # mass just inside the reach of the blur comes back in: a delta 3 px outside the window
    c = track_ref.predict_c(_delta(2, 50), [[-5.0, 0.0]], t.astype(np.float32), HW)
    assert c[0, 50, 0] == pytest.approx(t[3] * t[0], rel=1e-12)


def test_floor_and_the_logarithm():
    b = _delta(10, 10)
    out = track_ref.predict(b, [[0.0, 0.0]], [1.0], 0.0, HW)
    assert out[0, 10, 10] == 0.0 and np.isneginf(np.delete(out.reshape(-1), 10 * HW + 10)).all()
    out = track_ref.predict(np.concatenate([b, b]), [[0.0, 0.0], [1.0, 0.0]], [1.0], [1e-9, 0.25], HW)
    f0, f1 = float(np.float32(1e-9)), 0.25
    assert out[0, 0, 0] == np.log(f0) and out[0, 10, 10] == np.log(1.0 + f0)
    assert out[1, 0, 0] == np.log(f1) and out[1, 10, 11] == np.log(1.25) and out[1, 10, 10] == np.log(f1)
    # per-query taps
    taps = np.float32([[1.0, 0.0], [0.5, 0.25]])
    c = track_ref.predict_c(np.concatenate([b, b]), np.zeros((2, 2)), taps, HW)
    assert c[0, 10, 10] == 1.0 and c[1, 10, 10] == 0.25 and c[1, 9, 11] == 0.0625


def test_update_restatement_is_prior_ref_plus_the_map():
    rng = np.random.default_rng(3)
    lg = rng.normal(0, 2, size=(3, N)).astype(np.float32)
    a = rng.uniform(-np.pi, np.pi, size=(3, N))
    ori = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    lp = np.zeros((3, N), np.float32)
    lp[1] = -np.inf
    lp[2, :1000] = -np.inf
    rows, margin, h = track_ref.update(lg, ori, lp)
    assert rows[1, 0] == -1 and np.isnan(rows[1, 1]) and (h[1] == 0).all()
    for b in (0, 2):
        assert h[b].sum() == pytest.approx(1.0) and int(rows[b, 0]) == int(np.argmax(h[b])) and rows[b, 1] == np.float32(h[b].max())
    assert (h[2, :1000] == 0).all() and rows[2, 0] >= 1000
    rows0, _, h0 = track_ref.update(lg[:1], ori[:1])
    np.testing.assert_array_equal(rows0[0], rows[0])
    np.testing.assert_array_equal(h0[0], h[0])


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def test_gaussian_taps_closed_form():
    for sigma, r in ((2.0, 6), (0.5, 3), (40.0, 32), (3.0, 0)):
        t = aerial.gaussian_taps(sigma, r)
        assert t.shape == (r + 1,) and t.dtype == np.float32
        i = np.arange(-r, r + 1, dtype=np.float64)
        w = np.exp(-0.5 * i ** 2 / sigma ** 2)
        np.testing.assert_array_equal(t, (w / w.sum())[r:].astype(np.float32))
        assert abs(float(t[0]) + 2.0 * t[1:].astype(np.float64).sum() - 1.0) <= (2 * r + 1) * 2.0 ** -25
    assert aerial.gaussian_taps(1.0, 0).tolist() == [1.0]
    two = aerial.gaussian_taps([1.0, 5.0], 4)
    assert two.shape == (2, 5)
    np.testing.assert_array_equal(two[1], aerial.gaussian_taps(5.0, 4))
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="sigma"):
            aerial.gaussian_taps(bad, 3)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="radius"):
            aerial.gaussian_taps(1.0, bad)


def test_oxford_track_shift_closed_form_and_region_to_map():
    sh = aerial.oxford_track_shift([800, 400], [1200, 400], [[10.0, 5.0], [0.0, 0.0]])
    np.testing.assert_allclose(sh, [[(-400 + 10) * 0.64, 5 * 0.64], [-256.0, 0.0]], rtol=1e-15)
    assert aerial.oxford_track_shift([800, 400], [800, 400], [0, 0]).tolist() == [[0.0, 0.0]]
    with pytest.raises(ValueError, match="finite"):
        aerial.oxford_track_shift([800, 400], [800, 400], [np.inf, 0])
    with pytest.raises(ValueError, match="rows"):
        aerial.oxford_track_shift(np.zeros((2, 2)), np.zeros((3, 2)), [0, 0])
    # a map point keeps its map position across a tile change: pixel (col, row) of the old window and the pixel it is moved to in the
    # new one name the same map position (oxford_region_to_map is exact to the 800/512 px grid and 2.5 px on the centre lines)
    prev, nxt = np.array([800, 400]), np.array([1200, 800])
    (dx, dy), = aerial.oxford_track_shift(prev, nxt, [0.0, 0.0])
    assert (dx, dy) == (-256.0, -256.0)
    rng = np.random.default_rng(5)
    for col, row in rng.integers(260, 500, size=(50, 2)):
        a = aerial.oxford_region_to_map(prev, int(row) * 512 + int(col))
        b = aerial.oxford_region_to_map(nxt, int(row + dy) * 512 + int(col + dx))
        assert np.abs(a - b).max() <= 2.5 + 800 / 512, (col, row, a, b)
    # with motion: the moved pixel names the moved map position
    motion = np.array([37.0, -21.0])
    (dx, dy), = aerial.oxford_track_shift(prev, prev, motion)
    a = aerial.oxford_region_to_map(prev, 300 * 512 + 200) + motion
    b = aerial.oxford_region_to_map(prev, int(round(300 + dy)) * 512 + int(round(200 + dx)))
    assert np.abs(a - b).max() <= 2.5 + 800 / 512


def test_tracker_checks_its_streams():
    t = aerial.Tracker()
    assert t.belief is None and t.origin is None
    with pytest.raises(ValueError, match="origins"):
        t.step(_model(), torch.zeros(2, 3, 154, 231), torch.zeros(16), None, [[800, 400]], [0, 0], [1.0], 0.0)


# ---- the crafted stream of the GPU filter test -----------------------------------------------------------------------------

def test_the_crafted_stream_fools_the_argmax_and_not_the_filter():
    """float64 restatement of the filter on the stream tests/track_ref builds: the per-frame argmax sits on the distractor in the frames
    where it is the larger peak, the tracked argmax stays within 2 px of the true peak in every frame after the first."""
    taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
    ori = np.zeros((1, 2, N), np.float32)
    ori[:, 0] = 1.0
    belief = None
    for k in range(track_ref.SEQ_FRAMES):
        lg = track_ref.sequence_logits(k)[None]
        plain = int(np.argmax(lg[0]))
        on_distractor = track_ref.pixel_distance(plain, track_ref.SEQ_DISTRACTOR) <= 1.0
        assert on_distractor == (k in track_ref.SEQ_STRONG), (k, plain)
        if not on_distractor:
            assert track_ref.pixel_distance(plain, track_ref.sequence_truth(k)) <= 1.0
        lp = None
        if belief is not None:
            lp = track_ref.predict(belief, [track_ref.SEQ_STEP], taps, track_ref.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        rows, _, h = track_ref.update(lg, ori, lp)
        if k >= 1:
            assert track_ref.pixel_distance(int(rows[0, 0]), track_ref.sequence_truth(k)) <= 2.0, (k, rows[0])
        belief = h.astype(np.float32).reshape(1, 512, 512)
