"""The heading prior without a GPU: the four C entry points and their argument checks (all made before the handle is
used), the model methods' checks, the restatement of heading_predict (tests/heading_prior_ref.py) pinned to closed forms,
aerial.von_mises_heading_log_prior, the trackers' unchanged default path, and the edge cells of every field the GPU tests use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import heading_prior_ref as hp
from tests import heading_ref as hr

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_heading_prior_map", "ccvpe_localize_heading_prior", "ccvpe_localize_heading_prior_cached_indexed", "ccvpe_heading_predict")
BINS = (4, 20, 72, 360)


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    for name in ("heading_prior_map", "localize_heading_prior", "localize_heading_prior_cached", "heading_predict"):
        assert callable(getattr(models.CVM_OxfordRobotCar, name))
    assert callable(aerial.von_mises_heading_log_prior)


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def _callers(lib):
    bufs = [(C.c_float * 16)() for _ in range(9)]
    p, q, hd, hs, s, t, x, tb, om = (C.cast(b, C.c_void_p) for b in bufs)
    tidx = (C.c_int32 * 2)(0, 1)

    def full(prior=p, stride=0, table=tb, tstride=0, nb=72, radius=8, bins=72, rows=q, head=hd, hist=hs, summ=s, post=t, grd=x, sat=x):
        return lib.ccvpe_localize_heading_prior(None, grd, 154, 231, sat, 2, prior, stride, table, tstride, nb, radius, bins, rows, head,
                                                hist, summ, post, None)

    def cached(prior=p, stride=0, table=tb, tstride=0, nb=72, radius=8, bins=72, rows=q, head=hd, hist=hs, summ=s, post=t, grd=x,
               cache=x, index=tidx, n_tiles=2):
        return lib.ccvpe_localize_heading_prior_cached_indexed(None, grd, 154, 231, cache, n_tiles, index, 2, prior, stride, table,
                                                               tstride, nb, radius, bins, rows, head, hist, summ, post, None)

    def pmap(ori=x, batch=2, prior=p, stride=0, table=tb, tstride=0, nb=72, out=om):
        return lib.ccvpe_heading_prior_map(None, ori, batch, prior, stride, table, tstride, nb, out, None)

    def predict(hist=hs, batch=2, nb=72, turn=p, taps=q, tstride=0, radius=3, floor=s, out=om):
        return lib.ccvpe_heading_predict(None, hist, batch, nb, turn, taps, tstride, radius, floor, out, None)

    return {"full": full, "cached": cached, "map": pmap, "predict": predict}, (p, q, hd, hs, s, t, x, tb, om)


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    callers, (p, q, hd, hs, s, t, x, tb, om) = _callers(lib)
    for name in ("full", "cached", "map"):
        call = callers[name]
        assert call(table=None) == EINVAL and "table" in _msg(lib), (name, _msg(lib))
        for bad in (-1, 0, 3, 361, 100000):
            assert call(nb=bad) == EINVAL and "nb" in _msg(lib) and "nbins" not in _msg(lib), (name, bad, _msg(lib))
        for bad in (1, 72, 74, -73):
            assert call(tstride=bad) == EINVAL and "table_stride" in _msg(lib), (name, bad, _msg(lib))
        for bad in (1, N - 1, N + 1, -N):
            assert call(stride=bad) == EINVAL and "prior_stride" in _msg(lib), (name, bad, _msg(lib))
        for nb in (4, 72, 360):
            for tstride in (0, nb + 1):
                for stride in (0, N):
                    assert call(nb=nb, tstride=tstride, stride=stride) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
        assert call(prior=None, stride=7) == EINVAL and "handle" in _msg(lib), (name, _msg(lib))
    for name in ("full", "cached"):                     # then the checks of the matching heading form
        call = callers[name]
        for bad in (-1, 33):
            assert call(radius=bad) == EINVAL and "radius" in _msg(lib), (name, bad)
        for bad in (3, 361):
            assert call(bins=bad) == EINVAL and "nbins" in _msg(lib), (name, bad)
        assert call(rows=None) == EINVAL and "handle" not in _msg(lib), name
        assert call(head=None) == EINVAL and "heading" in _msg(lib), name
        assert call(hist=None) == EINVAL and "hist" in _msg(lib), name
        for kw in (dict(head=hs), dict(hist=q), dict(head=p), dict(summ=hd), dict(post=hs), dict(post=p), dict(summ=q)):
            assert call(**kw) == EINVAL and "alias" in _msg(lib), (name, kw, _msg(lib))
        for kw in (dict(table=q), dict(table=hd), dict(table=hs), dict(table=s), dict(table=t)):
            assert call(**kw) == EINVAL and "table" in _msg(lib) and "alias" in _msg(lib), (name, kw, _msg(lib))
        for kw in (dict(post=None), dict(summ=None), dict(summ=None, post=None), dict(prior=None, summ=None, post=None), dict(bins=20, nb=360)):
            assert call(**kw) == EINVAL and "handle" in _msg(lib), (name, kw, _msg(lib))
    for kw in ("grd", "sat"):
        assert callers["full"](**{kw: None}) == EINVAL and kw in _msg(lib)
    assert callers["cached"](cache=None) == EINVAL and "cache" in _msg(lib)
    assert callers["cached"](index=(C.c_int32 * 2)(0, 2)) == EINVAL and "tile_index[1] = 2" in _msg(lib)
    assert callers["cached"](index=None) == EINVAL and "handle" in _msg(lib)
    # the map alone
    pmap = callers["map"]
    assert pmap(ori=None) == EINVAL and "ori" in _msg(lib)
    assert pmap(out=None) == EINVAL and "out_map" in _msg(lib)
    for batch in (0, -1, 4097):
        assert pmap(batch=batch) == EINVAL and "batch" in _msg(lib)
    assert pmap(out=x) == EINVAL and "alias" in _msg(lib) and "ori" in _msg(lib)
    assert pmap(out=p) == EINVAL and "alias" in _msg(lib) and "log_prior" in _msg(lib)
    assert pmap(out=tb) == EINVAL and "alias" in _msg(lib)
    assert pmap(batch=4096) == EINVAL and "handle" in _msg(lib)
    # the predict step
    pred = callers["predict"]
    for kw, word in ((dict(hist=None), "hist"), (dict(turn=None), "turn_deg"), (dict(taps=None), "taps"), (dict(floor=None), "floor"),
                     (dict(out=None), "out")):
        assert pred(**kw) == EINVAL and word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    for bad in (3, 361, 0, -5):
        assert pred(nb=bad) == EINVAL and "nb" in _msg(lib), bad
    for bad in (-1, 33):
        assert pred(radius=bad, nb=360) == EINVAL and "radius" in _msg(lib), bad
    for nb, radius in ((4, 2), (72, 32 + 4), (64, 32), (6, 3)):
        assert pred(nb=nb, radius=radius) == EINVAL and "radius" in _msg(lib), (nb, radius, _msg(lib))
    for bad in (1, 3, 5, -4):
        assert pred(tstride=bad) == EINVAL and "taps_stride" in _msg(lib), bad
    for batch in (0, 4097):
        assert pred(batch=batch) == EINVAL and "batch" in _msg(lib)
    assert pred(out=hs) == EINVAL and "alias" in _msg(lib)
    for kw in (dict(), dict(tstride=4), dict(nb=4, radius=1), dict(nb=5, radius=2), dict(nb=65, radius=32), dict(nb=360, radius=0), dict(batch=4096)):
        assert pred(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))


# ---- model methods ---------------------------------------------------------------------------------------------------------

def test_model_methods_refuse_bad_arguments():
    m = models.CVM_OxfordRobotCar("cpu").eval()
    g, s = torch.zeros(3, 3, 154, 231), torch.zeros(3, 3, 512, 512)
    ori = torch.zeros(3, 2, 512, 512)
    tb = torch.zeros(73)
    for shape in ((4,), (362,), (2, 73), (3, 1, 73), ()):
        with pytest.raises(ValueError, match="heading_log_prior"):
            m.localize_heading_prior(g, s, torch.zeros(shape))
        with pytest.raises(ValueError, match="heading_log_prior"):
            m.localize_heading_prior_cached(g, torch.zeros(16), torch.zeros(shape))
        with pytest.raises(ValueError, match="heading_log_prior"):
            m.heading_prior_map(ori, torch.zeros(shape))
    for bad in (np.zeros(73, np.float32), torch.zeros(73, dtype=torch.float64), torch.zeros(3, 146)[:, ::2]):
        with pytest.raises(ValueError, match="heading_log_prior"):
            m.localize_heading_prior(g, s, bad)
    with pytest.raises(ValueError, match="cuda"):         # a well-formed table on the host
        m.localize_heading_prior(g, s, tb)
    with pytest.raises(ValueError, match="cuda"):
        m.heading_prior_map(ori, torch.zeros(3, 73))
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="radius"):
            m.localize_heading_prior(g, s, tb, radius=bad)
    for bad in (3, 361):
        with pytest.raises(ValueError, match="bins"):
            m.localize_heading_prior(g, s, tb, bins=bad)
        with pytest.raises(ValueError, match="bins"):
            m.localize_heading_prior_cached(g, torch.zeros(16), tb, bins=bad)
    with pytest.raises(ValueError, match="log_prior must be"):
        m.localize_heading_prior(g, s, tb, torch.zeros(2, 512, 512))
    with pytest.raises(ValueError, match="log_prior must be"):
        m.heading_prior_map(ori, tb, torch.zeros(512, 511))
    with pytest.raises(ValueError, match="ori"):
        m.heading_prior_map(torch.zeros(3, 2, 512, 511), tb)
    # heading_predict
    hist = torch.zeros(3, 72)
    taps = aerial.gaussian_taps(2.0, 6)
    for bad in (torch.zeros(72), torch.zeros(3, 3), torch.zeros(3, 361), torch.zeros(3, 72, dtype=torch.float64), torch.zeros(3, 144)[:, ::2]):
        with pytest.raises(ValueError, match="hist"):
            m.heading_predict(bad, 0.0, taps, 1e-3)
    with pytest.raises(ValueError, match="taps"):
        m.heading_predict(hist, 0.0, np.zeros((2, 7), np.float32), 1e-3)
    with pytest.raises(ValueError, match="radius"):
        m.heading_predict(hist, 0.0, np.zeros(34, np.float32), 1e-3)
    with pytest.raises(ValueError, match="radius"):
        m.heading_predict(torch.zeros(3, 4), 0.0, np.zeros(3, np.float32), 1e-3)       # 2 * 2 + 1 > 4
    with pytest.raises(ValueError, match="floor"):
        m.heading_predict(hist, 0.0, taps, -1.0)
    with pytest.raises(ValueError, match="turn_deg"):
        m.heading_predict(hist, [0.0, 1.0], taps, 1e-3)
    with pytest.raises(ValueError, match="cuda"):
        m.heading_predict(hist, 0.0, taps, 1e-3)
    m.train()
    for call in (lambda: m.localize_heading_prior(g, s, tb), lambda: m.heading_prior_map(ori, tb), lambda: m.heading_predict(hist, 0.0, taps, 1e-3)):
        with pytest.raises(RuntimeError, match="eval"):
            call()


# ---- the restatement of heading_predict against closed forms -----------------------------------------------------------------

def _hist(nb, seed=3):
    h = np.random.default_rng(seed).uniform(0.0, 1.0, size=(2, nb))
    return (h / h.sum(axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("nb", (4, 72, 360))
def test_predict_closed_forms(nb):
    h = _hist(nb)
    w = 360.0 / nb
    one = np.ones(1, np.float32)
    v = hp.predict(h, 0.0, one, 1e-3)                                             # turn 0, radius 0: log(hist + floor)
    np.testing.assert_allclose(v[:, :nb], h.astype(np.float64) + np.float64(np.float32(1e-3)), rtol=0, atol=0)
    np.testing.assert_allclose(v[:, nb], h.astype(np.float64).sum(axis=1) / nb + np.float64(np.float32(1e-3)), rtol=1e-15)
    for k in (1, -1, 3, nb, nb + 2, -2 * nb - 1):                                 # whole bins: a roll towards larger angles
        v = hp.predict(h, np.float32(k * w), one, 0.0)
        np.testing.assert_allclose(v[:, :nb], np.roll(h.astype(np.float64), k, axis=1), rtol=0, atol=1e-12)
    v = hp.predict(h, np.float32(0.5 * w), one, 0.0)                              # half a bin: the mean of the two neighbours
    np.testing.assert_allclose(v[:, :nb], 0.5 * (h + np.roll(h, 1, axis=1)).astype(np.float64), rtol=1e-6)
    r = min(3, (nb - 1) // 2)
    taps = aerial.gaussian_taps(1.5, r)
    for turn in (0.0, 0.3 * w, -7.7 * w, 725.0):                                  # the circle loses no mass, wrap included
        v = hp.predict(h, np.float32(turn), taps, 0.0)
        two_sided = float(taps[0]) + 2.0 * float(taps[1:].astype(np.float64).sum())
        np.testing.assert_allclose(v[:, :nb].sum(axis=1), h.astype(np.float64).sum(axis=1) * two_sided, rtol=1e-9)
        np.testing.assert_allclose(v[:, nb] * nb, v[:, :nb].sum(axis=1), rtol=1e-12)
    v = hp.predict(np.zeros((2, nb), np.float32), 12.3, taps, 1e-3)               # an all-zero hist: flat
    assert (v == np.float64(np.float32(1e-3))).all()
    v = hp.predict(h, np.array([np.nan, 0.0], np.float32), one, 1e-3)             # a NaN turn stays in its row
    assert np.isnan(v[0]).all() and np.isfinite(v[1]).all()


def test_predict_spike_moves_with_the_turn():
    h = np.zeros((1, 72), np.float32)
    h[0, 70] = 1.0
    v = hp.predict(h, np.float32(12.5), np.ones(1, np.float32), 0.0)[0]           # 2.5 bins on: bins 0 and 1 share the spike
    assert v[0] == pytest.approx(0.5) and v[1] == pytest.approx(0.5) and v[:72].sum() == pytest.approx(1.0)
    with np.errstate(divide="ignore"):
        got = np.log(v)
        hp.assert_predict(got[None, :].astype(np.float32), v[None, :], 0, "spike")
    bad = got.astype(np.float32).copy()
    bad[0] += 1e-5
    with pytest.raises(AssertionError, match="outside the bound"):
        hp.assert_predict(bad[None, :], v[None, :], 0, "spike")


# ---- aerial.von_mises_heading_log_prior -------------------------------------------------------------------------------------

def test_von_mises_heading_log_prior():
    for kappa in (0.0, 0.5, 8.0, 50.0):
        for mean in (1.0, 220.5, 359.9, -17.0):
            t = aerial.von_mises_heading_log_prior(mean, kappa, 72)
            assert t.dtype == np.float32 and t.shape == (73,)
            assert np.exp(t[:72].astype(np.float64)).sum() == pytest.approx(1.0, abs=1e-3)
            assert t[72] == np.float32(math.log(1.0 / 72))
            if kappa > 0:
                assert int(np.argmax(t[:72])) == int((mean % 360.0) // 5.0)
    t = aerial.von_mises_heading_log_prior(40.5, 8.0, 72)
    c = np.radians(aerial.heading_bin_centres(72))
    want = 8.0 * np.cos(c - np.radians(40.5)) - np.log(2.0 * np.pi * np.i0(8.0)) + np.log(2.0 * np.pi / 72)
    np.testing.assert_allclose(t[:72], want.astype(np.float32), rtol=1e-6)
    assert aerial.von_mises_heading_log_prior(10.0, 2.0, 20, none_log=-3.0)[20] == np.float32(-3.0)
    tb = aerial.von_mises_heading_log_prior([10.0, 200.2, 300.0], 4.0, 360)
    assert tb.shape == (3, 361) and int(np.argmax(tb[1, :360])) == 200
    np.testing.assert_array_equal(tb[2], aerial.von_mises_heading_log_prior(300.0, 4.0, 360))
    assert aerial.von_mises_heading_log_prior(10.0, [1.0, 2.0], 4).shape == (2, 5)
    assert np.isfinite(aerial.von_mises_heading_log_prior(10.0, 5000.0, 72)).all()
    for bad in (3, 361):
        with pytest.raises(ValueError, match="bins"):
            aerial.von_mises_heading_log_prior(0.0, 1.0, bad)
    with pytest.raises(ValueError, match="kappa"):
        aerial.von_mises_heading_log_prior(0.0, -1.0, 72)
    with pytest.raises(ValueError, match="mean_deg"):
        aerial.von_mises_heading_log_prior(float("nan"), 1.0, 72)
    with pytest.raises(ValueError, match="one per query"):
        aerial.von_mises_heading_log_prior([0.0, 1.0], [1.0, 2.0, 3.0], 72)


# ---- the trackers ------------------------------------------------------------------------------------------------------------

class _Fake:
    """records the model calls a tracker step makes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            B = a[0].shape[0]
            rows, post = torch.zeros(B, 5), torch.zeros(B, 512, 512)
            if name in ("track_predict", "track_predict_affine"):
                return post
            if name == "heading_predict":
                return torch.zeros(B, a[0].shape[1] + 1)
            if name.startswith("track_update"):
                return rows, post
            out = (rows,)
            if "heading" in name:
                out += (torch.zeros(B, 12), torch.zeros(B, k["bins"]))
            if "summary" in name or k.get("summary"):
                out += (torch.zeros(B, 16),)
            return out + (post,)
        return call


def test_trackers_with_default_arguments_take_the_old_path():
    g = torch.zeros(1, 3, 154, 231)
    taps = aerial.gaussian_taps(3.0, 9)
    for kw, update in ((dict(), "track_update_cached"), (dict(summary_radius=4), "localize_summary_cached"),
                       (dict(heading_bins=72), "localize_heading_cached"), (dict(heading_bins=72, summary_radius=4), "localize_heading_cached")):
        fake, tr = _Fake(), aerial.Tracker()
        for _ in range(3):
            tr.step(fake, g, None, [0], [[800, 400]], [0.0, 0.0], taps, 1e-7, **kw)
        assert fake.calls == [update, "track_predict", update, "track_predict", update] and tr.hist is None, (kw, fake.calls)
        fake, tr = _Fake(), aerial.AffineTracker()
        for _ in range(3):
            tr.step(fake, g, None, aerial.rigid_matrix(0.0, (0.0, 0.0)), taps, 1e-7, cache=torch.zeros(4), **kw)
        assert fake.calls == [update, "track_predict_affine", update, "track_predict_affine", update] and tr.hist is None, (kw, fake.calls)
    plain = {"track_update_cached": "track_update", "localize_summary_cached": "localize_summary", "localize_heading_cached": "localize_heading"}
    fake, tr = _Fake(), aerial.AffineTracker()
    tr.step(fake, g, torch.zeros(1, 3, 512, 512), None, taps, 1e-7, heading_bins=20)
    assert fake.calls == [plain["localize_heading_cached"]]


def test_trackers_filter_the_heading_when_asked():
    g = torch.zeros(1, 3, 154, 231)
    taps = aerial.gaussian_taps(3.0, 9)
    hk = dict(heading_bins=72, heading_turn_deg=0.0, heading_taps=aerial.gaussian_taps(2.0, 6), heading_floor=1e-3)
    fake, tr = _Fake(), aerial.Tracker()
    out = [tr.step(fake, g, None, [0], [[800, 400]], [0.0, 0.0], taps, 1e-7, **hk) for _ in range(3)]
    assert fake.calls == ["localize_heading_cached", "track_predict", "heading_predict", "localize_heading_prior_cached",
                          "track_predict", "heading_predict", "localize_heading_prior_cached"]
    assert all(len(o) == 3 for o in out) and tuple(tr.hist.shape) == (1, 72)
    tr.reset()
    assert tr.hist is None and tr.belief is None
    fake, tr = _Fake(), aerial.AffineTracker()
    for _ in range(2):
        tr.step(fake, g, torch.zeros(1, 3, 512, 512), aerial.rigid_matrix(0.0, (0.0, 0.0)), taps, 1e-7, summary_radius=2, **hk)
    assert fake.calls == ["localize_heading", "track_predict_affine", "heading_predict", "localize_heading_prior"]
    with pytest.raises(ValueError, match="heading_bins"):
        aerial.Tracker().step(fake, g, None, [0], [[800, 400]], [0.0, 0.0], taps, 1e-7, heading_turn_deg=0.0, heading_taps=taps, heading_floor=0.0)
    with pytest.raises(ValueError, match="go together"):
        aerial.Tracker().step(fake, g, None, [0], [[800, 400]], [0.0, 0.0], taps, 1e-7, heading_bins=72, heading_turn_deg=0.0)
    with pytest.raises(ValueError, match="go together"):
        aerial.AffineTracker().step(fake, g, None, None, taps, 1e-7, heading_bins=72, heading_floor=0.0, cache=torch.zeros(4))


# ---- edge cells of the fields the GPU tests use ---------------------------------------------------------------------------------

def test_edge_cells_stay_under_the_cap():
    fields = hr.crafted_fields()
    for name in ("constant", "two_mode", "smooth", "constant_wrap", "random", "special"):
        fld = hr.Field(fields[name])
        for nb in BINS:
            share = hp.edge_share(fld, nb)
            assert share <= hr.EDGE_CAP, (name, nb, share)
            if name in ("constant", "two_mode", "smooth", "constant_wrap"):   # angles at k + 0.5 degrees: interior points of every bin
                assert share == 0.0, (name, nb, share)
            else:                                                            # uniform angles: 2 * EDGE_DEG of every bin's width
                # ... plus, at the edges 0 and 180 that every bin count has, the cells whose float32 cosine rounds to +-1 (within
                # 2^-25: angles up to 0.0198 degrees either side, whose restated angle is exactly 0 or 180): at most 4 * 0.0198 / 360
                want = 2 * hr.EDGE_DEG * nb / 360.0
                sigma = math.sqrt(want / N)
                crafted = 40.0 / N if name == "special" else 0.0      # its 40 cells (0, s): exactly 90 or 270 degrees
                assert 0.9 * want - 4.0 * sigma <= share <= want + 4 * 0.0198 / 360.0 + crafted + 4.0 * sigma, (name, nb, share, want)
    # the restatement of the map: invalid cells take entry nb, a position prior is one float32 add, an edge cell names its neighbour
    fld = hr.Field(fields["special"])
    t = np.arange(73, dtype=np.float32)
    comb, alt, edge = hp.combined_map(fld, t, 72)
    assert (comb[~fld.valid] == 72).all() and (~fld.valid).sum() > 5000 and (comb[fld.valid] < 72).all()
    assert (np.abs(comb[edge] - alt[edge]) % 70 == 1).all() and (comb[~edge] == alt[~edge]).all()
    p = np.random.default_rng(1).normal(size=N).astype(np.float32)
    assert (hp.combined_map(fld, t, 72, p)[0] == p + comb).all()
    k, other, e = hp.cell_bins(hr.Field(hr.unit_field(89.9995)), 4)
    assert e.all() and (k == 0).all() and (other == 1).all()
    k, other, e = hp.cell_bins(hr.Field(hr.unit_field(0.0005)), 4)
    assert e.all() and (k == 0).all() and (other == 3).all()
