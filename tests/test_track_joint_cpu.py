"""The joint position-heading filter without a GPU: the entry points are exported and refuse bad arguments before
they use the handle; the float64 restatement tests/joint_ref.py does what the definition says on hand cases; the host helpers
(aerial.heading_emission, aerial.joint_shift_table) have their closed forms; the two model methods check their arguments without a
device; aerial.JointTracker is forward + predict + update, against a stub model; and the restatement alone separates the two peaks
of the crafted stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import joint_ref as jr
from tests import track_ref

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_track_joint_work_bytes", "ccvpe_track_joint_predict", "ccvpe_track_joint_update_logits")


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


# ---- C entry points ------------------------------------------------------------------------------------------------------------

def test_joint_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}


def test_work_bytes_is_host_arithmetic(built_library):
    lib = _lib.load()
    assert lib.ccvpe_track_joint_work_bytes(1, 4) == 4 * N * 4
    assert lib.ccvpe_track_joint_work_bytes(32, 36) == 32 * 36 * N * 4
    assert lib.ccvpe_track_joint_work_bytes(455, 72) == 455 * 72 * N * 4         # 32760 maps: past 2^32 bytes
    for batch, nb in ((0, 8), (-1, 8), (1, 3), (1, 73), (456, 72), (8193, 4)):
        assert lib.ccvpe_track_joint_work_bytes(batch, nb) == 0, (batch, nb)


def _buffers(count):
    keep = [(C.c_float * 32)() for _ in range(count)]
    return keep, [C.cast(a, C.c_void_p) for a in keep]


def test_predict_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    keep, (p, q, w) = _buffers(3)

    def call(joint=p, batch=2, nb=8, shift=p, taps=p, stride=0, radius=3, turn=p, htaps=p, hstride=0, rh=1, floor=p, work=w, prior=q):
        return lib.ccvpe_track_joint_predict(None, joint, batch, nb, shift, taps, stride, radius, turn, htaps, hstride, rh, floor, work,
                                             prior, None)

    for kw, word in (("joint", "joint"), ("shift", "shift"), ("taps", "taps"), ("turn", "turn_deg"), ("htaps", "htaps"), ("floor", "floor"),
                     ("work", "work"), ("prior", "prior")):
        assert call(**{kw: None}) == EINVAL and word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    for nb in (3, 0, -1, 73, 360):
        assert call(nb=nb, rh=0) == EINVAL and "nb" in _msg(lib), (nb, _msg(lib))
    for batch, nb in ((0, 8), (-1, 8), (4097, 8), (8193, 4), (456, 72)):
        assert call(batch=batch, nb=nb) == EINVAL and "batch" in _msg(lib), (batch, nb, _msg(lib))
    for r in (-1, 33):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for s in (1, 3, 5, -4):
        assert call(stride=s) == EINVAL and "taps_stride" in _msg(lib), (s, _msg(lib))
    for nb, rh in ((8, -1), (8, 4), (4, 2), (72, 33), (6, 3)):
        assert call(nb=nb, rh=rh) == EINVAL and "hradius" in _msg(lib), (nb, rh, _msg(lib))
    for s in (1, 3, -2):
        assert call(hstride=s) == EINVAL and "htaps_stride" in _msg(lib), (s, _msg(lib))
    for kw in (dict(prior=p), dict(prior=w), dict(work=p)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    assert call(joint=C.c_void_p(p.value + 4)) == EINVAL and "aligned" in _msg(lib)
    # valid arguments all the way: the null handle is the first thing refused
    for kw in (dict(), dict(nb=4, rh=1), dict(nb=6, rh=2), dict(nb=72, rh=32, hstride=33), dict(radius=0, stride=1), dict(radius=32, stride=33),
               dict(batch=4096, nb=8), dict(batch=455, nb=72, rh=0, hstride=1)):
        assert call(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))


def test_update_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    keep, (lg, ori, pr, em, rows, jo, mg, hs) = _buffers(8)

    def call(logits=lg, ori=ori, batch=2, prior=pr, emission=em, stride=0, nb=8, rows=rows, joint_out=jo, marginal=mg, hist=hs):
        return lib.ccvpe_track_joint_update_logits(None, logits, ori, batch, prior, emission, stride, nb, rows, joint_out, marginal, hist, None)

    for kw in ("logits", "ori", "emission", "rows", "joint_out", "marginal", "hist"):
        assert call(**{kw: None}) == EINVAL and kw in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    for nb in (3, 73, -8):
        assert call(nb=nb) == EINVAL and "nb" in _msg(lib), (nb, _msg(lib))
    for batch, nb in ((0, 8), (4097, 8), (456, 72)):
        assert call(batch=batch, nb=nb) == EINVAL and "batch" in _msg(lib), (batch, nb, _msg(lib))
    for s in (1, 8, 10, -9):
        assert call(stride=s) == EINVAL and "emission_stride" in _msg(lib), (s, _msg(lib))
    for kw in (dict(joint_out=lg), dict(marginal=ori), dict(hist=em), dict(rows=lg), dict(marginal=pr), dict(hist=pr), dict(rows=pr),
               dict(marginal=jo), dict(hist=rows), dict(rows=mg)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    assert call(marginal=C.c_void_p(mg.value + 8)) == EINVAL and "aligned" in _msg(lib)
    for kw in (dict(), dict(prior=None), dict(joint_out=pr), dict(stride=9), dict(nb=4, stride=5), dict(nb=72, stride=73, batch=455)):
        assert call(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))


# ---- the restatement on hand cases ---------------------------------------------------------------------------------------------------

def _delta_joint(nb, k, x, y):
    j = np.zeros((1, nb, 512, 512), np.float32)
    j[0, k, y, x] = 1.0
    return j


def test_a_delta_moves_to_exactly_one_bin_and_cell():
    nb = 6
    shift = np.zeros((1, nb, 2), np.float32)
    shift[0, 2] = (7, -3)                                # the source bin's own shift moves it ...
    shift[0, 3] = (100, 100)                             # ... and no other bin's
    out = jr.predict(_delta_joint(nb, 2, 40, 50), shift, [1.0], 120.0, [1.0], 0.0)       # 120 degrees = 2 bins of 60
    assert out[0, 4, 47, 47] == 1.0 and out.sum() == 1.0
    out = jr.predict(_delta_joint(nb, 5, 40, 50), np.zeros((1, nb, 2)), [1.0], 60.0, [1.0], 0.0)     # across the wrap
    assert out[0, 0, 50, 40] == 1.0 and out.sum() == 1.0
    out = jr.predict(_delta_joint(nb, 0, 40, 50), np.zeros((1, nb, 2)), [1.0], -90.0, [1.0], 0.0)    # 1.5 bins back: bins 4 and 5
    np.testing.assert_allclose(out[0, :, 50, 40], [0, 0, 0, 0, 0.5, 0.5])
    out = jr.predict(_delta_joint(nb, 1, 40, 50), np.zeros((1, nb, 2)), [1.0], 0.0, [1.0], 0.25)     # the floor, everywhere
    assert out[0, 1, 50, 40] == 1.25 and out[0, 0, 0, 0] == 0.25 and out.shape == (1, nb, 512, 512)


def test_blur_keeps_the_mass_away_from_the_border():
    nb = 8
    j = np.zeros((1, nb, 512, 512), np.float32)
    j[0, 1, 200, 300], j[0, 6, 255, 256], j[0, 7, 100, 90] = 0.5, 0.25, 0.125
    shift = np.random.default_rng(3).uniform(-20, 20, size=(1, nb, 2)).astype(np.float32)
    taps = np.array([0.4, 0.2, 0.05], np.float32)
    th = np.array([0.5, 0.2, 0.1], np.float32)
    out = jr.predict(j, shift, taps, 77.7, th, 0.0)
    st = float(taps[0]) + 2.0 * float(taps[1]) + 2.0 * float(taps[2])
    sh = float(th[0]) + 2.0 * float(th[1]) + 2.0 * float(th[2])
    np.testing.assert_allclose(out.sum(), 0.875 * st * st * sh, rtol=1e-12)
    lost = jr.predict(j, np.full((1, nb, 2), 600.0), taps, 0.0, th, 0.0)              # beyond the grid: the mass leaves
    assert lost.sum() == 0.0


def test_the_emission_wraps_on_the_circle_and_invalid_cells_take_the_last_entry():
    nb = 4
    lg = np.zeros((1, N), np.float32)
    ori = np.zeros((1, 2, N), np.float32)
    ori[0, 0, :] = np.cos(np.radians(315.0))             # bin 3 of 4 ...
    ori[0, 1, :] = np.sin(np.radians(315.0))
    ori[0, :, 0] = 0.0                                   # ... one cell without a heading, one with NaN
    ori[0, 0, 1] = np.nan
    e = np.array([0.5, 0.25, 0.0, 0.125, 2.0], np.float32)
    r = jr.update(lg, ori, e, nb)
    Z = (N - 2) * 0.875 + 2 * 4 * 2.0
    np.testing.assert_allclose(r["Z"][0], Z)
    # e[j] weighs bin own + j: bin 3 + 1 wraps to bin 0
    np.testing.assert_allclose(r["joint"][0, :, 5] * Z, [0.25, 0.0, 0.125, 0.5])
    np.testing.assert_allclose(r["joint"][0, :, 0] * Z, [2.0] * 4)
    np.testing.assert_allclose(r["joint"][0, :, 1] * Z, [2.0] * 4)
    np.testing.assert_allclose(r["hist"][0].sum(), 1.0)
    np.testing.assert_allclose(r["marginal"][0].sum(), 1.0)
    assert r["rows"][0, 0] == 0 and r["rows"][0, 2] == 0 and r["rows"][0, 3] == 0.0
    # a prior on one bin alone picks that bin
    pr = np.zeros((1, nb, N), np.float32)
    pr[0, 2] = 1.0
    r = jr.update(lg, ori, e, nb, pr)
    assert r["hist"][0, 2] == pytest.approx(1.0) and r["hist"][0, [0, 1, 3]].sum() == 0.0


def test_queries_without_a_finite_posterior_in_the_restatement():
    nb = 4
    lg = np.zeros((3, N), np.float32)
    lg[1, 77] = np.nan
    ori = np.ones((3, 2, N), np.float32)
    pr = np.ones((3, nb, N), np.float32)
    pr[2] = 0.0
    r = jr.update(lg, ori, np.full(nb + 1, 0.25, np.float32), nb, pr)
    assert r["finite"].tolist() == [True, False, False]
    assert np.isnan(r["Z"][1]) and r["Z"][2] == 0.0 and r["m"][1] == 0.0
    for b in (1, 2):
        assert r["rows"][b, 0] == -1 and np.isnan(r["rows"][b, 1]) and r["rows"][b, 2] == -1
        assert not r["joint"][b].any() and not r["marginal"][b].any() and not r["hist"][b].any()


# ---- host helpers ----------------------------------------------------------------------------------------------------------------

def test_heading_emission_closed_form():
    e = aerial.heading_emission(2.0, 8)
    assert e.shape == (9,) and e.dtype == np.float32
    k = np.exp(2.0 * np.cos(np.arange(8) * np.pi / 4))
    np.testing.assert_allclose(e[:8], k / k.sum(), rtol=1e-6)
    assert e[8] == np.float32(1 / 8) and abs(float(e[:8].sum()) - 1.0) < 1e-6
    np.testing.assert_array_equal(e[1:4], e[7:4:-1])                 # symmetric on the circle
    np.testing.assert_allclose(aerial.heading_emission(0.0, 6), np.full(7, 1 / 6), rtol=1e-7)
    per = aerial.heading_emission([0.0, 5.0, 700.0], 36, none=0.0)
    assert per.shape == (3, 37) and (per[:, 36] == 0).all() and np.isfinite(per).all()
    np.testing.assert_allclose(per[:, :36].sum(axis=1), 1.0, rtol=1e-6)
    assert per[2, 0] > 0.99
    for bad in (3, 73):
        with pytest.raises(ValueError, match="bins"):
            aerial.heading_emission(1.0, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kappa"):
            aerial.heading_emission(bad, 8)
    with pytest.raises(ValueError, match="none"):
        aerial.heading_emission(1.0, 8, none=-0.5)


def test_joint_shift_table_closed_form():
    t = aerial.joint_shift_table(10.0, 0.0, 4)                       # centres 45, 135, 225, 315: counter-clockwise from the x axis, y down
    assert t.shape == (1, 4, 2)
    h = 10.0 / np.sqrt(2.0)
    np.testing.assert_allclose(t[0], [[h, -h], [-h, -h], [-h, h], [h, h]], atol=1e-12)
    # KITTI's labels (zero_deg 0, counter-clockwise): 90 is up on the tile; left of up is -x
    t = aerial.joint_shift_table([2.0, 0.0], [0.0, 3.0], 72)
    k = int(90 // 5)                                                 # bin 18 = [90, 95), centre 92.5
    a = np.radians(92.5)
    np.testing.assert_allclose(t[0, k], [2 * np.cos(a), -2 * np.sin(a)], atol=1e-12)
    np.testing.assert_allclose(t[1, k], [-3 * np.sin(a), -3 * np.cos(a)], atol=1e-12)
    assert t.shape == (2, 72, 2) and t[0, k, 1] < -1.99 and t[1, k, 0] < -2.99
    # Oxford's labels (0 = north = up, clockwise): label 90 is east = +x; its left is north = up
    t = aerial.joint_shift_table(4.0, 1.0, 8, zero_deg=90.0, clockwise=True, common_px=[[100.0, -50.0]])
    a = np.radians(90.0 - 112.5)                                     # bin 2 = [90, 135), centre 112.5
    np.testing.assert_allclose(t[0, 2], [100 + 4 * np.cos(a) - np.sin(a), -50 - 4 * np.sin(a) - np.cos(a)], atol=1e-12)
    assert t[0, 2, 0] > 103 and t[0, 0, 1] < -53                     # label 22.5: mostly north
    np.testing.assert_allclose(np.hypot(*(t[0] - [100.0, -50.0]).T), np.hypot(4.0, 1.0))
    for kw, word in ((dict(bins=3), "bins"), (dict(bins=73), "bins"), (dict(forward_px=[1.0, 2.0], left_px=[1.0, 2.0, 3.0]), "forward_px must hold 1 or 3 rows"),
                     (dict(forward_px=float("nan")), "forward_px"), (dict(common_px=np.zeros((2, 2)), forward_px=np.zeros(3)), "common_px"),
                     (dict(zero_deg=float("inf")), "zero_deg")):
        args = dict(forward_px=1.0, left_px=0.0, bins=8)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            aerial.joint_shift_table(**args)
    assert len(aerial.JOINT_FIELDS) == 5


# ---- model methods -----------------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_predict_method_refuses_bad_arguments():
    m = _model()
    nb = 6
    jt = torch.zeros(2, nb, 512, 512)
    sh = np.zeros((2, nb, 2))
    ok = dict(shift_px=sh, taps=[1.0], floor=0.0, turn_deg=0.0, heading_taps=[1.0])

    def call(joint=jt, **kw):
        a = dict(ok)
        a.update(kw)
        return m.track_joint_predict(joint, a["shift_px"], a["taps"], a["floor"], a["turn_deg"], a["heading_taps"], out=a.get("out"))

    for bad in (torch.zeros(512, 512), torch.zeros(2, 512, 512), torch.zeros(2, nb, 512, 511), np.zeros((2, nb, 512, 512)),
                torch.zeros(2, 3, 512, 512), torch.zeros(1, 73, 1, 1).expand(1, 73, 512, 512)):
        with pytest.raises(ValueError, match="joint must"):
            call(bad)
    with pytest.raises(ValueError, match="joint must be float32"):
        call(jt.double())
    with pytest.raises(ValueError, match="joint must be contiguous"):
        call(jt.transpose(2, 3))
    for bad in (np.zeros((2, 2)), np.zeros((2, nb + 1, 2)), np.zeros((1, nb, 2)), np.zeros((2, nb, 3))):
        with pytest.raises(ValueError, match="shift_px"):
            call(shift_px=bad)
    for bad in (np.zeros((3, 4)), np.zeros(0), np.zeros(34), 1.0):
        with pytest.raises(ValueError, match="taps"):
            call(taps=bad)
    for bad in (np.zeros((3, 2)), np.zeros(0), np.zeros(4), np.zeros(34), 1.0):              # 4 taps: 2 * 3 + 1 > 6 bins
        with pytest.raises(ValueError, match="heading_taps"):
            call(heading_taps=bad)
    for bad in (-1.0, float("nan"), np.zeros(3)):
        with pytest.raises(ValueError, match="floor"):
            call(floor=bad)
    with pytest.raises(ValueError, match="turn_deg"):
        call(turn_deg=np.zeros(3))
    for bad in (torch.zeros(2, nb + 1, 512, 512), torch.zeros(1, nb, 512, 512), torch.zeros(2, nb, 512, 512, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must"):
            call(out=bad)
    with pytest.raises(ValueError, match="out must not be the joint"):
        call(out=jt)
    # accepted forms: the CPU joint is refused next
    for kw in (dict(), dict(taps=np.ones((2, 5), np.float32) / 9, heading_taps=torch.tensor([[0.5, 0.2, 0.05]] * 2), floor=np.full(2, 1e-6),
                            turn_deg=torch.tensor([3.0, -400.0])), dict(out=torch.zeros(2, nb, 512, 512), shift_px=torch.zeros(2, nb, 2))):
        with pytest.raises(ValueError, match="joint must be a cuda tensor"):
            call(**kw)
    with pytest.raises(RuntimeError, match="eval"):
        _model().train().track_joint_predict(jt, sh, [1.0], 0.0, 0.0, [1.0])


def test_update_method_refuses_bad_arguments():
    m = _model()
    nb = 4
    lg, ori = torch.zeros(2, N), torch.zeros(2, 2, 512, 512)
    em = np.full(nb + 1, 0.25, np.float32)
    with pytest.raises(ValueError, match="logits"):
        m.track_joint_update_logits(torch.zeros(2, 100), ori, em)
    for bad in (np.zeros((3, nb + 1)), np.zeros((2, 2, nb + 1)), 0.5):
        with pytest.raises(ValueError, match="emission must be"):
            m.track_joint_update_logits(lg, ori, bad)
    for bad in (np.zeros(4), np.zeros(74), np.zeros((2, 3))):
        with pytest.raises(ValueError, match="nb in 4..72"):
            m.track_joint_update_logits(lg, ori, bad)
    for bad in ([0.25, 0.25, -0.1, 0.25, 0.0], [0.25, float("nan"), 0.1, 0.25, 0.0]):
        with pytest.raises(ValueError, match="non-negative"):
            m.track_joint_update_logits(lg, ori, bad)
    for what in ("prior", "out"):
        for bad in (torch.zeros(2, nb + 1, 512, 512), torch.zeros(2, 512, 512), torch.zeros(3, nb, 512, 512), np.zeros((2, nb, 512, 512)),
                    torch.zeros(2, nb, 512, 512, dtype=torch.float16), torch.zeros(2, nb, 512, 512).transpose(2, 3)):
            with pytest.raises(ValueError, match=what + " must"):
                m.track_joint_update_logits(lg, ori, em, **{what: bad})
    # accepted forms: the CPU inputs are refused next
    for kw in (dict(), dict(prior=torch.zeros(2, nb, 512, 512)), dict(out=torch.zeros(2, nb, 512, 512))):
        for e in (em, np.tile(em, (2, 1)), torch.from_numpy(em), list(em)):
            with pytest.raises(RuntimeError, match="cuda"):
                m.track_joint_update_logits(lg, ori, e, **kw)
    with pytest.raises(RuntimeError, match="eval"):
        _model().train().track_joint_update_logits(lg, ori, em)


# ---- aerial.JointTracker against a stub model --------------------------------------------------------------------------------------

class _Stub:
    """records the calls a tracker step makes and returns tensors of the right shapes"""

    def __init__(self, nb):
        self.nb, self.calls = nb, []

    def forward_cached(self, grd, cache, tile_index=None):
        self.calls.append(("forward_cached", tile_index))
        B = grd.shape[0]
        return (torch.zeros(B, N), torch.zeros(B, 1, 512, 512), torch.ones(B, 2, 512, 512))

    def forward(self, grd, sat):
        self.calls.append(("forward",))
        B = grd.shape[0]
        return (torch.zeros(B, N), torch.zeros(B, 1, 512, 512), torch.ones(B, 2, 512, 512))

    def track_joint_predict(self, joint, shift_px, taps, floor, turn_deg, heading_taps, out=None):
        self.calls.append(("predict", joint, np.array(shift_px), taps, floor, turn_deg, heading_taps))
        return torch.full_like(joint, 2.0)

    def track_joint_update_logits(self, logits, ori, emission, prior=None, out=None):
        self.calls.append(("update", prior, out))
        B = logits.shape[0]
        joint = out if out is not None else torch.zeros(B, self.nb, 512, 512)
        return torch.zeros(B, 5), joint, torch.full((B, 512, 512), 1.0 / N), torch.zeros(B, self.nb)

    def belief_summary(self, belief, radius):
        self.calls.append(("summary", belief, radius))
        return torch.zeros(belief.shape[0], 16)

    def belief_credible(self, belief, levels):
        self.calls.append(("credible", belief, levels))
        return torch.zeros(belief.shape[0], 4 + 3 * len(levels))


def test_joint_tracker_is_forward_predict_update():
    nb = 8
    st = _Stub(nb)
    tr = aerial.JointTracker()
    em = aerial.heading_emission(2.0, nb)
    taps, ht = aerial.gaussian_taps(2.0, 6), [0.8, 0.1]
    g = torch.zeros(2, 3, 154, 231)
    origins = np.array([[800, 400], [1200, 400]])
    kw = dict(cache=torch.zeros(4), origins=origins, zero_deg=90.0, clockwise=True)
    res = tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, tile_index=[0, 0], **kw)
    assert len(res) == 3 and res[0].shape == (2, 5) and res[1].shape == (2, 512, 512) and res[2].shape == (2, nb)
    assert [c[0] for c in st.calls] == ["forward_cached", "update"] and st.calls[1][1] is None      # the first step has no prior
    assert tr.joint.shape == (2, nb, 512, 512) and tr.origin.tolist() == [[800, 400], [800, 400]]
    st.calls.clear()
    held = tr.joint
    res = tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, tile_index=[0, 1], summary_radius=8, credible_levels=[0.5, 0.9], **kw)
    assert [c[0] for c in st.calls] == ["forward_cached", "predict", "update", "summary", "credible"]
    pred = st.calls[1]
    assert pred[1] is held and pred[2].shape == (2, nb, 2) and pred[5] == 3.0
    common = aerial.oxford_track_shift(origins[[0, 0]], origins[[0, 1]], np.zeros(2))
    np.testing.assert_allclose(common, [[0.0, 0.0], [-400 * 0.64, 0.0]])
    np.testing.assert_allclose(pred[2], aerial.joint_shift_table(5.0, 0.5, nb, 90.0, True, common))
    assert st.calls[2][1] is st.calls[2][2] and bool((st.calls[2][1] == 2.0).all())           # the update runs in place on the prior
    assert tr.joint is st.calls[2][1] and tr.origin.tolist() == [[800, 400], [1200, 400]]
    assert len(res) == 5 and res[3].shape == (2, 16) and res[4].shape == (2, 10)
    assert st.calls[3][1] is res[1] and st.calls[4][1] is res[1]                                # ... of the marginal
    with pytest.raises(ValueError, match="streams"):
        tr.step(st, torch.zeros(3, 3, 154, 231), em, 5.0, 0.5, 3.0, taps, ht, 1e-9, cache=torch.zeros(4), origins=origins[[0, 0, 0]])
    with pytest.raises(ValueError, match="bins"):
        tr.step(st, g, aerial.heading_emission(2.0, 6), 5.0, 0.5, 3.0, taps, ht, 1e-9, tile_index=[0, 1], **kw)
    with pytest.raises(ValueError, match="origins"):
        tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, cache=torch.zeros(4))
    with pytest.raises(ValueError, match="one of the two"):
        tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9)
    with pytest.raises(ValueError, match="tile_index"):
        tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(2, 3, 512, 512), tile_index=[0, 1])
    tr.reset()
    assert tr.joint is None and tr.origin is None
    st.calls.clear()
    tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(2, 3, 512, 512))           # one grid for every frame, images
    tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(2, 3, 512, 512))
    assert [c[0] for c in st.calls] == ["forward", "update", "forward", "predict", "update"]
    np.testing.assert_allclose(st.calls[3][2], np.broadcast_to(aerial.joint_shift_table(5.0, 0.5, nb), (2, nb, 2)))


# ---- the crafted stream: the restatement alone ---------------------------------------------------------------------------------------

def test_the_restatement_separates_the_two_peaks_and_the_position_filter_does_not():
    """Two equal peaks, the field saying heading 0 degrees at both; A moves by the table's shift for that bin, B the opposite way.  The
    float64 joint filter ends with 0.999989 of the marginal within 8 px of A; the float64 position filter fed zero shift keeps 0.4999 at
    each."""
    nb = jr.SEQ_BINS
    table = aerial.joint_shift_table(jr.SEQ_FORWARD, 0.0, nb)
    step = jr.sequence_step(table)
    em = aerial.heading_emission(jr.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jr.SEQ_SIGMA, jr.SEQ_RADIUS)
    ori = np.zeros((1, 2, N), np.float32)
    ori[:, 0] = 1.0
    joint, bel = None, None
    for k in range(jr.SEQ_FRAMES):
        lg = jr.sequence_logits(k, step)[None]
        prior = None
        if joint is not None:
            prior = jr.predict(joint, table, taps, 0.0, jr.SEQ_HTAPS, jr.SEQ_FLOOR).astype(np.float32).reshape(1, nb, N)
        r = jr.update(lg, ori, em, nb, prior)
        joint = r["joint"].astype(np.float32).reshape(1, nb, 512, 512)
        lp = None if bel is None else track_ref.predict(bel, np.zeros((1, 2)), taps, jr.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        bel = track_ref.update(lg, ori, lp)[2].astype(np.float32).reshape(1, 512, 512)
    a, b = jr.sequence_peaks(jr.SEQ_FRAMES - 1, step)
    assert jr.mass_near(r["marginal"], a) > 0.999 and jr.mass_near(r["marginal"], b) < 1e-4
    assert int(r["rows"][0, 2]) == 0 and r["hist"][0, 0] > 0.9
    assert jr.mass_near(bel, a) > 0.45 and jr.mass_near(bel, b) > 0.45
