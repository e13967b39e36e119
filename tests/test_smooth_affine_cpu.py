"""The affine smoother without a GPU: the C entry points and every refusal of ccvpe_track_smooth_affine (all made
before the handle is used), the argument-check order of smooth.track_smooth_affine and its refusal of a host matrix beyond reach, the
float64 restatement tests/smooth_affine_ref.py against a dense forward-backward over all states of a small grid, the adjoint identity,
the restatement against tests/smooth_ref.py on integer translations, the degenerate rules, what the smoother does to the turning stream
of tests/track_affine_ref.py when the filter starts on a frame the distractor wins, and RecordingAffineTracker / smooth_stream_affine
against a fake model."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, smooth
from tests import smooth_affine_ref, smooth_ref, track_affine_ref, track_ref

EINVAL = -1
N = 512 * 512
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_track_smooth_affine", "ccvpe_track_smooth_affine_work_bytes"):
        assert hasattr(lib, n)
        assert n in {s for s, _, _ in _lib.SYMBOLS}
    assert issubclass(smooth.RecordingAffineTracker, aerial.AffineTracker)
    assert callable(smooth.track_smooth_affine) and callable(smooth.smooth_stream_affine) and callable(smooth.affine_reach)
    # the work buffer: ccvpe_track_smooth's, then h on the window plus the largest radius
    lib = _lib.load()
    last = 0
    for batch in (1, 2, 3, 6, 32, 4096):
        got = lib.ccvpe_track_smooth_affine_work_bytes(batch)
        assert got >= lib.ccvpe_track_smooth_work_bytes(batch) + batch * 4 * 576 * 576 and got > last and got % 16 == 0, (batch, got)
        last = got
    assert lib.ccvpe_track_smooth_affine_work_bytes(0) == 0 and lib.ccvpe_track_smooth_affine_work_bytes(-3) == 0


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs = [(C.c_float * 64)() for _ in range(8)]                     # (ctypes arrays of this size are 16-byte aligned)
    bel, nxt, mt, tp, fl, out, st, wk = (C.cast(b, C.c_void_p) for b in bufs)
    assert all(C.addressof(b) % 16 == 0 for b in bufs)

    def call(belief=bel, nxt=nxt, batch=2, matrix=mt, taps=tp, stride=0, radius=3, floor=fl, smoothed=out, stats=st, work=wk):
        return lib.ccvpe_track_smooth_affine(None, belief, nxt, batch, matrix, taps, stride, radius, floor, smoothed, stats, work, None)

    def msg():
        return (lib.ccvpe_last_error() or b"").decode()

    for kw, word in ((dict(belief=None), "belief"), (dict(nxt=None), "smoothed_next"), (dict(matrix=None), "matrix"), (dict(taps=None), "taps"),
                     (dict(floor=None), "floor"), (dict(smoothed=None), "smoothed"), (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**kw) == EINVAL and "null " + word in msg(), (kw, msg())
    for bad in (-1, 33, 1000):
        assert call(radius=bad) == EINVAL and "radius" in msg(), (bad, msg())
    for bad in (1, 3, 5, -4):
        assert call(stride=bad) == EINVAL and "taps_stride" in msg(), (bad, msg())
    for bad in (0, -1, 4097):
        assert call(batch=bad) == EINVAL and "batch" in msg(), (bad, msg())
    for kw in (dict(smoothed=bel), dict(smoothed=wk), dict(smoothed=st), dict(stats=bel), dict(stats=wk), dict(stats=out), dict(nxt=bel)):
        assert call(**kw) == EINVAL and "alias" in msg(), (kw, msg())
    for name in ("belief", "nxt", "smoothed", "work"):
        assert call(**{name: C.c_void_p(C.addressof(bufs[0]) + 64 + 4)}) == EINVAL and "aligned" in msg(), (name, msg())
    # what is allowed reaches the handle: the in-place form, every radius, both strides, the largest batch
    for kw in (dict(), dict(smoothed=nxt), dict(radius=0), dict(radius=32), dict(stride=4), dict(batch=4096), dict(batch=1)):
        assert call(**kw) == EINVAL and "null handle" in msg(), (kw, msg())


# ---- smooth.track_smooth_affine: the order of its checks, and the reach ------------------------------------------------------------

_M = {}


def model(training=False):
    if training not in _M:
        m = models.CVM_KITTI("cpu")
        _M[training] = m.train() if training else m.eval()
    return _M[training]


BEL, BEL_BAD = torch.zeros(2, 512, 512), torch.zeros(2, 512, 511)
TAPS, TAPS_BAD, TAPS_LONG = np.ones(4, np.float32), np.ones((3, 4), np.float32), np.ones(34, np.float32)
MAT, MAT_BAD, MAT_NAN = np.tile(IDENTITY, (2, 1)), np.tile(IDENTITY, (3, 1)), np.array([1.0, 0.0, np.nan, 0.0, 1.0, 0.0])
MAT_FAR = np.stack([IDENTITY, aerial.rigid_matrix(10.0, [3.0, -2.0], 1.0 / 0.3)])      # the linear part of query 1 has scale 0.3
R, V = RuntimeError, ValueError
sa = smooth.track_smooth_affine

# (id, training, call, exception, message): every call but the last carries two faults of neighbouring check groups, and reports the first
CASES = [
    ("T>S", 1, lambda m: sa(m, BEL_BAD, BEL, MAT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("S>next", 0, lambda m: sa(m, BEL_BAD, BEL_BAD, MAT, TAPS, 0.0), V, r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next>matrix", 0, lambda m: sa(m, BEL, BEL_BAD, MAT_BAD, TAPS, 0.0), V, r"smoothed_next must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next(count)>matrix", 0, lambda m: sa(m, BEL, torch.zeros(3, 512, 512), MAT_BAD, TAPS, 0.0), V, r"smoothed_next holds 3 maps, belief 2"),
    ("matrix(shape)>finite", 0, lambda m: sa(m, BEL, BEL, np.full((3, 6), np.nan), TAPS, 0.0), V, r"matrix must be \[6\] or \[2, 6\], got \(3, 6\)"),
    ("finite>reach", 0, lambda m: sa(m, BEL, BEL, MAT_NAN, TAPS_BAD, 0.0), V, r"matrix must be finite"),
    ("reach>taps", 0, lambda m: sa(m, BEL, BEL, MAT_FAR, TAPS_BAD, 0.0), V, r"matrix 1 is beyond the smoother's reach"),
    ("taps>floor", 0, lambda m: sa(m, BEL, BEL, MAT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("radius>floor", 0, lambda m: sa(m, BEL, BEL, MAT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("floor>D", 0, lambda m: sa(m, BEL, BEL, MAT, TAPS, -1.0), V, r"floor must be >= 0"),
    ("ends", 0, lambda m: sa(m, BEL, BEL.clone(), IDENTITY, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message):
        call(model(bool(training)))


def test_reach_of_a_host_matrix():
    # closed forms: the inverse of R^T / s is s R, so a turn by a at scale s (of the content) has hx = hy = s (|cos a| + |sin a|)
    for deg, s in ((0.0, 1.0), (37.5, 1.25), (45.0, 2.0), (90.0, 0.8), (-171.0, 1.0)):
        hx, hy = smooth.affine_reach(aerial.rigid_matrix(deg, [11.5, -3.25], s))
        want = s * (abs(np.cos(np.radians(deg))) + abs(np.sin(np.radians(deg))))
        assert abs(hx - want) <= 1e-12 and abs(hy - want) <= 1e-12, (deg, s, hx, hy)
        assert smooth_affine_ref.reach(aerial.rigid_matrix(deg, [11.5, -3.25], s)) == (True, hx, hy)
    hx, hy = smooth.affine_reach(np.stack([IDENTITY, [2.0, 0.0, 5.0, 1.0, 0.25, 0.0]]))       # a shear: N = [[0.5, 0], [-2, 4]]
    assert hx.tolist() == [1.0, 0.5] and hy.tolist() == [1.0, 6.0]
    with pytest.raises(ValueError, match="matrix must be"):
        smooth.affine_reach(np.zeros(5))
    # refused: a linear part of scale 0.3 at any angle, a singular matrix, a determinant that is zero in float32, the shear above;
    # accepted (the CPU belief is refused next): every rotation at scale 0.4715 of the linear part, scale 0.5
    bad = [aerial.rigid_matrix(0.0, [0.0, 0.0], 1.0 / 0.3), aerial.rigid_matrix(45.0, [0.0, 0.0], 1.0 / 0.3), [1.0, 2.0, 0.0, 2.0, 4.0, 0.0],
           [1e-30, 0.0, 0.0, 0.0, 1e-30, 0.0], [2.0, 0.0, 5.0, 1.0, 0.25, 0.0], aerial.rigid_matrix(45.0, [0.0, 0.0], 1.0 / 0.47)]
    for mat in bad:
        assert not smooth_affine_ref.reach(mat)[0]
        with pytest.raises(ValueError, match="beyond the smoother's reach"):
            sa(model(), BEL, BEL.clone(), mat, TAPS, 0.0)
    for mat in [aerial.rigid_matrix(d, [3.0, 4.0], 1.0 / 0.4715) for d in (0.0, 30.0, 45.0, 135.0)] + [aerial.rigid_matrix(45.0, [0.0, 0.0], 2.0), IDENTITY]:
        assert smooth_affine_ref.reach(mat)[0]
        with pytest.raises(ValueError, match="belief must be a cuda tensor"):
            sa(model(), BEL, BEL.clone(), mat, TAPS, 0.0)


# ---- the restatement against a dense forward-backward ------------------------------------------------------------------------------

HMM_HW, HMM_T = 12, 5
HMM_MATS = aerial.rigid_matrix([3.0, -5.0, 2.0, 7.0], [[1.3, -2.4], [2.0, -1.0], [-2.7, 0.6], [0.25, 2.9]], [0.9, 1.0, 0.9, 1.0 / 0.9],
                               centre=(5.5, 5.5))
HMM_TAPS = aerial.gaussian_taps(0.9, 2)
HMM_FLOOR = np.float32(1e-3)


@pytest.fixture(scope="module")
def hmm():
    """5 frames on a 12 x 12 grid: the dense filter and smoother, and the sweep of smooth_affine_ref over the dense filter's beliefs"""
    n = HMM_HW * HMM_HW
    like = np.random.default_rng(5).uniform(0.05, 1.0, size=(HMM_T, n)) ** 4
    alpha, post = smooth_affine_ref.dense_forward_backward(like, HMM_MATS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
    sweep, stats = [None] * HMM_T, [None] * HMM_T
    sweep[-1] = alpha[-1].reshape(1, HMM_HW, HMM_HW)
    for t in range(HMM_T - 2, -1, -1):
        res = smooth_affine_ref.smooth(alpha[t].reshape(1, HMM_HW, HMM_HW), sweep[t + 1], HMM_MATS[t], HMM_TAPS, HMM_FLOOR, HMM_HW)
        sweep[t], stats[t] = res["s"], res["stats"][0]
    return alpha, post, sweep, stats


def test_restatement_is_the_dense_forward_backward(hmm):
    alpha, post, sweep, stats = hmm
    # mass does leave the window, and the scale changes it: a column of the transition without the floor does not sum to 1
    u = smooth_affine_ref.dense_kernel(HMM_MATS[0], HMM_TAPS, HMM_HW)
    assert u.sum(axis=0).min() < 0.5 and u.sum(axis=0).max() > 0.99
    worst = 0.0
    for t in range(HMM_T):
        got, want = sweep[t].reshape(-1), post[t]
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
        assert abs(got.sum() - 1.0) <= 1e-12
    print(f"smooth_affine_ref against the dense forward-backward: worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    assert np.abs(post[0] / alpha[0] - 1.0).max() > 0.1
    # Z is the mass of the next map
    for t in range(HMM_T - 1):
        assert abs(stats[t][2] - sweep[t + 1].sum()) <= 1e-12, (t, stats[t][2])
        assert stats[t][3] > 0 and stats[t][0] == int(np.argmax(sweep[t]))


@pytest.mark.parametrize("hw,r", [(40, 0), (40, 3), (512, 6)])
def test_adjoint_identity(hw, r):
    """<Paff(b), g> = <b, A(blur(g))> for a 37.5 degree turn at scale 1.25, a shear and a quarter turn"""
    rng = np.random.default_rng(3)
    c = ((hw - 1) / 2.0,) * 2
    taps = aerial.gaussian_taps(1.2, r)
    for mat in (aerial.rigid_matrix(37.5, [3.3, -1.7], 1.25, centre=c), np.array([1.1, 0.3, -2.5, -0.2, 0.8, 4.25]),
                aerial.rigid_matrix(90.0, [0.0, 0.0], 1.0, centre=c)):
        b = rng.uniform(0.0, 1.0, size=(hw, hw)).astype(np.float32)
        g = rng.uniform(0.0, 1.0, size=(hw, hw))
        lhs = float((smooth_affine_ref.predict_c64(b, mat, taps, hw)[0] * g).sum())
        rhs = float((b.astype(np.float64) * smooth_affine_ref.adjoint(smooth_affine_ref.blur_ext(g, taps, hw), mat, hw)).sum())
        assert lhs > 0 and abs(lhs - rhs) <= 1e-12 * lhs, (hw, r, mat, lhs, rhs)


def test_restatement_is_smooth_ref_on_integer_translations():
    hw = 48
    rng = np.random.default_rng(17)
    b = rng.uniform(0.0, 1.0, size=(3, hw, hw)).astype(np.float32)
    nxt = rng.uniform(0.0, 1.0, size=(3, hw, hw)).astype(np.float32)
    shift = np.float32([[5.0, -3.0], [0.0, 0.0], [-17.0, 40.0]])
    mats = np.tile(IDENTITY, (3, 1))
    mats[:, 2], mats[:, 5] = -shift[:, 0], -shift[:, 1]
    for r in (0, 4):
        taps = aerial.gaussian_taps(1.5, r)
        got = smooth_affine_ref.smooth(b, nxt, mats, taps, 1e-4, hw)
        want = smooth_ref.smooth(b, nxt, shift, taps, 1e-4, hw)
        assert got["reach"].all()
        np.testing.assert_allclose(got["s"], want["s"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["stats"], want["stats"], rtol=1e-12, atol=0)


def test_degenerate_rules():
    hw = 12
    rng = np.random.default_rng(9)
    b = rng.uniform(0.0, 1.0, size=(hw, hw))
    b /= b.sum()
    nxt = rng.uniform(0.0, 1.0, size=(hw, hw))
    nxt /= nxt.sum()
    taps = aerial.gaussian_taps(1.0, 2)
    turn = aerial.rigid_matrix(8.0, [0.5, -1.25], 0.9, centre=(5.5, 5.5))

    def run(bb, nn, floor=1e-3, mat=turn):
        r = smooth_affine_ref.smooth(bb[None], nn[None], mat, taps, floor, hw)
        return r["s"][0], r["stats"][0]

    clean, cs = run(b, nxt)
    assert cs[0] >= 0 and abs(clean.sum() - 1.0) < 1e-12
    tie = b.copy()
    tie[2, 3] = tie[9, 1] = b.max() * 2

    def rule1(s, st, bb):
        np.testing.assert_array_equal(s, bb)
        assert st[0] == 2 * hw + 3 and st[1] == bb[2, 3] and np.isnan(st[2]) and st[3] == 0

    # rule 1: a zero next map
    rule1(*run(tie, np.zeros((hw, hw))), tie)
    # ... and a link beyond reach: det = 0 (the predict's prior is flat there), a linear part of scale 0.3, a NaN in the linear part
    for mat in ([1.0, 2.0, 0.0, 2.0, 4.0, 0.0], [0.0] * 6, aerial.rigid_matrix(8.0, [0.5, -1.25], 1.0 / 0.3, centre=(5.5, 5.5)),
                [np.nan, 0.0, 0.0, 0.0, 1.0, 0.0]):
        rule1(*run(tie, nxt, mat=np.array(mat)), tie)
    # rule 2: a zero belief, a NaN in the belief - a zero map and (-1, NaN, Z, G)
    s, st = run(np.zeros((hw, hw)), nxt)
    assert not s.any() and st[0] == -1 and np.isnan(st[1]) and st[2] == 0 and st[3] > 0
    poisoned = b.copy()
    poisoned[4, 4] = np.nan
    s, st = run(poisoned, nxt)
    assert not s.any() and st[0] == -1 and np.isnan(st[1]) and np.isnan(st[2])
    # a NaN or a negative cell in the next map is not taken
    holes, zeros = nxt.copy(), nxt.copy()
    holes[3, 4], holes[7, 7] = np.nan, -0.25
    zeros[3, 4], zeros[7, 7] = 0.0, 0.0
    s1, st1 = run(b, holes)
    s2, st2 = run(b, zeros)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(st1, st2)


# ---- the turning stream, started on a frame the distractor wins ------------------------------------------------------------------------

@pytest.mark.parametrize("first", [2, 5])
def test_smoother_moves_the_first_frame_off_the_distractor(first):
    """Frames first .. 11 of tests/track_affine_ref's turning stream in float64.  The first frame is a SEQ_STRONG frame and the filter has
    no prior for it: its argmax is the distractor, more than 250 px from the truth (observed 294 px at frame 2, 283 px at frame 5).
    Every later frame holds the true peak and the backward sweep carries that back through the turning grids: the smoothed argmax is
    within 1 px of the truth in every frame (observed at most 0.56 px), and the distractor's best cell is below 1e-5 of the peak in
    every frame (observed at most 2.7e-7)."""
    ref = track_affine_ref
    frames, beliefs, smoothed, evidence, _ = smooth_affine_ref.crafted_stream(first)
    assert frames == list(range(first, ref.SEQ_FRAMES)) and first in ref.SEQ_STRONG
    filt = int(np.argmax(beliefs[first]))
    far = track_ref.pixel_distance(filt, ref.sequence_truth(first))
    assert far > 250.0 and track_ref.pixel_distance(filt, ref.SEQ_DISTRACTOR) <= 1.0
    dx, dy = (int(v) for v in ref.SEQ_DISTRACTOR)
    worst_d, worst_r = 0.0, 0.0
    for k in frames:
        i = int(np.argmax(smoothed[k]))
        d = track_ref.pixel_distance(i, ref.sequence_truth(k))
        s = smoothed[k][0]
        ratio = float(s[dy - 8:dy + 9, dx - 8:dx + 9].max() / s.max())
        worst_d, worst_r = max(worst_d, d), max(worst_r, ratio)
        assert d <= 1.0, (k, i, d)
        assert ratio < 1e-5, (k, ratio)
        if k in evidence:
            assert abs(evidence[k] - 1.0) <= 1e-8, (k, evidence[k])
    print(f"start at frame {first}: filter {far:.0f} px off, smoother at most {worst_d:.2f} px, distractor at most {worst_r:.1e} of the peak")


# ---- RecordingAffineTracker and smooth_stream_affine against a fake model -----------------------------------------------------------------

class _Fake:
    """records the model calls of a tracker step; every update returns a new map that names its frame"""

    training = False

    def __init__(self):
        self.calls, self.frames = [], 0

    def track_predict_affine(self, belief, matrix, taps, floor):
        self.calls.append(("track_predict_affine", np.asarray(matrix).copy(), taps, floor))
        return torch.zeros_like(belief)

    def track_update(self, grd, sat, prior):
        self.calls.append(("track_update", prior is not None))
        self.frames += 1
        return torch.zeros(grd.shape[0], 5), torch.full((grd.shape[0], 512, 512), float(self.frames))

    def localize_summary(self, grd, sat, prior, radius=0, posterior=False):
        return torch.zeros(1, 5), torch.zeros(1, 16), torch.zeros(1, 512, 512)


def test_recording_tracker_logs_what_the_sweep_needs(monkeypatch):
    g, s = torch.zeros(1, 3, 256, 1024), torch.zeros(1, 3, 512, 512)
    taps = aerial.gaussian_taps(3.0, 9)
    mats = [aerial.rigid_matrix(4.0 * k, [2.0 * k, -1.5], 1.0) for k in range(4)]
    fake, tr, plain_fake, plain = _Fake(), smooth.RecordingAffineTracker(), _Fake(), aerial.AffineTracker()
    for k in range(4):
        floor = 1e-7 * (k + 1)
        rows = tr.step(fake, g, s, mats[k], taps, floor)
        want = plain.step(plain_fake, g, s, mats[k], taps, floor)
        assert torch.equal(rows, want) and torch.equal(tr.belief, plain.belief)
    assert [c[0] for c in fake.calls] == [c[0] for c in plain_fake.calls]
    assert [c[0] for c in fake.calls] == ["track_update"] + ["track_predict_affine", "track_update"] * 3
    assert len(tr.log) == 4 and tr.log[0][1] is None
    predicts = [c for c in fake.calls if c[0] == "track_predict_affine"]
    for k in range(1, 4):
        belief, matrix, tp, floor = tr.log[k]
        np.testing.assert_array_equal(matrix, predicts[k - 1][1])           # the matrix the step's own predict call was given
        np.testing.assert_array_equal(matrix, mats[k])
        assert matrix is not mats[k] and matrix.dtype == np.float64         # a copy: the caller may reuse its array
        assert tp is taps and floor == 1e-7 * (k + 1) == predicts[k - 1][3]
        assert float(belief[0, 0, 0]) == k + 1                              # the map this frame's update returned, not a copy
    assert tr.log[3][0] is tr.belief
    with pytest.raises(TypeError):
        tr.step(fake, g, s, mats[0], taps)                                  # the parent's signature: floor is required
    with pytest.raises(ValueError, match="sat or as cache"):
        tr.step(fake, g, None, mats[0], taps, 1e-7)                         # the parent's refusals, and nothing logged
    assert len(tr.log) == 4
    # keyword arguments of the parent pass through
    assert len(tr.step(fake, g, s, mats[1], taps, 1e-7, summary_radius=4)) == 2

    # the sweep: one call per frame, last frame first, entry t + 1's arguments for frame t, the running map handed on
    calls = []

    def fake_smooth(model, belief, nxt, matrix, tp, floor, out=None):
        calls.append((float(belief[0, 0, 0]), float(nxt[0, 0, 0]), np.asarray(matrix).tolist(), floor, out is nxt if out is not None else None))
        res = out if out is not None else torch.empty_like(belief)
        res.copy_(belief + 0.5)
        return res, torch.full((1, 4), float(belief[0, 0, 0]))

    def no_call(*a, **kw):
        raise AssertionError("the affine sweep goes through track_smooth_affine")

    monkeypatch.setattr(smooth, "track_smooth_affine", fake_smooth)
    monkeypatch.setattr(smooth, "track_smooth", no_call)
    log = tr.log[:4]
    for in_place in (False, True):
        calls.clear()
        maps, stats = smooth.smooth_stream_affine(fake, log, in_place=in_place)
        assert len(maps) == 4 and tuple(stats.shape) == (4, 1, 4)
        assert [c[0] for c in calls] == [4.0, 3.0, 2.0, 1.0]
        assert calls[0][1] == 0.0 and calls[0][2] == IDENTITY.tolist() and calls[0][3] == 0.0 and calls[0][4] is None   # the zero next map
        assert [c[1] for c in calls[1:]] == [4.0, 3.5, 2.5]
        assert [c[2] for c in calls[1:]] == [mats[k].tolist() for k in (3, 2, 1)]
        assert [c[3] for c in calls[1:]] == [log[k][3] for k in (3, 2, 1)]
        assert [c[4] for c in calls[1:]] == [True if in_place else None] * 3
        assert [float(m[0, 0, 0]) for m in maps] == [1.5, 2.5, 3.5, 4.0]
        assert stats[:, 0, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
        assert float(log[3][0][0, 0, 0]) == 4.0 and maps[3] is log[3][0]          # the log's beliefs are never written
    with pytest.raises(ValueError, match="empty"):
        smooth.smooth_stream_affine(fake, [])
    with pytest.raises(ValueError, match="no matrix"):
        smooth.smooth_stream_affine(fake, [log[0], log[0]])
    tr.reset()
    assert tr.log == [] and tr.belief is None and tr.hist is None
