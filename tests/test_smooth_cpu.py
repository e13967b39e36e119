"""The smoother without a GPU: the C entry points and every refusal of ccvpe_track_smooth (all made before the handle
is used), the argument-check order of smooth.track_smooth, the float64 restatement tests/smooth_ref.py against a dense forward-backward
over all states of a small grid, the Z = sum s' identity, the three degenerate rules, what the smoother does to the crafted stream of
tests/track_ref.py when the filter starts on a frame the distractor wins, and RecordingTracker / smooth_stream against a fake model."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, smooth
from tests import smooth_ref, track_ref

EINVAL = -1
N = 512 * 512


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_track_smooth", "ccvpe_track_smooth_work_bytes"):
        assert hasattr(lib, n)
        assert n in {s for s, _, _ in _lib.SYMBOLS}
    assert smooth.SMOOTH_FIELDS == ("index", "prob", "evidence", "future")
    assert issubclass(smooth.RecordingTracker, aerial.Tracker)
    assert callable(smooth.track_smooth) and callable(smooth.smooth_stream)


def test_work_bytes_grow_with_the_batch_and_hold_the_g_map(built_library):
    lib = _lib.load()
    last = 0
    for batch in (1, 2, 3, 6, 32, 4096):
        got = lib.ccvpe_track_smooth_work_bytes(batch)
        assert got >= batch * 4 * N and got > last and got % 16 == 0, (batch, got)
        last = got
    assert lib.ccvpe_track_smooth_work_bytes(0) == 0 and lib.ccvpe_track_smooth_work_bytes(-3) == 0


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs = [(C.c_float * 64)() for _ in range(8)]                     # (ctypes arrays of this size are 16-byte aligned)
    bel, nxt, sh, tp, fl, out, st, wk = (C.cast(b, C.c_void_p) for b in bufs)
    assert all(C.addressof(b) % 16 == 0 for b in bufs)

    def call(belief=bel, nxt=nxt, batch=2, shift=sh, taps=tp, stride=0, radius=3, floor=fl, smoothed=out, stats=st, work=wk):
        return lib.ccvpe_track_smooth(None, belief, nxt, batch, shift, taps, stride, radius, floor, smoothed, stats, work, None)

    def msg():
        return (lib.ccvpe_last_error() or b"").decode()

    for kw, word in ((dict(belief=None), "belief"), (dict(nxt=None), "smoothed_next"), (dict(shift=None), "shift"), (dict(taps=None), "taps"),
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


# ---- smooth.track_smooth: the order of its checks ----------------------------------------------------------------------------------

_M = {}


def model(training=False):
    if training not in _M:
        m = models.CVM_OxfordRobotCar("cpu")
        _M[training] = m.train() if training else m.eval()
    return _M[training]


BEL, BEL_BAD = torch.zeros(2, 512, 512), torch.zeros(2, 512, 511)
TAPS, TAPS_BAD, TAPS_LONG = np.ones(4, np.float32), np.ones((3, 4), np.float32), np.ones(34, np.float32)
SHIFT, SHIFT_BAD = np.zeros((2, 2)), np.zeros((3, 2))
R, V = RuntimeError, ValueError

# (id, training, call, exception, message): every call but the last carries two faults of neighbouring check groups, and reports the first
CASES = [
    ("T>S", 1, lambda m: smooth.track_smooth(m, BEL_BAD, BEL, SHIFT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("S>next", 0, lambda m: smooth.track_smooth(m, BEL_BAD, BEL_BAD, SHIFT, TAPS, 0.0), V, r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next>taps", 0, lambda m: smooth.track_smooth(m, BEL, BEL_BAD, SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next(count)>taps", 0, lambda m: smooth.track_smooth(m, BEL, torch.zeros(3, 512, 512), SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next holds 3 maps, belief 2"),
    ("next(dtype)>taps", 0, lambda m: smooth.track_smooth(m, BEL, BEL.double(), SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next must be float32"),
    ("taps>floor", 0, lambda m: smooth.track_smooth(m, BEL, BEL, SHIFT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("radius>floor", 0, lambda m: smooth.track_smooth(m, BEL, BEL, SHIFT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("floor>shift", 0, lambda m: smooth.track_smooth(m, BEL, BEL, SHIFT_BAD, TAPS, -1.0), V, r"floor must be >= 0"),
    ("shift>D", 0, lambda m: smooth.track_smooth(m, BEL, BEL, SHIFT_BAD, TAPS, 0.0), V, r"shift_px must have shape \(2, 2\), got \(3, 2\)"),
    ("ends", 0, lambda m: smooth.track_smooth(m, BEL, BEL.clone(), SHIFT, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message):
        call(model(bool(training)))


# ---- the restatement against a dense forward-backward ------------------------------------------------------------------------------

HMM_HW, HMM_T = 12, 5
HMM_SHIFTS = np.float32([[1.3, -2.4], [2.0, -1.0], [-2.7, 0.6], [0.25, 2.9]])       # one integer shift; all inside (-3, 3)
HMM_TAPS = aerial.gaussian_taps(0.9, 2)
HMM_FLOOR = np.float32(1e-3)


@pytest.fixture(scope="module")
def hmm():
    """5 frames on a 12 x 12 grid: the dense filter and smoother, and the sweep of smooth_ref over the dense filter's beliefs"""
    n = HMM_HW * HMM_HW
    like = np.random.default_rng(5).uniform(0.05, 1.0, size=(HMM_T, n)) ** 4
    alpha, post = smooth_ref.dense_forward_backward(like, HMM_SHIFTS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
    sweep, stats = [None] * HMM_T, [None] * HMM_T
    sweep[-1] = alpha[-1].reshape(1, HMM_HW, HMM_HW)
    for t in range(HMM_T - 2, -1, -1):
        res = smooth_ref.smooth(alpha[t].reshape(1, HMM_HW, HMM_HW), sweep[t + 1], HMM_SHIFTS[t][None], HMM_TAPS, HMM_FLOOR, HMM_HW)
        sweep[t], stats[t] = res["s"], res["stats"][0]
    return alpha, post, sweep, stats


def test_restatement_is_the_dense_forward_backward(hmm):
    alpha, post, sweep, _ = hmm
    # mass does leave the window: a column of the transition without the floor sums to less than 1 somewhere
    u = smooth_ref.dense_kernel(HMM_SHIFTS[0], HMM_TAPS, HMM_HW)
    assert u.sum(axis=0).min() < 0.5 and u.sum(axis=0).max() > 0.99
    worst = 0.0
    for t in range(HMM_T):
        got, want = sweep[t].reshape(-1), post[t]
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
        assert abs(got.sum() - 1.0) <= 1e-12
    print(f"smooth_ref against the dense forward-backward: worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    # and smoothing does something here: the smoothed first frame is not the filtered one
    assert np.abs(post[0] / alpha[0] - 1.0).max() > 0.1


def test_evidence_is_the_mass_of_the_next_map(hmm):
    _, _, sweep, stats = hmm
    for t in range(HMM_T - 1):
        assert abs(stats[t][2] - sweep[t + 1].sum()) <= 1e-12, (t, stats[t][2])
        assert stats[t][3] > 0 and stats[t][0] == int(np.argmax(sweep[t]))
        assert stats[t][1] == sweep[t].reshape(-1)[int(stats[t][0])]


def test_degenerate_rules():
    hw = 12
    rng = np.random.default_rng(9)
    b = rng.uniform(0.0, 1.0, size=(hw, hw))
    b /= b.sum()
    nxt = rng.uniform(0.0, 1.0, size=(hw, hw))
    nxt /= nxt.sum()
    taps, sh = aerial.gaussian_taps(1.0, 2), np.float32([[0.5, -1.25]])

    def run(bb, nn, floor=1e-3, shift=sh):
        r = smooth_ref.smooth(bb[None], nn[None], shift, taps, floor, hw)
        return r["s"][0], r["stats"][0]

    clean, cs = run(b, nxt)
    assert cs[0] >= 0 and abs(clean.sum() - 1.0) < 1e-12
    # a NaN or a negative cell in the next map is not taken: the result is that of the map with zeros there
    holes = nxt.copy()
    holes[3, 4], holes[7, 7] = np.nan, -0.25
    zeros = nxt.copy()
    zeros[3, 4], zeros[7, 7] = 0.0, 0.0
    s1, st1 = run(b, holes)
    s2, st2 = run(b, zeros)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(st1, st2)
    # rule 1: a next map without a positive cell - zero, all NaN, negative - gives the belief back, its argmax, Z = NaN, G = 0
    tie = b.copy()
    tie[2, 3] = tie[9, 1] = b.max() * 2
    for nn in (np.zeros((hw, hw)), np.full((hw, hw), np.nan), -nxt):
        s, st = run(tie, nn)
        np.testing.assert_array_equal(s, tie)
        assert st[0] == 2 * hw + 3 and st[1] == tie[2, 3] and np.isnan(st[2]) and st[3] == 0
    # ... under the taken-value rule: NaN never wins, a map without a value above -inf has no argmax
    poisoned = tie.copy()
    poisoned[0, 0] = np.nan
    s, st = run(poisoned, np.zeros((hw, hw)))
    assert st[0] == 2 * hw + 3 and np.isnan(s[0, 0])
    s, st = run(np.full((hw, hw), np.nan), np.zeros((hw, hw)))
    assert st[0] == -1 and np.isnan(st[1]) and np.isnan(st[2]) and st[3] == 0
    # rule 2: a zero belief, a NaN in the belief, floor 0 with an excluded cell under a positive s' - a zero map and (-1, NaN, Z, G)
    s, st = run(np.zeros((hw, hw)), nxt)
    assert not s.any() and st[0] == -1 and np.isnan(st[1]) and st[2] == 0 and st[3] > 0
    s, st = run(poisoned, nxt)
    assert not s.any() and st[0] == -1 and np.isnan(st[1]) and np.isnan(st[2])
    corner = np.zeros((hw, hw))
    corner[0, 0] = 1.0                       # radius 2: the prior is zero beyond 3 cells of the corner, s' is positive there
    s, st = run(corner, nxt, floor=0.0, shift=np.float32([[0.0, 0.0]]))
    assert not s.any() and st[0] == -1 and np.isnan(st[1]) and not np.isfinite(st[2]) and st[3] == np.inf
    # ... while floor 0 with s' inside the prior's support is an ordinary query
    near = np.zeros((hw, hw))
    near[1, 1] = 1.0
    s, st = run(corner, near, floor=0.0, shift=np.float32([[0.0, 0.0]]))
    assert st[0] == 0 and s[0, 0] == 1.0 and st[2] == 1.0


# ---- the crafted stream, started on a frame the distractor wins --------------------------------------------------------------------

def test_smoother_moves_the_first_frame_off_the_distractor():
    """Frames 2 .. 11 of tests/track_ref's stream in float64.  Frame 2 is a SEQ_STRONG frame and the filter has no prior for it: its
    argmax is the distractor, 306 px from the truth.  Every later frame holds the true peak, and the backward sweep carries that
    back: the smoothed frame 2 peaks on the truth, and the distractor's best cell is below 1e-5 of the peak."""
    first = 2
    frames, beliefs, smoothed, evidence, _ = smooth_ref.crafted_stream(first)
    assert frames == list(range(2, 12)) and first in track_ref.SEQ_STRONG
    filt = int(np.argmax(beliefs[first]))
    assert track_ref.pixel_distance(filt, track_ref.sequence_truth(first)) > 300.0
    assert track_ref.pixel_distance(filt, track_ref.SEQ_DISTRACTOR) <= 1.0
    for k in frames:
        i = int(np.argmax(smoothed[k]))
        assert track_ref.pixel_distance(i, track_ref.sequence_truth(k)) <= 1.0, (k, i)
        if k in evidence:
            assert abs(evidence[k] - 1.0) <= 1e-9, (k, evidence[k])
    dx, dy = (int(v) for v in track_ref.SEQ_DISTRACTOR)
    s = smoothed[first]
    assert s[0, dy - 8:dy + 9, dx - 8:dx + 9].max() < 1e-5 * s.max()


# ---- RecordingTracker and smooth_stream against a fake model --------------------------------------------------------------------------

class _Fake:
    """records the model calls of a tracker step and of a sweep; every update returns a new map that names its frame"""

    training = False

    def __init__(self):
        self.calls, self.frames = [], 0

    def track_predict(self, belief, shift, taps, floor):
        self.calls.append(("track_predict", np.asarray(shift).copy(), taps, floor))
        return torch.zeros_like(belief)

    def track_update_cached(self, grd, cache, prior, tile_index=None):
        self.calls.append(("track_update_cached", prior is not None))
        self.frames += 1
        return torch.zeros(grd.shape[0], 5), torch.full((grd.shape[0], 512, 512), float(self.frames))


def test_recording_tracker_logs_what_the_sweep_needs(monkeypatch):
    g = torch.zeros(1, 3, 154, 231)
    taps = aerial.gaussian_taps(3.0, 9)
    origins = np.array([[800, 400], [1200, 400]])
    tiles, motion = [0, 0, 1, 1], np.array([61.0, -9.5])
    fake, tr, plain_fake, plain = _Fake(), smooth.RecordingTracker(), _Fake(), aerial.Tracker()
    for k, tile in enumerate(tiles):
        floor = 1e-7 * (k + 1)
        rows = tr.step(fake, g, None, [tile], origins, motion, taps, floor)
        want = plain.step(plain_fake, g, None, [tile], origins, motion, taps, floor)
        assert torch.equal(rows, want) and torch.equal(tr.belief, plain.belief) and tr.origin.tolist() == plain.origin.tolist()
    assert [c[0] for c in fake.calls] == [c[0] for c in plain_fake.calls]
    assert [c[0] for c in fake.calls] == ["track_update_cached"] + ["track_predict", "track_update_cached"] * 3
    assert len(tr.log) == 4 and tr.log[0][1] is None
    predicts = [c for c in fake.calls if c[0] == "track_predict"]
    for k in range(1, 4):
        belief, shift, tp, floor = tr.log[k]
        np.testing.assert_array_equal(shift, predicts[k - 1][1])           # the shift the step's own predict call was given
        np.testing.assert_array_equal(shift, aerial.oxford_track_shift(origins[tiles[k - 1]], origins[tiles[k]], motion))
        assert tp is taps and floor == 1e-7 * (k + 1) == predicts[k - 1][3]
        assert float(belief[0, 0, 0]) == k + 1                              # the map this frame's update returned, not a copy
    assert tr.log[3][0] is tr.belief
    with pytest.raises(TypeError):
        tr.step(fake, g, None, [0], origins, motion, taps)                  # the parent's signature: floor is required
    # keyword arguments of the parent pass through
    assert len(tr.step(_FakeSummary(), g, None, [1], origins, motion, taps, 1e-7, summary_radius=4)) == 2

    # the sweep: one call per frame, last frame first, entry t + 1's arguments for frame t, the running map handed on
    calls = []

    def fake_smooth(model, belief, nxt, shift, tp, floor, out=None):
        calls.append((float(belief[0, 0, 0]), float(nxt[0, 0, 0]), None if shift is None else np.asarray(shift).tolist(), floor, out is nxt if out is not None else None))
        res = out if out is not None else torch.empty_like(belief)
        res.copy_(belief + 0.5)
        return res, torch.full((1, 4), float(belief[0, 0, 0]))

    monkeypatch.setattr(smooth, "track_smooth", fake_smooth)
    log = tr.log[:4]
    for in_place in (False, True):
        calls.clear()
        maps, stats = smooth.smooth_stream(fake, log, in_place=in_place)
        assert len(maps) == 4 and tuple(stats.shape) == (4, 1, 4)
        assert [c[0] for c in calls] == [4.0, 3.0, 2.0, 1.0]
        assert calls[0][1] == 0.0 and calls[0][2] == [[0.0, 0.0]] and calls[0][3] == 0.0 and calls[0][4] is None     # the zero next map
        assert [c[1] for c in calls[1:]] == [4.0, 3.5, 2.5]
        assert [c[2] for c in calls[1:]] == [np.asarray(log[k][1]).tolist() for k in (3, 2, 1)]
        assert [c[3] for c in calls[1:]] == [log[k][3] for k in (3, 2, 1)]
        assert [c[4] for c in calls[1:]] == [True if in_place else None] * 3
        assert [float(m[0, 0, 0]) for m in maps] == [1.5, 2.5, 3.5, 4.0]
        assert stats[:, 0, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
        assert float(log[3][0][0, 0, 0]) == 4.0 and maps[3] is log[3][0]          # the log's beliefs are never written
    with pytest.raises(ValueError, match="empty"):
        smooth.smooth_stream(fake, [])
    with pytest.raises(ValueError, match="no shift"):
        smooth.smooth_stream(fake, [log[0], log[0]])
    tr.reset()
    assert tr.log == [] and tr.belief is None


class _FakeSummary(_Fake):
    def localize_summary_cached(self, grd, cache, prior, radius=0, posterior=False, tile_index=None):
        return torch.zeros(1, 5), torch.zeros(1, 16), torch.zeros(1, 512, 512)
