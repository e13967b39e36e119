"""The joint smoother without a GPU: the entry points are exported and refuse bad arguments before they use the
handle; smooth.track_joint_smooth checks its arguments in track_joint_predict's order; the float64 restatement
tests/joint_smooth_ref.py is the textbook forward-backward recursion of a dense HMM over (bin, cell), has Z = sum s' and follows
the three degenerate rules; on the crafted two-peak stream the smoothed frame 0 has decided where the filter could not; and
smooth.RecordingJointTracker / smooth.smooth_joint_stream do what they say against a stub model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, smooth
from tests import joint_ref as jr
from tests import joint_smooth_ref as jsr
from tests import smooth_ref as sr

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_track_joint_smooth_work_bytes", "ccvpe_track_joint_smooth")


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


# ---- C entry points ------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    assert smooth.JOINT_SMOOTH_FIELDS == ("index", "prob", "bin", "evidence", "future")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ccvpe.h")) as fh:
        assert "#define CCVPE_JOINT_SMOOTH_COLS 5" in fh.read()


def test_work_bytes_is_host_arithmetic(built_library):
    lib = _lib.load()
    partial = 8 * (1024 + 72 * 256 + 72 * 64 + 2) + 4 * 128          # the sums of g, of w, of s per bin, (Z, G); the chunks' pairs
    assert lib.ccvpe_track_joint_smooth_work_bytes(1, 4) == 4 * N * 4 + partial
    assert lib.ccvpe_track_joint_smooth_work_bytes(8, 36) == 8 * (36 * N * 4 + partial)
    assert lib.ccvpe_track_joint_smooth_work_bytes(455, 72) == 455 * (72 * N * 4 + partial)         # past 2^32 bytes
    for batch, nb in ((0, 8), (-1, 8), (1, 3), (1, 73), (456, 72), (8193, 4)):
        assert lib.ccvpe_track_joint_smooth_work_bytes(batch, nb) == 0, (batch, nb)


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    keep = [(C.c_float * 32)() for _ in range(13)]
    jt, nx, sh, tp, tn, ht, fl, wk, sm, mg, hs, st, spare = [C.cast(a, C.c_void_p) for a in keep]

    def call(joint=jt, nxt=nx, batch=2, nb=8, shift=sh, taps=tp, stride=0, radius=3, turn=tn, htaps=ht, hstride=0, rh=1, floor=fl, work=wk,
             smoothed=sm, marginal=mg, hist=hs, stats=st):
        return lib.ccvpe_track_joint_smooth(None, joint, nxt, batch, nb, shift, taps, stride, radius, turn, htaps, hstride, rh, floor, work,
                                            smoothed, marginal, hist, stats, None)

    for kw, word in (("joint", "joint"), ("nxt", "smoothed_next"), ("shift", "shift"), ("taps", "taps"), ("turn", "turn_deg"), ("htaps", "htaps"),
                     ("floor", "floor"), ("work", "work"), ("smoothed", "smoothed"), ("marginal", "marginal"), ("hist", "hist"), ("stats", "stats")):
        assert call(**{kw: None}) == EINVAL and "null " + word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
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
    # every overlap of an output with an input, with work or with another output - smoothed == smoothed_next alone is allowed
    outs = ("smoothed", "marginal", "hist", "stats")
    for o in outs:
        for other in (jt, sh, tp, tn, ht, fl, wk):
            assert call(**{o: other}) == EINVAL and "alias" in _msg(lib), (o, _msg(lib))
        if o != "smoothed":
            assert call(**{o: nx}) == EINVAL and "alias" in _msg(lib), (o, _msg(lib))
        for o2 in outs:
            if o2 != o:
                assert call(**{o: dict(smoothed=sm, marginal=mg, hist=hs, stats=st)[o2]}) == EINVAL and "alias" in _msg(lib), (o, o2, _msg(lib))
    for kw in (dict(nxt=jt), dict(work=jt), dict(work=nx), dict(joint=wk)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    for kw in ("joint", "nxt", "work", "smoothed", "marginal"):
        assert call(**{kw: C.c_void_p(spare.value + 4)}) == EINVAL and "aligned" in _msg(lib), kw
    # valid arguments all the way: the null handle is the first thing refused
    for kw in (dict(), dict(smoothed=nx), dict(nb=4, rh=1), dict(nb=5, rh=2), dict(nb=72, rh=32, hstride=33), dict(radius=0, stride=1),
               dict(radius=32, stride=33), dict(batch=4096, nb=8), dict(batch=455, nb=72, rh=0, hstride=1)):
        assert call(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))


# ---- the method's checks, without a device ---------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_track_joint_smooth_checks_in_the_order_of_the_predict():
    m = _model()
    nb = 6
    jt, nx = torch.zeros(2, nb, 512, 512), torch.zeros(2, nb, 512, 512)
    ok = dict(shift_px=np.zeros((2, nb, 2)), taps=[1.0], floor=0.0, turn_deg=0.0, heading_taps=[1.0])

    def call(joint=jt, nxt=nx, **kw):
        a = dict(ok)
        a.update(kw)
        return smooth.track_joint_smooth(m, joint, nxt, a["shift_px"], a["taps"], a["floor"], a["turn_deg"], a["heading_taps"], out=a.get("out"))

    for bad in (torch.zeros(512, 512), torch.zeros(2, nb, 512, 511), np.zeros((2, nb, 512, 512)), torch.zeros(2, 3, 512, 512)):
        with pytest.raises(ValueError, match="joint must"):
            call(bad)
    for bad in (torch.zeros(2, nb + 1, 512, 512), torch.zeros(1, nb, 512, 512), torch.zeros(2, nb, 512, 512, dtype=torch.float64),
                torch.zeros(2, nb, 512, 512).transpose(2, 3), np.zeros((2, nb, 512, 512))):
        with pytest.raises(ValueError, match="smoothed_next must"):
            call(nxt=bad)
    for bad in (np.zeros((2, 2)), np.zeros((2, nb + 1, 2)), np.zeros((1, nb, 2))):
        with pytest.raises(ValueError, match="shift_px"):
            call(shift_px=bad)
    for bad in (np.zeros((3, 4)), np.zeros(0), np.zeros(34), 1.0):
        with pytest.raises(ValueError, match="taps"):
            call(taps=bad)
    for bad in (np.zeros((3, 2)), np.zeros(0), np.zeros(4), 1.0):
        with pytest.raises(ValueError, match="heading_taps"):
            call(heading_taps=bad)
    for bad in (-1.0, float("nan"), np.zeros(3)):
        with pytest.raises(ValueError, match="floor"):
            call(floor=bad)
    with pytest.raises(ValueError, match="turn_deg"):
        call(turn_deg=np.zeros(3))
    for bad in (torch.zeros(2, nb + 1, 512, 512), torch.zeros(2, nb, 512, 512, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must"):
            call(out=bad)
    with pytest.raises(ValueError, match="out must not be the joint"):
        call(out=jt)
    with pytest.raises(ValueError, match="smoothed_next must not be the joint"):
        call(nxt=jt)
    # the order: the joint, smoothed_next, taps and floor, heading_taps, out, then the small arguments' shapes
    with pytest.raises(ValueError, match="joint must"):
        call(torch.zeros(2, 3, 512, 512), nxt=torch.zeros(1), taps=1.0)
    with pytest.raises(ValueError, match="smoothed_next must"):
        call(nxt=torch.zeros(1), taps=1.0)
    with pytest.raises(ValueError, match="taps"):
        call(taps=np.zeros(0), heading_taps=np.zeros(4), out=jt)
    with pytest.raises(ValueError, match="heading_taps"):
        call(heading_taps=np.zeros(4), out=jt, shift_px=np.zeros(3))
    with pytest.raises(ValueError, match="out must"):
        call(out=jt, shift_px=np.zeros(3))
    # accepted forms (out=smoothed_next among them): the CPU joint is refused next, before any device use
    for kw in (dict(), dict(out=nx), dict(out=torch.zeros(2, nb, 512, 512)),
               dict(taps=np.ones((2, 5), np.float32) / 9, heading_taps=torch.tensor([[0.5, 0.2, 0.05]] * 2), floor=np.full(2, 1e-6),
                    turn_deg=torch.tensor([3.0, -400.0]))):
        with pytest.raises(ValueError, match="joint must be a cuda tensor"):
            call(**kw)
    with pytest.raises(RuntimeError, match="eval"):
        smooth.track_joint_smooth(_model().train(), jt, nx, ok["shift_px"], [1.0], 0.0, 0.0, [1.0])


# ---- the restatement against a dense HMM over (bin, cell) -----------------------------------------------------------------------------

HWS, NBS = 8, 5


def _small_stream(floor, shifts):
    """4 frames over hw 8, nb 5 with rh 2 (2 rh + 2 > nb: two d meet in one bin), a fractional turn, per-bin fractional shifts"""
    rng = np.random.default_rng(7)
    T, S = 4, NBS * HWS * HWS
    like = rng.uniform(0.05, 1.0, (T, S)) ** 3
    taps = aerial.gaussian_taps(0.9, 2)
    htaps = np.float32([0.5, 0.2, 0.05])
    turn = np.float32(100.3)
    trans = [jsr.dense_transition(shifts[t], taps, turn, htaps, floor, NBS, HWS) for t in range(T - 1)]
    return like, taps, htaps, turn, trans


def _run_small(floor, shifts):
    like, taps, htaps, turn, trans = _small_stream(floor, shifts)
    alpha, post = jsr.dense_forward_backward(like, trans)
    T = like.shape[0]
    # the filter by the restated predict
    J = [None] * T
    J[0] = (like[0] / like[0].sum()).reshape(1, NBS, HWS, HWS)
    for t in range(1, T):
        prior = jsr.predict(J[t - 1], shifts[t - 1][None], taps, turn, htaps, floor, HWS)
        v = like[t].reshape(1, NBS, HWS, HWS) * prior
        J[t] = v / v.sum()
        assert np.abs(J[t].reshape(-1) - alpha[t]).max() <= 1e-12
    s = J[-1]
    worst, zs = 0.0, []
    for t in range(T - 2, -1, -1):
        res = jsr.smooth(J[t], s, shifts[t][None], taps, turn, htaps, floor, HWS)
        zs.append((res["stats"][0, 3], float(np.asarray(s).sum())))
        s = res["s"]
        worst = max(worst, float(np.abs(s.reshape(-1) - post[t]).max()))
        np.testing.assert_allclose(res["marginal"][0].reshape(-1), post[t].reshape(NBS, -1).sum(axis=0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(res["hist"][0], post[t].reshape(NBS, -1).sum(axis=1), rtol=0, atol=1e-12)
    return worst, zs


def test_the_restatement_is_the_dense_forward_backward_recursion():
    rng = np.random.default_rng(3)
    inside = rng.uniform(-0.9, 0.9, (3, NBS, 2)).astype(np.float32)
    worst, zs = _run_small(np.float32(1e-3), inside)
    print(f"positive floor, small shifts: worst |s - dense| = {worst:.2e}")
    assert worst <= 1e-12
    for Z, mass in zs:                                       # Z = sum g prior = sum s'
        assert abs(Z - mass) <= 1e-12
    leaving = rng.uniform(-3.5, 3.5, (3, NBS, 2)).astype(np.float32)   # mass leaves the 8 x 8 window; the floor stands for it
    worst, zs = _run_small(np.float32(2e-3), leaving)
    print(f"mass leaving the window: worst |s - dense| = {worst:.2e}")
    assert worst <= 1e-12
    for Z, mass in zs:
        assert abs(Z - mass) <= 1e-12


def test_the_adjoint_mix_is_the_transpose_of_the_mix():
    rng = np.random.default_rng(5)
    for nb, ht, turn in ((5, [0.5, 0.2, 0.05], 100.3), (4, [1.0], 0.0), (8, [0.8, 0.1], -400.25), (6, [0.4, 0.2, 0.1], 359.5)):
        o, M = jsr.circle(turn, nb, ht)
        a, g = rng.uniform(size=(nb, 3)), rng.uniform(size=(nb, 3))
        assert abs((jsr.mix(a, o, M) * g).sum() - (a * jsr.mix_adjoint(g, o, M)).sum()) <= 1e-14


def test_the_three_rules_in_the_restatement():
    rng = np.random.default_rng(11)
    nb, hw = 4, 8
    J = rng.uniform(0.1, 1.0, (1, nb, hw, hw))
    J /= J.sum()
    nxt = rng.uniform(0.1, 1.0, (1, nb, hw, hw))
    nxt /= nxt.sum()
    sh = np.zeros((1, nb, 2), np.float32)
    args = (sh, [0.6, 0.2], 45.0, [0.8, 0.1])
    # a zero (or negative, or NaN) next joint says nothing: J itself, its own argmax, Z = NaN, G = 0
    for z in (np.zeros_like(nxt), -nxt, np.full_like(nxt, np.nan)):
        res = jsr.smooth(J, z, *args, 1e-3, hw)
        assert np.array_equal(res["s"], J)
        i = int(np.argmax(J.sum(axis=1)))
        st = res["stats"][0]
        assert st[0] == i and st[1] == J.sum(axis=1).reshape(-1)[i] and st[2] == int(np.argmax(J[0, :, i // hw, i % hw]))
        assert np.isnan(st[3]) and st[4] == 0.0
    res = jsr.smooth(np.full_like(J, -np.inf), np.zeros_like(nxt), *args, 1e-3, hw)          # ... and without a taken value
    assert res["stats"][0, 0] == -1 and np.isnan(res["stats"][0, 1]) and res["stats"][0, 2] == -1
    # a zero J, a NaN in J, floor 0 with a prior of 0 under a positive s': zeros and (-1, NaN, -1, Z, G)
    poisoned = J.copy()
    poisoned[0, 1, 2, 3] = np.nan
    lone = np.zeros_like(J)
    lone[0, 0, 0, 0] = 1.0                                  # a delta and no blur: the prior is zero almost everywhere
    for bad, floor, tp, htp in ((np.zeros_like(J), 1e-3, [0.6, 0.2], [0.8, 0.1]), (poisoned, 1e-3, [0.6, 0.2], [0.8, 0.1]), (lone, 0.0, [1.0], [1.0])):
        res = jsr.smooth(bad, nxt, sh, tp, 45.0, htp, floor, hw)
        st = res["stats"][0]
        assert st[0] == -1 and np.isnan(st[1]) and st[2] == -1 and not (np.isfinite(st[3]) and st[3] > 0) and not st[4] == 0.0
        assert not res["s"].any() and not res["marginal"].any() and not res["hist"].any()
    # a healthy step: mass 1, Z = sum s'
    res = jsr.smooth(J, nxt, *args, 1e-3, hw)
    assert abs(res["s"].sum() - 1.0) <= 1e-14 and abs(res["stats"][0, 3] - 1.0) <= 1e-12


# ---- the crafted stream ------------------------------------------------------------------------------------------------------------------

def test_the_sweep_decides_frame_0_of_the_two_peak_stream():
    """Measured here, float64 on float32-stored joints: frame 0's filter marginal has 0.4879 of its mass within 8 px of each peak;
    smoothed, 0.999988 near A and 3.4e-10 near B, hist[0] = 0.972; Z within 1e-9 of 1 on every link."""
    st = jsr.crafted_stream()
    a0, b0 = jr.sequence_peaks(0, st["step"])
    fa, fb = jr.mass_near(st["marginals"][0], a0), jr.mass_near(st["marginals"][0], b0)
    s0 = st["smoothed"][0]
    sa, sb = jr.mass_near(s0["marginal"][0], a0), jr.mass_near(s0["marginal"][0], b0)
    print(f"frame 0: filter {fa:.4f} near A, {fb:.4f} near B; smoothed {sa:.6f} near A, {sb:.1e} near B, hist[0] {s0['hist'][0, 0]:.3f}")
    assert fa < 0.5 and fb < 0.5 and fa > 0.4 and fb > 0.4
    assert sa > 0.999 and sb < 1e-6
    assert s0["hist"][0, 0] > 0.9
    for t in range(jr.SEQ_FRAMES - 1):
        Z = st["smoothed"][t]["stats"][0, 3]
        assert abs(Z - 1.0) <= 1e-6, (t, Z)
        a, _ = jr.sequence_peaks(t, st["step"])
        assert jr.mass_near(st["smoothed"][t]["marginal"][0], a) > 0.999
        assert int(st["smoothed"][t]["stats"][0, 2]) == 0
    last = st["smoothed"][-1]
    assert np.array_equal(last["s"], st["joints"][-1].astype(np.float64)) and np.isnan(last["stats"][0, 3]) and last["stats"][0, 4] == 0.0


# ---- RecordingJointTracker and smooth_joint_stream against a stub ---------------------------------------------------------------------

class _Stub:
    """the joint filter's and the smoother's model calls, recorded; tensors of the right shapes on the CPU"""

    def __init__(self, nb):
        self.nb, self.calls, self.n = nb, [], 0

    def forward(self, grd, sat):
        B = grd.shape[0]
        return (torch.zeros(B, N), torch.zeros(B, 1, 512, 512), torch.ones(B, 2, 512, 512))

    def forward_cached(self, grd, cache, tile_index=None):
        return self.forward(grd, None)

    def track_joint_predict(self, joint, shift_px, taps, floor, turn_deg, heading_taps, out=None):
        self.calls.append(("predict", joint, np.array(shift_px), taps, floor, turn_deg, heading_taps))
        return torch.full_like(joint, 2.0)

    def track_joint_update_logits(self, logits, ori, emission, prior=None, out=None):
        B = logits.shape[0]
        self.n += 1
        joint = torch.full((B, self.nb, 512, 512), float(self.n))
        return torch.zeros(B, 5), joint, torch.full((B, 512, 512), 1.0 / N), torch.zeros(B, self.nb)


def test_recording_joint_tracker_logs_the_predict_arguments():
    nb = 8
    st, tr = _Stub(nb), smooth.RecordingJointTracker()
    assert isinstance(tr, aerial.JointTracker) and "T * B * nb MB" in smooth.RecordingJointTracker.__doc__
    em = aerial.heading_emission(2.0, nb)
    taps, ht = aerial.gaussian_taps(2.0, 6), [0.8, 0.1]
    g = torch.zeros(2, 3, 154, 231)
    origins = np.array([[800, 400], [1200, 400]])
    kw = dict(cache=torch.zeros(4), origins=origins, zero_deg=90.0, clockwise=True)
    plain = aerial.JointTracker()
    ref = plain.step(_Stub(nb), g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, tile_index=[0, 0], **kw)
    res = tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, tile_index=[0, 0], **kw)
    assert len(res) == len(ref) and all(torch.equal(a, b) for a, b in zip(res, ref))
    assert len(tr.log) == 1 and tr.log[0][0] is tr.joint and tr.log[0][1] is None
    res = tr.step(st, g, em, 4.0, -0.5, [3.0, -2.0], taps, ht, 1e-7, tile_index=[0, 1], **kw)
    assert len(tr.log) == 2
    joint, table, ltaps, lfloor, lturn, lht = tr.log[1]
    assert joint is tr.joint and ltaps is taps and lfloor == 1e-7 and lturn == [3.0, -2.0] and lht is ht
    pred = st.calls[-1]
    assert pred[0] == "predict" and pred[1] is tr.log[0][0]
    assert table.shape == (2, nb, 2) and np.array_equal(table, pred[2])                   # the table the parent's predict got
    common = aerial.oxford_track_shift(origins[[0, 0]], origins[[0, 1]], np.zeros(2))
    np.testing.assert_array_equal(table, aerial.joint_shift_table(4.0, -0.5, nb, 90.0, True, common))
    tr.reset()
    assert tr.log == [] and tr.joint is None
    tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(2, 3, 512, 512))
    tr.step(st, g, em, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(2, 3, 512, 512))
    np.testing.assert_array_equal(tr.log[1][1], np.broadcast_to(aerial.joint_shift_table(5.0, 0.5, nb), (2, nb, 2)))


def test_smooth_joint_stream_walks_the_log_backwards(monkeypatch):
    nb, B, T = 4, 2, 3
    calls = []

    def fake(model, joint, nxt, shift_px, taps, floor, turn_deg, heading_taps, out=None):
        calls.append(dict(joint=joint, nxt=nxt, nxt_value=float(nxt.flatten()[0]), shift=np.array(shift_px), taps=taps, floor=floor, turn=turn_deg,
                          ht=heading_taps, out=out))
        s = joint + nxt
        if out is not None:
            out.copy_(s)
            s = out
        v = float(s.flatten()[0])
        return s, torch.full((B, 512, 512), v), torch.full((B, nb), v), torch.full((B, 5), v)

    monkeypatch.setattr(smooth, "track_joint_smooth", fake)
    joints = [torch.full((B, nb, 512, 512), float(10 ** t)) for t in range(T)]
    tables = [None] + [np.full((B, nb, 2), float(t)) for t in range(1, T)]
    log = [(joints[t], tables[t], [0.5 + t], 0.1 * t, 7.0 * t, [1.0 - 0.1 * t]) for t in range(T)]
    for in_place in (False, True):
        calls.clear()
        marg, hist, stats, kept = smooth.smooth_joint_stream(None, log, in_place=in_place, keep_joint=True)
        assert marg.shape == (T, B, 512, 512) and hist.shape == (T, B, nb) and stats.shape == (T, B, 5) and len(kept) == T
        assert [c["joint"] is joints[t] for c, t in zip(calls, (2, 1, 0))] == [True] * 3
        # the last frame: a zero next joint and a motion that moves nothing; frame t: entry t + 1's motion
        assert calls[0]["nxt_value"] == 0.0 and not calls[0]["shift"].any() and calls[0]["taps"] == [1.0] and calls[0]["ht"] == [1.0]
        assert calls[0]["floor"] == 0.0 and calls[0]["turn"] == 0.0
        for c, t in zip(calls[1:], (1, 0)):
            assert np.array_equal(c["shift"], tables[t + 1]) and c["taps"] == [0.5 + t + 1] and c["floor"] == 0.1 * (t + 1)
            assert c["turn"] == 7.0 * (t + 1) and c["ht"] == [1.0 - 0.1 * (t + 1)]
        assert [c["nxt_value"] for c in calls] == [0.0, 100.0, 110.0]
        assert all((c["out"] is c["nxt"]) == in_place for c in calls)
        assert [float(k.flatten()[0]) for k in kept] == [111.0, 110.0, 100.0] and [float(v) for v in stats[:, 0, 0]] == [111.0, 110.0, 100.0]
        assert len({k.data_ptr() for k in kept}) == T and all(float(j.flatten()[0]) == 10 ** t for t, j in enumerate(joints))
    assert len(smooth.smooth_joint_stream(None, log)) == 3
    with pytest.raises(ValueError, match="empty"):
        smooth.smooth_joint_stream(None, [])
    with pytest.raises(ValueError, match="first frame"):
        smooth.smooth_joint_stream(None, [log[0], log[0]])
