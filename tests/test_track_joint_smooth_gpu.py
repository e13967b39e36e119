"""The joint smoother on the device (ccvpe_track_joint_smooth) against the float64 restatement
tests/joint_smooth_ref.py fed the float32 inputs the device got.

All terms are non-negative, so the bound is relative and relative errors add to first order, u = 2^-24:
    prior   the predict's count (tests/test_track_joint_gpu.py)                              4r + 2rh + 18
    g       one IEEE division                                                                4r + 2rh + 19
    G       a float64 sum of g (its own error is 2^-29 u per add), rounded once              4r + 2rh + 20
    h       M[d] three roundings, 2 rh + 2 fused multiply-adds                               4r + 4rh + 24
    P(h)    ccvpe_track_predict's 4r + 12 on top                                             8r + 4rh + 36
    a       the fused multiply-add of floor (float)G and P(h): the larger term's, plus 1     8r + 4rh + 37
    w       the product with J                                                               8r + 4rh + 38
    s       w, the float64 sum Z of such w, (float)(1 / Z) and the product                   16r + 8rh + 78
    marginal  nb adds more;  hist  a float64 sum and one rounding more;  Z as w plus the conversion;  G as above
The tests allow twice the bound wherever the restatement is >= 2^-100 and below that ask for a value <= 2^-99 that is not NaN."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, smooth, weights
from tests import golden_util as gu
from tests import joint_ref as jr
from tests import joint_smooth_ref as jsr

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
TINY = 2.0 ** -100
_BASE, _CASES = {}, {}


def base():
    """one model and one forward of three queries, shared by the tests (and left unchanged)"""
    if not _BASE:
        cfg = gu.CONFIGS["oxford"]
        m = models.CVM_OxfordRobotCar("cuda")
        m.load_state_dict(weights.generate_state_dict(cfg["variant"], cfg["seed"]))
        m = m.to("cuda").eval()
        g, s = weights.generate_inputs(cfg["variant"], 3, 11, cfg["fov"])
        logits, _, ori = m(torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda())[:3]
        _BASE.update(m=m, logits=logits.contiguous(), ori=ori.contiguous())
    return _BASE


def eq(a, b):
    assert a.shape == b.shape and torch.equal(a, b), (a.double() - b.double()).abs().max().item()


def eq_nan(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def all_eq(got, want):
    for a, b in zip(got[:3], want[:3]):
        eq(a, b)
    eq_nan(got[3], want[3])


def rel_check(got, ref, bound, what):
    """|got - ref| <= bound * ref wherever ref >= 2^-100; below that got <= 2^-99; no NaN.  Prints worst error over bound."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert not np.isnan(got).any(), what
    big = ref >= TINY
    worst = float((np.abs(got - ref)[big] / (bound * ref[big])).max()) if big.any() else 0.0
    print(f"{what}: {int(big.sum())} values checked, worst error / (twice the bound) = {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    assert (np.abs(got[~big]) <= 2.0 ** -99).all(), what
    return worst


# fractional, integer, negative and off-window shifts; bin k of query b takes entry (3 b + k) mod 9
SHIFTS = [(0.0, 0.0), (12.0, -7.0), (3.37, 0.81), (-130.6, 200.2), (-0.5, -0.5), (530.0, 0.0), (100.0, -600.5), (5.5, 5.5), (-3.0, 0.25)]


def case(nb, r, rh, B=3):
    """A link of B streams, everything per query: J from a real predict + update, s' from a real later update (the filter joint of
    frame t + 1, as for the last link of a stream), and the arguments of the predict between them.  Turns 0, a fraction and beyond
    360; floors 0, 1e-9 and 0.37.  Kept per (nb, r, rh, B) and left unchanged."""
    key = (nb, r, rh, B)
    if key not in _CASES:
        b0 = base()
        m, lg, ori = b0["m"], b0["logits"][:B].contiguous(), b0["ori"][:B].contiguous()
        em = aerial.heading_emission(np.array([1.0, 2.0, 3.0])[:B], nb)
        shift = np.array([[SHIFTS[(3 * b + k) % len(SHIFTS)] for k in range(nb)] for b in range(B)], np.float32)
        taps = aerial.gaussian_taps(np.array([0.6, 1.5, 3.0])[:B], r)
        htaps = aerial.gaussian_taps(np.array([0.5, 1.0, 2.0])[:B], rh)
        turn, floor = np.float32([0.0, 7.3, -400.25])[:B], np.float32([0.0, 1e-9, 0.37])[:B]
        first = m.track_joint_update_logits(lg, ori, em)[1]
        before = np.broadcast_to(aerial.joint_shift_table(4.0, -1.5, nb), (B, nb, 2))
        prior = m.track_joint_predict(first, before, aerial.gaussian_taps(2.0, 4), 1e-6, 20.0, [0.8, 0.1])
        J = m.track_joint_update_logits(lg.roll(1, 0), ori.roll(1, 0), em, prior, out=prior)[1]
        del first
        nxt = m.track_joint_predict(J, shift, taps, floor, turn, htaps)
        nxt = m.track_joint_update_logits(lg.roll(2, 0), ori.roll(2, 0), em, nxt, out=nxt)[1]
        _CASES[key] = dict(J=J, nxt=nxt, shift=shift, taps=taps, htaps=htaps, turn=turn, floor=floor, nb=nb, r=r, rh=rh, B=B)
    return _CASES[key]


def run(c, q=None, **kw):
    """track_joint_smooth of a case, or of its queries q alone"""
    sl = slice(None) if q is None else q
    a = dict(J=c["J"][sl].contiguous(), nxt=c["nxt"][sl].contiguous(), shift=c["shift"][sl], taps=c["taps"][sl], floor=c["floor"][sl],
             turn=c["turn"][sl], htaps=c["htaps"][sl], out=None)
    a.update(kw)
    return smooth.track_joint_smooth(base()["m"], a["J"], a["nxt"], a["shift"], a["taps"], a["floor"], a["turn"], a["htaps"], out=a["out"])


def own_row(res, nb):
    """stats carries the marginal's own bits at its own first argmax and the first best bin of the smoothed joint there"""
    sm, mg, _, st = res
    B = st.shape[0]
    s32, m32, j32 = st.cpu().numpy(), mg.cpu().numpy().reshape(B, N), sm.cpu().numpy().reshape(B, nb, N)
    idx = m32.argmax(axis=1)
    np.testing.assert_array_equal(s32[:, 0], idx.astype(np.float32))
    np.testing.assert_array_equal(s32[:, 1], m32[np.arange(B), idx])
    np.testing.assert_array_equal(s32[:, 2], j32[np.arange(B), :, idx].argmax(axis=1).astype(np.float32))


# ---- 1. the bound ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb,r,rh,B", [(4, 0, 0, 3), (8, 1, 1, 3), (5, 2, 2, 3), (6, 8, 2, 3), (72, 1, 1, 1)])
def test_smooth_follows_the_float64_restatement(nb, r, rh, B):
    """worst error over twice the bound, measured: see DESIGN.md 4.27"""
    c = case(nb, r, rh, B)
    res = run(c)
    sm, mg, hs, st = res
    assert sm.shape == (B, nb, 512, 512) and mg.shape == (B, 512, 512) and hs.shape == (B, nb) and st.shape == (B, 5)
    ref = jsr.smooth(c["J"].cpu().numpy(), c["nxt"].cpu().numpy(), c["shift"], c["taps"], c["turn"], c["htaps"], c["floor"])
    assert (ref["stats"][:, 0] >= 0).all() and (ref["stats"][:, 4] > 0).all()
    bound = 16 * r + 8 * rh + 78
    what = f"nb {nb} r {r} rh {rh}"
    rel_check(sm.cpu().numpy(), ref["s"], 2 * bound * EPS, what + " smoothed")
    rel_check(mg.cpu().numpy(), ref["marginal"], 2 * (bound + nb) * EPS, what + " marginal")
    rel_check(hs.cpu().numpy(), ref["hist"], 2 * (bound + 1) * EPS, what + " hist")
    rel_check(st[:, 3].cpu().numpy(), ref["stats"][:, 3], 2 * (8 * r + 4 * rh + 39) * EPS, what + " Z")
    rel_check(st[:, 4].cpu().numpy(), ref["stats"][:, 4], 2 * (4 * r + 2 * rh + 20) * EPS, what + " G")
    assert (np.abs(st[:, 3].double().cpu().numpy() - c["nxt"].double().sum(dim=(1, 2, 3)).cpu().numpy()) <= 1e-4).all()      # Z = sum s'
    own_row(res, nb)


# ---- 2. the same bits -------------------------------------------------------------------------------------------------------------------

def test_the_same_inputs_give_the_same_bits():
    c = case(8, 1, 1)
    want = run(c)
    all_eq(run(c), want)                                                        # a second call
    buf = c["nxt"].clone()                                                      # out=smoothed_next
    got = run(c, nxt=buf, out=buf)
    assert got[0] is buf
    all_eq(got, want)
    for q in range(3):                                                          # each query alone
        all_eq(run(c, slice(q, q + 1)), tuple(t[q:q + 1] for t in want))
    # shared against repeated taps: query 0's taps for everybody, as one set and as one set per query
    one = run(c, taps=c["taps"][0], htaps=c["htaps"][0])
    all_eq(run(c, taps=np.tile(c["taps"][:1], (3, 1)), htaps=np.tile(c["htaps"][:1], (3, 1))), one)
    all_eq(tuple(t[:1] for t in one), tuple(t[:1] for t in want))
    # two streams, each call with a work buffer of its own
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for s in streams:
        with torch.cuda.stream(s):
            got.append(run(c))
    torch.cuda.synchronize()
    for g in got:
        all_eq(g, want)
    lib = _lib.load()
    n0 = lib.ccvpe_launch_count()
    run(c)
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) <= 5


# ---- 3. the position smoother -----------------------------------------------------------------------------------------------------------

def test_equal_bins_without_a_turn_are_the_position_smoother():
    """J = b / nb in every bin, s' = s'_pos / nb, one shift for all bins, no turn, no heading blur: g, a and Z are the position
    smoother's with the floor nb * floor (nb = 8: every division is exact), so the marginal is its map, within the two bounds."""
    b0 = base()
    m, nb, r = b0["m"], 8, 3
    lg, ori = b0["logits"][:2].contiguous(), b0["ori"][:2].contiguous()
    taps = aerial.gaussian_taps(np.array([1.2, 2.0]), r)
    shift = np.float32([[3.37, -0.81], [-12.0, 7.5]])
    floor = np.float32([2.0 ** -30, 2.0 ** -12])
    _, b = m.track_update_logits(lg, ori, None)
    lp = m.track_predict(b, shift, taps, nb * floor)
    _, nxt = m.track_update_logits(lg.roll(1, 0), ori.roll(1, 0), lp)
    pos, pstats = smooth.track_smooth(m, b, nxt, shift, taps, nb * floor)
    J = (b / nb)[:, None].expand(2, nb, 512, 512).contiguous()
    sn = (nxt / nb)[:, None].expand(2, nb, 512, 512).contiguous()
    sm, mg, hs, st = smooth.track_joint_smooth(m, J, sn, np.repeat(shift[:, None], nb, axis=1), taps, floor, 0.0, [1.0])
    assert bool((sm[:, 1:] == sm[:, :1]).all())
    want = pos.double().cpu().numpy().reshape(2, N)
    tol = ((16 * r + 78 + nb) + (16 * r + 97)) * EPS
    got = mg.double().cpu().numpy().reshape(2, N)
    big = want >= TINY
    worst = float((np.abs(got - want)[big] / (tol * want[big])).max())
    print(f"marginal against track_smooth: worst difference / the sum of the two bounds = {worst:.3f}")
    assert worst <= 1.0 and (got[~big] <= 2.0 ** -99).all()
    assert (np.abs(hs.double().cpu().numpy() - 1.0 / nb) <= tol / nb).all()
    ps = pstats.double().cpu().numpy()
    assert (np.abs(st[:, 3].double().cpu().numpy() - ps[:, 2]) <= tol * ps[:, 2]).all()                       # Z
    assert (np.abs(st[:, 4].double().cpu().numpy() - nb * ps[:, 3]) <= tol * nb * ps[:, 3]).all()             # G = nb G_pos


# ---- 4. degenerate queries --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["zero_next", "zero_joint", "nan_joint", "zero_prior"])
def test_a_degenerate_query_follows_the_rules_and_its_neighbours_keep_their_bits(what):
    c = case(8, 1, 1)
    nb = 8
    want = run(c)
    J, nxt, floor = c["J"].clone(), c["nxt"].clone(), c["floor"].copy()
    if what == "zero_next":
        nxt[1] = 0.0
    elif what == "zero_joint":
        J[1] = 0.0
    elif what == "nan_joint":
        J[1, 3, 100, 200] = float("nan")
    else:
        # floor 0 and a delta: the prior is zero beyond the blur's reach, under a next joint that is positive there
        J[1] = 0.0
        J[1, 2, 256, 256] = 1.0
        floor[1] = 0.0
        assert bool((nxt[1, :, :64, :64] > 0).all())
    sm, mg, hs, st = got = run(c, J=J, nxt=nxt, floor=floor)
    for q in (0, 2):
        all_eq(tuple(t[q:q + 1] for t in got), tuple(t[q:q + 1] for t in want))
    row = st[1].cpu().numpy()
    if what == "zero_next":
        # the future says nothing: J bit for bit, its marginal in ascending k, its histogram, its argmax; Z = NaN, G = 0
        eq(sm[1], J[1])
        acc = torch.zeros_like(mg[1])
        for k in range(nb):
            acc = acc + J[1, k]
        eq(mg[1], acc)
        hsum = J[1].double().sum(dim=(1, 2))
        assert bool(((hs[1].double() - hsum).abs() <= 2 * EPS * hsum).all())
        own_row(tuple(t[1:2] for t in got), nb)
        assert row[0] >= 0 and np.isnan(row[3]) and row[4] == 0.0
    else:
        assert not bool(sm[1].any()) and not bool(mg[1].any()) and not bool(hs[1].any())
        assert row[0] == -1 and np.isnan(row[1]) and row[2] == -1
        if what == "zero_joint":
            assert row[3] == 0.0 and row[4] > 0
        elif what == "nan_joint":
            assert np.isnan(row[3])
        else:
            assert not np.isfinite(row[3]) and row[4] == np.inf


def test_a_joint_without_a_taken_value_has_no_argmax():
    c = case(8, 1, 1)
    J = torch.full_like(c["J"][:1], float("nan"))
    sm, mg, hs, st = run(c, slice(0, 1), J=J, nxt=torch.zeros_like(J))
    row = st[0].cpu().numpy()
    assert row[0] == -1 and np.isnan(row[1]) and row[2] == -1 and np.isnan(row[3]) and row[4] == 0.0
    assert bool(torch.isnan(sm).all())


# ---- 5. the crafted stream, recorded and swept ------------------------------------------------------------------------------------------

def test_the_recorded_two_peak_stream_is_swept_to_the_float64_sweep():
    """aerial's crafted stream (tests/joint_ref.py) through smooth.RecordingJointTracker and smooth.smooth_joint_stream: both forms are
    the spelled-out calls bit for bit, and every frame has the float64 sweep's argmax cell and bin - frame 0 among them, where the
    filter has 0.4879 of its mass at each peak."""
    m = base()["m"]
    ref = jsr.crafted_stream()
    nb, T = jr.SEQ_BINS, jr.SEQ_FRAMES
    step, taps, em = ref["step"], ref["taps"], ref["em"]
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0

    class Held:
        """the model with the stream's crafted forward outputs in place of the network's"""

        def __init__(self):
            self.k = 0

        def forward(self, grd, sat):
            lg = torch.from_numpy(jr.sequence_logits(self.k, step)[None]).cuda()
            self.k += 1
            return lg, None, ori

        def __getattr__(self, name):
            return getattr(m, name)

    held, tr = Held(), smooth.RecordingJointTracker()
    grd, sat = torch.zeros(1, 3, 154, 231), torch.zeros(1, 3, 512, 512)
    for k in range(T):
        tr.step(held, grd, em, jr.SEQ_FORWARD, 0.0, 0.0, taps, list(jr.SEQ_HTAPS), jr.SEQ_FLOOR, sat=sat)
    log = tr.log
    assert len(log) == T and log[0][1] is None and log[-1][0] is tr.joint
    mg, hs, st, joints = smooth.smooth_joint_stream(m, log, keep_joint=True)
    assert mg.shape == (T, 1, 512, 512) and hs.shape == (T, 1, nb) and st.shape == (T, 1, 5) and len(joints) == T
    mg2, hs2, st2, joints2 = smooth.smooth_joint_stream(m, log, in_place=True, keep_joint=True)
    for a, b in ((mg2, mg), (hs2, hs)):
        eq(a, b)
    eq_nan(st2, st)
    assert len(smooth.smooth_joint_stream(m, log)) == 3
    # spelled out
    run_ = torch.zeros_like(log[-1][0])
    for t in range(T - 1, -1, -1):
        motion = (np.zeros((1, nb, 2)), [1.0], 0.0, 0.0, [1.0]) if t == T - 1 else log[t + 1][1:]
        run_, m1, h1, s1 = smooth.track_joint_smooth(m, log[t][0], run_, *motion)
        eq(joints[t], run_)
        eq(joints2[t], run_)
        eq(mg[t], m1)
        eq(hs[t], h1)
        eq_nan(st[t], s1)
    eq(joints[-1], log[-1][0])
    rows = st.cpu().numpy()
    assert np.isnan(rows[-1, 0, 3]) and rows[-1, 0, 4] == 0.0
    for t in range(T):
        want = ref["smoothed"][t]["stats"][0]
        assert rows[t, 0, 0] == want[0] and rows[t, 0, 2] == want[2], (t, rows[t, 0], want)
        if t < T - 1:
            assert abs(rows[t, 0, 3] - 1.0) <= 1e-4
    a0, b0 = jr.sequence_peaks(0, step)
    near_a, near_b = jr.mass_near(mg[0, 0].cpu().numpy(), a0), jr.mass_near(mg[0, 0].cpu().numpy(), b0)
    print(f"frame 0 smoothed on the device: {near_a:.6f} near A, {near_b:.2e} near B, hist[0] {hs[0, 0, 0].item():.3f}")
    assert near_a > 0.999 and near_b < 1e-6 and hs[0, 0, 0].item() > 0.9
