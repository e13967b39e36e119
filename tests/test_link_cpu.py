"""The link statistics without a GPU: the C entry points and every refusal of ccvpe_track_link (all made before the
handle is used), the argument-check order of motion.track_link, the float64 restatement tests/link_ref.py against the pairwise posterior
of a dense HMM over all states of a small grid, the identities Z = sum s' and M + J = Z, what the arithmetic gives for a future that
says nothing, a zero belief and a NaN, link_offsets and link_moments against closed forms, fit_motion on a synthetic random walk, and
link_stream against a fake model."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, motion, smooth
from tests import link_ref, smooth_ref

EINVAL = -1
N = 512 * 512


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_track_link", "ccvpe_track_link_work_bytes"):
        assert hasattr(lib, n)
        assert n in {s for s, _, _ in _lib.SYMBOLS}
    assert motion.LINK_FIELDS == ("evidence", "future", "jump", "move")
    assert motion.MOMENT_FIELDS == ("move", "jump", "mean_x", "mean_y", "var_x", "var_y", "cov_xy")
    for f in (motion.track_link, motion.link_stream, motion.link_offsets, motion.link_moments, motion.fit_motion):
        assert callable(f)


def test_work_bytes_are_the_smoothers_buffer_and_the_tile_sums(built_library):
    lib = _lib.load()
    for batch in (1, 2, 3, 6, 32, 4096):
        for radius in (0, 1, 6, 32):
            got = lib.ccvpe_track_link_work_bytes(batch, radius)
            assert got == lib.ccvpe_track_smooth_work_bytes(batch) + batch * 4 * 256 * (2 * radius + 2) ** 2, (batch, radius, got)
            assert got % 16 == 0
    for batch, radius in ((0, 6), (-3, 6), (2, -1), (2, 33), (0, -1)):
        assert lib.ccvpe_track_link_work_bytes(batch, radius) == 0, (batch, radius)


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs = [(C.c_float * 64)() for _ in range(8)]                     # (ctypes arrays of this size are 16-byte aligned)
    bel, nxt, sh, tp, fl, mv, st, wk = (C.cast(b, C.c_void_p) for b in bufs)
    assert all(C.addressof(b) % 16 == 0 for b in bufs)

    def call(belief=bel, nxt=nxt, batch=2, shift=sh, taps=tp, stride=0, radius=3, floor=fl, moves=mv, stats=st, work=wk):
        return lib.ccvpe_track_link(None, belief, nxt, batch, shift, taps, stride, radius, floor, moves, stats, work, None)

    def msg():
        return (lib.ccvpe_last_error() or b"").decode()

    for kw, word in ((dict(belief=None), "belief"), (dict(nxt=None), "smoothed_next"), (dict(shift=None), "shift"), (dict(taps=None), "taps"),
                     (dict(floor=None), "floor"), (dict(moves=None), "moves"), (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**kw) == EINVAL and "null " + word in msg(), (kw, msg())
    for bad in (-1, 33, 1000):
        assert call(radius=bad) == EINVAL and "radius" in msg(), (bad, msg())
    for bad in (1, 3, 5, -4):
        assert call(stride=bad) == EINVAL and "taps_stride" in msg(), (bad, msg())
    for bad in (0, -1, 4097):
        assert call(batch=bad) == EINVAL and "batch" in msg(), (bad, msg())
    for out in ("moves", "stats", "work"):
        for other in (bel, nxt, sh, tp, fl):
            assert call(**{out: other}) == EINVAL and "alias" in msg(), (out, msg())
    for kw in (dict(moves=st), dict(moves=wk), dict(stats=wk), dict(stats=mv), dict(work=mv), dict(work=st)):
        assert call(**kw) == EINVAL and "alias" in msg(), (kw, msg())
    for name in ("belief", "nxt", "work"):
        assert call(**{name: C.c_void_p(C.addressof(bufs[0]) + 64 + 4)}) == EINVAL and "aligned" in msg(), (name, msg())
    # what is allowed reaches the handle: the next map that is the belief, every radius, both strides, the largest batch
    for kw in (dict(), dict(nxt=bel), dict(radius=0), dict(radius=32), dict(stride=4), dict(batch=4096), dict(batch=1)):
        assert call(**kw) == EINVAL and "null handle" in msg(), (kw, msg())


# ---- motion.track_link: the order of its checks (smooth.track_smooth's) ---------------------------------------------------------------

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
    ("T>S", 1, lambda m: motion.track_link(m, BEL_BAD, BEL, SHIFT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("S>next", 0, lambda m: motion.track_link(m, BEL_BAD, BEL_BAD, SHIFT, TAPS, 0.0), V, r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next>taps", 0, lambda m: motion.track_link(m, BEL, BEL_BAD, SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("next(count)>taps", 0, lambda m: motion.track_link(m, BEL, torch.zeros(3, 512, 512), SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next holds 3 maps, belief 2"),
    ("next(dtype)>taps", 0, lambda m: motion.track_link(m, BEL, BEL.double(), SHIFT, TAPS_BAD, 0.0), V, r"smoothed_next must be float32"),
    ("taps>floor", 0, lambda m: motion.track_link(m, BEL, BEL, SHIFT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("radius>floor", 0, lambda m: motion.track_link(m, BEL, BEL, SHIFT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("floor>shift", 0, lambda m: motion.track_link(m, BEL, BEL, SHIFT_BAD, TAPS, -1.0), V, r"floor must be >= 0"),
    ("shift>D", 0, lambda m: motion.track_link(m, BEL, BEL, SHIFT_BAD, TAPS, 0.0), V, r"shift_px must have shape \(2, 2\), got \(3, 2\)"),
    ("ends", 0, lambda m: motion.track_link(m, BEL, BEL, SHIFT, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message):
        call(model(bool(training)))


# ---- the restatement against the pairwise posterior of a dense HMM ---------------------------------------------------------------------

HMM_HW, HMM_T, HMM_R = 12, 5, 2
HMM_SHIFTS = np.float32([[1.3, -2.4], [2.0, -1.0], [-2.7, 0.6], [0.25, 2.9]])       # one integer shift; all inside (-3, 3)
HMM_TAPS = aerial.gaussian_taps(0.9, HMM_R)
HMM_FLOOR = np.float32(1e-3)


@pytest.fixture(scope="module")
def hmm():
    """5 frames on a 12 x 12 grid: the dense filter and smoother, and link_ref per link over the dense filter's beliefs"""
    n = HMM_HW * HMM_HW
    like = np.random.default_rng(5).uniform(0.05, 1.0, size=(HMM_T, n)) ** 4
    alpha, post = smooth_ref.dense_forward_backward(like, HMM_SHIFTS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
    links = [link_ref.link(alpha[t].reshape(1, HMM_HW, HMM_HW), post[t + 1].reshape(1, HMM_HW, HMM_HW), HMM_SHIFTS[t][None], HMM_TAPS,
                           HMM_FLOOR, HMM_HW) for t in range(HMM_T - 1)]
    return alpha, post, links


def test_restatement_is_the_dense_pairwise_posterior(hmm):
    alpha, post, links = hmm
    K = 2 * HMM_R + 2
    worst = 0.0
    for t in range(HMM_T - 1):
        bins, jump = link_ref.dense_pairwise(alpha[t], post[t + 1], HMM_SHIFTS[t], HMM_TAPS, float(HMM_FLOOR), HMM_HW)
        ox, oy = motion.link_offsets(HMM_SHIFTS[t], HMM_R)
        mv, st = links[t]["moves"][0], links[t]["stats"][0]
        named = set()
        for ky in range(K):
            for kx in range(K):
                key = (int(ox[kx]), int(oy[ky]))
                named.add(key)
                worst = max(worst, abs(mv[ky, kx] - bins.get(key, 0.0)))
        # the dense transition moves nothing by a displacement the offsets do not name
        worst = max(worst, sum(v for k, v in bins.items() if k not in named), abs(st[2] - jump))
        assert mv.sum() > 0.5 and jump > 1e-3                      # both kinds of link carry mass here
    print(f"link_ref against the dense pairwise posterior: worst absolute difference {worst:.2e}")
    assert worst <= 1e-12


def test_evidence_is_the_mass_of_the_next_map(hmm):
    _, post, links = hmm
    for t in range(HMM_T - 1):
        Z, G, J, M = links[t]["stats"][0]
        assert abs(Z - post[t + 1].sum()) <= 1e-12 and Z == M + J and G > 0, (t, Z)
    # with cells of the next map that are not taken: Z is the sum over the taken ones
    alpha = hmm[0]
    holes = post[2].copy().reshape(HMM_HW, HMM_HW)
    holes[3, 4], holes[7, 7] = np.nan, -0.25
    res = link_ref.link(alpha[1].reshape(1, HMM_HW, HMM_HW), holes[None], HMM_SHIFTS[1][None], HMM_TAPS, HMM_FLOOR, HMM_HW)
    assert abs(res["stats"][0, 0] - holes[holes > 0].sum()) <= 1e-12


def test_what_the_arithmetic_gives_for_degenerate_queries(hmm):
    alpha, post, _ = hmm
    b, nxt = alpha[1].reshape(1, HMM_HW, HMM_HW), post[2].reshape(1, HMM_HW, HMM_HW)

    def run(bb, nn, floor=HMM_FLOOR):
        r = link_ref.link(bb, nn, HMM_SHIFTS[1][None], HMM_TAPS, floor, HMM_HW)
        return r["moves"][0], r["stats"][0]

    # a next map without a positive cell - zero, all NaN, negative: G = 0, zero moves, Z = 0; not usable
    for nn in (np.zeros_like(nxt), np.full_like(nxt, np.nan), -nxt):
        mv, st = run(b, nn)
        assert not mv.any() and tuple(st) == (0.0, 0.0, 0.0, 0.0)
        mom = motion.link_moments(mv[None], st[None], HMM_SHIFTS[1])
        assert bool(torch.isnan(mom).all())
    # a zero belief with floor > 0: g = s' / floor is finite, moves 0, Sb = 0, so Z = 0
    mv, st = run(np.zeros_like(b), nxt)
    assert not mv.any() and st[0] == 0 and st[1] > 0 and st[2] == 0 and st[3] == 0
    # a NaN in the belief: Sb, and with it J and Z, are NaN
    poisoned = b.copy()
    poisoned[0, 5, 5] = np.nan
    mv, st = run(poisoned, nxt)
    assert np.isnan(st[0]) and np.isnan(st[2]) and np.isnan(mv).any()
    assert bool(torch.isnan(motion.link_moments(mv[None], st[None], HMM_SHIFTS[1])).all())


# ---- link_offsets and link_moments against closed forms --------------------------------------------------------------------------------

def test_link_offsets():
    ox, oy = motion.link_offsets([1.3, -2.4], 2)
    assert ox.tolist() == [4, 3, 2, 1, 0, -1] and oy.tolist() == [0, -1, -2, -3, -4, -5]          # i = (1, -3)
    ox, oy = motion.link_offsets(np.float32([[2.0, -1.0], [-0.25, 700.5], [np.nan, 1e9]]), 0)
    assert ox.tolist() == [[3, 2], [0, -1], [-2047, -2048]] and oy.tolist() == [[0, -1], [701, 700], [2049, 2048]]
    # the shift is read as float32: the largest double below 3 rounds up to 3
    assert motion.link_offsets([np.nextafter(3.0, 0.0), 0.0], 1)[0].tolist() == [5, 4, 3, 2]
    with pytest.raises(ValueError, match="radius"):
        motion.link_offsets([0.0, 0.0], 33)
    with pytest.raises(ValueError, match="shift_px"):
        motion.link_offsets([0.0, 0.0, 0.0], 1)


def test_link_moments_closed_forms():
    r, K = 2, 6
    shift = np.float32([[1.25, -2.5], [1.25, -2.5], [1.25, -2.5]])
    ox, oy = motion.link_offsets(shift[0], r)                 # columns 4 .. -1, rows 0 .. -5
    moves = torch.zeros(3, K, K)
    stats = torch.zeros(3, 4)
    # a single cell: displacement (ox[1], oy[4]) = (3, -4), mass 0.75 of an evidence of 1
    moves[0, 4, 1] = 0.75
    stats[0] = torch.tensor([1.0, 5.0, 0.25, 0.75])
    # a symmetric pair about the displacement (1, -2.5): (0, -2) and (2, -3), equal masses; no jump
    moves[1, 2, 4] = moves[1, 3, 2] = 0.125
    stats[1] = torch.tensor([0.25, 5.0, 0.0, 0.25])
    # not usable
    moves[2, 0, 0] = 1.0
    stats[2] = torch.tensor([0.0, 0.0, 0.0, 0.0])
    assert (int(ox[1]), int(oy[4])) == (3, -4) and (int(ox[4]), int(oy[2])) == (0, -2) and (int(ox[2]), int(oy[3])) == (2, -3)
    mom = motion.link_moments(moves, stats, shift)
    assert mom.dtype == torch.float64 and tuple(mom.shape) == (3, 7)
    np.testing.assert_allclose(mom[0].numpy(), [0.75, 0.25, 3 - 1.25, -4 + 2.5, 0.0, 0.0, 0.0], rtol=0, atol=1e-15)
    # means (1 - 1.25, -2.5 + 2.5); var_x = 1, var_y = 0.25, cov = ((-1)(0.5) + (1)(-0.5)) / 2
    np.testing.assert_allclose(mom[1].numpy(), [1.0, 0.0, -0.25, 0.0, 1.0, 0.25, -0.5], rtol=0, atol=1e-15)
    assert bool(torch.isnan(mom[2]).all())
    # one shift for every query; numpy in, too
    np.testing.assert_array_equal(motion.link_moments(moves.numpy(), stats.numpy(), shift[0]).numpy(), mom.numpy())
    with pytest.raises(ValueError, match="moves must be"):
        motion.link_moments(torch.zeros(2, 5, 5), torch.zeros(2, 4), shift[:2])


# ---- fit_motion on a synthetic random walk -------------------------------------------------------------------------------------------------

def _sweeps(bias, count):
    like, shifts = link_ref.walk_stream(bias)
    sigma, fits = link_ref.WALK_SIGMA_START, []
    for _ in range(count):
        links = link_ref.walk_links(like, shifts, aerial.gaussian_taps(sigma, link_ref.WALK_RADIUS), link_ref.WALK_FLOOR)
        fits.append(motion.fit_motion(links, list(shifts), link_ref.WALK_RADIUS, cells=link_ref.WALK_HW ** 2))
        sigma = fits[-1]["sigma"]
    return fits


def test_fit_motion_moves_sigma_towards_the_truth_and_sees_a_bias():
    """The filter starts at sigma 3.0 on a walk whose motion noise has sigma 1.2: each of three sweeps (the filter run again with the
    refitted taps, the sweep, the links, fit_motion) gives a sigma strictly between the truth and the previous value.  A bias of
    (0.5, -0.4) px per frame added to the truth moves the pooled mean residual in those directions."""
    fits = _sweeps((0.0, 0.0), 3)
    last = link_ref.WALK_SIGMA_START
    for fit in fits:
        print(f"sigma {fit['sigma']:.4f} floor {fit['floor']:.3e} rho {fit['rho']:.3e} bias {fit['bias']}")
        assert link_ref.WALK_SIGMA_TRUE < fit["sigma"] < last
        assert fit["links"] == link_ref.WALK_T - 1 and 0 < fit["rho"] < 1e-2
        assert fit["floor"] == fit["rho"] / ((1 - fit["rho"]) * link_ref.WALK_HW ** 2)
        np.testing.assert_array_equal(fit["taps"], aerial.gaussian_taps(fit["sigma"], link_ref.WALK_RADIUS))
        last = fit["sigma"]
    biased = _sweeps((0.5, -0.4), 1)[0]
    delta = biased["bias"] - fits[0]["bias"]
    print(f"bias without {fits[0]['bias']}, with (0.5, -0.4) added {biased['bias']}")
    assert delta[0] > 0.25 and delta[1] < -0.2
    # the default is the 512 x 512 grid
    links = link_ref.walk_links(*link_ref.walk_stream(), aerial.gaussian_taps(3.0, link_ref.WALK_RADIUS), link_ref.WALK_FLOOR)
    fit = motion.fit_motion(links[:3], list(link_ref.walk_stream()[1][:3]), 4)
    assert fit["floor"] == fit["rho"] / ((1 - fit["rho"]) * N) and fit["taps"].shape == (5,)


def test_fit_motion_weighs_unusable_links_zero():
    K = 4
    good = (torch.zeros(1, K, K), torch.tensor([[1.0, 3.0, 0.25, 0.75]]))
    good[0][0, 1, 1] = 0.375                 # displacements (1, 1) and (0, 0) around a shift of (0.5, 0.5): residuals +-0.5
    good[0][0, 2, 2] = 0.375
    dead = (torch.full((1, K, K), 7.0), torch.tensor([[0.0, 0.0, 0.0, 0.0]]))
    nan = (torch.full((1, K, K), float("nan")), torch.tensor([[float("nan"), 1.0, float("nan"), 1.0]]))
    fit = motion.fit_motion([good, dead, nan], [[0.5, 0.5]] * 3, 1)
    assert fit["links"] == 1 and fit["rho"] == 0.25
    np.testing.assert_allclose(fit["bias"], [0.0, 0.0], atol=1e-15)
    # m2 = 0.25 per axis, the tent's variance 0.25: nothing is left for the taps
    assert fit["sigma"] == pytest.approx(1e-6)
    with pytest.raises(ValueError, match="no usable link"):
        motion.fit_motion([dead, nan], [[0.5, 0.5]] * 2, 1)
    with pytest.raises(ValueError, match="links"):
        motion.fit_motion([good], [], 1)


# ---- link_stream against a fake model -----------------------------------------------------------------------------------------------------

def test_link_stream_pairs_each_belief_with_the_next_smoothed_map(monkeypatch):
    calls = []

    def fake_link(model, belief, nxt, shift, taps, floor):
        calls.append((float(belief[0, 0, 0]), float(nxt[0, 0, 0]), np.asarray(shift).tolist(), len(taps) - 1, floor))
        K = 2 * len(taps)
        return torch.full((1, K, K), float(belief[0, 0, 0])), torch.zeros(1, 4)

    monkeypatch.setattr(motion, "track_link", fake_link)
    log = [(torch.full((1, 512, 512), float(k + 1)), None if k == 0 else np.float64([[k, -k]]), aerial.gaussian_taps(2.0, 3 + k), 1e-7 * k)
           for k in range(4)]
    maps = [torch.full((1, 512, 512), 10.0 * (k + 1)) for k in range(4)]
    links = motion.link_stream("model", log, maps)
    assert len(links) == 3
    assert calls == [(1.0, 20.0, [[1.0, -1.0]], 4, 1e-7), (2.0, 30.0, [[2.0, -2.0]], 5, 2e-7), (3.0, 40.0, [[3.0, -3.0]], 6, 3e-7)]
    assert [tuple(m.shape) for m, _ in links] == [(1, 10, 10), (1, 12, 12), (1, 14, 14)]      # radii differ per link: lists
    with pytest.raises(ValueError, match="empty"):
        motion.link_stream("model", [], [])
    with pytest.raises(ValueError, match="maps holds 3 frames, the log 4"):
        motion.link_stream("model", log, maps[:3])
    with pytest.raises(ValueError, match="no shift"):
        motion.link_stream("model", [log[0], log[0]], maps[:2])
    # one-frame stream: no link
    assert motion.link_stream("model", log[:1], maps[:1]) == []
    assert issubclass(smooth.RecordingTracker, aerial.Tracker)
