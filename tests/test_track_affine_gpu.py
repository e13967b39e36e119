"""The affine predict step on the device (ccvpe_track_predict_affine): it gives the bits of ccvpe_track_predict on integer
translations and moves pixels exactly under quarter turns and flips; it follows the float64 restatement tests/track_affine_ref.py
within the bound its term count gives, for rotations, scales, a shear and matrices that leave nothing in reach; |det| keeps the mass;
it is one launch; with the update it keeps a moving peak through a turning frame; and aerial.AffineTracker is those two calls."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial
from tests import track_affine_ref as ref
from tests import track_ref
from tests.test_track_gpu import eq, inputs, make

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
SHIFTS = [(0, 0), (1, 0), (0, -1), (37, -120), (-255, 256), (511, 511), (-511, 3), (512, 0), (0, -512), (700, -900)]
FLIP_X = np.array([-1.0, 0.0, 511.0, 0.0, 1.0, 0.0])
FLIP_Y = np.array([1.0, 0.0, 0.0, 0.0, -1.0, 511.0])
_MAPS = {}


def maps():
    """a forward's heatmap and a uniform-random map, [1,512,512] on the device (computed once)"""
    if not _MAPS:
        m = make("oxford")
        g, s = inputs("oxford", 1, seed=3)
        _MAPS["heat"] = m.track_update(g, s)[1]
        rng = np.random.default_rng(11)
        _MAPS["rnd"] = torch.from_numpy(rng.uniform(0, 1, size=(1, 512, 512)).astype(np.float32)).cuda()
    return _MAPS


def translations(shifts):
    out = np.tile(IDENTITY, (len(shifts), 1))
    out[:, 2], out[:, 5] = -np.asarray(shifts, np.float64)[:, 0], -np.asarray(shifts, np.float64)[:, 1]
    return out


def check_against_ref(got, belief, matrix, taps, floor, radius):
    """On every pixel with v = c_ref + floor >= 2^-100 the device's c may differ from the restatement's by
        d = 2 (4 r + 12) 2^-24 c_ref + 2^-38 max(belief of the query),
    i.e. log(v - d) <= log_got <= log(v + d) (no lower limit where d >= v), each side widened by 4 * 2^-24 * |log v| for logf.
    First term: all terms of c are non-negative, about 8 roundings in the sample and 2 r + 1 fused multiply-adds per pass give a
    relative (4 r + 10) 2^-24; the test allows twice (4 r + 12) 2^-24, the constant of tests/test_track_gpu.py.  Second term: the
    float64 coordinates of the device (fused) and of the restatement differ by <= 2^-42 px, which moves a sample by at most that times
    the neighbouring values; a factor of 8 is margin.  Below the threshold the same bound gives log_got <= log(2^-99 + 2^-38 max)."""
    got = got.double().cpu().numpy()
    bel = np.asarray(belief, np.float64).reshape(-1, 512, 512)
    c = ref.predict_c(belief, matrix, taps)
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (c.shape[0],))[:, None, None]
    absolute = 2.0 ** -38 * bel.max(axis=(1, 2))[:, None, None]
    v = c + fl
    big = v >= 2.0 ** -100
    d = 2 * (4 * radius + 12) * EPS * c + absolute
    with np.errstate(divide="ignore", invalid="ignore"):
        logv = np.log(v)
        hi = np.log1p(d / v)
        lo = -np.log1p(-np.minimum(d / v, 1.0))      # inf where d >= v
        slack = 4 * EPS * np.abs(logv)
        over = (got - logv) / (hi + slack)           # (-inf against -inf is NaN here; those pixels are below the threshold)
        under = np.where(np.isinf(lo), 0.0, (logv - got) / (lo + slack))
    worst = float(max(over[big].max(), under[big].max())) if big.any() else 0.0
    print(f"radius {radius}: {int(big.sum())} pixels checked, worst error / bound = {worst:.3f}")
    assert not np.isnan(got).any()
    assert worst <= 1.0, (radius, worst)
    limit = np.broadcast_to(np.log(2.0 ** -99 + absolute), v.shape)
    assert (got[~big] <= limit[~big] * (1 - 4 * EPS)).all()


# ---- 1. exact: integer translations give ccvpe_track_predict's bits ------------------------------------------------------------------

@pytest.mark.parametrize("src", ["heat", "rnd"])
def test_integer_translations_give_the_bits_of_track_predict(src):
    m = make("oxford")
    B = len(SHIFTS)
    bel = maps()[src].expand(B, 512, 512).contiguous()
    mats = translations(SHIFTS)
    for taps in (torch.ones(1), aerial.gaussian_taps(2.0, 6)):
        for floor in (0.0, 1e-9):
            got = m.track_predict_affine(bel, mats, taps, floor)
            eq(got, m.track_predict(bel, np.asarray(SHIFTS, np.float64), taps, floor))
            assert bool((got[9] == got[9, 0, 0]).all())      # nothing left in reach: logf(floor) everywhere


# ---- 2. exact: quarter turns and flips move pixels ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("src", ["heat", "rnd"])
def test_quarter_turns_and_flips_move_pixels_exactly(src):
    m = make("oxford")
    one = maps()[src]
    turned = [torch.rot90(one, k, dims=(1, 2)) for k in range(4)] + [torch.flip(one, dims=(2,)), torch.flip(one, dims=(1,))]
    mats = np.concatenate([aerial.rigid_matrix(90.0 * np.arange(4), [0, 0]), FLIP_X[None], FLIP_Y[None]])
    B = len(mats)
    bel = one.expand(B, 512, 512).contiguous()
    for floor in (0.0, 1e-9):
        got = m.track_predict_affine(bel, mats, torch.ones(1), floor)
        eq(got, m.track_predict_affine(torch.cat(turned).contiguous(), IDENTITY, torch.ones(1), floor))
        # a quarter turn swaps the x and the y pass of the blur, so with taps the sums differ in order: held to the restatement instead
        taps = aerial.gaussian_taps(2.0, 6)
        check_against_ref(m.track_predict_affine(bel, mats, taps, floor), bel.cpu().numpy(), mats, taps, floor, 6)


# ---- 3. against the float64 restatement ----------------------------------------------------------------------------------------------

def test_affine_predict_follows_the_float64_restatement():
    m = make("oxford")
    named = {"heat": maps()["heat"][0].cpu().numpy()}
    for name, (x, y) in (("corner", (0, 0)), ("far_corner", (511, 511)), ("centre", (256, 255))):
        d = np.zeros((512, 512), np.float32)
        d[y, x] = 1.0
        named[name] = d
    named["uniform"] = np.full((512, 512), 1.0 / N, np.float32)
    R = aerial.rigid_matrix
    shear = np.array([1.05, 0.31, -40.7, -0.12, 0.93, 22.15])
    cases = [("heat", R(0.5, [3.37, 0.81]), 1e-9), ("heat", R(5.0, [12.25, -7.5]), 0.0), ("heat", R(37.5, [-30.6, 20.2]), 1e-9),
             ("heat", R(90.0, [0.5, -0.25]), 0.0), ("heat", R(-171.0, [7.77, 3.33]), 1e-3), ("heat", R(5.0, [1.5, 2.5], 0.8), 1e-9),
             ("heat", R(-20.0, [-4.25, 9.0], 1.25), 0.0), ("heat", shear, 1e-9), ("corner", R(5.0, [20.3, 31.9]), 0.0),
             ("corner", R(0.0, [-0.25, 2.75]), 1e-9), ("far_corner", R(-37.5, [-11.5, 3.25], 1.25), 1e-9),
             ("centre", R(37.5, [0.125, -0.875], 0.8), 0.0), ("uniform", R(5.0, [0.0, 0.0]), 0.0), ("uniform", shear, 1e-9),
             ("heat", translations([(600.0, 0.0)])[0], 1e-9), ("heat", np.zeros(6), 1e-9), ("uniform", translations([(1e6, -1e6)])[0], 1e-9)]
    bel = np.stack([named[c[0]] for c in cases])
    mats = np.stack([c[1] for c in cases])
    floor = np.array([c[2] for c in cases], np.float32)
    dev = torch.from_numpy(bel).cuda()
    for r, sigma in ((0, 1.0), (1, 0.7), (8, 2.5), (32, 11.0)):
        taps = aerial.gaussian_taps(sigma, r)
        got = m.track_predict_affine(dev, mats, taps, floor)
        check_against_ref(got, bel, mats, taps, floor, r)
        for b in (14, 15, 16):      # nothing in reach, a degenerate matrix, a clamped translation: logf(floor) everywhere
            assert bool((got[b] == got[b, 0, 0]).all()) and abs(got[b, 0, 0].item() - np.log(1e-9)) <= 4 * EPS * abs(np.log(1e-9))
    # per-query taps of different widths in one call; the matrices as a float64 tensor on the device
    per = aerial.gaussian_taps(np.linspace(0.6, 9.0, len(cases)), 8)
    check_against_ref(m.track_predict_affine(dev, torch.from_numpy(mats).cuda(), per, floor), bel, mats, per, floor, 8)


# ---- 4. |det| keeps the mass ---------------------------------------------------------------------------------------------------------------

def test_the_determinant_keeps_the_mass_across_a_change_of_scale():
    m = make("oxford")
    y, x = np.mgrid[0:512, 0:512].astype(np.float64)
    heat = np.exp(-((x - 262.0) ** 2 + (y - 249.0) ** 2) / (2 * 12.0 ** 2)) + 0.5 * np.exp(-((x - 240.3) ** 2 + (y - 281.6) ** 2) / (2 * 5.0 ** 2))
    heat = (heat / heat.sum()).astype(np.float32)
    mats = np.stack([aerial.rigid_matrix(5.0, [2.5, -1.25], 0.8), aerial.rigid_matrix(5.0, [2.5, -1.25], 1.25),
                     aerial.rigid_matrix(5.0, [2.5, -1.25])])
    bel = np.stack([heat] * 3)
    out = m.track_predict_affine(torch.from_numpy(bel).cuda(), mats, [1.0], 0.0)
    total = float(heat.sum(dtype=np.float64))
    got = torch.exp(out.double()).sum(dim=(1, 2)).cpu().numpy()
    want = ref.predict_c(bel, mats, [1.0]).sum(axis=(1, 2))
    print("mass of the belief", total, "device", got, "restatement", want)
    assert np.abs(got - total).max() <= 1e-3 and np.abs(want - total).max() <= 1e-3
    assert np.abs(got - want).max() <= 1e-5


# ---- 5. launches, taps, zero beliefs, one matrix for all --------------------------------------------------------------------------------

def test_one_launch_shared_taps_zero_belief_and_a_broadcast_matrix():
    lib = _lib.load()
    m = make("oxford")
    rng = np.random.default_rng(12)
    bel = torch.from_numpy(rng.uniform(0, 1e-3, size=(3, 512, 512)).astype(np.float32)).cuda()
    mats = np.stack([aerial.rigid_matrix(5.0, [0.25, -3.5]), aerial.rigid_matrix(-60.0, [100.0, 7.75], 1.1), translations([(-0.5, 0.5)])[0]])

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    dm = torch.from_numpy(mats).cuda()
    fl = torch.full((3,), 1e-9, device="cuda")
    for r in (0, 6, 32):
        taps = torch.as_tensor(aerial.gaussian_taps(2.0, r)).cuda()
        m.track_predict_affine(bel, dm, taps, fl)
        assert count(lambda: m.track_predict_affine(bel, dm, taps, fl)) == 1
    for r in (0, 3, 32):
        t = aerial.gaussian_taps(4.0, r)
        eq(m.track_predict_affine(bel, mats, t, 1e-9), m.track_predict_affine(bel, mats, np.tile(t, (3, 1)), 1e-9))
    # per-query taps and matrices are read per query
    three = np.stack([aerial.gaussian_taps(1.0, 5), aerial.gaussian_taps(3.0, 5), aerial.gaussian_taps(9.0, 5)])
    got = m.track_predict_affine(bel, mats, three, 1e-9)
    for b in range(3):
        eq(got[b:b + 1], m.track_predict_affine(bel[b:b + 1], mats[b:b + 1], three[b], 1e-9))
    # a [6] matrix serves every query, from the host and from the device
    t = aerial.gaussian_taps(2.0, 6)
    want = m.track_predict_affine(bel, np.tile(mats[0], (3, 1)), t, 1e-9)
    eq(m.track_predict_affine(bel, mats[0], t, 1e-9), want)
    eq(m.track_predict_affine(bel, dm[0], t, 1e-9), want)
    # an all-zero belief: c is exactly 0, every pixel is logf(floor)
    zero = torch.zeros(3, 512, 512, device="cuda")
    floors = np.float32([1.0, 1e-9, 0.37])
    out = m.track_predict_affine(zero, mats, t, floors)
    assert bool((out[0] == 0).all())
    for b in range(3):
        v = out[b, 0, 0].item()
        assert bool((out[b] == v).all())
        want_v = float(np.log(np.float64(floors[b])))
        assert abs(v - want_v) <= 4 * EPS * abs(want_v), (b, v, want_v)
    assert bool((m.track_predict_affine(zero, mats, t, 0.0) == float("-inf")).all())


# ---- 6. the filter does its job in a turning frame -------------------------------------------------------------------------------------

def test_the_filter_keeps_the_moving_peak_in_a_turning_frame():
    m = make("oxford")
    taps = aerial.gaussian_taps(ref.SEQ_SIGMA, ref.SEQ_RADIUS)
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0
    ori_np = ori.cpu().numpy().reshape(1, 2, N)
    zero = torch.zeros(512, 512, device="cuda")
    belief, ref_belief = None, None
    for k in range(ref.SEQ_FRAMES):
        lg_np = ref.sequence_logits(k)[None]
        lg = torch.from_numpy(lg_np).cuda()
        plain = int(m.postprocess_prior(lg, ori, zero)[0, 0].item())     # the per-frame argmax: a prior without information
        on_distractor = track_ref.pixel_distance(plain, ref.SEQ_DISTRACTOR) <= 1.0
        assert on_distractor == (k in ref.SEQ_STRONG), (k, plain)
        mat = ref.sequence_matrix(k)
        lp = m.track_predict_affine(belief, mat, taps, ref.SEQ_FLOOR) if belief is not None else None
        rows, belief = m.track_update_logits(lg, ori, lp)
        # the float64 filter on the same stream (tests/test_track_affine_cpu.py: its margin is > 1e-4 in every frame)
        ref_lp = None
        if ref_belief is not None:
            ref_lp = ref.predict(ref_belief, mat, taps, ref.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        ref_rows, _, h = track_ref.update(lg_np, ori_np, ref_lp)
        ref_belief = h.astype(np.float32).reshape(1, 512, 512)
        idx = int(rows[0, 0].item())
        if k >= 1:
            assert track_ref.pixel_distance(idx, ref.sequence_truth(k)) <= 2.0, (k, idx)
        assert idx == int(ref_rows[0, 0]), (k, idx, ref_rows[0])


# ---- 7. aerial.AffineTracker -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cached", [("kitti", False), ("oxford", True)])
def test_affine_tracker_is_predict_plus_update(name, cached):
    m = make(name)
    F = 6
    g, s = inputs(name, F, seed=23)
    sc = m.encode_aerial(s[:2]) if cached else None
    tile = [0, 0, 0, 1, 1, 1]
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    mats = aerial.rigid_matrix(np.array([0.0, 4.0, -7.5, 120.0, 2.0, 0.0]), np.array([[0, 0], [6.5, -2.25], [-3.0, 8.0], [10.0, 10.0], [0.5, 0.5], [4.0, -6.0]]),
                               np.array([1.0, 1.0, 1.0, 1.0, 1.1, 1.0]))
    variants = {"plain": {}, "summary": dict(summary_radius=5), "heading": dict(heading_bins=36),
                "both": dict(summary_radius=5, heading_bins=36)}
    trackers = {v: aerial.AffineTracker() for v in variants}
    beliefs = {v: None for v in variants}
    for k in range(F):
        gk = g[k:k + 1]
        side = dict(cache=sc, tile_index=[tile[k]]) if cached else {}
        for v, kw in variants.items():
            got = trackers[v].step(m, gk, None if cached else s[k:k + 1], mats[k], taps, floor, **kw, **side)
            # the same step spelled out
            lp = None if beliefs[v] is None else m.track_predict_affine(beliefs[v], mats[k], taps, floor)
            if k == 0:
                assert lp is None
            aer = (sc,) if cached else (s[k:k + 1],)
            tix = dict(tile_index=[tile[k]]) if cached else {}
            if v == "plain":
                call = m.track_update_cached if cached else m.track_update
                rows, post = call(gk, *aer, lp, **tix)
                want = (rows,)
                got = (got,)
            elif v == "summary":
                call = m.localize_summary_cached if cached else m.localize_summary
                rows, summary, post = call(gk, *aer, lp, radius=5, posterior=True, **tix)
                want = (rows, summary)
            else:
                call = m.localize_heading_cached if cached else m.localize_heading
                res = call(gk, *aer, lp, radius=5 if v == "both" else 8, bins=36, summary=v == "both", posterior=True, **tix)
                post = res[-1]
                want = (res[0], res[3], res[1], res[2]) if v == "both" else (res[0], res[1], res[2])
            assert len(got) == len(want)
            for a, b in zip(got, want):
                torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
            eq(trackers[v].belief, post)
            assert trackers[v].belief.is_cuda
            beliefs[v] = post
        # every variant carries the same rows and belief
        for v in ("summary", "heading", "both"):
            eq(beliefs[v], beliefs["plain"])
    trackers["plain"].reset()
    assert trackers["plain"].belief is None


def test_affine_tracker_reproduces_the_oxford_tracker_at_integer_shifts():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]                       # the vehicle crosses the 400-px grid between frames 2 and 3
    motion = np.array([25.0, -50.0])                # map pixels per frame: (16, -32) output pixels
    taps = aerial.gaussian_taps(3.0, 9)
    old, new = aerial.Tracker(), aerial.AffineTracker()
    last = None
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        shift = np.zeros((1, 2)) if last is None else aerial.oxford_track_shift(origins[last], origins[tile[k]], motion)
        assert (shift == np.round(shift)).all()
        want = old.step(m, gk, sc, tk, origins, motion, taps, 1e-7, summary_radius=4)
        got = new.step(m, gk, None, aerial.rigid_matrix(0.0, shift), taps, 1e-7, summary_radius=4, cache=sc, tile_index=tk)
        for a, b in zip(got, want):
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
        eq(new.belief, old.belief)
        last = tile[k]
