"""Tracking a frame stream on the device (ccvpe_track_update*, ccvpe_track_predict): the update forms give the rows of
the prior forms and the map those rows are the argmax of, bit for bit and without a launch of their own; the predict kernel is exact
where exactness is defined (integer shifts, zero beliefs) and follows the float64 restatement tests/track_ref.py within the bound its
term count gives; the two together keep a moving peak through frames in which a distractor wins the per-frame argmax; and
aerial.Tracker is those two calls."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu
from tests import track_ref

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]
_MODELS = {}


def make(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _MODELS:
        cfg = gu.CONFIGS[name]
        v = cfg["variant"]
        if v == "vigor_ori_prior":
            m = models.CVM_VIGOR_ori_prior("cuda", cfg["ori_noise"], cfg["circular"], **kw)
        elif v == "vigor":
            m = models.CVM_VIGOR("cuda", cfg["circular"], **kw)
        elif v == "kitti":
            m = models.CVM_KITTI("cuda", **kw)
        else:
            m = models.CVM_OxfordRobotCar("cuda", **kw)
        m.load_state_dict(weights.generate_state_dict(v, cfg["seed"]))
        _MODELS[key] = m.to("cuda").eval()
    return _MODELS[key]


def inputs(name, batch, seed=7):
    cfg = gu.CONFIGS[name]
    g, s = weights.generate_inputs(cfg["variant"], batch, seed, cfg["fov"])
    return torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()


def gaussians(B, seed, sigma=60.0):
    c = np.random.default_rng(seed).uniform(60, 452, size=(B, 2))
    return aerial.gaussian_log_prior(c, sigma, "cuda")


def eq(a, b):
    assert a.shape == b.shape and torch.equal(a, b), (a - b).abs().max().item()


def eq_nan(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def map_carries_the_row(rows, post):
    """the map holds the bits of rows[b, 1] at rows[b, 0], and that pixel is its (first) argmax"""
    B = rows.shape[0]
    flat = post.view(B, -1)
    idx = rows[:, 0].to(torch.int64)
    assert bool((idx >= 0).all())
    eq(flat.gather(1, idx[:, None])[:, 0], rows[:, 1])
    eq(flat.argmax(dim=1), idx)


# ---- 1. update: the rows of the prior forms, the map of the forward ----------------------------------------------------------------

@pytest.mark.parametrize("name", SINGLE)
def test_update_is_the_prior_forms_rows_plus_their_map(name):
    m = make(name)
    g, s = inputs(name, 2)
    lp = gaussians(2, 1)
    logits, heat, ori = m(g, s)[:3]
    rows, post = m.track_update(g, s, lp)
    assert post.shape == (2, 512, 512) and post.dtype == torch.float32
    eq(rows, m.localize_prior(g, s, lp))
    eq(rows, m.postprocess_prior(logits, ori, lp))
    map_carries_the_row(rows, post)
    # no prior, and a zero prior (shared and per query): the forward's heatmap and localize's rows
    for z in (None, torch.zeros(512, 512, device="cuda"), torch.zeros(2, 512, 512, device="cuda")):
        r0, p0 = m.track_update(g, s, z)
        eq(r0, m.localize(g, s))
        eq(p0, heat.view(2, 512, 512))
        map_carries_the_row(r0, p0)
    # the logits form on the forward's outputs
    for prior in (lp, None):
        r1, p1 = m.track_update_logits(logits, ori, prior)
        r2, p2 = m.track_update(g, s, prior)
        eq(r1, r2)
        eq(p1, p2)
    # the cached forms: the rows of localize_prior_cached, and the logits form on forward_cached's outputs
    sc = m.encode_aerial(s)
    lc, hc, oc = m.forward_cached(g, sc)[:3]
    for tiles in (None, [0, 1]):
        r3, p3 = m.track_update_cached(g, sc, lp, tile_index=tiles)
        eq(r3, m.localize_prior_cached(g, sc, lp, tile_index=tiles))
        r4, p4 = m.track_update_logits(lc, oc, lp)
        eq(r3, r4)
        eq(p3, p4)
        map_carries_the_row(r3, p3)
        r5, p5 = m.track_update_cached(g, sc, None, tile_index=tiles)
        eq(r5, m.localize_cached(g, sc, tile_index=tiles))
        eq(p5, hc.view(2, 512, 512))
    # a shared tile: both queries read tile 1
    r6, p6 = m.track_update_cached(g, sc, lp, tile_index=[1, 1])
    eq(r6, m.localize_prior_cached(g, sc, lp, tile_index=[1, 1]))
    map_carries_the_row(r6, p6)


def test_micro_batch_slices_write_their_own_maps():
    """a micro_batch=2 handle runs five queries as slices of 2, 2, 1: every slice reads its own priors and writes its own maps (the bits
    of forward + the logits form on that handle), and agrees with the default handle wherever the posterior has no near-tie"""
    name = "vigor_prior180_circ"
    m, m2 = make(name), make(name, micro_batch=2)
    g, s = inputs(name, 5, seed=53)
    lp = gaussians(5, 4, sigma=3.0)
    logits2, _, ori2 = m2(g, s)[:3]
    for prior in (lp, None):
        got_r, got_p = m2.track_update(g, s, prior)
        ref_r, ref_p = m2.track_update_logits(logits2, ori2, prior)
        eq(got_r, ref_r)
        eq(got_p, ref_p)
    got_r, got_p = m2.track_update(g, s, lp)
    eq(got_r, m2.localize_prior(g, s, lp))
    map_carries_the_row(got_r, got_p)
    ref_r, ref_p = m.track_update(g, s, lp)
    logits, _, ori = m(g, s)[:3]
    _, margin, _ = track_ref.update(logits.cpu().numpy(), ori.cpu().numpy().reshape(5, 2, N), lp.cpu().numpy().reshape(5, N))
    sure = torch.as_tensor(margin > 1e-5)
    assert sure.sum() >= 3, margin
    eq(got_r[sure, 0], ref_r[sure, 0])
    assert ((got_r[sure, 1] - ref_r[sure, 1]).abs() <= 1e-4 * ref_r[sure, 1]).all()
    peak = ref_p.view(5, -1).max(dim=1).values[:, None, None]
    assert bool(((got_p - ref_p).abs() <= 1e-4 * peak).all())


def test_query_without_a_posterior_gets_the_empty_row_and_a_zero_map():
    name = "vigor_circ"
    m = make(name)
    g, s = inputs(name, 4, seed=47)
    lp = gaussians(4, 2)
    ok_r, ok_p = m.track_update(g, s, lp)
    lp[2] = float("-inf")
    rows, post = m.track_update(g, s, lp)
    assert rows[2, 0].item() == -1 and torch.isnan(rows[2, 1])
    assert bool((post[2] == 0).all())
    keep = [0, 1, 3]
    eq(rows[keep], ok_r[keep])
    eq(post[keep], ok_p[keep])
    eq_nan(rows, m.localize_prior(g, s, lp))
    logits, _, ori = m(g, s)[:3]
    r1, p1 = m.track_update_logits(logits, ori, lp)
    eq_nan(r1, rows)
    eq(p1, post)
    # +inf anywhere and NaN: no finite posterior either
    lp[2] = 0.0
    lp[2, 7, 9] = float("inf")
    lp[1, 100, 200] = float("nan")
    rows, post = m.track_update(g, s, lp)
    assert rows[1, 0].item() == -1 and rows[2, 0].item() == -1 and torch.isnan(rows[1:3, 1]).all()
    assert bool((post[1:3] == 0).all())
    eq(rows[[0, 3]], ok_r[[0, 3]])
    eq(post[[0, 3]], ok_p[[0, 3]])
    # the zero map restarts the filter: with a positive floor the next prior is flat
    nxt = m.track_predict(post, np.zeros((4, 2)), aerial.gaussian_taps(2.0, 6), 1e-9)
    assert bool((nxt[1:3] == nxt[1, 0, 0]).all()) and torch.isfinite(nxt[1, 0, 0])


# ---- 2. launches -----------------------------------------------------------------------------------------------------------

def test_update_adds_no_launch_and_predict_is_one():
    lib = _lib.load()
    m = make("oxford")
    g, s = inputs("oxford", 2, seed=17)
    lp = gaussians(2, 3)
    sc = m.encode_aerial(s)
    logits, _, ori = m(g, s)[:3]
    pairs = [(lambda: m.track_update(g, s, lp), lambda: m.localize_prior(g, s, lp)),
             (lambda: m.track_update_cached(g, sc, lp), lambda: m.localize_prior_cached(g, sc, lp)),
             (lambda: m.track_update_cached(g, sc, lp, tile_index=[1, 0]), lambda: m.localize_prior_cached(g, sc, lp, tile_index=[1, 0])),
             (lambda: m.track_update_logits(logits, ori, lp), lambda: m.postprocess_prior(logits, ori, lp)),
             (lambda: m.track_update(g, s), lambda: m.localize(g, s)),
             (lambda: m.track_update_cached(g, sc), lambda: m.localize_cached(g, sc))]

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for a, b in pairs:
        a(); b()                      # plans and lazy kernel attributes exist before anything is counted
        na, nb = count(a), count(b)
        assert na == nb and na > 0, (na, nb)
    _, post = m.track_update(g, s, lp)
    sh = torch.zeros(2, 2, device="cuda")
    fl = torch.full((2,), 1e-9, device="cuda")
    for r in (0, 6, 32):
        taps = torch.as_tensor(aerial.gaussian_taps(2.0, r)).cuda()
        m.track_predict(post, sh, taps, fl)
        assert count(lambda: m.track_predict(post, sh, taps, fl)) == 1


# ---- 3. predict, exact -------------------------------------------------------------------------------------------------------

def test_integer_shifts_move_pixels_exactly():
    m = make("oxford")
    g, s = inputs("oxford", 1, seed=3)
    _, heat = m.track_update(g, s)
    rng = np.random.default_rng(11)
    rnd = torch.from_numpy(rng.uniform(0, 1, size=(1, 512, 512)).astype(np.float32)).cuda()
    shifts = [(0, 0), (1, 0), (0, -1), (37, -120), (-255, 256), (511, 511), (-511, 3), (512, 0), (0, -512), (700, -900)]
    one = torch.ones(1)
    for src in (heat, rnd):
        B = len(shifts)
        bel = src.expand(B, 512, 512).contiguous()
        moved = torch.zeros_like(bel)
        for b, (dx, dy) in enumerate(shifts):       # content moves by (+dx, +dy), zero fill
            if abs(dx) < 512 and abs(dy) < 512:
                ys, yd = (slice(0, 512 - dy), slice(dy, 512)) if dy >= 0 else (slice(-dy, 512), slice(0, 512 + dy))
                xs, xd = (slice(0, 512 - dx), slice(dx, 512)) if dx >= 0 else (slice(-dx, 512), slice(0, 512 + dx))
                moved[b, yd, xd] = src[0, ys, xs]
        for floor in (0.0, 1e-9):
            got = m.track_predict(bel, np.asarray(shifts, np.float64), one, floor)
            want = m.track_predict(moved, np.zeros((B, 2)), one, floor)   # device against device: the logarithm cancels
            eq(got, want)
        # the zero-shift, radius-0 call itself is the logarithm of the belief (pixels in place)
        z = m.track_predict(bel[:1], np.zeros((1, 2)), one, 0.0)
        eq(z.argmax().reshape(1), bel[:1].argmax().reshape(1))
        assert bool(((z == float("-inf")) == (bel[:1] == 0)).all())


def test_shared_taps_equal_repeated_taps_and_a_zero_belief_gives_the_floor():
    m = make("oxford")
    rng = np.random.default_rng(12)
    bel = torch.from_numpy(rng.uniform(0, 1e-3, size=(3, 512, 512)).astype(np.float32)).cuda()
    sh = np.array([[0.25, -3.5], [100.0, 7.75], [-0.5, 0.5]])
    for r in (0, 3, 32):
        t = aerial.gaussian_taps(4.0, r)
        eq(m.track_predict(bel, sh, t, 1e-9), m.track_predict(bel, sh, np.tile(t, (3, 1)), 1e-9))
    # per-query taps are read per query
    two = np.stack([aerial.gaussian_taps(1.0, 5), aerial.gaussian_taps(3.0, 5), aerial.gaussian_taps(9.0, 5)])
    got = m.track_predict(bel, sh, two, 1e-9)
    for b in range(3):
        eq(got[b:b + 1], m.track_predict(bel[b:b + 1], sh[b:b + 1], two[b], 1e-9))
    # an all-zero belief: c is exactly 0, so every pixel is logf(floor) - exactly 0 for floor 1, one value per query otherwise, equal to
    # the float64 logarithm within logf's allowance of 4 * 2^-24 * |log|
    zero = torch.zeros(3, 512, 512, device="cuda")
    floors = np.float32([1.0, 1e-9, 0.37])
    out = m.track_predict(zero, sh, aerial.gaussian_taps(2.0, 6), floors)
    assert bool((out[0] == 0).all())
    for b in range(3):
        v = out[b, 0, 0].item()
        assert bool((out[b] == v).all())
        want = float(np.log(np.float64(floors[b])))
        assert abs(v - want) <= 4 * EPS * abs(want), (b, v, want)
    assert bool((m.track_predict(zero, sh, aerial.gaussian_taps(2.0, 6), 0.0) == float("-inf")).all())


# ---- 4. predict against the float64 restatement ------------------------------------------------------------------------------------

def check_against_ref(got, belief, shift, taps, floor, radius):
    """|log_got - log_ref| <= 2 * (4 r + 12) * 2^-24 + 4 * 2^-24 * |log_ref| wherever the reference c + floor >= 2^-100; below that
    only got <= log(2^-99) (or -inf) is required.  All terms of c are non-negative, so the float32 c is within a relative
    (4 r + 12) * 2^-24 of the float64 one (two passes of 2 r + 2 fused multiply-adds with weights of two roundings each, plus the
    two roundings of 1 - f); the test allows twice that, and 4 ulp-fractions of the result for logf."""
    got = got.double().cpu().numpy()
    c = track_ref.predict_c(belief, shift, taps)
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (c.shape[0],))[:, None, None]
    v = c + fl
    big = v >= 2.0 ** -100
    with np.errstate(divide="ignore"):
        ref = np.log(v)
    tol = 2 * (4 * radius + 12) * EPS + 4 * EPS * np.abs(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)       # (-inf against -inf is NaN here; those pixels are below the threshold)
    worst = float((err[big] / tol[big]).max()) if big.any() else 0.0
    print(f"radius {radius}: {int(big.sum())} pixels checked, worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (radius, worst)
    assert (got[~big] <= np.log(2.0 ** -99)).all()
    assert not np.isnan(got).any()


def test_predict_follows_the_float64_restatement():
    m = make("oxford")
    g, s = inputs("oxford", 1, seed=5)
    _, heat = m.track_update(g, s)
    maps = {"heat": heat[0].cpu().numpy()}
    for name, (x, y) in (("corner", (0, 0)), ("far_corner", (511, 511)), ("centre", (256, 255))):
        d = np.zeros((512, 512), np.float32)
        d[y, x] = 1.0
        maps[name] = d
    maps["uniform"] = np.full((512, 512), 1.0 / N, np.float32)
    cases = [("heat", 0.0, 0.0, 0.0), ("heat", 12.0, -7.0, 1e-9), ("heat", 3.37, 0.81, 1e-9), ("heat", -130.6, 200.2, 0.0),
             ("heat", -0.5, -0.5, 1e-3), ("corner", 0.0, 0.0, 0.0), ("corner", -0.25, 2.75, 1e-9), ("corner", 5.5, 5.5, 0.0),
             ("far_corner", 1.5, -3.25, 1e-9), ("centre", 0.125, -0.875, 0.0), ("centre", 255.5, 256.5, 1e-9),
             ("uniform", 0.0, 0.0, 0.0), ("uniform", -17.3, 40.9, 1e-9), ("uniform", 530.0, 0.0, 1e-9), ("heat", 100.0, -600.5, 1e-9),
             ("heat", -511.5, 511.25, 0.0)]
    bel = np.stack([maps[c[0]] for c in cases])
    shift = np.array([[c[1], c[2]] for c in cases], np.float32)
    floor = np.array([c[3] for c in cases], np.float32)
    dev = torch.from_numpy(bel).cuda()
    for r, sigma in ((0, 1.0), (1, 0.7), (8, 2.5), (32, 11.0)):
        taps = aerial.gaussian_taps(sigma, r)
        got = m.track_predict(dev, shift, taps, floor)
        check_against_ref(got, bel, shift, taps, floor, r)
    # per-query taps of different widths in one call
    per = aerial.gaussian_taps(np.linspace(0.6, 9.0, len(cases)), 8)
    check_against_ref(m.track_predict(dev, shift, per, floor), bel, shift, per, floor, 8)


# ---- 5. the filter does its job ------------------------------------------------------------------------------------------------

def test_the_filter_keeps_the_moving_peak_where_the_argmax_jumps_to_the_distractor():
    m = make("oxford")
    taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0
    ori_np = ori.cpu().numpy().reshape(1, 2, N)
    zero = torch.zeros(512, 512, device="cuda")
    step = np.array([track_ref.SEQ_STEP])
    belief, ref_belief = None, None
    for k in range(track_ref.SEQ_FRAMES):
        lg_np = track_ref.sequence_logits(k)[None]
        lg = torch.from_numpy(lg_np).cuda()
        plain = int(m.postprocess_prior(lg, ori, zero)[0, 0].item())     # the per-frame argmax: a prior without information
        on_distractor = track_ref.pixel_distance(plain, track_ref.SEQ_DISTRACTOR) <= 1.0
        assert on_distractor == (k in track_ref.SEQ_STRONG), (k, plain)
        lp = m.track_predict(belief, step, taps, track_ref.SEQ_FLOOR) if belief is not None else None
        rows, belief = m.track_update_logits(lg, ori, lp)
        # the float64 filter on the same stream
        ref_lp = None
        if ref_belief is not None:
            ref_lp = track_ref.predict(ref_belief, step, taps, track_ref.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        ref_rows, margin, h = track_ref.update(lg_np, ori_np, ref_lp)
        ref_belief = h.astype(np.float32).reshape(1, 512, 512)
        idx = int(rows[0, 0].item())
        if k >= 1:
            assert track_ref.pixel_distance(idx, track_ref.sequence_truth(k)) <= 2.0, (k, idx)
        if margin[0] > 1e-4:
            assert idx == int(ref_rows[0, 0]), (k, idx, ref_rows[0])


# ---- 6. aerial.Tracker ---------------------------------------------------------------------------------------------------------

def test_tracker_is_predict_plus_update_across_a_tile_change():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)             # six frames of one stream; two cached tiles
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]                       # the vehicle crosses the 400-px grid between frames 2 and 3
    motion = np.array([61.0, -9.5])                 # map pixels per frame
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    tr = aerial.Tracker()
    belief, last = None, None
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        rows = tr.step(m, gk, sc, tk, origins, motion, taps, floor)
        # the same step spelled out
        lp = None
        if belief is not None:
            shift = aerial.oxford_track_shift(origins[last], origins[tile[k]], motion)
            if tile[k] != last:
                np.testing.assert_allclose(shift, [[(-400 + 61.0) * 0.64, -9.5 * 0.64]])
            lp = m.track_predict(belief, shift, taps, floor)
            check_against_ref(lp, belief.cpu().numpy(), shift, taps, floor, 9)
        want_rows, new_belief = m.track_update_cached(gk, sc, lp, tile_index=tk)
        eq(rows, want_rows)
        eq(tr.belief, new_belief)
        assert tr.origin.tolist() == [origins[tile[k]].tolist()]
        # the update against the restatement on the forward's logits, with the prior the device used
        logits, _, ori = m.forward_cached(gk, sc, tile_index=tk)[:3]
        lg, o = logits.cpu().numpy(), ori.cpu().numpy().reshape(1, 2, N)
        ref_rows, margin, h = track_ref.update(lg, o, None if lp is None else lp.cpu().numpy().reshape(1, N))
        assert ref_rows[0, 0] >= 0
        i = int(rows[0, 0].item())
        if margin[0] > 1e-6:
            assert i == int(ref_rows[0, 0]), (k, rows[0], ref_rows[0])
        assert abs(rows[0, 1].item() - h[0, i]) <= 1e-5 * h[0, i]
        np.testing.assert_array_equal(rows[0, 2:4].cpu().numpy(), o[0, :, i])
        pk = h[0].max()
        assert np.abs(new_belief.double().cpu().numpy().reshape(-1) - h[0]).max() <= 1e-5 * pk
        belief, last = new_belief, tile[k]
    tr.reset()
    assert tr.belief is None
