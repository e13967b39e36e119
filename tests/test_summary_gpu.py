"""The posterior summary on the device (ccvpe_*_summary, ccvpe_belief_summary): the stored-map form follows the float64
restatement tests/summary_ref.py within the bounds the number formats give (summary_ref.assert_rows_close) on crafted maps and at a
misaligned address; the logits and network forms give the rows and the map of the track_update forms bit for bit, a summary that is
the restatement of that map, the same bits with or without the map and from call to call, and no launch of their own; a query without
a posterior gets the empty row; aerial.Tracker passes the summary through."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu
from tests import summary_ref as sr

pytestmark = pytest.mark.gpu

N = 512 * 512
RADII = (0, 1, 8, 32)
SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]
_MODELS = {}
_REFS = {}


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


def eq_bits(a, b):
    """the same bits, NaN included"""
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (a, b)


def crafted(name, r):
    """the restatement's row of a crafted map, computed once"""
    if (name, r) not in _REFS:
        _REFS[(name, r)] = sr.summary(MAPS[name], r)
    return _REFS[(name, r)]


def against_own_map(summary, post, r, what):
    """a summary against the restatement of the map the same call returned"""
    sr.assert_rows_close(summary.cpu().numpy(), sr.summaries(post.cpu().numpy(), r), what)


MAPS = sr.crafted_maps()
BATCHES = [("delta_origin", "gauss_border", "random"), ("delta_corner", "uniform", "two_deltas"),
           ("delta_inside", "two_deltas_scaled", "gauss_centre")]


def logits_case():
    """forward outputs without a network: three different logit maps (noise; noise with a sharp peak near the border; a broad blob
    with a second one) and a unit orientation field"""
    rng = np.random.default_rng(19)
    lg = rng.normal(0.0, 2.0, size=(3, 512, 512)).astype(np.float32)
    lg[1, 3, 500] += 30.0
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    lg[2] = 12.0 * np.exp(-0.5 * ((xx - 140) ** 2 + (yy - 380) ** 2) / 400.0) + 11.0 * np.exp(-0.5 * ((xx - 400) ** 2 + (yy - 90) ** 2) / 100.0)
    a = rng.uniform(-np.pi, np.pi, size=(3, 512, 512))
    ori = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    return torch.from_numpy(lg.reshape(3, N)).cuda(), torch.from_numpy(ori).cuda()


# ---- 1. the stored-map form against the restatement ------------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_stored_maps_follow_the_restatement(r):
    m = make("oxford")
    for names in BATCHES:                        # three different maps per call: a wrong per-sample offset shows
        bel = torch.from_numpy(np.stack([MAPS[n] for n in names])).cuda()
        got = m.belief_summary(bel, r)
        assert got.shape == (3, 16) and got.dtype == torch.float32
        sr.assert_rows_close(got.cpu().numpy(), np.stack([crafted(n, r) for n in names]), f"r={r} {names}")
        eq_bits(got, m.belief_summary(bel.view(3, 1, 512, 512), r))
    # the same maps at an address that is 4-byte but not 16-byte aligned: the value-by-value path (another order of the sums, so other
    # last bits) keeps the bounds and its own bits from call to call
    names = BATCHES[0]
    flat = torch.empty(3 * N + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(3, 512, 512)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    off.copy_(torch.from_numpy(np.stack([MAPS[n] for n in names])))
    got = m.belief_summary(off, r)
    sr.assert_rows_close(got.cpu().numpy(), np.stack([crafted(n, r) for n in names]), f"r={r} misaligned")
    eq_bits(got, m.belief_summary(off, r))
    eq_bits(got[:, [0, 1, 15]], m.belief_summary(off.clone(), r)[:, [0, 1, 15]])


# ---- 2. special maps -----------------------------------------------------------------------------------------------------------

def test_special_maps():
    m = make("oxford")
    zero = np.zeros((512, 512), np.float32)
    nan = MAPS["random"].copy()
    nan[10, 20] = np.nan
    nan[400, 17] = 2.0
    tie = sr.delta((300, 40), (30, 41), (31, 41), value=0.25)
    maps = np.stack([zero, nan, tie])
    for r in (1, 8):
        got = m.belief_summary(torch.from_numpy(maps).cuda(), r).cpu().numpy()
        assert (got[0, :3] == 0).all() and np.isnan(got[0, 3:]).all()
        assert got[1, 0] == 400 * 512 + 17 and got[1, 1] == 2.0 and 0 <= got[1, 0] < N      # the finite maximum, inside the map
        assert np.isnan(got[1, 2:10]).all() and got[1, 15] == (2 * r + 1) ** 2
        assert got[2, 0] == 40 * 512 + 300 and (got[2, 10], got[2, 11]) == (300.0, 40.0)   # the first of the equal maxima
        sr.assert_rows_close(got, sr.summaries(maps, r), f"special r={r}")


# ---- 3. the logits form --------------------------------------------------------------------------------------------------------

def test_logits_form_is_track_update_logits_plus_the_summary_of_its_map():
    m = make("oxford")
    lg, ori = logits_case()
    lp = gaussians(3, 5, sigma=80.0)
    zero = torch.zeros(512, 512, device="cuda")
    for prior in (lp, None):
        want_rows, want_map = m.track_update_logits(lg, ori, prior)
        eq(want_rows, m.postprocess_prior(lg, ori, prior if prior is not None else zero))
        for r in RADII:
            rows, summ, post = m.postprocess_summary(lg, ori, prior, radius=r, posterior=True)
            assert rows.shape == (3, 5) and summ.shape == (3, 16) and post.shape == (3, 512, 512)
            eq(rows, want_rows)
            eq(post, want_map)
            eq_bits(summ[:, 0:2], rows[:, 0:2])
            against_own_map(summ, post, r, f"logits r={r} prior={prior is not None}")
            rows2, summ2 = m.postprocess_summary(lg, ori, prior, radius=r)          # without the map: the same bits
            eq(rows2, rows)
            eq_bits(summ2, summ)
            eq_bits(m.postprocess_summary(lg, ori, prior, radius=r)[1], summ)       # and again
            eq_bits(m.belief_summary(post, r), summ)          # the stored-map form on that map: one accumulation, one order, the same bits
    # the default radius is 8, a shared prior map is read by every query
    eq_bits(m.postprocess_summary(lg, ori)[1], m.postprocess_summary(lg, ori, None, radius=8)[1])
    one = lp[:1].contiguous()
    eq_bits(m.postprocess_summary(lg, ori, one[0])[1], m.postprocess_summary(lg, ori, one.expand(3, 512, 512).contiguous())[1])


# ---- 4. the network forms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SINGLE)
def test_network_forms_are_the_prior_forms_rows_plus_the_summary_of_their_map(name):
    m = make(name)
    g, s = inputs(name, 2)
    lp = gaussians(2, 1)
    rows, summ, post = m.localize_summary(g, s, lp, posterior=True)
    eq(rows, m.localize_prior(g, s, lp))
    want_rows, want_map = m.track_update(g, s, lp)
    eq(rows, want_rows)
    eq(post, want_map)
    eq_bits(summ[:, 0:2], rows[:, 0:2])
    against_own_map(summ, post, 8, f"{name} full")
    r0, s0 = m.localize_summary(g, s, radius=32)                       # no prior, no map
    eq(r0, m.localize(g, s))
    eq_bits(s0, m.localize_summary(g, s, radius=32, posterior=True)[1])
    against_own_map(s0, m.track_update(g, s)[1], 32, f"{name} full, no prior")
    sc = m.encode_aerial(s)
    for tiles in (None, [0, 1], [1, 1]):
        r1, s1, p1 = m.localize_summary_cached(g, sc, lp, radius=1, posterior=True, tile_index=tiles)
        eq(r1, m.localize_prior_cached(g, sc, lp, tile_index=tiles))
        eq(p1, m.track_update_cached(g, sc, lp, tile_index=tiles)[1])
        against_own_map(s1, p1, 1, f"{name} cached {tiles}")
        r2, s2 = m.localize_summary_cached(g, sc, radius=1, tile_index=tiles)
        eq(r2, m.localize_cached(g, sc, tile_index=tiles))
        against_own_map(s2, m.track_update_cached(g, sc, tile_index=tiles)[1], 1, f"{name} cached {tiles}, no prior")


def test_micro_batch_slices_write_their_own_summaries():
    """a micro_batch=2 handle runs three queries as slices of 2 + 1: every slice reads its own prior and writes its own rows, summary
    and map - the bits of the same handle's calls on the two slices - and every summary is the restatement of its own map.  The default
    handle's one batch of 3 runs other plans with other convolution tiles, so its logits differ in their last bits (as
    tests/test_track_gpu.py records: maps within 1e-4 of the peak, no bit equality); against it the index agrees wherever the argmax has
    no near-tie, the probability within that test's 1e-4, and every summary column within what the difference of the two maps allows
    (across_handles)."""
    name = "vigor_prior180_circ"
    m, m2 = make(name), make(name, micro_batch=2)
    g, s = inputs(name, 3, seed=53)
    lp = gaussians(3, 4, sigma=3.0)
    for prior in (lp, None):
        rows, summ, post = m2.localize_summary(g, s, prior, radius=8, posterior=True)
        against_own_map(summ, post, 8, f"micro-batch prior={prior is not None}")
        eq_bits(summ[:, 0:2], rows[:, 0:2])
        for sl in (slice(0, 2), slice(2, 3)):
            ra, sa, pa = m2.localize_summary(g[sl], s[sl], None if prior is None else prior[sl].contiguous(), radius=8, posterior=True)
            eq(rows[sl], ra)
            eq_bits(summ[sl], sa)
            eq(post[sl], pa)
        r1, s1, p1 = m.localize_summary(g, s, prior, radius=8, posterior=True)
        top = p1.view(3, -1).topk(2, dim=1).values
        sure = (top[:, 0] - top[:, 1]) > 3e-4 * top[:, 0]          # the gap exceeds what 1e-4 of the peak on either map can close
        if prior is not None:
            assert int(sure.sum()) >= 2, top                        # (a prior of sigma 3 px leaves a clear peak)
        eq(rows[sure, 0], r1[sure, 0])
        assert ((rows[sure, 1] - r1[sure, 1]).abs() <= 1e-4 * r1[sure, 1]).all()
        peak = p1.view(3, -1).max(dim=1).values[:, None, None]
        assert bool(((post - p1).abs() <= 1e-4 * peak).all())
        across_handles(s1, summ, p1, post, sure.cpu().numpy(), f"across handles prior={prior is not None}")


def across_handles(sa, sb, pa, pb, same_argmax, what):
    """Two summaries of two maps a, b of the same queries that differ a little.  With b_i = a_i (1 + e_i), |e_i| <= eta, every
    normalised expectation moves by at most eta / (1 - eta) * E_a|f - E_a f|: a mean by eta' sigma, a variance by 2 eta' var (var_b <=
    E_b (x - mean_a)^2 <= var_a (1 + eta) / (1 - eta), and the same the other way), a covariance by 3 eta' sigma_x sigma_y, a mass or a
    ratio of masses by 2 eta' of itself, the entropy by 2 eta' (H + 1).  eta is taken from the two maps (values of at least 1e-30; the
    rest holds less than 3e-25 of the mass), the test allows 4 eta in every formula, plus twice the format tolerance of
    summary_ref.assert_rows_close (each summary is that close to the restatement of its own map).  The window columns are compared
    where both calls found the same argmax."""
    a, b = sa.double().cpu().numpy(), sb.double().cpu().numpy()
    ha, hb = pa.double().cpu().numpy().reshape(len(a), -1), pb.double().cpu().numpy().reshape(len(a), -1)
    for q in range(len(a)):
        big = ha[q] >= 1e-30
        eta = float(np.abs(hb[q][big] / ha[q][big] - 1.0).max())
        k = 4.0 * eta
        assert eta < 0.05, (what, q, eta)
        sx, sy = np.sqrt(max(a[q, 6], b[q, 6])), np.sqrt(max(a[q, 8], b[q, 8]))
        wx, wy = np.sqrt(max(a[q, 12], b[q, 12], 0.0)), np.sqrt(max(a[q, 14], b[q, 14], 0.0))
        bound = {2: k * a[q, 2] + 2e-6 * a[q, 2], 3: k * (a[q, 3] + 1.0) + 2e-4, 4: k * sx + 2e-4, 5: k * sy + 2e-4,
                 6: k * sx * sx + 2e-5 * max(sx * sx, 1.0), 7: k * sx * sy + 2e-5 * max(sx * sy, 1.0), 8: k * sy * sy + 2e-5 * max(sy * sy, 1.0)}
        if same_argmax[q]:
            bound.update({9: k * a[q, 9] + 2e-6 * a[q, 9], 10: k * wx + 2e-4, 11: k * wy + 2e-4, 12: k * wx * wx + 2e-5 * max(wx * wx, 1.0),
                          13: k * wx * wy + 2e-5 * max(wx * wy, 1.0), 14: k * wy * wy + 2e-5 * max(wy * wy, 1.0)})
            assert a[q, 0] == b[q, 0] and a[q, 15] == b[q, 15], (what, q)
        err = {c: abs(a[q, c] - b[q, c]) for c in bound}
        print(f"{what} query {q}: eta {eta:.3g}, error / bound = " + ", ".join(f"{c}: {err[c] / bound[c]:.3g}" for c in bound))
        bad = [c for c in bound if not err[c] <= bound[c]]
        assert not bad, (what, q, eta, {c: (a[q, c], b[q, c], bound[c]) for c in bad})


# ---- 5. a query without a posterior ------------------------------------------------------------------------------------------------

def test_query_without_a_posterior_gets_the_empty_row():
    m = make("oxford")
    lg, ori = logits_case()
    lp = gaussians(3, 6)
    ok_r, ok_s, ok_p = m.postprocess_summary(lg, ori, lp, posterior=True)
    lp[1] = float("-inf")
    rows, summ, post = m.postprocess_summary(lg, ori, lp, posterior=True)
    assert rows[1, 0].item() == -1 and torch.isnan(rows[1, 1])
    assert summ[1, 0].item() == -1 and bool(torch.isnan(summ[1, 1:]).all())
    assert bool((post[1] == 0).all())
    keep = [0, 2]
    eq(rows[keep], ok_r[keep])
    eq_bits(summ[keep], ok_s[keep])
    eq(post[keep], ok_p[keep])
    eq_bits(m.postprocess_summary(lg, ori, lp)[1], summ)
    # the network form: the same rule
    name = "vigor_circ"
    mv = make(name)
    g, s = inputs(name, 2, seed=47)
    lq = gaussians(2, 2)
    ok = mv.localize_summary(g, s, lq, posterior=True)
    lq[0] = float("-inf")
    r, su, p = mv.localize_summary(g, s, lq, posterior=True)
    assert r[0, 0].item() == -1 and su[0, 0].item() == -1 and bool(torch.isnan(su[0, 1:]).all()) and bool((p[0] == 0).all())
    eq(r[1], ok[0][1])
    eq_bits(su[1], ok[1][1])
    eq(p[1], ok[2][1])


# ---- 6. launches and tuning --------------------------------------------------------------------------------------------------------

def test_summary_adds_no_launch_and_measures_nothing():
    lib = _lib.load()
    m = make("oxford")
    g, s = inputs("oxford", 2, seed=17)       # Oxford at batch 2: a shape of the committed tuning table
    lp = gaussians(2, 3)
    sc = m.encode_aerial(s)
    logits, _, ori = m(g, s)[:3]
    m.track_update(g, s, lp)
    m.track_update_cached(g, sc, lp)
    gen = lib.ccvpe_tuning_generation(m._handle)
    pairs = [(lambda: m.localize_summary(g, s, lp), lambda: m.track_update(g, s, lp)),
             (lambda: m.localize_summary(g, s, lp, posterior=True), lambda: m.track_update(g, s, lp)),
             (lambda: m.localize_summary_cached(g, sc, lp, posterior=True), lambda: m.track_update_cached(g, sc, lp)),
             (lambda: m.localize_summary_cached(g, sc, lp, radius=32, tile_index=[1, 0]),
              lambda: m.track_update_cached(g, sc, lp, tile_index=[1, 0])),
             (lambda: m.postprocess_summary(logits, ori, lp, radius=32, posterior=True), lambda: m.track_update_logits(logits, ori, lp)),
             (lambda: m.localize_summary(g, s), lambda: m.track_update(g, s)),
             (lambda: m.localize_summary_cached(g, sc), lambda: m.track_update_cached(g, sc))]

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
    assert lib.ccvpe_tuning_generation(m._handle) == gen      # the summary plans took every tile from the table
    _, post = m.track_update(g, s, lp)
    for r in (0, 8, 32):
        m.belief_summary(post, r)
        assert count(lambda: m.belief_summary(post, r)) == 1


# ---- 7. aerial.Tracker ---------------------------------------------------------------------------------------------------------

def test_tracker_returns_the_summary_of_its_belief():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)             # the six frames of tests/test_track_gpu.py's tracker test
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]
    motion = np.array([61.0, -9.5])
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    plain, with_summary = aerial.Tracker(), aerial.Tracker()
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        rows = plain.step(m, gk, sc, tk, origins, motion, taps, floor)
        assert isinstance(rows, torch.Tensor)
        rows2, summ = with_summary.step(m, gk, sc, tk, origins, motion, taps, floor, summary_radius=8)
        eq(rows2, rows)
        eq(with_summary.belief, plain.belief)
        assert with_summary.origin.tolist() == plain.origin.tolist()
        assert summ.shape == (1, 16)
        eq_bits(summ[:, 0:2], rows[:, 0:2])
        sr.assert_rows_close(summ.cpu().numpy(), m.belief_summary(plain.belief, 8).double().cpu().numpy(), f"tracker frame {k}")
        against_own_map(summ, plain.belief, 8, f"tracker frame {k} (restatement)")
