"""The heading prior on the device: the combined map follows the float32 restatement tests/heading_prior_ref.py bit
for bit away from bin edges; heading_predict follows the float64 restatement within the bound of its structure; a heading measurement
picks the mode of a two-mode posterior; the network forms are the prior forms fed the combined map, cached or not, in micro-batch slices
or not, on one stream or two, for one launch more and without tuning anything; tables that leave no posterior get the special rows; the
tracker filters the heading with the spelled-out calls."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial
from tests import golden_util as gu
from tests import heading_prior_ref as hp
from tests import heading_ref as hr
from tests.test_heading_gpu import eq, eq_bits, field, gaussians, inputs, logit_maps, make, ori_batch

pytestmark = pytest.mark.gpu

N = 512 * 512
BINS = (4, 20, 72, 360)
SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]
FIELD_BATCHES = (("constant", "two_mode", "smooth"), ("constant_wrap", "random", "special"))


def tables(nb, seed=11):
    """float32 [3 kinds][3 queries][nb + 1]: random, random with -inf bins, von Mises"""
    rng = np.random.default_rng(seed + nb)
    rnd = rng.normal(0.0, 3.0, size=(3, nb + 1)).astype(np.float32)
    holes = rng.normal(0.0, 3.0, size=(3, nb + 1)).astype(np.float32)
    holes[:, ::3] = -np.inf
    holes[1, nb] = -np.inf
    vm = aerial.von_mises_heading_log_prior([40.5, 220.5, 359.0], [8.0, 0.5, 50.0], nb)
    return {"random": rnd, "holes": holes, "von_mises": vm}


# ---- 1. the combined map -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", BINS)
def test_combined_map_follows_the_restatement(nb):
    m = make("oxford")
    lp = gaussians(3, 5, sigma=80.0)
    lp_host = lp.cpu().numpy()
    moved = 0
    for names in FIELD_BATCHES:
        ori = ori_batch(names)
        flds = [field(n)[1] for n in names]
        for kind, tb in tables(nb).items():
            t = torch.from_numpy(tb).cuda()
            for prior, prior_host in ((None, None), (lp, lp_host)):
                got = m.heading_prior_map(ori, t, prior)
                assert got.shape == (3, 512, 512) and got.dtype == torch.float32
                eq_bits(got, m.heading_prior_map(ori, t, prior))                      # two calls, the same bits
                g = got.cpu().numpy()
                for q in range(3):
                    moved += hp.assert_map(g[q], flds[q], tb[q], nb, None if prior is None else prior_host[q], f"{names[q]} {kind} nb={nb}")
                    if names[q] == "special" and prior is None:                       # invalid cells carry T[nb] exactly
                        bad = ~flds[q].valid
                        assert bad.sum() > 5000 and hp.same_bits(g[q].reshape(N)[bad], np.full(int(bad.sum()), tb[q, nb], np.float32)).all()
            # one table for every query (stride 0) is the per-query call with that table three times (stride nb + 1)
            eq_bits(m.heading_prior_map(ori, t[1].contiguous(), lp), m.heading_prior_map(ori, t[1:2].expand(3, nb + 1).contiguous(), lp))
    print(f"nb={nb}: {moved} edge cells took the neighbouring bin's value")


# ---- 2. heading_predict ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", (4, 72, 360))
def test_heading_predict_follows_the_restatement(nb):
    m = make("oxford")
    w = 360.0 / nb
    rng = np.random.default_rng(nb)
    h = rng.uniform(0.0, 1.0, size=(3, nb)).astype(np.float32)
    h[1, : nb // 2] = 0.0
    h[2] = 0.0
    h[2, nb - 1] = 1.0                                                               # a spike at the wrap
    h /= h.sum(axis=1, keepdims=True)
    hist = torch.from_numpy(h).cuda()
    turns = (0.0, w, -3.0 * w, 0.5 * w, 0.37 * w, -12.34, 725.0, [0.25 * w, -400.0, 2.0 * w])
    for r in sorted({0, min(3, (nb - 1) // 2), min(32, (nb - 1) // 2)}):
        shared = aerial.gaussian_taps(max(0.6 * r, 0.5), r)
        per_query = aerial.gaussian_taps([0.5 + 0.09 * r, 1.0 + 0.15 * r, 2.0 + 0.3 * r], r)   # (no tap below float32's normal range)
        for turn in turns:
            for taps in (shared, per_query):
                for floor in (1e-3, [0.0, 1e-6, 0.5]):
                    got = m.heading_predict(hist, turn, taps, floor)
                    assert got.shape == (3, nb + 1) and got.dtype == torch.float32
                    hp.assert_predict(got.cpu().numpy(), hp.predict(h, turn, taps, floor), r, f"nb={nb} r={r} turn={turn}")
        a, b = m.heading_predict(hist, turns[-1], per_query, 1e-3), m.heading_predict(hist, turns[-1], per_query, 1e-3)
        eq_bits(a, b)
        # an all-zero hist: logf(floor) in every entry, exactly
        flat = m.heading_predict(torch.zeros(3, nb, device="cuda"), 12.5, shared, [1e-3, 0.25, 1.0]).cpu().numpy()
        want = np.log(np.array([1e-3, 0.25, 1.0], np.float32).astype(np.float64))
        assert (flat == flat[:, :1]).all() and np.abs(flat[:, 0] - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max() and flat[2, 0] == 0.0
        # a NaN turn: the call returns, the other queries are unaffected
        bad = m.heading_predict(hist, [0.25 * w, float("nan"), 2.0 * w], per_query, 1e-3)
        torch.cuda.synchronize()
        eq_bits(bad[[0, 2]], a[[0, 2]])
        inf = m.heading_predict(hist, [float("inf"), -400.0, -3e38], per_query, 1e-3)     # nor does an infinite or a huge one read outside hist
        torch.cuda.synchronize()
        eq_bits(inf[1], a[1])


# ---- 3. the point of the feature ---------------------------------------------------------------------------------------------------

def test_a_heading_measurement_picks_the_mode():
    m = make("oxford")
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    A, Bc = (140, 380), (400, 90)                                                    # (x, y) of the two blobs
    da, db = (xx - A[0]) ** 2 + (yy - A[1]) ** 2, (xx - Bc[0]) ** 2 + (yy - Bc[1]) ** 2
    lg = (12.0 * np.exp(-0.5 * da / 200.0) + 11.5 * np.exp(-0.5 * db / 200.0)).astype(np.float32)
    ori = hr.unit_field(np.where(da < db, 40.5, 220.5))
    table = aerial.von_mises_heading_log_prior(220.5, 8.0, 72)
    # the restatement on the host
    comb, _, edge = hp.combined_map(hr.Field(ori), table, 72)
    assert not edge.any()
    assert int(np.argmax(lg.reshape(N))) == A[1] * 512 + A[0] and int(np.argmax(lg.reshape(N) + comb)) == Bc[1] * 512 + Bc[0]
    logits, field_d, t = torch.from_numpy(lg.reshape(1, N)).cuda(), torch.from_numpy(ori[None]).cuda(), torch.from_numpy(table).cuda()
    zero = torch.zeros(512, 512, device="cuda")
    assert int(m.postprocess_prior(logits, field_d, zero)[0, 0].item()) == A[1] * 512 + A[0]
    cm = m.heading_prior_map(field_d, t)
    rows = m.postprocess_prior(logits, field_d, cm)
    assert int(rows[0, 0].item()) == Bc[1] * 512 + Bc[0] and abs(rows[0, 4].item() - 220.5) < 1e-2
    top = m.postprocess_prior(logits, field_d, cm, k=2, radius=16)                     # the top-K form takes the map as well
    assert top.shape == (1, 2, 5) and int(top[0, 0, 0].item()) == Bc[1] * 512 + Bc[0]
    _, head, hist = m.postprocess_heading(logits, field_d, cm)
    assert int(head[0, 5].item()) == 44 and hist[0, 44].item() > 0.9                  # the mass moved with the argmax


# ---- 4. the network forms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SINGLE)
def test_network_forms_are_the_prior_forms_fed_the_combined_map(name):
    m = make(name)
    g, s = inputs(name, 2)
    lp = gaussians(2, 1)
    t = torch.from_numpy(tables(72)["random"][:2]).cuda()
    t20 = torch.from_numpy(aerial.von_mises_heading_log_prior(123.0, 2.0, 20)).cuda()
    logits, _, ori = m(g, s)[:3]
    sc = m.encode_aerial(s)
    for prior in (lp, None):
        for table, bins, r in ((t, 72, 8), (t20, 360, 32)):                           # nb and the output's bin count are independent
            comb = m.heading_prior_map(ori, table, prior)
            want = m.postprocess_heading(logits, ori, comb, radius=r, bins=bins, summary=True, posterior=True)
            got = m.localize_heading_prior(g, s, table, prior, radius=r, bins=bins, summary=True, posterior=True)
            assert len(got) == 5
            for x, y in zip(got, want):
                eq_bits(x, y)
            short = m.localize_heading_prior(g, s, table, prior, radius=r, bins=bins)
            assert len(short) == 3
            for x, y in zip(short, want[:3]):
                eq_bits(x, y)
            for tiles in (None, [0, 1]):
                for x, y in zip(m.localize_heading_prior_cached(g, sc, table, prior, radius=r, bins=bins, tile_index=tiles), want[:3]):
                    eq_bits(x, y)
    # an all-zero table (the last entry included) is no prior at all
    z = torch.zeros(73, device="cuda")
    for x, y in zip(m.localize_heading_prior(g, s, z, lp, summary=True, posterior=True), m.localize_heading(g, s, lp, summary=True, posterior=True)):
        eq_bits(x, y)
    for x, y in zip(m.localize_heading_prior(g, s, z), m.localize_heading(g, s)):
        eq_bits(x, y)


def test_micro_batch_slices_read_their_own_tables():
    name = "vigor_prior180_circ"
    m2 = make(name, micro_batch=2)
    g, s = inputs(name, 3, seed=53)
    lp = gaussians(3, 4, sigma=3.0)
    t = torch.from_numpy(tables(72)["von_mises"]).cuda()
    for prior in (lp, None):
        out = m2.localize_heading_prior(g, s, t, prior, radius=8, bins=20, summary=True, posterior=True)
        for sl in (slice(0, 2), slice(2, 3)):
            part = m2.localize_heading_prior(g[sl], s[sl], t[sl].contiguous(), None if prior is None else prior[sl].contiguous(), radius=8,
                                             bins=20, summary=True, posterior=True)
            for x, y in zip(out, part):
                eq_bits(x[sl], y)
        assert not torch.equal(out[2][0], out[2][1])
    shared = m2.localize_heading_prior(g, s, t[1].contiguous(), lp, bins=20)          # one table: every slice reads the same one
    for x, y in zip(shared, m2.localize_heading_prior(g, s, t[1:2].expand(3, 73).contiguous(), lp, bins=20)):
        eq_bits(x, y)


def test_one_stream_one_launch_more_and_nothing_tuned():
    lib = _lib.load()
    m = make("oxford")
    g, s = inputs("oxford", 2, seed=17)       # Oxford at batch 2: a shape of the committed tuning table
    lp = gaussians(2, 3)
    t = torch.from_numpy(tables(72)["von_mises"][:2]).cuda()
    sc = m.encode_aerial(s)
    m.localize_heading(g, s, lp)
    m.localize_heading_cached(g, sc, lp)
    gen = lib.ccvpe_tuning_generation(m._handle)

    def count(fn):
        fn()                          # plans and lazy kernel attributes exist before anything is counted
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for a, b in ((lambda: m.localize_heading_prior(g, s, t, lp, summary=True), lambda: m.localize_heading(g, s, lp, summary=True)),
                 (lambda: m.localize_heading_prior(g, s, t, lp), lambda: m.localize_heading(g, s, lp)),
                 (lambda: m.localize_heading_prior_cached(g, sc, t, lp, posterior=True, tile_index=[1, 0]),
                  lambda: m.localize_heading_cached(g, sc, lp, posterior=True, tile_index=[1, 0]))):
        assert count(a) == count(b) + 1
    logits, _, ori = m(g, s)[:3]
    assert count(lambda: m.heading_prior_map(ori, t, lp)) == 1 and count(lambda: m.heading_prior_map(ori, t)) == 1
    assert count(lambda: m.heading_predict(torch.rand(2, 72, device="cuda"), [1.0, 2.0], aerial.gaussian_taps(2.0, 6), [1e-3, 1e-3])) == 1
    assert lib.ccvpe_tuning_generation(m._handle) == gen      # the heading-prior plans took every tile from the table
    two = m.localize_heading_prior(g, s, t, lp, summary=True, posterior=True)
    two_c = m.localize_heading_prior_cached(g, sc, t, lp, summary=True, posterior=True)
    m.set_streams(1)
    try:
        for x, y in zip(m.localize_heading_prior(g, s, t, lp, summary=True, posterior=True), two):
            eq_bits(x, y)
        for x, y in zip(m.localize_heading_prior_cached(g, sc, t, lp, summary=True, posterior=True), two_c):
            eq_bits(x, y)
    finally:
        m.set_streams(2)
    assert lib.ccvpe_tuning_generation(m._handle) == gen


# ---- 5. no posterior -----------------------------------------------------------------------------------------------------------

def test_tables_that_leave_no_posterior():
    m = make("oxford")
    g, s = inputs("oxford", 3, seed=29)
    lp = gaussians(3, 6)
    good = torch.from_numpy(tables(72)["random"]).cuda()
    ok = m.localize_heading_prior(g, s, good, lp, summary=True, posterior=True)
    logits, _, ori = m(g, s)[:3]
    fld = hr.Field(ori[1].cpu().numpy())
    used = int(np.bincount(fld.bins(72)[0][fld.valid], minlength=72).argmax())        # a bin cells of query 1 use: the fullest
    for kind in ("-inf", "nan", "+inf"):
        bad = good.clone()
        if kind == "-inf":
            bad[1] = float("-inf")
        else:
            bad[1, used] = float(kind)
        rows, head, hist, summ, post = m.localize_heading_prior(g, s, bad, lp, summary=True, posterior=True)
        assert rows[1, 0].item() == -1 and bool(torch.isnan(rows[1, 1]))              # (-1, NaN, the orientation of a cell of the map)
        assert head[1, 5].item() == -1 and bool(torch.isnan(head[1, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]]).all())
        assert bool((hist[1] == 0).all()) and bool((post[1] == 0).all()) and summ[1, 0].item() == -1
        for q in (0, 2):                                                             # the neighbours keep their bits
            for x, y in zip((rows, head, hist, summ, post), ok):
                eq_bits(x[q], y[q])
        for x, y in zip(m.postprocess_heading(logits, ori, m.heading_prior_map(ori, bad, lp), summary=True, posterior=True),
                        (rows, head, hist, summ, post)):
            eq_bits(x, y)
        for x, y in zip(m.localize_heading_prior(g, s, good, lp, summary=True, posterior=True), ok):       # the next call is unaffected
            eq_bits(x, y)


# ---- 6. aerial.Tracker ---------------------------------------------------------------------------------------------------------

def test_tracker_filters_the_heading():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)             # the six frames of tests/test_track_gpu.py's tracker test
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]
    motion = np.array([61.0, -9.5])
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    hk = dict(heading_bins=72, heading_turn_deg=0.0, heading_taps=aerial.gaussian_taps(2.0, 6), heading_floor=1e-3)
    old, defaults, filt = aerial.Tracker(), aerial.Tracker(), aerial.Tracker()
    last_hist = None
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        prior = None if filt.belief is None else m.track_predict(filt.belief, aerial.oxford_track_shift(filt.origin, origins[tk], motion),
                                                                 taps, floor)
        rows, head, hist = filt.step(m, gk, sc, tk, origins, motion, taps, floor, **hk)
        if k == 0:                                   # the first step has no heading prior: the run without the new arguments
            want = m.localize_heading_cached(gk, sc, None, radius=8, bins=72, posterior=True, tile_index=tk)
        else:                                        # later steps: the spelled-out calls
            table = m.heading_predict(last_hist, 0.0, hk["heading_taps"], 1e-3)
            want = m.localize_heading_prior_cached(gk, sc, table, prior, radius=8, bins=72, posterior=True, tile_index=tk)
        eq(rows, want[0])
        eq_bits(head, want[1])
        eq_bits(hist, want[2])
        eq(filt.belief, want[3])
        eq_bits(filt.hist, hist)
        last_hist = hist
        # with the arguments left out, today's run
        a = old.step(m, gk, sc, tk, origins, motion, taps, floor, heading_bins=72)
        b_prior = None if k == 0 else prior_old
        w = m.localize_heading_cached(gk, sc, b_prior, radius=8, bins=72, posterior=True, tile_index=tk)
        for x, y in zip(a, w[:3]):
            eq_bits(x, y)
        eq(old.belief, w[3])
        prior_old = None if k == F - 1 else m.track_predict(old.belief, aerial.oxford_track_shift(old.origin, origins[[tile[k + 1]]], motion),
                                                            taps, floor)
        d = defaults.step(m, gk, sc, tk, origins, motion, taps, floor, heading_bins=72, heading_turn_deg=None, heading_taps=None,
                          heading_floor=None)
        for x, y in zip(d, a):
            eq_bits(x, y)
        if k == 0:
            for x, y in zip((rows, head, hist), a):
                eq_bits(x, y)
    assert old.hist is None and defaults.hist is None
    # the affine tracker runs the same filter on its own update forms
    aff = aerial.AffineTracker()
    M = aerial.rigid_matrix(0.0, (0.0, 0.0))
    r0 = aff.step(m, g[:1], s[:1], M, taps, floor, **hk)
    prior = m.track_predict_affine(aff.belief, M, taps, floor)
    table = m.heading_predict(r0[2], 0.0, hk["heading_taps"], 1e-3)
    r1 = aff.step(m, g[1:2], s[:1], M, taps, floor, **hk)
    want = m.localize_heading_prior(g[1:2], s[:1], table, prior, radius=8, bins=72, posterior=True)
    for x, y in zip(r1, want[:3]):
        eq_bits(x, y)
    eq(aff.belief, want[3])
