"""Localize with a position prior (ccvpe_localize_prior, ccvpe_localize_prior_cached_indexed, ccvpe_postprocess_prior,
ccvpe_localize_region_prior): a zero prior gives the bits of the forms without one, the pose-only forms give the bits of forward +
postprocess_prior, the rows follow the numpy restatement tests/prior_ref.py on the forward's logits, and a mask moves the answer."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu
from tests import prior_ref, region_ref

pytestmark = pytest.mark.gpu

N = 512 * 512
SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]
EMPTY = torch.tensor([-1.0, 0.0, 0.0, 0.0, 0.0])


def make(name, **kw):
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
    return m.to("cuda").eval()


def inputs(name, batch, seed=7):
    cfg = gu.CONFIGS[name]
    g, s = weights.generate_inputs(cfg["variant"], batch, seed, cfg["fov"])
    return torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()


def gaussians(B, seed, sigma=60.0):
    """one Gaussian log-prior per query, different centres"""
    c = np.random.default_rng(seed).uniform(60, 452, size=(B, 2))
    return aerial.gaussian_log_prior(c, sigma, "cuda")


def eq(a, b):
    assert a.shape == b.shape and torch.equal(a, b), (a - b).abs().max().item()


def eq_nan(a, b):
    """bit-equal except that NaN matches NaN (the probability of a query without a posterior)"""
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def zero_checks(m, g, s):
    B = g.shape[0]
    for z in (torch.zeros(512, 512, device="cuda"), torch.zeros(B, 512, 512, device="cuda")):   # stride 0 and 512*512
        eq(m.localize_prior(g, s, z), m.localize(g, s))
        eq(m.localize_prior(g, s, z, k=8, radius=16), m.localize_topk(g, s, 8, 16))


# ---- 1. zero prior: the bits of the forms without a prior ---------------------------------------------------------------------

@pytest.mark.parametrize("name", SINGLE)
def test_zero_prior_is_bitwise_the_plain_forms(name):
    m = make(name)
    g, s = inputs(name, 2)
    zero_checks(m, g, s)


def test_zero_prior_bf16x3():
    m = make("vigor_prior180_circ", precision="bf16x3")
    g, s = inputs("vigor_prior180_circ", 2, seed=29)
    zero_checks(m, g, s)


def test_zero_prior_cached_indexed_and_region_oxford():
    m = make("oxford")
    g, s = inputs("oxford", 3, seed=17)
    sc = m.encode_aerial(s)
    tiles = [2, 0, 2]
    z = torch.zeros(512, 512, device="cuda")
    eq(m.localize_prior_cached(g, sc, z), m.localize_cached(g, sc))
    eq(m.localize_prior_cached(g, sc, z, tile_index=tiles), m.localize_cached(g, sc, tile_index=tiles))
    eq(m.localize_prior_cached(g, sc, z, 8, 16, tile_index=tiles), m.localize_topk_cached(g, sc, 8, 16, tile_index=tiles))
    eq(m.localize_prior_cached(g, sc, torch.zeros(3, 1, 512, 512, device="cuda"), 8, 16), m.localize_topk_cached(g, sc, 8, 16))
    gc = m.encode_ground(g)
    lists = [[1], [0, 2, 1], [2, 0]]
    ref = m.localize_region(gc, sc, lists)
    for zz in (z, torch.zeros(6, 512, 512, device="cuda")):
        got = m.localize_region_prior(gc, sc, lists, zz)
        for k in ("rows", "pair", "pair_rows", "pair_stats", "tile_prob"):
            eq(got[k], ref[k])
        np.testing.assert_array_equal(got["pair_tile"], ref["pair_tile"])


# ---- 2, 3, 4. pose-only forms against post-processing, the numpy restatement, a window mask ------------------------------------------

def test_pose_only_equals_forward_plus_postprocess_and_prior_ref():
    name = "vigor_prior180_circ"
    m = make(name)
    g, s = inputs(name, 3, seed=41)
    lp = gaussians(3, 1)
    logits, _, ori = m(g, s)[:3]
    for k, r in ((0, 0), (8, 16)):
        eq(m.localize_prior(g, s, lp, k, r), m.postprocess_prior(logits, ori, lp, k, r))
    rows = m.localize_prior(g, s, lp).cpu().numpy()
    lg, o, p = logits.cpu().numpy(), ori.cpu().numpy(), lp.cpu().numpy().reshape(3, N)
    want, margin = prior_ref.argmax_rows(lg, o, p)
    assert (want[:, 0] >= 0).all()
    for b in range(3):
        if margin[b] > 1e-6:
            assert rows[b, 0] == want[b, 0], (b, rows[b], want[b])
        i = int(rows[b, 0])
        h = prior_ref.posterior(lg[b:b + 1], p[b])["h"][0]
        assert abs(rows[b, 1] - h[i]) <= 1e-5 * h[i]
        np.testing.assert_array_equal(rows[b, 2:4], o[b, :, i // 512, i % 512])
    # the cached form on the same tiles
    sc = m.encode_aerial(s)
    lc, _, oc = m.forward_cached(g, sc)[:3]
    eq(m.localize_prior_cached(g, sc, lp), m.postprocess_prior(lc, oc, lp))
    eq(m.localize_prior_cached(g, sc, lp, 8, 16, tile_index=[0, 1, 2]), m.postprocess_prior(lc, oc, lp, 8, 16))


def test_window_mask_moves_every_hypothesis_inside():
    name = "kitti"
    m = make(name)
    g, s = inputs(name, 2, seed=43)
    free = m.localize(g, s)
    lp = torch.full((2, 512, 512), float("-inf"), device="cuda")
    box = []
    for b in range(2):
        y, x = divmod(int(free[b, 0].item()), 512)
        y0 = 300 if y < 256 else 60          # a 96 x 96 box away from the unconstrained argmax
        x0 = 300 if x < 256 else 60
        lp[b, y0:y0 + 96, x0:x0 + 96] = 0.0
        box.append((y0, x0))
    inside = lambda i, b: box[b][0] <= i // 512 < box[b][0] + 96 and box[b][1] <= i % 512 < box[b][1] + 96
    rows = m.localize_prior(g, s, lp)
    top = m.localize_prior(g, s, lp, 8, 4)
    for b in range(2):
        assert not inside(int(free[b, 0].item()), b)
        assert inside(int(rows[b, 0].item()), b)
        assert rows[b, 1].item() > 0
        idx = [int(v) for v in top[b, :, 0].tolist()]
        assert idx[0] == int(rows[b, 0].item()) and all(inside(i, b) for i in idx if i >= 0), idx
    # the numpy restatement agrees on the masked posterior
    logits, _, ori = m(g, s)[:3]
    want, margin = prior_ref.argmax_rows(logits.cpu().numpy(), ori.cpu().numpy(), lp.cpu().numpy().reshape(2, N))
    for b in range(2):
        if margin[b] > 1e-6:
            assert int(rows[b, 0].item()) == int(want[b, 0])


# ---- 5. a query without a finite posterior ---------------------------------------------------------------------------------------

def test_query_without_a_posterior():
    name = "vigor_circ"
    m = make(name)
    g, s = inputs(name, 4, seed=47)
    lp = gaussians(4, 2)
    ok = m.localize_prior(g, s, lp)
    ok_top = m.localize_prior(g, s, lp, 8, 16)
    lp[2] = float("-inf")
    rows = m.localize_prior(g, s, lp)
    top = m.localize_prior(g, s, lp, 8, 16)
    assert rows[2, 0].item() == -1 and torch.isnan(rows[2, 1])
    eq(top[2].cpu(), EMPTY.expand(8, 5))
    keep = [0, 1, 3]
    eq(rows[keep], ok[keep])
    eq(top[keep], ok_top[keep])
    logits, _, ori = m(g, s)[:3]
    eq_nan(m.postprocess_prior(logits, ori, lp), rows)
    eq(m.postprocess_prior(logits, ori, lp, 8, 16), top)
    # +inf anywhere and NaN: no finite posterior either, and the other queries keep their rows
    lp[2] = 0.0
    lp[2, 7, 9] = float("inf")
    lp[1, 100, 200] = float("nan")
    rows = m.localize_prior(g, s, lp)
    assert rows[1, 0].item() == -1 and rows[2, 0].item() == -1 and torch.isnan(rows[1:3, 1]).all()
    eq(rows[[0, 3]], ok[[0, 3]])


# ---- 6. shared and micro-batched priors --------------------------------------------------------------------------------------------

def test_shared_prior_and_micro_batch_slices():
    """stride 0 is the map repeated; a micro_batch=2 handle reads each slice's own maps (its rows are forward + postprocess_prior on
    that handle, and agree with the default handle wherever the posterior has no near-tie)"""
    name = "vigor_prior180_circ"
    m = make(name)
    g, s = inputs(name, 5, seed=53)
    one = gaussians(1, 3, sigma=40.0)
    eq(m.localize_prior(g, s, one), m.localize_prior(g, s, one.expand(5, 512, 512).contiguous()))
    eq(m.localize_prior(g, s, one[0], 8, 16), m.localize_prior(g, s, one.expand(5, 512, 512).contiguous(), 8, 16))
    lp = gaussians(5, 4, sigma=3.0)   # sharp and far apart: each query's argmax follows its own map
    m2 = make(name, micro_batch=2)    # slices of 2, 2, 1
    logits, _, ori = m2(g, s)[:3]
    for k, r in ((0, 0), (8, 16)):
        got = m2.localize_prior(g, s, lp, k, r)
        eq(got, m2.postprocess_prior(logits, ori, lp, k, r))
    got = m2.localize_prior(g, s, lp)
    ref = m.localize_prior(g, s, lp)
    logits, _, ori = m(g, s)[:3]
    _, margin = prior_ref.argmax_rows(logits.cpu().numpy(), ori.cpu().numpy(), lp.cpu().numpy().reshape(5, N))
    sure = torch.as_tensor(margin > 1e-5)
    assert sure.sum() >= 3, margin
    eq(got[sure, 0], ref[sure, 0])
    assert ((got[sure, 1] - ref[sure, 1]).abs() <= 1e-4 * ref[sure, 1]).all()


# ---- 7. the region form -----------------------------------------------------------------------------------------------------------

def test_region_prior_pairs_and_reduction():
    m = make("oxford")
    g, s = inputs("oxford", 3, seed=59)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    tiles = [2, 0, 1]
    lp3 = gaussians(3, 5, sigma=50.0)
    r = m.localize_region_prior(gc, sc, [[t] for t in tiles], lp3)
    eq(r["pair_rows"], m.localize_prior_cached(g, sc, lp3, tile_index=tiles))
    lists = [[1], [0, 2, 1], [2, 0]]
    off = np.array([0, 1, 4, 6], np.int32)
    ft = np.concatenate([np.asarray(t, np.int32) for t in lists])
    qop = region_ref.query_of_pair(off)
    lp = gaussians(6, 6, sigma=80.0)
    r = m.localize_region_prior(gc, sc, lists, lp)
    # one pair per query of the ground cache gathered in torch (the documented [G][Ltot] layout): the same per-pair bits
    gq = gc.view(3, -1)[torch.as_tensor(qop, dtype=torch.int64, device="cuda")].reshape(-1).contiguous()
    gq._ccvpe_batch, gq._ccvpe_grd_hw = 6, gc._ccvpe_grd_hw
    one = m.localize_region_prior(gq, sc, [[t] for t in ft], lp)
    eq(r["pair_rows"], one["pair_rows"])
    eq(r["pair_stats"], one["pair_stats"])
    # the posterior statistics against the forward's logits, and the reduction against its numpy restatement
    logits = m.forward_cached(g[torch.as_tensor(qop).cuda()], sc, tile_index=ft)[0].cpu().numpy()
    post = prior_ref.posterior(logits, lp.cpu().numpy().reshape(6, N))
    st = r["pair_stats"].double().cpu().numpy()
    assert np.abs(st[:, 0] - post["m"]).max() <= 1e-4 * np.abs(post["m"]).max()
    assert np.abs(st[:, 1] - post["inv"]).max() <= 1e-4 * np.abs(post["inv"]).max()
    want = region_ref.region_reduce(off, r["pair_stats"].cpu().numpy(), r["pair_rows"].cpu().numpy())
    sure = want["margin"] > 1e-6
    assert sure.sum() >= 2, want["margin"]
    np.testing.assert_array_equal(r["pair"].cpu().numpy()[sure], want["best_pair"][sure])
    rows = r["rows"].cpu().numpy()
    np.testing.assert_allclose(rows[sure, 1], want["rows"][sure, 1], rtol=1e-6)
    np.testing.assert_array_equal(rows[sure][:, [0, 2, 3, 4]], want["rows"][sure][:, [0, 2, 3, 4]])
    np.testing.assert_allclose(r["tile_prob"].cpu().numpy(), want["tile_prob"], rtol=1e-6)
    # a pair without a posterior carries no mass and never wins
    lp[1] = float("-inf")
    r2 = m.localize_region_prior(gc, sc, lists, lp)
    assert r2["tile_prob"][1].item() == 0 and int(r2["pair"][1].item()) != 1 and r2["pair_rows"][1, 0].item() == -1


# ---- 8. the committed tuning table covers the prior calls ----------------------------------------------------------------------------

def test_headline_batch32_measures_nothing(monkeypatch):
    monkeypatch.setenv("CCVPE_TUNE_CACHE", "off")
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 32, seed=11)
    rows = m.localize_prior(g, s, gaussians(32, 7))
    torch.cuda.synchronize()
    assert _lib.load().ccvpe_tuning_generation(m._handle) == 0, "a launch missed the tuning table and was measured"
    assert bool(((rows[:, 0] >= 0) & (rows[:, 0] < N)).all())
