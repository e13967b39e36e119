"""One poisoned query does not move its batch neighbours.

Workgroups of many kernels straddle samples on purpose (row tiles over 35-row samples, squeeze-excite tickets, the level-6 grouped
GEMM, lanes past the image that work on the last pixel) and some mask by multiplying with zero.  A read of a neighbour's data that is
then multiplied by 0 or lands in a padded lane is invisible to every finite-valued test and turns NaN the moment one query of a batch
is bad.  Here every case runs the clean batch, the batch with sample j replaced by poison, and the clean batch again: every output of
every sample != j is torch.equal to the clean run (forward is deterministic run to run, so no tolerance), and the second clean run
equals the first.  A call that returned did return 0: the Python wrapper raises on any other code.

Poisons: the ground image of j all NaN, the aerial image of j all NaN, the ground image of j at 3e38 (finite, overflows on the way).
The poisoned query's own results follow DESIGN.md 2.3: whatever its maps hold, the pose forms answer what the post-processing forms
answer on the forward's outputs (NaN matching NaN), and a query without a finite posterior gets the empty row of its form."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial
from tests import degenerate_ref as dr
from tests import golden_util as gu
from tests import region_ref
from tests.test_parity_gpu import build_model, inputs
from tests.test_topk_gpu import device_angle

pytestmark = pytest.mark.gpu

N = 512 * 512
POISONS = ("ground_nan", "aerial_nan", "ground_3e38")
K, R, RADIUS, BINS = 5, 4, 8, 72
POSE_CONFIG = "vigor_prior180_circ"


@pytest.fixture(scope="module")
def handles():
    """one model per (configuration, precision) for the whole file"""
    cache = {}

    def get(name, precision="fp32"):
        if (name, precision) not in cache:
            cache[name, precision] = build_model(gu.CONFIGS[name], precision=precision)
        return cache[name, precision]
    yield get
    cache.clear()


def poison(g, s, j, kind):
    g, s = g.clone(), s.clone()
    if kind == "ground_nan":
        g[j] = float("nan")
    elif kind == "aerial_nan":
        s[j] = float("nan")
    else:
        g[j] = 3e38
    return g, s


def positions(B):
    return [0, 13, 31] if B == 32 else sorted({0, B // 2, B - 1})


def neighbours_equal(clean, bad, j, what):
    for k, (c, p) in enumerate(zip(clean, bad)):
        keep = [b for b in range(c.shape[0]) if b != j]
        assert c.shape == p.shape and torch.equal(c[keep], p[keep]), \
            f"{what}: output {k} of samples {[b for b in keep if not torch.equal(c[b], p[b])]} moved when sample {j} was poisoned"


def all_equal(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: output {k}"


def equal_nan(a, b, what):
    """the same values, NaN in the same places (two NaNs may differ in sign and payload)"""
    for k, (x, y) in enumerate(zip(a, b)):
        nx, ny = torch.isnan(x), torch.isnan(y)
        assert x.shape == y.shape and torch.equal(nx, ny) and torch.equal(x[~nx], y[~ny]), f"{what}: output {k}"


# ---- 1. the full forward, nine outputs ------------------------------------------------------------------------------------------
# the six configurations at the batches of tests/test_stages_gpu.py (those it runs at batch 1 alone: at 2), one in bf16x3, and the two
# batch-32 plans: F(4x4) persistent tiles, the tail split, tickets that straddle samples, the composed level 6
FORWARD_CASES = [("oxford", 3, "fp32"), ("kitti", 2, "fp32"), ("vigor_circ", 2, "fp32"), ("vigor_prior72_fov108", 2, "fp32"),
                 ("vigor_prior180_circ", 4, "fp32"), ("vigor_prior180_b2", 2, "fp32"), ("vigor_prior180_circ", 4, "bf16x3"),
                 ("vigor_prior180_circ", 32, "fp32"), ("kitti", 32, "fp32")]


@pytest.mark.parametrize("name,batch,precision", FORWARD_CASES)
def test_forward_neighbours_keep_their_bits(handles, name, batch, precision):
    m = handles(name, precision)
    g, s = inputs(gu.CONFIGS[name], batch)
    clean = m(g, s)
    assert len(clean) == 9 and all(bool(torch.isfinite(t).all()) for t in clean)
    for kind in POISONS:
        for j in positions(batch):
            bad = m(*poison(g, s, j, kind))
            neighbours_equal(clean, bad, j, f"{name} batch {batch} {precision} {kind}")
            print(f"{name} batch {batch} {precision} {kind} sample {j}: outputs of the poisoned query that are not all finite: "
                  f"{[n for n, t in zip(gu.OUTPUT_NAMES, bad) if not bool(torch.isfinite(t[j]).all())]}")
    all_equal(m(g, s), clean, f"{name} batch {batch} {precision}: the clean batch afterwards")


# ---- 2. the pose forms ------------------------------------------------------------------------------------------------------------
def priors(B, seed=1):
    c = np.random.default_rng(seed).uniform(60, 452, size=(B, 2))
    return aerial.gaussian_log_prior(c, 60.0, "cuda")


POSE_FORMS = {
    # name: (the pose-only form on images, the same results from forward outputs the caller holds)
    "localize": (lambda m, g, s, lp: (m.localize(g, s),),
                 lambda m, lg, heat, ori, lp: (m.postprocess_rows(heat, ori),)),
    "localize_prior": (lambda m, g, s, lp: (m.localize_prior(g, s, lp),),
                       lambda m, lg, heat, ori, lp: (m.postprocess_prior(lg, ori, lp),)),
    "localize_topk": (lambda m, g, s, lp: (m.localize_topk(g, s, K, R),),
                      lambda m, lg, heat, ori, lp: (m.postprocess_topk(heat, ori, K, R),)),
    "localize_summary": (lambda m, g, s, lp: tuple(m.localize_summary(g, s, lp, radius=RADIUS, posterior=True)),
                         lambda m, lg, heat, ori, lp: tuple(m.postprocess_summary(lg, ori, lp, radius=RADIUS, posterior=True))),
    "localize_heading": (lambda m, g, s, lp: tuple(m.localize_heading(g, s, lp, radius=RADIUS, bins=BINS, summary=True, posterior=True)),
                         lambda m, lg, heat, ori, lp: tuple(m.postprocess_heading(lg, ori, lp, radius=RADIUS, bins=BINS, summary=True,
                                                                                 posterior=True))),
    "track_update": (lambda m, g, s, lp: tuple(m.track_update(g, s, lp)),
                     lambda m, lg, heat, ori, lp: tuple(m.track_update_logits(lg, ori, lp))),
}


def assert_empty(form, out, j):
    """the results of query j of a pose form without a finite posterior"""
    rows = out[0][j].cpu().numpy()
    if form == "localize_topk":
        np.testing.assert_array_equal(rows, np.tile(np.array([-1, 0, 0, 0, 0], np.float32), (K, 1)))
        return
    assert rows[0] == -1 and np.isnan(rows[1]), (form, rows)
    if form == "localize_summary":
        summ, post = out[1][j].cpu().numpy(), out[2][j]
        assert summ[0] == -1 and np.isnan(summ[1:]).all() and bool((post == 0).all()), (form, summ)
    elif form == "localize_heading":
        head, hist, summ, post = out[1][j].cpu().numpy(), out[2][j], out[3][j].cpu().numpy(), out[4][j]
        assert head[5] == -1 and np.isnan(np.delete(head, 5)).all() and bool((hist == 0).all()), (form, head)
        assert summ[0] == -1 and np.isnan(summ[1:]).all() and bool((post == 0).all()), (form, summ)
    elif form == "track_update":
        assert bool((out[1][j] == 0).all()), form


@pytest.mark.parametrize("form", list(POSE_FORMS))
def test_pose_forms_neighbours_keep_their_bits_and_the_poisoned_row_follows_the_rule(handles, form):
    m = handles(POSE_CONFIG)
    B = 4
    g, s = inputs(gu.CONFIGS[POSE_CONFIG], B)
    lp = priors(B)
    pose, post = POSE_FORMS[form]
    clean = pose(m, g, s, lp)
    takes_prior = form not in ("localize", "localize_topk")
    reached = 0                                                        # cases that met a query without a finite posterior
    for kind in POISONS + (("prior_neg_inf",) if takes_prior else ()):
        for j in positions(B):
            gp, sp = (g, s) if kind == "prior_neg_inf" else poison(g, s, j, kind)
            lq = lp
            if kind == "prior_neg_inf":                                 # the images are clean, query j's prior excludes every pixel
                lq = lp.clone()
                lq[j] = float("-inf")
            bad = pose(m, gp, sp, lq)
            neighbours_equal(clean, bad, j, f"{form} {kind}")
            # every sample, the poisoned one included: the form on the forward's outputs answers the same
            lg, heat, ori = m(gp, sp)[:3]
            equal_nan(bad, post(m, lg, heat, ori, lq), f"{form} {kind} sample {j} against the forward's outputs")
            no_posterior = kind == "prior_neg_inf" or bool(torch.isnan(heat[j]).any())   # (one bad logit leaves the whole map NaN)
            print(f"{form} {kind} sample {j}: {'no' if no_posterior else 'a'} finite posterior")
            if no_posterior:
                assert_empty(form, bad, j)
                reached += 1
            if form == "localize":                                      # and the row is the restatement's on that map
                want = dr.rows_ref(heat[j:j + 1].cpu().numpy(), ori[j:j + 1].cpu().numpy(), angle=device_angle)
                equal_nan((bad[0][j:j + 1].cpu(),), (torch.from_numpy(want),), f"{form} {kind} sample {j} against the restatement")
    all_equal(pose(m, g, s, lp), clean, f"{form}: the clean batch afterwards")
    if takes_prior:
        assert reached >= len(positions(B)), "no case reached a query without a finite posterior: the empty-row assertions did not run"
    if form == "localize":
        reached += plain_pose_tail_on_bad_logits(m, g, s, clean)
        assert reached >= 3 * len(positions(B)), "no case reached a query without a finite posterior: the empty-row assertions did not run"


def plain_pose_tail_on_bad_logits(m, g, s, clean):
    """No image drives a query's logits non-finite: every decoder level ends in a ReLU that is a maximum on the device and returns 0 for a
    NaN, and an overflow heals the same way (ground and aerial images scaled or filled with 1e20 .. 1e38.5 and +inf, and single pixels,
    all gave finite logits on this configuration).  So the empty row of the plain pose plan - pose_argmax_kernel without prior,
    posterior or summary, which only ccvpe_localize* launches - is driven through the kernel-level hook ccvpe_op_pose_rows, the launches
    ccvpe_localize runs behind its decoders, on the forward's own logits with one query made bad: the rows are those of localize on the
    clean logits, and with a bad query those postprocess_rows gives on the forward's heatmap with that query's map all NaN (what the
    softmax stores for such logits), for every sample.  Returns the number of cases that met the empty row."""
    lg, heat, ori = m(g, s)[:3]
    all_equal((_lib.op_pose_rows(m._handle, lg, ori),), clean, "the hook on the forward's logits against localize")
    n = 0
    for j in positions(lg.shape[0]):
        for what in ("nan", "inf", "all_neg_inf"):
            lg2, heat2 = lg.clone(), heat.clone()
            if what == "all_neg_inf":
                lg2[j] = float("-inf")
            else:
                lg2[j, 777 + 4099 * j] = float(what)
            heat2[j] = float("nan")
            rows = (_lib.op_pose_rows(m._handle, lg2, ori),)
            equal_nan(rows, (m.postprocess_rows(heat2, ori),), f"plain pose tail, {what} in query {j}, against postprocess_rows")
            neighbours_equal(clean, rows, j, f"plain pose tail, {what} in query {j}")
            assert_empty("localize", rows, j)
            n += 1
    all_equal((_lib.op_pose_rows(m._handle, lg, ori),), clean, "the hook on the clean logits afterwards")
    return n


# ---- 3. cached and indexed forms ----------------------------------------------------------------------------------------------------
CACHED_FORMS = {
    "forward_cached": (lambda m, g, sc, ti, lp: tuple(m.forward_cached(g, sc, tile_index=ti)), None),
    "localize_cached": (lambda m, g, sc, ti, lp: (m.localize_cached(g, sc, tile_index=ti),),
                        lambda m, lg, heat, ori, lp: (m.postprocess_rows(heat, ori),)),
    "track_update_cached": (lambda m, g, sc, ti, lp: tuple(m.track_update_cached(g, sc, lp, tile_index=ti)),
                            lambda m, lg, heat, ori, lp: tuple(m.track_update_logits(lg, ori, lp))),
}
TILE_INDEX = [0, 1, 2, 1]


@pytest.mark.parametrize("form", list(CACHED_FORMS))
def test_cached_forms_one_bad_tile_then_one_bad_query(handles, form):
    m = handles(POSE_CONFIG)
    B = 4
    g, s = inputs(gu.CONFIGS[POSE_CONFIG], B)
    lp = priors(B, seed=2)
    run, post = CACHED_FORMS[form]
    sc = m.encode_aerial(s[:3])
    sbad = s[:3].clone()
    sbad[1] = float("nan")
    sc_bad = m.encode_aerial(sbad)
    clean = run(m, g, sc, TILE_INDEX, lp)
    bad = run(m, g, sc_bad, TILE_INDEX, lp)
    hit = [b for b, t in enumerate(TILE_INDEX) if t == 1]
    for k, (c, p) in enumerate(zip(clean, bad)):
        keep = [b for b in range(B) if b not in hit]
        assert torch.equal(c[keep], p[keep]), f"{form}: output {k} of a query on a clean tile moved when another tile was poisoned"
    if post is not None:
        lg, heat, ori = m.forward_cached(g, sc_bad, tile_index=TILE_INDEX)[:3]
        equal_nan(bad, post(m, lg, heat, ori, lp), f"{form} bad tile against the forward's outputs")
        for j in hit:
            if bool(torch.isnan(heat[j]).any()):
                assert_empty("track_update" if form == "track_update_cached" else "localize", bad, j)
    # one poisoned query against clean tiles
    for kind in ("ground_nan", "ground_3e38"):
        for j in positions(B):
            gp, _ = poison(g, s, j, kind)
            out = run(m, gp, sc, TILE_INDEX, lp)
            neighbours_equal(clean, out, j, f"{form} {kind}")
            if post is not None:
                lg, heat, ori = m.forward_cached(gp, sc, tile_index=TILE_INDEX)[:3]
                equal_nan(out, post(m, lg, heat, ori, lp), f"{form} {kind} sample {j} against the forward's outputs")
                if bool(torch.isnan(heat[j]).any()):
                    assert_empty("track_update" if form == "track_update_cached" else "localize", out, j)
    all_equal(run(m, g, sc, TILE_INDEX, lp), clean, f"{form}: the clean call afterwards")


# ---- 4. localize_region ---------------------------------------------------------------------------------------------------------------
def test_region_one_bad_tile(handles):
    """query 0 over three tiles, one of them encoded from a NaN image; query 1 over the two clean ones in the same call"""
    from tests.test_region_gpu import flat
    m = handles(POSE_CONFIG)
    g, s = inputs(gu.CONFIGS[POSE_CONFIG], 3)
    gc = m.encode_ground(g[:2])
    sc = m.encode_aerial(s)
    sbad = s.clone()
    sbad[1] = float("nan")
    sc_bad = m.encode_aerial(sbad)
    tiles = [[0, 1, 2], [0, 2]]
    off, _ = flat(tiles)
    clean = m.localize_region(gc, sc, tiles)
    bad = m.localize_region(gc, sc_bad, tiles)
    # the clean query, and the clean pairs of the other one
    assert torch.equal(bad["rows"][1], clean["rows"][1]) and bad["pair"][1] == clean["pair"][1]
    for p in (0, 2, 3, 4):
        for k in ("pair_rows", "pair_stats"):
            assert torch.equal(bad[k][p], clean[k][p]), (k, p)
    assert torch.equal(bad["tile_prob"][3:5], clean["tile_prob"][3:5])
    # the query with the bad tile: the reduction's restatement on the device's own pair statistics
    stats, pr = bad["pair_stats"].cpu().numpy(), bad["pair_rows"].cpu().numpy()
    want = region_ref.region_reduce(off, stats, pr)
    print(f"pair statistics {stats.tolist()}, pair rows {pr[:, :2].tolist()}, margin {want['margin']}")
    assert (want["margin"] > 1e-6).all(), want["margin"]
    np.testing.assert_array_equal(bad["pair"].cpu().numpy(), want["best_pair"])
    rows = bad["rows"].cpu().numpy()
    np.testing.assert_allclose(rows[:, 1], want["rows"][:, 1], rtol=1e-6)
    np.testing.assert_array_equal(rows[:, [0, 2, 3, 4]], want["rows"][:, [0, 2, 3, 4]])
    np.testing.assert_allclose(bad["tile_prob"].cpu().numpy(), want["tile_prob"], rtol=1e-6)
    if not np.isfinite(stats[1]).all():          # the pair without a finite posterior: the empty row, no share of the mass
        assert pr[1, 0] == -1 and np.isnan(pr[1, 1]) and bad["tile_prob"][1].item() == 0
    again = m.localize_region(gc, sc, tiles)
    for k in ("rows", "pair", "pair_rows", "pair_stats", "tile_prob"):
        assert torch.equal(again[k], clean[k]), k
