"""The heading posterior on the device (ccvpe_*_heading): the logits form follows the float64 restatement
tests/heading_ref.py, taken of the posterior map the same call returned, within the bounds the number formats give
(heading_ref.assert_close) on crafted fields at every bin count and radius, with and without a prior; the same call gives the same bits
twice, and the rows, summary and map of postprocess_summary; a query without a posterior and a field without a valid cell get their
special rows; the network forms give the rows of the prior forms and the heading of the logits form over the full forward's outputs,
cached or not, in micro-batch slices or not; nothing is tuned and the heading is one launch; aerial.Tracker passes it through."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu
from tests import heading_ref as hr

pytestmark = pytest.mark.gpu

N = 512 * 512
BINS = (4, 20, 72, 360)
RADII = (0, 8, 32)
SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]
FIELD_BATCHES = {"a": ("constant", "random", "special"), "b": ("two_mode", "smooth", "constant_wrap")}
_MODELS = {}
_FIELDS = {}


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


def field(name):
    """(float32 [2, 512, 512], its heading_ref.Field), made once"""
    if not _FIELDS:
        _FIELDS.update({k: (v, hr.Field(v)) for k, v in hr.crafted_fields().items()})
    return _FIELDS[name]


def logit_maps():
    """three different logit maps without a network: noise; noise with a sharp peak near the border; a broad blob with a second one"""
    rng = np.random.default_rng(19)
    lg = rng.normal(0.0, 2.0, size=(3, 512, 512)).astype(np.float32)
    lg[1, 3, 500] += 30.0
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    lg[2] = 12.0 * np.exp(-0.5 * ((xx - 140) ** 2 + (yy - 380) ** 2) / 400.0) + 11.0 * np.exp(-0.5 * ((xx - 400) ** 2 + (yy - 90) ** 2) / 100.0)
    return torch.from_numpy(lg.reshape(3, N)).cuda()


def ori_batch(names):
    return torch.from_numpy(np.stack([field(n)[0] for n in names])).cuda()


def against_own_map(head, hist, post, fields, bins, radius, what):
    """heading and hist against the restatement of the map the same call returned"""
    hd, hs, pm = head.cpu().numpy(), hist.cpu().numpy(), post.cpu().numpy()
    for q, fld in enumerate(fields):
        hr.assert_close(hd[q], hs[q], hr.heading(pm[q], fld, bins, radius), f"{what} query {q}")


# ---- 1. the logits form against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("prior", (False, True))
@pytest.mark.parametrize("batch", sorted(FIELD_BATCHES))
def test_logits_form_follows_the_restatement(batch, prior):
    m = make("oxford")
    names = FIELD_BATCHES[batch]
    lg, ori = logit_maps(), ori_batch(names)
    lp = gaussians(3, 5, sigma=80.0) if prior else None
    flds = [field(n)[1] for n in names]
    first = None
    for bins in BINS:
        for r in RADII:
            rows, head, hist, post = m.postprocess_heading(lg, ori, lp, radius=r, bins=bins, posterior=True)
            assert rows.shape == (3, 5) and head.shape == (3, 12) and hist.shape == (3, bins) and post.shape == (3, 512, 512)
            assert head.dtype == torch.float32 and hist.dtype == torch.float32
            if first is None:
                first = post
            eq(post, first)                            # one map whatever is asked of it
            against_own_map(head, hist, post, flds, bins, r, f"{names} prior={prior} bins={bins} r={r}")


# ---- 2. the same bits from call to call, and the summary forms' other outputs ------------------------------------------------------

def test_same_bits_twice_and_the_outputs_of_the_summary_form():
    m = make("oxford")
    lg = logit_maps()
    lp = gaussians(3, 5, sigma=80.0)
    for names in FIELD_BATCHES.values():
        ori = ori_batch(names)
        for prior in (lp, None):
            for bins, r in ((72, 8), (360, 32), (4, 0)):
                a = m.postprocess_heading(lg, ori, prior, radius=r, bins=bins, summary=True, posterior=True)
                b = m.postprocess_heading(lg, ori, prior, radius=r, bins=bins, summary=True, posterior=True)
                assert len(a) == 5
                for x, y in zip(a, b):
                    eq_bits(x, y)
                rows, summ, post = m.postprocess_summary(lg, ori, prior, radius=r, posterior=True)
                eq(a[0], rows)
                eq_bits(a[3], summ)
                eq(a[4], post)
                c = m.postprocess_heading(lg, ori, prior, radius=r, bins=bins)            # without the optional outputs: the same bits
                assert len(c) == 3
                eq(c[0], rows)
                eq_bits(c[1], a[1])
                eq_bits(c[2], a[2])
                d = m.postprocess_heading(lg, ori, prior, radius=r, bins=bins, summary=True)
                assert len(d) == 4
                eq_bits(d[3], summ)
    # the defaults are radius 8 and 72 bins; a shared prior map is read by every query
    ori = ori_batch(FIELD_BATCHES["a"])
    eq_bits(m.postprocess_heading(lg, ori)[1], m.postprocess_heading(lg, ori, None, radius=8, bins=72)[1])
    one = lp[:1].contiguous()
    for x, y in zip(m.postprocess_heading(lg, ori, one[0]), m.postprocess_heading(lg, ori, one.expand(3, 512, 512).contiguous())):
        eq_bits(x, y)


# ---- 3. special rows ---------------------------------------------------------------------------------------------------------------

def test_query_without_a_posterior_and_field_without_a_valid_cell():
    m = make("oxford")
    lg = logit_maps()
    names = FIELD_BATCHES["a"]
    ori = ori_batch(names)
    lp = gaussians(3, 6)
    ok = m.postprocess_heading(lg, ori, lp, posterior=True)
    for poison in (float("-inf"), float("nan")):
        bad = lp.clone()
        bad[1] = poison
        rows, head, hist, post = m.postprocess_heading(lg, ori, bad, posterior=True)
        assert rows[1, 0].item() == -1 and torch.isnan(rows[1, 1])
        assert head[1, 5].item() == -1 and bool(torch.isnan(head[1, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]]).all())
        assert bool((hist[1] == 0).all()) and bool((post[1] == 0).all())
        hr.assert_close(head[1].cpu().numpy(), hist[1].cpu().numpy(), hr.heading(None, field(names[1])[1], 72, 8, ok=False), "no posterior")
        for k in (0, 2):
            for x, y in zip((rows, head, hist, post), ok):
                eq_bits(x[k], y[k])
        for x, y in zip(m.postprocess_heading(lg, ori, bad, posterior=True), (rows, head, hist, post)):    # and the bins are back at zero
            eq_bits(x, y)
    # a field without a valid cell under a finite posterior: M == 0, the ratios NaN, hist zero, mode 0
    dead = ori.clone()
    dead[0] = 0.0
    dead[2] = float("nan")
    rows, head, hist, post = m.postprocess_heading(lg, dead, lp, radius=32, bins=20, posterior=True)
    eq(rows[:, :2], ok[0][:, :2])
    for q in (0, 2):
        assert head[q, 0].item() == 0 and head[q, 7].item() == 0 and head[q, 5].item() == 0
        assert bool(torch.isnan(head[q, [1, 2, 3, 4, 6, 8, 9, 10, 11]]).all()) and bool((hist[q] == 0).all())
    against_own_map(head, hist, post, [hr.Field(f) for f in dead.cpu().numpy()], 20, 32, "dead fields")


# ---- 4. the network forms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SINGLE)
def test_network_forms_are_the_prior_forms_rows_plus_the_heading_of_the_full_forward(name):
    m = make(name)
    g, s = inputs(name, 2)
    lp = gaussians(2, 1)
    logits, _, ori = m(g, s)[:3]
    rows, head, hist, summ, post = m.localize_heading(g, s, lp, radius=8, bins=72, summary=True, posterior=True)
    eq(rows, m.localize_prior(g, s, lp))
    want = m.postprocess_heading(logits, ori, lp, radius=8, bins=72, summary=True, posterior=True)
    for x, y in zip((rows, head, hist, summ, post), want):
        eq_bits(x, y)
    r2, s2, p2 = m.localize_summary(g, s, lp, radius=8, posterior=True)
    eq(rows, r2)
    eq_bits(summ, s2)
    eq(post, p2)
    against_own_map(head, hist, post, [hr.Field(f) for f in ori.cpu().numpy()], 72, 8, f"{name} full")
    r0, h0, c0 = m.localize_heading(g, s, radius=32, bins=360)                       # no prior, no optional output
    eq(r0, m.localize(g, s))
    w0 = m.postprocess_heading(logits, ori, radius=32, bins=360)
    eq_bits(h0, w0[1])
    eq_bits(c0, w0[2])
    sc = m.encode_aerial(s)
    for tiles in (None, [0, 1]):
        r1, h1, c1 = m.localize_heading_cached(g, sc, lp, radius=8, bins=72, tile_index=tiles)
        eq(r1, rows)
        eq_bits(h1, head)
        eq_bits(c1, hist)
    r3, h3, c3 = m.localize_heading_cached(g, sc, lp, radius=8, bins=72, tile_index=[1, 1])
    eq(r3, m.localize_prior_cached(g, sc, lp, tile_index=[1, 1]))
    eq_bits(h3[1], head[1])                                                           # query 1 on its own tile, as before
    eq_bits(c3[1], hist[1])


def test_micro_batch_slices_write_their_own_headings():
    """a micro_batch=2 handle runs three queries as slices of 2 + 1: every slice reads its own prior and field and writes its own rows,
    heading, hist, summary and map - the bits of the same handle's calls on the two slices (whose forms the test above holds to the
    restatement)"""
    name = "vigor_prior180_circ"
    m2 = make(name, micro_batch=2)
    g, s = inputs(name, 3, seed=53)
    lp = gaussians(3, 4, sigma=3.0)
    for prior in (lp, None):
        out = m2.localize_heading(g, s, prior, radius=8, bins=20, summary=True, posterior=True)
        for sl in (slice(0, 2), slice(2, 3)):
            part = m2.localize_heading(g[sl], s[sl], None if prior is None else prior[sl].contiguous(), radius=8, bins=20, summary=True,
                                       posterior=True)
            for x, y in zip(out, part):
                eq_bits(x[sl], y)
        assert bool((out[2].sum(dim=1) - out[1][:, 0]).abs().max() <= 2.0 ** -22)


# ---- 5. launches and tuning --------------------------------------------------------------------------------------------------------

def test_heading_is_one_launch_and_measures_nothing():
    lib = _lib.load()
    m = make("oxford")
    g, s = inputs("oxford", 2, seed=17)       # Oxford at batch 2: a shape of the committed tuning table
    lp = gaussians(2, 3)
    sc = m.encode_aerial(s)
    logits, _, ori = m(g, s)[:3]
    m.localize_summary(g, s, lp)
    m.localize_summary_cached(g, sc, lp)
    gen = lib.ccvpe_tuning_generation(m._handle)

    def count(fn):
        fn()                          # plans and lazy kernel attributes exist before anything is counted
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for bins, r in ((72, 8), (360, 32), (4, 0)):
        assert count(lambda: m.postprocess_heading(logits, ori, lp, radius=r, bins=bins, summary=True, posterior=True)) == \
            count(lambda: m.postprocess_summary(logits, ori, lp, radius=r, posterior=True)) + 1
    assert count(lambda: m.postprocess_heading(logits, ori)) == count(lambda: m.postprocess_summary(logits, ori)) + 1
    # the pose plans: pose.heading, and - with the fused level 1 - the whole-field launch and the gather in place of the one-tile launch
    for a, b in ((lambda: m.localize_heading(g, s, lp, summary=True), lambda: m.localize_summary(g, s, lp)),
                 (lambda: m.localize_heading(g, s), lambda: m.localize(g, s)),
                 (lambda: m.localize_heading_cached(g, sc, lp, posterior=True, tile_index=[1, 0]),
                  lambda: m.localize_summary_cached(g, sc, lp, posterior=True, tile_index=[1, 0]))):
        assert count(a) - count(b) in (1, 2)
    assert lib.ccvpe_tuning_generation(m._handle) == gen      # the heading plans took every tile from the table


# ---- 6. aerial.Tracker ---------------------------------------------------------------------------------------------------------

def test_tracker_returns_the_heading_of_its_belief():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)             # the six frames of tests/test_track_gpu.py's tracker test
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]
    motion = np.array([61.0, -9.5])
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    plain, with_heading, with_both = aerial.Tracker(), aerial.Tracker(), aerial.Tracker()
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        prior = None if plain.belief is None else m.track_predict(plain.belief, aerial.oxford_track_shift(plain.origin, origins[tk], motion),
                                                                  taps, floor)
        rows = plain.step(m, gk, sc, tk, origins, motion, taps, floor)
        assert isinstance(rows, torch.Tensor)
        rows2, head, hist = with_heading.step(m, gk, sc, tk, origins, motion, taps, floor, heading_bins=72)
        eq(rows2, rows)
        eq(with_heading.belief, plain.belief)
        assert with_heading.origin.tolist() == plain.origin.tolist()
        assert head.shape == (1, 12) and hist.shape == (1, 72)
        want = m.localize_heading_cached(gk, sc, prior, radius=8, bins=72, tile_index=tk)      # the spelled-out call
        eq(rows, want[0])
        eq_bits(head, want[1])
        eq_bits(hist, want[2])
        rows3, summ, head3, hist3 = with_both.step(m, gk, sc, tk, origins, motion, taps, floor, summary_radius=1, heading_bins=20)
        eq(rows3, rows)
        eq(with_both.belief, plain.belief)
        want = m.localize_heading_cached(gk, sc, prior, radius=1, bins=20, summary=True, tile_index=tk)
        eq_bits(summ, want[3])
        eq_bits(head3, want[1])
        eq_bits(hist3, want[2])
