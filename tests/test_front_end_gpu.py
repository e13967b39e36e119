"""The Python front end on the device: what every form returns - a tuple or a bare tensor, how many, each one's shape,
dtype and device - against a table written out here, over every combination of the optional outputs; the image, cached and
held-outputs forms of one family byte for byte; and the two trackers, which share their update step, against each other over their
option matrix.  Oxford variant, its ground size and seeded weights as tests/test_track_gpu.py, batch 2, no autotuning."""
import itertools

import numpy as np
import pytest
import torch

from ccvpe_amd import aerial, models, weights

pytestmark = pytest.mark.gpu

F32, U8 = torch.float32, torch.uint8
BINS, LEVELS, K = 36, (0.5, 0.9), 3

# ---- the table: a (shape, dtype) pair is a bare tensor, a list of them a tuple of that arity ------------------------------------------
ROWS, TOPK, MAP = ((2, 5), F32), ((2, 3, 5), F32), ((2, 512, 512), F32)
SUMM, HEAD, HIST = ((2, 16), F32), ((2, 12), F32), ((2, 36), F32)
CRED, LMAP = ((2, 10), F32), ((2, 512, 512), U8)
HEADING = {(False, False): [ROWS, HEAD, HIST], (True, False): [ROWS, HEAD, HIST, SUMM],            # (summary, posterior)
           (False, True): [ROWS, HEAD, HIST, MAP], (True, True): [ROWS, HEAD, HIST, SUMM, MAP]}
EXPECT = {
    "forward": {(): [((2, 512 * 512), F32), ((2, 1, 512, 512), F32), ((2, 2, 512, 512), F32), ((2, 20, 8, 8), F32), ((2, 20, 16, 16), F32),
                     ((2, 20, 32, 32), F32), ((2, 20, 64, 64), F32), ((2, 20, 128, 128), F32), ((2, 20, 256, 256), F32)]},   # Oxford: 20 rolls
    "localize": {(): ROWS},
    "topk": {(): TOPK},
    "prior": {(0,): ROWS, (3,): TOPK},                                                                                # (k,)
    "update": {(False,): [ROWS, MAP], (True,): [ROWS, MAP]},                                                          # (with a prior,)
    "summary": {(False,): [ROWS, SUMM], (True,): [ROWS, SUMM, MAP]},                                                  # (posterior,)
    "heading": HEADING,
    "heading_prior": HEADING,
    "credible": {(False, False): [ROWS, CRED], (True, False): [ROWS, CRED, LMAP],                                     # (level_map, posterior)
                 (False, True): [ROWS, CRED, MAP], (True, True): [ROWS, CRED, LMAP, MAP]},
    "belief_summary": {(): SUMM},
    "belief_credible": {(False,): CRED, (True,): [CRED, LMAP]},                                                       # (level_map,)
}
# a tracker step by (summary_radius given, heading_bins given, credible_levels given)
CRED_T = ((2, 10), F32)
STEP = {(False, False, False): ROWS, (True, False, False): [ROWS, SUMM], (False, True, False): [ROWS, HEAD, HIST],
        (True, True, False): [ROWS, SUMM, HEAD, HIST], (False, False, True): [ROWS, CRED_T], (True, False, True): [ROWS, SUMM, CRED_T],
        (False, True, True): [ROWS, HEAD, HIST, CRED_T], (True, True, True): [ROWS, SUMM, HEAD, HIST, CRED_T]}


def check_structure(got, want, what, device):
    if isinstance(want, list):
        assert type(got) is tuple and len(got) == len(want), (what, type(got), len(got) if isinstance(got, tuple) else None)
    else:
        assert isinstance(got, torch.Tensor), (what, type(got))
        got, want = (got,), [want]
    for i, (t, (shape, dtype)) in enumerate(zip(got, want)):
        assert isinstance(t, torch.Tensor) and t.device == device and t.dtype == dtype, (what, i, t.dtype, t.device)
        assert tuple(t.shape) == shape, (what, i, tuple(t.shape), shape)


def same_bytes(a, b, what):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, i)


class Ctx:
    pass


@pytest.fixture(scope="module")
def c():
    """the model and one set of seeded inputs, the forward's outputs among them: computed once, shared, never written to"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CCVPE_AUTOTUNE", "0")          # read when the handle is created, which the forward below does
        c = Ctx()
        c.m = models.CVM_OxfordRobotCar("cuda")
        c.m.load_state_dict(weights.generate_state_dict("oxford", 0))
        c.m = c.m.to("cuda").eval()
        g, s = weights.generate_inputs("oxford", 2, 7, 360.0)
        c.g, c.s = torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()
        c.fwd = c.m(c.g, c.s)
    c.lg, c.heat, c.ori = c.fwd[:3]
    c.sc = c.m.encode_aerial(c.s)
    centres = np.random.default_rng(1).uniform(60, 452, size=(2, 2))
    c.lp = aerial.gaussian_log_prior(centres, 60.0, "cuda")
    c.tb = torch.from_numpy(aerial.von_mises_heading_log_prior([40.0, 200.0], 2.0, 24)).cuda()
    c.probe = [512 * 100 + 7, 512 * 300 + 300]
    return c


def sides(c, family, opt):
    """every side's call of one family under one combination of options -> {side: result}"""
    m, g, s, sc, lg, heat, ori, lp, tb = c.m, c.g, c.s, c.sc, c.lg, c.heat, c.ori, c.lp, c.tb
    idx = [0, 1]
    if family == "forward":
        return {"image": m(g, s), "cached": m.forward_cached(g, sc), "indexed": m.forward_cached(g, sc, idx)}
    if family == "localize":
        return {"image": m.localize(g, s), "cached": m.localize_cached(g, sc), "indexed": m.localize_cached(g, sc, idx),
                "held": m.postprocess_rows(heat, ori)}
    if family == "topk":
        return {"image": m.localize_topk(g, s, K, 8), "cached": m.localize_topk_cached(g, sc, K, 8),
                "indexed": m.localize_topk_cached(g, sc, K, 8, idx), "held": m.postprocess_topk(heat, ori, K, 8)}
    if family == "prior":
        k, r = opt[0], 8 if opt[0] else 0
        return {"image": m.localize_prior(g, s, lp, k, r), "cached": m.localize_prior_cached(g, sc, lp, k, r),
                "indexed": m.localize_prior_cached(g, sc, lp, k, r, tile_index=idx), "held": m.postprocess_prior(lg, ori, lp, k, r)}
    if family == "update":
        p = lp if opt[0] else None
        return {"image": m.track_update(g, s, p), "cached": m.track_update_cached(g, sc, p),
                "indexed": m.track_update_cached(g, sc, p, tile_index=idx), "held": m.track_update_logits(lg, ori, p)}
    if family == "summary":
        kw = dict(radius=8, posterior=opt[0])
        return {"image": m.localize_summary(g, s, lp, **kw), "cached": m.localize_summary_cached(g, sc, lp, **kw),
                "indexed": m.localize_summary_cached(g, sc, lp, tile_index=idx, **kw), "held": m.postprocess_summary(lg, ori, lp, **kw)}
    if family == "heading":
        kw = dict(radius=8, bins=BINS, summary=opt[0], posterior=opt[1])
        return {"image": m.localize_heading(g, s, lp, **kw), "cached": m.localize_heading_cached(g, sc, lp, **kw),
                "indexed": m.localize_heading_cached(g, sc, lp, tile_index=idx, **kw), "held": m.postprocess_heading(lg, ori, lp, **kw)}
    if family == "heading_prior":
        kw = dict(radius=8, bins=BINS, summary=opt[0], posterior=opt[1])
        return {"image": m.localize_heading_prior(g, s, tb, lp, **kw), "cached": m.localize_heading_prior_cached(g, sc, tb, lp, **kw),
                "indexed": m.localize_heading_prior_cached(g, sc, tb, lp, tile_index=idx, **kw),
                "held": m.postprocess_heading(lg, ori, m.heading_prior_map(ori, tb, lp), **kw)}
    if family == "credible":
        kw = dict(log_prior=lp, probe=c.probe, level_map=opt[0], posterior=opt[1])
        return {"image": m.localize_credible(g, s, LEVELS, **kw), "cached": m.localize_credible_cached(g, sc, LEVELS, **kw),
                "indexed": m.localize_credible_cached(g, sc, LEVELS, tile_index=idx, **kw),
                "held": m.postprocess_credible(lg, ori, LEVELS, **kw)}
    if family == "belief_summary":
        return {"stored": m.belief_summary(heat, 8), "stored3": m.belief_summary(heat.view(2, 512, 512), 8)}
    if family == "belief_credible":
        return {"stored": m.belief_credible(heat, LEVELS, c.probe, level_map=opt[0])}
    raise KeyError(family)


@pytest.mark.parametrize("family", sorted(EXPECT))
def test_every_form_returns_what_the_table_says(c, family):
    for opt, want in EXPECT[family].items():
        got = sides(c, family, opt)
        first = None
        for side, res in got.items():
            check_structure(res, want, (family, opt, side), c.g.device)
            if first is None:
                first = res
            else:
                same_bytes(first, res, (family, opt, side))
    if family == "forward":
        same_bytes(c.fwd, sides(c, family, ())["image"], "forward twice")
    if family == "credible":      # cred and the level map are belief_credible's on the posterior the form returns
        rows, cred, lmap, post = c.m.localize_credible(c.g, c.s, LEVELS, c.lp, c.probe, level_map=True, posterior=True)
        same_bytes((cred, lmap), c.m.belief_credible(post, LEVELS, c.probe, level_map=True), "credible on its own posterior")


def test_an_option_changes_no_shared_result(c):
    """asking for one more output leaves the others' bytes alone: the full combination holds every smaller one"""
    m, g, s, lp = c.m, c.g, c.s, c.lp
    full = m.localize_heading(g, s, lp, radius=8, bins=BINS, summary=True, posterior=True)
    same_bytes(m.localize_heading(g, s, lp, radius=8, bins=BINS), full[:3], "heading bare")
    same_bytes(m.localize_summary(g, s, lp, radius=8, posterior=True), (full[0], full[3], full[4]), "summary")
    same_bytes(m.track_update(g, s, lp), (full[0], full[4]), "update")
    same_bytes(m.localize_prior(g, s, lp), full[0], "prior")
    cred = m.localize_credible(g, s, LEVELS, lp, c.probe, level_map=True, posterior=True)
    same_bytes(m.localize_credible(g, s, LEVELS, lp, c.probe), cred[:2], "credible bare")
    same_bytes((cred[0], cred[3]), (full[0], full[4]), "credible's rows and posterior")


# ---- the trackers -------------------------------------------------------------------------------------------------------------------

HEADING_OPTIONS = {"none": {}, "bins": dict(heading_bins=BINS),
                   "filter": dict(heading_bins=BINS, heading_turn_deg=10.0, heading_taps=aerial.gaussian_taps(2.0, 6), heading_floor=1e-3)}


@pytest.mark.parametrize("summary,heading,credible", list(itertools.product((False, True), sorted(HEADING_OPTIONS), (False, True))))
def test_both_trackers_take_the_same_step(c, summary, heading, credible):
    """two frames at an integer shift, where track_predict_affine under rigid_matrix(0, shift) is track_predict bit for bit"""
    m = c.m
    kw = dict(HEADING_OPTIONS[heading])
    if summary:
        kw["summary_radius"] = 8
    if credible:
        kw["credible_levels"] = LEVELS
    want = STEP[(summary, heading != "none", credible)]
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    origins, motion = np.array([[800, 400], [800, 400]]), np.array([25.0, -50.0])           # 25, -50 map pixels = 16, -32 output pixels
    shift = aerial.oxford_track_shift(origins, origins, motion)
    assert shift.tolist() == [[16.0, -32.0]] * 2
    matrix = aerial.rigid_matrix(0, shift)
    frames = [c.g, torch.roll(c.g, 37, dims=3)]
    a, b, d = aerial.Tracker(), aerial.AffineTracker(), aerial.AffineTracker()
    for k, g in enumerate(frames):
        ra = a.step(m, g, c.sc, [0, 1], origins, motion, taps, floor, **kw)
        rb = b.step(m, g, None, matrix, taps, floor, cache=c.sc, tile_index=[0, 1], **kw)
        rd = d.step(m, g, c.s, matrix, taps, floor, **kw)
        for who, res in (("Tracker", ra), ("AffineTracker cached", rb), ("AffineTracker sat", rd)):
            check_structure(res, want, (who, k, summary, heading, credible), c.g.device)
        same_bytes(ra, rb, ("Tracker / AffineTracker", k))
        same_bytes(rb, rd, ("AffineTracker cached / sat", k))
        same_bytes(a.belief, b.belief, ("belief", k))
        same_bytes(b.belief, d.belief, ("belief, sat", k))
        for t in (a, b, d):
            assert (t.hist is not None) == (heading == "filter")
        if heading == "filter":
            same_bytes(a.hist, b.hist, ("hist", k))
            same_bytes(ra[-2 if credible else -1], a.hist, ("the kept hist is the returned one", k))
    if not (summary or credible or heading != "none"):      # the plain step spelled out once: predict, then update
        lp = m.track_predict(m.track_update_cached(frames[0], c.sc, None, tile_index=[0, 1])[1], shift, taps, floor)
        same_bytes(ra, m.track_update_cached(frames[1], c.sc, lp, tile_index=[0, 1])[0], "Tracker is predict plus update")
