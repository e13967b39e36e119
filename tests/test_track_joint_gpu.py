"""The joint position-heading filter on the device (ccvpe_track_joint_predict, ccvpe_track_joint_update_logits)
against the float64 restatement tests/joint_ref.py fed the float32 inputs the device got.

Predict.  All terms are non-negative, so the bound is relative, u = 2^-24:
    A = the xy pass                              ccvpe_track_predict's count (tests/test_track_gpu.py)                  4r + 12
    M[d] = fmaf(f, th, (1 - f) * th)             1 - f, the product, the fused multiply-add                             + 3
    C = 2 rh + 2 fused multiply-adds             one rounding each                                                      + 2rh + 2
    prior = C + floor                            the add                                                                + 1
so prior is within (4 r + 2 rh + 18) u of the restatement; the tests allow twice that wherever the restatement is >= 2^-100 and
below that ask for a small value that is not NaN.  (f: the kernel takes it at k = 0, the restatement per k; for the turns of these
tests the two differ by less than 2^-44 relative, far below u.)

Update.  The tolerance is measured, as the issue sets it: E = the largest relative error of ccvpe_track_update_logits' posterior
(no prior) against the float64 softmax of the same logits - the error of __expf and of the float32 normaliser -, plus the four
roundings the joint adds (w * E, * prior, (float)(1 / Z), U * inv): joint within 2 (E + 4 u); marginal and hist within
2 (E + 4 u + (nb + 1) u) (nb adds, one rounding).  The heading bins are the device's own (ccvpe_heading_prior_map of the table
0..nb reads them out; they are checked against the float64 bins away from the bin edges), so a cell within 1e-3 degree of an edge
does not move mass between bins of the two sides."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu
from tests import heading_ref as hr
from tests import joint_ref as jr
from tests import track_ref

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
TINY = 2.0 ** -100
_BASE = {}


def base():
    """one model, one forward of three queries and its float64 softmax, shared by the tests (and left unchanged)"""
    if not _BASE:
        cfg = gu.CONFIGS["oxford"]
        m = models.CVM_OxfordRobotCar("cuda")
        m.load_state_dict(weights.generate_state_dict(cfg["variant"], cfg["seed"]))
        m = m.to("cuda").eval()
        g, s = weights.generate_inputs(cfg["variant"], 3, 11, cfg["fov"])
        logits, heat, ori = m(torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda())[:3]
        lg = logits.double().cpu().numpy()
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        soft = e / e.sum(axis=1, keepdims=True)
        _, post = m.track_update_logits(logits, ori, None)
        got = post.double().cpu().numpy().reshape(3, N)
        big = soft >= TINY
        E = float((np.abs(got - soft)[big] / soft[big]).max())
        print(f"track_update_logits against the float64 softmax: worst relative error {E:.3e} = {E / EPS:.2f} u")
        _BASE.update(m=m, logits=logits, ori=ori, heat=heat.view(3, 512, 512), soft=soft, E=E)
    return _BASE


def eq(a, b):
    assert a.shape == b.shape and torch.equal(a, b), (a.double() - b.double()).abs().max().item()


def eq_nan(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def rel_check(got, ref, bound, what):
    """|got - ref| <= bound * ref wherever ref >= 2^-100; below that got <= 2^-99; no NaN.  Prints worst error over bound."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert not np.isnan(got).any(), what
    big = ref >= TINY
    worst = float((np.abs(got - ref)[big] / (bound * ref[big])).max()) if big.any() else 0.0
    print(f"{what}: {int(big.sum())} values checked, worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    assert (np.abs(got[~big]) <= 2.0 ** -99).all(), what


# ---- 1. predict against the restatement -----------------------------------------------------------------------------------------------

SHIFTS = [(0.0, 0.0), (12.0, -7.0), (3.37, 0.81), (-130.6, 200.2), (-0.5, -0.5), (530.0, 0.0), (100.0, -600.5), (5.5, 5.5), (-3.0, 0.25)]


def predict_inputs(nb):
    """three queries: deltas at the corners and the centre in different bins; a uniform joint; a forward's heatmap split over the bins"""
    rng = np.random.default_rng(nb)
    j = np.zeros((3, nb, 512, 512), np.float32)
    j[0, 0, 0, 0], j[0, nb - 1, 511, 511], j[0, nb // 2, 255, 256] = 0.5, 0.25, 0.25
    j[1] = 1.0 / (N * nb)
    split = rng.dirichlet(np.ones(nb)).astype(np.float32)
    j[2] = base()["heat"][0].cpu().numpy()[None] * split[:, None, None]
    shift = np.array([[SHIFTS[(3 * b + k) % len(SHIFTS)] for k in range(nb)] for b in range(3)], np.float32)
    return j, shift


@pytest.mark.parametrize("nb,r,rh", [(4, 0, 0), (8, 1, 1), (6, 8, 2), (8, 8, 0)])
def test_predict_follows_the_float64_restatement(nb, r, rh):
    m = base()["m"]
    j, shift = predict_inputs(nb)
    dev = torch.from_numpy(j).cuda()
    w = 360.0 / nb
    taps = aerial.gaussian_taps(1.0 + 0.3 * r, r)
    th = aerial.gaussian_taps(0.8, rh)
    bound = 2 * (4 * r + 2 * rh + 18) * EPS
    # shared taps; turns 0, an exact bin multiple, a fraction; floor 0 and positive
    turn, floor = np.array([0.0, 2 * w, 7.3], np.float32), np.array([0.0, 1e-9, 1e-3], np.float32)
    got = m.track_joint_predict(dev, shift, taps, floor, turn, th)
    assert got.shape == (3, nb, 512, 512) and got.dtype == torch.float32
    rel_check(got.cpu().numpy(), jr.predict(j, shift, taps, turn, th, floor), bound, f"nb {nb} r {r} rh {rh} shared taps")
    # per-query taps on both axes; turns negative, across the wrap, more than a full circle; one floor for all
    turn = np.array([-33.0, 359.5, -400.25], np.float32)
    taps = aerial.gaussian_taps(np.array([0.6, 1.5, 3.0]), r)
    th = aerial.gaussian_taps(np.array([0.5, 1.0, 2.0]), rh)
    out = torch.empty_like(dev)
    got = m.track_joint_predict(dev, torch.from_numpy(shift).cuda(), taps, 1e-12, turn, th, out=out)
    assert got is out
    rel_check(got.cpu().numpy(), jr.predict(j, shift, taps, turn, th, 1e-12), bound, f"nb {nb} r {r} rh {rh} per-query taps")


def test_predict_is_exact_where_exactness_is_defined():
    """integer shifts and a whole-bin turn move a delta to exactly one (bin, cell) with exactly its value; a zero joint gives the floor"""
    m = base()["m"]
    nb = 6
    j = np.zeros((2, nb, 512, 512), np.float32)
    j[0, 2, 50, 40] = 0.75
    shift = np.zeros((2, nb, 2), np.float32)
    shift[0, 2] = (7, -3)
    shift[0, 3] = (100, 100)
    got = m.track_joint_predict(torch.from_numpy(j).cuda(), shift, [1.0], [0.0, 0.25], [120.0, 77.0], [1.0])
    assert got[0, 4, 47, 47].item() == 0.75 and got[0].sum().item() == 0.75
    assert bool((got[1] == 0.25).all())
    lib = _lib.load()
    torch.cuda.synchronize()
    n0 = lib.ccvpe_launch_count()
    m.track_joint_predict(torch.from_numpy(j).cuda(), shift, [1.0], 0.0, 0.0, [1.0])
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 2


# ---- 2. update against the restatement ------------------------------------------------------------------------------------------------

def device_bins(m, ori, nb):
    """the heading bin of every cell as the device computes it (nb: no heading), checked against the float64 bins away from the edges"""
    table = torch.arange(nb + 1, dtype=torch.float32, device="cuda")
    got = m.heading_prior_map(ori, table).cpu().numpy().reshape(-1, N).astype(np.int64)
    o = ori.cpu().numpy().reshape(-1, 2, N)
    for b in range(o.shape[0]):
        fld = hr.Field(o[b])
        k, edge = fld.bins(nb)
        want = np.where(fld.valid, k, nb)
        off = (edge < 0) | ~fld.valid
        assert (got[b][off] == want[off]).all()
        assert (~off).mean() <= hr.EDGE_CAP
    return got


def poisoned_field():
    """the forward's field of two queries with stretches of cells without a heading: (0, 0) and NaN"""
    ori = base()["ori"][:2].clone()
    ori[0, :, 100:110, :] = 0.0
    ori[1, 0, 200:205, 17:300] = float("nan")
    ori[1, 1, 300:303, :] = float("inf")
    return ori


def check_update(res, ref, nb, E, what):
    rows, joint, marg, hist = res
    B = rows.shape[0]
    assert ref["finite"].all()
    rel_check(joint.cpu().numpy().reshape(B, nb, N), ref["joint"], 2 * (E + 4 * EPS), what + " joint")
    tol = 2 * (E + 4 * EPS + (nb + 1) * EPS)
    rel_check(marg.cpu().numpy().reshape(B, N), ref["marginal"], tol, what + " marginal")
    rel_check(hist.cpu().numpy(), ref["hist"], tol, what + " hist")
    # the rows carry the marginal's own bits at its own first argmax, the first best bin there, the largest logit and Z
    # (numpy's argmax is the first index on ties, as the kernel's)
    r32, mg, jn = rows.cpu().numpy(), marg.cpu().numpy().reshape(B, N), joint.cpu().numpy().reshape(B, nb, N)
    idx = mg.argmax(axis=1)
    np.testing.assert_array_equal(r32[:, 0], idx.astype(np.float32))
    np.testing.assert_array_equal(r32[:, 1], mg[np.arange(B), idx])
    np.testing.assert_array_equal(r32[:, 2], jn[np.arange(B), :, idx].argmax(axis=1).astype(np.float32))
    r = rows.double().cpu().numpy()
    np.testing.assert_array_equal(r[:, 3], ref["m"])
    assert (np.abs(r[:, 4] - ref["Z"]) <= 2 * (E + 3 * EPS) * ref["Z"]).all(), (r[:, 4], ref["Z"])


def test_update_follows_the_float64_restatement():
    b0 = base()
    m, E, nb = b0["m"], b0["E"], 8
    logits, ori = b0["logits"][:2].contiguous(), poisoned_field()
    lg, o = logits.cpu().numpy(), ori.cpu().numpy().reshape(2, 2, N)
    bins = device_bins(m, ori, nb)
    assert (bins == nb).sum() >= 5120 + 283 * 5 + 3 * 512
    single = np.zeros(nb + 1, np.float32)
    single[0] = 1.0
    single[nb] = 0.125
    wrap = np.array([0.3, 0.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.4, 0.05], np.float32)          # most of the weight BEHIND the cell's own bin
    # the first frame: no prior, an emission with a single 1
    first = m.track_joint_update_logits(logits, ori, single)
    check_update(first, jr.update(lg, o, single, nb, None, bins), nb, E, "no prior, single-1 emission")
    jn = first[1].cpu().numpy().reshape(2, nb, N)
    for k in range(nb):                                   # a cell with a heading has its mass in its own bin alone
        assert not jn[:, k][(bins != k) & (bins != nb)].any(), k
    # a predicted prior, an emission that wraps
    shift = aerial.joint_shift_table([6.0, -3.5], [0.5, 2.0], nb)
    prior = m.track_joint_predict(first[1], shift, aerial.gaussian_taps(2.0, 6), [1e-9, 1e-7], [30.0, -100.0], [0.7, 0.15])
    p = prior.cpu().numpy().reshape(2, nb, N)
    check_update(m.track_joint_update_logits(logits, ori, wrap, prior), jr.update(lg, o, wrap, nb, p, bins), nb, E, "predicted prior, wrapping emission")
    # per-query tables: a uniform one and the wrapping one, on the device
    both = np.stack([np.full(nb + 1, 0.125, np.float32), wrap])
    res = m.track_joint_update_logits(logits, ori, torch.from_numpy(both).cuda(), prior)
    check_update(res, jr.update(lg, o, both, nb, p, bins), nb, E, "predicted prior, per-query emission")
    lib = _lib.load()
    torch.cuda.synchronize()
    n0 = lib.ccvpe_launch_count()
    m.track_joint_update_logits(logits, ori, wrap, prior)
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 4


# ---- 3. consistency -------------------------------------------------------------------------------------------------------------------

def test_uniform_emission_and_one_prior_for_every_bin_is_the_position_filter():
    b0 = base()
    m, E, nb = b0["m"], b0["E"], 6
    logits, ori = b0["logits"][:2].contiguous(), b0["ori"][:2].contiguous()
    # p: powers of two in steps over the map, so that p is exact and differs from cell to cell
    y, x = np.mgrid[0:512, 0:512]
    p = np.stack([2.0 ** -((x // 64) + (y // 128)), 2.0 ** -(((x + y) // 100) % 5)]).astype(np.float32)
    prior = torch.from_numpy(np.repeat(p[:, None], nb, axis=1).copy()).cuda()
    em = np.full(nb + 1, 0.5, np.float32)
    rows, joint, marg, hist = m.track_joint_update_logits(logits, ori, em, prior)
    lp = torch.log(torch.from_numpy(p).cuda())
    prow, post = m.track_update_logits(logits, ori, lp)
    # the float64 softmax of l + log p (p is exact), and the position filter itself: both within the bound of test 2
    l2 = logits.double().cpu().numpy() + np.log(p.astype(np.float64)).reshape(2, N)
    e = np.exp(l2 - l2.max(axis=1, keepdims=True))
    soft = e / e.sum(axis=1, keepdims=True)
    big = soft >= TINY
    tol = 2 * (E + 4 * EPS + (nb + 1) * EPS)
    rel_check(marg.cpu().numpy().reshape(2, N), soft, tol, "marginal against the float64 position posterior")
    d = np.abs(marg.double().cpu().numpy().reshape(2, N) - post.double().cpu().numpy().reshape(2, N))
    worst = float((d[big] / (tol * soft[big])).max())
    print(f"marginal against track_update_logits: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0
    assert (d[~big] <= 2.0 ** -99).all()
    h = hist.double().cpu().numpy()
    assert (np.abs(h - 1.0 / nb) <= tol / nb).all(), h
    assert bool((joint[:, 1:] == joint[:, :1]).all())
    # in place, and again: the same bits
    scratch = prior.clone()
    r2, j2, m2, h2 = m.track_joint_update_logits(logits, ori, em, scratch, out=scratch)
    assert j2 is scratch
    for a, b in ((r2, rows), (j2, joint), (m2, marg), (h2, hist)):
        eq(a, b)
    r3, j3, m3, h3 = m.track_joint_update_logits(logits, ori, em, prior)
    for a, b in ((r3, rows), (j3, joint), (m3, marg), (h3, hist)):
        eq(a, b)


# ---- 4. empty and poisoned queries ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["nan_logit", "zero_prior", "zero_emission", "tiny_z"])
def test_a_query_without_a_finite_posterior_is_zero_and_its_neighbours_keep_their_bits(case):
    b0 = base()
    m, nb = b0["m"], 4
    logits, ori = b0["logits"].clone(), b0["ori"].contiguous()
    prior = torch.rand(3, nb, 512, 512, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) + 0.5
    em = np.tile(aerial.heading_emission(1.5, nb), (3, 1))
    if case == "nan_logit":
        logits[1, 123457] = float("nan")
    elif case == "zero_prior":
        prior[1] = 0.0
    elif case == "zero_emission":
        em[1] = 0.0
    else:
        # one cell carries all of Z = nb * 1e-10 * 1e-30: positive but without a float32 reciprocal (Z = 0 if the product is flushed)
        logits[1] = float("-inf")
        logits[1, 1000] = 0.0
        em[1] = 1e-10
        prior[1] = 1e-30
    rows, joint, marg, hist = m.track_joint_update_logits(logits, ori, em, prior)
    r = rows[1].cpu().numpy()
    finite = logits[1][~torch.isnan(logits[1])]
    assert r[0] == -1 and np.isnan(r[1]) and r[2] == -1 and r[3] == finite.max().item()
    if case == "nan_logit":
        assert np.isnan(r[4])
    elif case == "tiny_z":
        assert r[4] == 0.0 or abs(float(r[4]) - nb * 1e-40) <= 1e-43       # (every bin of the cell adds 1e-40)
    else:
        assert r[4] == 0.0
    assert not bool(joint[1].any()) and not bool(marg[1].any()) and not bool(hist[1].any())
    keep = [0, 2]
    r2, j2, m2, h2 = m.track_joint_update_logits(logits[keep].contiguous(), ori[keep].contiguous(), em[keep], prior[keep].contiguous())
    for a, b in ((rows[keep], r2), (joint[keep], j2), (marg[keep], m2), (hist[keep], h2)):
        eq(a, b)
    assert bool((rows[keep, 0] >= 0).all()) and abs(hist[keep].sum().item() - 2.0) < 1e-4
    # with a positive floor the next predict of the empty query is flat: the stream starts over
    nxt = m.track_joint_predict(joint, np.zeros((3, nb, 2)), [1.0], 1e-6, 0.0, [1.0])
    assert bool((nxt[1] == 1e-6).all())


# ---- 5. the C ABI refuses, with nothing launched ----------------------------------------------------------------------------------------

def test_the_entry_points_refuse_bad_arguments_with_nothing_launched():
    m = base()["m"]
    lib = _lib.load()
    nb, B = 4, 1
    joint = torch.zeros(B, nb, 512, 512, device="cuda")
    prior = torch.zeros_like(joint)
    work = torch.empty(lib.ccvpe_track_joint_work_bytes(B, nb), dtype=torch.uint8, device="cuda")
    small = torch.zeros(64, device="cuda")
    logits, ori = base()["logits"][:1].contiguous(), base()["ori"][:1].contiguous()
    marg, rows, hist = torch.zeros(B, N, device="cuda"), torch.zeros(B, 5, device="cuda"), torch.zeros(B, nb, device="cuda")
    h = m._handle
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def predict(joint=joint, batch=B, nb=nb, shift=small, taps=small, stride=0, radius=1, turn=small, htaps=small, hstride=0, rh=1, floor=small,
                work=work, prior=prior):
        return lib.ccvpe_track_joint_predict(h, P(joint), batch, nb, P(shift), P(taps), stride, radius, P(turn), P(htaps), hstride, rh, P(floor),
                                             P(work), P(prior), None)

    def update(logits=logits, ori=ori, batch=B, prior=prior, emission=small, stride=0, nb=nb, rows=rows, joint_out=joint, marginal=marg, hist=hist):
        return lib.ccvpe_track_joint_update_logits(h, P(logits), P(ori), batch, P(prior), P(emission), stride, nb, P(rows), P(joint_out),
                                                   P(marginal), P(hist), None)

    torch.cuda.synchronize()
    n0 = lib.ccvpe_launch_count()
    for kw in ([dict(**{k: None}) for k in ("joint", "shift", "taps", "turn", "htaps", "floor", "work", "prior")] +
               [dict(nb=3), dict(nb=73), dict(batch=0), dict(batch=8193), dict(radius=-1), dict(radius=33), dict(rh=-1), dict(rh=2), dict(rh=33, nb=72),
                dict(stride=1), dict(stride=3), dict(hstride=1), dict(hstride=3), dict(prior=joint), dict(prior=work), dict(work=joint)]):
        assert predict(**kw) == -1, kw
    for kw in ([dict(**{k: None}) for k in ("logits", "ori", "emission", "rows", "joint_out", "marginal", "hist")] +
               [dict(nb=3), dict(nb=73), dict(batch=0), dict(batch=8193), dict(stride=1), dict(stride=4), dict(joint_out=logits), dict(marginal=ori),
                dict(marginal=prior), dict(hist=small), dict(rows=marg), dict(marginal=joint)]):
        assert update(**kw) == -1, kw
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 0
    assert predict() == 0 and update() == 0 and update(prior=None) == 0 and update(prior=joint) == 0      # (the last: in place)
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 2 + 3 * 4


# ---- 6. the filter does its job ---------------------------------------------------------------------------------------------------------

def test_the_joint_filter_follows_the_peak_whose_motion_fits_its_heading():
    """Two equal peaks A and B over six frames, the field saying heading 0 degrees at both; A moves by the table's shift for that
    bin each frame, B the opposite way.  aerial.JointTracker ends with more than 0.9 of the marginal within 8 px of A (the float64
    restatement alone: 0.999989, tests/test_track_joint_cpu.py); the position filter fed zero shift keeps both peaks (0.4999 each in
    float64)."""
    m = base()["m"]
    nb = jr.SEQ_BINS
    table = aerial.joint_shift_table(jr.SEQ_FORWARD, 0.0, nb)
    step = jr.sequence_step(table)
    em = aerial.heading_emission(jr.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jr.SEQ_SIGMA, jr.SEQ_RADIUS)
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

    held, tr = Held(), aerial.JointTracker()
    grd, sat = torch.zeros(1, 3, 154, 231), torch.zeros(1, 3, 512, 512)
    belief = None
    for k in range(jr.SEQ_FRAMES):
        rows, marg, hist = tr.step(held, grd, em, jr.SEQ_FORWARD, 0.0, 0.0, taps, list(jr.SEQ_HTAPS), jr.SEQ_FLOOR, sat=sat)
        lg = torch.from_numpy(jr.sequence_logits(k, step)[None]).cuda()
        lp = m.track_predict(belief, np.zeros((1, 2)), taps, jr.SEQ_FLOOR) if belief is not None else None
        _, belief = m.track_update_logits(lg, ori, lp)
    a, b = jr.sequence_peaks(jr.SEQ_FRAMES - 1, step)
    near_a, near_b = jr.mass_near(marg.cpu().numpy(), a), jr.mass_near(marg.cpu().numpy(), b)
    pa, pb = jr.mass_near(belief.cpu().numpy(), a), jr.mass_near(belief.cpu().numpy(), b)
    print(f"joint filter: {near_a:.6f} near A, {near_b:.2e} near B; position filter with zero shift: {pa:.4f} near A, {pb:.4f} near B")
    assert near_a > 0.9
    assert track_ref.pixel_distance(int(rows[0, 0].item()), a) <= 1.0 and int(rows[0, 2].item()) == 0
    assert hist[0, 0].item() > 0.8
    assert pa > 0.4 and pb > 0.4
