"""The affine smoother on the device (ccvpe_track_smooth_affine, smooth.track_smooth_affine / RecordingAffineTracker /
smooth_stream_affine): against the float64 restatement tests/smooth_affine_ref.py within the bound the term counts give,
bit-equal to ccvpe_track_smooth on integer translations, exact under quarter turns and flips where exactness is defined, the forms of
one call, the degenerate rules between ordinary queries, at most four launches, the turning stream of tests/track_affine_ref.py started
on a frame the distractor wins, and a recorded KITTI-style stream swept backward.

The bound.  u = 2^-24; every term is non-negative, so relative errors add (first order).  The matrices are quantised to 2^-20
(smooth_affine_ref.quantise): every coordinate is exact in float64, fused or not, so the device and the restatement take the same
floor and the same float32 fraction, the absolute term of the affine predict's bound vanishes and the weights 1.f - f are exact.
    prior = c + floor                       (4r + 12) u for the affine predict's c, + 1 for the add       4r + 13
    g = s' / prior                          one rounding (the IEEE division)                                                4r + 14
    G = sum g                               the chain of 21 additions of DESIGN.md 4.20                                     4r + 35
    h = blur(g)                             2r + 1 fused multiply-adds per pass, two passes                                 8r + 16
    a term det * (wy * (wx * h))            two weight roundings (1.f - f; none for these matrices), three products         8r + 21
    A = sum of the terms                    at most T additions, T the most samples that can touch one cell: an open
                                            interval of length 2 hx holds at most ceil(2 hx) integers, so
                                            T = ceil(2 hx) ceil(2 hy) <= 36 within reach                                    8r + 21 + T
    a = fma(floor, G, A)                    one rounding on top of the larger term's error          E = max(4r + 35, 8r + 21 + T) + 1
    w = b * a                                                                                                               E + 1
    Z = sum w                               the same chain of 21                                                            E + 22
    s = w * (1 / Z)                         two roundings on top of w's and Z's                                            2E + 25
The tests allow twice (2E + 25) u on the map wherever the reference s >= 2^-100 (below: got <= 2^-99), twice (E + 22) u on Z and twice
(4r + 35) u on G, as tests/test_smooth_gpu.py does."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth
from tests import smooth_affine_ref as sref
from tests import track_affine_ref, track_ref
from tests.test_track_gpu import eq, eq_nan, inputs, make

pytestmark = pytest.mark.gpu

N = 512 * 512
U = 2.0 ** -24
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
FLIP_X = np.array([-1.0, 0.0, 511.0, 0.0, 1.0, 0.0])
FLIP_Y = np.array([1.0, 0.0, 0.0, 0.0, -1.0, 511.0])


def terms(matrix):
    """T of the docstring for one matrix"""
    ok, hx, hy = sref.reach(matrix)
    assert ok
    return int(np.ceil(2 * hx) * np.ceil(2 * hy))


def err_a(r, matrix):
    return max(4 * r + 35, 8 * r + 21 + terms(matrix)) + 1


def bound_s(r, matrix):
    return (2 * err_a(r, matrix) + 25) * U


def bound_z(r, matrix):
    return (err_a(r, matrix) + 22) * U


def bound_g(r):
    return (4 * r + 35) * U


def rigid(deg, shift, scale=1.0):
    return sref.quantise(aerial.rigid_matrix(deg, shift, scale))


_BASE = {}


def base():
    """the model, a forward's heatmap, a next map that an actual track_predict_affine + track_update_logits step produced from it,
    crafted maps (computed once; not to be written)"""
    if not _BASE:
        m = make("oxford")
        g, s = inputs("oxford", 2, seed=5)
        logits, _, ori = m(g, s)[:3]
        _, heat = m.track_update_logits(logits[:1], ori[:1])
        lp = m.track_predict_affine(heat, rigid(0.5, [3.37, 0.81]), aerial.gaussian_taps(2.5, 6), 1e-9)
        _, step = m.track_update_logits(logits[1:], ori[1:], lp)
        rng = np.random.default_rng(21)
        rnd = rng.uniform(0.0, 1.0, size=(2, 512, 512)).astype(np.float32)
        rnd /= rnd.reshape(2, -1).sum(axis=1)[:, None, None]
        corner = np.full((512, 512), 1e-12, np.float32)
        corner[0, 0], corner[511, 511], corner[300, 17] = 0.5, 0.25, 0.25
        _BASE.update(m=m, heat=heat[0].cpu().numpy(), step=step[0].cpu().numpy(), rnd=rnd[0], rnd2=rnd[1], corner=corner,
                     uniform=np.full((512, 512), 1.0 / N, np.float32))
    return _BASE


# (belief, next map, matrix, floor): turns of 0.5, 5, 37.5, 90 and -171 degrees with fractional shifts; the content at scale 0.8, 1.25
# and 0.5, and at scale 2 (a linear part of scale 0.5) turned by 30 degrees - (hx, hy) = (2.73, 2.73), T = 36, the far end of the reach;
# a shear; translations by 600 px and by 1e6 px, off the window, where a = floor * G; floors 1e-9 and 0.37
QUERIES = [("heat", "step", rigid(0.5, [3.37, 0.81]), 1e-9), ("heat", "step", rigid(5.0, [12.0, -7.0]), 0.37),
           ("rnd", "heat", rigid(37.5, [-30.6, 20.2]), 1e-9), ("rnd2", "rnd", rigid(90.0, [0.5, -0.5]), 1e-9),
           ("corner", "rnd2", rigid(-171.0, [0.25, -2.75]), 1e-9), ("uniform", "step", sref.quantise([1.0, 0.0, -600.0, 0.0, 1.0, 3.5]), 1e-9),
           ("heat", "rnd", rigid(10.0, [4.0, 4.0], 0.8), 1e-9), ("rnd", "step", rigid(-20.0, [-6.5, 3.0], 1.25), 0.37),
           ("rnd2", "heat", rigid(15.0, [2.0, 2.0], 0.5), 1e-9), ("rnd", "rnd2", rigid(30.0, [1.5, -2.5], 2.0), 1e-9),
           ("corner", "rnd", sref.quantise([1.1, 0.3, -40.5, -0.2, 0.8, 60.25]), 1e-9), ("rnd", "step", sref.quantise([1.0, 0.0, 1e6, 0.0, 1.0, 0.0]), 0.37)]
OFF_WINDOW = (5, 11)


def batch_of(cases):
    b = base()
    bel = np.stack([b[c[0]] for c in cases])
    nxt = np.stack([b[c[1]] for c in cases])
    return bel, nxt, np.stack([c[2] for c in cases]), np.float32([c[3] for c in cases])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_against_ref(got_s, got_st, ref, r, mats, what):
    """the map, the stats and their consistency, for the ordinary queries of a call -> the worst error over the bound"""
    s = got_s.double().cpu().numpy()
    st = got_st.double().cpu().numpy()
    flat = got_s.view(got_s.shape[0], -1)
    worst = 0.0
    for q in range(s.shape[0]):
        want, wst = ref["s"][q], ref["stats"][q]
        bs, bz = bound_s(r, mats[q]), bound_z(r, mats[q])
        assert wst[0] >= 0, (what, q, "the reference takes this query for a degenerate one")
        big = want >= 2.0 ** -100
        ratio = float((np.abs(s[q][big] - want[big]) / (bs * want[big])).max())
        worst = max(worst, ratio)
        print(f"{what}: radius {r} query {q}: T = {terms(mats[q])}, error / bound: map {ratio:.3f}, "
              f"Z {abs(st[q, 2] - wst[2]) / (bz * wst[2]):.3f}, G {abs(st[q, 3] - wst[3]) / (bound_g(r) * wst[3]):.3f}")
        assert ratio <= 2.0, (what, q, ratio)
        assert (s[q][~big] <= 2.0 ** -99).all() and not np.isnan(s[q]).any(), (what, q)
        i = int(st[q, 0])
        assert 0 <= i < N
        top = want.reshape(-1)[int(wst[0])]
        assert i == int(wst[0]) or want.reshape(-1)[i] >= top * (1.0 - 2 * bs), (what, q, i, wst[0])
        assert got_st[q, 1].item() == flat[q, i].item() and flat[q, i].item() == flat[q].max().item(), (what, q)
        assert abs(st[q, 2] - wst[2]) <= 2 * bz * wst[2], (what, q, st[q, 2], wst[2])
        assert abs(st[q, 3] - wst[3]) <= 2 * bound_g(r) * wst[3], (what, q, st[q, 3], wst[3])
    print(f"{what}: radius {r}: worst error / bound = {worst:.3f}")
    return worst


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("r,sigma", [(0, 1.0), (1, 0.7), (6, 2.5), (32, 11.0)])
def test_follows_the_float64_restatement(r, sigma, half):
    m = base()["m"]
    pick = list(range(6 * half, 6 * half + 6))
    bel, nxt, mats, floor = batch_of([QUERIES[q] for q in pick])
    taps = aerial.gaussian_taps(np.linspace(0.6 * sigma, 1.2 * sigma, len(pick)), r)     # per-query taps
    got_s, got_st = smooth.track_smooth_affine(m, dev(bel), dev(nxt), mats, taps, floor)
    ref = sref.smooth(bel, nxt, mats, taps, floor)
    check_against_ref(got_s, got_st, ref, r, mats, "restatement")
    for k, q in enumerate(pick):
        if q in OFF_WINDOW:     # a = floor * G for every cell, so the smoothed map is the belief over its mass
            u = bel[k].astype(np.float64)
            np.testing.assert_allclose(got_s[k].double().cpu().numpy(), u / u.sum(), rtol=2 * bound_s(r, mats[k]))
    if half == 0:               # Z is the mass of the next map up to the belief's own distance from mass 1
        for k in (0, 1):
            mass, nm = float(bel[k].astype(np.float64).sum()), float(nxt[k].astype(np.float64).sum())
            assert abs(got_st[k, 2].item() - nm) <= (2 * bound_z(r, mats[k]) + abs(mass - 1.0)) * nm, (k, got_st[k, 2].item(), nm, mass)


# ---- 2. integer translations are ccvpe_track_smooth -------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [0, 6])
def test_integer_translations_give_the_bits_of_track_smooth(r):
    m = base()["m"]
    shifts = np.float32([[0, 0], [37, -60], [-64, 5], [3, 511], [-530, 2], [700, -900]])
    cases = [QUERIES[q] for q in (0, 2, 3, 4, 6, 7)]
    bel, nxt, _, _ = batch_of(cases)
    mats = np.tile(IDENTITY, (len(shifts), 1))
    mats[:, 2], mats[:, 5] = -shifts[:, 0], -shifts[:, 1]
    b_dev, n_dev = dev(bel), dev(nxt)
    taps = aerial.gaussian_taps(2.5, r)
    for floor in (1e-9, 1.0 / 16):
        got, st = smooth.track_smooth_affine(m, b_dev, n_dev, mats, taps, floor)
        want, wst = smooth.track_smooth(m, b_dev, n_dev, shifts, taps, floor)
        eq(got, want)
        eq(st, wst)
        assert bool((st[:, 0] >= 0).all())


# ---- 3. quarter turns and flips ----------------------------------------------------------------------------------------------------

def turns(t):
    """the six moved forms of maps [.., 512, 512] and their matrices: the affine predict of the map through mats[k] is the predict of
    moved[k] through the identity (tests/test_track_affine_gpu.py)"""
    moved = [torch.rot90(t, k, dims=(-2, -1)) for k in range(4)] + [torch.flip(t, dims=(-1,)), torch.flip(t, dims=(-2,))]
    mats = np.concatenate([aerial.rigid_matrix(90.0 * np.arange(4), [0, 0]), FLIP_X[None], FLIP_Y[None]])
    return moved, mats


def test_quarter_turns_and_flips_move_the_result():
    """Radius 0, taps [1].  The belief moved by a quarter turn or a flip and smoothed through the identity is the moved result of the
    belief smoothed through the turn's matrix: prior, g, G and w are the same numbers at moved cells - one sample touches every cell,
    with weight exactly 1 - and only the order of the sum Z changes.  Each side is within bound_s(0) of the exact map, so the two
    within twice that; on maps whose every sum is exact in float32 (an integer belief on 4096 cells, floor 1/16, s' = prior * 2^k on
    256 cells) they are the same bits."""
    b = base()
    m = b["m"]
    one = torch.ones(1)
    # ordinary maps
    bel, nxt = dev(b["rnd"][None]), dev(b["heat"][None])
    moved, mats = turns(bel)
    got, st = smooth.track_smooth_affine(m, bel.expand(6, 512, 512).contiguous(), nxt.expand(6, 512, 512).contiguous(), mats, one, 1e-9)
    want, wst = smooth.track_smooth_affine(m, torch.cat(moved).contiguous(), nxt.expand(6, 512, 512).contiguous(), IDENTITY, one, 1e-9)
    for k in range(6):
        a, w = turns(got[k:k + 1])[0][k].double(), want[k:k + 1].double()
        lim = 2 * bound_s(0, mats[k])
        assert bool(((a - w).abs() <= lim * w).all()), (k, ((a - w).abs() / w.clamp_min(1e-300)).max().item() / lim)
        assert abs(st[k, 2].item() - wst[k, 2].item()) <= 2 * bound_z(0, mats[k]) * wst[k, 2].item()
        eq(st[k, 3], wst[k, 3])                     # G is summed over the next map's cells, in one order
    # exact maps
    rng = np.random.default_rng(33)
    ib = np.zeros((512, 512), np.float32)
    cells = rng.choice(384 * 384, size=4096, replace=False)
    ib[64 + cells // 384, 64 + cells % 384] = rng.integers(1, 4, size=4096).astype(np.float32)
    floor = np.float32(1.0 / 16)
    bel = dev(ib[None])
    moved, mats = turns(bel)
    at = rng.choice(N, size=256, replace=False)
    pw = np.zeros(N)
    pw[at] = 2.0 ** rng.integers(0, 2, size=256)
    for k in range(6):
        prior = moved[k][0].double().cpu().numpy() + float(floor)          # radius 0: the prior is the moved belief plus the floor
        nx = (prior * pw.reshape(512, 512)).astype(np.float32)
        assert (nx.astype(np.float64) == prior * pw.reshape(512, 512)).all()
        n_dev = dev(nx[None])
        got, st = smooth.track_smooth_affine(m, bel, n_dev, mats[k], one, floor)
        want, wst = smooth.track_smooth_affine(m, moved[k].contiguous(), n_dev, IDENTITY, one, floor)
        eq(turns(got)[0][k].contiguous(), want)
        eq(st[:, 1:], wst[:, 1:])
        assert st[0, 0].item() >= 0 and st[0, 3].item() == pw.sum() and got.view(-1)[int(st[0, 0].item())].item() == st[0, 1].item()
        # the sums are exact, so they are the float64 ones
        ref = sref.smooth(ib[None], nx[None], mats[k], np.float32([1.0]), floor)
        assert st[0, 2].item() == ref["stats"][0, 2] and st[0, 3].item() == ref["stats"][0, 3]


# ---- 4. the forms of one call ---------------------------------------------------------------------------------------------------------

FORMS = [QUERIES[q] for q in (0, 2, 6, 9, 10, 5)]


def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    bel, nxt, mats, floor = batch_of(FORMS)
    B = len(FORMS)
    b_dev, n_dev = dev(bel), dev(nxt)
    t = aerial.gaussian_taps(2.5, 6)
    got, st = smooth.track_smooth_affine(m, b_dev, n_dev, mats, t, floor)
    # shared taps against repeated taps
    rep, rst = smooth.track_smooth_affine(m, b_dev, n_dev, mats, np.tile(t, (B, 1)), floor)
    eq(got, rep); eq(st, rst)
    # host against device matrices
    on, ost = smooth.track_smooth_affine(m, b_dev, n_dev, dev(mats), t, floor)
    eq(got, on); eq(st, ost)
    # a second call
    again, ast = smooth.track_smooth_affine(m, b_dev, n_dev, mats, t, floor)
    eq(got, again); eq(st, ast)
    # in place
    run = n_dev.clone()
    out, ost = smooth.track_smooth_affine(m, b_dev, run, mats, t, floor, out=run)
    assert out.data_ptr() == run.data_ptr()
    eq(got, run); eq(st, ost)
    eq(n_dev, dev(nxt))
    # each query alone, its matrix as [6], as [1,6] and on the device
    for q in range(B):
        for mat in (mats[q], mats[q:q + 1], dev(mats[q])):
            one, ost = smooth.track_smooth_affine(m, b_dev[q:q + 1], n_dev[q:q + 1], mat, t, floor[q:q + 1])
            eq(got[q:q + 1], one); eq(st[q:q + 1], ost)
    # [6] against [B,6]
    same, sst = smooth.track_smooth_affine(m, b_dev, n_dev, mats[2], t, floor)
    tiled, tst = smooth.track_smooth_affine(m, b_dev, n_dev, np.tile(mats[2], (B, 1)), t, floor)
    eq(same, tiled); eq(sst, tst)
    eq(same[2], got[2])
    # the [B,1,512,512] form of the maps
    four, fst = smooth.track_smooth_affine(m, b_dev[:, None], n_dev[:, None], mats, t, floor)
    eq(got, four); eq(st, fst)


def test_two_streams_with_two_work_buffers_do_not_meet():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, mats, floor = batch_of(FORMS)
    B = len(FORMS)
    b_dev, n_dev = dev(bel), dev(nxt)
    t6, t32 = aerial.gaussian_taps(2.5, 6), aerial.gaussian_taps(11.0, 32)
    back = mats[::-1].copy()
    serial = [smooth.track_smooth_affine(m, b_dev, n_dev, mats, t6, floor), smooth.track_smooth_affine(m, n_dev, b_dev, back, t32, floor)]
    mt = [dev(mats), dev(back)]
    tp = [dev(t6), dev(t32)]
    fl = dev(floor)
    args = [(b_dev, n_dev, mt[0], tp[0], 6), (n_dev, b_dev, mt[1], tp[1], 32)]
    outs = [(torch.empty(B, 512, 512, device="cuda"), torch.empty(B, 4, device="cuda"),
             torch.empty(lib.ccvpe_track_smooth_affine_work_bytes(B), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for (bb, nn, m_, t_, r), (o, st, wk), stream in zip(args, outs, streams):
            rc = lib.ccvpe_track_smooth_affine(m._handle, bb.data_ptr(), nn.data_ptr(), B, m_.data_ptr(), t_.data_ptr(), 0, r, fl.data_ptr(),
                                               o.data_ptr(), st.data_ptr(), wk.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (ws, wst) in zip(outs, serial):
        eq(o, ws); eq(st, wst)


# ---- 5. degenerate queries between ordinary ones -------------------------------------------------------------------------------------

def test_degenerate_queries_get_their_rule_and_their_neighbours_keep_their_bits():
    m = base()["m"]
    r, t = 6, aerial.gaussian_taps(2.5, 6)
    ordinary = [QUERIES[0], QUERIES[2], QUERIES[9]]
    cases = [ordinary[i % 3] for i in range(8)]
    bel, nxt, clean_mats, floor = batch_of(cases)
    clean_b, clean_n = dev(bel), dev(nxt)
    clean, clean_st = smooth.track_smooth_affine(m, clean_b, clean_n, dev(clean_mats), t, floor)
    assert bool((clean_st[:, 0] >= 0).all())

    def rule1(s, st, q):
        eq(s[q], clean_b[q])
        i = int(clean_b[q].argmax().item())
        assert st[q, 0].item() == i and st[q, 1].item() == clean_b[q].view(-1)[i].item() and np.isnan(st[q, 2].item()) and st[q, 3].item() == 0

    def rule2(s, st, q):
        assert not bool(s[q].any()), q
        assert st[q, 0].item() == -1 and np.isnan(st[q, 1].item()), (q, st[q])

    # first batch: the maps
    bad_b, bad_n = bel.copy(), nxt.copy()
    bad_n[1] = 0.0                                   # a zero next map: rule 1
    bad_b[3] = 0.0                                   # a zero belief: rule 2
    bad_b[5, 200, 300] = np.nan                      # a NaN in the belief: rule 2
    bad_n[7, 100, 100], bad_n[7, 17, 400] = np.nan, -1.0     # a NaN and a negative cell in the next map: not taken, an ordinary query
    got, st = smooth.track_smooth_affine(m, dev(bad_b), dev(bad_n), dev(clean_mats), t, floor)
    for q in (0, 2, 4, 6):
        eq(got[q], clean[q]); eq(st[q], clean_st[q])
    rule1(got, st, 1)
    rule2(got, st, 3)
    rule2(got, st, 5)
    assert st[3, 2].item() == 0 and st[3, 3].item() > 0 and np.isnan(st[5, 2].item())
    ref = sref.smooth(bad_b[7:8], bad_n[7:8], clean_mats[7], t, floor[7:8])
    check_against_ref(got[7:8], st[7:8], ref, r, clean_mats[7:8], "holes in the next map")
    # second batch: the matrices, as a device tensor (host matrices of this kind are refused): links beyond reach are broken links
    mats = clean_mats.copy()
    mats[1] = [1.0, 2.0, 5.0, 2.0, 4.0, -3.0]                            # det = 0
    mats[3] = aerial.rigid_matrix(25.0, [3.0, -4.0], 1.0 / 0.3)          # a linear part of scale 0.3
    mats[5] = clean_mats[5]
    mats[5, 0] = np.nan                                                  # a NaN in the linear part
    mats[7] = 0.0
    got, st = smooth.track_smooth_affine(m, clean_b, clean_n, dev(mats), t, floor)
    for q in (0, 2, 4, 6):
        eq(got[q], clean[q]); eq(st[q], clean_st[q])
    for q in (1, 3, 5, 7):
        rule1(got, st, q)
    with pytest.raises(ValueError, match="reach|finite"):
        smooth.track_smooth_affine(m, clean_b, clean_n, mats, t, floor)
    # a NaN in the translation is within reach: the predict's prior is NaN everywhere, so G and Z are: rule 2, and nothing non-finite
    # in the map
    mats = clean_mats.copy()
    mats[2, 2] = np.nan
    mats[4, 5] = np.inf
    got, st = smooth.track_smooth_affine(m, clean_b, clean_n, dev(mats), t, floor)
    for q in (0, 1, 3, 5, 6, 7):
        eq(got[q], clean[q]); eq(st[q], clean_st[q])
    for q in (2, 4):
        rule2(got, st, q)
        assert np.isnan(st[q, 2].item())
    # nothing is left behind: the clean batch again
    again, again_st = smooth.track_smooth_affine(m, clean_b, clean_n, dev(clean_mats), t, floor)
    eq(again, clean); eq(again_st, clean_st)
    # a belief without a value above -inf has no argmax under rule 1
    nan_b = torch.full((1, 512, 512), float("nan"), device="cuda")
    s1, st1 = smooth.track_smooth_affine(m, nan_b, torch.zeros(1, 512, 512, device="cuda"), IDENTITY, t, 1e-9)
    eq_nan(s1, nan_b)
    assert st1[0, 0].item() == -1 and np.isnan(st1[0, 1].item()) and np.isnan(st1[0, 2].item()) and st1[0, 3].item() == 0


# ---- 6. launches -------------------------------------------------------------------------------------------------------------------

def test_four_launches():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, mats, floor = batch_of(QUERIES[:2])
    b_dev, n_dev, mt, fl = dev(bel), dev(nxt), dev(mats), dev(floor)

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for r in (0, 6, 32):
        taps = torch.as_tensor(aerial.gaussian_taps(2.0, r)).cuda()
        smooth.track_smooth_affine(m, b_dev, n_dev, mt, taps, fl)
        assert 1 <= count(lambda: smooth.track_smooth_affine(m, b_dev, n_dev, mt, taps, fl)) <= 4


# ---- 7. the smoother does its job in a turning frame ---------------------------------------------------------------------------------

def test_the_smoother_moves_the_first_frame_off_the_distractor():
    m = base()["m"]
    ref = track_affine_ref
    frames, _, ref_smoothed, _, (taps, floor) = sref.crafted_stream(2)
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0
    beliefs, belief = {}, None
    for k in frames:
        lg = torch.from_numpy(ref.sequence_logits(k)[None]).cuda()
        lp = m.track_predict_affine(belief, ref.sequence_matrix(k), taps, floor) if belief is not None else None
        rows, belief = m.track_update_logits(lg, ori, lp)
        beliefs[k] = belief
        if k == frames[0]:
            i = int(rows[0, 0].item())
            assert track_ref.pixel_distance(i, ref.SEQ_DISTRACTOR) <= 1.0 and track_ref.pixel_distance(i, ref.sequence_truth(k)) > 250.0
    s = beliefs[frames[-1]]
    for k in reversed(frames):
        if k != frames[-1]:
            s, st = smooth.track_smooth_affine(m, beliefs[k], s, ref.sequence_matrix(k + 1), taps, floor)      # unquantised matrices
            i = int(st[0, 0].item())
            assert abs(st[0, 2].item() - 1.0) <= 1e-4
        else:
            i = int(s.argmax().item())
        assert i == int(np.argmax(ref_smoothed[k])), (k, i)
        assert track_ref.pixel_distance(i, ref.sequence_truth(k)) <= 1.0, (k, i)


# ---- 8. RecordingAffineTracker and smooth_stream_affine ---------------------------------------------------------------------------------

def test_recorded_stream_is_swept_by_the_spelled_out_calls():
    m = make("kitti")
    F = 6
    g, s = inputs("kitti", F, seed=23)              # six frames of one stream whose heading-up tiles turn
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    mats = aerial.rigid_matrix(np.array([0.0, 4.0, -7.5, 120.0, 2.0, 0.0]), np.array([[0, 0], [6.5, -2.25], [-3.0, 8.0], [10.0, 10.0], [0.5, 0.5], [4.0, -6.0]]),
                               np.array([1.0, 1.0, 1.0, 1.0, 1.1, 1.0]))
    tr, plain = smooth.RecordingAffineTracker(), aerial.AffineTracker()
    for k in range(F):
        rows = tr.step(m, g[k:k + 1], s[k:k + 1], mats[k], taps, floor)
        eq(rows, plain.step(m, g[k:k + 1], s[k:k + 1], mats[k], taps, floor))
        eq(tr.belief, plain.belief)
    assert len(tr.log) == F and tr.log[0][1] is None
    kept = [e[0].clone() for e in tr.log]
    maps, stats = smooth.smooth_stream_affine(m, tr.log)
    maps2, stats2 = smooth.smooth_stream_affine(m, tr.log, in_place=True)
    for k in range(F):
        eq(tr.log[k][0], kept[k])                   # neither sweep writes to the log's beliefs
    # spelled out
    want = tr.log[-1][0]
    eq(maps[-1], want)
    i = int(want.argmax().item())
    assert stats[-1, 0, 0].item() == i and stats[-1, 0, 1].item() == want.view(-1)[i].item() and np.isnan(stats[-1, 0, 2].item())
    for k in range(F - 2, -1, -1):
        want, wst = smooth.track_smooth_affine(m, tr.log[k][0], want, mats[k + 1], taps, floor)
        eq(maps[k], want); eq(stats[k], wst)
        assert wst[0, 0].item() >= 0 and abs(wst[0, 2].item() - 1.0) <= 1e-4
    for a, b_ in zip(maps, maps2):
        eq(a, b_)
    eq_nan(stats, stats2)
