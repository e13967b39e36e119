"""The MAP trajectory behind an affine predict on the device (ccvpe_track_viterbi_affine, ccvpe_track_viterbi_back_affine,
viterbi.track_viterbi_affine / track_viterbi_back_affine / map_path_affine): bit-equal to the translation form at
integer translations, against the float64 definition tests/viterbi_affine_ref.py within the bound the roundings give, bit-equal to the
float32 restatement on inputs with exact arithmetic (ties included), the same bits across call forms, the degenerate rules between
ordinary queries, the launch counts, the turning and the relocalising stream, and a recorded KITTI stream.

The bound.  u = 2^-24, relative, first order, against a float64 evaluation on the same float32 inputs, the same float32 fractions and
the same float32 det, for matrices whose coordinate arithmetic is exact in float64 (smooth_affine_ref.quantise):
    lik = b / prior                          the affine predict's c (4r + 12) u, the floor add, one IEEE division   4r + 14
    cand = det * (wy * (wx * v-))            1 - fx and 1 - fy one rounding each, three products                                     5
    win = ty * (tx * q)                      two products on top of cand; the taps are inputs and the maxima exact                   7
    jump = floor * peak                                                                                                              1
    w = lik * max(win, jump)                 (4r + 14) + 7 + 1                                                                       4r + 22
    v = ldexpf(w, -e)                        exact (the results here are not subnormal)
The tests allow twice (4r + 22) u on w wherever the reference is >= 2^-100, and twice 7 u between backtrack candidates."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth, viterbi
from tests import smooth_affine_ref as sref, track_affine_ref, track_ref, viterbi_affine_ref as vref
from tests.test_track_gpu import eq, eq_nan, inputs, make

pytestmark = pytest.mark.gpu

N = 512 * 512
U = 2.0 ** -24
BOUND_WIN = 7 * U
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
FLIP_X = np.array([-1.0, 0.0, 511.0, 0.0, 1.0, 0.0])
FLIP_Y = np.array([1.0, 0.0, 0.0, 0.0, -1.0, 511.0])


def bound_w(r):
    return (4 * r + 22) * U


def rigid(deg, shift, scale=1.0):
    return sref.quantise(aerial.rigid_matrix(deg, shift, scale))


def translation(dx, dy):
    return np.array([1.0, 0.0, -float(dx), 0.0, 1.0, -float(dy)])


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_BASE = {}


def base():
    """the model, a forward's heatmap, the belief an actual track_predict_affine + track_update_logits step made of it, random maps, and
    the first-frame score map and stats of each map that serves as a previous frame (computed once; not to be written)"""
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
        maps = dict(heat=heat[0].cpu().numpy(), step=step[0].cpu().numpy(), rnd=rnd[0], rnd2=rnd[1])
        first = {}
        for k in ("heat", "rnd", "rnd2"):
            v, st = viterbi.track_viterbi_affine(m, torch.from_numpy(maps[k][None]).cuda())
            first[k] = (v[0].cpu().numpy(), st[0].cpu().numpy())
        _BASE.update(m=m, maps=maps, first=first)
    return _BASE


def batch_of(cases):
    """cases (belief, previous belief, matrix, floor) -> bel, prev, sprev, pst, mats, floor"""
    b = base()
    bel = np.stack([b["maps"][c[0]] for c in cases])
    prev = np.stack([b["maps"][c[1]] for c in cases])
    sprev = np.stack([b["first"][c[1]][0] for c in cases])
    pst = np.stack([b["first"][c[1]][1] for c in cases])
    return bel, prev, sprev, pst, np.stack([c[2] for c in cases]), np.float32([c[3] for c in cases])


def run_step(m, bel, prev, sprev, pst, mats, taps, floor):
    return viterbi.track_viterbi_affine(m, cu(bel), cu(prev), cu(sprev), cu(pst), mats, taps, floor)


# ---- 1. integer translations: the translation form's bits --------------------------------------------------------------------------

SHIFTS = [(0, 0), (3, -2), (-37, 60), (64, -5), (600, -3)]          # the last one leaves the grid: win = 0, every cell jumps or is lost


@pytest.mark.parametrize("r", [0, 6])
def test_integer_translations_give_the_bits_of_track_viterbi(r):
    b = base()
    m = b["m"]
    B = len(SHIFTS)
    taps = aerial.gaussian_taps(2.0, r)
    shift = np.float64(SHIFTS)
    mats = np.stack([translation(dx, dy) for dx, dy in SHIFTS])
    rng = np.random.default_rng(7 + r)
    for cur, old in (("step", "heat"), ("rnd2", "rnd")):
        args = [cu(np.stack([a] * B)) for a in (b["maps"][cur], b["maps"][old], b["first"][old][0], b["first"][old][1])]
        for floor in (0.0, 1e-9):
            got, st = viterbi.track_viterbi_affine(m, *args, mats, taps, floor)
            want, wst = viterbi.track_viterbi(m, *args, shift, taps, floor)
            eq(got, want)
            eq_nan(st, wst)
            cells = [st[:, 0].to(torch.int32), cu(rng.integers(0, N, size=B).astype(np.int32)), cu(np.int32([0, N - 1, -1, N, 511]))]
            for c in cells:
                eq(viterbi.track_viterbi_back_affine(m, args[2], args[3], c, mats, taps, floor),
                   viterbi.track_viterbi_back(m, args[2], args[3], c, shift, taps, floor))


def test_first_frame_form_is_track_viterbi_itself():
    b = base()
    m = b["m"]
    for k in ("heat", "rnd"):
        bel = cu(b["maps"][k][None])
        got, st = viterbi.track_viterbi_affine(m, bel)
        want, wst = viterbi.track_viterbi(m, bel)
        eq(got, want); eq(st, wst)
        assert st[0, 3].item() == 1 and 1.0 <= st[0, 1].item() < 2.0


# ---- 2. against the float64 definition -------------------------------------------------------------------------------------------

def definition_cases():
    """DESIGN.md 4.14's seventeen matrices, quantised; b the belief a real predict + update step made, b- a forward's heatmap or a
    random map; floors 0, 1e-9 and 0.37"""
    R = rigid
    shear = sref.quantise([1.05, 0.31, -40.7, -0.12, 0.93, 22.15])
    mats = [R(0.5, [3.37, 0.81]), R(5.0, [12.25, -7.5]), R(37.5, [-30.6, 20.2]), R(90.0, [0.5, -0.25]), R(-171.0, [7.77, 3.33]),
            R(5.0, [1.5, 2.5], 0.8), R(-20.0, [-4.25, 9.0], 1.25), shear, R(5.0, [20.3, 31.9]), R(0.0, [-0.25, 2.75]),
            R(-37.5, [-11.5, 3.25], 1.25), R(37.5, [0.125, -0.875], 0.8), R(5.0, [0.0, 0.0]), shear, translation(600.0, 0.0), np.zeros(6),
            translation(1e6, -1e6)]
    floors = [1e-9, 0.0, 1e-9, 0.37, 1e-9, 1e-9, 0.0, 1e-9, 0.37, 1e-9, 1e-9, 0.0, 1e-9, 0.37, 1e-9, 1e-9, 0.37]
    olds = ["heat", "heat", "rnd", "heat", "rnd2", "heat", "rnd", "heat", "heat", "rnd", "heat", "rnd2", "heat", "rnd", "heat", "rnd", "heat"]
    return [("step", olds[k], mats[k], floors[k]) for k in range(17)]


OFF_GRID = (14, 15, 16)       # nothing in reach, a singular matrix, a clamped translation: win = 0, the floor is the only link


@pytest.mark.parametrize("r,sigma", [(0, 1.0), (1, 0.7), (6, 2.5), (32, 11.0)])
def test_follows_the_float64_definition(r, sigma):
    m = base()["m"]
    cases = definition_cases()
    B = len(cases)
    bel, prev, sprev, pst, mats, floor = batch_of(cases)
    taps = aerial.gaussian_taps(np.linspace(0.6 * sigma, 1.2 * sigma, B), r)          # per-query taps
    got_v, got_st = run_step(m, bel, prev, sprev, pst, mats, taps, floor)
    dv, dst = run_step(m, bel, prev, sprev, pst, cu(mats), taps, floor)              # the matrices as a device tensor: the same bits
    eq(got_v, dv)
    eq_nan(got_st, dst)
    v, st = got_v.double().cpu().numpy(), got_st.double().cpu().numpy()
    rng = np.random.default_rng(100 + r)
    cells = np.stack([np.where(st[:, 0] >= 0, st[:, 0], 0).astype(np.int64), np.zeros(B, np.int64), np.full(B, N - 1), np.full(B, 511), np.full(B, N - 512),
                      rng.integers(0, N, size=B), rng.integers(0, N, size=B)])
    backs = [viterbi.track_viterbi_back_affine(m, cu(sprev), cu(pst), cu(c.astype(np.int32)), mats, taps, floor).cpu().numpy() for c in cells]
    worst = worst_back = 0.0
    for q in range(B):
        ref = vref.step(bel[q:q + 1], prev[q:q + 1], sprev[q:q + 1], pst[q:q + 1], mats[q], taps[q], floor[q])
        want = ref["w"][0]
        assert st[q, 3] == 0 == ref["stats"][0, 3]
        if q in OFF_GRID:
            assert not ref["win"].any()
        if not ref["stats"][0, 0] >= 0:                                  # floor 0 with nothing in reach: lik = inf or every link lost
            assert q in OFF_GRID and st[q, 0] == -1 and not v[q].any()
            continue
        w = np.ldexp(v[q], int(st[q, 2]))
        big = want >= 2.0 ** -100
        ratio = float((np.abs(w[big] - want[big]) / (bound_w(r) * want[big])).max())
        worst = max(worst, ratio)
        print(f"radius {r} query {q}: worst error / bound = {ratio:.3f}, exponent {int(st[q, 2])}")
        assert ratio <= 2.0, (q, ratio)
        assert not np.isnan(v[q]).any() and (v[q] >= 0).all()
        i = int(st[q, 0])
        assert 0 <= i < N and want.reshape(-1)[i] >= want.max() * (1.0 - 2 * bound_w(r)), (q, i)
        assert 1.0 <= st[q, 1] < 2.0 and st[q, 1] == v[q].reshape(-1)[i] == v[q].max() and i == int(np.argmax(v[q]))
        # the backtrack against the float64 candidates
        j = int(pst[q, 0])
        jump = float(np.float64(floor[q]) * np.float64(sprev[q].reshape(-1)[j]))
        tol = 2 * BOUND_WIN
        for c, back in zip(cells, backs):
            idx, vals = vref.back_candidates(sprev[q], int(c[q]), mats[q], taps[q])
            best = float(vals.max()) if vals.size else -np.inf
            prev_cell, kind = int(back[q, 0]), int(back[q, 1])
            if jump > best * (1 + tol) and jump > 0:
                assert (prev_cell, kind) == (j, viterbi.LINK_JUMP), (q, c[q], back[q], best, jump)
            elif best > jump * (1 + tol) and best > 0:
                assert kind == viterbi.LINK_MOVE, (q, c[q], back[q], best, jump)
            if kind == viterbi.LINK_MOVE:
                at = idx == prev_cell
                assert at.any() and vals[at].max() >= best * (1 - tol), (q, c[q], back[q])
                worst_back = max(worst_back, float((best - vals[at].max()) / (BOUND_WIN * best)))
            elif kind == viterbi.LINK_JUMP:
                assert prev_cell == j and jump >= best * (1 - tol)
            else:
                assert prev_cell == j and not best > 0 and not jump > 0
    print(f"radius {r}: worst w error / bound {worst:.3f}, worst backtrack gap / bound {worst_back:.3f}")


# ---- 3. exact ----------------------------------------------------------------------------------------------------------------------

def exact_case():
    """Eight queries on which every operation of the step is exact in float32: the four quarter turns, the two flips, an integer
    translation and a map of scale (1/2, 1) - whose samples weigh their cells with 1 or 1/2, so that two samples of one window
    reach the same source cell with the same product -, taps (1/2, 1/4), floor 1/16, an integer previous belief on 4096 cells, a
    previous score map of 1, 2 and 4 on a 160 x 160 block - so the products tie all over the place - and a belief prior * 2^k."""
    rng = np.random.default_rng(33)
    mats = np.concatenate([aerial.rigid_matrix(90.0 * np.arange(4), [0, 0]), FLIP_X[None], FLIP_Y[None], translation(37, -60)[None],
                           np.array([[0.5, 0.0, 128.0, 0.0, 1.0, 3.0]])])
    B = len(mats)
    taps, floor = np.float32([0.5, 0.25]), np.float32(1.0 / 16)
    prev = np.zeros((B, 512, 512), np.float32)
    sprev = np.zeros((B, 512, 512), np.float32)
    for q in range(B):
        cells = rng.choice(384 * 384, size=4096, replace=False)
        prev[q, 64 + cells // 384, 64 + cells % 384] = rng.integers(1, 4, size=4096).astype(np.float32)
        sprev[q, 176:336, 176:336] = 2.0 ** rng.integers(0, 3, size=(160, 160))
    sprev[2, 10:14, 500:504] = 8.0                                # a plateau of the largest score: the jump target is its first cell
    pst = np.float32([[np.argmax(sprev[q]), sprev[q].max(), 0.0, 0.0] for q in range(B)])
    prior = track_affine_ref.predict_c(prev, mats, taps) + float(floor)
    k = 2.0 ** rng.integers(0, 2, size=(B, 512, 512))
    k[:, ::7, ::5] = 0.0                                           # cells the belief leaves out
    bel = (prior * k).astype(np.float32)
    assert (bel.astype(np.float64) == prior * k).all()
    return bel, prev, sprev, pst, mats, taps, floor


def test_exact_inputs_give_the_bits_of_the_float32_restatement():
    m = base()["m"]
    bel, prev, sprev, pst, mats, taps, floor = exact_case()
    B = len(mats)
    got_v, got_st = run_step(m, bel, prev, sprev, pst, mats, taps, floor)
    ref = vref.step(bel, prev, sprev, pst, mats, taps, floor, dtype=np.float32)
    eq(got_v.cpu(), torch.from_numpy(ref["v"]))
    eq(got_st.cpu(), torch.from_numpy(ref["stats"].astype(np.float32)))
    for q in range(B):                                             # the plateaus are there: the largest score is taken by many cells
        assert int((ref["v"][q] == ref["v"][q].max()).sum()) > 1, q
    assert (ref["jump"] > 0).all() and all((ref["win"][q] > ref["jump"][q]).any() and (ref["win"][q] < ref["jump"][q]).any() for q in range(B))
    # the backtrack: cells all over the images of the block and outside them, the third query's plateau as the jump target
    rng = np.random.default_rng(34)
    kinds = set()
    inv = [aerial.affine_invert(mt) for mt in mats]                # source position -> output position
    for _ in range(12):
        src = 256 + rng.integers(-90, 90, size=(B, 2))
        cells = np.int32([int(round(iv[3] * sx + iv[4] * sy + iv[5])) * 512 + int(round(iv[0] * sx + iv[1] * sy + iv[2])) for iv, (sx, sy) in zip(inv, src)])
        cells = np.where((cells >= 0) & (cells < N), cells, 0).astype(np.int32)
        cells[-1] |= 1                                             # an odd column of the half-scale map: its middle sample sits between two cells
        back = viterbi.track_viterbi_back_affine(m, cu(sprev), cu(pst), cu(cells), mats, taps, floor).cpu().numpy()
        for q in range(B):
            want = vref.back(sprev[q], pst[q], int(cells[q]), mats[q], taps, floor, dtype=np.float32)
            assert tuple(back[q]) == want, (q, cells[q], back[q], want)
            kinds.add(want[1])
            if want[1] == vref.MOVE:                               # ... and the candidates do tie, across cells and within one
                idx, vals = vref.back_candidates(sprev[q], int(cells[q]), mats[q], taps, dtype=np.float32)
                top = idx[vals == vals.max()]
                kinds.add("tie" if np.unique(top).size > 1 else "single")
                if top.size > np.unique(top).size:
                    kinds.add("two samples, one cell")
    assert {vref.MOVE, "tie", "two samples, one cell"} <= kinds, kinds
    far = np.int32([5 * 512 + 5] * B)                              # off every image of the block: no window value, the jump
    back = viterbi.track_viterbi_back_affine(m, cu(sprev), cu(pst), cu(far), mats, taps, floor).cpu().numpy()
    for q in range(B):
        assert tuple(back[q]) == (int(pst[q, 0]), viterbi.LINK_JUMP) == vref.back(sprev[q], pst[q], int(far[q]), mats[q], taps, floor, dtype=np.float32), q
    assert int(pst[2, 0]) == 10 * 512 + 500


# ---- 4. the same bits across call forms ---------------------------------------------------------------------------------------------

FORM_CASES = [("step", "heat", rigid(0.5, [3.37, 0.81]), 1e-9), ("step", "heat", rigid(37.5, [-30.6, 20.2]), 0.37),
              ("rnd", "rnd2", rigid(-20.0, [-4.25, 9.0], 1.25), 1e-9)]


def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    bel, prev, sprev, pst, mats, floor = batch_of(FORM_CASES)
    t = aerial.gaussian_taps(2.5, 6)
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    got, st = viterbi.track_viterbi_affine(m, *args, mats, t, floor)
    cells = st[:, 0].to(torch.int32)
    back = viterbi.track_viterbi_back_affine(m, args[2], args[3], cells, mats, t, floor)
    assert (back[:, 1] == viterbi.LINK_MOVE).any()
    rep, rst = viterbi.track_viterbi_affine(m, *args, mats, np.tile(t, (3, 1)), floor)          # shared against repeated taps
    eq(got, rep); eq(st, rst)
    eq(back, viterbi.track_viterbi_back_affine(m, args[2], args[3], cells, mats, np.tile(t, (3, 1)), floor))
    again, ast = viterbi.track_viterbi_affine(m, *args, mats, t, floor)                         # a second call, and into a tensor of the caller
    eq(got, again); eq(st, ast)
    out = torch.empty_like(got)
    o, ost = viterbi.track_viterbi_affine(m, *args, mats, t, floor, out=out)
    assert o.data_ptr() == out.data_ptr()
    eq(got, out); eq(st, ost)
    eq(back, viterbi.track_viterbi_back_affine(m, args[2], args[3], cells, cu(mats), t, floor))
    with pytest.raises(ValueError, match="none of the input maps"):
        viterbi.track_viterbi_affine(m, *args, mats, t, floor, out=args[2])
    for q in range(3):                                                                          # each query alone
        one, ost = viterbi.track_viterbi_affine(m, *[a[q:q + 1] for a in args], mats[q:q + 1], t, floor[q:q + 1])
        eq(got[q:q + 1], one); eq(st[q:q + 1], ost)
        eq(back[q:q + 1], viterbi.track_viterbi_back_affine(m, args[2][q:q + 1], args[3][q:q + 1], cells[q:q + 1], mats[q], t, floor[q:q + 1]))
    same = [a[:1].expand(3, *a.shape[1:]).contiguous() for a in args]                            # [6] against the repeated [B,6]
    one, ost = viterbi.track_viterbi_affine(m, *same, mats[1], t, floor)
    rep, rst = viterbi.track_viterbi_affine(m, *same, np.tile(mats[1], (3, 1)), t, floor)
    eq(one, rep); eq(ost, rst)
    eq(viterbi.track_viterbi_back_affine(m, same[2], same[3], cells, mats[1], t, floor),
       viterbi.track_viterbi_back_affine(m, same[2], same[3], cells, np.tile(mats[1], (3, 1)), t, floor))
    for a, raw in zip(args, (bel, prev, sprev, pst)):              # no input is written
        eq(a, cu(raw))


def test_two_streams_with_two_work_buffers_do_not_meet():
    m = base()["m"]
    lib = _lib.load()
    bel, prev, sprev, pst, mats, floor = batch_of(FORM_CASES)
    B = 3
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    t6, t32 = aerial.gaussian_taps(2.5, 6), aerial.gaussian_taps(11.0, 32)
    other = np.stack([rigid(-5.0, [1.0, 2.0]), rigid(90.0, [0.5, -0.25]), rigid(10.0, [4.0, 4.0], 0.8)])
    serial = [viterbi.track_viterbi_affine(m, *args, mats, t6, floor), viterbi.track_viterbi_affine(m, *args, other, t32, floor)]
    mt = [cu(mats), cu(other)]
    tp = [cu(t6), cu(t32)]
    fl = cu(floor)
    outs = [(torch.empty(B, 512, 512, device="cuda"), torch.empty(B, 4, device="cuda"),
             torch.empty(lib.ccvpe_track_viterbi_work_bytes(B), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for m_, t_, r, (o, st, wk), stream in zip(mt, tp, (6, 32), outs, streams):
            rc = lib.ccvpe_track_viterbi_affine(m._handle, *[a.data_ptr() for a in args], B, m_.data_ptr(), t_.data_ptr(), 0, r, fl.data_ptr(),
                                                o.data_ptr(), st.data_ptr(), wk.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (ws, wst) in zip(outs, serial):
        eq(o, ws); eq(st, wst)


# ---- 5. degenerate queries between ordinary ones -------------------------------------------------------------------------------------

def test_degenerate_queries_get_their_rule_and_the_healthy_query_keeps_its_bits():
    m = base()["m"]
    t = aerial.gaussian_taps(2.5, 6)
    B = 9
    bel, prev, sprev, pst, mats, floor = batch_of([FORM_CASES[0]] * B)
    h_v, h_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], mats[:1], t, floor[:1])
    j = int(pst[0, 0])
    h_cell = h_st[:, 0].to(torch.int32)
    h_back = viterbi.track_viterbi_back_affine(m, cu(sprev[:1]), cu(pst[:1]), h_cell, mats[:1], t, floor[:1])
    bel, prev, sprev, pst = bel.copy(), prev.copy(), sprev.copy(), pst.copy()
    bel[1] = 0.0                                     # a zero belief: degenerate
    bel[2, 200, 300] = np.nan                        # a NaN in the belief: not taken, the query with a zero there
    prev[3, 250, 250] = np.nan                       # a NaN in the previous belief: the prior around it is NaN, those cells score 0
    sprev[4] = 0.0                                   # a zero previous score map: a restart
    pst[5, 0], pst[6, 0], pst[7, 0] = -1.0, np.nan, float(N)        # no previous index: restarts
    got, st = run_step(m, bel, prev, sprev, pst, mats, t, floor)
    cells = np.int32([int(h_cell[0]), 5, 5, 5, 5, 5, -1, N, int(h_cell[0])])
    back = viterbi.track_viterbi_back_affine(m, cu(sprev), cu(pst), cu(cells), mats, t, floor).cpu().numpy()
    for q in (0, 8):                                 # the healthy query, at both ends of the batch
        eq(got[q:q + 1], h_v); eq(st[q:q + 1], h_st)
        assert tuple(back[q]) == tuple(h_back[0].cpu().numpy())
    assert not bool(got[1].any()) and st[1, 0].item() == -1 and np.isnan(st[1, 1].item()) and np.isnan(st[1, 2].item()) and st[1, 3].item() == 0
    zeroed = bel[2:3].copy()
    zeroed[0, 200, 300] = 0.0
    z_v, z_st = run_step(m, zeroed, prev[2:3], sprev[2:3], pst[2:3], mats[2:3], t, floor[2:3])
    eq(got[2:3], z_v); eq(st[2:3], z_st)
    assert got[2, 200, 300].item() == 0
    # the NaN of the previous belief poisons the prior of the cells whose samples and blur reach it, and nothing else
    assert not bool(torch.isnan(got[3]).any()) and st[3, 0].item() >= 0 and st[3, 3].item() == 0
    changed = (got[3] != h_v[0]).nonzero()
    if int(h_st[0, 0].item()) == int(st[3, 0].item()):
        assert changed.numel() > 0 and not bool(got[3][changed[:, 0], changed[:, 1]].any())
        assert int((changed[:, 0] - 250).abs().max()) <= 16 and int((changed[:, 1] - 250).abs().max()) <= 16
    for q in (4, 5, 6, 7):                           # the four restarts hold the same maps: the same bits, restarted = 1
        eq(got[q], got[4]); eq(st[q], st[4])
    assert st[4, 3].item() == 1 and st[4, 0].item() >= 0 and 1.0 <= st[4, 1].item() < 2.0
    ref = vref.step(bel[4:5], prev[4:5], sprev[4:5], pst[4:5], mats[4], t, floor[4:5])
    w = np.ldexp(got[4].double().cpu().numpy(), int(st[4, 2].item()))
    big = ref["w"][0] >= 2.0 ** -100
    assert (np.abs(w[big] - ref["w"][0][big]) <= 2 * bound_w(6) * ref["w"][0][big]).all() and ref["stats"][0, 3] == 1
    assert tuple(back[4]) == (j, viterbi.LINK_START)
    assert tuple(back[5]) == (-1, viterbi.LINK_START)
    assert tuple(back[6]) == (-1, viterbi.LINK_START) and tuple(back[7]) == (-1, viterbi.LINK_START)
    lone = viterbi.track_viterbi_back_affine(m, cu(sprev[:2]), cu(pst[:2]), cu(np.int32([-1, N])), mats[:2], t, floor[:2]).cpu().numpy()
    assert tuple(lone[0]) == (j, viterbi.LINK_START) and tuple(lone[1]) == (j, viterbi.LINK_START)
    a_v, a_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], mats[:1], t, floor[:1])      # nothing is left behind
    eq(a_v, h_v); eq(a_st, h_st)
    # a singular matrix under a positive floor: every surviving link is a JUMP through the floor
    s_v, s_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], np.zeros((1, 6)), t, np.float32([1e-3]))
    assert s_st[0, 0].item() >= 0 and s_st[0, 3].item() == 0
    s_back = viterbi.track_viterbi_back_affine(m, cu(sprev[:1]), cu(pst[:1]), s_st[:, 0].to(torch.int32), np.zeros((1, 6)), t, np.float32([1e-3]))
    assert tuple(s_back[0].cpu().numpy()) == (j, viterbi.LINK_JUMP)
    # ... and under floor 0 the belief cannot be reached at all: lik = inf, degenerate
    d_v, d_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], translation(700.0, 0.0)[None], t, np.float32([0.0]))
    assert not bool(d_v.any()) and d_st[0, 0].item() == -1 and np.isnan(d_st[0, 1].item()) and d_st[0, 3].item() == 0


# ---- 6. launches -------------------------------------------------------------------------------------------------------------------

def test_two_launches_per_step_and_one_per_link():
    m = base()["m"]
    lib = _lib.load()
    bel, prev, sprev, pst, mats, floor = batch_of(FORM_CASES[:2])
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    mt, fl = cu(mats), cu(floor)
    cells = torch.tensor([1000, -1], dtype=torch.int32, device="cuda")

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    assert count(lambda: viterbi.track_viterbi_affine(m, args[0])) == 2
    for r in (0, 6, 32):
        taps = cu(aerial.gaussian_taps(2.0, r))
        assert count(lambda: viterbi.track_viterbi_affine(m, *args, mt, taps, fl)) == 2
        assert count(lambda: viterbi.track_viterbi_back_affine(m, args[2], args[3], cells, mt, taps, fl)) == 1


# ---- 7. streams --------------------------------------------------------------------------------------------------------------------

class _LogitsStream:
    """the model behind a tracker whose update half reads the next logits of a list instead of running the network"""

    def __init__(self, m, logits):
        self._m, self._logits = m, iter(logits)
        self._ori = torch.zeros(1, 2, 512, 512, device="cuda")
        self._ori[:, 0] = 1.0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def track_update(self, grd, sat, prior):
        return self._m.track_update_logits(cu(next(self._logits)[None]), self._ori, prior)


def device_path(m, logits, matrices, taps, floor):
    tr = smooth.RecordingAffineTracker()
    stream = _LogitsStream(m, logits)
    grd, sat = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8)
    for k in range(len(logits)):
        tr.step(stream, grd, sat, IDENTITY if matrices[k] is None else matrices[k], taps, floor)
    return tr, viterbi.map_path_affine(m, tr.log)


def test_turning_stream_on_the_device_walks_the_float64_path():
    m = base()["m"]
    ref = track_affine_ref
    frames, _, matrices, want_cells, want_links, _, (taps, floor) = vref.turning_path()
    tr, (cells, links, stats, scores) = device_path(m, [ref.sequence_logits(k) for k in frames], matrices, taps, floor)
    first = int(tr.log[0][0].argmax().item())
    assert track_ref.pixel_distance(first, ref.SEQ_DISTRACTOR) <= 1.0               # the filter starts on the distractor ...
    assert cells[:, 0].tolist() == want_cells.tolist()                               # ... the path does not
    assert links[:, 0].tolist() == want_links.tolist() == [viterbi.LINK_START] + [viterbi.LINK_MOVE] * (len(frames) - 1)
    assert stats[:, 0, 3].tolist() == [1.0] + [0.0] * (len(frames) - 1) and len(scores) == len(frames)


def test_relocalising_turning_stream_on_the_device_jumps_once():
    m = base()["m"]
    truth, _, matrices, want_cells, want_links, _, (taps, floor) = vref.reloc_path()
    _, (cells, links, _, _) = device_path(m, [vref.reloc_logits(k) for k in range(vref.RELOC_T)], matrices, taps, floor)
    assert cells[:, 0].tolist() == want_cells.tolist()
    assert links[:, 0].tolist() == want_links.tolist()
    assert [t for t, k in enumerate(links[:, 0].tolist()) if k == viterbi.LINK_JUMP] == [vref.RELOC_AT]


# ---- 8. a recorded stream ------------------------------------------------------------------------------------------------------------

def test_recorded_stream_path_is_the_spelled_out_calls():
    m = make("kitti")
    F = 6
    g, s = inputs("kitti", F, seed=23)              # six frames of one stream whose heading-up tiles turn
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    mats = aerial.rigid_matrix(np.array([0.0, 4.0, -7.5, 120.0, 2.0, 0.0]), np.array([[0, 0], [6.5, -2.25], [-3.0, 8.0], [10.0, 10.0], [0.5, 0.5], [4.0, -6.0]]),
                               np.array([1.0, 1.0, 1.0, 1.0, 1.1, 1.0]))
    tr = smooth.RecordingAffineTracker()
    for k in range(F):
        tr.step(m, g[k:k + 1], s[k:k + 1], mats[k], taps, floor)
    kept = [e[0].clone() for e in tr.log]
    cells, links, stats, scores = viterbi.map_path_affine(m, tr.log)
    assert tuple(cells.shape) == (F, 1) == tuple(links.shape) and cells.dtype == torch.int32 and tuple(stats.shape) == (F, 1, 4)
    for k in range(F):
        eq(tr.log[k][0], kept[k])                   # the sweep writes to none of the log's beliefs
    v, st = viterbi.track_viterbi_affine(m, tr.log[0][0])
    vs, sts = [v], [st]
    for k in range(1, F):
        v, st = viterbi.track_viterbi_affine(m, tr.log[k][0], tr.log[k - 1][0], vs[-1], sts[-1], mats[k], taps, floor)
        vs.append(v); sts.append(st)
    for k in range(F):
        eq(scores[k], vs[k]); eq(stats[k], sts[k])
        assert sts[k][0, 0].item() >= 0 and sts[k][0, 3].item() == (1.0 if k == 0 else 0.0)
    cell = sts[-1][:, 0].to(torch.int32)
    eq(cells[F - 1], cell)
    assert links[0, 0].item() == viterbi.LINK_START
    for k in range(F - 1, 0, -1):
        back = viterbi.track_viterbi_back_affine(m, vs[k - 1], sts[k - 1], cell, mats[k], taps, floor)
        eq(links[k], back[:, 1]); eq(cells[k - 1], back[:, 0])
        assert back[0, 1].item() in (viterbi.LINK_MOVE, viterbi.LINK_JUMP) and 0 <= back[0, 0].item() < N
        cell = back[:, 0].contiguous()
