"""The smoother on the device (ccvpe_track_smooth, smooth.track_smooth / RecordingTracker / smooth_stream): against the
float64 restatement tests/smooth_ref.py within the bound the term counts give, exact where exactness is defined, the degenerate rules
between ordinary queries, at most three launches, the crafted stream of tests/track_ref.py started on a frame the distractor wins,
and a recorded Oxford stream swept backward.

The bound.  u = 2^-24; every term is non-negative, so relative errors add (first order):
    prior = c + floor                       (4r + 12) u for predict's c, + 1 for the add                       4r + 13
    g = s' / prior                          one rounding: the compiler emits the IEEE division (v_div_scale /
                                            v_div_fmas / v_div_fixup), not a reciprocal                          4r + 14
    G = sum g                               longest chain of additions: 3 in the thread, 6 shuffles, 3 waves,
                                            then 3 + 6 over the 256 tile sums = 21                               4r + 35
    P(g; -d)                                (4r + 12) u on top of g's                                            8r + 26
    a = fma(floor, G, P(g; -d))             one rounding on top of the larger term's error                      <= 8r + 36
    w = b * a                                                                                                    8r + 37
    Z = sum w                               the same chain of 21                                                 8r + 58
    s = w * (1 / Z)                         two roundings                                                       16r + 97
The tests allow twice (16r + 97) u on the map wherever the reference s >= 2^-100 (below: got <= 2^-99), twice (8r + 58) u on Z and
twice (4r + 35) u on G."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth
from tests import smooth_ref, track_ref
from tests.test_track_gpu import eq, eq_nan, inputs, make

pytestmark = pytest.mark.gpu

N = 512 * 512
U = 2.0 ** -24


def bound_s(r):
    return (16 * r + 97) * U


def bound_z(r):
    return (8 * r + 58) * U


def bound_g(r):
    return (4 * r + 35) * U


_BASE = {}


def base():
    """the model, a forward's heatmap, a next map that an actual track_predict + track_update_logits step produced from it, crafted maps"""
    if not _BASE:
        m = make("oxford")
        g, s = inputs("oxford", 2, seed=5)
        logits, _, ori = m(g, s)[:3]
        _, heat = m.track_update_logits(logits[:1], ori[:1])
        lp = m.track_predict(heat, np.array([[3.37, 0.81]]), aerial.gaussian_taps(2.5, 6), 1e-9)
        _, step = m.track_update_logits(logits[1:], ori[1:], lp)
        rng = np.random.default_rng(21)
        rnd = rng.uniform(0.0, 1.0, size=(2, 512, 512)).astype(np.float32)
        rnd /= rnd.reshape(2, -1).sum(axis=1)[:, None, None]
        corner = np.full((512, 512), 1e-12, np.float32)
        corner[0, 0], corner[511, 511], corner[300, 17] = 0.5, 0.25, 0.25
        _BASE.update(m=m, heat=heat[0].cpu().numpy(), step=step[0].cpu().numpy(), rnd=rnd[0], rnd2=rnd[1], corner=corner,
                     uniform=np.full((512, 512), 1.0 / N, np.float32))
    return _BASE


# (belief, next map, dx, dy, floor): fractional, integer, negative and off-window shifts (|d| > 544: a = floor * G), floors 0, 1e-9, 0.37
QUERIES = [("heat", "step", 3.37, 0.81, 1e-9), ("heat", "step", 12.0, -7.0, 0.37), ("rnd", "heat", -130.6, 200.2, 1e-9),
           ("uniform", "step", 600.0, -3.5, 1e-9), ("rnd2", "rnd", -0.5, -0.5, 0.0), ("corner", "rnd2", 0.25, -2.75, 1e-9)]


def batch_of(cases):
    b = base()
    bel = np.stack([b[c[0]] for c in cases])
    nxt = np.stack([b[c[1]] for c in cases])
    return bel, nxt, np.float32([[c[2], c[3]] for c in cases]), np.float32([c[4] for c in cases])


def check_against_ref(got_s, got_st, ref, r, what):
    """the map, the stats and their consistency, for the ordinary queries of a call"""
    s = got_s.double().cpu().numpy()
    st = got_st.double().cpu().numpy()
    flat = got_s.view(got_s.shape[0], -1)
    worst = 0.0
    for q in range(s.shape[0]):
        want, wst = ref["s"][q], ref["stats"][q]
        assert wst[0] >= 0, (what, q, "the reference takes this query for a degenerate one")
        big = want >= 2.0 ** -100
        ratio = float((np.abs(s[q][big] - want[big]) / (bound_s(r) * want[big])).max())
        worst = max(worst, ratio)
        assert ratio <= 2.0, (what, q, ratio)
        assert (s[q][~big] <= 2.0 ** -99).all() and not np.isnan(s[q]).any(), (what, q)
        i = int(st[q, 0])
        assert 0 <= i < N
        top = want.reshape(-1)[int(wst[0])]
        assert i == int(wst[0]) or want.reshape(-1)[i] >= top * (1.0 - 2 * bound_s(r)), (what, q, i, wst[0])
        assert got_st[q, 1].item() == flat[q, i].item() and flat[q, i].item() == flat[q].max().item(), (what, q)
        assert abs(st[q, 2] - wst[2]) <= 2 * bound_z(r) * wst[2], (what, q, st[q, 2], wst[2])
        assert abs(st[q, 3] - wst[3]) <= 2 * bound_g(r) * wst[3], (what, q, st[q, 3], wst[3])
    print(f"{what}: radius {r}: worst error / bound = {worst:.3f}")
    return worst


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,sigma", [(0, 1.0), (1, 0.7), (6, 2.5), (32, 11.0)])
def test_follows_the_float64_restatement(r, sigma):
    m = base()["m"]
    bel, nxt, shift, floor = batch_of(QUERIES)
    taps = aerial.gaussian_taps(np.linspace(0.6 * sigma, 1.2 * sigma, len(QUERIES)), r)     # per-query taps
    got_s, got_st = smooth.track_smooth(m, torch.from_numpy(bel).cuda(), torch.from_numpy(nxt).cuda(), shift, taps, floor)
    ref = smooth_ref.smooth(bel, nxt, shift, taps, floor)
    check_against_ref(got_s, got_st, ref, r, "restatement")
    # the off-window query: a = floor * G for every cell, so the smoothed map is the belief over its mass
    q = 3
    u = bel[q].astype(np.float64)
    np.testing.assert_allclose(got_s[q].double().cpu().numpy(), u / u.sum(), rtol=2 * bound_s(r))
    # Z is the mass of the next map up to the belief's own distance from mass 1
    for q in (0, 1):
        mass, nm = float(bel[q].astype(np.float64).sum()), float(nxt[q].astype(np.float64).sum())
        assert abs(got_st[q, 2].item() - nm) <= (2 * bound_z(r) + abs(mass - 1.0)) * nm, (q, got_st[q, 2].item(), nm, mass)


# ---- 2. exact ----------------------------------------------------------------------------------------------------------------------

def dyadic_case():
    """Maps on which every sum of the recursion is exact in float32, whatever its order: an integer belief on 4096 cells of the middle
    of the grid, taps (1/2, 1/4), floor 1/16 - so prior is a multiple of 1/16 - and a next map prior * 2^k on 256 cells, so g = 2^k."""
    rng = np.random.default_rng(33)
    bel = np.zeros((512, 512), np.float32)
    cells = rng.choice(384 * 384, size=4096, replace=False)
    bel[64 + cells // 384, 64 + cells % 384] = rng.integers(1, 4, size=4096).astype(np.float32)
    return bel, np.float32([0.5, 0.25]), np.float32(1.0 / 16), rng


def moved(t, dx, dy):
    """content moves by (+dx, +dy), zero fill"""
    out = torch.zeros_like(t)
    ys, yd = (slice(0, 512 - dy), slice(dy, 512)) if dy >= 0 else (slice(-dy, 512), slice(0, 512 + dy))
    xs, xd = (slice(0, 512 - dx), slice(dx, 512)) if dx >= 0 else (slice(-dx, 512), slice(0, 512 + dx))
    out[..., yd, xd] = t[..., ys, xs]
    return out


def test_an_integer_shift_is_a_zero_shift_on_moved_maps():
    m = base()["m"]
    bel, taps, floor, rng = dyadic_case()
    for dx, dy in ((37, -60), (-64, 5), (0, 0)):
        sh = np.float32([[dx, dy]])
        prior = track_ref.predict_c(bel[None], sh, taps)[0] + float(floor)
        k = np.zeros((512, 512))
        at = rng.choice(N, size=256, replace=False)
        k.reshape(-1)[at] = 2.0 ** rng.integers(0, 2, size=256)
        nxt = (prior * k).astype(np.float32)
        assert (nxt.astype(np.float64) == prior * k).all()
        b_dev, n_dev = torch.from_numpy(bel[None]).cuda(), torch.from_numpy(nxt[None]).cuda()
        got, st = smooth.track_smooth(m, b_dev, n_dev, sh, taps, floor)
        want, wst = smooth.track_smooth(m, moved(b_dev, dx, dy), n_dev, np.zeros((1, 2)), taps, floor)
        eq(moved(got, dx, dy), want)
        eq(st[:, 1:], wst[:, 1:])
        i, j = int(st[0, 0].item()), int(wst[0, 0].item())
        assert (j % 512 - i % 512, j // 512 - i // 512) == (dx, dy)
        # the sums are exact, so they are the float64 ones
        ref = smooth_ref.smooth(bel[None], nxt[None], sh, taps, floor)
        assert st[0, 2].item() == ref["stats"][0, 2] and st[0, 3].item() == ref["stats"][0, 3] == k.sum()


def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    bel, nxt, shift, floor = batch_of(QUERIES)
    b_dev, n_dev = torch.from_numpy(bel).cuda(), torch.from_numpy(nxt).cuda()
    t = aerial.gaussian_taps(2.5, 6)
    got, st = smooth.track_smooth(m, b_dev, n_dev, shift, t, floor)
    # shared taps against repeated taps
    rep, rst = smooth.track_smooth(m, b_dev, n_dev, shift, np.tile(t, (len(QUERIES), 1)), floor)
    eq(got, rep); eq(st, rst)
    # a second call
    again, ast = smooth.track_smooth(m, b_dev, n_dev, shift, t, floor)
    eq(got, again); eq(st, ast)
    # in place
    run = n_dev.clone()
    out, ost = smooth.track_smooth(m, b_dev, run, shift, t, floor, out=run)
    assert out.data_ptr() == run.data_ptr()
    eq(got, run); eq(st, ost)
    eq(n_dev, torch.from_numpy(nxt).cuda())
    # each query alone
    for q in range(len(QUERIES)):
        one, ost = smooth.track_smooth(m, b_dev[q:q + 1], n_dev[q:q + 1], shift[q:q + 1], t, floor[q:q + 1])
        eq(got[q:q + 1], one); eq(st[q:q + 1], ost)
    # the [B,1,512,512] form of the maps
    four, fst = smooth.track_smooth(m, b_dev[:, None], n_dev[:, None], shift, t, floor)
    eq(got, four); eq(st, fst)


def test_two_streams_with_two_work_buffers_do_not_meet():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, shift, floor = batch_of(QUERIES)
    B = len(QUERIES)
    b_dev, n_dev = torch.from_numpy(bel).cuda(), torch.from_numpy(nxt).cuda()
    t6, t32 = aerial.gaussian_taps(2.5, 6), aerial.gaussian_taps(11.0, 32)
    serial = [smooth.track_smooth(m, b_dev, n_dev, shift, t6, floor), smooth.track_smooth(m, n_dev, b_dev, -shift, t32, floor)]
    sh = [torch.from_numpy(shift).cuda(), torch.from_numpy(-shift).cuda()]
    tp = [torch.from_numpy(t6).cuda(), torch.from_numpy(t32).cuda()]
    fl = torch.from_numpy(floor).cuda()
    args = [(b_dev, n_dev, sh[0], tp[0], 6), (n_dev, b_dev, sh[1], tp[1], 32)]
    outs = [(torch.empty(B, 512, 512, device="cuda"), torch.empty(B, 4, device="cuda"),
             torch.empty(lib.ccvpe_track_smooth_work_bytes(B), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for (bb, nn, s_, t_, r), (o, st, wk), stream in zip(args, outs, streams):
            rc = lib.ccvpe_track_smooth(m._handle, bb.data_ptr(), nn.data_ptr(), B, s_.data_ptr(), t_.data_ptr(), 0, r, fl.data_ptr(),
                                        o.data_ptr(), st.data_ptr(), wk.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (ws, wst) in zip(outs, serial):
        eq(o, ws); eq(st, wst)


def test_radius_zero_is_the_product_of_the_belief_and_the_moved_ratio():
    """radius 0, taps [1], an integer shift, floor 0: prior_j = b_(j - d) exactly, a_i = g_(i + d) exactly, so w_i = fl(b_i * fl(s'_(i + d)
    / b_i)) - two roundings -, Z one chain of 21 additions, 1 / Z and the scale two more: s is within (2 + 2 + 21 + 2) u <= (8 + 21) u of
    the product normalised in float64."""
    b = base()
    m, bel, nxt = b["m"], b["rnd"], b["rnd2"]
    dx, dy = 19, -33
    # cells of the next map whose source lies outside the grid have prior 0 under floor 0: this query keeps clear of them
    inside = moved(torch.ones(512, 512), dx, dy).numpy() > 0
    nxt = np.where(inside, nxt, np.float32(0.0))
    got, st = smooth.track_smooth(m, torch.from_numpy(bel[None]).cuda(), torch.from_numpy(nxt[None]).cuda(), np.float32([[dx, dy]]), np.float32([1.0]), 0.0)
    b64 = bel.astype(np.float64)
    assert (b64 > 0).all()
    w = b64 * (moved(torch.from_numpy(nxt.astype(np.float64)), -dx, -dy).numpy() / b64)       # b_i * (s'_(i + d) / b_i)
    want = w / w.sum()
    err = np.abs(got[0].double().cpu().numpy() - want)
    assert st[0, 0].item() >= 0 and (err <= 29 * U * want).all(), float((err[want > 0] / want[want > 0]).max() / U)


# ---- 3. degenerate queries between ordinary ones -------------------------------------------------------------------------------------

def test_degenerate_queries_get_their_rule_and_their_neighbours_keep_their_bits():
    m = base()["m"]
    r, t = 6, aerial.gaussian_taps(2.5, 6)
    ordinary = [QUERIES[0], QUERIES[2], QUERIES[5]]
    cases = [ordinary[i % 3] for i in range(11)]
    bel, nxt, clean_shift, floor = batch_of(cases)
    shift = clean_shift.copy()
    clean_b, clean_n = torch.from_numpy(bel).cuda(), torch.from_numpy(nxt).cuda()
    clean, clean_st = smooth.track_smooth(m, clean_b, clean_n, clean_shift, t, floor)
    bad_b, bad_n, bad_floor = bel.copy(), nxt.copy(), floor.copy()
    bad_n[1] = 0.0                                   # a zero next map: rule 1
    bad_b[3] = 0.0                                   # a zero belief: rule 2
    bad_b[5, 200, 300] = np.nan                      # a NaN in the belief: rule 2
    bad_n[7, 100, 100], bad_n[7, 17, 400] = np.nan, -1.0     # a NaN and a negative cell in the next map: not taken, an ordinary query
    bad_b[9] = 0.0
    bad_b[9, 256, 256] = 1.0                         # floor 0 and a belief the blur cannot carry to the next map's positive cells: rule 2
    bad_floor[9] = 0.0
    shift[9] = (0.0, 0.0)
    got, st = smooth.track_smooth(m, torch.from_numpy(bad_b).cuda(), torch.from_numpy(bad_n).cuda(), shift, t, bad_floor)
    for q in (0, 2, 4, 6, 8, 10):
        eq(got[q], clean[q]); eq(st[q], clean_st[q])
    # rule 1
    eq(got[1], clean_b[1])
    i = int(clean_b[1].argmax().item())
    assert st[1, 0].item() == i and st[1, 1].item() == clean_b[1].view(-1)[i].item() and np.isnan(st[1, 2].item()) and st[1, 3].item() == 0
    # rule 2
    for q in (3, 5, 9):
        assert not bool(got[q].any()), q
        assert st[q, 0].item() == -1 and np.isnan(st[q, 1].item()), (q, st[q])
    assert st[3, 2].item() == 0 and st[3, 3].item() > 0
    assert np.isnan(st[5, 2].item())
    assert not np.isfinite(st[9, 2].item()) and st[9, 3].item() == float("inf")
    # the next map with holes is the next map with zeros there
    ref = smooth_ref.smooth(bad_b[7:8], bad_n[7:8], shift[7:8], t, bad_floor[7:8])
    check_against_ref(got[7:8], st[7:8], ref, r, "holes in the next map")
    zeros = bad_n[7:8].copy()
    zeros[0, 100, 100], zeros[0, 17, 400] = 0.0, 0.0
    z, zst = smooth.track_smooth(m, torch.from_numpy(bad_b[7:8]).cuda(), torch.from_numpy(zeros).cuda(), shift[7:8], t, bad_floor[7:8])
    eq(got[7:8], z); eq(st[7:8], zst)
    # nothing is left behind: the clean batch again
    again, again_st = smooth.track_smooth(m, clean_b, clean_n, clean_shift, t, floor)
    eq(again, clean); eq(again_st, clean_st)
    # a belief without a value above -inf has no argmax under rule 1
    nan_b = torch.full((1, 512, 512), float("nan"), device="cuda")
    s1, st1 = smooth.track_smooth(m, nan_b, torch.zeros(1, 512, 512, device="cuda"), np.zeros((1, 2)), t, 1e-9)
    eq_nan(s1, nan_b)
    assert st1[0, 0].item() == -1 and np.isnan(st1[0, 1].item()) and np.isnan(st1[0, 2].item()) and st1[0, 3].item() == 0


# ---- 4. launches -------------------------------------------------------------------------------------------------------------------

def test_three_launches_and_predict_is_still_one():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, shift, floor = batch_of(QUERIES[:2])
    b_dev, n_dev = torch.from_numpy(bel).cuda(), torch.from_numpy(nxt).cuda()
    sh, fl = torch.from_numpy(shift).cuda(), torch.from_numpy(floor).cuda()

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for r in (0, 6, 32):
        taps = torch.as_tensor(aerial.gaussian_taps(2.0, r)).cuda()
        smooth.track_smooth(m, b_dev, n_dev, sh, taps, fl)
        assert 1 <= count(lambda: smooth.track_smooth(m, b_dev, n_dev, sh, taps, fl)) <= 3
        m.track_predict(b_dev, sh, taps, fl)
        assert count(lambda: m.track_predict(b_dev, sh, taps, fl)) == 1


# ---- 5. the smoother does its job ----------------------------------------------------------------------------------------------------

def test_the_smoother_moves_the_first_frame_off_the_distractor():
    m = base()["m"]
    frames, _, ref_smoothed, _, (step, taps, floor) = smooth_ref.crafted_stream(2)
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0
    beliefs, belief = {}, None
    for k in frames:
        lg = torch.from_numpy(track_ref.sequence_logits(k)[None]).cuda()
        lp = m.track_predict(belief, step, taps, floor) if belief is not None else None
        rows, belief = m.track_update_logits(lg, ori, lp)
        beliefs[k] = belief
        if k == frames[0]:
            i = int(rows[0, 0].item())
            assert track_ref.pixel_distance(i, track_ref.SEQ_DISTRACTOR) <= 1.0 and track_ref.pixel_distance(i, track_ref.sequence_truth(k)) > 300.0
    s = beliefs[frames[-1]]
    for k in reversed(frames):
        if k != frames[-1]:
            s, st = smooth.track_smooth(m, beliefs[k], s, step, taps, floor)
            i = int(st[0, 0].item())
            assert abs(st[0, 2].item() - 1.0) <= 1e-4
        else:
            i = int(s.argmax().item())
        assert i == int(np.argmax(ref_smoothed[k])), (k, i)
        assert track_ref.pixel_distance(i, track_ref.sequence_truth(k)) <= 1.0, (k, i)


# ---- 6. RecordingTracker and smooth_stream ---------------------------------------------------------------------------------------------

def test_recorded_stream_is_swept_by_the_spelled_out_calls():
    m = base()["m"]
    F = 6
    g, s = inputs("oxford", F, seed=23)             # six frames of one stream; two cached tiles
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]                       # the vehicle crosses the 400-px grid between frames 2 and 3
    motion = np.array([61.0, -9.5])
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    tr, plain = smooth.RecordingTracker(), aerial.Tracker()
    for k in range(F):
        rows = tr.step(m, g[k:k + 1], sc, [tile[k]], origins, motion, taps, floor)
        eq(rows, plain.step(m, g[k:k + 1], sc, [tile[k]], origins, motion, taps, floor))
        eq(tr.belief, plain.belief)
    assert len(tr.log) == F and tr.log[0][1] is None
    kept = [e[0].clone() for e in tr.log]
    maps, stats = smooth.smooth_stream(m, tr.log)
    maps2, stats2 = smooth.smooth_stream(m, tr.log, in_place=True)
    for k in range(F):
        eq(tr.log[k][0], kept[k])                   # neither sweep writes to the log's beliefs
    # spelled out
    want = tr.log[-1][0]
    eq(maps[-1], want)
    i = int(want.argmax().item())
    assert stats[-1, 0, 0].item() == i and stats[-1, 0, 1].item() == want.view(-1)[i].item() and np.isnan(stats[-1, 0, 2].item())
    for k in range(F - 2, -1, -1):
        shift = aerial.oxford_track_shift(origins[tile[k]], origins[tile[k + 1]], motion)
        want, wst = smooth.track_smooth(m, tr.log[k][0], want, shift, taps, floor)
        eq(maps[k], want); eq(stats[k], wst)
        assert wst[0, 0].item() >= 0 and abs(wst[0, 2].item() - 1.0) <= 1e-4
    for a, b_ in zip(maps, maps2):
        eq(a, b_)
    eq_nan(stats, stats2)
