"""The link statistics on the device (ccvpe_track_link, motion.track_link / link_stream / link_moments): against the
float64 restatement tests/link_ref.py within the bound the term counts give, exact where exactness is defined, G the smoother's bits
and Z its evidence, a poisoned query between ordinary ones, four launches, the crafted stream of tests/track_ref.py and a recorded
Oxford stream.

The bound.  u = 2^-24; every term is non-negative, so relative errors add (first order):
    g = s' / prior                          tests/test_smooth_gpu.py's row                                                4r + 14
    a tile's D[ky][kx]                      32 fused multiply-adds in a row, 5 additions over the 32 rows         + 37     4r + 51
    an offset's 256 tile sums               four chains of 63 additions, then 2                                   + 65     4r + 116
    moves = (uy * ux) * D                   2 u in each merged weight (against the exact f t + (1 - f) t'),
                                            the product of the two, the product with D                            + 6      4r + 122
    M = sum moves                           17 additions in a thread, 6 shuffles, 3 waves                         + 26     4r + 148
    G, Sb                                   tests/test_smooth_gpu.py's chain of 21 on g and on b                           4r + 35, 21
    J = (floor * G) * Sb                    two products                                                                   4r + 58
    Z = M + J                               one addition on the larger of the two errors                                   4r + 149
The tests allow twice these wherever the reference value is >= 2^-100 (below: got <= 2^-99)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, motion, smooth
from tests import link_ref, smooth_ref, track_ref
from tests.test_smooth_gpu import QUERIES, base, batch_of, bound_z, dyadic_case, moved
from tests.test_track_gpu import eq, eq_nan, inputs

pytestmark = pytest.mark.gpu

N = 512 * 512
U = 2.0 ** -24
TINY = 2.0 ** -100


def bounds(r):
    """relative bounds of (moves, Z, G, J, M)"""
    return (4 * r + 122) * U, (4 * r + 149) * U, (4 * r + 35) * U, (4 * r + 58) * U, (4 * r + 148) * U


def check_against_ref(got_mv, got_st, ref, r, what):
    """moves and stats of every query of a call against the restatement -> worst error over bound"""
    mv, st = got_mv.double().cpu().numpy(), got_st.double().cpu().numpy()
    bm, *bs = bounds(r)
    worst = 0.0
    for q in range(mv.shape[0]):
        want, wst = ref["moves"][q], ref["stats"][q]
        assert np.isfinite(wst).all() and wst[0] > 0, (what, q, "the reference takes this query for an unusable one")
        big = want >= TINY
        if big.any():
            ratio = float((np.abs(mv[q][big] - want[big]) / (bm * want[big])).max())
            worst = max(worst, ratio)
            assert ratio <= 2.0, (what, q, "moves", ratio)
        assert (mv[q][~big] <= 2 * TINY).all() and (mv[q][want == 0] == 0).all() and not np.isnan(mv[q]).any(), (what, q)
        for col, b in enumerate(bs):
            if wst[col] >= TINY:
                ratio = abs(st[q, col] - wst[col]) / (b * wst[col])
                worst = max(worst, ratio)
                assert ratio <= 2.0, (what, q, motion.LINK_FIELDS[col], st[q, col], wst[col], ratio)
            else:
                assert 0 <= st[q, col] <= 2 * TINY and (wst[col] != 0 or st[q, col] == 0), (what, q, col, st[q, col], wst[col])
        assert got_st[q, 0].item() == np.float32(np.float32(st[q, 3]) + np.float32(st[q, 2])), (what, q)      # Z = M + J, one addition
    print(f"{what}: radius {r}: worst error / bound = {worst:.3f}")
    return worst


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,sigma", [(0, 1.0), (1, 0.7), (6, 2.5)])
def test_follows_the_float64_restatement(r, sigma):
    """Six queries - a forward's heatmap with a next map from a real predict + update, random, corner and uniform maps; fractional,
    integer, negative and off-window shifts; per-query taps; floors 0, 1e-9 and 0.37 - within twice the bounds of the module docstring."""
    m = base()["m"]
    bel, nxt, shift, floor = batch_of(QUERIES)
    taps = aerial.gaussian_taps(np.linspace(0.6 * sigma, 1.2 * sigma, len(QUERIES)), r)     # per-query taps
    b_dev, n_dev = dev(bel, nxt)
    got_mv, got_st = motion.track_link(m, b_dev, n_dev, shift, taps, floor)
    assert tuple(got_mv.shape) == (len(QUERIES), 2 * r + 2, 2 * r + 2) and tuple(got_st.shape) == (len(QUERIES), 4)
    ref = link_ref.link(bel, nxt, shift, taps, floor)
    check_against_ref(got_mv, got_st, ref, r, "restatement")
    # the off-window query (|dx| > 544): nothing can have moved, Z = J
    q = 3
    assert not bool(got_mv[q].any()) and got_st[q, 3].item() == 0 and got_st[q, 0].item() == got_st[q, 2].item() > 0
    # G is the smoother's, bit for bit, and Z its evidence
    _, sst = smooth.track_smooth(m, b_dev, n_dev, shift, taps, floor)
    eq(got_st[:, 1], sst[:, 3])
    for q in range(len(QUERIES)):
        assert sst[q, 0].item() >= 0
        z, e = got_st[q, 0].item(), sst[q, 2].item()
        assert abs(z - e) <= 2 * (bounds(r)[1] + bound_z(r)) * ref["stats"][q, 0], (q, z, e)


def test_follows_the_float64_restatement_at_radius_32():
    """one query: the host reference is 4356 map products"""
    m = base()["m"]
    r = 32
    bel, nxt, shift, floor = batch_of(QUERIES[:1])
    taps = aerial.gaussian_taps(11.0, r)
    b_dev, n_dev = dev(bel, nxt)
    got_mv, got_st = motion.track_link(m, b_dev, n_dev, shift, taps, floor)
    ref = link_ref.link(bel, nxt, shift, taps, floor)
    check_against_ref(got_mv, got_st, ref, r, "restatement")
    _, sst = smooth.track_smooth(m, b_dev, n_dev, shift, taps, floor)
    eq(got_st[:, 1], sst[:, 3])
    assert abs(got_st[0, 0].item() - sst[0, 2].item()) <= 2 * (bounds(r)[1] + bound_z(r)) * ref["stats"][0, 0]
    # next map = belief is allowed: nothing is written to a map
    same_mv, same_st = motion.track_link(m, b_dev, b_dev, shift, taps, floor)
    other_mv, other_st = motion.track_link(m, b_dev, b_dev.clone(), shift, taps, floor)
    eq(same_mv, other_mv); eq(same_st, other_st)


# ---- 2. exact ----------------------------------------------------------------------------------------------------------------------

def dyadic_link(dx, dy, rng, bel, taps, floor):
    """4.20's recipe: an integer belief, taps (1/2, 1/4), floor 1/16 and a next map prior * 2^k on 256 cells, so g = 2^k: every sum exact"""
    sh = np.float32([[dx, dy]])
    prior = track_ref.predict_c(bel[None], sh, taps)[0] + float(floor)
    k = np.zeros((512, 512))
    at = rng.choice(N, size=256, replace=False)
    k.reshape(-1)[at] = 2.0 ** rng.integers(0, 2, size=256)
    nxt = (prior * k).astype(np.float32)
    assert (nxt.astype(np.float64) == prior * k).all()
    return sh, nxt, k


def test_exact_inputs_give_the_rounded_float64_reference_and_an_integer_shift_is_a_zero_shift_on_moved_maps():
    m = base()["m"]
    bel, taps, floor, rng = dyadic_case()
    for dx, dy in ((37, -60), (-64, 5), (0, 0), (12.5, -3.0), (-7.0, 20.5)):
        sh, nxt, k = dyadic_link(dx, dy, rng, bel, taps, floor)
        b_dev, n_dev = dev(bel[None], nxt[None])
        mv, st = motion.track_link(m, b_dev, n_dev, sh, taps, floor)
        ref = link_ref.link(bel[None], nxt[None], sh, taps, floor)
        assert ref["stats"][0, 1] == k.sum() and ref["stats"][0, 3] > 0 and ref["stats"][0, 2] > 0
        eq(mv, torch.from_numpy(ref["moves"].astype(np.float32)).cuda())
        eq(st, torch.from_numpy(ref["stats"].astype(np.float32)).cuda())
        assert (ref["moves"].astype(np.float32).astype(np.float64) == ref["moves"]).all()          # (nothing was rounded)
        if dx == int(dx) and dy == int(dy):
            # the support (cells 64 .. 447) stays inside the window under these moves
            zmv, zst = motion.track_link(m, moved(b_dev, int(dx), int(dy)), n_dev, np.zeros((1, 2)), taps, floor)
            eq(mv, zmv); eq(st, zst)


def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    bel, nxt, shift, floor = batch_of(QUERIES)
    b_dev, n_dev = dev(bel, nxt)
    t = aerial.gaussian_taps(2.5, 6)
    got, st = motion.track_link(m, b_dev, n_dev, shift, t, floor)
    # shared taps against repeated taps
    rep, rst = motion.track_link(m, b_dev, n_dev, shift, np.tile(t, (len(QUERIES), 1)), floor)
    eq(got, rep); eq(st, rst)
    # a second call
    again, ast = motion.track_link(m, b_dev, n_dev, shift, t, floor)
    eq(got, again); eq(st, ast)
    # each query alone
    for q in range(len(QUERIES)):
        one, ost = motion.track_link(m, b_dev[q:q + 1], n_dev[q:q + 1], shift[q:q + 1], t, floor[q:q + 1])
        eq(got[q:q + 1], one); eq(st[q:q + 1], ost)
    # the [B,1,512,512] form of the maps
    four, fst = motion.track_link(m, b_dev[:, None], n_dev[:, None], shift, t, floor)
    eq(got, four); eq(st, fst)


def test_two_streams_with_two_work_buffers_do_not_meet():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, shift, floor = batch_of(QUERIES[:3])
    B = 3
    b_dev, n_dev = dev(bel, nxt)
    t6, t1 = aerial.gaussian_taps(2.5, 6), aerial.gaussian_taps(0.7, 1)
    serial = [motion.track_link(m, b_dev, n_dev, shift, t6, floor), motion.track_link(m, n_dev, b_dev, -shift, t1, floor)]
    sh, tp = dev(shift, -shift), dev(t6, t1)
    fl, = dev(floor)
    args = [(b_dev, n_dev, sh[0], tp[0], 6), (n_dev, b_dev, sh[1], tp[1], 1)]
    outs = [(torch.empty(B, 2 * r + 2, 2 * r + 2, device="cuda"), torch.empty(B, 4, device="cuda"),
             torch.empty(lib.ccvpe_track_link_work_bytes(B, r), dtype=torch.uint8, device="cuda")) for r in (6, 1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for (bb, nn, s_, t_, r), (o, st, wk), stream in zip(args, outs, streams):
            rc = lib.ccvpe_track_link(m._handle, bb.data_ptr(), nn.data_ptr(), B, s_.data_ptr(), t_.data_ptr(), 0, r, fl.data_ptr(),
                                      o.data_ptr(), st.data_ptr(), wk.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (wmv, wst) in zip(outs, serial):
        eq(o, wmv); eq(st, wst)


# ---- 3. queries the arithmetic gives no usable link for, between ordinary ones --------------------------------------------------------

def test_a_poisoned_query_changes_no_bit_of_its_neighbours():
    m = base()["m"]
    t = aerial.gaussian_taps(2.5, 6)
    ordinary = [QUERIES[0], QUERIES[2], QUERIES[5]]
    cases = [ordinary[i % 3] for i in range(5)]
    bel, nxt, shift, floor = batch_of(cases)
    clean, clean_st = motion.track_link(m, *dev(bel, nxt), shift, t, floor)
    bad_b, bad_n = bel.copy(), nxt.copy()
    bad_b[1, 200, 300] = np.nan                      # a NaN in the belief
    bad_n[3] = 0.0                                   # a next map without a positive cell
    got, st = motion.track_link(m, *dev(bad_b, bad_n), shift, t, floor)
    for q in (0, 2, 4):
        eq(got[q], clean[q]); eq(st[q], clean_st[q])
    assert np.isnan(st[1, 0].item()) and np.isnan(st[1, 2].item()) and bool(torch.isnan(got[1]).any())
    assert not bool(got[3].any()) and st[3].tolist() == [0.0, 0.0, 0.0, 0.0]
    mom = motion.link_moments(got, st, shift)
    assert bool(torch.isnan(mom[[1, 3]]).all()) and bool(torch.isfinite(mom[[0, 2, 4]]).all())
    # a zero belief: g is finite under a positive floor, nothing moves, Sb = 0
    zero_b = bel.copy()
    zero_b[0] = 0.0
    got, st = motion.track_link(m, *dev(zero_b, nxt), shift, t, floor)
    assert not bool(got[0].any()) and st[0, 0].item() == 0 and st[0, 1].item() > 0 and st[0, 2].item() == 0
    eq(got[1:], clean[1:]); eq(st[1:], clean_st[1:])
    # nothing is left behind: the clean batch again
    again, again_st = motion.track_link(m, *dev(bel, nxt), shift, t, floor)
    eq(again, clean); eq(again_st, clean_st)


# ---- 4. launches -------------------------------------------------------------------------------------------------------------------

def test_four_launches():
    m = base()["m"]
    lib = _lib.load()
    bel, nxt, shift, floor = batch_of(QUERIES[:2])
    b_dev, n_dev, sh, fl = dev(bel, nxt, shift, floor)
    for r in (0, 6, 32):
        taps = torch.as_tensor(aerial.gaussian_taps(2.0, r)).cuda()
        motion.track_link(m, b_dev, n_dev, sh, taps, fl)
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        motion.track_link(m, b_dev, n_dev, sh, taps, fl)
        torch.cuda.synchronize()
        assert int(lib.ccvpe_launch_count() - n0) == 4


# ---- 5. streams ----------------------------------------------------------------------------------------------------------------------

def test_links_of_the_crafted_stream_are_moves_by_the_odometry():
    """Frames 2 .. 11 of tests/track_ref's stream: the true peak moves by exactly the shift every frame, so every link's mean residual
    is within 0.5 px of 0 and the share of a jump below 1e-3 (tests/link_ref.py on the float64 stream: |mean| < 1e-9, jump <= 1e-6)."""
    m = base()["m"]
    frames = list(range(2, track_ref.SEQ_FRAMES))
    taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
    step, floor = np.float32([track_ref.SEQ_STEP]), np.float32(track_ref.SEQ_FLOOR)
    ori = torch.zeros(1, 2, 512, 512, device="cuda")
    ori[:, 0] = 1.0
    log, belief = [], None
    for k in frames:
        lg = torch.from_numpy(track_ref.sequence_logits(k)[None]).cuda()
        lp = m.track_predict(belief, step, taps, floor) if belief is not None else None
        _, belief = m.track_update_logits(lg, ori, lp)
        log.append((belief, None if k == frames[0] else step, taps, floor))
    maps, _ = smooth.smooth_stream(m, log)
    links = motion.link_stream(m, log, maps)
    assert len(links) == len(frames) - 1
    for t, (mv, st) in enumerate(links):
        mom = motion.link_moments(mv, st, step)[0].tolist()
        assert abs(mom[2]) <= 0.5 and abs(mom[3]) <= 0.5 and mom[1] < 1e-3, (t, mom)
        assert abs(st[0, 0].item() - 1.0) <= 1e-4 and 1.0 < mom[4] < 2.0 and 1.0 < mom[5] < 2.0
    fit = motion.fit_motion(links, [step] * len(links), track_ref.SEQ_RADIUS)
    assert fit["links"] == len(links) and abs(fit["bias"][0]) <= 0.5 and abs(fit["bias"][1]) <= 0.5 and fit["rho"] < 1e-3


def test_recorded_stream_gives_the_spelled_out_links():
    m = base()["m"]
    F = 6
    g, s = inputs("oxford", F, seed=23)             # six frames of one stream; two cached tiles
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]                       # the vehicle crosses the 400-px grid between frames 2 and 3
    odo = np.array([61.0, -9.5])
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    tr = smooth.RecordingTracker()
    for k in range(F):
        tr.step(m, g[k:k + 1], sc, [tile[k]], origins, odo, taps, floor)
    kept = [e[0].clone() for e in tr.log]
    maps, _ = smooth.smooth_stream(m, tr.log)
    links = motion.link_stream(m, tr.log, maps)
    assert len(links) == F - 1
    for k in range(F - 1):
        shift = aerial.oxford_track_shift(origins[tile[k]], origins[tile[k + 1]], odo)
        want, wst = motion.track_link(m, tr.log[k][0], maps[k + 1], shift, taps, floor)
        eq(links[k][0], want); eq_nan(links[k][1], wst)
        assert tuple(want.shape) == (1, 20, 20) and abs(wst[0, 0].item() - 1.0) <= 1e-4
    for k in range(F):
        eq(tr.log[k][0], kept[k])                   # the links write to no belief of the log
    fit = motion.fit_motion(links, [e[1] for e in tr.log[1:]], 9)
    assert fit["links"] == F - 1 and np.isfinite(fit["sigma"]) and 0 <= fit["rho"] <= 1
