"""The MAP trajectory on the device (ccvpe_track_viterbi, ccvpe_track_viterbi_back, viterbi.track_viterbi / track_viterbi_back /
map_path): against the float64 definition tests/viterbi_ref.py within the bound the roundings give, bit-equal to the
float32 restatement on inputs with exact arithmetic (ties included), the same bits across call forms, the degenerate rules between
ordinary queries, the launch counts, the crafted and the relocalisation stream, and a recorded Oxford stream.

The bound.  u = 2^-24, relative, first order, against a float64 evaluation on the same float32 inputs:
    lik = b / prior                         prior (4r + 13) u as in tests/test_smooth_gpu.py, one IEEE division               4r + 14
    a merged weight fma(f, ta, (1 - f) tc)  1 - f exact or one rounding, the product, the fma                                 2
    win = uy * (ux * v-)                    two weights, two products; the maxima are exact                                   6
    jump = floor * peak                                                                                                       1
    w = lik * max(win, jump)                (4r + 14) + 6 + 1                                                                  4r + 21
    v = ldexpf(w, -e)                       exact (the results here are not subnormal)
The tests allow twice (4r + 21) u on w wherever the reference is >= 2^-100, and twice 6 u between backtrack candidates."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth, viterbi
from tests import track_ref, viterbi_ref
from tests.test_track_gpu import eq, inputs, make

pytestmark = pytest.mark.gpu

N = 512 * 512
U = 2.0 ** -24


def bound_w(r):
    return (4 * r + 21) * U


BOUND_WIN = 6 * U

_BASE = {}


def base():
    """the model, a forward's heatmap, the belief an actual track_predict + track_update_logits step made of it, random maps, and the
    first-frame score map and stats of each map that serves as a previous frame"""
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
        maps = dict(heat=heat[0].cpu().numpy(), step=step[0].cpu().numpy(), rnd=rnd[0], rnd2=rnd[1])
        first = {}
        for k in ("heat", "rnd", "rnd2"):
            v, st = viterbi.track_viterbi(m, torch.from_numpy(maps[k][None]).cuda())
            first[k] = (v[0].cpu().numpy(), st[0].cpu().numpy())
        _BASE.update(m=m, maps=maps, first=first)
    return _BASE


# (belief, previous belief, dx, dy, floor): fractional, integer, negative and off-window shifts (|d| > 544: win = 0, every cell jumps),
# floors 0, 1e-9, 0.37
QUERIES = [("step", "heat", 3.37, 0.81, 1e-9), ("step", "heat", 12.0, -7.0, 0.37), ("rnd", "heat", -130.6, 200.2, 1e-9),
           ("step", "rnd2", 600.0, -3.5, 1e-9), ("rnd2", "rnd", -0.5, -0.5, 0.0)]
BATCHES = [QUERIES[:3], QUERIES[3:]]


def batch_of(cases):
    b = base()
    bel = np.stack([b["maps"][c[0]] for c in cases])
    prev = np.stack([b["maps"][c[1]] for c in cases])
    sprev = np.stack([b["first"][c[1]][0] for c in cases])
    pst = np.stack([b["first"][c[1]][1] for c in cases])
    return bel, prev, sprev, pst, np.float32([[c[2], c[3]] for c in cases]), np.float32([c[4] for c in cases])


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_step(m, bel, prev, sprev, pst, shift, taps, floor):
    return viterbi.track_viterbi(m, cu(bel), cu(prev), cu(sprev), cu(pst), shift, taps, floor)


# ---- 1. against the float64 definition -------------------------------------------------------------------------------------------

def test_first_frame_is_the_belief_scaled_by_a_power_of_two():
    b = base()
    for k in ("heat", "rnd"):
        v, st = b["first"][k]
        src = b["maps"][k]
        i = int(np.argmax(src))
        e = int(st[2])
        assert st[0] == i and st[3] == 1 and 1.0 <= st[1] < 2.0 and st[1] == v.reshape(-1)[i]
        np.testing.assert_array_equal(v, np.ldexp(src, -e))
        assert np.ldexp(np.float64(src.max()), -e) == st[1]


@pytest.mark.parametrize("r,sigma", [(0, 1.0), (1, 0.7), (6, 2.5), (32, 11.0)])
def test_follows_the_float64_definition(r, sigma):
    m = base()["m"]
    worst = worst_back = 0.0
    rng = np.random.default_rng(100 + r)
    for cases in BATCHES:
        B = len(cases)
        bel, prev, sprev, pst, shift, floor = batch_of(cases)
        taps = aerial.gaussian_taps(np.linspace(0.6 * sigma, 1.2 * sigma, B), r)          # per-query taps
        got_v, got_st = run_step(m, bel, prev, sprev, pst, shift, taps, floor)
        ref = viterbi_ref.step(bel, prev, sprev, pst, shift, taps, floor)
        v, st = got_v.double().cpu().numpy(), got_st.double().cpu().numpy()
        for q in range(B):
            want = ref["w"][q]
            assert ref["stats"][q, 0] >= 0 and st[q, 3] == 0 == ref["stats"][q, 3], (cases[q], st[q])
            w = np.ldexp(v[q], int(st[q, 2]))
            big = want >= 2.0 ** -100
            ratio = float((np.abs(w[big] - want[big]) / (bound_w(r) * want[big])).max())
            worst = max(worst, ratio)
            print(f"radius {r} {cases[q]}: worst error / bound = {ratio:.3f}, exponent {int(st[q, 2])}")
            assert ratio <= 2.0, (cases[q], ratio)
            assert not np.isnan(v[q]).any() and (v[q] >= 0).all()
            i = int(st[q, 0])
            assert 0 <= i < N and want.reshape(-1)[i] >= want.max() * (1.0 - 2 * bound_w(r)), (cases[q], i)
            assert 1.0 <= st[q, 1] < 2.0 and st[q, 1] == v[q].reshape(-1)[i] == v[q].max()
            assert i == int(np.argmax(v[q]))                                                # the first index of the largest score
        # the backtrack of a few cells per query against the float64 candidates: the step's argmax, the corners, random cells
        for cells in [st[:, 0].astype(np.int64)] + [np.full(B, c) for c in (0, N - 1)] + [rng.integers(0, N, size=B) for _ in range(3)]:
            back = viterbi.track_viterbi_back(m, cu(sprev), cu(pst), cu(cells.astype(np.int32)), shift, taps, floor).cpu().numpy()
            for q in range(B):
                j = int(pst[q, 0])
                idx, vals = viterbi_ref.back_candidates(sprev[q], int(cells[q]), shift[q], taps[q])
                best = float(vals.max()) if vals.size else -np.inf
                jump = float(np.float64(floor[q]) * np.float64(sprev[q].reshape(-1)[j]))
                prev_cell, kind = int(back[q, 0]), int(back[q, 1])
                tol = 2 * BOUND_WIN
                if jump > best * (1 + tol) and jump > 0:
                    assert (prev_cell, kind) == (j, viterbi.LINK_JUMP), (cases[q], cells[q], back[q], best, jump)
                elif best > jump * (1 + tol) and best > 0:
                    assert kind == viterbi.LINK_MOVE, (cases[q], cells[q], back[q], best, jump)
                if kind == viterbi.LINK_MOVE:
                    at = np.nonzero(idx == prev_cell)[0]
                    assert at.size == 1 and vals[at[0]] >= best * (1 - tol), (cases[q], cells[q], back[q])
                    worst_back = max(worst_back, float((best - vals[at[0]]) / (BOUND_WIN * best)))
                elif kind == viterbi.LINK_JUMP:
                    assert prev_cell == j and jump >= best * (1 - tol)
                else:
                    assert prev_cell == j and not best > 0 and not jump > 0
    print(f"radius {r}: worst w error / bound {worst:.3f}, worst backtrack gap / bound {worst_back:.3f}")


# ---- 2. exact ----------------------------------------------------------------------------------------------------------------------

def exact_case():
    """Three queries on which every operation of the step is exact in float32: integer shifts, taps (1/2, 1/4), floor 1/16, an integer
    previous belief on 4096 cells - so prior is a multiple of 1/16 -, a previous score map of 1, 2 and 4 on a 160 x 160 block - so the
    products tie all over the place - and a belief prior * 2^k, so lik = 2^k."""
    rng = np.random.default_rng(33)
    shift = np.float32([[37, -60], [-64, 5], [0, 0]])
    taps, floor = np.float32([0.5, 0.25]), np.float32(1.0 / 16)
    prev = np.zeros((3, 512, 512), np.float32)
    sprev = np.zeros((3, 512, 512), np.float32)
    for q in range(3):
        cells = rng.choice(384 * 384, size=4096, replace=False)
        prev[q, 64 + cells // 384, 64 + cells % 384] = rng.integers(1, 4, size=4096).astype(np.float32)
        sprev[q, 176:336, 176:336] = 2.0 ** rng.integers(0, 3, size=(160, 160))
    sprev[2, 10:14, 500:504] = 8.0                                # a plateau of the largest score: the jump target is its first cell
    pst = np.float32([[np.argmax(sprev[q]), sprev[q].max(), 0.0, 0.0] for q in range(3)])
    prior = track_ref.predict_c(prev, shift, taps) + float(floor)
    k = 2.0 ** rng.integers(0, 2, size=(3, 512, 512))
    k[:, ::7, ::5] = 0.0                                           # cells the belief leaves out
    bel = (prior * k).astype(np.float32)
    assert (bel.astype(np.float64) == prior * k).all()
    return bel, prev, sprev, pst, shift, taps, floor


def test_exact_inputs_give_the_bits_of_the_float32_restatement():
    m = base()["m"]
    bel, prev, sprev, pst, shift, taps, floor = exact_case()
    got_v, got_st = run_step(m, bel, prev, sprev, pst, shift, taps, floor)
    ref = viterbi_ref.step(bel, prev, sprev, pst, shift, taps, floor, dtype=np.float32)
    eq(got_v.cpu(), torch.from_numpy(ref["v"]))
    eq(got_st.cpu(), torch.from_numpy(ref["stats"].astype(np.float32)))
    for q in range(3):                                             # the plateaus are there: the largest score is taken by many cells
        assert int((ref["v"][q] == ref["v"][q].max()).sum()) > 1, q
    assert (ref["jump"] > 0).all() and all((ref["win"][q] > ref["jump"][q]).any() and (ref["win"][q] < ref["jump"][q]).any() for q in range(3))
    # the backtrack: cells all over the moved block and outside it, the last query's plateau as the jump target
    rng = np.random.default_rng(34)
    kinds = set()
    for _ in range(16):
        cells = np.int32([(256 + rng.integers(-90, 90) + int(shift[q, 1])) * 512 + 256 + rng.integers(-90, 90) + int(shift[q, 0]) for q in range(3)])
        back = viterbi.track_viterbi_back(m, cu(sprev), cu(pst), cu(cells), shift, taps, floor).cpu().numpy()
        for q in range(3):
            want = viterbi_ref.back(sprev[q], pst[q], int(cells[q]), shift[q], taps, floor, dtype=np.float32)
            assert tuple(back[q]) == want, (q, cells[q], back[q], want)
            kinds.add(want[1])
            if want[1] == viterbi_ref.MOVE:                        # ... and the candidates do tie
                _, vals = viterbi_ref.back_candidates(sprev[q], int(cells[q]), shift[q], taps, dtype=np.float32)
                kinds.add("tie" if int((vals == vals.max()).sum()) > 1 else "single")
    assert {viterbi_ref.MOVE, "tie"} <= kinds
    far = np.int32([5 * 512 + 5, 500 * 512 + 20, 12 * 512 + 400])   # off the block: no window value, the jump
    back = viterbi.track_viterbi_back(m, cu(sprev), cu(pst), cu(far), shift, taps, floor).cpu().numpy()
    for q in range(3):
        assert tuple(back[q]) == (int(pst[q, 0]), viterbi.LINK_JUMP) == viterbi_ref.back(sprev[q], pst[q], int(far[q]), shift[q], taps, floor, dtype=np.float32)
    assert int(pst[2, 0]) == 10 * 512 + 500


# ---- 3. the same bits across call forms ---------------------------------------------------------------------------------------------

def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    bel, prev, sprev, pst, shift, floor = batch_of(QUERIES[:3])
    t = aerial.gaussian_taps(2.5, 6)
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    got, st = viterbi.track_viterbi(m, *args, shift, t, floor)
    cells = st[:, 0].to(torch.int32)
    back = viterbi.track_viterbi_back(m, args[2], args[3], cells, shift, t, floor)
    # shared taps against repeated taps
    rep, rst = viterbi.track_viterbi(m, *args, shift, np.tile(t, (3, 1)), floor)
    eq(got, rep); eq(st, rst)
    eq(back, viterbi.track_viterbi_back(m, args[2], args[3], cells, shift, np.tile(t, (3, 1)), floor))
    # a second call, and into a tensor of the caller
    again, ast = viterbi.track_viterbi(m, *args, shift, t, floor)
    eq(got, again); eq(st, ast)
    out = torch.empty_like(got)
    o, ost = viterbi.track_viterbi(m, *args, shift, t, floor, out=out)
    assert o.data_ptr() == out.data_ptr()
    eq(got, out); eq(st, ost)
    eq(back, viterbi.track_viterbi_back(m, args[2], args[3], cells, shift, t, floor))
    with pytest.raises(ValueError, match="none of the input maps"):
        viterbi.track_viterbi(m, *args, shift, t, floor, out=args[2])
    # each query alone
    for q in range(3):
        one, ost = viterbi.track_viterbi(m, *[a[q:q + 1] for a in args], shift[q:q + 1], t, floor[q:q + 1])
        eq(got[q:q + 1], one); eq(st[q:q + 1], ost)
        eq(back[q:q + 1], viterbi.track_viterbi_back(m, args[2][q:q + 1], args[3][q:q + 1], cells[q:q + 1], shift[q:q + 1], t, floor[q:q + 1]))
    for a, raw in zip(args, (bel, prev, sprev, pst)):              # no input is written
        eq(a, cu(raw))


def test_two_streams_with_two_work_buffers_do_not_meet():
    m = base()["m"]
    lib = _lib.load()
    bel, prev, sprev, pst, shift, floor = batch_of(QUERIES[:3])
    B = 3
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    t6, t32 = aerial.gaussian_taps(2.5, 6), aerial.gaussian_taps(11.0, 32)
    serial = [viterbi.track_viterbi(m, *args, shift, t6, floor), viterbi.track_viterbi(m, *args, -shift, t32, floor)]
    sh = [cu(shift), cu(-shift)]
    tp = [cu(t6), cu(t32)]
    fl = cu(floor)
    outs = [(torch.empty(B, 512, 512, device="cuda"), torch.empty(B, 4, device="cuda"),
             torch.empty(lib.ccvpe_track_viterbi_work_bytes(B), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for s_, t_, r, (o, st, wk), stream in zip(sh, tp, (6, 32), outs, streams):
            rc = lib.ccvpe_track_viterbi(m._handle, *[a.data_ptr() for a in args], B, s_.data_ptr(), t_.data_ptr(), 0, r, fl.data_ptr(),
                                         o.data_ptr(), st.data_ptr(), wk.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (ws, wst) in zip(outs, serial):
        eq(o, ws); eq(st, wst)


# ---- 4. degenerate queries between ordinary ones -------------------------------------------------------------------------------------

def test_degenerate_queries_get_their_rule_and_the_healthy_query_keeps_its_bits():
    m = base()["m"]
    t = aerial.gaussian_taps(2.5, 6)
    B = 9
    bel, prev, sprev, pst, shift, floor = batch_of([QUERIES[0]] * B)
    h_v, h_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], shift[:1], t, floor[:1])
    j = int(pst[0, 0])
    h_cell = h_st[:, 0].to(torch.int32)
    h_back = viterbi.track_viterbi_back(m, cu(sprev[:1]), cu(pst[:1]), h_cell, shift[:1], t, floor[:1])
    bel, prev, sprev, pst = bel.copy(), prev.copy(), sprev.copy(), pst.copy()
    bel[1] = 0.0                                     # a zero belief: degenerate
    bel[2, 200, 300] = np.nan                        # a NaN in the belief: not taken, the query with a zero there
    prev[3, 250, 250] = np.nan                       # a NaN in the previous belief: the prior around it is NaN, those cells score 0
    sprev[4] = 0.0                                   # a zero previous score map: a restart
    pst[5, 0], pst[6, 0], pst[7, 0] = -1.0, np.nan, float(N)        # no previous index: restarts
    got, st = run_step(m, bel, prev, sprev, pst, shift, t, floor)
    cells = np.int32([int(h_cell[0]), 5, 5, 5, 5, 5, -1, N, int(h_cell[0])])
    back = viterbi.track_viterbi_back(m, cu(sprev), cu(pst), cu(cells), shift, t, floor).cpu().numpy()
    for q in (0, 8):                                 # the healthy query, at both ends of the batch
        eq(got[q:q + 1], h_v); eq(st[q:q + 1], h_st)
        assert tuple(back[q]) == tuple(h_back[0].cpu().numpy())
    assert not bool(got[1].any()) and st[1, 0].item() == -1 and np.isnan(st[1, 1].item()) and np.isnan(st[1, 2].item()) and st[1, 3].item() == 0
    zeroed = bel[2:3].copy()
    zeroed[0, 200, 300] = 0.0
    z_v, z_st = run_step(m, zeroed, prev[2:3], sprev[2:3], pst[2:3], shift[2:3], t, floor[2:3])
    eq(got[2:3], z_v); eq(st[2:3], z_st)
    assert got[2, 200, 300].item() == 0
    assert not bool(torch.isnan(got[3]).any()) and st[3, 0].item() >= 0 and st[3, 3].item() == 0
    hit = torch.zeros(512, 512, dtype=torch.bool, device="cuda")
    # the cells whose blur window (radius 6, shift (3.37, 0.81)) holds the NaN are columns 247 .. 260 of rows 244 .. 257; the x pass
    # makes four adjacent outputs from one run of source columns, under zero weights where a column is not theirs, and 0 * NaN is NaN:
    # the whole groups 244 .. 263, in ccvpe_track_predict's prior as here
    hit[244:258, 244:264] = True
    assert not bool(got[3][hit].any())
    if not bool(hit.view(-1)[int(h_st[0, 0].item())]):
        eq(got[3][~hit], h_v[0][~hit]); eq(st[3], h_st[0])
    # the four restarts hold the same maps: the same bits, the frame's likelihood scaled, restarted = 1
    for q in (4, 5, 6, 7):
        eq(got[q], got[4]); eq(st[q], st[4])
    assert st[4, 3].item() == 1 and st[4, 0].item() >= 0 and 1.0 <= st[4, 1].item() < 2.0
    ref = viterbi_ref.step(bel[4:5], prev[4:5], sprev[4:5], pst[4:5], shift[4:5], t, floor[4:5])
    w = np.ldexp(got[4].double().cpu().numpy(), int(st[4, 2].item()))
    big = ref["w"][0] >= 2.0 ** -100
    assert (np.abs(w[big] - ref["w"][0][big]) <= 2 * bound_w(6) * ref["w"][0][big]).all() and ref["stats"][0, 3] == 1
    # the backtrack: a zero score map has a previous index but nothing positive to point at; no previous index; a cell outside the grid
    assert tuple(back[4]) == (j, viterbi.LINK_START)
    assert tuple(back[5]) == (-1, viterbi.LINK_START)
    assert tuple(back[6]) == (-1, viterbi.LINK_START) and tuple(back[7]) == (-1, viterbi.LINK_START)
    lone = viterbi.track_viterbi_back(m, cu(sprev[:2]), cu(pst[:2]), cu(np.int32([-1, N])), shift[:2], t, floor[:2]).cpu().numpy()
    assert tuple(lone[0]) == (j, viterbi.LINK_START) and tuple(lone[1]) == (j, viterbi.LINK_START)
    # nothing is left behind: the healthy query again
    a_v, a_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], shift[:1], t, floor[:1])
    eq(a_v, h_v); eq(a_st, h_st)
    # a belief the floor-less prior cannot reach is degenerate: floor 0 under an off-window shift gives lik = inf
    d_v, d_st = run_step(m, bel[:1], prev[:1], sprev[:1], pst[:1], np.float32([[700.0, 0.0]]), t, np.float32([0.0]))
    assert not bool(d_v.any()) and d_st[0, 0].item() == -1 and np.isnan(d_st[0, 1].item()) and d_st[0, 3].item() == 0


# ---- 5. launches -------------------------------------------------------------------------------------------------------------------

def test_two_launches_per_step_and_one_per_link():
    """the first-frame form is the same two launches (the step kernel without its staging, then the scale kernel)"""
    m = base()["m"]
    lib = _lib.load()
    bel, prev, sprev, pst, shift, floor = batch_of(QUERIES[:2])
    args = [cu(a) for a in (bel, prev, sprev, pst)]
    sh, fl = cu(shift), cu(floor)
    cells = torch.tensor([1000, -1], dtype=torch.int32, device="cuda")

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    assert count(lambda: viterbi.track_viterbi(m, args[0])) == 2
    for r in (0, 6, 32):
        taps = cu(aerial.gaussian_taps(2.0, r))
        assert count(lambda: viterbi.track_viterbi(m, *args, sh, taps, fl)) == 2
        assert count(lambda: viterbi.track_viterbi_back(m, args[2], args[3], cells, sh, taps, fl)) == 1


# ---- 6. streams --------------------------------------------------------------------------------------------------------------------

class _LogitsStream:
    """the model behind a tracker whose update half reads the next logits of a list instead of running the network"""

    def __init__(self, m, logits):
        self._m, self._logits = m, iter(logits)
        self._ori = torch.zeros(1, 2, 512, 512, device="cuda")
        self._ori[:, 0] = 1.0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def track_update_cached(self, grd, cache, prior, tile_index=None):
        return self._m.track_update_logits(cu(next(self._logits)[None]), self._ori, prior)


def device_path(m, logits, step_px, taps, floor):
    tr = smooth.RecordingTracker()
    stream = _LogitsStream(m, logits)
    motion = np.float64(step_px) * 800.0 / 512.0
    grd = torch.zeros(1, 3, 8, 8)
    for _ in logits:
        tr.step(stream, grd, None, None, np.array([[0, 0]]), motion, taps, floor)
    return tr, viterbi.map_path(m, tr.log)


def test_crafted_stream_on_the_device_walks_the_float64_path():
    m = base()["m"]
    frames, _, want_cells, want_links, _ = viterbi_ref.crafted_path()
    taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
    tr, (cells, links, stats, scores) = device_path(m, [track_ref.sequence_logits(k) for k in frames], track_ref.SEQ_STEP, taps, track_ref.SEQ_FLOOR)
    first = int(tr.log[0][0].argmax().item())
    assert track_ref.pixel_distance(first, track_ref.SEQ_DISTRACTOR) <= 1.0         # the filter starts on the distractor ...
    assert cells[:, 0].tolist() == want_cells.tolist()                               # ... the path does not
    assert links[:, 0].tolist() == want_links.tolist() == [viterbi.LINK_START] + [viterbi.LINK_MOVE] * (len(frames) - 1)
    assert stats[:, 0, 3].tolist() == [1.0] + [0.0] * (len(frames) - 1) and len(scores) == len(frames)


def test_relocalisation_stream_on_the_device_jumps_once():
    m = base()["m"]
    truth, _, want_cells, want_links, _ = viterbi_ref.reloc_path()
    taps = aerial.gaussian_taps(viterbi_ref.RELOC_SIGMA, viterbi_ref.RELOC_RADIUS)
    _, (cells, links, _, _) = device_path(m, [viterbi_ref.peak_logits(xy) for xy in truth], viterbi_ref.RELOC_STEP, taps, viterbi_ref.RELOC_FLOOR)
    assert cells[:, 0].tolist() == want_cells.tolist()
    assert links[:, 0].tolist() == want_links.tolist()
    assert [t for t, k in enumerate(links[:, 0].tolist()) if k == viterbi.LINK_JUMP] == [5]


def test_recorded_stream_path_is_the_spelled_out_calls():
    m = base()["m"]
    F = 6
    g, s = inputs("oxford", F, seed=23)             # six frames of one stream; two cached tiles
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]                       # the vehicle crosses the 400-px grid between frames 2 and 3
    motion = np.array([61.0, -9.5])
    taps, floor = aerial.gaussian_taps(3.0, 9), 1e-7
    tr = smooth.RecordingTracker()
    for k in range(F):
        tr.step(m, g[k:k + 1], sc, [tile[k]], origins, motion, taps, floor)
    kept = [e[0].clone() for e in tr.log]
    cells, links, stats, scores = viterbi.map_path(m, tr.log)
    assert tuple(cells.shape) == (F, 1) == tuple(links.shape) and cells.dtype == torch.int32 and tuple(stats.shape) == (F, 1, 4)
    for k in range(F):
        eq(tr.log[k][0], kept[k])                   # the sweep writes to none of the log's beliefs
    # spelled out
    v, st = viterbi.track_viterbi(m, tr.log[0][0])
    vs, sts = [v], [st]
    for k in range(1, F):
        shift = aerial.oxford_track_shift(origins[tile[k - 1]], origins[tile[k]], motion)
        v, st = viterbi.track_viterbi(m, tr.log[k][0], tr.log[k - 1][0], vs[-1], sts[-1], shift, taps, floor)
        vs.append(v); sts.append(st)
    for k in range(F):
        eq(scores[k], vs[k]); eq(stats[k], sts[k])
        assert sts[k][0, 0].item() >= 0 and sts[k][0, 3].item() == (1.0 if k == 0 else 0.0)
    cell = sts[-1][:, 0].to(torch.int32)
    eq(cells[F - 1], cell)
    assert links[0, 0].item() == viterbi.LINK_START
    for k in range(F - 1, 0, -1):
        shift = aerial.oxford_track_shift(origins[tile[k - 1]], origins[tile[k]], motion)
        back = viterbi.track_viterbi_back(m, vs[k - 1], sts[k - 1], cell, shift, taps, floor)
        eq(links[k], back[:, 1]); eq(cells[k - 1], back[:, 0])
        assert back[0, 1].item() in (viterbi.LINK_MOVE, viterbi.LINK_JUMP) and 0 <= back[0, 0].item() < N
        cell = back[:, 0].contiguous()
