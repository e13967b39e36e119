"""The MAP trajectory of a joint stream on the device (ccvpe_track_joint_viterbi, ccvpe_track_joint_viterbi_back)
against tests/joint_viterbi_ref.py fed the float32 inputs the device got.

All terms are non-negative, so the bound is relative and relative errors add to first order, u = 2^-24:
    prior             the predict's count (tests/test_track_joint_gpu.py)                     4r + 2rh + 18
    lik               one IEEE division                                                       4r + 2rh + 19
    window candidate  each merged weight 2 (a product and a fused multiply-add), two products 6
    M[d]              a subtraction, a product, a fused multiply-add                          3
    mix candidate     the product of the two                                                  10
    jump              one product                                                             1
    w                 lik times the larger of the two, one product                            4r + 2rh + 30
The scaling by a power of two adds none.  The tests allow twice the bound wherever the restatement is >= 2^-100 and below that ask
for a value <= 2^-99 that is not NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth, viterbi
from tests import joint_ref as jr
from tests import joint_smooth_ref as jsr
from tests import joint_viterbi_ref as jvr
from tests.test_track_joint_smooth_gpu import base, case, eq, eq_nan

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
TINY = 2.0 ** -100
BOUND_CANDIDATE = 10 * EPS
_LINKS = {}


def bound_w(r, rh):
    return (4 * r + 2 * rh + 30) * EPS


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def link(nb, r, rh, B=3):
    """The smoother test's link of B streams read forwards: J- its J, J its next joint (a real predict + update behind J-), the
    arguments of the predict between them, and v-, prev_stats from the first-frame call on J-.  Kept and left unchanged."""
    key = (nb, r, rh, B)
    if key not in _LINKS:
        c = case(nb, r, rh, B)
        vp, ps = viterbi.track_joint_viterbi(base()["m"], c["J"])
        _LINKS[key] = dict(c, Jp=c["J"], J=c["nxt"], vp=vp, ps=ps)
    return _LINKS[key]


def run(c, q=None, **kw):
    """track_joint_viterbi of a link, or of its queries q alone"""
    sl = slice(None) if q is None else q
    a = dict(J=c["J"][sl].contiguous(), Jp=c["Jp"][sl].contiguous(), vp=c["vp"][sl].contiguous(), ps=c["ps"][sl].contiguous(),
             shift=c["shift"][sl], taps=c["taps"][sl], floor=c["floor"][sl], turn=c["turn"][sl], htaps=c["htaps"][sl], out=None)
    a.update(kw)
    return viterbi.track_joint_viterbi(base()["m"], a["J"], a["Jp"], a["vp"], a["ps"], a["shift"], a["taps"], a["floor"], a["turn"], a["htaps"],
                                       out=a["out"])


def run_back(c, cells, bins, q=None, **kw):
    sl = slice(None) if q is None else q
    a = dict(vp=c["vp"][sl].contiguous(), ps=c["ps"][sl].contiguous(), shift=c["shift"][sl], taps=c["taps"][sl], floor=c["floor"][sl],
             turn=c["turn"][sl], htaps=c["htaps"][sl])
    a.update(kw)
    return viterbi.track_joint_viterbi_back(base()["m"], a["vp"], a["ps"], cu(cells, torch.int32), cu(bins, torch.int32), a["shift"], a["taps"],
                                            a["floor"], a["turn"], a["htaps"])


def own_argmax(score, stats, nb):
    """stats carries the first flat argmax of the device's own score, split into (cell, bin), and the score there, in [1, 2)"""
    B = stats.shape[0]
    v, st = score.cpu().numpy().reshape(B, nb * N), stats.cpu().numpy()
    flat = v.argmax(axis=1)
    np.testing.assert_array_equal(st[:, 0], (flat % N).astype(np.float32))
    np.testing.assert_array_equal(st[:, 1], (flat // N).astype(np.float32))
    np.testing.assert_array_equal(st[:, 2], v[np.arange(B), flat])
    assert ((st[:, 2] >= 1.0) & (st[:, 2] < 2.0)).all()


# ---- 1. the float64 definition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb,r,rh,B", [(4, 0, 0, 3), (8, 1, 1, 3), (5, 2, 2, 3), (6, 8, 2, 3), (4, 32, 1, 1), (72, 1, 1, 1)])
def test_follows_the_float64_definition(nb, r, rh, B):
    """worst error over the bound, measured: see DESIGN.md 4.29"""
    c = link(nb, r, rh, B)
    score, stats = run(c)
    assert score.shape == (B, nb, 512, 512) and stats.shape == (B, 5)
    vp, ps = c["vp"].cpu().numpy(), c["ps"].cpu().numpy()
    ref = jvr.step(c["J"].cpu().numpy(), c["Jp"].cpu().numpy(), vp, ps, c["shift"], c["taps"], c["turn"], c["htaps"], c["floor"])
    v, st = score.double().cpu().numpy(), stats.double().cpu().numpy()
    what = f"nb {nb} r {r} rh {rh}"
    worst = worst_back = 0.0
    for q in range(B):
        want = ref["w"][q]
        assert ref["stats"][q, 0] >= 0 and st[q, 4] == 0 == ref["stats"][q, 4], (q, st[q])
        assert not np.isnan(v[q]).any() and (v[q] >= 0).all()
        w = np.ldexp(v[q], int(st[q, 3]))
        big = want >= TINY
        ratio = float((np.abs(w[big] - want[big]) / (bound_w(r, rh) * want[big])).max())
        worst = max(worst, ratio)
        print(f"{what} query {q}: {int(big.sum())} values checked, worst error / bound = {ratio:.3f}, exponent {int(st[q, 3])}")
        assert ratio <= 2.0, (q, ratio)
        assert (np.abs(w[~big]) <= 2.0 ** -99).all()
        i, k = int(st[q, 0]), int(st[q, 1])
        assert 0 <= i < N and 0 <= k < nb and want[k].reshape(-1)[i] >= want.max() * (1.0 - 2 * bound_w(r, rh)), (q, i, k)
    own_argmax(score, stats, nb)
    # the backtrack against the float64 candidates: the step's argmax, the corners, random pairs
    rng = np.random.default_rng(100 + nb + r)
    pairs = [(st[:, 0].astype(np.int64), st[:, 1].astype(np.int64)), (np.zeros(B, np.int64), np.zeros(B, np.int64)),
             (np.full(B, N - 1), np.full(B, nb - 1))] + [(rng.integers(0, N, B), rng.integers(0, nb, B)) for _ in range(3)]
    tol = 2 * BOUND_CANDIDATE
    for cells, bins in pairs:
        back = run_back(c, cells, bins).cpu().numpy()
        for q in range(B):
            jc, jk = int(ps[q, 0]), int(ps[q, 1])
            idx, vals = jvr.back_candidates(vp[q], int(cells[q]), int(bins[q]), c["shift"][q], c["taps"][q], c["turn"][q], c["htaps"][q])
            best = float(vals.max()) if vals.size else -np.inf
            jump = float(np.float64(c["floor"][q]) * np.float64(vp[q, jk].reshape(-1)[jc]))
            pc, pb, kind = (int(x) for x in back[q])
            if jump > best * (1 + tol) and jump > 0:
                assert (pc, pb, kind) == (jc, jk, viterbi.LINK_JUMP), (q, cells[q], bins[q], back[q], best, jump)
            elif best > jump * (1 + tol) and best > 0:
                assert kind == viterbi.LINK_MOVE, (q, cells[q], bins[q], back[q], best, jump)
            if kind == viterbi.LINK_MOVE:
                at = np.nonzero(idx == pb * N + pc)[0]
                assert at.size >= 1 and vals[at].max() >= best * (1 - tol), (q, cells[q], bins[q], back[q])
                worst_back = max(worst_back, float((best - vals[at].max()) / (BOUND_CANDIDATE * best)))
            elif kind == viterbi.LINK_JUMP:
                assert (pc, pb) == (jc, jk) and jump >= best * (1 - tol)
            else:
                assert (pc, pb) == (jc, jk) and not best > 0 and not jump > 0
    print(f"{what}: worst w error / bound {worst:.3f}, worst backtrack gap / bound {worst_back:.3f}")


# ---- 2. exact inputs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("turn", [-90.0, -45.0])
def test_exact_inputs_give_the_bits_of_the_float32_restatement(turn):
    m = base()["m"]
    e = jvr.exact_case(turn)
    args = (e["J"][None], e["Jp"][None], e["vp"][None], e["prev_stats"], e["shift"][None], e["taps"], e["turn"], e["htaps"], e["floor"])
    ref = jvr.step(*args, dtype=np.float32)
    vp, ps = cu(e["vp"][None]), cu(e["prev_stats"])
    score, stats = viterbi.track_joint_viterbi(m, cu(e["J"][None]), cu(e["Jp"][None]), vp, ps, e["shift"][None], e["taps"], e["floor"], e["turn"],
                                               e["htaps"])
    np.testing.assert_array_equal(score.cpu().numpy()[0], ref["v"][0])
    np.testing.assert_array_equal(stats.cpu().numpy(), ref["stats"].astype(np.float32))
    # 16 random pairs around the blocks, the cells over the plateau and its hole, off-block cells
    rng = np.random.default_rng(5)
    pairs = [((40 + int(y)) * 512 + 60 + int(x), int(k)) for y, x, k in zip(rng.integers(-2, 14, 16), rng.integers(-2, 14, 16), rng.integers(0, 4, 16))]
    pairs += [(y * 512 + x, k) for y in (313, 314, 315) for x in (209, 210) for k in (0, 1)]
    pairs += [(0, 0), (N - 1, 3), (200 * 512 + 400, 2), (105 * 512 + 70, 1)]
    B = len(pairs)
    back = viterbi.track_joint_viterbi_back(m, vp.expand(B, -1, -1, -1).contiguous(), ps.expand(B, -1).contiguous(),
                                            cu([p[0] for p in pairs], torch.int32), cu([p[1] for p in pairs], torch.int32),
                                            np.broadcast_to(e["shift"], (B, 4, 2)).copy(), e["taps"], e["floor"], e["turn"], e["htaps"]).cpu().numpy()
    kinds, tie = set(), False
    for (cell, k), got in zip(pairs, back):
        want = jvr.back(e["vp"], e["prev_stats"][0], cell, k, e["shift"], e["taps"], e["turn"], e["htaps"], e["floor"], dtype=np.float32)
        assert tuple(int(x) for x in got) == want, (cell, k, got, want)
        kinds.add(want[2])
        idx, vals = jvr.back_candidates(e["vp"], cell, k, e["shift"], e["taps"], e["turn"], e["htaps"], dtype=np.float32)
        tie |= want[2] == jvr.MOVE and len(set(idx[vals == vals.max()].tolist())) > 1
    assert viterbi.LINK_MOVE in kinds and viterbi.LINK_JUMP in kinds and tie


# ---- 3. one occupied bin is the position Viterbi -----------------------------------------------------------------------------------------

def test_one_occupied_bin_is_the_position_viterbi_bit_for_bit():
    m = base()["m"]
    c = case(4, 1, 1, 3)
    nb, ks, B = 5, 3, 3
    bp, b = c["J"][:, 0].contiguous(), c["nxt"][:, 1].contiguous()
    taps, floor = aerial.gaussian_taps(np.array([0.6, 1.5, 3.0]), 6), np.float32([0.0, 1e-9, 0.37])
    shift = np.array([[[3.37, 0.81], [12.0, -7.0], [-0.5, -0.5], [5.5, 5.5], [-3.0, 0.25]]] * B, np.float32)
    v0, st0 = viterbi.track_viterbi(m, bp)
    v1, st1 = viterbi.track_viterbi(m, b, bp, v0, st0, shift[:, ks], taps, floor)
    Jp = torch.zeros(B, nb, 512, 512, device="cuda")
    Jp[:, ks] = bp
    vj, sj = viterbi.track_joint_viterbi(m, Jp)
    eq(vj[:, ks], v0)
    eq(sj[:, 0], st0[:, 0]); eq(sj[:, 2:], st0[:, 1:])
    assert (sj[:, 1] == ks).all()
    rng = np.random.default_rng(9)
    for bins in (0, 2, -2):
        ko = (ks + bins) % nb
        J = torch.zeros(B, nb, 512, 512, device="cuda")
        J[:, ko] = b
        score, stats = viterbi.track_joint_viterbi(m, J, Jp, vj, sj, shift, taps, floor, np.float32(bins * 360.0 / nb), [1.0])
        eq(score[:, ko], v1)
        assert not score[:, [k for k in range(nb) if k != ko]].any()
        eq(stats[:, 0], st1[:, 0]); eq(stats[:, 2:], st1[:, 1:])
        assert (stats[:, 1] == ko).all()
        for cells in [st1[:, 0].to(torch.int32)] + [cu(rng.integers(0, N, B), torch.int32) for _ in range(3)]:
            want = viterbi.track_viterbi_back(m, v0, st0, cells, shift[:, ks], taps, floor)
            got = viterbi.track_joint_viterbi_back(m, vj, sj, cells, torch.full_like(cells, ko), shift, taps, floor, np.float32(bins * 360.0 / nb), [1.0])
            eq(got[:, 0], want[:, 0]); eq(got[:, 2], want[:, 1])
            assert (got[:, 1] == ks).all()


# ---- 4. the same bits across forms -------------------------------------------------------------------------------------------------------

def test_forms_of_one_call_give_the_same_bits():
    m = base()["m"]
    lib = _lib.load()
    c = link(8, 1, 1, 3)
    nb, B = 8, 3
    score, stats = run(c)
    again = run(c)
    eq(again[0], score); eq(again[1], stats)
    cells, bins = stats[:, 0].to(torch.int32).cpu().numpy(), stats[:, 1].to(torch.int32).cpu().numpy()
    back = run_back(c, cells, bins)
    eq(run_back(c, cells, bins), back)
    for q in range(B):                                               # a query alone
        alone = run(c, slice(q, q + 1))
        eq(alone[0], score[q:q + 1]); eq(alone[1], stats[q:q + 1])
        eq(run_back(c, cells[q:q + 1], bins[q:q + 1], slice(q, q + 1)), back[q:q + 1])
    # shared taps, htaps and scalars against the same values per query
    sh = dict(taps=c["taps"][1], htaps=c["htaps"][1], floor=float(c["floor"][1]), turn=float(c["turn"][1]))
    pq = dict(taps=np.repeat(c["taps"][1:2], B, 0), htaps=np.repeat(c["htaps"][1:2], B, 0), floor=np.repeat(c["floor"][1:2], B), turn=np.repeat(c["turn"][1:2], B))
    a, b = run(c, **sh), run(c, **pq)
    eq(a[0], b[0]); eq(a[1], b[1])
    eq(run_back(c, cells, bins, **sh), run_back(c, cells, bins, **pq))
    out = torch.empty_like(score)                                    # out= given
    given = run(c, out=out)
    assert given[0] is out
    eq(out, score); eq(given[1], stats)
    # two interleaved streams with two work buffers
    serial = [(score, stats), run(c, shift=-c["shift"])]
    args = [c["J"], c["Jp"], c["vp"], c["ps"]]
    shs = [cu(c["shift"]), cu(-c["shift"])]
    tp, ht, tn, fl = cu(c["taps"]), cu(c["htaps"]), cu(c["turn"]), cu(c["floor"])
    outs = [(torch.empty(B, nb, 512, 512, device="cuda"), torch.empty(B, 5, device="cuda"),
             torch.empty(lib.ccvpe_track_joint_viterbi_work_bytes(B, nb), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(2):
        for s_, (o, st, wk), stream in zip(shs, outs, streams):
            rc = lib.ccvpe_track_joint_viterbi(m._handle, *[a.data_ptr() for a in args], B, nb, s_.data_ptr(), tp.data_ptr(), 2, 1, tn.data_ptr(),
                                               ht.data_ptr(), 2, 1, fl.data_ptr(), wk.data_ptr(), o.data_ptr(), st.data_ptr(),
                                               C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.ccvpe_last_error()
    torch.cuda.synchronize()
    for (o, st, _), (ws, wst) in zip(outs, serial):
        eq(o, ws); eq(st, wst)


# ---- 5. degenerate queries between healthy ones -----------------------------------------------------------------------------------------

def test_degenerate_queries_get_their_rule_and_the_healthy_queries_keep_their_bits():
    c = link(4, 1, 1, 3)
    nb = 4
    healthy = run(c)
    names = ["healthy0", "zero J", "healthy1", "NaN in J", "zero v-", "no previous pair", "NaN prev_stats", "healthy2", "zero prior"]
    src = [0, 0, 1, 1, 2, 2, 0, 2, 1]
    pick = lambda key: c[key][src].clone() if isinstance(c[key], torch.Tensor) else c[key][src].copy()
    J, Jp, vp, ps = pick("J"), pick("Jp"), pick("vp"), pick("ps")
    shift, taps, floor, turn, htaps = pick("shift"), pick("taps"), pick("floor"), pick("turn"), pick("htaps")
    J[1] = 0.0
    nan_at = (2, 300, 200)
    J[(3,) + nan_at] = float("nan")
    vp[4] = 0.0
    ps[5] = torch.tensor([-1.0, -1.0, float("nan"), float("nan"), 0.0])
    ps[6] = float("nan")
    floor[8] = 0.0
    shift[8] = (600.0, -700.0)                                        # everything leaves the grid: A = 0, win = 0, and the floor is 0
    kw = dict(J=J, Jp=Jp, vp=vp, ps=ps, shift=shift, taps=taps, floor=floor, turn=turn, htaps=htaps)
    score, stats = run(c, **kw)
    st = stats.cpu().numpy()
    for at, q in ((0, 0), (2, 1), (7, 2)):                             # the healthy neighbours: the bits of the call without the poisoned ones
        eq(score[at], healthy[0][q]); eq(stats[at], healthy[1][q])
    for at in (1, 8):                                                 # W is not positive: a zero joint and (-1, -1, NaN, NaN, restarted)
        assert not score[at].any(), names[at]
        assert st[at, 0] == -1 and st[at, 1] == -1 and np.isnan(st[at, 2]) and np.isnan(st[at, 3]) and st[at, 4] == 0.0, (names[at], st[at])
    # a NaN in J is not taken: that state scores 0, every other bit is the healthy query's
    want = healthy[0][1].clone()
    assert want[nan_at] > 0
    want[nan_at] = 0.0
    eq(score[3], want); eq(stats[3], healthy[1][1])
    # the three restarts: the frame's likelihood, scaled, restarted = 1
    for at in (4, 5, 6):
        assert st[at, 4] == 1.0 and st[at, 0] >= 0 and 1.0 <= st[at, 2] < 2.0, (names[at], st[at])
    eq(score[5], score[4]); eq(stats[5], stats[4])                    # (both are query 2)
    ref = jvr.step(J[4:7].cpu().numpy(), Jp[4:7].cpu().numpy(), vp[4:7].cpu().numpy(), ps[4:7].cpu().numpy(), shift[4:7], taps[4:7], turn[4:7],
                   htaps[4:7], floor[4:7])
    for i, at in enumerate((4, 5, 6)):
        assert ref["stats"][i, 4] == 1.0
        w, lik = np.ldexp(score[at].double().cpu().numpy(), int(st[at, 3])), ref["w"][i]
        big = lik >= TINY
        ratio = float((np.abs(w[big] - lik[big]) / ((4 * 1 + 2 * 1 + 19) * EPS * lik[big])).max())
        print(f"{names[at]}: worst error of the likelihood / bound = {ratio:.3f}")
        assert ratio <= 2.0 and (np.abs(w[~big]) <= 2.0 ** -99).all()
    own_argmax(score[[0, 2, 3, 4, 5, 6, 7]], stats[[0, 2, 3, 4, 5, 6, 7]], nb)
    # the backtrack: a cell or a bin out of range gives the previous pair, a previous frame without one (-1, -1), both START
    cells = np.array([N, 5, -1, 7, 7, 7, 7, 1 << 30, 9], np.int32)
    bins = np.array([0, nb, 0, -1, 0, 0, 0, 72, 0], np.int32)
    back = run_back(c, cells, bins, **{k: v for k, v in kw.items() if k not in ("J", "Jp")}).cpu().numpy()
    prev = ps.cpu().numpy()
    for at in (0, 1, 2, 3, 7):
        assert tuple(back[at]) == (int(prev[at, 0]), int(prev[at, 1]), viterbi.LINK_START), (at, back[at])
    for at in (5, 6):
        assert tuple(back[at]) == (-1, -1, viterbi.LINK_START), (names[at], back[at])
    assert tuple(back[4]) == (int(prev[4, 0]), int(prev[4, 1]), viterbi.LINK_START)       # a zero v-: neither a move nor a jump
    ok = run_back(c, np.array([9], np.int32), np.array([0], np.int32), slice(1, 2), floor=np.float32([0.0]), shift=shift[8:9])
    assert tuple(ok.cpu().numpy()[0]) == tuple(back[8])               # the poisoned batch leaves this link's bits alone, too


# ---- 6. launch counts ---------------------------------------------------------------------------------------------------------------------

def test_four_launches_per_step_two_for_a_first_frame_and_one_per_link():
    lib = _lib.load()
    c = link(4, 1, 1, 3)

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    assert count(lambda: viterbi.track_joint_viterbi(base()["m"], c["Jp"])) == 2
    assert count(lambda: run(c)) == 4
    assert count(lambda: run_back(c, np.array([1000, -1, 5], np.int32), np.array([1, 0, 2], np.int32))) == 1


# ---- 7. the crafted stream ----------------------------------------------------------------------------------------------------------------

def test_the_recorded_two_peak_stream_walks_the_float64_path():
    """aerial's crafted stream (tests/joint_ref.py) through smooth.RecordingJointTracker and viterbi.map_joint_path: the float64 path's
    cells, bins and links (tests/test_joint_viterbi_cpu.py holds its margin), frame 0 at the right peak, and the spelled-out calls bit
    for bit."""
    m = base()["m"]
    ref = jsr.crafted_stream()
    want = jvr.crafted_path()
    nb, T = jr.SEQ_BINS, jr.SEQ_FRAMES
    step, taps, em = ref["step"], ref["taps"], ref["em"]
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

    held, tr = Held(), smooth.RecordingJointTracker()
    grd, sat = torch.zeros(1, 3, 154, 231), torch.zeros(1, 3, 512, 512)
    for k in range(T):
        tr.step(held, grd, em, jr.SEQ_FORWARD, 0.0, 0.0, taps, list(jr.SEQ_HTAPS), jr.SEQ_FLOOR, sat=sat)
    log = tr.log
    cells, bins, links, stats, scores = viterbi.map_joint_path(m, log)
    assert cells.shape == bins.shape == links.shape == (T, 1) and stats.shape == (T, 1, 5) and len(scores) == T
    assert cells.dtype == bins.dtype == links.dtype == torch.int32
    got = (cells[:, 0].cpu().numpy(), bins[:, 0].cpu().numpy(), links[:, 0].cpu().numpy())
    print("cells", got[0], "bins", got[1], "links", got[2])
    np.testing.assert_array_equal(got[0], want["cells"])
    np.testing.assert_array_equal(got[1], want["bins"])
    np.testing.assert_array_equal(got[2], want["links"])
    a0, _ = jr.sequence_peaks(0, step)
    assert np.hypot(got[0][0] % 512 - a0[0], got[0][0] // 512 - a0[1]) <= jr.SEQ_NEAR and got[1][0] == 0
    # spelled out
    sc, st = viterbi.track_joint_viterbi(m, log[0][0])
    eq(scores[0], sc); eq_nan(stats[0], st)
    for t in range(1, T):
        sc, st = viterbi.track_joint_viterbi(m, log[t][0], log[t - 1][0], scores[t - 1], stats[t - 1], *log[t][1:])
        eq(scores[t], sc); eq_nan(stats[t], st)
    eq(cells[-1], stats[-1][:, 0].to(torch.int32)); eq(bins[-1], stats[-1][:, 1].to(torch.int32))
    for t in range(T - 1, 0, -1):
        back = viterbi.track_joint_viterbi_back(m, scores[t - 1], stats[t - 1], cells[t].contiguous(), bins[t].contiguous(), *log[t][1:])
        eq(back[:, 0], cells[t - 1]); eq(back[:, 1], bins[t - 1]); eq(back[:, 2], links[t])
    assert (links[0] == viterbi.LINK_START).all()
