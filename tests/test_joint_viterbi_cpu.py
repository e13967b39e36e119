"""The MAP trajectory of a joint stream without a GPU: the entry points are exported, bound and refuse bad arguments
before they use the handle; the three Python calls refuse theirs before any device is touched; and the restatement
tests/joint_viterbi_ref.py is the position Viterbi of tests/viterbi_ref.py when one heading bin is occupied, finds the right peak at
every frame of the crafted two-peak stream with a path that is unique by a margin, and is exact in float32 on the exact case."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, models, viterbi
from tests import joint_ref as jr
from tests import joint_viterbi_ref as jvr
from tests import viterbi_ref as vr

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_track_joint_viterbi_work_bytes", "ccvpe_track_joint_viterbi", "ccvpe_track_joint_viterbi_back")
U = 2.0 ** -24
CANDIDATE_BOUND = 10 * U          # a mix candidate: window 6, M[d] 3, the product 1 (include/ccvpe.h)


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


# ---- C entry points ------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    assert viterbi.JOINT_VITERBI_FIELDS == ("index", "bin", "peak", "exponent", "restarted")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ccvpe.h")) as fh:
        text = fh.read()
    assert "#define CCVPE_JOINT_VITERBI_COLS 5" in text
    for n in NEW:
        assert n + "(" in text


def test_work_bytes_is_host_arithmetic(built_library):
    lib = _lib.load()
    pairs = 4 * 1024 * 2
    assert lib.ccvpe_track_joint_viterbi_work_bytes(1, 4) == 2 * 4 * N * 4 + pairs
    assert lib.ccvpe_track_joint_viterbi_work_bytes(8, 72) == 8 * (2 * 72 * N * 4 + pairs)          # past 2^32 bytes
    for batch, nb in ((1, 4), (8, 36), (455, 72)):      # at most two joints plus the partial pairs
        assert lib.ccvpe_track_joint_viterbi_work_bytes(batch, nb) <= 2 * batch * nb * N * 4 + batch * pairs
    for batch, nb in ((0, 8), (-1, 8), (1, 3), (1, 73), (456, 72), (8193, 4)):
        assert lib.ccvpe_track_joint_viterbi_work_bytes(batch, nb) == 0, (batch, nb)


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    keep = [(C.c_float * 32)() for _ in range(15)]
    jt, jp, sp, ps, sh, tp, tn, ht, fl, wk, sc, st, ce, bn, spare = [C.cast(a, C.c_void_p) for a in keep]

    def call(joint=jt, jprev=jp, sprev=sp, pstats=ps, batch=2, nb=8, shift=sh, taps=tp, stride=0, radius=3, turn=tn, htaps=ht, hstride=0, rh=1,
             floor=fl, work=wk, score=sc, stats=st):
        return lib.ccvpe_track_joint_viterbi(None, joint, jprev, sprev, pstats, batch, nb, shift, taps, stride, radius, turn, htaps, hstride, rh,
                                             floor, work, score, stats, None)

    for kw, word in (("joint", "joint"), ("taps", "taps"), ("turn", "turn_deg"), ("htaps", "htaps"), ("floor", "floor"), ("work", "work"),
                     ("score", "score"), ("stats", "stats")):
        assert call(**{kw: None}) == EINVAL and "null " + word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    for kw in (dict(jprev=None), dict(sprev=None), dict(pstats=None), dict(shift=None), dict(jprev=None, sprev=None), dict(jprev=None, sprev=None, pstats=None)):
        assert call(**kw) == EINVAL and "all null" in _msg(lib), (kw, _msg(lib))
    for nb in (3, 0, -1, 73):
        assert call(nb=nb, rh=0) == EINVAL and "nb" in _msg(lib), (nb, _msg(lib))
    for batch, nb in ((0, 8), (-1, 8), (8193, 4), (456, 72)):
        assert call(batch=batch, nb=nb) == EINVAL and "batch" in _msg(lib), (batch, nb, _msg(lib))
    for r in (-1, 33):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for s in (1, 3, 5):
        assert call(stride=s) == EINVAL and "taps_stride" in _msg(lib), (s, _msg(lib))
    for nb, rh in ((8, -1), (8, 4), (4, 2), (72, 33)):
        assert call(nb=nb, rh=rh) == EINVAL and "hradius" in _msg(lib), (nb, rh, _msg(lib))
    for s in (1, 3, -2):
        assert call(hstride=s) == EINVAL and "htaps_stride" in _msg(lib), (s, _msg(lib))
    for o in ("score", "stats"):
        for other in (jt, jp, sp, ps, sh, tp, tn, ht, fl, wk):
            assert call(**{o: other}) == EINVAL and "alias" in _msg(lib), (o, _msg(lib))
    assert call(score=st) == EINVAL and "alias" in _msg(lib)
    for kw in (dict(work=jt), dict(work=jp), dict(work=sp)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    for kw in ("joint", "jprev", "sprev", "work", "score"):
        assert call(**{kw: C.c_void_p(spare.value + 4)}) == EINVAL and "aligned" in _msg(lib), kw
    first = dict(jprev=None, sprev=None, pstats=None, shift=None)
    for kw in (dict(), dict(nb=5, rh=2), dict(nb=72, rh=32, hstride=33), dict(radius=32, stride=33), first,
               dict(first, taps=None, turn=None, htaps=None, floor=None, radius=0, rh=0)):
        assert call(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))

    bk = C.cast((C.c_int32 * 32)(), C.c_void_p)

    def link(sprev=sp, pstats=ps, cell=ce, bin=bn, batch=2, nb=8, shift=sh, taps=tp, stride=0, radius=3, turn=tn, htaps=ht, hstride=0, rh=1,
             floor=fl, back=bk):
        return lib.ccvpe_track_joint_viterbi_back(None, sprev, pstats, cell, bin, batch, nb, shift, taps, stride, radius, turn, htaps, hstride,
                                                  rh, floor, back, None)

    for kw, word in (("sprev", "score_prev"), ("pstats", "prev_stats"), ("cell", "cell"), ("bin", "bin"), ("shift", "shift"), ("taps", "taps"),
                     ("turn", "turn_deg"), ("htaps", "htaps"), ("floor", "floor"), ("back", "back")):
        assert link(**{kw: None}) == EINVAL and "null " + word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    assert link(nb=3, rh=0) == EINVAL and "nb" in _msg(lib)
    assert link(nb=4, rh=2) == EINVAL and "hradius" in _msg(lib)
    assert link(radius=33) == EINVAL and "radius" in _msg(lib)
    for other in (sp, ps, ce, bn):
        assert link(back=other) == EINVAL and "alias" in _msg(lib)
    assert link(sprev=C.c_void_p(spare.value + 4)) == EINVAL and "aligned" in _msg(lib)
    assert link() == EINVAL and "handle" in _msg(lib)


# ---- the Python calls' checks, without a device ----------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_the_python_calls_refuse_before_any_device_is_touched():
    m = _model()
    nb, B = 6, 2
    z = lambda *s, **kw: torch.zeros(*s, **kw)
    jt, jp, sp, ps = z(B, nb, 512, 512), z(B, nb, 512, 512), z(B, nb, 512, 512), z(B, 5)
    ok = dict(shift_px=np.zeros((B, nb, 2)), taps=[1.0], floor=0.0, turn_deg=0.0, heading_taps=[1.0])

    def call(joint=jt, joint_prev=jp, score_prev=sp, prev_stats=ps, **kw):
        a = dict(ok)
        a.update(kw)
        return viterbi.track_joint_viterbi(m, joint, joint_prev, score_prev, prev_stats, **a)

    # partial "go together" sets
    for kw in (dict(joint_prev=None), dict(score_prev=None), dict(prev_stats=None), dict(shift_px=None), dict(joint_prev=None, score_prev=None),
               dict(joint_prev=None, score_prev=None, prev_stats=None)):
        with pytest.raises(ValueError, match="go together"):
            call(**kw)
    with pytest.raises(ValueError, match="are needed behind"):
        call(heading_taps=None)
    for bad in (torch.zeros(512, 512), torch.zeros(B, 3, 512, 512), np.zeros((B, nb, 512, 512))):
        with pytest.raises(ValueError, match="joint must"):
            call(bad)
    with pytest.raises(ValueError, match="joint_prev must"):
        call(joint_prev=z(B, nb + 1, 512, 512))
    with pytest.raises(ValueError, match="score_prev must"):
        call(score_prev=z(1, nb, 512, 512))
    for bad in (z(B, 4), z(B, 6), z(B, 5, dtype=torch.float64), np.zeros((B, 5), np.float32), z(1, 5)):      # [B,4] is the position form's
        with pytest.raises(ValueError, match="prev_stats must"):
            call(prev_stats=bad)
    with pytest.raises(ValueError, match="heading_taps give radius 3"):                                      # 2 rh + 1 > nb
        call(heading_taps=[0.4, 0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="shift_px"):
        call(shift_px=np.zeros((B, 2)))
    with pytest.raises(ValueError, match="floor"):
        call(floor=-1.0)
    for bad in (jt, jp, sp):                                                                                # out aliasing an input
        with pytest.raises(ValueError, match="out must be none of the input joints"):
            call(out=bad)
    with pytest.raises(ValueError, match="out must"):
        call(out=z(B, nb + 1, 512, 512))
    # accepted forms: the CPU joint is refused next, before any device use
    for kw in (dict(), dict(out=z(B, nb, 512, 512)), dict(joint_prev=None, score_prev=None, prev_stats=None, shift_px=None),
               dict(taps=np.ones((B, 5), np.float32) / 9, heading_taps=torch.tensor([[0.5, 0.2, 0.05]] * B), floor=np.full(B, 1e-6),
                    turn_deg=torch.tensor([3.0, -400.0]))):
        with pytest.raises(ValueError, match="joint must be a cuda tensor"):
            call(**kw)
    with pytest.raises(RuntimeError, match="eval"):
        viterbi.track_joint_viterbi(_model().train(), jt)

    ce, bn = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    def link(score_prev=sp, prev_stats=ps, cell=ce, bin=bn, **kw):
        a = dict(ok)
        a.update(kw)
        return viterbi.track_joint_viterbi_back(m, score_prev, prev_stats, cell, bin, a["shift_px"], a["taps"], a["floor"], a["turn_deg"], a["heading_taps"])

    with pytest.raises(ValueError, match="score_prev must"):
        link(score_prev=z(B, 512, 512))
    with pytest.raises(ValueError, match="prev_stats must"):
        link(prev_stats=z(B, 4))
    for bad in (torch.zeros(B, dtype=torch.int64), torch.zeros(B + 1, dtype=torch.int32), torch.zeros(B, 1, dtype=torch.int32), [0, 0]):
        with pytest.raises(ValueError, match="bin must be an int32"):
            link(bin=bad)
        with pytest.raises(ValueError, match="cell must be an int32"):
            link(cell=bad)
    with pytest.raises(ValueError, match="heading_taps give radius 3"):
        link(heading_taps=[0.4, 0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="score_prev must be a cuda tensor"):
        link()

    with pytest.raises(ValueError, match="empty"):
        viterbi.map_joint_path(m, [])
    entry = (jt, None, [1.0], 0.0, 0.0, [1.0])
    with pytest.raises(ValueError, match="log entry 1 has no shift table"):
        viterbi.map_joint_path(m, [entry, entry])
    with pytest.raises(ValueError, match="log entry 2 has no shift table"):
        viterbi.map_joint_path(m, [entry, (jt, np.zeros((B, nb, 2)), [1.0], 0.0, 0.0, [1.0]), entry])


# ---- the restatement alone -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("floor", [0.0, 1e-9, 0.37])
def test_one_occupied_bin_is_the_position_path(floor):
    """J, J-, v- non-zero in one bin, rh = 0, htaps [1], a turn of a whole number of bins: the occupied output bin is the source bin
    moved by the turn (joint_ref.predict's convention: the mass of bin k' goes to k' + turn / w), and score, stats and backtrack there
    are viterbi_ref's for the position maps."""
    hw, nb, ks = 24, 5, 3
    rng = np.random.default_rng(29)
    taps = np.float32([0.5, 0.2, 0.05])
    shift = rng.uniform(-3, 3, (nb, 2)).astype(np.float32)
    bp = rng.uniform(0.0, 1.0, (hw, hw)).astype(np.float32) ** 4
    b = rng.uniform(0.0, 1.0, (hw, hw)).astype(np.float32) ** 4
    first = vr.step(bp[None], hw=hw)
    for bins in (0, 2, -2):
        turn = np.float32(bins * 360.0 / nb)
        ko = (ks + bins) % nb
        # joint_ref's convention, on a 512 grid: the predict of a joint with mass in bin ks has it in bin ko
        Jp, J, vp = np.zeros((1, nb, hw, hw), np.float32), np.zeros((1, nb, hw, hw), np.float32), np.zeros((1, nb, hw, hw), np.float32)
        Jp[0, ks], J[0, ko], vp[0, ks] = bp, b, first["v"][0]
        ps = np.float32([[first["stats"][0, 0], ks, first["stats"][0, 1], first["stats"][0, 2], 1.0]])
        res = jvr.step(J, Jp, vp, ps, shift[None], taps, turn, [1.0], floor, hw)
        ref = vr.step(b[None], bp[None], first["v"], first["stats"], shift[ks][None], taps, floor, hw)
        assert np.array_equal(res["v"][0, ko], ref["v"][0])
        assert not np.delete(res["v"][0], ko, axis=0).any()
        assert res["stats"][0, 1] == ko and res["stats"][0, 0] == ref["stats"][0, 0]
        assert np.array_equal(res["stats"][0, 2:], ref["stats"][0, 1:])
        for cell in [int(ref["stats"][0, 0]), 0, hw * hw - 1] + rng.integers(0, hw * hw, 12).tolist():
            got = jvr.back(vp[0], ps[0], cell, ko, shift, taps, turn, [1.0], floor, hw)
            want = vr.back(first["v"][0], first["stats"][0], cell, shift[ks], taps, floor, hw)
            assert got == (want[0], ks, want[1]), (bins, cell, got, want)
    # the convention itself, against joint_ref.predict on its own grid: the prior of a one-bin joint is above the floor in bin ko only
    full = np.zeros((1, nb, 512, 512), np.float32)
    full[0, ks, 200:210, 300:310] = 1.0
    prior = jr.predict(full, np.zeros((1, nb, 2)), [1.0], np.float32(2 * 360.0 / nb), [1.0], 0.0)
    assert prior[0, (ks + 2) % nb].sum() > 0 and not np.delete(prior[0], (ks + 2) % nb, axis=0).any()


def test_the_path_of_the_two_peak_stream_is_at_the_right_peak_from_frame_0_on():
    """The filter has 0.4879 of frame 0's mass at each peak (tests/test_track_joint_smooth_cpu.py); the path is within SEQ_NEAR of peak
    A at every frame, in A's heading bin, every link a MOVE - and unique by a margin: at every backtracked link the best and the
    second-best distinct source differ by more than twice the candidate bound, so the device's path can be held to equality."""
    p = jvr.crafted_path()
    T = jr.SEQ_FRAMES
    worst = np.inf
    for t in range(T):
        a, _ = jr.sequence_peaks(t, p["step"])
        x, y = p["cells"][t] % 512, p["cells"][t] // 512
        d = float(np.hypot(x - a[0], y - a[1]))
        print(f"frame {t}: cell ({x}, {y}), bin {p['bins'][t]}, {d:.2f} px from A, link {p['links'][t]}")
        assert d <= jr.SEQ_NEAR and p["bins"][t] == 0
        assert p["links"][t] == (jvr.START if t == 0 else jvr.MOVE)
        assert p["stats"][t][4] == (1.0 if t == 0 else 0.0)
    for t in range(T - 1, 0, -1):
        _, table, taps, floor, turn, htaps = p["log"][t]
        best, second = jvr.back_margin(p["scores"][t - 1], int(p["cells"][t]), int(p["bins"][t]), table, taps, turn, htaps)
        gap = (best - second) / best
        worst = min(worst, gap)
        assert best > 0 and gap > 2 * CANDIDATE_BOUND, (t, best, second)
        jump = float(np.float32(floor)) * p["scores"][t - 1].max()
        assert best > jump * (1 + 2 * CANDIDATE_BOUND)
    print(f"smallest relative gap between the best and the second-best source: {worst:.3e} (needed {2 * CANDIDATE_BOUND:.3e})")


@pytest.mark.parametrize("turn", [-90.0, -45.0])
def test_the_exact_case_is_exact_in_float32_and_has_ties(turn):
    hw = 512
    c = jvr.exact_case(turn, hw)
    args = (c["J"][None], c["Jp"][None], c["vp"][None], c["prev_stats"], c["shift"][None], c["taps"], c["turn"], c["htaps"], c["floor"], hw)
    r64, r32 = jvr.step(*args, dtype=np.float64), jvr.step(*args, dtype=np.float32)
    for key in ("lik", "mix", "w", "v"):
        assert np.array_equal(r32[key].astype(np.float64), r64[key]), key
    assert np.array_equal(r32["stats"], r64["stats"]) and r32["jump"][0] == r64["jump"][0] == 1.0 / 16
    assert r64["stats"][0, 4] == 0.0 and 1.0 <= r64["stats"][0, 2] < 2.0
    # the jump target: the first flat index of the largest v-, in bin 1 although bin 2 holds the same value
    flat = c["vp"].reshape(-1)
    assert int(np.argmax(flat)) == int(c["prev_stats"][0, 1]) * hw * hw + int(c["prev_stats"][0, 0]) and (flat == flat.max()).sum() == 16
    kinds, window_tie, circle_tie = set(), False, False
    back_args = (c["shift"], c["taps"], c["turn"], c["htaps"])
    for y in range(306, 320):
        for x in range(206, 216):
            for k in range(4):
                cell = y * hw + x
                idx, vals = jvr.back_candidates(c["vp"], cell, k, *back_args, hw)
                i32, v32 = jvr.back_candidates(c["vp"], cell, k, *back_args, hw, np.float32)
                assert np.array_equal(idx, i32) and np.array_equal(v32.astype(np.float64), vals)
                got = jvr.back(c["vp"], c["prev_stats"][0], cell, k, *back_args, c["floor"], hw)
                assert got == jvr.back(c["vp"], c["prev_stats"][0], cell, k, *back_args, c["floor"], hw, np.float32)
                kinds.add(got[2])
                top = idx[vals == vals.max()]
                if got[2] == jvr.MOVE and len(set(top.tolist())) > 1:
                    bins = set((top // (hw * hw)).tolist())
                    circle_tie |= len(bins) > 1
                    window_tie |= any((top // (hw * hw) == b).sum() > 1 for b in bins)
    assert jvr.MOVE in kinds and jvr.JUMP in kinds
    if turn == -90.0:                                   # f = 0: the four neighbours of the plateau's hole, M[0] / 8 = the jump, a MOVE
        assert window_tie
    else:                                               # f = 1/2: M[0] == M[1], two source bins with one weight
        assert circle_tie
