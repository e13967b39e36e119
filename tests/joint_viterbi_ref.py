"""numpy restatements of the MAP trajectory of a joint stream (ccvpe_track_joint_viterbi, ccvpe_track_joint_viterbi_back,
include/ccvpe.h), built on tests/joint_smooth_ref.py's predict (tests/joint_ref.py's conventions with the map side hw
as a parameter) and tests/viterbi_ref.py's passes, scaling and conventions.

per query, (o, M) = joint_smooth_ref.circle, u the merged weights of a pass under shift[k']:
    prior(k)  = sum over d of M[d] P(J-[(k + o + d) mod nb]; shift[..]) + floor
    lik       = J > 0 ? J / prior : 0
    (jk, j)   = prev_stats' (bin, cell) when both are inside the grid, else none;  peak = v-(jk, j)
    win(k')   = viterbi_ref.max_passes(v-[k'], shift[k'])
    mix(k)    = max over d of M[d] win((k + o + d) mod nb)                each max as `c > acc ? c : acc` from 0
    m         = jump > mix ? jump : mix,  jump = floor * peak             (no (jk, j), or peak not > 0: m = 1, restarted)
    w         = lik * m, not > 0 stored as 0;  W = max w at its first flat index k n + i, e with W 2^-e in [1, 2);  v = ldexp(w, -e)

step(.., dtype=np.float64) is the definition evaluated in float64 on the inputs as they are; step(.., dtype=np.float32) rounds every
product to float32 as the device does - the max passes, the circle maximum, w, the scaling and the backtrack - with the prior taken
from the float64 predict and rounded once, which is the device's prior wherever that predict is exact (the exact-input tests).  The
float32 M[d] is fmaf(f, th[|d - 1|], fl((1 - f) th[|d|])) evaluated through float64.
"""
import numpy as np

from tests import joint_ref as jr
from tests import joint_smooth_ref as jsr
from tests import viterbi_ref as vr

HW = vr.HW
MOVE, JUMP, START = vr.MOVE, vr.JUMP, vr.START


def circle(turn_deg, nb, htaps, dtype):
    """(o, M [2 rh + 2]) as the kernels hold them, M in dtype"""
    o, M = jsr.circle(turn_deg, nb, htaps)
    if dtype == np.float64:
        return o, M
    th = np.asarray(htaps, np.float32).reshape(-1)
    rh = th.shape[0] - 1
    u0 = -float(np.float32(turn_deg)) / (360.0 / nb)
    f = np.float32(u0 - np.floor(u0))
    t = lambda a: th[a] if a <= rh else np.float32(0)
    M32 = np.zeros(2 * rh + 2, np.float32)
    for i, d in enumerate(range(-rh, rh + 2)):
        low = np.float32(np.float32(1) - f) * t(abs(d))
        M32[i] = np.float32(np.float64(f) * np.float64(t(abs(d - 1))) + np.float64(low))
    return o, M32


def prev_pair(prev_stats_row, n, nb):
    """(cell, bin) of a stats row when both are inside the grid, else (-1, -1)"""
    c, k = np.float32(prev_stats_row[0]), np.float32(prev_stats_row[1])
    return (int(c), int(k)) if c >= 0 and c < n and k >= 0 and k < nb else (-1, -1)


def scale(w):
    """(v, (cell, bin, peak, e)) of one query's cleaned w [nb, hw, hw]: one power of two for all bins, or the degenerate rule"""
    n = w.shape[1] * w.shape[2]
    v, (i, peak, e) = vr.scale(w)
    if i < 0:
        return v, (-1.0, -1.0, np.nan, np.nan)
    return v, (float(int(i) % n), float(int(i) // n), peak, e)


def _per_query(v, B, width=False):
    v = np.asarray(v, np.float32)
    return np.broadcast_to(v.reshape(-1, v.shape[-1]) if width else v.reshape(-1), (B, v.shape[-1]) if width else (B,))


def step(joint, joint_prev=None, score_prev=None, prev_stats=None, shift=None, taps=None, turn_deg=None, htaps=None, floor=None, hw=HW,
         dtype=np.float64):
    """joint, joint_prev, score_prev [B, nb, hw, hw], prev_stats [B, 5], shift [B, nb, 2], taps [r+1] or [B, r+1], turn_deg a number or
    [B], htaps [rh+1] or [B, rh+1], floor a number or [B] (read as float32) -> dict(v the scaled joint, w the products before the
    scaling, mix, jump [B], lik, stats [B, 5] = (cell, bin, peak, exponent, restarted))."""
    J = np.asarray(joint, dtype)
    B, nb = J.shape[:2]
    J = J.reshape(B, nb, hw, hw)
    out = {"v": np.zeros_like(J), "w": np.zeros_like(J), "mix": np.zeros_like(J), "lik": np.zeros_like(J), "jump": np.zeros(B, dtype),
           "stats": np.zeros((B, 5))}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if joint_prev is None:
            lik = J
        else:
            vp = np.asarray(score_prev, dtype).reshape(B, nb, hw, hw)
            sh = np.asarray(shift, np.float32).reshape(B, nb, 2)
            tp, ht = _per_query(taps, B, True), _per_query(htaps, B, True)
            turn, fl = _per_query(turn_deg, B), _per_query(floor, B).astype(dtype)
            prior = jsr.predict(np.asarray(joint_prev, np.float64).reshape(B, nb, hw, hw), sh, tp, turn, ht, fl, hw).astype(dtype)
            lik = np.where(J > 0, (J / prior).astype(dtype), dtype(0))
        for q in range(B):
            w, restarted = lik[q], True
            if joint_prev is not None:
                jc, jk = prev_pair(np.asarray(prev_stats).reshape(B, 5)[q], hw * hw, nb)
                peak = vp[q, jk].reshape(-1)[jc] if jc >= 0 else dtype(0)
                if peak > 0:
                    restarted = False
                    o, M = circle(turn[q], nb, ht[q], dtype)
                    rh = (M.shape[0] - 2) // 2
                    win = np.stack([vr.max_passes(vp[q, k], sh[q, k], tp[q], hw, dtype) for k in range(nb)])
                    mix = np.zeros_like(win)
                    for i, d in enumerate(range(-rh, rh + 2)):
                        mix = vr._take(mix, (M[i] * np.roll(win, -(o + d), axis=0)).astype(dtype))
                    jump = dtype(fl[q] * peak)
                    w = (lik[q] * np.where(jump > mix, jump, mix)).astype(dtype)
                    out["mix"][q], out["jump"][q] = mix, jump
            w = np.where(w > 0, w, dtype(0))
            out["w"][q], out["lik"][q] = w, lik[q]
            out["v"][q], head = scale(w)
            out["stats"][q] = (*head, float(restarted))
    return out


def back_candidates(score_prev, cell, bin, shift, taps, turn_deg, htaps, hw=HW, dtype=np.float64):
    """(flat source indices k' n + g, values) of the in-grid candidates of (cell, bin) for one query: d ascending, the window of
    k' = (bin + o + d) mod nb in raster order"""
    v = np.asarray(score_prev, dtype)
    nb = v.shape[0]
    v = v.reshape(nb, hw, hw)
    n = hw * hw
    o, M = circle(turn_deg, nb, htaps, dtype)
    rh = (M.shape[0] - 2) // 2
    sh = np.asarray(shift, np.float32).reshape(nb, 2)
    idx, vals = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i, d in enumerate(range(-rh, rh + 2)):
            k = (bin + o + d) % nb
            gi, gv = vr.back_candidates(v[k], cell, sh[k], taps, hw, dtype)
            idx.append(k * n + gi)
            vals.append((M[i] * gv).astype(dtype))
    return np.concatenate(idx), np.concatenate(vals)


def back(score_prev, prev_stats, cell, bin, shift, taps, turn_deg, htaps, floor, hw=HW, dtype=np.float64):
    """one query: (previous cell, previous bin, kind) by the rules of ccvpe_track_joint_viterbi_back"""
    nb = np.asarray(score_prev).shape[0]
    n = hw * hw
    jc, jk = prev_pair(prev_stats, n, nb)
    if not (0 <= cell < n and 0 <= bin < nb):
        return jc, jk, START
    if jc < 0:
        return -1, -1, START
    idx, vals = back_candidates(score_prev, cell, bin, shift, taps, turn_deg, htaps, hw, dtype)
    ok = vals > -np.inf                                        # NaN never wins
    best, bi = -np.inf, -1
    if ok.any():
        top = np.where(ok, vals, -np.inf).max()
        best, bi = top, int(idx[ok & (vals == top)].min())     # the smallest flat source index on ties
    with np.errstate(invalid="ignore", over="ignore"):
        jump = dtype(dtype(np.float32(floor)) * np.asarray(score_prev, dtype).reshape(nb, n)[jk, jc])
    if not best > 0 and not jump > 0:
        return jc, jk, START
    if jump > best:
        return jc, jk, JUMP
    return bi % n, bi // n, MOVE


def sweep(log, hw=HW, dtype=np.float64):
    """viterbi.map_joint_path on host joints, one query: log a list of T entries (joint [nb, hw, hw], table [nb, 2], taps, floor,
    turn_deg, htaps) -> (cells [T], bins [T], links [T], stats [T, 5], scores)."""
    T = len(log)
    scores, stats = [None] * T, [None] * T
    res = step(np.asarray(log[0][0])[None], hw=hw, dtype=dtype)
    scores[0], stats[0] = res["v"][0], res["stats"][0]
    for t in range(1, T):
        joint, table, taps, floor, turn, htaps = log[t]
        res = step(np.asarray(joint)[None], np.asarray(log[t - 1][0])[None], scores[t - 1][None], stats[t - 1][None], np.asarray(table)[None],
                   taps, turn, htaps, floor, hw, dtype)
        scores[t], stats[t] = res["v"][0], res["stats"][0]
    cells, bins, links = [0] * T, [0] * T, [START] * T
    cells[-1], bins[-1] = int(stats[-1][0]), int(stats[-1][1])
    for t in range(T - 1, 0, -1):
        _, table, taps, floor, turn, htaps = log[t]
        cells[t - 1], bins[t - 1], links[t] = back(scores[t - 1], stats[t - 1], cells[t], bins[t], table, taps, turn, htaps, floor, hw, dtype)
    return np.array(cells), np.array(bins), np.array(links), np.array(stats), scores


def back_margin(score_prev, cell, bin, shift, taps, turn_deg, htaps, hw=HW):
    """(best, second): the largest candidate of (cell, bin) and the largest among the other distinct sources, float64"""
    idx, vals = back_candidates(score_prev, cell, bin, shift, taps, turn_deg, htaps, hw, np.float64)
    per = {}
    for i, v in zip(idx.tolist(), vals.tolist()):
        per[i] = max(per.get(i, 0.0), v)
    top = sorted(per.values(), reverse=True)
    return top[0], (top[1] if len(top) > 1 else 0.0)


# ---- the crafted two-peak stream of tests/joint_ref.py -------------------------------------------------------------------------------

_PATH = {}


def crafted_path():
    """The float64 path over joint_smooth_ref.crafted_stream()'s float32-stored joints -> dict(log, cells, bins, links, stats, scores,
    step); computed once."""
    if not _PATH:
        st = jsr.crafted_stream()
        nb = jr.SEQ_BINS
        table = np.asarray(st["table"], np.float32).reshape(nb, 2)
        log = [(st["joints"][t][0], None if t == 0 else table, st["taps"], jr.SEQ_FLOOR, 0.0, jr.SEQ_HTAPS) for t in range(jr.SEQ_FRAMES)]
        cells, bins, links, stats, scores = sweep(log)
        _PATH.update(log=log, cells=cells, bins=bins, links=links, stats=stats, scores=scores, step=st["step"])
    return _PATH


# ---- exact inputs: every intermediate is exact in float32 ----------------------------------------------------------------------------

def exact_case(turn_deg, hw=HW):
    """nb 4: integer shifts that differ per bin, taps (1/2, 1/4), htaps (1/2, 1/4), floor 1/16, a turn of a whole number of bins
    (turn_deg = -90: o = 1, f = 0) or of half a bin (turn_deg = -45: o = 0, f = 1/2).  J- holds small integers in two blocks, v- powers
    of two in blocks, with ties across cells and across bins and a plateau of the largest value spanning bins 1 and 2, so the jump
    target is the first flat index; J = prior * 2^k.  -> dict of float32 arrays for one query."""
    nb = 4
    rng = np.random.default_rng(17)
    shift = np.float32([[3, -2], [-1, 4], [0, 0], [2, 5]])
    taps, htaps, floor = np.float32([0.5, 0.25]), np.float32([0.5, 0.25]), np.float32(1.0 / 16)
    Jp = np.zeros((nb, hw, hw), np.float32)
    vp = np.zeros((nb, hw, hw), np.float32)
    y0, x0 = 40, 60
    Jp[:, y0:y0 + 12, x0:x0 + 12] = rng.integers(0, 8, (nb, 12, 12)).astype(np.float32)
    Jp[1, 300:306, 200:206] = rng.integers(1, 5, (6, 6)).astype(np.float32)
    vp[:, y0:y0 + 12, x0:x0 + 12] = np.ldexp(np.float32(1), rng.integers(-6, -1, (nb, 12, 12))).astype(np.float32)
    vp[0, y0 + 2:y0 + 6, x0 + 2:x0 + 6] = 0.25                     # a tie across cells ...
    vp[3, y0 + 2:y0 + 6, x0 + 2:x0 + 6] = 0.25                     # ... and across bins
    # the plateau of the largest v-, in bins 1 and 2 at the cells that reach the same targets under the two bins' shifts: the first flat
    # index is bin 1's.  Each has a hole: its four neighbours tie in the window above it.
    vp[1, 310:313, 210:213] = 1.0
    vp[2, 314:317, 209:212] = 1.0
    vp[1, 311, 211] = vp[2, 315, 210] = 0.25
    prev_stats = np.float32([[310 * hw + 210, 1, 1.0, 0.0, 0.0]])
    prior = jsr.predict(Jp[None], shift[None], taps, turn_deg, htaps, floor, hw)[0]
    assert np.array_equal(prior.astype(np.float32).astype(np.float64), prior)
    k = rng.integers(-3, 3, (nb, hw, hw))
    J = np.ldexp(prior, k).astype(np.float32)
    J[:, 100:110, :] = 0.0                                          # cells that are not taken
    return dict(J=J, Jp=Jp, vp=vp, prev_stats=prev_stats, shift=shift, taps=taps, htaps=htaps, floor=floor, turn=np.float32(turn_deg))
