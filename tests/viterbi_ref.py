"""numpy restatements of the MAP trajectory (ccvpe_track_viterbi, ccvpe_track_viterbi_back, include/ccvpe.h) and a dense
Viterbi over all hw * hw states to hold them against.

per query, P(m; d) = track_ref.predict_c(m, d, taps), u the merged weights of a pass (merged_weights):
    prior = P(b-; d) + floor
    lik   = b > 0 ? b / prior : 0
    j     = (int) prev_stats[0] when that is a cell index, else none;  peak = v-[j]
    win   = max_ky uy[ky] * max_kx ux[kx] * v-(source cell)          each max as `c > acc ? c : acc` from 0
    m     = jump > win ? jump : win,  jump = floor * peak            (no j, or peak not > 0: m = 1, restarted)
    w     = lik * m, not > 0 stored as 0;  W = max w at its first index, e with W 2^-e in [1, 2);  v = ldexp(w, -e)

step(.., dtype=np.float64) is the definition evaluated in float64 on the inputs as they are; step(.., dtype=np.float32) rounds every
product to float32 as the device does - the max passes, w, the scaling and the backtrack, with the prior taken from the float64 blur
and rounded once, which is the device's prior wherever that blur is exact (the exact-input tests).  The float32 merged weight is
fmaf(f, ta, fl((1 - f) tc)) evaluated through float64, which is the fused result whenever f ta + fl(..) is exact in float64 - always
for an integer shift (f = 0).
"""
import numpy as np

from tests import smooth_ref, track_ref

HW = track_ref.HW
MOVE, JUMP, START = 0, 1, 2


def shift_axis(d):
    """(i, f) of one float32 shift component as track_stage_shifted splits it: floor clamped to +-2048 (NaN to -2048), the fraction"""
    d = np.float32(d)
    fd = np.floor(d)
    with np.errstate(invalid="ignore"):
        i = int(np.fmin(np.fmax(fd, np.float32(-2048)), np.float32(2048))) if not np.isnan(fd) else -2048
        return i, np.float32(d - fd)


def merged_weights(taps, f, dtype):
    """u[k], k = 0 .. 2r + 1, of one pass from the one-sided float32 taps [r + 1] and the float32 fraction f"""
    t = np.asarray(taps, np.float32)
    r = t.shape[0] - 1
    u = np.zeros(2 * r + 2, dtype)
    for k in range(2 * r + 2):
        a, c = abs(k - r), abs(k - 1 - r)
        ta = t[a] if a <= r else np.float32(0)
        tc = t[c] if c <= r else np.float32(0)
        if dtype == np.float32:
            low = np.float32(np.float32(1) - f) * tc                       # float32 product
            u[k] = np.float32(np.float64(f) * np.float64(ta) + np.float64(low))
        else:
            u[k] = np.float64(f) * np.float64(ta) + (1.0 - np.float64(f)) * np.float64(tc)
    return u


def _moved(a, off, axis):
    """out[.., x] = a[.., x + off] along axis, zero outside"""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if abs(off) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(off, 0), n + min(off, 0))
    dst[axis] = slice(max(-off, 0), n - max(off, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _take(acc, c):
    return np.where(c > acc, c, acc)


def max_passes(v, shift, taps, hw, dtype):
    """win [hw, hw] of one query's v- [hw, hw]: the x pass, then the y pass; weight k reads source index x' - i - r - 1 + k"""
    v = np.asarray(v, dtype).reshape(hw, hw)
    r = np.asarray(taps).shape[-1] - 1
    (ix, fx), (iy, fy) = shift_axis(shift[0]), shift_axis(shift[1])
    ux, uy = merged_weights(taps, fx, dtype), merged_weights(taps, fy, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = np.zeros((hw, hw), dtype)
        for k in range(2 * r + 2):
            mid = _take(mid, (ux[k] * _moved(v, -ix - r - 1 + k, 1)).astype(dtype))
        win = np.zeros((hw, hw), dtype)
        for k in range(2 * r + 2):
            win = _take(win, (uy[k] * _moved(mid, -iy - r - 1 + k, 0)).astype(dtype))
    return win


def prev_index(prev_stats_row, n):
    s = np.float32(prev_stats_row[0])
    return int(s) if s >= 0 and s < n else -1


def scale(w):
    """(v, stats[:3]) of one query's cleaned w: the power-of-two scaling, or the degenerate rule"""
    flat = w.reshape(-1)
    i = int(np.argmax(flat))
    W = flat[i]
    if not (W > 0 and np.isfinite(W)):
        return np.zeros_like(w), (-1.0, np.nan, np.nan)
    e = int(np.frexp(W)[1]) - 1
    v = np.ldexp(w, -e).astype(w.dtype)
    return v, (float(i), float(v.reshape(-1)[i]), float(e))


def step(belief, belief_prev=None, score_prev=None, prev_stats=None, shift=None, taps=None, floor=None, hw=HW, dtype=np.float64):
    """belief, belief_prev, score_prev [B, hw, hw] (read as they are, in float64, or through float32), prev_stats [B, 4], shift [B, 2],
    taps [r+1] or [B, r+1], floor a number or [B] (read as float32) -> dict(v [B, hw, hw] the scaled map, w the products before the
    scaling, win, jump [B], stats [B, 4] = (index, peak, exponent, restarted))."""
    b = np.asarray(belief, dtype).reshape(-1, hw, hw)
    B = b.shape[0]
    out = {"v": np.zeros_like(b), "w": np.zeros_like(b), "win": np.zeros_like(b), "jump": np.zeros(B, dtype), "stats": np.zeros((B, 4))}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if belief_prev is None:
            lik, restarted = b, np.ones(B, bool)
        else:
            bp = np.asarray(belief_prev, np.float64).reshape(B, hw, hw)
            vp = np.asarray(score_prev, dtype).reshape(B, hw, hw)
            sh = np.asarray(shift, np.float32).reshape(B, 2)
            tp = np.asarray(taps, np.float32)
            tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
            fl = np.broadcast_to(np.asarray(floor, np.float32).reshape(-1), (B,)).astype(dtype)
            prior = (smooth_ref.predict_c64(bp, sh, tp, hw) + fl.astype(np.float64)[:, None, None]).astype(dtype)
            lik = np.where(b > 0, (b / prior).astype(dtype), dtype(0))
            restarted = np.ones(B, bool)
        for q in range(B):
            w = lik[q]
            if belief_prev is not None:
                j = prev_index(np.asarray(prev_stats).reshape(B, 4)[q], hw * hw)
                peak = vp[q].reshape(-1)[j] if j >= 0 else dtype(0)
                if peak > 0:
                    restarted[q] = False
                    win = max_passes(vp[q], sh[q], tp[q], hw, dtype)
                    jump = dtype(fl[q] * peak)
                    w = (lik[q] * np.where(jump > win, jump, win)).astype(dtype)
                    out["win"][q], out["jump"][q] = win, jump
            w = np.where(w > 0, w, dtype(0))
            out["w"][q] = w
            out["v"][q], head = scale(w)
            out["stats"][q] = (*head, float(restarted[q]))
    return out


def back_candidates(score_prev, cell, shift, taps, hw=HW, dtype=np.float64):
    """(source indices, values) of the in-grid window candidates of `cell` for one query, in raster order"""
    v = np.asarray(score_prev, dtype).reshape(hw, hw)
    r = np.asarray(taps).shape[-1] - 1
    (ix, fx), (iy, fy) = shift_axis(shift[0]), shift_axis(shift[1])
    ux, uy = merged_weights(taps, fx, dtype), merged_weights(taps, fy, dtype)
    gx = cell % hw - ix - r - 1 + np.arange(2 * r + 2)
    gy = cell // hw - iy - r - 1 + np.arange(2 * r + 2)
    okx, oky = (gx >= 0) & (gx < hw), (gy >= 0) & (gy < hw)
    gx, gy, ux, uy = gx[okx], gy[oky], ux[okx], uy[oky]
    with np.errstate(invalid="ignore", over="ignore"):
        inner = (ux[None, :] * v[np.ix_(gy, gx)]).astype(dtype)
        vals = (uy[:, None] * inner).astype(dtype)
    return (gy[:, None] * hw + gx[None, :]).reshape(-1), vals.reshape(-1)


def back(score_prev, prev_stats, cell, shift, taps, floor, hw=HW, dtype=np.float64):
    """one query: (previous cell, kind) by the rules of ccvpe_track_viterbi_back"""
    n = hw * hw
    j = prev_index(prev_stats, n)
    if not 0 <= cell < n:
        return j, START
    if j < 0:
        return -1, START
    idx, vals = back_candidates(score_prev, cell, shift, taps, hw, dtype)
    ok = vals > -np.inf                                        # NaN never wins
    best, bi = -np.inf, -1
    if ok.any():
        k = int(np.argmax(np.where(ok, vals, -np.inf)))        # raster order is ascending source index: the first is the smallest
        best, bi = vals[k], int(idx[k])
    with np.errstate(invalid="ignore", over="ignore"):
        jump = dtype(dtype(np.float32(floor)) * np.asarray(score_prev, dtype).reshape(-1)[j])
    if not best > 0 and not jump > 0:
        return j, START
    if jump > best:
        return j, JUMP
    return bi, MOVE


def sweep(beliefs, shifts, taps, floor, hw=HW, dtype=np.float64):
    """viterbi.map_path on host maps, one query: beliefs a list of T maps [hw, hw], shifts[t] the shift of the link into frame t
    (shifts[0] unused) -> (cells [T], links [T], stats [T, 4], scores)."""
    T = len(beliefs)
    scores, stats = [None] * T, [None] * T
    res = step(beliefs[0][None], hw=hw, dtype=dtype)
    scores[0], stats[0] = res["v"][0], res["stats"][0]
    for t in range(1, T):
        res = step(beliefs[t][None], beliefs[t - 1][None], scores[t - 1][None], stats[t - 1][None], np.float32(shifts[t])[None], taps, floor, hw, dtype)
        scores[t], stats[t] = res["v"][0], res["stats"][0]
    cells, links = [0] * T, [START] * T
    cells[-1] = int(stats[-1][0])
    for t in range(T - 1, 0, -1):
        cells[t - 1], links[t] = back(scores[t - 1], stats[t - 1], cells[t], np.float32(shifts[t]), taps, floor, hw, dtype)
    return np.array(cells), np.array(links), np.array(stats), scores


def dense_viterbi(likelihoods, shifts, taps, floor, hw):
    """The textbook Viterbi recursion over the hw * hw cells of the augmented model with transition max(u_t[x', x], floor) and a flat
    first prior: likelihoods [T, n], shifts [T-1, 2] -> (cells [T], kinds [T]; kinds[t] says whether the link into frame t took u or
    the floor, kinds[0] = START)."""
    T, n = likelihoods.shape
    delta = likelihoods[0] / likelihoods[0].max()
    ptr, kind = np.zeros((T, n), np.int64), np.zeros((T, n), np.int64)
    for t in range(1, T):
        u = smooth_ref.dense_kernel(shifts[t - 1], taps, hw)
        move, jump = u * delta[None, :], np.broadcast_to(floor * delta[None, :], u.shape)
        both = np.maximum(move, jump)
        ptr[t] = np.argmax(both, axis=1)
        at = (np.arange(n), ptr[t])
        kind[t] = np.where(jump[at] > move[at], JUMP, MOVE)
        delta = likelihoods[t] * both[at]
        delta = delta / delta.max()
    cells, kinds = [0] * T, [START] * T
    cells[-1] = int(np.argmax(delta))
    for t in range(T - 1, 0, -1):
        cells[t - 1], kinds[t] = int(ptr[t][cells[t]]), int(kind[t][cells[t]])
    return np.array(cells), np.array(kinds)


# ---- streams ---------------------------------------------------------------------------------------------------------------------

def peak_logits(xy, hw=HW, height=8.0):
    """float32 [hw*hw] logits of one peak height exp(-d^2 / 18) at xy = (x, y) on a zero ground"""
    y, x = np.mgrid[0:hw, 0:hw].astype(np.float64)
    return (height * np.exp(-((x - xy[0]) ** 2 + (y - xy[1]) ** 2) / 18.0)).astype(np.float32).reshape(-1)


def filter_beliefs(logits, step, taps, floor, hw=HW):
    """The filter in float64 over a list of float32 logits [hw*hw], started without a prior, one shift for every link -> beliefs, a
    list of maps [hw, hw]"""
    beliefs = []
    for k, lg in enumerate(logits):
        lg = np.asarray(lg, np.float64)
        if k:
            with np.errstate(divide="ignore"):
                lg = lg + np.log(smooth_ref.predict_c64(beliefs[-1][None], np.float32(step)[None], taps, hw)[0].reshape(-1) + float(np.float32(floor)))
        e = np.exp(lg - lg.max())
        beliefs.append((e / e.sum()).reshape(hw, hw))
    return beliefs


_PATHS = {}


def crafted_path(first=2):
    """Frames first .. SEQ_FRAMES - 1 of tests/track_ref's crafted stream: the float64 filter started at `first`, then the float64 path
    -> (frames, beliefs, cells, links, scores); computed once."""
    if ("crafted", first) not in _PATHS:
        from ccvpe_amd import aerial
        frames = list(range(first, track_ref.SEQ_FRAMES))
        taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
        floor = np.float32(track_ref.SEQ_FLOOR)
        beliefs = filter_beliefs([track_ref.sequence_logits(k) for k in frames], track_ref.SEQ_STEP, taps, floor)
        cells, links, _, scores = sweep(beliefs, [None] + [track_ref.SEQ_STEP] * (len(frames) - 1), taps, floor)
        _PATHS[("crafted", first)] = (frames, beliefs, cells, links, scores)
    return _PATHS[("crafted", first)]


RELOC_T, RELOC_STEP, RELOC_SIGMA, RELOC_RADIUS, RELOC_FLOOR = 9, (7.3, 4.6), 2.0, 6, 1e-9


def reloc_truth(k):
    x0, y0 = (100.0, 200.0) if k < 5 else (300.0, 120.0)
    return x0 + RELOC_STEP[0] * k, y0 + RELOC_STEP[1] * k


def reloc_path():
    """Nine frames of one peak that moves by RELOC_STEP and is somewhere else from frame 5 on: the float64 filter and path -> (truth,
    beliefs, cells, links, scores); computed once."""
    if "reloc" not in _PATHS:
        from ccvpe_amd import aerial
        taps, floor = aerial.gaussian_taps(RELOC_SIGMA, RELOC_RADIUS), np.float32(RELOC_FLOOR)
        truth = [reloc_truth(k) for k in range(RELOC_T)]
        beliefs = filter_beliefs([peak_logits(xy) for xy in truth], RELOC_STEP, taps, floor)
        cells, links, _, scores = sweep(beliefs, [None] + [RELOC_STEP] * (RELOC_T - 1), taps, floor)
        _PATHS["reloc"] = (truth, beliefs, cells, links, scores)
    return _PATHS["reloc"]
