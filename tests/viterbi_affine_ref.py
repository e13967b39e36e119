"""numpy restatements of the MAP trajectory behind an affine predict (ccvpe_track_viterbi_affine, ccvpe_track_viterbi_back_affine,
include/ccvpe.h), written like tests/viterbi_ref.py, and a dense Viterbi over all hw * hw states of the augmented model
to hold them against.

per query, Paff(m; M) = track_affine_ref.predict_c(m, M, taps); for a plane position y (ix, iy), the weights wx_a, wy_b and det are
predict_c's (float64 coordinates, fractions rounded once to float32, det rounded to float32):
    prior = Paff(b-; M) + floor
    lik   = b > 0 ? b / prior : 0
    cand(y, a, b) = det * (wy_b * (wx_a * v-(ix + a, iy + b)))            v- zero-extended
    q(y)  = max over the four taps of cand                                each max as `c > acc ? c : acc` from 0
    win   = max_ky t[|ky - r|] * max_kx t[|kx - r|] * q(x' - r + kx, y' - r + ky)
    m, w, W, e, v, stats                                                  tests/viterbi_ref.py's lines

step(.., dtype=np.float64) is the definition in float64 on the inputs as they are (the weights 1 - f and f from the rounded fractions,
as predict_c takes them); step(.., dtype=np.float32) rounds every product to float32 as the device does - the weights 1.f - f, cand, the
passes, w, the scaling, the backtrack - with the prior taken from the float64 blur and rounded once, which is the device's prior
wherever that blur is exact (the exact-input tests).  The coordinates are m0 x + m1 y + m2 unfused: the device's fma chain wherever
the arithmetic is exact (smooth_affine_ref.quantise).
"""
import numpy as np

from tests import smooth_affine_ref, track_affine_ref, viterbi_ref
from tests.viterbi_ref import JUMP, MOVE, START, _take, prev_index, scale

HW = track_affine_ref.HW


def taps_at(matrix, X, Y, hw, dtype):
    """The samples at plane positions (X, Y) (float64 arrays of integers) -> (ix, iy int64, brought next to the grid; (wx_0, wx_1),
    (wy_0, wy_1) in dtype; det in dtype)"""
    m0, m1, m2, m3, m4, m5 = np.asarray(matrix, np.float64).reshape(6)
    det = np.float32(abs(m0 * m4 - m1 * m3))
    sx = m0 * X + m1 * Y + m2
    sy = m3 * X + m4 * Y + m5
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - fx0).astype(np.float32), (sy - fy0).astype(np.float32)
    ix = np.clip(fx0, -4.0, hw + 4.0).astype(np.int64)
    iy = np.clip(fy0, -4.0, hw + 4.0).astype(np.int64)
    if dtype == np.float32:
        one = np.float32(1)
        return ix, iy, (one - fx, fx), (one - fy, fy), det
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    return ix, iy, (1.0 - fx, fx), (1.0 - fy, fy), np.float64(det)


def cand(det, wx, wy, v, dtype):
    return (det * (wy * (wx * v).astype(dtype)).astype(dtype)).astype(dtype)


def q_map(v, matrix, r, hw, dtype):
    """q [hw + 2r, hw + 2r] on the plane positions -r .. hw - 1 + r of one query's v- [hw, hw]"""
    ext = np.arange(-r, hw + r, dtype=np.float64)
    ix, iy, wx, wy, det = taps_at(matrix, ext[None, :], ext[:, None], hw, dtype)
    pad = np.zeros((hw + 2, hw + 2), dtype)           # index -1 .. hw: one ring of the zero extension
    pad[1:-1, 1:-1] = np.asarray(v, dtype).reshape(hw, hw)
    q = np.zeros(ix.shape, dtype)
    for b in (0, 1):
        for a in (0, 1):
            src = pad[np.clip(iy + b, -1, hw) + 1, np.clip(ix + a, -1, hw) + 1]
            q = _take(q, cand(det, wx[a], wy[b], src, dtype))
    return q


def full_taps(taps, dtype):
    t = np.asarray(taps, np.float32).reshape(-1)
    return np.concatenate([t[:0:-1], t]).astype(dtype)          # t[|k - r|], k = 0 .. 2r


def max_passes(v, matrix, taps, hw, dtype):
    """win [hw, hw] of one query's v- [hw, hw]: the four-tap max-gather, the x pass, then the y pass"""
    full = full_taps(taps, dtype)
    r = (full.shape[0] - 1) // 2
    with np.errstate(invalid="ignore", over="ignore"):
        q = q_map(v, matrix, r, hw, dtype)
        mid = np.zeros((hw + 2 * r, hw), dtype)
        for k in range(2 * r + 1):
            mid = _take(mid, (full[k] * q[:, k:k + hw]).astype(dtype))
        win = np.zeros((hw, hw), dtype)
        for k in range(2 * r + 1):
            win = _take(win, (full[k] * mid[k:k + hw, :]).astype(dtype))
    return win


def step(belief, belief_prev=None, score_prev=None, prev_stats=None, matrix=None, taps=None, floor=None, hw=HW, dtype=np.float64):
    """viterbi_ref.step with a matrix [B, 6] or [6] for its shift: -> dict(v, w, win [B, hw, hw], jump [B], stats [B, 4])"""
    if belief_prev is None:
        return viterbi_ref.step(belief, hw=hw, dtype=dtype)
    b = np.asarray(belief, dtype).reshape(-1, hw, hw)
    B = b.shape[0]
    out = {"v": np.zeros_like(b), "w": np.zeros_like(b), "win": np.zeros_like(b), "jump": np.zeros(B, dtype), "stats": np.zeros((B, 4))}
    bp = np.asarray(belief_prev, np.float64).reshape(B, hw, hw)
    vp = np.asarray(score_prev, dtype).reshape(B, hw, hw)
    mat = np.broadcast_to(np.asarray(matrix, np.float64).reshape(-1, 6), (B, 6))
    tp = np.asarray(taps, np.float32)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    fl = np.broadcast_to(np.asarray(floor, np.float32).reshape(-1), (B,)).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for q in range(B):
            prior = (smooth_affine_ref.predict_c64(bp[q], mat[q], tp[q], hw)[0] + np.float64(fl[q])).astype(dtype)
            w = np.where(b[q] > 0, (b[q] / prior).astype(dtype), dtype(0))
            restarted = True
            j = prev_index(np.asarray(prev_stats).reshape(B, 4)[q], hw * hw)
            peak = vp[q].reshape(-1)[j] if j >= 0 else dtype(0)
            if peak > 0:
                restarted = False
                win = max_passes(vp[q], mat[q], tp[q], hw, dtype)
                jump = dtype(fl[q] * peak)
                w = (w * np.where(jump > win, jump, win)).astype(dtype)
                out["win"][q], out["jump"][q] = win, jump
            w = np.where(w > 0, w, dtype(0))
            out["w"][q] = w
            out["v"][q], head = scale(w)
            out["stats"][q] = (*head, float(restarted))
    return out


def back_candidates(score_prev, cell, matrix, taps, hw=HW, dtype=np.float64):
    """(source indices, values) of the (sample, tap) pairs of `cell` whose source cell lies inside the grid, for one query: samples in
    raster order, each one's taps (0,0), (1,0), (0,1), (1,1)"""
    v = np.asarray(score_prev, dtype).reshape(hw, hw)
    full = full_taps(taps, dtype)
    r = (full.shape[0] - 1) // 2
    k = np.arange(2 * r + 1)
    X = (cell % hw - r + k).astype(np.float64)[None, :]
    Y = (cell // hw - r + k).astype(np.float64)[:, None]
    ix, iy, wx, wy, det = taps_at(matrix, X, Y, hw, dtype)
    idx, vals = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in (0, 1):
            for a in (0, 1):
                sy, sx = iy + b, ix + a
                ok = (sx >= 0) & (sx < hw) & (sy >= 0) & (sy < hw)
                c = cand(det, wx[a], wy[b], v[np.clip(sy, 0, hw - 1), np.clip(sx, 0, hw - 1)], dtype)
                val = (full[:, None] * (full[None, :] * c).astype(dtype)).astype(dtype)
                idx.append(np.where(ok, sy * hw + sx, -1))
                vals.append(val)
    idx, vals = np.stack(idx, -1).reshape(-1), np.stack(vals, -1).reshape(-1)
    return idx[idx >= 0], vals[idx >= 0]


def back(score_prev, prev_stats, cell, matrix, taps, floor, hw=HW, dtype=np.float64):
    """one query: (previous cell, kind) by the rules of ccvpe_track_viterbi_back_affine"""
    n = hw * hw
    j = prev_index(prev_stats, n)
    if not 0 <= cell < n:
        return j, START
    if j < 0:
        return -1, START
    idx, vals = back_candidates(score_prev, cell, matrix, taps, hw, dtype)
    ok = vals > -np.inf                                        # NaN never wins
    best, bi = -np.inf, -1
    if ok.any():
        best = vals[ok].max()
        bi = int(idx[ok][vals[ok] == best].min())              # the smallest source cell among the largest, whatever sample it came through
    with np.errstate(invalid="ignore", over="ignore"):
        jump = dtype(dtype(np.float32(floor)) * np.asarray(score_prev, dtype).reshape(-1)[j])
    if not best > 0 and not jump > 0:
        return j, START
    if jump > best:
        return j, JUMP
    return bi, MOVE


def sweep(beliefs, matrices, taps, floor, hw=HW, dtype=np.float64):
    """viterbi.map_path_affine on host maps, one query: beliefs a list of T maps [hw, hw], matrices[t] the matrix of the link into frame
    t (matrices[0] unused) -> (cells [T], links [T], stats [T, 4], scores)."""
    T = len(beliefs)
    scores, stats = [None] * T, [None] * T
    res = step(beliefs[0][None], hw=hw, dtype=dtype)
    scores[0], stats[0] = res["v"][0], res["stats"][0]
    for t in range(1, T):
        res = step(beliefs[t][None], beliefs[t - 1][None], scores[t - 1][None], stats[t - 1][None], matrices[t], taps, floor, hw, dtype)
        scores[t], stats[t] = res["v"][0], res["stats"][0]
    cells, links = [0] * T, [START] * T
    cells[-1] = int(stats[-1][0])
    for t in range(T - 1, 0, -1):
        cells[t - 1], links[t] = back(scores[t - 1], stats[t - 1], cells[t], matrices[t], taps, floor, hw, dtype)
    return np.array(cells), np.array(links), np.array(stats), scores


# ---- the augmented model on dense matrices, built without the definition's gather ----------------------------------------------------

def dense_augmented(matrix, taps, hw):
    """T_aug [hw*hw, hw*hw]: T_aug[x', x] = the largest det * u(x' - y) * w_k(y) over the samples y within the taps of x' and their taps
    k that read source cell x.  A scatter: every sample of the plane throws its four (cell, weight) pairs at every target it serves."""
    n = hw * hw
    full = full_taps(taps, np.float64)
    r = (full.shape[0] - 1) // 2
    out = np.zeros((n, n))
    m = np.asarray(matrix, np.float64).reshape(6)
    det = float(np.float32(abs(m[0] * m[4] - m[1] * m[3])))
    for yy in range(-r, hw + r):
        for yx in range(-r, hw + r):
            sx, sy = m[0] * yx + m[1] * yy + m[2], m[3] * yx + m[4] * yy + m[5]
            ix, iy = int(np.floor(sx)), int(np.floor(sy))
            fx, fy = float(np.float32(sx - ix)), float(np.float32(sy - iy))
            pairs = [((iy + b) * hw + ix + a, (fx if a else 1.0 - fx) * (fy if b else 1.0 - fy))
                     for b in (0, 1) for a in (0, 1) if 0 <= ix + a < hw and 0 <= iy + b < hw]
            if not pairs:
                continue
            cells, wgt = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
            for ty in range(max(yy - r, 0), min(yy + r, hw - 1) + 1):
                for tx in range(max(yx - r, 0), min(yx + r, hw - 1) + 1):
                    u = full[yy - ty + r] * full[yx - tx + r]
                    np.maximum.at(out, (np.full(len(cells), ty * hw + tx), cells), det * u * wgt)
    return out


def dense_viterbi(likelihoods, matrices, taps, floor, hw):
    """The textbook Viterbi recursion over the hw * hw cells with transition max(T_aug, floor) and a flat first prior: likelihoods
    [T, n], matrices [T-1, 6] -> (cells [T], kinds [T]; kinds[0] = START)."""
    T, n = likelihoods.shape
    delta = likelihoods[0] / likelihoods[0].max()
    ptr, kind = np.zeros((T, n), np.int64), np.zeros((T, n), np.int64)
    for t in range(1, T):
        u = dense_augmented(matrices[t - 1], taps, hw)
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


# ---- streams: float64 paths, computed once; the maps are not to be written -----------------------------------------------------------

_PATHS = {}


def turning_path(first=2):
    """Frames first .. SEQ_FRAMES - 1 of tests/track_affine_ref's turning stream: the float64 filter of smooth_affine_ref.crafted_stream,
    then the float64 path -> (frames, beliefs [T] of [hw, hw], matrices [T], cells, links, scores, (taps, floor))."""
    if ("turning", first) not in _PATHS:
        frames, bel, _, _, (taps, floor) = smooth_affine_ref.crafted_stream(first)
        beliefs = [bel[k][0] for k in frames]
        matrices = [None] + [track_affine_ref.sequence_matrix(k) for k in frames[1:]]
        cells, links, _, scores = sweep(beliefs, matrices, taps, floor)
        _PATHS[("turning", first)] = (frames, beliefs, matrices, cells, links, scores, (taps, floor))
    return _PATHS[("turning", first)]


# The turning stream's true peak alone (no distractor), which is elsewhere from frame RELOC_AT on: SEQ_START moved by RELOC_MOVE world
# pixels for the later frames.  The frames turn as before, so every link's matrix is track_affine_ref.sequence_matrix's.
RELOC_T, RELOC_AT, RELOC_MOVE = 9, 5, (150.0, -120.0)


def reloc_truth(k):
    ref = track_affine_ref
    c = np.array(ref.SEQ_CENTRE)
    w = np.array(ref.SEQ_START) + k * np.array(ref.SEQ_STEP) + (np.array(RELOC_MOVE) if k >= RELOC_AT else 0.0)
    p = c + ref._rot(k) @ (w - c)
    return float(p[0]), float(p[1])


def reloc_logits(k):
    return viterbi_ref.peak_logits(reloc_truth(k))


def reloc_path():
    """-> (truth [T], beliefs, matrices, cells, links, scores, (taps, floor)): the float64 filter over reloc_logits, then the path"""
    if "reloc" not in _PATHS:
        from ccvpe_amd import aerial
        ref = track_affine_ref
        taps, floor = aerial.gaussian_taps(ref.SEQ_SIGMA, ref.SEQ_RADIUS), np.float32(ref.SEQ_FLOOR)
        matrices = [None] + [ref.sequence_matrix(k) for k in range(1, RELOC_T)]
        beliefs = []
        for k in range(RELOC_T):
            lg = reloc_logits(k).astype(np.float64)
            if k:
                with np.errstate(divide="ignore"):
                    lg = lg + np.log(smooth_affine_ref.predict_c64(beliefs[-1], matrices[k], taps)[0].reshape(-1) + float(floor))
            e = np.exp(lg - lg.max())
            beliefs.append((e / e.sum()).reshape(HW, HW))
        cells, links, _, scores = sweep(beliefs, matrices, taps, floor)
        _PATHS["reloc"] = ([reloc_truth(k) for k in range(RELOC_T)], beliefs, matrices, cells, links, scores, (taps, floor))
    return _PATHS["reloc"]
