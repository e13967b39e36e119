"""numpy float64 restatement of one backward step of the smoother behind an affine predict (ccvpe_track_smooth_affine, include/ccvpe.h;
DESIGN.md 4.22), from tests/track_affine_ref.predict_c, and a dense forward-backward over all hw * hw states to hold it against.

per query, Paff(m; M) = track_affine_ref.predict_c(m, M, taps), wgt(y, x) the bilinear weight the sample at plane position y gives cell x
(from the float32-rounded fractions, as predict_c takes them):
    prior = Paff(b; M) + floor
    g     = s' > 0 ? s' / prior : 0
    G     = sum g
    h     = g, zero-extended, blurred along x then y, on the window plus r
    A(x)  = sum_y det * wgt(y, x) * h(y)                 a scatter of h through the sample's four weights (np.add.at)
    a     = A + floor * G
    w     = b * a,  Z = sum w,  s = w / Z
A query beyond reach (det not finite or zero in float32, or a half extent above 3): g = 0.  G == 0: s = b, (index, prob) = b's argmax
among the values above -inf, Z = NaN.  Else Z not finite or <= 0: s = 0, (-1, NaN, Z, G).
"""
import numpy as np

from tests import track_affine_ref
from tests.smooth_ref import argmax_taken

HW = track_affine_ref.HW


def quantise(matrix):
    """round(M * 2^20) / 2^20.  For entries below 2^20 and positions within +-1024 every product (31 bits of an entry times 11 of a
    position) and every sum of a coordinate is then exact in float64: fused and unfused evaluation agree bit for bit, so the absolute
    2^-38 max(B) term of the affine predict's bound vanishes and the smoother's bound is purely relative."""
    return np.round(np.asarray(matrix, np.float64) * 2.0 ** 20) / 2.0 ** 20


def reach(matrix):
    """one matrix [6] -> (supported, hx, hy): the reach rule of ccvpe_track_smooth_affine"""
    m0, m1, _, m3, m4, _ = (float(v) for v in np.asarray(matrix, np.float64).reshape(6))
    with np.errstate(all="ignore"):
        d = np.float64(m0) * m4 - np.float64(m1) * m3
        det = np.float32(abs(d))
        hx = abs(np.float64(m4) / d) + abs(np.float64(-m1) / d)
        hy = abs(np.float64(-m3) / d) + abs(np.float64(m0) / d)
        ok = bool(np.isfinite(det)) and det != 0 and bool(hx <= 3.0) and bool(hy <= 3.0)
    return ok, float(hx), float(hy)


def predict_c64(m, matrix, taps, hw=HW):
    """track_affine_ref.predict_c of a float64 map: predict_c reads its map as float32 and is linear in it, so the map goes in as three
    float32 pieces whose sum is the map to 2^-72 of its largest entry."""
    m = np.asarray(m, np.float64)
    out = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(3):
            piece = m.astype(np.float32)
            out = out + track_affine_ref.predict_c(piece, matrix, taps, hw)
            m = np.where(np.isfinite(piece), m - piece.astype(np.float64), 0.0)
            if not m.any():             # (a float32 map is its own first piece)
                break
    return out


def blur_ext(g, taps, hw=HW):
    """g [hw, hw] float64, zero outside, blurred with t[|k|] along x then y -> h [hw + 2r, hw + 2r]: plane positions -r .. hw - 1 + r"""
    tp = np.asarray(taps, np.float32).astype(np.float64).reshape(-1)
    r = tp.shape[0] - 1
    full = np.concatenate([tp[:0:-1], tp])
    pad = np.zeros((hw + 4 * r, hw + 4 * r))
    pad[2 * r:2 * r + hw, 2 * r:2 * r + hw] = g
    n = hw + 2 * r
    hx = np.zeros((hw + 4 * r, n))
    for k in range(2 * r + 1):
        hx += full[k] * pad[:, k:k + n]
    h = np.zeros((n, n))
    for k in range(2 * r + 1):
        h += full[k] * hx[k:k + n, :]
    return h


def adjoint(h, matrix, hw=HW):
    """h [hw + 2r, hw + 2r] on the plane positions -r .. hw - 1 + r -> A [hw, hw]: every position scatters det * weight * h(y) to the
    four source cells its sample reads, with predict_c's coordinates, float32-rounded fractions and float32 det"""
    r = (h.shape[0] - hw) // 2
    m0, m1, m2, m3, m4, m5 = np.asarray(matrix, np.float64).reshape(6)
    det = float(np.float32(abs(m0 * m4 - m1 * m3)))
    ext = np.arange(-r, hw + r, dtype=np.float64)
    X, Y = ext[None, :], ext[:, None]
    sx = m0 * X + m1 * Y + m2
    sy = m3 * X + m4 * Y + m5
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx = (sx - fx0).astype(np.float32).astype(np.float64)
    fy = (sy - fy0).astype(np.float32).astype(np.float64)
    ix = np.clip(fx0, -4.0, hw + 4.0).astype(np.int64)
    iy = np.clip(fy0, -4.0, hw + 4.0).astype(np.int64)
    acc = np.zeros((hw + 2, hw + 2))                # index -1 .. hw: one ring that takes what falls outside the grid
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            wgt = wy * wx
            hit = wgt > 0                           # (a zero weight times an infinite h is no term)
            np.add.at(acc, (np.clip(iy + dy, -1, hw)[hit] + 1, np.clip(ix + dx, -1, hw)[hit] + 1), (det * wgt * h)[hit])
    return acc[1:-1, 1:-1]


def smooth(belief, smoothed_next, matrix, taps, floor, hw=HW):
    """belief, smoothed_next [B, hw, hw] (the device's float32 maps, or float64 maps, read as they are), matrix [B, 6] or [6], taps
    [r+1] or [B, r+1], floor a number or [B] (read as float32, as the device reads them) -> dict(s [B, hw, hw], w [B, hw, hw],
    stats [B, 4] = (index, prob, Z, G), reach [B] bool), all float64."""
    b = np.asarray(belief, np.float64).reshape(-1, hw, hw)
    sn = np.asarray(smoothed_next, np.float64).reshape(-1, hw, hw)
    B = b.shape[0]
    mat = np.broadcast_to(np.asarray(matrix, np.float64).reshape(-1, 6), (B, 6))
    tp = np.asarray(taps, np.float32)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (B,))
    s, w, stats, ok = np.zeros_like(b), np.zeros_like(b), np.zeros((B, 4)), np.zeros(B, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for q in range(B):
            ok[q] = reach(mat[q])[0]
            if ok[q]:
                prior = predict_c64(b[q], mat[q], tp[q], hw)[0] + fl[q]
                g = np.where(sn[q] > 0, sn[q] / prior, 0.0)
            else:
                g = np.zeros((hw, hw))
            G = g.sum()
            if G == 0:
                s[q], w[q] = b[q], b[q]
                stats[q] = (*argmax_taken(b[q]), np.nan, 0.0)
                continue
            w[q] = b[q] * (adjoint(blur_ext(g, tp[q], hw), mat[q], hw) + fl[q] * G)
            Z = w[q].sum()
            if not np.isfinite(Z) or Z <= 0:
                stats[q] = (-1, np.nan, Z, G)
            else:
                s[q] = w[q] / Z
                i, _ = argmax_taken(w[q])
                stats[q] = (i, s[q].reshape(-1)[i], Z, G)
    return {"s": s, "w": w, "stats": stats, "reach": ok}


def dense_kernel(matrix, taps, hw):
    """u [hw*hw, hw*hw]: u[x', x] = the weight predict_c gives source cell x at target cell x', by predict_c on the unit maps"""
    n = hw * hw
    eye = np.eye(n, dtype=np.float32).reshape(n, hw, hw)
    return track_affine_ref.predict_c(eye, np.asarray(matrix, np.float64).reshape(6), taps, hw).reshape(n, n).T.copy()


def dense_forward_backward(likelihoods, matrices, taps, floor, hw):
    """An HMM over the hw * hw cells with transition T[x', x] = u_t[x', x] + floor between frames t and t + 1 and a flat first prior:
    likelihoods [T, n], matrices [T-1, 6] -> (filtered [T, n], each normalised to mass 1; smoothed [T, n]) by the textbook
    forward-backward recursion on dense matrices."""
    T, n = likelihoods.shape
    trans = [dense_kernel(matrices[t], taps, hw) + floor for t in range(T - 1)]
    alpha = np.zeros((T, n))
    alpha[0] = likelihoods[0] / likelihoods[0].sum()
    for t in range(1, T):
        v = likelihoods[t] * (trans[t - 1] @ alpha[t - 1])
        alpha[t] = v / v.sum()
    beta = np.ones((T, n))
    for t in range(T - 2, -1, -1):
        v = trans[t].T @ (likelihoods[t + 1] * beta[t + 1])
        beta[t] = v / v.max()
    post = alpha * beta
    return alpha, post / post.sum(axis=1, keepdims=True)


_STREAMS = {}


def crafted_stream(first=2):
    """Frames first .. SEQ_FRAMES - 1 of tests/track_affine_ref's turning stream in float64: the filter started at `first` without a
    prior, then the backward sweep -> (frames, beliefs {k: [1, hw, hw]}, smoothed {k: [1, hw, hw]}, evidence {k: Z}, (taps, floor));
    frame k is reached through track_affine_ref.sequence_matrix(k).  Computed once per `first`; the maps are not to be written."""
    if first in _STREAMS:
        return _STREAMS[first]
    from ccvpe_amd import aerial
    ref = track_affine_ref
    frames = list(range(first, ref.SEQ_FRAMES))
    taps = aerial.gaussian_taps(ref.SEQ_SIGMA, ref.SEQ_RADIUS)
    floor = np.float32(ref.SEQ_FLOOR)
    beliefs, smoothed, evidence = {}, {}, {}
    for k in frames:
        lg = ref.sequence_logits(k).astype(np.float64)
        if k > first:
            with np.errstate(divide="ignore"):
                lg = lg + np.log(predict_c64(beliefs[k - 1], ref.sequence_matrix(k), taps)[0].reshape(-1) + float(floor))
        e = np.exp(lg - lg.max())
        beliefs[k] = (e / e.sum()).reshape(1, HW, HW)
    smoothed[frames[-1]] = beliefs[frames[-1]]
    for k in reversed(frames[:-1]):
        res = smooth(beliefs[k], smoothed[k + 1], ref.sequence_matrix(k + 1), taps, floor)
        smoothed[k], evidence[k] = res["s"], float(res["stats"][0, 2])
    _STREAMS[first] = (frames, beliefs, smoothed, evidence, (taps, floor))
    return _STREAMS[first]
