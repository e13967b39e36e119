"""numpy float64 restatement of one backward step of the smoother (ccvpe_track_smooth, include/ccvpe.h), from
tests/track_ref.predict_c, and a dense forward-backward over all hw * hw states to hold it against.

per query, P(m; d) = track_ref.predict_c(m, d, taps):
    prior = P(b; d) + floor
    g     = s' > 0 ? s' / prior : 0
    G     = sum g
    a     = P(g; -d) + floor * G
    w     = b * a,  Z = sum w,  s = w / Z
G == 0: s = b, (index, prob) = b's argmax among the values above -inf, Z = NaN.  Else Z not finite or <= 0: s = 0, (-1, NaN, Z, G).
"""
import numpy as np

from tests import track_ref

HW = track_ref.HW


def predict_c64(m, shift, taps, hw=HW):
    """track_ref.predict_c of a float64 map: predict_c reads its map as float32 and is linear in it, so the map goes in as three float32
    pieces whose sum is the map to 2^-72 of its largest entry."""
    m = np.asarray(m, np.float64)
    out = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(3):
            piece = m.astype(np.float32)
            out = out + track_ref.predict_c(piece, shift, taps, hw)
            m = np.where(np.isfinite(piece), m - piece.astype(np.float64), 0.0)
            if not m.any():             # (a float32 map is its own first piece)
                break
    return out


def argmax_taken(v):
    """(index, value) of the largest value above -inf, first index on ties, NaN never; (-1, NaN) without one"""
    v = np.asarray(v, np.float64).reshape(-1)
    ok = v > -np.inf
    if not ok.any():
        return -1, np.nan
    i = int(np.argmax(np.where(ok, v, -np.inf)))
    return i, float(v[i])


def smooth(belief, smoothed_next, shift, taps, floor, hw=HW):
    """belief, smoothed_next [B, hw, hw] (the device's float32 maps, or float64 maps, read as they are), shift [B, 2], taps [r+1] or
    [B, r+1], floor a number or [B] (read as float32, as the device reads them) -> dict(s [B, hw, hw], w [B, hw, hw],
    stats [B, 4] = (index, prob, Z, G)), all float64."""
    b = np.asarray(belief, np.float64).reshape(-1, hw, hw)
    sn = np.asarray(smoothed_next, np.float64).reshape(-1, hw, hw)
    B = b.shape[0]
    sh = np.asarray(shift, np.float32).reshape(B, 2)
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (B,))
    s, w, stats = np.zeros_like(b), np.zeros_like(b), np.zeros((B, 4))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        prior = predict_c64(b, sh, taps, hw) + fl[:, None, None]
        g = np.where(sn > 0, sn / prior, 0.0)
        G = g.reshape(B, -1).sum(axis=1)
        a = predict_c64(g, -sh, taps, hw) + (fl * G)[:, None, None]
        w[:] = b * a
        Z = w.reshape(B, -1).sum(axis=1)
        for q in range(B):
            if G[q] == 0:
                s[q], w[q] = b[q], b[q]
                stats[q] = (*argmax_taken(b[q]), np.nan, 0.0)
            elif not np.isfinite(Z[q]) or Z[q] <= 0:
                stats[q] = (-1, np.nan, Z[q], G[q])
            else:
                s[q] = w[q] / Z[q]
                i, _ = argmax_taken(w[q])
                stats[q] = (i, s[q].reshape(-1)[i], Z[q], G[q])
    return {"s": s, "w": w, "stats": stats}


def dense_kernel(shift, taps, hw):
    """u [hw*hw, hw*hw]: u[x', x] = the weight predict_c gives source cell x at target cell x', by predict_c on the unit maps"""
    n = hw * hw
    u = np.zeros((n, n))
    eye = np.eye(n, dtype=np.float32).reshape(n, hw, hw)
    sh = np.broadcast_to(np.asarray(shift, np.float32).reshape(1, 2), (n, 2))
    u[:, :] = track_ref.predict_c(eye, sh, taps, hw).reshape(n, n).T
    return u


def dense_forward_backward(likelihoods, shifts, taps, floor, hw):
    """An HMM over the hw * hw cells with transition T[x', x] = u_t[x', x] + floor between frames t and t + 1 and a flat first prior:
    likelihoods [T, n], shifts [T-1, 2] -> (filtered [T, n], each normalised to mass 1; smoothed [T, n]) by the textbook
    forward-backward recursion on dense matrices."""
    T, n = likelihoods.shape
    trans = [dense_kernel(shifts[t], taps, hw) + floor for t in range(T - 1)]
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


def crafted_stream(first=2):
    """Frames first .. SEQ_FRAMES - 1 of tests/track_ref's crafted stream in float64: the filter started at `first` without a prior,
    then the backward sweep -> (frames, beliefs {k: [1, hw, hw]}, smoothed {k: [1, hw, hw]}, evidence {k: Z}, (step, taps, floor))."""
    from ccvpe_amd import aerial
    frames = list(range(first, track_ref.SEQ_FRAMES))
    taps = aerial.gaussian_taps(track_ref.SEQ_SIGMA, track_ref.SEQ_RADIUS)
    step = np.float32([track_ref.SEQ_STEP])
    floor = np.float32(track_ref.SEQ_FLOOR)
    beliefs, smoothed, evidence = {}, {}, {}
    for k in frames:
        lg = track_ref.sequence_logits(k).astype(np.float64)
        if k > first:
            with np.errstate(divide="ignore"):
                lg = lg + np.log(predict_c64(beliefs[k - 1], step, taps)[0].reshape(-1) + float(floor))
        e = np.exp(lg - lg.max())
        beliefs[k] = (e / e.sum()).reshape(1, HW, HW)
    smoothed[frames[-1]] = beliefs[frames[-1]]
    for k in reversed(frames[:-1]):
        res = smooth(beliefs[k], smoothed[k + 1], step, taps, floor)
        smoothed[k], evidence[k] = res["s"], float(res["stats"][0, 2])
    return frames, beliefs, smoothed, evidence, (step, taps, floor)
