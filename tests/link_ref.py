"""numpy float64 restatement of the link statistics (ccvpe_track_link, include/ccvpe.h), from tests/smooth_ref.predict_c64
and a direct correlation; the pairwise posterior of a dense HMM over all hw * hw states, binned by displacement, to hold it against; and
a synthetic random-walk stream to fit a motion model to.

per query, K = 2r + 2, i = floor(d) clamped to +-2048 and f = d - floor(d) per axis, u[k] = f t[|k - r|] + (1 - f) t[|k - 1 - r|]:
    prior = P(b; d) + floor,  g = s' > 0 ? s' / prior : 0,  G = sum g,  Sb = sum b
    D[ky][kx]     = sum over (y', x') of g(y', x') b(y' - iy - r - 1 + ky, x' - ix - r - 1 + kx)            b zero-extended
    moves[ky][kx] = uy[ky] ux[kx] D[ky][kx],  M = sum moves,  J = floor G Sb,  Z = M + J,  stats = (Z, G, J, M)
"""
import numpy as np

from tests import smooth_ref, track_ref

HW = track_ref.HW


def split_shift(shift):
    """shift [B, 2] read as float32 -> (i int64 [B, 2], f float64 [B, 2]) as the kernels split it"""
    s = np.asarray(shift, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        fl = np.floor(s)
        i = np.fmin(np.fmax(fl, np.float32(-2048)), np.float32(2048)).astype(np.int64)
        f = s.astype(np.float64) - fl.astype(np.float64)
    return i, f


def merged_weights(taps, f, r):
    """u[k], k = 0 .. 2r + 1, of one axis in float64 from the float32 taps t [r+1] and the fraction f"""
    t = np.concatenate([np.asarray(taps, np.float32).astype(np.float64), [0.0]])      # t[r + 1] = 0
    k = np.arange(2 * r + 2)
    return f * t[np.minimum(np.abs(k - r), r + 1)] + (1.0 - f) * t[np.minimum(np.abs(k - 1 - r), r + 1)]


def correlate(g, b, iy, ix, r):
    """D [K, K] of one query: g, b [hw, hw] float64"""
    hw = g.shape[0]
    K = 2 * r + 2
    D = np.zeros((K, K))
    for ky in range(K):
        oy = -iy - r - 1 + ky                     # source row = y' + oy
        y0, y1 = max(0, -oy), min(hw, hw - oy)
        if y0 >= y1:
            continue
        for kx in range(K):
            ox = -ix - r - 1 + kx
            x0, x1 = max(0, -ox), min(hw, hw - ox)
            if x0 >= x1:
                continue
            D[ky, kx] = np.sum(g[y0:y1, x0:x1] * b[y0 + oy:y1 + oy, x0 + ox:x1 + ox])
    return D


def link(belief, smoothed_next, shift, taps, floor, hw=HW):
    """belief, smoothed_next [B, hw, hw] (read as they are), shift [B, 2], taps [r+1] or [B, r+1], floor a number or [B] (read as
    float32) -> dict(moves [B, K, K], stats [B, 4] = (Z, G, J, M), D [B, K, K], g [B, hw, hw]), all float64."""
    b = np.asarray(belief, np.float64).reshape(-1, hw, hw)
    sn = np.asarray(smoothed_next, np.float64).reshape(-1, hw, hw)
    B = b.shape[0]
    sh = np.asarray(shift, np.float32).reshape(B, 2)
    tp = np.asarray(taps, np.float32)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    r = tp.shape[1] - 1
    K = 2 * r + 2
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (B,))
    i, f = split_shift(sh)
    moves, D, stats = np.zeros((B, K, K)), np.zeros((B, K, K)), np.zeros((B, 4))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        prior = smooth_ref.predict_c64(b, sh, tp, hw) + fl[:, None, None]
        g = np.where(sn > 0, sn / prior, 0.0)
        for q in range(B):
            D[q] = correlate(g[q], b[q], int(i[q, 1]), int(i[q, 0]), r)
            ux, uy = merged_weights(tp[q], f[q, 0], r), merged_weights(tp[q], f[q, 1], r)
            moves[q] = uy[:, None] * ux[None, :] * D[q]
            G, M = g[q].sum(), moves[q].sum()
            J = fl[q] * G * b[q].sum()
            stats[q] = (M + J, G, J, M)
    return {"moves": moves, "stats": stats, "D": D, "g": g}


def dense_pairwise(alpha_t, post_next, shift, taps, floor, hw):
    """The pairwise posterior of one link of the dense HMM of smooth_ref.dense_forward_backward, xi[x', x] = alpha_t[x] T[x', x]
    post_next[x'] / (T alpha_t)[x'] with T = u + floor, split into its move part (through u = smooth_ref.dense_kernel) binned by the
    displacement x' - x and its jump part (through floor) -> (bins {(dx, dy): mass}, jump mass)."""
    n = hw * hw
    u = smooth_ref.dense_kernel(shift, taps, hw)
    T = u + floor
    ratio = post_next / (T @ alpha_t)
    xi_move = ratio[:, None] * u * alpha_t[None, :]
    jump = float((ratio[:, None] * floor * alpha_t[None, :]).sum())
    ys, xs = np.divmod(np.arange(n), hw)
    bins = {}
    for xp in range(n):
        row = xi_move[xp]
        for x in np.nonzero(row)[0]:
            key = (int(xs[xp] - xs[x]), int(ys[xp] - ys[x]))
            bins[key] = bins.get(key, 0.0) + row[x]
    return bins, jump


# ---- a synthetic random-walk stream ----------------------------------------------------------------------------------------------------
WALK_HW, WALK_T = 48, 25
WALK_SIGMA_TRUE, WALK_SIGMA_START, WALK_RADIUS, WALK_FLOOR = 1.2, 3.0, 8, 1e-6
WALK_OBS_SIGMA = 2.0                 # width of a frame's likelihood blob, and the noise of its centre


def walk_stream(bias=(0.0, 0.0), seed=11):
    """A vehicle on a 48 x 48 grid over 25 frames: the odometry reports shifts [T-1, 2] (fractional, within +-1.5 px); the true position
    moves by the shift plus `bias` plus Gaussian noise of sigma 1.2 px per axis; every frame's likelihood is a Gaussian blob of sigma 2 px
    around the true position displaced by observation noise of that sigma -> (likelihoods [T, hw, hw] float64, shifts [T-1, 2] float32)."""
    rng = np.random.default_rng(seed)
    hw, T = WALK_HW, WALK_T
    shifts = rng.uniform(-1.5, 1.5, size=(T - 1, 2)).astype(np.float32)
    noise = rng.normal(0.0, WALK_SIGMA_TRUE, size=(T - 1, 2))
    obs = rng.normal(0.0, WALK_OBS_SIGMA, size=(T, 2))
    pos = np.zeros((T, 2))
    pos[0] = (hw / 2.0, hw / 2.0)
    for t in range(T - 1):
        pos[t + 1] = pos[t] + shifts[t].astype(np.float64) + np.asarray(bias) + noise[t]
    assert pos.min() > 4 and pos.max() < hw - 4, (pos.min(), pos.max())       # the walk stays on the grid for the seed in use
    y, x = np.mgrid[0:hw, 0:hw].astype(np.float64)
    like = np.zeros((T, hw, hw))
    for t in range(T):
        cx, cy = pos[t] + obs[t]
        like[t] = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * WALK_OBS_SIGMA ** 2))
    return like, shifts


def walk_links(like, shifts, taps, floor):
    """One E-step in float64: the filter over the likelihoods (flat first prior), the backward sweep of smooth_ref.smooth, link() per link
    -> a list of T - 1 pairs (moves [1, K, K], stats [1, 4])"""
    hw, T = like.shape[1], like.shape[0]
    beliefs = [None] * T
    for t in range(T):
        v = like[t].copy()
        if t > 0:
            v = v * (smooth_ref.predict_c64(beliefs[t - 1], shifts[t - 1][None], taps, hw)[0] + float(np.float32(floor)))
        beliefs[t] = (v / v.sum()).reshape(1, hw, hw)
    smoothed = [None] * T
    smoothed[-1] = beliefs[-1]
    for t in range(T - 2, -1, -1):
        smoothed[t] = smooth_ref.smooth(beliefs[t], smoothed[t + 1], shifts[t][None], taps, floor, hw)["s"]
    links = []
    for t in range(T - 1):
        res = link(beliefs[t], smoothed[t + 1], shifts[t][None], taps, floor, hw)
        links.append((res["moves"], res["stats"]))
    return links
