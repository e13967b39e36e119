"""numpy float64 restatement of the two halves of a tracking step (ccvpe_track_predict, ccvpe_track_update*, include/ccvpe.h).

predict, per query:
    belief extended by zero outside its 512 x 512 grid
    s(x, y)   = bilinear sample of the belief at (x - dx, y - dy)      (dx, dy the float32 shift, read as float64)
    c         = s convolved with t[|i|], i = -r..r, along x, then along y     (t the float32 taps, read as float64)
    out(x, y) = log(c(x, y) + floor)                                   on the 512 x 512 window
update, per query: tests/prior_ref.posterior (l' = fl32(logits + log_prior), m', inv', h'), the argmax row, and the map h' - all zeros
    for a query without a finite posterior.
"""
import numpy as np

from tests import prior_ref

HW = 512
N = HW * HW


def predict_c(belief, shift, taps, hw=HW):
    """belief [B, hw, hw], shift [B, 2] = (dx, dy), taps [r+1] or [B, r+1] -> c [B, hw, hw] float64 (before floor and log)."""
    bel = np.asarray(belief, np.float32).astype(np.float64).reshape(-1, hw, hw)
    B = bel.shape[0]
    sh = np.asarray(shift, np.float32).astype(np.float64).reshape(B, 2)
    tp = np.asarray(taps, np.float32).astype(np.float64)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    r = tp.shape[1] - 1
    out = np.zeros((B, hw, hw))
    # the plane is evaluated on the window plus the blur's reach; everything beyond is zero or cannot reach the window
    ext = np.arange(-r, hw + r, dtype=np.float64)
    for b in range(B):
        dx, dy = sh[b]

        def axis(d):
            """source index and weights of the 2-tap bilinear filter along one axis, for every extended coordinate"""
            pos = ext - d
            i0 = np.floor(pos)
            f = pos - i0
            return i0.astype(np.int64), 1.0 - f, f

        ix, wx0, wx1 = axis(dx)
        iy, wy0, wy1 = axis(dy)
        pad = np.zeros((hw + 2, hw + 2))          # index -1 .. hw: one ring of the zero extension
        pad[1:-1, 1:-1] = bel[b]

        def take(iy_, ix_):
            yy = np.clip(iy_, -1, hw) + 1
            xx = np.clip(ix_, -1, hw) + 1
            return pad[yy[:, None], xx[None, :]]

        s = (wy0[:, None] * (wx0[None, :] * take(iy, ix) + wx1[None, :] * take(iy, ix + 1)) +
             wy1[:, None] * (wx0[None, :] * take(iy + 1, ix) + wx1[None, :] * take(iy + 1, ix + 1)))
        full = np.concatenate([tp[b, :0:-1], tp[b]])                                  # t[|i|], i = -r..r
        cx = np.zeros((hw + 2 * r, hw))
        for k in range(2 * r + 1):
            cx += full[k] * s[:, k:k + hw]
        c = np.zeros((hw, hw))
        for k in range(2 * r + 1):
            c += full[k] * cx[k:k + hw, :]
        out[b] = c
    return out


def predict(belief, shift, taps, floor, hw=HW):
    """-> log(c + floor) float64 [B, hw, hw] (-inf where c + floor == 0)."""
    c = predict_c(belief, shift, taps, hw)
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (c.shape[0],))
    with np.errstate(divide="ignore"):
        return np.log(c + fl[:, None, None])


def update(logits, ori, log_prior=None):
    """logits [B, n], ori [B, 2, n], log_prior [B, n] / [n] / None -> (rows [B, 5], margin [B], posterior [B, n] float64)."""
    lg = np.asarray(logits, np.float32).reshape(logits.shape[0], -1)
    lp = np.zeros(lg.shape[1], np.float32) if log_prior is None else log_prior
    rows, margin = prior_ref.argmax_rows(lg, ori, lp)
    post = prior_ref.posterior(lg, lp)
    h = np.where(post["finite"][:, None], post["h"], 0.0)
    return rows, margin, h


# ---- the crafted stream of the filter test -----------------------------------------------------------------------------------------
SEQ_FRAMES = 12
SEQ_START = (100.0, 200.0)       # (x, y) of the true peak in frame 0
SEQ_STEP = (7.0, 5.0)            # its motion per frame, output pixels
SEQ_DISTRACTOR = (400.0, 100.0)  # a static second peak ...
SEQ_STRONG = (2, 5, 8, 11)       # ... which is the larger of the two in these frames (10 against 8; 6 otherwise)
SEQ_SIGMA, SEQ_RADIUS, SEQ_FLOOR = 2.0, 6, 1e-9


def sequence_truth(k):
    return SEQ_START[0] + SEQ_STEP[0] * k, SEQ_START[1] + SEQ_STEP[1] * k


def sequence_logits(k, hw=HW):
    """float32 [hw*hw] logits of frame k: the true peak 8 exp(-d^2 / 18) plus the distractor of the same width, on a zero ground."""
    y, x = np.mgrid[0:hw, 0:hw].astype(np.float64)
    tx, ty = sequence_truth(k)
    d2t = (x - tx) ** 2 + (y - ty) ** 2
    d2d = (x - SEQ_DISTRACTOR[0]) ** 2 + (y - SEQ_DISTRACTOR[1]) ** 2
    height = 10.0 if k in SEQ_STRONG else 6.0
    return (8.0 * np.exp(-d2t / 18.0) + height * np.exp(-d2d / 18.0)).astype(np.float32).reshape(-1)


def pixel_distance(index, xy, hw=HW):
    return float(np.hypot(index % hw - xy[0], index // hw - xy[1]))
