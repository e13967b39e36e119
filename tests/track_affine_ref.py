"""numpy float64 restatement of the affine predict step (ccvpe_track_predict_affine, include/ccvpe.h), written like tests/track_ref.py.

per query, with the belief extended by zero outside its 512 x 512 grid and M = (m0..m5) float64:
    (sx, sy)  = (m0 x + m1 y + m2, m3 x + m4 y + m5)       x, y integer pixel indices, float64
    ix, iy    = floor;  fx, fy = float32(sx - ix), float32(sy - iy), used as float64; weights 1 - f (from the rounded f) and f
    s(x, y)   = float32(|m0 m4 - m1 m3|) * bilinear sample of the belief at (sx, sy)
    c         = s convolved with t[|i|], i = -r..r, along x, then along y     (t the float32 taps, read as float64)
    out(x, y) = log(c(x, y) + floor)                        on the 512 x 512 window
"""
import numpy as np

HW = 512
N = HW * HW


def predict_c(belief, matrix, taps, hw=HW):
    """belief [B, hw, hw], matrix [B, 6] or [6], taps [r+1] or [B, r+1] -> c [B, hw, hw] float64 (before floor and log)."""
    bel = np.asarray(belief, np.float32).astype(np.float64).reshape(-1, hw, hw)
    B = bel.shape[0]
    mat = np.broadcast_to(np.asarray(matrix, np.float64).reshape(-1, 6), (B, 6))
    tp = np.asarray(taps, np.float32).astype(np.float64)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    r = tp.shape[1] - 1
    out = np.zeros((B, hw, hw))
    # the plane is evaluated on the window plus the blur's reach; nothing beyond can reach the window
    ext = np.arange(-r, hw + r, dtype=np.float64)
    X, Y = ext[None, :], ext[:, None]
    for b in range(B):
        m0, m1, m2, m3, m4, m5 = mat[b]
        det = float(np.float32(abs(m0 * m4 - m1 * m3)))
        sx = m0 * X + m1 * Y + m2
        sy = m3 * X + m4 * Y + m5
        fx0, fy0 = np.floor(sx), np.floor(sy)
        fx = (sx - fx0).astype(np.float32).astype(np.float64)
        fy = (sy - fy0).astype(np.float32).astype(np.float64)
        # (far positions are brought next to the grid before the conversion; they read zeros either way)
        ix = np.clip(fx0, -4.0, hw + 4.0).astype(np.int64)
        iy = np.clip(fy0, -4.0, hw + 4.0).astype(np.int64)
        pad = np.zeros((hw + 2, hw + 2))          # index -1 .. hw: one ring of the zero extension
        pad[1:-1, 1:-1] = bel[b]

        def take(iy_, ix_):
            # clipped AFTER the neighbour offset was added: index -5 + 1 is still outside, not column 0
            return pad[np.clip(iy_, -1, hw) + 1, np.clip(ix_, -1, hw) + 1]

        s = det * ((1.0 - fy) * ((1.0 - fx) * take(iy, ix) + fx * take(iy, ix + 1)) +
                   fy * ((1.0 - fx) * take(iy + 1, ix) + fx * take(iy + 1, ix + 1)))
        full = np.concatenate([tp[b, :0:-1], tp[b]])                                  # t[|i|], i = -r..r
        cx = np.zeros((hw + 2 * r, hw))
        for k in range(2 * r + 1):
            cx += full[k] * s[:, k:k + hw]
        c = np.zeros((hw, hw))
        for k in range(2 * r + 1):
            c += full[k] * cx[k:k + hw, :]
        out[b] = c
    return out


def predict(belief, matrix, taps, floor, hw=HW):
    """-> log(c + floor) float64 [B, hw, hw] (-inf where c + floor == 0)."""
    c = predict_c(belief, matrix, taps, hw)
    fl = np.broadcast_to(np.asarray(floor, np.float32).astype(np.float64).reshape(-1), (c.shape[0],))
    with np.errstate(divide="ignore"):
        return np.log(c + fl[:, None, None])


# ---- the crafted stream of the filter test: tests/track_ref's stream seen from a frame that turns ------------------------------------
# World coordinates are frame 0's.  Frame k shows the world turned by k * SEQ_TURN_DEG about the frame's centre:
#     p_k(w) = c + R_k (w - c),   R_k = [[cos a, sin a], [-sin a, cos a]],  a = k * SEQ_TURN_DEG   (aerial.rigid_matrix's convention)
# The true peak moves by SEQ_STEP per frame in the WORLD; the distractor keeps its FRAME position.
SEQ_FRAMES = 12
SEQ_TURN_DEG = 4.0
SEQ_CENTRE = (255.5, 255.5)
SEQ_START = (180.0, 300.0)       # world (x, y) of the true peak in frame 0
SEQ_STEP = (7.0, 5.0)            # its motion per frame, world pixels
SEQ_DISTRACTOR = (400.0, 100.0)  # a second peak, fixed in the frame ...
SEQ_STRONG = (2, 5, 8, 11)       # ... which is the larger of the two in these frames (10 against 8; 6 otherwise)
SEQ_SIGMA, SEQ_RADIUS, SEQ_FLOOR = 2.0, 6, 1e-9


def _rot(k):
    a = np.radians(SEQ_TURN_DEG * k)
    return np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])


def sequence_truth(k):
    """frame-k position (x, y) of the true peak"""
    c = np.array(SEQ_CENTRE)
    w = np.array(SEQ_START) + k * np.array(SEQ_STEP)
    p = c + _rot(k) @ (w - c)
    return float(p[0]), float(p[1])


def sequence_matrix(k):
    """float64 [6]: pixel index of frame k -> the position in frame k - 1 whose content (moved by the peak's step) it shows: the
    inverse of p_k = c + R_1 (p_{k-1} - c) + R_k SEQ_STEP."""
    c = np.array(SEQ_CENTRE)
    inv = _rot(1).T
    t = c - inv @ (c + _rot(k) @ np.array(SEQ_STEP))
    return np.array([inv[0, 0], inv[0, 1], t[0], inv[1, 0], inv[1, 1], t[1]])


def sequence_logits(k, hw=HW):
    """float32 [hw*hw] logits of frame k: the true peak 8 exp(-d^2 / 18) plus the distractor of the same width, on a zero ground."""
    y, x = np.mgrid[0:hw, 0:hw].astype(np.float64)
    tx, ty = sequence_truth(k)
    d2t = (x - tx) ** 2 + (y - ty) ** 2
    d2d = (x - SEQ_DISTRACTOR[0]) ** 2 + (y - SEQ_DISTRACTOR[1]) ** 2
    height = 10.0 if k in SEQ_STRONG else 6.0
    return (8.0 * np.exp(-d2t / 18.0) + height * np.exp(-d2d / 18.0)).astype(np.float32).reshape(-1)
