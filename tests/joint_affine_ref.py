"""numpy float64 restatement of the joint predict under an affine map per source heading bin (ccvpe_track_joint_predict_affine,
include/ccvpe.h), fed the float32 inputs the device got.

per query (w = 360 / nb):
    A(k', .)   = tests/track_affine_ref.predict_c of joint[k'] under matrix[k'] and taps          (|det| included, before floor and log)
    u          = k - turn_deg / w,  i0 = floor(u),  f = (float)(u - i0)            (the fraction rounded once to float32, per k)
    g(k, i)    = (1 - f) A(i0 mod nb, i) + f A((i0 + 1) mod nb, i)
    C(k, i)    = sum over j = -rh..rh of th[|j|] g((k - j) mod nb, i)
    prior(k,i) = C(k, i) + floor
the heading half exactly as tests/joint_ref.predict reads it.
"""
import numpy as np

from tests import joint_ref as jr
from tests import track_affine_ref as ar

HW = 512
N = HW * HW


def predict(joint, matrix, taps, turn_deg, htaps, floor):
    """joint [B, nb, 512, 512], matrix [B, nb, 6] or [nb, 6] float64, taps [r+1] or [B, r+1], turn_deg [B] or a number, htaps [rh+1]
    or [B, rh+1], floor [B] or a number -> prior float64 [B, nb, 512, 512]."""
    J = np.asarray(joint, np.float32)
    B, nb = J.shape[:2]
    mat = np.broadcast_to(np.asarray(matrix, np.float64), (B, nb, 6))
    tp = np.asarray(taps, np.float32)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    A = ar.predict_c(J.reshape(B * nb, HW, HW), mat.reshape(B * nb, 6), np.repeat(tp, nb, axis=0)).reshape(B, nb, HW, HW)
    turn = np.broadcast_to(np.asarray(turn_deg, np.float32), (B,)).astype(np.float64)
    fl = np.broadcast_to(np.asarray(floor, np.float32), (B,)).astype(np.float64)
    th = np.asarray(htaps, np.float32).astype(np.float64)
    th = np.broadcast_to(th.reshape(-1, th.shape[-1]), (B, th.shape[-1]))
    rh = th.shape[1] - 1
    assert 2 * rh + 1 <= nb
    out = np.empty((B, nb, HW, HW))
    for b in range(B):
        u = np.arange(nb, dtype=np.float64) - turn[b] / (360.0 / nb)
        i0 = np.floor(u)
        f = (u - i0).astype(np.float32).astype(np.float64)
        i = np.mod(i0, nb).astype(np.int64)
        g = (1.0 - f)[:, None, None] * A[b, i] + f[:, None, None] * A[b, (i + 1) % nb]
        c = np.zeros((nb, HW, HW))
        for j in range(-rh, rh + 1):
            c += th[b, abs(j)] * np.roll(g, j, axis=0)           # c(k) += th[|j|] g((k - j) mod nb)
        out[b] = c + fl[b]
    return out


# ---- the crafted stream: tests/joint_ref's two peaks seen from a frame that turns -----------------------------------------------------
# World coordinates are frame 0's.  Frame k shows the world turned by k * SEQ_TURN_DEG about the frame's centre, as
# tests/track_affine_ref's stream: p_k(w) = c + R_k (w - c), R_k = [[cos a, sin a], [-sin a, cos a]], a = k * SEQ_TURN_DEG
# (aerial.rigid_matrix's convention: the content turns counter-clockwise as displayed).  A street seen in both directions: peak A moves
# by the step per frame in the WORLD, peak B by minus the step; the vehicle drives along the step, so the orientation field says the
# step's heading at every cell - the centre of bin 0 in the world, SEQ_HEADING_DEG + k * SEQ_TURN_DEG as frame k's grid labels it
# (counter-clockwise labels, zero_deg 0) - and only A's motion fits it.  Logits and field of frame k are expressed in frame k's grid.
# The constants are tests/joint_ref's; eight frames at 4 degrees per frame carry the label from bin 0 into bin 1 (45 degrees).
SEQ_FRAMES = 8
SEQ_TURN_DEG = 4.0
SEQ_CENTRE = (255.5, 255.5)
SEQ_BINS = jr.SEQ_BINS
SEQ_HEADING_DEG = 180.0 / SEQ_BINS             # the centre of bin 0: the direction of joint_shift_table's shift for it
SEQ_A, SEQ_B = jr.SEQ_A, jr.SEQ_B
SEQ_FORWARD, SEQ_HEIGHT, SEQ_KAPPA = jr.SEQ_FORWARD, jr.SEQ_HEIGHT, jr.SEQ_KAPPA
SEQ_SIGMA, SEQ_RADIUS, SEQ_FLOOR = jr.SEQ_SIGMA, jr.SEQ_RADIUS, jr.SEQ_FLOOR
SEQ_HTAPS = jr.SEQ_HTAPS
SEQ_NEAR = jr.SEQ_NEAR


def _rot(k):
    a = np.radians(SEQ_TURN_DEG * k)
    return np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])


def sequence_step():
    """the per-frame world motion of peak A, (dx, dy): SEQ_FORWARD pixels along SEQ_HEADING_DEG (x right, y down)"""
    a = np.radians(SEQ_HEADING_DEG)
    return SEQ_FORWARD * np.array([np.cos(a), -np.sin(a)])


def sequence_peaks(k):
    """frame-k positions (x, y) of the two peaks"""
    c, st = np.array(SEQ_CENTRE), sequence_step()
    a = c + _rot(k) @ (np.array(SEQ_A) + k * st - c)
    b = c + _rot(k) @ (np.array(SEQ_B) - k * st - c)
    return (float(a[0]), float(a[1])), (float(b[0]), float(b[1]))


def sequence_matrix():
    """float64 [6]: pixel index of frame k -> the position in frame k - 1 that shows the same world point - the frame change alone,
    the inverse of p_k = c + R_1 (p_{k-1} - c); aerial.rigid_matrix(SEQ_TURN_DEG, (0, 0)) to rounding"""
    c = np.array(SEQ_CENTRE)
    inv = _rot(1).T
    t = c - inv @ c
    return np.array([inv[0, 0], inv[0, 1], t[0], inv[1, 0], inv[1, 1], t[1]])


def sequence_logits(k):
    """float32 [512*512] logits of frame k"""
    y, x = np.mgrid[0:HW, 0:HW].astype(np.float64)
    a, b = sequence_peaks(k)
    d2a = (x - a[0]) ** 2 + (y - a[1]) ** 2
    d2b = (x - b[0]) ** 2 + (y - b[1]) ** 2
    return (SEQ_HEIGHT * (np.exp(-d2a / 18.0) + np.exp(-d2b / 18.0))).astype(np.float32).reshape(-1)


def sequence_ori(k):
    """float32 [2, 512*512] orientation field of frame k: the step's heading as frame k's grid labels it, at every cell"""
    a = np.radians(SEQ_HEADING_DEG + k * SEQ_TURN_DEG)
    o = np.empty((2, N), np.float32)
    o[0], o[1] = np.cos(a), np.sin(a)
    return o


mass_near = jr.mass_near
