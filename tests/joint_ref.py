"""numpy float64 restatement of the joint position-heading filter (ccvpe_track_joint_predict, ccvpe_track_joint_update_logits,
include/ccvpe.h), fed the float32 inputs the device got.

predict, per query (w = 360 / nb):
    A(k', .)   = tests/track_ref.predict_c of joint[k'] under shift[k'] and taps
    u          = k - turn_deg / w,  i0 = floor(u),  f = (float)(u - i0)            (the fraction rounded once to float32)
    g(k, i)    = (1 - f) A(i0 mod nb, i) + f A((i0 + 1) mod nb, i)
    C(k, i)    = sum over j = -rh..rh of th[|j|] g((k - j) mod nb, i)
    prior(k,i) = C(k, i) + floor
update, per query:
    m = max l_i (NaN ignored, as fmaxf),  w_i = exp(l_i - m)
    E(k | i) = valid(c_i, s_i) ? e[(k - bin(c_i, s_i)) mod nb] : e[nb]             (bins: tests/heading_ref.Field, or the caller's)
    U = w E prior,  Z = sum U,  J' = U / Z,  marginal = sum over k,  hist = sum over i
    a query whose Z is zero, not finite, or without a finite float32 reciprocal: rows (-1, NaN, -1, m, Z), everything else zero
"""
import numpy as np

from tests import heading_ref as hr
from tests import track_ref

HW = 512
N = HW * HW


def predict(joint, shift, taps, turn_deg, htaps, floor):
    """joint [B, nb, 512, 512], shift [B, nb, 2], taps [r+1] or [B, r+1], turn_deg [B] or a number, htaps [rh+1] or [B, rh+1],
    floor [B] or a number -> prior float64 [B, nb, 512, 512]."""
    J = np.asarray(joint, np.float32)
    B, nb = J.shape[:2]
    tp = np.asarray(taps, np.float32)
    tp = np.broadcast_to(tp.reshape(-1, tp.shape[-1]), (B, tp.shape[-1]))
    A = track_ref.predict_c(J.reshape(B * nb, HW, HW), np.asarray(shift, np.float32).reshape(B * nb, 2), np.repeat(tp, nb, axis=0))
    A = A.reshape(B, nb, HW, HW)
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


def field_bins(ori, nb):
    """ori [B, 2, n] -> the table entry of every cell, int64 [B, n]: its heading bin, nb for a cell without a heading (float64 angles)"""
    o = np.asarray(ori, np.float32).reshape(-1, 2, N)
    out = np.empty((o.shape[0], N), np.int64)
    for b in range(o.shape[0]):
        fld = hr.Field(o[b])
        out[b] = np.where(fld.valid, fld.bins(nb)[0], nb)
    return out


def update(logits, ori, emission, nb, prior=None, bins=None):
    """logits [B, n], ori [B, 2, n], emission [nb+1] or [B, nb+1], prior [B, nb, n] or None, bins: field_bins' result or the
    device's own -> dict(rows [B, 5] float64, joint [B, nb, n], marginal [B, n], hist [B, nb], Z [B], m [B], finite [B])."""
    lg = np.asarray(logits, np.float32).reshape(-1, N)
    B = lg.shape[0]
    e = np.asarray(emission, np.float32).astype(np.float64)
    e = np.broadcast_to(e.reshape(-1, nb + 1), (B, nb + 1))
    kb = field_bins(ori, nb) if bins is None else np.asarray(bins, np.int64).reshape(B, N)
    pr = None if prior is None else np.asarray(prior, np.float32).reshape(B, nb, N)
    res = {"rows": np.zeros((B, 5)), "joint": np.zeros((B, nb, N)), "marginal": np.zeros((B, N)), "hist": np.zeros((B, nb)),
           "Z": np.zeros(B), "m": np.zeros(B), "finite": np.zeros(B, bool)}
    k = np.arange(nb)[:, None]
    for b in range(B):
        l = lg[b].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.nan if np.isnan(l).all() else np.max(np.where(np.isnan(l), -np.inf, l))
            w = np.exp(l - m)
            E = np.where(kb[b][None, :] == nb, e[b, nb], e[b, np.mod(k - np.minimum(kb[b], nb - 1)[None, :], nb)])
            U = w[None, :] * E
            if pr is not None:
                U = U * pr[b].astype(np.float64)
            Z = U.sum()
        res["Z"][b], res["m"][b] = Z, m
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            has_inv = bool(np.isfinite(np.float32(1.0 / Z))) if Z > 0 else False
        if not (np.isfinite(Z) and Z > 0 and has_inv):
            res["rows"][b] = (-1, np.nan, -1, m, Z)
            continue
        res["finite"][b] = True
        Jp = U / Z
        res["joint"][b] = Jp
        res["marginal"][b] = Jp.sum(axis=0)
        res["hist"][b] = Jp.sum(axis=1)
        i = int(np.argmax(res["marginal"][b]))
        res["rows"][b] = (i, res["marginal"][b, i], int(np.argmax(Jp[:, i])), m, Z)
    return res


# ---- the crafted stream of the filter test: two equal peaks that only the heading tells apart ----------------------------------------
SEQ_FRAMES = 6
SEQ_BINS = 8
SEQ_A, SEQ_B = (150.0, 300.0), (350.0, 200.0)   # (x, y) of the two peaks in frame 0
SEQ_FORWARD = 10.0                             # body-frame motion per frame, output pixels ahead
SEQ_HEIGHT = 14.0                              # both peaks are SEQ_HEIGHT exp(-d^2 / 18) on a zero ground
SEQ_KAPPA = 4.0                                # aerial.heading_emission
SEQ_SIGMA, SEQ_RADIUS, SEQ_FLOOR = 5.0, 14, 1e-12
SEQ_HTAPS = (0.8, 0.1)
SEQ_NEAR = 8.0                                 # the mass within this many pixels of a peak counts as that peak's


def sequence_step(table):
    """the per-frame motion of peak A: the table's shift for the bin of heading 0 degrees (the field of the stream); B moves by minus that"""
    return np.asarray(table, np.float64).reshape(SEQ_BINS, 2)[0]


def sequence_peaks(k, step):
    a = (SEQ_A[0] + step[0] * k, SEQ_A[1] + step[1] * k)
    b = (SEQ_B[0] - step[0] * k, SEQ_B[1] - step[1] * k)
    return a, b


def sequence_logits(k, step):
    """float32 [512*512] logits of frame k"""
    y, x = np.mgrid[0:HW, 0:HW].astype(np.float64)
    a, b = sequence_peaks(k, step)
    d2a = (x - a[0]) ** 2 + (y - a[1]) ** 2
    d2b = (x - b[0]) ** 2 + (y - b[1]) ** 2
    return (SEQ_HEIGHT * (np.exp(-d2a / 18.0) + np.exp(-d2b / 18.0))).astype(np.float32).reshape(-1)


def mass_near(marginal, xy, radius=SEQ_NEAR):
    """the share of a map's mass within `radius` pixels of xy"""
    m = np.asarray(marginal, np.float64).reshape(HW, HW)
    y, x = np.mgrid[0:HW, 0:HW]
    return float(m[(x - xy[0]) ** 2 + (y - xy[1]) ** 2 <= radius * radius].sum() / m.sum())
