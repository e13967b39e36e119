"""numpy float64 restatement of one backward step of the joint filter (ccvpe_track_joint_smooth, include/ccvpe.h), built
on tests/joint_ref.py's conventions and tests/smooth_ref.predict_c64, with the map side hw as a parameter; a dense forward-backward over
all nb * hw * hw states to hold it against; and the backward sweep over the crafted two-peak stream of tests/joint_ref.py.

per query, P(m; d) = smooth_ref.predict_c64(m, d, taps), w = 360 / nb:
    u0 = -turn_deg / w,  o = floor(u0),  f = (float)(u0 - o)                      (as the kernel takes them: at k = 0)
    M[d] = f th[|d - 1|] + (1 - f) th[|d|],  d = -rh .. rh + 1                     (th = 0 outside 0 .. rh)
    A(k')      = P(J[k']; shift[k'])
    prior(k)   = sum over d of M[d] A((k + o + d) mod nb) + floor
    g          = s' > 0 ? s' / prior : 0,   G = sum g
    h(k')      = sum over d of M[d] g((k' - o - d) mod nb)
    a(k')      = P(h[k']; -shift[k']) + floor G
    w = J a,  Z = sum w,  s = w / Z,  marginal = sum over k,  hist = sum over cells
G == 0: s = J, marginal / hist / (index, prob, bin) those of J (values above -inf, first index; none: -1, NaN, -1), Z = NaN.
Else Z not finite, <= 0 or without a finite float32 reciprocal: zeros and (-1, NaN, -1, Z, G).
"""
import numpy as np

from tests import joint_ref as jr
from tests import smooth_ref as sr
from tests import track_ref

HW = track_ref.HW


def circle(turn_deg, nb, htaps):
    """(o, M): the whole bins of the turn, reduced modulo nb, and the merged weights M[d + rh], d = -rh .. rh + 1, float64, f rounded
    once to float32 as the kernel holds it"""
    th = np.asarray(htaps, np.float32).astype(np.float64).reshape(-1)
    rh = th.shape[0] - 1
    u0 = -float(np.float32(turn_deg)) / (360.0 / nb)
    o = np.floor(u0)
    f = float(np.float32(u0 - o))
    t = lambda a: th[a] if a <= rh else 0.0
    M = np.array([f * t(abs(d - 1)) + (1.0 - f) * t(abs(d)) for d in range(-rh, rh + 2)])
    return int(o % nb), M


def mix(A, o, M):
    """C(k) = sum over d of M[d] A((k + o + d) mod nb): the predict's heading half, A [nb, ...]"""
    nb, rh = A.shape[0], (M.shape[0] - 2) // 2
    out = np.zeros_like(A)
    for i, d in enumerate(range(-rh, rh + 2)):
        out += M[i] * np.roll(A, -(o + d), axis=0)            # roll(A, -s)[k] = A[(k + s) mod nb]
    return out


def mix_adjoint(g, o, M):
    """h(k') = sum over d of M[d] g((k' - o - d) mod nb)"""
    nb, rh = g.shape[0], (M.shape[0] - 2) // 2
    out = np.zeros_like(g)
    with np.errstate(invalid="ignore"):
        for i, d in enumerate(range(-rh, rh + 2)):
            out += M[i] * np.roll(g, o + d, axis=0)           # roll(g, s)[k'] = g[(k' - s) mod nb]
    return out


def _per_query(v, B, width=None):
    v = np.asarray(v, np.float32)
    return np.broadcast_to(v.reshape(-1, v.shape[-1]) if width else v.reshape(-1), (B, v.shape[-1]) if width else (B,))


def predict(joint, shift, taps, turn_deg, htaps, floor, hw=HW):
    """joint_ref.predict with f taken at k = 0 and a float64 joint [B, nb, hw, hw] read as it is -> prior float64 [B, nb, hw, hw]"""
    J = np.asarray(joint, np.float64)
    B, nb = J.shape[:2]
    J = J.reshape(B, nb, hw, hw)
    sh = np.asarray(shift, np.float32).reshape(B, nb, 2)
    tp, ht = _per_query(taps, B, True), _per_query(htaps, B, True)
    turn, fl = _per_query(turn_deg, B), _per_query(floor, B).astype(np.float64)
    out = np.empty_like(J)
    for b in range(B):
        o, M = circle(turn[b], nb, ht[b])
        A = sr.predict_c64(J[b], sh[b], np.repeat(tp[b][None], nb, axis=0), hw)
        out[b] = mix(A, o, M) + fl[b]
    return out


def smooth(joint, smoothed_next, shift, taps, turn_deg, htaps, floor, hw=HW):
    """joint, smoothed_next [B, nb, hw, hw] (the device's float32 values or float64, read as they are), shift [B, nb, 2], taps [r+1] or
    [B, r+1], turn_deg a number or [B], htaps [rh+1] or [B, rh+1], floor a number or [B] (read as float32) -> dict(s [B, nb, hw, hw],
    marginal [B, hw, hw], hist [B, nb], stats [B, 5] = (index, prob, bin, Z, G), g, prior), all float64."""
    J = np.asarray(joint, np.float64)
    B, nb = J.shape[:2]
    J = J.reshape(B, nb, hw, hw)
    sn = np.asarray(smoothed_next, np.float64).reshape(B, nb, hw, hw)
    sh = np.asarray(shift, np.float32).reshape(B, nb, 2)
    tp, ht = _per_query(taps, B, True), _per_query(htaps, B, True)
    turn, fl = _per_query(turn_deg, B), _per_query(floor, B).astype(np.float64)
    res = {"s": np.zeros_like(J), "marginal": np.zeros((B, hw, hw)), "hist": np.zeros((B, nb)), "stats": np.zeros((B, 5)),
           "g": np.zeros_like(J), "prior": np.zeros_like(J)}
    for b in range(B):
        o, M = circle(turn[b], nb, ht[b])
        tps = np.repeat(tp[b][None], nb, axis=0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            prior = mix(sr.predict_c64(J[b], sh[b], tps, hw), o, M) + fl[b]
            g = np.where(sn[b] > 0, sn[b] / prior, 0.0)
            G = g.sum()
            a = sr.predict_c64(mix_adjoint(g, o, M), -sh[b], tps, hw) + fl[b] * G
            w = J[b] * a
            Z = w.sum()
            has_inv = bool(np.isfinite(np.float32(1.0 / Z))) if Z > 0 else False
        res["g"][b], res["prior"][b] = g, prior
        if G == 0:
            s, Zs = J[b], np.nan
        elif not (np.isfinite(Z) and Z > 0 and has_inv):
            res["stats"][b] = (-1, np.nan, -1, Z, G)
            continue
        else:
            s, Zs = w / Z, Z
        res["s"][b] = s
        res["marginal"][b] = s.sum(axis=0)
        res["hist"][b] = s.reshape(nb, -1).sum(axis=1)
        i, v = sr.argmax_taken(res["marginal"][b])
        k = sr.argmax_taken(s.reshape(nb, -1)[:, i])[0] if i >= 0 else -1
        res["stats"][b] = (i, v, k, Zs, G)
    return res


# ---- a dense HMM over (bin, cell) -----------------------------------------------------------------------------------------------------

def dense_transition(shift, taps, turn_deg, htaps, floor, nb, hw):
    """T [(k, x), (k', x')] = sum over d with (k + o + d) mod nb == k' of M[d] u_k'[x, x'] + floor, dense, from the unit maps"""
    n = hw * hw
    o, M = circle(turn_deg, nb, htaps)
    rh = (M.shape[0] - 2) // 2
    sh = np.asarray(shift, np.float32).reshape(nb, 2)
    u = [sr.dense_kernel(sh[k], taps, hw) for k in range(nb)]
    T = np.zeros((nb, n, nb, n))
    for k in range(nb):
        for i, d in enumerate(range(-rh, rh + 2)):
            kp = (k + o + d) % nb
            T[k, :, kp, :] += M[i] * u[kp]
    return T.reshape(nb * n, nb * n) + float(np.float32(floor))


def dense_forward_backward(likelihoods, transitions):
    """likelihoods [T, S], transitions T - 1 dense [S, S] matrices (target, source), a flat first prior -> (filtered [T, S], each of
    mass 1; smoothed [T, S]) by the textbook recursion"""
    Tn, S = likelihoods.shape
    alpha = np.zeros((Tn, S))
    alpha[0] = likelihoods[0] / likelihoods[0].sum()
    for t in range(1, Tn):
        v = likelihoods[t] * (transitions[t - 1] @ alpha[t - 1])
        alpha[t] = v / v.sum()
    beta = np.ones((Tn, S))
    for t in range(Tn - 2, -1, -1):
        v = transitions[t].T @ (likelihoods[t + 1] * beta[t + 1])
        beta[t] = v / v.max()
    post = alpha * beta
    return alpha, post / post.sum(axis=1, keepdims=True)


# ---- the crafted stream of tests/joint_ref.py: filter, then the backward sweep ----------------------------------------------------------

_STREAM = {}


def crafted_stream():
    """The filter of tests/test_track_joint_cpu.py over jr.SEQ_FRAMES frames (joints stored as float32, as the device stores them), then
    the float64 sweep -> dict(step, table, taps, joints [T] of [1, nb, 512, 512] float32, marginals [T] (the filter's), smoothed [T]
    of smooth()'s dicts (the last: the call with a zero next joint)).  Computed once."""
    if _STREAM:
        return _STREAM
    from ccvpe_amd import aerial
    nb, N = jr.SEQ_BINS, jr.N
    table = aerial.joint_shift_table(jr.SEQ_FORWARD, 0.0, nb)
    step = jr.sequence_step(table)
    em = aerial.heading_emission(jr.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jr.SEQ_SIGMA, jr.SEQ_RADIUS)
    ori = np.zeros((1, 2, N), np.float32)
    ori[:, 0] = 1.0
    joints, marginals = [], []
    joint = None
    for k in range(jr.SEQ_FRAMES):
        prior = None
        if joint is not None:
            prior = jr.predict(joint, table, taps, 0.0, jr.SEQ_HTAPS, jr.SEQ_FLOOR).astype(np.float32).reshape(1, nb, N)
        r = jr.update(jr.sequence_logits(k, step)[None], ori, em, nb, prior)
        joint = r["joint"].astype(np.float32).reshape(1, nb, 512, 512)
        joints.append(joint)
        marginals.append(r["marginal"].reshape(512, 512))
    T = jr.SEQ_FRAMES
    sm = [None] * T
    sm[-1] = smooth(joints[-1], np.zeros_like(joints[-1]), np.zeros((1, nb, 2)), [1.0], 0.0, [1.0], 0.0)
    for t in range(T - 2, -1, -1):
        sm[t] = smooth(joints[t], sm[t + 1]["s"], table, taps, 0.0, jr.SEQ_HTAPS, jr.SEQ_FLOOR)
    _STREAM.update(step=step, table=table, taps=taps, em=em, joints=joints, marginals=marginals, smoothed=sm)
    return _STREAM
