"""Link statistics of a smoothed stream: what a recorded stream says about the motion model of its tracker.

aerial.Tracker's filter rests on three numbers its caller has to choose: the blur `taps` (a sigma), the relocalisation `floor` and the
odometry behind `shift`.  A hidden Markov model gets its transition model from the pairwise posterior p(x_t, x_t+1 | frames 1..T),
summarised as expected transition counts - the E-step of Baum-Welch.  track_link computes it for one link, binned by displacement:

    tracker = smooth.RecordingTracker()
    for frame in stream:
        rows = tracker.step(model, grd, cache, tile_index, origins, motion_map_px, taps, floor)
    maps, _ = smooth.smooth_stream(model, tracker.log)
    links = motion.link_stream(model, tracker.log, maps)                   # one (moves, stats) per link t -> t + 1
    shifts = [entry[1] for entry in tracker.log[1:]]
    fit = motion.fit_motion(links, shifts, radius)                         # sigma, floor, taps, bias: the M-step, on the host

moves[b, ky, kx] / Z is the posterior probability that the link was a move under the motion kernel by the integer displacement
link_offsets names, stats' jump / evidence that it was a jump through the floor (ccvpe_track_link, include/ccvpe.h: the definition and
the error bound).  link_moments turns a link into shares and residual moments, fit_motion pools the links of a stream.

Out of scope: links of aerial.AffineTracker (the displacement grid is not the tap grid through a matrix; the analogue works on the h
plane of DESIGN.md 4.22), the heading belief, re-running the filter inside fit_motion, fitting taps that are not Gaussian (moves is
returned whole, so a caller can).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, aerial, smooth

# columns of stats: Z = M + J, the evidence (smooth.SMOOTH_FIELDS' evidence up to rounding); G = sum s' / prior, the future's total
# weight (the smoother's bits); J, the mass of a jump through the floor; M = sum moves, the mass of a move under the motion kernel
LINK_FIELDS = ("evidence", "future", "jump", "move")
# columns of link_moments: the shares M / Z and J / Z; mean and central second moments of the residual displacement - shift, in pixels
MOMENT_FIELDS = ("move", "jump", "mean_x", "mean_y", "var_x", "var_y", "cov_xy")
_CELLS = 512 * 512


class _LinkResults:
    """track_link's results behind models._Layout's interface: moves and stats, then the work buffer as the last pointer before the
    stream (torch's allocator keeps its memory for this stream's launches after the tensor is dropped)."""

    def __init__(self, radius: int):
        self.radius = radius

    def alloc(self, B: int, dev):
        K = 2 * self.radius + 2
        moves = torch.empty((B, K, K), dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(LINK_FIELDS)), dtype=torch.float32, device=dev)
        work = torch.empty(_lib.load().ccvpe_track_link_work_bytes(B, self.radius), dtype=torch.uint8, device=dev)
        return [moves, stats], [moves.data_ptr(), stats.data_ptr(), work.data_ptr()]


def track_link(model, belief, smoothed_next, shift_px, taps, floor):
    """One link: (moves [B, 2r+2, 2r+2], stats [B,4]) from belief [B,512,512], the filter posterior of frame t, smoothed_next, the
    smoothed map of frame t + 1, and shift_px, taps, floor, the arguments of the model.track_predict call that carried belief into
    frame t + 1 - smooth.track_smooth's arguments, checked as it checks them and in its order.  stats: LINK_FIELDS.  Row ky, column kx
    of moves is the displacement link_offsets gives.  There is no degenerate rule: a next map without a positive cell gives zero moves
    and evidence 0, a NaN in belief NaN; a link is usable when its evidence is finite and > 0.  smoothed_next may be belief.  Four
    launches; the work buffer is allocated here, per call."""
    model._require_eval()
    B = model._stored_maps(belief)
    if model._stored_maps(smoothed_next, "smoothed_next") != B:
        raise ValueError(f"smoothed_next holds {smoothed_next.shape[0]} maps, belief {B}")
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    dev = belief.device
    sh = model._track_vec(shift_px, "shift_px", (B, 2), dev)
    tp = model._track_vec(taps, "taps", tshape, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    smooth._check_placement(model, belief, smoothed_next, None, B)
    model._ensure_handle(dev)
    return model._launch("track_link", dev, B, (belief, smoothed_next, B, sh, tp, stride, radius, fl), _LinkResults(radius))


def link_stream(model, log, maps):
    """The links of a smooth.RecordingTracker's log (T entries (belief, shift, taps, floor)) and the maps of smooth.smooth_stream over
    it -> a list of T - 1 pairs (moves, stats), entry t the link from frame t to frame t + 1: track_link of log[t]'s belief and
    maps[t + 1] with entry t + 1's shift, taps and floor.  Lists, because the radius may differ per link."""
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    if len(maps) != T:
        raise ValueError(f"maps holds {len(maps)} frames, the log {T}")
    links = []
    for t in range(T - 1):
        _, shift, taps, floor = log[t + 1]
        if shift is None:
            raise ValueError(f"log entry {t + 1} has no shift: a stream's first frame can only stand first")
        links.append(track_link(model, log[t][0], maps[t + 1], shift, taps, floor))
    return links


def _shift_f32(shift_px):
    s = shift_px.detach().cpu().numpy() if isinstance(shift_px, torch.Tensor) else np.asarray(shift_px)
    s = s.astype(np.float32)
    if s.shape[-1:] != (2,) or s.ndim not in (1, 2):
        raise ValueError(f"shift_px must be [2] or [B,2], got {s.shape}")
    return s


def link_offsets(shift_px, radius: int):
    """(dx, dy): the integer displacement x' - x of every column kx and row ky of moves, ix + r + 1 - kx and iy + r + 1 - ky with
    i = floor(shift) clamped to +-2048 as the kernel computes it (the shift read as float32; NaN clamps to -2048).  int64 [2r+2] each
    for shift_px [2], [B, 2r+2] for [B,2]."""
    r = int(radius)
    if not 0 <= r <= 32:
        raise ValueError(f"radius must be in 0..32, got {radius}")
    s = _shift_f32(shift_px)
    with np.errstate(invalid="ignore"):
        i = np.fmin(np.fmax(np.floor(s), np.float32(-2048)), np.float32(2048)).astype(np.int64)
    k = np.arange(2 * r + 2, dtype=np.int64)
    return i[..., 0, None] + r + 1 - k, i[..., 1, None] + r + 1 - k


def link_moments(moves, stats, shift_px):
    """A link as seven numbers per query, float64 [B,7] on moves' device (MOMENT_FIELDS): the shares M / Z of a move and J / Z of a
    jump, and the mean and the central second moments of the residual displacement - shift_px (pixels) under moves / sum moves.  A
    link that is not usable (evidence not finite or not > 0) gives a NaN row; a usable link without move mass has its two shares and
    NaN moments.  shift_px: host data [B,2] or [2] (a device tensor is downloaded)."""
    moves, stats = torch.as_tensor(moves), torch.as_tensor(stats)
    B, K = moves.shape[0], moves.shape[-1]
    if moves.ndim != 3 or moves.shape[1] != K or K % 2 or K < 2 or tuple(stats.shape) != (B, len(LINK_FIELDS)):
        raise ValueError(f"moves must be [B, 2r+2, 2r+2] and stats [B, 4], got {tuple(moves.shape)} and {tuple(stats.shape)}")
    r = K // 2 - 1
    s = np.broadcast_to(_shift_f32(shift_px).reshape(-1, 2), (B, 2)).astype(np.float64)
    ox, oy = link_offsets(s.astype(np.float32), r)
    dev = moves.device
    rx = torch.as_tensor(ox - s[:, 0, None], device=dev)[:, None, :]                   # [B, 1, K]
    ry = torch.as_tensor(oy - s[:, 1, None], device=dev)[:, :, None]                   # [B, K, 1]
    m = moves.to(torch.float64)
    st = stats.to(torch.float64)
    Z = st[:, 0]
    total = m.sum(dim=(1, 2))
    p = m / total[:, None, None]
    mx, my = (p * rx).sum(dim=(1, 2)), (p * ry).sum(dim=(1, 2))
    cx, cy = rx - mx[:, None, None], ry - my[:, None, None]
    out = torch.stack([st[:, 3] / Z, st[:, 2] / Z, mx, my, (p * cx * cx).sum(dim=(1, 2)), (p * cy * cy).sum(dim=(1, 2)),
                       (p * cx * cy).sum(dim=(1, 2))], dim=1)
    usable = torch.isfinite(Z) & (Z > 0)
    return torch.where(usable[:, None], out, torch.full_like(out, float("nan")))


def fit_motion(links, shifts, radius: int, cells: int = _CELLS):
    """The M-step over the links of a stream, in float64 on the host: links a list of (moves, stats) as link_stream returns them,
    shifts the shift_px of every link ([B,2] or [2]; log[t + 1][1]), radius that of the taps to make.  Over the usable link queries
    (evidence finite and > 0; every other weighs 0):
        rho    the mean of J / Z, the posterior share of jumps; floor = rho / ((1 - rho) * cells), cells = 262144 - the filter's
               u + floor is the mixture (1 - rho) u + rho / N up to the scale the update's softmax removes
        bias   the pooled mean residual (x, y) in pixels - an odometry bias such as a scale error in motion_map_px; reported, not applied
        sigma  sqrt(max(m2 - tent, tiny)): m2 the pooled second moment of the residual about zero, averaged over the two axes, tent the
               pooled (fx (1 - fx) + fy (1 - fy)) / 2, the variance the bilinear split of a fractional shift itself adds
        taps   aerial.gaussian_taps(sigma, radius)
    pooled: weighted by moves / Z over all usable links.  -> dict(sigma, floor, rho, bias, taps, links), links the number of usable
    link queries; sigma, bias and taps are NaN / None when no move mass was seen.
    This is moment matching, not a likelihood maximisation over the taps: exact for a Gaussian that the radius does not truncate, low
    when the radius of the links clips the tails.  The log of a stream holds posteriors, not likelihoods, so the next E-step needs the
    tracker run again with the new parameters.  An offline tool: it downloads a few hundred numbers per link and so synchronises with
    the device."""
    if len(links) != len(shifts):
        raise ValueError(f"{len(links)} links, {len(shifts)} shifts")
    rho_sum, used, mass, m2, tent = 0.0, 0, 0.0, 0.0, 0.0
    mean = np.zeros(2)
    for (moves, stats), shift in zip(links, shifts):
        mv = torch.as_tensor(moves).detach().cpu().numpy().astype(np.float64)
        st = torch.as_tensor(stats).detach().cpu().numpy().astype(np.float64)
        B, K = mv.shape[0], mv.shape[-1]
        r = K // 2 - 1
        s = np.broadcast_to(_shift_f32(shift).reshape(-1, 2), (B, 2)).astype(np.float64)
        ox, oy = link_offsets(s.astype(np.float32), r)
        for q in range(B):
            Z = st[q, 0]
            if not (np.isfinite(Z) and Z > 0):
                continue
            used += 1
            rho_sum += st[q, 2] / Z
            p = mv[q] / Z
            rx, ry = (ox[q] - s[q, 0])[None, :], (oy[q] - s[q, 1])[:, None]
            w = p.sum()
            mass += w
            mean += ((p * rx).sum(), (p * ry).sum())
            m2 += 0.5 * ((p * rx * rx).sum() + (p * ry * ry).sum())
            f = s[q] - np.floor(s[q])
            tent += w * 0.5 * float((f * (1.0 - f)).sum())
    if used == 0:
        raise ValueError("no usable link: every evidence is zero or not finite")
    rho = rho_sum / used
    floor = rho / ((1.0 - rho) * cells) if rho < 1.0 else float("inf")
    if not mass > 0:
        return {"sigma": float("nan"), "floor": floor, "rho": rho, "bias": np.full(2, np.nan), "taps": None, "links": used}
    sigma = float(np.sqrt(max(m2 / mass - tent / mass, 1e-12)))
    return {"sigma": sigma, "floor": floor, "rho": rho, "bias": mean / mass, "taps": aerial.gaussian_taps(sigma, radius), "links": used}
