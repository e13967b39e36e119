"""Smoothing a tracked stream: the backward half of the histogram filter of aerial.Tracker.

The filter answers p(x_t | frames 1..t).  An offline user - re-evaluating a traverse, building a map, labelling a calibration study -
wants p(x_t | frames 1..T), with the later frames counted in: the filter is weakest at the start of a stream and after every restart,
where it has no prior yet and a distractor wins.

    tracker = smooth.RecordingTracker()
    for frame in stream:
        rows = tracker.step(model, grd, cache, tile_index, origins, motion_map_px, taps, floor)
    maps, stats = smooth.smooth_stream(model, tracker.log)      # maps[t] [B,512,512], stats [T,B,4] (SMOOTH_FIELDS)

track_smooth is one backward step (ccvpe_track_smooth, include/ccvpe.h: the definition, the degenerate rules, the error bound).

Streams of aerial.AffineTracker - frames whose grids turn or change scale, KITTI's heading-up tiles - have the same three pieces
(DESIGN.md 4.22): RecordingAffineTracker, smooth_stream_affine and track_smooth_affine (ccvpe_track_smooth_affine), whose adjoint of
the bilinear gather through the matrix is a gather over every cell's candidate samples in a fixed order, within the reach
affine_reach measures.

Out of scope: the heading belief (hist is not smoothed), pose rows with orientation at the smoothed cell.  The MAP trajectory - one
consistent sequence of cells instead of T marginals - is ccvpe_amd.viterbi's, over the same logs: map_path and, for a
RecordingAffineTracker's, map_path_affine.
What a stream says about taps, floor and the odometry - the pairwise posterior of every link - is ccvpe_amd.motion's.

Streams of aerial.JointTracker - the filter over (heading bin, cell) - have the same three pieces:
RecordingJointTracker, smooth_joint_stream and track_joint_smooth (ccvpe_track_joint_smooth), which give p(cell, heading bin | frames
1..T) with its marginal map, heading histogram and a stats row per frame.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, aerial, spec

# columns of stats: the first index of the largest smoothed cell, the map's value there, Z = sum_i belief_i a_i - the evidence the
# later frames give this belief, sum s' (about 1) when the belief has mass 1 - and G = sum_i s'_i / prior_i, the future's total weight
SMOOTH_FIELDS = ("index", "prob", "evidence", "future")


# columns of track_joint_smooth's stats: the first argmax cell of the smoothed marginal, the marginal there, the first argmax heading bin
# of the smoothed joint at that cell, Z and G as above
JOINT_SMOOTH_FIELDS = ("index", "prob", "bin", "evidence", "future")


class _SmoothResults:
    """track_smooth's results behind models._Layout's interface: the smoothed map - `out` when the caller gave one - and stats, then the
    work buffer as the last pointer before the stream (torch's allocator keeps its memory for this stream's launches after the tensor
    is dropped).  work_bytes: the library's size function of the entry point."""

    def __init__(self, out, work_bytes: str = "ccvpe_track_smooth_work_bytes"):
        self.out = out
        self.work_bytes = work_bytes

    def alloc(self, B: int, dev):
        smoothed = self.out if self.out is not None else torch.empty((B,) + spec.OUT_HW, dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(SMOOTH_FIELDS)), dtype=torch.float32, device=dev)
        work = torch.empty(getattr(_lib.load(), self.work_bytes)(B), dtype=torch.uint8, device=dev)
        return [smoothed, stats], [smoothed.data_ptr(), stats.data_ptr(), work.data_ptr()]


def _check_placement(model, belief, smoothed_next, out, B: int) -> None:
    """where the maps of a backward step live, and the out tensor: the last checks of track_smooth, in its order"""
    dev = belief.device
    if not belief.is_cuda:
        raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
    if smoothed_next.device != dev:
        raise ValueError(f"smoothed_next is on {smoothed_next.device}, belief on {dev}")
    if out is not None:
        if model._stored_maps(out, "out") != B or out.device != dev:
            raise ValueError(f"out must hold {B} maps on {dev}")
        if out.data_ptr() == belief.data_ptr():
            raise ValueError("out must not be belief")


def track_smooth(model, belief, smoothed_next, shift_px, taps, floor, out=None):
    """One backward step: (smoothed [B,512,512], stats [B,4]) of frame t from belief [B,512,512], the filter posterior of frame t
    (track_update's map), smoothed_next, the smoothed map of frame t + 1 (for the last frame but one: the last frame's belief), and
    shift_px, taps, floor, the arguments of the model.track_predict call that carried belief into frame t + 1 - checked as that
    method checks them and in its order, smoothed_next like belief and directly after it.  stats: SMOOTH_FIELDS.  A next map
    without a positive cell says nothing: smoothed is belief bit for bit and stats (belief's argmax, its value, NaN, 0); a belief
    the recursion cannot weigh (all zero, a NaN) gives a zero map and (-1, NaN, Z, G).  out: the tensor that receives the smoothed
    map (same shape, float32, contiguous, on belief's device); out=smoothed_next is the in-place form of a backward sweep, with the
    bits of the out-of-place call.  Three launches; the work buffer is allocated here, per call."""
    model._require_eval()
    B = model._stored_maps(belief)
    if model._stored_maps(smoothed_next, "smoothed_next") != B:
        raise ValueError(f"smoothed_next holds {smoothed_next.shape[0]} maps, belief {B}")
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    dev = belief.device
    sh = model._track_vec(shift_px, "shift_px", (B, 2), dev)
    tp = model._track_vec(taps, "taps", tshape, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    _check_placement(model, belief, smoothed_next, out, B)
    model._ensure_handle(dev)
    return model._launch("track_smooth", dev, B, (belief, smoothed_next, B, sh, tp, stride, radius, fl), _SmoothResults(out))


def affine_reach(matrix):
    """(hx, hy) of an affine map [6] or [B,6] (model.track_predict_affine's matrix): the half extents, in pixels of the predict's
    output grid, of the box of sample positions that can touch one source cell - hx = |N00| + |N01|, hy = |N10| + |N11| with N the
    inverse of [[m0, m1], [m3, m4]], in float64 as ccvpe_track_smooth_affine computes them.  Numbers for [6], arrays [B] for [B,6];
    inf or NaN for a singular matrix.  track_smooth_affine supports a link when |m0 m4 - m1 m3|, rounded to float32, is finite and
    non-zero and both are <= 3."""
    m = np.asarray(matrix, dtype=np.float64)
    if m.ndim not in (1, 2) or m.shape[-1] != 6:
        raise ValueError(f"matrix must be [6] or [B,6], got {m.shape}")
    m0, m1, _, m3, m4, _ = np.moveaxis(m, -1, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = m0 * m4 - m1 * m3
        hx, hy = np.abs(m4 / d) + np.abs(-m1 / d), np.abs(-m3 / d) + np.abs(m0 / d)
    return (float(hx), float(hy)) if m.ndim == 1 else (hx, hy)


def _within_reach(matrix) -> np.ndarray:
    """the reach rule of ccvpe_track_smooth_affine per row of a host matrix [.., 6] -> bool [..]"""
    m = np.asarray(matrix, dtype=np.float64)
    hx, hy = affine_reach(m)
    with np.errstate(over="ignore", invalid="ignore"):
        det = np.abs(m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]).astype(np.float32)
        return np.isfinite(det) & (det != 0) & (np.asarray(hx) <= 3.0) & (np.asarray(hy) <= 3.0)


def _matrix_checked(matrix, B: int):
    """model.track_predict_affine's checks of its matrix, in its order, for the calls that take that call's arguments (track_smooth_affine,
    viterbi.track_viterbi_affine) -> (tensor [6] or [B,6], on_device): host data as a float64 host tensor, finite; a device tensor
    float64 and not looked at."""
    on_device = isinstance(matrix, torch.Tensor) and matrix.device.type != "cpu"
    if on_device:
        mt = matrix.detach()
        if mt.dtype != torch.float64:
            raise ValueError(f"matrix on the device must be float64, got {mt.dtype}")
    else:
        mt = torch.as_tensor(np.asarray(matrix.detach() if isinstance(matrix, torch.Tensor) else matrix, dtype=np.float64))
    if tuple(mt.shape) not in ((6,), (B, 6)):
        raise ValueError(f"matrix must be [6] or [{B}, 6], got {tuple(mt.shape)}")
    if not on_device and not bool(torch.isfinite(mt).all()):
        raise ValueError("matrix must be finite")
    return mt, on_device


def _matrix_placed(mt, on_device: bool, B: int, dev, ref: str = "belief"):
    """the checked matrix as the library reads it: [B,6] float64 on dev, the device of the map `ref`; a device tensor must be there"""
    if on_device and mt.device != dev:
        raise ValueError(f"matrix is on {mt.device}, {ref} on {dev}")
    return mt.expand(B, 6).to(dev).contiguous()


def track_smooth_affine(model, belief, smoothed_next, matrix, taps, floor, out=None):
    """track_smooth for a link made by model.track_predict_affine: matrix ([B,6] or [6]), taps, floor are that call's arguments, checked
    as that method checks them and in its order, smoothed_next like belief and directly after it; everything else - the results,
    stats, the degenerate rules, out - is track_smooth's (ccvpe_track_smooth_affine, include/ccvpe.h: the definition, the reach rule,
    the error bound).  A host matrix beyond reach (affine_reach) is refused with ValueError; a float64 tensor on the belief's device
    is not looked at, and the kernel's rule applies: a query beyond reach is a broken link - smoothed is belief bit for bit, stats
    (belief's argmax, its value, NaN, 0).  Four launches; the work buffer is allocated here, per call."""
    model._require_eval()
    B = model._stored_maps(belief)
    if model._stored_maps(smoothed_next, "smoothed_next") != B:
        raise ValueError(f"smoothed_next holds {smoothed_next.shape[0]} maps, belief {B}")
    mt, on_device = _matrix_checked(matrix, B)
    if not on_device:
        ok = np.atleast_1d(_within_reach(mt.numpy()))
        if not ok.all():
            q = int(np.argmin(ok))
            hx, hy = affine_reach(mt.numpy().reshape(-1, 6)[q])
            raise ValueError(f"matrix {q} is beyond the smoother's reach: a determinant that is finite and non-zero in float32 and "
                             f"half extents <= 3 are needed, got (hx, hy) = ({hx:.4g}, {hy:.4g})")
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    dev = belief.device
    tp = model._track_vec(taps, "taps", tshape, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    _check_placement(model, belief, smoothed_next, out, B)
    mt = _matrix_placed(mt, on_device, B, dev)
    model._ensure_handle(dev)
    return model._launch("track_smooth_affine", dev, B, (belief, smoothed_next, B, mt, tp, stride, radius, fl),
                         _SmoothResults(out, "ccvpe_track_smooth_affine_work_bytes"))


class RecordingTracker(aerial.Tracker):
    """aerial.Tracker that keeps what a backward sweep needs: step() is the parent's - the same arguments, the same returns, the same
    rows and beliefs bit for bit - and appends (belief, shift, taps, floor) to self.log, one entry per frame: the posterior the step
    stored and the arguments of the model.track_predict call that led into this frame (shift None for the first frame of a stream,
    which has no such call).  The beliefs are the tensors the update returned, not copies: every call into the library allocates its
    results anew (models._launch), so nothing writes to them again.  reset() clears the log."""

    def __init__(self):
        super().__init__()
        self.log = []

    def reset(self) -> None:
        super().reset()
        self.log = []

    def step(self, model, grd, cache, tile_index, origins, motion_map_px, taps, floor, *args, **kwargs):
        shift = None
        if self.belief is not None:
            now = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
            if tile_index is not None:
                now = now[np.asarray(tile_index, dtype=np.int64)]
            shift = aerial.oxford_track_shift(self.origin, now, motion_map_px)
        res = super().step(model, grd, cache, tile_index, origins, motion_map_px, taps, floor, *args, **kwargs)
        self.log.append((self.belief, shift, taps, floor))
        return res


def smooth_stream(model, log, in_place: bool = False):
    """The backward sweep over a RecordingTracker's log (T entries (belief, shift, taps, floor)) -> (maps, stats): maps a list of T
    tensors [B,512,512], maps[t] = p(x_t | frames 1..T); stats [T,B,4] (SMOOTH_FIELDS).  The last frame's map is its own belief, and
    its stats row comes from a call against a zero next map (the rule of a future that says nothing: its argmax, NaN, 0).  Frame t
    takes entry t + 1's shift, taps and floor.  in_place: the sweep runs in one running buffer (out=smoothed_next) and each frame's
    map is copied out of it; the bits are the same.  A zero belief in the log (a frame without a finite posterior) needs no special
    case here: the rules of track_smooth restart the sweep behind it."""
    return _sweep(model, log, in_place, lambda *a, **kw: track_smooth(*a, **kw), lambda B: [[0.0, 0.0]] * B, "shift")


def _sweep(model, log, in_place: bool, step, still, what: str):
    """The backward sweep of smooth_stream and smooth_stream_affine over T entries (belief, motion, taps, floor).  step: the backward
    step of the log's tracker (track_smooth's signature); still(B): the motion that moves nothing, for the last frame's call against
    a zero next map; what: the motion's name in the refusal of an entry without one."""
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    last = log[-1][0]
    B = last.shape[0]
    maps, stats = [None] * T, [None] * T
    _, stats[-1] = step(model, last, torch.zeros_like(last), still(B), [1.0], 0.0)
    maps[-1] = last
    run = last.clone() if in_place else last
    for t in range(T - 2, -1, -1):
        _, motion, taps, floor = log[t + 1]
        if motion is None:
            raise ValueError(f"log entry {t + 1} has no {what}: a stream's first frame can only stand first")
        if in_place:
            _, stats[t] = step(model, log[t][0], run, motion, taps, floor, out=run)
            maps[t] = run.clone()
        else:
            run, stats[t] = step(model, log[t][0], run, motion, taps, floor)
            maps[t] = run
    return maps, torch.stack(stats)


class RecordingAffineTracker(aerial.AffineTracker):
    """aerial.AffineTracker that keeps what a backward sweep needs, as RecordingTracker does for aerial.Tracker: step() is the parent's
    - the same arguments, the same returns, the same rows and beliefs bit for bit - and appends (belief, matrix, taps, floor) to
    self.log: the posterior the step stored and the arguments of the model.track_predict_affine call that led into this frame (matrix
    None for the first frame of a stream, which has no such call).  A host matrix is kept as a float64 copy, a device tensor as it is;
    the beliefs are the tensors the update returned.  reset() clears the log."""

    def __init__(self):
        super().__init__()
        self.log = []

    def reset(self) -> None:
        super().reset()
        self.log = []

    def step(self, model, grd, sat, matrix, taps, floor, *args, **kwargs):
        kept = None
        if self.belief is not None:
            on_device = isinstance(matrix, torch.Tensor) and matrix.device.type != "cpu"
            kept = matrix if on_device else np.array(matrix, dtype=np.float64)
        res = super().step(model, grd, sat, matrix, taps, floor, *args, **kwargs)
        self.log.append((self.belief, kept, taps, floor))
        return res


def smooth_stream_affine(model, log, in_place: bool = False):
    """smooth_stream over a RecordingAffineTracker's log (T entries (belief, matrix, taps, floor)): frame t takes entry t + 1's matrix,
    taps and floor through track_smooth_affine; the last frame's stats row comes from a call with a zero next map and the identity
    matrix.  A link beyond the smoother's reach is refused when its matrix is host data, and is a broken link (the sweep restarts
    behind it) when it is a device tensor."""
    return _sweep(model, log, in_place, lambda *a, **kw: track_smooth_affine(*a, **kw), lambda B: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], "matrix")


# ---- the joint position-heading filter's backward half ---------------------------------------------------------------

class _JointSmoothResults:
    """track_joint_smooth's results behind models._Layout's interface: the work buffer as the last pointer before the results (torch's
    allocator keeps its memory for this stream's launches after the tensor is dropped), then smoothed - `out` when the caller gave one
    -, marginal, hist and stats."""

    def __init__(self, nb: int, out):
        self.nb, self.out = nb, out

    def alloc(self, B: int, dev):
        nb = self.nb
        work = torch.empty(_lib.load().ccvpe_track_joint_smooth_work_bytes(B, nb), dtype=torch.uint8, device=dev)
        smoothed = self.out if self.out is not None else torch.empty((B, nb) + spec.OUT_HW, dtype=torch.float32, device=dev)
        marginal = torch.empty((B,) + spec.OUT_HW, dtype=torch.float32, device=dev)
        hist = torch.empty((B, nb), dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(JOINT_SMOOTH_FIELDS)), dtype=torch.float32, device=dev)
        res = [smoothed, marginal, hist, stats]
        return res, [work.data_ptr()] + [t.data_ptr() for t in res]


def track_joint_smooth(model, joint, smoothed_next, shift_px, taps, floor, turn_deg, heading_taps, out=None):
    """One backward step of the joint filter: (smoothed [B,nb,512,512], marginal [B,512,512], hist [B,nb], stats [B,5]) of frame t from
    joint [B,nb,512,512], the filter joint of frame t (track_joint_update_logits' joint), smoothed_next, the smoothed joint of frame
    t + 1 (for the last frame but one: the last frame's joint), and shift_px, taps, floor, turn_deg, heading_taps, the arguments of
    the model.track_joint_predict call that carried joint into frame t + 1 - checked as that method checks them and in its order,
    smoothed_next like joint and directly after it.  stats: JOINT_SMOOTH_FIELDS.  A next joint without a positive value says nothing:
    smoothed is joint bit for bit and stats (its marginal's argmax, the value, the best bin, NaN, 0); a joint the recursion cannot
    weigh (all zero, a NaN) gives zeros and (-1, NaN, -1, Z, G).  out: the tensor that receives the smoothed joint (same shape,
    float32, contiguous, on joint's device), not the joint; out=smoothed_next is the in-place form of a backward sweep, with the bits
    of the out-of-place call.  Five launches (ccvpe_track_joint_smooth, include/ccvpe.h: the definition, the rules, the error bound);
    the work buffer - one more joint - is allocated here, per call."""
    model._require_eval()
    B, nb = model._joint_maps(joint, "joint")
    model._joint_maps(smoothed_next, "smoothed_next", nb, B)
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    hshape = tuple(heading_taps.shape) if isinstance(heading_taps, (torch.Tensor, np.ndarray)) else np.shape(heading_taps)
    if len(hshape) not in (1, 2) or hshape[-1] < 1 or (len(hshape) == 2 and hshape[0] != B):
        raise ValueError(f"heading_taps must be [rh+1] or [{B}, rh+1], got {tuple(hshape)}")
    rh = int(hshape[-1]) - 1
    if rh > 32 or 2 * rh + 1 > nb:
        raise ValueError(f"heading_taps give radius {rh}, must be in 0..32 with 2 radius + 1 <= nb = {nb}")
    if out is not None:
        model._joint_maps(out, "out", nb, B)
        if out.data_ptr() == joint.data_ptr():
            raise ValueError("out must not be the joint")
    if smoothed_next.data_ptr() == joint.data_ptr():
        raise ValueError("smoothed_next must not be the joint")
    dev = joint.device
    sh = model._track_vec(shift_px, "shift_px", (B, nb, 2), dev)
    tp = model._track_vec(taps, "taps", tshape, dev)
    ht = model._track_vec(heading_taps, "heading_taps", hshape, dev)
    tn = model._per_query(turn_deg, np.ndim(turn_deg) == 0 and not isinstance(turn_deg, torch.Tensor), "turn_deg", B, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    if not joint.is_cuda:
        raise ValueError(f"joint must be a cuda tensor, not a {joint.device.type} tensor")
    if smoothed_next.device != dev:
        raise ValueError(f"smoothed_next is on {smoothed_next.device}, joint on {dev}")
    if out is not None and out.device != dev:
        raise ValueError(f"out is on {out.device}, joint on {dev}")
    model._ensure_handle(dev)
    return model._launch("track_joint_smooth", dev, B,
                         (joint, smoothed_next, B, nb, sh, tp, stride, radius, tn, ht, (rh + 1) if len(hshape) == 2 else 0, rh, fl),
                         _JointSmoothResults(nb, out))


class RecordingJointTracker(aerial.JointTracker):
    """aerial.JointTracker that keeps what a backward sweep needs: step() is the parent's - the same arguments, the same returns, the
    same rows and joints bit for bit - and appends (joint, table, taps, floor, turn_deg, heading_taps) to self.log, one entry per
    frame: the joint the step stored and the arguments of the model.track_joint_predict call that led into this frame (table, the
    shift table [B,nb,2] recomputed with the parent's own calls; None for the first frame of a stream, which has no such call).  The
    joints are the tensors the update returned, not copies: every call into the library allocates its results anew, so nothing writes
    to them again.  Memory: a stored joint is 1 MB per stream and heading bin, so a log of T frames holds T * B * nb MB on the device
    (T = 100, B = 1, nb = 36: 3.6 GB).  reset() clears the log."""

    def __init__(self):
        super().__init__()
        self.log = []

    def reset(self) -> None:
        super().reset()
        self.log = []

    def step(self, model, grd, emission, forward_px, left_px, turn_deg, taps, heading_taps, floor, cache=None, tile_index=None, sat=None,
             origins=None, zero_deg: float = 0.0, clockwise: bool = False, summary_radius=None, credible_levels=None):
        had, before = self.joint is not None, self.origin
        res = super().step(model, grd, emission, forward_px, left_px, turn_deg, taps, heading_taps, floor, cache=cache, tile_index=tile_index,
                           sat=sat, origins=origins, zero_deg=zero_deg, clockwise=clockwise, summary_radius=summary_radius,
                           credible_levels=credible_levels)
        table = None
        if had:
            # the table the parent's predict just got, by the parent's own calls (self.origin is this frame's window now)
            B, nb = self.joint.shape[:2]
            common = None if self.origin is None else aerial.oxford_track_shift(before, self.origin, np.zeros(2))
            table = np.broadcast_to(aerial.joint_shift_table(forward_px, left_px, nb, zero_deg, clockwise, common), (B, nb, 2)).copy()
        self.log.append((self.joint, table, taps, floor, turn_deg, heading_taps))
        return res


def smooth_joint_stream(model, log, in_place: bool = False, keep_joint: bool = False):
    """The backward sweep over a RecordingJointTracker's log (T entries (joint, table, taps, floor, turn_deg, heading_taps)) ->
    (marginals [T,B,512,512], hists [T,B,nb], stats [T,B,5] (JOINT_SMOOTH_FIELDS)); with keep_joint a list of the T smoothed joints
    [B,nb,512,512] is appended (T * B * nb MB more).  marginals[t] = p(cell | frames 1..T), hists[t] = p(heading bin | frames 1..T).
    The last frame goes through a call with a zero next joint - the rule of a future that says nothing: its own joint, marginal, hist
    and argmax, NaN, 0.  Frame t takes entry t + 1's motion.  in_place: the sweep runs in one running buffer (out=smoothed_next); the
    bits are the same.  A zero joint in the log (a frame without a finite posterior) needs no special case here: the rules of
    track_joint_smooth restart the sweep behind it."""
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    last = log[-1][0]
    B, nb = last.shape[:2]
    run = torch.zeros_like(last)
    marginals, hists, stats, joints = [None] * T, [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            motion = (np.zeros((B, nb, 2)), [1.0], 0.0, 0.0, [1.0])
        else:
            motion = log[t + 1][1:]
            if motion[0] is None:
                raise ValueError(f"log entry {t + 1} has no shift table: a stream's first frame can only stand first")
        table, taps, floor, turn_deg, heading_taps = motion
        if in_place:
            _, marginals[t], hists[t], stats[t] = track_joint_smooth(model, log[t][0], run, table, taps, floor, turn_deg, heading_taps, out=run)
            if keep_joint:
                joints[t] = run.clone()
        else:
            run, marginals[t], hists[t], stats[t] = track_joint_smooth(model, log[t][0], run, table, taps, floor, turn_deg, heading_taps)
            joints[t] = run if keep_joint else None
    res = (torch.stack(marginals), torch.stack(hists), torch.stack(stats))
    return res + (joints,) if keep_joint else res
