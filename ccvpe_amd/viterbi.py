"""The MAP trajectory of a tracked stream: the one most probable sequence of cells under the histogram filter of
aerial.Tracker.

The filter gives p(x_t | frames 1..t), smooth.smooth_stream p(x_t | frames 1..T); the argmaxes of T marginals are not a path - with
two plausible modes consecutive argmaxes can sit hundreds of pixels apart.  The path maximises over cells and link kinds jointly:
every link is a move under the filter's motion kernel or a jump under its relocalisation floor, and the links' kinds are part of the
result.

    tracker = smooth.RecordingTracker()
    for frame in stream:
        rows = tracker.step(model, grd, cache, tile_index, origins, motion_map_px, taps, floor)
    cells, links, stats, scores = viterbi.map_path(model, tracker.log)      # cells, links [T,B] int32; stats [T,B,4] (VITERBI_FIELDS)

track_viterbi is one step of the forward sweep and track_viterbi_back one link of the backtrack (ccvpe_track_viterbi,
ccvpe_track_viterbi_back, include/ccvpe.h: the definition, the restart and degenerate rules, the error bounds).

Streams of aerial.AffineTracker - frames that turn or change scale, KITTI's heading-up tiles - have the same three pieces (DESIGN.md
4.24): map_path_affine over a smooth.RecordingAffineTracker's log, track_viterbi_affine and track_viterbi_back_affine
(ccvpe_track_viterbi_affine, ccvpe_track_viterbi_back_affine).  The maximum over the exact transition - a sum over the samples that
touch a cell - is not separable; the affine move is read as one more latent choice instead, of the sample position the blur reads and
of the one of its four bilinear taps that carried the mass.  That link weight T_aug satisfies T_aug <= T <= N T_aug with N =
ceil(2 hx) ceil(2 hy) of smooth.affine_reach (9 for a rotation at scale 1; the largest ratio seen is 3.9), and T_aug = T at integer
translations: the path is the MAP path of a model whose moves are weighed at most N times lighter against the floor than the
filter's, and it never takes a link the filter rules out.

Streams of aerial.JointTracker - the filter over (heading bin, cell) - have the same three pieces: map_joint_path
over a smooth.RecordingJointTracker's log, track_joint_viterbi and track_joint_viterbi_back (ccvpe_track_joint_viterbi,
ccvpe_track_joint_viterbi_back).  The path is a sequence of (cell, heading bin) pairs - a full (x, y, heading) track - and a link
is one more latent choice: which of the 2 rh + 2 merged circle weights carried the mass from which source bin, then the window
position under that bin's own shift, or a jump through the floor to any state.  The heading is part of the path, so consecutive
frames never pair a cell with a heading no single hypothesis held, which the smoothed marginal's argmax and "the best bin there" can.

    tracker = smooth.RecordingJointTracker()
    ...
    cells, bins, links, stats, scores = viterbi.map_joint_path(model, tracker.log)    # stats [T,B,5] (JOINT_VITERBI_FIELDS)

Out of scope: the exact (summed-over-samples) transition as the link weight, the sample position of a link, joint streams across
turning frames, link statistics of joint streams, recomputing scores instead of storing them, fusing the scale launch into the next
step.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, smooth, spec

# columns of stats: the first index of the largest score, the score there (in [1, 2)), the exponent e the frame's products were scaled
# by (w = score * 2^e), and 1 where the frame starts a segment (a stream's first frame, a frame behind one without a finite posterior)
VITERBI_FIELDS = ("index", "peak", "exponent", "restarted")
LINK_MOVE, LINK_JUMP, LINK_START = 0, 1, 2


class _ViterbiResults:
    """track_viterbi's results behind models._Layout's interface: the score map - `out` when the caller gave one - and stats, then the
    work buffer as the last pointer before the stream."""

    def __init__(self, out):
        self.out = out

    def alloc(self, B: int, dev):
        score = self.out if self.out is not None else torch.empty((B,) + spec.OUT_HW, dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(VITERBI_FIELDS)), dtype=torch.float32, device=dev)
        work = torch.empty(_lib.load().ccvpe_track_viterbi_work_bytes(B), dtype=torch.uint8, device=dev)
        return [score, stats], [score.data_ptr(), stats.data_ptr(), work.data_ptr()]


class _BackResults:
    def alloc(self, B: int, dev):
        back = torch.empty((B, 2), dtype=torch.int32, device=dev)
        return [back], [back.data_ptr()]


def _prev_stats(prev_stats, B: int):
    if not isinstance(prev_stats, torch.Tensor) or tuple(prev_stats.shape) != (B, len(VITERBI_FIELDS)) or prev_stats.dtype != torch.float32:
        raise ValueError(f"prev_stats must be a float32 tensor [{B}, 4]: the stats of the call that made score_prev")
    return prev_stats.detach().contiguous()


def _same_device(dev, ref: str, **tensors) -> None:
    for name, t in tensors.items():
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {ref} on {dev}")


def _check_out(model, out, B: int, dev, maps) -> None:
    """the out tensor of a step: the last check of track_viterbi and track_viterbi_affine"""
    if out is not None:
        if model._stored_maps(out, "out") != B or out.device != dev:
            raise ValueError(f"out must hold {B} maps on {dev}")
        if any(t is not None and out.data_ptr() == t.data_ptr() for t in maps):
            raise ValueError("out must be none of the input maps: the step reads their halos")


def track_viterbi(model, belief, belief_prev=None, score_prev=None, prev_stats=None, shift_px=None, taps=None, floor=None, out=None):
    """One step of the forward sweep: (score [B,512,512], stats [B,4]) of frame t from belief [B,512,512], the filter posterior of frame
    t (track_update's map), belief_prev, that of frame t - 1, score_prev and prev_stats, this function's results for frame t - 1, and
    shift_px, taps, floor, the arguments of the model.track_predict call that carried belief_prev into frame t - checked as that method
    checks them and in its order, belief_prev and score_prev like belief and directly after it.  belief alone: the first frame of a
    stream, score is belief (cells that are not > 0 as 0) scaled to a peak in [1, 2).  stats: VITERBI_FIELDS.  A frame behind one
    without a positive score restarts (restarted = 1, score the frame's likelihood); a frame whose largest product is not positive and
    finite gives a zero map and (-1, NaN, NaN, restarted).  out: the tensor that receives the score map; it must be none of the input
    maps.  Two launches; the work buffer is allocated here, per call."""
    model._require_eval()
    B = model._stored_maps(belief)
    given = [a is not None for a in (belief_prev, score_prev, prev_stats, shift_px)]
    if any(given) and not all(given):
        raise ValueError("belief_prev, score_prev, prev_stats and shift_px go together: all of them, or none for a stream's first frame")
    first = not any(given)
    dev = belief.device
    if first:
        cargs = (belief, None, None, None, B, None, None, 0, 0, None)
    else:
        for name, t in (("belief_prev", belief_prev), ("score_prev", score_prev)):
            if model._stored_maps(t, name) != B:
                raise ValueError(f"{name} holds {t.shape[0]} maps, belief {B}")
        ps = _prev_stats(prev_stats, B)
        if taps is None or floor is None:
            raise ValueError("taps and floor of the predict call are needed behind a stream's first frame")
        tshape, stride, radius, number = model._blur_checks(taps, floor, B)
        sh = model._track_vec(shift_px, "shift_px", (B, 2), dev)
        tp = model._track_vec(taps, "taps", tshape, dev)
        fl = model._per_query(floor, number, "floor", B, dev)
        cargs = (belief, belief_prev, score_prev, ps, B, sh, tp, stride, radius, fl)
    if not belief.is_cuda:
        raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
    if not first:
        _same_device(dev, "belief", belief_prev=belief_prev, score_prev=score_prev, prev_stats=ps)
    _check_out(model, out, B, dev, (belief, belief_prev, score_prev))
    model._ensure_handle(dev)
    return model._launch("track_viterbi", dev, B, cargs, _ViterbiResults(out))


def track_viterbi_back(model, score_prev, prev_stats, cell, shift_px, taps, floor):
    """One link of the backtrack: back [B,2] int32 = (previous cell, kind) from score_prev and prev_stats, track_viterbi's results for
    frame t - 1, cell [B] int32 on their device, the path's cell at frame t, and the arguments of the model.track_predict call between
    the two frames.  kind: LINK_MOVE (the best of the cell's window of source cells), LINK_JUMP (the frame's argmax, through the floor)
    or LINK_START (cell outside the grid: the previous frame's argmax, or -1 where it has none - the end of a backtrack or the frame
    behind a broken one).  One launch; nothing synchronises."""
    model._require_eval()
    B = model._stored_maps(score_prev, "score_prev")
    ps = _prev_stats(prev_stats, B)
    if not isinstance(cell, torch.Tensor) or tuple(cell.shape) != (B,) or cell.dtype != torch.int32:
        raise ValueError(f"cell must be an int32 tensor [{B}]")
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    dev = score_prev.device
    sh = model._track_vec(shift_px, "shift_px", (B, 2), dev)
    tp = model._track_vec(taps, "taps", tshape, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    if not score_prev.is_cuda:
        raise ValueError(f"score_prev must be a cuda tensor, not a {score_prev.device.type} tensor")
    _same_device(dev, "score_prev", prev_stats=ps, cell=cell)
    model._ensure_handle(dev)
    return model._launch("track_viterbi_back", dev, B, (score_prev, ps, cell.contiguous(), B, sh, tp, stride, radius, fl), _BackResults())


def map_path(model, log):
    """The MAP trajectory over a smooth.RecordingTracker's log (T entries (belief, shift, taps, floor)) -> (cells [T,B] int32, links
    [T,B] int32, stats [T,B,4], scores): cells[t] the path's cell at frame t (-1 for a frame without a finite posterior), links[t] the
    kind of the link from frame t - 1 into frame t (links[0] = LINK_START), stats and scores (a list of T maps [B,512,512]) the
    forward sweep's.  T track_viterbi calls, frame t with entry t - 1's belief and entry t's shift, taps and floor; then T - 1
    track_viterbi_back calls from the last frame back.  The last frame's cell is its own argmax, stats[T - 1]'s index - a cell of -1
    there starts the backtrack one frame earlier, as behind any broken frame.  Indices stay on the device and nothing synchronises.  A
    zero belief in the log needs no special case: the rules of the two calls end one segment and start the next."""
    return _sweep(model, log, lambda *a: track_viterbi(*a), lambda *a: track_viterbi_back(*a), "shift")


def _sweep(model, log, step, back_step, what: str):
    """The forward sweep and the backtrack of map_path and map_path_affine over T entries (belief, motion, taps, floor).  step,
    back_step: the two calls of the log's tracker (track_viterbi's and track_viterbi_back's signatures); what: the motion's name in the
    refusal of an entry without one."""
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    scores, stats = [None] * T, [None] * T
    scores[0], stats[0] = step(model, log[0][0])
    for t in range(1, T):
        belief, motion, taps, floor = log[t]
        if motion is None:
            raise ValueError(f"log entry {t} has no {what}: a stream's first frame can only stand first")
        scores[t], stats[t] = step(model, belief, log[t - 1][0], scores[t - 1], stats[t - 1], motion, taps, floor)
    cells, links = [None] * T, [None] * T
    cells[-1] = stats[-1][:, 0].to(torch.int32)
    for t in range(T - 1, 0, -1):
        _, motion, taps, floor = log[t]
        back = back_step(model, scores[t - 1], stats[t - 1], cells[t], motion, taps, floor)
        cells[t - 1], links[t] = back[:, 0].contiguous(), back[:, 1]
    links[0] = torch.full_like(cells[0], LINK_START)
    return torch.stack(cells), torch.stack(links), torch.stack(stats), scores


def track_viterbi_affine(model, belief, belief_prev=None, score_prev=None, prev_stats=None, matrix=None, taps=None, floor=None, out=None):
    """track_viterbi for a link made by model.track_predict_affine: matrix ([B,6] or [6]), taps, floor are that call's arguments, checked
    as that method checks them and in its order - host data must be finite, a float64 tensor on the belief's device is not looked at -
    behind belief_prev, score_prev and prev_stats; everything else - the results, stats, the first-frame form (belief alone), the
    restart and degenerate rules, out - is track_viterbi's (ccvpe_track_viterbi_affine, include/ccvpe.h: the definition, the error
    bound).  No matrix is refused for its reach: the recursion only gathers, and a matrix that is singular or moves everything off the
    grid leaves the floor as the only link.  Two launches; the work buffer is allocated here, per call."""
    model._require_eval()
    B = model._stored_maps(belief)
    given = [a is not None for a in (belief_prev, score_prev, prev_stats, matrix)]
    if any(given) and not all(given):
        raise ValueError("belief_prev, score_prev, prev_stats and matrix go together: all of them, or none for a stream's first frame")
    first = not any(given)
    dev = belief.device
    if first:
        cargs = (belief, None, None, None, B, None, None, 0, 0, None)
    else:
        for name, t in (("belief_prev", belief_prev), ("score_prev", score_prev)):
            if model._stored_maps(t, name) != B:
                raise ValueError(f"{name} holds {t.shape[0]} maps, belief {B}")
        ps = _prev_stats(prev_stats, B)
        if taps is None or floor is None:
            raise ValueError("taps and floor of the predict call are needed behind a stream's first frame")
        mt, on_device = smooth._matrix_checked(matrix, B)
        tshape, stride, radius, number = model._blur_checks(taps, floor, B)
        tp = model._track_vec(taps, "taps", tshape, dev)
        fl = model._per_query(floor, number, "floor", B, dev)
    if not belief.is_cuda:
        raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
    if not first:
        _same_device(dev, "belief", belief_prev=belief_prev, score_prev=score_prev, prev_stats=ps)
        cargs = (belief, belief_prev, score_prev, ps, B, smooth._matrix_placed(mt, on_device, B, dev), tp, stride, radius, fl)
    _check_out(model, out, B, dev, (belief, belief_prev, score_prev))
    model._ensure_handle(dev)
    return model._launch("track_viterbi_affine", dev, B, cargs, _ViterbiResults(out))


def track_viterbi_back_affine(model, score_prev, prev_stats, cell, matrix, taps, floor):
    """track_viterbi_back for a link made by model.track_predict_affine: back [B,2] int32 = (previous cell, kind), the arguments and the
    kinds track_viterbi_back's with that call's matrix for its shift, checked as in track_viterbi_affine.  A MOVE's candidates are the
    4 (2 radius + 1)^2 pairs of a sample position in the cell's window and one of its four taps; the largest wins, the smallest
    source cell on ties.  One launch; nothing synchronises."""
    model._require_eval()
    B = model._stored_maps(score_prev, "score_prev")
    ps = _prev_stats(prev_stats, B)
    if not isinstance(cell, torch.Tensor) or tuple(cell.shape) != (B,) or cell.dtype != torch.int32:
        raise ValueError(f"cell must be an int32 tensor [{B}]")
    mt, on_device = smooth._matrix_checked(matrix, B)
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    dev = score_prev.device
    tp = model._track_vec(taps, "taps", tshape, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    if not score_prev.is_cuda:
        raise ValueError(f"score_prev must be a cuda tensor, not a {score_prev.device.type} tensor")
    _same_device(dev, "score_prev", prev_stats=ps, cell=cell)
    mt = smooth._matrix_placed(mt, on_device, B, dev, "score_prev")
    model._ensure_handle(dev)
    return model._launch("track_viterbi_back_affine", dev, B, (score_prev, ps, cell.contiguous(), B, mt, tp, stride, radius, fl), _BackResults())


def map_path_affine(model, log):
    """map_path over a smooth.RecordingAffineTracker's log (T entries (belief, matrix, taps, floor)): the same return tuple and rules,
    frame t through track_viterbi_affine with entry t - 1's belief and entry t's matrix, taps and floor, the links through
    track_viterbi_back_affine."""
    return _sweep(model, log, lambda *a: track_viterbi_affine(*a), lambda *a: track_viterbi_back_affine(*a), "matrix")


# ---- the joint position-heading filter's MAP trajectory ---------------------------------------------------------------

# columns of a joint step's stats: the cell and the heading bin of the first flat index (bin * 512 * 512 + cell) of the largest score -
# two columns, the flat index does not fit a float32 -, the score there (in [1, 2)), the exponent e the frame's products were scaled by
# (one per query, not per bin) and 1 where the frame starts a segment
JOINT_VITERBI_FIELDS = ("index", "bin", "peak", "exponent", "restarted")


class _JointViterbiResults:
    """track_joint_viterbi's results behind models._Layout's interface: the work buffer as the last pointer before the results (as
    smooth._JointSmoothResults), then the score joint - `out` when the caller gave one - and stats."""

    def __init__(self, nb: int, out):
        self.nb, self.out = nb, out

    def alloc(self, B: int, dev):
        nb = self.nb
        work = torch.empty(_lib.load().ccvpe_track_joint_viterbi_work_bytes(B, nb), dtype=torch.uint8, device=dev)
        score = self.out if self.out is not None else torch.empty((B, nb) + spec.OUT_HW, dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(JOINT_VITERBI_FIELDS)), dtype=torch.float32, device=dev)
        return [score, stats], [work.data_ptr(), score.data_ptr(), stats.data_ptr()]


class _JointBackResults:
    def alloc(self, B: int, dev):
        back = torch.empty((B, 3), dtype=torch.int32, device=dev)
        return [back], [back.data_ptr()]


def _joint_prev_stats(prev_stats, B: int):
    if not isinstance(prev_stats, torch.Tensor) or tuple(prev_stats.shape) != (B, len(JOINT_VITERBI_FIELDS)) or prev_stats.dtype != torch.float32:
        raise ValueError(f"prev_stats must be a float32 tensor [{B}, 5]: the stats of the call that made score_prev")
    return prev_stats.detach().contiguous()


def _joint_motion(model, B: int, nb: int, dev, shift_px, taps, floor, turn_deg, heading_taps):
    """The arguments of a model.track_joint_predict call, checked as smooth.track_joint_smooth checks them and in its order -> the C
    arguments from shift to floor."""
    tshape, stride, radius, number = model._blur_checks(taps, floor, B)
    hshape = tuple(heading_taps.shape) if isinstance(heading_taps, (torch.Tensor, np.ndarray)) else np.shape(heading_taps)
    if len(hshape) not in (1, 2) or hshape[-1] < 1 or (len(hshape) == 2 and hshape[0] != B):
        raise ValueError(f"heading_taps must be [rh+1] or [{B}, rh+1], got {tuple(hshape)}")
    rh = int(hshape[-1]) - 1
    if rh > 32 or 2 * rh + 1 > nb:
        raise ValueError(f"heading_taps give radius {rh}, must be in 0..32 with 2 radius + 1 <= nb = {nb}")
    sh = model._track_vec(shift_px, "shift_px", (B, nb, 2), dev)
    tp = model._track_vec(taps, "taps", tshape, dev)
    ht = model._track_vec(heading_taps, "heading_taps", hshape, dev)
    tn = model._per_query(turn_deg, np.ndim(turn_deg) == 0 and not isinstance(turn_deg, torch.Tensor), "turn_deg", B, dev)
    fl = model._per_query(floor, number, "floor", B, dev)
    return (sh, tp, stride, radius, tn, ht, (rh + 1) if len(hshape) == 2 else 0, rh, fl)


def track_joint_viterbi(model, joint, joint_prev=None, score_prev=None, prev_stats=None, shift_px=None, taps=None, floor=None, turn_deg=None,
                        heading_taps=None, out=None):
    """One step of the joint forward sweep: (score [B,nb,512,512], stats [B,5]) of frame t from joint [B,nb,512,512], the filter joint of
    frame t (track_joint_update_logits' joint), joint_prev, that of frame t - 1, score_prev and prev_stats, this function's results for
    frame t - 1, and shift_px [B,nb,2], taps, floor, turn_deg, heading_taps, the arguments of the model.track_joint_predict call that
    carried joint_prev into frame t - checked as smooth.track_joint_smooth checks them and in its order, joint_prev and score_prev like
    joint and directly after it.  joint alone: the first frame of a stream, score is joint (values that are not > 0 as 0) scaled to a
    peak in [1, 2).  stats: JOINT_VITERBI_FIELDS.  A frame behind one without a positive score restarts (restarted = 1, score the
    frame's likelihood); a frame whose largest product is not positive and finite gives a zero joint and (-1, -1, NaN, NaN,
    restarted).  out: the tensor that receives the score joint; it must be none of the input joints.  Four launches, two for a first
    frame (ccvpe_track_joint_viterbi, include/ccvpe.h: the definition, the rules, the error bound); the work buffer - two more joints
    - is allocated here, per call."""
    model._require_eval()
    B, nb = model._joint_maps(joint, "joint")
    given = [a is not None for a in (joint_prev, score_prev, prev_stats, shift_px)]
    if any(given) and not all(given):
        raise ValueError("joint_prev, score_prev, prev_stats and shift_px go together: all of them, or none for a stream's first frame")
    first = not any(given)
    dev = joint.device
    if first:
        cargs = (joint, None, None, None, B, nb, None, None, 0, 0, None, None, 0, 0, None)
    else:
        model._joint_maps(joint_prev, "joint_prev", nb, B)
        model._joint_maps(score_prev, "score_prev", nb, B)
        ps = _joint_prev_stats(prev_stats, B)
        if taps is None or floor is None or turn_deg is None or heading_taps is None:
            raise ValueError("taps, floor, turn_deg and heading_taps of the predict call are needed behind a stream's first frame")
        cargs = (joint, joint_prev, score_prev, ps, B, nb) + _joint_motion(model, B, nb, dev, shift_px, taps, floor, turn_deg, heading_taps)
    if out is not None:
        model._joint_maps(out, "out", nb, B)
        if any(t is not None and out.data_ptr() == t.data_ptr() for t in (joint, joint_prev, score_prev)):
            raise ValueError("out must be none of the input joints: the step reads their halos")
    if not joint.is_cuda:
        raise ValueError(f"joint must be a cuda tensor, not a {joint.device.type} tensor")
    if not first:
        _same_device(dev, "joint", joint_prev=joint_prev, score_prev=score_prev, prev_stats=ps)
    if out is not None and out.device != dev:
        raise ValueError(f"out is on {out.device}, joint on {dev}")
    model._ensure_handle(dev)
    return model._launch("track_joint_viterbi", dev, B, cargs, _JointViterbiResults(nb, out))


def track_joint_viterbi_back(model, score_prev, prev_stats, cell, bin, shift_px, taps, floor, turn_deg, heading_taps):
    """One link of the joint backtrack: back [B,3] int32 = (previous cell, previous bin, kind) from score_prev and prev_stats,
    track_joint_viterbi's results for frame t - 1, cell and bin [B] int32 on their device, the path's pair at frame t, and the
    arguments of the model.track_joint_predict call between the two frames.  kind: LINK_MOVE (the best of the pair's candidates: a
    source bin within the circle weights' reach and a cell of the window under that bin's shift; the smallest bin * 512 * 512 + cell on
    ties), LINK_JUMP (the frame's argmax pair, through the floor) or LINK_START (cell or bin outside the grid: the previous frame's
    argmax pair, or (-1, -1) where it has none - the end of a backtrack or the frame behind a broken one).  One launch; nothing
    synchronises."""
    model._require_eval()
    B, nb = model._joint_maps(score_prev, "score_prev")
    ps = _joint_prev_stats(prev_stats, B)
    for name, t in (("cell", cell), ("bin", bin)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B,) or t.dtype != torch.int32:
            raise ValueError(f"{name} must be an int32 tensor [{B}]")
    dev = score_prev.device
    motion = _joint_motion(model, B, nb, dev, shift_px, taps, floor, turn_deg, heading_taps)
    if not score_prev.is_cuda:
        raise ValueError(f"score_prev must be a cuda tensor, not a {score_prev.device.type} tensor")
    _same_device(dev, "score_prev", prev_stats=ps, cell=cell, bin=bin)
    model._ensure_handle(dev)
    return model._launch("track_joint_viterbi_back", dev, B, (score_prev, ps, cell.contiguous(), bin.contiguous(), B, nb) + motion,
                         _JointBackResults())


def map_joint_path(model, log):
    """The MAP trajectory over a smooth.RecordingJointTracker's log (T entries (joint, table, taps, floor, turn_deg, heading_taps)) ->
    (cells [T,B] int32, bins [T,B] int32, links [T,B] int32, stats [T,B,5], scores): (cells[t], bins[t]) the path's cell and heading
    bin at frame t ((-1, -1) for a frame without a finite posterior), links[t] the kind of the link from frame t - 1 into frame t
    (links[0] = LINK_START), stats and scores (a list of T joints [B,nb,512,512]) the forward sweep's.  T track_joint_viterbi calls,
    frame t with entry t - 1's joint and entry t's table, taps, floor, turn_deg and heading_taps; then T - 1 track_joint_viterbi_back
    calls from the last frame back.  The last frame's pair is its own stats' (index, bin).  Indices stay on the device and nothing
    synchronises.  Memory: scores is T more joints, as large as the log itself (T * B * nb MB), and every step's work buffer two more.
    A zero joint in the log needs no special case: the rules of the two calls end one segment and start the next."""
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    for t in range(1, T):
        if log[t][1] is None:
            raise ValueError(f"log entry {t} has no shift table: a stream's first frame can only stand first")
    scores, stats = [None] * T, [None] * T
    scores[0], stats[0] = track_joint_viterbi(model, log[0][0])
    for t in range(1, T):
        joint, table, taps, floor, turn_deg, heading_taps = log[t]
        scores[t], stats[t] = track_joint_viterbi(model, joint, log[t - 1][0], scores[t - 1], stats[t - 1], table, taps, floor, turn_deg, heading_taps)
    cells, bins, links = [None] * T, [None] * T, [None] * T
    cells[-1], bins[-1] = stats[-1][:, 0].to(torch.int32), stats[-1][:, 1].to(torch.int32)
    for t in range(T - 1, 0, -1):
        _, table, taps, floor, turn_deg, heading_taps = log[t]
        back = track_joint_viterbi_back(model, scores[t - 1], stats[t - 1], cells[t], bins[t], table, taps, floor, turn_deg, heading_taps)
        cells[t - 1], bins[t - 1], links[t] = back[:, 0].contiguous(), back[:, 1].contiguous(), back[:, 2]
    links[0] = torch.full_like(cells[0], LINK_START)
    return torch.stack(cells), torch.stack(bins), torch.stack(links), torch.stack(stats), scores
