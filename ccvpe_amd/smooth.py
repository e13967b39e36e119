"""Smoothing a tracked stream: the backward half of the histogram filter of aerial.Tracker.

The filter answers p(x_t | frames 1..t).  An offline user - re-evaluating a traverse, building a map, labelling a calibration study -
wants p(x_t | frames 1..T), with the later frames counted in: the filter is weakest at the start of a stream and after every restart,
where it has no prior yet and a distractor wins.

    tracker = smooth.RecordingTracker()
    for frame in stream:
        rows = tracker.step(model, grd, cache, tile_index, origins, motion_map_px, taps, floor)
    maps, stats = smooth.smooth_stream(model, tracker.log)      # maps[t] [B,512,512], stats [T,B,4] (SMOOTH_FIELDS)

track_smooth is one backward step (ccvpe_track_smooth, include/ccvpe.h: the definition, the degenerate rules, the error bound).  Out
of scope: aerial.AffineTracker (the adjoint of a bilinear gather through a matrix is a scatter, not a predict call with the inverse
matrix), the heading belief (hist is not smoothed), the MAP trajectory, pose rows with orientation at the smoothed cell.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, aerial, spec

# columns of stats: the first index of the largest smoothed cell, the map's value there, Z = sum_i belief_i a_i - the evidence the
# later frames give this belief, sum s' (about 1) when the belief has mass 1 - and G = sum_i s'_i / prior_i, the future's total weight
SMOOTH_FIELDS = ("index", "prob", "evidence", "future")


class _SmoothResults:
    """track_smooth's results behind models._Layout's interface: the smoothed map - `out` when the caller gave one - and stats, then the
    work buffer as the last pointer before the stream (torch's allocator keeps its memory for this stream's launches after the tensor
    is dropped)."""

    def __init__(self, out):
        self.out = out

    def alloc(self, B: int, dev):
        smoothed = self.out if self.out is not None else torch.empty((B,) + spec.OUT_HW, dtype=torch.float32, device=dev)
        stats = torch.empty((B, len(SMOOTH_FIELDS)), dtype=torch.float32, device=dev)
        work = torch.empty(_lib.load().ccvpe_track_smooth_work_bytes(B), dtype=torch.uint8, device=dev)
        return [smoothed, stats], [smoothed.data_ptr(), stats.data_ptr(), work.data_ptr()]


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
    if not belief.is_cuda:
        raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
    if smoothed_next.device != dev:
        raise ValueError(f"smoothed_next is on {smoothed_next.device}, belief on {dev}")
    if out is not None:
        if model._stored_maps(out, "out") != B or out.device != dev:
            raise ValueError(f"out must hold {B} maps on {dev}")
        if out.data_ptr() == belief.data_ptr():
            raise ValueError("out must not be belief")
    model._ensure_handle(dev)
    return model._launch("track_smooth", dev, B, (belief, smoothed_next, B, sh, tp, stride, radius, fl), _SmoothResults(out))


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
    T = len(log)
    if T == 0:
        raise ValueError("the log is empty")
    last = log[-1][0]
    B = last.shape[0]
    maps, stats = [None] * T, [None] * T
    _, stats[-1] = track_smooth(model, last, torch.zeros_like(last), [[0.0, 0.0]] * B, [1.0], 0.0)
    maps[-1] = last
    run = last.clone() if in_place else last
    for t in range(T - 2, -1, -1):
        _, shift, taps, floor = log[t + 1]
        if shift is None:
            raise ValueError(f"log entry {t + 1} has no shift: a stream's first frame can only stand first")
        if in_place:
            _, stats[t] = track_smooth(model, log[t][0], run, shift, taps, floor, out=run)
            maps[t] = run.clone()
        else:
            run, stats[t] = track_smooth(model, log[t][0], run, shift, taps, floor)
            maps[t] = run
    return maps, torch.stack(stats)
