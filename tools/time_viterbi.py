"""The MAP trajectory of a recorded stream (viterbi.map_path, ccvpe_track_viterbi / ccvpe_track_viterbi_back) against
the same recursion written in torch - what a caller has to do without it - in one process.

    python tools/time_viterbi.py [--frames 100] [--iters 10] [--warmup 2] [--out profiles/time_viterbi.json]

The log is tools/time_smooth.py's synthetic one, so that no network runs: sigma 2 px, radius 6, floor 1e-9, a fractional shift.
Cases: batch 1 and batch 32, --frames frames each.  Two forms, each a whole forward sweep and backtrack that leave every frame's score
map, the cells and the link kinds on the device:

    a  library  viterbi.map_path(model, log)
    b  torch    per frame: the zero-filled bilinear shift and the two conv2d blur passes for the prior, the divide, the two max passes
                as unfold + multiply + max over the 2r + 2 merged weights, the jump, the product, max, frexp and ldexp; per link a
                gather of the cell's (2r + 2)^2 window, multiply, argmax and the comparison with the jump

The torch form is checked first: its step, fed the library's previous score map, must give the library's map to 1e-5 relative on the
first frames (a path score is a product of one factor per frame, so two free-running sweeps drift apart by a rounding per frame); the
share of the free-running torch path's cells and kinds that are the library's is reported.  Every shape is warmed up; then the two forms alternate --iters times per
case (the order rotates), each timed on the host between two device synchronisations; the whole measurement runs twice.  Prints one
JSON line: per case, run and form the median / p99 ms per path, per frame, the library's launches per path, the ratio b / a, and the
library form's compulsory traffic - per query and frame six map passes of 1 MB: b, b-, v- read and w written; w read and v written - as
a rate against the copy rate of tools/ubench_hbm.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_smooth import FLOOR, HBM_COPY_TBPS, MAP_BYTES, RADIUS, SHIFT, SIGMA, synthetic_log, torch_predict_c  # noqa: E402

N = 512 * 512
PAD = 600


def merged(taps, f):
    """the 2r + 2 merged weights of a pass: u[k] = f t[|k - r|] + (1 - f) t[|k - 1 - r|], a tap index above r read as 0"""
    import torch
    z = taps.new_zeros(1)
    full = torch.cat([taps.flip(0)[:-1], taps])          # t[|i|], i = -r .. r
    return f * torch.cat([full, z]) + (1.0 - f) * torch.cat([z, full])


def split(d):
    i = int(np.floor(d))
    return i, float(np.float32(d) - np.float32(i))


def torch_step(belief, belief_prev, score_prev, shift, taps, floor):
    """one step of the recursion for a batch under one shift -> (score, (index, exponent))"""
    import torch
    import torch.nn.functional as F
    B = belief.shape[0]
    r = taps.numel() - 1
    K = 2 * r + 2
    if belief_prev is None:
        w = torch.where(belief > 0, belief, torch.zeros_like(belief))
    else:
        prior = torch_predict_c(belief_prev, shift, taps) + floor
        lik = torch.where(belief > 0, belief / prior, torch.zeros_like(belief))
        (ix, fx), (iy, fy) = split(shift[0]), split(shift[1])
        ux, uy = merged(taps, fx), merged(taps, fy)
        pad = F.pad(score_prev.view(B, 512, 512), (PAD, PAD, PAD, PAD))
        x0, y0 = PAD - ix - r - 1, PAD - iy - r - 1
        rows = pad[:, y0:y0 + 512 + K - 1, x0:x0 + 512 + K - 1]
        mid = (rows.unfold(2, K, 1) * ux).amax(dim=3)                    # [B, 512 + K - 1, 512]
        win = (mid.unfold(1, K, 1) * uy).amax(dim=3)                     # [B, 512, 512]
        peak = score_prev.view(B, -1).amax(dim=1)
        w = lik * torch.maximum(win, (floor * peak).view(B, 1, 1))
        w = torch.where(w > 0, w, torch.zeros_like(w))
    W, idx = w.view(B, -1).max(dim=1)
    _, ex = torch.frexp(W)
    e = ex - 1
    return torch.ldexp(w, -e.view(B, 1, 1)), (idx, e)


def torch_back(score_prev, idx_prev, cell, shift, taps, floor):
    """one link for a batch under one shift -> (previous cell, kind 0 move / 1 jump)"""
    import torch
    B = score_prev.shape[0]
    r = taps.numel() - 1
    K = 2 * r + 2
    (ix, fx), (iy, fy) = split(shift[0]), split(shift[1])
    ux, uy = merged(taps, fx), merged(taps, fy)
    k = torch.arange(K, device=cell.device)
    gx = (cell % 512 - ix - r - 1).view(B, 1) + k
    gy = (cell // 512 - iy - r - 1).view(B, 1) + k
    ok = ((gy >= 0) & (gy < 512)).view(B, K, 1) & ((gx >= 0) & (gx < 512)).view(B, 1, K)
    src = gy.clamp(0, 511).view(B, K, 1) * 512 + gx.clamp(0, 511).view(B, 1, K)
    vals = uy.view(1, K, 1) * (ux.view(1, 1, K) * score_prev.view(B, -1).gather(1, src.view(B, -1)).view(B, K, K))
    vals = torch.where(ok, vals, torch.full_like(vals, -float("inf"))).view(B, -1)
    best, at = vals.max(dim=1)
    jump = floor * score_prev.view(B, -1).gather(1, idx_prev.view(B, 1)).view(B)
    jumped = jump > best
    return torch.where(jumped, idx_prev, src.view(B, -1).gather(1, at.view(B, 1)).view(B)), jumped.to(torch.int32)


def torch_path(log, taps):
    import torch
    T = len(log)
    scores, heads = [None] * T, [None] * T
    scores[0], heads[0] = torch_step(log[0][0], None, None, None, taps, FLOOR)
    for t in range(1, T):
        scores[t], heads[t] = torch_step(log[t][0], log[t - 1][0], scores[t - 1], SHIFT, taps, FLOOR)
    cells, kinds = [None] * T, [None] * T
    cells[-1] = heads[-1][0]
    for t in range(T - 1, 0, -1):
        cells[t - 1], kinds[t] = torch_back(scores[t - 1], heads[t - 1][0], cells[t], SHIFT, taps, FLOOR)
    kinds[0] = torch.full_like(kinds[1], 2)
    return torch.stack(cells), torch.stack(kinds), scores


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, models, viterbi, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()
    taps = torch.as_tensor(aerial.gaussian_taps(SIGMA, RADIUS)).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del res
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_viterbi.py", "frames": args.frames, "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "shift_px": list(SHIFT)},
           "hbm_copy_TBps": HBM_COPY_TBPS, "cases": {}}
    for batch in (1, 32):
        log = synthetic_log(args.frames, batch, taps, dev)

        def library(log=log):
            return viterbi.map_path(model, log)

        def torch_form(log=log):
            return torch_path(log, taps)

        paths = {"library": library, "torch": torch_form}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        cells, links, _, scores = library()
        tcells, tkinds, _ = torch_form()
        diff = 0.0
        for t in range(min(4, args.frames)):           # the torch step fed the library's previous map
            s, _ = torch_step(log[t][0], log[t - 1][0] if t else None, scores[t - 1] if t else None, SHIFT, taps, FLOOR)
            big = scores[t] > 1e-12
            diff = max(diff, float(((s - scores[t]).abs()[big] / scores[t][big]).max().item()))
        same = float(((cells.to(torch.int64) == tcells) & (links == tkinds)).float().mean().item())
        if diff > 1e-5:
            raise SystemExit(f"the torch form is not the library's recursion: step difference {diff:.3g}")
        del cells, links, scores, tcells, tkinds
        torch.cuda.synchronize()
        res = {"batch": batch, "torch_step_against_library_max_rel_diff": diff, "torch_path_share_of_library_cells_and_kinds": same, "runs": []}
        names = list(paths)
        for run in range(2):
            ms = {n: [] for n in names}
            launches = {n: 0 for n in names}
            for i in range(args.iters):
                k = i % len(names)
                for n in names[k:] + names[:k]:
                    t, c = timed(paths[n])
                    ms[n].append(t)
                    launches[n] = c
            r = {}
            for n in names:
                v = np.asarray(ms[n])
                r[n] = {"median_ms": round(float(np.median(v)), 4), "p99_ms": round(float(np.percentile(v, 99)), 4),
                        "per_frame_ms": round(float(np.median(v)) / args.frames, 5), "library_launches_per_path": launches[n]}
            r["torch_over_library"] = round(r["torch"]["median_ms"] / r["library"]["median_ms"], 3)
            bytes_per_frame = 6 * MAP_BYTES * batch
            rate = bytes_per_frame / (r["library"]["per_frame_ms"] * 1e-3) / 1e12
            r["library_bytes_per_frame"] = bytes_per_frame
            r["library_TBps"] = round(rate, 4)
            r["library_share_of_hbm_copy_rate"] = round(rate / HBM_COPY_TBPS, 4)
            res["runs"].append(r)
        out["cases"][f"b{batch}"] = res
        del log
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
