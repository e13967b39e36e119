"""The MAP trajectory of a stream recorded across turning frames (viterbi.map_path_affine, ccvpe_track_viterbi_affine /
ccvpe_track_viterbi_back_affine) against the same recursion written in torch - what a caller has to do without it -
and against viterbi.map_path on a translation log of the same length, the yardstick for what the resampling costs; in one process.

    python tools/time_viterbi_affine.py [--frames 100] [--iters 10] [--warmup 2] [--out profiles/time_viterbi_affine.json]

The log is tools/time_smooth_affine.py's synthetic one, so that no network runs: sigma 2 px, radius 6, floor 1e-9, every link a turn
by 4 degrees about the grid's centre with the fractional shift of tools/time_smooth.py.  Cases: batch 1 and batch 32, --frames frames
each.  Three forms, each a whole forward sweep and backtrack that leave every frame's score map, the cells and the link kinds on the
device:

    a  library      viterbi.map_path_affine(model, log)
    b  torch        once per sweep the sampling grid and the four gather index / weight maps of the matrix (time_smooth_affine.TorchLink);
                    per frame grid_sample on the window plus the radius and the two conv2d blur passes for the prior, the divide, a
                    gather of the four taps with amax, the two max passes as unfold + multiply + amax over the 2r + 1 taps, the jump,
                    the product, max, frexp and ldexp; per link a gather of the four taps of the cell's (2r + 1)^2 samples, multiply,
                    argmax and the comparison with the jump
    c  translation  viterbi.map_path(model, log) on the same beliefs with the shift in place of the matrix

The torch form is checked first: its step, fed the library's previous score map, must give the library's map to 1e-4 relative on the
first frames (grid_sample takes normalised float32 coordinates, which place a sample to about 3e-5 px); the share of the free-running
torch path's cells and kinds that are the library's is reported.  Every shape is warmed up; then the forms alternate --iters times per case (the order rotates), each timed on the host between two device synchronisations;
the whole measurement runs twice.  Prints one JSON line: per case, run and form the median / p99 ms per path, per frame, the launches
per path, the ratios b / a and a / c, and the library form's compulsory traffic - per query and frame six map passes of 1 MB: b, b-,
v- read and w written; w read and v written - as a rate against the copy rate of tools/ubench_hbm.py.
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

from time_smooth_affine import FLOOR, HBM_COPY_TBPS, MAP_BYTES, RADIUS, SHIFT, SIGMA, TorchLink, synthetic_log  # noqa: E402

TURN_DEG = 4.0


def torch_step(belief, belief_prev, score_prev, link, taps, floor):
    """one step of the recursion for a batch under one matrix -> (score, (index, exponent))"""
    import torch
    import torch.nn.functional as F
    B = belief.shape[0]
    if belief_prev is None:
        w = torch.where(belief > 0, belief, torch.zeros_like(belief))
    else:
        r, n = link.r, link.n
        K = 2 * r + 1
        full = torch.cat([taps.flip(0)[:-1], taps])
        s = link.det * F.grid_sample(belief_prev.view(B, 1, 512, 512), link.grid.expand(B, n, n, 2), mode="bilinear", padding_mode="zeros",
                                     align_corners=True)
        prior = F.conv2d(F.conv2d(s, full.view(1, 1, 1, -1)), full.view(1, 1, -1, 1)).view(B, 512, 512) + floor
        lik = torch.where(belief > 0, belief / prior, torch.zeros_like(belief))
        flat = score_prev.view(B, -1)
        q = torch.stack([flat[:, idx] * wgt for idx, wgt in link.taps]).amax(dim=0).view(B, n, n)
        mid = (q.unfold(2, K, 1) * full).amax(dim=3)                     # [B, n, 512]
        win = (mid.unfold(1, K, 1) * full).amax(dim=3)                   # [B, 512, 512]
        peak = flat.amax(dim=1)
        w = lik * torch.maximum(win, (floor * peak).view(B, 1, 1))
        w = torch.where(w > 0, w, torch.zeros_like(w))
    W, idx = w.view(B, -1).max(dim=1)
    _, ex = torch.frexp(W)
    e = ex - 1
    return torch.ldexp(w, -e.view(B, 1, 1)), (idx, e)


def torch_back(score_prev, idx_prev, cell, link, taps, floor):
    """one link for a batch under one matrix -> (previous cell, kind 0 move / 1 jump)"""
    import torch
    B = score_prev.shape[0]
    r, n = link.r, link.n
    K = 2 * r + 1
    full = torch.cat([taps.flip(0)[:-1], taps])
    k = torch.arange(K, device=cell.device)
    # sample (x' - r + kx, y' - r + ky) is entry (y' + ky, x' + kx) of the link's maps, which start at -r
    at = ((cell // 512).view(B, 1, 1) + k.view(1, K, 1)) * n + (cell % 512).view(B, 1, 1) + k.view(1, 1, K)
    u = (full.view(K, 1) * full.view(1, K)).view(1, K, K)
    flat = score_prev.view(B, -1)
    vals, srcs = [], []
    for idx, wgt in link.taps:
        src = idx[at]
        vals.append(u * (wgt[at] * flat.gather(1, src.view(B, -1)).view(B, K, K)))
        srcs.append(src)
    vals, srcs = torch.stack(vals, dim=1).view(B, -1), torch.stack(srcs, dim=1).view(B, -1)
    best, pick = vals.max(dim=1)
    jump = floor * flat.gather(1, idx_prev.view(B, 1)).view(B)
    jumped = jump > best
    return torch.where(jumped, idx_prev, srcs.gather(1, pick.view(B, 1)).view(B)), jumped.to(torch.int32)


def torch_path(log, link, taps):
    import torch
    T = len(log)
    scores, heads = [None] * T, [None] * T
    scores[0], heads[0] = torch_step(log[0][0], None, None, link, taps, FLOOR)
    for t in range(1, T):
        scores[t], heads[t] = torch_step(log[t][0], log[t - 1][0], scores[t - 1], link, taps, FLOOR)
    cells, kinds = [None] * T, [None] * T
    cells[-1] = heads[-1][0]
    for t in range(T - 1, 0, -1):
        cells[t - 1], kinds[t] = torch_back(scores[t - 1], heads[t - 1][0], cells[t], link, taps, FLOOR)
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
    matrix = aerial.rigid_matrix(TURN_DEG, list(SHIFT))

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del res
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_viterbi_affine.py", "frames": args.frames, "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "turn_deg": TURN_DEG, "shift_px": list(SHIFT)},
           "hbm_copy_TBps": HBM_COPY_TBPS, "cases": {}}
    for batch in (1, 32):
        log, plain = synthetic_log(args.frames, batch, matrix, SHIFT, taps, dev)
        link = TorchLink(matrix, RADIUS, dev)

        def library(log=log):
            return viterbi.map_path_affine(model, log)

        def torch_form(log=log, link=link):
            return torch_path(log, link, taps)

        def translation(plain=plain):
            return viterbi.map_path(model, plain)

        paths = {"library": library, "torch": torch_form, "translation": translation}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        cells, links, _, scores = library()
        tcells, tkinds, _ = torch_form()
        diff = 0.0
        for t in range(min(4, args.frames)):           # the torch step fed the library's previous map
            s, _ = torch_step(log[t][0], log[t - 1][0] if t else None, scores[t - 1] if t else None, link, taps, FLOOR)
            big = scores[t] > 1e-12
            diff = max(diff, float(((s - scores[t]).abs()[big] / scores[t][big]).max().item()))
        same = float(((cells.to(torch.int64) == tcells) & (links == tkinds)).float().mean().item())
        if diff > 1e-4:
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
            r["library_over_translation"] = round(r["library"]["median_ms"] / r["translation"]["median_ms"], 3)
            bytes_per_frame = 6 * MAP_BYTES * batch
            rate = bytes_per_frame / (r["library"]["per_frame_ms"] * 1e-3) / 1e12
            r["library_bytes_per_frame"] = bytes_per_frame
            r["library_TBps"] = round(rate, 4)
            r["library_share_of_hbm_copy_rate"] = round(rate / HBM_COPY_TBPS, 4)
            res["runs"].append(r)
        out["cases"][f"b{batch}"] = res
        del log, plain, link
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
