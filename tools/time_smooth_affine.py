"""A backward sweep over a stream recorded across turning frames (smooth.smooth_stream_affine, ccvpe_track_smooth_affine)
against the same recursion written in torch - what a caller has to do without it - and, where the frames only translate, against
smooth.smooth_stream, in one process.

    python tools/time_smooth_affine.py [--frames 100] [--iters 10] [--warmup 2] [--out profiles/time_smooth_affine.json]

The log is synthetic, so that no network runs: per frame a belief of two Gaussian bumps on a small ground, normalised to mass 1, the
true bump moving as the frames' matrix says; sigma 2 px, radius 6, floor 1e-9 - the predict settings of tools/time_smooth.py.  Every
link of a stream has the same matrix: a turn about the grid's centre by 0, 5 or 45 degrees with the fractional shift of
tools/time_smooth.py.  Cases: batch 1 and batch 32 at each angle, --frames frames each.  Forms, each a whole sweep that leaves every
frame's smoothed map on the device:

    a  library      smooth.smooth_stream_affine(model, log)
    b  torch        once per sweep the sampling grid and the four scatter index / weight maps of the matrix; per frame grid_sample
                    (bilinear, zeros, align_corners) on the window plus the radius and the two conv2d blur passes for the prior, the
                    divide, sum, the two conv2d passes on the padded ratio map, the adjoint of grid_sample as four index_add_ calls,
                    the product, its sum and the scale, and max for the stats row
    c  translation  smooth.smooth_stream(model, log) with the shift in place of the matrix - the 0 degree cases only

Every shape is warmed up first; then the forms alternate --iters times per case (the order rotates), each sweep timed on the host
between two device synchronisations; the whole measurement runs twice.  Prints one JSON line: per case, run and form the median / p99
ms per sweep, per frame, the launches per sweep, the ratios b / a and a / c, the largest relative difference between the library's and
torch's maps where they are above 1e-12 of the peak, and the library form's compulsory traffic - per query and frame 8 + 2 e map
passes of 1 MB, e = ((512 + 2 r) / 512)^2: b, s' read and g written; g read and h written; h, b read and w written; w read and s
written - as a rate against the streaming rates of tools/ubench_hbm.py.
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

SIGMA, RADIUS, FLOOR = 2.0, 6, 1e-9
SHIFT = (3.37, -1.81)
ANGLES = (0.0, 5.0, 45.0)
MAP_BYTES = 4 * 512 * 512
HBM_COPY_TBPS = 5.02      # profiles/r03_ubench_hbm.log: 1 GiB copy (read + write), TB/s moved


class TorchLink:
    """what the torch form keeps per matrix: grid_sample's grid over the window plus r, and for the adjoint the flat source index and
    the weight of each of the sample's four cells (weight 0 where the cell lies outside the grid)"""

    def __init__(self, matrix, r, dev):
        import torch
        m0, m1, m2, m3, m4, m5 = (float(v) for v in matrix)
        self.r, self.n = r, 512 + 2 * r
        self.det = abs(m0 * m4 - m1 * m3)
        ext = torch.arange(-r, 512 + r, device=dev, dtype=torch.float64)
        X, Y = ext[None, :], ext[:, None]
        sx, sy = m0 * X + m1 * Y + m2, m3 * X + m4 * Y + m5
        self.grid = torch.stack([sx * (2.0 / 511.0) - 1.0, sy * (2.0 / 511.0) - 1.0], dim=-1).to(torch.float32)[None]
        fx0, fy0 = torch.floor(sx), torch.floor(sy)
        fx, fy = (sx - fx0).to(torch.float32), (sy - fy0).to(torch.float32)
        ix, iy = fx0.clamp(-4, 516).to(torch.int64), fy0.clamp(-4, 516).to(torch.int64)
        self.taps = []
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                jj, ii = iy + dy, ix + dx
                inside = (jj >= 0) & (jj < 512) & (ii >= 0) & (ii < 512)
                idx = (jj.clamp(0, 511) * 512 + ii.clamp(0, 511)).reshape(-1)
                self.taps.append((idx, (self.det * wy * wx * inside).reshape(-1)))


def torch_smooth(belief, nxt, link, taps, floor):
    import torch
    import torch.nn.functional as F
    B, r, n = belief.shape[0], link.r, link.n
    full = torch.cat([taps.flip(0)[:-1], taps])
    kx, ky = full.view(1, 1, 1, -1), full.view(1, 1, -1, 1)
    s = link.det * F.grid_sample(belief.view(B, 1, 512, 512), link.grid.expand(B, n, n, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    prior = F.conv2d(F.conv2d(s, kx), ky).view(B, 512, 512) + floor
    g = torch.where(nxt > 0, nxt / prior, torch.zeros_like(nxt))
    G = g.view(B, -1).sum(dim=1)
    h = F.conv2d(F.conv2d(F.pad(g.view(B, 1, 512, 512), (2 * r,) * 4), kx), ky).view(B, n * n)
    A = torch.zeros(B, 512 * 512, device=belief.device)
    for idx, wgt in link.taps:
        A.index_add_(1, idx, h * wgt)
    w = belief * (A.view(B, 512, 512) + (floor * G).view(B, 1, 1))
    Z = w.view(B, -1).sum(dim=1)
    out = w * (1.0 / Z).view(B, 1, 1)
    prob, idx = out.view(B, -1).max(dim=1)
    return out, torch.stack([idx.to(torch.float32), prob, Z, G], dim=1)


def synthetic_log(frames, batch, matrix, shift, taps, dev):
    """(the affine log, the same log with `shift` in place of the matrix): the true bump moves as the content does, p -> M^-1 p"""
    import torch
    from ccvpe_amd import aerial
    inv = aerial.affine_invert(matrix)
    y, x = torch.meshgrid(torch.arange(512, device=dev, dtype=torch.float32), torch.arange(512, device=dev, dtype=torch.float32), indexing="ij")
    log, plain = [], []
    tx, ty = 200.0, 300.0
    for t in range(frames):
        if t:
            tx, ty = inv[0] * tx + inv[1] * ty + inv[2], inv[3] * tx + inv[4] * ty + inv[5]
        m = torch.exp(-((x - tx) ** 2 + (y - ty) ** 2) / 18.0) + 0.5 * torch.exp(-((x - 400.0) ** 2 + (y - 100.0) ** 2) / 18.0) + 1e-6
        m = (m / m.sum()).expand(batch, 512, 512).contiguous()
        log.append((m, None if t == 0 else np.tile(matrix, (batch, 1)), taps, FLOOR))
        plain.append((m, None if t == 0 else np.asarray([shift] * batch), taps, FLOOR))
    return log, plain


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, models, smooth, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    model = models.CVM_KITTI(dev)
    model.load_state_dict(weights.generate_state_dict("kitti", 0))
    model = model.to(dev).eval()
    taps_np = aerial.gaussian_taps(SIGMA, RADIUS)
    taps = torch.as_tensor(taps_np).to(dev)
    e = ((512 + 2 * RADIUS) / 512.0) ** 2

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del res
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_smooth_affine.py", "frames": args.frames, "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "shift_px": list(SHIFT), "angles_deg": list(ANGLES)},
           "hbm_copy_TBps": HBM_COPY_TBPS, "cases": {}}
    for batch in (1, 32):
        for angle in ANGLES:
            matrix = aerial.rigid_matrix(angle, list(SHIFT))
            log, plain = synthetic_log(args.frames, batch, matrix, SHIFT, taps, dev)

            def library(log=log):
                return smooth.smooth_stream_affine(model, log)

            def torch_form(log=log, matrix=matrix):
                link = TorchLink(matrix, RADIUS, dev)
                maps = [None] * len(log)
                maps[-1] = run = log[-1][0]
                for t in range(len(log) - 2, -1, -1):
                    run, _ = torch_smooth(log[t][0], run, link, taps, FLOOR)
                    maps[t] = run
                return maps

            def translation(plain=plain):
                return smooth.smooth_stream(model, plain)

            paths = {"library": library, "torch": torch_form}
            if angle == 0.0:
                paths["translation"] = translation
            for _ in range(args.warmup):
                for fn in paths.values():
                    fn()
            a, b = library()[0][0], torch_form()[0]
            big = b > 1e-12 * b.max()
            diff = float(((a - b).abs()[big] / b[big]).max().item())
            del a, b, big
            torch.cuda.synchronize()
            res = {"batch": batch, "angle_deg": angle, "reach": list(smooth.affine_reach(matrix)),
                   "library_against_torch_max_rel_diff_frame0": diff, "runs": []}
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
                            "per_frame_ms": round(float(np.median(v)) / args.frames, 5), "library_launches_per_sweep": launches[n]}
                r["torch_over_library"] = round(r["torch"]["median_ms"] / r["library"]["median_ms"], 3)
                if "translation" in r:
                    r["library_over_translation"] = round(r["library"]["median_ms"] / r["translation"]["median_ms"], 3)
                bytes_per_frame = int((8 + 2 * e) * MAP_BYTES * batch)
                rate = bytes_per_frame / (r["library"]["per_frame_ms"] * 1e-3) / 1e12
                r["library_bytes_per_frame"] = bytes_per_frame
                r["library_TBps"] = round(rate, 4)
                r["library_share_of_hbm_copy_rate"] = round(rate / HBM_COPY_TBPS, 4)
                res["runs"].append(r)
            out["cases"][f"b{batch}_deg{angle:g}"] = res
            del log, plain
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
