"""A backward sweep over a recorded stream (smooth.smooth_stream, ccvpe_track_smooth) against the same recursion written
in torch - what a caller has to do without it - in one process.

    python tools/time_smooth.py [--frames 100] [--iters 10] [--warmup 2] [--out profiles/time_smooth.json]

The log is synthetic, so that no network runs: per frame a belief of two Gaussian bumps on a small ground, normalised to mass 1, the
true bump moving by the shift; sigma 2 px, radius 6, floor 1e-9, a fractional shift - the predict settings of tools/time_track.py.
Cases: batch 1 and batch 32, --frames frames each.  Two forms, each a whole sweep that leaves every frame's smoothed map on the device:

    a  library  smooth.smooth_stream(model, log)
    b  torch    per frame: the zero-filled bilinear shift (four weighted slices) and the two conv2d blur passes for the prior, the
                divide, sum, the shift and passes again with the negated shift, the product, its sum and the scale, and max for the
                stats row

Every shape is warmed up first; then the two forms alternate --iters times per case (the order rotates), each sweep timed on the host
between two device synchronisations; the whole measurement runs twice.  Prints one JSON line: per case, run and form the median / p99
ms per sweep, per frame, the library's launches per sweep, the ratio b / a, the largest relative difference between the two forms'
maps where they are above 1e-12 of the peak, and the library form's compulsory traffic - per query and frame eight map passes of 1 MB:
b, s' read and g written; g, b read and w written; w read and s written - as a rate against the streaming rates of tools/ubench_hbm.py.
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
MAP_BYTES = 4 * 512 * 512
HBM_COPY_TBPS = 5.02      # profiles/r03_ubench_hbm.log: 1 GiB copy (read + write), TB/s moved


def torch_predict_c(m, shift, taps):
    """track_predict's c in torch ops (one shift for the batch): zero-filled bilinear shift, blur along x then y"""
    import torch
    import torch.nn.functional as F
    B = m.shape[0]
    dx, dy = float(shift[0]), float(shift[1])
    ix, iy = int(np.floor(dx)), int(np.floor(dy))
    fx, fy = dx - ix, dy - iy
    r = taps.numel() - 1
    pad = F.pad(m.view(B, 1, 512, 512), (513, 513, 513, 513))

    def at(oy, ox):   # the map moved by (ix + ox, iy + oy) whole pixels
        y0, x0 = 513 - iy - oy, 513 - ix - ox
        return pad[:, :, y0 - r:y0 + 512 + r, x0 - r:x0 + 512 + r]

    s = (1 - fy) * ((1 - fx) * at(0, 0) + fx * at(0, 1)) + fy * ((1 - fx) * at(1, 0) + fx * at(1, 1))
    full = torch.cat([taps.flip(0)[:-1], taps])
    return F.conv2d(F.conv2d(s, full.view(1, 1, 1, -1)), full.view(1, 1, -1, 1)).view(B, 512, 512)


def torch_smooth(belief, nxt, shift, taps, floor):
    import torch
    B = belief.shape[0]
    prior = torch_predict_c(belief, shift, taps) + floor
    g = torch.where(nxt > 0, nxt / prior, torch.zeros_like(nxt))
    G = g.view(B, -1).sum(dim=1)
    a = torch_predict_c(g, (-shift[0], -shift[1]), taps) + (floor * G).view(B, 1, 1)
    w = belief * a
    Z = w.view(B, -1).sum(dim=1)
    s = w * (1.0 / Z).view(B, 1, 1)
    prob, idx = s.view(B, -1).max(dim=1)
    return s, torch.stack([idx.to(torch.float32), prob, Z, G], dim=1)


def synthetic_log(frames, batch, taps, dev):
    import torch
    y, x = torch.meshgrid(torch.arange(512, device=dev, dtype=torch.float32), torch.arange(512, device=dev, dtype=torch.float32), indexing="ij")
    log = []
    for t in range(frames):
        tx, ty = 60.0 + SHIFT[0] * t, 400.0 + SHIFT[1] * t
        m = torch.exp(-((x - tx) ** 2 + (y - ty) ** 2) / 18.0) + 0.5 * torch.exp(-((x - 400.0) ** 2 + (y - 100.0) ** 2) / 18.0) + 1e-6
        m = (m / m.sum()).expand(batch, 512, 512).contiguous()
        log.append((m, None if t == 0 else np.asarray([SHIFT] * batch), taps, FLOOR))
    return log


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
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()
    taps_np = aerial.gaussian_taps(SIGMA, RADIUS)
    taps = torch.as_tensor(taps_np).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del res
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_smooth.py", "frames": args.frames, "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "shift_px": list(SHIFT)},
           "hbm_copy_TBps": HBM_COPY_TBPS, "cases": {}}
    for batch in (1, 32):
        log = synthetic_log(args.frames, batch, taps, dev)

        def library(log=log):
            return smooth.smooth_stream(model, log)

        def torch_form(log=log):
            maps = [None] * len(log)
            maps[-1] = run = log[-1][0]
            for t in range(len(log) - 2, -1, -1):
                run, _ = torch_smooth(log[t][0], run, SHIFT, taps, FLOOR)
                maps[t] = run
            return maps

        paths = {"library": library, "torch": torch_form}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        a, b = library()[0][0], torch_form()[0]
        big = b > 1e-12 * b.max()
        diff = float(((a - b).abs()[big] / b[big]).max().item())
        del a, b, big
        torch.cuda.synchronize()
        res = {"batch": batch, "library_against_torch_max_rel_diff_frame0": diff, "runs": []}
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
            bytes_per_frame = 8 * MAP_BYTES * batch
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
