"""Device time of the KITTI and Oxford aerial preparation at batch 32, beside Pillow's host time per sample.

    python tools/time_aerial_prep.py [--batch 32] [--warmup 10] [--iters 50] [--host-samples 4]

Prints one JSON line.  Device times are hipEvent pairs around --iters back-to-back calls after --warmup calls (mean ms per call):
KITTI = ccvpe_preprocess_affine on 1280^2 tiles -> 512^2 (rotate, two BILINEAR shifts, rotate, crop, normalise; one launch);
Oxford = ccvpe_preprocess_window_resize of 800^2 windows of one resident 6000^2 map -> 512^2 (two launches).  Host times are the
reference's Pillow calls (datasets.py:577-598, datasets.py:306-321 + Resize) on one core, mean ms per sample, with the CPU model.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _device_ms(fn, warmup: int, iters: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def _host_ms(tiles, heading, sx, sy, th, mp, coords, n: int):
    """Pillow's per-sample cost of the reference's sequence of calls; None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None, None
    from ccvpe_amd import aerial
    mpp = aerial.get_meter_per_pixel(scale=1)
    pix = 20 / mpp
    n = min(n, len(tiles))
    pil = [Image.fromarray(t) for t in tiles[:n]]
    t = time.perf_counter()
    for b in range(n):
        s = pil[b].rotate(-float(heading[b]) / np.pi * 180)
        s = s.transform(s.size, Image.AFFINE, (1, 0, 1.08 / mpp, 0, 1, 0.26 / mpp), resample=Image.BILINEAR)
        s = s.transform(s.size, Image.AFFINE, (1, 0, -float(sx[b]) * pix, 0, 1, float(sy[b]) * pix), resample=Image.BILINEAR)
        s = s.rotate(float(th[b]) * 10)
        top, left = aerial.center_crop_box(s.height, s.width)
        s = s.crop((left, top, left + 512, top + 512))
        np.asarray(s)
    kitti = (time.perf_counter() - t) / n * 1e3
    big = Image.fromarray(mp)
    win = aerial.oxford_window(coords[:n])["origin"]
    t = time.perf_counter()
    for x0, y0 in win:
        np.asarray(big.crop((int(x0), int(y0), int(x0) + 800, int(y0) + 800)).resize((512, 512), Image.BILINEAR))
    oxford = (time.perf_counter() - t) / n * 1e3
    return kitti, oxford


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-samples", type=int, default=4)
    a = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial
    if not torch.cuda.is_available():
        sys.exit("time_aerial_prep.py needs a GPU: device times are not measured on the host")
    rng = np.random.default_rng(0)
    B = a.batch
    tiles = rng.integers(0, 256, size=(B, 1280, 1280, 3), dtype=np.uint8)
    heading = rng.uniform(-np.pi, np.pi, B)
    sx, sy, th = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    mp = rng.integers(0, 256, size=(6000, 6000, 3), dtype=np.uint8)
    coords = rng.uniform(400, 5600, size=(B, 2))

    tiles_d = torch.from_numpy(tiles).cuda()
    mats, filters = aerial.kitti_matrices(heading, sx, sy, th, (1280, 1280))
    mats_d = torch.from_numpy(mats).cuda()
    top, left = aerial.center_crop_box(1280, 1280)
    kitti_ms = _device_ms(lambda: _lib.preprocess_affine(tiles_d, mats_d, filters, (top, left, 512, 512)), a.warmup, a.iters)

    mp_d = torch.from_numpy(mp).cuda()
    origins_d = torch.from_numpy(aerial.oxford_window(coords)["origin"]).cuda()
    oxford_ms = _device_ms(lambda: _lib.preprocess_window_resize(mp_d, origins_d, (800, 800), (512, 512)), a.warmup, a.iters)

    host_kitti, host_oxford = _host_ms(tiles, heading, sx, sy, th, mp, coords, a.host_samples)
    print(json.dumps({
        "batch": B,
        "kitti_chain_ms": round(kitti_ms, 4),
        "kitti_samples_per_s": round(B / kitti_ms * 1e3, 1),
        "oxford_window_resize_ms": round(oxford_ms, 4),
        "oxford_samples_per_s": round(B / oxford_ms * 1e3, 1),
        "host_pillow_kitti_ms_per_sample": None if host_kitti is None else round(host_kitti, 2),
        "host_pillow_oxford_ms_per_sample": None if host_oxford is None else round(host_oxford, 2),
        "host_cpu": _cpu_model(),
        "host_cores_visible": len(os.sched_getaffinity(0)),
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
