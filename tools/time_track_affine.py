"""The affine predict step (ccvpe_track_predict_affine) against the translation kernel it generalises and against what a
caller has to do without it, in one process.

    python tools/time_track_affine.py [--iters 40] [--warmup 5] [--out profiles/time_track_affine.json]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 1
of oxford_stream through the cached update, batch 1 and batch 32 of kitti through the full update.  Per case, on the belief a first
update left on the device (sigma 2 px, radius 6, floor 1e-9):

    a   shift       track_predict with a fractional shift: the existing kernel, the yardstick for a translation
    b0  affine_0    track_predict_affine with the same translation as a matrix
    b5  affine_5    ... with a 5 degree turn about the centre on top
    b45 affine_45   ... with a 45 degree turn
    c   torch       the 5 degree step in torch ops: affine_grid + grid_sample(bilinear, zeros, align_corners=True - index i sits at
                    normalised coordinate 2 i / 511 - 1, the index convention of the matrix) on the window plus the blur's reach,
                    times |det|, the two conv2d blur passes, add floor, log
    d5  step_affine the whole tracked frame: b5 + track_update_cached / track_update
    dc  step_torch  the whole tracked frame: c + the same update

Every shape is warmed up first; then the forms alternate --iters times per case (the order rotates), each call timed on the host
between two device synchronisations.  Prints one JSON line: per case and form the median / p99 ms per call, the ratios b / a and
c / b5, and the largest difference between b5's and c's log-prior where both are above log(2 floor).
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


def build_model(variant, dev):
    from ccvpe_amd import models, weights
    m = {"kitti": models.CVM_KITTI, "oxford": models.CVM_OxfordRobotCar}[variant](dev)
    m.load_state_dict(weights.generate_state_dict(variant, 0))
    return m.to(dev).eval()


def torch_predict(belief, matrix, taps, floor):
    """track_predict_affine in torch ops (one matrix for the batch)"""
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import aerial
    B = belief.shape[0]
    r = taps.numel() - 1
    S = 512 + 2 * r
    half = (S - 1) / 2.0
    to_pixel = np.array([half, 0.0, half - r, 0.0, half, half - r])            # normalised output coordinate -> pixel index
    to_norm = np.array([1 / 255.5, 0.0, -1.0, 0.0, 1 / 255.5, -1.0])          # source index position -> normalised coordinate
    theta = aerial.affine_compose(to_norm, aerial.affine_compose(matrix, to_pixel))
    th = torch.as_tensor(theta.reshape(1, 2, 3), dtype=torch.float32, device=belief.device).expand(B, 2, 3)
    grid = F.affine_grid(th, (B, 1, S, S), align_corners=True)
    s = F.grid_sample(belief.view(B, 1, 512, 512), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    s = s * float(abs(matrix[0] * matrix[4] - matrix[1] * matrix[3]))
    full = torch.cat([taps.flip(0)[:-1], taps])
    c = F.conv2d(F.conv2d(s, full.view(1, 1, 1, -1)), full.view(1, 1, -1, 1))
    return torch.log(c + floor).view(B, 512, 512)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import aerial, weights
    dev = torch.device("cuda", 0)
    taps = torch.as_tensor(aerial.gaussian_taps(SIGMA, RADIUS)).to(dev)
    mats_np = {deg: aerial.rigid_matrix(float(deg), SHIFT) for deg in (0, 5, 45)}

    models_ = {}
    cases = []
    for case, variant, batch, cached in (("oxford_stream_b1_cached", "oxford", 1, True), ("kitti_b1", "kitti", 1, False),
                                         ("kitti_b32", "kitti", 32, False)):
        if variant not in models_:
            models_[variant] = build_model(variant, dev)
        m = models_[variant]
        g, s = weights.generate_inputs(variant, batch, 0, 360.0)
        g, s = torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev)
        cache = m.encode_aerial(s) if cached else None
        _, belief = m.track_update_cached(g, cache) if cached else m.track_update(g, s)
        shift = torch.tensor([SHIFT] * batch, dtype=torch.float32, device=dev)
        floor = torch.full((batch,), FLOOR, dtype=torch.float32, device=dev)
        mats = {deg: torch.as_tensor(np.tile(v, (batch, 1))).to(dev) for deg, v in mats_np.items()}

        def update(lp, m=m, g=g, s=s, c=cache):
            return m.track_update_cached(g, c, lp) if c is not None else m.track_update(g, s, lp)

        def affine(deg, m=m, bel=belief, mats=mats, fl=floor):
            return m.track_predict_affine(bel, mats[deg], taps, fl)

        def torch_form(bel=belief):
            return torch_predict(bel, mats_np[5], taps, FLOOR)

        paths = {"shift": lambda m=m, bel=belief, sh=shift, fl=floor: m.track_predict(bel, sh, taps, fl),
                 "affine_0": lambda f=affine: f(0), "affine_5": lambda f=affine: f(5), "affine_45": lambda f=affine: f(45),
                 "torch": torch_form,
                 "step_affine": lambda f=affine, u=update: u(f(5))[0],
                 "step_torch": lambda f=torch_form, u=update: u(f())[0]}
        cases.append((case, variant, batch, paths))

    diff = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        a, b = paths["affine_5"](), paths["torch"]()
        both = (a > np.log(2 * FLOOR)) & (b > np.log(2 * FLOOR))
        diff[case] = float((a - b)[both].abs().max().item()) if bool(both.any()) else 0.0
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"tool": "tools/time_track_affine.py", "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "shift_px": list(SHIFT)}, "cases": {}}
    for case, variant, batch, paths in cases:
        names = list(paths)
        ms = {n: [] for n in names}
        for i in range(args.iters):
            k = i % len(names)
            for n in names[k:] + names[:k]:
                ms[n].append(timed(paths[n]))
        res = {"variant": variant, "batch": batch, "max_abs_log_difference_affine_5_vs_torch": round(diff[case], 6)}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4)}
        med = {n: res[n]["median_ms"] for n in names}
        for n in ("affine_0", "affine_5", "affine_45"):
            res[n + "_over_shift"] = round(med[n] / med["shift"], 3)
        res["torch_over_affine_5"] = round(med["torch"] / med["affine_5"], 3)
        res["step_torch_over_step_affine"] = round(med["step_torch"] / med["step_affine"], 3)
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
