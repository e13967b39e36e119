"""Times of the joint MAP trajectory (ccvpe_track_joint_viterbi, ccvpe_track_joint_viterbi_back) next to the joint
smoother's (ccvpe_track_joint_smooth) on the same shapes in the same session.

    python tools/time_joint_viterbi.py [--iters 5] [--warmup 2] [--window 20] [--repeats 5] [--out FILE]

Cases: (nb, batch) in (36, 1), (72, 8); xy blur sigma 2 px, radius 6; heading blur radius 2; floor 1e-9; a fractional shift per bin
and a fractional turn.  The joints are synthetic (uniform random, scaled to mass 1; the score joint the first-frame call's): no value
changes what a launch moves.

The tool starts fresh child processes, one after the other - tools/time_track_joint_smooth.py's protocol.  The first runs under
`rocprofv3 --kernel-trace` (the per-launch times are the dispatches' own durations): per case a separator launch
(ccvpe_heading_predict), then --warmup + --iters steps and as many links.  The second runs with no profiler attached: per case,
after --warmup calls, --window back-to-back calls between two device events, --repeats times, for the step, the link and the
smoother's step; median and largest time per call.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((36, 1), (72, 8))
SIGMA, RADIUS, HTAPS, FLOOR, TURN = 2.0, 6, (0.6, 0.15, 0.05), 1e-9, 7.3
SEPARATOR = "heading_predict_kernel"
LAUNCHES = {"track_joint_xy_kernel": "viterbi.xy", "track_joint_viterbi_win_kernel": "viterbi.win", "track_joint_viterbi_mix_kernel": "viterbi.mix",
            "track_joint_viterbi_scale_kernel": "viterbi.scale", "track_joint_viterbi_back_kernel": "viterbi.back"}


def worker(args) -> int:
    """one child: args.mode "trace" (under the profiler) or "calls" (no profiler: whole calls)"""
    import torch
    from ccvpe_amd import aerial, models, smooth, viterbi, weights
    dev = torch.device("cuda", 0)

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e-3

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = [events(fn, args.window) * 1e3 for _ in range(args.repeats)]
        return round(float(np.median(ms)), 4), round(float(max(ms)), 4)

    out = {"device": torch.cuda.get_device_name(dev), "cases": {}}
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()
    taps = torch.as_tensor(aerial.gaussian_taps(SIGMA, RADIUS)).to(dev)
    htaps = torch.tensor(HTAPS, device=dev)
    sep_hist = torch.full((1, 8), 0.125, device=dev)
    for nb, batch in CASES:
        joint = torch.rand(batch, nb, 512, 512, device=dev)
        joint /= joint.sum(dim=(1, 2, 3), keepdim=True)
        prev = torch.rand(batch, nb, 512, 512, device=dev)
        prev /= prev.sum(dim=(1, 2, 3), keepdim=True)
        shift = torch.as_tensor(aerial.joint_shift_table(np.full(batch, 9.37), np.full(batch, -0.6), nb), dtype=torch.float32).to(dev)
        turn, floor = torch.full((batch,), TURN, device=dev), torch.full((batch,), FLOOR, device=dev)
        case = {"nb": nb, "batch": batch}
        score_prev, prev_stats = viterbi.track_joint_viterbi(model, prev)
        score = torch.empty_like(joint)
        cell, bin_ = prev_stats[:, 0].to(torch.int32), prev_stats[:, 1].to(torch.int32)

        def step():
            return viterbi.track_joint_viterbi(model, joint, prev, score_prev, prev_stats, shift, taps, floor, turn, htaps, out=score)

        def back():
            return viterbi.track_joint_viterbi_back(model, score_prev, prev_stats, cell, bin_, shift, taps, floor, turn, htaps)

        if args.mode == "trace":
            model.heading_predict(sep_hist, 0.0, taps[:1] * 0 + 1.0, 0.0)        # the separator of the trace
            for _ in range(args.warmup + args.iters):
                step()
                back()
            torch.cuda.synchronize()
        else:
            case["step_call_ms"], case["step_call_ms_max"] = timed(step)
            case["back_call_ms"], case["back_call_ms_max"] = timed(back)
            del score
            run = prev                                                        # (prev is not needed any more)

            def smooth_step():
                return smooth.track_joint_smooth(model, joint, run, shift, taps, floor, turn, htaps, out=run)

            case["smooth_call_ms"], case["smooth_call_ms_max"] = timed(smooth_step)
            case["step_over_smooth"] = round(case["step_call_ms"] / case["smooth_call_ms"], 3)
        out["cases"][f"nb{nb}_b{batch}"] = case
        del joint, prev
        torch.cuda.empty_cache()
    with open(args.worker, "w") as fh:
        json.dump(out, fh)
    return 0


def read_trace(trace_dir: str, warmup: int, iters: int) -> list:
    """the trace split at the separators: per segment {launch: median duration in us of the timed dispatches}"""
    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segments = []
    for r in rows:
        m = re.search("(" + "|".join([SEPARATOR] + list(LAUNCHES)) + ")", r["Kernel_Name"])
        if m and m.group(1) == SEPARATOR:
            segments.append({})
        elif m and segments:
            segments[-1].setdefault(LAUNCHES[m.group(1)], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [{k: round(float(np.median(v[-iters:])), 2) for k, v in seg.items()} for seg in segments]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=20, help="back-to-back calls per timed window of the untraced children")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case and entry point")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="calls", choices=["trace", "calls"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as tmp:
        me = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup), "--window", str(args.window),
              "--repeats", str(args.repeats)]
        runs = [("trace", [prof, "--kernel-trace", "-d", os.path.join(tmp, "trace"), "-o", "run", "--output-format", "csv", "--"]), ("calls", [])]
        results = {}
        for mode, front in runs:
            res = os.path.join(tmp, mode + ".json")
            p = subprocess.run(front + me + ["--worker", res, "--mode", mode], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=500)
            if p.returncode != 0 or not os.path.exists(res):
                sys.stderr.write(p.stdout[-4000:])
                raise SystemExit(f"the {mode} child failed with status {p.returncode}")
            with open(res) as fh:
                results[mode] = json.load(fh)
        segments = read_trace(os.path.join(tmp, "trace"), args.warmup, args.iters)
    out = results["calls"]
    for i, (key, case) in enumerate(out["cases"].items()):
        case["launch_us"] = segments[i] if i < len(segments) else {}
    out = {"tool": "tools/time_joint_viterbi.py", "iters": args.iters, "warmup": args.warmup, "window": args.window, "repeats": args.repeats,
           "settings": {"sigma_px": SIGMA, "radius": RADIUS, "heading_taps": list(HTAPS), "floor": FLOOR, "turn_deg": TURN}, **out}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
