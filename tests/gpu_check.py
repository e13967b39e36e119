"""Manual parity script (GPU box; lives under tests/ because it uses the oracle): run the HIP forward with debug taps, print the per-stage
table of tests/stage_ref.py (every stage against the fp64 oracle on the device's own input) and compare the nine outputs with the oracle's forward."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ccvpe_amd import models, weights
from oracle import ccvpe_oracle as orc
from tests import stage_ref

CASES = {
    "vigor_ori_prior": (models.CVM_VIGOR_ori_prior, dict(ori_noise=180.0, circular_padding=True), 360.0),
    "vigor_ori_prior_fov108": (models.CVM_VIGOR_ori_prior, dict(ori_noise=72.0, circular_padding=False), 108.0),
    "vigor": (models.CVM_VIGOR, dict(circular_padding=True), 360.0),
    "kitti": (models.CVM_KITTI, {}, 360.0),
    "oxford": (models.CVM_OxfordRobotCar, {}, 360.0),
}


def run(case, B=1, debug=True):
    cls, kw, fov = CASES[case]
    variant = cls._variant
    sd = weights.generate_state_dict(variant, 0)
    grd, sat = weights.generate_inputs(variant, B, 0, fov)
    grd, sat = torch.from_numpy(grd), torch.from_numpy(sat)
    t0 = time.time()
    ref = orc.forward(variant, sd, grd, sat, kw.get("circular_padding", False), kw.get("ori_noise"))
    print(f"[{case}] oracle {time.time()-t0:.2f}s", flush=True)
    m = cls("cuda", **kw)
    m.load_state_dict(sd)
    m.to("cuda").eval()
    m.set_debug(debug)
    t0 = time.time()
    out = m(grd.cuda(), sat.cuda())
    torch.cuda.synchronize()
    print(f"[{case}] hip first call {time.time()-t0:.2f}s", flush=True)
    names = ["logits", "heatmap", "ori", "ms1", "ms2", "ms3", "ms4", "ms5", "ms6"]
    worst = 0.0
    if debug:   # every stage against the fp64 oracle on the device's own input (tests/stage_ref.py; asserted in tests/test_stages_gpu.py)
        circ, noise = kw.get("circular_padding", False), kw.get("ori_noise")
        print(stage_ref.format_table(stage_ref.check_stages(m.read_tap, out, variant, sd, grd, sat, circ, noise)))
    for n, a, b in zip(names, ref, out):
        b = b.cpu()
        d = (a - b).abs().max().item()
        s = a.abs().max().item()
        rel = d / s
        if n != "ori":
            worst = max(worst, rel)
        print(f"  out {n:8s} {tuple(b.shape)} maxdiff {d:.3g} rel {rel:.3g} nan={bool(torch.isnan(b).any())}")
    return worst


if __name__ == "__main__":
    cases = sys.argv[1:] or list(CASES)
    bad = 0
    for c in cases:
        w = run(c)
        print(f"[{c}] worst rel (non-ori) {w:.3g}")
        bad += w > 1e-3
    sys.exit(1 if bad else 0)
