"""Capture tests/golden/reference_<variant>[_fov<fov>].npz from the REAL reference (build container only) - TEST INFRASTRUCTURE.

    python -m oracle.make_reference_golden

For every case of tests/golden_util.REFERENCE_CASES (batch 1, seed REFERENCE_SEED): the reference nn.Module (imported
through oracle/reference_harness.py) runs under no_grad; its 9 outputs and the un-normalised orientation map (a forward
hook on conv1_ori, before F.normalize) are stored on a lattice of ~16k positions per tensor (everything below that) with
whole-tensor statistics, plus the orientation magnitude on the ori lattice; the KITTI file also holds the reference
module's state_dict key order.  The fixtures are data only; tests/test_oracle_vs_reference.py checks the oracle against them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvpe_amd import weights  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402
from tests import golden_util as gu  # noqa: E402

N = gu.REFERENCE_LATTICE


def capture(variant, circ, noise, fov) -> dict:
    sd = weights.generate_state_dict(variant, gu.REFERENCE_SEED)
    grd, sat = weights.generate_inputs(variant, 1, gu.REFERENCE_SEED, fov)
    net = rh.build(variant, sd, circ, noise)
    raw = {}
    hook = net.conv1_ori.register_forward_hook(lambda _m, _i, out: raw.__setitem__("ref", out.detach()))
    with torch.no_grad():
        outs = net(torch.from_numpy(grd), torch.from_numpy(sat))
    hook.remove()
    fx = {}
    for name, t in zip(gu.OUTPUT_NAMES, outs):
        fx.update(gu.summarize(f"{variant}/{name}", t.numpy(), N, N))
    r = raw["ref"].numpy()
    fx.update(gu.summarize(f"{variant}/ori_level1", r, N, N))
    mag = np.sqrt((r.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).repeat(2, axis=1).astype(np.float32)
    fx[f"{variant}/ori/magnitude"] = mag.reshape(-1)[gu.lattice(mag.size, N, N)]
    # drift guards on the generator itself
    fx[f"{variant}/meta/grd_abs_sum"] = np.array([np.abs(grd.astype(np.float64)).sum()])
    fx[f"{variant}/meta/sat_abs_sum"] = np.array([np.abs(sat.astype(np.float64)).sum()])
    fx[f"{variant}/meta/weight_abs_sum"] = np.array([sum(float(v.double().abs().sum()) for v in sd.values())])
    return fx


def main():
    assert rh.available(), "reference tree not present: goldens can only be made in the build container"
    torch.set_num_threads(os.cpu_count())
    for case in gu.REFERENCE_CASES:
        variant = case[0]
        fx = capture(*case)
        if variant == "kitti" and case[3] == 360.0:
            net = rh.build("kitti", weights.generate_state_dict("kitti", 0))
            fx["kitti/state_dict_keys"] = np.array(list(net.state_dict().keys()))
        path = gu.reference_fixture(variant, case[3])
        np.savez_compressed(path, **fx)
        print(f"{path}: {len(fx)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
