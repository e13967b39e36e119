"""Shared helpers for the golden fixtures under tests/golden/ (data only: expected values on a fixed
lattice + whole-tensor statistics, captured from the reference by oracle/make_golden.py)."""
from __future__ import annotations

import os
from typing import Dict

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (variant, ctor kwargs, fov, batch, seed)
CONFIGS = {
    "vigor_prior180_circ": dict(variant="vigor_ori_prior", circular=True, ori_noise=180.0, fov=360.0, batch=1, seed=0),
    "vigor_prior72_fov108": dict(variant="vigor_ori_prior", circular=False, ori_noise=72.0, fov=108.0, batch=1, seed=0),
    "vigor_circ": dict(variant="vigor", circular=True, ori_noise=None, fov=360.0, batch=1, seed=0),
    "kitti": dict(variant="kitti", circular=False, ori_noise=None, fov=360.0, batch=1, seed=0),
    "oxford": dict(variant="oxford", circular=False, ori_noise=None, fov=360.0, batch=1, seed=0),
    "vigor_prior180_b2": dict(variant="vigor_ori_prior", circular=True, ori_noise=180.0, fov=360.0, batch=2, seed=3),
}

# tests/test_oracle_vs_reference.py: (variant, circular, ori_noise, fov) at batch 1, seed 5 - all four model classes of the
# reference; fixtures tests/golden/reference_<variant>.npz (oracle/make_reference_golden.py) - and three cropped, odd ground widths, the
# driver's crop grd[..., :int(W * fov / 360)]: fixtures reference_<variant>_fov<fov>.npz
REFERENCE_CASES = [
    ("vigor_ori_prior", True, 36.0, 360.0),
    ("vigor", True, None, 360.0),
    ("kitti", False, None, 360.0),
    ("oxford", False, None, 360.0),
    ("vigor", True, None, 270.0),      # width 480: feature width 15, L6 = 30
    ("kitti", False, None, 120.0),     # width 341: 170, 85, 42, 21, 10 down the encoder
    ("oxford", False, None, 312.0),    # width 200: feature width 6
]
REFERENCE_SEED = 5
REFERENCE_LATTICE = 16384


def reference_fixture(variant: str, fov: float) -> str:
    """Path of the fixture of a REFERENCE_CASES entry."""
    name = f"reference_{variant}" + ("" if fov == 360.0 else f"_fov{int(fov)}")
    return os.path.join(GOLDEN_DIR, name + ".npz")


OUTPUT_NAMES = ["logits", "heatmap", "ori", "ms1", "ms2", "ms3", "ms4", "ms5", "ms6"]
FULL_LIMIT = 32768
LATTICE_TARGET = 16384


def lattice(numel: int, target: int = LATTICE_TARGET, full: int = FULL_LIMIT) -> np.ndarray:
    """Deterministic sample positions in a flattened tensor: everything for small tensors, otherwise
    ~`target` (default 16k) positions on an odd stride (odd => not aligned with the power-of-two image widths)."""
    if numel <= full:
        return np.arange(numel, dtype=np.int64)
    stride = (numel + target - 1) // target
    stride |= 1
    return np.arange(0, numel, stride, dtype=np.int64)


def summarize(name: str, a: np.ndarray, target: int = LATTICE_TARGET, full: int = FULL_LIMIT) -> Dict[str, np.ndarray]:
    a = np.ascontiguousarray(a, dtype=np.float32)
    flat = a.reshape(-1)
    a64 = flat.astype(np.float64)
    return {
        f"{name}/shape": np.array(a.shape, dtype=np.int64),
        f"{name}/values": flat[lattice(flat.size, target, full)].copy(),
        f"{name}/stats": np.array([a64.sum(), np.abs(a64).sum(), np.sqrt((a64 * a64).sum()), np.abs(a64).max()]),
        f"{name}/argmax": np.array([int(np.argmax(flat))], dtype=np.int64),
    }


def compare(name: str, fx, got: np.ndarray, rtol: float, target: int = LATTICE_TARGET, full: int = FULL_LIMIT) -> float:
    """Assert `got` matches the fixture entry `name`; returns the scale-relative max error.
    Error is measured relative to the tensor's max |value| (fixture stats[3])."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    shape = tuple(int(s) for s in fx[f"{name}/shape"])
    assert tuple(got.shape) == shape, f"{name}: shape {got.shape} != fixture {shape}"
    flat = got.reshape(-1)
    exp = fx[f"{name}/values"]
    idx = lattice(flat.size, target, full)
    assert idx.size == exp.size
    scale = float(fx[f"{name}/stats"][3])
    err = float(np.abs(flat[idx].astype(np.float64) - exp.astype(np.float64)).max()) / max(scale, 1e-30)
    assert np.isfinite(flat).all(), f"{name}: non-finite values"
    assert err <= rtol, f"{name}: lattice error {err:.3g} > {rtol:g} (scale {scale:.3g})"
    g64 = flat.astype(np.float64)
    st = fx[f"{name}/stats"]
    n = flat.size
    # whole-tensor statistics catch errors off the lattice; tolerances scale with sqrt(n) rounding growth
    assert abs(np.abs(g64).sum() - st[1]) <= rtol * max(st[1], 1e-30), f"{name}: abs-sum {np.abs(g64).sum():.6g} vs {st[1]:.6g}"
    assert abs(np.sqrt((g64 * g64).sum()) - st[2]) <= rtol * max(st[2], 1e-30), f"{name}: l2 mismatch"
    assert abs(g64.sum() - st[0]) <= rtol * max(st[1], 1e-30), f"{name}: sum mismatch"
    return err


def load(name: str):
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    return np.load(path, allow_pickle=False)
