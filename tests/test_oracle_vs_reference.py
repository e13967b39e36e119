"""Oracle vs the real reference on all four model classes - and at three cropped, odd ground widths (480, 341, 200) -, through the
fixtures tests/golden/reference_<variant>[_fov<fov>].npz that
oracle/make_reference_golden.py captured from the reference (data only: every output and the un-normalised orientation map
on a ~16k-position lattice, everything for smaller tensors, plus whole-tensor sum / abs-sum / L2 / max)."""
import numpy as np
import pytest
import torch

from ccvpe_amd import weights
from oracle import ccvpe_oracle as orc
from tests import golden_util as gu

RTOL = 2e-5
N = gu.REFERENCE_LATTICE


def _load(variant, fov=360.0):
    return np.load(gu.reference_fixture(variant, fov), allow_pickle=False)


def _check(fx, name, got):
    gu.compare(name, fx, got, RTOL, N, N)
    scale = float(fx[f"{name}/stats"][3])
    assert abs(float(np.abs(got.astype(np.float64)).max()) - scale) <= RTOL * scale, f"{name}: max |value| differs"


@pytest.mark.parametrize("variant,circ,noise,fov", gu.REFERENCE_CASES)   # reference models.py:49, 346, 655, 954
def test_full_tensor_agreement(variant, circ, noise, fov):
    fx = _load(variant, fov)
    torch.set_num_threads(8)
    sd = weights.generate_state_dict(variant, gu.REFERENCE_SEED)
    grd, sat = weights.generate_inputs(variant, 1, gu.REFERENCE_SEED, fov)
    # generator drift guard: the fixture is only meaningful for the same synthetic weights / inputs
    for key, a in (("grd_abs_sum", grd), ("sat_abs_sum", sat)):
        ref = fx[f"{variant}/meta/{key}"][0]
        assert abs(np.abs(a.astype(np.float64)).sum() - ref) < 1e-6 * ref
    ref = fx[f"{variant}/meta/weight_abs_sum"][0]
    assert abs(sum(float(v.double().abs().sum()) for v in sd.values()) - ref) < 1e-9 * ref
    taps = {}
    got = orc.forward(variant, sd, torch.from_numpy(grd), torch.from_numpy(sat), circ, noise, taps)
    assert len(got) == 9
    for name, t in zip(gu.OUTPUT_NAMES, got):
        if name == "ori":
            continue
        _check(fx, f"{variant}/{name}", t.numpy())
    # orientation: the un-normalised map, and the unit field weighted by the un-normalised magnitude
    # (F.normalize is ill-conditioned where the raw vector is ~0)
    _check(fx, f"{variant}/ori_level1", taps["ori_level1"].numpy())
    ori = got[2].numpy()
    assert tuple(ori.shape) == tuple(fx[f"{variant}/ori/shape"])
    idx = gu.lattice(ori.size, N, N)
    mag = fx[f"{variant}/ori/magnitude"].astype(np.float64)
    err = np.abs(ori.reshape(-1)[idx].astype(np.float64) - fx[f"{variant}/ori/values"].astype(np.float64)) * mag
    assert err.max() <= RTOL * mag.max()


def test_reference_state_dict_keys_match_spec():
    from ccvpe_amd import spec
    fx = _load("kitti")
    assert list(fx["kitti/state_dict_keys"]) == [k for k, _, _ in spec.state_dict_spec(spec.VARIANTS["kitti"])]
