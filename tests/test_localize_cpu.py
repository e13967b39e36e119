"""Pose-only forward entry points without a GPU: argument checks of the C ABI and of the model methods."""
import ctypes as C

import pytest
import torch

from ccvpe_amd import _lib, models

EINVAL = -1


def test_null_arguments_return_einval(built_library):
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    # null handle
    assert lib.ccvpe_localize(None, p, 320, 640, p, 1, p, None) == EINVAL
    assert lib.ccvpe_localize_cached(None, p, 320, 640, p, 1, p, None) == EINVAL
    # null inputs / rows / cache (checked before the handle is used)
    assert lib.ccvpe_localize(None, None, 320, 640, p, 1, p, None) == EINVAL
    assert lib.ccvpe_localize(None, p, 320, 640, None, 1, p, None) == EINVAL
    assert lib.ccvpe_localize(None, p, 320, 640, p, 1, None, None) == EINVAL
    assert b"rows" in lib.ccvpe_last_error()
    assert lib.ccvpe_localize_cached(None, p, 320, 640, None, 1, p, None) == EINVAL
    assert lib.ccvpe_localize_cached(None, p, 320, 640, p, 1, None, None) == EINVAL


def _model():
    return models.CVM_VIGOR_ori_prior("cpu", 180.0, True)


def test_localize_requires_eval_mode():
    m = _model().train()
    g, s = torch.zeros(1, 3, 320, 640), torch.zeros(1, 3, 512, 512)
    with pytest.raises(RuntimeError, match="eval"):
        m.localize(g, s)
    with pytest.raises(RuntimeError, match="eval"):
        m.localize_cached(g, torch.zeros(16))


def test_localize_refuses_cpu_tensors():
    m = _model().eval()
    g, s = torch.zeros(1, 3, 320, 640), torch.zeros(1, 3, 512, 512)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.localize(g, s)
    with pytest.raises(ValueError, match="cuda"):
        m.localize_cached(g, torch.zeros(16))
