"""Top-K pose hypotheses without a GPU: the numpy restatement (tests/topk_ref.py) against a brute-force reading of the
definition, and the argument checks of the C entry points and the model methods."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, models
from tests import topk_ref

EINVAL = -1


# ---- the restatement against the definition, pixel pair by pixel pair ---------------------------------------------------

def brute_peaks(H, r):
    h, w = H.shape
    out = np.zeros((h, w), bool)
    for py in range(h):
        for px in range(w):
            v = H[py, px]
            if not v > 0:
                continue
            p = py * w + px
            suppressed = False
            for qy in range(max(0, py - r), min(h, py + r + 1)):
                for qx in range(max(0, px - r), min(w, px + r + 1)):
                    q = qy * w + qx
                    if q == p:
                        continue
                    u = H[qy, qx]
                    if u > v or (u == v and q < p):   # (a NaN u fails both comparisons)
                        suppressed = True
            out[py, px] = not suppressed
    return out


def brute_topk(H, r, k):
    h, w = H.shape
    mask = brute_peaks(H, r)
    cand = sorted(((-float(H[y, x]), y * w + x) for y in range(h) for x in range(w) if mask[y, x]))
    return [i for _, i in cand[:k]]


def crafted_maps():
    rng = np.random.default_rng(5)
    h, w = 16, 24
    maps = []
    maps.append(rng.random((h, w), dtype=np.float32))                  # generic
    a = np.zeros((h, w), np.float32)                                    # exact ties inside and across windows
    a[3, 4] = a[3, 6] = a[5, 4] = 0.5
    a[10, 10] = a[10, 20] = a[15, 0] = 0.5
    a[0, 0] = a[0, 23] = a[15, 23] = 0.75                               # corners
    maps.append(a)
    b = np.full((h, w), 0.25, np.float32)                               # plateau with a bump and a zero region
    b[4:8, 8:12] = 0.0
    b[12, 2] = 0.3
    maps.append(b)
    c = rng.random((h, w), dtype=np.float32)                            # NaN pixels next to maxima
    c[2, 2] = np.nan
    c[8, 8] = np.nan
    c[8, 9] = 2.0
    c[0, 12] = np.nan
    maps.append(c)
    d = np.round(rng.random((h, w)) * 4).astype(np.float32) / 4         # many exact ties, zeros, border peaks
    maps.append(d)
    e = np.zeros((h, w), np.float32)                                    # nothing positive
    e[3, 3] = -1.0
    maps.append(e)
    f = rng.random((h, w), dtype=np.float32)                            # negative values and underflowed tiny values
    f[:, :5] = -f[:, :5]
    f[6, 6] = np.float32(1e-45)
    maps.append(f)
    return maps


@pytest.mark.parametrize("r", [0, 1, 3, 40])
def test_restatement_matches_brute_force(r):
    for i, H in enumerate(crafted_maps()):
        ref = brute_peaks(H, r)
        got = topk_ref.peaks(H, r)
        assert np.array_equal(got, ref), (i, r)
        for k in (1, 3, 64):
            assert list(topk_ref.peak_indices(H, r, k)) == brute_topk(H, r, k), (i, r, k)


def test_restatement_properties():
    rng = np.random.default_rng(9)
    for r in (0, 1, 2, 5):
        H = (rng.random((16, 24)) * 3).round().astype(np.float32) / 3
        idx = topk_ref.peak_indices(H, r, 64)
        ys, xs = idx // 24, idx % 24
        for i in range(len(idx)):   # any two peaks lie more than r apart
            for j in range(i + 1, len(idx)):
                assert max(abs(ys[i] - ys[j]), abs(xs[i] - xs[j])) > r
        if H.max() > 0:             # the first argmax is the strongest peak
            assert idx[0] == int(np.argmax(H))


def test_topk_rows_layout():
    H = np.zeros((2, 16, 24), np.float32)
    H[0, 2, 3] = 0.5
    H[0, 10, 20] = 0.25
    ori = np.zeros((2, 2, 16, 24), np.float32)
    ori[0, 0, 2, 3], ori[0, 1, 2, 3] = 0.6, -0.8
    rows = topk_ref.topk_rows(H, ori, 4, 1)
    assert rows.shape == (2, 4, 5)
    assert rows[0, 0, 0] == 2 * 24 + 3 and rows[0, 0, 1] == np.float32(0.5)
    assert rows[0, 0, 2] == np.float32(0.6) and rows[0, 0, 3] == np.float32(-0.8)
    assert 180 < rows[0, 0, 4] < 360
    assert rows[0, 1, 0] == 10 * 24 + 20
    assert (rows[0, 2:] == np.array([-1, 0, 0, 0, 0], np.float32)).all()
    assert (rows[1] == np.array([-1, 0, 0, 0, 0], np.float32)).all()


# ---- C ABI: argument checks before the handle is used -----------------------------------------------------------------

def test_null_and_range_arguments_return_einval(built_library):
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for fn in (lib.ccvpe_localize_topk, lib.ccvpe_localize_topk_cached):
        assert fn(None, p, 320, 640, p, 1, 8, 16, p, None) == EINVAL                 # null handle
        assert fn(None, None, 320, 640, p, 1, 8, 16, p, None) == EINVAL              # null ground input
        assert fn(None, p, 320, 640, None, 1, 8, 16, p, None) == EINVAL              # null aerial input / cache
        assert fn(None, p, 320, 640, p, 1, 8, 16, None, None) == EINVAL              # null rows
        assert b"rows" in lib.ccvpe_last_error()
        for k, r in ((0, 16), (65, 16), (-1, 0), (8, -1), (8, 33)):
            assert fn(p, p, 320, 640, p, 1, k, r, p, None) == EINVAL                 # (a bogus handle is never read)
            assert (b"k must" if not 1 <= k <= 64 else b"radius") in lib.ccvpe_last_error()
    f = lib.ccvpe_postprocess_topk
    assert f(None, p, p, 1, 8, 16, p, None) == EINVAL
    assert f(p, None, p, 1, 8, 16, p, None) == EINVAL
    assert f(p, p, None, 1, 8, 16, p, None) == EINVAL
    assert f(p, p, p, 1, 8, 16, None, None) == EINVAL
    for k, r in ((0, 0), (65, 0), (1, -1), (1, 33)):
        assert f(p, p, p, 1, k, r, p, None) == EINVAL
    assert f(p, p, p, 0, 8, 16, p, None) == EINVAL
    assert f(p, p, p, 4097, 8, 16, p, None) == EINVAL


# ---- model methods ----------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_VIGOR_ori_prior("cpu", 180.0, True)


def test_topk_methods_require_eval_mode():
    m = _model().train()
    g, s = torch.zeros(1, 3, 320, 640), torch.zeros(1, 3, 512, 512)
    with pytest.raises(RuntimeError, match="eval"):
        m.localize_topk(g, s, 8, 16)
    with pytest.raises(RuntimeError, match="eval"):
        m.localize_topk_cached(g, torch.zeros(16), 8, 16)
    with pytest.raises(RuntimeError, match="eval"):
        m.postprocess_topk(torch.zeros(1, 1, 512, 512), torch.zeros(1, 2, 512, 512), 8, 16)


def test_topk_methods_refuse_cpu_tensors():
    m = _model().eval()
    g, s = torch.zeros(1, 3, 320, 640), torch.zeros(1, 3, 512, 512)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.localize_topk(g, s, 8, 16)
    with pytest.raises(ValueError, match="cuda"):
        m.localize_topk_cached(g, torch.zeros(16), 8, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.postprocess_topk(torch.zeros(1, 1, 512, 512), torch.zeros(1, 2, 512, 512), 8, 16)
