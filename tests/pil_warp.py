"""numpy restatement of the Pillow resamplings in front of the KITTI and Oxford test loops - TEST INFRASTRUCTURE, NOT PRODUCT.

The datasets call Pillow (reference datasets.py:577-598 KITTI: Image.rotate, Image.transform(AFFINE, BILINEAR),
TF.center_crop; datasets.py:306-321 Oxford: Image.crop + Resize).  Pillow's libImaging/Geometry.c, for an RGB image:

  NEAREST affine (affine_fixed), 16.16 fixed point with FIX(v) = floor(v * 65536 + 0.5):
      A0, A1, A3, A4 = FIX(m0), FIX(m1), FIX(m3), FIX(m4);  A2 = FIX(m2 + m0*0.5 + m1*0.5);  A5 = FIX(m5 + m3*0.5 + m4*0.5)
      out[y, x] = in[(A5 + x*A3 + y*A4) >> 16, (A2 + x*A0 + y*A1) >> 16], 0 outside the canvas
  BILINEAR affine (generic transform, double):
      xin = m0*(x+.5) + m1*(y+.5) + m2, yin = m3*(x+.5) + m4*(y+.5) + m5;  0 unless 0 <= xin < W and 0 <= yin < H
      xin -= .5; yin -= .5; xf, yf = floor; dx, dy = fractions; columns clamp(xf), clamp(xf+1)
      v1 = a + (b - a)*dx on row clamp(yf); v2 likewise on row yf+1, or v2 = v1 when that row is outside; v = v1 + (v2-v1)*dy
      out = (uint8)v (truncation)

tests/test_aerial_prep_cpu.py pins both against live Pillow and against tests/golden/aerial_prep.npz (written by
tools/make_aerial_golden.py with Pillow itself); the GPU tests then hold the kernels to this file.
"""
from __future__ import annotations

import numpy as np

NEAREST, BILINEAR = 0, 2


def _fix(v: float) -> int:
    return int(np.floor(v * 65536.0 + 0.5))


def affine_nearest(img: np.ndarray, m) -> np.ndarray:
    """img.transform(img.size, AFFINE, m, NEAREST) for uint8 [H, W, 3]."""
    H, W = img.shape[:2]
    m = [float(v) for v in m]
    a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
    a2 = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    xi, yi = np.broadcast_arrays((a2 + x * a0 + y * a1) >> 16, (a5 + x * a3 + y * a4) >> 16)
    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    out = np.zeros_like(img)
    out[ok] = img[yi[ok], xi[ok]]
    return out


def affine_bilinear(img: np.ndarray, m) -> np.ndarray:
    """img.transform(img.size, AFFINE, m, BILINEAR) for uint8 [H, W, 3]."""
    H, W = img.shape[:2]
    m = [float(v) for v in m]
    xo = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yo = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = m[0] * xo + m[1] * yo + m[2]
    yin = m[3] * xo + m[4] * yo + m[5]
    xin, yin = np.broadcast_arrays(xin, yin)
    ok = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin = xin[ok] - 0.5
    yin = yin[ok] - 0.5
    xf = np.floor(xin).astype(np.int64)
    yf = np.floor(yin).astype(np.int64)
    dx = (xin - xf)[:, None]
    dy = (yin - yf)[:, None]
    x0 = np.clip(xf, 0, W - 1)
    x1 = np.clip(xf + 1, 0, W - 1)
    y0 = np.clip(yf, 0, H - 1)
    src = img.astype(np.float64)
    a, b = src[y0, x0], src[y0, x1]
    v1 = a + (b - a) * dx
    has2 = (yf + 1 < H)
    y1 = np.where(has2, yf + 1, 0)
    a2, b2 = src[y1, x0], src[y1, x1]
    v2 = np.where(has2[:, None], a2 + (b2 - a2) * dx, v1)
    out = np.zeros_like(img)
    out[ok] = (v1 + (v2 - v1) * dy).astype(np.uint8)
    return out


def chain(img: np.ndarray, matrices, filters) -> np.ndarray:
    """Stages in order, uint8 between them."""
    for m, f in zip(matrices, filters):
        img = affine_nearest(img, m) if f == NEAREST else affine_bilinear(img, m)
    return img


def crop(img: np.ndarray, top: int, left: int, h: int, w: int) -> np.ndarray:
    """PIL.Image.crop((left, top, left + w, top + h)): zeros where the box leaves the image."""
    out = np.zeros((h, w) + img.shape[2:], dtype=img.dtype)
    H, W = img.shape[:2]
    y0, y1 = max(top, 0), min(top + h, H)
    x0, x1 = max(left, 0), min(left + w, W)
    if y1 > y0 and x1 > x0:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = img[y0:y1, x0:x1]
    return out
