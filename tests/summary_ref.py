"""float64 numpy restatement of the posterior summary (include/ccvpe.h): one row of 16 numbers per float32 map h of
512 x 512 values, x = index % 512 the column, y = index // 512 the row.

    0        argmax index: the first maximal index, NaN never wins, always a position inside the map
    1        h at the argmax
    2        S0 = sum h
    3        entropy -sum_{h>0} (h/S0) ln(h/S0), nats
    4, 5     mean x, y = sum h x / S0, sum h y / S0
    6, 7, 8  var_xx, cov_xy, var_yy about that mean
    9        sum of h over the window |x - x*| <= R, |y - y*| <= R around the argmax, clipped to the grid, over S0
    10, 11   mean x, y of the window, weights h over the window's own sum
    12 - 14  var_xx, cov_xy, var_yy of the window about its own mean
    15       cells of the clipped window

S0 == 0: (0, 0, 0, NaN ...).  The moments are taken about the mean (no cancellation), every sum is numpy's pairwise float64 sum."""
import numpy as np

HW = 512
N = HW * HW
COLS = 16
EXACT = (0, 1, 15)
MEANS = (4, 5, 10, 11)
COVS = (6, 7, 8, 12, 13, 14)
MASSES = (2, 9)
ENTROPY = 3


def _moments(h, x, y):
    """(sum, mean x, mean y, var_xx, cov_xy, var_yy) of the weights h (float64) at the coordinates x, y (broadcast against h)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = h.sum()
        mx, my = (h * x).sum() / s, (h * y).sum() / s
        dx, dy = x - mx, y - my
        return s, mx, my, (h * dx * dx).sum() / s, (h * dx * dy).sum() / s, (h * dy * dy).sum() / s


def summary(h, radius):
    """the row (float64 [16]) of one map h (float32, 512 * 512 values in any shape)"""
    f32 = np.ascontiguousarray(h, dtype=np.float32).reshape(HW, HW)
    flat = f32.reshape(-1)
    ok = ~np.isnan(flat)
    idx = int(np.argmax(np.where(ok, flat, -np.inf))) if ok.any() else 0
    hd = f32.astype(np.float64)
    x = np.arange(HW, dtype=np.float64)[None, :]
    y = np.arange(HW, dtype=np.float64)[:, None]
    row = np.full(COLS, np.nan)
    s0, mx, my, vxx, vxy, vyy = _moments(hd, x, y)
    row[0], row[1], row[2] = idx, flat[idx], s0
    if s0 == 0:
        return row
    with np.errstate(invalid="ignore", divide="ignore"):
        p = hd[hd > 0] / s0
        row[3] = -(p * np.log(p)).sum()
    row[4:9] = mx, my, vxx, vxy, vyy
    ys, xs = divmod(idx, HW)
    r = int(radius)
    y0, y1, x0, x1 = max(ys - r, 0), min(ys + r, HW - 1), max(xs - r, 0), min(xs + r, HW - 1)
    w0, wx, wy, wxx, wxy, wyy = _moments(hd[y0:y1 + 1, x0:x1 + 1], x[:, x0:x1 + 1], y[y0:y1 + 1, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        row[9] = w0 / s0
    row[10:15] = wx, wy, wxx, wxy, wyy
    row[15] = (y1 - y0 + 1) * (x1 - x0 + 1)
    return row


def summaries(maps, radius):
    """[B, 16] float64 of maps [B, 512, 512]"""
    return np.stack([summary(m, radius) for m in np.asarray(maps)])


def assert_rows_close(got, ref, what=""):
    """A device summary (float32 [B, 16]) against the restatement (float64 [B, 16]).  Tolerances from the formats, not from the device:
    columns 0, 1, 15 exact; the means within 1e-4 cells; the (co)variances within 1e-5 * max(|ref|, 1) (float64 sums good to ~3e-11
    relative, the cancellation in sum / S0 - mean^2 leaves ~3e-5 absolute at worst before the float32 rounding of 6e-8 relative); S0 and
    the peak mass within 1e-6 relative; the entropy within 1e-4 (a float32 logarithm is off by at most ~88 * 2^-23 for the smallest
    normal h, and the weights sum to 1).  NaN exactly where the restatement has NaN."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and got.shape[-1] == COLS, (got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN pattern\n{got}\n{ref}")
    for c in EXACT:
        np.testing.assert_array_equal(got[..., c], ref[..., c].astype(np.float32).astype(np.float64), err_msg=f"{what}: column {c}")
    live = ~np.isnan(ref)
    err = np.where(live, np.abs(got - ref), 0.0)
    tol = np.zeros_like(ref)
    tol[..., list(MEANS)] = 1e-4
    tol[..., list(COVS)] = 1e-5 * np.maximum(np.abs(np.nan_to_num(ref[..., list(COVS)])), 1.0)
    tol[..., list(MASSES)] = 1e-6 * np.abs(np.nan_to_num(ref[..., list(MASSES)]))
    tol[..., ENTROPY] = 1e-4
    ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)
    worst = {c: float(ratio[..., c].max()) for c in range(COLS) if c not in EXACT and live[..., c].any()}
    print(f"{what}: worst error / bound per column = " + ", ".join(f"{c}: {v:.3g}" for c, v in worst.items()))
    bad = err > tol
    for c in EXACT:
        bad[..., c] = False
    assert not bad.any(), f"{what}: columns {sorted(set(np.nonzero(bad)[-1].tolist()))} miss their bounds\n got {got[bad]}\n ref {ref[bad]}\n tol {tol[bad]}"


def delta(*cells, value=1.0):
    """a map that is `value` at the cells (x, y) and 0 elsewhere"""
    m = np.zeros((HW, HW), np.float32)
    for x, y in cells:
        m[y, x] = value
    return m


def crafted_maps():
    """name -> float32 [512, 512]: the maps of the closed forms (tests/test_summary_cpu.py), a discretised Gaussian whose window the
    border clips and a positive random map that does not sum to 1"""
    yy, xx = np.mgrid[0:HW, 0:HW].astype(np.float64)
    gauss = np.exp(-0.5 * ((xx - 509.0) ** 2 + (yy - 2.0) ** 2) / 9.0)
    rng = np.random.default_rng(41)
    return {
        "delta_origin": delta((0, 0)),
        "delta_corner": delta((511, 511)),
        "delta_inside": delta((200, 300)),
        "uniform": np.full((HW, HW), 1.0 / N, np.float32),
        "two_deltas": delta((150, 77), (250, 77), value=0.5),
        "two_deltas_scaled": delta((150, 77), (250, 77), value=0.5) * np.float32(3.5),
        "gauss_border": (gauss / gauss.sum()).astype(np.float32),
        "random": rng.uniform(0.05, 1.0, size=(HW, HW)).astype(np.float32),
        "gauss_centre": np.exp(-0.5 * ((xx - 255.3) ** 2 / 16.0 + (yy - 300.8) ** 2 / 400.0)).astype(np.float32),
    }
