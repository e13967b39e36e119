"""Aerial-side input preparation of the KITTI and Oxford test loops on device.

The datasets prepare the aerial image with Pillow on the host (reference datasets.py:306-321 Oxford, datasets.py:577-598 KITTI) and
build a 512 x 512 float32 Gaussian ground-truth map per sample only for the test loop to take its argmax (train_KITTI.py:312,
train_OxfordRobotCar.py:220).  This module restates the dataset arithmetic - the parameters of every Pillow call, the crop
boxes, the ground-truth offsets and orientation - and hands the pixel work to ccvpe_preprocess_affine /
ccvpe_preprocess_window_resize, whose output equals the reference's satmap tensor bit for bit.  The ground-truth helpers return
exactly what the test loop reads off the maps: the flat argmax index (ties broken as np.argmax does), the (cos, sin) at that pixel
and the heading in degrees, ready for `model.evaluate`.

Host scalars follow the reference's own operations (Python floats, np.cos / np.sin, Python's round), so they are the same doubles.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

from . import _lib

SAT_HW = 512                       # SatMap_process_sidelength (datasets.py:359) = Resize([512, 512]) of the Oxford transform
NEAREST, BILINEAR = 0, 2           # PIL.Image.NEAREST / BILINEAR = CCVPE_RESAMPLE_*

# KITTI (datasets.py:355-374)
DEFAULT_LAT = 49.015
SATMAP_ZOOM = 18
CAMERA_GPS_SHIFT_LEFT = (1.08, 0.26)
KITTI_FILTERS = (NEAREST, BILINEAR, BILINEAR, NEAREST)

# Oxford (datasets.py:306-321): 800 x 800 windows on a 400-px grid
OXFORD_GRID = 400
OXFORD_WIN = 800


def get_meter_per_pixel(lat: float = DEFAULT_LAT, zoom: int = SATMAP_ZOOM, scale: float = 1.0) -> float:
    """datasets.py:366-371; the datasets use scale=1 (datasets.py:375, 459)."""
    meter_per_pixel = 156543.03392 * np.cos(lat * np.pi / 180.) / (2 ** zoom)
    meter_per_pixel /= 2
    meter_per_pixel /= scale
    return meter_per_pixel


def rotate_matrix(angle_deg: float, width: int, height: int) -> Tuple[float, ...]:
    """The affine `data` PIL.Image.rotate(angle_deg) passes to Image.transform with default arguments (NEAREST, centre
    (w/2, h/2), no translation, no expand).  Its shortcuts (copy at 0, transposes at 180 and at 90/270 on square images) give the
    same bytes as the fixed-point NEAREST path fed this matrix."""
    angle = angle_deg % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = width / 2.0, height / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def center_crop_box(height: int, width: int, size: int = SAT_HW) -> Tuple[int, int]:
    """torchvision center_crop on a PIL image: (top, left) = (int(round((H - size) / 2.0)), int(round((W - size) / 2.0)))."""
    return int(round((height - size) / 2.0)), int(round((width - size) / 2.0))


def _vec(v, n=None) -> np.ndarray:
    a = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return a if n is None else np.broadcast_to(a, (n,))


def kitti_matrices(heading_rad, gt_shift_x, gt_shift_y, theta, tile_hw: Sequence[int], shift_range_lat: float = 20,
                   shift_range_lon: float = 20, rotation_range: float = 10) -> Tuple[np.ndarray, Tuple[int, ...]]:
    """The four Pillow calls of SatGrdDatasetTest.__getitem__ (datasets.py:577-594) as affine `data` tuples, per sample.

    heading_rad: oxts field 5; gt_shift_x, gt_shift_y, theta: the test-split file's values AS READ (the dataset negates the shifts
    itself, datasets.py:585-586); tile_hw: the satellite tile's (H, W).  shift_range_* / rotation_range are the dataset's
    constructor arguments (train_KITTI.py passes its --shift_range_lat/lon and --rotation_range).  Returns (matrices [B,4,6]
    float64, filters): rotate(-heading), camera-GPS shift (BILINEAR), ground-truth shift (BILINEAR), rotate(theta * range)."""
    heading = _vec(heading_rad)
    B = heading.shape[0]
    sx, sy, th = _vec(gt_shift_x, B), _vec(gt_shift_y, B), _vec(theta, B)
    H, W = int(tile_hw[0]), int(tile_hw[1])
    mpp = get_meter_per_pixel(scale=1)
    pix_lat = shift_range_lat / mpp
    pix_lon = shift_range_lon / mpp
    cam = (1, 0, CAMERA_GPS_SHIFT_LEFT[0] / mpp, 0, 1, CAMERA_GPS_SHIFT_LEFT[1] / mpp)
    out = np.empty((B, 4, 6), dtype=np.float64)
    for b in range(B):
        shift_x = -float(sx[b])
        shift_y = -float(sy[b])
        out[b, 0] = rotate_matrix(-float(heading[b]) / np.pi * 180, W, H)
        out[b, 1] = cam
        out[b, 2] = (1, 0, shift_x * pix_lon, 0, 1, -shift_y * pix_lat)
        out[b, 3] = rotate_matrix(float(th[b]) * rotation_range, W, H)
    return out, KITTI_FILTERS


def kitti_aerial(sat_u8, heading_rad, gt_shift_x, gt_shift_y, theta, shift_range_lat: float = 20, shift_range_lon: float = 20,
                 rotation_range: float = 10, mean=_lib.IMAGENET_MEAN, std=_lib.IMAGENET_STD):
    """uint8 satellite tiles [B,H,W,3] (cuda, as decoded, H and W >= 512) -> the KITTI test split's `sat_map` tensor [B,3,512,512]
    (datasets.py:577-598 + satmap_transform, train_KITTI.py:60-64), in one launch."""
    H, W = int(sat_u8.shape[1]), int(sat_u8.shape[2])
    mats, filters = kitti_matrices(heading_rad, gt_shift_x, gt_shift_y, theta, (H, W), shift_range_lat, shift_range_lon, rotation_range)
    top, left = center_crop_box(H, W)
    return _lib.preprocess_affine(sat_u8, mats, filters, (top, left, SAT_HW, SAT_HW), mean, std)


def gt_argmax(x_offset: int, y_offset: int, size: int = SAT_HW) -> int:
    """Flat index of np.argmax of the reference's float32 Gaussian map, built from
    np.meshgrid(np.linspace(-256 + x_offset, 256 + x_offset, 512), np.linspace(-256 + y_offset, 256 + y_offset, 512)),
    d = sqrt(x^2 + y^2), exp(-(d^2) / 32) (datasets.py:323-329, 600-606), without building it: the map falls off with |x| and |y|
    separately, so the maximum lies at the grid line nearest 0 of each axis; the 3 x 3 window around it is evaluated with the
    reference's formula and scanned in np.argmax's order, which settles exact ties (offset 0 puts two lines at +-256/511).
    Offsets beyond +-255 (peak off the map) are refused."""
    xo, yo = int(x_offset), int(y_offset)
    half = size // 2
    if abs(xo) > half - 1 or abs(yo) > half - 1:
        raise ValueError(f"ground-truth offset ({xo}, {yo}) outside +-{half - 1}: the Gaussian's peak is not on the map")
    xs = np.linspace(-half + xo, half + xo, size)
    ys = np.linspace(-half + yo, half + yo, size)
    cx, cy = int(np.argmin(np.abs(xs))), int(np.argmin(np.abs(ys)))
    cols = np.arange(max(cx - 1, 0), min(cx + 2, size))
    rows = np.arange(max(cy - 1, 0), min(cy + 2, size))
    x, y = np.meshgrid(xs[cols], ys[rows])
    d = np.sqrt(x * x + y * y)
    sigma, mu = 4, 0.0
    g = np.exp(-((d - mu) ** 2 / (2.0 * sigma ** 2))).astype(np.float32)
    k = int(np.argmax(g))
    return int(rows[k // len(cols)]) * size + int(cols[k % len(cols)])


def _cos_sin_f32(angle_deg: np.ndarray) -> np.ndarray:
    """torch.full([2, H, W], np.cos(a * np.pi / 180)) + [1] = np.sin(...): the float32 values the test loop reads at the GT pixel."""
    out = np.empty((len(angle_deg), 2), dtype=np.float32)
    for b, a in enumerate(angle_deg):                  # scalar calls, as the dataset makes them
        out[b] = (np.cos(float(a) * np.pi / 180), np.sin(float(a) * np.pi / 180))
    return out


def kitti_ground_truth(gt_shift_x, gt_shift_y, theta, shift_range_lat: float = 20, shift_range_lon: float = 20,
                       rotation_range: float = 10) -> Dict[str, np.ndarray]:
    """Ground-truth side of a KITTI test sample (datasets.py:600-634) from the split file's values as read: gt_index [B] int32 =
    flat argmax of `gt`, gt_cos_sin [B,2] float32 = `orientation_map` at that pixel, heading_deg [B] float64 =
    `orientation_angle`.  With meter_per_pixel = get_meter_per_pixel(scale=1) these are the arguments of model.evaluate."""
    sx, sy, th = _vec(gt_shift_x), _vec(gt_shift_y), _vec(theta)
    B = max(sx.shape[0], sy.shape[0], th.shape[0])
    sx, sy, th = np.broadcast_to(sx, (B,)), np.broadcast_to(sy, (B,)), np.broadcast_to(th, (B,))
    mpp = get_meter_per_pixel(scale=1)
    pix_lat = shift_range_lat / mpp
    pix_lon = shift_range_lon / mpp
    idx = np.empty(B, dtype=np.int32)
    heading = np.empty(B, dtype=np.float64)
    for b in range(B):
        shift_x = -float(sx[b])
        shift_y = -float(sy[b])
        random_ori = float(th[b]) * rotation_range
        x_offset = int(shift_x * pix_lon * np.cos(random_ori / 180 * np.pi) - shift_y * pix_lat * np.sin(random_ori / 180 * np.pi))
        y_offset = int(-shift_y * pix_lat * np.cos(random_ori / 180 * np.pi) - shift_x * pix_lon * np.sin(random_ori / 180 * np.pi))
        idx[b] = gt_argmax(x_offset, y_offset)
        orientation_angle = 90 - random_ori
        if orientation_angle < 0:
            orientation_angle = orientation_angle + 360
        elif orientation_angle > 360:
            orientation_angle = orientation_angle - 360
        heading[b] = orientation_angle
    return {"gt_index": idx, "gt_cos_sin": _cos_sin_f32(heading), "heading_deg": heading}


def oxford_window(image_coord) -> Dict[str, np.ndarray]:
    """Test / val window of OxfordRobotCarDataset (datasets.py:306-321) for pixel coordinates image_coord [B,2] = (col, row):
    origin [B,2] int32 = (x0, y0) of the 800 x 800 crop box on the 400-px grid, offset [B,2] int = (col_offset_resized,
    row_offset_resized) of the ground-truth Gaussian."""
    ic = np.asarray(image_coord, dtype=np.float64).reshape(-1, 2)
    B = ic.shape[0]
    origin = np.empty((B, 2), dtype=np.int32)
    offset = np.empty((B, 2), dtype=np.int64)
    for b in range(B):
        col_split = int((ic[b, 0]) // OXFORD_GRID)
        if np.round(ic[b, 0] - OXFORD_GRID * col_split) < 200:
            col_split -= 1
        col_pixel = int(np.round(ic[b, 0] - OXFORD_GRID * col_split))
        row_split = int((ic[b, 1]) // OXFORD_GRID)
        if np.round(ic[b, 1] - OXFORD_GRID * row_split) < 200:
            row_split -= 1
        row_pixel = int(np.round(ic[b, 1] - OXFORD_GRID * row_split))
        origin[b] = (col_split * OXFORD_GRID, row_split * OXFORD_GRID)
        offset[b] = (int(-(col_pixel / 800 * 512 - 256)), int(-(row_pixel / 800 * 512 - 256)))
    return {"origin": origin, "offset": offset}


def oxford_aerial(map_u8, image_coords, mean=_lib.IMAGENET_MEAN, std=_lib.IMAGENET_STD):
    """The resident satellite map [map_h,map_w,3] (cuda uint8) -> the Oxford test split's `sat` tensors [B,3,512,512] for ground
    images at image_coords [B,2] (datasets.py:306-321 crop + transform_sat, train_OxfordRobotCar.py:56-60), in two launches."""
    win = oxford_window(image_coords)
    return _lib.preprocess_window_resize(map_u8, win["origin"], (OXFORD_WIN, OXFORD_WIN), (SAT_HW, SAT_HW), mean, std)


def oxford_tiles(image_coords) -> Dict[str, np.ndarray]:
    """The distinct test windows of a batch of ground images at image_coords [B,2]: origin [T,2] int32 = the crop origins of
    oxford_window in order of first appearance, tile_index [B] int32 with origin[tile_index] == oxford_window(image_coords)["origin"].
    A sequential drive (the test loader does not shuffle, train_OxfordRobotCar.py:81-83) visits a handful of tiles per batch: encode
    oxford_tile_aerial(map_u8, origin) once and pass tile_index to the model's cached calls."""
    win = oxford_window(image_coords)["origin"]
    seen: Dict[Tuple[int, int], int] = {}
    index = np.empty(win.shape[0], dtype=np.int32)
    for b, (x0, y0) in enumerate(win):
        index[b] = seen.setdefault((int(x0), int(y0)), len(seen))
    origin = np.array(list(seen), dtype=np.int32).reshape(-1, 2)
    return {"origin": origin, "tile_index": index}


def oxford_tile_aerial(map_u8, origins, mean=_lib.IMAGENET_MEAN, std=_lib.IMAGENET_STD):
    """The resident satellite map [map_h,map_w,3] (cuda uint8) -> the `sat` tensors [T,3,512,512] of the 800 x 800 windows at crop
    origins [T,2] = (x0, y0) (oxford_tiles), in two launches: the second half of oxford_aerial, once per distinct tile."""
    org = np.asarray(origins, dtype=np.int32).reshape(-1, 2)
    return _lib.preprocess_window_resize(map_u8, org, (OXFORD_WIN, OXFORD_WIN), (SAT_HW, SAT_HW), mean, std)


def _axis_gap(p: float, lo: float, hi: float) -> Tuple[float, bool]:
    """Distance from p to the half-open interval [lo, hi), and whether it is measured to the excluded end."""
    if p < lo:
        return lo - p, False
    if p >= hi:
        return p - hi, True
    return 0.0, False


def oxford_region(prior_coords, radius_px: float) -> Dict[str, object]:
    """The Oxford test windows around position priors: for each prior (col, row) in prior_coords [B,2], the 800 x 800 windows on the
    400-px grid whose central 400 x 400 cell [x0+200, x0+600) x [y0+200, y0+600) meets the closed disc of radius_px around it - the
    windows oxford_window picks for the points of that disc.  oxford_window rounds the position to the nearest pixel (half to even),
    so the cell of window x0 is [x0+199.5, x0+599.5) in map coordinates.  Returns origin [T,2] int32 = the distinct windows in order
    of first appearance (queries in order, each query's windows row-major), and tiles = one list of tile ids per prior, the form
    model.localize_region takes.  radius_px = 0 gives oxford_tiles' windows."""
    pc = np.asarray(prior_coords, dtype=np.float64).reshape(-1, 2)
    r = float(radius_px)
    if not r >= 0.0 or not np.isfinite(r):
        raise ValueError(f"radius_px must be a finite non-negative number, got {radius_px}")
    if not np.isfinite(pc).all():
        raise ValueError("prior_coords must be finite")
    seen: Dict[Tuple[int, int], int] = {}
    tiles = []
    for px, py in pc:
        own = []
        ys = range(int(np.floor((py - r - 599.5) / OXFORD_GRID)), int(np.floor((py + r - 199.5) / OXFORD_GRID)) + 1)
        xs = range(int(np.floor((px - r - 599.5) / OXFORD_GRID)), int(np.floor((px + r - 199.5) / OXFORD_GRID)) + 1)
        for ry in ys:
            y0 = ry * OXFORD_GRID
            gy, oy = _axis_gap(py, y0 + 199.5, y0 + 599.5)
            for rx in xs:
                x0 = rx * OXFORD_GRID
                gx, ox = _axis_gap(px, x0 + 199.5, x0 + 599.5)
                d2 = gx * gx + gy * gy
                if d2 < r * r or (d2 == r * r and not (ox or oy)):
                    own.append(seen.setdefault((x0, y0), len(seen)))
        tiles.append(own)
    origin = np.array(list(seen), dtype=np.int32).reshape(-1, 2)
    return {"origin": origin, "tiles": tiles}


_OXFORD_CENTRE = None


def _oxford_index_centre() -> np.ndarray:
    """[512] window coordinate of each heatmap column: the centre of the window pixels whose ground-truth column (oxford_window's
    offset -> gt_argmax) it is.  The construction is many-to-one (an offset step is 800/512 window pixels, and two offsets share the
    centre column 255); columns no window pixel maps to are interpolated."""
    global _OXFORD_CENTRE
    if _OXFORD_CENTRE is None:
        lo = np.full(SAT_HW, np.inf)
        hi = np.full(SAT_HW, -np.inf)
        for cp in range(1, OXFORD_WIN):   # (window pixel 0 puts the peak off the map)
            col = gt_argmax(int(-(cp / 800 * 512 - 256)), 0) % SAT_HW
            lo[col] = min(lo[col], cp)
            hi[col] = max(hi[col], cp)
        hit = np.isfinite(lo)
        cols = np.arange(SAT_HW)
        centre = np.interp(cols, cols[hit], (lo[hit] + hi[hit]) / 2)
        # beyond the first / last hit column: the linear scale of the grid
        centre[cols < cols[hit][0]] = cols[cols < cols[hit][0]] * OXFORD_WIN / (SAT_HW - 1)
        centre[cols > cols[hit][-1]] = cols[cols > cols[hit][-1]] * OXFORD_WIN / (SAT_HW - 1)
        _OXFORD_CENTRE = centre
    return _OXFORD_CENTRE


def oxford_region_to_map(origin, index) -> np.ndarray:
    """A flat 512 x 512 heatmap index in the window at origin (x0, y0) -> map pixel coordinates (col, row) float64, the inverse of
    the test split's ground-truth construction (datasets.py:315-329): the centre of the map pixels whose ground-truth index it is.
    origin [2] or [B,2], index scalar or [B]; returns [B,2] (or [2] for one scalar index).  The round trip from a position to its
    ground-truth index and back is within 800/512 px, and within 2.5 px on the window's centre column / row, which two
    ground-truth offsets share."""
    idx = np.asarray(index)
    scalar = idx.ndim == 0
    idx = idx.reshape(-1).astype(np.int64)
    if ((idx < 0) | (idx >= SAT_HW * SAT_HW)).any():
        raise ValueError("heatmap index outside 0 .. 512*512-1")
    org = np.broadcast_to(np.asarray(origin, dtype=np.float64).reshape(-1, 2), (idx.shape[0], 2))
    centre = _oxford_index_centre()
    out = np.stack([org[:, 0] + centre[idx % SAT_HW], org[:, 1] + centre[idx // SAT_HW]], axis=1)
    return out[0] if scalar else out


def _sigma(sigma_px, n: int) -> np.ndarray:
    sig = np.broadcast_to(np.asarray(sigma_px, dtype=np.float64).reshape(-1), (n,)).copy()
    if not (np.isfinite(sig).all() and (sig > 0).all()):
        raise ValueError(f"sigma_px must be finite and positive, got {sigma_px}")
    return sig


def gaussian_log_prior(center_px, sigma_px, device):
    """Isotropic Gaussian log-priors in the output-map frame (the localize_prior / postprocess_prior input): float32 [B,512,512] with
    -0.5 * ((x - cx)^2 + (y - cy)^2) / sigma^2 at column x, row y, for centres center_px [B,2] = (cx, cy) in output pixels (a GNSS fix,
    the previous pose plus odometry) and sigma_px a scalar or [B].  Evaluated in float64, rounded once to float32."""
    import torch
    c = np.asarray(center_px, dtype=np.float64).reshape(-1, 2)
    if not np.isfinite(c).all():
        raise ValueError("center_px must be finite")
    sig = _sigma(sigma_px, c.shape[0])
    t = torch.arange(SAT_HW, dtype=torch.float64, device=device)
    cx = torch.as_tensor(c[:, 0], device=device)[:, None, None]
    cy = torch.as_tensor(c[:, 1], device=device)[:, None, None]
    s2 = torch.as_tensor(sig * sig, device=device)[:, None, None]
    return (-0.5 * ((t[None, None, :] - cx) ** 2 + (t[None, :, None] - cy) ** 2) / s2).to(torch.float32).contiguous()


def oxford_log_prior(origin, prior_coords, sigma_px, device):
    """Per-pair log-priors for localize_region_prior on the Oxford windows: float32 [P,512,512], for window origins origin [P,2] = (x0, y0)
    and map positions prior_coords [P,2] = (col, row) (either may be one row for all pairs), the Gaussian
    -0.5 * ((X - px)^2 + (Y - py)^2) / sigma^2 in MAP pixels at each heatmap pixel's map position (X, Y) = oxford_region_to_map(origin,
    index).  One scale across windows: pairs of one query compare through it (ccvpe_localize_region_prior)."""
    import torch
    org = np.asarray(origin, dtype=np.float64).reshape(-1, 2)
    pc = np.asarray(prior_coords, dtype=np.float64).reshape(-1, 2)
    P = max(org.shape[0], pc.shape[0])
    org, pc = np.broadcast_to(org, (P, 2)).copy(), np.broadcast_to(pc, (P, 2)).copy()
    if not (np.isfinite(org).all() and np.isfinite(pc).all()):
        raise ValueError("origin and prior_coords must be finite")
    sig = _sigma(sigma_px, P)
    centre = torch.as_tensor(_oxford_index_centre(), dtype=torch.float64, device=device)
    col = torch.as_tensor(org[:, 0], device=device)[:, None] + centre[None, :]   # [P, 512] map column of each heatmap column
    row = torch.as_tensor(org[:, 1], device=device)[:, None] + centre[None, :]   # [P, 512] map row of each heatmap row
    dx = col - torch.as_tensor(pc[:, 0], device=device)[:, None]
    dy = row - torch.as_tensor(pc[:, 1], device=device)[:, None]
    s2 = torch.as_tensor(sig * sig, device=device)[:, None, None]
    return (-0.5 * (dx[:, None, :] ** 2 + dy[:, :, None] ** 2) / s2).to(torch.float32).contiguous()


def oxford_ground_truth(image_coords, yaw) -> Dict[str, np.ndarray]:
    """Ground-truth side of an Oxford test sample (datasets.py:323-351): gt_index [B] int32 = flat argmax of `gt`, gt_cos_sin [B,2]
    float32 = `orientation` at that pixel, heading_deg [B] float64 = `orientation_angle` (yaw: grdYaw, radians)."""
    win = oxford_window(image_coords)
    yaw = _vec(yaw, win["origin"].shape[0])
    B = yaw.shape[0]
    idx = np.empty(B, dtype=np.int32)
    heading = np.empty(B, dtype=np.float64)
    for b in range(B):
        col_off, row_off = (int(v) for v in win["offset"][b])
        idx[b] = gt_argmax(col_off, row_off)
        orientation_angle = (float(yaw[b]) / np.pi * 180) - 90
        if orientation_angle < 0:
            orientation_angle = orientation_angle + 360
        heading[b] = orientation_angle
    return {"gt_index": idx, "gt_cos_sin": _cos_sin_f32(heading), "heading_deg": heading}


# ---- posterior summary ------------------------------------------------------------------------------------------

# the 16 columns of model.localize_summary's / belief_summary's rows, in order (include/ccvpe.h): positions in cells of the 512 grid
SUMMARY_FIELDS = ("index", "prob", "mass", "entropy", "mean_x", "mean_y", "var_xx", "cov_xy", "var_yy",
                  "peak_mass", "peak_mean_x", "peak_mean_y", "peak_var_xx", "peak_cov_xy", "peak_var_yy", "peak_cells")
_SUMMARY_LENGTHS = (4, 5, 10, 11)
_SUMMARY_AREAS = (6, 7, 8, 12, 13, 14)


def summary_to_metres(summary, metres_per_px):
    """Summary rows [..., 16] (a tensor or an array) with the means in metres and the (co)variances in square metres: metres_per_px
    is the ground size of one cell of the 512 grid, a number or one per row ([B]; KITTI / Oxford: their map resolution times the
    resize factor, VIGOR: the tile's).  The four means scale by it, the six (co)variances by its square; index, prob, mass,
    entropy, peak_mass and peak_cells are unchanged.  The means stay relative to the centre of cell (0, 0)."""
    import torch
    if isinstance(summary, torch.Tensor):
        out = summary.clone()
        f = torch.as_tensor(metres_per_px, dtype=out.dtype, device=out.device)
    else:
        out = np.array(summary, dtype=np.float64 if np.asarray(summary).dtype == np.float64 else np.float32)
        f = np.asarray(metres_per_px, dtype=out.dtype)
    if out.shape[-1] != len(SUMMARY_FIELDS):
        raise ValueError(f"summary must be [..., {len(SUMMARY_FIELDS)}], got {tuple(out.shape)}")
    if f.ndim > 0:
        f = f.reshape(tuple(f.shape) + (1,))
    for cols, g in ((_SUMMARY_LENGTHS, f), (_SUMMARY_AREAS, f * f)):
        out[..., list(cols)] = out[..., list(cols)] * g
    return out


# ---- credible regions -------------------------------------------------------------------------------------------

# the columns of model.belief_credible's / localize_credible's cred rows (include/ccvpe.h): four per query, then three per level
CREDIBLE_HEAD_FIELDS = ("mass", "positive_cells", "probe_mass_above", "probe_rank")
CREDIBLE_LEVEL_FIELDS = ("threshold", "cells", "mass_share")


def _credible_cols(cred):
    n = cred.shape[-1]
    if n < 7 or (n - len(CREDIBLE_HEAD_FIELDS)) % len(CREDIBLE_LEVEL_FIELDS) != 0:
        raise ValueError(f"cred must be [..., 4 + 3 L] with L >= 1, got {tuple(cred.shape)}")
    return (n - len(CREDIBLE_HEAD_FIELDS)) // len(CREDIBLE_LEVEL_FIELDS)


def credible_to_metres(cred, metres_per_px):
    """cred rows [..., 4 + 3 L] (a tensor or an array) with every level's area in square metres: metres_per_px is the ground size
    of one cell of the 512 grid, a number or one per row ([B], as summary_to_metres takes it).  The "cells" column of every level
    scales by its square; every other column - the counts of the head among them - is unchanged."""
    import torch
    if isinstance(cred, torch.Tensor):
        out = cred.clone()
        f = torch.as_tensor(metres_per_px, dtype=out.dtype, device=out.device)
    else:
        out = np.array(cred, dtype=np.float64 if np.asarray(cred).dtype == np.float64 else np.float32)
        f = np.asarray(metres_per_px, dtype=out.dtype)
    L = _credible_cols(out)
    if f.ndim > 0:
        f = f.reshape(tuple(f.shape) + (1,))
    cols = [5 + 3 * j for j in range(L)]
    out[..., cols] = out[..., cols] * (f * f)
    return out


def credible_contains(cred, levels) -> np.ndarray:
    """Whether each query's probe cell lies in the region of each level: bool [..., L] from cred rows [..., 4 + 3 L'] of a call with
    a probe and any levels p - the rule above < T(p) of include/ccvpe.h, evaluated in float64 from the columns "mass" and
    "probe_mass_above": T = ceil(p Q), raised to 1 and capped at Q, Q = mass * 2^44.  The columns are float32 roundings of Q and of
    above / Q, so a probe within 2^-23 of a level's boundary may fall on either side; the device's own rule, from the exact
    integers, is the level map.  False where the probe columns are NaN (no probe, a bad index, an empty map)."""
    c = np.asarray(cred.detach().cpu() if hasattr(cred, "detach") else cred, dtype=np.float64)
    _credible_cols(c)
    p = np.atleast_1d(np.asarray(levels, dtype=np.float32)).astype(np.float64)
    if p.ndim != 1 or not (np.isfinite(p) & (p > 0) & (p <= 1)).all():
        raise ValueError(f"levels must be numbers in (0, 1], got {p.tolist()}")
    Q = c[..., 0:1] * 2.0 ** 44
    above = c[..., 2:3] * Q
    T = np.minimum(np.maximum(np.ceil(p * Q), 1.0), Q)
    with np.errstate(invalid="ignore"):
        return (above < T) & (Q > 0)


def _step_result(model, rows, summary, heading, belief, levels):
    """what a tracker step returns: rows alone, or (rows, summary if any, heading and hist if any, belief_credible's cred of the
    stored belief if levels are given)"""
    out = (rows,) + (() if summary is None else (summary,)) + (() if heading is None else tuple(heading))
    if levels is not None:
        out += (model.belief_credible(belief, levels),)
    return out[0] if len(out) == 1 else out


# ---- heading posterior ------------------------------------------------------------------------------------------

# the 12 columns of model.localize_heading's heading rows, in order (include/ccvpe.h): angles in degrees [0, 360)
HEADING_FIELDS = ("mass", "mean_cos", "mean_sin", "mean_deg", "resultant", "mode_bin", "mode_share",
                  "peak_mass", "peak_mean_cos", "peak_mean_sin", "peak_mean_deg", "peak_resultant")


def heading_bin_centres(bins: int) -> np.ndarray:
    """The centre of every bin of model.localize_heading's hist, float64 [bins], degrees: bin b covers [b w, (b + 1) w) with
    w = 360 / bins."""
    bins = int(bins)
    if not 4 <= bins <= 360:
        raise ValueError(f"bins must be in 4..360, got {bins}")
    return (np.arange(bins, dtype=np.float64) + 0.5) * (360.0 / bins)


def heading_sigma_deg(resultant):
    """The circular standard deviation sqrt(-2 ln R) in degrees of a mean resultant length R in [0, 1] (HEADING_FIELDS' "resultant"
    / "peak_resultant"), float64 in the shape of R: 0 for R = 1, inf for R = 0, NaN outside [0, 1] - what an EKF takes as the
    measurement noise of the mean heading."""
    R = np.asarray(resultant.detach().cpu() if hasattr(resultant, "detach") else resultant, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.degrees(np.sqrt(-2.0 * np.log(R)))
    return np.where((R >= 0.0) & (R <= 1.0), out, np.nan)


def von_mises_heading_log_prior(mean_deg, kappa, bins: int, none_log=None) -> np.ndarray:
    """A heading prior for model.localize_heading_prior / heading_prior_map from a heading measurement: float32
    [bins+1] (mean_deg and kappa numbers) or [B, bins+1] (either one [B]).  Entry b < bins is the von Mises log-density at the centre
    of bin b times the bin width, kappa cos(centre_b - mean) - log(2 pi I0(kappa)) + log(w in radians), evaluated in float64 - so
    exp of the entries sums to about 1; the last entry, the weight of a cell without a heading, is none_log or by default
    log(1 / bins), what a flat prior gives a bin.  Angles as rows[:, 4] and heading_bin_centres; kappa >= 0 is about
    1 / sigma^2 in radians."""
    centres = np.radians(heading_bin_centres(bins))
    bins = int(bins)
    scalar = np.ndim(mean_deg) == 0 and np.ndim(kappa) == 0
    mean = np.radians(np.asarray(mean_deg, dtype=np.float64).reshape(-1, 1))
    kap = np.asarray(kappa, dtype=np.float64).reshape(-1, 1)
    if mean.shape[0] != kap.shape[0] and 1 not in (mean.shape[0], kap.shape[0]):
        raise ValueError(f"mean_deg and kappa must hold one value or one per query each, got {mean.shape[0]} and {kap.shape[0]}")
    if not np.isfinite(mean).all():
        raise ValueError("mean_deg must be finite")
    if not (np.isfinite(kap).all() and (kap >= 0).all()):
        raise ValueError("kappa must be finite and >= 0")
    # log I0(kappa) = kappa + log(i0e(kappa)): no overflow at large kappa
    log_i0 = kap + np.log(np.i0(np.minimum(kap, 500.0)) * np.exp(-np.minimum(kap, 500.0)))
    big = kap > 500.0                                   # asymptotically I0(k) e^-k = 1 / sqrt(2 pi k)
    log_i0 = np.where(big, kap - 0.5 * np.log(2.0 * np.pi * np.maximum(kap, 1.0)), log_i0)
    body = kap * np.cos(centres[None, :] - mean) - np.log(2.0 * np.pi) - log_i0 + np.log(2.0 * np.pi / bins)
    last = np.full((body.shape[0], 1), np.log(1.0 / bins) if none_log is None else float(none_log))
    out = np.concatenate([body, last], axis=1).astype(np.float32)
    return out[0] if scalar else out


# ---- tracking a frame stream ------------------------------------------------------------------------------------

def gaussian_taps(sigma_px, radius: int) -> np.ndarray:
    """One-sided blur weights for model.track_predict: float32 [radius+1] (sigma_px a number) or [B, radius+1] (sigma_px [B]),
    t[i] = exp(-0.5 i^2 / sigma^2) / Z with Z the sum over i = -radius..radius, so the two-sided filter sums to 1 (evaluated in
    float64, rounded once to float32)."""
    r = int(radius)
    if not 0 <= r <= 32:
        raise ValueError(f"radius must be in 0..32, got {radius}")
    scalar = np.ndim(sigma_px) == 0
    sig = _sigma(sigma_px, 1 if scalar else np.asarray(sigma_px).reshape(-1).shape[0])
    i = np.arange(r + 1, dtype=np.float64)
    w = np.exp(-0.5 * i[None, :] ** 2 / sig[:, None] ** 2)
    w /= w[:, :1] + 2.0 * w[:, 1:].sum(axis=1, keepdims=True)
    w = w.astype(np.float32)
    return w[0] if scalar else w


def oxford_track_shift(origin_prev, origin_next, motion_map_px) -> np.ndarray:
    """The shift (dx, dy) in OUTPUT pixels, float64 [B,2], that carries a belief over the window at origin_prev = (x0, y0) into the
    window at origin_next after the vehicle moved by motion_map_px = (d col, d row) MAP pixels (each [2] or [B,2]).  Both 800-px
    windows are resized to 512, so one scale serves: (origin_prev - origin_next + motion) * 512 / 800 - the inverse convention of
    oxford_region_to_map, so a map point keeps its map position when the window changes."""
    a = np.asarray(origin_prev, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(origin_next, dtype=np.float64).reshape(-1, 2)
    m = np.asarray(motion_map_px, dtype=np.float64).reshape(-1, 2)
    B = max(a.shape[0], b.shape[0], m.shape[0])
    for what, v in (("origin_prev", a), ("origin_next", b), ("motion_map_px", m)):
        if v.shape[0] not in (1, B):
            raise ValueError(f"{what} must hold 1 or {B} rows, got {v.shape[0]}")
        if not np.isfinite(v).all():
            raise ValueError(f"{what} must be finite")
    return (a - b + m) * (SAT_HW / OXFORD_WIN) + np.zeros((B, 2))


def _heading_filter_args(heading_bins, turn_deg, taps, floor) -> bool:
    """The heading half of a tracker step is on when heading_turn_deg, heading_taps and heading_floor are given - all three, beside
    heading_bins."""
    given = [a is not None for a in (turn_deg, taps, floor)]
    if not any(given):
        return False
    if not all(given):
        raise ValueError("heading_turn_deg, heading_taps and heading_floor go together: give all three or none")
    if heading_bins is None:
        raise ValueError("heading_turn_deg, heading_taps and heading_floor require heading_bins")
    return True


def _heading_table(model, hist, B: int, heading_bins, turn_deg, taps, floor):
    """the heading prior of this step from the hist the tracker holds (None before it holds one: the first step has no heading prior)"""
    if hist is None:
        return None
    if tuple(hist.shape) != (B, int(heading_bins)):
        raise ValueError(f"the tracker holds a hist of shape {tuple(hist.shape)}, this step has {B} streams and heading_bins={heading_bins}")
    return model.heading_predict(hist, turn_deg, taps, floor)


def _update(model, grd, sat, cache, tile_index, prior, table, summary_radius, heading_bins):
    """The update half of both trackers' steps -> (rows, summary or None, (heading, hist) or None, belief).  The aerial side is sat, or
    (sat is None) cache and tile_index; prior: the predicted position prior or None; table: the predicted heading prior or None.
    The family follows from what the step returns: heading_bins -> the heading forms (under the table: the heading-prior forms),
    else summary_radius -> the summary forms, else the update forms; all of them give the same rows and belief."""
    cached = sat is None
    side = (cache,) if cached else (sat,)
    kw = {"tile_index": tile_index} if cached else {}
    if heading_bins is not None:
        kw.update(radius=8 if summary_radius is None else summary_radius, bins=heading_bins, summary=summary_radius is not None,
                  posterior=True)
        if table is not None:
            res = (model.localize_heading_prior_cached if cached else model.localize_heading_prior)(grd, *side, table, prior, **kw)
        else:
            res = (model.localize_heading_cached if cached else model.localize_heading)(grd, *side, prior, **kw)
        return res[0], (res[3] if summary_radius is not None else None), res[1:3], res[-1]
    if summary_radius is not None:
        fn = model.localize_summary_cached if cached else model.localize_summary
        rows, summary, belief = fn(grd, *side, prior, radius=summary_radius, posterior=True, **kw)
        return rows, summary, None, belief
    rows, belief = (model.track_update_cached if cached else model.track_update)(grd, *side, prior, **kw)
    return rows, None, None, belief


class Tracker:
    """A histogram filter over the Oxford windows, host side: holds the posterior map of the last frame (a device tensor
    [B,512,512]) and the window origin it lives in.  step() = model.track_predict (the last posterior moved into this frame's
    window by the odometry, blurred, floored) + model.track_update_cached (this frame's posterior); the first step has no prior."""

    def __init__(self):
        self.belief = None    # posterior of the last frame, or None before the first step
        self.origin = None    # [B,2] int64 window origin (x0, y0) of each query's belief
        self.hist = None      # heading filter: hist [B,heading_bins] of the last frame, or None

    def reset(self) -> None:
        self.belief = None
        self.origin = None
        self.hist = None

    def step(self, model, grd, cache, tile_index, origins, motion_map_px, taps, floor, summary_radius=None, heading_bins=None,
             heading_turn_deg=None, heading_taps=None, heading_floor=None, credible_levels=None):
        """One frame of B parallel streams.  cache / tile_index: as model.localize_cached; origins [T,2]: the crop origin of every
        cached tile (oxford_tiles' "origin"; one per query when tile_index is None); motion_map_px [B,2] or [2]: the motion since
        the last step in map pixels (ignored by the first step); taps, floor: as model.track_predict.  Returns the rows [B,5];
        with summary_radius (0..32) the update is model.localize_summary_cached - the same rows and belief - and the step returns
        (rows, summary [B,16]): entropy, covariance and peak mass of the new belief (SUMMARY_FIELDS), to gate on.  With heading_bins
        (4..360) the update is model.localize_heading_cached - the same rows, belief and summary - and (heading [B,12], hist
        [B,heading_bins]) of the new belief (HEADING_FIELDS) are appended to what the step returns; their window radius is
        summary_radius, or 8 without one.  With heading_turn_deg (a number or [B]: the heading change since the last step, positive
        when the heading angle grows), heading_taps and heading_floor (as model.heading_predict; they require heading_bins) the
        heading is filtered too: the tracker keeps the last hist, and every step after the first runs model.heading_predict on it
        and takes the result as the heading prior of model.localize_heading_prior_cached.  Returns are unchanged.
        With credible_levels (1..8 levels in (0, 1]) the step runs model.belief_credible on the belief it has just stored and appends
        cred [B, 4 + 3 L] (CREDIBLE_HEAD_FIELDS, CREDIBLE_LEVEL_FIELDS) to what it returns; nothing else changes."""
        filt = _heading_filter_args(heading_bins, heading_turn_deg, heading_taps, heading_floor)
        org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
        B = grd.shape[0]
        now = org if tile_index is None else org[np.asarray(tile_index, dtype=np.int64)]
        if now.shape[0] != B:
            raise ValueError(f"origins must name one window per query: {B} expected, got {now.shape[0]}")
        prior = None
        if self.belief is not None:
            if self.belief.shape[0] != B:
                raise ValueError(f"the tracker holds {self.belief.shape[0]} streams, this step has {B}")
            prior = model.track_predict(self.belief, oxford_track_shift(self.origin, now, motion_map_px), taps, floor)
        table = _heading_table(model, self.hist, B, heading_bins, heading_turn_deg, heading_taps, heading_floor) if filt else None
        rows, summary, heading, self.belief = _update(model, grd, None, cache, tile_index, prior, table, summary_radius, heading_bins)
        self.origin = now.copy()
        self.hist = heading[1] if filt else None
        return _step_result(model, rows, summary, heading, self.belief, credible_levels)


# ---- tracking across rotated or rescaled frames -----------------------------------------------------------------
# Affine maps are float64 rows (m0..m5): (x, y) -> (m0 x + m1 y + m2, m3 x + m4 y + m5); every helper takes [6] or [B,6] and returns
# the shape it was given (the broadcast of two).  model.track_predict_affine reads them as OUTPUT pixel index -> SOURCE index position.

def _affine(m, what: str = "matrix") -> np.ndarray:
    a = np.asarray(m, dtype=np.float64)
    if a.ndim not in (1, 2) or a.shape[-1] != 6:
        raise ValueError(f"{what} must be [6] or [B,6], got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite")
    return a


def affine_compose(a, b) -> np.ndarray:
    """The map p -> a(b(p)): b is applied first."""
    a, b = _affine(a, "a"), _affine(b, "b")
    a0, a1, a2, a3, a4, a5 = np.moveaxis(a, -1, 0)
    b0, b1, b2, b3, b4, b5 = np.moveaxis(b, -1, 0)
    return np.stack([a0 * b0 + a1 * b3, a0 * b1 + a1 * b4, a0 * b2 + a1 * b5 + a2,
                     a3 * b0 + a4 * b3, a3 * b1 + a4 * b4, a3 * b2 + a4 * b5 + a5], axis=-1)


def affine_invert(a) -> np.ndarray:
    """The inverse map; a singular matrix is refused."""
    a = _affine(a)
    a0, a1, a2, a3, a4, a5 = np.moveaxis(a, -1, 0)
    det = a0 * a4 - a1 * a3
    if (det == 0).any():
        raise ValueError("matrix is singular")
    i0, i1, i3, i4 = a4 / det, -a1 / det, -a3 / det, a0 / det
    return np.stack([i0, i1, -(i0 * a2 + i1 * a5), i3, i4, -(i3 * a2 + i4 * a5)], axis=-1)


def affine_index_form(m_pil) -> np.ndarray:
    """A Pillow-convention matrix (Image.transform's AFFINE data, ccvpe_preprocess_affine: it acts on the pixel CENTRE (x + 0.5,
    y + 0.5) and gives a position whose pixel centres are at i + 0.5) as the same map between pixel INDICES: index x -> index
    position m0 x + m1 y + (m2 + (m0 + m1 - 1) / 2), likewise y."""
    m = _affine(m_pil).copy()
    m[..., 2] += 0.5 * (m[..., 0] + m[..., 1] - 1.0)
    m[..., 5] += 0.5 * (m[..., 3] + m[..., 4] - 1.0)
    return m


def affine_pillow_form(m_index) -> np.ndarray:
    """The inverse of affine_index_form: an index-coordinate matrix as Pillow AFFINE data."""
    m = _affine(m_index).copy()
    m[..., 2] -= 0.5 * (m[..., 0] + m[..., 1] - 1.0)
    m[..., 5] -= 0.5 * (m[..., 3] + m[..., 4] - 1.0)
    return m


def rigid_matrix(rotation_deg, shift_px, scale=1.0, centre=(255.5, 255.5)) -> np.ndarray:
    """The OUTPUT -> SOURCE index map (model.track_predict_affine's matrix), float64 [B,6] ([6] when every argument is one value),
    of a frame change under which the content moves as

        p_new = centre + scale * R (p_old - centre) + shift_px,      R = [[cos a, sin a], [-sin a, cos a]],  a = rotation_deg

    in index coordinates (x right, y down): the content turns by rotation_deg counter-clockwise as displayed, as
    PIL.Image.rotate(rotation_deg) turns an image - what a viewer sees whose own frame has turned by rotation_deg clockwise -
    about centre (the default is the middle of the 512 grid), grows by scale and moves by shift_px = (dx, dy).  rotation_deg
    and scale are numbers or [B], shift_px [2] or [B,2].  Rotation 0 and scale 1 give (1, 0, -dx, 0, 1, -dy), track_predict's shift;
    multiples of 90 degrees give integer entries (cos and sin are rounded at the 15th decimal, as PIL does)."""
    scalar = np.ndim(rotation_deg) == 0 and np.ndim(scale) == 0 and np.ndim(shift_px) == 1
    sh = np.asarray(shift_px, dtype=np.float64).reshape(-1, 2)
    rot = np.asarray(rotation_deg, dtype=np.float64).reshape(-1)
    sc = np.asarray(scale, dtype=np.float64).reshape(-1)
    B = max(sh.shape[0], rot.shape[0], sc.shape[0])
    for what, v in (("shift_px", sh), ("rotation_deg", rot), ("scale", sc)):
        if v.shape[0] not in (1, B):
            raise ValueError(f"{what} must hold 1 or {B} rows, got {v.shape[0]}")
        if not np.isfinite(v).all():
            raise ValueError(f"{what} must be finite")
    if not (sc > 0).all():
        raise ValueError(f"scale must be positive, got {scale}")
    cx, cy = (float(v) for v in centre)
    a = np.radians(rot)
    cos, sin = np.round(np.cos(a), 15) + 0.0, np.round(np.sin(a), 15) + 0.0
    m0, m1, m3, m4 = cos / sc, -sin / sc, sin / sc, cos / sc          # R^T / scale
    dx, dy = sh[:, 0], sh[:, 1]
    m2 = (cx - m0 * cx - m1 * cy) - (m0 * dx + m1 * dy)
    m5 = (cy - m3 * cx - m4 * cy) - (m3 * dx + m4 * dy)
    out = np.stack(np.broadcast_arrays(m0, m1, m2, m3, m4, m5), axis=-1) + np.zeros((B, 6))
    return out[0] if scalar else out


def kitti_crop_to_tile(matrices, tile_hw: Sequence[int]) -> np.ndarray:
    """kitti_matrices' stage matrices of one sample ([4,6]; [B,4,6] for a batch) and the centre crop (center_crop_box) as ONE
    index-form matrix ([6] / [B,6]): pixel index of the 512 x 512 crop -> index position on the satellite tile it shows.  Stage k
    reads stage k - 1 through its matrix, so the crop reads the tile through stage 0 o stage 1 o ... o the crop's offset."""
    m = np.asarray(matrices, dtype=np.float64)
    if m.ndim not in (2, 3) or m.shape[-1] != 6:
        raise ValueError(f"matrices must be [S,6] or [B,S,6], got {m.shape}")
    top, left = center_crop_box(int(tile_hw[0]), int(tile_hw[1]))
    total = np.zeros(m.shape[:-2] + (6,)) + np.array([1.0, 0.0, float(left), 0.0, 1.0, float(top)])
    for k in range(m.shape[-2] - 1, -1, -1):
        total = affine_compose(m[..., k, :], total)
    return affine_index_form(total)


def kitti_track_matrix(mats_prev, mats_next, tile_hw: Sequence[int], centre_motion_px) -> np.ndarray:
    """The matrix that carries the belief over the previous frame's crop into the next frame's (model.track_predict_affine):
    invert(kitti_crop_to_tile(mats_prev)) o translate(centre_motion_px) o kitti_crop_to_tile(mats_next) - a pixel of the next crop
    -> its position on the next tile -> the same ground point on the previous tile -> its position in the previous crop.
    mats_prev, mats_next: kitti_matrices' output for the two frames ([4,6] or [B,4,6]); both tiles are tile_hw, north-up and at
    one scale, and the next tile is centred centre_motion_px = (d col, d row) tile pixels from the previous one ([2] or [B,2])."""
    mv = np.asarray(centre_motion_px, dtype=np.float64)
    if mv.shape[-1:] != (2,) or mv.ndim not in (1, 2) or not np.isfinite(mv).all():
        raise ValueError(f"centre_motion_px must be finite [2] or [B,2], got {mv.shape}")
    move = np.zeros(mv.shape[:-1] + (6,)) + np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    move[..., 2], move[..., 5] = mv[..., 0], mv[..., 1]
    return affine_compose(affine_invert(kitti_crop_to_tile(mats_prev, tile_hw)),
                          affine_compose(move, kitti_crop_to_tile(mats_next, tile_hw)))


class AffineTracker:
    """Tracker for frames whose aerial grids differ by more than a translation (KITTI's heading-up tiles, tiles cut at another
    zoom): holds the posterior map of the last frame (a device tensor [B,512,512]).  step() = model.track_predict_affine (the last
    posterior resampled into this frame's grid through the caller's matrix, blurred, floored) + the update on this frame's
    aerial image or cache; the first step has no prior."""

    def __init__(self):
        self.belief = None    # posterior of the last frame, or None before the first step
        self.hist = None      # heading filter: hist [B,heading_bins] of the last frame, or None

    def reset(self) -> None:
        self.belief = None
        self.hist = None

    def step(self, model, grd, sat, matrix, taps, floor, summary_radius=None, heading_bins=None, cache=None, tile_index=None,
             heading_turn_deg=None, heading_taps=None, heading_floor=None, credible_levels=None):
        """One frame of B parallel streams.  sat: this frame's aerial images [B,3,512,512], or None with cache / tile_index as
        model.localize_cached; matrix [B,6] or [6]: this frame's pixel index -> the position in the LAST frame's grid it shows
        (rigid_matrix, kitti_track_matrix; ignored by the first step); taps, floor: as model.track_predict.  Returns what
        Tracker.step returns: the rows [B,5]; with summary_radius (rows, summary [B,16]); with heading_bins (heading [B,12], hist
        [B,heading_bins]) appended - the updates are model.track_update / localize_summary / localize_heading, or their _cached
        forms beside a cache.  heading_turn_deg, heading_taps, heading_floor: the heading filter of Tracker.step (the updates are
        then model.localize_heading_prior / _cached).  The orientation field is expressed in each frame's own grid, so here the turn
        must include the rotation between the two grids: the change of the heading angle as THIS frame's grid measures it against
        the last frame's, not the vehicle's turn alone.  credible_levels: as Tracker.step - cred of the stored belief, appended."""
        filt = _heading_filter_args(heading_bins, heading_turn_deg, heading_taps, heading_floor)
        if (sat is None) == (cache is None):
            raise ValueError("give this frame's aerial side as sat or as cache, one of the two")
        if sat is not None and tile_index is not None:
            raise ValueError("tile_index belongs to a cache")
        B = grd.shape[0]
        prior = None
        if self.belief is not None:
            if self.belief.shape[0] != B:
                raise ValueError(f"the tracker holds {self.belief.shape[0]} streams, this step has {B}")
            prior = model.track_predict_affine(self.belief, matrix, taps, floor)
        table = _heading_table(model, self.hist, B, heading_bins, heading_turn_deg, heading_taps, heading_floor) if filt else None
        rows, summary, heading, self.belief = _update(model, grd, sat, cache, tile_index, prior, table, summary_radius, heading_bins)
        self.hist = heading[1] if filt else None
        return _step_result(model, rows, summary, heading, self.belief, credible_levels)


# ---- joint position-heading filter --------------------------------------------------------------------------------

# the 5 columns of model.track_joint_update_logits' rows, in order (include/ccvpe.h): the marginal's first argmax cell, the marginal
# there, the first argmax heading bin at that cell, the largest logit, the normaliser Z
JOINT_FIELDS = ("index", "prob", "heading_bin", "logit_max", "norm")


def heading_emission(kappa, bins: int, none=None) -> np.ndarray:
    """The emission table of model.track_joint_update_logits from the concentration of the orientation field's error: float32
    [bins+1] (kappa a number) or [B, bins+1] (kappa [B]).  Entry j < bins is the von Mises kernel exp(kappa cos(j w)), w = 360 / bins,
    on the bin offsets, normalised to sum 1 over the bins (float64, rounded once): the weight of a heading j bins ahead of the bin of
    the cell's own orientation, symmetric on the circle.  The last entry, the weight of any heading at a cell without an
    orientation, is `none` or by default 1 / bins - what a flat kernel gives a bin.  kappa >= 0 is about 1 / sigma^2 in radians;
    kappa = 0 is the uniform table."""
    bins = int(bins)
    if not 4 <= bins <= 72:
        raise ValueError(f"bins must be in 4..72, got {bins}")
    scalar = np.ndim(kappa) == 0
    kap = np.asarray(kappa, dtype=np.float64).reshape(-1, 1)
    if not (np.isfinite(kap).all() and (kap >= 0).all()):
        raise ValueError("kappa must be finite and >= 0")
    last = 1.0 / bins if none is None else float(none)
    if not (np.isfinite(last) and last >= 0.0):
        raise ValueError(f"none must be finite and >= 0, got {none}")
    off = np.arange(bins, dtype=np.float64) * (2.0 * np.pi / bins)
    body = np.exp(kap * (np.cos(off)[None, :] - 1.0))              # (the common factor exp(-kappa) cancels: no overflow)
    body /= body.sum(axis=1, keepdims=True)
    out = np.concatenate([body, np.full((body.shape[0], 1), last)], axis=1).astype(np.float32)
    return out[0] if scalar else out


def joint_shift_table(forward_px, left_px, bins: int, zero_deg: float = 0.0, clockwise: bool = False, common_px=None) -> np.ndarray:
    """The shift table of model.track_joint_predict from a body-frame motion: float64 [B, bins, 2] = (dx, dy) in image pixels (x right,
    y down) for a vehicle whose heading is the centre of each bin (heading_bin_centres) and which moved forward_px ahead and left_px
    to its left (numbers or [B], output pixels).  A heading label a stands for the image direction at zero_deg + a degrees, or
    zero_deg - a with clockwise, measured counter-clockwise on the screen from the x axis (90 = up): the orientation labels of
    kitti_ground_truth are (zero_deg=0, clockwise=False) - 90 is up on the heading-up tile -, those of oxford_ground_truth
    (zero_deg=90, clockwise=True) - 0 is north, which is up.  common_px ([2] or [B,2]) is added to every bin: the shift a window
    change causes (oxford_track_shift with the motion left out)."""
    centres = heading_bin_centres(bins)
    if int(bins) > 72:
        raise ValueError(f"bins must be in 4..72, got {bins}")
    fw = np.asarray(forward_px, dtype=np.float64).reshape(-1)
    lf = np.asarray(left_px, dtype=np.float64).reshape(-1)
    cm = np.zeros((1, 2)) if common_px is None else np.asarray(common_px, dtype=np.float64).reshape(-1, 2)
    B = max(fw.shape[0], lf.shape[0], cm.shape[0])
    for what, v in (("forward_px", fw), ("left_px", lf), ("common_px", cm)):
        if v.shape[0] not in (1, B):
            raise ValueError(f"{what} must hold 1 or {B} rows, got {v.shape[0]}")
        if not np.isfinite(v).all():
            raise ValueError(f"{what} must be finite")
    if not np.isfinite(zero_deg):
        raise ValueError("zero_deg must be finite")
    phi = np.radians(float(zero_deg) + (-centres if clockwise else centres))       # the image direction of every bin centre
    ahead = np.stack([np.cos(phi), -np.sin(phi)], axis=1)                           # (x right, y down)
    left = np.stack([-np.sin(phi), -np.cos(phi)], axis=1)                           # 90 degrees counter-clockwise of it on the screen
    return fw[:, None, None] * ahead[None] + lf[:, None, None] * left[None] + cm[:, None, :] + np.zeros((B, 1, 1))


class JointTracker:
    """A histogram filter over (heading bin, cell), host side: holds the joint posterior of the last frame (a device tensor
    [B,nb,512,512]) and, for windows that move, the window origins it lives in.  step() = the forward, model.track_joint_predict
    (every heading bin moved by the body-frame odometry as that heading sees it, the bins turned, both blurred, floored) and
    model.track_joint_update_logits; the first step has no prior."""

    def __init__(self):
        self.joint = None     # joint posterior of the last frame, or None before the first step
        self.origin = None    # [B,2] int64 window origin (x0, y0) of each query's maps, or None without origins

    def reset(self) -> None:
        self.joint = None
        self.origin = None

    def step(self, model, grd, emission, forward_px, left_px, turn_deg, taps, heading_taps, floor, cache=None, tile_index=None, sat=None,
             origins=None, zero_deg: float = 0.0, clockwise: bool = False, summary_radius=None, credible_levels=None):
        """One frame of B parallel streams.  The aerial side is cache / tile_index (model.forward_cached) or sat (model.forward).
        emission [nb+1] or [B,nb+1]: heading_emission; forward_px, left_px (numbers or [B], output pixels) and turn_deg (a number or
        [B], the change of the heading label): the body-frame motion since the last step, ignored by the first; zero_deg, clockwise:
        what the dataset's heading labels mean on the image (joint_shift_table); taps, heading_taps, floor: as
        model.track_joint_predict.  origins [T,2]: the crop origin of every cached tile as in Tracker.step, for windows that move
        (Oxford); None: every frame shares one grid.  Returns (rows [B,5], marginal [B,512,512], hist [B,nb]); with summary_radius
        model.belief_summary of the marginal is appended, with credible_levels model.belief_credible of it."""
        if (sat is None) == (cache is None):
            raise ValueError("give this frame's aerial side as sat or as cache, one of the two")
        if sat is not None and tile_index is not None:
            raise ValueError("tile_index belongs to a cache")
        B = grd.shape[0]
        nb = int(np.shape(emission)[-1]) - 1
        now = None
        if origins is not None:
            org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
            now = org if tile_index is None else org[np.asarray(tile_index, dtype=np.int64)]
            if now.shape[0] != B:
                raise ValueError(f"origins must name one window per query: {B} expected, got {now.shape[0]}")
        out = model.forward(grd, sat) if cache is None else model.forward_cached(grd, cache, tile_index=tile_index)
        logits, ori = out[0], out[2]
        prior = None
        if self.joint is not None:
            if tuple(self.joint.shape[:2]) != (B, nb):
                raise ValueError(f"the tracker holds a joint of shape {tuple(self.joint.shape[:2])}, this step has {B} streams of {nb} bins")
            if (now is None) != (self.origin is None):
                raise ValueError("origins must be given on every step of a stream or on none")
            common = None if now is None else oxford_track_shift(self.origin, now, np.zeros(2))
            table = joint_shift_table(forward_px, left_px, nb, zero_deg, clockwise, common)
            prior = model.track_joint_predict(self.joint, np.broadcast_to(table, (B, nb, 2)), taps, floor, turn_deg, heading_taps)
        # in place: the prior is this step's alone
        rows, self.joint, marginal, hist = model.track_joint_update_logits(logits, ori, emission, prior, out=prior)
        self.origin = None if now is None else now.copy()
        res = (rows, marginal, hist)
        if summary_radius is not None:
            res += (model.belief_summary(marginal, summary_radius),)
        if credible_levels is not None:
            res += (model.belief_credible(marginal, credible_levels),)
        return res


# ---- the joint filter across rotated or rescaled frames -----------------------------------------------------------

def matrix_rotation_deg(matrix) -> np.ndarray:
    """rigid_matrix's rotation_deg recovered from an OUTPUT -> SOURCE index map ([6] -> a float64 number, [B,6] -> [B]), in
    (-180, 180]: atan2(m3 - m1, m0 + m4), the content's counter-clockwise turn as displayed.  Exact (to rounding) for similarities -
    rigid_matrix with any scale and shift, kitti_track_matrix.  For a sheared or unevenly scaled matrix of positive determinant it
    is the rotation of the polar part: the linear part factors into a rotation times a symmetric positive definite stretch, and this
    is that rotation's angle - the turn nearest to the map.  A matrix whose m3 - m1 and m0 + m4 are both zero (the zero matrix, a
    pure reflection) has no such angle and gives 0."""
    m = _affine(matrix)
    return np.degrees(np.arctan2(m[..., 3] - m[..., 1], m[..., 0] + m[..., 4])) + 0.0


def joint_matrix_table(matrix, shift_table) -> np.ndarray:
    """The matrix table of model.track_joint_predict_affine, float64 [B, nb, 6], from the frame change and a body-frame motion.
    matrix ([6] or [B,6]): this frame's pixel index -> the position in the LAST frame's grid it shows - rigid_matrix or
    kitti_track_matrix with the vehicle's own motion left out, the frame change alone.  shift_table [B, nb, 2] ([nb, 2]: one
    query): joint_shift_table's output in the LAST frame's pixels and heading labels.  Content with source heading k sits at p_old
    in the old grid and moves to p_old + d[k] there, so the source of an output pixel is M(p_out) - d[k]: entries 2 and 5 become
    m2 - dx[k] and m5 - dy[k], the other four are copied."""
    m = _affine(matrix)
    d = np.asarray(shift_table, dtype=np.float64)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3 or d.shape[-1] != 2:
        raise ValueError(f"shift_table must be [B,nb,2], got {d.shape}")
    if not np.isfinite(d).all():
        raise ValueError("shift_table must be finite")
    m = m.reshape(-1, 6)
    B = max(m.shape[0], d.shape[0])
    if m.shape[0] not in (1, B) or d.shape[0] not in (1, B):
        raise ValueError(f"matrix holds {m.shape[0]} rows, shift_table {d.shape[0]}: 1 or {B} each")
    out = np.broadcast_to(m[:, None, :], (B, d.shape[1], 6)).copy()
    out[..., 2] -= d[..., 0]
    out[..., 5] -= d[..., 1]
    return out


class AffineJointTracker:
    """JointTracker for frames whose aerial grids differ by more than a translation (KITTI's heading-up tiles): holds the joint
    posterior of the last frame (a device tensor [B,nb,512,512]).  step() = the forward, model.track_joint_predict_affine (every
    heading bin read through the frame change and moved by the body-frame odometry as that heading sees it, the bins turned, both
    blurred, floored) and model.track_joint_update_logits; the first step has no prior."""

    def __init__(self):
        self.joint = None     # joint posterior of the last frame, or None before the first step

    def reset(self) -> None:
        self.joint = None

    def step(self, model, grd, emission, matrix, forward_px, left_px, turn_deg, taps, heading_taps, floor, sat=None, cache=None,
             tile_index=None, zero_deg: float = 0.0, clockwise: bool = False, summary_radius=None, credible_levels=None):
        """One frame of B parallel streams.  The aerial side is sat (model.forward) or cache / tile_index (model.forward_cached).
        matrix [6] or [B,6]: this frame's pixel index -> the position in the LAST frame's grid it shows, the frame change alone
        (rigid_matrix, kitti_track_matrix with the vehicle's own motion left out; ignored by the first step).  forward_px, left_px
        (numbers or [B]): the body-frame motion since the last step in pixels of the LAST frame's grid, as the last frame's heading
        labels see it - the predict reads every source bin through joint_matrix_table(matrix, joint_shift_table(forward_px,
        left_px, nb, zero_deg, clockwise)).  turn_deg (a number or [B]): the vehicle's change of heading label ALONE.  The
        orientation field is expressed in each frame's own grid, so the labels also change by the rotation between the two grids;
        this step adds that part itself, + matrix_rotation_deg(matrix) for counter-clockwise labels and - for clockwise ones.  That
        differs from AffineTracker.step, whose heading_turn_deg must already be the sum: do not add the grid's rotation here.
        emission, taps, heading_taps, floor, zero_deg, clockwise, summary_radius, credible_levels: as JointTracker.step.  Returns
        what JointTracker.step returns: (rows [B,5], marginal [B,512,512], hist [B,nb]), then model.belief_summary and
        model.belief_credible of the marginal where asked for."""
        if (sat is None) == (cache is None):
            raise ValueError("give this frame's aerial side as sat or as cache, one of the two")
        if sat is not None and tile_index is not None:
            raise ValueError("tile_index belongs to a cache")
        B = grd.shape[0]
        nb = int(np.shape(emission)[-1]) - 1
        out = model.forward(grd, sat) if cache is None else model.forward_cached(grd, cache, tile_index=tile_index)
        logits, ori = out[0], out[2]
        prior = None
        if self.joint is not None:
            if tuple(self.joint.shape[:2]) != (B, nb):
                raise ValueError(f"the tracker holds a joint of shape {tuple(self.joint.shape[:2])}, this step has {B} streams of {nb} bins")
            table = joint_matrix_table(matrix, joint_shift_table(forward_px, left_px, nb, zero_deg, clockwise))
            grid = matrix_rotation_deg(matrix)
            grid = -grid if clockwise else grid
            if hasattr(turn_deg, "data_ptr"):            # a tensor: the sum is formed where it lives
                import torch
                turn = turn_deg + torch.as_tensor(grid, dtype=turn_deg.dtype, device=turn_deg.device)
            else:
                turn = np.asarray(turn_deg, dtype=np.float64) + grid
                turn = float(turn) if turn.ndim == 0 else turn
            prior = model.track_joint_predict_affine(self.joint, np.broadcast_to(table, (B, nb, 6)), taps, floor, turn, heading_taps)
        # in place: the prior is this step's alone
        rows, self.joint, marginal, hist = model.track_joint_update_logits(logits, ori, emission, prior, out=prior)
        res = (rows, marginal, hist)
        if summary_radius is not None:
            res += (model.belief_summary(marginal, summary_radius),)
        if credible_levels is not None:
            res += (model.belief_credible(marginal, credible_levels),)
        return res
