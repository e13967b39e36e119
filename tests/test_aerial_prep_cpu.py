"""The numpy restatement of the KITTI / Oxford aerial preparation (tests/pil_warp.py) and the dataset arithmetic of
ccvpe_amd.aerial, against live Pillow where it is installed and against Pillow's recorded bytes (tests/golden/aerial_prep.npz)
where it is not; the ground-truth helpers against np.argmax of the reference's own float32 map."""
import math

import numpy as np
import pytest

from ccvpe_amd import aerial
from oracle import resize_oracle as ro
from tests import golden_util as gu
from tests import pil_warp as pw

ANGLES = [0.0, 90.0, 180.0, 270.0, -90.0, 540.0, 1e-3, 359.99, 33.7, -71.25, 123.456, 200.1, -359.5, 45.0]


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(96, 96), (128, 160), (97, 131)])
def test_nearest_rotation_equals_pillow(h, w):
    Image = pytest.importorskip("PIL.Image")
    img = _img(h, w, h * w)
    pil = Image.fromarray(img)
    for angle in ANGLES:
        assert np.array_equal(pw.affine_nearest(img, aerial.rotate_matrix(angle, w, h)), np.asarray(pil.rotate(angle))), angle


@pytest.mark.parametrize("h,w", [(96, 96), (128, 160)])
def test_bilinear_affine_equals_pillow(h, w):
    Image = pytest.importorskip("PIL.Image")
    img = _img(h, w, h + w)
    pil = Image.fromarray(img)
    for m in [(1, 0, 2.3, 0, 1, -1.7), (1, 0, -5.5, 0, 1, 3.25), (1, 0, -0.49, 0, 1, -0.51), (1, 0, 150.5, 0, 1, 0),
              (1, 0, 0, 0, 1, -140.75), (1, 0, 60.1, 0, 1, 70.9), (0.93, 0.21, -3.1, -0.17, 1.08, 4.7)]:
        want = np.asarray(pil.transform(pil.size, Image.AFFINE, m, resample=Image.BILINEAR))
        assert np.array_equal(pw.affine_bilinear(img, m), want), m


# split-file-style (heading_rad, gt_shift_x, gt_shift_y, theta) values, shortcut angles included
KITTI_PARAMS = [(0.7, 0.3, -0.8, 0.25), (-2.1, -1.0, 1.0, -1.0), (-math.pi / 2, 0.0, 0.0, 0.0), (math.pi, 0.51, 0.49, 0.9),
                (0.0, -0.123, 0.877, 18.0), (1.234, 0.999, -0.001, -0.5), (3.0, -0.66, -0.66, 0.01), (-0.4, 0.2, 0.7, 27.0)]


def test_kitti_chain_equals_the_reference_pillow_calls():
    """datasets.py:577-594 on a 1280^2 tile, call by call, against the restatement fed kitti_matrices."""
    Image = pytest.importorskip("PIL.Image")
    img = _img(1280, 1280, 7)
    sat_map = Image.fromarray(img)
    mpp = aerial.get_meter_per_pixel(scale=1)
    shift_range_pixels_lat = 20 / mpp
    shift_range_pixels_lon = 20 / mpp
    heading, sx, sy, th = (np.array(v) for v in zip(*KITTI_PARAMS))
    mats, filters = aerial.kitti_matrices(heading, sx, sy, th, (1280, 1280))
    top, left = aerial.center_crop_box(1280, 1280)
    for b, (hd, gsx, gsy, theta) in enumerate(KITTI_PARAMS):
        sat_rot = sat_map.rotate(-hd / np.pi * 180)
        sat_align_cam = sat_rot.transform(sat_rot.size, Image.AFFINE, (1, 0, 1.08 / mpp, 0, 1, 0.26 / mpp), resample=Image.BILINEAR)
        gt_shift_x, gt_shift_y = -float(gsx), -float(gsy)
        sat_rand_shift = sat_align_cam.transform(sat_align_cam.size, Image.AFFINE,
                                                 (1, 0, gt_shift_x * shift_range_pixels_lon, 0, 1, -gt_shift_y * shift_range_pixels_lat),
                                                 resample=Image.BILINEAR)
        sat_rand_shift_rand_rot = sat_rand_shift.rotate(float(theta) * 10)
        want = np.asarray(sat_rand_shift_rand_rot.crop((left, top, left + 512, top + 512)))    # TF.center_crop(512)
        got = pw.crop(pw.chain(img, mats[b], filters), top, left, 512, 512)
        assert np.array_equal(got, want), KITTI_PARAMS[b]


def test_oxford_window_partly_outside_the_map_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    mp = _img(1100, 1300, 8)
    pil = Image.fromarray(mp)
    coords = np.array([[150.0, 990.0], [1250.5, 60.2]])
    win = aerial.oxford_window(coords)
    assert (win["origin"] < 0).any() and (win["origin"] + 800 > np.array([1300, 1100])).any()
    for x0, y0 in win["origin"]:
        x0, y0 = int(x0), int(y0)
        want = np.asarray(pil.crop((x0, y0, x0 + 800, y0 + 800)).resize((512, 512), Image.BILINEAR))
        assert np.array_equal(ro.resize_bilinear_u8(pw.crop(mp, y0, x0, 800, 800), 512, 512), want)


def test_restatement_equals_the_recorded_pillow_bytes():
    fx = np.load(gu.GOLDEN_DIR + "/aerial_prep.npz", allow_pickle=False)
    assert str(fx["pillow_version"])
    i = 0
    while f"case{i}_out" in fx:
        img = fx[f"img{int(fx[f'case{i}_src'])}"]
        top, left, h, w = (int(v) for v in fx[f"case{i}_crop"])
        got = pw.crop(pw.chain(img, fx[f"case{i}_mats"], list(fx[f"case{i}_filters"])), top, left, h, w)
        assert np.array_equal(got, fx[f"case{i}_out"]), f"case {i}"
        i += 1
    assert i >= 13
    j = 0
    while f"win{j}_out" in fx:
        img = fx[f"img{int(fx[f'win{j}_src'])}"]
        x0, y0, wh, ww = (int(v) for v in fx[f"win{j}_box"])
        oh, ow = (int(v) for v in fx[f"win{j}_size"])
        assert np.array_equal(ro.resize_bilinear_u8(pw.crop(img, y0, x0, wh, ww), oh, ow), fx[f"win{j}_out"]), f"window {j}"
        j += 1
    assert j >= 2


def test_fixture_matrices_are_the_rotate_matrices_of_the_helpers():
    """The generator recorded aerial.rotate_matrix for every rotate stage: the helper and the fixture agree."""
    fx = np.load(gu.GOLDEN_DIR + "/aerial_prep.npz", allow_pickle=False)
    h, w = fx["img0"].shape[:2]
    assert np.array_equal(fx["case0_mats"][0], np.array(aerial.rotate_matrix(33.7, w, h)))


def _reference_gt_map_argmax(x_offset, y_offset):
    """datasets.py:600-606 (= datasets.py:323-329 with the Oxford offsets): the float32 map, then the test loop's argmax"""
    x, y = np.meshgrid(np.linspace(-256 + x_offset, 256 + x_offset, 512), np.linspace(-256 + y_offset, 256 + y_offset, 512))
    d = np.sqrt(x * x + y * y)
    sigma, mu = 4, 0.0
    gt = np.zeros([1, 512, 512], dtype=np.float32)
    gt[0, :, :] = np.exp(-((d - mu) ** 2 / (2.0 * sigma ** 2)))
    return int(gt.argmax())


@pytest.mark.parametrize("xo,yo", [(0, 0), (0, 17), (-33, 0), (255, -255), (-255, 255), (255, 255), (-255, -255), (1, -1),
                                   (100, -7), (-128, 128), (37, 254)])
def test_gt_argmax_equals_numpy_argmax_of_the_reference_map(xo, yo):
    assert aerial.gt_argmax(xo, yo) == _reference_gt_map_argmax(xo, yo)


def test_gt_argmax_ties_at_offset_zero():
    """offset 0: lines +-256/511 tie on both axes; np.argmax takes the first of the four maxima, (255, 255)."""
    assert aerial.gt_argmax(0, 0) == 255 * 512 + 255
    with pytest.raises(ValueError):
        aerial.gt_argmax(256, 0)


def test_kitti_ground_truth_restates_the_test_split():
    """datasets.py:596-634 per sample: offsets from the negated split values and theta, orientation_angle and its (cos, sin)."""
    mpp = aerial.get_meter_per_pixel(scale=1)
    pix = 20 / mpp
    heading, sx, sy, th = (np.array(v) for v in zip(*KITTI_PARAMS))
    got = aerial.kitti_ground_truth(sx, sy, th)
    for b in range(len(sx)):
        gt_shift_x, gt_shift_y, random_ori = -float(sx[b]), -float(sy[b]), float(th[b]) * 10
        x_offset = int(gt_shift_x * pix * np.cos(random_ori / 180 * np.pi) - gt_shift_y * pix * np.sin(random_ori / 180 * np.pi))
        y_offset = int(-gt_shift_y * pix * np.cos(random_ori / 180 * np.pi) - gt_shift_x * pix * np.sin(random_ori / 180 * np.pi))
        assert got["gt_index"][b] == _reference_gt_map_argmax(x_offset, y_offset)
        orientation_angle = 90 - random_ori
        if orientation_angle < 0:
            orientation_angle = orientation_angle + 360
        elif orientation_angle > 360:
            orientation_angle = orientation_angle - 360
        assert got["heading_deg"][b] == orientation_angle
        import torch
        orientation_map = torch.full([2, 4, 4], np.cos(orientation_angle * np.pi / 180))
        orientation_map[1, :, :] = np.sin(orientation_angle * np.pi / 180)
        assert np.array_equal(got["gt_cos_sin"][b], orientation_map[:, 0, 0].numpy())
    assert got["gt_index"].dtype == np.int32 and got["gt_cos_sin"].dtype == np.float32


def test_oxford_window_and_ground_truth_restate_the_test_split():
    """datasets.py:306-351 for the val / test split."""
    rng = np.random.default_rng(9)
    coords = np.concatenate([rng.uniform(0, 8000, size=(40, 2)), [[400.0, 800.0], [599.5, 199.6], [600.4, 1000.5]]])
    yaw = rng.uniform(-np.pi, np.pi, size=len(coords))
    win = aerial.oxford_window(coords)
    gt = aerial.oxford_ground_truth(coords, yaw)
    for b, image_coord in enumerate(coords):
        col_split = int((image_coord[0]) // 400)
        if np.round(image_coord[0] - 400 * col_split) < 200:
            col_split -= 1
        col_pixel = int(np.round(image_coord[0] - 400 * col_split))
        row_split = int((image_coord[1]) // 400)
        if np.round(image_coord[1] - 400 * row_split) < 200:
            row_split -= 1
        row_pixel = int(np.round(image_coord[1] - 400 * row_split))
        assert tuple(win["origin"][b]) == (col_split * 400, row_split * 400)
        row_offset_resized = int(-(row_pixel / 800 * 512 - 256))
        col_offset_resized = int(-(col_pixel / 800 * 512 - 256))
        assert gt["gt_index"][b] == _reference_gt_map_argmax(col_offset_resized, row_offset_resized)
        orientation_angle = (yaw[b] / np.pi * 180) - 90
        if orientation_angle < 0:
            orientation_angle = orientation_angle + 360
        assert gt["heading_deg"][b] == orientation_angle
        assert np.array_equal(gt["gt_cos_sin"][b], np.array([np.cos(orientation_angle * np.pi / 180),
                                                             np.sin(orientation_angle * np.pi / 180)], dtype=np.float32))
