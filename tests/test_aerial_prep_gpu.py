"""Device-side aerial preparation for the KITTI and Oxford test loops: ccvpe_preprocess_affine and
ccvpe_preprocess_window_resize against Pillow's bytes (tests/golden/aerial_prep.npz) and against the numpy restatement
tests/pil_warp.py (pinned to live Pillow by tests/test_aerial_prep_cpu.py), through the public helpers of ccvpe_amd.aerial."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from oracle import ccvpe_oracle as orc
from oracle import resize_oracle as ro
from tests import golden_util as gu
from tests import pil_warp as pw

pytestmark = pytest.mark.gpu


def _kitti_reference(tiles, heading, sx, sy, th):
    """restatement-prepared KITTI `sat_map` tensors [B,3,512,512] (float32, CPU)"""
    H, W = tiles.shape[1:3]
    mats, filters = aerial.kitti_matrices(heading, sx, sy, th, (H, W))
    top, left = aerial.center_crop_box(H, W)
    u8 = np.stack([pw.crop(pw.chain(t, m, filters), top, left, 512, 512) for t, m in zip(tiles, mats)])
    return orc.preprocess(torch.from_numpy(u8))


def _gt_map_argmax(x_offset, y_offset):
    """np.argmax of the reference's float32 Gaussian map (datasets.py:600-606)"""
    x, y = np.meshgrid(np.linspace(-256 + x_offset, 256 + x_offset, 512), np.linspace(-256 + y_offset, 256 + y_offset, 512))
    d = np.sqrt(x * x + y * y)
    gt = np.zeros([1, 512, 512], dtype=np.float32)
    gt[0, :, :] = np.exp(-((d - 0.0) ** 2 / (2.0 * 4 ** 2)))
    return int(gt.argmax())


def test_affine_chain_matches_the_pillow_fixture():
    fx = np.load(gu.GOLDEN_DIR + "/aerial_prep.npz", allow_pickle=False)
    i = 0
    while f"case{i}_out" in fx:
        img = fx[f"img{int(fx[f'case{i}_src'])}"]
        got = _lib.preprocess_affine(torch.from_numpy(img[None]).cuda(), fx[f"case{i}_mats"][None], list(fx[f"case{i}_filters"]),
                                     tuple(fx[f"case{i}_crop"]))
        ref = orc.preprocess(torch.from_numpy(fx[f"case{i}_out"][None]))
        assert got.shape == ref.shape, i
        assert torch.equal(got.cpu(), ref), f"case {i}"
        i += 1
    assert i >= 13


def test_window_resize_matches_the_pillow_fixture():
    fx = np.load(gu.GOLDEN_DIR + "/aerial_prep.npz", allow_pickle=False)
    i = 0
    while f"win{i}_out" in fx:
        img = fx[f"img{int(fx[f'win{i}_src'])}"]
        x0, y0, wh, ww = (int(v) for v in fx[f"win{i}_box"])
        got = _lib.preprocess_window_resize(torch.from_numpy(img).cuda(), [[x0, y0]], (wh, ww), tuple(fx[f"win{i}_size"]))
        assert torch.equal(got.cpu(), orc.preprocess(torch.from_numpy(fx[f"win{i}_out"][None]))), f"window {i}"
        i += 1
    assert i >= 2


def test_kitti_geometry_per_sample_parameters_with_shortcut_angles():
    """1280^2 tiles -> 512^2 at B=4; sample 0 rotates by 90 then 0, sample 1 by 180 then 90, sample 2 by 0 then 270 (Pillow's
    copy / transpose shortcuts), sample 3 by arbitrary angles."""
    rng = np.random.default_rng(11)
    tiles = rng.integers(0, 256, size=(4, 1280, 1280, 3), dtype=np.uint8)
    heading = [-np.pi / 2, np.pi, 0.0, 0.731]
    sx, sy, th = [0.31, -0.9, 1.0, -0.27], [-0.55, 0.12, -1.0, 0.83], [0.0, 9.0, 27.0, -0.618]
    got = aerial.kitti_aerial(torch.from_numpy(tiles).cuda(), heading, sx, sy, th)
    assert got.shape == (4, 3, 512, 512)
    assert torch.equal(got.cpu(), _kitti_reference(tiles, heading, sx, sy, th))


def test_kitti_batch_32_equals_per_sample_calls():
    rng = np.random.default_rng(12)
    B = 32
    tiles = torch.from_numpy(rng.integers(0, 256, size=(B, 1280, 1280, 3), dtype=np.uint8)).cuda()
    heading = rng.uniform(-np.pi, np.pi, B)
    sx, sy, th = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    got = aerial.kitti_aerial(tiles, heading, sx, sy, th)
    for b in range(B):
        one = aerial.kitti_aerial(tiles[b:b + 1], heading[b:b + 1], sx[b:b + 1], sy[b:b + 1], th[b:b + 1])
        assert torch.equal(got[b:b + 1], one), b


def test_oxford_windows_at_the_map_edges():
    """A synthetic 4000 x 5000 map; ground positions whose 800^2 windows leave the map on each side."""
    rng = np.random.default_rng(13)
    mp = rng.integers(0, 256, size=(4000, 5000, 3), dtype=np.uint8)
    coords = np.array([[10.3, 12.7], [4990.2, 3995.5], [2511.6, 150.1], [120.0, 3870.9], [2600.4, 2100.8]])
    got = aerial.oxford_aerial(torch.from_numpy(mp).cuda(), coords)
    win = aerial.oxford_window(coords)
    assert (win["origin"] < 0).any() and (win["origin"][:, 0] + 800 > 5000).any() and (win["origin"][:, 1] + 800 > 4000).any()
    ref = np.stack([ro.resize_bilinear_u8(pw.crop(mp, int(y0), int(x0), 800, 800), 512, 512) for x0, y0 in win["origin"]])
    assert torch.equal(got.cpu(), orc.preprocess(torch.from_numpy(ref)))


def test_kitti_forward_and_evaluate_on_device_prepared_inputs():
    """CVM_KITTI at B=2: device-prepared aerial inputs give the nine outputs of restatement-prepared ones, and model.evaluate fed
    kitti_ground_truth equals the restated test loop fed the reference's own ground-truth maps."""
    m = models.CVM_KITTI("cuda")
    m.load_state_dict(weights.generate_state_dict("kitti", 0))
    m.to("cuda").eval()
    rng = np.random.default_rng(14)
    tiles = rng.integers(0, 256, size=(2, 1280, 1280, 3), dtype=np.uint8)
    heading, sx, sy, th = [0.42, -2.6], [0.37, -0.81], [-0.66, 0.05], [0.5, -0.93]
    g, _ = weights.generate_inputs("kitti", 2, 3)
    g = torch.from_numpy(g).cuda()
    sat_dev = aerial.kitti_aerial(torch.from_numpy(tiles).cuda(), heading, sx, sy, th)
    sat_ref = _kitti_reference(tiles, heading, sx, sy, th).cuda()
    a = [o.clone() for o in m(g, sat_dev)]
    b = m(g, sat_ref)
    assert len(a) == 9
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), k
    gt = aerial.kitti_ground_truth(sx, sy, th)
    mpp = aerial.get_meter_per_pixel(scale=1)
    heat, ori = a[1], a[2]
    got = m.evaluate(heat, ori, gt["gt_index"], mpp, gt["gt_cos_sin"], gt["heading_deg"])
    # reference side: offsets, maps and orientation exactly as datasets.py:596-634 builds them
    pix = 20 / mpp
    gt_index, cos_sin, heading_deg = [], [], []
    for b_ in range(2):
        gx, gy, ro_ = -float(sx[b_]), -float(sy[b_]), float(th[b_]) * 10
        xo = int(gx * pix * np.cos(ro_ / 180 * np.pi) - gy * pix * np.sin(ro_ / 180 * np.pi))
        yo = int(-gy * pix * np.cos(ro_ / 180 * np.pi) - gx * pix * np.sin(ro_ / 180 * np.pi))
        gt_index.append(_gt_map_argmax(xo, yo))
        oa = 90 - ro_
        oa = oa + 360 if oa < 0 else (oa - 360 if oa > 360 else oa)
        heading_deg.append(oa)
        cos_sin.append(np.array([np.cos(oa * np.pi / 180), np.sin(oa * np.pi / 180)], dtype=np.float32))
    assert list(gt["gt_index"]) == gt_index
    ref = orc.eval_metrics(heat.cpu().numpy(), ori.cpu().numpy(), gt_index, mpp, np.stack(cos_sin), np.array(heading_deg))
    for k, v in ref.items():
        gk = got[k].cpu().numpy()
        assert np.array_equal(np.isnan(gk), np.isnan(v)), k
        assert np.allclose(gk, v, rtol=1e-9, atol=1e-7, equal_nan=True), (k, gk, v)


def test_bad_arguments_are_refused():
    img = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
    eye = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

    def affine(n, filters=None, crop=(0, 0, 64, 64), im=img):
        filters = filters if filters is not None else ["nearest"] * n
        return _lib.preprocess_affine(im, np.tile(np.array(eye), (im.shape[0], n, 1)), filters, crop)

    assert torch.equal(affine(4, ["bilinear", "nearest", "bilinear", "nearest"]).cpu(), orc.preprocess(torch.zeros((1, 64, 64, 3), dtype=torch.uint8)))
    refusals = [
        lambda: affine(5),                                                       # more than 4 stages
        lambda: affine(0, []),                                                   # no stage
        lambda: affine(3, ["bilinear"] * 3),                                     # more than 2 BILINEAR stages
        lambda: affine(1, [1]),                                                  # unknown filter (PIL's LANCZOS / ANTIALIAS id)
        lambda: affine(1, [3]),                                                  # BICUBIC
        lambda: affine(1, crop=(1, 0, 64, 64)),                                  # crop leaves the canvas
        lambda: affine(1, crop=(0, -1, 32, 32)),
        lambda: affine(1, crop=(0, 0, 0, 32)),
        lambda: affine(1, im=torch.zeros((1, 16385, 1, 3), dtype=torch.uint8, device="cuda"), crop=(0, 0, 1, 1)),   # canvas > 16384
        lambda: _lib.preprocess_window_resize(img[0], [[0, 0]], (800, 800), (64, 64)),   # 12.5x down-scaling
        lambda: _lib.preprocess_window_resize(img[0], [[0, 0]], (0, 64), (64, 64)),
    ]
    for i, f in enumerate(refusals):
        with pytest.raises(_lib.CcvpeError):
            f()
            pytest.fail(f"refusal {i} was accepted")
    lib = _lib.load()
    m3 = (_lib.C.c_float * 3)(0, 0, 0)
    flt = (_lib.C.c_int32 * 1)(0)
    dummy = _lib.C.c_void_p(img.data_ptr())
    assert lib.ccvpe_preprocess_affine(None, 1, 64, 64, dummy, flt, 1, 0, 0, 64, 64, _lib.C.byref(m3), _lib.C.byref(m3), dummy, None) == -1
    assert lib.ccvpe_preprocess_affine(dummy, 1, 64, 64, None, flt, 1, 0, 0, 64, 64, _lib.C.byref(m3), _lib.C.byref(m3), dummy, None) == -1
    assert lib.ccvpe_preprocess_affine(dummy, 1, 64, 64, dummy, None, 1, 0, 0, 64, 64, _lib.C.byref(m3), _lib.C.byref(m3), dummy, None) == -1
    assert lib.ccvpe_preprocess_window_resize(dummy, 64, 64, None, 1, 8, 8, 8, 8, _lib.C.byref(m3), _lib.C.byref(m3), dummy, dummy, None) == -1
    assert lib.ccvpe_preprocess_window_resize(dummy, 64, 64, dummy, 1, 8, 8, 8, 8, _lib.C.byref(m3), _lib.C.byref(m3), None, dummy, None) == -1
    torch.cuda.synchronize()
