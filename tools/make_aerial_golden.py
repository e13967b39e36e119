"""Write tests/golden/aerial_prep.npz: Pillow's own output for the resamplings of the KITTI and Oxford aerial preparation on
reduced canvases (reference datasets.py:577-598 rotate / transform(AFFINE, BILINEAR) / center_crop; datasets.py:306-321
crop + Resize).  Needs Pillow; records its version.  tests/test_aerial_prep_cpu.py holds tests/pil_warp.py to the file,
tests/test_aerial_prep_gpu.py holds the kernels to it.

    python tools/make_aerial_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccvpe_amd import aerial  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "aerial_prep.npz")

# (input index, stages, crop (top, left, h, w) or None = whole canvas); a stage is ("rotate", degrees) or ("bilinear", data)
AFFINE_CASES = [
    (0, [("rotate", 33.7)], None),
    (0, [("rotate", 180.0)], None),
    (0, [("rotate", -90.0)], None),                                    # square: Pillow transposes
    (1, [("rotate", 90.0)], None),                                     # non-square: the affine path
    (1, [("rotate", 540.0)], (20, 30, 96, 100)),
    (2, [("rotate", 1e-3)], (36, 36, 128, 128)),
    (2, [("rotate", 359.99)], (0, 72, 128, 128)),
    (0, [("bilinear", (1, 0, 2.3, 0, 1, -1.7))], None),
    (1, [("bilinear", (1, 0, -7.25, 0, 1, 3.6))], (0, 0, 128, 128)),
    (0, [("bilinear", (1, 0, 80.5, 0, 1, -60.25))], None),            # most of the content pushed off the canvas
    (0, [("bilinear", (0.93, 0.21, -3.1, -0.17, 1.08, 4.7))], None),  # general matrix
    (2, [("rotate", -47.3), ("bilinear", (1, 0, 5.513, 0, 1, 1.327)), ("bilinear", (1, 0, -12.7, 0, 1, 31.9)), ("rotate", 6.4)],
     (36, 36, 128, 128)),                                              # the KITTI chain
    (1, [("bilinear", (1, 0, 0.5, 0, 1, -0.25)), ("rotate", 270.0)], (16, 16, 96, 128)),
]
# (map index, (x0, y0, win_h, win_w), (out_h, out_w)): windows partly outside the map
WINDOW_CASES = [
    (2, (-40, 130, 120, 120), (77, 77)),
    (2, (150, -30, 100, 90), (64, 50)),
]


def main() -> None:
    import PIL
    from PIL import Image

    rng = np.random.default_rng(20261016)
    imgs = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((96, 96, 3), (128, 160, 3), (200, 200, 3))]
    data = {"pillow_version": np.array(PIL.__version__)}
    for k, im in enumerate(imgs):
        data[f"img{k}"] = im
    for i, (src, stages, box) in enumerate(AFFINE_CASES):
        im = Image.fromarray(imgs[src])
        mats, filters = [], []
        for kind, arg in stages:
            if kind == "rotate":
                mats.append(aerial.rotate_matrix(arg, im.width, im.height))
                filters.append(aerial.NEAREST)
                im = im.rotate(arg)
            else:
                mats.append(tuple(float(v) for v in arg))
                filters.append(aerial.BILINEAR)
                im = im.transform(im.size, Image.AFFINE, arg, resample=Image.BILINEAR)
        top, left, h, w = box if box is not None else (0, 0, im.height, im.width)
        data[f"case{i}_src"] = np.array(src)
        data[f"case{i}_mats"] = np.array(mats, dtype=np.float64)
        data[f"case{i}_filters"] = np.array(filters, dtype=np.int32)
        data[f"case{i}_crop"] = np.array((top, left, h, w), dtype=np.int32)
        data[f"case{i}_out"] = np.asarray(im.crop((left, top, left + w, top + h)))
    for i, (src, (x0, y0, wh, ww), (oh, ow)) in enumerate(WINDOW_CASES):
        win = Image.fromarray(imgs[src]).crop((x0, y0, x0 + ww, y0 + wh))
        data[f"win{i}_src"] = np.array(src)
        data[f"win{i}_box"] = np.array((x0, y0, wh, ww), dtype=np.int32)
        data[f"win{i}_size"] = np.array((oh, ow), dtype=np.int32)
        data[f"win{i}_out"] = np.asarray(win.resize((ow, oh), Image.BILINEAR))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
