"""The fused last decoder level on its own (ccvpe_op_level1, kernels_level1_tile.inc) at the smallest shapes at which its tiling can go
wrong, on 32 x 16 and 16 x 16 output tiles: against a float64 reference (transposed conv, conv + ReLU, conv, normalize) computed here on
the CPU, and the two tile shapes against each other bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import _lib

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # scale-relative, as tests/test_level1_composed_gpu.py holds the level against its oracle

# (output H, output W, batch, workgroup cap).  32 x 32: one row pair of 32 x 16 tiles, every tile on all four borders (each row of the
# bias-case table).  48 x 96, batch 2: 3 x 3 tiles of 32 x 16 per sample - one fully interior - and 8 workgroups for 18 tiles, so the
# loop over tiles runs and one workgroup's run crosses the sample boundary.  48 x 48: no multiple of 32, the 16 x 16 fallback.
SHAPES = {"32x32": (32, 32, 1, 0), "48x96": (48, 96, 2, 8), "48x48": (48, 48, 1, 0)}
# (descriptor channels, score channel, output channels): the three real width classes and one generic width (NG == 0)
WIDTHS = {"score+40": (40, True, 1), "score+32": (32, True, 1), "ori32": (32, False, 2), "score+24": (24, True, 1)}


@functools.lru_cache(maxsize=None)
def case(shape, width):
    """(input NHWC, weights, float64 reference NCHW) of one case, on the CPU; computed once."""
    H, W, B, _ = SHAPES[shape]
    cd, score, cout = WIDTHS[width]
    cin = cd + (1 if score else 0)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + cd + cout)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    x = rnd(B, H // 2, W // 2, cin)
    wd, bd = rnd(cin, 16, 2, 2) / (4 * cin) ** 0.5, rnd(16)        # a deconv bias of the size of the terms: a wrong border case shows
    wa, ba = rnd(16, 16, 3, 3) / 12.0, rnd(16) * 0.5
    wt, bt = rnd(cout, 16, 3, 3) / 12.0, rnd(cout) * 0.5
    d = lambda t: t.double()
    y = F.conv_transpose2d(d(x).permute(0, 3, 1, 2), d(wd), d(bd), stride=2)
    y = F.relu(F.conv2d(y, d(wa), d(ba), padding=1))
    y = F.conv2d(y, d(wt), d(bt), padding=1)
    if cout == 2:
        y = F.normalize(y, dim=1)
    return x, (wd, bd, wa, ba, wt, bt), y


def run(shape, width, tile):
    x, ws, _ = case(shape, width)
    out, ran = _lib.op_level1(x.cuda(), *[t.cuda() for t in ws], score=WIDTHS[width][1], tile=tile, max_wg=SHAPES[shape][3])
    return out.cpu(), ran


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


@pytest.mark.parametrize("width", list(WIDTHS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_level1_tiles_match_reference_and_each_other(shape, width):
    ref = case(shape, width)[2]
    small, ran_small = run(shape, width, 0)
    large, ran_large = run(shape, width, 1)
    assert ran_small == 0
    assert ran_large == (1 if SHAPES[shape][1] % 32 == 0 else 0), "the plan's choice of tile"
    e_small, e_large = rel(small, ref), rel(large, ref)
    print(f"{shape} {width}: 16x16 {e_small:.3g} 32x16 {e_large:.3g}")
    assert e_small < RTOL
    assert e_large < RTOL
    assert torch.equal(large, small), "every tile shape gives every output the same bits"
