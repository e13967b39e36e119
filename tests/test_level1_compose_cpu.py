"""The fused last decoder level composes ConvTranspose2d(k2, s2) with the first 3x3 conv (zero padding 1) into one convolution per
output parity plus a 9-case border bias table (ccvpe_weights.hip build_decoder, j == 5; kernels_level1_tile.inc).  This checks the
composition formula in double precision against the two convolutions run one after the other, on every image border and corner."""
import numpy as np
import torch
import torch.nn.functional as F


def compose(wd, bd, wa, ba):
    """wd [cin][m][2][2], bd [m], wa [o][m][3][3], ba [o] -> Wc [py][px][a][b][cin][o], bias table [9][o] (row case * 3 + column case;
    case 0 interior, 1 first row / column, 2 last)."""
    cin, mid = wd.shape[:2]
    o = wa.shape[0]
    wc = np.zeros((2, 2, 2, 2, cin, o))
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    ty, tx = py + ky + 1, px + kx + 1
                    a, b = (ty >> 1) - py, (tx >> 1) - px
                    wc[py, px, a, b] += wd[:, :, ty & 1, tx & 1] @ wa[:, :, ky, kx].T
    bc = np.zeros((9, o))
    for rc in range(3):
        for cc in range(3):
            acc = ba.copy()
            for ky in range(3):
                for kx in range(3):
                    if (rc == 1 and ky == 0) or (rc == 2 and ky == 2) or (cc == 1 and kx == 0) or (cc == 2 and kx == 2):
                        continue
                    acc = acc + wa[:, :, ky, kx] @ bd
            bc[rc * 3 + cc] = acc
    return wc, bc


def composed_forward(x, wc, bc):
    """x [cin][h][w] -> conv_a pre-activation [o][2h][2w], one output pixel at a time from its 2x2 input window."""
    cin, h, w = x.shape
    o = wc.shape[-1]
    xp = np.zeros((cin, h + 2, w + 2))
    xp[:, 1:-1, 1:-1] = x                       # zero input outside the image
    out = np.zeros((o, 2 * h, 2 * w))
    for r in range(2 * h):
        for c in range(2 * w):
            py, px, i, j = r & 1, c & 1, r >> 1, c >> 1
            acc = np.zeros(o)
            for a in range(2):
                for b in range(2):
                    # input row i - 1 + py + a, column j - 1 + px + b (+1 in the padded copy)
                    acc += xp[:, i + py + a, j + px + b] @ wc[py, px, a, b]
            rcase = 1 if r == 0 else 2 if r == 2 * h - 1 else 0
            ccase = 1 if c == 0 else 2 if c == 2 * w - 1 else 0
            out[:, r, c] = acc + bc[rcase * 3 + ccase]
    return out


def reference(x, wd, bd, wa, ba):
    d = F.conv_transpose2d(torch.from_numpy(x)[None], torch.from_numpy(wd), torch.from_numpy(bd), stride=2)
    return F.conv2d(d, torch.from_numpy(wa), torch.from_numpy(ba), padding=1)[0].numpy()


def _case(seed, cin, h, w, bias_scale=1.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((cin, h, w))
    wd = rng.standard_normal((cin, 16, 2, 2)) * 0.3
    bd = rng.standard_normal(16) * bias_scale
    wa = rng.standard_normal((16, 16, 3, 3)) * 0.1
    ba = rng.standard_normal(16)
    wc, bc = compose(wd, bd, wa, ba)
    got = composed_forward(x, wc, bc)
    ref = reference(x, wd, bd, wa, ba)
    return got, ref


def test_composition_matches_deconv_then_conv_on_every_border():
    got, ref = _case(0, 5, 4, 5)
    assert got.shape == ref.shape == (16, 8, 10)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max())


def test_border_bias_cases_with_a_dominant_deconv_bias():
    # zero input: every value is the bias table; a wrong border case would differ by whole taps of Wa . bd
    rng = np.random.default_rng(3)
    wd = rng.standard_normal((3, 16, 2, 2))
    bd = rng.standard_normal(16) * 10.0
    wa = rng.standard_normal((16, 16, 3, 3)) * 0.1
    ba = rng.standard_normal(16) * 0.01
    wc, bc = compose(wd, bd, wa, ba)
    x = np.zeros((3, 3, 4))
    got = composed_forward(x, wc, bc)
    ref = reference(x, wd, bd, wa, ba)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max())
    # the nine cases really differ (corners, edges, interior)
    assert len({tuple(np.round(ref[:, r, c], 6)) for r in (0, 3, 5) for c in (0, 3, 7)}) == 9


def test_composition_with_dominant_bias_and_input():
    got, ref = _case(11, 9, 3, 3, bias_scale=20.0)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max())
