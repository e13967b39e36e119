"""tests/split_wino_ref.py - the split Winograd form of a level-6 3x3 layer as kernels_level6.hip runs it - against conv2d in float64:
the three matrices, the row order, the channel padding (C = 12 is not a multiple of 8: four real channels in the last group of a
32-channel k-tile) and the weight order.  1e-10 of the output's scale; also with a bias fifty times the usual, and with ReLU."""
import pytest
import torch

from tests import split_wino_ref as ref

TOL = 1e-10


def case(C, N=8, B=2, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    x = torch.randn(B, C, 16, 16, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64) / (3.0 * C ** 0.5)
    b = torch.randn(N, generator=g, dtype=torch.float64) * 0.1
    return x, w, b


@pytest.mark.parametrize("C", [8, 12])
def test_split_form_is_the_convolution(C):
    x, w, b = case(C)
    want = torch.nn.functional.conv2d(x, w, padding=1)
    got = ref.conv3x3(x, w)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"C {C}: {err:.3g}")
    assert err < TOL


@pytest.mark.parametrize("C", [8, 12])
def test_bias_scaled_by_fifty_and_relu(C):
    x, w, b = case(C)
    b = b * 50.0
    want = torch.nn.functional.conv2d(x, w, b, padding=1)
    got = ref.conv3x3(x, w, b)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"C {C} bias x 50: {err:.3g}")
    assert err < TOL
    got = ref.conv3x3(x, w, b, relu=True)
    assert (got - want.clamp_min(0)).abs().max().item() / want.abs().max().item() < TOL


def test_layouts():
    x, w, _ = case(12)
    V, Wc = ref.transform(x), ref.weights(w)
    assert V.shape == (36, 32, 32) and Wc.shape == (36, 128, 32)               # batch 2: 32 rows, one 32-row tile; Kc 32; Npad 128
    assert V[:, :, 12:].abs().max() == 0 and Wc[:, 8:].abs().max() == 0 and Wc[:, :, 12:].abs().max() == 0
    assert ref.rows(9) == (160, 32) and ref.rows(32) == (512, 64) and ref.rows(64) == (1024, 128)
    assert ref.transform(torch.zeros(9, 4, 16, 16)).shape == (36, 160, 32)     # 144 rows padded to the tile: zero rows
    # position 0 is the corner (r, q) = (0, 0): G[0] = (1/4, 0, 0), so Wc[0] = g[0][0] / 16
    assert torch.allclose(Wc[0, :8, :12], w[:, :, 0, 0] / 16.0, rtol=0, atol=1e-15)
