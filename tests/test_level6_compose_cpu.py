"""The algebra of the composed decoder level 6 (tests/level6_ref.py, the float64 restatement of kernels_level6.hip): against
conv(cat[deconv(x), skip]) + ReLU at tiny sizes, for both Winograd forms, also with a transposed-conv bias large enough that a wrong
border case shows."""
import pytest
import torch

from tests import level6_ref as ref

K, CD, CS, N, B = 12, 8, 4, 8, 2


def operands(bias_scale=1.0):
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=r(B, K, 8, 8), skip=r(B, CS, 16, 16), wd=r(K, CD, 2, 2) / K ** 0.5, bd=r(CD) * bias_scale,
                wa=r(N, CD + CS, 3, 3) / (9 * (CD + CS)) ** 0.5, ba=r(N))


@pytest.mark.parametrize("m", [4, 2])
def test_winograd_matrices(m):
    """y[i] = sum_k d[i + k] g[k] for i < m, k < 2, in one dimension."""
    mt = ref.matrices(m)
    g = torch.Generator().manual_seed(m)
    d, f = torch.randn(m + 1, generator=g, dtype=torch.float64), torch.randn(2, generator=g, dtype=torch.float64)
    y = mt["AT"] @ ((mt["G"] @ f) * (mt["BT"] @ d))
    want = torch.stack([d[i] * f[0] + d[i + 1] * f[1] for i in range(m)])
    assert (y - want).abs().max().item() < 1e-13


@pytest.mark.parametrize("m", [4, 2])
@pytest.mark.parametrize("bias_scale", [1.0, 50.0])
def test_composed_equals_direct(m, bias_scale):
    op = operands(bias_scale)
    got = ref.level6_composed(m=m, **op)
    want = ref.level6_direct(**op)
    assert got.shape == want.shape == (B, N, 16, 16)
    assert (want > 0).any() and (want == 0).any()   # the ReLU is active and not everywhere
    assert (got - want).abs().max().item() < 1e-10
    # the border rows and columns (edge and corner bias cases) on their own
    edge = lambda t: torch.cat([t[..., 0, :], t[..., -1, :], t[..., :, 0], t[..., :, -1]], -1)
    assert (edge(got) - edge(want)).abs().max().item() < 1e-10
