"""tests/conv_ref.py against plain torch calls, on the CPU: the NHWC handling, the gate, the residual, the transposed conv's pixel
order, the sentinel channels and the pre-filled destinations - at every shape tests/test_ops_forms_gpu.py uses, so the reference is
known to be good before a device is involved."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref
from tests import test_ops_forms_gpu as forms
from tests import tile_rules as tr


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("cin,n", [(192, n) for n in forms.PROJECT_N] + [(328, 80)])
def test_gated_project_reference(cin, n):
    """out[b,y,x,o] = sum_c x[b,y,x,c] gate[b,c] w[o,c] + bias[o] + resid[b,y,x,o], written out as one einsum."""
    g = gen(n)
    B, H, W = 3, 5, 7
    x, w, b = torch.randn(B, H, W, cin, generator=g), torch.randn(n, cin, 1, 1, generator=g), torch.randn(n, generator=g)
    gate, resid = torch.rand(B, cin, generator=g), torch.randn(B, H, W, n + 8, generator=g)
    want = torch.einsum("byxc,bc,oc->byxo", x.double(), gate.double(), w[:, :, 0, 0].double()) + b.double() + resid[..., :n].double()
    got = conv_ref.conv_forms_ref(x, w, b, gate=gate, resid=resid)
    assert got.dtype == torch.float64 and got.shape == (B, H, W, n)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # a gate row taken from the wrong sample must show
    wrong = conv_ref.conv_forms_ref(x, w, b, gate=gate.roll(1, 0), resid=resid)
    assert (wrong - want).abs().max().item() > 1e-3


@pytest.mark.parametrize("ch", forms.DECONV_CH)
@pytest.mark.parametrize("hw", forms.DECONV_HW)
@pytest.mark.parametrize("B", [1, 2])
def test_transposed_conv_reference(B, hw, ch):
    """out[b, 2y+dy, 2x+dx, o] = sum_c x[b,y,x,c] w[c,o,dy,dx] + bias[o]."""
    g = gen(B + hw[0] + ch[0])
    (h, w_), (cin, cout) = hw, ch
    x, w, b = torch.randn(B, h, w_, cin, generator=g), torch.randn(cin, cout, 2, 2, generator=g), torch.randn(cout, generator=g)
    want = torch.empty(B, 2 * h, 2 * w_, cout, dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            want[:, dy::2, dx::2, :] = torch.einsum("byxc,co->byxo", x.double(), w[:, :, dy, dx].double()) + b.double()
    got = conv_ref.conv_forms_ref(x, w, b, deconv=True)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("extra", [8, 40])
@pytest.mark.parametrize("cin", [40, 104])
@pytest.mark.parametrize("kind,hw,cout", forms.WIDE_CASES)
def test_wide_input_reference(kind, hw, cout, cin, extra):
    """The sentinel channels do not reach the result, and the helper agrees with torch's own fp32 NCHW conv + ReLU."""
    K, stride, pad = {"3x3": (3, 1, 1), "1x1": (1, 1, 0), "k2s2": (2, 2, 0)}[kind]
    g = gen(cout + cin + extra)
    xs = torch.randn(2, hw[0], hw[1], cin, generator=g)
    w, b = torch.randn(cout, cin, K, K, generator=g) / (cin * K * K) ** 0.5, torch.randn(cout, generator=g)
    x = conv_ref.pad_input(xs, cin + extra)
    assert x.shape[3] == cin + extra and bool((x[..., cin:] == conv_ref.SENTINEL).all()) and torch.equal(x[..., :cin], xs)
    got = conv_ref.conv_forms_ref(x, w, b, stride=stride, pad=pad, act=1)
    assert torch.equal(got, conv_ref.conv_forms_ref(xs, w, b, stride=stride, pad=pad, act=1))
    want = F.relu(F.conv2d(xs.permute(0, 3, 1, 2), w, b, stride=stride, padding=pad)).permute(0, 2, 3, 1)
    assert got.shape == want.shape
    assert conv_ref.rel_err(want, got) <= 2e-6      # fp32 torch against the fp64 helper


@pytest.mark.parametrize("shape", tr.WINO_SHAPES)
def test_winograd_shapes_reference(shape):
    B, H, W, cin, cout = shape
    g = gen(sum(shape))
    x, w, b = torch.randn(B, H, W, cin, generator=g), torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5, torch.randn(cout, generator=g)
    want = F.relu(F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)).permute(0, 2, 3, 1)
    assert conv_ref.rel_err(want, conv_ref.conv_forms_ref(x, w, b, pad=1, act=1)) <= 2e-6


def test_swish_and_residual_order():
    g = gen(1)
    x, w, b = torch.randn(1, 3, 3, 8, generator=g), torch.randn(4, 8, 1, 1, generator=g), torch.randn(4, generator=g)
    y = torch.einsum("byxc,oc->byxo", x.double(), w[:, :, 0, 0].double()) + b.double()
    assert torch.allclose(conv_ref.conv_forms_ref(x, w, b, act=2), y * torch.sigmoid(y), rtol=0, atol=1e-14)
    r = torch.randn(1, 3, 3, 4, generator=g)
    assert torch.allclose(conv_ref.conv_forms_ref(x, w, b, act=1, resid=r), F.relu(y) + r.double(), rtol=0, atol=1e-14)   # after the activation


def test_prefilled_destination_checks():
    flat, view = conv_ref.make_dst(2, 3, 4, 10, "cpu")
    assert flat.numel() == 2 * 3 * 4 * 10 + 10 and view.shape == (2, 3, 4, 10) and view.data_ptr() == flat.data_ptr()
    assert bool(torch.isnan(flat).all())
    view[..., 2:7] = 1.0
    assert conv_ref.untouched_outside(flat, view, 2, 5)
    assert not conv_ref.untouched_outside(flat, view, 3, 4) and not conv_ref.untouched_outside(flat, view, 2, 4)
    view[1, 2, 3, 7] = float("nan")                       # another NaN is not the pre-fill
    assert not conv_ref.untouched_outside(flat, view, 2, 5)
    flat2, view2 = conv_ref.make_dst(1, 1, 2, 4, "cpu")
    view2[..., 0:4] = 0.0
    assert conv_ref.untouched_outside(flat2, view2, 0, 4)
    flat2[-1] = 0.0                                       # the guard row behind the last pixel
    assert not conv_ref.untouched_outside(flat2, view2, 0, 4)


def test_rule_table_examples():
    """The rules the GPU tests expect from, on the cases the suite's documents name."""
    assert not tr.tile_runs("conv_pw_160", tr.Launch(2, 16, 16, 480, 80))[0]          # slab of 160 x (480 + 4) floats
    assert not tr.tile_runs("conv_pw_80", tr.Launch(2, 16, 16, 480, 80))[0]
    assert tr.tile_runs("conv_pw_48", tr.Launch(2, 16, 16, 480, 80))[0]
    assert not tr.tile_runs("conv_pw_160", tr.Launch(3, 5, 7, 192, 80, gate=True))[0] and tr.tile_runs("conv_pw_128", tr.Launch(3, 5, 7, 192, 80))[0]
    assert tr.tile_runs("conv_proj_r2", tr.Launch(3, 5, 7, 192, 80, gate=True))[0] and not tr.tile_runs("conv_proj_r2", tr.Launch(3, 5, 7, 192, 80))[0]
    assert not tr.tile_runs("conv_proj_r1", tr.Launch(3, 5, 7, 192, 80, gate=True))[0] and tr.tile_runs("conv_proj_r1", tr.Launch(3, 5, 7, 192, 318, gate=True))[0]
    assert not tr.tile_runs("conv_projl_4", tr.Launch(3, 5, 7, 192, 80, gate=True))[0] and tr.tile_runs("conv_projl_2", tr.Launch(3, 5, 7, 192, 80, gate=True))[0]
    assert not tr.tile_runs("conv_projl_r4", tr.Launch(1, 5, 8, 1152, 320))[0] and tr.tile_runs("conv_projl_r2", tr.Launch(1, 5, 8, 1152, 320))[0]
    assert tr.expected_split("conv_wino4x_64", tr.Launch(2, 16, 32, 88, 64, 3, 1, 1), 66)[0] == 2
    assert tr.expected_split("conv_igemm_64x32_m16", tr.Launch(1, 16, 16, 1152, 192), 72)[0] == 72
    assert tr.expected_split("conv_projl_1", tr.Launch(1, 16, 16, 1152, 192), 8)[0] == 1
