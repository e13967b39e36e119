"""The decoder's transposed convolutions on their own kernel (deconv_k2s2_kernel, kernels_deconv.hip).

Op level (ccvpe_op_deconv_k2s2) against fp64 torch (tests/conv_ref.py) at the smallest shapes at which the kernel can go wrong: 105
rows (a ragged last row tile, tiles that straddle samples and image rows) at the widths of the levels it serves - the four-tap and the
two-tap form, a scored input whose unused channels hold NaN, an input row wider than the layer, zero columns behind the layer's
channels - one pixel, exactly one row tile; destinations pre-filled and bit-identical to the pre-fill outside their channel slice; a
second launch the same bits; a poisoned sample leaves the others' bits alone.  The bound is the pointwise family's (2e-5 of the
reference's maximum: K <= 168 products of fp32 operands, one rounding each, accumulated in fp32).

Plan level: CCVPE_DECONV_K2S2=1 against =0 (CCVPE_AUTOTUNE=0) on the same seeded weights - outputs and taps to 1e-4 of scale, the
profile rows name the kernel exactly on the launches it serves, repeated and cached forwards bit-equal, the automatic rule."""
import pytest
import torch

from ccvpe_amd import _lib
from tests import conv_ref
from tests import golden_util as gu
from tests import test_level6_composed_gpu as c6

pytestmark = pytest.mark.gpu

TOL = 2e-5
MIN_BATCH, MIN_BATCH_L3 = 8, 16   # DECONV_K2S2_MIN_BATCH, DECONV_K2S2_MIN_BATCH_L3 (ccvpe_internal.h)
SERVED = {f"{d}{lv}.deconv" for d in ("loc", "ori") for lv in (2, 3)}   # the launches whose shapes the kernel takes (every variant)
LEVEL2 = {"loc2.deconv", "ori2.deconv"}                                  # ... and those the automatic rule gives it below MIN_BATCH_L3 samples
FORM = "conv_pw_k2s2"

# (Cin, in_ld, cout, cw, ld, coff), taps a workgroup holds
WIDTHS = {
    "loc2_scored_nan": ((88, 88, 40, 48, 64, 0), 4),
    "ori2": ((64, 64, 32, 32, 48, 0), 4),
    "loc3_two_tap": ((168, 168, 80, 80, 104, 0), 2),
    "wide_input_row": ((128, 136, 64, 64, 88, 0), 2),
    "kitti_level2": ((136, 136, 32, 32, 48, 0), 4),
}
SHAPES = {"ragged": (3, 5, 7), "one_pixel": (1, 1, 1), "one_row_tile": (1, 4, 4)}


def case(width, shape):
    (cin, in_ld, cout, cw, ld, coff), taps = WIDTHS[width]
    B, H, W = SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(4160 + cin + 7 * cout + B * H * W)
    x = torch.randn(B, H, W, cin, device="cuda", generator=g)
    w = torch.randn(cin, cout, 2, 2, device="cuda", generator=g) / cin ** 0.5
    b = torch.randn(cout, device="cuda", generator=g)
    xin = conv_ref.pad_input(x, in_ld)
    if width == "loc2_scored_nan":   # [score | 7 unused | C]: the unused channels have zero weights and must never be multiplied
        w[1:8] = 0.0
        x[..., 1:8] = 0.0
        xin[..., 1:8] = float("nan")
    ref = conv_ref.conv_forms_ref(x, w, b, deconv=True)
    return xin, w, b, ref, (cout, cw, ld, coff), taps


def launch(xin, w, b, dims):
    cout, cw, ld, coff = dims
    B, H, W, _ = xin.shape
    flat, view = conv_ref.make_dst(B, 2 * H, 2 * W, ld, "cuda")
    taps = _lib.op_deconv_k2s2(xin, w, b, view, coff=coff, cw=cw)
    torch.cuda.synchronize()
    return flat, view, taps


OP_CASES = [(wd, "ragged") for wd in WIDTHS] + [(wd, sh) for wd in ("loc2_scored_nan", "loc3_two_tap") for sh in ("one_pixel", "one_row_tile")]


@pytest.mark.parametrize("width,shape", OP_CASES)
def test_op_matches_fp64(width, shape):
    xin, w, b, ref, dims, want_taps = case(width, shape)
    cout, cw, ld, coff = dims
    flat, view, taps = launch(xin, w, b, dims)
    assert taps == want_taps
    err = conv_ref.rel_err(view[..., coff:coff + cout], ref)
    print(f"{width} {shape}: {err:.3g}")
    assert err <= TOL, (width, shape, err)
    assert bool((view[..., coff + cout:coff + cw] == 0).all()), "the columns behind the layer's channels are zeros"
    assert conv_ref.untouched_outside(flat, view, coff, cw)
    flat2, _, _ = launch(xin, w, b, dims)
    assert torch.equal(flat.view(torch.int32), flat2.view(torch.int32)), "a second launch gives other bits"


def test_channel_offset_destination():
    """coff > 0: the slice lands behind 16 channels that stay untouched."""
    xin, w, b, ref, (cout, cw, ld, _), _ = case("ori2", "ragged")
    flat, view, _ = launch(xin, w, b, (cout, cw, ld, 16))
    assert conv_ref.rel_err(view[..., 16:16 + cout], ref) <= TOL
    assert conv_ref.untouched_outside(flat, view, 16, cw)


@pytest.mark.parametrize("width", ["ori2", "loc3_two_tap"])
def test_poisoned_sample_is_isolated(width):
    xin, w, b, _, dims, _ = case(width, "ragged")
    clean, view, _ = launch(xin, w, b, dims)
    bad = xin.clone()
    bad[1] = float("nan")
    _, pview, _ = launch(bad, w, b, dims)
    for s in (0, 2):
        assert torch.equal(view[s].view(torch.int32), pview[s].view(torch.int32)), f"sample {s} changed beside a NaN sample"
    cout, cw, ld, coff = dims
    assert bool(torch.isnan(pview[1][..., coff:coff + cout]).all())


def test_unsupported_shapes_are_refused():
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(1, 2, 2, 328, device="cuda", generator=g)
    for cin, cout, cw, ld, coff in [(328, 160, 160, 200, 0),      # level 4: wider than the kernel's slices
                                    (256, 64, 64, 88, 0),         # more than 192 live channels
                                    (64, 32, 32, 46, 0),          # ld no multiple of 4
                                    (64, 32, 40, 48, 0),          # cw no multiple of 16
                                    (64, 32, 32, 48, 20)]:        # coff + cw > ld
        w = torch.randn(cin, cout, 2, 2, device="cuda", generator=g)
        _, view = conv_ref.make_dst(1, 4, 4, ld, "cuda")
        with pytest.raises(RuntimeError):
            _lib.op_deconv_k2s2(x[..., :cin].contiguous(), w, None, view, coff=coff, cw=cw)


# ---- plans -----------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def forms(m, g, s):
    """launch name -> form of every launch whose profile row names one ("name|form")."""
    return dict(row[0].split("|", 1) for row in m.profile(g, s) if "|" in row[0])


def run(name, batch, switch, monkeypatch):
    """Nine outputs, the level-6 taps and the un-normalised orientation field of one debug forward under CCVPE_DECONV_K2S2=switch with
    CCVPE_AUTOTUNE=0, on the CPU, and the launches that ran the kernel; computed once."""
    key = (name, batch, switch)
    if key not in _RUNS:
        monkeypatch.setenv("CCVPE_DECONV_K2S2", switch)   # read at ccvpe_create
        monkeypatch.setenv("CCVPE_AUTOTUNE", "0")
        m = c6.make(name, c6.state_dict(name, False))
        m.set_debug(True)
        g, s = c6.inputs(name, batch)
        g, s = g.cuda(), s.cuda()
        outs = m(g, s)
        torch.cuda.synchronize()
        _RUNS[key] = dict(outs=[o.cpu() for o in outs], taps={t: m.read_tap(t).cpu() for t in c6.TAPS}, raw=m.read_tap("ori_level1_nchw").cpu(),
                          k2s2={n for n, f in forms(m, g, s).items() if f == FORM})
        monkeypatch.delenv("CCVPE_DECONV_K2S2")
        monkeypatch.delenv("CCVPE_AUTOTUNE")
    return _RUNS[key]


@pytest.mark.parametrize("name,batch", [("vigor_circ", 8), ("vigor_circ", 9), ("kitti", 8)])
def test_plans_match_the_tiled_launches(name, batch, monkeypatch):
    new = run(name, batch, "1", monkeypatch)
    old = run(name, batch, "0", monkeypatch)
    assert new["k2s2"] == SERVED, sorted(new["k2s2"])
    assert old["k2s2"] == set(), sorted(old["k2s2"])
    c6.compare_runs(new, old, f"{name} b{batch} vs DECONV_K2S2=0")


def test_repeated_and_cached_forwards_are_bit_equal(monkeypatch):
    monkeypatch.setenv("CCVPE_DECONV_K2S2", "1")
    monkeypatch.setenv("CCVPE_AUTOTUNE", "0")
    m = c6.make("vigor_circ", c6.state_dict("vigor_circ", False))
    g, s = c6.inputs("vigor_circ", 8)
    g, s = g.cuda(), s.cuda()
    first = [o.clone() for o in m(g, s)]
    assert {n for n, f in forms(m, g, s).items() if f == FORM} == SERVED
    again = m(g, s)
    for i, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a, b), gu.OUTPUT_NAMES[i]
    cache = m.encode_aerial(s)
    cached = m.forward_cached(g, cache)
    for i, (a, b) in enumerate(zip(first, cached)):
        assert torch.equal(a, b), gu.OUTPUT_NAMES[i]


def test_automatic_rule(monkeypatch):
    """Nothing set: the kernel from DECONV_K2S2_MIN_BATCH samples on level 2 and from DECONV_K2S2_MIN_BATCH_L3 on level 3 as well; one
    sample fewer and bf16x3 plans keep the tiled launches."""
    monkeypatch.delenv("CCVPE_DECONV_K2S2", raising=False)
    monkeypatch.setenv("CCVPE_AUTOTUNE", "0")
    sd = c6.state_dict("vigor_circ", False)

    def ran(m, batch):
        g, s = c6.inputs("vigor_circ", batch)
        g, s = g.cuda(), s.cuda()
        m(g, s)
        return {n for n, f in forms(m, g, s).items() if f == FORM}

    auto = c6.make("vigor_circ", sd)
    assert ran(auto, MIN_BATCH - 1) == set()
    assert ran(auto, MIN_BATCH) == LEVEL2
    assert ran(auto, MIN_BATCH_L3 - 1) == LEVEL2
    assert ran(auto, MIN_BATCH_L3) == SERVED
    bf = c6.make("vigor_circ", sd, precision="bf16x3")
    assert ran(bf, MIN_BATCH) == set()
