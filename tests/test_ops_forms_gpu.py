"""Every convolution tile family in every form the plans launch it in - gate, residual, extra destinations with a channel offset,
the pixel-shuffled store of a transposed conv, an input row wider than the layer - through ccvpe_op_conv2d_ex, against fp64 torch
(tests/conv_ref.py, pinned on the CPU by tests/test_conv_ref_cpu.py) at small ragged shapes.

Every launch goes through tile_rules.run_checked: the tile that ran is the one requested with the split the rules derive, or the rule
table names the rule that refuses it, the fallback is asserted and its result is compared all the same; every destination is
pre-filled and must be bit-identical to the pre-fill outside its [coff, coff + Cout) channels.  Bounds are the suite's own
(tile_rules.tol_for), by the tile that ran.  A second identical launch must give the same bits."""
import pytest
import torch

from tests import conv_ref
from tests import tile_rules as tr

pytestmark = pytest.mark.gpu


FAMILIES = ("conv_igemm_", "conv_bf16x3_", "conv_wino4x_", "conv_wino4_", "conv_wino_", "conv_pw_", "conv_proj_r", "conv_projl_")
WORST = {}      # (form, family of the tile that ran) -> worst error of this session, printed by the last test (pytest -rP shows it)


def family_names(*prefixes):
    return [n for n in tr.tile_names() if n.startswith(prefixes)]


def check(x, w, b, name, code, ref, what, **form):
    """run_checked twice: every destination within the bound of the tile that ran, the second launch the same bits."""
    outs, ran, split, as_req = tr.run_checked(x, w, b, name, code, what=what, **form)
    tol = tr.tol_for(ran)
    fam = next(f for f in FAMILIES if ran.startswith(f))
    for k, o in enumerate(outs):
        err = conv_ref.rel_err(o, ref)
        WORST[(what.split()[0], fam)] = max(WORST.get((what.split()[0], fam), 0.0), err)
        assert err <= tol, f"{what} tile {name} code {code} (ran {ran} split {split}) destination {k}: {err:.3g} > {tol:g}"
    again, _, _, _ = tr.run_checked(x, w, b, name, code, what=what, **form)
    for o, a in zip(outs, again):
        assert torch.equal(o, a), f"{what} tile {name} code {code}: a second launch gives other bits"
    return outs, ran, split


def rand(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


# ---- case 1: the MBConv project conv: gated 1x1, residual, extra destinations ---------------------------------------------------
PROJECT_N = [80, 72, 112, 100, 192, 184, 320, 318]    # 5 / 7 / 12 / 20 column tiles, full and ragged; 318: the scalar epilogue
PROJECT_VARIANTS = ["gate", "gate_resid", "gate_resid_dst2", "gate_resid_dst2_odd_ld"]
NON_WINO = ("conv_igemm_", "conv_bf16x3_", "conv_pw_", "conv_proj_r", "conv_projl_")


def project_case(cin, n, variant, seed):
    """B = 3 samples of 5 x 7 = 35 rows: 16-, 32-, 64- and 128-row tiles all straddle samples."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    B, H, W = 3, 5, 7
    x = rand(g, B, H, W, cin)
    w = rand(g, n, cin, 1, 1) / cin ** 0.5
    b = rand(g, n)
    gate = torch.rand(B, cin, device="cuda", generator=g)
    form = {"gate": gate}
    if variant != "gate":
        form["resid"] = rand(g, B, H, W, n + 8).contiguous()
    if variant == "gate_resid_dst2":
        form["dst_specs"] = [(n, 0), (n + 24, 8)]
    if variant == "gate_resid_dst2_odd_ld":
        form["dst_specs"] = [(n, 0), (n + 25, 8)]       # a row that is no multiple of 4 floats: the element-wise epilogue
    ref = conv_ref.conv_forms_ref(x, w, b, gate=gate, resid=form.get("resid"))
    return x, w, b, form, ref


@pytest.mark.parametrize("variant", PROJECT_VARIANTS)
@pytest.mark.parametrize("n", PROJECT_N)
def test_gated_project_forms(n, variant):
    x, w, b, form, ref = project_case(192, n, variant, 1000 + n)
    for name in family_names(*NON_WINO):
        check(x, w, b, name, 0, ref, f"project N {n} {variant}", **form)


def test_gated_project_cin_not_multiple_of_16():
    """Cin = 328: conv_proj_* and the gated latency form must refuse it (the rule table says so and run_checked asserts the
    fallback); the implicit GEMM and the pointwise tiles whose slab fits run it."""
    x, w, b, form, ref = project_case(328, 80, "gate_resid_dst2", 1328)
    for name in family_names(*NON_WINO):
        check(x, w, b, name, 0, ref, "project Cin 328", **form)


SPLIT_TILES = ("conv_igemm_64x32_m16", "conv_igemm_64x64_m32_s1", "conv_igemm_128x128_m16")


@pytest.mark.parametrize("n", [192, 318])
def test_gated_project_split_k(n):
    """splitk_reduce_kernel and splitk_finish repeat the gate-free sum, bias, residual and both destinations."""
    x, w, b, form, ref = project_case(192, n, "gate_resid_dst2", 1500 + n)
    for name in SPLIT_TILES:
        plain, _, s0 = check(x, w, b, name, 4, ref, f"project N {n} split", **form)
        fused, _, s1 = check(x, w, b, name, 64 + 4, ref, f"project N {n} split", **form)
        assert (s0, s1) == (4, 68)
        for p, f in zip(plain, fused):
            assert torch.equal(p, f), f"{name}: the self-reducing split and slab + reduce differ"


# ---- case 2: the decoder's transposed conv into a concat row -----------------------------------------------------------------
DECONV_HW = [(5, 12), (7, 9), (8, 8)]
DECONV_CH = [(1288, 64), (320, 40), (128, 6)]    # deep K that is no multiple of 16; the narrow pointwise slabs only; cout % 4 != 0


def deconv_case(B, hw, ch, offset):
    h, w_ = hw
    cin, cout = ch
    g = torch.Generator(device="cuda").manual_seed(2000 + B + 7 * h + w_ + cin)
    x = rand(g, B, h, w_, cin)
    w = rand(g, cin, cout, 2, 2) / cin ** 0.5
    b = rand(g, cout)
    form = {"deconv": True}
    if offset:
        form["dst_specs"] = [(cout + 24, 8)]
    return x, w, b, form, conv_ref.conv_forms_ref(x, w, b, deconv=True)


@pytest.mark.parametrize("offset", [True, False])
@pytest.mark.parametrize("ch", DECONV_CH)
@pytest.mark.parametrize("hw", DECONV_HW)
@pytest.mark.parametrize("B", [1, 2])
def test_transposed_conv_forms(B, hw, ch, offset):
    x, w, b, form, ref = deconv_case(B, hw, ch, offset)
    for name in family_names(*NON_WINO):
        check(x, w, b, name, 0, ref, f"deconv B {B} {hw} {ch} offset {offset}", **form)


def test_transposed_conv_split_k():
    x, w, b, form, ref = deconv_case(2, (7, 9), (1288, 64), True)
    for name in SPLIT_TILES:
        plain, _, _ = check(x, w, b, name, 8, ref, "deconv split", **form)
        fused, _, _ = check(x, w, b, name, 64 + 8, ref, "deconv split", **form)
        assert torch.equal(plain[0], fused[0]), f"{name}: the self-reducing split and slab + reduce differ"
    for name in family_names("conv_projl_") + ["conv_bf16x3_64x64_m32", "conv_pw_16"]:
        for code in (8, 64 + 8):
            check(x, w, b, name, code, ref, "deconv split", **form)


# ---- case 3: an input row wider than the layer (a conv that reads a concat tensor) ------------------------------------------
X_COUTS = [32, 40, 64, 80, 88, 100]      # one Cout per xi-split width WINO_SHAPES uses (32, 48, 64, 80, 96, 128)
WIDE_CASES = ([("3x3", (16, 32), co) for co in X_COUTS] + [("3x3", (19, 23), co) for co in (40, 88)] +
              [(k, hw, co) for k in ("1x1", "k2s2") for hw in ((16, 32), (19, 23)) for co in (40, 88)])


@pytest.mark.parametrize("extra", [8, 40])
@pytest.mark.parametrize("cin", [40, 104])
@pytest.mark.parametrize("kind,hw,cout", WIDE_CASES)
def test_input_wider_than_layer(kind, hw, cout, cin, extra):
    K, stride, pad = {"3x3": (3, 1, 1), "1x1": (1, 1, 0), "k2s2": (2, 2, 0)}[kind]
    g = torch.Generator(device="cuda").manual_seed(3000 + cout + cin + extra + hw[0] + K)
    xs = rand(g, 2, hw[0], hw[1], cin)
    x = conv_ref.pad_input(xs, cin + extra)           # the pad channels hold 1e30
    w = rand(g, cout, cin, K, K) / (cin * K * K) ** 0.5
    b = rand(g, cout)
    ref = conv_ref.conv_forms_ref(x, w, b, stride=stride, pad=pad, act=1)
    families = ("conv_igemm_", "conv_bf16x3_") + (("conv_wino",) if K == 3 else ("conv_pw_", "conv_proj_r", "conv_projl_"))
    for name in family_names(*families):
        check(x, w, b, name, 0, ref, f"{kind} {hw} Cin {cin}+{extra} Cout {cout}", stride=stride, pad=pad, act=1)


# ---- case 4: Winograd into an offset destination ----------------------------------------------------------------------------
@pytest.mark.parametrize("coff", [8, 6])
@pytest.mark.parametrize("shape", tr.WINO_SHAPES)
def test_winograd_offset_destination(shape, coff):
    """ld = N + 16 rounded to the 16-byte path where N allows it; coff = 6 is off that path: F(2x2) and F(4x4) must refuse it (the
    xi-split form stores one channel per lane and has no such rule).  Plain, split-K 2 and its self-reducing form."""
    B, H, W, cin, cout = shape
    g = torch.Generator(device="cuda").manual_seed(4000 + sum(shape) + coff)
    x = rand(g, B, H, W, cin)
    w = rand(g, cout, cin, 3, 3) / (cin * 9) ** 0.5
    b = rand(g, cout)
    ref = conv_ref.conv_forms_ref(x, w, b, pad=1, act=1)
    for name in family_names("conv_wino"):
        for code in (0, 2, 64 + 2):
            if code and cin < 32:
                continue          # fewer than two 16-channel groups: the F(4x4) launchers clamp such a split to one slice
            check(x, w, b, name, code, ref, f"wino {shape} coff {coff}", pad=1, act=1, dst_specs=[(cout + 16, coff)])


# ---- case 5: a poisoned sample does not move its batch neighbours ------------------------------------------------------------
def poisoned(t):
    """sample 1 of a [3, ...] tensor all NaN"""
    p = t.clone()
    p[1] = float("nan")
    return p


def check_isolated(x, w, b, name, code, what, **form):
    """run_checked on the clean launch and on the same launch with sample 1 of x (and of its gate and residual) all NaN: the same
    tile and split, samples 0 and 2 of every destination the same bits, nothing written outside the destinations either time.
    Neither launch is held to an error bound here, so neither is recorded as "ran as requested" (tile_rules.RAN): that record stays
    with the cases that compare with the fp64 reference.  With an activation (act = 1: the device's ReLU is a maximum, which returns 0
    for a NaN) sample 1 of the result need not be NaN; the NaN is in every input tile the kernel reads all the same."""
    clean, ran, split, _ = tr.run_checked(x, w, b, name, code, what=what, record=False, **form)
    bad_form = {k: (poisoned(v) if k in ("gate", "resid") else v) for k, v in form.items()}
    bad, ran2, split2, _ = tr.run_checked(poisoned(x), w, b, name, code, what=what + " poisoned", record=False, **bad_form)
    assert (ran2, split2) == (ran, split), f"{what} tile {name} code {code}: {ran} / {split} clean, {ran2} / {split2} poisoned"
    for k, (c, p) in enumerate(zip(clean, bad)):
        assert not bool(torch.isnan(c).any())
        for s in (0, 2):
            assert torch.equal(c[s], p[s]), (f"{what} tile {name} code {code} (ran {ran} split {split}) destination {k}: sample {s} moved "
                                             f"at {(c[s] != p[s]).nonzero()[:4].tolist()} when sample 1 was poisoned")
        if not form.get("act"):
            assert bool(torch.isnan(p[1]).all()), f"{what} tile {name} code {code}: the poison did not reach sample 1"


ISOLATION_CODES = (0, 4, 64 + 4)


@pytest.mark.parametrize("n", [80, 192])
def test_poisoned_sample_gated_project(n):
    """project_case: 3 samples of 35 rows, every row tile straddles samples; gate, residual and two destinations (the form that
    holds every operand a sample owns: its rows of x, its gate vector, its residual rows), at 5 and 12 column tiles"""
    x, w, b, form, _ = project_case(192, n, "gate_resid_dst2", 6000 + n)
    for name in family_names(*NON_WINO):
        for code in ISOLATION_CODES:
            check_isolated(x, w, b, name, code, f"isolation project N {n}", **form)


@pytest.mark.parametrize("ch", [(1288, 64), (320, 40)])
def test_poisoned_sample_transposed_conv_offset(ch):
    x, w, b, form, _ = deconv_case(3, (5, 7), ch, True)
    for name in family_names(*NON_WINO):
        check_isolated(x, w, b, name, 0, f"isolation deconv {ch}", **form)
    for name in list(SPLIT_TILES) + family_names("conv_projl_") + ["conv_bf16x3_64x64_m32", "conv_pw_16"]:
        for code in ISOLATION_CODES[1:]:
            check_isolated(x, w, b, name, code, f"isolation deconv {ch}", **form)


def test_poisoned_sample_winograd():
    B, H, W, cin, cout = tr.WINO_SHAPES[1]          # 3 x 16 x 16 x 64 -> 88
    assert B == 3
    g = torch.Generator(device="cuda").manual_seed(6500)
    x = rand(g, B, H, W, cin)
    w = rand(g, cout, cin, 3, 3) / (cin * 9) ** 0.5
    b = rand(g, cout)
    for name in family_names("conv_wino", "conv_igemm_", "conv_bf16x3_"):
        for code in ISOLATION_CODES:
            check_isolated(x, w, b, name, code, "isolation wino", pad=1, act=1, dst_specs=[(cout + 16, 8)])


@pytest.mark.parametrize("width", [(40, True, 1), (32, True, 1), (32, False, 2), (24, True, 1)])
def test_poisoned_sample_level1(width):
    """ccvpe_op_level1 at B = 3: 48 x 96 outputs are 3 x 3 tiles of 32 x 16 per sample, 8 workgroups loop over the 27 tiles (54 of
    16 x 16), so a workgroup's run crosses both sample boundaries"""
    from ccvpe_amd import _lib
    cd, score, cout = width
    cin = cd + (1 if score else 0)
    g = torch.Generator(device="cuda").manual_seed(6600 + cd + cout)
    x = rand(g, 3, 24, 48, cin)
    ws = [rand(g, cin, 16, 2, 2) / (4 * cin) ** 0.5, rand(g, 16), rand(g, 16, 16, 3, 3) / 12.0, rand(g, 16) * 0.5,
          rand(g, cout, 16, 3, 3) / 12.0, rand(g, cout) * 0.5]
    for tile in (0, 1):
        clean, ran = _lib.op_level1(x, *ws, score=score, tile=tile, max_wg=8)
        bad, ran2 = _lib.op_level1(poisoned(x), *ws, score=score, tile=tile, max_wg=8)
        assert ran == ran2 == tile and not bool(torch.isnan(clean).any())
        for s in (0, 2):
            assert torch.equal(clean[s], bad[s]), f"level1 {width} tile {tile}: sample {s} moved when sample 1 was poisoned"


# ---- every tile of the registry ran somewhere ----------------------------------------------------------------------------
def test_every_registry_tile_ran():
    """Every name of the registry must have been seen to run as requested by a checked launch.  The launches below give each
    family its smallest admitting shape, so the test also stands alone; the cases above and tests/test_ops_gpu.py add to the
    same record."""
    g = torch.Generator(device="cuda").manual_seed(5000)
    names = tr.tile_names()
    # a 3x3 conv per xi-split width (and F(2x2), F(4x4), implicit GEMM, bf16x3)
    for cout in X_COUTS:
        x, w, b = rand(g, 1, 16, 16, 24), rand(g, cout, 24, 3, 3) / 15.0, rand(g, cout)
        ref = conv_ref.conv_forms_ref(x, w, b, pad=1)
        L = tr.Launch(1, 16, 16, 24, cout, 3, 1, 1)
        for name in names:
            if tr.tile_runs(name, L)[0] and name not in tr.RAN:
                check(x, w, b, name, 0, ref, f"3x3 Cout {cout}", pad=1)
    # the gated project widths of PROJ_CFGS; the pointwise tiles (K = 192 fits every slab)
    for n in (80, 112, 192, 320):
        x, w, b, form, ref = project_case(192, n, "gate", 5000 + n)
        L = tr.Launch(3, 5, 7, 192, n, gate=True)
        for name in names:
            if tr.tile_runs(name, L)[0] and name not in tr.RAN:
                check(x, w, b, name, 0, ref, f"project N {n}", **form)
    # the latency forms without a gate: 64 rows for conv_projl_r4
    x, w, b = rand(g, 1, 8, 8, 480), rand(g, 48, 480, 1, 1) / 22.0, rand(g, 48)
    ref = conv_ref.conv_forms_ref(x, w, b)
    L = tr.Launch(1, 8, 8, 480, 48)
    for name in names:
        if tr.tile_runs(name, L)[0] and name not in tr.RAN:
            check(x, w, b, name, 0, ref, "1x1 K 480")
    # conv_pw_160: a slab of 160 rows fits up to K = 160
    x, w, b = rand(g, 1, 5, 7, 40), rand(g, 160, 40, 1, 1) / 6.0, rand(g, 160)
    check(x, w, b, "conv_pw_160", 0, conv_ref.conv_forms_ref(x, w, b), "1x1 K 40")
    for (form, fam), err in sorted(WORST.items()):
        print(f"worst error {form:8s} {fam:14s} {err:.3g}")
    never = [n for n in names if n not in tr.RAN]
    assert not never, f"tiles that no checked launch ran as requested: {never}"
