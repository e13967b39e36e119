"""Parity of the HIP path (through the C ABI) against the reference golden vectors and the CPU oracle.

Tolerance: BASELINE.json north_star asks for 1e-3 relative fp32; errors are measured relative to each
tensor's max |value|.  The fp32-MFMA path is exact fp32 arithmetic, so we hold it to 1e-4 - tighter
than the contract - and the contract bound is asserted separately.
"""
import numpy as np
import pytest
import torch

from ccvpe_amd import models, weights
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

CONTRACT_RTOL = 1e-3
RTOL = 1e-4


def build_model(cfg, micro_batch=0, precision="fp32"):
    v = cfg["variant"]
    kw = dict(micro_batch=micro_batch, precision=precision)
    if v == "vigor":
        m = models.CVM_VIGOR("cuda", cfg["circular"], **kw)
    elif v == "vigor_ori_prior":
        m = models.CVM_VIGOR_ori_prior("cuda", cfg["ori_noise"], cfg["circular"], **kw)
    elif v == "kitti":
        m = models.CVM_KITTI("cuda", **kw)
    else:
        m = models.CVM_OxfordRobotCar("cuda", **kw)
    m.load_state_dict(weights.generate_state_dict(v, cfg["seed"]))
    return m.to("cuda").eval()


def inputs(cfg, batch=None):
    g, s = weights.generate_inputs(cfg["variant"], batch or cfg["batch"], cfg["seed"], cfg["fov"])
    return torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()


def raw_ori_magnitude(cfg, g, s, precision="fp32"):
    """|un-normalised orientation vector| per pixel [B,1,512,512] (CPU), from a debug run of the same model on the same inputs:
    the weight of every comparison of the unit (cos, sin) field - F.normalize is ill-conditioned where the raw vector is ~0."""
    m = build_model(cfg, precision=precision)
    m.set_debug(True)
    m(g, s)
    raw = m.read_tap("ori_level1_nchw")
    return raw.pow(2).sum(dim=1, keepdim=True).sqrt()


def ori_weighted_error(a, b, mag):
    """max |a - b| * mag / max mag: the unit orientation fields a, b [n,2,512,512] compared where they are well defined."""
    return ((a.cpu() - b.cpu()).abs() * mag).max().item() / mag.max().item()


def launch_tiles(m, g, s):
    """Launch name -> tile of every tiled launch of the model's plan for (g, s), from its profile rows ("name|tile")."""
    return dict(row[0].split("|", 1) for row in m.profile(g, s) if "|" in row[0])


def assert_hook_moved(forced, default, family):
    """A candidate-filter hook took effect: at least one launch runs a tile of `family` under it that the default plan of the same
    model does not run there (the hook not honoured: the same tuner, the same choices)."""
    moved = [op for op, t in forced.items() if t.startswith(family) and not default.get(op, "").startswith(family)]
    assert moved, f"no launch moved onto a {family} tile: {forced}"


def check_against_fixture(fx, outs, rtol):
    worst = 0.0
    for n, t in zip(gu.OUTPUT_NAMES, outs):
        if n == "ori":
            continue
        worst = max(worst, gu.compare(n, fx, t.cpu().numpy(), rtol))
    ori = outs[2].cpu().numpy().reshape(-1)
    idx = gu.lattice(ori.size)
    mag = fx["ori/magnitude"].astype(np.float64)
    err = (np.abs(ori[idx].astype(np.float64) - fx["ori/values"].astype(np.float64)) * mag).max() / mag.max()
    assert err <= rtol, f"ori: magnitude-weighted error {err:.3g}"
    return max(worst, err)


@pytest.mark.parametrize("name", list(gu.CONFIGS))
def test_forward_matches_reference_golden(name):
    cfg = gu.CONFIGS[name]
    fx = gu.load(name)
    m = build_model(cfg)
    g, s = inputs(cfg)
    outs = m(g, s)
    assert len(outs) == 9 and all(o.is_cuda and o.dtype == torch.float32 for o in outs)
    worst = check_against_fixture(fx, outs, RTOL)
    assert worst <= CONTRACT_RTOL
    # outputs are fresh tensors owned by the caller (a second call must not alias them)
    again = m(g, s)
    assert again[0].data_ptr() != outs[0].data_ptr()
    assert torch.equal(again[0], outs[0]), "forward is deterministic run to run"
    # test-loop post-processing on device vs the reference's numpy result
    post = m.postprocess(outs[1], outs[2])
    assert np.array_equal(post["index"].cpu().numpy(), fx["post/index"])
    assert np.allclose(post["prob"].cpu().numpy(), fx["post/prob"], rtol=1e-3)
    assert np.allclose(post["cos"].cpu().numpy(), fx["post/cos"], atol=2e-3)
    assert np.allclose(post["sin"].cpu().numpy(), fx["post/sin"], atol=2e-3)


def test_intermediate_taps_match_reference_golden():
    cfg = gu.CONFIGS["vigor_prior180_circ"]
    fx = gu.load("vigor_prior180_circ")
    m = build_model(cfg)
    m.set_debug(True)
    g, s = inputs(cfg)
    m(g, s)
    for tap in ["sat_block0", "sat_block2", "sat_block4", "sat_block10", "sat_block15", "grd_desc1", "grd_desc3", "grd_desc6",
                "loc_level6", "loc_level4", "loc_level2", "ori_level6", "ori_level3"]:
        t = m.read_tap(tap).numpy()
        if tap.startswith("grd_desc"):
            t = t.reshape(t.shape[0], -1)
        gu.compare("tap_" + tap, fx, t, RTOL)
    gu.compare("tap_ori_level1", fx, m.read_tap("ori_level1_nchw").numpy(), RTOL)


def test_full_tensor_against_oracle_oxford():
    """Full-tensor comparison (not just the lattice) on the smallest-ground variant, odd image sizes."""
    from oracle import ccvpe_oracle as orc
    cfg = gu.CONFIGS["oxford"]
    sd = weights.generate_state_dict("oxford", 11)
    g, s = weights.generate_inputs("oxford", 2, 11)
    taps = {}
    ref = orc.forward("oxford", sd, torch.from_numpy(g), torch.from_numpy(s), taps=taps)
    m = models.CVM_OxfordRobotCar("cuda")
    m.load_state_dict(sd)
    m.to("cuda").eval()
    outs = m(torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda())
    mag = taps["ori_level1"].pow(2).sum(dim=1, keepdim=True).sqrt()
    for i, (a, b) in enumerate(zip(ref, outs)):
        if i == 2:   # unit orientation field: weighted by the oracle's un-normalised magnitude
            assert ori_weighted_error(a, b, mag) <= 5 * RTOL
            continue
        err = (a - b.cpu()).abs().max().item() / a.abs().max().item()
        # full tensors include the worst-conditioned cosine scores (near-cancelling 224-term dot products);
        # hold them to half the 1e-3 contract rather than the lattice's 1e-4
        assert err <= 5 * RTOL, f"{gu.OUTPUT_NAMES[i]}: {err:.3g}"


def test_batch32_properties_and_micro_batching():
    """BASELINE config 2 shape (B=32): size-independent properties + consistency with B=1 and with
    an internal micro-batch that does not divide the batch."""
    cfg = gu.CONFIGS["vigor_prior180_circ"]
    m = build_model(cfg)
    g, s = inputs(cfg, batch=32)
    outs = m(g, s)
    logits, heat, ori = outs[0], outs[1], outs[2]
    assert torch.isfinite(logits).all()
    sums = heat.double().sum(dim=(1, 2, 3))
    assert torch.allclose(sums, torch.ones_like(sums), atol=1e-4), "softmax over 512*512 sums to 1 per sample"
    assert torch.allclose(heat.flatten(1), torch.softmax(logits, dim=1), rtol=2e-4, atol=1e-9)
    norm = ori.double().pow(2).sum(dim=1).sqrt()
    assert (norm - 1).abs().max().item() < 1e-4, "orientation field is unit-norm everywhere"
    for k in range(6):
        assert outs[3 + k].abs().max().item() <= 1.0 + 1e-5, "cosine scores are bounded by 1"
    # sample 0 of the generator at batch 32 == the single golden sample (same seed, same first draw?) - use B=1 run instead
    one = m(g[5:6], s[5:6])
    # the unit orientation field (index 2) is compared weighted by the un-normalised magnitude (a debug run of the same batch):
    # F.normalize amplifies last-bit differences where the raw vector is tiny
    mag = raw_ori_magnitude(cfg, g, s)
    assert ori_weighted_error(ori[5:6], one[2], mag[5:6]) <= 1e-4, "batch-size invariance (ori)"
    for i, (a, b) in enumerate(zip(outs, one)):
        if i != 2:
            # the batch-1 plan autotunes different tiles (implicit GEMM / F(2x2) where the batch-32 plan runs Winograd F(4x4),
            # 1.4e-5 of scale per layer against fp64): 1e-4 of the tensor's scale, a tenth of the path's contract
            assert (a[5:6] - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-30), "batch-size invariance"
    # permutation equivariance
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(1)).cuda()
    outs_p = m(g[perm], s[perm])
    assert (outs_p[0] - logits[perm]).abs().max().item() <= 2e-5 * logits.abs().max().item()
    # micro-batch 5 (32 = 6*5 + 2): looped passes must agree with the single pass
    m5 = build_model(cfg, micro_batch=5)
    outs5 = m5(g, s)
    for i, (a, b) in enumerate(zip(outs, outs5)):
        if i != 2:
            assert (a - b).abs().max().item() <= 2e-5 * max(a.abs().max().item(), 1e-30)
    assert ori_weighted_error(ori, outs5[2], mag) <= 2e-5, "micro-batching (ori)"


def test_argument_errors_are_loud():
    cfg = gu.CONFIGS["kitti"]
    m = build_model(cfg)
    g, s = inputs(cfg)
    with pytest.raises(RuntimeError):
        m(g[:, :, :250], s)            # ground height that does not give 8 feature rows
    with pytest.raises(ValueError):
        m(g, s[:, :, :256, :256])
    with pytest.raises(RuntimeError):
        m(g.cpu(), s.cpu())


def test_reload_state_dict_changes_result():
    cfg = gu.CONFIGS["oxford"]
    m = build_model(cfg)
    g, s = inputs(cfg)
    a = m(g, s)[0].clone()
    m.load_state_dict(weights.generate_state_dict("oxford", 99))
    b = m(g, s)[0]
    assert not torch.allclose(a, b)
    m.load_state_dict(weights.generate_state_dict("oxford", cfg["seed"]))
    c = m(g, s)[0]
    # re-ingesting the weights rebuilds the plan from the handle's tuning table: the same launches, the same bits
    assert torch.equal(a, c)


@pytest.mark.parametrize("name", ["vigor_prior180_circ", "kitti", "oxford"])
def test_bf16x3_mode_stays_inside_the_contract(name):
    """Opt-in precision mode: fp32 operands split into two bf16, three bf16 MFMAs per product.  Expected error
    ~1e-5 of each tensor's scale; asserted at 5e-4 (half the 1e-3 contract)."""
    cfg = gu.CONFIGS[name]
    fx = gu.load(name)
    m = build_model(cfg, precision="bf16x3")
    g, s = inputs(cfg)
    outs = m(g, s)
    worst = check_against_fixture(fx, outs, 5e-4)
    assert worst <= CONTRACT_RTOL
    post = m.postprocess(outs[1], outs[2])
    assert np.array_equal(post["index"].cpu().numpy(), fx["post/index"])


@pytest.mark.parametrize("name,batch,mode", [
    ("vigor_prior180_circ", 1, "fp32"), ("vigor_prior180_circ", 6, "fp32"), ("kitti", 2, "fp32"), ("oxford", 1, "fp32"),
    ("vigor_prior72_fov108", 5, "fp32"), ("vigor_circ", 3, "fp32"),
    # the small-grid implicit-GEMM decoder (no persistent Winograd grids that fill the chip) under two streams
    ("vigor_prior180_circ", 6, "fp32-igemm"),
    # bf16x3: two streams since round 2.  Round 1's run-to-run differences were a gfx950 hazard, not a missing edge:
    # packed fp32 VALU ops with op_sel[1] = 1 (match_kernel via the SLP vectoriser, conv_wino_kernel by hand) go wrong in
    # lanes 48-63 beside another wave's bf16 MFMAs (tools/repro_pk_mfma.hip); bf16x3 plans no longer
    # contain such kernels (tests/test_isa_hazard.py).  Batch 32 is the configuration that showed it.
    ("vigor_prior180_circ", 6, "bf16x3"), ("kitti", 2, "bf16x3"), ("vigor_prior180_circ", 32, "bf16x3"), ("oxford", 1, "bf16x3"),
])
def test_two_stream_schedule_is_bitwise_identical_to_program_order(name, batch, mode, monkeypatch):
    """The second stream (aerial encoder, orientation decoder) only changes WHEN kernels run.  One handle, so the
    autotuned tiles / split-K choices are the same: every output of the two-stream schedule must be bit-identical to
    the same plan issued in program order on one stream (ccvpe_set_streams), for the eager path and for the hipGraph
    replay path (batch <= 4: three calls, so the captured graph is what is compared)."""
    cfg = gu.CONFIGS[name]
    g, s = inputs(cfg, batch=batch)
    if mode == "fp32-igemm":
        monkeypatch.setenv("CCVPE_WINOGRAD", "0")
    if batch <= 4:
        monkeypatch.setenv("CCVPE_GRAPH", "1")   # hipGraph replay is opt-in since round 4: the small batches keep covering it
    m = build_model(cfg, precision="bf16x3" if mode == "bf16x3" else "fp32")
    results = []
    for n_streams in (2, 1, 2):
        m.set_streams(n_streams)
        outs = None
        for _ in range(3):
            outs = m(g, s)
        torch.cuda.synchronize()
        results.append([o.clone() for o in outs])
    for a, b, c in zip(*results):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("name", ["vigor_prior180_circ", "kitti"])
def test_pointwise_persistent_tiles_everywhere_match_golden(name, monkeypatch):
    """CCVPE_TUNE_PREFER_PW routes every 1x1 layer with K <= 512 (expand, gated project with residual and concat taps,
    head, transposed convs with the pixel-shuffle epilogue) through conv_pw_kernel, whatever the autotuner would pick."""
    monkeypatch.setenv("CCVPE_TUNE_PREFER_PW", "1")
    cfg = gu.CONFIGS[name]
    fx = gu.load(name)
    m = build_model(cfg)
    g, s = inputs(cfg)
    worst = check_against_fixture(fx, m(g, s), RTOL)
    assert worst <= CONTRACT_RTOL
    # choices measured under a candidate filter stay in the handle's plans: nothing is recorded, exported or written to the shared cache
    from ccvpe_amd import _lib
    assert _lib.load().ccvpe_tuning_generation(m._handle) == 0
    # the hook took effect (pointwise family: conv_pw_* and the deep-K conv_proj* tiles)
    forced = launch_tiles(m, g, s)
    monkeypatch.delenv("CCVPE_TUNE_PREFER_PW")
    default = launch_tiles(build_model(cfg), g, s)
    assert_hook_moved(forced, default, "conv_pw_")


@pytest.mark.parametrize("name,batch", [("vigor_prior180_circ", 1), ("kitti", 1), ("oxford", 3)])
def test_deep_k_project_gemm_everywhere_matches_golden(name, batch, monkeypatch):
    """CCVPE_TUNE_PREFER_PROJ routes every gated project conv whose width conv_proj_kernel takes (80 / 112 / 192 / 320 columns, K = 240
    .. 1152 split over a workgroup's four waves, residual and concat-tap epilogues) through it, whatever the autotuner would pick:
    goldens for the 9 outputs plus the aerial encoder taps; Oxford's 10 x 15 / 5 x 8 maps give ragged row tiles that span samples."""
    monkeypatch.setenv("CCVPE_TUNE_PREFER_PROJ", "1")
    cfg = gu.CONFIGS[name]
    fx = gu.load(name)
    m = build_model(cfg)
    if batch == cfg["batch"]:
        m.set_debug(True)
        g, s = inputs(cfg)
        worst = check_against_fixture(fx, m(g, s), RTOL)
        assert worst <= CONTRACT_RTOL
        if name == "vigor_prior180_circ":
            for tap in ["sat_block4", "sat_block10", "sat_block15"]:
                gu.compare("tap_" + tap, fx, m.read_tap(tap).numpy(), RTOL)
        monkeypatch.delenv("CCVPE_TUNE_PREFER_PROJ")
        ref_model = build_model(cfg)
    else:   # a batch the goldens do not hold: against the default plan of the same model
        g, s = inputs(cfg, batch=batch)
        out = [t.clone() for t in m(g, s)]
        monkeypatch.delenv("CCVPE_TUNE_PREFER_PROJ")
        ref_model = build_model(cfg)
        ref = ref_model(g, s)
        mag = raw_ori_magnitude(cfg, g, s)
        for i, (a, b) in enumerate(zip(ref, out)):
            if i == 2:
                assert ori_weighted_error(a, b, mag) <= 1e-4
            else:
                assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]
    # the hook took effect: the deep-K GEMM (conv_proj_r*, or its latency form conv_projl_*) on launches the default plan runs elsewhere
    assert_hook_moved(launch_tiles(m, g, s), launch_tiles(ref_model, g, s), "conv_proj")


@pytest.mark.parametrize("name,batch", [("vigor_prior180_circ", 1), ("kitti", 1), ("oxford", 1), ("oxford", 3), ("vigor_prior180_b2", 2)])
def test_latency_form_project_gemm_matches_golden(name, batch, monkeypatch):
    """Round 4: conv_proj_lat_kernel (sixteen waves of a workgroup split K, every operand requested up front, partial sums meet in LDS;
    the batch <= 4 form of the gated project convs of blocks 5-15, model.py:113-122) forced wherever it applies (CCVPE_TUNE_PREFER_PROJ=lat)
    against the goldens: residual and concat-tap epilogues, Oxford's 40-row maps (ragged row tiles that span samples at batch 3)."""
    monkeypatch.setenv("CCVPE_TUNE_PREFER_PROJ", "lat")
    cfg = gu.CONFIGS[name]
    m = build_model(cfg)
    if batch == cfg["batch"]:
        fx = gu.load(name)
        m.set_debug(True)
        g, s = inputs(cfg)
        worst = check_against_fixture(fx, m(g, s), RTOL)
        assert worst <= CONTRACT_RTOL
        if name == "vigor_prior180_circ":
            for tap in ["sat_block4", "sat_block10", "sat_block15"]:
                gu.compare("tap_" + tap, fx, m.read_tap(tap).numpy(), RTOL)
    else:
        g, s = inputs(cfg, batch=batch)
        out = [t.clone() for t in m(g, s)]
    # the hook took effect: the latency form runs, and no gated project conv it covers (every one the deep-K GEMM takes: blocks 5-15,
    # at most 4096 rows at these batches) runs the throughput form conv_proj_r*
    forced = launch_tiles(m, g, s)
    assert any(t.startswith("conv_projl_") for t in forced.values()), forced
    assert not [op for op, t in forced.items() if op.endswith(".project") and t.startswith("conv_proj_r")], forced
    if batch != cfg["batch"]:
        monkeypatch.delenv("CCVPE_TUNE_PREFER_PROJ")
        ref = build_model(cfg)(g, s)
        mag = raw_ori_magnitude(cfg, g, s)
        for i, (a, b) in enumerate(zip(ref, out)):
            if i == 2:
                assert ori_weighted_error(a, b, mag) <= 1e-4
            else:
                assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]


@pytest.mark.parametrize("name", ["vigor_prior180_circ", "kitti", "oxford"])
def test_image_resident_front_kernel_agrees_with_separate_launches(name, monkeypatch):
    """mbconv_image_kernel (blocks 2-15: expand + depthwise + pooling with the expanded image / strip in LDS) against the same
    blocks as separate expand GEMM and depthwise launches (CCVPE_MBCONV_IMAGE=0), batch 3: circular VIGOR panoramas, KITTI's
    16 x 64 / 8 x 32 maps, Oxford's odd 10 x 15 / 5 x 8 maps (ragged m-tiles and patches)."""
    cfg = gu.CONFIGS[name]
    g, s = inputs(cfg, batch=3)
    monkeypatch.setenv("CCVPE_MBCONV_IMAGE", "0")
    ref = [t.clone() for t in build_model(cfg)(g, s)]
    monkeypatch.setenv("CCVPE_MBCONV_IMAGE", "1")
    out = build_model(cfg)(g, s)
    mag = raw_ori_magnitude(cfg, g, s)
    for i, (a, b) in enumerate(zip(ref, out)):
        if i == 2:   # ori: weighted by the un-normalised magnitude
            assert ori_weighted_error(a, b, mag) <= 1e-4, "ori"
            continue
        assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]


@pytest.mark.parametrize("name", ["vigor_prior180_circ", "kitti", "oxford"])
def test_fused_stem_and_block0_depthwise_agree_with_separate_launches(name, monkeypatch):
    """stem_dw_kernel (conv_stem + bn0 + swish and block 0's depthwise conv + bn1 + swish + SE pooling in one launch, the stem
    output kept in LDS) against the two separate launches (CCVPE_STEM_DW=0): circular VIGOR panoramas (wrapped halo columns),
    KITTI / Oxford images whose half-resolution maps are not multiples of the 32 x 8 tile.  Per output both convs accumulate in
    the same order; only the squeeze-excite pooling order differs (last-bit gates; the cosine scores of Oxford's ms6 move by 4e-5)."""
    cfg = gu.CONFIGS[name]
    g, s = inputs(cfg, batch=3)
    monkeypatch.setenv("CCVPE_STEM_DW", "0")
    ref = [t.clone() for t in build_model(cfg)(g, s)]
    monkeypatch.delenv("CCVPE_STEM_DW")
    out = build_model(cfg)(g, s)
    mag = raw_ori_magnitude(cfg, g, s)
    for i, (a, b) in enumerate(zip(ref, out)):
        if i == 2:   # ori: weighted by the un-normalised magnitude
            assert ori_weighted_error(a, b, mag) <= 1e-4, "ori"
            continue
        assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]


@pytest.mark.parametrize("name,batch", [("vigor_prior180_circ", 1), ("oxford", 1), ("kitti", 2), ("vigor_prior72_fov108", 1)])
def test_latency_plan_forms_agree_with_throughput_forms(name, batch, monkeypatch):
    """Round 4, latency plans (batch <= 4): the fused MBConv fronts cut their work finer so that a block's 15-72 chunks spread over
    the chip (more strips of the image-resident form - halo rows expanded twice -, channel ranges per tile group of the wave form) and
    the matching levels run sixteen waves per workgroup / four waves per 64 pixels.  Against the same plan with the batch-32 forms
    (CCVPE_FRONT_SPREAD=0, CCVPE_MATCH_WIDE=0): the same numbers up to the order of the pooling / channel sums, and the same bits on
    every repeat."""
    cfg = gu.CONFIGS[name]
    g, s = inputs(cfg, batch=batch)
    monkeypatch.setenv("CCVPE_FRONT_SPREAD", "0")
    monkeypatch.setenv("CCVPE_MATCH_WIDE", "0")
    ref = [t.clone() for t in build_model(cfg)(g, s)]
    monkeypatch.delenv("CCVPE_FRONT_SPREAD")
    monkeypatch.delenv("CCVPE_MATCH_WIDE")
    m = build_model(cfg)
    out = [t.clone() for t in m(g, s)]
    mag = raw_ori_magnitude(cfg, g, s)
    for i, (a, b) in enumerate(zip(ref, out)):
        if i == 2:   # ori: weighted by the un-normalised magnitude
            assert ori_weighted_error(a, b, mag) <= 1e-4, "ori"
            continue
        assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]
    for _ in range(3):
        again = m(g, s)
        torch.cuda.synchronize()
        for a, b in zip(out, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name,batch,prologue", [("vigor_prior180_circ", 3, 0), ("kitti", 2, 0), ("oxford", 5, 0), ("vigor_prior72_fov108", 32, 0),
                                                 ("vigor_prior180_circ", 2, 1), ("oxford", 1, 1)])
def test_squeeze_excite_ticket_agrees_with_separate_launches(name, batch, prologue, monkeypatch):
    """Round 4 (ticket.h): the squeeze-excite of a block (model.py:113-118) is computed by whichever workgroup of the fused front kernel
    finishes a sample last - pooling partials handed over write-through, one device-scope ticket per workgroup and sample - against
    the same blocks with se_squeeze / se_excite as their own launches (CCVPE_SE_TICKET=0).  Batch 32 makes workgroups straddle samples
    (several tickets per workgroup) and samples finish in any order; three repeats must return the same bits (the combining step reads
    every partial in a fixed order, whoever arrives last)."""
    cfg = gu.CONFIGS[name]
    g, s = inputs(cfg, batch=batch)
    monkeypatch.setenv("CCVPE_SE_TICKET", "0")
    ref = [t.clone() for t in build_model(cfg)(g, s)]
    monkeypatch.delenv("CCVPE_SE_TICKET")
    if prologue:   # the opt-in form: no ticket, the gates computed in the prologue of the latency-form project GEMM (kernels_proj.hip)
        monkeypatch.setenv("CCVPE_SE_PROLOGUE", "1")
    m = build_model(cfg)
    out = [t.clone() for t in m(g, s)]
    monkeypatch.delenv("CCVPE_SE_PROLOGUE", raising=False)
    mag = raw_ori_magnitude(cfg, g, s)
    for i, (a, b) in enumerate(zip(ref, out)):
        if i == 2:   # ori: weighted by the un-normalised magnitude
            assert ori_weighted_error(a, b, mag) <= 1e-4, "ori"
            continue
        assert (a - b).abs().max().item() <= 1e-4 * max(a.abs().max().item(), 1e-30), gu.OUTPUT_NAMES[i]
    for _ in range(3):
        again = m(g, s)
        torch.cuda.synchronize()
        for a, b in zip(out, again):
            assert torch.equal(a, b)
