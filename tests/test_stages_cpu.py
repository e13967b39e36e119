"""The stage checker (tests/stage_ref.py) checked on the CPU: it passes the fp32 oracle, and it catches and localises faults of the
size today's end-to-end bounds tolerate.

The "device" here is the fp32 CPU oracle run stage by stage (`oracle_device`): the same oracle functions orc.forward strings
together, every tensor the plan taps kept under the plan's tap name and layout (pad channels of loc_in* / ori_in6 included).  Its nine
outputs are asserted equal to orc.forward's, so it is the oracle and not a third implementation.  A fault is applied where the tensor
is produced and everything downstream is computed from the damaged tensor, as a wrong kernel on the device would have it: the stage
that produces the tensor must fail, and every later stage - fed the damaged tensor as its input - must still pass.

Bound: the non-Winograd class of stage_ref.bound for every stage, min(2e-5, 8 * e_ref).  The oracle passes by construction
(e_dev == e_ref); each fault is 1e-4 of its tensor's max |value| > 2e-5.

The last section does the same for the trained-like family of tests/stress_weights.py and the per-channel rows: the conditions the cases of
tests/test_stress_stages_gpu.py meet on the reference alone, faults in a tensor's smallest channel that the global row misses, and the
two wider channel bounds re-derived in plain arithmetic.
"""
import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import spec, weights
from oracle import ccvpe_oracle as orc
from tests import stage_ref as sr

CASES = {
    "oxford": dict(variant="oxford", circular=False, ori_noise=None, fov=360.0),
    "vigor_ori_prior": dict(variant="vigor_ori_prior", circular=True, ori_noise=180.0, fov=360.0),
}
FAULT = 1e-4


def oracle_device(variant, sd, grd, sat, circular, ori_noise, fault=None):
    """(taps, outputs) of the fp32 oracle run stage by stage.  `fault`: (tensor name, fn) - fn damages that tensor in place where it is
    produced; tensor names are the plan's tap names and the output names logits, heatmap, ori, ms1..ms6."""
    v = spec.VARIANTS[variant]
    taps = {}

    def keep(name, t):
        t = t.clone()
        if fault is not None and fault[0] == name:
            fault[1](t)
        taps[name] = t
        return t

    with torch.no_grad():
        for tag, img, circ in (("grd", grd, circular), ("sat", sat, False)):
            p = tag + "_efficientnet"
            x = keep(f"{tag}_block0", sr.stem_block0(img, sd, p, circ))
            for i in range(1, 16):
                x = keep(f"{tag}_block{i}", orc.mbconv(x, sd, f"{p}._blocks.{i}", spec.B0_BLOCKS[i], circ))
            keep(f"{tag}_volume", sr.head_conv(x, sd, p))
        descs = [keep(f"grd_desc{k}", orc.ground_descriptor(taps["grd_volume"], sd, k)[:, :, None, None]).flatten(1) for k in range(1, 7)]
        x = keep("sat_descriptor_map", orc.aerial_descriptor_map(taps["sat_volume"], sd))
        dmap = x
        ms = []
        for k in range(1, 7):
            n = 7 - k
            g = descs[k - 1]
            score = orc.rolling_match(x, g, spec.roll_shifts(v, k, g.shape[1], ori_noise))
            smax = score.max(dim=1, keepdim=True).values
            if k == 1 and variant == "vigor_ori_prior":
                score = orc.rolling_match(x, g, spec.full_roll_shifts(v, 1, g.shape[1]))
            ms.append(keep(f"ms{k}", score))
            pad = torch.zeros_like(smax).expand(-1, sr.LOC_IN_PAD - 1, -1, -1)
            lin = keep(f"loc_in{n}", torch.cat([smax, pad, F.normalize(x, p=2, dim=1)], dim=1))
            if k == 1:
                rpad = -(-v.n_rolls // 8) * 8
                pad = torch.zeros_like(smax).expand(-1, rpad - v.n_rolls, -1, -1)
                keep("ori_in6", torch.cat([ms[0], pad, F.normalize(x, p=2, dim=1)], dim=1))
            lin = torch.cat([lin[:, :1], lin[:, sr.LOC_IN_PAD:]], dim=1)
            skip = taps[f"sat_block{spec.TAP_BLOCKS[k - 1]}"] if k <= 5 else None
            x = orc._decoder_level(lin, skip, sd, n, "")
            x = keep(f"loc_level{n}", x) if n >= 2 else keep("logits", x.flatten(1))
        logits = x
        heat = keep("heatmap", torch.softmax(logits, dim=-1).reshape(-1, 1, *spec.OUT_HW))
        t = taps["ori_in6"]
        xo = torch.cat([t[:, :v.n_rolls], t[:, t.shape[1] - dmap.shape[1]:]], dim=1)
        for k in range(1, 7):
            n = 7 - k
            skip = taps[f"sat_block{spec.TAP_BLOCKS[k - 1]}"] if k <= 5 else None
            xo = keep(f"ori_level{n}" if n >= 2 else "ori_level1_nchw", orc._decoder_level(xo, skip, sd, n, "_ori"))
        ori = keep("ori", F.normalize(xo, p=2, dim=1))
    return taps, (logits, heat, ori, *ms)


_made = {}


def case(name):
    if name not in _made:
        c = CASES[name]
        sd = weights.generate_state_dict(c["variant"], 0)
        g, s = weights.generate_inputs(c["variant"], 1, 0, c["fov"])
        _made[name] = (c, sd, torch.from_numpy(g), torch.from_numpy(s))
    return _made[name]


def run_checker(name, fault=None):
    c, sd, g, s = case(name)
    taps, outs = oracle_device(c["variant"], sd, g, s, c["circular"], c["ori_noise"], fault)
    return sr.check_stages(taps.__getitem__, outs, c["variant"], sd, g, s, c["circular"], c["ori_noise"]), outs


def failing(results):
    return sorted(r.name for r in results if not r.e_dev <= sr.bound(r))


def scaled(t):
    return FAULT * t.abs().max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_oracle_passes_every_stage(name):
    c, sd, g, s = case(name)
    results, outs = run_checker(name)
    # the staged device is the oracle: the same nine outputs as orc.forward
    for a, b in zip(orc.forward(c["variant"], sd, g, s, c["circular"], c["ori_noise"]), outs):
        assert torch.equal(a, b.reshape(a.shape))
    print(sr.format_table(results))
    names = [r.name for r in results]
    assert len(names) == len(set(names))
    # the whole table of the forward: 2 x (16 blocks + head), 6 + 1 descriptors, 6 matching levels (ms + max + loc_in, + ori_in6 at level 1),
    # 6 localisation levels, softmax (twice), 6 orientation levels, normalise
    assert len(names) == 2 * 17 + 7 + (6 * 3 + 1) + 6 + 2 + 6 + 1
    for r in results:
        assert 0 < r.e_ref < 5e-6, r           # fp32 against fp64 on one stage: a few ulp of scale, never zero (a zero yardstick forbids everything)
        assert r.e_dev == r.e_ref, r
    assert failing(results) == []


def wrap_column(t): t[:, :, :, 0] += scaled(t)
def last_row(t): t[:, :, -1, :] += scaled(t)
def one_roll(t): t[:, 2] += scaled(t)
def one_channel(t): t[:, 5] += scaled(t)
def one_pixel(t): t[:, 200 * 512 + 300] += scaled(t)


# (config, damaged tensor, fault, the one stage that must fail)
FAULTS = [
    ("vigor_ori_prior", "grd_block7", wrap_column, "grd_block7"),      # a wrap column under circular padding
    ("oxford", "sat_block3", last_row, "sat_block3"),
    ("oxford", "ms3", one_roll, "match3:ms"),
    ("vigor_ori_prior", "loc_level4", one_channel, "loc_level4"),
    ("oxford", "logits", one_pixel, "logits"),
]


@pytest.mark.parametrize("name,tensor,fn,stage", FAULTS, ids=[f[1] for f in FAULTS])
def test_injected_fault_fails_exactly_the_producing_stage(name, tensor, fn, stage):
    results, _ = run_checker(name, (tensor, fn))
    by_name = {r.name: r for r in results}
    r = by_name[stage]
    assert r.e_dev > sr.BOUND_FP32 and r.e_dev == pytest.approx(FAULT, rel=0.05), r
    # localisation: the stage that produced the damaged tensor, and no other - every consumer of the damaged tensor takes it as its
    # input (teacher forcing) and still passes
    assert failing(results) == [stage], sr.format_table(results)
    consumers = {"grd_block7": ["grd_block8"], "sat_block3": ["sat_block4"], "ms3": [], "loc_level4": ["match4:ms", "match4:max", "match4:loc_in3"],
                 "logits": ["heatmap", "heatmap:over_max"]}[tensor]
    for cn in consumers:
        assert by_name[cn].e_dev <= sr.bound(by_name[cn]), by_name[cn]
    # the worst element is inside the damaged region
    w = r.worst_index
    assert {"grd_block7": w[3] == 0, "sat_block3": w[2] == r.shape[2] - 1, "ms3": w[1] == 2, "loc_level4": w[1] == 5,
            "logits": w[2:] == (200, 300)}[tensor], r


# ---- the stage filter: stages=("grd_", "match") computes the ground side and the matching levels only ----
GROUND_STAGES = ("grd_", "match")
N_GROUND_ROWS = 16 + 1 + 6 + (6 * 3 + 1)     # ground blocks, head, descriptors, six matching levels (ms + max + loc_in, + ori_in6 at level 1)


def run_filtered(name, fault=None):
    """The filtered checker on the staged oracle of a case, and the names of the taps it read."""
    c, sd, g, s = case(name)
    taps, outs = oracle_device(c["variant"], sd, g, s, c["circular"], c["ori_noise"], fault)
    read = []

    def read_tap(n):
        read.append(n)
        return taps[n]

    return sr.check_stages(read_tap, outs, c["variant"], sd, g, s, c["circular"], c["ori_noise"], stages=GROUND_STAGES), read


@pytest.mark.parametrize("name", list(CASES))
def test_filtered_run_returns_the_rows_of_the_full_run(name):
    full, _ = run_checker(name)
    part, read = run_filtered(name)
    assert len(part) == N_GROUND_ROWS
    assert part == [r for r in full if r.name.startswith(GROUND_STAGES)]   # the same rows in the same order: names, e_dev, e_ref, worst element
    # no aerial encoder, no decoder: the only aerial-side taps read are the matching levels' x inputs
    assert not [n for n in read if n.startswith(("sat_block", "sat_volume", "ori_level"))], read
    assert {n for n in read if n.startswith(("sat_", "loc_level"))} == {"sat_descriptor_map"} | {f"loc_level{n}" for n in range(2, 7)}


@pytest.mark.parametrize("name,tensor,fn,stage", [f for f in FAULTS if f[1] in ("grd_block7", "ms3")], ids=["grd_block7", "ms3"])
def test_injected_fault_fails_exactly_its_stage_under_the_filter(name, tensor, fn, stage):
    results, _ = run_filtered(name, (tensor, fn))
    assert len(results) == N_GROUND_ROWS
    r = {r.name: r for r in results}[stage]
    assert r.e_dev > sr.BOUND_FP32 and r.e_dev == pytest.approx(FAULT, rel=0.05), r
    assert failing(results) == [stage], sr.format_table(results)


# ---- the geometry table of tests/test_ground_geometry_gpu.py: a condition on its inputs ----
def geometry_rows():
    from tests import test_ground_geometry_gpu as geo
    return geo


def _geometry_params():
    geo = geometry_rows()
    return [pytest.param(row, id=geo.case_id(row)) for row in geo.GEOMETRY]


@pytest.mark.parametrize("row", _geometry_params())
def test_geometry_table_inputs_keep_the_reference_error_small(row):
    """The bound of the GPU test is min(2e-5, 8 * e_ref): with descriptors of 2 or 3 floats a window's norm can be near zero (the
    reference divides without an epsilon) and e_ref - then the bound - would blow up or degenerate.  The fp32 oracle through the
    filtered checker, on the samples the GPU test checks: e_dev == e_ref (it is the oracle) and e_ref <= 2.5e-6 on every row, so
    8 * e_ref stays under the 2e-5 cap.  The GPU test compares the nine outputs with the fp32 oracle end to end: that oracle against
    the fp64 oracle end to end stays under E2E_REF_MAX on every output (the orientation field weighted by the un-normalised magnitude)
    - but for an output the row's E2E_EXEMPT entry names, which must MISS it: an exemption holds only where the reference alone fails
    the condition.  Conditions on the row's inputs (its seed), not measurements of the library."""
    geo = geometry_rows()
    variant, circular, ori_noise, gh, gw, batch, samples, _ = row
    sd = geo.state_dict(variant)
    g, s = geo.geometry_inputs(row)
    assert tuple(g.shape) == (batch, 3, gh, gw)
    if samples is not None:     # per-sample arithmetic: the checked samples alone
        g, s = g[list(samples)], s[list(samples)]
    taps, outs = oracle_device(variant, sd, g, s, circular, ori_noise)
    results = sr.check_stages(taps.__getitem__, outs, variant, sd, g, s, circular, ori_noise, stages=geo.STAGES)
    print(sr.format_table(results))
    assert len(results) == geo.N_ROWS == N_GROUND_ROWS
    for r in results:
        assert r.e_dev == r.e_ref, r
        assert 0 < r.e_ref <= 2.5e-6, r
    exempt = geo.E2E_EXEMPT.get(geo.case_id(row), {})
    t64 = {}
    with torch.no_grad():
        ref64 = orc.forward(variant, sr._f64(sd), g.double(), s.double(), circular, ori_noise, taps=t64)
    mag = t64["ori_level1"].norm(dim=1, keepdim=True)
    for n, a, b in zip(["logits", "heatmap", "ori", "ms1", "ms2", "ms3", "ms4", "ms5", "ms6"], outs, ref64):
        d = (a.reshape(b.shape).double() - b).abs()
        e = (d * mag).max().item() / mag.max().item() if n == "ori" else d.max().item() / b.abs().max().item()
        print(f"end to end, fp32 oracle against fp64 oracle: {n} {e:.2e}" + (" (exempt)" if n in exempt else ""))
        assert (e > geo.E2E_REF_MAX) if n in exempt else (e <= geo.E2E_REF_MAX), (n, e)


def test_minimum_circular_width_is_where_the_reference_padding_stops():
    """MIN_CIRCULAR_W of the geometry table: the oracle's circular encoder runs at that width and leaves a feature volume 2 wide; one
    pixel narrower torch refuses the padding (it would wrap more than once)."""
    geo = geometry_rows()
    sd = geo.state_dict("vigor")
    w = geo.MIN_CIRCULAR_W
    with torch.no_grad():
        vol, _ = orc.encoder(torch.zeros(1, 3, 320, w), sd, "grd_efficientnet", True)
        assert vol.shape[-1] == 2
        with pytest.raises(RuntimeError, match="wrapping around more than once"):
            orc.encoder(torch.zeros(1, 3, 320, w - 1), sd, "grd_efficientnet", True)


# ---- the stress family of tests/stress_weights.py: conditions on the reference alone, and the per-channel checker ----
def stress():
    from tests import test_stress_stages_gpu as st
    return st


def stress_inputs(name):
    """(cfg, sd, grd, sat) of a case of tests/test_stress_stages_gpu.py, its checked samples alone (per-sample arithmetic: samples 0 and
    31 of the batch-32 case at batch 2)."""
    st = stress()
    cfg, sd, g, s = st.stress_case(name)
    samples = st.CASES[name]["samples"]
    if samples is not None:
        g, s = g[list(samples)], s[list(samples)]
    return cfg, sd, g, s


def stress_checker(cfg, sd, g, s, fault=None):
    taps, outs = oracle_device(cfg["variant"], sd, g, s, cfg["circular"], cfg["ori_noise"], fault)
    pc = sr.PerChannel()
    results = sr.check_stages(taps.__getitem__, outs, cfg["variant"], sd, g, s, cfg["circular"], cfg["ori_noise"], per_channel=pc)
    return taps, outs, results, pc


_stress_ref = {}


def stress_reference(name):
    """The fp32 staged oracle of a case through the checker, and the fp64 oracle end to end; computed once per case, the figures kept:
    (rows, PerChannel, all taps finite, staged outputs == orc.forward's, logits span of the fp64 oracle per sample, its smallest heatmap value)."""
    if name not in _stress_ref:
        cfg, sd, g, s = stress_inputs(name)
        taps, outs, results, pc = stress_checker(cfg, sd, g, s)
        finite = all(torch.isfinite(t).all().item() for t in list(taps.values()) + list(outs))
        with torch.no_grad():
            fwd = orc.forward(cfg["variant"], sd, g, s, cfg["circular"], cfg["ori_noise"])
            ref64 = orc.forward(cfg["variant"], sr._f64(sd), g.double(), s.double(), cfg["circular"], cfg["ori_noise"])
        same = all(torch.equal(a, b.reshape(a.shape)) for a, b in zip(fwd, outs))
        finite = finite and all(torch.isfinite(t).all().item() for t in ref64)
        span = (ref64[0].max(dim=1).values - ref64[0].min(dim=1).values).tolist()
        _stress_ref[name] = (results, pc, finite, same, span, ref64[1].min().item())
    return _stress_ref[name]


def channel_failing(pc):
    return {c.name: v for c, v in ((c, sr.channel_verdict(c)) for c in pc.channels) if not v.ok}


def _stress_names():
    return list(stress().CASES)


def test_stress_family_has_the_channels_it_promises():
    """Every encoder BatchNorm scale holds an exact zero and a negative entry next to positive ones, over several decades, at rms 1 of the
    generator's; every first decoder conv has one output channel that is zero in weights and bias; the inputs hold constant regions."""
    from tests import stress_weights as sw
    base = weights.generate_state_dict("oxford", 0)
    sd = sw.stress_state_dict("oxford", 0)
    assert set(sd) == set(base) and sw.stress_state_dict("oxford", 0)["conv3.0.weight"].equal(sd["conv3.0.weight"])
    n_bn = 0
    for k, t in sd.items():
        if "._bn" in k and k.endswith(".weight"):
            n_bn += 1
            f = (t / base[k]).double()
            assert (t == 0).any() and (t < 0).any() and (t > 0).any(), k
            assert f.pow(2).mean().sqrt().item() == pytest.approx(1.0, rel=1e-5), k
            live = f.abs()[f != 0]
            assert live.max() / live.min() > 30, k
    assert n_bn == 2 * (1 + 16 * 3 - 1 + 1)
    for sfx in ("", "_ori"):
        for n in range(1, 7):
            w, b = sd[f"conv{n}{sfx}.0.weight"], sd[f"conv{n}{sfx}.0.bias"]
            dead = (w.flatten(1).abs().amax(dim=1) == 0) & (b == 0)
            assert int(dead.sum()) == 1, (n, sfx)
            assert not (sd[f"conv{n}{sfx}.2.weight"] == 0).any()
    assert torch.equal(sd["conv1.2.weight"], base["conv1.2.weight"] * sw.LOGIT_SCALE)
    g, s = sw.structured_inputs("oxford", 3, 0)
    for img in (g, s):
        assert img.dtype.name == "float32"
        third = img.shape[2] // 3
        assert (img[:, :, :third] == img[:, :, :1, :1]).all()                       # the constant upper third
        assert (img[sw.CONSTANT_SAMPLE] == img[sw.CONSTANT_SAMPLE][:, :1, :1]).all()  # the single-colour sample
        lo, hi = (0.0 - sw.MEAN) / sw.STD, (1.0 - sw.MEAN) / sw.STD
        assert ((img[0] == lo).all(axis=0).sum() >= 16 * 16) and ((img[0] == hi).all(axis=0).sum() >= 16 * 16)   # the all-0 and all-255 rectangles
        assert len({float(x) for x in img[0, 0, third:].ravel()}) > 200           # and noise
    g32, _ = sw.structured_inputs("oxford", 32, 0)
    assert (g32[[0, 2]] == g[[0, 2]]).all()                                           # a sample depends on (seed, index) alone


@pytest.mark.parametrize("name", _stress_names())
def test_stress_case_keeps_the_reference_well_conditioned(name):
    """Conditions on a GPU case's exact weights and inputs, met by the reference alone (its seed is the first of 0, 1, 2, ... that does):
    every tap and output finite; global e_ref <= 2.5e-6 on every stage (8 * e_ref stays under the 2e-5 cap); no channel ill-conditioned
    (8 * e_ref_c <= 1e-4 everywhere, so the GPU test leaves no channel out); the fp64 oracle's logits span >= 60 units; and the staged
    oracle is orc.forward bit for bit on this family too."""
    results, pc, finite, same, span, _ = stress_reference(name)
    print(sr.format_table(results))
    print(sr.format_channel_table(pc.channels, [sr.channel_verdict(c) for c in pc.channels]))
    print(f"logits span of the fp64 oracle per sample: {span}; heatmap:log of the fp32 oracle {pc.heatmap_log.e_ref:.3g}")
    assert finite and same
    assert len(results) == 2 * 17 + 7 + (6 * 3 + 1) + 6 + 2 + 6 + 1
    for r in results:
        assert r.e_dev == r.e_ref and 0 < r.e_ref <= 2.5e-6, r
    assert failing(results) == []
    # 2 x (16 blocks + head), the descriptor map, ms1..ms6 less the levels with a single roll, 6 loc_in + ori_in6, 5 + 6 decoder levels
    single = sum(1 for c in pc.channels if c.name.endswith(":ms"))
    assert len(pc.channels) == 2 * 17 + 1 + single + 7 + 11 and single >= 1
    for c in pc.channels:
        v = sr.channel_verdict(c)
        assert v.ok and v.excluded == () and v.over == (), v
        assert torch.equal(c.e_dev, c.e_ref)
        assert (sr.REF_FACTOR * c.e_ref <= sr.BOUND_F4).all(), c.name
    assert min(span) >= 60.0
    h = pc.heatmap_log
    assert h.e_dev == h.e_ref and 0 < h.e_ref < 1e-4, h


def test_stress_heatmaps_reach_below_the_smallest_normal_fp32():
    """On at least one case the fp64 heatmap holds values under 2^-126: the underflow rule of heatmap:log is exercised."""
    lows = {n: stress_reference(n)[5] for n in _stress_names()}
    print(lows)
    assert min(lows.values()) < sr.FP32_MIN_NORMAL


STRESS_FAULT = 1e-3     # of the channel's own maximum
STRESS_FAULT_CASE = "oxford_b1"


# (damaged tap, the row of the checker that compares it, whether the global row misses the fault)
STRESS_FAULTS = [
    ("sat_volume", "sat_volume", True),
    ("grd_block15", "grd_block15", True),
    # the tensor the level-6 decoder reads: cat(max score, normalize(x)); its channels span three decades
    ("loc_in6", "match1:loc_in6", True),
    # a decoder level's own output: the family scales the channels of conv{n}.0 and deconv{n}, not of conv{n}.2, so the channels of a
    # level lie within a factor 3 of each other and 1e-3 of the smallest is 4e-4 of the tensor - the global row sees this one too
    ("loc_level4", "loc_level4", False),
]


@pytest.mark.parametrize("tensor,row,gap", STRESS_FAULTS, ids=[f[0] for f in STRESS_FAULTS])
def test_fault_in_the_smallest_channel_fails_its_channel_row(tensor, row, gap):
    """1e-3 of its own maximum added to the smallest live channel of a tensor: the per-channel row of the producing stage fails and
    names the channel; every other stage, the consumers of the damaged tensor included, passes both checks.  Where the channels of the
    tensor span decades (`gap`) the stage's global row still passes: the gap the per-channel rows close."""
    cfg, sd, g, s = stress_inputs(STRESS_FAULT_CASE)
    _, pc0, *_ = stress_reference(STRESS_FAULT_CASE)
    scale = {c.name: c.scale for c in pc0.channels}[row]
    ch = int(torch.where(scale > 0, scale, torch.full_like(scale, float("inf"))).argmin())
    tap_ch = ch + sr.LOC_IN_PAD - 1 if tensor == "loc_in6" and ch > 0 else ch     # the tap holds its 7 pad channels

    def fault(t):
        t[:, tap_ch] += STRESS_FAULT * t[:, tap_ch].abs().max()

    _, _, results, pc = stress_checker(cfg, sd, g, s, (tensor, fault))
    r = {r.name: r for r in results}[row]
    print(f"{row}: channel {ch} of maximum {scale[ch].item():.3g} in a tensor of maximum {scale.max().item():.3g}; global e_dev {r.e_dev:.3g}, "
          f"bound {sr.bound(r):.3g}")
    assert failing(results) == ([] if gap else [row]), sr.format_table(results)
    bad = channel_failing(pc)
    assert list(bad) == [row], bad
    v = bad[row]
    assert v.over == (ch,) and v.worst == ch and v.e_dev == pytest.approx(STRESS_FAULT, rel=0.05), v
    assert pc.heatmap_log.e_dev <= sr.heatmap_log_bound(pc.heatmap_log)


def test_nonzero_value_in_an_all_zero_channel_fails():
    """A channel whose reference is all zero - block 3 of the aerial encoder (stride 2, no residual), a zero BatchNorm scale and, here,
    a zero bias - passes only while the device holds exact zeros there; the smallest value fails it, and so does a NaN."""
    cfg, sd, g, s = stress_inputs(STRESS_FAULT_CASE)
    sd = dict(sd)
    p = "sat_efficientnet._blocks.3"
    assert spec.B0_BLOCKS[3][2] == 2
    ch = int((sd[p + "._bn2.weight"] == 0).nonzero()[0])
    sd[p + "._bn2.bias"] = sd[p + "._bn2.bias"].clone()
    sd[p + "._bn2.bias"][ch] = 0.0
    with torch.no_grad():
        x0 = sr.stem_block0(s, sd, "sat_efficientnet", False)
        for i in (1, 2):
            x0 = orc.mbconv(x0, sd, f"sat_efficientnet._blocks.{i}", spec.B0_BLOCKS[i], False)
        x1 = orc.mbconv(x0, sd, p, spec.B0_BLOCKS[3], False)
    assert (x1[:, ch] == 0).all() and (x1[:, ch - 1] != 0).any()
    unused = [torch.zeros(len(s), 1)] * 9
    for value, ok in ((0.0, True), (1e-30, False), (float("nan"), False)):
        dev = x1.clone()
        dev[0, ch, 3, 5] = value
        pc = sr.PerChannel()
        rows = sr.check_stages({"sat_block2": x0, "sat_block3": dev}.__getitem__, unused, cfg["variant"], sd, g, s, cfg["circular"],
                               cfg["ori_noise"], stages=("sat_block3",), per_channel=pc)
        assert [r.name for r in rows] == [c.name for c in pc.channels] == ["sat_block3"]
        v = sr.channel_verdict(pc.channels[0])
        assert pc.channels[0].scale[ch] == 0
        assert v.ok == ok and v.over == (() if ok else (ch,)), v
        if value == 1e-30:      # invisible to the global row
            assert rows[0].e_dev <= sr.bound(rows[0])


def test_descriptor_map_factor_is_what_a_plain_fp32_chain_needs():
    """FACTORS['sat_descriptor_map'] of tests/test_stress_stages_gpu.py, from arithmetic alone: the aerial descriptor map (K = 5120) summed
    in plain numpy fp32 as the batch-32 plan's split-K-2 implicit GEMM orders it - two chains of 2560 additions, product and sum rounded
    separately - on the fp32 oracle's own sat_volume of the batch-32 case, per channel against max(e_ref_c, median): some channel needs
    more than the default 8, none more than the table's 16."""
    import numpy as np
    st = stress()
    cfg, sd, g, s = stress_inputs("vigor_prior180_circ_b32")
    with torch.no_grad():
        vol, _ = orc.encoder(s, sd, "sat_efficientnet", False)
        r32 = orc.aerial_descriptor_map(vol, sd)
        r64 = orc.aerial_descriptor_map(vol.double(), sr._f64(sd))
    w = sd["sat_feature_to_descriptors.1.weight"].numpy()           # [D, 5120], k = ch * 4 + dy * 2 + dx
    B, K = vol.shape[0], w.shape[1]
    patches = vol.reshape(B, spec.HEAD_CH, 8, 2, 8, 2).permute(0, 2, 4, 1, 3, 5).reshape(B * 64, K).numpy()
    total = np.zeros((B * 64, w.shape[0]), np.float32)
    for half in range(2):
        acc = np.zeros_like(total)
        for k in range(half * K // 2, (half + 1) * K // 2):
            acc += patches[:, k:k + 1] * w[None, :, k]
        total += acc
    total += sd["sat_feature_to_descriptors.1.bias"].numpy()[None]
    chain = torch.from_numpy(total).reshape(B, 8, 8, -1).permute(0, 3, 1, 2)
    c = sr._channel_result("sat_descriptor_map", chain, r32, r64, ())
    need = (c.e_dev / c.e_ref.clamp(min=c.e_ref.median().item())).max().item()
    print(f"plain fp32 chain of 2 x 2560: worst channel needs {need:.2f} x its yardstick; over at 8: {len(sr.channel_verdict(c).over)} channels")
    assert sr.REF_FACTOR < need <= st.FACTORS["sat_descriptor_map"]
    assert sr.channel_verdict(c, factor=st.FACTORS["sat_descriptor_map"]).ok


def test_flat_bound_is_out_of_reach_of_bf16x3_on_a_cancelling_channel():
    """The bf16x3 class of stage_ref.channel_verdict, from arithmetic alone: the aerial descriptor map of the Oxford batch-3 stress case
    with every operand split into hi = bf16(x), lo = bf16(x - hi) and the three products hi*hi + hi*lo + lo*hi summed exactly (fp64) -
    the best any bf16x3 kernel can do.  Some channels miss BOUND_F4 of their own maximum; every channel is within BF16X3_OPERAND times
    its yardstick."""
    cfg, sd, g, s = stress_inputs("oxford_b3")
    with torch.no_grad():
        vol, _ = orc.encoder(s, sd, "sat_efficientnet", False)
        r32 = orc.aerial_descriptor_map(vol, sd)
        r64 = orc.aerial_descriptor_map(vol.double(), sr._f64(sd))

    def split(x):
        hi = x.bfloat16().float()
        return hi.double(), (x - hi).bfloat16().double()

    w = sd["sat_feature_to_descriptors.1.weight"]
    B = vol.shape[0]
    patches = vol.reshape(B, spec.HEAD_CH, 8, 2, 8, 2).permute(0, 2, 4, 1, 3, 5).reshape(B * 64, -1)
    (ph, pl), (wh, wl) = split(patches), split(w)
    out = ph @ wh.T + ph @ wl.T + pl @ wh.T + sd["sat_feature_to_descriptors.1.bias"].double()[None]
    c = sr._channel_result("sat_descriptor_map", out.reshape(B, 8, 8, -1).permute(0, 3, 1, 2), r32, r64, ())
    yardstick = c.e_ref.clamp(min=c.e_ref.median().item())
    print(f"exact bf16x3: worst channel {c.e_dev.max().item():.3g} of its maximum, {int((c.e_dev > sr.BOUND_F4).sum())} channels over {sr.BOUND_F4}; "
          f"at most {(c.e_dev / yardstick).max().item():.1f} x the yardstick")
    assert (c.e_dev > sr.BOUND_F4).any()
    v = sr.channel_verdict(c, bf16x3=True)
    assert v.ok and v.excluded == (), v
