"""The stage checker (tests/stage_ref.py) checked on the CPU: it passes the fp32 oracle, and it catches and localises faults of the
size today's end-to-end bounds tolerate.

The "device" here is the fp32 CPU oracle run stage by stage (`oracle_device`): the same oracle functions orc.forward strings
together, every tensor the plan taps kept under the plan's tap name and layout (pad channels of loc_in* / ori_in6 included).  Its nine
outputs are asserted equal to orc.forward's, so it is the oracle and not a third implementation.  A fault is applied where the tensor
is produced and everything downstream is computed from the damaged tensor, as a wrong kernel on the device would have it: the stage
that produces the tensor must fail, and every later stage - fed the damaged tensor as its input - must still pass.

Bound: the non-Winograd class of stage_ref.bound for every stage, min(2e-5, 8 * e_ref).  The oracle passes by construction
(e_dev == e_ref); each fault is 1e-4 of its tensor's max |value| > 2e-5.
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
