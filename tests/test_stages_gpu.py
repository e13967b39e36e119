"""Every stage of the HIP forward against an fp64 oracle fed the device's own input (tests/stage_ref.py).

One debug forward per case; `check_stages` then walks the forward: each stage reads its input from the device taps, computes that one
stage on the CPU in fp64 and in fp32, and compares the device's output tap full-tensor.  Errors do not compound, so the bound is an
order of magnitude tighter than the end-to-end ones, and a failure names the stage, its launches' tiles and the worst element.

Bounds (stage_ref.bound; e_ref = |fp32 oracle - fp64 oracle| on the same input, measured by the test):
  - a stage none of whose launches ran an F(4x4) Winograd tile (decided from the plan's own rows, launch_tiles): min(2e-5, 8 * e_ref);
  - a stage that ran an F(4x4) tile: 1e-4;
  - bf16x3 handles: 1e-4 per stage.
Measured per-stage figures: DESIGN.md 2.1.
"""
import pytest
import torch

from ccvpe_amd import weights
from tests import golden_util as gu
from tests import stage_ref as sr
from tests.test_parity_gpu import assert_hook_moved, build_model, inputs

pytestmark = pytest.mark.gpu

B32_SAMPLES = [0, 13, 31]

# Per-stage factor on e_ref where the default 8 does not hold; each with its cause.
FACTORS = {}


def tiles_and_names(m, g, s):
    """(launch name -> tile of every tiled launch, the name of every launch) of the model's plan for (g, s): one profile run, the rows
    parsed as launch_tiles parses them ("name|tile")."""
    rows = [row[0].split("|", 1) for row in m.profile(g, s)]
    return {r[0]: r[1] for r in rows if len(r) == 2}, [r[0] for r in rows]


def stage_check(cfg, batch, precision="fp32", samples=None):
    """One debug forward of cfg at `batch`, every stage checked.  Returns (model, g, s, launch name -> tile, every row name)."""
    m = build_model(cfg, precision=precision)
    m.set_debug(True)
    g, s = inputs(cfg, batch=batch)
    outs = m(g, s)
    torch.cuda.synchronize()
    sd = weights.generate_state_dict(cfg["variant"], cfg["seed"])
    results = sr.check_stages(m.read_tap, outs, cfg["variant"], sd, g.cpu(), s.cpu(), cfg["circular"], cfg["ori_noise"], samples)
    tiles, names = tiles_and_names(m, g, s)
    print(f"\n{cfg['variant']} circular={cfg['circular']} ori_noise={cfg['ori_noise']} batch={batch} precision={precision} samples={samples}")
    print(sr.format_table(results))
    assert_global_bounds(results, tiles, precision)
    return m, g, s, tiles, names


def stage_tiles(r, tiles):
    """(launch name -> tile of the launches of a stage, whether one of them ran an F(4x4) Winograd tile)."""
    mine = {op: t for op, t in tiles.items() if op in sr.launches_of(r, list(tiles))}
    return mine, any("wino4" in t for t in mine.values())


def assert_global_bounds(results, tiles, precision="fp32"):
    """Every row of a full stage table under its bound; `tiles`: launch name -> tile of the plan that computed it."""
    # every row of the stage table: 2 x (16 blocks + head), 6 + 1 descriptors, 6 matching levels (ms + max + loc_in, + ori_in6 at level 1),
    # 6 localisation levels, softmax (twice), 6 orientation levels, normalise
    assert len({r.name for r in results}) == len(results) == 2 * 17 + 7 + (6 * 3 + 1) + 6 + 2 + 6 + 1
    bad = []
    for r in results:
        mine, f4 = stage_tiles(r, tiles)
        b = sr.bound(r, f4=f4, bf16x3=precision == "bf16x3", factor=FACTORS.get(r.name, sr.REF_FACTOR))
        if not r.e_dev <= b:
            bad.append(f"{r.name} {r.shape}: e_dev {r.e_dev:.3g} > {b:.3g} (e_ref {r.e_ref:.3g}) worst at {r.worst_index}, launches {mine}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,batch", [("oxford", 1), ("oxford", 3), ("kitti", 2), ("vigor_circ", 1), ("vigor_prior72_fov108", 1),
                                        ("vigor_prior180_circ", 1), ("vigor_prior180_circ", 4), ("vigor_prior180_b2", 2)])
def test_every_stage_matches_the_fp64_oracle(name, batch):
    """All six configurations; Oxford at batch 3: ragged row tiles that span samples."""
    stage_check(gu.CONFIGS[name], batch)


@pytest.mark.parametrize("name", ["vigor_prior180_circ", "kitti"])
def test_every_stage_of_the_batch32_plans_matches_the_fp64_oracle(name):
    """The plans the benchmark times: F(4x4) persistent tiles, tail split, squeeze-excite tickets with workgroups straddling samples.
    Taps are read for the whole batch; samples 0, 13 and 31 are checked."""
    _, _, _, tiles, _ = stage_check(gu.CONFIGS[name], 32, samples=B32_SAMPLES)
    assert any("wino4" in t for t in tiles.values()), tiles


_default_plan = {}


def default_plan(cfg_name, batch, g, s):
    """(launch tiles, launch names) of the default plan (no switch in the environment) of a configuration."""
    if (cfg_name, batch) not in _default_plan:
        _default_plan[cfg_name, batch] = tiles_and_names(build_model(gu.CONFIGS[cfg_name]), g, s)
    return _default_plan[cfg_name, batch]


# switch id -> (environment, precision)
SWITCHES = {
    "mbconv_image0": ({"CCVPE_MBCONV_IMAGE": "0"}, "fp32"),
    "stem_dw0": ({"CCVPE_STEM_DW": "0"}, "fp32"),
    "se_ticket0": ({"CCVPE_SE_TICKET": "0"}, "fp32"),
    "se_prologue1": ({"CCVPE_SE_PROLOGUE": "1"}, "fp32"),
    "front_spread0_match_wide0": ({"CCVPE_FRONT_SPREAD": "0", "CCVPE_MATCH_WIDE": "0"}, "fp32"),
    "winograd0": ({"CCVPE_WINOGRAD": "0"}, "fp32"),
    "prefer_pw": ({"CCVPE_TUNE_PREFER_PW": "1"}, "fp32"),
    "prefer_proj": ({"CCVPE_TUNE_PREFER_PROJ": "1"}, "fp32"),
    "prefer_proj_lat": ({"CCVPE_TUNE_PREFER_PROJ": "lat"}, "fp32"),
    "bf16x3": ({}, "bf16x3"),
}


@pytest.mark.parametrize("name,batch", [("oxford", 3), ("vigor_prior180_circ", 1)])
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_every_stage_under_each_plan_switch(switch, name, batch, monkeypatch):
    """Each plan-variant switch the suite exercises end to end, stage by stage; where launch names or tiles show that the switch took
    effect, that is asserted (a variant that silently did not apply is not covered)."""
    env, precision = SWITCHES[switch]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    m, g, s, tiles, names = stage_check(gu.CONFIGS[name], batch, precision=precision)
    for k in env:
        monkeypatch.delenv(k)
    if switch == "mbconv_image0":   # blocks the image-resident front serves by default run their expand GEMM and depthwise conv as launches of their own
        new = set(names) - set(default_plan(name, batch, g, s)[1])
        assert [n for n in new if n.endswith(".expand")] and [n for n in new if n.endswith(".dw")], names
    elif switch == "stem_dw0":
        assert "grd.stem" in names and "sat.stem" in names and "sat.stem_b0dw" not in names, names
    elif switch == "se_ticket0":
        assert [n for n in names if n.endswith(".se")], names
    elif switch == "se_prologue1":
        assert [n for n in names if n.endswith(".se_project")], names
    elif switch == "winograd0":
        assert not [t for t in tiles.values() if "wino" in t], tiles
    elif switch == "prefer_pw":
        assert_hook_moved(tiles, default_plan(name, batch, g, s)[0], "conv_pw_")
    elif switch == "prefer_proj":
        assert_hook_moved(tiles, default_plan(name, batch, g, s)[0], "conv_proj")
    elif switch == "prefer_proj_lat":
        assert any(t.startswith("conv_projl_") for t in tiles.values()), tiles
        assert not [op for op, t in tiles.items() if op.endswith(".project") and t.startswith("conv_proj_r")], tiles
    elif switch == "bf16x3":
        assert any(t.startswith("conv_bf16x3_") for t in tiles.values()), tiles
    # front_spread0_match_wide0: both switches choose a form inside a launch (work items of a front kernel, waves per workgroup of the
    # matching kernel); neither the launch names nor the tiles of the plan show them, as in the existing end-to-end test of the pair
