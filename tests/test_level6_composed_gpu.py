"""Decoder level 6 with the transposed conv composed into the first 3x3 conv (kernels_level6.hip), forced on with
CCVPE_COMPOSE_L6=1 at batch 1 and 3 - four and twelve tile rows per group, padded with zero rows to the GEMM's 32-row tile - against
today's three launches (CCVPE_COMPOSE_L6=0) and the oracle's taps for every variant; the same with a transposed-conv bias large enough
that a wrong border-bias case shows; the 64-row GEMM tile (batch 9) and the F(2x2,2x2) form (CCVPE_COMPOSE_L6=2); a handle loaded from
a packed-weight file; the automatic rule; repeated forwards bit-equal, and the pose-only form bit-identical to forward + post-processing.
Every run also checks, from the plan's launch list, that the path it means to test is the one that ran."""
import os
import tempfile

import pytest
import torch

from ccvpe_amd import _lib, models, weights
from oracle import ccvpe_oracle as orc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # scale-relative, as tests/test_parity_gpu.py holds the fp32 path
NAMES = ["vigor_circ", "kitti", "oxford"]
TAPS = ["loc_level6", "ori_level6"]
COMPOSED_OPS = {f"{d}6.{op}" for d in ("loc", "ori") for op in ("l6_transform", "l6_gemm", "conv_skip", "l6_combine")}
THREE_LAUNCH_OPS = {f"{d}6.{op}" for d in ("loc", "ori") for op in ("deconv", "conv_a")}


def make(name, sd, **kw):
    cfg = gu.CONFIGS[name]
    v = cfg["variant"]
    if v == "vigor":
        m = models.CVM_VIGOR("cuda", cfg["circular"], **kw)
    elif v == "vigor_ori_prior":
        m = models.CVM_VIGOR_ori_prior("cuda", cfg["ori_noise"], cfg["circular"], **kw)
    elif v == "kitti":
        m = models.CVM_KITTI("cuda", **kw)
    else:
        m = models.CVM_OxfordRobotCar("cuda", **kw)
    m.load_state_dict(sd)
    return m.to("cuda").eval()


def state_dict(name, big_bias):
    sd = weights.generate_state_dict(gu.CONFIGS[name]["variant"], gu.CONFIGS[name]["seed"])
    if big_bias:
        for key in ("deconv6.bias", "deconv6_ori.bias"):
            sd[key] = sd[key] * 50.0 + torch.sign(sd[key])
    return sd


def inputs(name, batch):
    cfg = gu.CONFIGS[name]
    g, s = weights.generate_inputs(cfg["variant"], batch, cfg["seed"], cfg["fov"])
    return torch.from_numpy(g), torch.from_numpy(s)


def plan_ops(m):
    """Launch names of the plan of the model's last forward (ccvpe_debug_dump_plan)."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "plan.txt")
        _lib.check(_lib.load().ccvpe_debug_dump_plan(m._handle, path.encode()), "ccvpe_debug_dump_plan")
        with open(path) as fh:
            return {line.split()[2] for line in fh if line.startswith("op ")}


def assert_path(ops, composed):
    want, never = (COMPOSED_OPS, THREE_LAUNCH_OPS) if composed else (THREE_LAUNCH_OPS, COMPOSED_OPS)
    assert want <= ops and not (never & ops), sorted(o for o in ops if "6." in o)


_RUNS = {}
_ORACLE = {}


def run(name, batch, big_bias, switch, monkeypatch):
    """Nine outputs, the level-6 taps and the un-normalised orientation field of one debug forward under CCVPE_COMPOSE_L6=switch, on the
    CPU; computed once."""
    key = (name, batch, big_bias, switch)
    if key not in _RUNS:
        monkeypatch.setenv("CCVPE_COMPOSE_L6", switch)   # read at ccvpe_create
        m = make(name, state_dict(name, big_bias))
        m.set_debug(True)
        g, s = inputs(name, batch)
        outs = m(g.cuda(), s.cuda())
        torch.cuda.synchronize()
        assert_path(plan_ops(m), switch != "0")
        _RUNS[key] = dict(outs=[o.cpu() for o in outs], taps={t: m.read_tap(t).cpu() for t in TAPS}, raw=m.read_tap("ori_level1_nchw").cpu())
        monkeypatch.delenv("CCVPE_COMPOSE_L6")
    return _RUNS[key]


def oracle_taps(name, batch, big_bias):
    key = (name, batch, big_bias)
    if key not in _ORACLE:
        cfg = gu.CONFIGS[name]
        g, s = inputs(name, batch)
        taps = {}
        orc.forward(cfg["variant"], state_dict(name, big_bias), g, s, cfg["circular"], cfg["ori_noise"], taps)
        _ORACLE[key] = {t: taps[t] for t in TAPS}
    return _ORACLE[key]


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


def border_rel(a, b):
    """The 16 x 16 map's border rows and columns on their own, over the whole map's scale."""
    assert a.shape[-2:] == (16, 16) and a.shape == b.shape
    edge = lambda t: torch.cat([t[..., 0, :], t[..., -1, :], t[..., :, 0], t[..., :, -1]], -1).double()
    return (edge(a) - edge(b)).abs().max().item() / b.double().abs().max().item()


def ori_weighted(a, b, raw):
    """The unit orientation fields compared where they are well defined: weighted by the un-normalised magnitude (tests/test_parity_gpu.py)."""
    mag = raw.double().pow(2).sum(dim=1, keepdim=True).sqrt()
    n = mag.shape[0]
    return ((a.double().reshape(n, 2, 512, 512) - b.double().reshape(n, 2, 512, 512)).abs() * mag).max().item() / mag.max().item()


def compare_runs(new, old, label):
    for t in TAPS:
        e = rel(new["taps"][t], old["taps"][t])
        print(f"{label} {t}: {e:.3g}")
        assert e < RTOL, (label, t, e)
    for i, (a, b) in enumerate(zip(new["outs"], old["outs"])):
        e = ori_weighted(a, b, old["raw"]) if i == 2 else rel(a, b)
        print(f"{label} {gu.OUTPUT_NAMES[i]}: {e:.3g}")
        assert e < RTOL, (label, gu.OUTPUT_NAMES[i], e)


def compare_oracle(new, name, batch, big_bias, label):
    want = oracle_taps(name, batch, big_bias)
    for t in TAPS:
        e, eb = rel(new["taps"][t], want[t]), border_rel(new["taps"][t], want[t])
        print(f"{label} vs oracle {t}: {e:.3g}, border {eb:.3g}")
        assert e < RTOL and eb < RTOL, (label, t, e, eb)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_composed_level6_matches_three_launches_and_oracle(name, batch, monkeypatch):
    new = run(name, batch, False, "1", monkeypatch)
    old = run(name, batch, False, "0", monkeypatch)
    compare_runs(new, old, f"{name} b{batch} vs COMPOSE_L6=0")
    compare_oracle(new, name, batch, False, f"{name} b{batch}")


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_dominant_deconv_bias(name, batch, monkeypatch):
    """The transposed conv's bias reaches conv6.0 through the border-case table; scaled up, it dominates the level-6 input terms.
    conv6.0's output is not a tap; the level's output (conv6.2 behind it) is - the whole map, and its border rows and columns on their
    own, where the edge and corner cases of the table apply."""
    new = run(name, batch, True, "1", monkeypatch)
    old = run(name, batch, True, "0", monkeypatch)
    label = f"{name} b{batch} big bias"
    compare_runs(new, old, label + " vs COMPOSE_L6=0")
    for t in TAPS:
        e = border_rel(new["taps"][t], old["taps"][t])
        print(f"{label} {t} border vs COMPOSE_L6=0: {e:.3g}")
        assert e < RTOL, (name, t, e)
    compare_oracle(new, name, batch, True, label)


def test_sixty_four_row_tile(monkeypatch):
    """Batch 9: 36 tile rows per group, the 64-row GEMM tile (batches 1 and 3 run the 32-row tile, batch 32 the 128-row one)."""
    new = run("oxford", 9, False, "1", monkeypatch)
    old = run("oxford", 9, False, "0", monkeypatch)
    compare_runs(new, old, "oxford b9 vs COMPOSE_L6=0")


def test_f2x2_form(monkeypatch):
    """CCVPE_COMPOSE_L6=2: F(2x2,2x2), nine positions, sixteen tiles per sample (48 rows at batch 3: the 64-row tile)."""
    new = run("oxford", 3, False, "2", monkeypatch)
    old = run("oxford", 3, False, "0", monkeypatch)
    compare_runs(new, old, "oxford b3 F(2x2,2x2) vs COMPOSE_L6=0")
    compare_oracle(new, "oxford", 3, False, "oxford b3 F(2x2,2x2)")


def test_handle_loaded_from_a_pack_file(tmp_path, monkeypatch):
    """The composed weights are derived from the packed weights, never stored: a handle that loaded a pack file runs the composed path
    with the bits of the handle that packed it, and composing adds nothing to the file."""
    monkeypatch.setenv("CCVPE_COMPOSE_L6", "1")
    sd = state_dict("oxford", False)
    g, s = inputs("oxford", 3)
    g, s = g.cuda(), s.cuda()
    a = make("oxford", sd, weight_cache=str(tmp_path))
    ref = [o.clone() for o in a(g, s)]
    assert a.last_weight_source == "state_dict"
    assert_path(plan_ops(a), True)
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 1 and files[0].endswith(".ccvpepack")
    size = os.path.getsize(tmp_path / files[0])
    monkeypatch.setenv("CCVPE_COMPOSE_L6", "0")
    plain = make("oxford", sd, weight_cache=str(tmp_path / "plain"))
    plain(g, s)
    assert_path(plan_ops(plain), False)
    plain_files = os.listdir(tmp_path / "plain")
    assert len(plain_files) == 1 and os.path.getsize(tmp_path / "plain" / plain_files[0]) == size
    monkeypatch.setenv("CCVPE_COMPOSE_L6", "1")
    b = make("oxford", sd, weight_cache=str(tmp_path))
    outs = b(g, s)
    assert b.last_weight_source == "packed-cache"
    assert_path(plan_ops(b), True)
    for i, (x, y) in enumerate(zip(ref, outs)):
        assert torch.equal(x, y), gu.OUTPUT_NAMES[i]


def test_automatic_rule(monkeypatch):
    """Nothing set: composed from 8 samples; batch 1 keeps the three launches and their launch count; bf16x3 plans keep them too."""
    monkeypatch.delenv("CCVPE_COMPOSE_L6", raising=False)
    lib = _lib.load()
    sd = state_dict("oxford", False)

    def launches(m, batch):
        g, s = inputs("oxford", batch)
        g, s = g.cuda(), s.cuda()
        m(g, s)   # builds (and, where the table does not know it, measures) the plan
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        m(g, s)
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    auto = make("oxford", sd)
    n1 = launches(auto, 1)
    assert_path(plan_ops(auto), False)
    launches(auto, 7)
    assert_path(plan_ops(auto), False)
    launches(auto, 8)
    assert_path(plan_ops(auto), True)
    monkeypatch.setenv("CCVPE_COMPOSE_L6", "0")
    off = make("oxford", sd)
    assert launches(off, 1) == n1
    monkeypatch.delenv("CCVPE_COMPOSE_L6")
    bf = make("oxford", sd, precision="bf16x3")
    launches(bf, 8)
    assert_path(plan_ops(bf), False)


def test_repeated_forwards_and_localize_are_bit_equal(monkeypatch):
    monkeypatch.setenv("CCVPE_COMPOSE_L6", "1")
    m = make("kitti", state_dict("kitti", False))
    g, s = inputs("kitti", 3)
    g, s = g.cuda(), s.cuda()
    first = [o.clone() for o in m(g, s)]
    assert_path(plan_ops(m), True)
    for _ in range(2):
        again = m(g, s)
        for i, (a, b) in enumerate(zip(first, again)):
            assert torch.equal(a, b), gu.OUTPUT_NAMES[i]
    rows = m.postprocess_rows(first[1], first[2])
    assert torch.equal(m.localize(g, s), rows)
