"""conv6.2 and the skip half of conv6.0 in split Winograd form on the grouped GEMM (kernels_level6.hip: split6_transform, level6_gemm
over 36 positions, split6_inverse), CCVPE_SPLIT_L6=1 against the tiled launches (=0) on the same seeded weights and
inputs: VIGOR at batch 8 (the smallest automatic batch: 128 rows, four 32-row tiles) and 9 (144 rows padded to 160: the zero-row path),
KITTI at batch 8 (512-channel level 6).  Both paths form the same Winograd products in another summation order, so the nine outputs and
the level-6 taps are held to the 1e-4 of scale of tests/test_level6_composed_gpu.py (`ori` weighted by the un-normalised magnitude).
Repeated forwards are bit-equal, forward_cached equals forward, and every run checks from the plan's launch list which path ran."""
import pytest
import torch

from tests import golden_util as gu
from tests import test_level6_composed_gpu as c6

pytestmark = pytest.mark.gpu

SPLIT_OPS = {f"{d}6.{op}" for d in ("loc", "ori") for op in ("b_transform", "conv_b", "b_inverse", "skip_transform", "conv_skip", "skip_inverse")}
ONLY_SPLIT = {o for o in SPLIT_OPS if o.endswith(("_transform", "_inverse"))}
CASES = [("vigor_prior180_circ", 8), ("vigor_prior180_circ", 9), ("kitti", 8)]

_RUNS = {}


def assert_split(ops, on):
    assert c6.COMPOSED_OPS <= ops, sorted(o for o in ops if "6." in o)          # the split form runs beside the composed level 6 only
    assert (SPLIT_OPS <= ops) if on else not (ONLY_SPLIT & ops), sorted(o for o in ops if "6." in o)


def run(name, batch, switch, monkeypatch):
    """Nine outputs, the level-6 taps and the un-normalised orientation field of one debug forward under CCVPE_SPLIT_L6=switch, on the
    CPU, and the model; computed once."""
    key = (name, batch, switch)
    if key not in _RUNS:
        monkeypatch.setenv("CCVPE_SPLIT_L6", switch)   # read at ccvpe_create, which the first forward reaches
        monkeypatch.setenv("CCVPE_AUTOTUNE", "0")      # batches 8 and 9 are not in the committed table: both handles run the heuristic's tiles
        m = c6.make(name, c6.state_dict(name, False))
        m.set_debug(True)
        g, s = c6.inputs(name, batch)
        outs = m(g.cuda(), s.cuda())
        torch.cuda.synchronize()
        monkeypatch.delenv("CCVPE_SPLIT_L6")
        monkeypatch.delenv("CCVPE_AUTOTUNE")
        assert_split(c6.plan_ops(m), switch == "1")
        _RUNS[key] = dict(outs=[o.cpu() for o in outs], taps={t: m.read_tap(t).cpu() for t in c6.TAPS}, raw=m.read_tap("ori_level1_nchw").cpu(),
                          model=m if key == (*CASES[0], "1") else None)   # (one handle is kept, for the bit-equality test)
    return _RUNS[key]


@pytest.mark.parametrize("name,batch", CASES)
def test_split_form_matches_the_tiled_launches(name, batch, monkeypatch):
    new = run(name, batch, "1", monkeypatch)
    old = run(name, batch, "0", monkeypatch)
    c6.compare_runs(new, old, f"{name} b{batch} vs SPLIT_L6=0")


def test_repeated_forwards_are_bit_equal_and_cached_equals_forward(monkeypatch):
    name, batch = CASES[0]
    m = run(name, batch, "1", monkeypatch)["model"]
    m.set_debug(False)
    g, s = c6.inputs(name, batch)
    g, s = g.cuda(), s.cuda()
    first = [o.clone() for o in m(g, s)]
    assert_split(c6.plan_ops(m), True)
    for _ in range(2):
        for i, (a, b) in enumerate(zip(first, m(g, s))):
            assert torch.equal(a, b), gu.OUTPUT_NAMES[i]
    cached = m.forward_cached(g, m.encode_aerial(s))
    assert_split(c6.plan_ops(m), True)
    for i, (a, b) in enumerate(zip(first, cached)):
        assert torch.equal(a, b), gu.OUTPUT_NAMES[i]
    m.set_debug(True)


def test_automatic_rule(monkeypatch):
    """Nothing set: split from 8 samples where the composed level 6 runs; batch 7 and bf16x3 plans keep the parent's launches."""
    monkeypatch.delenv("CCVPE_SPLIT_L6", raising=False)
    monkeypatch.setenv("CCVPE_AUTOTUNE", "0")
    sd = c6.state_dict("oxford", False)
    auto = c6.make("oxford", sd)
    for batch, on in ((7, False), (8, True)):
        g, s = c6.inputs("oxford", batch)
        auto(g.cuda(), s.cuda())
        torch.cuda.synchronize()
        ops = c6.plan_ops(auto)
        if on:
            assert_split(ops, True)
        else:
            assert not (ONLY_SPLIT & ops) and c6.THREE_LAUNCH_OPS <= ops
    bf = c6.make("oxford", sd, precision="bf16x3")
    g, s = c6.inputs("oxford", 8)
    bf(g.cuda(), s.cuda())
    torch.cuda.synchronize()
    ops = c6.plan_ops(bf)
    assert not (ONLY_SPLIT & ops) and c6.THREE_LAUNCH_OPS <= ops
