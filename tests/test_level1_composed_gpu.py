"""The fused last decoder level with the transposed conv composed into the first 3x3 conv (kernels_level1_tile.inc): against the unfused
launches (CCVPE_FUSE_L1=0) and the oracle's taps for every variant, with a deconv bias large enough that a wrong border-bias case shows,
and the pose-only forms bit-identical to forward + post-processing."""
import pytest
import torch

from ccvpe_amd import models, weights
from oracle import ccvpe_oracle as orc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # scale-relative, as tests/test_parity_gpu.py holds the fp32 path


def make(name, sd=None):
    cfg = gu.CONFIGS[name]
    v = cfg["variant"]
    if v == "vigor":
        m = models.CVM_VIGOR("cuda", cfg["circular"])
    elif v == "vigor_ori_prior":
        m = models.CVM_VIGOR_ori_prior("cuda", cfg["ori_noise"], cfg["circular"])
    elif v == "kitti":
        m = models.CVM_KITTI("cuda")
    else:
        m = models.CVM_OxfordRobotCar("cuda")
    m.load_state_dict(sd if sd is not None else weights.generate_state_dict(v, cfg["seed"]))
    return m.to("cuda").eval()


def inputs(name, batch=1, seed=None):
    cfg = gu.CONFIGS[name]
    g, s = weights.generate_inputs(cfg["variant"], batch, cfg["seed"] if seed is None else seed, cfg["fov"])
    return torch.from_numpy(g), torch.from_numpy(s)


def level1_outputs(name, sd, g, s):
    """(logits, un-normalised orientation field) of one debug forward, on the CPU."""
    m = make(name, sd)
    m.set_debug(True)
    outs = m(g.cuda(), s.cuda())
    torch.cuda.synchronize()
    return grid(outs[0].cpu()), m.read_tap("ori_level1_nchw").cpu()


def grid(logits):
    """[B, 1, 512, 512] view of the (flattened) logits."""
    return logits.reshape(logits.shape[0], 1, 512, 512)


def rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


def fused_vs_unfused(name, sd, g, s, monkeypatch):
    fused = level1_outputs(name, sd, g, s)
    monkeypatch.setenv("CCVPE_FUSE_L1", "0")   # read at ccvpe_create
    unfused = level1_outputs(name, sd, g, s)
    monkeypatch.delenv("CCVPE_FUSE_L1")
    return fused, unfused


@pytest.mark.parametrize("name", ["vigor_circ", "kitti", "oxford"])
def test_composed_level1_matches_unfused_and_oracle(name, monkeypatch):
    v = gu.CONFIGS[name]["variant"]
    sd = weights.generate_state_dict(v, gu.CONFIGS[name]["seed"])
    g, s = inputs(name)
    (logits, raw), (logits_u, raw_u) = fused_vs_unfused(name, sd, g, s, monkeypatch)
    assert rel(logits, logits_u) < RTOL, name
    assert rel(raw, raw_u) < RTOL, name
    taps = {}
    ref = orc.forward(v, sd, g, s, gu.CONFIGS[name]["circular"], gu.CONFIGS[name]["ori_noise"], taps)
    assert rel(logits, grid(ref[0])) < RTOL, name
    assert rel(raw, taps["ori_level1"]) < RTOL, name


@pytest.mark.parametrize("name", ["vigor_circ", "kitti"])
def test_dominant_deconv_bias(name, monkeypatch):
    """The transposed conv's bias reaches conv_a through the border-case table; scaled up, it dominates the level-1 input terms."""
    v = gu.CONFIGS[name]["variant"]
    sd = weights.generate_state_dict(v, gu.CONFIGS[name]["seed"])
    for key in ("deconv1.bias", "deconv1_ori.bias"):
        sd[key] = sd[key] * 50.0 + torch.sign(sd[key])
    g, s = inputs(name)
    (logits, raw), (logits_u, raw_u) = fused_vs_unfused(name, sd, g, s, monkeypatch)
    assert rel(logits, logits_u) < RTOL
    assert rel(raw, raw_u) < RTOL
    # the image border (where the table's edge and corner cases apply) on its own
    for a, b in ((logits, logits_u), (raw, raw_u)):
        edge = torch.cat([a[..., 0, :], a[..., -1, :], a[..., :, 0], a[..., :, -1]], -1)
        edge_u = torch.cat([b[..., 0, :], b[..., -1, :], b[..., :, 0], b[..., :, -1]], -1)
        assert (edge.double() - edge_u.double()).abs().max().item() < RTOL * b.double().abs().max().item()


@pytest.mark.parametrize("name", ["kitti", "oxford"])
def test_pose_forms_equal_forward(name):
    m = make(name)
    g, s = inputs(name, batch=2, seed=5)
    g, s = g.cuda(), s.cuda()
    outs = m(g, s)
    rows = m.postprocess_rows(outs[1], outs[2])
    topk = m.postprocess_topk(outs[1], outs[2], 4, 8)
    assert torch.equal(m.localize(g, s), rows)
    assert torch.equal(m.localize_topk(g, s, 4, 8), topk)
