"""The C-ABI library: builds for gfx950, loads, exports every symbol include/ccvpe.h declares, and
fails loudly without a GPU (no compute calls here)."""
import ctypes as C
import os
import re

import pytest
import torch

from ccvpe_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "ccvpe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ccvpe_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_header_symbols(built_library):
    lib = C.CDLL(built_library)
    names = header_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ccvpe.h but not exported"
    assert sorted(n for n, _, _ in _lib.SYMBOLS) == names, "ccvpe_amd._lib binds exactly the header's functions"


def test_struct_layouts_match_header():
    assert C.sizeof(_lib.Config) == 32
    assert C.sizeof(_lib.Outputs) == 9 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.Pose) == 20


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_create_fails_loudly_without_gpu(built_library):
    lib = _lib.load()
    cfg = _lib.Config(variant=1, circular_padding=1, ori_noise=180.0, device=0, micro_batch=0)
    h = C.c_void_p()
    rc = lib.ccvpe_create(C.byref(cfg), C.byref(h))
    assert rc < 0
    assert b"no CPU fallback" in lib.ccvpe_last_error() or b"HIP" in lib.ccvpe_last_error()


def test_null_arguments_are_rejected(built_library):
    lib = _lib.load()
    assert lib.ccvpe_create(None, None) == -1
    assert lib.ccvpe_forward(None, None, 0, 0, None, 0, None, None) == -1
    assert lib.ccvpe_destroy(None) == 0
    assert lib.ccvpe_version().startswith(b"ccvpe-hip")


def test_micro_batch_bound_is_host_arithmetic():
    """Every kernel addresses tensors with 32-bit byte offsets; the library must refuse (not wrap) a micro-batch whose
    largest tensor reaches 2 GiB.  ccvpe_max_micro_batch is pure host code: the 6x-expanded 256x256x96 tensor of the
    aerial encoder (25.2 MB per sample) caps every variant at 85 samples per pass."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    for variant, noise, gh, gw in [(0, 0.0, 320, 640), (1, 180.0, 320, 640), (1, 72.0, 320, 192), (2, 0.0, 256, 1024), (3, 0.0, 154, 231)]:
        cap = lib.ccvpe_max_micro_batch(variant, noise, gh, gw)
        assert cap == (2 ** 31 - 1) // (256 * 256 * 96 * 4), (variant, cap)
    assert lib.ccvpe_max_micro_batch(2, 0.0, 250, 1024) < 0          # 7 feature rows: not a KITTI-shaped ground image
    assert b"feature volume" in lib.ccvpe_last_error()
    assert lib.ccvpe_max_micro_batch(7, 0.0, 320, 640) < 0


def test_environment_is_read_only_by_read_switches():
    """Every environment switch of the library is read once per handle, at ccvpe_create, by read_switches() (ccvpe_api.hip):
    no other function under ccvpe_amd/csrc calls getenv - a switch latched elsewhere (a function-local static, a plan builder) would
    give the process, a plan or the packed-weight cache key a different value than the handle."""
    csrc = os.path.join(ROOT, "ccvpe_amd", "csrc")
    offenders, readers = [], 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
        m = re.search(r"^Switches read_switches\(\) \{\n.*?^\}\n", text, flags=re.S | re.M)
        if m:
            readers += 1
            assert re.search(r"\bgetenv\s*\(", m.group(0))
            text = text[:m.start()] + text[m.end():]
        offenders += [f"{f}: {line.strip()}" for line in text.splitlines() if re.search(r"\bgetenv\s*\(", line)]
    assert readers == 1, "read_switches() is defined once"
    assert not offenders, "getenv outside read_switches():\n" + "\n".join(offenders)


def test_pose_tail_has_one_definition():
    """The output side's forms promise each other's bits (the recomputed posterior against the stored heatmap, logits forms against
    network forms, ties and NaN alike), so what they must agree on is written once: the (value, first index) tie-break and the
    posterior expression `__expf(x - m) * inv` occur in tail_shared.h alone, and ccvpe_api.hip fills no tail kernel's parameters
    itself - it issues the tail through ccvpe_plan.hip's issue_* functions like the plans.  The one exception is the stored-heatmap
    top-K of ccvpe_postprocess_topk, which has no softmax and reads no logits."""
    csrc = os.path.join(ROOT, "ccvpe_amd", "csrc")

    def code(f):
        return re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())

    tie = re.compile(r"(\w+)\s*>\s*(\w+)\s*\|\|\s*\(\s*\1\s*==\s*\2\s*&&\s*\w+\s*<\s*\w+\s*\)")
    post = re.compile(r"__expf\s*\([^;]*?-\s*m\s*\)\s*\*\s*inv\b")
    sources = ["kernels_tail.hip", "kernels_heading.hip", "kernels_hprior.hip", "tail_shared.h"]
    sources += sorted(f for f in os.listdir(csrc) if f.startswith(("kernels_track", "track_")) and f.endswith((".hip", ".h")))
    assert len(sources) > 4, "the track kernels' files"
    for f in sources:
        text = code(f)
        if f == "kernels_tail.hip":   # region_reduce_kernel's pair reduction (float64 joint probabilities, an eligibility flag) is another merge
            m = re.search(r"void region_reduce_kernel\(.*?^\}\n", text, flags=re.S | re.M)
            assert m
            text = text[:m.start()] + text[m.end():]
        want = 1 if f == "tail_shared.h" else 0
        assert len(tie.findall(text)) == want, f"{f}: the tie-break comparison is argmax_merge (tail_shared.h)"
        assert len(post.findall(text)) == want, f"{f}: the posterior expression is posterior_value (tail_shared.h)"
    api = code("ccvpe_api.hip")
    for name in ("PoseArgmaxParams", "HeadingParams", "SoftmaxParams"):
        assert not re.search(r"\b%s\b" % name, api), f"ccvpe_api.hip fills a {name} of its own"
    inits = [m.start() for m in re.finditer(r"\bTopkParams\b", api)]
    assert len(inits) == 1, "ccvpe_api.hip: one TopkParams, the stored-heatmap form's"
    fn = api.rfind("\nint ccvpe_", 0, inits[0])
    assert api[fn:].startswith("\nint ccvpe_postprocess_topk("), api[fn:fn + 60]
    plan = code("ccvpe_plan.hip")
    for fn_name in ("issue_softmax_partial", "issue_pose_argmax", "issue_topk_peaks", "issue_pose_heading"):
        assert len(re.findall(r"^void %s\(" % fn_name, plan, flags=re.M)) == 1 and re.search(r"\b%s\(" % fn_name, api), fn_name


def test_plan_launches_have_one_description():
    """build_plan is an ordered list of stages over one file-local builder, and the launches that several plan forms
    share are described once: the Level1Params fill from a DecoderW (level1_params: the fused full-plan launch, ori1.pose / ori1.topk and
    ccvpe_op_level1), the 3x3 eligibility flags (one setter, and the level-6 skip layer's own conditions beside it), the read of an aerial
    cache section (gather when indexed, else scatter) and sat.descmap (the full and the aerial-encode plan).  A plan outlives its builder:
    build_plan nests no by-reference lambda, and the builder's stages hold no lambda at all - every closure is made in a free function,
    where there is no builder to capture."""
    csrc = os.path.join(ROOT, "ccvpe_amd", "csrc")
    plan = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "ccvpe_plan.hip")).read())
    both = plan + re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "ccvpe_api.hip")).read())
    assert len(re.findall(r"\.wc\s*=\s*\w+\.l1_wc\b", both)) == 1, "the Level1Params fill is level1_params"
    assert re.search(r"^Level1Params level1_params\(", plan, flags=re.M) and re.search(r"\blevel1_params\(", both[len(plan):])
    assert 1 <= len(re.findall(r"\bwino4x_ok\s*=[^=]", both)) <= 2, "the 3x3 flag setter and the level-6 skip layer's conditions"
    assert both.count("launch_scatter_channels(c.cache_in") == 1, "one description of a cache section's read"
    assert both.count('"sat.descmap"') == 1
    assert not re.search(r"\bfused_done\b", both)
    m = re.search(r"^int build_plan\(.*?^\}\n", plan, flags=re.S | re.M)
    assert m and "[&" not in m.group(0), "build_plan nests no lambda that captures by reference"
    assert len([ln for ln in m.group(0).splitlines() if ln.strip()]) < 60, "build_plan fits on one screen"
    b = re.search(r"^struct PlanBuilder \{.*?^\};\n", plan, flags=re.S | re.M)
    assert b and not re.search(r"\[[=&][^\]]*\]|\[\]\s*\(|\[this\]", b.group(0)), "a stage of the builder holds no lambda"


def test_conv_hook_descriptor_refusals(built_library):
    """ccvpe_op_conv2d_ex refuses a bad descriptor before it touches the device: the pointers below are never dereferenced."""
    lib = _lib.load()
    assert C.sizeof(_lib.OpConvDesc) == 192 and C.sizeof(_lib.OpConvDst) == 16
    assert lib.ccvpe_op_conv2d_ex(None, None) == -1
    fake = 0x1000

    def desc(**kw):
        d = _lib.OpConvDesc()
        d.x, d.w = fake, fake
        d.B, d.H, d.W, d.Cin, d.in_ld = 1, 8, 8, 16, 16
        d.Cout, d.KH, d.KW, d.stride, d.pad, d.act, d.tile, d.mode = 8, 1, 1, 1, 0, 0, 0, 0
        d.ndst = 1
        d.dst[0].ptr, d.dst[0].ld, d.dst[0].coff = fake, 8, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d, text):
        assert lib.ccvpe_op_conv2d_ex(C.byref(d), None) == -1
        assert text in lib.ccvpe_last_error(), lib.ccvpe_last_error()

    refused(desc(x=None), b"null argument")
    refused(desc(Cin=12, in_ld=12), b"Cin must be a multiple of 8")
    refused(desc(mode=2), b"unknown mode")
    refused(desc(mode=1), b"transposed conv is 2x2")
    refused(desc(in_ld=12), b"in_ld")
    refused(desc(in_ld=18), b"in_ld")
    refused(desc(B=1 << 15, H=1 << 8, W=1 << 8, in_ld=16), b"2^31")
    refused(desc(gate=fake, KH=3, KW=3, pad=1), b"gate")
    refused(desc(gate=fake, mode=1, KH=2, KW=2, stride=2), b"gate")
    refused(desc(resid=fake, resid_ld=8, act=2), b"residual")
    refused(desc(resid=fake, resid_ld=4), b"resid_ld")
    refused(desc(resid=fake, resid_ld=8, mode=1, KH=2, KW=2, stride=2), b"residual")
    refused(desc(ndst=0), b"ndst")
    refused(desc(ndst=4), b"ndst")
    d = desc(ndst=2)
    refused(d, b"null destination 1")
    d = desc()
    d.dst[0].coff = 4
    refused(d, b"coff + Cout")
    d = desc(B=1 << 11, H=1 << 8, W=1 << 8)      # 2^27 pixels: the input fits, a 16-float destination row does not
    d.dst[0].ld = 16
    refused(d, b"2^31")
