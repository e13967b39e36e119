"""The launch list of every plan form, with no GPU: tools/plan_text.cpp runs build_plan on a device-less stand-in handle over variants x
streams x level-1 fusion x handle flavours x batch x modes x forms (8960 keys, refused combinations included) and prints one line per
plan - label, return code, launches, tensors, workspace floats, ticket words and a 64-bit hash of the plan's full text (every launch's
name, stream, waits, FLOPs, bytes, GEMM shape, eligibility flags, tensors with sizes and offsets, the probed ConvParams of every tiled
launch, taps and issue order).  tests/plan_text_parent.txt holds the low 32 bits of those hashes, one line of 40 per (variant, streams,
fusion, flavour, batch) in the order modes 0-4 x forms (`plan_text --compact`), recorded before build_plan was restated as stages over
one builder: the plans must be the same, line for line.  A change that means to alter a plan re-records the file and
says so."""
import os
import subprocess

from ccvpe_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_are_the_recorded_ones(built_library, tmp_path):
    exe = str(tmp_path / "plan_text")
    csrc = os.path.dirname(built_library)
    cmd = [B._hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tools", "plan_text.cpp"), "-I" + csrc, "-L" + csrc,
           "-lccvpe_hip", "-Wl,-rpath," + csrc, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("CCVPE_")}      # the library's defaults: the program sets its own switches
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [line.split(" | ") for line in r.stdout.splitlines()]                     # (label, "rc ops tensors total tickets hash")
    want = {}
    for line in open(os.path.join(ROOT, "tests", "plan_text_parent.txt")).read().splitlines():
        group, hashes = line.split(" |")
        want[group] = hashes.split()
        assert len(want[group]) == 5 * 8
    assert len(want) == 4 * 2 * 2 * 7 * 2 and len(got) == 40 * len(want), "the grid: 224 groups of 40 keys"
    refused = sum(1 for _, rest in got if not rest.startswith("0 "))
    assert refused == 1344, "combinations refused (credible, heading and pair refusals)"
    seen = {}
    for label, rest in got:
        group = " ".join(label.split()[:5])
        k = seen[group] = seen.get(group, -1) + 1
        assert rest.split()[-1][-8:] == want[group][k], ("first differing plan: %s\n  built %s, recorded hash ...%s\n  (plan_text --plan \"%s\" prints it in full)"
                                                          % (label, rest, want[group][k], label))
