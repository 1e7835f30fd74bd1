"""The demodulator's launch plan (csrc/launch_plan.hpp) against launches recorded on the device.

Every workgroup shape of k_fused gives the same bits, so a wrong plan passes every parity test and only costs time.  The fixture
tests/golden/demod_launch_plan.json is what profiles/trace_launch_plan.py's handles launched under a kernel trace (channels x create
flags x design, and handles moved into another domain by the setters); here the plan function, built for the host, must imply
exactly those launches for every case.  No GPU needed."""
import json
import os

import pytest

from tests.emul import launch_plan_shim_bind as shim

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "demod_launch_plan.json")) as f:
    FIX = json.load(f)

# workgroup sizes of the three shapes (kernel_fused.hpp: six waves for 16 channels, eight for 4 and 32)
THREADS = {16: 384, 4: 512, 32: 512}
RELEASE_KERNELS = (["k_generic", "k_fused<true,false,32,0,false>"] +
                   ["k_fused<true,false,4,%d,%s>" % (d, l) for d in (0, 1, 2) for l in ("false", "true")] +
                   ["k_fused<true,false,16,%d,%s>" % (d, l) for d in (0, 1) for l in ("false", "true")])


def implied_launches(p, channels):
    """The ordered launches [kernel, workgroups, workgroup size] a plan means for a handle of `channels`."""
    if p["generic"]:
        return [["k_generic", -(-channels // p["lanes"]), 64]]
    out = []
    if p["n_wide"] > 0:
        out.append(["k_fused<true,false,32,0,false>", -(-p["n_wide"] // 32), THREADS[32]])
    rest = channels - p["n_wide"]
    if rest > 0:
        ch = p["rest_ch"]
        out.append(["k_fused<true,false,%d,%d,%s>" % (ch, p["deep"], "true" if p["long_rows"] else "false"), -(-rest // ch), THREADS[ch]])
    return out


def test_fixture_is_the_whole_matrix():
    chans = {1, 4, 5, 16, 17, 800, 1024, 1025, 4096, 4112, 8192, 8208, 12288, 16400}
    flags = {0, 16, 32, 64, 128}
    grid = {(c["design"], c["channels"], c["flags"]) for c in FIX["cases"] if "setter" not in c}
    assert grid == {(d, ch, fl) for d in FIX["designs"] for ch in chans for fl in flags}
    assert len(FIX["designs"]) >= 8
    assert sorted(c["setter"] for c in FIX["cases"] if "setter" in c) == ["set_param", "set_rrc_params", "set_tables"]


def test_fixture_reaches_every_release_kernel():
    seen = {l[0] for c in FIX["cases"] for l in c["launches"]}
    assert seen == set(RELEASE_KERNELS)      # all eleven k_fused instantiations and k_generic, and nothing else


def _case_id(c):
    return "%s-%d-%d" % (c["design"], c["channels"], c["flags"]) + ("-" + c["setter"] if "setter" in c else "")


@pytest.mark.parametrize("c", FIX["cases"], ids=_case_id)
def test_plan_implies_the_recorded_launches(c):
    # a handle moved by a setter plans like a fresh one of the design it was moved to
    p = shim.plan(c["channels"], c["cus"], c["flags"], **FIX["designs"][c["design"]])
    if c["status"] != 0:
        assert c["launches"] == []
        assert p is None      # the only refusal that depends on these inputs is the design's
        return
    assert p is not None
    assert implied_launches(p, c["channels"]) == c["launches"]
