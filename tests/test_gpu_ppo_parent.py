"""The device path of the update (fp32: fused GRU re-unroll, k_gae, HIP FK) and of `CopycatAgent.sample` against the words the commit before
kinpoly_amd/ppo.py computed: tests/golden/ppo_parent_fp32_bits.npz, recorded on an MI355X by tools/make_golden_ppo_parent.py --device (the cases are
listed there; the update cases are those of tests/test_ppo_parent_cpu.py at the same shapes).

The bound is the parent's own run-to-run spread: three recordings in fresh processes on that commit agreed word for word in every array (largest
difference 0), so every array is held to bit equality."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("joint", "joint_alt0", "joint_alt1", "cc_train", "cc_eval", "uhc_fix", "uhc_std", "sample_expert", "sample_takes")


@pytest.fixture(scope="module")
def replayed():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_ppo_parent as tool
    finally:
        sys.path.pop(0)
    out = tool.update_cases("cuda", torch.float32)
    out.update(tool.sample_cases())
    return {k: (v.view(np.uint32) if v.dtype == np.float32 else v) for k, v in out.items()}


@pytest.mark.parametrize("case", CASES)
def test_device_path_equals_the_parent_commits_words(golden, replayed, case):
    g = golden("ppo_parent_fp32_bits")
    prefix = case + ("_" if case.startswith("sample") else "_c")          # "joint_c0_..." but not "joint_alt0_c0_..."
    keys = [k for k in g.files if k.startswith(prefix)]
    assert keys and set(keys) == {k for k in replayed if k.startswith(prefix)}
    for k in keys:
        assert g[k].dtype == replayed[k].dtype and np.array_equal(g[k], replayed[k]), k
    if case == "sample_takes":
        assert len(g["sample_takes_log"]) >= 64                    # every env finished an episode: the take ids, percents and the draw order are in the log
