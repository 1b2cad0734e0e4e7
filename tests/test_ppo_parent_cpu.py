"""The update paths no reference fixture reaches -- `PPOTrainer.update_joint` (both forms), `PPOTrainer.update` with a controller (trained, and the
single evaluation) and `CopycatAgent.optimize_policy` -- against what the four separate loops computed before they were folded onto the shared steps of
kinpoly_amd/ppo.py: tests/golden/ppo_parent_fp64.npz, recorded by tools/make_golden_ppo_parent.py on that earlier commit (CPU, fp64, one torch thread;
the cases are listed there).  The replay here is that tool's own `update_cases`.

Tolerances are those of tests/test_update_cpu.py for the same arithmetic across hosts: losses 1e-12, parameters and advantages 1e-13.  On the host the
fixture was recorded on the largest difference over all 448 arrays is exactly 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_LOSS, TOL_PARAM, TOL_ADV = 1e-12, 1e-13, 1e-13
CASES = ("joint", "joint_alt0", "joint_alt1", "cc_train", "cc_eval", "uhc_fix", "uhc_std")


@pytest.fixture(scope="module")
def replayed():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_ppo_parent as tool
    finally:
        sys.path.pop(0)
    return tool.update_cases()


def test_fixture_exercises_what_it_pins(golden):
    g = golden("ppo_parent_fp64")
    assert {k.split("_c")[0] for k in g.files if k.endswith("_stats")} == set(CASES)
    assert g["joint_c0_clip"].shape == (1,) and g["joint_c0_clip"][0] > 40 and g["joint_c1_clip"].size == 0        # the consumed clip: one call per run sees the parameters
    assert g["joint_alt0_c0_clip"].size == 0 and g["joint_alt1_c0_clip"].shape == (1,)                              # supervised steps are not clipped
    assert g["uhc_fix_c0_clip"].shape == (3,)                                                                      # the UHC agent clips every step
    assert g["cc_train_c0_surr"].shape == (6,) and g["cc_eval_c0_surr"].shape == (4,)                              # 3 policy epochs + 3 controller epochs / 1 evaluation
    assert g["cc_eval_c0_stats"][2] == g["cc_eval_c0_surr"][3] == g["cc_train_c0_surr"][3]                        # epoch 0 of the trained controller is that evaluation
    assert g["uhc_fix_c1_moved"][0] == 0 and g["uhc_std_c1_moved"][0] > 1e-3                                       # log_std moves only with fix_std=False
    for case in ("joint", "joint_alt1", "uhc_fix"):
        assert abs(g[case + "_c0_surr"][0]) < 1e-15 and abs(g[case + "_c0_surr"][-1]) > 1e-2                       # epoch 0's ratio is 1; later epochs are not


@pytest.mark.parametrize("case", CASES)
def test_update_paths_land_on_the_parent_commits_numbers(golden, replayed, case):
    g = golden("ppo_parent_fp64")
    keys = [k for k in g.files if k.startswith(case + "_c")]
    assert keys and set(keys) == {k for k in replayed if k.startswith(case + "_c")}
    worst = {"loss": 0.0, "param": 0.0, "adv": 0.0}
    for k in keys:
        want, got = g[k], replayed[k]
        assert want.shape == got.shape, k
        kind = k.rsplit("_", 1)[1]
        if want.size == 0:
            continue
        err = float(np.abs(got - want).max())
        if ":" in k:                                       # <case>_c<call>_<p|v|cc>:<parameter name>
            worst["param"] = max(worst["param"], err)
            assert err <= TOL_PARAM, (k, err)
        elif kind in ("adv", "ret"):
            worst["adv"] = max(worst["adv"], err)
            assert err <= TOL_ADV, (k, err)
        elif kind == "moved":
            # every tensor that moved moved by far more than the tolerance it is met to; the others (log_std, the context network, an untrained UHC) stayed put
            assert ((want == 0) == (got == 0)).all() and (got[got > 0] > 1e8 * TOL_PARAM).all(), (k, got)
        elif kind == "surr":
            worst["loss"] = max(worst["loss"], err)
            np.testing.assert_allclose(got, want, rtol=0, atol=TOL_LOSS, err_msg=k)
        else:                                              # vloss, step, stats, clip: relative as well, as test_update_cpu.compare does
            worst["loss"] = max(worst["loss"], err)
            np.testing.assert_allclose(got, want, rtol=TOL_LOSS, atol=TOL_LOSS, err_msg=k)
    print(case, "max |difference| to the parent:", worst)
