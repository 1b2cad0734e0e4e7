"""CPU: the UHC's take data set (kinpoly_amd.dataset.AmassSingleDataset) and the agent's freq_dict bookkeeping, against the rules of
uhc/data_loaders/dataset_amass_single.py and uhc/core/agent_copycat.py restated here with their line numbers."""
import os
import types

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PKL = os.path.join(GOLD, "uhc_takes_small.pkl")
SPECS = {"file_path": PKL, "test_file_path": PKL, "t_min": 90}


def _ds(**kw):
    from kinpoly_amd.dataset import AmassSingleDataset
    return AmassSingleDataset({**SPECS, **kw}, "train")


def test_dataset_keeps_the_takes_of_t_min_in_file_order():
    ds = _ds()
    assert ds.data_keys == ["take_b_95", "take_c_96", "take_d_130", "take_e_200"]          # process_data_pickle :91-118: seq_len < t_min dropped
    assert ds.get_len() == 4 and list(ds.lens) == [95, 96, 130, 200]
    assert _ds(t_min=10).get_len() == 6


def test_singles_mode_reads_key_subsets():
    ds = _ds(mode="singles", key_subsets=["take_e_200", "take_b_95", "take_a_20"])
    assert ds.data_keys == ["take_e_200", "take_b_95"]                                    # :88-89, then the t_min rule


def test_takes_with_objects_are_refused_by_name():
    import joblib
    from kinpoly_amd.dataset import AmassSingleDataset
    takes = joblib.load(PKL)
    t = dict(takes["take_d_130"]); t["obj_pose"] = np.zeros((130, 7)); t[True] = 1          # the one way :103-107 keeps a take's own obj_pose
    with pytest.raises(NotImplementedError, match="take_d_130"):
        AmassSingleDataset(SPECS, "train", takes={**takes, "take_d_130": t})
    t2 = dict(takes["take_d_130"]); t2["obj_pose"] = np.zeros((130, 7))                    # without it obj_pose := qpos and has_obj is False
    assert AmassSingleDataset(SPECS, "train", takes={**takes, "take_d_130": t2}).get_len() == 4


def test_sample_probs_equal_the_reference_init_probs():
    """tests/golden/uhc_takes.npz holds the init_probs the reference's sample_seq (dataset_amass_single.py:162-175, ewma of math_utils.py:8-12) computed
    for three recorded freq_dicts: no history, all successes, mixed"""
    import json
    g = np.load(os.path.join(GOLD, "uhc_takes.npz"))
    ds = _ds()
    cases = json.loads(str(g["freq_cases"]))
    assert set(cases) == {"empty", "all_successes", "mixed"}
    for name, fd in cases.items():
        assert list(fd.keys()) == ds.data_keys
        np.testing.assert_allclose(ds.sample_probs(fd), g[f"probs_{name}"], rtol=0, atol=1e-12)
        d = ds.draw_probs(fd)                                                               # :177-181: init_probs with frequency 0.75, else uniform
        np.testing.assert_allclose(d, 0.75 * g[f"probs_{name}"] + 0.25 / 4, rtol=0, atol=1e-12)
    assert np.ptp(g["probs_empty"]) == 0 and np.ptp(g["probs_mixed"]) > 0.1


def test_eval_uhc_refuses_the_viewer_modes_and_takes_the_reference_command_line():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in (["--mode", "vis"], [], ["--mode", "disp_stats"], ["--mode", "stats", "--record"]):
        p = subprocess.run([sys.executable, "scripts/eval_uhc.py", *extra], cwd=root, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "viewer" in p.stderr and "--mode stats" in p.stderr, (extra, p.stderr)
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        import eval_uhc
    finally:
        sys.path.pop(0)
    # scripts/eval_uhc.py:245-262 of the reference: every option it defines parses, with its defaults
    a = eval_uhc.build_parser().parse_args(["--cfg", "uhc", "--iter", "1000", "--mode", "stats", "--data", "test", "--fail_safe", "--no_full", "--num_threads", "10",
                                            "--vis_model_file", "m", "--hide_expert", "--azimuth", "30", "--video_dir", "v", "--input", "--no_root", "--focus"])
    assert (a.cfg, a.iter, a.mode, a.data, a.fail_safe, a.no_full, a.num_threads, a.no_root) == ("uhc", 1000, "stats", "test", True, True, 10, True)
    d = eval_uhc.build_parser().parse_args([])
    assert (d.mode, d.data, d.iter, d.fail_safe, d.no_full, d.num_threads) == ("vis", "usr", -1, False, False, 20)
    with pytest.raises(SystemExit, match="no_root"):
        eval_uhc.check_mode(a)


def _agent(ds, tmp):
    from kinpoly_amd.uhc_env import CopycatAgent
    a = CopycatAgent.__new__(CopycatAgent)                                                  # the bookkeeping alone: no env, no GPU
    a.dataset, a.output_dir, a.freq_dict = ds, str(tmp), ds.new_freq_dict()
    return a


def test_freq_dict_append_cap_save_reload(tmp_path):
    import joblib
    ds = _ds()
    a = _agent(ds, tmp_path)
    a.record_episodes([(0, 0.5, 0), (3, 1.0, 0), (0, 1.0, 0)])
    assert a.freq_dict["take_b_95"] == [[0.5, 0], [1.0, 0]] and a.freq_dict["take_e_200"] == [[1.0, 0]] and a.freq_dict["take_c_96"] == []
    a.record_episodes([(1, i / 6000.0, 0) for i in range(6000)])
    assert len(a.freq_dict["take_c_96"]) == 5000 and a.freq_dict["take_c_96"][-1][0] == 5999 / 6000.0 and a.freq_dict["take_c_96"][0][0] == 1000 / 6000.0   # v[-5000:], :220
    a.save_freq_dict()
    assert joblib.load(os.path.join(tmp_path, "freq_dict.pt")) == a.freq_dict


def test_eval_feedback_is_one_or_three_entries(tmp_path):
    import joblib
    ds = _ds()
    a = _agent(ds, tmp_path)
    cov = a.feed_eval({"take_b_95": {"percent": 1.0}, "take_c_96": {"percent": 0.5}, "not_a_train_take": {"percent": 1.0}}, "train", 7)
    assert cov == 2                                                                          # :74-75 counts every result with percent == 1
    assert a.freq_dict["take_b_95"] == [[1.0, 0]] and a.freq_dict["take_c_96"] == [[0.5, 0]] * 3 and "not_a_train_take" not in a.freq_dict      # :76-78
    ev = joblib.load(os.path.join(tmp_path, "eval_dict_train.pt"))
    assert ev[7] == {"take_b_95": 1.0, "take_c_96": 0.5, "not_a_train_take": 1.0}            # :80-83


def test_uhc_config_reads_data_specs():
    from kinpoly_amd.uhc_config import UhcConfig
    specs = UhcConfig(os.path.join(GOLD, "uhc_variants", "uhc_v2_root.yml")).data_specs       # uhc.yml's block, read and not checked
    assert specs["t_min"] == 15 and specs["file_path"] == "sample_data/h36m_test.pkl" and specs["adaptive_iter"] == 200
