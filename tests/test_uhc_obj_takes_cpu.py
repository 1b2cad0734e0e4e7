"""CPU: the UHC take library with objects -- SmplObjDataset against what the reference's DatasetSMPLObj makes of the same pickle
(tests/golden/uhc_obj_takes.npz, tools/make_golden_uhc_obj.py), AmassSingleDataset's 35-wide object block, KpTakes' shape refusals, the scripts' --dataset
flag and the new symbols of the built library."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PKL = os.path.join(GOLD, "uhc_obj_takes_small.pkl")
AMASS_PKL = os.path.join(GOLD, "uhc_takes_small.pkl")
SPECS = {"file_path": PKL, "test_file_path": PKL, "t_min": 90}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "uhc_obj_takes.npz"))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))       # 0 ulp, and -0.0 is not 0.0


def test_the_fixture_is_what_the_issue_asks_for(gold):
    import joblib
    takes = joblib.load(PKL)
    assert len(takes) == 6 and list(takes) == list(gold["take_names"])
    actions = [str(gold[f"action_{k}"]) for k in takes]
    assert sorted(actions) == ["avoid", "none", "push", "push", "sit", "step"]
    for k, v in takes.items():
        assert 95 <= v["qpos"].shape[0] <= 130 and v["qpos"].shape[1] == 76
        assert float(np.abs(v["qpos"][:, 7:] - v["qpos"][0, 7:]).max()) <= 2 * 0.05 + 1e-6          # amplitude <= 0.05 rad about the standing pose
    assert os.path.getsize(PKL) < 1.5 * os.path.getsize(AMASS_PKL)


def test_smpl_obj_dataset_against_the_reference(gold):
    from kinpoly_amd.dataset import SmplObjDataset, convert_obj_qpos_np
    import joblib
    raw = joblib.load(PKL)
    ds = SmplObjDataset(SPECS, "train")
    names = list(gold["take_names"])
    assert ds.data_keys == names and ds.get_len() == 6
    assert ds.lens.tolist() == [raw[k]["qpos"].shape[0] for k in names]
    for t_min in (90, 120):                                # the loader has no t_min filter: data_keys do not depend on it
        assert SmplObjDataset({**SPECS, "t_min": t_min}, "test").data_keys == list(gold[f"data_keys_tmin{t_min}"])
    none = list(gold["no_action_takes"])
    assert len(none) == 1
    for k in names:
        assert (ds.action[k] or "none") == str(gold[f"action_{k}"])
        assert _same_bits(ds.obj_qpos[k], gold[f"conv_{k}"]), k
        assert _same_bits(convert_obj_qpos_np(raw[k]["obj_pose"], ds.action[k]), gold[f"conv_{k}"]), k
    parked = gold[f"conv_{none[0]}"]
    assert np.array_equal(parked[:, 0::7], np.tile([100.0, 200, 300, 400, 500], (len(parked), 1))) and float(np.abs(parked[:, 3:7]).max()) == 0.0
    order = list(gold["iter_order"])
    assert order == names + names[:2]                       # once round, then the counter wraps
    for i, key in enumerate(order):
        s = ds.iter_seq()
        assert s["seq_name"] == key == ds.curr_key
        assert s["has_obj"] is True and bool(gold[f"iter{i}_has_obj"]) is True and s["num_obj"] == int(gold[f"iter{i}_num_obj"]) == 5
        assert _same_bits(s["qpos"], gold[f"iter{i}_qpos"]), key
        if key in none:                                     # the documented departure: the reference puts this take's placeholder chair at the origin
            assert _same_bits(s["obj_pose"], gold[f"conv_{key}"]) and not _same_bits(s["obj_pose"], gold[f"iter{i}_obj_pose"])
        else:
            assert _same_bits(s["obj_pose"], gold[f"iter{i}_obj_pose"]), key
    ds.set_seq_counter(3)
    assert ds.iter_seq()["seq_name"] == names[3]


def test_smpl_obj_dataset_modes_and_sampling():
    from kinpoly_amd.dataset import SmplObjDataset
    import joblib
    raw = joblib.load(PKL)
    names = list(raw)
    sub = SmplObjDataset({**SPECS, "mode": "singles", "key_subsets": [names[3], names[1]]}, "train")
    assert sub.data_keys == [names[3], names[1]]
    with pytest.raises(ValueError, match="mode"):
        SmplObjDataset({**SPECS, "mode": "some"}, "train")
    ds = SmplObjDataset(SPECS, "train")
    assert list(ds.new_freq_dict()) == names and all(v == [] for v in ds.new_freq_dict().values())
    p = ds.draw_probs(ds.new_freq_dict())
    np.testing.assert_array_equal(p, np.full(6, 1 / 6))     # uniform over sample_keys, whatever the history
    fd = ds.new_freq_dict(); fd[names[0]] = [[0.1, 0]] * 20
    np.testing.assert_array_equal(ds.draw_probs(fd), p)
    for _ in range(20):                                     # t_min: the rest of the take from a start that leaves at least t_min frames
        s = ds.sample_seq()
        n = raw[s["seq_name"]]["qpos"].shape[0]
        assert 0 <= s["fr_start"] < max(n - 90, 1) and s["qpos"].shape[0] == n - s["fr_start"] == s["obj_pose"].shape[0]
    win = SmplObjDataset({**SPECS, "t_max": 50}, "train")    # t_max: windows of t_max frames, a take counted len // t_max + 1 times
    assert [win.sample_keys.count(k) for k in names] == [raw[k]["qpos"].shape[0] // 50 + 1 for k in names]
    assert abs(win.draw_probs().sum() - 1.0) < 1e-15
    for _ in range(20):
        s = win.sample_seq()
        assert s["qpos"].shape[0] == 50 and s["fr_start"] + 50 <= raw[s["seq_name"]]["qpos"].shape[0]
    bad = {k: dict(v) for k, v in raw.items()}
    push = next(k for k in names if k.startswith("push"))
    bad[push]["obj_pose"] = bad[push]["obj_pose"][:, :7]
    with pytest.raises(ValueError, match=push):
        SmplObjDataset(SPECS, "train", takes=bad)


class _Recorder:
    """stands in for KpTakes: keeps what to_library hands over"""
    def __init__(self, sim, qpos_rows, take_off, dt, obj_rows=None):
        self.qpos_rows, self.take_off, self.dt, self.obj_rows = qpos_rows, take_off, dt, obj_rows


class _FakeSim:
    class model:
        @staticmethod
        def get_option(name):
            return 1.0 / 450.0


def test_amass_single_accepts_a_35_wide_object_block(monkeypatch):
    import joblib
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.dataset import AmassSingleDataset, convert_obj_qpos_np
    monkeypatch.setattr(kpsim, "KpTakes", _Recorder)
    takes = joblib.load(AMASS_PKL)
    own = np.arange(130 * 35, dtype=np.float64).reshape(130, 35) / 64.0
    t = dict(takes["take_d_130"]); t["obj_pose"] = own; t[True] = 1          # the one way :103-107 keeps a take's own obj_pose
    ds = AmassSingleDataset({"t_min": 90}, "train", takes={**takes, "take_d_130": t})
    assert ds.get_len() == 4 and list(ds.obj_pose) == ["take_d_130"]
    lib = ds.to_library(_FakeSim())
    assert lib.obj_rows.dtype == np.float32 and lib.obj_rows.shape == (int(ds.lens.sum()), 35) and lib.qpos_rows.shape == (int(ds.lens.sum()), 76)
    a = int(lib.take_off[ds.data_keys.index("take_d_130")])
    np.testing.assert_array_equal(lib.obj_rows[a:a + 130], own.astype(np.float32))
    np.testing.assert_array_equal(lib.obj_rows[:a], convert_obj_qpos_np(np.zeros((a, 7)), None).astype(np.float32))      # the others: everything parked
    assert AmassSingleDataset({"t_min": 90}, "train", takes=takes).to_library(_FakeSim()).obj_rows is None               # no object take, no object library
    for width in (14, 34):
        t = dict(takes["take_d_130"]); t["obj_pose"] = np.zeros((130, width)); t[True] = 1
        with pytest.raises(NotImplementedError, match="take_d_130"):
            AmassSingleDataset({"t_min": 90}, "train", takes={**takes, "take_d_130": t})


class _NoLibrary:
    """a KpSim whose library must not be reached"""
    device = "cpu"

    @property
    def L(self):
        return self

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the shapes were checked")


def test_kptakes_shape_refusals_come_before_any_library_call():
    from kinpoly_amd.sim import KpTakes
    q = np.zeros((10, 76), np.float32)
    for obj, msg in ((np.zeros((10, 34), np.float32), r"obj_rows must be \[R, 35\]"), (np.zeros((10, 7), np.float32), r"obj_rows must be \[R, 35\]"),
                     (np.zeros(350, np.float32), r"obj_rows must be \[R, 35\]"), (np.zeros((9, 35), np.float32), "obj_rows has 9 rows")):
        with pytest.raises(ValueError, match=msg):
            KpTakes(_NoLibrary(), q, [0, 10], obj_rows=obj)
    with pytest.raises(ValueError, match=r"qpos_rows must be \[R, 76\]"):
        KpTakes(_NoLibrary(), np.zeros((10, 75), np.float32), [0, 10], obj_rows=np.zeros((10, 35), np.float32))
    with pytest.raises(AssertionError, match="the library was reached"):          # the stand-in does catch a call
        _NoLibrary().L.kp_takes_create_obj


def _script(name):
    spec = importlib.util.spec_from_file_location(f"_script_{name}", os.path.join(ROOT, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["train_uhc", "eval_uhc"])
def test_scripts_accept_dataset(name):
    parser = _script(name).build_parser()
    assert parser.parse_args([]).dataset == "amass_single"
    assert parser.parse_args(["--dataset", "smpl_obj"]).dataset == "smpl_obj"
    with pytest.raises(SystemExit):
        parser.parse_args(["--dataset", "other"])


def test_library_exports_the_new_symbols():
    from kinpoly_amd import sim as kpsim
    L = kpsim.load_library()
    for sym in ("kp_takes_create_obj", "kp_takes_has_objects"):
        assert sym in kpsim._SIGNATURES and getattr(L, sym) is not None
    assert L.kp_takes_has_objects(None) == 0
    header = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    assert "kp_takes* kp_takes_create_obj(" in header and "int kp_takes_has_objects(" in header
