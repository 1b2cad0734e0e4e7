"""CPU: the reward functions beside world_rfc_implicit / dynamic_supervision_v1 against tests/golden/reward_variants.npz, which holds the reference's
own five functions in fp64 (tools/make_golden_rewards.py): the numpy restatements of tests/reward_oracle.py, the torch functions of
kinpoly_amd.uhc_env in fp64, the config readers' per-function defaults and refusals, and the exported symbols."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

from kinpoly_amd import build as kpbuild
from kinpoly_amd.config import REWARD_DEFAULTS as KIN_DEFAULTS, Config, ConfigError
from kinpoly_amd.uhc_config import REWARD_DEFAULTS, UhcConfig
import reward_oracle as R

GOLD = R.GOLD
G, EX = R.load_fixture()
CASES = list(range(len(G["rid"])))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def test_fixture_covers_the_cases():
    names = {rid: {str(n) for n, r in zip(G["name"], G["rid"]) if str(r) == rid} for rid in R.UHC_IDS}
    for rid in R.UHC_IDS:
        assert {"plain", "expert", "sign_flip", "joint_pi", "heading_pi", "heading_minus_pi", "last_row", "past_the_end"} <= names[rid]
        sel = [i for i in CASES if str(G["rid"][i]) == rid]
        assert {int(G["vf_dim"][i]) for i in sel} == {0, 6}
        assert any(json.loads(str(G["ws"][i])) == {} for i in sel) and any(len(json.loads(str(G["ws"][i]))) > 3 for i in sel)
    assert any(str(G["rid"][i]) == "local_rfc_implicit" and json.loads(str(G["ws"][i])).get("w_vf") == 0.0 and G["info"][i][5] == 0.0 for i in CASES)
    T = G["k_gt_bquat"].shape[1]
    assert {1, T - 1} <= {int(t) for t in G["k_t"]}
    # the state that IS the expert: every term that compares like with like is exactly 1
    for i in CASES:
        if str(G["name"][i]) == "expert" and str(G["rid"][i]) != "local_rfc_implicit":
            assert np.all(G["info"][i][:int(G["info_dim"][i])] > 1 - 1e-12)


@pytest.mark.parametrize("i", CASES)
def test_restatement_matches_reference(i):
    rid, s, ind, action, vf_dim, ws, jw, reward, info = R.uhc_case(G, EX, i)
    r, inf = R.UHC_FUNCS[rid](s, EX, ind, action, vf_dim, ws, G["b_diffw"], jw, float(G["dt"]))
    assert inf.shape == info.shape
    assert _rel(r, reward) <= 1e-12 and _rel(inf, info) <= 1e-12


@pytest.mark.parametrize("i", range(len(G["k_t"])))
def test_kin_v2_restatement_matches_reference(i):
    args, reward, info = R.kin_case(G, i)
    r, inf = R.dynamic_supervision_v2(*args)
    assert _rel(r, reward) <= 1e-12 and _rel(inf, info) <= 1e-12


@pytest.mark.parametrize("i", CASES)
def test_torch_fp64_matches_reference(i):
    from oracle import np_oracle as O
    rid, s, ind, action, vf_dim, ws, jw, reward, info = R.uhc_case(G, EX, i)
    rows = {k: np.asarray(v).reshape(1, -1) for k, v in s.items()}
    rows["bquat"] = O.get_body_quat(s["qpos"])[None]
    ex_row = {k: EX[k][ind][None] for k in ("qpos", "bquat", "bangvel", "ee_wpos", "ee_pos", "com", "rq_rmh", "rlinv_local", "rangv", "wbquat", "wbpos", "body_com")}
    r, inf = R.torch_reward(rid, rows, ex_row, action[None], vf_dim, ws, np.concatenate([[1.0], G["b_diffw"]]), jw, float(G["dt"]))
    assert inf.shape == (1, len(info))
    assert _rel(r.numpy()[0], reward) <= 1e-10 and _rel(inf.numpy()[0], info) <= 1e-10


@pytest.mark.parametrize("i", range(len(G["k_t"])))
def test_kin_v2_torch_form_matches_reference(i):
    """the torch form the GPU test takes its fp32 figure from, in fp64"""
    from oracle import np_oracle as O
    (qpos, xpos, xquat, prev_bquat, hp, gb, gbp, gw, ws, b_diffw, dt), reward, info = R.kin_case(G, i)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64).reshape(1, -1))      # noqa: E731
    r, inf = R.dynamic_supervision_v2_t(t(O.get_body_quat(qpos)), t(xpos), t(xquat), t(prev_bquat), t(hp), t(gb), t(gbp), t(gw), ws,
                                        torch.as_tensor(np.concatenate([[1.0], b_diffw])), dt)
    assert _rel(r.numpy()[0], reward) <= 1e-10 and _rel(inf.numpy()[0], info) <= 1e-10


# ------------------------------------------------------------------ config readers
@pytest.mark.parametrize("rid", R.UHC_IDS)
def test_uhc_config_accepts_the_id_with_its_own_defaults(rid):
    cfg = UhcConfig(os.path.join(GOLD, "uhc_rewards", rid + ".yml"))
    assert cfg.reward_id == rid
    ws = cfg.full_reward_weights()
    jw = ws.pop("jpos_diffw", None)
    assert ws == {k: float(v) for k, v in R.DEFAULTS[rid].items()} and set(REWARD_DEFAULTS[rid]) == set(R.DEFAULTS[rid])
    assert (jw == [1.0] * 24) if rid in ("world_rfc_implicit_v2", "world_rfc_implicit_v3") else jw is None
    from kinpoly_amd.sim import UHC_REWARD_IDS, uhc_reward_info_dim
    assert rid in UHC_REWARD_IDS and uhc_reward_info_dim(rid) == (5 if rid == "world_rfc_implicit_v1_mul" else 6)


def test_uhc_config_overrides_and_the_default_id_unchanged(tmp_path):
    y = yaml.safe_load(open(os.path.join(GOLD, "uhc_rewards", "world_rfc_implicit_v2.yml")))
    y["reward_weights"] = {"k_j": 40.0, "jpos_diffw": [0.5] * 24, "w_p": 9.0}          # w_p: a key v2 does not read
    p = tmp_path / "v.yml"; p.write_text(yaml.safe_dump(y))
    ws = UhcConfig(str(p)).full_reward_weights()
    assert ws["k_j"] == 40.0 and ws["k_p"] == 0.4 and ws["jpos_diffw"] == [0.5] * 24 and "w_p" not in ws
    y["reward_weights"]["jpos_diffw"] = [1.0] * 23
    p.write_text(yaml.safe_dump(y))
    with pytest.raises(ConfigError, match="jpos_diffw"):
        UhcConfig(str(p))
    d = UhcConfig(os.path.join(GOLD, "uhc_variants", "uhc_v2_root.yml"))
    assert d.reward_id == "world_rfc_implicit" and d.full_reward_weights() == dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)


@pytest.mark.parametrize("rid,why", [("quat", "registry"), ("world_rfc_explicit", "vf_bodies"), ("local_rfc_explicit", "vf_bodies")])
def test_uhc_config_still_refuses(tmp_path, rid, why):
    y = yaml.safe_load(open(os.path.join(GOLD, "uhc_rewards", "local_rfc_implicit.yml")))
    y["reward_id"] = rid
    p = tmp_path / "v.yml"; p.write_text(yaml.safe_dump(y))
    with pytest.raises(ConfigError) as e:
        UhcConfig(str(p))
    msg = str(e.value)
    assert f"reward_id: {rid!r} (implemented: " in msg and why in msg and "'world_rfc_implicit_v3'" in msg


class _Env:
    """what Config.apply_reward_weights touches of an env"""
    def __init__(self):
        from kinpoly_amd.sim import KpRewardCfg
        self.reward_cfg, self.reward_id = KpRewardCfg.default(), "dynamic_supervision_v1"

    def set_reward(self, rid):
        from kinpoly_amd.sim import KpRewardCfgV2
        if rid == "dynamic_supervision_v2":
            self.reward_cfg = KpRewardCfgV2()
        self.reward_id = rid


@pytest.mark.parametrize("entry", ["policy", "policy_ctx"])
def test_kin_config_accepts_v2(entry):
    cfg = Config(os.path.join(GOLD, "kin_poly_reward_v2.yml"), entry=entry)
    assert cfg.reward_id == "dynamic_supervision_v2"
    env = _Env()
    rc = cfg.apply_reward_weights(env)
    want = {**R.DEFAULTS["dynamic_supervision_v2"], "w_p": 0.5, "k_e": 10.0}
    assert env.reward_id == "dynamic_supervision_v2" and set(KIN_DEFAULTS["dynamic_supervision_v2"]) == set(want)
    for k, v in want.items():
        assert getattr(rc, k) == pytest.approx(float(v), rel=1e-7)
    v1 = Config(os.path.join(GOLD, "kin_poly_wo_action.yml"))
    assert v1.reward_id == "dynamic_supervision_v1" and v1.apply_reward_weights(_Env()).k_jp == pytest.approx(float(v1.reward_weights.get("k_jp", 0.1)))


def test_kin_config_still_refuses_v3(tmp_path):
    y = yaml.safe_load(open(os.path.join(GOLD, "kin_poly_reward_v2.yml")))
    y["policy_specs"]["reward_id"] = "dynamic_supervision_v3"
    p = tmp_path / "v.yml"; p.write_text(yaml.safe_dump(y))
    with pytest.raises(ConfigError) as e:
        Config(str(p))
    assert "policy_specs.reward_id: 'dynamic_supervision_v3'" in str(e.value) and "reward_function.py:1055-1056" in str(e.value)


def test_new_symbols_are_exported():
    if not os.path.exists(kpbuild.LIB):
        kpbuild.build_native()
    L = ctypes.CDLL(kpbuild.LIB)
    for sym in ("kp_sim_uhc_track_r", "kp_uhc_reward_info_dim", "kp_sim_term_reward_v2", "kp_sim_post_step_v2"):
        assert hasattr(L, sym), sym
    L.kp_uhc_reward_info_dim.restype = ctypes.c_int
    assert [L.kp_uhc_reward_info_dim(i) for i in range(-1, 6)] == [-1, 5, 5, 6, 6, 6, -1]
    from kinpoly_amd.sim import KpRewardCfgV2, KpUhcCfg, KpUhcCfgR
    assert ctypes.sizeof(KpUhcCfgR) == ctypes.sizeof(KpUhcCfg) + 4 + 10 * 4 + 4 + 2 * 8 and ctypes.sizeof(KpRewardCfgV2) == 13 * 4 + 4 + 8      # the C structs' layout
