#!/usr/bin/env python
"""Pin the PPO update paths that no reference fixture reaches: `PPOTrainer.update_joint`, `PPOTrainer.update` with a trained controller
(`update_controller`, train_uhc=True and the single evaluation of train_uhc=False) and `CopycatAgent.optimize_policy`.  The fixtures hold what a
build computed for seeded inputs; they were recorded on the commit before these paths were folded onto shared epoch steps (kinpoly_amd/ppo.py), so
that the folded code is held to the numbers of the four separate loops.  Running the tool again pins whatever the current build computes.

    python tools/make_golden_ppo_parent.py [--out FILE]              CPU, fp64, one torch thread -> tests/golden/ppo_parent_fp64.npz
    python tools/make_golden_ppo_parent.py --device [--out FILE]     MI355X, fp32 (fused GRU re-unroll, k_gae, HIP FK) plus two CopycatAgent.sample(8)
                                                                     calls at 64 envs -> tests/golden/ppo_parent_fp32_bits.npz (uint32 views)

tests/test_ppo_parent_cpu.py and tests/test_gpu_ppo_parent.py replay `update_cases` / `sample_cases` and compare key by key.  The device fixture was
recorded three times in fresh processes on that earlier commit; the three files agreed word for word, so the GPU test asserts bit equality.

Cases (batch of tests/golden/update_params.npz, 8 envs x 12 rows; 3 epochs per call, two calls, so Adam state and the consumed clip are in the loop):
    joint, joint_alt0, joint_alt1   update_joint with grad_alternate False, and True at epoch 0 (supervised steps) and 1 (surrogate steps)
    cc_train, cc_eval               update() with cc_policy = PolicyGaussian(16, 4, (32, 16)), seeded cc_state / cc_action and an `exps` mask with zeros
    uhc_fix, uhc_std                optimize_policy on seeded (S, A, R, M) fed in place of sample(); uhc_std has fix_std=False (log_std gets a gradient)
Per call: every epoch's surrogate, value and step loss, adv, ret, every clip norm reported, and the first SLICE entries of every parameter.
The losses are taken where the code computes them (the module-level functions are wrapped for the duration of a case), not recomputed.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLD = os.path.join(ROOT, "tests", "golden")
SLICE, EPOCHS, SUP_LR = 32, 3, 1e-5
UHC_CASES = {"uhc_fix": True, "uhc_std": False}


class Recorder:
    """what the update computed on its way, taken at the functions it calls: (adv, ret), every surrogate, every step loss, every clip norm, and the
    value net's grad-enabled forwards (the regression steps; the GAE forwards run under no_grad)"""
    NAMES = ("estimate_advantages", "ppo_surrogate", "compute_loss_lite")

    def __init__(self, value):
        self.value, self.got, self.undo = value, {k: [] for k in self.NAMES + ("clip", "v")}, []

    def _wrap(self, owner, name, key):
        f = getattr(owner, name)

        def g(*a, **k):
            out = f(*a, **k)
            self.got[key].append(out)
            return out
        setattr(owner, name, g)
        self.undo.append((owner, name, f))

    def __enter__(self):
        import kinpoly_amd.supervised  # noqa: F401  (update_joint reads compute_loss_lite from it)
        for name in self.NAMES:
            for k, m in list(sys.modules.items()):
                if k.startswith("kinpoly_amd.") and name in getattr(m, "__dict__", {}):
                    self._wrap(m, name, name)
        self._wrap(torch.nn.utils, "clip_grad_norm_", "clip")
        self.hook = self.value.register_forward_hook(lambda m, i, o: self.got["v"].append(o.detach()) if torch.is_grad_enabled() else None)
        return self

    def __exit__(self, *exc):
        self.hook.remove()
        for owner, name, f in reversed(self.undo):
            setattr(owner, name, f)

    def arrays(self):
        f64 = lambda ts: np.array([float(t.detach()) for t in ts], np.float64)  # noqa: E731
        adv, ret = self.got["estimate_advantages"][0]
        return dict(adv=adv.reshape(-1).cpu().numpy(), ret=ret.reshape(-1).cpu().numpy(), surr=f64(self.got["ppo_surrogate"]),
                    vloss=f64([(v - ret.reshape(-1, 1)).pow(2).mean() for v in self.got["v"]]), step=f64([x[0] for x in self.got["compute_loss_lite"]]),
                    clip=f64(self.got["clip"]))


def seed_module(mod, seed, scale=0.1):
    """parameters from a numpy stream (not torch's initialisers), in the module's own dtype and device"""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k != "action_log_std":
                p.copy_(torch.tensor(rng.normal(size=tuple(p.shape)) * scale, dtype=p.dtype))
    return mod


def params_of(groups, before=None):
    """{kind:name -> first SLICE entries}, and per tensor how far it moved from `before` (max |change| over the whole tensor)"""
    full = {f"{kind}:{k}": v.detach().reshape(-1).cpu().numpy().copy() for kind, mod in groups.items() for k, v in mod.named_parameters()}
    moved = None if before is None else np.array([np.abs(full[k].astype(np.float64) - before[k].astype(np.float64)).max() for k in full])
    return full, moved


def _store(out, tag, rec, groups, before):
    for k, v in rec.arrays().items():
        out[f"{tag}_{k}"] = v
    full, moved = params_of(groups, before)
    out[f"{tag}_moved"] = moved
    for k, v in full.items():
        out[f"{tag}_{k}"] = v[:SLICE]
    return full


def joint_case(g, out, name, alternate, epoch, device, dtype, fk_sim):
    from test_update_cpu import batch_of, build
    net, val, upd = build(g, dtype=dtype, device=device)
    if fk_sim is not None:                     # the HIP FK kernels, as AgentAR wires them
        from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
        from kinpoly_amd.supervised import TorchFK
        kpm = read_kpm(DEFAULT_KPM)
        upd.fk = TorchFK(kpm["body_pos"], kpm["body_parent"], torch.device(device), dtype=dtype, sim=fk_sim)
    tr = upd.trainer
    tr.num_optim_epoch = EPOCHS
    for gr in upd.opt_sup.param_groups:        # grad_alternate's supervised steps at the fixture's 5e-4 carry the means 1e2 sigma away within a call and the surrogate
        gr["lr"] = SUP_LR                      # (reported, never stepped on, in those epochs) to 1e96, where no tolerance means anything; at 1e-5 it stays O(1)
    groups = {"p": net, "v": val}
    before, _ = params_of(groups)
    for call in range(2):
        upd.per_epoch_update()
        with Recorder(val) as rec:
            stats = tr.update_joint(batch_of(g, call, device, dtype), upd.fk, alternate, epoch, upd.opt_sup)
        tag = f"{name}_c{call}"
        out[tag + "_stats"] = np.array([stats["value_loss"], stats["surr_loss"], stats["step_loss"]], np.float64)
        before = _store(out, tag, rec, groups, before)


def controller_batch(g, call, device, dtype):
    from test_update_cpu import batch_of
    rng = np.random.default_rng(500 + call)
    N, T = int(g["N"]), int(g["T"])
    b = batch_of(g, call, device, dtype)
    b.cc_state = torch.tensor(rng.normal(size=(N, T, 16)), dtype=dtype, device=device)
    b.cc_action = torch.tensor(rng.normal(size=(N, T, 4)) * 0.3, dtype=dtype, device=device)
    exps = np.ones((N, T)); exps[rng.random((N, T)) < 0.25] = 0
    assert 0 < exps.sum() < N * T
    b.exps = torch.tensor(exps, dtype=dtype, device=device)
    return b


def controller_case(g, out, name, train_uhc, device, dtype):
    from test_update_cpu import build
    from kinpoly_amd.nets import PolicyGaussian
    net, val, upd = build(g, dtype=dtype, device=device)
    cc = seed_module(PolicyGaussian(16, 4, (32, 16)).to(dtype).to(device), 41)
    tr = type(upd.trainer)(net, val, policy_lr=float(g["policy_lr"]), value_lr=float(g["value_lr"]), num_optim_epoch=EPOCHS, cc_policy=cc, train_uhc=train_uhc)
    groups = {"p": net, "v": val, "cc": cc}
    before, _ = params_of(groups)
    for call in range(2 if train_uhc else 1):
        tr.per_epoch_update()
        with Recorder(val) as rec:
            stats = tr.update(controller_batch(g, call, device, dtype))
        tag = f"{name}_c{call}"
        out[tag + "_stats"] = np.array([stats["value_loss"], stats["surr_loss"], stats["cc_surr_loss"]], np.float64)
        before = _store(out, tag, rec, groups, before)


def uhc_case(out, name, fix_std, device, dtype):
    from kinpoly_amd.nets import MLP, PolicyGaussian, Value
    from kinpoly_amd.uhc_env import CopycatAgent
    a = CopycatAgent.__new__(CopycatAgent)          # the update alone: no env; sample() is replaced by the seeded tensors
    a.policy = seed_module(PolicyGaussian(16, 4, (32, 16), log_std=-1.0, fix_std=fix_std).to(dtype).to(device), 61)
    a.value = seed_module(Value(MLP(16, (32,), "relu")).to(dtype).to(device), 62)
    a.group, a.gamma, a.tau, a.clip_epsilon, a.num_optim_epoch = None, 0.95, 0.95, 0.2, EPOCHS
    a.opt_p = torch.optim.Adam([p for p in a.policy.parameters() if p.requires_grad], lr=1e-3)
    a.opt_v = torch.optim.Adam(a.value.parameters(), lr=1e-3)
    if not hasattr(sys.modules.get("kinpoly_amd.ppo"), "PPOTrainer"):      # a commit on which the agent's constructor parks the update's functions on the instance
        from kinpoly_amd import rollout as R
        park = lambda: a.__dict__.update(_ar=R._allreduce_grads, _ea=R.estimate_advantages, _surr=R.ppo_surrogate)  # noqa: E731
    else:
        park = lambda: None  # noqa: E731
    groups = {"p": a.policy, "v": a.value}
    before, _ = params_of(groups)
    for call in range(2):
        rng = np.random.default_rng(700 + call)
        t = lambda x: torch.tensor(x, dtype=dtype, device=device)  # noqa: E731
        masks = np.ones((8, 12)); masks[rng.random((8, 12)) < 0.1] = 0
        a.sample = lambda horizon, b=(t(rng.normal(size=(8, 12, 16))), t(rng.normal(size=(8, 12, 4)) * 0.5), t(rng.random((8, 12))), t(masks)): b
        with Recorder(a.value) as rec:
            park()
            stats = a.optimize_policy(12)
        tag = f"{name}_c{call}"
        out[tag + "_stats"] = np.array([stats["value_loss"], stats["surr_loss"], stats["avg_reward"], stats["fail_rate"]], np.float64)
        before = _store(out, tag, rec, groups, before)


def update_cases(device="cpu", dtype=torch.float64):
    """every update case on `device`; CPU runs under one torch thread (summation order), restored afterwards"""
    g = np.load(os.path.join(GOLD, "update_params.npz"), allow_pickle=False)
    out, fk_sim = {}, None
    if device != "cpu":
        from kinpoly_amd import sim as kpsim
        fk_sim = kpsim.KpSim(kpsim.KpModel(), int(g["N"]) * int(g["T"]), 0)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        joint_case(g, out, "joint", False, 0, device, dtype, fk_sim)
        joint_case(g, out, "joint_alt0", True, 0, device, dtype, fk_sim)
        joint_case(g, out, "joint_alt1", True, 1, device, dtype, fk_sim)
        controller_case(g, out, "cc_train", True, device, dtype)
        controller_case(g, out, "cc_eval", False, device, dtype)
        for name, fix_std in UHC_CASES.items():
            uhc_case(out, name, fix_std, device, dtype)
    finally:
        torch.set_num_threads(threads)
    return out


def thin(x):
    """every fourth env of a sampled tensor (and every fourth column of the 784-wide states): what the fixture keeps next to the whole tensor's SHA-256"""
    x = x.cpu().numpy()[::4]
    return np.ascontiguousarray(x[..., ::4] if x.ndim == 3 and x.shape[-1] > 100 else x)


def sample_cases():
    """CopycatAgent.sample(8) at 64 envs: on one rectangular clip (load_expert) and on the takes library of tests/golden/uhc_takes_small.pkl"""
    from kinpoly_amd.dataset import AmassSingleDataset
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent
    out = {}
    std = np.load(os.path.join(GOLD, "standing_neutral.npz"))
    pkl = os.path.join(GOLD, "uhc_takes_small.pkl")
    for name in ("expert", "takes"):
        torch.manual_seed(0)
        if name == "expert":
            env = BatchedHumanoidEnv(64, 0, env_init_noise=0.01)
            env.load_expert(torch.tensor(np.tile(std["qpos"], (64, 20, 1)), dtype=torch.float32))
            agent = CopycatAgent(env, num_optim_epoch=1)
        else:
            env = BatchedHumanoidEnv(64, 0, seed=1, env_episode_len=6)       # every env finishes an episode inside the 8 steps
            agent = CopycatAgent(env, num_optim_epoch=1, dataset=AmassSingleDataset({"file_path": pkl, "test_file_path": pkl, "t_min": 90}, "train"), seed=17)
        for k, x in zip("SARM", agent.sample(8)):
            out[f"sample_{name}_{k}"] = thin(x)
            out[f"sample_{name}_{k}_sha"] = np.frombuffer(hashlib.sha256(x.contiguous().cpu().numpy().tobytes()).digest(), np.uint8).copy()
        if name == "takes":
            out["sample_takes_log"] = np.array(agent.take_log[-1], np.float64).reshape(-1, 3)
            assert len(out["sample_takes_log"]) >= 64
    return out


def main():
    device = "--device" in sys.argv
    out = os.path.join(GOLD, "ppo_parent_fp32_bits.npz" if device else "ppo_parent_fp64.npz")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    if device:
        g = update_cases("cuda", torch.float32)
        g.update(sample_cases())
        g = {k: (v.view(np.uint32) if v.dtype == np.float32 else v) for k, v in g.items()}
    else:
        g = update_cases()
    np.savez_compressed(out, **g)
    print(out, os.path.getsize(out), len(g), "arrays")


if __name__ == "__main__":
    main()
