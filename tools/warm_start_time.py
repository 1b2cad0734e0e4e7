#!/usr/bin/env python
"""Time of AgentAR.train_init's two phases at kin_poly.yml's sizes (num_sample 2000, batch_size 256, fr_num 100) on the synthetic feature set:
seconds per epoch of update_init_supervised (x 500 in the reference) and of train_full_supervised (x 50).   python tools/warm_start_time.py [epochs]

    python tools/warm_start_time.py --fused [--unfused_only]

compares train_full_supervised on the torch path and on the taped HIP roll-out (fused=True) in ONE process, alternating: one warm-up epoch each, then
three repeats of three epochs; prints each path's median and min .. max seconds per epoch.  The taped path counts as faster when its median is below
the torch path's median by more than the torch path's own max - min.  --context: the same comparison at kin_only.yml's sizes -- the kinematic model
with a context block and the synthetic 512-wide `of` features (rnn_hdim 256, state 357, kinpoly_amd.exp_arnet.build_net), 256 clips x 100 frames.  --unfused_only: the torch path alone, same protocol; to time a commit that lacks this flag, copy this file into that checkout's tools/ and run it there."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup():
    from kinpoly_amd import dataset as D
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.model_compiler import read_kpm
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    fk_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), 256, 0)
    takes = D.synthetic_takes(fk_sim, std["qpos"], n_per_action=4, T_range=(110, 160), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=4)
    ds = D.StateARDataset(takes, fr_num=100, seed=4, device=fk_sim.device)
    return AgentAR(256, dataset=ds, device=0, horizon=4), ds


def _setup_context(of_dim=512):
    """kin_only.yml: use_context + use_of, model_specs.rnn_hdim 256, cnn_fdim 512; the network of scripts/exp_arnet_all.py (as_policy=False: 357-d state)"""
    from types import SimpleNamespace
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.supervised import TorchFK
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    net = E.build_net(use_context=True, of_dim=of_dim, rnn_hdim=256).cuda()
    fk_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM, **E.model_options(net)), 256, 0)
    takes = D.synthetic_takes(fk_sim, std["qpos"], n_per_action=4, T_range=(110, 160), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=4)
    ds = D.StateARDataset(takes, fr_num=100, seed=4, device=fk_sim.device, of_features=D.synthetic_of_features(takes, of_dim, seed=4))
    kpm = read_kpm(DEFAULT_KPM)
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], fk_sim.device, sim=fk_sim)
    print(f"context model: state {net.state_dim}, context {net.context_dim}, rnn_hdim {net.rnn_hdim}, of {of_dim} (synthetic)", flush=True)
    return SimpleNamespace(policy_net=net, opt_sup=torch.optim.Adam(net.parameters(), lr=1e-4), fk=fk), ds


def compare(paths, epochs=3, repeats=3, context=False):
    """paths: names out of ("torch", "fused")"""
    from kinpoly_amd import pretrain as P
    agent, ds = _setup_context() if context else _setup()
    run = lambda name, n: P.train_full_supervised(agent.policy_net, agent.opt_sup, agent.fk, ds, n, 0.3, 2000, 256, noise_std=0.01,      # noqa: E731
                                                  rng=np.random.RandomState(0), **({"fused": True} if name == "fused" else {}))
    times = {p: [] for p in paths}
    for p in paths:
        run(p, 1)
    for _ in range(repeats):
        for p in paths:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loss = run(p, epochs)
            torch.cuda.synchronize(); times[p].append((time.perf_counter() - t0) / epochs)
            print(f"  {p}: {times[p][-1]:.3f} s per epoch (loss {loss:.4f})", flush=True)
    for p in paths:
        t = np.array(times[p])
        print(f"train_full_supervised [{p}]: median {np.median(t):.3f} s per epoch, min .. max {t.min():.3f} .. {t.max():.3f} ({repeats} x {epochs} epochs of 8 batches of 256 clips x 100 frames)", flush=True)
    if len(paths) == 2:
        a, b = np.array(times["torch"]), np.array(times["fused"])
        faster = np.median(b) < np.median(a) - (a.max() - a.min())
        print(f"taped path faster by the rule (median below the torch median by more than its max - min): {bool(faster)}; ratio of medians {np.median(a) / np.median(b):.2f}", flush=True)


def main():
    if "--fused" in sys.argv or "--unfused_only" in sys.argv:
        return compare(("torch",) if "--unfused_only" in sys.argv else ("torch", "fused"), context="--context" in sys.argv)
    from kinpoly_amd import pretrain as P
    ep = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    agent, ds = _setup()
    for name, fn in (("update_init_supervised", lambda n: P.update_init_supervised(agent.policy_net, agent.opt_sup, agent.fk, ds, n, 2000, 256)),
                     ("train_full_supervised", lambda n: P.train_full_supervised(agent.policy_net, agent.opt_sup, agent.fk, ds, n, 0.3, 2000, 256, noise_std=0.01))):
        first = fn(1)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        last = fn(ep)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / ep
        print(f"{name}: {dt:.2f} s per epoch (8 batches of 256 clips x 100 frames); loss after 1 epoch {first:.4f}, after {ep + 1} epochs {last:.4f}", flush=True)


if __name__ == "__main__":
    main()
