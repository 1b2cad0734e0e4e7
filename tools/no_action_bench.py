#!/usr/bin/env python
"""Env-steps/s of the rollout (VectorSampler.sample: kinematic policy GEMMs, UHC GEMMs, physics, observation, reward, record) with and without the
action one-hot in the observation (use_action: true = 105-d, kin_poly.yml; false = 101-d, kin_poly_wo_action.yml), alternating the two in one process.

The 101-d shapes (the GRU input GEMM at K = 101, the action MLP's first layer at K = 1125) are not in kinpoly_amd/assets/tunableop_gfx950.csv: they
run on the library's heuristic picks.  Standing clips (bench.py's set-up) with a random-init policy of the matching width; prints one JSON line per block.

    python tools/no_action_bench.py [envs] [steps per block] [blocks]        default 4096 40 3
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context  # noqa: E402
from kinpoly_amd.nets import KinPolicy, enable_tuned_gemms  # noqa: E402
from kinpoly_amd.rollout import VectorSampler  # noqa: E402


def setup(n, use_action, std, seed=0):
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=seed, use_action=use_action)
    policy = KinPolicy(state_dim=env.obs_dim).to(env.device).float()
    g = torch.Generator().manual_seed(seed)
    env.load_context(standing_context(n, 100, std["qpos"], std["qvel"], env.sim, (torch.rand(n, generator=g) * 2 - 1) * np.pi))
    sampler = VectorSampler(env, policy)
    sampler.start()
    return env, sampler


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch.cuda.set_device(0)
    enable_tuned_gemms()
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    runs = {ua: setup(n, ua, std) for ua in (True, False)}
    with torch.no_grad():
        for ua, (env, sampler) in runs.items():          # warm-up: code objects, library picks for every shape of the timed window
            sampler.sample(8)
        torch.cuda.synchronize()
        rates = {True: [], False: []}
        for b in range(blocks):
            for ua, (env, sampler) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch = sampler.sample(steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert batch.states.shape[2] == env.obs_dim and bool(torch.isfinite(batch.rewards).all())
                rates[ua].append(n * steps / dt)
                print(json.dumps({"block": b, "use_action": ua, "obs_dim": env.obs_dim, "envs": n, "steps": steps, "env_steps_per_s": round(n * steps / dt),
                                  "ms_per_step": round(dt / steps * 1e3, 3)}), flush=True)
    print(json.dumps({"envs": n, "median_env_steps_per_s": {("use_action" if ua else "no_action"): round(float(np.median(r))) for ua, r in rates.items()}}), flush=True)


if __name__ == "__main__":
    main()
