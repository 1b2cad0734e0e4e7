#!/usr/bin/env python
"""Env-steps/s of the rollout (VectorSampler.sample: kinematic policy GEMMs, UHC GEMMs, physics, observation, reward, record) for the 105-d observation of
kin_poly.yml and for each use_vel / use_head variant (kinpoly_amd.sim.ar_obs_dim: 180, 176, 85, 160 -- and, with --all, 101 and 81, 156, the two widths Config
refuses), alternating them in one process.  The yardstick is the 105-d figure of the same run.

The variants' GEMM shapes (the GRU input GEMM at K = state_dim, the action MLP's first layer at K = 1024 + state_dim, the value net's first layer) are not
in kinpoly_amd/assets/tunableop_gfx950.csv: they run on the library's heuristic picks.  Standing clips (bench.py's set-up) with a random-init policy of
the matching width; prints one JSON line per block and a final line with the median of the blocks per variant.

    python tools/obs_variants_bench.py [envs] [steps per block] [blocks] [--all]        default 4096 40 3
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

# (use_vel, use_head, use_action): 105 first (the yardstick), then the variants a yml can ask for
VARIANTS = [(False, True, True), (True, True, True), (True, True, False), (False, False, True), (True, False, True)]
KERNEL_ONLY = [(False, False, False), (True, False, False)]
NO_ACTION = (False, True, False)        # 101: kin_poly_wo_action.yml (tools/no_action_bench.py measures it end to end)


def setup(n, s, std, seed=0):
    env = BatchedHumanoidAREnv(n, 0, mode="train", seed=seed, use_vel=s[0], use_head=s[1], use_action=s[2])
    policy = KinPolicy(state_dim=env.obs_dim).to(env.device).float()
    g = torch.Generator().manual_seed(seed)
    env.load_context(standing_context(n, 100, std["qpos"], std["qvel"], env.sim, (torch.rand(n, generator=g) * 2 - 1) * np.pi))
    sampler = VectorSampler(env, policy)
    sampler.start()
    return env, sampler


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 4096
    steps = int(args[1]) if len(args) > 1 else 40
    blocks = int(args[2]) if len(args) > 2 else 3
    variants = VARIANTS + ([NO_ACTION] + KERNEL_ONLY if "--all" in sys.argv else [])
    torch.cuda.set_device(0)
    enable_tuned_gemms()
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    runs = {s: setup(n, s, std) for s in variants}
    with torch.no_grad():
        for s, (env, sampler) in runs.items():          # warm-up: code objects, library picks for every shape of the timed window
            sampler.sample(8)
        torch.cuda.synchronize()
        rates = {s: [] for s in variants}
        for b in range(blocks):
            for s, (env, sampler) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch = sampler.sample(steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert batch.states.shape[2] == env.obs_dim and bool(torch.isfinite(batch.rewards).all())
                rates[s].append(n * steps / dt)
                print(json.dumps({"block": b, "use_vel": s[0], "use_head": s[1], "use_action": s[2], "obs_dim": env.obs_dim, "envs": n, "steps": steps,
                                  "env_steps_per_s": round(n * steps / dt), "ms_per_step": round(dt / steps * 1e3, 3)}), flush=True)
    print(json.dumps({"envs": n, "median_env_steps_per_s": {str(runs[s][0].obs_dim): round(float(np.median(r))) for s, r in rates.items()}}), flush=True)


if __name__ == "__main__":
    main()
