#!/usr/bin/env python
"""UHC env-steps/s (CopycatAgent.sample: policy, step_ctrl's 15 substeps, reward, observation + running ZFilter) per controller variant, alternating
the variants in one process: uhc.yml (obs_v 1, 784-d, PolicyMCP), obs_v 2 with root velocities (571-d, PolicyMCP), obs_v 0 (220-d, PolicyGaussian), and
uhc.yml with meta_pd (105-d action: the extended controller, which runs on the full layout, and PolicyMCP's torch path past kp_mcp_tail's 80 columns).
The variant files are tests/golden/uhc_variants/*.yml.  Standing clips with seeded sinusoids (scripts/train_uhc.py's expert); prints one JSON line per block.

    python tools/uhc_variants_bench.py [envs] [steps per block] [blocks]        default 4096 32 3
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kinpoly_amd.nets import enable_tuned_gemms  # noqa: E402
from kinpoly_amd.uhc_config import UhcConfig  # noqa: E402
from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent  # noqa: E402

VARIANTS = {"uhc.yml": None, "obs_v2_root": "uhc_v2_root", "obs_v0_gauss": "uhc_v0_gauss", "meta_pd": "uhc_meta_pd"}


def setup(n, name, clips):
    cfg = None if name is None else UhcConfig(os.path.join(ROOT, "tests", "golden", "uhc_variants", name + ".yml"))
    env = BatchedHumanoidEnv(n, 0, seed=1, cfg=cfg)
    env.load_expert(clips)
    return env, CopycatAgent(env)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch.cuda.set_device(0)
    enable_tuned_gemms()
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    rng = np.random.default_rng(1)
    T = 64
    clips = np.tile(std["qpos"], (n, T, 1))
    amp, freq, ph = rng.uniform(0, 0.15, (n, 1, 69)), rng.uniform(0.2, 1.0, (n, 1, 69)), rng.uniform(0, 2 * np.pi, (n, 1, 69))
    clips[:, :, 7:] += amp * (np.sin(2 * np.pi * freq * (np.arange(T)[None, :, None] / 30.0) + ph) - np.sin(ph))
    clips = torch.tensor(clips, dtype=torch.float32)
    runs = {k: setup(n, v, clips) for k, v in VARIANTS.items()}
    rates = {k: [] for k in runs}
    for k, (env, agent) in runs.items():              # warm-up: code objects, library picks for every shape of the timed window
        agent.sample(4)
    torch.cuda.synchronize()
    for b in range(blocks):
        for k, (env, agent) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S, A, R, M = agent.sample(steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert S.shape[2] == env.obs_dim and bool(torch.isfinite(R).all())
            rates[k].append(n * steps / dt)
            print(json.dumps({"block": b, "variant": k, "obs_dim": env.obs_dim, "envs": n, "steps": steps, "env_steps_per_s": round(n * steps / dt),
                              "ms_per_step": round(dt / steps * 1e3, 3)}), flush=True)
    print(json.dumps({"envs": n, "median_env_steps_per_s": {k: round(float(np.median(r))) for k, r in rates.items()}}), flush=True)


if __name__ == "__main__":
    main()
