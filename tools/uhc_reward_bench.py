#!/usr/bin/env python
"""The fused tracking launch of the UHC env, per reward function: microseconds per launch of kp_sim_uhc_track (world_rfc_implicit) and of
kp_sim_uhc_track_r with every id of the reward registry, at --num_envs envs on the mixed-length takes of tests/golden/uhc_takes_small.pkl.  Each figure
is the device time between two events around --launches back-to-back launches, divided by their number, the median of --blocks such blocks after a
warm-up block; prints one JSON line.

    python tools/uhc_reward_bench.py --num_envs 4096
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.dataset import AmassSingleDataset
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv
    pkl = os.path.join(ROOT, "tests", "golden", "uhc_takes_small.pkl")
    ds = AmassSingleDataset({"file_path": pkl, "t_min": 90}, "train")
    n, res = args.num_envs, {}
    a = torch.zeros((n, 75), device="cuda")
    lib = None
    for rid in kpsim.UHC_REWARD_IDS:
        env = BatchedHumanoidEnv(n, 0, seed=1, reward_id=rid)
        lib = ds.to_library(env.sim)
        env.load_takes(lib)
        env.reset()
        env.step(a)                                          # a state after a control step, prev_qpos recorded
        f = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=env.device)      # noqa: E731
        o = [f(n), f(n, env.info_dim), f(n), f(n, dt=torch.uint8), f(n, dt=torch.uint8), f(n, dt=torch.uint8), f(n)]
        track, tc = (env.sim.uhc_track, env._tc) if env._tcr is None else (env.sim.uhc_track_r, env._tcr)
        us = []
        for b in range(args.blocks + 1):
            env.cur_t.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                track(env.takes, env._st, tc, a, *o)
            e1.record(); torch.cuda.synchronize()
            if b:
                us.append(e0.elapsed_time(e1) * 1e3 / args.launches)
        res[rid] = {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us))}
        del env
    print(json.dumps({"metric": "fused tracking launch, us per launch (back-to-back, events)", "num_envs": n, "launches": args.launches, "blocks": args.blocks, **res}))


if __name__ == "__main__":
    main()
