#!/usr/bin/env python
"""CopycatAgent.sample on uhc.yml's env at --num_envs envs: env-steps/s of the rectangular torch path (load_expert), of the take-library path
with equal-length takes, and of the library path with the mixed lengths of tests/golden/uhc_takes_small.pkl.  Medians of --blocks timed
blocks of --horizon steps after one warm-up block; prints one JSON line.

    python tools/uhc_takes_bench.py --num_envs 4096
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(agent, horizon, blocks):
    agent.sample(horizon); torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter(); agent.sample(horizon); torch.cuda.synchronize()
        out.append(agent.env.n * horizon / (time.perf_counter() - t0))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--path", default="all", choices=("all", "torch", "equal", "mixed"), help="one path alone (for a kernel trace of it)")
    args = ap.parse_args()
    from kinpoly_amd.dataset import AmassSingleDataset
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent
    pkl = os.path.join(ROOT, "tests", "golden", "uhc_takes_small.pkl")
    mixed = AmassSingleDataset({"file_path": pkl, "t_min": 90}, "train")
    q = mixed.qpos["take_c_96"]
    equal = AmassSingleDataset({"file_path": pkl, "t_min": 90}, "train", takes={f"t{i}": {"pose_aa": np.zeros((96, 72)), "qpos": np.roll(q, 7 * i, 0)} for i in range(4)})
    n, res = args.num_envs, {}
    if args.path in ("all", "torch"):
        torch.manual_seed(0)
        env = BatchedHumanoidEnv(n, 0, seed=1)
        env.load_expert(torch.tensor(np.tile(q[None], (n, 1, 1)), dtype=torch.float32))
        res["torch_rectangular"] = timed(CopycatAgent(env), args.horizon, args.blocks)
        del env
    for name, ds in (("library_equal_lengths", equal), ("library_mixed_lengths", mixed)):
        if args.path not in ("all", name.split("_")[1]):
            continue
        torch.manual_seed(0)
        env = BatchedHumanoidEnv(n, 0, seed=1)
        res[name] = timed(CopycatAgent(env, dataset=ds, seed=1), args.horizon, args.blocks)
        del env
    print(json.dumps({"metric": "CopycatAgent.sample env-steps/s", "num_envs": n, "horizon": args.horizon, "blocks": args.blocks, **res}))


if __name__ == "__main__":
    main()
