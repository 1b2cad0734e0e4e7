#!/usr/bin/env python
"""CopycatAgent.sample on uhc.yml's env at --num_envs envs: env-steps/s of the rectangular torch path (load_expert), of the take-library path
with equal-length takes, and of the library path with the mixed lengths of tests/golden/uhc_takes_small.pkl.  Medians of --blocks timed
blocks of --horizon steps after one warm-up block; prints one JSON line.

    python tools/uhc_takes_bench.py --num_envs 4096

--objects: the takes of tests/golden/uhc_obj_takes_small.pkl instead, three configurations in one process with their blocks alternating: the library with
objects (the fused reset, k_uhc_assign_obj), the same qpos as a library without objects with the objects placed from Python before every reset (the
composed reset: a gather of the rows, kp_sim_set_objects, kp_sim_uhc_assign), and that library alone on the floor as the scale.  --warmup steps first,
then --blocks blocks of --horizon steps each; per configuration the median and min .. max of the blocks.  Pass rule: the fused median is at least the
composed median minus the composed run's own max - min.

    python tools/uhc_takes_bench.py --objects --num_envs 4096 --warmup 8 --blocks 3 --horizon 40
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


def objects_bench(args):
    from kinpoly_amd.dataset import SmplObjDataset
    from kinpoly_amd.sim import KpTakes
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent

    class ComposedEnv(BatchedHumanoidEnv):
        """places the objects with today's calls before every reset of a library without objects"""
        def _reset_takes(self, env_mask, take_ids, start):
            dev = self.device
            first = take_ids is None and self._next_ids is not None
            ids = self._next_ids if first else take_ids
            k = self.take_id.long() if ids is None else torch.as_tensor(np.asarray(ids, np.int64), device=dev)
            st = self.start_ind.long() if ids is None else torch.zeros_like(k) if start is None else torch.as_tensor(np.asarray(start, np.int64), device=dev)
            row = self._off[k] + torch.minimum(st, self._take_len.long()[k] - 1)
            m8 = None if env_mask is None or first else env_mask.to(dev, torch.uint8).contiguous()
            self.sim.set_objects(self._obj_tab[row].contiguous(), m8)
            return super()._reset_takes(env_mask, take_ids, start)

    class PlainLibrary(SmplObjDataset):
        def to_library(self, sim, dt=None):
            off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
            return KpTakes(sim, np.concatenate([self.qpos[k] for k in self.data_keys], 0).astype(np.float32), off, sim.model.get_option("timestep") * 15 if dt is None else dt)

    pkl = os.path.join(ROOT, "tests", "golden", "uhc_obj_takes_small.pkl")
    n = args.num_envs
    agents = {}
    for name, cls, ds in (("fused", BatchedHumanoidEnv, SmplObjDataset({"file_path": pkl}, "train")), ("composed", ComposedEnv, PlainLibrary({"file_path": pkl}, "train")),
                          ("floor_only", BatchedHumanoidEnv, PlainLibrary({"file_path": pkl}, "train"))):
        torch.manual_seed(0)
        env = cls(n, 0, seed=1)
        if cls is ComposedEnv:
            full = SmplObjDataset({"file_path": pkl}, "train")
            env._obj_tab = torch.tensor(np.concatenate([full.obj_qpos[k] for k in full.data_keys], 0), dtype=torch.float32, device=env.device)
            env._off = torch.as_tensor(np.concatenate([[0], np.cumsum(full.lens)[:-1]]).astype(np.int64), device=env.device)
        agents[name] = CopycatAgent(env, dataset=ds, seed=1)
    for a in agents.values():
        a.sample(args.warmup); torch.cuda.synchronize()
    rates = {k: [] for k in agents}
    for _ in range(args.blocks):
        for name, a in agents.items():
            t0 = time.perf_counter(); a.sample(args.horizon); torch.cuda.synchronize()
            rates[name].append(n * args.horizon / (time.perf_counter() - t0))
    res = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in rates.items()}
    c = res["composed"]
    print(json.dumps({"metric": "CopycatAgent.sample env-steps/s, takes with objects", "num_envs": n, "horizon": args.horizon, "blocks": args.blocks, "warmup": args.warmup,
                      **res, "pass": bool(res["fused"]["median"] >= c["median"] - (c["max"] - c["min"]))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", action="store_true", help="the takes with objects: fused reset, composed reset and the floor-only library, alternating")
    ap.add_argument("--warmup", type=int, default=8, help="--objects: warm-up steps of every configuration")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--path", default="all", choices=("all", "torch", "equal", "mixed"), help="one path alone (for a kernel trace of it)")
    args = ap.parse_args()
    if args.objects:
        return objects_bench(args)
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
