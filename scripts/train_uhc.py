#!/usr/bin/env python
"""Counterpart of the reference's scripts/train_uhc.py on the batched MI355X engine: PPO training of the UHC (PolicyMCP) on
the imitation env.  The AMASS clips of the reference are not part of its repository, so the expert is the standing clip of
`sample_data/standing_neutral.pkl` (tests/golden/standing_neutral.npz) with small seeded joint-space sinusoids.

    python scripts/train_uhc.py --num_envs 4096 --iters 3
    python scripts/train_uhc.py --cfg uhc --config_root /path/to/KinPoly       (or --cfg path/to/controller.yml)

With --cfg the controller follows the file (kinpoly_amd/uhc_config.py: observation variant, actor, PPO constants, reward weights, termination);
without it the env and agent are uhc.yml's, as before.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 scripts/train_uhc.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def save_uhc_checkpoint(path, agent, env):
    from kinpoly_amd import checkpoint as ck
    import pickle
    rs = ck.ZFilter((env.obs_dim,), clip=agent.running_state.clip); rs.rs._n = agent.running_state.count
    rs.rs._M = agent.running_state._mean64.cpu().numpy(); rs.rs._S = agent.running_state._m2.cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with ck._RefModulePath(), open(path, "wb") as f:
        pickle.dump({"policy_dict": {k: v.cpu() for k, v in agent.policy.state_dict().items()},
                     "value_dict": {k: v.cpu() for k, v in agent.value.state_dict().items()}, "running_state": rs}, f)


def train_on_takes(args, rank, local, world):
    """--data: the reference's training loop on a take library (agent_copycat.py): freq_dict.pt is read from / written next to the checkpoint"""
    from kinpoly_amd.dataset import AmassSingleDataset, SmplObjDataset
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent
    Dataset = {"amass_single": AmassSingleDataset, "smpl_obj": SmplObjDataset}[args.dataset]
    cfg = None
    if args.cfg:
        from kinpoly_amd.uhc_config import UhcConfig
        cfg = UhcConfig(args.cfg, config_root=args.config_root)
    specs = {**(cfg.data_specs if cfg is not None else {}), "file_path": args.data, "test_file_path": args.test_data or args.data}
    if args.t_min is not None:
        specs["t_min"] = args.t_min
    elif cfg is None:
        specs.setdefault("t_min", 90)
    ds = Dataset(specs, "train")
    out_dir = os.path.dirname(os.path.abspath(args.save)) if args.save else None
    env = BatchedHumanoidEnv(args.num_envs, local, seed=1 + rank, cfg=cfg) if cfg is not None else BatchedHumanoidEnv(args.num_envs, local, env_init_noise=0.0, seed=1 + rank)
    group = dist.group.WORLD if world > 1 else None
    kw = {**(cfg.ppo_kwargs() if cfg is not None else {}), "num_optim_epoch": args.num_optim_epoch}
    from kinpoly_amd.push import schedule_from_args
    agent = CopycatAgent(env, group=group, dataset=ds, seed=1, output_dir=out_dir, push_schedule=schedule_from_args(args, args.num_envs, env.device), **kw)
    if world > 1:
        for p in list(agent.policy.parameters()) + list(agent.value.parameters()):
            dist.broadcast(p.data, 0)
    for it in range(args.iters):
        stats = agent.optimize_policy(args.horizon)
        if rank == 0:
            print(json.dumps({"iter": it, "episodes": len(agent.take_log[-1]), **{k: (round(v, 5) if isinstance(v, float) else v) for k, v in stats.items()}}), flush=True)
    if args.test_data and rank == 0:
        print(agent.eval_policy("test", args.iters, dataset=Dataset(specs, "test")), flush=True)
    if args.save and rank == 0:
        save_uhc_checkpoint(args.save, agent, env)
        agent.save_freq_dict(out_dir)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--clip_len", type=int, default=64)
    ap.add_argument("--num_optim_epoch", type=int, default=10)
    ap.add_argument("--save", type=str, default="")
    ap.add_argument("--cfg", type=str, default="", help="UHC config id (config/**/<id>.yml under --config_root) or a .yml path")
    ap.add_argument("--config_root", type=str, default=None)
    ap.add_argument("--data", type=str, default="", help="take pickle of the reference's UHC data ({take: {pose_aa, qpos, ...}}): train on its takes, a newly drawn whole take per episode")
    ap.add_argument("--test_data", type=str, default="", help="take pickle evaluated (eval_policy, mode 'test') after the last iteration")
    ap.add_argument("--t_min", type=int, default=None, help="shortest take kept (default: the config's data_specs, else 90)")
    ap.add_argument("--dataset", choices=("amass_single", "smpl_obj"), default="amass_single",
                    help="the loader of --data / --test_data: amass_single (DatasetAMASSSingle's pickle) or smpl_obj (DatasetSMPLObj's: takes that carry objects)")
    from kinpoly_amd.push import add_push_arguments
    return add_push_arguments(ap)      # --push_impulse LO [HI] and friends: train under perturbation pushes (off by default)


def main(argv=None):
    args = build_parser().parse_args(argv)
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd.push import schedule_from_args
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    rng = np.random.default_rng(1 + rank)
    n, T = args.num_envs, args.clip_len
    clips = np.tile(std["qpos"], (n, T, 1))
    amp, freq, ph = rng.uniform(0, 0.15, (n, 1, 69)), rng.uniform(0.2, 1.0, (n, 1, 69)), rng.uniform(0, 2 * np.pi, (n, 1, 69))
    tt = np.arange(T)[None, :, None] / 30.0
    clips[:, :, 7:] += amp * (np.sin(2 * np.pi * freq * tt + ph) - np.sin(ph))
    torch.manual_seed(1 + rank)
    if args.data:
        return train_on_takes(args, rank, local, world)
    if args.cfg:
        from kinpoly_amd.uhc_config import UhcConfig
        cfg = UhcConfig(args.cfg, config_root=args.config_root)
        env = BatchedHumanoidEnv(n, local, seed=1 + rank, cfg=cfg)
        env.load_expert(torch.tensor(clips, dtype=torch.float32))
        agent = CopycatAgent(env, **{**cfg.ppo_kwargs(), "num_optim_epoch": args.num_optim_epoch}, push_schedule=schedule_from_args(args, n, env.device))
    else:
        env = BatchedHumanoidEnv(n, local, env_init_noise=0.0, seed=1 + rank)
        env.load_expert(torch.tensor(clips, dtype=torch.float32))
        agent = CopycatAgent(env, num_optim_epoch=args.num_optim_epoch, push_schedule=schedule_from_args(args, n, env.device))
    if world > 1:
        for p in list(agent.policy.parameters()) + list(agent.value.parameters()):
            dist.broadcast(p.data, 0)
    for it in range(args.iters):
        stats = agent.optimize_policy(args.horizon)
        if rank == 0:
            print(json.dumps({"iter": it, **{k: (round(v, 5) if isinstance(v, float) else v) for k, v in stats.items()}}), flush=True)
    if args.save and rank == 0:
        rs = ck.ZFilter((env.obs_dim,), clip=agent.running_state.clip); rs.rs._n = agent.running_state.count      # the clip the controller was trained under (uhc.yml: 5)
        rs.rs._M = agent.running_state._mean64.cpu().numpy(); rs.rs._S = agent.running_state._m2.cpu().numpy()
        import pickle
        with ck._RefModulePath(), open(args.save, "wb") as f:
            pickle.dump({"policy_dict": {k: v.cpu() for k, v in agent.policy.state_dict().items()},
                         "value_dict": {k: v.cpu() for k, v in agent.value.state_dict().items()}, "running_state": rs}, f)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


if __name__ == "__main__":
    main()
