#!/usr/bin/env python
"""Counterpart of the reference's scripts/eval_uhc.py (`--mode stats`: run_seq / test_coverage, :158-241) on the batched MI355X engine: every take of
a take pickle played whole by a trained UHC, env.n takes at a time; writes `<iter>_<data>_coverage.pkl` and `_coverage_full.pkl` next to the checkpoint.

    python scripts/eval_uhc.py --cfg uhc --config_root /path/to/KinPoly --iter 1000 --mode stats --data test --fail_safe
    python scripts/eval_uhc.py --mode stats --ckpt out/iter_0002.p --takes takes.pkl --iter 2 --data usr

--cfg names the controller's yml (its data_specs give test_file_path and t_min); --takes overrides the take file, --ckpt the checkpoint;
--dataset smpl_obj reads the take file as DatasetSMPLObj's (takes that carry objects: the objects are simulated and `pred` rows are 111 wide)
(default <config_root>/results/motion_im/<cfg>/models/iter_%04d.p).  The viewer modes of the reference (--mode vis / disp_stats, --record, --preview)
need its MuJoCo viewer and are refused by name; scripts/render_results.py turns the `_coverage_full.pkl` this writes into frames with the engine's own
ray-caster.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWER_MODES = ("vis", "disp_stats")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default=None)
    p.add_argument("--vis_model_file", default="humanoid_smpl_neutral_mesh_vis")
    p.add_argument("--iter", type=int, default=-1)
    p.add_argument("--focus", action="store_true", default=True)
    p.add_argument("--hide_expert", action="store_true", default=False)
    p.add_argument("--preview", action="store_true", default=False)
    p.add_argument("--azimuth", type=float, default=45)
    p.add_argument("--video_dir", default="out/videos/motion_im")
    p.add_argument("--mode", type=str, default="vis")
    p.add_argument("--input", action="store_true", default=False)
    p.add_argument("--num_threads", type=int, default=20)
    p.add_argument("--record", action="store_true", default=False)
    p.add_argument("--record_expert", action="store_true", default=False)
    p.add_argument("--data", type=str, default="usr")
    p.add_argument("--fail_safe", action="store_true", default=False)
    p.add_argument("--no_root", action="store_true", default=False)
    p.add_argument("--no_full", action="store_true", default=False)
    # this engine's additions
    p.add_argument("--config_root", type=str, default=None)
    p.add_argument("--ckpt", type=str, default="")
    p.add_argument("--takes", type=str, default="")
    p.add_argument("--t_min", type=int, default=None)
    p.add_argument("--num_envs", type=int, default=64)
    p.add_argument("--dataset", choices=("amass_single", "smpl_obj"), default="amass_single",
                   help="the loader of the take file: amass_single (DatasetAMASSSingle's pickle) or smpl_obj (DatasetSMPLObj's: takes that carry objects)")
    p.add_argument("--grf", action="store_true", help="record ground reaction forces after every env step (grf / cop / foot_contact / load in the "
                   "coverage_full record) and write grf_metrics_<iter>_<data>.json; off: every output file is what it is without the flag")
    p.add_argument("--dynamics_metrics", action="store_true", help="inverse dynamics of the simulated (pred) and the expert (gt) poses of every take (root "
                   "residual force / body weight, residual torque, joint torque rms, share over torque_lim, power) printed and written to "
                   "dynamics_metrics_<iter>_<data>.json; off: every output file is what it is without the flag")
    p.add_argument("--dynamics_contacts", choices=("soft", "estimated", "both"), default="soft", help="with --dynamics_metrics: the contact forces the score "
                   "credits: soft (the soft-constraint forces of inverse dynamics), estimated (forces inside the friction cones of the points near a "
                   "surface that best explain the root residual; keys *_est of the same json) or both")
    p.add_argument("--balance_metrics", action="store_true", help="balance of the simulated (pred) and the expert (gt) poses of every take (margins of the "
                   "centre of mass, the capture point and the zero-moment point to the support polygon, stable / airborne share) printed and written to "
                   "balance_metrics_<iter>_<data>.json; off: every output file is what it is without the flag")
    from kinpoly_amd.push import add_push_arguments
    return add_push_arguments(p)       # --push_impulse LO [HI] and friends: perturbation pushes while the takes play (off by default)


def check_mode(args):
    if args.mode in VIEWER_MODES or args.record or args.preview or args.record_expert:
        raise SystemExit(f"eval_uhc.py: --mode {args.mode}" + (" with --record / --preview" if args.mode == "stats" else "") +
                         " needs the reference's MuJoCo viewer, which this engine does not have; use --mode stats")
    if args.mode != "stats":
        raise SystemExit(f"eval_uhc.py: unknown --mode {args.mode!r} (this engine runs --mode stats)")
    if args.no_root:
        raise SystemExit("eval_uhc.py: --no_root is not supported")


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_mode(args)
    import numpy as np
    import torch
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd.dataset import AmassSingleDataset, SmplObjDataset
    from kinpoly_amd.evaluate import eval_uhc_takes, write_uhc_coverage
    from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent
    cfg = None
    if args.cfg:
        from kinpoly_amd.uhc_config import UhcConfig
        cfg = UhcConfig(args.cfg, config_root=args.config_root)
    specs = dict(cfg.data_specs) if cfg is not None else {"t_min": 90}
    if args.takes:
        specs["test_file_path"] = args.takes
    if args.t_min is not None:
        specs["t_min"] = args.t_min
    if "test_file_path" not in specs:
        raise SystemExit("eval_uhc.py: no take file: give --takes, or a --cfg whose data_specs has test_file_path")
    ckpt = args.ckpt or os.path.join(args.config_root or os.getcwd(), "results", "motion_im", str(args.cfg), "models", "iter_%04d.p" % args.iter)
    ds = {"amass_single": AmassSingleDataset, "smpl_obj": SmplObjDataset}[args.dataset](specs, "test")
    torch.cuda.set_device(0)
    n = min(args.num_envs, ds.get_len())
    env = BatchedHumanoidEnv(n, 0, cfg=cfg) if cfg is not None else BatchedHumanoidEnv(n, 0, env_init_noise=0.0)
    agent = CopycatAgent(env, **(cfg.ppo_kwargs() if cfg is not None else {}))
    cp = ck.load_checkpoint(ckpt)
    agent.policy.load_state_dict({k: torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v for k, v in cp["policy_dict"].items()})
    rs = None
    if cp.get("running_state") is not None:
        st = cp["running_state"].rs
        rs = agent.running_state
        rs.count = int(st._n)
        rs._mean64.copy_(torch.as_tensor(st._M, dtype=torch.float64)); rs._m2.copy_(torch.as_tensor(st._S, dtype=torch.float64))
        rs.mean.copy_(rs._mean64.float())
        rs.std.copy_((torch.sqrt(rs._m2 / (rs.count - 1)) if rs.count > 1 else rs._mean64.abs()).float())
    from kinpoly_amd.push import schedule_from_args
    sched = schedule_from_args(args, n, env.device, record=True)
    res = eval_uhc_takes(env, agent.policy, rs, ds, fail_safe=args.fail_safe, push_schedule=sched, grf=args.grf)
    for k, r in res.items():
        print(f"{r['percent']}  | {k} | {r['fail_safe']}")
    out_dir = os.path.dirname(os.path.abspath(ckpt))
    cov = write_uhc_coverage(res, out_dir, args.iter, args.data, no_full=args.no_full)
    print(f"Coverage of {cov} out of {ds.get_len()}")
    if args.grf:
        from kinpoly_amd import metrics as M
        from kinpoly_amd.contact import body_weight
        m = M.write_grf_metrics(res, body_weight(env), out_dir, args.iter, args.data)       # env.body_mass: the masses of the model the env runs
        print("".join(f"{k}:{v:.3f} \t " for k, v in m.items()))
    if args.dynamics_metrics:          # a dynamics score of the expert takes themselves (gt) beside the simulated states (pred): floor scene, rows API of the env's handle
        from kinpoly_amd import metrics as M
        gt = {k: {"qpos": np.asarray(r["gt"])} for k, r in res.items()}
        dm = M.write_dynamics_metrics(res, gt, env.sim, out_dir, args.iter, args.data, dt=env.dt, contacts=args.dynamics_contacts)
        print("".join(f"{k}:{v:.4f} \t " for k, v in dm.items() if k not in ("per_take", "by_action")))
    if args.balance_metrics:           # the same for balance: floor scene, rows API of the env's handle
        from kinpoly_amd import metrics as M
        gt = {k: {"qpos": np.asarray(r["gt"])} for k, r in res.items()}
        bm = M.write_balance_metrics(res, gt, env.sim, out_dir, args.iter, args.data, dt=env.dt)
        print("".join(f"{k}:{v:.4f} \t " for k, v in bm.items() if k not in ("per_take", "by_action")))
    if sched is not None:              # the coverage pickles keep their keys; the pushes go to a file of their own
        import joblib
        joblib.dump(sched.by_take, os.path.join(out_dir, f"push_log_{args.iter}_{args.data}.pkl"))
        print(f"pushes applied: {sum(len(v) for v in sched.by_take.values())}")
        print(f"coverage under pushes: {cov} out of {ds.get_len()}")


if __name__ == "__main__":
    main()
