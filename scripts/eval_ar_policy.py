#!/usr/bin/env python
"""Counterpart of the reference's scripts/eval_ar_policy.py --mode stats on the batched engine: every sequence of the test
set is one environment; writes `<iter>_<data_file>_coverage(.|_full).pkl` in the reference's format.

The reference's test sets are not part of its repository; without `--data` this evaluates synthetic standing sequences.

    python scripts/eval_ar_policy.py --num_seq 256 [--ckpt results/.../iter_0750.p] [--fail_safe] [--ar_mode]
    python scripts/eval_ar_policy.py --data sample_data/features/mocap_annotations.p --ckpt ... [--wild]       # every take of a feature file, played whole
    python scripts/eval_ar_policy.py --cfg kin_poly --config_root /path/to/KinPoly --iter 750 [--data test]     # the reference's command line (--mode stats)

With --cfg the feature file, the take list (`meta/<meta_id>.yml`), the checkpoint (`models_policy/iter_%04d.p`) and the result directory come from
the reference's yml (kinpoly_amd/config.py), and the coverage pickles land where eval_pose_all.py looks for them.  A yml with `use_context` / `use_of` evaluates
the video-conditioned policy: the image features are `<dataset_path>/features/<of_file>.p` (`of_file_wild` with --wild) or, without that file, this repository's
synthetic stand-in (said on stdout); such a policy needs takes (--data or the yml's feature file), not the synthetic standing sequences.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_seq", type=int, default=256)
    ap.add_argument("--clip_len", type=int, default=100)
    ap.add_argument("--ckpt", type=str, default="")
    ap.add_argument("--iter", type=int, default=0)
    ap.add_argument("--fail_safe", action="store_true")
    ap.add_argument("--ar_mode", action="store_true")
    ap.add_argument("--wild", action="store_true")
    ap.add_argument("--result_dir", type=str, default="results/eval")
    ap.add_argument("--data_file", type=str, default="synthetic_standing")
    ap.add_argument("--data", type=str, default="", help="feature file in the reference's schema, or train / test with --cfg")
    ap.add_argument("--metrics", action="store_true", help="with --data: root_dist / mpjpe / accel_dist / vel_dist / head_dist / succ over the takes (eval_pose_all.py's kinematic metrics)")
    ap.add_argument("--physics_metrics", action="store_true", help="with --data: pen_pred / pen_gt / slide_pred / slide_gt / succ (eval_pose_all.py's "
                    "compute_physcis_metris) on the scene the run used, printed after the kinematic line")
    ap.add_argument("--grf", action="store_true", help="record ground reaction forces after every env step (grf / cop / foot_contact / load in the "
                    "coverage_full record) and write grf_metrics_<iter>_<data>.json; off: every output file is what it is without the flag")
    ap.add_argument("--dynamics_metrics", action="store_true", help="with --data: inverse dynamics of the predicted and the ground-truth poses (root residual "
                    "force / body weight, residual torque, joint torque rms, share over torque_lim, power; pred and gt) printed and written to "
                    "dynamics_metrics_<iter>_<data>.json; off: every output is what it is without the flag")
    ap.add_argument("--dynamics_contacts", choices=("soft", "estimated", "both"), default="soft", help="with --dynamics_metrics: the contact forces the score "
                    "credits: soft (the soft-constraint forces of inverse dynamics), estimated (forces inside the friction cones of the points near a "
                    "surface that best explain the root residual; keys *_est of the same json) or both")
    ap.add_argument("--balance_metrics", action="store_true", help="with --data: balance of the predicted and the ground-truth poses (margins of the centre of "
                    "mass, the capture point and the zero-moment point to the support polygon, stable / airborne share; pred and gt) printed and written to "
                    "balance_metrics_<iter>_<data>.json; off: every output is what it is without the flag")
    ap.add_argument("--cfg", type=str, default=None)
    ap.add_argument("--config_root", type=str, default=None)
    from kinpoly_amd.dataset import add_of_source_argument
    add_of_source_argument(ap)
    from kinpoly_amd.push import add_push_arguments
    return add_push_arguments(ap)      # --push_impulse LO [HI] and friends: perturbation pushes while the sequences play (off by default)


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from kinpoly_amd.dataset import of_source_refusal
    no = of_source_refusal(args.of_source, args.wild)
    if no:
        ap.error(no)
    return args


def report_pushes(sched, res, result_dir, iter_num, data_file):
    """`pushes applied`, `coverage under pushes` and <result_dir>/push_log_<iter>_<data>.pkl = {take: [(step, body, impulse[6])]}"""
    import joblib
    os.makedirs(result_dir, exist_ok=True)
    joblib.dump(sched.by_take, os.path.join(result_dir, f"push_log_{iter_num}_{data_file}.pkl"))
    print(f"pushes applied: {sum(len(v) for v in sched.by_take.values())}")
    print(f"coverage under pushes: {sum(1 for r in res.values() if r['percent'] == 1 and not r['fail_safe'])} out of {len(res)}")


def report_grf(res, result_dir, iter_num, data_file):
    """the --grf line and <result_dir>/grf_metrics_<iter>_<data>.json"""
    from kinpoly_amd import metrics as M
    from kinpoly_amd.contact import body_weight
    from kinpoly_amd.model_compiler import DEFAULT_KPM
    m = M.write_grf_metrics(res, body_weight(DEFAULT_KPM), result_dir, iter_num, data_file)
    print("".join(f"{k}:{v:.3f} \t " for k, v in m.items()))


def main():
    args = parse_args()
    from kinpoly_amd import checkpoint as ck
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.context import PolicyARContext, TrajARNet
    from kinpoly_amd.env import BatchedHumanoidAREnv, standing_context
    from kinpoly_amd.evaluate import run_sequences, write_coverage
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    n, T = args.num_seq, args.clip_len
    torch.manual_seed(0)
    cfg, takes = None, None
    if args.cfg:
        from kinpoly_amd.config import Config
        if args.config_root:
            os.chdir(args.config_root)
        cfg = Config(args.cfg, wild=args.wild, entry="policy_ctx")
        mode = args.data if args.data in ("train", "test") else "test"
        takes = cfg.takes[mode] or None
        args.data = cfg.feature_path() if args.data in ("", "train", "test") else args.data
        args.result_dir, args.data_file, T = cfg.result_dir, cfg.data_file, int(cfg.fr_num)
        if args.iter > 0 and not args.ckpt:
            args.ckpt = cfg.checkpoint_path(args.iter)
    # the observation variant of the yml (use_action false: kin_poly_wo_action.yml, 101-d; use_vel / use_head: kinpoly_amd.sim.ar_obs_dim)
    obs_kw = dict(use_action=cfg.use_action, use_vel=cfg.use_vel, use_head=cfg.use_head) if cfg is not None else {}
    # the video-conditioned policy of the yml (use_context / use_of): the features first, their width is the `of` block's
    ctx_kw, feats, of = {}, None, None
    if cfg is not None and (cfg.use_context or cfg.use_of):
        if not args.data:
            raise SystemExit("use_context / use_of: the policy reads a context sequence of real takes; give --data (or a yml whose feature file exists)")
        import joblib
        from kinpoly_amd import dataset as D
        feats = joblib.load(args.data)
        if cfg.use_of:
            render_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), 1, 0) if args.of_source == "rendered" else None
            of, said = D.select_of_features(args.of_source, feats, cfg.of_feature_path(), int(cfg.model_specs.get("cnn_fdim", 512)), cfg.seed, render_sim, args.wild)
            print(f"of features: {said}", flush=True)
            of = joblib.load(of) if isinstance(of, str) else of
    if cfg is not None:          # the net sizes the yml names (as train_ar_policy.py builds the agent), the context block and the `of` block
        ctx_kw = cfg.context_kwargs(int(np.asarray(next(iter(of.values()))).shape[1]) if of else None)
    ctx_block = int(ctx_kw.get("rnn_hdim", 1024)) if (ctx_kw.get("use_context") or ctx_kw.get("of_dim")) else 0          # TrajARNet.ctx_block
    env = BatchedHumanoidAREnv(n, 0, mode="test", wild=args.wild, ar_mode=args.ar_mode, seed=0, **obs_kw, ctx_dim=ctx_block, of_dim=ctx_kw.get("of_dim", 0))
    from kinpoly_amd.push import schedule_from_args
    sched = schedule_from_args(args, n, env.device, record=True)
    if cfg is not None:
        cfg.apply_reward_weights(env)
    net = TrajARNet(log_std=cfg.policy_specs["log_std"] if cfg else -3.2, **obs_kw, **ctx_kw, of_in_state=bool(ctx_kw.get("of_dim", 0))).to(env.device)
    assert net.ctx_block == ctx_block and net.state_dim == env.obs_dim
    if args.ckpt:
        cp = ck.load_checkpoint(args.ckpt)
        sd = ck.split_policy_dict(cp["policy_dict"])
        ck.check_policy_obs_dim(sd, net.state_dim, args.ckpt)
        ck.check_state_shapes(sd, net, args.ckpt)          # other net sizes (rnn_hdim, mlp_hsize): refused with both shapes
        net.load_state_dict(sd, strict=False)
    if args.data:                                   # every take of the feature file, whole, env.n at a time (run_seq over data_loader.iter_seq)
        from kinpoly_amd import dataset as D
        from kinpoly_amd.evaluate import eval_dataset
        ds = D.StateARDataset(args.data if feats is None else feats, takes=takes, data_mode="test", fr_num=T, wild=args.wild, seed=0, device=env.device, of_features=of)
        builder = PolicyARContext(net, kpsim.KpSim(env.model, n, 0), smooth=bool(cfg.smooth) if cfg else True, keep_context_feat=bool(ctx_block))
        res = eval_dataset(env, net, builder, ds, fail_safe=args.fail_safe, push_schedule=sched, grf=args.grf)
        data_file = args.data_file if args.cfg else os.path.splitext(os.path.basename(args.data))[0]
        cov = write_coverage(res, args.result_dir, args.iter, data_file)
        if args.grf:
            report_grf(res, args.result_dir, args.iter, data_file)
        if sched is not None:
            report_pushes(sched, res, args.result_dir, args.iter, data_file)
        pct = np.array([r["percent"] for r in res.values()])
        print(f"Coverage of {cov} out of {len(res)} | mean percent {pct.mean():.3f} | fail-safe used in {sum(r['fail_safe'] for r in res.values())}")
        if args.metrics or args.physics_metrics or args.dynamics_metrics or args.balance_metrics:    # the paper metrics of scripts/eval_pose_all.py --mode stats (kinpoly_amd/metrics.py)
            from kinpoly_amd import metrics as M
            gt = {k: {"qpos": ds.data["qpos"][i].double().numpy(), "head_pose": ds.data["head_pose"][i].double().numpy()} for i, k in enumerate(ds.takes)}
        if args.metrics:                            # the kinematic ones
            from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
            from kinpoly_amd.supervised import TorchFK
            kpm = read_kpm(DEFAULT_KPM)
            tfk = TorchFK(kpm["body_pos"], kpm["body_parent"], "cpu", dtype=torch.float64)
            m = M.coverage_metrics(res, gt, lambda q: tuple(x.numpy() for x in tfk.chain_torch(torch.as_tensor(q))))
            print("".join(f"{k}:{v:.3f} \t " for k, v in m.items() if k != "per_take"))
        if args.physics_metrics:                    # compute_physcis_metris on the scene the run used: contact walk on the device, rules on the host
            pm = M.coverage_physics_metrics(res, gt, kpsim.KpSim(env.model, 1, 0))     # env.model: _all.xml with --wild, else _all_step.xml (env.py)
            print("".join(f"{k}:{v:.3f} \t " for k, v in pm.items() if k not in ("per_take", "succ_by_action")))
            print({k: round(v, 3) for k, v in pm["succ_by_action"].items()})
        if args.dynamics_metrics:                   # inverse dynamics of poses that were never simulated (kinematic target and ground truth), on the run's scene
            dm = M.write_dynamics_metrics(res, gt, kpsim.KpSim(env.model, 1, 0), args.result_dir, args.iter, data_file, contacts=args.dynamics_contacts)
            print("".join(f"{k}:{v:.4f} \t " for k, v in dm.items() if k not in ("per_take", "by_action")))
        if args.balance_metrics:                    # balance of the same poses, floor scene
            bm = M.write_balance_metrics(res, gt, kpsim.KpSim(env.model, 1, 0), args.result_dir, args.iter, data_file)
            print("".join(f"{k}:{v:.4f} \t " for k, v in bm.items() if k not in ("per_take", "by_action")))
        return
    g = torch.Generator().manual_seed(0)
    ctx = standing_context(n, T, std["qpos"], std["qvel"], env.sim, (torch.rand(n, generator=g) * 2 - 1) * np.pi)
    ctx["obj_pose"] = torch.tensor([0.0, 0, 0, 1, 0, 0, 0], device=env.device).repeat(n, T, 1)
    ctx = PolicyARContext(net, kpsim.KpSim(env.model, n, 0), smooth=True).init_context(ctx)
    env.load_context(ctx)
    keys = [f"standing-{i:05d}" for i in range(n)]
    res = run_sequences(env, net, keys, fail_safe=args.fail_safe, push_schedule=sched, grf=args.grf)
    cov = write_coverage(res, args.result_dir, args.iter, args.data_file)
    if args.grf:
        report_grf(res, args.result_dir, args.iter, args.data_file)
    if sched is not None:
        report_pushes(sched, res, args.result_dir, args.iter, args.data_file)
    pct = np.array([r["percent"] for r in res.values()])
    print(f"Coverage of {cov} out of {n} | mean percent {pct.mean():.3f} | fail-safe used in {sum(r['fail_safe'] for r in res.values())}")


if __name__ == "__main__":
    main()
