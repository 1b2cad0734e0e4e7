#!/usr/bin/env python
"""Supervised training / testing of the kinematic model (the reference's scripts/exp_arnet_all.py:62-183).

    python scripts/exp_arnet_all.py --cfg kin_poly --mode train            # results/all/statear/<cfg>/models/iter_%04d.p
    python scripts/exp_arnet_all.py --cfg kin_poly --mode test --iter 2000 # results/.../results/iter_2000_test_<data_file>.p + metrics per action

Without a feature file (<dataset_path>/features/<data_file>.p) the synthetic feature set of the other scripts is used.  --dtype fp32 (default) trains on
the path --path names (default taped): `taped` = the HIP roll-out with its gradient kernels (kinpoly_amd/kin_tape.py), `torch` = pretrain.forward_supervised; fp64 -- the
reference's precision -- always runs on the torch path.  --as_policy trains the network with the action
one-hot in its state (105-d under kin_poly.yml), which train_ar_policy.py --load can start from; the default is the reference's as_policy=False (101-d).
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default=None)
    ap.add_argument("--mode", default="train", choices=("train", "test"))
    ap.add_argument("--data", default=None)
    ap.add_argument("--gpu-index", type=int, default=0)
    ap.add_argument("--iter", type=int, default=0)
    ap.add_argument("--action", type=str, default="all")
    ap.add_argument("--wild", action="store_true", default=False)
    ap.add_argument("--config_root", type=str, default=None, help="directory that holds config/ and the dataset_path of the yml (default: cwd)")
    ap.add_argument("--dtype", choices=("fp32", "fp64"), default="fp32", help="fp32: the path --path names; fp64: the reference's precision, torch path only")
    ap.add_argument("--path", choices=("torch", "taped"), default=None, help="fp32 only: the roll-out on torch ops (pretrain.forward_supervised) or on the taped HIP kernels "
                    "(kinpoly_amd/kin_tape.py); default: kinpoly_amd.exp_arnet.DEFAULT_PATH")
    ap.add_argument("--as_policy", action="store_true", help="train the network with the action one-hot in its state (what train_ar_policy.py --load takes)")
    ap.add_argument("--epochs", type=int, default=0, help="stop after this many epochs of this run (0: up to cfg.num_epoch)")
    ap.add_argument("--num_sample", type=int, default=None); ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--save_interval", type=int, default=None)
    from kinpoly_amd.dataset import add_of_source_argument
    return add_of_source_argument(ap)


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from kinpoly_amd.dataset import of_source_refusal
    no = of_source_refusal(args.of_source, args.wild)
    if no:
        ap.error(no)
    return ap, args


def main():
    ap, args = parse_args()
    if args.cfg is None:
        ap.error("--cfg is required (a config id under --config_root, or a .yml path)")
    if args.data is None:
        args.data = args.mode
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.config import Config
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.ppo import lambda_lr
    from kinpoly_amd.supervised import TorchFK
    if args.config_root:
        os.chdir(args.config_root)
    cfg = Config(args.cfg, action=args.action, wild=args.wild, create_dirs=True, entry="kin_model")
    torch.cuda.set_device(args.gpu_index)
    device = torch.device("cuda", args.gpu_index)
    dtype = torch.float64 if args.dtype == "fp64" else torch.float32
    if args.dtype == "fp64" and args.path == "taped":
        ap.error("--path taped runs the fp32 kernels; --dtype fp64 stays on the torch path")
    np.random.seed(cfg.seed); torch.manual_seed(cfg.seed)
    mk = cfg.model_kwargs()
    loss_weights = {k: mk.pop(k) for k in list(mk) if k.startswith("w_")}
    kin_model = kpsim.KpModel(kpsim.STEP_KPM, **kpsim.ar_obs_options(cfg.use_vel, cfg.use_head, bool(cfg.use_action) and args.as_policy))
    fk_sim = kpsim.KpSim(kin_model, 1, args.gpu_index)
    y = cfg.yaml_data
    num_sample = int(y.get("num_sample", 20000)) if args.num_sample is None else args.num_sample
    batch_size = int(cfg.batch_size) if args.batch_size is None else args.batch_size
    feat = cfg.feature_path()
    data_mode = "train" if args.mode == "train" else "test"
    of_path = cfg.feature_path(cfg.of_file)
    if os.path.exists(feat):
        import joblib
        takes, take_list = joblib.load(feat), cfg.takes[args.data if args.data in ("train", "test") else data_mode] or None
    else:
        std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
        takes = D.synthetic_takes(fk_sim, std["qpos"], n_per_action=4, T_range=(E.FR_NUM_END + 10, E.FR_NUM_END + 60), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=4)
        take_list = None
    of = None
    if cfg.use_of:      # the file's features (their width is the file's), or this repository's synthetic stand-in model_specs.cnn_fdim wide
        of, said = D.select_of_features(args.of_source, takes, of_path, int(cfg.model_specs.get("cnn_fdim", 512)), cfg.seed, fk_sim, args.wild)
        print(f"of features: {said}", flush=True)
    ds = D.StateARDataset(takes, takes=take_list, data_mode=data_mode, fr_num=E.FR_NUM_START, wild=args.wild, seed=cfg.seed, device=device, of_features=of)
    net = E.build_net(cfg.use_vel, cfg.use_head, cfg.use_action, as_policy=args.as_policy, use_context=bool(cfg.use_context), of_dim=ds.of_dim, **mk).to(device)
    # the training path: --path, else the default measured for the file's kind (DESIGN.md section 10 holds both records)
    fused = args.dtype == "fp32" and (args.path or (E.DEFAULT_PATH_CONTEXT if net.ctx_block else E.DEFAULT_PATH)) == "taped"
    print(f"dataset: {ds.get_len()} takes; net: state {net.state_dim}, context {net.context_dim}; {'taped HIP roll-out' if fused else 'torch path'} {args.dtype}", flush=True)
    if args.iter > 0:
        cp_path = os.path.join(cfg.model_dir, "iter_%04d.p" % args.iter)
        print(f"loading model from checkpoint: {cp_path}", flush=True)
        E.load_arnet(cp_path, net)
    kpm = read_kpm(DEFAULT_KPM)
    if args.mode == "train":
        net.to(dtype).train()
        if dtype == torch.float64:
            net.refresh_log_std()
        fk = TorchFK(kpm["body_pos"], kpm["body_parent"], device, dtype=dtype, sim=fk_sim if dtype == torch.float32 else None)
        # the LambdaLR of get_scheduler(policy='lambda') acts on the optimiser built before the loop; every epoch trains with a fresh Adam at cfg.lr (:131)
        sched_opt = torch.optim.Adam(net.parameters(), lr=cfg.lr, weight_decay=cfg.weightdecay)
        scheduler = lambda_lr(sched_opt, cfg.num_epoch_fix, cfg.num_epoch)
        interval = cfg.save_model_interval if args.save_interval is None else args.save_interval
        last = cfg.num_epoch if not args.epochs else min(cfg.num_epoch, args.iter + args.epochs)
        log = open(os.path.join(cfg.log_dir, "log.txt"), "a")
        for i_epoch in range(args.iter, last):
            t0 = time.time()
            loss, comp, rate, fr_num = E.train_epoch(net, fk, ds, i_epoch, cfg.num_epoch, cfg.lr, cfg.weightdecay, num_sample, batch_size,
                                                     noise_std=float(cfg.noise_std) if cfg.add_noise else 0.0, fused=fused, weights=loss_weights)
            line = (f"epoch {i_epoch:4d}    time {time.time() - t0:.2f}   loss {loss:.4f} {np.round(np.array(comp) * 100, 4).tolist()} lr: {cfg.lr} "
                    f"sampling_rate: {rate:.3f}, fr_num: {fr_num}")
            print(line, flush=True); log.write(line + "\n"); log.flush()
            scheduler.step()
            if interval > 0 and (i_epoch + 1) % interval == 0:
                E.save_arnet(os.path.join(cfg.model_dir, "iter_%04d.p" % (i_epoch + 1)), net)
    else:
        net.float().eval()
        res = E.test_takes(net, kin_model, ds, device)
        res_path = os.path.join(cfg.result_dir, "iter_%04d_%s_%s.p" % (args.iter, args.data, cfg.data_file))
        print(f"results dir: {res_path}")
        with open(res_path, "wb") as f:
            pickle.dump(res, f)
        # scripts/eval_pose_all.py --mode stats, in process: the kinematic metrics per action
        from kinpoly_amd import metrics as M
        tfk = TorchFK(kpm["body_pos"], kpm["body_parent"], "cpu", dtype=torch.float64)
        per = {}
        for take, r in res.items():
            jp, jg = (tfk.chain_torch(torch.as_tensor(r[k], dtype=torch.float64))[0].numpy() for k in ("qpos", "qpos_gt"))
            per.setdefault(take.split("-")[0], []).append(M.sequence_metrics(r["qpos"], r["qpos_gt"], jp, jg))
        for action, ms in sorted(per.items()):
            print(json.dumps({"action": action, "takes": len(ms), **{k: round(float(np.mean([m[k] for m in ms])), 4) for k in ms[0]}}), flush=True)


if __name__ == "__main__":
    main()
