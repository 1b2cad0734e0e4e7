#!/usr/bin/env python
"""Measurements of the video-conditioned policy's context ring on one GPU (DESIGN.md section 8 holds the record).

    python tools/ctx_ring_bench.py refill  [--clips 4096 --frames 100 --H 256 --F 512 --blocks 3 --calls 20]
    python tools/ctx_ring_bench.py sampler [--num_envs 4096 --horizon 24 --blocks 3]

refill   kp_ctx_rows_write against the torch composition it replaces (transpose, last-frame pad, index_copy_ per table), both in this process,
         alternating block by block after a warm-up; per side the median and min .. max of the per-call times of the blocks, and the peak memory of
         one call (torch.cuda.max_memory_allocated above what is allocated before it).  Pass rule (the one tools/uhc_takes_bench.py prints): the kernel's
         median is no worse than the composition's median plus the composition's own max - min.
sampler  VectorSampler.sample env-steps/s with tests/golden/kin_poly_of.yml (use_context + use_of, rnn_hdim 256, features 512 wide) next to kin_poly.yml's
         switches (both off, rnn_hdim 1024) on the same synthetic takes, and the HBM the ring holds (torch.cuda.memory_allocated before and after
         _pool_init).  No gate: the figures are what a user plans with.

One JSON line per measurement.
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


def _time_calls(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def refill(args):
    from kinpoly_amd import sim as kpsim
    m, T, H, F, Tp = args.clips, args.frames, args.H, args.F, args.clip_frames or args.frames
    R = m + 64
    g = torch.Generator(device="cuda").manual_seed(0)
    seq, of = torch.randn((Tp, m, H), device="cuda", generator=g), torch.randn((m, Tp, F), device="cuda", generator=g)
    ct, ot = torch.zeros((R, T, H), device="cuda"), torch.zeros((R, T, F), device="cuda")
    rows = torch.randperm(R, device="cuda", generator=g)[:m].contiguous()
    rows_host = rows.cpu()

    def fit(v):
        return v if v.shape[1] == T else torch.cat([v, v[:, -1:].expand(-1, T - v.shape[1], -1)], 1)

    def composed():
        ct.index_copy_(0, rows, fit(seq.transpose(0, 1)))
        ot.index_copy_(0, rows, fit(of))

    def kernel():
        kpsim.ctx_rows_write(rows_host, seq, of, ct, ot)      # host rows: the range check costs no device read
    composed()
    want_c, want_o = ct.clone(), ot.clone()
    ct.zero_(); ot.zero_()
    kernel()
    same = torch.equal(ct, want_c) and torch.equal(ot, want_o)
    del want_c, want_o
    for fn in (composed, kernel):
        _time_calls(fn, 5)
    t = {"composed": [], "kernel": []}
    for _ in range(args.blocks):
        t["composed"].append(_time_calls(composed, args.calls))
        t["kernel"].append(_time_calls(kernel, args.calls))
    res = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in t.items()}
    c = res["composed"]
    moved = 2.0 * m * T * (H + F) * 4
    print(json.dumps({"bench": "ctx_rows_write", "clips": m, "frames": T, "clip_frames": Tp, "H": H, "F": F, "blocks": args.blocks, "calls": args.calls, "same_words": same, **res,
                      "kernel_GBps": moved / res["kernel"]["median_ms"] / 1e6, "peak_bytes": {"composed": _peak(composed), "kernel": _peak(kernel)},
                      "pass": bool(res["kernel"]["median_ms"] <= c["median_ms"] + (c["max_ms"] - c["min_ms"]))}), flush=True)


def sampler(args):
    from kinpoly_amd import dataset as D
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.agent import AgentAR
    from kinpoly_amd.config import Config
    from kinpoly_amd.model_compiler import read_kpm
    import tempfile
    import yaml
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    tmp = tempfile.mkdtemp()
    wide = os.path.join(ROOT, "tests", "golden", "kin_poly_of.yml")
    y = yaml.safe_load(open(wide))
    plain = os.path.join(tmp, "kin_poly.yml")
    with open(plain, "w") as f:                          # kin_poly.yml: the same file with the two switches off and its own rnn_hdim
        yaml.safe_dump(dict(y, use_of=False, use_context=False, model_specs=dict(y["model_specs"], rnn_hdim=1024)), f)
    fk_sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), 64, 0)
    fr = int(y["fr_num"])
    takes = D.synthetic_takes(fk_sim, std["qpos"], n_per_action=4, T_range=(fr + 10, fr + 60), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=4)
    for name, path in (("kin_poly", plain), ("kin_poly_of", wide)):
        cfg = Config(path, base_dir=os.path.join(tmp, "results"), entry="policy_ctx")
        of = D.synthetic_of_features(takes, int(cfg.model_specs.get("cnn_fdim", 512)), seed=cfg.seed) if cfg.use_of else None
        ds = D.StateARDataset(takes, fr_num=fr, seed=4, device=fk_sim.device, of_features=of)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        from kinpoly_amd import rollout as R
        orig = R.VectorSampler._pool_init

        def measured(smp):                                   # the ring: what _pool_init leaves allocated (the constructor starts the sampler)
            torch.cuda.synchronize()
            a = torch.cuda.memory_allocated()
            orig(smp)
            torch.cuda.synchronize()
            smp.ring_bytes = torch.cuda.memory_allocated() - a
        R.VectorSampler._pool_init = measured
        try:
            agent = AgentAR(args.num_envs, dataset=ds, device=0, horizon=args.horizon, **cfg.agent_kwargs(ds.of_dim or None))
        finally:
            R.VectorSampler._pool_init = orig
        cfg.apply_reward_weights(agent.env)
        agent.sampler.sample(args.horizon)                 # warm-up
        torch.cuda.synchronize()
        rates = []
        for _ in range(args.blocks):
            t0 = time.time()
            agent.sampler.sample(args.horizon)
            torch.cuda.synchronize()
            rates.append(args.num_envs * args.horizon / (time.time() - t0))
        c = agent.env.ctx
        rows = c["qpos"].shape[0]
        print(json.dumps({"bench": "sampler", "cfg": name, "num_envs": args.num_envs, "horizon": args.horizon, "obs_dim": agent.env.obs_dim,
                          "env_steps_per_s": {"median": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates))},
                          "ring_rows": rows, "pool_init_bytes": agent.sampler.ring_bytes, "wide_table_bytes": sum(c[k].numel() * 4 for k in ("context_feat_rnn", "of") if k in c),
                          "allocated_before_agent": before, "top_ups": agent.sampler.top_ups}), flush=True)
        del agent
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("refill", "sampler"))
    ap.add_argument("--clips", type=int, default=4096); ap.add_argument("--frames", type=int, default=100); ap.add_argument("--clip_frames", type=int, default=0)
    ap.add_argument("--H", type=int, default=256); ap.add_argument("--F", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=3); ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--num_envs", type=int, default=4096); ap.add_argument("--horizon", type=int, default=24)
    args = ap.parse_args()
    {"refill": refill, "sampler": sampler}[args.what](args)


if __name__ == "__main__":
    main()
