"""Rows per second of the batched pose-contact query (KpSim.pose_contacts: fk + kp_sim_pose_contacts) on a synthetic evaluation set with
objects: 10^5 rows = the predicted and the ground-truth frames of takes with one active object each (chair, box, table, Can, step).  Device
time by events after a warm-up; next to it the single-core fp64 oracle's rows per second (OracleSim reset = sim.forward, one run per frame).

    python tools/pose_contacts_bench.py [--rows 100000] [--oracle_rows 2000]
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


def synthetic_rows(n, seed=0):
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))["qpos"]
    rng = np.random.default_rng(seed)
    q = np.tile(std, (n, 1))
    q[:, 7:] += rng.normal(size=(n, 69)) * 0.1
    q[:, :2] += rng.normal(size=(n, 2)) * 0.05
    q[:, 2] += rng.normal(size=n) * 0.01
    blk = np.zeros((n, 35))
    for i in range(5):
        blk[:, 7 * i: 7 * i + 3] = [(i + 1) * 100, 100, 0]
    x0, y0 = std[0], std[1]
    poses = {0: [x0 + 0.35, y0, 0.38], 1: [x0 + 0.4, y0, 0.22], 2: [x0 + 0.55, y0, 0.95], 3: [x0 + 0.36, y0 + 0.05, 0.69], 4: [x0 + 0.3, y0, 0.3705]}
    obj = rng.integers(0, 5, n)
    for e in range(n):
        oi = int(obj[e])
        blk[e, 7 * oi: 7 * oi + 7] = [*poses[oi], 1, 0, 0, 0]
        blk[e, 7 * oi: 7 * oi + 2] += rng.normal(size=2) * 0.05
    return q, blk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--oracle_rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_contacts_bench: no HIP device visible (the query has no CPU path)")
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.model_compiler import STEP_KPM, read_kpm
    q, blk = synthetic_rows(args.rows)
    s = kpsim.KpSim(kpsim.KpModel(STEP_KPM), 1)
    qd = torch.tensor(q, dtype=torch.float32, device="cuda"); bd = torch.tensor(blk, dtype=torch.float32, device="cuda")
    out = s.pose_contacts(qd, bd)                                  # warm-up (code object load)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = s.pose_contacts(qd, bd); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1000.0)
    ncon = out["ncon"].cpu().numpy(); hits = out["hits"].cpu().numpy()
    from oracle.kpo import OracleSim, object_geoms
    kpm = read_kpm(STEP_KPM)
    o = OracleSim(kpm=STEP_KPM)
    m = min(args.oracle_rows, args.rows)
    t0 = time.perf_counter()
    for e in range(m):
        o.set_geoms(object_geoms(kpm, blk[e]))
        o.reset(q[e], np.zeros(75))
        o.contacts_full()
    t_or = time.perf_counter() - t0
    dev_s = float(np.median(times))
    print(json.dumps({"rows": args.rows, "device_seconds_median": dev_s, "device_seconds": times, "rows_per_s": args.rows / dev_s,
                      "oracle_rows_per_s_single_core": m / t_or, "speedup_vs_oracle_core": (args.rows / dev_s) / (m / t_or),
                      "mean_ncon": float(ncon.mean()), "max_ncon": int(ncon.max()), "rows_with_object_hits": int((hits != 0).any(1).sum()),
                      "device": torch.cuda.get_device_name(0)}))
    assert dev_s < 1.0, f"{args.rows} rows took {dev_s:.3f} s of device time (gate: 1 s)"


if __name__ == "__main__":
    main()
