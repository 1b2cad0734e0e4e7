#!/usr/bin/env python
"""Kernel launches per frame (forward + backward) of the supervised whole-clip roll-out, torch path and taped HIP path: per path two
`rocprofv3 --kernel-trace --stats` runs of ONE batch of 256 clips that differ only in the clip length; the difference of the call counts / the
difference of the lengths is what one frame launches (context GRU's per-frame share and the loss included; set-up cancels).
    python tools/kin_tape_launches.py <out_dir> [frames_a frames_b]"""
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(path, T):
    import numpy as np
    import torch
    from kinpoly_amd import dataset as D
    from kinpoly_amd import kin_tape
    from kinpoly_amd import pretrain as P
    from kinpoly_amd import sim as kpsim
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.supervised import TorchFK
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM), 256, 0)
    takes = D.synthetic_takes(sim, std["qpos"], n_per_action=2, T_range=(T + 5, T + 10), body_mass=read_kpm(kpsim.STEP_KPM)["body_mass"], seed=4)
    ds = D.StateARDataset(takes, fr_num=T, seed=4, device=sim.device)
    torch.manual_seed(0)
    net = TrajARNet().to(sim.device)
    kpm = read_kpm(DEFAULT_KPM)
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], sim.device, sim=sim)
    data = next(iter(P.sampling_batches(ds, 256, 256, sim.device, torch.float32)))
    fwd = kin_tape.forward_supervised_taped if path == "fused" else P.forward_supervised
    loss, _ = P.compute_loss(fwd(net, fk, data, 0.0, None, 0.0), data)
    loss.backward()
    torch.cuda.synchronize()
    print(f"{path} T={T} loss {float(loss):.4f}")


def main():
    if sys.argv[1] == "child":
        return child(sys.argv[2], int(sys.argv[3]))
    out = sys.argv[1]
    ta, tb = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (10, 30)
    for path in ("torch", "fused"):
        counts = {}
        for T in (ta, tb):
            d = os.path.join(out, f"{path}_T{T}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "stats", "--", sys.executable, os.path.abspath(__file__), "child", path, str(T)]
            subprocess.run(cmd, stdout=subprocess.DEVNULL, env=dict(os.environ, TMPDIR="/tmp"), timeout=300, check=True)
            with open(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
                counts[T] = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)}
            for big in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                os.remove(big)
        rows = []
        for name in set(counts[ta]) | set(counts[tb]):
            ca, na = counts[ta].get(name, (0, 0.0)); cb, nb = counts[tb].get(name, (0, 0.0))
            if cb != ca:
                rows.append((name, (cb - ca) / (tb - ta), (nb - na) / (tb - ta) * 1e-3))
        rows.sort(key=lambda r: -r[1])
        print(f"# {path}: {sum(r[1] for r in rows):.1f} kernel launches and {sum(r[2] for r in rows):.1f} us of device time per frame, forward + backward "
              f"(256 clips; call counts at {tb} frames minus {ta} frames, / {tb - ta})")
        for name, c, us in rows[:12]:
            print(f"{c:8.2f} {us:9.1f} us  {name[:110]}")


if __name__ == "__main__":
    main()
