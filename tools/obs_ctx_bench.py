#!/usr/bin/env python
"""The wide observation launch (kp_sim_obs_ar_ex: k_obs_ar_ctx writes [context | base | of] in one launch) against the composition it replaces
(kp_sim_obs_ar + torch.cat of the frame's context slab, the base row and the frame's `of` rows), at 4096 rows, rnn_hdim 256, `of` 0 and 512 wide,
the 101-d base row of scripts/exp_arnet_all.py's network.

    python tools/obs_ctx_bench.py [rows] [launches per block] [blocks]        default 4096 200 5
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/obs_ctx_bench.py          per-kernel device times (k_obs_ar_ctx; k_obs_ar_thread + the cat's copy kernel)

Prints per form the median and min .. max over the blocks of the device time per launch (hip events around a block), alternating the two forms, and whether
the wide launch stays by the rule: its median at most the composition's median plus the composition's own max - min."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kinpoly_amd import sim as kpsim  # noqa: E402


def main():
    args = [int(a) for a in sys.argv[1:]]
    n, per, blocks = (args + [4096, 200, 5][len(args):])[:3]
    T, H = 100, 256
    torch.cuda.set_device(0)
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    sim = kpsim.KpSim(kpsim.KpModel(kpsim.STEP_KPM, **kpsim.ar_obs_options(False, True, False)), n, 0)
    sim.set_state(torch.tensor(std["qpos"], dtype=torch.float32, device="cuda").repeat(n, 1).contiguous(), torch.zeros((n, 75), device="cuda"))
    r = lambda *s: torch.randn(s, device="cuda")      # noqa: E731
    one_hot = torch.zeros((n, 4), device="cuda"); one_hot[:, 0] = 1
    cur_t = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx = sim.make_ctx(T, r(n, T, 7), r(n, T, 6), r(n, T, 7), one_hot, torch.zeros((n, T, 96), device="cuda"), torch.zeros((n, T, 72), device="cuda"), cur_t, obj_qpos=r(n, 7))
    seq = r(T, n, H)
    for F in (0, 512):
        of = r(n, T, F) if F else None
        ext = sim.make_obs_ext(T, n, H, seq, of)
        out = torch.empty((n, H + sim.obs_ar_dim + F), device="cuda")
        base = torch.empty((n, sim.obs_ar_dim), device="cuda")
        wide = lambda: sim.obs_ar_ex(ctx, ext, out=out)      # noqa: E731
        comp = lambda: torch.cat([seq[7], sim.obs_ar(ctx, out=base)] + ([of[:, 7]] if F else []), 1)      # noqa: E731
        assert torch.equal(wide(), comp())
        times = {"wide": [], "composition": []}
        for f in (wide, comp):
            for _ in range(20):
                f()
        for _ in range(blocks):
            for name, f in (("wide", wide), ("composition", comp)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    f()
                e1.record(); torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / per)
        w, c = np.array(times["wide"]), np.array(times["composition"])
        print(json.dumps({"rows": n, "H": H, "F": F, "row_floats": H + sim.obs_ar_dim + F,
                          "wide_us": [round(float(np.median(w)), 2), round(float(w.min()), 2), round(float(w.max()), 2)],
                          "composition_us": [round(float(np.median(c)), 2), round(float(c.min()), 2), round(float(c.max()), 2)],
                          "wide_stays": bool(np.median(w) <= np.median(c) + (c.max() - c.min()))}), flush=True)


if __name__ == "__main__":
    main()
