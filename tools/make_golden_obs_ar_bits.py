#!/usr/bin/env python
"""Pin kp_sim_obs_ar's 105- and 101-wide rows bit for bit: tests/golden/obs_ar_parent_bits.npz holds the inputs (the stored state rows the kernel reads and
a context table) and the uint32 views of the rows a build wrote for them.  It was run once, on the commit before kp_sim_obs_ar's dispatch became one table
(the one-thread-per-env kernel wrote both layouts), so that whatever kernel the table launches for them is held to those words
(tests/test_gpu_obs_variants.py); running it again pins whatever the current build computes.  Needs the GPU.

67 envs (eight full blocks of the 8-envs-per-block mapping and a partial block of 3), a context table of 72 rows of 6 frames.  Among the rows: cur_t below
0, at T - 1 and above T - 1; a row map that is a non-identity permutation with repeats; context rows whose one-hot is all zero; root quaternions with
negative w; every layout once with an obj_qpos pointer and once with a null one (the non-zero one-hots then fall back to the identity pose).

    python tools/make_golden_obs_ar_bits.py [--out FILE]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kinpoly_amd import sim as kp  # noqa: E402

N, T, R = 67, 6, 72


def unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_inputs():
    rng = np.random.default_rng(67)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    std = np.load(os.path.join(ROOT, "tests", "golden", "standing_neutral.npz"))
    q = np.tile(std["qpos"].astype(np.float64), (N, 1))
    q[:, :2] += rng.normal(size=(N, 2)); q[:, 2] += rng.normal(size=N) * 0.1
    q[:, 3:7] = unit(rng.normal(size=(N, 4)))
    q[:, 3] = np.where(np.arange(N) % 3 == 0, -np.abs(q[:, 3]), np.abs(q[:, 3]))          # every third root quaternion has negative w
    q[:, 7:] += rng.normal(size=(N, 69)) * 0.4
    stale = q.copy(); stale[:, 7:] += rng.normal(size=(N, 69)) * 0.05                      # the kinematics the kernel reads are one substep old
    fk = kp.KpSim(kp.KpModel(), N).fk(torch.tensor(f32(stale), device="cuda"))
    row = rng.permutation(R)[:N].astype(np.int32)
    row[5], row[40], row[66] = row[4], row[4], row[0]                                       # repeats
    oh = np.zeros((R, 4), np.float32)
    for r in range(R):
        if r % 5 < 4:
            oh[r, r % 5] = 1.0                                                              # each action, and the all-zero one-hot
    g = dict(qpos=f32(q), xpos=fk["wbpos"].cpu().numpy(), xquat=fk["wbquat"].cpu().numpy(),
             head_pose=f32(np.concatenate([rng.normal(size=(R, T, 3)), unit(rng.normal(size=(R, T, 4)))], -1)), head_vels=f32(rng.normal(size=(R, T, 6))),
             obj_rel=f32(rng.normal(size=(R, T, 7))), action_one_hot=oh,
             obj_qpos=f32(np.concatenate([q[:, :3] + rng.normal(size=(N, 3)) * 0.5, unit(rng.normal(size=(N, 4)))], -1)), row=row,
             cur_t=np.asarray([-2, 0, 1, T - 2, T - 1, T + 3], np.int32)[np.arange(N) % 6])
    assert (g["qpos"][:, 3] < 0).any() and len(set(row)) < N and not (row == np.arange(N)).all() and (oh[row].sum(1) == 0).any() and (oh[row].sum(1) != 0).any()
    return g


def obs_ar_words(g, n, action, with_obj):
    """the first n envs of the stored inputs through kp_sim_obs_ar on a handle of n envs: the rows as uint32 [n, 105 or 101]"""
    sim = kp.KpSim(kp.KpModel(**kp.ar_obs_options(use_action=action)), n)
    dev = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    for k in ("qpos", "xpos", "xquat"):
        sim.view(k).copy_(torch.from_numpy(g[k][:n]))
    z = torch.zeros((R, T, 96), device="cuda")
    ctx = sim.make_ctx(T, dev(g["head_pose"]), dev(g["head_vels"]), dev(g["obj_rel"]), dev(g["action_one_hot"]), z, z[:, :, :72].contiguous(), dev(g["cur_t"][:n]),
                       obj_qpos=dev(g["obj_qpos"][:n]) if with_obj else None, row=dev(g["row"][:n]))
    out = sim.obs_ar(ctx)
    assert tuple(out.shape) == (n, 105 if action else 101)
    return out.cpu().numpy().view(np.uint32)


def main():
    out = os.path.join(ROOT, "tests", "golden", "obs_ar_parent_bits.npz")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    g = make_inputs()
    for action in (True, False):
        for with_obj in (True, False):
            g[f"bits_{105 if action else 101}{'' if with_obj else '_null_obj'}"] = obs_ar_words(g, N, action, with_obj)
    assert not np.array_equal(g["bits_105"], g["bits_105_null_obj"])
    np.savez_compressed(out, **g)
    print(out, os.path.getsize(out), {k: (v.shape, str(v.dtype)) for k, v in g.items()})


if __name__ == "__main__":
    main()
