#!/usr/bin/env python
"""Every output of the read-out kernels (contact_forces, inverse_dynamics, apply_impulse) on the named states of their GPU tests, written to one .npz, so
that two builds of the library can be compared bit for bit (needs a GPU):

    python tools/readout_dump.py --out this.npz                     # this tree
    python tools/readout_dump.py --root other/checkout --out other.npz
    python tools/readout_dump.py --compare this.npz other.npz       # np.array_equal on the int32 views; exit 1 and the largest deviation per array otherwise

The states, inputs and handles are those tests/test_gpu_contact_force.py, test_gpu_inverse_dynamics.py and test_gpu_push.py build (imported from --root),
at 1, 5 and 67 envs / rows: contact forces in modes 0, 1 and 2 on floor and object handles with the default and the extended controller, inverse dynamics
on the floor and sitting cases with the cases' own blocks, a parked block and none, body pushes on the six poses and object pushes on the push scene.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

SIZES = (1, 5, 67)


def dump(root: str) -> dict:
    root = os.path.abspath(root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch
    import test_gpu_contact_force as TC
    import test_gpu_inverse_dynamics as TI
    import test_gpu_push as TP
    from kinpoly_amd import sim as kp
    out = {}
    # ---- contact forces: default controller (action width 75) and the extended one (action_v + rfc + meta-PD, width 105)
    XC = dict(cc_action_v=1, cc_rfc=1, cc_meta_pd=1)
    for ctrl, opts, width in (("default", {}, 75), ("extended", XC, 69 + 6 + 30)):
        for scene in ("floor", "parked", "g_sit", "h_push"):
            base = TC.states(kp, scene)
            for n in SIZES:
                sts = [base[e % len(base)] for e in range(n)]
                sim = TC.make_sim(kp, scene, sts, **opts)
                for mode in (0, 1, 2):
                    for k, v in TC.call(sim, sts, mode, width=width).items():
                        out[f"cf/{ctrl}/{scene}/n{n}/mode{mode}/{k}"] = v
                assert int(sim.diag()[:, 2].max()) == 0
    # ---- inverse dynamics: rows of the named cases, cycled
    for scene in ("floor", "g_sit"):
        base = TI.cases(scene)
        path = TI.STEP_KPM if scene == "g_sit" else TI.DEFAULT_KPM
        for n in SIZES:
            cs = [base[e % len(base)] for e in range(n)]
            for blk in ("own", None) + (("parked",) if scene == "floor" else ()):
                sim = TI.handle(kp, TI.STEP_KPM if blk == "parked" else path)
                for k, v in TI.run(sim, cs, blk=blk).items():
                    out[f"id/{scene}/n{n}/{blk}/{k}"] = v
    # ---- pushes: every body in turn on the six poses; the two object slots of the push scene
    poses = TP.six_poses()
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        qpos, qvel = poses[np.arange(n) % 6], TP.f32(rng.normal(size=(n, 75)) * 0.5)
        imp = TP.f32(rng.normal(size=(n, 6)) * [20, 20, 20, 2, 2, 2])
        off = TP.f32(rng.uniform(-0.15, 0.15, (n, 3)))
        sim = kp.KpSim(kp.KpModel(), n)
        sim.set_state(TP.dev(qpos), TP.dev(qvel))
        dq = sim.apply_impulse(TP.dev((np.arange(n) * 7) % 24, torch.int32), TP.dev(imp), TP.dev(off), want_dqvel=True)
        out[f"push/body/n{n}/dqvel"], out[f"push/body/n{n}/qvel"] = dq.cpu().numpy(), sim.get("qvel").cpu().numpy()
    n = 5
    rng = np.random.default_rng(9)
    x, y = TP.STD["qpos"][0] + 1.2, TP.STD["qpos"][1]
    box = [TP.f32(np.concatenate([[x, y, 0.921], TP._quat(rng.normal(size=3), 0.4 * (e + 1))])) for e in range(n)]
    tab = [TP.f32(np.concatenate([[x, y, 0.7905], TP._quat(rng.normal(size=3), 0.3 * (e + 1))])) for e in range(n)]
    sim = kp.KpSim(kp.KpModel(TP.STEP_KPM), n)
    sim.set_objects(TP.dev(TP._obj_block(n, [{1: box[e], 2: tab[e]} for e in range(n)])))
    sim.set_state(TP.dev(np.tile(TP.STD["qpos"], (n, 1))), TP.dev(rng.normal(size=(n, 75)) * 0.3))
    sim.set_obj_state(sim.get("obj_qpos"), TP.dev(TP.f32(rng.normal(size=(n, 30)) * 0.2)))
    for slot in (0, 1):
        sim.apply_impulse(TP.dev([24 + slot] * n, torch.int32), TP.dev(TP.f32(rng.normal(size=(n, 6)) * [30, 30, 30, 3, 3, 3])), TP.dev(TP.f32(rng.uniform(-0.15, 0.15, (n, 3)))))
        out[f"push/object/slot{slot}/obj_qvel"] = sim.get("obj_qvel").cpu().numpy()
    out["push/object/qvel"] = sim.get("qvel").cpu().numpy()
    return out


def compare(pa: str, pb: str) -> int:
    a, b = np.load(pa), np.load(pb)
    bits = lambda v: v.view(np.int32) if v.dtype == np.float32 else v  # noqa: E731
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].shape != b[k].shape or not np.array_equal(bits(a[k]), bits(b[k]))]
    print(f"{len(a.files)} arrays in {pa}, {len(b.files)} in {pb}, {len(bad)} differ")
    for k in bad:
        both = k in a.files and k in b.files and a[k].shape == b[k].shape
        print(f"  {k}: " + (f"max |a - b| {np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max():.3e} on max |a| {np.abs(a[k]).max():.3e}" if both else "missing or another shape"))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose library and tests are used")
    ap.add_argument("--out", default=None, help="the .npz to write")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps and exit")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out or --compare is needed")
    arrays = dump(a.root)
    np.savez(os.path.abspath(a.out), **arrays)
    print(f"{len(arrays)} arrays -> {a.out}")


if __name__ == "__main__":
    main()
