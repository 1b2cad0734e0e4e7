"""Write tests/golden/uhc_take_edges.npz: what the reference's own get_expert (uhc/utils/tools.py:20-85) computes on the edge takes of tests/take_edges.py,
fed rows_for_reference(rows) (the fp32 values of the rows, the root quaternion renormalised in fp64), on the scaffolding of tools/make_golden_uhc_takes.py:
a HumanoidEnv of a reference checkout whose sim.forward() is this repository's fp64 oracle.  All nine takes at env.frame_skip = 15 (dt = 1 / 30 s), the five
edge takes again at env.frame_skip = 450 (dt = 1 s, where the +-10 clamp no longer hides the size of a wrapped velocity).  Arrays and names only:
rows, take_off, take_names, dts (the doubles env.dt reported), and per dt index i and take `d{i}_{take}_{table}` for the tables of take_edges.DERIVED and
the two minima.

    python tools/make_golden_take_edges.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from make_golden_uhc_takes import reference_env  # noqa: E402
import take_edges as E  # noqa: E402


def main():
    rows, take_off = E.build()
    ref = E.rows_for_reference(rows)
    sl = E.take_slice(take_off)
    out = {"rows": rows, "take_off": take_off, "take_names": np.array(E.NAMES)}
    dts = []
    for di, (frame_skip, names) in enumerate(((15, E.NAMES), (450, E.EDGE))):
        _, env, _, _ = reference_env(frame_skip)
        from uhc.utils.tools import get_expert
        dts.append(float(env.dt))
        for name in names:
            ex = get_expert(ref[sl[name]].copy(), {"cyclic": False, "seq_name": name}, env)
            for t in E.DERIVED:
                out[E.fixture_key(di, name, t)] = np.asarray(ex[t], np.float64)
            out[E.fixture_key(di, name, "height_lb")], out[E.fixture_key(di, name, "head_height_lb")] = np.float64(ex["height_lb"]), np.float64(ex["head_height_lb"])
    out["dts"] = np.array(dts, np.float64)
    path = os.path.join(ROOT, "tests", "golden", "uhc_take_edges.npz")
    np.savez_compressed(path, **out)
    print("dt =", dts, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
