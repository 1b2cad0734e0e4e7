"""Record how kp_model_set_option / kp_model_get_option answer, for tests/golden/model_options.json (needs no GPU).

The fixture is the answer of the build it was taken from and pins every later build to it (tests/test_host_cpu.py replays it), so it is
recorded on the commit BEFORE a change of the option code, never on the code under test:

    python tools/gen_model_options.py --library <that build's libkinpoly_sim.so> [--force]

Without --force an existing fixture is left alone.  For every option name: the read-back of a fresh default-blob model; then, each on a fresh
model, for every probe value the return code of set, the option's read-back afterwards, the read-backs of job_auto / ar_obs_dim / cc_obs_dim /
cc_action_dim, and the error text of a refusal; plus a set and a get of an unknown name.  All probes stay below 2^31 (the library casts with
(int)v, which is undefined beyond it)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "model_options.json")
KPM = os.path.join(ROOT, "kinpoly_amd", "assets", "smpl_humanoid.kpm")

SETTABLE = ["contact", "limits", "gravity_z", "gravity_x", "gravity_y", "actuation", "ar_obs_action", "cc_action_v", "cc_rfc", "cc_meta_pd", "cc_obs_v",
            "cc_obs_vel_root", "cc_obs_heading", "cc_obs_deheading", "cc_obs_phase", "stale_kinematics", "solver_iter", "solver_tol", "dynamic_objects",
            "planemesh_max", "planemesh_tol", "lpt_order", "job_taper", "queue_fence", "queue_heavy", "queue_late", "queue_prio", "warm_extrap",
            "lean_queue", "lean_adaptive", "lean_max_contacts", "lds_pad", "queue_slots", "substeps_per_job", "threads_per_env"]
READ_ONLY = ["ar_obs_dim", "cc_obs_dim", "cc_action_dim", "n_obj_geoms", "lds_bytes_per_env_lean", "job_auto", "timestep", "lds_bytes_per_env",
             "lds_bytes_per_env_objects"]
PROBES = [-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 8.0, 9.0, 16.0, 64.0, 128.0, 255.0, 256.0, 65536.0, 65537.0, 1e9]
DERIVED = ["job_auto", "ar_obs_dim", "cc_obs_dim", "cc_action_dim"]
UNKNOWN = "no_such_option"


def num(x):
    """JSON has no NaN: it is written as the string "nan" """
    return "nan" if math.isnan(x) else x


def load(path):
    L = C.CDLL(path)
    L.kp_model_load.restype = C.c_void_p; L.kp_model_load.argtypes = [C.c_char_p]
    L.kp_model_free.argtypes = [C.c_void_p]
    L.kp_model_set_option.restype = C.c_int; L.kp_model_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.kp_model_get_option.restype = C.c_double; L.kp_model_get_option.argtypes = [C.c_void_p, C.c_char_p]
    L.kp_last_error.restype = C.c_char_p
    return L


def probe(L, name, v):
    """set `name` to v on a fresh model: {v, rc, value, job_auto, ar_obs_dim, cc_obs_dim, cc_action_dim, error}"""
    m = L.kp_model_load(KPM.encode())
    assert m, L.kp_last_error()
    rc = L.kp_model_set_option(m, name.encode(), v)
    r = {"v": v, "rc": rc, "value": num(L.kp_model_get_option(m, name.encode())), "error": L.kp_last_error().decode() if rc else None}
    for d in DERIVED:
        r[d] = num(L.kp_model_get_option(m, d.encode()))
    L.kp_model_free(m)
    return r


def record(L):
    m = L.kp_model_load(KPM.encode())
    assert m, L.kp_last_error()
    defaults = {k: num(L.kp_model_get_option(m, k.encode())) for k in SETTABLE + READ_ONLY}
    L.kp_model_free(m)
    out = {"blob": "kinpoly_amd/assets/smpl_humanoid.kpm", "options": {}}
    for k in SETTABLE + READ_ONLY:
        vals = list(PROBES)
        if k == "lean_max_contacts":      # the lean layout's own cap (the default) and one beyond it
            vals += [defaults[k], defaults[k] + 1.0]
        out["options"][k] = {"default": defaults[k], "settable": k in SETTABLE, "probes": [probe(L, k, v) for v in vals]}
    out["unknown"] = probe(L, UNKNOWN, 1.0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--library", required=True, help="the libkinpoly_sim.so to record (the parent commit's build)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--force", action="store_true", help="overwrite an existing fixture")
    a = ap.parse_args()
    if os.path.exists(a.out) and not a.force:
        sys.exit(f"{a.out} exists: it is the parent build's answer; pass --force only to re-record it on a parent build")
    with open(a.out, "w") as f:
        json.dump(record(load(a.library)), f, indent=1)
        f.write("\n")
    print(a.out)
