"""Batched evaluation roll-outs: `run_seq` / `test_coverage` (here `run_sequences` / `write_coverage`) of scripts/eval_ar_policy.py:178-262 for N sequences at once.

Every environment plays one sequence with the mean action of the kinematic policy (test mode => mean UHC action too); the
per-sequence record has the reference's keys (`target`, `pred`, `obj_pose`, `percent`, `fail_safe`) so that the reference's
metric script (eval_pose_all.py) reads the `*_coverage_full.pkl` this writes.  With `fail_safe` a sequence that terminates
early is put back on the kinematic roll-out (`env.ar_fail_safe`) and continues, exactly as the reference does.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .contact import ground_reaction

GRF_KEYS = ("grf", "cop", "foot_contact", "load")


def _grf_frame(env):
    """what grf=True records after an env step: the feet's ground reaction from the contact-force read-out of the state the step left (controller = the
    step's own action): grf [N,2,3], cop [N,2,2], foot_contact [N,2] bool, load [N,26] = |force| per entity"""
    w = env.contact_forces(want=("wrench",))["wrench"]
    g = ground_reaction(w)
    return {"grf": g["force"], "cop": g["cop"], "foot_contact": g["support"], "load": w[..., :3].norm(dim=-1)}


def _grf_result(frames, steps, e):
    """the recorded frames of env e at its running steps: {key: array [T, ...]}"""
    return {k: np.stack([frames[t][k][e] for t in steps]) if len(steps) else np.zeros((0,) + frames[0][k].shape[1:], frames[0][k].dtype) for k in GRF_KEYS}



@torch.no_grad()
def run_sequences(env, policy_net, keys, fail_safe=False, max_steps=100000, push_schedule=None, grf=False):
    """env: BatchedHumanoidAREnv with its context loaded (one sequence per env, mode 'test').  Returns {key: seq_result}.
    push_schedule (kinpoly_amd.push.PushSchedule for env.n envs): the env pushes its humanoids while the sequences play; a recording schedule gets the
    pushes of every sequence in its by_take.
    grf: after every env step also record, for the sequences still running, grf [T,2,3] (L, R foot), cop [T,2,2], foot_contact [T,2] bool and
    load [T,26] = |contact force| per entity (env.contact_forces); T = the sequence's recorded length.  Off: the result is what it always was."""
    if push_schedule is not None:
        return _with_pushes(env, push_schedule, lambda: run_sequences(env, policy_net, keys, fail_safe, max_steps, grf=grf), keys)
    n = env.n
    if fail_safe and "ar_qpos" not in env.ctx:            # checked once, up front: the fail-safe runs (masked) every step, whether or not an env ended early
        raise ValueError("run_sequences(fail_safe=True) needs the kinematic roll-out in the context (ctx['ar_qpos'] / ['ar_qvel']: PolicyARContext(need_rollout=True))")
    env.set_mode("test")
    obs = env.reset()
    hx = policy_net.init_hidden(n, env.device)
    active = torch.ones(n, dtype=torch.bool, device=env.device)
    used_fs = torch.zeros(n, dtype=torch.bool, device=env.device)
    percent = torch.zeros(n, device=env.device)
    rec = {"target": [], "pred": [], "obj_pose": [], "active": []}
    frames = []
    for step in range(max_steps):
        rec["target"].append(env.sim.get("target_qpos")); rec["pred"].append(env.get_humanoid_qpos())
        rec["obj_pose"].append(env.obj_qpos); rec["active"].append(active.clone())
        action, hx = policy_net.select_action(obs, hx, True, env.gen)
        obs, _, done, info = env.step(action.contiguous())
        if grf:
            frames.append(_grf_frame(env))
        newly = done & active
        percent = torch.where(newly, info["percent"], percent)
        early = newly & (info["percent"] != 1)
        if fail_safe:                               # masked on the device (no host read per step): envs that ended early go back onto the kinematic roll-out
            used_fs |= early
            env.ar_fail_safe(early)
            obs = env._obs_ar(env._obs)
            newly = newly & ~early
        active = active & ~newly
        if step % 8 == 7 and not bool(active.any()):      # one host read every 8 steps; the records of finished envs are dropped by `active` below
            break
    act = torch.stack(rec["active"], 0).cpu().numpy()                       # [steps, n]
    env._played = act
    tgt = torch.stack(rec["target"], 0).double().cpu().numpy(); pred = torch.stack(rec["pred"], 0).double().cpu().numpy()
    parked = np.zeros(35); parked[0::7] = [100.0 * (i + 1) for i in range(5)]; parked[1::7] = 100.0
    objs = None if rec["obj_pose"][0] is None else torch.stack(rec["obj_pose"], 0).double().cpu().numpy()
    frames = [{k: v.cpu().numpy() for k, v in f.items()} for f in frames]
    out = {}
    for e, key in enumerate(keys):
        steps = np.nonzero(act[:, e])[0]
        out[key] = {"target": [tgt[t, e] for t in steps], "pred": [pred[t, e] for t in steps],
                    "obj_pose": [(objs[t, e] if objs is not None else parked.copy()) for t in steps],
                    "percent": float(percent[e]), "fail_safe": bool(used_fs[e])}
        if grf:
            out[key].update(_grf_result(frames, steps, e))
    return out


@torch.no_grad()
def _with_pushes(env, schedule, play, keys):
    """play() with the schedule installed in env; afterwards the env is as it was and a recording schedule holds the pushes of `keys`"""
    first = 0 if schedule.log is None else len(schedule.log)
    before, env.push_schedule = env.push_schedule, schedule
    try:
        out = play()
    finally:
        env.push_schedule = before
    if schedule.log is not None:
        schedule.collect(first, env._played, [k for k in keys if not str(k).startswith("__fill_")])
    return out


@torch.no_grad()
def eval_dataset(env, policy_net, ctx_builder, dataset, fail_safe=False, inds=None, push_schedule=None, grf=False):
    """`eval_seq` for every take of a data set (agent_ar.py:463-503; eval_ar_policy.py's run_seq loop :178-262), env.n takes at a time: each
    env plays one WHOLE take (`get_seq_by_ind(ind, full_sample=True)`), takes of different length share a batch padded to its longest
    (`ctx['len']` ends every env on its own last frame; init_context averages every row's context over its own frames).  ctx_builder:
    PolicyARContext (its kinematic twin may hold any number of rows: other batch sizes go through it in chunks); the kinematic roll-out is
    computed (need_rollout=True: the fail-safe and ar_mode read it).  Returns {take name: seq_result} in the data set's order."""
    inds = list(range(dataset.get_len())) if inds is None else [int(i) for i in inds]
    out = {}
    for i in range(0, len(inds), env.n):
        chunk = inds[i:i + env.n]
        rows = chunk + [chunk[-1]] * (env.n - len(chunk))                  # a short last chunk is filled with copies of its last take
        data = dataset.batch(np.asarray(rows, np.int64), None, None)
        data = {k: (v.to(env.device) if torch.is_tensor(v) else v) for k, v in data.items()}
        ctx = ctx_builder.init_context(data, need_rollout=True)
        env.load_context(ctx)
        keys = [dataset.takes[j] for j in chunk] + [f"__fill_{j}" for j in range(env.n - len(chunk))]
        res = run_sequences(env, policy_net, keys, fail_safe=fail_safe, push_schedule=push_schedule, grf=grf)
        out.update({k: res[k] for k in keys[:len(chunk)]})
    return out


def write_coverage(results: dict, result_dir: str, iter_num: int, data_file: str):
    """Write `<iter>_<data_file>_coverage.pkl` / `_coverage_full.pkl` (eval_ar_policy.py:225-262); returns the coverage count."""
    import joblib
    cov = {k: {"percent": r["percent"], "values": r.get("values", []), "fail_safe": r["fail_safe"]} for k, r in results.items()}
    coverage = sum(1 for r in results.values() if r["percent"] == 1 and not r["fail_safe"])
    os.makedirs(result_dir, exist_ok=True)
    joblib.dump(cov, os.path.join(result_dir, f"{iter_num:04d}_{data_file}_coverage.pkl"))
    joblib.dump(results, os.path.join(result_dir, f"{iter_num:04d}_{data_file}_coverage_full.pkl"))
    return coverage


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The UHC's own evaluation: run_seq / test_coverage of the reference's scripts/eval_uhc.py:158-241 (and AgentCopycat.eval_seq,
# uhc/core/agent_copycat.py:101-131), env.n takes at a time on a take library (BatchedHumanoidEnv.load_takes).

@torch.no_grad()
def run_uhc_sequences(env, policy_net, running_state, take_ids, keys, fail_safe=False, max_steps=100000, push_schedule=None, grf=False):
    """Every env plays one WHOLE take (take_ids [env.n], library ids) with the mean action and running_state(update=False).  Per step, before the
    action: gt = the expert's qpos at get_expert_index(t), pred = the simulated qpos (eval_uhc.py:175-178; on a library with objects env.data.qpos is
    the full 111-wide row, so pred = [qpos 76 | object block 35] while gt stays 76 wide).  An env that ends early (percent != 1) is,
    with fail_safe, put back on the expert and goes on (:188-196); without it the episode is over.  Returns {key: {gt, pred, percent, fail_safe}}
    for the first len(keys) envs.  push_schedule, grf: as in run_sequences."""
    if push_schedule is not None:
        return _with_pushes(env, push_schedule, lambda: run_uhc_sequences(env, policy_net, running_state, take_ids, keys, fail_safe, max_steps, grf=grf), keys)
    n, dev, lib = env.n, env.device, env.takes
    norm = (lambda o: running_state(o, update=False)) if running_state is not None else (lambda o: o)
    everyone = torch.ones(n, dtype=torch.bool, device=dev)
    obs = norm(env.reset(everyone, take_ids=np.ascontiguousarray(take_ids, np.int32)))
    off, lens = torch.as_tensor(lib.take_off[:-1].astype(np.int64), device=dev), torch.as_tensor(lib.lens.astype(np.int64), device=dev)
    qtab = lib.table("qpos")
    active = everyone.clone()
    used_fs = torch.zeros(n, dtype=torch.bool, device=dev)
    percent = torch.zeros(n, device=dev)
    gt, pred, act, frames = [], [], [], []
    for step in range(max_steps):
        k = env.take_id.long()
        row = off[k] + torch.minimum(env.start_ind.long() + env.cur_t.long(), lens[k] - 1)
        gt.append(qtab[row]); act.append(active.clone())
        pred.append(torch.cat([env.sim.get("qpos"), env.sim.get("obj_qpos")], 1) if lib.has_objects else env.sim.get("qpos"))
        a = policy_net.select_action(obs, True, env.gen).contiguous()
        obs, _, done, info = env.step(a)
        if grf:
            frames.append(_grf_frame(env))
        newly = done & active
        percent = torch.where(newly, info["percent"], percent)
        if fail_safe:                               # masked on the device: no host read per step
            early = newly & (info["percent"] != 1)
            used_fs |= early
            obs = env.fail_safe(early)
            newly = newly & ~early
        active = active & ~newly
        obs = norm(env.reset(done & ~active))       # a finished env waits on its take's first frame; its records are dropped by `active`
        if step % 8 == 7 and not bool(active.any()):
            break
    act = env._played = torch.stack(act, 0).cpu().numpy()
    gt, pred = torch.stack(gt, 0).double().cpu().numpy(), torch.stack(pred, 0).double().cpu().numpy()
    frames_np = [{k: v.cpu().numpy() for k, v in f.items()} for f in frames]
    out = {}
    for e, key in enumerate(keys):
        steps = np.nonzero(act[:, e])[0]
        out[key] = {"gt": [gt[t, e] for t in steps], "pred": [pred[t, e] for t in steps], "percent": float(percent[e]), "fail_safe": bool(used_fs[e])}
        if grf:
            out[key].update(_grf_result(frames_np, steps, e))
    return out


@torch.no_grad()
def eval_uhc_takes(env, policy_net, running_state, dataset, fail_safe=False, inds=None, library=None, push_schedule=None, grf=False):
    """test_coverage's loop (eval_uhc.py:202-224) over the takes of an AmassSingleDataset or SmplObjDataset, env.n at a time; a short last chunk is padded with copies of
    its last take.  Loads the data set's library into env (library: one already built with env.sim).  Returns {take name: seq_result} in data-set order."""
    lib = library if library is not None else dataset.to_library(env.sim)
    env.load_takes(lib)
    inds = list(range(dataset.get_len())) if inds is None else [int(i) for i in inds]
    out = {}
    for i in range(0, len(inds), env.n):
        chunk = inds[i:i + env.n]
        ids = chunk + [chunk[-1]] * (env.n - len(chunk))
        out.update(run_uhc_sequences(env, policy_net, running_state, ids, [dataset.data_keys[j] for j in chunk], fail_safe=fail_safe, push_schedule=push_schedule, grf=grf))
    return out


def write_uhc_coverage(results: dict, output_dir: str, iter_num: int, data: str, no_full=False):
    """`<iter>_<data>_coverage.pkl` ({take: {percent}}) and, unless no_full, `<iter>_<data>_coverage_full.pkl` (eval_uhc.py:225-241: the iteration is
    not zero-padded there, unlike write_coverage's).  Returns the coverage count (percent == 1 and no fail-safe)."""
    import joblib
    os.makedirs(output_dir, exist_ok=True)
    joblib.dump({k: {"percent": r["percent"]} for k, r in results.items()}, os.path.join(output_dir, f"{iter_num}_{data}_coverage.pkl"))
    if not no_full:
        joblib.dump(results, os.path.join(output_dir, f"{iter_num}_{data}_coverage_full.pkl"))
    return sum(1 for r in results.values() if r["percent"] == 1 and not r["fail_safe"])
