"""The data formats either side of the rollout path: the per-take feature file the reference trains from
(`<data_dir>/features/<data_file>.p`, a joblib dict  take -> {qpos, qvel, head_pose, head_vels, obj_pose,
obj_head_relative_poses, action_one_hot, wbpos, wbquat, bquat, of_files, ...}, written by
kin_poly/data_process/process_smpl.py:140-235) and the sampler that serves clips from it
(kin_poly/data_loaders/statear_smpl_dataset.py), here batched: N episodes per call instead of one.

    build_take_features   process_smpl.post_process_expert on top of the batched get_expert (one FK launch per take)
    StateARDataset        preprocess_data (derived `target` trajectory), sample_seq x N -> [N, fr_num, .] tensors,
                          adaptive take sampling (freq_dict / ewma), get_seq_by_ind / iter_seq, padded ragged batches
    synthetic_takes       SURVEY.md section 8(d) config 4 stand-in for the absent MoCap set, in the same schema
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .context import heading_q, quat_acos_w, quat_inv, quat_mul, quat_rotate_t, quat_sin_half, quat_small

ACTIONS = ("sit", "push", "avoid", "step")             # cfg.all_actions order = action_one_hot columns
TRAIN_KEYS = ("wbpos", "wbquat", "bquat")


# ------------------------------------------------------------------ feature construction (torch, any device, any float dtype)
def _fd_vel(cur7, nxt7, dt):
    """get_head_vel / get_root_vel body (process_smpl.py:30-55, statear_smpl_dataset.py:186-214): linear velocity in the
    heading frame, angular velocity (axis * angle / dt, angle wrapped once) in the root frame; [T-1, 6]."""
    v = quat_rotate_t(heading_q(cur7[:, 3:7]), (nxt7[:, :3] - cur7[:, :3]) / dt)
    qrel = quat_mul(nxt7[:, 3:7], quat_inv(cur7[:, 3:7]))
    w = qrel[:, 0]
    small = quat_small(qrel)                          # 1 - |w| < 1e-8, sqrt(1 - w^2), acos(w): in the forms that keep a slow turn's digits in fp32
    s = quat_sin_half(qrel).clamp_min(1e-30)
    angle = torch.where(small, torch.zeros_like(w), 2 * quat_acos_w(qrel))
    axis = torch.where(small[:, None], torch.tensor([1.0, 0.0, 0.0], device=w.device, dtype=w.dtype).expand_as(qrel[:, 1:]), qrel[:, 1:] / s[:, None])
    angle = torch.where(angle > math.pi, angle - 2 * math.pi, angle)
    rv = quat_rotate_t(cur7[:, 3:7], axis * angle[:, None] / dt)
    return torch.cat([v, rv], 1)


def get_head_vel(pose7, dt=1.0 / 30.0):
    v = _fd_vel(pose7[:-1], pose7[1:], dt)
    return torch.cat([v, v[-1:]], 0)


def get_obj_relative_pose(obj_poses, ref_poses, num_objs=1):
    """process_smpl.py:110-135: object position in the reference's heading frame + heading^-1 (x) object quaternion."""
    qh = heading_q(ref_poses[:, 3:7])
    out = []
    for o in range(num_objs):
        out.append(quat_rotate_t(qh, obj_poses[:, 7 * o:7 * o + 3] - ref_poses[:, :3]))
        out.append(quat_mul(quat_inv(qh), obj_poses[:, 7 * o + 3:7 * o + 7]))
    return torch.cat(out, 1)


def get_traj_de_heading(qpos):
    """statear_smpl_dataset.py:153-181 with cfg.has_z: qpos[2:] with the root quaternion de-headed."""
    t = qpos[:, 2:].clone()
    t[:, 1:5] = quat_mul(quat_inv(heading_q(qpos[:, 3:7])), qpos[:, 3:7])
    return t


def build_take_features(sim, qpos, obj_pose=None, action: str | None = None, body_mass=None, dt=1.0 / 30.0) -> dict:
    """One take of the feature file from its qpos clip [T, 76] (+ object poses [T, 7k]): get_expert features, then
    post_process_expert (process_smpl.py:137-152, 217-226).  Returns numpy float64 arrays like the reference's file."""
    from .uhc_env import get_expert_batch
    q = torch.as_tensor(np.asarray(qpos), dtype=torch.float32)
    T = q.shape[0]
    mass = body_mass if body_mass is not None else torch.ones(24)
    ex = get_expert_batch(sim, q[None], torch.as_tensor(mass, dtype=torch.float32, device=sim.device), dt)
    out = {k: ex[k][0].double().cpu().numpy() for k in ("qpos", "qvel", "wbpos", "wbquat", "bquat", "head_pose", "body_com", "com", "ee_pos", "ee_wpos", "bangvel", "rq_rmh")}
    out["qpos"] = np.asarray(qpos, np.float64)
    if obj_pose is None:
        obj = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (T, 1)); one_hot = np.zeros((T, 4))
    else:
        obj = np.asarray(obj_pose, np.float64); one_hot = np.zeros((T, 4)); one_hot[:, ACTIONS.index(action)] = 1.0
    nobj = obj.shape[1] // 7
    hp, ob = torch.as_tensor(out["head_pose"]), torch.as_tensor(obj)
    out.update(obj_pose=obj, action_one_hot=one_hot, action=action or "none", head_vels=get_head_vel(hp, dt).numpy(),
               obj_head_relative_poses=get_obj_relative_pose(ob, hp, nobj).numpy(),
               obj_root_relative_poses=get_obj_relative_pose(ob, torch.as_tensor(out["qpos"][:, :7]), nobj).numpy(),
               of_files=[f"{i:05d}.npy" for i in range(T)], len=T)
    return out


def write_features(path, takes: dict):
    import joblib
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    joblib.dump(takes, path)


# ------------------------------------------------------------------ the dataset
class StateARDataset:
    KEYS = ("qvel", "target", "qpos", "head_vels", "head_pose", "action_one_hot", "obj_head_relative_poses", "obj_pose")

    def __init__(self, features, takes=None, data_mode="train", fr_num=100, wild=False, dt=1.0 / 30.0, seed=0, device="cpu", of_features=None):
        """of_features (`use_of`): <dataset_path>/features/<of_file>.p or its content, a dict take -> [T, F] of per-frame image features
        (statear_smpl_dataset.py:87-90, 286, 369); batches then carry data['of'] [n, T, F], gathered like every other key.  F is the file's: every
        take must have the same, and as many frames as the take."""
        if isinstance(features, (str, os.PathLike)):
            import joblib
            features = joblib.load(features)
        if isinstance(of_features, (str, os.PathLike)):
            import joblib
            of_features = joblib.load(of_features)
        self.of_dim = 0
        self.rng = np.random.RandomState(seed)
        self.data_mode, self.fr_num, self.dt, self.wild, self.device = data_mode, int(fr_num), dt, wild, torch.device(device)
        self.takes, self.data = [], {k: [] for k in self.KEYS + (TRAIN_KEYS if data_mode == "train" and not wild else ())}
        for take in (takes if takes is not None else sorted(features)):
            e = features[take]
            q = torch.as_tensor(np.asarray(e["qpos"]), dtype=torch.float64)
            if data_mode == "train" and q.shape[0] < self.fr_num and not wild:
                continue                                        # :100-102
            assert len(e["of_files"]) == q.shape[0]
            if of_features is not None:
                if take not in of_features:
                    raise ValueError(f"StateARDataset: take '{take}' is absent from the of features")
                of = torch.as_tensor(np.asarray(of_features[take]), dtype=torch.float32)
                if of.dim() != 2 or of.shape[0] != q.shape[0]:
                    raise ValueError(f"StateARDataset: the of features of take '{take}' have shape {tuple(of.shape)}, the take has {q.shape[0]} frames")
                if self.of_dim and of.shape[1] != self.of_dim:
                    raise ValueError(f"StateARDataset: the of features of take '{take}' are {of.shape[1]} wide, those of '{self.takes[0]}' {self.of_dim}")
                self.of_dim = int(of.shape[1])
                self.data.setdefault("of", []).append(of)
            target = torch.cat([get_traj_de_heading(q), torch.cat([_fd_vel(q[:-1, :7], q[1:, :7], dt)] + [_fd_vel(q[-2:-1, :7], q[-1:, :7], dt)], 0)], 1)
            row = dict(qvel=e["qvel"], target=target, qpos=q, head_vels=e["head_vels"], head_pose=e["head_pose"], action_one_hot=e["action_one_hot"],
                       obj_head_relative_poses=np.asarray(e["obj_head_relative_poses"])[:, :7], obj_pose=e["obj_pose"])
            for k in self.data:
                if k == "of":
                    continue
                v = row[k] if k in row else e[k]
                v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32)
                if k == "obj_pose" and v.shape[1] < 14:       # one width for every take (push carries two objects): zero-padded, the env
                    v = torch.cat([v, torch.zeros((v.shape[0], 14 - v.shape[1]))], 1)      # reads only the action's slice (convert_obj_qpos)
                self.data[k].append(v)
            self.takes.append(take)
        self.freq_indices = np.array([i for i, q in enumerate(self.data["qpos"]) for _ in range(int(np.ceil(q.shape[0] / self.fr_num)))])
        self.all_indices = list(range(len(self.takes)))
        self.traj_dim = self.data["target"][0].shape[1] if self.takes else 0
        self.counter = 0

    def get_len(self):
        return len(self.takes)

    def get_seq_len(self, ind):
        return self.data["qpos"][ind].shape[0]

    def get_seq_key(self, ind):
        return self.takes[ind]

    def _slice(self, ind, start, end):
        return {k: v[ind][start:end] for k, v in self.data.items()}

    def take_probs(self, freq_dict, sampling_temp=0.5):
        """:281-286: exp(-ewma(success history) / T), normalised; takes without history get ewma 0.  The reference's recursion
        avg <- alpha x_i + (1 - alpha) avg from avg = x_0 in closed form: (1 - alpha)^(n-1) x_0 + sum_i>0 alpha (1 - alpha)^(n-1-i) x_i."""
        alpha = 0.05
        e = np.zeros(len(freq_dict))
        for j, k in enumerate(freq_dict):
            h = freq_dict[k]
            if len(h) > 0:
                x = (np.asarray(h, np.float64)[:, 0] == 1).astype(np.float64)
                w = alpha * (1.0 - alpha) ** np.arange(len(x) - 1, -1, -1.0)
                w[0] = (1.0 - alpha) ** (len(x) - 1)
                e[j] = float(w @ x)
        p = np.exp(-e / sampling_temp)
        return p / p.sum()

    @property
    def has_objects(self):
        """does any take carry an action object (action_one_hot != 0)?  host-side, evaluated once"""
        if getattr(self, "_has_obj", None) is None:
            self._has_obj = any(bool((a.abs().sum() > 0).item()) for a in self.data["action_one_hot"])
        return self._has_obj

    def sample_batch(self, n, freq_dict=None, use_freq=True, full_sample=False, sampling_temp=0.5, sampling_freq=0.9, probs=None):
        """n independent `sample_seq` draws (:264-327) -> dict of [n, fr_num, .] tensors (+ 'take_ind', 'fr_start').  The draws are made as
        arrays (one rng call per quantity, not per row): the same distributions as n sequential sample_seq calls."""
        starts = np.zeros(n, np.int64)
        if use_freq and freq_dict is None:
            inds = self.rng.choice(self.freq_indices, size=n)
        elif use_freq:
            probs = self.take_probs(freq_dict, sampling_temp) if probs is None else probs      # probs: the caller's cached take_probs(freq_dict)
            coin = self.rng.binomial(1, sampling_freq, size=n).astype(bool)
            inds = np.where(coin, self.rng.choice(self.all_indices, size=n, p=probs), self.rng.choice(self.all_indices, size=n))
            if not full_sample:
                hi = np.maximum(self._seq_lens()[inds] - self.fr_num, 1)
                starts = np.minimum((self.rng.random_sample(n) * hi).astype(np.int64), hi - 1)
        else:
            inds = self.rng.choice(self.all_indices, size=n)
        return self.batch(np.asarray(inds, np.int64), starts, None if full_sample else self.fr_num)

    def _seq_lens(self):
        if getattr(self, "_lens_np", None) is None or len(self._lens_np) != len(self.takes):
            self._lens_np = np.array([q.shape[0] for q in self.data["qpos"]], np.int64)
        return self._lens_np

    def _flat_store(self):
        """every take's rows back to back on self.device, per key [sum T, dim], + the takes' offsets: a batch is one gather per key"""
        if getattr(self, "_flat", None) is None or self._flat_n != len(self.takes):
            lens = self._seq_lens()
            self._flat_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
            self._flat = {k: torch.cat(v, 0).to(self.device) for k, v in self.data.items()} if len(lens) else {}
            self._flat_n = len(self.takes)
        return self._flat, self._flat_off

    def batch(self, inds, starts=None, length=None):
        """Rows (take, start) as one padded batch; `len` holds each row's valid frame count (ragged when length is None).  Rows shorter than
        the batch's longest are padded with their last frame."""
        inds = np.asarray(inds, np.int64); starts = np.zeros(len(inds), np.int64) if starts is None else np.asarray(starts, np.int64)
        avail = self._seq_lens()[inds] - starts
        lens = np.minimum(avail, length) if length else avail
        T = int(lens.max())
        flat, off = self._flat_store()
        idx = (off[inds] + starts)[:, None] + np.minimum(np.arange(T)[None, :], (lens - 1)[:, None])             # [n, T] rows of the flat store
        idx_t = torch.as_tensor(idx, device=self.device)
        out = {k: v[idx_t] for k, v in flat.items()}
        out["len"] = torch.as_tensor(lens.astype(np.int32), device=self.device)
        out["ragged"] = bool(lens.min() < T)           # host-side flag: rows are padded (init_context then averages every row over its own frames)
        out["take_ind"], out["fr_start"] = torch.as_tensor(inds), torch.as_tensor(starts)
        return out

    def get_seq_by_ind(self, ind, full_sample=False):
        return self.batch([ind], [0], None if full_sample else self.fr_num)

    def iter_seq(self):
        ind = self.counter % len(self.takes)
        self.counter += 1
        self.curr_key = self.takes[ind]
        return self.batch([ind], [0], None)

    def set_seq_counter(self, idx):
        self.counter = idx


# ------------------------------------------------------------------ synthetic stand-in for the absent MoCap set
def synthetic_takes(sim, std_qpos, n_per_action=2, T_range=(110, 160), body_mass=None, seed=0, with_objects=True, amp_max=0.3):
    """standing -> seeded smooth joint-space sinusoids (amplitude <= 0.3 rad, <= 1 Hz), four action
    classes with their object(s) at constant poses in front of / behind the humanoid, yaw U(-pi, pi).  with_objects=False: the same
    motions as takes without an action (obj_pose = [0,0,0,1,0,0,0], action_one_hot = 0; process_smpl.py:223-225) -- config 3's
    object-free MoCap clips.  amp_max: the sinusoids' amplitude bound (0.3 rad = SURVEY's figure; the pelvis does not move, so at that amplitude the
    legs swing the feet through the floor and no controller can follow the clip for long -- fine as a workload, not as a learning target)."""
    rng = np.random.default_rng(seed)
    std_qpos = np.asarray(std_qpos, np.float64)
    obj_local = {"sit": [[0.0, -0.6, 0.3805]], "push": [[0.0, 0.8, 0.921], [0.0, 0.8, 0.7905]], "avoid": [[0.0, 1.0, 0.69]], "step": [[0.0, 0.8, 0.3705]]}
    takes = {}
    for a in ACTIONS:
        for j in range(n_per_action):
            T = int(rng.integers(*T_range))
            yaw = rng.uniform(-np.pi, np.pi)
            qz = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
            q = np.tile(std_qpos, (T, 1))
            w, x, y, z = std_qpos[3:7]
            q[:, 3:7] = [qz[0] * w - qz[3] * z, qz[0] * x - qz[3] * y, qz[0] * y + qz[3] * x, qz[0] * z + qz[3] * w]     # qz (x) q_root
            amp, fr, ph = rng.uniform(0, amp_max, 69), rng.uniform(0.1, 1.0, 69), rng.uniform(0, 2 * np.pi, 69)
            tt = np.arange(T)[:, None] / 30.0
            q[:, 7:] += amp * (np.sin(2 * np.pi * fr * tt + ph) - np.sin(ph)) * np.minimum(tt / 0.5, 1.0)
            c, s_ = np.cos(yaw), np.sin(yaw)
            obj = []
            for lx, ly, lz in obj_local[a]:
                obj += [std_qpos[0] + c * lx - s_ * ly, std_qpos[1] + s_ * lx + c * ly, lz, *qz]
            if with_objects:
                takes[f"{a}-synthetic-{j:02d}"] = build_take_features(sim, q, np.tile(np.array(obj), (T, 1)), a, body_mass)
            else:
                takes[f"none-synthetic-{a}-{j:02d}"] = build_take_features(sim, q, None, None, body_mass)
    return takes


def synthetic_of_features(takes: dict, dim: int = 512, seed: int = 0) -> dict:
    """A stand-in of THIS repository for <dataset_path>/features/<of_file>.p (the reference's per-frame image features, which no public sample
    carries), as synthetic_takes stands in for the MoCap set: take -> [T, dim] float32, a seeded random projection of the take's head velocities
    and pose -- smooth in time and a function of the motion, as an optical-flow feature is -- plus N(0, 0.1) noise.  A workload and a test input,
    not a learning target."""
    rng = np.random.default_rng(seed)
    proj = rng.standard_normal((6 + 69, int(dim))) / np.sqrt(75.0)
    out = {}
    for take in sorted(takes):
        e = takes[take]
        x = np.concatenate([np.asarray(e["head_vels"], np.float64), np.asarray(e["qpos"], np.float64)[:, 7:]], 1)
        out[take] = (np.tanh(x @ proj) + 0.1 * rng.standard_normal((x.shape[0], int(dim)))).astype(np.float32)
    return out


def take_object_block(e: dict):
    """The [T, 35] object block of a feature take (obj_pose [T, 7] / [T, 14] at its action's offset, the rest parked: convert_obj_qpos_np), an
    obj_pose that already is the block as it stands, None for a take without an action object."""
    obj = e.get("obj_pose")
    if obj is None:
        return None
    obj = np.asarray(obj, np.float64)
    if obj.ndim == 2 and obj.shape[1] == OBJ_QPOS_DIM:
        return obj
    one_hot = np.asarray(e.get("action_one_hot", np.zeros((1, 4))), np.float64).reshape(-1, 4)[0]
    if not one_hot.sum() > 0:
        return None
    action = ACTIONS[int(np.argmax(one_hot))]
    return convert_obj_qpos_np(obj[:, :OBJ_ACTION_LEN[action]], action)


def rendered_of_features(takes: dict, sim, dim: int = 512, **kw) -> dict:
    """The schema of synthetic_of_features -- take -> [T, dim] float32 -- computed instead of drawn: the exact optical flow of the head camera over
    each take's qpos and objects, pooled over a grid (kinpoly_amd.render.ego_flow_features; kw: size, camera, scale).  A function of egocentric
    motion and scene, which is what the context GRU is meant to read; needs the ground-truth body, so a wild take has none."""
    from .render import ego_flow_features, flow_grid
    flow_grid(dim)
    return {take: ego_flow_features(sim, np.asarray(takes[take]["qpos"]), take_object_block(takes[take]), dim=dim, **kw) for take in sorted(takes)}


OF_SOURCES = ("auto", "file", "standin", "rendered")


def add_of_source_argument(ap):
    ap.add_argument("--of_source", choices=OF_SOURCES, default="auto", help="use_of: where the per-frame image features come from.  auto: the yml's feature file if it "
                    "exists, else the synthetic stand-in; file: the file or an error; standin: synthetic_of_features; rendered: the head camera's exact optical "
                    "flow over each take (rendered_of_features; not with --wild)")
    return ap


def of_source_refusal(of_source: str, wild: bool):
    """the message of a refused --of_source, or None"""
    if of_source not in OF_SOURCES:
        return f"--of_source must be one of {', '.join(OF_SOURCES)}, got {of_source}"
    if of_source == "rendered" and wild:
        return "--of_source rendered cannot go with --wild: a wild take has no ground-truth body to render"
    return None


def select_of_features(of_source: str, takes: dict, of_path: str, dim: int, seed: int, sim=None, wild: bool = False):
    """The `of` features of a run -> (a feature file's path or a dict take -> [T, dim], a line that says which).  auto is the rule the scripts always
    had: the file if it exists, else the stand-in."""
    no = of_source_refusal(of_source, wild)
    if no:
        raise ValueError(no)
    have = os.path.exists(of_path)
    if of_source == "file" and not have:
        raise FileNotFoundError(f"--of_source file: {of_path} does not exist")
    if of_source == "file" or (of_source == "auto" and have):
        return of_path, of_path
    if of_source == "rendered":
        if sim is None:
            raise ValueError("--of_source rendered needs a simulator handle to render with")
        return rendered_of_features(takes, sim, dim), f"rendered from the head camera ({dim} wide)"
    return synthetic_of_features(takes, dim, seed=seed), "synthetic stand-in" + ("" if of_source == "standin" else f" (no {of_path})")


def _ewma(x, alpha=0.05):
    """uhc/utils/math_utils.py:8-12, the recursion as written"""
    avg = x[0]
    for i in x[1:]:
        avg = alpha * i + (1 - alpha) * avg
    return avg


class AmassSingleDataset:
    """DatasetAMASSSingle (uhc/data_loaders/dataset_amass_single.py:24-241): the UHC's library of whole takes.

    Reads the reference's take pickle `{take: {pose_aa, pose_6d, trans, qpos, obj_pose}}` from data_specs['file_path'] (data_mode 'train') or
    ['test_file_path'] ('test'), keeps the takes of at least t_min (default 90) frames in the file's order -- or, with mode 'singles', those of
    data_specs['key_subsets'] -- and hands them to the device as one KpTakes library.  A take that carries objects (`obj_pose` of another shape than
    `qpos`: has_obj, :223) has its obj_pose appended raw to the 76 humanoid coordinates by the reference's reset_model, which only works when it is the
    model's whole object block: such a take is accepted when its obj_pose is [T, 35] (the library then carries objects and every reset places them; the
    takes without an own obj_pose get all five objects parked) and refused by name for every other width -- a 7- or 14-wide obj_pose needs the action's
    slot, which this file format does not carry (SmplObjDataset reads the format that does)."""

    SAMPLING_TEMP, SAMPLING_FREQ = 0.2, 0.75          # sample_seq's constants (:162-163)

    def __init__(self, data_specs: dict, data_mode: str = "train", takes: dict | None = None):
        if data_mode not in ("train", "test"):
            raise ValueError(f"data_mode must be 'train' or 'test', got {data_mode!r}")
        self.data_specs, self.data_mode = dict(data_specs), data_mode
        self.t_min, self.t_max, self.mode = data_specs.get("t_min", 90), data_specs.get("t_max", -1), data_specs.get("mode", "all")
        if takes is None:
            self.data_root = data_specs["file_path" if data_mode == "train" else "test_file_path"]
            import joblib
            takes = joblib.load(self.data_root)
        if self.mode == "all":
            keys = list(takes.keys())
        elif self.mode == "singles":
            keys = list(data_specs["key_subsets"])
        else:
            raise ValueError(f"data_specs['mode'] must be 'all' or 'singles', got {self.mode!r}")
        self.data_keys, self.qpos, self.obj_pose = [], {}, {}      # obj_pose: the takes that keep a [T, 35] object block of their own
        for k in keys:
            v = takes[k]
            if v["pose_aa"].shape[0] < self.t_min:             # :94-97
                continue
            qpos = np.asarray(v["qpos"], np.float64)
            # :103-107 as written: `(not v["obj_pose"] is None) in v` looks the BOOLEAN up among the take's keys, so obj_pose is the take's own only
            # for a take that has such a key; every other take gets its qpos, and has_obj (:223) is False
            obj = v["obj_pose"] if ("obj_pose" in v) and ((v["obj_pose"] is not None) in v) else v["qpos"]
            if np.shape(obj) != qpos.shape:
                if np.shape(obj) != (qpos.shape[0], OBJ_QPOS_DIM):
                    raise NotImplementedError(f"take '{k}' carries objects (obj_pose {np.shape(obj)} against qpos {qpos.shape}): objects in UHC takes are not supported "
                                              f"unless obj_pose is the whole [T, {OBJ_QPOS_DIM}] object block")
                self.obj_pose[k] = np.asarray(obj, np.float64)
            if qpos.ndim != 2 or qpos.shape[1] != 76 or qpos.shape[0] < 2:
                raise ValueError(f"take '{k}': qpos must be [T >= 2, 76], got {qpos.shape}")
            self.data_keys.append(k); self.qpos[k] = qpos
        if not self.data_keys:
            raise ValueError(f"no take of at least t_min = {self.t_min} frames")
        self.lens = np.array([self.qpos[k].shape[0] for k in self.data_keys], np.int64)

    def get_len(self):
        return len(self.data_keys)

    def new_freq_dict(self):
        return {k: [] for k in self.data_keys}

    def sample_probs(self, freq_dict: dict) -> np.ndarray:
        """sample_seq's init_probs (:164-175): exp(-ewma(success history) / 0.2) normalised over data_keys, a take without history counting as ewma 0; fp64"""
        e = np.array([_ewma(np.array(freq_dict[k])[:, 0] == 1) if len(freq_dict[k]) > 0 else 0 for k in self.data_keys], np.float64)
        p = np.exp(-e / self.SAMPLING_TEMP)
        return p / p.sum()

    def draw_probs(self, freq_dict: dict) -> np.ndarray:
        """the distribution one sample_seq draw follows (:177-181): sample_probs three times out of four, uniform otherwise"""
        return self.SAMPLING_FREQ * self.sample_probs(freq_dict) + (1 - self.SAMPLING_FREQ) / len(self.data_keys)

    def to_library(self, sim, dt=None):
        """all kept takes as one device-resident KpTakes (take k = data_keys[k]), built with sim's forward kinematics; dt: env.dt (default: the model's
        timestep x 15 substeps, as BatchedHumanoidEnv has it)"""
        from .sim import KpTakes
        off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        obj = None
        if any(k in self.obj_pose for k in self.data_keys):
            obj = np.concatenate([self.obj_pose[k] if k in self.obj_pose else convert_obj_qpos_np(np.zeros((len(self.qpos[k]), 7)), None) for k in self.data_keys], 0).astype(np.float32)
        return KpTakes(sim, np.concatenate([self.qpos[k] for k in self.data_keys], 0).astype(np.float32), off, sim.model.get_option("timestep") * 15 if dt is None else dt,
                       obj_rows=obj)


OBJ_QPOS_DIM = 35                                       # data.qpos[76:111]: five free joints
OBJ_ACTION_IDX = {"sit": 0, "push": 7, "avoid": 21, "step": 28}      # dataset_smpl_obj.py:62-67
OBJ_ACTION_LEN = {"sit": 7, "push": 14, "avoid": 7, "step": 7}       # :56-61


def convert_obj_qpos_np(obj_pose, action):
    """DatasetSMPLObj.convert_obj_qpos (dataset_smpl_obj.py:230-243) in fp64: [T, 35], all five objects parked at [(i + 1) * 100, 100, 0] with an all-zero
    quaternion, the take's own 7 (push: 14) floats written at the action's offset; an action outside the four (None) leaves everything parked."""
    obj_pose = np.asarray(obj_pose)
    out = np.zeros((obj_pose.shape[0], OBJ_QPOS_DIM))
    for i in range(5):
        out[:, 7 * i:7 * i + 3] = [(i + 1) * 100, 100, 0]
    if action in OBJ_ACTION_IDX:
        a = OBJ_ACTION_IDX[action]
        out[:, a:a + OBJ_ACTION_LEN[action]] = obj_pose
    return out


class SmplObjDataset:
    """DatasetSMPLObj (uhc/data_loaders/dataset_smpl_obj.py:25-243): the UHC's library of whole MoCap takes that carry objects, as
    scripts/eval_pose_all.py:560 runs the controller on the sit, push, avoid and step takes.

    Reads the pickle `{take: {qpos [T,76], obj_pose [T,7] or [T,14], action_one_hot [T,4], ...}}` from data_specs['file_path'] ('train') or
    ['test_file_path'] ('test'); keeps the takes in the file's order (mode 'all') or those of data_specs['key_subsets'] (mode 'singles') -- every one of
    them: this loader has no t_min filter (process_data_pickle, :96-130).  A take's action is argmax(action_one_hot[0]) over (sit, push, avoid, step) and
    `obj_qpos[take]` its [T, 35] object block (convert_obj_qpos).  Departure: a take whose action_one_hot[0] is all zero has no action here and gets all
    five objects parked, where the reference's argmax calls it a sit take and puts its placeholder obj_pose (a chair at the origin) under the humanoid.
    has_obj is True and num_obj 5 for every take (get_single_sample, :213-214).

    `iter_seq()` walks data_keys from frame 0 (:187-198); `sample_seq()` draws a take from sample_keys and fr_start honouring t_min / t_max (:154-178).
    `to_library(sim)` hands all takes to the device as one KpTakes with objects.  For CopycatAgent it offers AmassSingleDataset's sampling-frequency
    interface (data_keys, lens, new_freq_dict, draw_probs): the reference's class has NO success-weighted form (its sample_seq is random.choice over
    sample_keys, or value-based hard-negative mining, which needs recorded states), so draw_probs is that uniform draw over sample_keys -- a take
    counts qpos_len // t_max + 1 times when t_max is set -- whatever the freq_dict says; the agent still records every episode in it."""

    ACTIONS = ACTIONS

    def __init__(self, data_specs: dict, data_mode: str = "train", takes: dict | None = None):
        if data_mode not in ("train", "test"):
            raise ValueError(f"data_mode must be 'train' or 'test', got {data_mode!r}")
        self.data_specs, self.data_mode = dict(data_specs), data_mode
        self.t_min, self.t_max, self.mode = data_specs.get("t_min", 90), data_specs.get("t_max", -1), data_specs.get("mode", "all")
        if takes is None:
            self.data_root = data_specs["file_path" if data_mode == "train" else "test_file_path"]
            import joblib
            takes = joblib.load(self.data_root)
        if self.mode == "all":
            keys = list(takes.keys())
        elif self.mode == "singles":
            keys = list(data_specs["key_subsets"])
        else:
            raise ValueError(f"data_specs['mode'] must be 'all' or 'singles', got {self.mode!r}")
        self.data_keys, self.sample_keys, self.qpos, self.obj_qpos, self.action = [], [], {}, {}, {}
        for k in keys:
            v = takes[k]
            qpos = np.asarray(v["qpos"], np.float64)
            if qpos.ndim != 2 or qpos.shape[1] != 76 or qpos.shape[0] < 2:
                raise ValueError(f"take '{k}': qpos must be [T >= 2, 76], got {qpos.shape}")
            first = np.asarray(v["action_one_hot"])[0]
            action = ACTIONS[int(np.argmax(first))] if np.any(first != 0) else None
            obj = np.asarray(v["obj_pose"], np.float64)
            if action is not None and obj.shape != (qpos.shape[0], OBJ_ACTION_LEN[action]):
                raise ValueError(f"take '{k}': a '{action}' take needs obj_pose [{qpos.shape[0]}, {OBJ_ACTION_LEN[action]}], got {obj.shape}")
            self.qpos[k], self.action[k], self.obj_qpos[k] = qpos, action, convert_obj_qpos_np(obj if action is not None else np.zeros((qpos.shape[0], 7)), action)
            self.sample_keys += [k] * (qpos.shape[0] // self.t_max + 1 if self.t_max != -1 else 1)      # :123-126
            self.data_keys.append(k)
        if not self.data_keys:
            raise ValueError("the take file holds no take")
        self.lens = np.array([self.qpos[k].shape[0] for k in self.data_keys], np.int64)
        self.seq_counter, self.curr_key = 0, ""
        self.rng = np.random.RandomState(0)

    def get_len(self):
        return len(self.data_keys)

    def set_seq_counter(self, idx):
        self.seq_counter = idx

    def get_single_sample(self, key, fr_start, fr_end):
        return {"qpos": self.qpos[key][fr_start:fr_end], "obj_pose": self.obj_qpos[key][fr_start:fr_end], "action": self.action[key], "seq_name": key,
                "has_obj": True, "num_obj": 5, "fr_start": int(fr_start)}

    def iter_seq(self):
        self.curr_key = self.data_keys[self.seq_counter % len(self.data_keys)]
        self.seq_counter += 1
        return self.get_single_sample(self.curr_key, 0, self.qpos[self.curr_key].shape[0])

    def sample_seq(self):
        """:154-178 without hard-negative mining: a uniform draw over sample_keys; with t_max a window of at most t_max frames from a uniform fr_start,
        without it the rest of the take from a uniform fr_start in [0, len - t_min)"""
        self.curr_key = self.sample_keys[self.rng.randint(len(self.sample_keys))]
        n = self.qpos[self.curr_key].shape[0]
        if self.t_max != -1:
            fr_start = int(self.rng.randint(n - self.t_max)) if n - self.t_max > 0 else 0
            fr_end = min(fr_start + self.t_max, n)
        else:
            fr_start = int(self.rng.randint(n - self.t_min)) if n - self.t_min > 0 else 0
            fr_end = n
        return self.get_single_sample(self.curr_key, fr_start, fr_end)

    def new_freq_dict(self):
        return {k: [] for k in self.data_keys}

    def draw_probs(self, freq_dict: dict | None = None) -> np.ndarray:
        """the distribution one sample_seq draw follows: uniform over sample_keys (see the class docstring), the freq_dict plays no part"""
        p = np.array([self.sample_keys.count(k) for k in self.data_keys], np.float64)
        return p / p.sum()

    def to_library(self, sim, dt=None):
        """all takes as one device-resident KpTakes with objects (take k = data_keys[k]); dt as AmassSingleDataset.to_library"""
        from .sim import KpTakes
        off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        return KpTakes(sim, np.concatenate([self.qpos[k] for k in self.data_keys], 0).astype(np.float32), off, sim.model.get_option("timestep") * 15 if dt is None else dt,
                       obj_rows=np.concatenate([self.obj_qpos[k] for k in self.data_keys], 0).astype(np.float32))
