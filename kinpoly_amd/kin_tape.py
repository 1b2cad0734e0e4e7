"""The kinematic roll-out of a clip WITH a tape: TrajARNet.forward in train form (kin_poly/models/traj_ar_smpl_net.py:346-383) on the HIP kernels
of the untaped roll-out (kinpoly_amd/context.py: TrajARNet.rollout), with their gradient kernels (kinpoly_amd/csrc/kp_kin_tape.hip) behind
`torch.autograd.Function`s.

pretrain.forward_supervised builds every frame from about a hundred small torch ops so that autograd reaches the networks; here a frame is
set_state (forward kinematics), kp_sim_obs_ar, kp_sim_fk, the GRU + MLP (torch, `net.get_action`) and kp_kin_advance, and its backward is
kp_kin_advance_backward, kp_sim_obs_ar_backward and kp_sim_fk_head_backward.  Same contract as forward_supervised: same arguments, same dict.

Two deviations from the torch path: the gradients are those of the kernels' formulas, which normalise a quaternion where
supervised._qrot does not (parameter gradients agree: every root quaternion on the tape comes out of a normalisation); and the input noise is
drawn once per clip batch into noisy copies of the head tables instead of frame by frame (same elements, same distribution, another order of draws).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import sim as kpsim

FUSED_LAYOUTS = tuple(kpsim.ar_obs_dim(v, h, a) for v, h, a in ((0, 1, 1), (0, 1, 0), (1, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 1)))      # 105, 101, 180, 176, 85, 160


class KinAdvance(torch.autograd.Function):
    """(qpos [N,76], action [N,80], dt) -> (next_qpos [N,76], qvel [N,75]): kp_kin_advance / kp_kin_advance_backward."""

    @staticmethod
    def forward(ctx, qpos, action, dt):
        q, a = qpos.contiguous(), action.contiguous()
        nxt, qvel = kpsim.kin_advance(q, a, dt)
        ctx.dt = float(dt)
        ctx.save_for_backward(q, a)
        ctx.set_materialize_grads(False)
        return nxt, qvel

    @staticmethod
    def backward(ctx, g_next, g_qvel):
        q, a = ctx.saved_tensors
        gq, ga = kpsim.kin_advance_backward(q, a, ctx.dt, None if g_next is None else g_next.contiguous(), None if g_qvel is None else g_qvel.contiguous())
        return gq, ga, None


class ObserveFrame(torch.autograd.Function):
    """(qpos [N,76], qvel [N,75], slab) -> (obs [N,W], wbpos [N,72], obj_2_head [N,7]) of one frame on a physics-free KpSim of N rows: set_state +
    kp_sim_obs_ar + kp_sim_fk forward, kp_sim_obs_ar_backward + kp_sim_fk_head_backward backward.  `frame` is the frame's own kp_ctx (its cur_t and
    object rows are not reused by later frames: the backward pass reads them again).  With `ext` (a network with a context / `of` block) the row is
    kp_sim_obs_ar_ex's [context | base | of]; slab [N,H] is then the frame's slab of the time-major context sequence ext points into -- the third
    differentiable input, whose gradient is the first H columns of the row's cotangent; the `of` block is data.  Without ext, slab is None."""

    @staticmethod
    def forward(ctx, qpos, qvel, slab, sim, frame, ext=None):
        q, v = qpos.contiguous(), qvel.contiguous()
        sim.set_state(q, v)
        obs = sim.obs_ar(frame) if ext is None else sim.obs_ar_ex(frame, ext)
        fk = sim.fk(q)
        o = (0 if ext is None else ext.ctx_dim) + 74 + 75 * sim.obs_ar_vel + 7 * sim.obs_ar_head
        ctx.sim, ctx.frame, ctx.ext = sim, frame, ext
        ctx.save_for_backward(q, fk["wbpos"], fk["wbquat"])
        ctx.set_materialize_grads(False)
        return obs, fk["wbpos"], obs[:, o:o + 7].clone()

    @staticmethod
    def backward(ctx, g_obs, g_wb, g_obj):
        q, wbpos, wbquat = ctx.saved_tensors
        sim, ext = ctx.sim, ctx.ext
        g_obj = None if g_obj is None else g_obj.contiguous()
        gc = None
        if ext is None:
            g_obs = torch.zeros((q.shape[0], sim.obs_ar_dim), device=q.device) if g_obs is None else g_obs.contiguous()
            gq, gv, ghp, ghq = sim.obs_ar_backward(ctx.frame, q, wbpos, wbquat, g_obs, g_obj)
        else:
            g_obs = torch.zeros((q.shape[0], ext.ctx_dim + sim.obs_ar_dim + ext.of_dim), device=q.device) if g_obs is None else g_obs.contiguous()
            gq, gv, ghp, ghq, gc = sim.obs_ar_ex_backward(ctx.frame, ext, q, wbpos, wbquat, g_obs, g_obj)
        gq = sim.fk_head_backward(q, wbpos, wbquat, None if g_wb is None else g_wb.contiguous(), ghp, ghq, gq)
        return gq, gv, (gc if ctx.needs_input_grad[2] else None), None, None, None


_TWINS: dict = {}
_MAX_TWINS = 4


def twin_sim(sim: kpsim.KpSim, n: int) -> kpsim.KpSim:
    """A physics-free simulator of `n` rows on `sim`'s model and device (the observation kernel works on a handle's own rows): `sim` itself when it has
    that many -- its state is then overwritten by the roll-out (set_state every frame), so a caller that keeps a state in it sets it again afterwards,
    as AgentAR.train_init does by restarting its sampler -- else a twin.  At most _MAX_TWINS twins are kept (an epoch is full batches and one short
    one); the least recently used one is dropped beyond that."""
    if sim.n == n:
        sim.use_current_stream()
        return sim
    key = (id(sim.model), sim.device.index, int(n))
    t = _TWINS.pop(key, None)
    if t is None or t.model is not sim.model:
        t = kpsim.KpSim(sim.model, int(n), sim.device.index)
    _TWINS[key] = t                    # most recent last
    while len(_TWINS) > _MAX_TWINS:
        _TWINS.pop(next(iter(_TWINS)))
    t.use_current_stream()
    return t


def check_fused(net, fk, data=None):
    """Raises with the reason when the taped path cannot run: it needs an fp32 network on a HIP device, the library's FK behind `fk`, and one of the six
    layouts Config accepts as the network's base row (a context block before it and an `of` block after it ride along: kp_sim_obs_ar_ex)."""
    p = next(net.parameters())
    if not (p.is_cuda and p.dtype == torch.float32):
        raise ValueError(f"fused=True runs the fp32 HIP kernels: the network is {p.dtype} on {p.device} (fp64 master copies, --update_dtype fp64, stay on the torch path)")
    if getattr(fk, "sim", None) is None:
        raise ValueError("fused=True needs a TorchFK built on a KpSim (sim=...): the taped roll-out runs on a physics-free twin of it")
    base = getattr(net, "base_dim", net.state_dim)
    if base not in FUSED_LAYOUTS:
        raise ValueError(f"fused=True: no gradient kernel for the {base}-d observation (layouts: {', '.join(map(str, FUSED_LAYOUTS))})")
    if fk.sim.obs_ar_dim != base:
        raise ValueError(f"fused=True: the kinematic simulator writes {fk.sim.obs_ar_dim}-d observations, the policy takes {base}-d (kpsim.ar_obs_options)")
    if data is not None:
        for k in ("qpos", "head_pose", "head_vels", "obj_head_relative_poses", "obj_pose") + (("of",) if getattr(net, "of_dim", 0) else ()):
            if not (data[k].is_cuda and data[k].dtype == torch.float32):
                raise ValueError(f"fused=True: data['{k}'] is {data[k].dtype} on {data[k].device}, the kernels read fp32 device tensors")


def _frame_ctx(base: kpsim.KpCtx, cur_t: torch.Tensor, obj: torch.Tensor) -> kpsim.KpCtx:
    c = kpsim.KpCtx()
    C.memmove(C.byref(c), C.byref(base), C.sizeof(kpsim.KpCtx))
    c.cur_t, c.obj_qpos = cur_t.data_ptr(), obj.data_ptr()
    c._keep = (base, cur_t, obj)
    return c


def forward_supervised_taped(net, fk, data, gt_rate=0.0, rng=None, noise_std=0.0, generator=None, dt=1.0 / 30.0):
    """pretrain.forward_supervised's contract on the kernels: init_states -> T x (observation, action, kinematic step) with a tape; the
    scheduled-sampling coins are drawn in the reference's order (initial state, then after every step), and a frame put on the ground-truth pose
    cuts the pose tape while the GRU state keeps carrying gradient.  noise_std > 0: N(0, noise_std) on every element of the head_pose, head_vels
    and obj_head_relative_poses tables the observation reads (traj_ar_smpl_net.py:241-246), drawn once for the batch; the loss reads the clean ones.
    Returns qpos [B,T,76], qvel [B,T,75] (after fix_qvel), action [B,T,80], pred_wbpos [B,T,72], obj_2_head [B,T,7]."""
    check_fused(net, fk, data)
    rng = np.random if rng is None else rng
    B, T = data["qpos"].shape[:2]
    sim = twin_sim(fk.sim, B)
    dev = data["qpos"].device
    ctx_block = getattr(net, "ctx_block", 0)
    qpos, qvel, ctx_feat = net.init_states(data, keep_feat=bool(ctx_block))
    # a context block: the time-major sequence the init mean came from (clean tables: the noise below is the observation's); frame t's slab is a view
    # of it, so a frame put on the ground-truth pose still hands its context cotangent back, and the backward over the frames is one stack
    seq = ctx_feat.transpose(0, 1) if ctx_block else None
    slabs = seq.unbind(0) if ctx_block else None
    ext = net.obs_ext(sim, data, None if seq is None else seq.detach())
    if gt_rate > 0.0 and rng.binomial(1, gt_rate):
        qpos, qvel = data["qpos"][:, 0], data["qvel"][:, 0]
    tabs = [data[k].contiguous() for k in ("head_pose", "head_vels", "obj_head_relative_poses")]
    if noise_std > 0.0:
        tabs = [x + torch.randn(x.shape, device=dev, dtype=x.dtype, generator=generator) * noise_std for x in tabs]
    one_hot = data["action_one_hot"] if data["action_one_hot"].dim() == 2 else data["action_one_hot"][:, 0]
    cur = torch.arange(T, dtype=torch.int32, device=dev)[:, None].expand(T, B).contiguous()          # frame-major: row t is that frame's cur_t
    obj = data["obj_pose"][:, :, :7].transpose(0, 1).contiguous()
    z96, z72 = torch.zeros((B, T, 96), device=dev), torch.zeros((B, T, 72), device=dev)
    base = sim.make_ctx(T, *tabs, one_hot.contiguous(), z96, z72, cur[0], obj_qpos=obj[0])
    hx = torch.zeros((B, net.rnn_hdim), device=dev, dtype=qpos.dtype)
    Q, V, A, W, O = [], [], [], [], []
    for t in range(T):
        obs, wb, orel = ObserveFrame.apply(qpos, qvel, slabs[t] if ctx_block else None, sim, _frame_ctx(base, cur[t], obj[t]), ext)
        Q.append(qpos); V.append(qvel); W.append(wb); O.append(orel)
        action, hx = net.get_action(obs, hx)
        A.append(action)
        if t == T - 1:
            break
        qpos, qvel = KinAdvance.apply(qpos, action, dt)
        if gt_rate > 0.0 and rng.binomial(1, gt_rate):
            qpos, qvel = data["qpos"][:, t + 1], data["qvel"][:, t + 1]
    V = torch.stack(V, 1)
    return {"qpos": torch.stack(Q, 1), "qvel": torch.cat([V[:, 1:], V[:, -2:-1]], 1), "action": torch.stack(A, 1),
            "pred_wbpos": torch.stack(W, 1), "obj_2_head": torch.stack(O, 1)}
