"""A torch restatement of the FORWARD kernels of the kinematic roll-out, formula for formula, for any dtype and device: k_kin_advance
(kinpoly_amd/csrc/kp_obs_kernels.hpp), the chain of k_target_fk, and the blocks of k_obs_ar (kp_obs_ar_row.hpp).  Run in fp64 on the CPU with
autograd it is the reference of the gradient kernels (kp_kin_tape.hip); run in fp32 on the device it is their yardstick.  Not a test module.

Where the kernels branch (the expmap's constant axis, the `no rotation` rows of the finite-difference velocity) the restatement selects with
torch.where over operands made safe first, so a branch that is not taken contributes a zero gradient and no NaN.
"""
import math

import torch

HEAD = 13


def qmul(a, b):
    aw, ax, ay, az = a.unbind(-1); bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def qconj(q):
    return torch.cat([q[..., :1], -q[..., 1:]], -1)


def q_inverse(q):
    return qconj(q) / (q * q).sum(-1, keepdim=True)


def q_matrix(q):
    """q_matrix: the rotation of q / |q| (s = sqrt(2 / |q|^2) scales the components first) -> [..., 3, 3]"""
    s = torch.sqrt(2.0 / (q * q).sum(-1, keepdim=True))
    w, x, y, z = (q * s).unbind(-1)
    return torch.stack([torch.stack([1 - y * y - z * z, x * y - z * w, x * z + y * w], -1),
                        torch.stack([x * y + z * w, 1 - x * x - z * z, y * z - x * w], -1),
                        torch.stack([x * z - y * w, y * z + x * w, 1 - x * x - y * y], -1)], -2)


def q_mul_vec(q, v):
    return (q_matrix(q) @ v[..., None])[..., 0]


def q_tmul_vec(q, v):
    return (q_matrix(q).transpose(-1, -2) @ v[..., None])[..., 0]


def q_heading(q):
    z = torch.zeros_like(q[..., 0])
    return torch.stack([q[..., 0], z, z, q[..., 3]], -1) / torch.sqrt(q[..., 0] ** 2 + q[..., 3] ** 2)[..., None]


def tv_heading(v, q):
    return q_tmul_vec(q_heading(q), v)


def _unit_x(like):
    return torch.tensor([1.0, 0.0, 0.0], dtype=like.dtype, device=like.device).expand_as(like)


def q_from_expmap(e):
    angle0 = torch.sqrt((e * e).sum(-1).detach())
    guard = angle0 < 1e-12
    es = torch.where(guard[:, None], _unit_x(e), e)
    angle = torch.sqrt((es * es).sum(-1))
    axis = torch.where(guard[:, None], _unit_x(e), es / angle[:, None])
    half = 0.5 * torch.where(guard, torch.zeros_like(angle), angle)
    k = torch.sin(half) / torch.sqrt((axis * axis).sum(-1))
    return torch.cat([torch.cos(half)[:, None], axis * k[:, None]], -1)


def q_euler_rzyx(ang):
    h = 0.5 * ang
    s, c = torch.sin(h), torch.cos(h)
    z = torch.zeros_like(c[..., 0])
    qz = torch.stack([c[..., 0], z, z, s[..., 0]], -1); qy = torch.stack([c[..., 1], z, s[..., 1], z], -1); qx = torch.stack([c[..., 2], s[..., 2], z, z], -1)
    return qmul(qmul(qz, qy), qx)


def kin_advance(qpos, act, dt=1.0 / 30.0):
    """k_kin_advance -> (next_qpos [n,76], qvel [n,75])"""
    rot = qpos[:, 3:7]
    linv = q_mul_vec(q_heading(rot), act[:, 74:77])
    nxy = qpos[:, :2] + linv[:, :2] * dt
    angv = q_mul_vec(rot, act[:, 77:80])
    ev = dt * angv
    nr = qmul(q_from_expmap(ev), rot)
    nr = nr / torch.sqrt((nr * nr).sum(-1, keepdim=True))
    nxt = torch.cat([nxy, act[:, :1], nr, act[:, 5:74]], 1)
    idt = 1.0 / dt
    vlin = (nxt[:, :3] - qpos[:, :3]) * idt
    c2 = (rot * rot).sum(-1, keepdim=True)
    qrel = qmul(nr, qconj(rot) / c2)
    xyz = qrel[:, 1:]
    small = ~((xyz * xyz).sum(-1).detach() > 0) | (ev.detach() == 0).all(-1)
    xs = torch.where(small[:, None], _unit_x(xyz), xyz)
    sn = torch.sqrt((xs * xs).sum(-1))
    axis = torch.where(small[:, None], _unit_x(xyz), xs / sn[:, None])
    angle = torch.where(small, torch.zeros_like(sn), 2.0 * torch.atan2(sn, qrel[:, 0]))
    angle = torch.where(angle > 3.14159265358979, angle - 6.28318530717959, angle)
    angle = torch.where(angle < -3.14159265358979, angle + 6.28318530717959, angle)
    rv = (angle * idt)[:, None] * axis
    cn = torch.sqrt(c2)
    u = -rot[:, 1:] / cn
    t = 2.0 * torch.cross(u, rv, dim=-1)
    wv = rv + (rot[:, :1] / cn) * t + torch.cross(u, t, dim=-1)
    return nxt, torch.cat([vlin, wv, (act[:, 5:74] - qpos[:, 7:]) * idt], 1)


def fk(qpos, body_pos, parents):
    """k_target_fk's chain -> (wbpos [n,24,3], wbquat [n,24,4]); body_pos [24,3] in qpos' dtype, parents: 24 ints (parent before child)"""
    rq = qpos[:, 3:7] / torch.sqrt((qpos[:, 3:7] ** 2).sum(-1, keepdim=True))
    pos, wq = [qpos[:, :3]], [rq]
    for b in range(1, 24):
        p = int(parents[b])
        lq = q_euler_rzyx(qpos[:, 7 + 3 * (b - 1):10 + 3 * (b - 1)])
        pos.append(q_mul_vec(wq[p], body_pos[b].expand(qpos.shape[0], 3)) + pos[p])
        wq.append(qmul(wq[p], lq))
    return torch.stack(pos, 1), torch.stack(wq, 1)


def observe(qpos, qvel, hpos, hrot, head_pose, head_vels, obj_rel, one_hot, obj_pose, vel=False, head=True, action=True):
    """k_obs_ar's row for one frame: head_pose [n,7], head_vels [n,6], obj_rel [n,7], one_hot [n,4], obj_pose [n,7] are that frame's table rows;
    hpos / hrot the head's position and world quaternion (fk).  -> (obs [n,W], obj_2_head [n,7])"""
    rq = qpos[:, 3:7]
    local = torch.cat([qpos[:, 2:3], qmul(q_inverse(q_heading(rq)), rq), qpos[:, 7:]], 1)
    on = (one_hot.sum(1) != 0)[:, None]
    opos = torch.where(on, obj_pose[:, :3], torch.zeros_like(obj_pose[:, :3]))
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=qpos.dtype, device=qpos.device).expand(qpos.shape[0], 4)
    orot = torch.where(on, obj_pose[:, 3:7], ident)
    obj = torch.cat([tv_heading(opos - hpos, hrot), qmul(q_inverse(q_heading(hrot)), orot)], 1)
    blocks = [local]
    if vel:
        blocks.append(qvel)
    if head:
        blocks += [tv_heading(head_pose[:, :3] - hpos, hrot), qmul(q_inverse(head_pose[:, 3:]), hrot)]
    blocks.append(obj)
    if head:
        blocks += [head_vels[:, 3:6], head_vels[:, 0:3], obj_rel]
    if action:
        blocks.append(one_hot)
    return torch.cat(blocks, 1), obj


def observe_frame(qpos, qvel, body_pos, parents, tables, vel=False, head=True, action=True):
    """fk + observe: -> (obs, wbpos [n,72], obj_2_head); tables = (head_pose, head_vels, obj_rel, one_hot, obj_pose) rows of the frame"""
    wbpos, wbquat = fk(qpos, body_pos, parents)
    obs, obj = observe(qpos, qvel, wbpos[:, HEAD], wbquat[:, HEAD], *tables, vel=vel, head=head, action=action)
    return obs, wbpos.reshape(qpos.shape[0], 72), obj


def edge_rows(n, seed=0, dtype=torch.float64):
    """n rows of (qpos [n,76], action [n,80]) for the gradient sweeps: random poses and actions, with the first rows (as many as fit) replaced by the
    edge cases -- 0: an exactly zero angular action; 1: a turn of 1e-4 rad per frame; 2: a turn within 1e-3 of pi per frame (not at it); 3 / 4: headings
    within 1e-3 of +pi / -pi; 5: joint angles near +-3 pi; 6: a root quaternion unit only to 3e-7.  dt = 1 / 30."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    q = torch.zeros((n, 76), dtype=torch.float64)
    q[:, :3] = r(n, 3) * torch.tensor([2.0, 2.0, 0.1]) + torch.tensor([0.0, 0.0, 0.9])
    yaw = r(n) * 2.0      # any heading, a tilt of up to about a radian: |(w, z)|, which the heading divides by, stays away from 0
    rq = torch.stack([torch.cos(yaw), 0.3 * r(n), 0.3 * r(n), torch.sin(yaw)], 1); q[:, 3:7] = rq / rq.norm(dim=1, keepdim=True)
    q[:, 7:] = r(n, 69) * 0.5
    a = torch.zeros((n, 80), dtype=torch.float64)
    a[:, 0] = 0.9 + 0.1 * r(n); a[:, 1:5] = r(n, 4); a[:, 5:74] = r(n, 69) * 0.5; a[:, 74:77] = r(n, 3); a[:, 77:80] = r(n, 3) * 2.0
    dt = 1.0 / 30.0
    unit = lambda v: v / v.norm()                                         # noqa: E731

    def yaw_tilt(yaw):      # heading `yaw` with a small tilt on top: heading(q) stays within 1e-3 of yaw's
        qz = torch.tensor([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)], dtype=torch.float64)
        tl = torch.tensor([math.cos(0.15), math.sin(0.15) * 0.6, math.sin(0.15) * 0.8, 0.0], dtype=torch.float64)
        return qmul(qz[None], tl[None])[0]
    edits = [lambda i: a[i, 77:80].zero_(),
             lambda i: a[i, 77:80].copy_(unit(a[i, 77:80]) * (1e-4 / dt)),
             lambda i: a[i, 77:80].copy_(unit(a[i, 77:80]) * ((math.pi - 7e-4) / dt)),
             lambda i: q[i, 3:7].copy_(yaw_tilt(math.pi - 6e-4)),
             lambda i: q[i, 3:7].copy_(yaw_tilt(-math.pi + 6e-4)),
             lambda i: q[i, 7:].copy_(torch.sign(q[i, 7:]) * 3 * math.pi + q[i, 7:] * 0.02),
             lambda i: q[i, 3:7].mul_(1.0 + 3e-7)]
    for i in range(min(n, len(edits))):      # fewer rows than cases: start at case `seed`, so that small batches of different seeds meet them all
        edits[(i + (seed if n < len(edits) else 0)) % len(edits)](i)
    return q.to(dtype), a.to(dtype)


def frame_tables(n, seed=0, dtype=torch.float64):
    """one frame's table rows for `observe`: (head_pose, head_vels, obj_rel, one_hot, obj_pose); every fourth row has no action (all-zero one-hot)"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    hp = torch.cat([r(n, 3) + torch.tensor([0.0, 0.0, 1.5]), torch.nn.functional.normalize(r(n, 4), dim=1) * (1.0 + 1e-7 * r(n, 1))], 1)
    ob = torch.cat([r(n, 3), torch.nn.functional.normalize(r(n, 4), dim=1)], 1)
    oh = torch.zeros((n, 4), dtype=torch.float64)
    idx = torch.arange(n)
    oh[idx, idx % 4] = 1.0
    oh[idx % 4 == 3] = 0.0
    return tuple(t.to(dtype) for t in (hp, r(n, 6), torch.cat([r(n, 3), torch.nn.functional.normalize(r(n, 4), dim=1)], 1), oh, ob))
