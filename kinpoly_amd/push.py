"""Perturbation pushes: a schedule that decides, per env and step, whether a body is pushed and with which impulse (no reference counterpart;
DESIGN.md section 12).  The envs apply what it draws with kp_sim_apply_impulse at the tail of step(): after the physics, the reward and the
episode bookkeeping of the step that just ended, before the observation of the next state is written.

Everything is drawn with device-side torch ops from the schedule's own seeded generator: no host read per step, and the number of draws per call
does not depend on what was drawn, so two schedules with one seed give identical pushes.
"""
from __future__ import annotations

import math

import torch

from .env import SMPL_BODY_NAMES


def body_ids(names) -> list:
    """indices (0..23, the entity numbering of kp_sim_apply_impulse) of body names; unknown names are refused"""
    ids = []
    for b in names:
        if b not in SMPL_BODY_NAMES:
            raise ValueError(f"push: unknown body {b!r} (bodies: {', '.join(SMPL_BODY_NAMES)})")
        ids.append(SMPL_BODY_NAMES.index(b))
    if not ids:
        raise ValueError("push: no body named")
    return ids


class PushSchedule:
    """Every `interval` steps of an env's episode clock, with probability `prob`, push a body drawn from `bodies` with a linear impulse whose magnitude is
    uniform in impulse = (lo, hi) N s and whose direction is uniform in the horizontal plane (horizontal=True: p_z = 0) or on the sphere; the angular
    impulse is zero.  offset: a fixed point (x, y, z) in the body frame, or None = the body origin.  record=True keeps every call's draw on the device
    (`log`); the evaluation roll-outs turn it into `by_take` = {take: [(step, body name, impulse[6]), ...]} with one host read per batch of takes."""

    def __init__(self, n_envs, device, interval, prob=1.0, bodies=("Pelvis",), impulse=(0.0, 0.0), horizontal=True, offset=None, seed=0, record=False):
        self.n, self.device = int(n_envs), torch.device(device)
        self.interval, self.prob, self.horizontal = int(interval), float(prob), bool(horizontal)
        if self.interval < 1:
            raise ValueError(f"push: interval must be >= 1, got {interval}")
        if not 0.0 <= self.prob <= 1.0:
            raise ValueError(f"push: prob must be in [0, 1], got {prob}")
        lo, hi = (float(impulse), float(impulse)) if isinstance(impulse, (int, float)) else (float(impulse[0]), float(impulse[-1]))
        if not 0.0 <= lo <= hi:
            raise ValueError(f"push: impulse must be 0 <= lo <= hi, got {impulse}")
        self.lo, self.hi = lo, hi
        self.body_names = tuple(bodies)
        self.bodies = torch.tensor(body_ids(bodies), dtype=torch.int32, device=self.device)
        self.offset = None if offset is None else torch.tensor(offset, dtype=torch.float32, device=self.device).reshape(1, 3).expand(self.n, 3).contiguous()
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self.count = torch.zeros((), dtype=torch.int64, device=self.device)      # pushes drawn so far
        self.log = [] if record else None
        self.by_take = {}

    def draw(self, cur_t: torch.Tensor, alive: torch.Tensor | None = None):
        """cur_t [N]: every env's episode clock; alive [N] (bool, optional): envs whose episode goes on -- the others get no push.
        -> (entity int32 [N]: a body, or -1 where no push falls due; impulse float32 [N, 6]; offset [N, 3] or None)"""
        n, dev, g = self.n, self.device, self.gen
        u = torch.rand((n, 5), device=dev, generator=g)               # chance, body, magnitude, azimuth, height: one draw per call, whatever falls due
        due = (cur_t.to(dev).long() % self.interval == 0) & (u[:, 0] < self.prob)
        if alive is not None:
            due = due & alive.to(dev, torch.bool)
        body = self.bodies[(u[:, 1] * len(self.bodies)).long().clamp_(max=len(self.bodies) - 1)]
        mag = self.lo + (self.hi - self.lo) * u[:, 2]
        az = 2 * math.pi * u[:, 3]
        z = torch.zeros(n, device=dev) if self.horizontal else 2 * u[:, 4] - 1      # uniform on the sphere: uniform height, uniform azimuth
        rho = torch.sqrt((1 - z * z).clamp_min(0))
        imp = torch.zeros((n, 6), device=dev)
        imp[:, 0], imp[:, 1], imp[:, 2] = mag * rho * torch.cos(az), mag * rho * torch.sin(az), mag * z
        entity = torch.where(due, body, torch.full_like(body, -1))
        imp = imp * due[:, None]
        self.count += due.sum()
        if self.log is not None:
            self.log.append((cur_t.to(dev).clone(), entity, imp))
        return entity, imp, self.offset

    def collect(self, first_call, active, keys):
        """The calls log[first_call:] as a push log: active [steps, n] (numpy bool: env e was still playing its take at that step), keys: the take of the
        first len(keys) envs.  Adds {key: [(step, body name, impulse[6])]} to by_take and drops the calls from the log."""
        calls = self.log[first_call:]
        del self.log[first_call:]
        for k in keys:
            self.by_take.setdefault(k, [])
        if not calls:
            return
        t = torch.stack([c[0] for c in calls], 0).cpu().numpy(); ent = torch.stack([c[1] for c in calls], 0).cpu().numpy()
        imp = torch.stack([c[2] for c in calls], 0).double().cpu().numpy()
        for e, key in enumerate(keys):
            for s in range(min(len(calls), active.shape[0])):
                if active[s, e] and ent[s, e] >= 0:
                    self.by_take[key].append((int(t[s, e]), SMPL_BODY_NAMES[int(ent[s, e])], imp[s, e].tolist()))


def add_push_arguments(parser):
    """the five flags of the training / evaluation scripts; all default to off"""
    parser.add_argument("--push_impulse", type=float, nargs="+", default=None, metavar=("LO", "HI"), help="push with a linear impulse of LO [.. HI] N s (off by default)")
    parser.add_argument("--push_interval", type=int, default=30, help="steps of an env's episode clock between pushes")
    parser.add_argument("--push_prob", type=float, default=1.0, help="probability of a push when one falls due")
    parser.add_argument("--push_bodies", type=str, default="Pelvis", help="comma-separated body names a push draws from")
    parser.add_argument("--push_seed", type=int, default=0)
    return parser


def schedule_from_args(args, n_envs, device, record=False):
    """the PushSchedule the flags ask for; None when --push_impulse is absent (then nothing changes)"""
    if args.push_impulse is None:
        return None
    if len(args.push_impulse) > 2:
        raise SystemExit("--push_impulse takes LO [HI]")
    return PushSchedule(n_envs, device, args.push_interval, args.push_prob, tuple(b for b in args.push_bodies.split(",") if b), tuple(args.push_impulse),
                        seed=args.push_seed, record=record)
