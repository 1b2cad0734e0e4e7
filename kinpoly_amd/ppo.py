"""GAE + PPO update: the replacement of estimate_advantages / update_policy / ppo_loss / update_value / update_controller / update_policy_joint
(uhc/khrylib/rl/core/common.py:5-25; kin_poly/core/agent_ar.py:756-870; uhc/khrylib/rl/agents/agent_ppo.py:53-65) on env-major [N, T, .] batches.
No environment in here: the kinematic agent (`PPOTrainer`, through kinpoly_amd/update.py) and the UHC agent (uhc_env.CopycatAgent) build their update
from the functions below (collectives, GAE, the surrogate, `value_step`, `optimizer_step`) and say themselves only where the value steps sit, which
forward gives the means, what the loss is and which clip rule holds.  Across GPUs: one all-gather of advantages / returns, one gradient all-reduce.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import sim as kpsim
from .nets import KinPolicy, Value, gaussian_log_prob


FORCE_COLLECTIVES = False      # tests: run the all-gather / all-reduce even in a 1-rank group (so a 1-GPU box pushes device tensors through RCCL)


def _collective_on(group=None):
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or FORCE_COLLECTIVES)


def normalize_advantages_global(adv: torch.Tensor, ret: torch.Tensor, group=None):
    """The reference normalises advantages over its whole concatenated batch (common.py:22, unbiased std).
    Sharded over ranks, the per-rank advantages / returns are all-gathered (one RCCL all-gather over xGMI per
    PPO iteration; gloo in the CPU tests) so every rank applies the whole-job mean / std.  Returns
    (normalised local adv, local ret, gathered returns [world * n])."""
    if _collective_on(group):
        ws = dist.get_world_size(group)
        packed = torch.stack([adv.reshape(-1), ret.reshape(-1)], 1).contiguous()
        gathered = [torch.empty_like(packed) for _ in range(ws)]
        dist.all_gather(gathered, packed, group=group)
        all_adv = torch.cat([g[:, 0] for g in gathered]); all_ret = torch.cat([g[:, 1] for g in gathered])
    else:
        all_adv, all_ret = adv.reshape(-1), ret.reshape(-1)
    return (adv - all_adv.mean()) / all_adv.std(), ret, all_ret


def gae_scan(rewards, masks, values, gamma, tau, last_values=None):
    """estimate_advantages' recurrence (common.py:11-19) as a reverse scan over the time axis of env-major [N, T] tensors, in the tensors' own
    dtype: the fp64 update (`update_dtype=torch.float64`) and CPU tensors go through this; fp32 device tensors through k_gae.  The reference
    scans one flat batch whose workers' rows end on `masks == 0`; an env's row here may be cut by the horizon, then `last_values` [N] = V of
    the state after the last row enters as the value behind it (kp_gae_bootstrap's rule)."""
    N, T = rewards.shape
    adv = torch.empty_like(values)
    prev_v = torch.zeros(N, dtype=values.dtype, device=values.device) if last_values is None else last_values.to(values.dtype)
    prev_a = torch.zeros(N, dtype=values.dtype, device=values.device)
    for t in range(T - 1, -1, -1):
        delta = rewards[:, t] + gamma * prev_v * masks[:, t] - values[:, t]
        prev_a = delta + gamma * tau * prev_a * masks[:, t]
        adv[:, t] = prev_a
        prev_v = values[:, t]
    return adv, values + adv


def estimate_advantages(rewards, masks, values, gamma, tau, group=None, last_values=None):
    """GAE on the device (k_gae, env-major reverse scan; `gae_scan` for fp64 / CPU tensors) + the global normalisation above."""
    if values.is_cuda and values.dtype == torch.float32:
        adv, ret = kpsim.gae(rewards.contiguous(), masks.contiguous(), values.contiguous(), gamma, tau,
                             None if last_values is None else last_values.contiguous())
    else:
        adv, ret = gae_scan(rewards.to(values.dtype), masks.to(values.dtype), values, gamma, tau, last_values)
    adv, ret, _ = normalize_advantages_global(adv, ret, group)
    return adv, ret


def _allreduce_grads(params, group=None):
    """Mean of the ranks' gradients over a FIXED parameter list: every rank sends one flat buffer of the same length whatever its own backward
    reached (a parameter without a gradient on this rank -- scheduled sampling threw the context network's output away here but not there --
    contributes zeros), plus one flag per parameter, so that a parameter NO rank has a gradient for keeps `grad = None` and its optimiser state
    untouched, exactly as in a single process (ranks with different None sets used to call all_reduce with different lengths)."""
    if not _collective_on(group):
        return
    params = [p for p in params if p.requires_grad]
    if not params:
        return
    ref = params[0]
    flat = torch.cat([(p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel(), dtype=p.dtype, device=p.device)).to(ref.dtype) for p in params]
                     + [torch.tensor([0.0 if p.grad is None else 1.0 for p in params], dtype=ref.dtype, device=ref.device)])
    dist.all_reduce(flat, group=group)
    n_flags = len(params)
    have = (flat[-n_flags:] > 0).tolist()
    flat = flat[:-n_flags] / dist.get_world_size(group)
    off = 0
    for p, h in zip(params, have):
        n = p.numel()
        if h:
            g = flat[off:off + n].view_as(p).to(p.dtype)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
        off += n


def ppo_surrogate(log_probs, fixed_log_probs, advantages, clip_epsilon=0.2, ind=None):
    """AgentPPO.ppo_loss (uhc/khrylib/rl/agents/agent_ppo.py:58-65): clipped surrogate over the rows `ind` (the `exps` mask)."""
    if ind is not None:
        log_probs, fixed_log_probs, advantages = log_probs[ind], fixed_log_probs[ind], advantages[ind]
    ratio = torch.exp(log_probs - fixed_log_probs)
    return -torch.min(ratio * advantages, torch.clamp(ratio, 1.0 - clip_epsilon, 1.0 + clip_epsilon) * advantages).mean()


def lambda_lr(optimizer, nepoch_fix, nepoch):
    """get_scheduler(policy='lambda') (uhc/khrylib/utils/torch.py:166-171): lr factor 1 for nepoch_fix epochs, then linear decay."""
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda epoch: 1.0 - max(0, epoch - nepoch_fix) / float(nepoch - nepoch_fix + 1))


def value_targets(value, flat_states, rewards, masks, gamma, tau, group=None, last_states=None):
    """V of every row under the value net as it stands ([N * T, .] -> [N, T]; `last_states` [N, .]: the observation behind each env's last row, whose V
    bootstraps a row cut by the horizon) -> normalised advantages and returns, [N * T, 1] each."""
    N, T = rewards.shape
    with torch.no_grad():
        values = value(flat_states).view(N, T)
        last_v = None if last_states is None else value(last_states).view(N)
    adv, ret = estimate_advantages(rewards, masks, values, gamma, tau, group, last_v)
    return adv.reshape(-1, 1), ret.reshape(-1, 1)


def optimizer_step(opt, loss, group=None, max_norm=None):
    """zero_grad -> backward -> mean of the ranks' gradients over the optimiser's own (fixed) parameter list -> clip to `max_norm` (None: no clip) ->
    step.  Returns the norm the clip saw, on the device."""
    params = [p for g in opt.param_groups for p in g["params"]]
    opt.zero_grad(); loss.backward()
    _allreduce_grads(params, group)
    norm = None if max_norm is None else torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    return norm


def value_step(value, opt_v, flat_states, ret, group=None):
    """`update_value` (agent_ppo.py:53-56): one regression step of the value net onto the fixed targets `ret`; returns the loss it stepped on"""
    vloss = (value(flat_states) - ret).pow(2).mean()
    optimizer_step(opt_v, vloss, group)
    return vloss


class PPOTrainer:
    """AgentPPO.update_policy / ppo_loss / update_value (agent_ar.py:756-772, 852-870; agent_ppo.py:53-56), the LambdaLR schedules of
    agent_ar.py:215-225 stepped once per iteration (`per_epoch_update`, :268-269), and `update_controller` (:774-794) for
    joint_controller runs.

    The optimiser owns the kinematic policy's parameters ONLY, as the reference's does (`Adam(self.policy_net.parameters())`,
    agent_ar.py:184-199; `policy_grad_clip=[(self.policy_net.parameters(), 40)]`, :93): `joint_controller` appends env.cc_policy to
    update_modules / sample_modules (:97-99, train / eval mode and device moves), not to the optimiser.  The reference's
    update_controller therefore back-propagates the surrogate into the UHC and then steps an optimiser that does not hold the UHC
    weights: the UHC is never trained there, and neither is it here by default.  `train_uhc=True` is this engine's opt-in extension:
    the UHC gets its own Adam (same lr / weight decay) and its own 40-norm clip, so that the kinematic policy's clip is untouched."""

    def __init__(self, policy: KinPolicy, value: Value, gamma=0.95, tau=0.95, clip_epsilon=0.2, policy_lr=1e-5, value_lr=3e-4,
                 num_optim_epoch=10, policy_grad_clip=40.0, group=None, num_epoch_fix=100, num_epoch=10000, value_opt_niter=1,
                 cc_policy=None, policy_weightdecay=0.0, value_weightdecay=0.0, train_uhc=False, reference_bugs=True):
        """policy / value: the modules the optimisers own.  Their dtype is the update's dtype: fp32 modules on the device run the fused HIP re-unroll
        and k_gae; fp64 modules (the reference trains in fp64, scripts/train_ar_policy.py:76-77) run the same update through the GRUCell loop and
        `gae_scan` -- `AgentAR(update_dtype=torch.float64)` keeps such fp64 master copies and writes them back into the fp32 roll-out modules.

        reference_bugs (default True: results identical to the reference's): the gradient clip acts on the FIRST optimiser step of a run only.
        The reference hands `policy_grad_clip=[(self.policy_net.parameters(), 40)]` (agent_ar.py:92-93) -- a generator -- to
        clip_policy_grad (agent_ppo.py:53-56); the first clip call consumes it, every later call sees no parameters and returns 0
        (tests/golden/update_params.npz holds the norms the reference's calls reported: 45.99, 0, 0, ...).  False clips every step."""
        self.policy, self.value, self.group, self.cc_policy = policy, value, group, cc_policy
        self.reference_bugs, self._clip_calls, self.clip_norms = bool(reference_bugs), 0, []
        self.debug_reset_momentum = __import__("os").environ.get("KP_DEBUG_RESET_PPO_MOMENTUM") == "1"      # tools/update_ablation.sh only; read once, not per update
        self.gamma, self.tau, self.clip_epsilon, self.num_optim_epoch, self.policy_grad_clip = gamma, tau, clip_epsilon, num_optim_epoch, policy_grad_clip
        self.value_opt_niter = value_opt_niter
        self.opt_p = torch.optim.Adam([p for p in policy.parameters() if p.requires_grad], lr=policy_lr, weight_decay=policy_weightdecay)
        self.opt_v = torch.optim.Adam(value.parameters(), lr=value_lr, weight_decay=value_weightdecay)
        self.sched_p = lambda_lr(self.opt_p, num_epoch_fix, num_epoch)
        self.sched_v = lambda_lr(self.opt_v, num_epoch_fix, num_epoch)
        self.opt_cc = self.sched_cc = None
        if cc_policy is not None and train_uhc:
            cc_params = [p for p in cc_policy.parameters() if p.dtype.is_floating_point and p is not cc_policy.action_log_std]
            for p in cc_params:
                p.requires_grad_(True)
            self.opt_cc = torch.optim.Adam(cc_params, lr=policy_lr, weight_decay=policy_weightdecay)
            self.sched_cc = lambda_lr(self.opt_cc, num_epoch_fix, num_epoch)

    def per_epoch_update(self):
        """scheduler_policy.step(); scheduler_value.step()   (agent_ar.py:268-269, called at the top of optimize_policy)."""
        self.sched_p.step(); self.sched_v.step()
        if self.sched_cc is not None:
            self.sched_cc.step()

    def _policy_step(self, loss, opt=None):
        """one step of `opt` (default: the policy's) under the reference's clip rule: its generator of parameters was consumed by the run's first call"""
        self._clip_calls += 1
        clip = not (self.reference_bugs and self._clip_calls > 1)
        norm = optimizer_step(opt or self.opt_p, loss, self.group, self.policy_grad_clip if clip else None)
        if self._clip_calls == 1:
            self.clip_norms.append(norm.detach())              # kept on the device (read by tests / the update fixture)

    def _cast(self, t):
        """batch tensors in the update's dtype (the roll-out records fp32; an fp64 update reads them as fp64 like the reference's `.to(self.dtype)`, agent_ar.py:685-695)"""
        dt = next(self.policy.parameters()).dtype
        return None if t is None else (t if t.dtype == dt or not t.dtype.is_floating_point else t.to(dt))

    def _prepare(self, batch, bootstrap: bool):
        """what update() and update_joint() start from: (states [N, T, .], hx0, flat states, flat actions) in the update's dtype, the rows `ind` the
        surrogate is taken over (None: all), and the normalised advantages / returns [N * T, 1] under the value net as it stands"""
        N, T, _ = batch.states.shape
        states, hx0 = self._cast(batch.states), self._cast(batch.hx0)
        flat_states = states.reshape(N * T, -1)
        flat_actions = self._cast(batch.actions).reshape(N * T, -1)
        ind = None if batch.exps is None else batch.exps.reshape(-1).nonzero(as_tuple=False).squeeze(1)      # `ind = exps.nonzero()` (agent_ar.py:763, 813)
        if ind is not None and ind.numel() == N * T:
            ind = None
        adv, ret = value_targets(self.value, flat_states, self._cast(batch.rewards), self._cast(batch.masks), self.gamma, self.tau, self.group,
                                 self._cast(batch.last_states) if bootstrap else None)
        return (states, hx0, flat_states, flat_actions), ind, adv, ret

    @torch.no_grad()
    def behaviour_log_probs(self, batch):
        """[N * T, 1] log-probabilities of the batch's actions under the policy as it stands: taken before the first slice of a batch that is updated on in
        slices moves the parameters (`RolloutBatch.behaviour_log_probs`)"""
        N, T, _ = batch.states.shape
        means = self.policy.unroll(self._cast(batch.states), batch.episode_start, self._cast(batch.hx0))
        return self.policy.log_prob(means.reshape(N * T, -1), self._cast(batch.actions).reshape(N * T, -1))

    def update(self, batch, bootstrap: bool = True):
        N, T, _ = batch.states.shape
        (states, hx0, flat_states, flat_actions), ind, adv, ret = self._prepare(batch, bootstrap)
        self.last_adv, self.last_ret = adv, ret
        # the value net's steps of all epochs first: they share nothing with the policy passes (fixed targets, own optimiser).  On a side stream underneath
        # the policy epochs they DEADLOCKED on ROCm 7.2 / torch 2.10 (tools/micro/dbg_train_hang.py, profiles/r04/side_stream_hang.log) -- one stream.
        vloss, self.vloss_history = None, []
        for _ in range(self.num_optim_epoch * self.value_opt_niter):
            vloss = value_step(self.value, self.opt_v, flat_states, ret, self.group)
            self.vloss_history.append(vloss.detach())
        # fixed_log_probs (agent_ar.py:758-759) is the policy's forward at the parameters the update starts from: epoch 0's own forward, reused
        # (the reference evaluates it twice; one of its 11 policy forwards is redundant), so epoch 0's ratio is exactly 1 as it is there
        # a batch updated on in slices carries the log-probabilities under the policy that sampled it (behaviour_log_probs): the ratio is then taken against
        # those, not against parameters the earlier slices have already moved
        fixed_log_probs, surr = self._cast(batch.behaviour_log_probs), None
        self.surr_history = []                     # every epoch's surrogate, on the device (one host read at the end)
        if self.debug_reset_momentum:
            # diagnosis only (tools/update_ablation.sh, KP_DEBUG_RESET_PPO_MOMENTUM=1 read once by the constructor): Adam's first moment of the policy optimiser is
            # zeroed at the start of every iteration, to tell a stale momentum (built at parameters the supervised step updates have since moved) from a wrong gradient
            for st in self.opt_p.state.values():
                if "exp_avg" in st:
                    st["exp_avg"].zero_()
        for _ in range(self.num_optim_epoch):
            means = self.policy.unroll(states, batch.episode_start, hx0)
            log_probs = self.policy.log_prob(means.reshape(N * T, -1), flat_actions)
            if fixed_log_probs is None:
                fixed_log_probs = log_probs.detach()
            surr = ppo_surrogate(log_probs, fixed_log_probs, adv, self.clip_epsilon, ind)
            self.surr_history.append(surr.detach())
            self._policy_step(surr)
        stats = {"value_loss": float(vloss.detach()), "surr_loss": float(surr.detach())} if surr is not None else {}
        if surr is not None:
            # how far the epochs moved the policy on its own batch: the log-ratio of the LAST epoch's forward against the behaviour policy (one host read for
            # the three numbers).  A surrogate that ends above 0 is the signature of a log-ratio spread far beyond the clip range: min(r A, clip(r) A) caps the
            # gain of a sample the step moved the right way at 0.2 |A| and leaves the loss of one it moved the wrong way unbounded
            lr_ = (log_probs.detach() - fixed_log_probs).reshape(-1)
            d = torch.stack([lr_.std(), (lr_.abs() > 0.2).float().mean()]).tolist()
            stats.update(ppo_log_ratio_std=d[0], ppo_frac_outside_clip=d[1])
        if self.cc_policy is not None and batch.cc_state is not None:
            stats["cc_surr_loss"] = self.update_controller(batch, adv, ind)
        return stats

    def update_joint(self, batch, fk, grad_alternate: bool = False, epoch: int = 0, sup_optimizer=None, bootstrap: bool = True):
        """AgentAR.update_policy_joint (agent_ar.py:796-850; `grad_joint` runs): per epoch one value step, then the PPO surrogate and the
        supervised one-step loss (TrajARNet.step on the mean action + compute_loss_lite against the GT next pose) in ONE policy step,
        loss = 10 * loss_step + surr; with `grad_alternate` odd epochs take the surrogate step and even epochs the supervised step (on
        `sup_optimizer`, the reference's policy_net.optimizer, unclipped).  fk: kinpoly_amd.supervised.TorchFK."""
        from .supervised import compute_loss_lite, kinematic_step
        assert batch.curr_qpos is not None and batch.gt_target_qpos is not None, "sample with record_qpos=True"
        N, T, _ = batch.states.shape
        (states, hx0, flat_states, flat_actions), ind, adv, ret = self._prepare(batch, bootstrap)
        curr, tgt = self._cast(batch.curr_qpos).reshape(N * T, 76), self._cast(batch.gt_target_qpos).reshape(N * T, 76)
        with torch.no_grad():
            tgt_wbpos = fk.wbpos(tgt)
        stats, fixed_log_probs = {}, None
        for _ in range(self.num_optim_epoch):
            vloss = value_step(self.value, self.opt_v, flat_states, ret, self.group)
            means = self.policy.unroll(states, batch.episode_start, hx0).reshape(N * T, -1)
            log_probs = self.policy.log_prob(means, flat_actions)
            if fixed_log_probs is None:            # the forward at the starting parameters is epoch 0's own (see update())
                fixed_log_probs = log_probs.detach()
            surr = ppo_surrogate(log_probs, fixed_log_probs, adv, self.clip_epsilon, ind)
            loss_step, _ = compute_loss_lite(fk, kinematic_step(curr, means), tgt, gt_wbpos=tgt_wbpos)
            if not grad_alternate:
                self._policy_step(loss_step * 10 + surr)
            elif epoch % 2 == 1:
                self._policy_step(surr)
            else:
                optimizer_step(sup_optimizer if sup_optimizer is not None else self.opt_p, loss_step, self.group)
            stats = {"value_loss": float(vloss.detach()), "surr_loss": float(surr.detach()), "step_loss": float(loss_step.detach())}
        if self.cc_policy is not None and batch.cc_state is not None:      # update_params runs update_controller after either branch (agent_ar.py:748-749)
            stats["cc_surr_loss"] = self.update_controller(batch, adv, ind)
        return stats

    def update_controller(self, batch, adv, ind=None):
        """AgentAR.update_controller (agent_ar.py:774-794): the clipped surrogate of env.cc_policy over the recorded (cc_state, cc_action)
        with the kinematic policy's advantages; no value step.  The reference steps `optimizer_policy`, which holds policy_net's
        parameters only, after a backward that reaches the UHC only: with torch >= 2.0 (`zero_grad(set_to_none=True)`) policy_net's
        gradients are None and the step changes nothing, so its num_optim_epoch passes all evaluate the same loss -- computed once here
        and reported.  (Under torch < 2.0 the same code takes ten zero-gradient Adam steps on policy_net, i.e. momentum drift; not
        reproduced.)  With `train_uhc` the epochs run on the UHC's own optimiser."""
        pol = self.cc_policy
        dt = next(pol.parameters()).dtype
        cs, ca = batch.cc_state.reshape(-1, batch.cc_state.shape[-1]).to(dt), batch.cc_action.reshape(-1, batch.cc_action.shape[-1]).to(dt)
        adv = adv.to(dt)
        with torch.no_grad():
            fixed = gaussian_log_prob(*pol.forward(cs), ca)
            if self.opt_cc is None:
                return float(ppo_surrogate(fixed, fixed, adv, self.clip_epsilon, ind))
        loss = None
        for _ in range(self.num_optim_epoch):
            surr = ppo_surrogate(gaussian_log_prob(*pol.forward(cs), ca), fixed, adv, self.clip_epsilon, ind)
            self._policy_step(surr, self.opt_cc)
            loss = float(surr.detach())
        return loss
