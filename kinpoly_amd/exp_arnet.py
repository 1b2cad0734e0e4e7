"""Supervised training and testing of the kinematic model on its own: scripts/exp_arnet_all.py of the reference (:62-183) -- TrajARNet built
with as_policy=False (no action one-hot in its state: 101-d under kin_poly.yml, traj_ar_smpl_net.py:281-282; the context GRU still reads the
one-hot, 17-d), whole-clip roll-outs against the GT clip with a per-epoch schedule of the scheduled-sampling rate and the clip length, a fresh Adam
per epoch, checkpoints `models/iter_%04d.p` = ({'stateAR_net_dict': state_dict}, {}).  The functions behind scripts/exp_arnet_all.py.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from . import pretrain as P
from . import sim as kpsim
from .checkpoint import load_state_strict
from .context import TrajARNet

FR_NUM_START, FR_NUM_END = 80, 150         # exp_arnet_all.py:116-117
# what `scripts/exp_arnet_all.py --dtype fp32` trains on without --path: the taped roll-out, measured faster than the torch path by the rule of
# tools/warm_start_time.py --fused (DESIGN.md section 10 holds the record)
DEFAULT_PATH = "taped"
# the same for a network with a context block (kin_only.yml, use_of.yml): section 10's second record
DEFAULT_PATH_CONTEXT = "taped"


def sampling_rate_at(i_epoch: int, num_epoch: int) -> float:
    """exp_arnet_all.py:120: the scheduled-sampling rate of epoch i, 0.3 falling linearly to 0"""
    return max((1 - i_epoch / num_epoch) * 0.3, 0)


def fr_num_at(i_epoch: int, num_epoch: int) -> int:
    """exp_arnet_all.py:122: the clip length of epoch i, 80 growing to 150 in steps of 5 (the reference's expression, operator for operator)"""
    return int(FR_NUM_START + i_epoch / num_epoch * (FR_NUM_END - FR_NUM_START) // 5 * 5)


def build_net(use_vel=False, use_head=True, use_action=True, as_policy=False, use_context=False, of_dim=0, **kw) -> TrajARNet:
    """The reference's TrajARNet(as_policy=False): the state has no action one-hot whatever use_action says, the context GRU's input follows
    use_action.  as_policy: the state carries the one-hot when use_action does (the network train_ar_policy.py --load can start from) and, with
    of_dim > 0 (`use_of`), the frame's image feature (traj_ar_smpl_net.py:281-285).  use_context / of_dim: kin_only.yml / use_of.yml's context block.
    kw: rnn_hdim, mlp_hsize (Config.model_kwargs)."""
    state_action = bool(use_action) and bool(as_policy)
    ctx_block = int(kw.get("rnn_hdim", 1024)) if (use_context or of_dim) else 0
    net = TrajARNet(state_dim=ctx_block + kpsim.ar_obs_dim(use_vel, use_head, state_action) + int(of_dim) * bool(as_policy),
                    use_action=use_action, use_vel=use_vel, use_head=use_head, use_context=use_context, of_dim=of_dim, of_in_state=bool(as_policy) and bool(of_dim), **kw)
    net.obs_action = state_action          # the kinematic handle's ar_obs_action
    return net


def model_options(net) -> dict:
    """KpModel options of the kinematic handle whose observation `net` takes"""
    return kpsim.ar_obs_options(net.use_vel, net.use_head, getattr(net, "obs_action", net.use_action))


def arnet_state(net) -> dict:
    """the reference's stateAR_net_dict: TrajARNet's own parameters under its names (action_log_std belongs to PolicyAR, not to the network)"""
    return {k: v.detach().cpu() for k, v in net.state_dict().items() if k != "action_log_std"}


def save_arnet(path, net):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(({"stateAR_net_dict": arnet_state(net)}, {}), f)


def load_arnet(path, net):
    """-> net with the checkpoint's parameters; a width mismatch or a key that does not fit raises (checkpoint.load_state_strict)"""
    with open(path, "rb") as f:
        model_cp, _ = pickle.load(f)
    return load_state_strict(net, dict(model_cp["stateAR_net_dict"]), allow_missing=frozenset({"action_log_std"}), what=str(path))


def set_fr_num(dataset, fr_num: int):
    """sampling_generator(fr_num=...) of the reference: the data set serves windows of this many frames from now on"""
    dataset.fr_num = int(fr_num)
    dataset.freq_indices = np.array([i for i, q in enumerate(dataset.data["qpos"]) for _ in range(int(np.ceil(q.shape[0] / dataset.fr_num)))])


def train_epoch(net, fk, dataset, i_epoch, num_epoch, lr, weightdecay, num_sample, batch_size, noise_std=0.0, fused=False, rng=None, weights=None):
    """One epoch of exp_arnet_all.py:119-151: schedule, fresh Adam, num_sample / batch_size batches.  -> (mean loss per clip as the reference logs it
    (sum of batch losses / num_sample), the eight summed components / num_sample, sampling_rate, fr_num)"""
    rate, fr_num = sampling_rate_at(i_epoch, num_epoch), fr_num_at(i_epoch, num_epoch)
    set_fr_num(dataset, fr_num)
    forward = P.forward_supervised
    if fused:
        from . import kin_tape
        kin_tape.check_fused(net, fk)
        forward = kin_tape.forward_supervised_taped
    p0 = next(net.parameters())
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=lr, weight_decay=weightdecay)
    tot, comp = torch.zeros((), device=p0.device, dtype=p0.dtype), torch.zeros(8, device=p0.device, dtype=p0.dtype)
    for data in P.sampling_batches(dataset, num_sample, batch_size, p0.device, p0.dtype):
        pred = forward(net, fk, data, rate, rng, noise_std)
        loss, idv = P.compute_loss(pred, data, weights)
        opt.zero_grad(); loss.backward(); opt.step()
        tot += loss.detach(); comp += torch.stack([c.detach() for c in idv])
    return float(tot) / num_sample, (comp / num_sample).tolist(), rate, fr_num


@torch.no_grad()
def test_takes(net, kin_model, dataset, device):
    """eval_sequences (:31-59): every take rolled out whole with the untaped roll-out -> {take: {'qpos', 'qpos_gt', 'obj_pose'}} (numpy)"""
    out = {}
    sim = kpsim.KpSim(kin_model, 1, device.index or 0)
    for ind, take in enumerate(dataset.takes):
        data = dataset.batch([ind], [0], None)
        data = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in data.items()}
        q0, v0, ctx_feat = net.init_states(data, keep_feat=bool(net.ctx_block))      # a context block reads the sequence in every frame's observation
        Q, _, _ = net.rollout(data, sim, q0.contiguous(), v0.contiguous(), ctx_feat=ctx_feat)
        out[take] = {"qpos": Q[0].cpu().numpy(), "qpos_gt": data["qpos"][0].cpu().numpy(), "obj_pose": data["obj_pose"][0].cpu().numpy()}
    return out
