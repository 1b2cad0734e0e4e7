"""CPU: what the taped kinematic roll-out (kinpoly_amd/kin_tape.py, kp_kin_tape.hip) rests on that needs no GPU -- the torch restatement of the forward
kernels (tests/kin_tape_oracle.py) against the torch path, the schedules and checkpoints of scripts/exp_arnet_all.py, and the library's new symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kin_tape_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fk64():
    from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
    from kinpoly_amd.supervised import TorchFK
    kpm = read_kpm(DEFAULT_KPM)
    return TorchFK(kpm["body_pos"], kpm["body_parent"], "cpu", dtype=torch.float64), kpm


def test_restatement_equals_the_torch_path_on_unit_quaternions():
    """On unit quaternions the kernels' formulas and the torch path are the same function: kinematic_step + get_qvel_fd_batch and pretrain.observe in fp64
    at 1e-12.  (Unit: the torch path's _qrot does not normalise; turns of a few degrees per frame: its fp64 acos form loses 1e-16 / sin(angle / 2).)"""
    from kinpoly_amd import pretrain as P
    from kinpoly_amd.context import get_qvel_fd_batch
    from kinpoly_amd.supervised import kinematic_step
    n = 33
    g = torch.Generator().manual_seed(5)
    q, a = KO.edge_rows(n, seed=1)
    q, a = q[7:], a[7:]                                   # the random rows (unit root quaternions)
    n = q.shape[0]
    dt = 1.0 / 30.0
    nxt, qvel = KO.kin_advance(q, a, dt)
    want = kinematic_step(q, a, dt)
    np.testing.assert_allclose(nxt.numpy(), want.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(qvel.numpy(), get_qvel_fd_batch(q, want, dt).numpy(), rtol=0, atol=1e-12)
    fk, kpm = _fk64()
    hp, hv, orl, oh, ob = KO.frame_tables(n, seed=2)
    oh = oh.clone(); oh[oh.sum(1) == 0, 0] = 1.0          # pretrain.observe reads obj_pose whatever the one-hot says: compare on rows with an action
    hp = torch.cat([hp[:, :3], torch.nn.functional.normalize(hp[:, 3:], dim=1)], 1)
    v = torch.randn(n, 75, generator=g, dtype=torch.float64)
    data = {"head_pose": hp[:, None], "head_vels": hv[:, None], "obj_head_relative_poses": orl[:, None], "obj_pose": ob[:, None], "action_one_hot": oh}
    body_pos = torch.tensor(kpm["body_pos"], dtype=torch.float64).view(24, 3)
    for vel, head, action in ((False, True, True), (False, True, False), (True, True, True), (True, True, False), (False, False, True), (True, False, True)):
        obs, wb, obj = KO.observe_frame(q, v, body_pos, kpm["body_parent"], (hp, hv, orl, oh, ob), vel=vel, head=head, action=action)
        w_obs, w_wb, w_obj = P.observe(fk, q, data, 0, use_action=action, use_vel=vel, use_head=head, qvel=v)
        from kinpoly_amd.sim import ar_obs_dim
        assert obs.shape[1] == ar_obs_dim(vel, head, action)
        np.testing.assert_allclose(obs.numpy(), w_obs.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(wb.numpy(), w_wb.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(obj.numpy(), w_obj.numpy(), rtol=0, atol=1e-12)


def test_restatement_has_finite_gradients_on_the_edge_rows():
    """the branches of the restatement (zero angular action, the expmap guard) leave no NaN in its autograd, and the zero-action row's angular velocity
    carries no gradient to the action"""
    q, a = KO.edge_rows(16, seed=0)
    q.requires_grad_(True); a.requires_grad_(True)
    nxt, qvel = KO.kin_advance(q, a)
    (nxt.sum() + qvel.pow(2).sum()).backward()
    assert torch.isfinite(q.grad).all() and torch.isfinite(a.grad).all()
    q2, a2 = KO.edge_rows(16, seed=0)
    a2.requires_grad_(True)
    KO.kin_advance(q2, a2)[1][:, 3:6].sum().backward()
    assert float(a2.grad[0].abs().max()) == 0.0 and float(a2.grad[1, 77:].abs().max()) > 0.0


def test_schedules_give_the_reference_values():
    """exp_arnet_all.py:120-122 at epochs 0, 1, 999 and 1999 of 2000 (the reference's expressions evaluated by hand)"""
    from kinpoly_amd.exp_arnet import fr_num_at, sampling_rate_at
    assert [fr_num_at(i, 2000) for i in (0, 1, 999, 1999)] == [80, 80, 110, 145]
    for i, want in ((0, 0.3), (1, 0.29985), (999, 0.15015), (1999, 0.00015)):
        assert abs(sampling_rate_at(i, 2000) - want) < 1e-12
    assert sampling_rate_at(2500, 2000) == 0


def test_checkpoint_round_trip_uses_the_reference_key_names(golden, tmp_path):
    """models/iter_%04d.p = ({'stateAR_net_dict': state_dict}, {}) with the reference's parameter names (the key list of tests/golden/pretrain.npz is the
    reference TrajARNet's own); a file of that form loads, and a network of another width is refused"""
    import pickle
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd.checkpoint import CheckpointWidthError
    ref_keys = {str(k) for k in golden("pretrain")["keys"]}
    torch.manual_seed(0)
    kw = dict(rnn_hdim=16, mlp_hsize=(16, 8, 8))
    net = E.build_net(**kw)
    assert (net.state_dim, net.context_dim) == (101, 17) and E.model_options(net) == {"ar_obs_action": 0}
    pol = E.build_net(as_policy=True, **kw)
    assert (pol.state_dim, pol.context_dim) == (105, 17) and E.model_options(pol) == {}
    path = str(tmp_path / "models" / "iter_0001.p")
    E.save_arnet(path, net)
    model_cp, meta = pickle.load(open(path, "rb"))
    assert meta == {} and set(model_cp) == {"stateAR_net_dict"} and set(model_cp["stateAR_net_dict"]) == ref_keys
    other = E.build_net(**kw)
    E.load_arnet(path, other)
    for k, v in net.state_dict().items():
        assert torch.equal(v, other.state_dict()[k]), k
    # a file as the reference writes it: plain tensors under those names
    pickle.dump(({"stateAR_net_dict": {k: v.clone() for k, v in E.arnet_state(net).items()}}, {}), open(path, "wb"))
    E.load_arnet(path, E.build_net(**kw))
    with pytest.raises(CheckpointWidthError):
        E.load_arnet(path, pol)


def test_library_exports_the_tape_symbols():
    """kp_kin_advance_backward, kp_sim_obs_ar_backward, kp_sim_fk_head_backward: declared, typed and exported"""
    from kinpoly_amd import build as kpbuild
    from kinpoly_amd.sim import ABI_SYMBOLS
    if not os.path.exists(kpbuild.LIB):
        kpbuild.build_native()
    L = ctypes.CDLL(kpbuild.LIB)
    hdr = open(os.path.join(ROOT, "include", "kinpoly_sim.h")).read()
    for sym in ("kp_kin_advance_backward", "kp_sim_obs_ar_backward", "kp_sim_fk_head_backward"):
        assert hasattr(L, sym), sym
        assert sym in ABI_SYMBOLS and sym + "(" in hdr


def test_fused_refuses_what_it_cannot_run():
    """fused=True with an fp64 network, a CPU network or a TorchFK without a simulator raises with the reason (nothing runs)"""
    from kinpoly_amd import kin_tape
    from kinpoly_amd.context import TrajARNet
    fk, _ = _fk64()
    net = TrajARNet(rnn_hdim=8, mlp_hsize=(8, 8))
    with pytest.raises(ValueError, match="fp32 HIP kernels"):
        kin_tape.check_fused(net.double(), fk)
    with pytest.raises(ValueError, match="fp32 HIP kernels"):
        kin_tape.check_fused(net.float(), fk)              # fp32 but on the CPU


def test_train_epoch_on_the_torch_path_with_the_reference_width():
    """exp_arnet.train_epoch(fused=False) in fp64 on the CPU with the reference's as_policy=False network: the state is 101 wide (no one-hot) while the
    context GRU reads the one-hot (17), so the torch path must build the observation the network takes; two epochs lower the loss"""
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    fk, _ = _fk64()
    feats = {}
    for i, T in enumerate((14, 19)):
        q = np.zeros((T, 76)); q[:, 2] = 0.9; q[:, 3] = 1.0; q[:, 7:] = 0.1 * np.sin(np.arange(T)[:, None] * 0.3 + rng.uniform(0, 6, 69))
        wb = fk.wbpos(torch.tensor(q)).reshape(T, 72).numpy()
        hp = np.concatenate([wb[:, 39:42], np.tile([1.0, 0, 0, 0], (T, 1))], 1)
        feats[f"sit-{i}"] = dict(qpos=q, qvel=np.zeros((T, 75)), head_pose=hp, head_vels=np.zeros((T, 6)), action_one_hot=np.tile([1.0, 0, 0, 0], (T, 1)),
                                 obj_head_relative_poses=np.tile([0.5, 0, 0, 1.0, 0, 0, 0], (T, 1)), obj_pose=np.tile([0.5, 0, 0.4, 1.0, 0, 0, 0], (T, 1)),
                                 wbpos=wb, wbquat=np.zeros((T, 96)), bquat=np.zeros((T, 96)), of_files=["x"] * T)
    ds = D.StateARDataset(feats, fr_num=8, seed=3)
    ds.data = {k: [x.double() for x in v] for k, v in ds.data.items()}
    net = E.build_net(rnn_hdim=32, mlp_hsize=(32, 16, 16)).double()
    assert (net.state_dim, net.context_dim, net.use_action, net.obs_action) == (101, 17, True, False)
    E.FR_NUM_START, keep = 8, E.FR_NUM_START          # the schedule's clip lengths are 80 .. 150; these takes are 14 and 19 frames
    E.FR_NUM_END, keep_end = 8, E.FR_NUM_END
    try:
        losses = [E.train_epoch(net, fk, ds, i, 2000, 5e-3, 0.0, 8, 4, fused=False, rng=np.random.RandomState(0))[0] for i in range(6)]
    finally:
        E.FR_NUM_START, E.FR_NUM_END = keep, keep_end
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    with pytest.raises(ValueError, match="fp32 HIP kernels"):
        E.train_epoch(net, fk, ds, 0, 2000, 5e-3, 0.0, 8, 4, fused=True)
