"""GPU: the gradient kernels of the kinematic roll-out (kp_kin_tape.hip) and the taped roll-out on top of them (kinpoly_amd/kin_tape.py).

Reference of the row-level sweeps: fp64 autograd of tests/kin_tape_oracle.py (the forward kernels' own formulas) on the CPU.  Yardstick: the same
restatement in fp32 on the device.  Rule (tests/test_gpu_uhc_takes.py's): kernel error <= 2 x yardstick error + 1e-6 x max |reference|, per output
array, over ALL rows -- the edge rows of kin_tape_oracle.edge_rows included.  Every figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kin_tape_oracle as KO
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
DT = 1.0 / 30.0
LAYOUTS = {105: (False, True, True), 101: (False, True, False), 180: (True, True, True), 176: (True, True, False), 85: (False, False, True), 160: (True, False, True)}
SIZES = (1, 63, 64, 65, 257)
_CACHE = {}


def _dev():
    return torch.device("cuda", 0)


def _kpm():
    if "kpm" not in _CACHE:
        from kinpoly_amd.model_compiler import DEFAULT_KPM, read_kpm
        _CACHE["kpm"] = read_kpm(DEFAULT_KPM)
    return _CACHE["kpm"]


def _sim(width, n=257):
    """one physics-free handle per layout, shared by the tests"""
    from kinpoly_amd import sim as kp
    key = ("sim", width, n)
    if key not in _CACHE:
        vel, head, action = LAYOUTS.get(width, (False, False, False))
        _CACHE[key] = kp.KpSim(kp.KpModel(**kp.ar_obs_options(vel, head, action)), n)
    return _CACHE[key]


def _rule(name, got, yard, ref):
    ref = ref.double().cpu().numpy()
    ek, ey = float(np.abs(got.double().cpu().numpy() - ref).max()), float(np.abs(yard.double().cpu().numpy() - ref).max())
    mx = float(np.abs(ref).max())
    print(f"{name}: kernel {ek:.3e}  yardstick {ey:.3e}  max|ref| {mx:.3e}")
    assert np.isfinite(ek) and ek <= 2 * ey + 1e-6 * mx, (name, ek, ey, mx)


# ---------------------------------------------------------------- the kinematic step
def _kin_case(n):
    """inputs, cotangents and the fp64 reference of n rows (computed once)"""
    key = ("kin", n)
    if key not in _CACHE:
        q, a = KO.edge_rows(n, seed=n)
        g = torch.Generator().manual_seed(10 + n)
        gn, gv = torch.randn(n, 76, generator=g, dtype=torch.float64), torch.randn(n, 75, generator=g, dtype=torch.float64)
        q32, a32 = q.float().double(), a.float().double()          # the reference differentiates at the fp32 inputs the kernel gets
        qr, ar = q32.clone().requires_grad_(True), a32.clone().requires_grad_(True)
        nxt, qv = KO.kin_advance(qr, ar, DT)
        ((nxt * gn.float().double()).sum() + (qv * gv.float().double()).sum()).backward()
        _CACHE[key] = (q.float(), a.float(), gn.float(), gv.float(), qr.grad, ar.grad, nxt.detach(), qv.detach())
    return _CACHE[key]


def _kin_yardstick(q, a, gn, gv):
    qr, ar = q.clone().requires_grad_(True), a.clone().requires_grad_(True)
    nxt, qv = KO.kin_advance(qr, ar, DT)
    ((nxt * gn).sum() + (qv * gv).sum()).backward()
    return qr.grad, ar.grad


@pytest.mark.parametrize("n", SIZES)
def test_kin_advance_gradient_sweep(n):
    from kinpoly_amd import sim as kp
    q, a, gn, gv, ref_q, ref_a, ref_next, ref_qvel = _kin_case(n)
    q, a, gn, gv = (t.to(_dev()) for t in (q, a, gn, gv))
    gq, ga = kp.kin_advance_backward(q, a, DT, gn, gv)
    yq, ya = _kin_yardstick(q, a, gn, gv)
    # the restatement IS the forward kernel, edge rows included: k_kin_advance against the fp64 restatement, yardstick the fp32 restatement
    k_next, k_qvel = kp.kin_advance(q, a, DT)
    with torch.no_grad():
        y_next, y_qvel = KO.kin_advance(q, a, DT)
    _rule(f"kin_advance n={n} forward next_qpos", k_next, y_next, ref_next)
    _rule(f"kin_advance n={n} forward qvel", k_qvel, y_qvel, ref_qvel)
    _rule(f"kin_advance n={n} grad_qpos", gq, yq, ref_q)
    _rule(f"kin_advance n={n} grad_action", ga, ya, ref_a)
    if n >= 7:          # row 0, the `no rotation` row: the angular velocity's cotangent reaches neither the action nor the pose; row 1 (1e-4 rad) does
        gw = torch.zeros_like(gv); gw[:, 3:6] = gv[:, 3:6]
        gq_w, ga_w = kp.kin_advance_backward(q, a, DT, None, gw)
        assert float(ga_w[0].abs().max()) == 0.0 and float(gq_w[0].abs().max()) == 0.0 and float(ga_w[1, 77:].abs().max()) > 0.0
        gq_0, ga_0 = kp.kin_advance_backward(q, a, DT, None, None)          # null cotangents are zero
        assert float(ga_0.abs().max()) == 0.0 and float(gq_0.abs().max()) == 0.0


# ---------------------------------------------------------------- observation + forward kinematics
def _obs_case(n, width):
    key = ("obs", n, width)
    if key not in _CACHE:
        vel, head, action = LAYOUTS[width]
        kpm = _kpm()
        q, _ = KO.edge_rows(n, seed=100 + n)
        tabs = KO.frame_tables(n, seed=n)
        g = torch.Generator().manual_seed(20 + n + width)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()      # noqa: E731
        v, go, gw, gj = r(n, 75), r(n, width), r(n, 72), r(n, 7)
        body_pos = torch.tensor(kpm["body_pos"], dtype=torch.float64).view(24, 3).float().double()
        qr, vr = q.float().double().requires_grad_(True), v.double().requires_grad_(True)
        obs, wb, obj = KO.observe_frame(qr, vr, body_pos, kpm["body_parent"], tuple(t.float().double() for t in tabs), vel=vel, head=head, action=action)
        ((obs * go.double()).sum() + (wb * gw.double()).sum() + (obj * gj.double()).sum()).backward()
        _CACHE[key] = (q.float(), v, tuple(t.float() for t in tabs), go, gw, gj, qr.grad, vr.grad if vel else None, obs.detach(), wb.detach())
    return _CACHE[key]


def _obs_ctx(sim, tabs, n):
    """kp_ctx of one frame (T = 1) on a handle of sim.n >= n rows: the tables' first n rows are the case's"""
    N = sim.n
    pad = lambda t, fill=0.0: torch.cat([t, torch.full((N - n,) + t.shape[1:], fill, device=t.device)], 0).contiguous()      # noqa: E731
    hp, hv, orl, oh, ob = (t.to(_dev()) for t in tabs)
    hp, ob = pad(hp, 1.0), pad(ob, 1.0)
    cur = torch.zeros(N, dtype=torch.int32, device=_dev())
    return sim.make_ctx(1, hp[:, None].contiguous(), pad(hv)[:, None].contiguous(), pad(orl)[:, None].contiguous(), pad(oh), torch.zeros((N, 1, 96), device=_dev()),
                        torch.zeros((N, 1, 72), device=_dev()), cur, obj_qpos=ob)


def _obs_kernel(sim, ctx, q, go, gw, gj):
    f = sim.fk(q)
    gq, gv, ghp, ghq = sim.obs_ar_backward(ctx, q, f["wbpos"], f["wbquat"], go, gj)
    return sim.fk_head_backward(q, f["wbpos"], f["wbquat"], gw, ghp, ghq, gq), gv


def _obs_yardstick(q, v, tabs, go, gw, gj, width):
    vel, head, action = LAYOUTS[width]
    kpm = _kpm()
    body_pos = torch.tensor(kpm["body_pos"], dtype=torch.float32, device=q.device).view(24, 3)
    qr, vr = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    obs, wb, obj = KO.observe_frame(qr, vr, body_pos, kpm["body_parent"], tuple(t.to(q.device) for t in tabs), vel=vel, head=head, action=action)
    ((obs * go).sum() + (wb * gw).sum() + (obj * gj).sum()).backward()
    return qr.grad, vr.grad if vel else None


def _obs_sweep(n, width):
    q, v, tabs, go, gw, gj, ref_q, ref_v, ref_obs, ref_wb = _obs_case(n, width)
    q, v, go, gw, gj = (t.to(_dev()) for t in (q, v, go, gw, gj))
    sim = _sim(width)
    ctx = _obs_ctx(sim, tabs, n)
    gq, gv = _obs_kernel(sim, ctx, q, go, gw, gj)
    yq, yv = _obs_yardstick(q, v, tabs, go, gw, gj, width)
    # the restatement IS the forward kernels, edge rows included: set_state + kp_sim_obs_ar and kp_sim_fk on these rows (the handle's other rows repeat row 0)
    rows = lambda t: torch.cat([t, t[:1].expand(sim.n - n, -1)], 0).contiguous()      # noqa: E731
    sim.set_state(rows(q), rows(v))
    vel, head, action = LAYOUTS[width]
    kpm = _kpm()
    with torch.no_grad():
        y_obs, y_wb, _ = KO.observe_frame(q, v, torch.tensor(kpm["body_pos"], dtype=torch.float32, device=q.device).view(24, 3), kpm["body_parent"],
                                          tuple(t.to(q.device) for t in tabs), vel=vel, head=head, action=action)
    _rule(f"obs+fk {width} n={n} forward obs", sim.obs_ar(ctx)[:n], y_obs, ref_obs)
    _rule(f"obs+fk {width} n={n} forward wbpos", sim.fk(q)["wbpos"], y_wb, ref_wb)
    _rule(f"obs+fk {width} n={n} grad_qpos", gq, yq, ref_q)
    if ref_v is not None:
        _rule(f"obs+fk {width} n={n} grad_qvel", gv, yv, ref_v)
    else:
        assert gv is None


@pytest.mark.parametrize("n", SIZES)
def test_obs_fk_gradient_sweep(n):
    _obs_sweep(n, 105)


@pytest.mark.parametrize("width", sorted(LAYOUTS))
def test_obs_fk_gradient_six_layouts(width):
    _obs_sweep(65, width)


# ---------------------------------------------------------------- bits
def test_gradients_do_not_depend_on_batch_position_or_run():
    """row 200 of 257 alone and in place: the same bits; two runs: the same bits"""
    from kinpoly_amd import sim as kp
    n, r = 257, 200
    q, a, gn, gv = _kin_case(n)[:4]
    q, a, gn, gv = (t.to(_dev()) for t in (q, a, gn, gv))
    gq, ga = kp.kin_advance_backward(q, a, DT, gn, gv)
    gq2, ga2 = kp.kin_advance_backward(q, a, DT, gn, gv)
    assert torch.equal(gq, gq2) and torch.equal(ga, ga2)
    sq, sa = kp.kin_advance_backward(*(t[r:r + 1].contiguous() for t in (q, a)), DT, *(t[r:r + 1].contiguous() for t in (gn, gv)))
    assert torch.equal(sq[0], gq[r]) and torch.equal(sa[0], ga[r])
    for width in (105, 180):
        q, v, tabs, go, gw, gj = _obs_case(n, width)[:6]
        q, go, gw, gj = (t.to(_dev()) for t in (q, go, gw, gj))
        sim = _sim(width)
        ctx = _obs_ctx(sim, tabs, n)
        g1, v1 = _obs_kernel(sim, ctx, q, go, gw, gj)
        g2, v2 = _obs_kernel(sim, ctx, q, go, gw, gj)
        assert torch.equal(g1, g2) and (v1 is None or torch.equal(v1, v2))
        one = lambda t: t[r:r + 1].contiguous()      # noqa: E731
        s1, sv = _obs_kernel(sim, _obs_ctx(sim, tuple(one(t) for t in tabs), 1), one(q), one(go), one(gw), one(gj))
        assert torch.equal(s1[0], g1[r]) and (sv is None or torch.equal(sv[0], v1[r]))


# ---------------------------------------------------------------- the taped roll-out
class _Coins:
    def __init__(self, seq):
        self.seq = iter(int(x) for x in seq)

    def binomial(self, n, p):
        return next(self.seq)


def _fixture_setup(g, dtype=torch.float32):
    """the seeded network and inputs of tests/golden/pretrain.npz on the device (tests/test_pretrain_cpu.py's set-up) + a TorchFK on a 3-row handle"""
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.supervised import TorchFK
    net = TrajARNet(state_dim=int(g["state_dim"]), context_dim=int(g["context_dim"]))
    shapes = [tuple(int(x) for x in row if x > 0) for row in g["shapes"]]
    sd = O.seeded_state_dict(list(zip([str(k) for k in g["keys"]], shapes)), int(g["seed"]))
    for k in sd:
        if k.startswith(("action_fc", "context_fc")):
            sd[k] = sd[k] * 0.05
    net.load_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in sd.items()}, strict=False)
    net = net.to(_dev(), dtype)
    data = {k[3:]: torch.tensor(g[k], dtype=dtype, device=_dev()) for k in g.files if k.startswith("in_")}
    kpm = _kpm()
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), dtype=dtype, sim=_sim(105, 3) if dtype == torch.float32 else None)
    return net, fk, data


def _random_clips(B, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.stack([KO.edge_rows(B, seed=seed + t)[0][torch.randperm(B, generator=g)] for t in range(T)], 1)
    tabs = [KO.frame_tables(B, seed=seed + 50 + t) for t in range(T)]
    hp, hv, orl, _, ob = (torch.stack([tb[i] for tb in tabs], 1) for i in range(5))
    data = {"qpos": q, "qvel": torch.randn(B, T, 75, generator=g, dtype=torch.float64), "head_pose": hp, "head_vels": hv, "obj_head_relative_poses": orl,
            "obj_pose": ob, "action_one_hot": tabs[0][3]}
    return {k: v.float().to(_dev()).contiguous() for k, v in data.items()}


def _identity(net, fk, data, sim):
    from kinpoly_amd import kin_tape
    with torch.no_grad():          # the network's no-grad form, as TrajARNet.rollout runs it: then every launch of the two roll-outs is the same kernel
        pred = kin_tape.forward_supervised_taped(net, fk, data)
        q0, v0, _ = net.init_states(data, keep_feat=False)
        Q, V, A = net.rollout(data, sim, q0.contiguous(), v0.contiguous())
    for k, want in (("qpos", Q), ("qvel", V), ("action", A)):
        assert torch.equal(pred[k], want), k
    assert pred["pred_wbpos"].shape == (Q.shape[0], Q.shape[1], 72) and pred["obj_2_head"].shape == (Q.shape[0], Q.shape[1], 7)


def test_taped_forward_is_the_untaped_rollout_bit_for_bit(golden):
    """gt_rate = 0, no noise: qpos, qvel and action of the taped roll-out equal TrajARNet.rollout's, on the fixture's 3 x 6 inputs and on 65 random clips x 5"""
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.supervised import TorchFK
    net, fk, data = _fixture_setup(golden("pretrain"))
    _identity(net, fk, data, _sim(105, 3))
    torch.manual_seed(1)
    small = TrajARNet(rnn_hdim=128, mlp_hsize=(64, 32, 32)).to(_dev())
    kpm = _kpm()
    sim = _sim(105, 65)
    _identity(small, TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), sim=sim), _random_clips(65, 5), sim)


@pytest.mark.parametrize("tag,rate", [("", 0.0), ("_gt", 0.3)])
def test_taped_loss_and_gradients_against_the_reference_fixture(golden, tag, rate):
    """tests/golden/pretrain.npz (the reference's loss and four parameter gradients, without coins and with coins 0, 0, 1, 0, 1, 0): the taped fp32 path
    against the fixture, yardstick the untaped fp32 device path (forward_supervised) against the same fixture."""
    from kinpoly_amd import kin_tape
    from kinpoly_amd.pretrain import compute_loss, forward_supervised
    g = golden("pretrain")
    out = {}
    for name, fwd in (("taped", kin_tape.forward_supervised_taped), ("torch", forward_supervised)):
        net, fk, data = _fixture_setup(g)
        pred = fwd(net, fk, data, gt_rate=rate, rng=_Coins(g["coins"]))
        loss, _ = compute_loss(pred, data)
        loss.backward()
        out[name] = (pred, loss.detach(), {k: p.grad for k, p in net.named_parameters()})
        if rate > 0:          # the coins put exactly those frames on the ground-truth pose
            for t in range(1, data["qpos"].shape[1]):
                assert bool(torch.equal(pred["qpos"][:, t], data["qpos"][:, t])) == bool(g["coins"][t]), (name, t)
    for k in ("qpos", "qvel", "action", "obj_2_head", "pred_wbpos"):
        _rule(f"fixture{tag} {k}", out["taped"][0][k].detach().reshape(g[k + tag].shape), out["torch"][0][k].detach().reshape(g[k + tag].shape), torch.tensor(g[k + tag]))
    _rule(f"fixture{tag} loss", out["taped"][1].reshape(1), out["torch"][1].reshape(1), torch.tensor(float(g["loss" + tag])).reshape(1))
    n = 0
    for key in g.files:
        if key.startswith(f"grad{tag}:"):
            p = key.split(":", 1)[1]
            _rule(f"fixture{tag} grad {p}", out["taped"][2][p], out["torch"][2][p], torch.tensor(g[key]))
            n += 1
    assert n == 4


def test_refusals():
    from kinpoly_amd import kin_tape
    from kinpoly_amd import pretrain as P
    from kinpoly_amd import sim as kp
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.supervised import TorchFK
    L = kp.load_library()
    err = lambda: L.kp_last_error().decode()      # noqa: E731
    n = 4
    z = lambda *s: torch.zeros(s, device=_dev())      # noqa: E731
    P_ = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    q, a, gq, ga = z(n, 76), z(n, 80), z(n, 76), z(n, 80)
    q[:, 3] = 1.0
    assert L.kp_kin_advance_backward(n, None, P_(a), DT, None, None, P_(gq), P_(ga), None) == -1 and "null" in err()
    assert L.kp_kin_advance_backward(n, P_(q), P_(a), DT, None, None, None, P_(ga), None) == -1 and "null" in err()
    assert L.kp_kin_advance_backward(-1, P_(q), P_(a), DT, None, None, P_(gq), P_(ga), None) == -1 and "n < 0" in err()
    assert L.kp_kin_advance_backward(0, P_(q), P_(a), DT, None, None, P_(gq), P_(ga), None) == 0
    sim = _sim(105, 65)
    tabs = KO.frame_tables(n, seed=0)
    ctx = _obs_ctx(sim, tuple(t.float() for t in tabs), n)
    wb, wq, go, hp, hq = z(n, 72), z(n, 96), z(n, 105), z(n, 3), z(n, 4)
    args = lambda **k: [k.get("sim", sim.h), k.get("ctx", C.byref(ctx)), k.get("n", n), k.get("w", 105), k.get("q", P_(q)), P_(wb), P_(wq), k.get("go", P_(go)), None,      # noqa: E731
                        k.get("gq", P_(gq)), None, P_(hp), P_(hq)]
    assert L.kp_sim_obs_ar_backward(*args(w=101)) == -1 and "101 wide" in err()
    assert L.kp_sim_obs_ar_backward(*args(n=-1)) == -1 and "n_rows" in err()
    assert L.kp_sim_obs_ar_backward(*args(n=66)) == -1 and "n_rows" in err()
    assert L.kp_sim_obs_ar_backward(*args(q=None)) == -1 and "null" in err()
    assert L.kp_sim_obs_ar_backward(*args(gq=None)) == -1 and "null" in err()
    assert L.kp_sim_obs_ar_backward(*args(ctx=None)) == -1 and "context" in err()
    assert L.kp_sim_obs_ar_backward(*args(sim=None)) == -1 and "null sim" in err()
    assert L.kp_sim_obs_ar_backward(*args(n=0)) == 0
    s81 = kp.KpSim(kp.KpModel(ar_obs_head=0, ar_obs_action=0), 8)
    assert s81.obs_ar_dim == 81
    assert L.kp_sim_obs_ar_backward(*args(sim=s81.h, w=81)) == -1 and "81-d layout" in err()
    assert L.kp_sim_fk_head_backward(sim.h, n, None, P_(wb), P_(wq), None, None, None, None, P_(gq)) == -1 and "null" in err()
    assert L.kp_sim_fk_head_backward(sim.h, n, P_(q), P_(wb), P_(wq), None, None, None, None, None) == -1 and "null output" in err()
    assert L.kp_sim_fk_head_backward(sim.h, -2, P_(q), P_(wb), P_(wq), None, None, None, None, P_(gq)) == -1 and "n_rows < 0" in err()
    assert L.kp_sim_fk_head_backward(sim.h, 0, P_(q), P_(wb), P_(wq), None, None, None, None, P_(gq)) == 0
    with pytest.raises(ValueError, match="grad_obs"):          # the binding's own width check
        sim.obs_ar_backward(ctx, q, wb, wq, z(n, 105)[:, :101], None)
    # fused=True with fp64 master copies: refused with the reason, before anything runs
    kpm = _kpm()
    net64 = TrajARNet(rnn_hdim=16, mlp_hsize=(16, 8, 8)).to(_dev()).double()
    fk64 = TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), dtype=torch.float64)
    with pytest.raises(ValueError, match="fp32 HIP kernels"):
        P.train_full_supervised(net64, None, fk64, None, fused=True)
    net81 = TrajARNet(rnn_hdim=16, mlp_hsize=(16, 8, 8), state_dim=81, context_dim=4).to(_dev())
    with pytest.raises(ValueError, match="81-d"):
        kin_tape.check_fused(net81, TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), sim=s81))


def test_fused_training_smoke():
    """sixteen synthetic clips x 12 frames, three epochs with fused=True: the loss falls and every parameter of the context and action networks has a finite gradient"""
    from kinpoly_amd import dataset as D
    from kinpoly_amd import pretrain as P
    from kinpoly_amd import sim as kp
    from kinpoly_amd.context import TrajARNet
    from kinpoly_amd.model_compiler import read_kpm
    from kinpoly_amd.supervised import TorchFK
    import os
    std = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "standing_neutral.npz"))
    sim = _sim(105, 16)
    takes = D.synthetic_takes(sim, std["qpos"], n_per_action=4, T_range=(12, 13), body_mass=read_kpm(kp.STEP_KPM)["body_mass"], seed=2)
    ds = D.StateARDataset(takes, fr_num=12, seed=3, device=_dev())
    assert ds.get_len() == 16
    torch.manual_seed(0)
    net = TrajARNet(rnn_hdim=128, mlp_hsize=(128, 64, 64)).to(_dev())
    kpm = _kpm()
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), sim=sim)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    losses = [P.train_full_supervised(net, opt, fk, ds, num_epoch=1, scheduled_sampling=0.3, num_sample=64, batch_size=16, rng=np.random.RandomState(0), fused=True)
              for _ in range(3)]
    print("fused training losses:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    for k, p in net.named_parameters():
        if k.startswith(("context_", "action_rnn", "action_mlp", "action_fc")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_exp_arnet_trains_and_tests_the_reference_width_on_both_paths(tmp_path):
    """kinpoly_amd.exp_arnet (scripts/exp_arnet_all.py's functions) with the reference's as_policy=False network -- 101-wide state, 17-wide context -- on a
    small synthetic set: one epoch of train_epoch on the torch path and one on the taped path (finite losses, the schedule's clip length), a checkpoint
    round trip, and test_takes' result dict for every take"""
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import sim as kp
    from kinpoly_amd.model_compiler import read_kpm
    from kinpoly_amd.supervised import TorchFK
    import os
    std = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "standing_neutral.npz"))
    torch.manual_seed(0)
    net = E.build_net(rnn_hdim=128, mlp_hsize=(128, 64, 64)).to(_dev())
    assert (net.state_dim, net.context_dim) == (101, 17)
    model = kp.KpModel(kp.STEP_KPM, **E.model_options(net))
    sim = kp.KpSim(model, 8)
    assert sim.obs_ar_dim == 101
    takes = D.synthetic_takes(sim, std["qpos"], n_per_action=1, T_range=(84, 90), body_mass=read_kpm(kp.STEP_KPM)["body_mass"], seed=2)
    ds = D.StateARDataset(takes, fr_num=E.FR_NUM_START, seed=3, device=_dev())
    kpm = _kpm()
    fk = TorchFK(kpm["body_pos"], kpm["body_parent"], _dev(), sim=sim)
    for fused in (False, True):
        loss, comp, rate, fr_num = E.train_epoch(net, fk, ds, 0, 2000, 1e-4, 0.0, 8, 8, fused=fused, rng=np.random.RandomState(0))
        print(f"train_epoch fused={fused}: loss {loss:.4f}")
        assert np.isfinite(loss) and len(comp) == 8 and np.isfinite(comp).all() and (rate, fr_num) == (0.3, 80)
    path = str(tmp_path / "iter_0001.p")
    E.save_arnet(path, net)
    E.load_arnet(path, net)
    tds = D.StateARDataset(takes, data_mode="test", fr_num=E.FR_NUM_START, seed=3, device=_dev())
    res = E.test_takes(net, model, tds, _dev())
    assert set(res) == set(takes)
    for k, r in res.items():
        T = tds.data["qpos"][tds.takes.index(k)].shape[0]
        assert r["qpos"].shape == (T, 76) and r["qpos_gt"].shape == (T, 76) and r["obj_pose"].shape[0] == T and np.isfinite(r["qpos"]).all()
