"""GPU: the kinematic model's observation row with a context block and an `of` block (kinpoly_amd/csrc/kp_obs_ctx.hip: k_obs_ar_ctx through
kp_sim_obs_ar_ex, its backward, kp_gru_cell_step with a state wider than the hidden state), and the roll-outs, the taped path and kinpoly_amd.exp_arnet on top of it.

The row's three blocks are copies or the base kernel's own expressions, so the row-level checks are bit equality: the base block against
kp_sim_obs_ar on the same handle, the two wide blocks against the tables' rows at the clamped frame, h' of the wide GRU step against the D <= H
kernel, the backward's base outputs against kp_sim_obs_ar_backward on the sliced cotangent.  Against the reference's fixture
(tests/golden/ar_obs_context.npz) the rows are held to tests/test_gpu_obs_variants.py's 5e-6, and the taped roll-out to DESIGN 10's rule
(tests/test_gpu_kin_tape.py): taped error <= 2 x the fp32 torch path's + 1e-6 x max |reference|.  Every figure is printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_context_obs_cpu as CC  # noqa: E402  (the fixture's cases and its seeded networks; its tests are not collected from here)
import test_gpu_side_kernels as K  # noqa: E402  (state / context builders; nothing of it is collected from here)

LAYOUTS = {105: (False, True, True), 101: (False, True, False), 180: (True, True, True), 176: (True, True, False), 85: (False, False, True), 160: (True, False, True)}
NS = (1, 7, 8, 9, 65, 257)          # below one 8-env block, one block, one block and one env, many blocks with a partial one
HS, FS = (1, 31, 32, 33, 256), (0, 1, 33)      # around the 32-lane stride, and kin_only.yml's 256
T = 6
GUARD = 64
dev, host = K.dev, K.host


@pytest.fixture(scope="module")
def kp():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from kinpoly_amd import sim as kpsim
    yield kpsim
    K._SIMS.clear()
    torch.cuda.empty_cache()


def _guarded(n, w, fill=-7.0):
    """[n, w] view in the middle of a buffer with GUARD sentinel floats on either side"""
    buf = torch.full((GUARD + n * w + GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n * w].view(n, w)


def _guards_intact(buf, n, w, fill=-7.0):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n * w:] == fill).all())


def _same_words(got, want, what):
    """bit equality of two float32 tensors; the differing words are printed before the assert"""
    a, b = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    bad = (a != b).nonzero()
    if len(bad):
        print(f"MEASURED {what}: {len(bad)} of {a.numel()} words differ; rows {sorted(set(bad[:, 0].tolist()))[:12]} columns {sorted(set(bad[:, 1].tolist()))}; "
              f"max |difference| {float((got - want).abs().max()):.3e}")
    return len(bad) == 0


def _case(kp, width, n, seed):
    """a handle of this layout with a stored state, and a context of R = n + 5 rows read through a permuted row map, cur_t over -1, 0, T - 1, T and an interior frame"""
    sim = K.get_sim(kp, n, **kp.ar_obs_options(*LAYOUTS[width]))
    K._sim_state(kp, sim, n, seed)
    c = K._ctx(kp, sim, n, seed + 1, T=T, cur_t=np.asarray([-1, 0, T - 1, T, 2], np.int32)[np.arange(n) % 5])
    return sim, c


def _tables(R, H, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((R, T, max(H, 1)), generator=g)[:, :, :H].contiguous().cuda(), torch.randn((R, T, max(F, 1)), generator=g)[:, :, :F].contiguous().cuda()


@pytest.mark.parametrize("width", sorted(LAYOUTS))
def test_wide_row_words(kp, width):
    """every n x H x F: base block = kp_sim_obs_ar's words, context / of blocks = the tables' rows at the clamped frame through the row map, env-major and
    time-major storage, a null context table = zeros, guard words untouched"""
    for n in NS:
        sim, c = _case(kp, width, n, 3000 + n)
        ctx = K._make_ctx(sim, c)
        base = sim.obs_ar(ctx)
        R = n + 5
        row = torch.tensor(c["row"], device="cuda").long()
        tc = torch.tensor(np.clip(c["cur_t"], 0, T - 1), device="cuda").long()
        for H in HS:
            for F in FS:
                cf, of = _tables(R, H, F, 10 * H + F)
                W = H + width + F
                for time_major in (False, True):
                    a, b = (cf.transpose(0, 1).contiguous(), of.transpose(0, 1).contiguous()) if time_major else (cf, of)
                    ext = sim.make_obs_ext(T, R, H, a, b if F else None, ctx_time_major=time_major, of_time_major=time_major)
                    buf, out = _guarded(n, W)
                    got = sim.obs_ar_ex(ctx, ext, out=out)
                    assert got.data_ptr() == out.data_ptr() and _guards_intact(buf, n, W), (n, H, F, time_major)
                    assert _same_words(out[:, H:H + width], base, f"base block {width} n={n} H={H} F={F}"), (n, H, F, time_major)
                    assert torch.equal(out[:, :H], cf[row, tc]) and torch.equal(out[:, H + width:], of[row, tc]), (n, H, F, time_major)
                buf, out = _guarded(n, W)
                sim.obs_ar_ex(ctx, sim.make_obs_ext(T, R, H, None, of if F else None), out=out)          # no sequence yet: the zero block
                assert _guards_intact(buf, n, W) and bool((out[:, :H] == 0).all()) and torch.equal(out[:, H:H + width], base) and torch.equal(out[:, H + width:], of[row, tc])
    for key in [k for k in K._SIMS if k[1]]:
        del K._SIMS[key]


def test_a_row_alone_is_the_row_at_position_200_of_257(kp):
    n, r, H, F = 257, 200, 33, 33
    for width in (105, 180):
        sim, c = _case(kp, width, n, 4000)
        cf, of = _tables(n + 5, H, F, 5)
        whole = sim.obs_ar_ex(K._make_ctx(sim, c), sim.make_obs_ext(T, n + 5, H, cf, of, ctx_time_major=False))
        one = K.get_sim(kp, 1, **kp.ar_obs_options(*LAYOUTS[width]))
        K.load(one, **{k: host(sim.view(k)[r:r + 1]) for k in ("qpos", "qvel", "xpos", "xquat")})
        rr = int(c["row"][r])
        c1 = dict(c, head_pose=c["head_pose"][rr:rr + 1], head_vels=c["head_vels"][rr:rr + 1], obj_rel=c["obj_rel"][rr:rr + 1], gt_bquat=c["gt_bquat"][rr:rr + 1],
                  gt_wbpos=c["gt_wbpos"][rr:rr + 1], action_one_hot=c["action_one_hot"][rr:rr + 1], cur_t=c["cur_t"][r:r + 1], obj_qpos=c["obj_qpos"][r:r + 1],
                  row=np.zeros(1, np.int32))
        alone = one.obs_ar_ex(K._make_ctx(one, c1), one.make_obs_ext(T, 1, H, cf[rr:rr + 1].contiguous(), of[rr:rr + 1].contiguous(), ctx_time_major=False))
        assert torch.equal(alone[0], whole[r])
    for key in [k for k in K._SIMS if k[1]]:
        del K._SIMS[key]


@pytest.mark.parametrize("case", CC.CASES, ids=CC.IDS)
def test_fixture_rows(kp, golden, case):
    """the reference's get_obs rows at every frame (state set to the clip's frame, the fixture's own context sequence) and the zero block before init_states:
    5e-6, tests/test_gpu_obs_variants.py's bound on its fixture rows"""
    g = golden("ar_obs_context")
    c, o, p = case
    k = f"c{c}o{o}p{p}"
    B, Tn = g["in_qpos"].shape[:2]
    sim = kp.KpSim(kp.KpModel(**kp.ar_obs_options(False, True, bool(p))), B)
    seq = dev(g["ctx_" + k]).transpose(0, 1).contiguous()          # time-major
    of = dev(g["in_of"]) if (o and p) else None
    z = torch.zeros((B, Tn, 96), device="cuda")
    cur_t = torch.zeros(B, dtype=torch.int32, device="cuda")
    obj = torch.empty((B, 7), device="cuda")
    ctx = sim.make_ctx(Tn, dev(g["in_head_pose"]), dev(g["in_head_vels"]), dev(g["in_obj_head_relative_poses"]), dev(g["in_action_one_hot"][:, 0]), z,
                       z[:, :, :72].contiguous(), cur_t, obj_qpos=obj)
    ext, ext0 = sim.make_obs_ext(Tn, B, CC.H, seq, of), sim.make_obs_ext(Tn, B, CC.H, None, of)
    worst = 0.0
    for t in range(Tn):
        cur_t.fill_(t)
        obj.copy_(dev(g["in_obj_pose"][:, t, :7]))
        sim.set_state(dev(g["in_qpos"][:, t]), dev(g["in_qvel"][:, t]))
        got = sim.obs_ar_ex(ctx, ext)
        assert tuple(got.shape) == (B, int(g["dims_" + k][0]))
        worst = max(worst, K.worst(f"obs_ar_ex {k} frame {t} vs the reference rows", host(got), g["obs_" + k][:, t]))
        np.testing.assert_allclose(got.double().cpu().numpy(), g["obs_" + k][:, t], atol=5e-6, rtol=0)
        if t == 0:
            np.testing.assert_allclose(sim.obs_ar_ex(ctx, ext0).double().cpu().numpy(), g["obs0_" + k], atol=5e-6, rtol=0)
    print(f"MEASURED obs_ar_ex {k} worst over frames: {worst:.3e}")


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("H,D", [(32, 1), (32, 31), (32, 32), (32, 33), (32, 64), (32, 65), (256, 357)])
def test_gru_cell_step_with_a_state_wider_than_the_hidden_state(kp, n, H, D):
    """one kernel for every width: thread (e, j) copies the state's columns j, j + H, ...; D <= H (one column at most, the former `if`) is checked at 1, H - 1 and H"""
    g = torch.Generator().manual_seed(H + D + n)
    r = lambda *s: torch.randn(*s, generator=g).cuda()      # noqa: E731
    gi, gh, bi, bh, h, x = r(n, 3 * H), r(n, 3 * H), r(3 * H), r(3 * H), r(n, H), r(n, D)
    want = kp.gru_cell_step(gi, gh, bi, bh, h)                                   # no [state | h] row
    buf, xcat = _guarded(n, D + H)
    got = kp.gru_cell_step(gi, gh, bi, bh, h, x, None, xcat)
    assert torch.equal(got, want) and torch.equal(xcat[:, :D], x) and torch.equal(xcat[:, D:], want) and _guards_intact(buf, n, D + H)
    Dn = min(D, H)
    narrow = torch.empty((n, Dn + H), device="cuda")
    assert torch.equal(kp.gru_cell_step(gi, gh, bi, bh, h, x[:, :Dn].contiguous(), None, narrow), want)      # and with a row no wider than the hidden state
    h2 = h.clone()
    kp.gru_cell_step(gi, gh, bi, bh, h2, x, h2, xcat)                           # in place
    assert torch.equal(h2, want)


def test_get_action_takes_the_kernel_path_for_a_wide_state(kp):
    """KinPolicy.get_action without grad on the device, state 357 > hidden 256 (kin_only.yml's widths): the gate GEMMs + kp_gru_cell_step against GRUCell +
    cat + MLP in fp64, at tests/test_gpu_policy_kernels.py::test_kin_policy_rollout_step_is_the_module_math's bounds"""
    from kinpoly_amd.nets import KinPolicy
    torch.manual_seed(5)
    kw = dict(state_dim=357, rnn_hdim=256, mlp_hsize=(64, 32))
    pol = KinPolicy(**kw).cuda()
    s, h = torch.randn(129, 357, device="cuda"), torch.randn(129, 256, device="cuda") * 0.3
    with torch.no_grad():
        mean, h1 = pol.get_action(s, h)
        ref = KinPolicy(**kw).double()
        ref.load_state_dict({k: v.double().cpu() for k, v in pol.state_dict().items()})
        mean_r, h1_r = ref.get_action(s.double().cpu(), h.double().cpu())
    eh, ea = float((h1.double().cpu() - h1_r).abs().max()), float((mean.double().cpu() - mean_r).abs().max())
    print(f"MEASURED get_action, state 357 / hidden 256: h {eh:.3e}  action {ea:.3e}")
    assert eh < 5e-6 and ea < 2e-5


@pytest.mark.parametrize("width", sorted(LAYOUTS))
def test_wide_backward_is_the_base_backward_on_the_sliced_cotangent(kp, width):
    H, F = 33, 5
    for n in (1, 63, 64, 65):
        sim, c = _case(kp, width, n, 5000 + n)
        ctx = K._make_ctx(sim, c)
        q = sim.view("qpos").clone()
        f = sim.fk(q)
        g = torch.Generator().manual_seed(n + width)
        go, gj = torch.randn((n, H + width + F), generator=g).cuda(), torch.randn((n, 7), generator=g).cuda()
        cf, of = _tables(n + 5, H, F, 7)
        ext = sim.make_obs_ext(T, n + 5, H, cf, of, ctx_time_major=False)
        want = sim.obs_ar_backward(ctx, q, f["wbpos"], f["wbquat"], go[:, H:H + width].contiguous(), gj)
        got = sim.obs_ar_ex_backward(ctx, ext, q, f["wbpos"], f["wbquat"], go, gj)
        for a, b in zip(got[:4], want):
            assert (a is None and b is None) or torch.equal(a, b), (n, width)
        assert torch.equal(got[4], go[:, :H]) and got[4].is_contiguous()
        none = sim.obs_ar_ex_backward(ctx, sim.make_obs_ext(T, n + 5, 0, None, None), q, f["wbpos"], f["wbquat"], go[:, H:H + width].contiguous(), gj)
        assert none[4] is None and torch.equal(none[0], want[0])
    for key in [k for k in K._SIMS if k[1]]:
        del K._SIMS[key]


# ---------------------------------------------------------------- the roll-outs against the fixture
def _rule(name, got, yard, ref):
    ref = np.asarray(ref, np.float64)
    ek, ey = float(np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref).max()), float(np.abs(yard.double().cpu().numpy().reshape(ref.shape) - ref).max())
    mx = float(np.abs(ref).max())
    print(f"{name}: taped {ek:.3e}  yardstick {ey:.3e}  max|ref| {mx:.3e}")
    assert np.isfinite(ek) and ek <= 2 * ey + 1e-6 * mx, (name, ek, ey, mx)


def _device_setup(kp, g, case):
    net, data, k = CC.build(g, case, dtype=torch.float32, device="cuda")
    sim = kp.KpSim(kp.KpModel(**kp.ar_obs_options(False, True, net.obs_action)), data["qpos"].shape[0])
    return net, data, k, sim, CC.torch_fk(torch.float32, "cuda", sim)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.IDS)
def test_taped_rollout_against_the_reference_fixture(kp, golden, case):
    """loss and named gradients (context_rnn.rnn_f.weight_ih is the one that goes wrong when a frame's context cotangent is dropped) of the taped fp32 path
    against the fixture, yardstick the fp32 torch path on the device against the same fixture; and with the network in its no-grad form the taped roll-out
    is TrajARNet.rollout's bit for bit"""
    from kinpoly_amd import kin_tape
    from kinpoly_amd.pretrain import compute_loss, forward_supervised
    g = golden("ar_obs_context")
    out = {}
    for name, fwd in (("taped", kin_tape.forward_supervised_taped), ("torch", forward_supervised)):
        net, data, k, sim, fk = _device_setup(kp, g, case)
        pred = fwd(net, fk, data)
        loss, _ = compute_loss(pred, data)
        loss.backward()
        out[name] = (pred, loss.detach(), {n_: p_.grad for n_, p_ in net.named_parameters()})
    for key in ("qpos", "qvel"):
        _rule(f"{k} {key}", out["taped"][0][key].detach(), out["torch"][0][key].detach(), g[f"{key}_{k}"])
    _rule(f"{k} loss", out["taped"][1].reshape(1), out["torch"][1].reshape(1), np.asarray([float(g["loss_" + k])]))
    for w in CC.WATCH:
        _rule(f"{k} grad {w}", out["taped"][2][w], out["torch"][2][w], g[f"grad_{k}:{w}"])
    net, data, k, sim, fk = _device_setup(kp, g, case)
    with torch.no_grad():
        pred = kin_tape.forward_supervised_taped(net, fk, data)
        q0, v0, cf = net.init_states(data, keep_feat=True)
        Q, V, A = net.rollout(data, sim, q0.contiguous(), v0.contiguous(), ctx_feat=cf)
    for key, want in (("qpos", Q), ("qvel", V), ("action", A)):
        assert torch.equal(pred[key], want), key


def test_scheduled_sampling_keeps_the_context_cotangent(kp, golden):
    """every frame put on the ground-truth pose (all coins 1): the pose tape is cut everywhere, and context_rnn's input weights still receive the
    gradient that reaches them through the frames' context blocks alone -- the two paths agree by the rule, reference the fp64 torch path"""
    from kinpoly_amd import kin_tape
    from kinpoly_amd.pretrain import compute_loss, forward_supervised
    g = golden("ar_obs_context")

    class Ones:
        def binomial(self, n, p):
            return 1
    grads = {}
    for name, fwd, dtype in (("taped", kin_tape.forward_supervised_taped, torch.float32), ("torch", forward_supervised, torch.float32), ("ref", forward_supervised, torch.float64)):
        if dtype == torch.float32:
            net, data, k, sim, fk = _device_setup(kp, g, (1, 1, 1))
        else:
            net, data, k = CC.build(g, (1, 1, 1))
            fk = CC.torch_fk()
        pred = fwd(net, fk, data, gt_rate=0.5, rng=Ones())
        assert torch.equal(pred["qpos"], data["qpos"])
        # the action alone carries the loss: qpos / qvel are the clip's
        (pred["action"] ** 2).sum().backward()
        grads[name] = net.context_rnn.rnn_f.weight_ih.grad
    assert float(grads["ref"].abs().max()) > 0
    _rule("all-GT frames grad context_rnn.rnn_f.weight_ih", grads["taped"], grads["torch"], grads["ref"].numpy())


def test_exp_arnet_with_context_and_of_on_both_paths(kp, tmp_path):
    """kinpoly_amd.exp_arnet on 8 synthetic clips x 12 frames with a context block and an `of` block (rnn_hdim 32 < state): one train_epoch on each path,
    the first batch's loss of the two paths by the rule (reference: the fp64 torch path), the checkpoint round trip, test_takes' shapes"""
    from kinpoly_amd import dataset as D
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import kin_tape
    from kinpoly_amd import pretrain as P
    from kinpoly_amd.model_compiler import read_kpm
    std = np.load(os.path.join(CC.GOLDEN, "standing_neutral.npz"))
    torch.manual_seed(0)
    F = 20
    net = E.build_net(use_context=True, of_dim=F, rnn_hdim=32, mlp_hsize=(64, 32, 32)).cuda()
    assert (net.state_dim, net.context_dim, net.base_dim) == (32 + 101, F + 17, 101)
    model = kp.KpModel(kp.STEP_KPM, **E.model_options(net))
    sim = kp.KpSim(model, 8)
    takes = D.synthetic_takes(sim, std["qpos"], n_per_action=2, T_range=(12, 13), body_mass=read_kpm(kp.STEP_KPM)["body_mass"], seed=2)
    of = D.synthetic_of_features(takes, F, seed=1)
    ds = D.StateARDataset(takes, fr_num=12, seed=3, device="cuda", of_features=of)
    assert ds.get_len() == 8 and ds.of_dim == F
    fk = CC.torch_fk(torch.float32, "cuda", sim)
    data = next(P.sampling_batches(ds, 8, 8, "cuda"))
    assert tuple(data["of"].shape) == (8, 12, F)
    loss = {}
    for name, fwd in (("taped", kin_tape.forward_supervised_taped), ("torch", P.forward_supervised)):
        loss[name] = P.compute_loss(fwd(net, fk, data), data)[0].detach().reshape(1)
    net64 = E.build_net(use_context=True, of_dim=F, rnn_hdim=32, mlp_hsize=(64, 32, 32)).cuda().double()
    net64.load_state_dict({k_: v.double() for k_, v in net.state_dict().items()})
    d64 = {k_: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k_, v in data.items()}
    ref = P.compute_loss(P.forward_supervised(net64, CC.torch_fk(torch.float64, "cuda"), d64), d64)[0].detach()
    _rule("first batch loss", loss["taped"], loss["torch"], np.asarray([float(ref)]))
    for fused in (False, True):
        l, comp, rate, fr_num = E.train_epoch(net, fk, ds, 0, 2000, 1e-4, 0.0, 8, 8, fused=fused, rng=np.random.RandomState(0))
        print(f"train_epoch context + of, fused={fused}: loss {l:.4f}")
        assert np.isfinite(l) and len(comp) == 8 and np.isfinite(comp).all() and (rate, fr_num) == (0.3, 80)
    for n_, p_ in net.named_parameters():
        if n_ != "action_log_std":
            assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), n_
    path = str(tmp_path / "iter_0001.p")
    E.save_arnet(path, net)
    other = E.build_net(use_context=True, of_dim=F, rnn_hdim=32, mlp_hsize=(64, 32, 32)).cuda()
    E.load_arnet(path, other)
    assert all(torch.equal(a, b) for (ka, a), (kb, b) in zip(net.state_dict().items(), other.state_dict().items()) if ka != "action_log_std")
    tds = D.StateARDataset(takes, data_mode="test", fr_num=12, seed=3, device="cuda", of_features=of)
    res = E.test_takes(net, model, tds, torch.device("cuda", 0))
    assert set(res) == set(takes)
    for k_, r in res.items():
        assert r["qpos"].shape == (12, 76) and r["qpos_gt"].shape == (12, 76) and r["obj_pose"].shape[0] == 12 and np.isfinite(r["qpos"]).all()
    # a chunked roll-out (more clips than the twin's rows) hands `of` and the sequence along
    from kinpoly_amd.context import PolicyARContext
    pol = E.build_net(use_context=True, of_dim=F, as_policy=True, rnn_hdim=32, mlp_hsize=(64, 32, 32)).cuda()
    sim3 = kp.KpSim(kp.KpModel(kp.STEP_KPM), 3)
    full = PolicyARContext(pol, kp.KpSim(kp.KpModel(kp.STEP_KPM), 8), smooth=False).init_context(data)
    part = PolicyARContext(pol, sim3, smooth=False).init_context(data)
    eq, ev = float((full["ar_qpos"] - part["ar_qpos"]).abs().max()), float((full["ar_qvel"] - part["ar_qvel"]).abs().max())
    print(f"MEASURED roll-out in chunks of 3 against all 8 clips at once: qpos {eq:.3e}  qvel {ev:.3e}")
    # the same clips through GEMMs of 3 rows and of 8: tests/test_gpu_driver.py's bounds on a pair of fp32 roll-outs of one network (2e-4 pose, 2e-2 velocity)
    assert tuple(full["ar_qpos"].shape) == (8, 12, 76) and eq < 2e-4 and ev < 2e-2


def test_refusals_come_before_any_launch(kp):
    L = kp.load_library()
    err = lambda: L.kp_last_error().decode()      # noqa: E731
    n, H, F = 4, 8, 3
    sim, c = _case(kp, 105, n, 6000)
    ctx = K._make_ctx(sim, c)
    cf, of = _tables(n + 5, H, F, 1)
    W = H + 105 + F
    buf, out = _guarded(n, W)
    P_ = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def ext(**kw):
        x = sim.make_obs_ext(T, n + 5, H, cf, of, ctx_time_major=False)
        for k_, v in kw.items():
            setattr(x, k_, v)
        return x
    fwd = lambda x, ctx_=ctx, o=out: L.kp_sim_obs_ar_ex(sim.h, None if ctx_ is None else C.byref(ctx_), None if x is None else C.byref(x), None if o is None else P_(o))      # noqa: E731
    assert fwd(ext(ctx_dim=-1)) == -1 and "negative" in err()
    assert fwd(ext(of_dim=-2)) == -1 and "negative" in err()
    assert fwd(ext(of=None)) == -1 and "null `of`" in err()
    assert fwd(ext(ctx_stride_row=0)) == -1 and "ctx_feat needs strides" in err()
    assert fwd(ext(ctx_stride_t=0)) == -1 and "ctx_feat needs strides" in err()
    assert fwd(ext(of_stride_row=0)) == -1 and "`of` needs strides" in err()
    assert fwd(ext(of_stride_t=0)) == -1 and "`of` needs strides" in err()
    assert fwd(None) == -1 and "null kp_obs_ext" in err()
    assert fwd(ext(), ctx_=None) == -1 and fwd(ext(), o=None) == -1
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())                                            # nothing was launched
    q = sim.view("qpos").clone()
    f = sim.fk(q)
    go = torch.zeros((n, W), device="cuda")
    outs = [torch.full((n, d), -7.0, device="cuda") for d in (76, 3, 4, H)]

    def bwd(x, sim_=sim, w=W, rows=n, gc=True):
        return L.kp_sim_obs_ar_ex_backward(sim_.h, C.byref(ctx), None if x is None else C.byref(x), rows, w, P_(q), P_(f["wbpos"]), P_(f["wbquat"]), P_(go), None,
                                           P_(outs[0]), None, P_(outs[1]), P_(outs[2]), P_(outs[3]) if gc else None)
    assert bwd(ext(ctx_dim=-1)) == -1 and "negative" in err()
    assert bwd(ext(of=None)) == -1 and "null `of`" in err()
    assert bwd(ext(ctx_stride_t=0)) == -1 and "strides" in err()
    assert bwd(ext(of_stride_row=0)) == -1 and "strides" in err()
    assert bwd(None) == -1 and "null kp_obs_ext" in err()
    assert bwd(ext(), w=105) == -1 and "105 wide" in err()
    assert bwd(ext(), rows=n + 1) == -1 and "n_rows" in err()
    assert bwd(ext(), gc=False) == -1 and "null output" in err()
    for opts, wd in ((dict(ar_obs_head=0, ar_obs_action=0), 81), (dict(ar_obs_vel=1, ar_obs_head=0, ar_obs_action=0), 156)):
        s = kp.KpSim(kp.KpModel(**opts), n)
        assert s.obs_ar_dim == wd and bwd(ext(), sim_=s, w=H + wd + F) == -1 and f"{wd}-d layout" in err()
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)
    assert bwd(ext(), rows=0) == 0
    with pytest.raises(ValueError, match="ctx_feat"):                            # the binding's own checks: a table of another shape, a strided one
        sim.make_obs_ext(T, n + 5, H, cf[:, :, :H - 1].contiguous(), None, ctx_time_major=False)
    with pytest.raises(ValueError, match="of"):
        sim.make_obs_ext(T, n + 5, H, None, of.transpose(0, 1))
    with pytest.raises(ValueError):
        sim.obs_ar_ex(ctx, ext(), out=torch.empty((n, W - 1), device="cuda"))
    from kinpoly_amd import exp_arnet as E
    from kinpoly_amd import kin_tape
    net = E.build_net(use_context=True, rnn_hdim=16, mlp_hsize=(16, 8, 8)).cuda()
    with pytest.raises(ValueError, match="105-d observations, the policy takes 101-d"):
        kin_tape.check_fused(net, CC.torch_fk(torch.float32, "cuda", sim))
    for key in [k for k in K._SIMS if k[1]]:
        del K._SIMS[key]
