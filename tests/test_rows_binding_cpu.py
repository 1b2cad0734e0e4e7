"""The shape handling the rows tools' bindings share (kinpoly_amd/sim.py: _rows_want, _rows_inputs, _rows_outputs, _rows_view) on CPU tensors: no
library, no GPU.  The device pointers (_rows_ptrs -> _dev) need a GPU and are covered by the tools' own GPU tests."""
import pytest

torch = pytest.importorskip("torch")

from kinpoly_amd import sim as S  # noqa: E402

LEADS = [(), (5,), (2, 3), (0,)]
F32 = torch.float32


def spec(lead, qvel=True, body=True):
    """a spec as point_jacobian and the motion tools build them: qpos, an optional float input, a required int input without a tail"""
    return [("qpos", torch.zeros(lead + (76,)), (76,), F32, True), ("qvel", torch.ones(lead + (75,)) if qvel else None, (75,), F32, False),
            ("body", torch.zeros(lead, dtype=torch.int32) if body else None, (), torch.int32, True)]


@pytest.mark.parametrize("lead", LEADS)
def test_inputs_are_flattened_to_rows(lead):
    R = 1
    for n in lead:
        R *= n
    got_lead, got_R, flat = S._rows_inputs("tool", spec(lead))
    assert got_lead == lead and got_R == R and isinstance(got_R, int)
    assert [tuple(t.shape) for t in flat] == [(R, 76), (R, 75), (R,)] and flat[2].dtype == torch.int32
    assert bool((flat[1] == 1).all())
    # an optional input given as None stays None, in its place
    _, _, flat = S._rows_inputs("tool", spec(lead, qvel=False))
    assert flat[1] is None and tuple(flat[0].shape) == (R, 76) and tuple(flat[2].shape) == (R,)


def test_inputs_that_do_not_fit_are_refused_by_name():
    with pytest.raises(ValueError, match=r"tool: qpos must be \[\.\.\., 76\], got \(5, 75\)"):
        S._rows_inputs("tool", [("qpos", torch.zeros(5, 75), (76,), F32, True)])
    with pytest.raises(ValueError, match=r"tool: qpos must be \[\.\.\., 76\], got \(\)"):
        S._rows_inputs("tool", [("qpos", torch.zeros(()), (76,), F32, True)])
    bad = spec((5,))
    bad[1] = ("qvel", torch.zeros(5, 76), (75,), F32, False)                    # a wrong trailing dimension
    with pytest.raises(ValueError, match=r"tool: qvel must be \(5, 75\), got \(5, 76\)"):
        S._rows_inputs("tool", bad)
    bad = spec((2, 3))
    bad[1] = ("qvel", torch.zeros(6, 75), (75,), F32, False)                    # a leading shape that disagrees with qpos
    with pytest.raises(ValueError, match=r"tool: qvel must be \(2, 3, 75\), got \(6, 75\)"):
        S._rows_inputs("tool", bad)
    bad = spec((2, 3))
    bad[2] = ("body", torch.zeros(6, dtype=torch.int32), (), torch.int32, True)
    with pytest.raises(ValueError, match=r"tool: body must be \(2, 3\), got \(6,\)"):
        S._rows_inputs("tool", bad)
    with pytest.raises(ValueError, match="tool: body is required"):
        S._rows_inputs("tool", spec((5,), body=False))


def test_want_names_some_of_the_table():
    T = S.INVDYN_OUTPUTS
    assert S._rows_want("tool", ["ncon", "contact"], T) == ("ncon", "contact")
    assert S._rows_want("tool", iter(T), T) == tuple(T)
    with pytest.raises(ValueError, match=r"tool: want must name some of \('qfrc_inverse', .*\), got \('qacc',\)"):
        S._rows_want("tool", ("qacc",), T)
    with pytest.raises(ValueError, match=r"tool: want must name some of .*, got \(\)"):
        S._rows_want("tool", (), T)
    with pytest.raises(ValueError, match=r"tool: outputs must name some of .*, got \('ncon', 'nope'\)"):
        S._rows_want("tool", ("ncon", "nope"), T, "outputs")


@pytest.mark.parametrize("table", ["CONTACT_OUTPUTS", "INVDYN_OUTPUTS", "MOTION_OUTPUTS", "ESTIMATE_OUTPUTS", "_JAC_OUTPUTS", "_FIT_OUTPUTS"])
@pytest.mark.parametrize("lead", LEADS)
def test_outputs_have_the_leading_shape_and_the_table_dtype(table, lead):
    T = getattr(S, table)
    _, R, _ = S._rows_inputs("tool", spec(lead))
    want = tuple(T)[::2]
    flat = S._rows_outputs(R, T, want, "cpu")
    assert tuple(flat) == want
    out = S._rows_view(flat, lead)
    for k in want:
        shape, dtype = T[k]
        assert tuple(flat[k].shape) == (R,) + shape and flat[k].is_contiguous()
        assert tuple(out[k].shape) == lead + shape and out[k].dtype == dtype
        assert out[k].data_ptr() == flat[k].data_ptr(), "a view, not a copy"
        assert out[k].numel() == 0 if R == 0 else out[k].numel() > 0


class _Recorder:
    """stands in for the loaded library and for a handle: records the entry points a method calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


def test_no_rows_no_native_call(monkeypatch):
    """R == 0: every rows method returns empty tensors of the right shape without calling the library (the device check is stubbed out: CPU tensors)"""
    monkeypatch.setattr(S, "_dev", lambda name, t, shape, dtype=F32: None)
    sim = object.__new__(S.KpSim)
    sim.L, sim.h, sim.device, sim.model = _Recorder(), None, "cpu", None
    q = torch.zeros(2, 0, 76)
    assert tuple(sim.inverse_dynamics(q, want=("qfrc_inverse", "ncon"))["ncon"].shape) == (2, 0)
    assert tuple(sim.estimate_contacts(q, cfg=S.KpEstimateCfg(), want=("lambda",))["lambda"].shape) == (2, 0, 64, 4)
    assert tuple(sim.body_motion(q, torch.zeros(2, 0, 75))["centroid"].shape) == (2, 0, 18)
    assert tuple(sim.point_jacobian(q, torch.zeros(2, 0, dtype=torch.int32)).shape) == (2, 0, 6, 75)
    out = sim.fit_pose(q, torch.zeros(2, 0, 24, 3), cfg=S.KpFitCfg(), want_dq=True)
    assert {k: tuple(v.shape) for k, v in out.items()} == {"qpos": (2, 0, 76), "info": (2, 0, 8), "dq": (2, 0, 75)}
    assert sim.L.calls == []
    # and with rows the same path does call, once
    sim.body_motion(torch.zeros(3, 76), outputs=("centroid",))
    assert sim.L.calls == ["kp_sim_body_motion"]
