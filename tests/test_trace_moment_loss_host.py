"""
`track_along_vjp(..., moment_targets=)` without a GPU: the numpy restatement of the values (tests/moment_loss_reference.py)
against the traces' own properties, `MomentTargets` by value -- term order, shared and per-sample rows, every refusal with
its text --, and with the fake runtime of tests/reverse_host_fakes.py what the constructor and a reverse call make in each
of the five modes: the uploads, the buffers zero-filled on the device and the arguments of the two new entry points.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import moment_loss_reference as ml
from .reverse_host_fakes import fabricated_energy, fabricated_moments, fabricated_records, fake_gpu, no_gpu  # noqa: F401 (fixture)

ROOT = Path(__file__).resolve().parent.parent
FORWARD, BACKWARD, MEMSET = "lynx_moments_along_loss", "lynx_moments_along_loss_backward", "lynx_buf_memset"

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731


# ---------------------------------------------------------------------------------------------
# 1. the restated values are the traces' properties
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("form", ["records", "moments"])
def test_the_restated_values_are_the_traces_properties_to_four_units_in_the_last_place(form, dtype, ddof, monkeypatch):
    from lynx_amd import config
    from lynx_amd.trace import BeamTrace

    monkeypatch.setattr(config, "std_ddof", ddof)
    batch, P = (3,), 5
    energy = fabricated_energy((*batch, P), 4).astype(dtype)
    lengths, names = [1.0] * (P - 1), [f"E{k}" for k in range(P - 1)]
    if form == "records":
        records = fabricated_records(batch, P, 5)
        trace = BeamTrace.from_records(records, energy, lengths, names, dtype)
        values, kappa = ml.values_of(dtype, energy, records=records, ddof=ddof)
    else:
        mu, cov = fabricated_moments(batch, (P,), dtype, 6)
        trace = BeamTrace.from_moments(mu, cov, energy, lengths, names, dtype)
        values, kappa = ml.values_of(dtype, energy, mu=mu, cov=cov)
    assert set(values) == set(ml.PROPERTIES) and len(ml.PROPERTIES) == 23
    worst = 0.0
    for name in ml.PROPERTIES:
        have = np.asarray(getattr(trace, name))
        assert have.dtype == np.dtype(dtype) and have.shape == (*batch, P), name
        units = np.abs(values[name] - have.astype(np.float64)) / np.spacing(np.abs(have)).astype(np.float64)
        worst = max(worst, float(units.max()))
        assert units.max() <= 4, (name, float(units.max()))
        assert np.all(kappa[name] >= 1.0)
    print(f"{form} {np.dtype(dtype).name} ddof={ddof}: worst distance {worst:.2f} units in the last place")


def test_the_reference_and_the_library_name_the_same_properties_in_the_same_order():
    from lynx_amd import grad

    assert grad.MOMENT_PROPERTIES == ml.PROPERTIES
    # every name has a host rule, and no other name has one
    shape = (1, 2)
    assert len(list(grad._walk_properties({name: 0.0 for name in ml.PROPERTIES}, shape, "trace",
                                          ("emittance", "normalized_emittance", "beta", "alpha"), ("energy",)))) == 23


# ---------------------------------------------------------------------------------------------
# 2. MomentTargets by value
# ---------------------------------------------------------------------------------------------

NAMES = ["Q1", "D1", "M1", "Q2", "D2", "M2"]  # 7 points


def test_the_terms_are_ordered_by_point_and_property_code_and_scalar_rows_are_shared(no_gpu):
    from lynx_amd import grad

    targets = grad.MomentTargets({"M2": {"beta_y": 2.0, "mu_x": 0.0}, -4: {"energy": 1e8, "alpha_x": 0.5, "sigma_xxp": 1e-9}, 0: {"sigma_p": 1e-3}},
                                 weights={"M2": {"beta_y": 0.25}, 3: {"energy": 1e-16}})
    with pytest.raises(ValueError, match="once the targets have met a trace"):
        targets.terms
    layout = targets._layout(NAMES, (2, 3))
    assert targets.terms == [(0, "sigma_p"), (3, "sigma_xxp"), (3, "alpha_x"), (3, "energy"), (6, "mu_x"), (6, "beta_y")]
    assert layout.points == [[0, 1 << 11], [3, (1 << 12) | (1 << 20) | (1 << 22)], [6, (1 << 0) | (1 << 19)]] and layout.first == [0, 1, 4]
    assert layout.arguments[0] == 3 and list(layout.arguments[1]) == [0, 1 << 11, 3, (1 << 12) | (1 << 20) | (1 << 22), 6, (1 << 0) | (1 << 19)]
    assert layout.stride == 0 and layout.host.shape == (1, 6, 2) and layout.host.dtype == np.float64
    assert np.array_equal(layout.host[0], [[1e-3, 1], [1e-9, 1], [0.5, 1], [1e8, 1e-16], [0.0, 1], [2.0, 0.25]])
    assert layout.energy and layout.moments
    assert ml.terms_of([tuple(pair) for pair in layout.points]) == targets.terms
    # the layout is reused for the same trace shape and remade for another batch
    assert targets._layout(NAMES, (2, 3)) is layout
    other = targets._layout(NAMES, (4,))
    assert other is not layout and other.host.shape == (1, 6, 2)
    only_energy = grad.MomentTargets({1: {"energy": 1.0}})._layout(NAMES, (1,))
    assert only_energy.energy and not only_energy.moments
    assert not grad.MomentTargets({1: {"beta_x": 1.0}})._layout(NAMES, (1,)).energy
    assert grad.MomentTargets({1: {"normalized_emittance_y": 1.0}})._layout(NAMES, (1,)).energy


def test_an_array_target_or_weight_makes_rows_per_sample(no_gpu):
    from lynx_amd import grad

    per_sample = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    targets = grad.MomentTargets({"M1": {"beta_x": per_sample, "beta_y": 7.0}}, weights={"M1": {"beta_y": np.array([0.5, 0.25, 0.125])}})
    layout = targets._layout(NAMES, (2, 3))
    assert layout.stride == 4 and layout.host.shape == (6, 2, 2)
    assert np.array_equal(layout.host[:, 0, 0], per_sample.reshape(-1)) and np.all(layout.host[:, 0, 1] == 1.0)  # a scalar weight next to an array target
    assert np.all(layout.host[:, 1, 0] == 7.0) and np.array_equal(layout.host[:, 1, 1], [0.5, 0.25, 0.125] * 2)
    per_sample[0, 0] = 99.0  # (the object holds copies: the upload is made once)
    assert targets._layout(NAMES, (2, 3)).host[0, 0, 0] == 1.0


def test_every_refusal_by_value_carries_its_text(no_gpu):
    from lynx_amd import grad

    with pytest.raises(KeyError) as info:
        grad.MomentTargets({"M1": {"beta_z": 1.0}})
    assert info.value.args[0] == "no cotangent rule for trace property 'beta_z'"
    with pytest.raises(KeyError) as info:
        grad.trace_property_cotangents(_host_trace(), {"beta_z": 1.0})
    assert info.value.args[0] == "no cotangent rule for trace property 'beta_z'"  # (the text of `_walk_properties`)
    with pytest.raises(KeyError, match="no cotangent rule for trace property 'gamma'"):
        grad.MomentTargets({"M1": {"beta_x": 1.0}}, weights={"M1": {"gamma": 1.0}})
    with pytest.raises(TypeError, match="targets is a dict"):
        grad.MomentTargets([("M1", "beta_x", 1.0)])
    with pytest.raises(TypeError, match="targets is a dict"):
        grad.MomentTargets({"M1": 1.0})
    with pytest.raises(ValueError, match="no target is given"):
        grad.MomentTargets({"M1": {}})
    with pytest.raises(ValueError) as info:  # two keys that mean the same (point, property)
        grad.MomentTargets({"M1": {"beta_x": 1.0}, 3: {"beta_x": 2.0}})._layout(NAMES, (2,))
    assert str(info.value) == "track_along_vjp: 'beta_x' at point 3 is given two targets"
    with pytest.raises(ValueError) as info:
        grad.MomentTargets({"M1": {"beta_x": 1.0}}, weights={"M1": {"beta_x": 1.0}, -4: {"beta_x": 2.0}})._layout(NAMES, (2,))
    assert str(info.value) == "track_along_vjp: 'beta_x' at point 3 is given two weights"
    with pytest.raises(ValueError) as info:
        grad.MomentTargets({"M1": {"beta_x": 1.0}}, weights={"M2": {"beta_x": 1.0}})._layout(NAMES, (2,))
    assert str(info.value) == "track_along_vjp: a weight of 'beta_x' at point 6, which has no target"
    with pytest.raises(KeyError) as info:  # a point outside the trace: the errors of `trace.index_of`
        grad.MomentTargets({"M9": {"beta_x": 1.0}})._layout(NAMES, (2,))
    assert info.value.args[0] == "no element named 'M9' in this trace"
    with pytest.raises(IndexError) as info:
        grad.MomentTargets({7: {"beta_x": 1.0}})._layout(NAMES, (2,))
    assert str(info.value) == "point 7 of a trace of 7"
    with pytest.raises(IndexError, match="point -8 of a trace of 7"):
        grad.MomentTargets({-8: {"beta_x": 1.0}})._layout(NAMES, (2,))
    with pytest.raises(ValueError) as info:  # a target that does not broadcast
        grad.MomentTargets({"M1": {"beta_x": np.ones(3)}})._layout(NAMES, (2,))
    assert str(info.value) == "track_along_vjp: the target of 'beta_x' at point 3 has shape (3,), which does not broadcast to the batch (2,)"
    with pytest.raises(ValueError, match=r"the weight of 'beta_x' at point 3 has shape \(2, 2\)"):
        grad.MomentTargets({"M1": {"beta_x": 1.0}}, weights={"M1": {"beta_x": np.ones((2, 2))}})._layout(NAMES, (2,))


def test_index_of_is_the_function_the_targets_use():
    from lynx_amd.trace import point_index

    trace = _host_trace()
    for key in ("E0", "E2", 0, 3, -1, -4):
        assert trace.index_of(key) == point_index(trace.names, key)
    for key, error in (("nobody", KeyError), (4, IndexError), (-5, IndexError)):
        with pytest.raises(error) as of_trace:
            trace.index_of(key)
        with pytest.raises(error) as of_function:
            point_index(trace.names, key)
        assert of_trace.value.args == of_function.value.args


def _host_trace():
    from lynx_amd.trace import BeamTrace

    mu, cov = fabricated_moments((2,), (4,), np.float64, 1)
    return BeamTrace.from_moments(mu, cov, fabricated_energy((2, 4), 1), [1.0] * 3, ["E0", "E1", "E2"], np.float64)


def test_the_constructor_refuses_by_value_before_anything_touches_the_gpu(no_gpu):
    import lynx_amd as lx

    segment, beam = _plain(lx), _parameters(lx)
    with pytest.raises(TypeError, match="moment_targets is a dict"):
        lx.grad.track_along_vjp(segment, beam, moment_targets=[1.0])
    with pytest.raises(KeyError, match="beta_z"):
        lx.grad.track_along_vjp(segment, beam, moment_targets={"M1": {"beta_z": 1.0}})
    with pytest.raises(KeyError, match="no element named 'M7' in this trace"):
        lx.grad.track_along_vjp(segment, beam, moment_targets={"M7": {"beta_x": 1.0}})
    with pytest.raises(ValueError, match="does not broadcast to the batch"):
        lx.grad.track_along_vjp(segment, beam, moment_targets={"M1": {"beta_x": np.ones(5)}})


# ---------------------------------------------------------------------------------------------
# 3. the calls, mode by mode
# ---------------------------------------------------------------------------------------------

B = 2


def _plain(lx):
    return lx.Segment([lx.Quadrupole(f(0.2), k1=f(1.5), name="Q1"), lx.Drift(f(0.5), name="D1"), lx.Marker(name="M1"),
                       lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q2"), lx.Drift(f(0.5), name="D2"), lx.Marker(name="M2")])


def _parameters(lx):
    full = lambda v: np.full((B,), v, dtype=np.float32)  # noqa: E731
    return lx.ParameterBeam.from_parameters(sigma_x=full(1e-4), sigma_y=full(1e-4), energy=full(1e8))


def _particles(lx):
    return lx.ParticleBeam(o.gaussian_particles((B,), 16, seed=1), np.full((B,), 1e8, dtype=np.float32))


def _case(lx, mode):
    """(segment, beam, keywords of track_along_vjp, the sweep's entry point, where it takes its cotangent buffers)."""
    if mode == "moments":
        return _plain(lx), _parameters(lx), {}, "lynx_track_moments_along_backward", {"mb": 5, "cb": 6, "eb": 7}
    if mode == "particles":
        return _plain(lx), _particles(lx), {}, "lynx_track_particles_along_backward", {"rec": 5, "eb": 6}
    if mode == "trajectories":
        return (_plain(lx), _particles(lx), {"trajectories": 2}, "lynx_track_particles_along_backward_trajectories",
                {"rec": 5, "eb": 6, "wb": 13})
    if mode == "survivors":
        segment = _plain(lx)
        segment = lx.Segment([*segment.elements[:3], lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=True, name="COL"), *segment.elements[3:]])
        return segment, _particles(lx), {"losses": True}, "lynx_track_particles_along_backward_losses", {"rec": 5, "eb": 6}
    assert mode == "kicks"
    segment = lx.Segment([lx.Drift(f(0.5), name="D1"), lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="CAV"),
                          lx.Quadrupole(f(0.2), k1=f(1.5), name="Q1"), lx.Marker(name="M1"), lx.Marker(name="M2")])
    return segment, _particles(lx), {"cavities": True}, "lynx_track_particles_along_backward_cavities", {"rec": 7, "eb": 8}


MODES = ("moments", "particles", "trajectories", "survivors", "kicks")


@pytest.fixture
def recorded_with_energy(monkeypatch):
    """
    The fake runtime with the fabricated forward pass (asked to keep the energies it also leaves them on the device, as the
    real `engine.track_along` does); the incoming energy over the batch is a forward array (the real one is uploaded once
    and remembered on the beam): (lynx_amd, the runtime, the keyword arguments of every forward pass).
    """
    import lynx_amd as lx
    from lynx_amd.device import Dual

    rt, forward = fake_gpu(monkeypatch)
    monkeypatch.setattr(Dual, "broadcast_device", lambda self, runtime, shape: rt.forward("e_in", tuple(shape), self.host().dtype))
    return lx, rt, forward


def uploads(rt, since=0):
    return [a for a in rt.allocations[since:] if a.how in ("to_device", "to_device_result")]


def calls_of(rt, entry):
    return [args for name, args in rt.lib.records if name == entry]


TARGETS = {"M1": {"beta_x": 4.0, "beta_y": 2.0}, -1: {"sigma_x": 1e-4, "energy": 1e8}}


@pytest.mark.parametrize("mode", MODES)
def test_the_forward_call_goes_right_behind_the_trace(recorded_with_energy, mode):
    lx, rt, forward = recorded_with_energy
    segment, beam, keywords, _, _ = _case(lx, mode)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets=TARGETS, **keywords)
    assert forward[-1]["keep_energy"] is True and forward[-1]["keep_device"] is True
    assert [name for name in rt.lib.calls if name not in ("lynx_moments_by_loss",)] == [FORWARD]
    (args,) = calls_of(rt, FORWARD)
    P = vjp.trace.num_points
    m1 = vjp.trace.index_of("M1")
    # ctx, dtype, batch, n_points, records, mu, cov, energy, ddof, n_target_points, target_points, rows, row_stride, values, point_loss, loss
    assert len(args) == 16 and args[1:4] == [0, B, P] and args[8] == 1 and args[9] == 2
    if mode == "moments":
        assert args[4] is None and args[5]["how"] == "forward:mu" and args[6]["how"] == "forward:cov"
    else:
        assert args[4]["how"] == "forward:records" and args[5] is None and args[6] is None
    assert args[7]["how"] == "forward:energy" and args[7]["shape"] == [B, P] and args[7]["dtype"] == "<f4"
    assert args[10] == {"ctypes": [m1, (1 << 18) | (1 << 19), P - 1, (1 << 6) | (1 << 22)]}
    assert args[11]["how"] == "to_device" and args[11]["shape"] == [1, 4, 2] and args[11]["dtype"] == "<f8" and args[12] == 0
    assert np.array_equal(args[11]["host"][0], [[4.0, 1], [2.0, 1], [1e-4, 1], [1e8, 1]])
    assert [(a["how"], a["shape"], a["dtype"]) for a in args[13:]] == [("empty", [B, 4], "<f8"), ("empty", [B, 2], "<f8"), ("empty", [B], "<f8")]
    assert vjp.moment_values.shape == (B, 4) and vjp.moment_loss.shape == (B,) and vjp.moment_loss.dtype == np.float64
    assert vjp.moment_loss_of("M1").shape == (B,) and np.array_equal(vjp.moment_loss_of(-1), vjp.moment_loss_of(P - 1))
    with pytest.raises(KeyError, match="point 0 has no target"):
        vjp.moment_loss_of(0)


@pytest.mark.parametrize("mode", MODES)
def test_moment_loss_bar_alone_uploads_eight_bytes_per_sample_and_the_buffers_are_zero_filled_on_the_device(recorded_with_energy, mode):
    lx, rt, forward = recorded_with_energy
    segment, beam, keywords, sweep, where = _case(lx, mode)
    targets = lx.grad.MomentTargets(TARGETS)
    rows = []
    for _ in range(3):  # three passes of a loop with the same object: the rows are uploaded once
        vjp = lx.grad.track_along_vjp(segment, beam, moment_targets=targets, **keywords)
        if mode != "moments":  # (the fabricated forward pass has not read the particles; the real one has, and they are on the device)
            beam._particles.device(rt)
        since = len(rt.allocations)
        del rt.lib.calls[:], rt.lib.records[:]
        g = vjp(moment_loss_bar=np.array([1.0, -0.5]))
        sent = uploads(rt, since)
        assert [(a.shape, a.dtype.str) for a in sent] == [((B,), "<f8")] and sum(a.host.nbytes for a in sent) == B * 8
        assert np.array_equal(sent[0].host, [1.0, -0.5])
        rows.append(calls_of(rt, BACKWARD)[0][11])
    assert len([a for a in rt.allocations if a.how == "to_device" and a.shape == (1, 4, 2)]) == 1 and rows[0] == rows[1] == rows[2]
    P, K = vjp.trace.num_points, 2
    shapes = {"mb": ([B, P, 7], "<f4"), "cb": ([B, P, 7, 7], "<f4"), "rec": ([B, P, 36], "<f8"), "eb": ([B, P], "<f4"), "wb": ([B, P, K, 7], "<f8")}
    filled = calls_of(rt, MEMSET)
    assert [name for name in rt.lib.calls if name != MEMSET] == [BACKWARD, sweep]
    assert len(filled) == len(where) and all(args[2] == 0 for args in filled)
    (loss,), (swept,) = calls_of(rt, BACKWARD), calls_of(rt, sweep)
    for name, at in where.items():
        shape, dtype = shapes[name]
        buffer = swept[at]
        assert (buffer["how"], buffer["shape"], buffer["dtype"]) == ("empty", shape, dtype), (name, buffer)
        assert sum(args[1] == buffer and args[3] == int(np.prod(shape)) * np.dtype(dtype).itemsize for args in filled) >= 1, name
    # ... and the loss's reverse half adds into the buffers the sweep is handed:
    # ..., row_stride, loss_bar, grad_trace, mu_bar, cov_bar, energy_bar
    assert len(loss) == 18 and loss[13]["host"].dtype == np.float64
    if mode == "moments":
        assert loss[14] is None and loss[15] == swept[where["mb"]] and loss[16] == swept[where["cb"]]
        assert g.mu.shape == (B, 7)
    else:
        assert loss[14] == swept[where["rec"]] and loss[15] is None and loss[16] is None
    assert loss[17] == swept[where["eb"]]


@pytest.mark.parametrize("mode", MODES)
def test_beside_another_cotangent_the_uploads_are_those_of_the_call_without_the_loss(recorded_with_energy, mode):
    lx, rt, forward = recorded_with_energy
    segment, beam, keywords, sweep, where = _case(lx, mode)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets={"M1": {"beta_x": 4.0}}, **keywords)
    P = vjp.trace.num_points
    w = np.zeros((B, P))
    w[:, 2] = [0.5, -1.0]
    if mode != "moments":  # (as above: the real forward pass has left the particles on the device)
        beam._particles.device(rt)
    since = len(rt.allocations)
    del rt.lib.calls[:], rt.lib.records[:]
    vjp(beta_x=w)
    without, calls_without = uploads(rt, since), list(rt.lib.calls)
    assert calls_without == [sweep]
    since = len(rt.allocations)
    del rt.lib.calls[:], rt.lib.records[:]
    vjp(beta_x=w, moment_loss_bar=2.0)
    beside = uploads(rt, since)
    assert rt.lib.calls == [BACKWARD, sweep]  # no energy term, and every buffer came from the host: nothing is zero-filled
    bars = [a for a in beside if a.shape == (B,) and a.dtype == np.float64]
    assert len(bars) == 1 and np.array_equal(bars[0].host, [2.0, 2.0])
    rest = [a for a in beside if a is not bars[0]]
    assert len(rest) == len(without) and len(without) >= 1
    for a, b in zip(rest, without):
        assert (a.how, a.shape, a.dtype) == (b.how, b.shape, b.dtype) and a.host.tobytes() == b.host.tobytes()
    (loss,), (swept,) = calls_of(rt, BACKWARD), calls_of(rt, sweep)
    assert loss[17] is None and swept[where["eb"]] is None  # (no term touches the energy: no energy cotangent is made)
    first = where.get("rec", where.get("mb"))
    assert swept[first]["how"] == "to_device" and (loss[14] == swept[first] or loss[15] == swept[first])


def test_an_energy_term_beside_a_host_cotangent_gets_a_zero_filled_energy_buffer(recorded_with_energy):
    lx, rt, forward = recorded_with_energy
    segment, beam, keywords, sweep, where = _case(lx, "particles")
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets={"M1": {"normalized_emittance_x": 1e-6}})
    del rt.lib.calls[:], rt.lib.records[:]
    vjp(sigma_x=1.0, moment_loss_bar=1.0)
    assert rt.lib.calls == [MEMSET, BACKWARD, sweep]
    (filled,), (loss,), (swept,) = calls_of(rt, MEMSET), calls_of(rt, BACKWARD), calls_of(rt, sweep)
    assert filled[1] == loss[17] == swept[where["eb"]] and filled[1]["shape"] == [B, vjp.trace.num_points]
    del rt.lib.calls[:], rt.lib.records[:]
    vjp(energy_bar=np.ones((B, vjp.trace.num_points)), moment_loss_bar=1.0)  # the host's energy cotangent is uploaded and added into
    (loss,), (swept,) = calls_of(rt, BACKWARD), calls_of(rt, sweep)
    assert loss[17]["how"] == "to_device" and loss[17] == swept[where["eb"]] and MEMSET not in rt.lib.calls


def test_energy_targets_alone_behind_a_cavity_with_trajectories_leave_the_moment_path_out(recorded_with_energy):
    lx, rt, forward = recorded_with_energy
    segment, beam, _, _, _ = _case(lx, "kicks")
    sweep = "lynx_track_particles_along_backward_trajectories"
    vjp = lx.grad.track_along_vjp(segment, beam, trajectories=2, moment_targets={-1: {"energy": 1.1e8}})
    del rt.lib.calls[:], rt.lib.records[:]
    g = vjp(moment_loss_bar=1.0)
    (loss,), (swept,) = calls_of(rt, BACKWARD), calls_of(rt, sweep)
    assert loss[14]["shape"] == [B, 6, 36] and swept[4] is None and swept[5] is None and swept[9] is None and swept[10] is None
    assert loss[17] == swept[6] and swept[6]["how"] == "empty"
    with pytest.raises(KeyError):
        g.mu
    with pytest.raises(NotImplementedError, match="active Cavity 'CAV'") as info:  # exactly where a moment cotangent is refused
        lx.grad.track_along_vjp(segment, beam, trajectories=2, moment_targets={-1: {"energy": 1.1e8, "beta_x": 1.0}})
    with pytest.raises(NotImplementedError) as of_call:
        vjp(beta_x=1.0)
    assert str(info.value) == str(of_call.value)


def test_a_target_on_a_point_nobody_reaches_is_refused_with_the_text_of_the_cotangent(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import engine

    rt, forward = fake_gpu(monkeypatch, nobody=((1, 5),))
    fabricated = engine.track_along

    def track_along(owner, leaves, incoming, **kwargs):
        trace = fabricated(owner, leaves, incoming, **kwargs)
        trace._device["energy"] = rt.forward("energy", (B, trace.num_points), incoming.dtype)
        return trace

    monkeypatch.setattr(engine, "track_along", track_along)
    segment, beam, keywords, _, _ = _case(lx, "survivors")
    with pytest.raises(ValueError) as info:
        lx.grad.track_along_vjp(segment, beam, moment_targets={5: {"sigma_x": 1e-4}}, **keywords)
    assert FORWARD not in rt.lib.calls
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets={5: {"energy": 1e8}, 4: {"sigma_x": 1e-4}}, **keywords)  # (the energy is there)
    w = np.zeros((B, vjp.trace.num_points))
    w[1, 5] = 1.0
    with pytest.raises(ValueError) as of_call:
        vjp(sigma_x=w)
    assert str(info.value) == str(of_call.value) and "sample (1,), point 5, which no particle reaches" in str(info.value)


def test_moment_loss_bar_without_targets_and_one_that_does_not_broadcast(recorded_with_energy):
    lx, rt, forward = recorded_with_energy
    segment, beam, keywords, _, _ = _case(lx, "moments")
    vjp = lx.grad.track_along_vjp(segment, beam)
    assert "keep_energy" not in forward[-1]
    with pytest.raises(ValueError) as info:
        vjp(moment_loss_bar=1.0)
    assert str(info.value) == ("track_along_vjp: moment_loss_bar needs the moment loss of the forward pass -- pass moment_targets= to "
                               "track_along_vjp")
    with pytest.raises(ValueError) as image:
        vjp(image_loss_bar=1.0)
    assert str(image.value) == str(info.value).replace("moment", "image")
    for read in ("moment_loss", "moment_values"):
        with pytest.raises(ValueError, match="pass moment_targets= to track_along_vjp"):
            getattr(vjp, read)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets=TARGETS)
    with pytest.raises(ValueError, match=r"moment_loss_bar has shape \(3,\), which does not broadcast to the batch \(2,\)"):
        vjp(moment_loss_bar=np.ones(3))


def test_with_image_targets_and_screens_all_three_go_in_front_of_one_sweep(recorded_with_energy, monkeypatch):
    lx, rt, forward = recorded_with_energy
    from lynx_amd import engine

    from .test_trace_screens_grad_host import _lattice as screened
    from .test_trace_screens_grad_host import _parameters as float64_parameters

    segment, first, idle, last, quad, aperture = screened(lx, batch=(B,))
    vjp = lx.grad.track_along_vjp(segment, float64_parameters(lx, (B,)), screens=True, image_targets={last: np.ones((33, 17))},
                                  moment_targets={"Q": {"beta_x": 3.0}})
    assert forward[-1] == dict(keep_outgoing=True, keep_device=True, screens=True, keep_energy=True)
    assert rt.lib.calls == ["lynx_gaussian_images_along_mse", FORWARD]
    del rt.lib.calls[:], rt.lib.records[:]
    vjp(screen_images_bar={first: 1.0}, image_loss_bar=1.0, moment_loss_bar=1.0)
    assert rt.lib.calls == [MEMSET, MEMSET, "lynx_gaussian_images_along_backward", "lynx_gaussian_images_along_mse_backward", BACKWARD,
                            "lynx_track_moments_along_backward"]
    (loss,), (swept,) = calls_of(rt, BACKWARD), calls_of(rt, "lynx_track_moments_along_backward")
    assert loss[15] == swept[5] and loss[16] == swept[6] and loss[1] == 1  # float64


# ---------------------------------------------------------------------------------------------
# 4. the entries are declared
# ---------------------------------------------------------------------------------------------


def test_the_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for entry in (FORWARD, BACKWARD):
        assert entry in _ffi.SIGNATURES and f"int {entry}(" in header
    names = lambda entry: [part.split()[-1].lstrip("*") for part in re.search(rf"int {entry}\((.*?)\);", header, re.S).group(1).split(",")]  # noqa: E731
    shared = ["ctx", "dtype", "batch", "n_points", "d_records", "d_mu_trace", "d_cov_trace", "d_energy_trace", "ddof", "n_target_points",
              "target_points", "d_rows", "row_stride"]
    assert names(FORWARD) == shared + ["d_values", "d_point_loss", "d_loss"]
    assert names(BACKWARD) == shared + ["d_loss_bar", "d_grad_trace", "d_mu_bar", "d_cov_bar", "d_energy_bar"]
    assert len(_ffi.SIGNATURES[FORWARD][1]) == 16 and len(_ffi.SIGNATURES[BACKWARD][1]) == 18
    assert _ffi.SIGNATURES[FORWARD][1][:13] == _ffi.SIGNATURES[BACKWARD][1][:13]
    flat = re.sub(r"\s+\*?\s*", " ", header)
    assert 'starts with "moment loss along the trace: "' in flat and flat.count("the same call returns the same bits") >= 6


def test_the_new_kernels_use_no_atomics_and_have_a_header_of_their_own():
    source = (ROOT / "lynx_amd" / "csrc" / "lynx_moment_loss.hpp").read_text()
    code = re.sub(r"//.*", "", source)
    assert "atomic" not in code.lower() and "__shared__" not in code
    for kernel in ("k_moment_loss_fwd", "k_moment_loss_finish", "k_moment_loss_bwd"):
        assert kernel in code
    assert '#include "lynx_moment_loss.hpp"' in (ROOT / "lynx_amd" / "csrc" / "lynx_hip.hip").read_text()
