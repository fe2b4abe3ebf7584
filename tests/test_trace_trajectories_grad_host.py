"""
Gradients of chosen particles' trajectories (`track_along_vjp(..., trajectories=)`, `vjp(trajectories_bar=)`) without a
GPU: the C entry point being declared, every refusal raised by value before a runtime exists, and `track_along_vjp`
without `trajectories=` making the calls it made before -- the new entry point is never named.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .reverse_host_fakes import no_gpu, recorded  # noqa: F401 (fixtures)

ROOT = Path(__file__).resolve().parent.parent
N = 16
ENTRY = "lynx_track_particles_along_backward_trajectories"

f = lambda v: np.array([v], dtype=np.float64)  # noqa: E731


def test_the_entry_point_is_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    assert ENTRY in _ffi.SIGNATURES and f"int {ENTRY}(" in header
    # lynx_track_particles_along_backward's arguments, then n_chosen, d_trajectories, d_trajectories_bar, d_grad_chosen_in
    base = _ffi.SIGNATURES["lynx_track_particles_along_backward"][1]
    args = _ffi.SIGNATURES[ENTRY][1]
    assert args[:len(base)] == base and len(args) == len(base) + 4
    assert args[len(base)] is _ffi._i64
    declaration = re.search(rf"int {ENTRY}\((.*?)\);", header, re.S).group(1)
    names = [part.split()[-1].lstrip("*") for part in declaration.split(",")]
    assert names[-4:] == ["n_chosen", "d_trajectories", "d_trajectories_bar", "d_grad_chosen_in"]
    old = re.search(r"int lynx_track_particles_along_backward\((.*?)\);", header, re.S).group(1)
    assert names[:-4] == [part.split()[-1].lstrip("*") for part in old.split(",")]
    assert "beam trace gradients with trajectories: " in header.replace("\n * ", " ").replace("  ", " ")


def _line(lx):
    return lx.Segment([lx.Drift(f(1.0), dtype=np.float64), lx.Quadrupole(f(0.2), k1=f(2.0), dtype=np.float64)])


def _beam(lx, batch=(1,)):
    return lx.ParticleBeam(o.gaussian_particles(batch, N, seed=1, dtype=np.float64), np.full(batch, 1e8), dtype=np.float64)


def test_without_trajectories_the_calls_are_the_ones_they_were(recorded):
    lx, calls, forward = recorded
    vjp = lx.grad.track_along_vjp(_line(lx), _beam(lx))
    assert forward == [dict(keep_outgoing=True, keep_device=True)]  # (no `trajectories` argument at all)
    vjp(mu_bar=np.ones((1, 3, 6)), energy_bar=np.ones((1, 3)))
    vjp(sigma_x=1.0)
    assert calls == ["lynx_track_particles_along_backward"] * 2
    with pytest.raises(KeyError):
        vjp(mu_x=1.0).chosen_particles


def test_with_trajectories_every_cotangent_goes_into_one_call(recorded):
    lx, calls, forward = recorded
    vjp = lx.grad.track_along_vjp(_line(lx), _beam(lx), trajectories=[3, 0, 3])
    assert list(forward[0]["trajectories"]) == [3, 0, 3] and forward[0]["keep_device"] is True
    g = vjp(trajectories_bar=np.ones((1, 3, 3, 6)), mu_bar=np.ones((1, 3, 6)), energy_bar=np.ones((1, 3)), sigma_y=1.0)
    assert calls == [ENTRY]
    assert g.chosen_particles.shape == (1, 3, 7) and g.mu.shape == (1, 7)
    only = vjp(trajectories_bar=np.ones(6))  # (broadcast over batch, points and particles)
    assert calls == [ENTRY] * 2 and only.chosen_particles.shape == (1, 3, 7)
    with pytest.raises(KeyError):  # no moment cotangent: the moment path did not run
        only.mu


def test_trajectories_bar_without_trajectories_is_a_value_error(recorded):
    lx, calls, _ = recorded
    vjp = lx.grad.track_along_vjp(_line(lx), _beam(lx))
    with pytest.raises(ValueError, match="trajectories=") as info:
        vjp(trajectories_bar=np.ones((1, 3, 2, 6)))
    assert "trajectories_bar" in str(info.value)
    assert calls == []


@pytest.mark.parametrize("shape", [(1, 3, 4, 6), (1, 2, 3, 6), (2, 3, 3, 7), (1, 3, 3, 5), (3, 3), ()])
def test_a_shape_that_does_not_broadcast_is_a_value_error_that_names_both_shapes(recorded, no_gpu, shape):
    lx, calls, _ = recorded
    vjp = lx.grad.track_along_vjp(_line(lx), _beam(lx), trajectories=3)
    with pytest.raises(ValueError) as info:
        vjp(trajectories_bar=np.ones(shape))
    assert str(shape) in str(info.value) and "(1, 3, 3, 6)" in str(info.value) and "(1, 3, 3, 7)" in str(info.value)
    assert calls == []


def test_a_parameter_beam_is_the_type_error_of_track_along(no_gpu):
    import lynx_amd as lx

    beam = lx.ParameterBeam.from_parameters()
    segment = lx.Segment([lx.Drift(np.array([1.0], dtype=np.float32))])
    with pytest.raises(TypeError, match="ParameterBeam") as info:
        lx.grad.track_along_vjp(segment, beam, trajectories=3)
    with pytest.raises(TypeError) as forward:
        segment.track_along(beam, trajectories=3)
    assert str(info.value) == str(forward.value)


@pytest.mark.parametrize("selection, named", [(True, "True"), (0, "0"), ([], r"\[\]"), ([1.5], "1.5"), (N + 1, str(N + 1)), ([-1], "-1")])
def test_a_bad_selection_is_the_value_error_of_track_along(no_gpu, selection, named):
    import lynx_amd as lx

    with pytest.raises(ValueError, match=named) as info:
        lx.grad.track_along_vjp(_line(lx), _beam(lx), trajectories=selection)
    assert "trajectories" in str(info.value)


def _with_cavity(lx):
    return lx.Segment([lx.Drift(f(1.0), dtype=np.float64),
                       lx.Cavity(f(1.0377), voltage=f(1.8e7), phase=f(3.0), frequency=f(1.3e9), name="CAV1", dtype=np.float64),
                       lx.Drift(f(0.4), dtype=np.float64)])


def test_a_cavity_without_trajectories_stays_refused_at_construction(no_gpu):
    import lynx_amd as lx

    with pytest.raises(NotImplementedError, match="CAV1"):
        lx.grad.track_along_vjp(_with_cavity(lx), _beam(lx))


def test_a_cavity_with_trajectories_refuses_moment_cotangents_only(recorded):
    lx, calls, _ = recorded
    bpm = lx.BPM(is_active=True, name="BPM1")
    segment = lx.Segment([*_with_cavity(lx).elements, bpm])
    vjp = lx.grad.track_along_vjp(segment, _beam(lx), trajectories=2)
    for moment in (dict(mu_bar=np.ones((1, 5, 6))), dict(cov_bar=np.ones((1, 5, 6, 6))), dict(beta_x=1.0),
                   dict(readings={bpm: np.ones((2, 1))}), dict(mu_bar=np.ones((1, 5, 6)), trajectories_bar=np.ones(6))):
        with pytest.raises(NotImplementedError, match="CAV1") as info:
            vjp(**moment)
        assert "not closed under a cavity's kick" in str(info.value)
    assert calls == []
    g = vjp(trajectories_bar=np.ones(7), energy_bar=np.ones((1, 5)), energy=1.0)
    assert calls == [ENTRY] and g.chosen_particles.shape == (1, 2, 7)
