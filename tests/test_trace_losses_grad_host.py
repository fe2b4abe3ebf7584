"""
`lynx_amd.grad.track_along_vjp(..., losses=True)` without a GPU: the two C entry points being declared, and the refusals
by value, which are raised before anything touches the GPU.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .reverse_host_fakes import no_gpu  # noqa: F401 (fixture)

ROOT = Path(__file__).resolve().parent.parent


def test_both_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for name in ("lynx_moments_by_loss", "lynx_track_particles_along_backward_losses"):
        assert name in _ffi.SIGNATURES
        assert f"int {name}(" in header
    assert len(_ffi.SIGNATURES["lynx_moments_by_loss"][1]) == 9
    assert len(_ffi.SIGNATURES["lynx_track_particles_along_backward_losses"][1]) == 12


def _f(v):
    return np.array([v], dtype=np.float32)


def _particles(lx):
    return lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), _f(1e8))


def _collimated(lx, apertures):
    elements = [lx.Drift(_f(1.0), name="D")]
    for k in range(apertures):
        elements += [lx.Aperture(x_max=_f(1e-3), y_max=_f(1e-3), is_active=True, name=f"COL{k}"), lx.Drift(_f(0.1), name=f"D{k}")]
    return lx.Segment(elements)


def test_refusals_are_raised_before_any_gpu_call(no_gpu):
    import lynx_amd as lx
    from lynx_amd import grad

    particles = _particles(lx)
    # `losses` is a bool
    for bad in ("particles", 1, None, 0.0):
        with pytest.raises(ValueError, match="losses"):
            grad.track_along_vjp(_collimated(lx, 1), particles, losses=bad)
    # not together with trajectories
    with pytest.raises(NotImplementedError, match="losses=True.*trajectories="):
        grad.track_along_vjp(_collimated(lx, 1), particles, trajectories=4, losses=True)
    # more than 15 active apertures: the 16th is named
    with pytest.raises(NotImplementedError, match="16 active apertures.*'COL15'"):
        grad.track_along_vjp(_collimated(lx, 16), particles, losses=True)
    # ... inactive ones do not count (15 active ones reach the GPU runtime: that is the stub's AssertionError)
    segment = _collimated(lx, 16)
    segment.COL3.is_active = False
    with pytest.raises(AssertionError, match="touched the GPU runtime"):
        grad.track_along_vjp(segment, particles, losses=True)
    # an active cavity in front of a ParticleBeam is refused as without losses
    cavity = lx.Cavity(_f(1.0), voltage=_f(1e7), phase=_f(0.0), frequency=_f(1.3e9), name="ACC1")
    with pytest.raises(NotImplementedError, match="ACC1"):
        grad.track_along_vjp(lx.Segment([*_collimated(lx, 1).elements, cavity]), particles, losses=True)
    # an active Screen has no place in the differentiated trace
    with pytest.raises(NotImplementedError, match="SCR7"):
        grad.track_along_vjp(lx.Segment([*_collimated(lx, 1).elements, lx.Screen(is_active=True, name="SCR7")]), particles, losses=True)
    # more than 256 leaves
    long = lx.Segment([*_collimated(lx, 1).elements, *[lx.Drift(_f(0.1), name=f"T{k}") for k in range(254)]])
    with pytest.raises(NotImplementedError, match="257 leaf elements.*'T253'"):
        grad.track_along_vjp(long, particles, losses=True)


def test_losses_false_still_refuses_an_active_aperture(no_gpu):
    import lynx_amd as lx
    from lynx_amd import grad

    for kwargs in ({}, {"losses": False}):
        with pytest.raises(NotImplementedError, match="COL0"):
            grad.track_along_vjp(_collimated(lx, 1), _particles(lx), **kwargs)
