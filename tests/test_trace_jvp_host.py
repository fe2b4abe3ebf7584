"""
`lynx_amd.grad.track_along_jvp` without a GPU: the NumPy restatement of the forward-mode recursion (tests/trace_jvp_reference.py)
against central differences of the oracle's `element_track` chain, the CSR assembly of `wrt`, the refusals -- raised before
anything touches the GPU -- and the two C entry points being declared.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import trace_jvp_reference as ref
from .helpers import make_lattice
from .test_gpu_grad import PARAMS_TO_CHECK, _desc
from .test_gpu_trace_grad import _chain

ROOT = Path(__file__).resolve().parent.parent
TOL_FD = 2e-4  # of the value: the tolerance of test_gpu_trace_grad's finite-difference tests


def lattice_without_cavities(B, rng):
    """The nine-element lattice of test_gpu_grad._desc with its two cavities replaced by drifts of their lengths."""
    return [("drift", dict(length=kw["length"])) if kind == "cavity" else (kind, kw) for kind, kw in _desc(B, rng)]


def incoming_moments(B, rng):
    A = rng.normal(size=(B, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3]
    cov = np.zeros((B, 7, 7))
    cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2)
    mu = np.concatenate([rng.normal(size=(B, 6)) * [1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3], np.ones((B, 1))], axis=-1)
    return mu, cov


def directions_to_check(desc, specs):
    """[(label, [(leaf, name, component, weight)])]: every parameter of PARAMS_TO_CHECK of every element, and the energy."""
    out = []
    for e, (kind, _) in enumerate(desc):
        for name in PARAMS_TO_CHECK.get(kind, []):
            if specs[e][name] is None:
                continue
            for component in ((0, 1) if specs[e][name].ndim == 2 else (None,)):
                out.append(((e, name, component), [(e, name, component, 1.0)]))
    out.append(("energy", [(e, "energy", None, 1.0) for e in range(len(desc))]))
    return out


def test_the_restatement_matches_central_differences_of_the_oracle_chain():
    rng = np.random.default_rng(23)
    B = 2
    desc = lattice_without_cavities(B, rng)
    _, specs = make_lattice(desc, np.float64)
    mu, cov = incoming_moments(B, rng)
    energy = np.array([6e6, 8e6])
    make_beam = lambda e: o.parameter_beam(mu, cov, e, np.float64)  # noqa: E731
    beams = _chain(specs, make_beam(energy))
    checked = 0
    for label, direction in directions_to_check(desc, specs):
        mu_t, cov_t, mu_dot, cov_dot = ref.sweep(specs, energy, mu, cov, direction)
        assert np.allclose(mu_t, np.stack([b["mu"] for b in beams], axis=1), rtol=1e-12, atol=1e-18)
        assert np.allclose(cov_t, np.stack([b["cov"] for b in beams], axis=1), rtol=1e-10, atol=1e-24)
        fd_mu, fd_cov, noise_mu, noise_cov = ref.chain_tangents(specs, make_beam, ref.parameter_moments, energy, direction)
        assert np.any(fd_mu != 0), label  # (a misalignment or a corrector's angle moves the mean alone: cov_dot = 0 exactly)
        assert np.any(fd_cov != 0) or label[1] in ("misalignment", "angle"), label
        assert ref.distance(mu_dot, fd_mu, noise_mu) <= TOL_FD, (label, "mu_dot", ref.distance(mu_dot, fd_mu, noise_mu))
        assert ref.distance(cov_dot, fd_cov, noise_cov) <= TOL_FD, (label, "cov_dot", ref.distance(cov_dot, fd_cov, noise_cov))
        assert not mu_dot[:, 0].any() and not cov_dot[:, 0].any() and not mu_dot[..., 6].any()
        assert not cov_dot[..., 6, :].any() and not cov_dot[..., :, 6].any()
        checked += 1
    assert checked > 20


def _f(v, dtype=np.float64):
    return np.array([v], dtype=dtype)


def test_the_csr_assembly_of_wrt():
    import lynx_amd as lx
    from lynx_amd import grad

    q = lx.Quadrupole(_f(0.2), k1=_f(2.0), misalignment=np.array([[1e-4, -2e-4]]), dtype=np.float64)
    d = lx.Drift(_f(0.5), dtype=np.float64)
    bend = lx.RBend(_f(0.3), angle=_f(0.1), dtype=np.float64)
    marker = lx.Marker(name="M")
    leaves = [q, d, bend, marker, q, d, q]
    start, leaf, row, weight = grad._jvp_directions(
        leaves, [(q, "k1"), (bend, "angle"), (q, "misalignment", 1), "energy", (d, "length"), (q, "misalignment", 0)])
    assert (start.dtype, leaf.dtype, row.dtype, weight.dtype) == (np.int32, np.int32, np.int32, np.float64)
    assert start.tolist() == [0, 3, 6, 9, 16, 18, 21]
    per = lambda k: (leaf[start[k]:start[k + 1]].tolist(), row[start[k]:start[k + 1]].tolist(), weight[start[k]:start[k + 1]].tolist())  # noqa: E731
    # an element object placed three times: an entry per place
    assert per(0) == ([0, 4, 6], [1, 1, 1], [1.0, 1.0, 1.0])
    # RBend.angle also feeds e1 and e2 with weight 1/2 (rows of a dipole: length, angle, e1, e2, ...)
    assert per(1) == ([2, 2, 2], [1, 2, 3], [1.0, 0.5, 0.5])
    # a vector parameter's rows (a quadrupole's: length, k1, tilt, misalignment_x, misalignment_y)
    assert per(2) == ([0, 4, 6], [4, 4, 4], [1.0, 1.0, 1.0]) and per(5)[1] == [3, 3, 3]
    # the incoming energy: one entry per leaf, the marker included, on the energy's row
    assert per(3) == (list(range(7)), [grad.ENERGY_ROW] * 7, [1.0] * 7) and grad.ENERGY_ROW == 8
    assert per(4) == ([1, 5], [0, 0], [1.0, 1.0])
    # a Dipole's angle is its own row alone
    dipole = lx.Dipole(_f(0.3), angle=_f(0.1), dtype=np.float64)
    _, leaf, row, weight = grad._jvp_directions([dipole], [(dipole, "angle")])
    assert (leaf.tolist(), row.tolist(), weight.tolist()) == ([0], [1], [1.0])


def test_refusals_are_raised_before_any_gpu_call(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine, grad

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along_jvp touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    parameters = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), sigma_xp=f(1e-5), energy=f(1e8))
    drift, quadrupole = lx.Drift(f(1.0), name="D1"), lx.Quadrupole(f(0.2), k1=f(1.0), name="Q1")
    corrector, bpm = lx.HorizontalCorrector(f(0.1), angle=f(0.0), name="HC"), lx.BPM(name="BPM1")
    plain = lx.Segment([drift, quadrupole, corrector, bpm])
    for beam in (particles, parameters):
        # a Cavity that has voltage, whatever the beam
        cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
        with pytest.raises(NotImplementedError, match="ACC1"):
            grad.track_along_jvp(lx.Segment([drift, cavity]), beam, [(drift, "length")])
        # an active Screen or Aperture: `trace_program` names it
        with pytest.raises(NotImplementedError, match="SCR7"):
            grad.track_along_jvp(lx.Segment([drift, lx.Screen(is_active=True, name="SCR7")]), beam, [(drift, "length")])
        with pytest.raises(NotImplementedError, match="AP1"):
            grad.track_along_jvp(lx.Segment([drift, lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=True, name="AP1")]), beam,
                                 [(drift, "length")])
        # a parameter the element does not have; a component of a scalar and a vector without one
        with pytest.raises(KeyError, match="k1"):
            grad.track_along_jvp(plain, beam, [(drift, "k1")])
        with pytest.raises(KeyError, match="angle"):
            grad.track_along_jvp(plain, beam, [(bpm, "angle")])
        with pytest.raises(ValueError, match="two components"):
            grad.track_along_jvp(plain, beam, [(quadrupole, "misalignment")])
        with pytest.raises(ValueError, match="one component"):
            grad.track_along_jvp(plain, beam, [(quadrupole, "k1", 0)])
        with pytest.raises(KeyError, match="only direction given by a string"):
            grad.track_along_jvp(plain, beam, ["k1"])
        # an element that is not in the lattice
        with pytest.raises(KeyError, match="not an element of this lattice"):
            grad.track_along_jvp(plain, beam, [(lx.Drift(f(1.0)), "length")])
        # an empty wrt
        with pytest.raises(ValueError, match="wrt is empty"):
            grad.track_along_jvp(plain, beam, [])
        # `resolution=` is not offered
        with pytest.raises(TypeError):
            grad.track_along_jvp(plain, beam, [(drift, "length")], resolution=0.1)
        # the response matrix: the same refusals, and one of each is needed
        with pytest.raises(ValueError, match="0 BPMs"):
            grad.orbit_response_matrix(lx.Segment([drift, corrector]), beam)
        with pytest.raises(ValueError, match="0 correctors"):
            grad.orbit_response_matrix(lx.Segment([drift, bpm]), beam)
        with pytest.raises(KeyError, match="not an element of this lattice"):
            grad.orbit_response_matrix(plain, beam, bpms=[lx.BPM(name="other")])
    with pytest.raises(TypeError, match="ParticleBeam or a ParameterBeam"):
        grad.track_along_jvp(plain, None, [(drift, "length")])
    # the parameters of a cavity without voltage (a drift-like element of a run): only its length has no say in the energy
    idle = lx.Cavity(f(1.0), voltage=f(0.0), phase=f(0.0), frequency=f(1.3e9), name="IDLE")
    with pytest.raises(NotImplementedError, match="IDLE"):
        grad.track_along_jvp(lx.Segment([drift, idle]), parameters, [(idle, "voltage")])


def test_both_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    names = lambda entry: [part.split()[-1].lstrip("*") for part in re.search(rf"int {entry}\((.*?)\);", header, re.S).group(1).split(",")]  # noqa: E731
    directions = ["dir_start", "dir_leaf", "dir_row", "dir_weight", "n_directions", "n_entries", "d_mu_dot", "d_cov_dot"]
    moments, particles = "lynx_track_moments_along_forward", "lynx_track_particles_along_forward"
    for entry in (moments, particles):
        assert entry in _ffi.SIGNATURES and f"int {entry}(" in header
        assert len(_ffi.SIGNATURES[entry][1]) == 13 and len(names(entry)) == 13
        assert names(entry)[-8:] == directions
    # the arguments in front of the directions are those of the two reverse entries
    assert names(moments)[:5] == names("lynx_track_moments_along_backward")[:5]
    assert names(particles)[:5] == names("lynx_track_particles_along_backward")[:5]
    assert _ffi.SIGNATURES[moments][1][:5] == _ffi.SIGNATURES["lynx_track_moments_along_backward"][1][:5]
    assert _ffi.SIGNATURES[particles][1][:5] == _ffi.SIGNATURES["lynx_track_particles_along_backward"][1][:5]
    flat = re.sub(r"\s+\*?\s*", " ", header)
    assert 'starts with "beam trace tangents: "' in flat and "left for a later version" in flat
