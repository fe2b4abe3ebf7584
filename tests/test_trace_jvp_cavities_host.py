"""
`lynx_amd.grad.track_along_jvp(..., cavities=True)` without a GPU: the NumPy restatement of the forward-mode recursion through
cavities (tests/trace_jvp_cavities_reference.py) against central differences of the oracle's `element_track` chain, the CSR
assembly of `wrt` with the energy entries behind a cavity, the refusals -- raised before anything touches the GPU -- and the
new C entry point being declared.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import trace_jvp_cavities_reference as cref
from . import trace_jvp_reference as ref
from .helpers import make_lattice
from .test_gpu_grad import _desc
from .test_gpu_trace_grad import _chain
from .test_trace_jvp_host import TOL_FD, directions_to_check, incoming_moments

ROOT = Path(__file__).resolve().parent.parent


def test_the_restatement_matches_central_differences_of_the_oracle_chain_through_cavities():
    """The nine-element lattice of test_gpu_grad._desc WITH its two cavities, seed 23, B = 2, 6 and 8 MeV: every direction of
    `directions_to_check` -- both cavities' length, voltage, phase and frequency and the incoming energy among them -- at
    TOL_FD; states and energies against the oracle chain; e_dot behind a cavity along its voltage is cos(phi)."""
    rng = np.random.default_rng(23)
    B = 2
    desc = _desc(B, rng)
    _, specs = make_lattice(desc, np.float64)
    mu, cov = incoming_moments(B, rng)
    energy = np.array([6e6, 8e6])
    make_beam = lambda e: o.parameter_beam(mu, cov, e, np.float64)  # noqa: E731
    beams = _chain(specs, make_beam(energy))
    labelled = directions_to_check(desc, specs)
    assert len(labelled) == 29
    worst, where = 0.0, None
    for label, direction in labelled:
        mu_t, cov_t, e_t, mu_dot, cov_dot, e_dot = cref.sweep(specs, energy, mu, cov, direction)
        assert np.allclose(mu_t, np.stack([b["mu"] for b in beams], axis=1), rtol=1e-10, atol=1e-18), label
        assert np.allclose(cov_t, np.stack([b["cov"] for b in beams], axis=1), rtol=1e-10, atol=1e-24), label
        assert np.allclose(e_t, np.stack([b["energy"] for b in beams], axis=1), rtol=1e-10, atol=0), label
        fd_mu, fd_cov, noise_mu, noise_cov = ref.chain_tangents(specs, make_beam, ref.parameter_moments, energy, direction)
        fd_e, _, noise_e, _ = ref.chain_tangents(specs, make_beam, cref.energy_moments, energy, direction)
        dist = (ref.distance(mu_dot, fd_mu, noise_mu), ref.distance(cov_dot, fd_cov, noise_cov))
        if max(dist) > worst:
            worst, where = max(dist), label
        assert max(dist) <= TOL_FD, (label, dist)
        if np.any(fd_e != 0):
            assert ref.distance(e_dot[..., None], fd_e, noise_e) <= TOL_FD, (label, "e_dot")
        else:
            assert not e_dot.any(), label
        assert not mu_dot[:, 0].any() and not cov_dot[:, 0].any() and not mu_dot[..., 6].any()
        assert not cov_dot[..., 6, :].any() and not cov_dot[..., :, 6].any()
        if label != "energy" and label[1] == "voltage":  # behind the cavity: cos(phi) per sample, and nothing in front of it
            e = label[0]
            assert np.array_equal(e_dot[:, -1], np.cos(np.deg2rad(specs[e]["phase"]))) and not e_dot[:, : e + 1].any()
    print(f"restatement through cavities against central differences of the oracle chain: worst distance {worst:.1e} at {where}")


def _f(v, dtype=np.float64):
    return np.array([v], dtype=dtype)


def test_the_csr_assembly_of_wrt_with_cavities():
    import lynx_amd as lx
    from lynx_amd import grad

    q = lx.Quadrupole(_f(0.2), k1=_f(2.0), dtype=np.float64)
    d = lx.Drift(_f(0.5), dtype=np.float64)
    cav = lx.Cavity(_f(1.0), voltage=_f(1e7), phase=_f(5.0), frequency=_f(1.3e9), dtype=np.float64, name="CAV")
    idle = lx.Cavity(_f(1.0), voltage=_f(0.0), phase=_f(0.0), frequency=_f(1.3e9), dtype=np.float64, name="IDLE")
    leaves = [q, cav, d, idle, q, d]
    E = grad.ENERGY_ROW
    per = lambda out, k: tuple(a[out[0][k]:out[0][k + 1]].tolist() for a in out[1:])  # noqa: E731
    out = grad._jvp_directions(leaves, [(cav, "voltage"), (cav, "phase"), "energy", (cav, "frequency"), (cav, "length")], cavities=True)
    assert [a.dtype for a in out] == [np.int32, np.int32, np.int32, np.float64]
    assert out[0].tolist() == [0, 5, 10, 16, 17, 18]
    # voltage (row 1), phase (row 2): the entry itself, then the energy at every leaf BEHIND the cavity, weight 1
    assert per(out, 0) == ([1, 2, 3, 4, 5], [1, E, E, E, E], [1.0] * 5)
    assert per(out, 1) == ([1, 2, 3, 4, 5], [2, E, E, E, E], [1.0] * 5)
    # the incoming energy: one entry per leaf, as without the keyword
    assert per(out, 2) == (list(range(6)), [E] * 6, [1.0] * 6)
    # frequency and length do not move the energy
    assert per(out, 3) == ([1], [3], [1.0]) and per(out, 4) == ([1], [0], [1.0])
    # a mixed item list keeps its order; the quadrupole placed twice has an entry per place and no energy entry
    mixed = grad._jvp_directions(leaves, [(q, "k1"), (cav, "phase"), (d, "length")], cavities=True)
    assert mixed[0].tolist() == [0, 2, 7, 9]
    assert per(mixed, 0) == ([0, 4], [1, 1], [1.0, 1.0]) and per(mixed, 2) == ([2, 5], [0, 0], [1.0, 1.0])
    assert per(mixed, 1) == per(out, 1)
    # a cavity object placed twice: an entry per place, the energy behind the FIRST place (once per leaf)
    twice = grad._jvp_directions([d, cav, q, cav, d], [(cav, "voltage")], cavities=True)
    assert per(twice, 0) == ([1, 3, 2, 3, 4], [1, 1, E, E, E], [1.0] * 5)
    # the default output is what it was: the cases of test_trace_jvp_host, with and without the keyword's default
    bend = lx.RBend(_f(0.3), angle=_f(0.1), dtype=np.float64)
    plain_leaves = [q, d, bend, lx.Marker(name="M"), q, d, q]
    wrt = [(q, "k1"), (bend, "angle"), "energy", (d, "length")]
    for a, b, c in zip(grad._jvp_directions(plain_leaves, wrt), grad._jvp_directions(plain_leaves, wrt, cavities=False),
                       grad._jvp_directions(plain_leaves, wrt, cavities=True)):
        assert a.tobytes() == b.tobytes() == c.tobytes() and a.dtype == b.dtype == c.dtype
    assert grad._jvp_directions(plain_leaves, wrt)[0].tolist() == [0, 3, 6, 13, 15]
    with pytest.raises(NotImplementedError, match="CAV"):  # without the keyword: today's refusal
        grad._jvp_directions(leaves, [(cav, "voltage")])


def test_refusals_with_cavities_are_raised_before_any_gpu_call(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine, grad

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along_jvp touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    parameters = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), sigma_xp=f(1e-5), energy=f(1e8))
    drift, corrector, bpm = lx.Drift(f(1.0), name="D1"), lx.HorizontalCorrector(f(0.1), angle=f(0.0), name="HC"), lx.BPM(name="BPM1")
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
    idle = lx.Cavity(f(1.0), voltage=f(0.0), phase=f(0.0), frequency=f(1.3e9), name="IDLE")
    # a ParticleBeam and an active cavity: its moments are not closed under the kick
    with pytest.raises(NotImplementedError, match="ACC1"):
        grad.track_along_jvp(lx.Segment([drift, cavity]), particles, [(drift, "length")], cavities=True)
    with pytest.raises(NotImplementedError, match="ACC1"):
        grad.orbit_response_matrix(lx.Segment([corrector, cavity, bpm]), particles, cavities=True)
    # voltage, phase, frequency of a cavity without voltage: today's refusal, with the keyword too
    for name in ("voltage", "phase", "frequency"):
        with pytest.raises(NotImplementedError, match="IDLE"):
            grad.track_along_jvp(lx.Segment([drift, idle, cavity]), parameters, [(idle, name)], cavities=True)
    # the keyword is True or False
    with pytest.raises(ValueError, match="cavities is True or False"):
        grad.track_along_jvp(lx.Segment([drift, cavity]), parameters, [(drift, "length")], cavities="yes")
    # and without it everything is refused as before
    with pytest.raises(NotImplementedError, match="ACC1"):
        grad.track_along_jvp(lx.Segment([drift, cavity]), parameters, [(drift, "length")])


def test_the_entry_point_is_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    names = lambda entry: [part.split()[-1].lstrip("*") for part in re.search(rf"int {entry}\((.*?)\);", header, re.S).group(1).split(",")]  # noqa: E731
    entry, sibling = "lynx_track_moments_along_forward_cavities", "lynx_track_moments_along_forward"
    assert entry in _ffi.SIGNATURES and f"int {entry}(" in header
    assert len(_ffi.SIGNATURES[entry][1]) == 15 and len(names(entry)) == 15
    assert _ffi.SIGNATURES[entry][1][:13] == _ffi.SIGNATURES[sibling][1] and names(entry)[:13] == names(sibling)
    assert names(entry)[13:] == ["dir_energy_seed", "d_energy_dot"]
