"""
`lynx_amd.grad.track_along_vjp(..., cavities=True)` without a GPU: the entry point's declaration, the refusals by value, and
the mathematics of lynx_track_particles_along_backward_cavities -- a moment cotangent at EVERY point of a lattice with a
gaining cavity, carried back per particle -- stated in NumPy float64 and held to central differences of the oracle's
particle chain (`o.element_track`, element by element).
"""

import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAME = "lynx_track_particles_along_backward_cavities"


def test_the_entry_point_is_declared_with_twelve_arguments():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    assert NAME in _ffi.SIGNATURES and f"int {NAME}(" in header
    assert len(_ffi.SIGNATURES[NAME][1]) == 12
    declared = header.split(f"int {NAME}(")[1].split(");")[0]
    assert declared.count(",") == 11


def _no_gpu(monkeypatch):
    from lynx_amd import device, engine

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along_vjp touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)


def test_refusals_are_raised_before_any_gpu_call(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import grad

    _no_gpu(monkeypatch)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
    segment = lx.Segment([lx.Drift(f(1.0)), cavity])
    for bad in (1, 0, None, "yes", np.float32(1.0)):
        with pytest.raises(ValueError, match="cavities is True or False"):
            grad.track_along_vjp(segment, particles, cavities=bad)
    with pytest.raises(NotImplementedError, match="cavities=True together with trajectories="):
        grad.track_along_vjp(segment, particles, trajectories=[0, 1], cavities=True)
    with pytest.raises(NotImplementedError, match="cavities=True together with losses=True"):
        grad.track_along_vjp(segment, particles, losses=True, cavities=True)
    # more than 64 leaves, nested segments opened up: the first one beyond is named
    long = lx.Segment([lx.Segment([lx.Drift(f(0.1), name=f"D{k}") for k in range(60)]), cavity,
                       lx.Segment([lx.Drift(f(0.1), name=f"T{k}") for k in range(4)])])
    with pytest.raises(NotImplementedError, match="65 leaf elements, more than 64.*'T3'"):
        grad.track_along_vjp(long, particles, cavities=True)
    # an active Screen is still named by the trace's plan
    with pytest.raises(NotImplementedError, match="SCR7"):
        grad.track_along_vjp(lx.Segment([cavity, lx.Screen(is_active=True, name="SCR7")]), particles, cavities=True)


def test_without_the_switch_a_cavity_is_still_refused(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import grad

    _no_gpu(monkeypatch)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
    for kwargs in ({}, {"cavities": False}):
        with pytest.raises(NotImplementedError, match="ACC1") as info:
            grad.track_along_vjp(lx.Segment([lx.Drift(f(1.0)), cavity]), particles, **kwargs)
        assert "not closed under a cavity's kick" in str(info.value) and "cavities=True" in str(info.value)


# ---- the recursion ----------------------------------------------------------------------------------------------------

B, N = 1, 16
ME, CLIGHT = o.ELECTRON_MASS_EV, o.SPEED_OF_LIGHT


def _lattice(voltage=1.2e7, phase=-8.0):
    a = lambda v: np.array([v])  # noqa: E731
    desc = [("drift", dict(length=a(0.6))), ("quadrupole", dict(length=a(0.2), k1=a(3.1))),
            ("cavity", dict(length=a(1.0377), voltage=a(voltage), phase=a(phase), frequency=a(1.3e9))),
            ("drift", dict(length=a(0.4)))]
    return make_lattice(desc, np.float64)[1]


def _steps(specs, energy):
    """[(T (7, 7), coefficients c0..c7 or None)] per element of sample 0 at the energy that enters it (cavity.py:141-226)."""
    out, E = [], float(energy)
    for spec in specs:
        if spec["kind"] != "cavity":
            out.append((o.element_transfer_map(spec, np.array([E]), np.float64)[0], None))
            continue
        T = o.cavity_rmatrix(spec, np.array([E]), np.float64)[0]
        V, phi = float(spec["voltage"][0]), float(np.deg2rad(spec["phase"][0]))
        L, k = float(spec["length"][0]), 2 * np.pi * float(spec["frequency"][0]) / CLIGHT
        E1 = E + V * np.cos(phi)
        g0, g1 = E / ME, E1 / ME
        b0, b1 = np.sqrt(1 - 1 / g0**2), np.sqrt(1 - 1 / g1**2)
        dg = V / ME
        t566 = L * (b0**3 * g0**3 - b1**3 * g1**3) / (2 * b0 * b1**3 * g0 * (g0 - g1) * g1**3)
        t556 = b0 * k * L * dg * g0 * (b1**3 * g1**3 + b0 * (g0 - g1**3)) * np.sin(phi) / (b1**3 * g1**3 * (g0 - g1) ** 2)
        t555 = b0**2 * k**2 * L * dg / 2.0 * (
            dg * (2 * g0 * g1**3 * (b0 * b1**3 - 1) + g0**2 + 3 * g1**2 - 2) / (b1**3 * g1**3 * (g0 - g1) ** 3) * np.sin(phi) ** 2
            - (g1 * g0 * (b1 * b0 - 1) + 1) / (b1 * g1 * (g0 - g1) ** 2) * np.cos(phi))
        coef = np.array([E * b0 / (E1 * b1), V * b0 / (E1 * b1), b0 * k, phi, np.cos(phi), t566, t556, t555])
        out.append((T, coef))
        E = E1
    return out


def _apply(step, z):
    T, c = step
    out = z @ T.T
    if c is not None:
        out[:, 5] = z[:, 5] * c[0] + c[1] * (np.cos(-z[:, 4] * c[2] + c[3]) - c[4])
        out[:, 4] += c[5] * z[:, 5] ** 2 + c[6] * z[:, 4] * z[:, 5] + c[7] * z[:, 4] ** 2
    return out


def _reverse(steps, z0, w_mu, w_cov):
    """
    The recursion of lynx_track_particles_along_backward_cavities for one sample.  w_mu (P, 7), w_cov (P, 6, 6) entry by
    entry -> lambda_0 (N, 7), T_bar per step, the kick's coefficient cotangents per step (kick_cotangents of lynx_grad.hpp:
    the phase's complete, the slot of cos(phi) zero).
    """
    S, n = len(steps), z0.shape[0]
    states = [z0]
    for step in steps:
        states.append(_apply(step, states[-1]))

    def inj(p):
        z = states[p]
        m = z[:, :6].mean(axis=0)
        # record cotangent: an off-diagonal entry counted once, the diagonal as it is; G_hat: diagonal doubled
        tri = w_cov[p] + w_cov[p].T
        tri[np.diag_indices(6)] = np.diag(w_cov[p])
        G = tri + np.diag(np.diag(tri))
        out = np.zeros((n, 7))
        out[:, :6] = (w_mu[p, :6] + (z[:, :6] - m) @ G.T) / n
        out[:, 6] = w_mu[p, 6] / n
        return out

    lam = inj(S)
    tbars, cbars = [None] * S, [None] * S
    for s in range(S - 1, -1, -1):
        T, c = steps[s]
        z = states[s]
        olin = lam.copy()
        d4 = d5 = 0.0
        if c is not None:
            o4b, o5b = lam[:, 4], lam[:, 5]
            z4, z5 = z[:, 4], z[:, 5]
            d = -z4 * c[2]
            dsin = np.sin(c[3]) * (np.cos(d) - 1) + np.cos(c[3]) * np.sin(d)
            dcos = np.cos(c[3]) * (np.cos(d) - 1) - np.sin(c[3]) * np.sin(d)
            sa = dsin + np.sin(c[3])
            ab = -o5b * c[1] * sa
            cbars[s] = np.array([np.sum(o5b * z5), np.sum(o5b * dcos), np.sum(ab * -z4), np.sum(-o5b * c[1] * dsin), 0.0,
                                 np.sum(o4b * z5**2), np.sum(o4b * z4 * z5), np.sum(o4b * z4**2)])
            d4 = o4b * (z5 * c[6] + 2 * z4 * c[7]) + ab * -c[2]
            d5 = o4b * (2 * z5 * c[5] + z4 * c[6]) + o5b * c[0]
            olin[:, 5] = 0.0  # the linear delta was overwritten
        tbars[s] = olin.T @ z
        lam = olin @ T
        lam[:, 4] += d4
        lam[:, 5] += d5
        lam += inj(s)
    return lam, tbars, cbars


def _chain_loss(specs, particles, energy, w_mu, w_cov):
    beam = o.particle_beam(particles[None], np.array([energy]), np.float64)
    total = 0.0
    for p in range(len(specs) + 1):
        Q = beam["particles"][0]
        mean = Q.mean(axis=0)
        d = Q[:, :6] - mean[:6]
        total += np.sum(w_mu[p] * mean) + np.sum(w_cov[p] * (d.T @ d) / Q.shape[0])
        if p < len(specs):
            beam = o.element_track(specs[p], beam, np.float64)
    return total


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(31)
    particles = o.gaussian_particles((B,), N, seed=5, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])[0]
    P = 5
    w_mu = rng.normal(size=(P, 7))  # (the 7th coordinate, too: it is 1 for every particle and takes mu_bar[6] / n alone)
    w_cov = rng.normal(size=(P, 6, 6)) * 1e3
    return particles, 6e6, w_mu, w_cov


def test_the_numpy_steps_are_the_oracles(case):
    particles, energy, _, _ = case
    specs = _lattice()
    beam = o.particle_beam(particles[None], np.array([energy]), np.float64)
    z = particles
    for spec, step in zip(specs, _steps(specs, energy)):
        beam = o.element_track(spec, beam, np.float64)
        z = _apply(step, z)
        assert np.allclose(z, beam["particles"][0], rtol=1e-12, atol=1e-18)


def test_the_cotangent_of_the_incoming_particles_matches_central_differences(case):
    """lambda_0 of three particles, every coordinate: pins inj_p -- the factor 2 on the diagonal, the masked 7th coordinate."""
    particles, energy, w_mu, w_cov = case
    specs = _lattice()
    lam, _, _ = _reverse(_steps(specs, energy), particles, w_mu, w_cov)
    for n in (0, 7, 15):
        for c in range(6):
            h = 1e-7
            up, down = particles.copy(), particles.copy()
            up[n, c] += h
            down[n, c] -= h
            ref = (_chain_loss(specs, up, energy, w_mu, w_cov) - _chain_loss(specs, down, energy, w_mu, w_cov)) / (2 * h)
            assert abs(lam[n, c] - ref) <= 1e-6 * abs(ref) + 1e-9 * np.max(np.abs(lam)), (n, c, lam[n, c], ref)
    # the 7th coordinate takes the mean's cotangent alone, at every point, through the maps' 7th columns
    only7, _, _ = _reverse(_steps(specs, energy), particles, w_mu * [0, 0, 0, 0, 0, 0, 1], np.zeros_like(w_cov))
    assert np.allclose(only7[:, 6], w_mu[:, 6].sum() / N, rtol=1e-13) and np.all(only7[:, :6] == 0)
    # with a diagonal cotangent counted once instead of twice the x coordinate is off by far more than the bound
    wrong = _reverse(_steps(specs, energy), particles, w_mu, w_cov * (1 - 0.5 * np.eye(6)))[0]
    assert np.max(np.abs(wrong - lam)) > 1e-2 * np.max(np.abs(lam))


@pytest.mark.parametrize("name", ["voltage", "phase"])
def test_voltage_and_phase_through_the_kicks_coefficient_cotangents(case, name):
    """
    dL/dV and dL/dphase = sum_s <T_bar_s, dT_s> + <coef_bar, dcoef> with the maps' and coefficients' own derivatives by
    central differences (smooth closed forms), against central differences of the oracle's chain.
    """
    particles, energy, w_mu, w_cov = case
    x0 = {"voltage": 1.2e7, "phase": -8.0}[name]
    specs = _lattice()
    steps = _steps(specs, energy)
    _, tbars, cbars = _reverse(steps, particles, w_mu, w_cov)
    h = 1e-6 * abs(x0)
    up, down = _steps(_lattice(**{name: x0 + h}), energy), _steps(_lattice(**{name: x0 - h}), energy)
    got = 0.0
    for s in range(len(steps)):
        got += np.sum(tbars[s] * (up[s][0] - down[s][0]) / (2 * h))
        if cbars[s] is not None:
            dcoef = (up[s][1] - down[s][1]) / (2 * h)
            got += np.sum(cbars[s] * dcoef)  # (the slot of cos(phi) is zero: the phase's cotangent is complete)
    ref = (_chain_loss(_lattice(**{name: x0 + h}), particles, energy, w_mu, w_cov)
           - _chain_loss(_lattice(**{name: x0 - h}), particles, energy, w_mu, w_cov)) / (2 * h)
    assert abs(got - ref) <= 2e-4 * abs(ref), (name, got, ref)
