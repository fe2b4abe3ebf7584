"""
`lynx_amd.grad.track_along_vjp` without a GPU: the cotangent rules of every property of a `BeamTrace` against central
differences of the property itself (float64 NumPy on both sides), the two C entry points being declared, and the
refusals, which are raised before anything touches the GPU.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

ROOT = Path(__file__).resolve().parent.parent

PROPERTIES = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
              "sigma_p", "sigma_xxp", "sigma_yyp", "emittance_x", "emittance_y", "normalized_emittance_x",
              "normalized_emittance_y", "beta_x", "beta_y", "alpha_x", "alpha_y")
BATCH, POINTS = 3, 5
STEP = 1e-6  # relative; the truncation term of the central difference is ~ STEP^2


def _tri(i, j):
    return 7 + i * 6 - (i * (i - 1)) // 2 + (j - i)


def _random_moments(rng):
    """Random means, positive-definite covariances (the scales of a beam) and energies, (BATCH, POINTS, ...)."""
    A = rng.normal(size=(BATCH, POINTS, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]
    cov = A @ np.swapaxes(A, -1, -2)
    mu = rng.normal(size=(BATCH, POINTS, 6)) * [1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3]
    energy = rng.uniform(5e6, 2e8, size=(BATCH, POINTS))
    return mu, cov, energy


def _direction(rng, x):
    """A perturbation of the size of `x` itself, entry by entry (a relative step keeps a covariance positive definite)."""
    return x * rng.uniform(0.5, 1.5, size=x.shape) * rng.choice([-1.0, 1.0], size=x.shape)


def _records(mu, cov):
    rec = np.zeros((BATCH, POINTS, 36))
    rec[..., :6] = mu
    rec[..., 6] = 1.0
    for i in range(6):
        for j in range(i, 6):
            rec[..., _tri(i, j)] = cov[..., i, j]
    rec[..., 34] = 1.0
    rec[..., 35] = 1000.0
    return rec


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("kind", ["records", "moments"])
def test_every_property_rule_against_a_central_difference_of_the_property(kind, ddof, monkeypatch):
    from lynx_amd import config, grad
    from lynx_amd.trace import BeamTrace

    monkeypatch.setattr(config, "std_ddof", ddof)
    rng = np.random.default_rng(3 + ddof)
    mu, cov, energy = _random_moments(rng)
    lengths, names = [np.array([0.5])] * (POINTS - 1), [f"e{k}" for k in range(POINTS - 1)]

    def trace_of(mu_, cov_, energy_):
        if kind == "records":
            return BeamTrace.from_records(_records(mu_, cov_), energy_, lengths, names, dtype=np.float64)
        mu7 = np.concatenate([mu_, np.ones((BATCH, POINTS, 1))], axis=-1)
        cov7 = np.zeros((BATCH, POINTS, 7, 7))
        cov7[..., :6, :6] = cov_
        return BeamTrace.from_moments(mu7, cov7, energy_, lengths, names, dtype=np.float64)

    d_mu, d_energy = _direction(rng, mu), _direction(rng, energy)
    d_cov = _direction(rng, cov)
    if kind == "records":  # a record holds the upper triangle: the covariance it stands for stays symmetric
        d_cov = np.triu(d_cov) + np.swapaxes(np.triu(d_cov, 1), -1, -2)
    trace = trace_of(mu, cov, energy)
    up = trace_of(mu + STEP * d_mu, cov + STEP * d_cov, energy + STEP * d_energy)
    down = trace_of(mu - STEP * d_mu, cov - STEP * d_cov, energy - STEP * d_energy)
    weight = rng.uniform(0.5, 1.5, size=(BATCH, POINTS))
    for name in PROPERTIES + ("energy",):
        mu_bar, cov_bar, energy_bar = grad.trace_property_cotangents(trace, {name: weight})
        assert mu_bar.shape == (BATCH, POINTS, 7) and cov_bar.shape == (BATCH, POINTS, 7, 7) and energy_bar.shape == (BATCH, POINTS)
        got = (np.sum(mu_bar[..., :6] * d_mu, axis=-1) + np.sum(cov_bar[..., :6, :6] * d_cov, axis=(-1, -2))
               + energy_bar * d_energy)
        assert not np.any(mu_bar[..., 6]) and not np.any(cov_bar[..., 6, :]) and not np.any(cov_bar[..., :, 6])
        ref = weight * (np.asarray(getattr(up, name), dtype=np.float64) - np.asarray(getattr(down, name), dtype=np.float64)) / (2 * STEP)
        assert np.all(ref != 0), name
        assert np.allclose(got, ref, rtol=1e-6, atol=0.0), (name, np.max(np.abs(got / ref - 1)))


def test_a_scalar_cotangent_is_the_same_weight_at_every_point_and_rules_add_up():
    from lynx_amd import grad
    from lynx_amd.trace import BeamTrace

    mu, cov, energy = _random_moments(np.random.default_rng(8))
    trace = BeamTrace.from_records(_records(mu, cov), energy, [None] * (POINTS - 1), ["m"] * (POINTS - 1), dtype=np.float64)
    one = grad.trace_property_cotangents(trace, {"beta_x": 2.0})
    full = grad.trace_property_cotangents(trace, {"beta_x": np.full((BATCH, POINTS), 2.0)})
    assert all(np.array_equal(a, b) for a, b in zip(one, full))
    both = grad.trace_property_cotangents(trace, {"beta_x": 2.0, "alpha_y": -1.0, "energy": 3.0})
    alpha = grad.trace_property_cotangents(trace, {"alpha_y": -1.0})
    assert np.allclose(both[1], one[1] + alpha[1], rtol=1e-13, atol=0.0) and np.all(both[2] == 3.0)
    with pytest.raises(KeyError, match="sigma_q"):
        grad.trace_property_cotangents(trace, {"sigma_q": 1.0})


def test_a_clamped_variance_of_a_parameter_beam_trace_has_no_derivative():
    from lynx_amd import grad
    from lynx_amd.trace import BeamTrace

    mu, cov, energy = _random_moments(np.random.default_rng(9))
    cov7 = np.zeros((BATCH, POINTS, 7, 7))
    cov7[..., :6, :6] = cov
    cov7[0, 2, 0, 0] = 1e-24  # below the floor of ParameterBeam._sigma: sigma_x = 1e-10 whatever the entry
    mu7 = np.concatenate([mu, np.ones((BATCH, POINTS, 1))], axis=-1)
    trace = BeamTrace.from_moments(mu7, cov7, energy, [None] * (POINTS - 1), ["m"] * (POINTS - 1), dtype=np.float64)
    assert trace.sigma_x[0, 2] == 1e-10
    _, cov_bar, _ = grad.trace_property_cotangents(trace, {"sigma_x": 1.0})
    assert cov_bar[0, 2, 0, 0] == 0.0 and np.all(cov_bar[1:, :, 0, 0] > 0)


def test_both_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for name in ("lynx_track_moments_along_backward", "lynx_track_particles_along_backward"):
        assert name in _ffi.SIGNATURES
        assert f"int {name}(" in header
    assert len(_ffi.SIGNATURES["lynx_track_moments_along_backward"][1]) == 12
    assert len(_ffi.SIGNATURES["lynx_track_particles_along_backward"][1]) == 11


def test_refusals_are_raised_before_any_gpu_call(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine, grad

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along_vjp touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    # an active Screen or Aperture: `trace_program` names it
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Segment([lx.Screen(is_active=True, name="SCR7")]), lx.Drift(f(1.0))])
    with pytest.raises(NotImplementedError, match="SCR7"):
        grad.track_along_vjp(segment, particles)
    with pytest.raises(NotImplementedError, match="AP1"):
        grad.track_along_vjp(lx.Segment([lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=True, name="AP1")]), particles)
    # a ParticleBeam through an active cavity: the moments are not closed under the kick
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
    with pytest.raises(NotImplementedError, match="ACC1"):
        grad.track_along_vjp(lx.Segment([lx.Drift(f(1.0)), cavity]), particles)
    # more than 256 leaves, nested segments opened up
    long = lx.Segment([lx.Segment([lx.Drift(f(0.1), name=f"D{k}") for k in range(200)]),
                       lx.Segment([lx.Drift(f(0.1), name=f"T{k}") for k in range(57)])])
    with pytest.raises(NotImplementedError, match="257 leaf elements.*'T56'"):
        grad.track_along_vjp(long, particles)
    # `resolution=` is not offered: the leaves of a split lattice are not the user's elements
    with pytest.raises(TypeError):
        grad.track_along_vjp(lx.Segment([lx.Drift(f(1.0))]), particles, resolution=0.1)
    with pytest.raises(TypeError, match="ParticleBeam or a ParameterBeam"):
        grad.track_along_vjp(lx.Segment([lx.Drift(f(1.0))]), None)
