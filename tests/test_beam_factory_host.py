"""
The host side of the device beam factory (`ParticleBeam.from_parameters(on_device=True)`, `from_twiss(on_device=True)`,
`from_parameter_beam`, `transformed_to(on_device=True)`); no GPU.

  * `covariance_factor`: L L^T is the covariance, L is lower triangular, singular covariances give a factor and no NaN;
  * the formula of tests/beam_factory_reference.py is a sound generator of correlated beams: means and the whole 6 x 6
    covariance within 5 standard errors at 3 x 100 000 (tests/test_gpu_beam_factory.py shows that the kernel IS the formula);
  * with a diagonal factor the formula is `fill_gaussian_reference` bit for bit: it extends the generator
    tests/test_synthetic_host.py examines and is no second random stream;
  * what is refused is refused before anything touches the device.
"""

import math

import numpy as np
import pytest

from lynx_amd import ParameterBeam, ParticleBeam
from lynx_amd.particles.particle_beam import covariance_factor, gaussian_rows

from .beam_factory_reference import TRIL, fill_gaussian_rows_reference, rows_of
from .synthetic_reference import fill_gaussian_reference

N = 100_000
SEED = 11


def plane(beta, alpha, emittance):
    """(variance of position, variance of angle, covariance) of Twiss values, as `from_twiss` forms them."""
    return beta * emittance, emittance * (1 + alpha**2) / beta, -emittance * alpha


def covariance(x, y, sigma_s, sigma_p, cor_s):
    cov = np.zeros((6, 6))
    for at, (pos, ang, cross) in ((0, x), (2, y)):
        cov[at, at], cov[at + 1, at + 1], cov[at, at + 1], cov[at + 1, at] = pos, ang, cross, cross
    cov[4, 4], cov[5, 5], cov[4, 5], cov[5, 4] = sigma_s**2, sigma_p**2, cor_s, cor_s
    return cov


# the three samples of the generator test: two from Twiss values with alpha != 0 in both planes and cor_s != 0, one
# with an uncorrelated x plane, a y plane that is a line in phase space (cor_y = sigma_y sigma_yp) and sigma_s = 0
COVS = np.stack([
    covariance(plane(61.475, -1.2124, 3.5e-9), plane(74.9, 1.0, 2.3e-9), 1e-5, 2e-3, 0.6 * 1e-5 * 2e-3),
    covariance(plane(5.9, 3.556, 2e-8), plane(0.7, -0.4, 1e-8), 8e-6, 1e-3, -0.9 * 8e-6 * 1e-3),
    covariance((2e-4**2, 3e-5**2, 0.0), (1e-4**2, 2e-5**2, 1e-4 * 2e-5), 0.0, 5e-4, 0.0),
])
MEANS = np.array([[3e-4, -2e-5, -1e-4, 4e-6, 0, 0], [-1e-3, 1e-5, 2e-4, -3e-6, 0, 0], [0, 0, 0, 0, 0, 0.0]])


def coupled_covariance():
    """A full 6 x 6 covariance with x-y coupling (and every other pair): A A^T of a fixed dense matrix, scaled per axis."""
    A = np.random.default_rng(3).standard_normal((6, 6))
    scale = np.array([2e-4, 3e-5, 1e-4, 2e-5, 1e-5, 1e-3])
    return (A @ A.T) * np.outer(scale, scale)


@pytest.mark.parametrize("cov", [*COVS, coupled_covariance()], ids=["twiss-a", "twiss-b", "singular", "coupled"])
def test_the_factor_times_its_transpose_is_the_covariance(cov):
    L = covariance_factor(cov)
    assert L.shape == (6, 6) and L.dtype == np.float64 and np.all(np.isfinite(L))
    assert np.all(L[np.triu_indices(6, 1)] == 0)
    assert np.allclose(L @ L.T, cov, rtol=1e-12, atol=0.0)  # (an entry that is zero is reproduced as zero)


def test_the_factor_of_a_batch_is_the_factor_of_each_sample():
    stacked = covariance_factor(COVS.reshape(3, 1, 6, 6))
    assert stacked.shape == (3, 1, 6, 6)
    for b in range(3):
        assert np.array_equal(stacked[b, 0], covariance_factor(COVS[b]))


def test_singular_covariances_leave_a_zero_column():
    L = covariance_factor(COVS[2])
    assert np.all(L[:, 3] == 0) and np.all(L[:, 4] == 0)  # y' is a multiple of y; s has no spread
    assert L[3, 2] == pytest.approx(2e-5, rel=1e-12) and L[5, 5] == pytest.approx(5e-4, rel=1e-12)


def test_a_diagonal_covariance_gives_the_sigmas_exactly():
    sigma = np.array([1e-4, 1e-7, 1e-3, 1e-5, 1e-6, 3e-4])
    assert np.array_equal(covariance_factor(np.diag(sigma**2)), np.diag(sigma))
    sigma32 = sigma.astype(np.float32).astype(np.float64)  # (what from_parameters squares in float64 for a float32 beam)
    assert np.array_equal(covariance_factor(np.diag(sigma32**2)), np.diag(sigma32))


def test_rows_are_the_mean_and_the_factor_row_by_row():
    rows = gaussian_rows(MEANS, COVS)
    assert rows.shape == (3, 27) and rows.dtype == np.float64 and rows.flags.c_contiguous
    assert np.array_equal(rows[:, :6], MEANS)
    L = covariance_factor(COVS)
    assert np.array_equal(rows[:, 6:9], np.stack([L[:, 0, 0], L[:, 1, 0], L[:, 1, 1]], axis=-1))
    assert np.array_equal(rows, rows_of(MEANS, L)) and rows[0, 26] == L[0, 5, 5]
    assert list(zip(*TRIL))[:4] == [(0, 0), (1, 0), (1, 1), (2, 0)]


def test_the_formula_is_a_sound_generator_of_correlated_beams():
    P, _ = fill_gaussian_rows_reference((3,), N, gaussian_rows(MEANS, COVS), SEED)
    assert np.all(P[..., 6] == 1.0)
    x = P[..., :6]
    mean = x.mean(axis=1)
    c = x - mean[:, None, :]
    got = np.einsum("bni,bnj->bij", c, c) / N
    var = np.einsum("bii->bi", COVS)
    mean_se = np.sqrt(var / N)
    cov_se = np.sqrt((var[:, :, None] * var[:, None, :] + COVS**2) / N)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst_mean = np.nanmax(np.abs(mean - MEANS) / mean_se)
        worst_cov = np.nanmax(np.abs(got - COVS) / cov_se)
    print(f"worst mean {worst_mean:.2f} standard errors, worst covariance entry {worst_cov:.2f}")
    assert np.all(np.abs(mean - MEANS) <= 5.0 * mean_se)  # (a coordinate without spread sits on its mean exactly)
    assert np.all(np.abs(got - COVS) <= 5.0 * cov_se)


@pytest.mark.parametrize("batch,n", [((2, 3), 1000), ((1,), 257)])
def test_with_a_diagonal_factor_the_formula_is_the_old_generator(batch, n):
    mu = np.array([3e-4, -2e-5, -1e-4, 4e-6, 2e-6, 1e-3])
    sigma = np.array([1e-4, 1e-7, 1e-3, 1e-5, 1e-6, 3e-4])
    B = math.prod(batch)
    rows = gaussian_rows(np.tile(mu, (B, 1)), np.tile(np.diag(sigma**2), (B, 1, 1)))
    new, scale = fill_gaussian_rows_reference(batch, n, rows, SEED)
    old, r = fill_gaussian_reference(batch, n, mu, sigma, SEED)
    assert np.array_equal(new, old)
    assert np.array_equal(scale, np.abs(mu) + sigma * r[..., :6])


def host_beam(batch=(1,), n=5, dtype=np.float32):
    particles = np.ones((*batch, n, 7), dtype=dtype)
    particles[..., :6] = np.random.default_rng(0).standard_normal((*batch, n, 6))
    return ParticleBeam(particles, np.full(batch, 1e8), dtype=dtype)


def test_transformed_to_on_device_keeps_the_dtype():
    with pytest.raises(TypeError, match="dtype"):
        host_beam(dtype=np.float32).transformed_to(mu_x=np.zeros(1), dtype=np.float64, on_device=True)
    with pytest.raises(TypeError, match="dtype"):
        host_beam(dtype=np.float64).transformed_to(dtype=np.float32, on_device=True)


def test_arguments_of_the_wrong_shape_are_refused():
    with pytest.raises(AssertionError, match="same shape"):
        host_beam(batch=(2,)).transformed_to(mu_x=np.zeros(3), on_device=True)
    with pytest.raises(AssertionError, match="same shape"):
        host_beam(batch=(2,)).transformed_to(sigma_x=np.ones((2, 1)), energy=np.ones(2), on_device=True)
    with pytest.raises(AssertionError, match="same shape"):
        ParticleBeam.from_parameters(num_particles=10, mu_x=np.zeros(2), sigma_x=np.ones(3), on_device=True)
    with pytest.raises(AssertionError, match="same shape"):
        ParticleBeam.from_twiss(num_particles=10, beta_x=np.ones(2), alpha_x=np.zeros((2, 1)), on_device=True)
    with pytest.raises(AssertionError):
        covariance_factor(np.eye(7))


def test_from_parameter_beam_takes_a_parameter_beam():
    with pytest.raises(AssertionError, match="ParameterBeam"):
        ParticleBeam.from_parameter_beam(host_beam(), 10)
    with pytest.raises(AssertionError, match="ParameterBeam"):
        ParticleBeam.from_parameter_beam(np.zeros((1, 7)), 10)
    with pytest.raises(AssertionError, match="at least one particle"):
        ParticleBeam.from_parameter_beam(ParameterBeam.from_parameters(), 0)
