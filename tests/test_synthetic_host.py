"""
The formula of `ParticleBeam.synthetic` (tests/synthetic_reference.py: splitmix64 counter -> Box-Muller) is a sound
Gaussian generator.  tests/test_gpu_synthetic.py shows that the kernel IS this formula; here the formula itself is held,
per seed, to 5 standard errors in every first- to fourth-order statistic that a tracking test could be sensitive to,
and to a Kolmogorov-Smirnov distance of 2 / sqrt(N).

With 5 seeds x 3 samples x 6 coordinates (and 15 correlations each) about 700 statistics are looked at; a sound generator
exceeds 5 standard errors in one of them with probability 700 x 5.7e-7 = 4e-4, and sqrt(N) D_KS > 2.0 in one of 90 series
with probability 90 x 2 exp(-8) = 0.06 if the seeds were drawn anew -- they are fixed, and the largest values seen
with them are 3.8 standard errors and 1.64.
"""

import math

import numpy as np
import pytest

from .synthetic_reference import fill_gaussian_reference, splitmix64

B, N = 3, 100_000
SEEDS = [0, 1, 2, 3, 2**63 + 5]
ZERO, ONE = np.zeros(6), np.ones(6)


@pytest.fixture(scope="module")
def draws():
    """seed -> (B, N, 6) float64 unit normals of the restatement; made once, read by every test."""
    out = {}
    for seed in SEEDS:
        P, _ = fill_gaussian_reference((B,), N, ZERO, ONE, seed)
        assert np.all(P[..., 6] == 1.0)
        z = P[..., :6]
        z.setflags(write=False)
        out[seed] = z
    return out


def correlation(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def ks_distance(x):
    """sup |F_n - Phi| of a sample against the standard normal distribution."""
    x = np.sort(x)
    n = len(x)
    cdf = 0.5 * (1.0 + np.fromiter(map(math.erf, x / math.sqrt(2.0)), dtype=np.float64, count=n))
    k = np.arange(n)
    return float(max(np.max((k + 1) / n - cdf), np.max(cdf - k / n)))


def test_splitmix64_known_answers():
    """The published test vector of splitmix64: the first outputs of the generator seeded with 1234567."""
    state = np.uint64(1234567) + np.arange(3, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    assert [int(v) for v in splitmix64(state)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]


@pytest.mark.parametrize("seed", SEEDS)
def test_moments_of_every_coordinate(draws, seed):
    z = draws[seed]
    mean, std = z.mean(axis=1), z.std(axis=1)
    c = z - mean[:, None, :]
    skew = (c**3).mean(axis=1) / std**3
    kurt = (c**4).mean(axis=1) / std**4 - 3.0
    stats = {"mean": mean * math.sqrt(N), "std": (std - 1.0) * math.sqrt(2 * N), "skewness": skew * math.sqrt(N / 6),
             "excess kurtosis": kurt * math.sqrt(N / 24)}
    for name, value in stats.items():
        print(f"seed {seed}: {name}: max {np.abs(value).max():.2f} standard errors")
        assert np.all(np.abs(value) < 5.0), (name, value)


@pytest.mark.parametrize("seed", SEEDS)
def test_coordinates_samples_and_neighbours_are_uncorrelated(draws, seed):
    z = draws[seed]
    worst = {"coordinates": 0.0, "samples": 0.0, "lag 1": 0.0}
    for b in range(B):
        rho = np.corrcoef(z[b].T)
        worst["coordinates"] = max(worst["coordinates"], float(np.abs(rho[~np.eye(6, dtype=bool)]).max()))
        for c in range(6):
            worst["samples"] = max(worst["samples"], abs(correlation(z[b, :, c], z[(b + 1) % B, :, c])))
            worst["lag 1"] = max(worst["lag 1"], abs(correlation(z[b, :-1, c], z[b, 1:, c])))
    for name, value in worst.items():
        print(f"seed {seed}: correlation between {name}: {value * math.sqrt(N):.2f} standard errors")
        assert value * math.sqrt(N) < 5.0, (name, value)


@pytest.mark.parametrize("seed", SEEDS)
def test_kolmogorov_smirnov_distance_to_the_normal_distribution(draws, seed):
    z = draws[seed]
    worst = max(ks_distance(z[b, :, c]) for b in range(B) for c in range(6)) * math.sqrt(N)
    print(f"seed {seed}: sqrt(N) D_KS = {worst:.2f}")
    assert worst < 2.0


def test_two_seeds_share_no_value(draws):
    for first, second in zip(SEEDS[:-1], SEEDS[1:]):
        a, b = draws[first].reshape(-1), draws[second].reshape(-1)
        assert len(np.intersect1d(a, b)) == 0 and not np.any(a == b)
    assert len(np.unique(draws[0].reshape(-1))) == B * N * 6  # ... and a seed repeats none of its own


def test_mu_and_sigma_act_affinely_per_column():
    mu = np.array([1e-3, -2e-4, 3e-5, 0.0, 7.0, -1e-6])
    sigma = np.array([1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 2.0])
    unit, r_unit = fill_gaussian_reference((2,), 1000, ZERO, ONE, seed=5)
    P, r = fill_gaussian_reference((2,), 1000, mu, sigma, seed=5)
    assert np.array_equal(r, r_unit) and np.all(r[..., 6] == 0) and np.all(r[..., :6] >= 0)
    assert np.array_equal(P[..., :6], mu + sigma * unit[..., :6]) and np.all(P[..., 6] == 1.0)
    assert np.all(np.abs(unit[..., :6]) <= r[..., :6])  # |z| = r |cos| <= r: the scale of the GPU test's bound
    # one column's mu and sigma move that column alone
    only = fill_gaussian_reference((2,), 1000, mu * (np.arange(6) == 2), np.where(np.arange(6) == 2, sigma, 1.0), seed=5)[0]
    assert np.array_equal(only[..., 2], P[..., 2]) and np.array_equal(np.delete(only, 2, axis=-1), np.delete(unit, 2, axis=-1))
