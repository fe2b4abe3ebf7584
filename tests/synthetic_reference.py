"""
`k_fill_gaussian` (lynx_amd/csrc/lynx_device.hpp) restated in numpy: what `ParticleBeam.synthetic` must produce.

Scalar `idx` of the flat [B][N][7] array is column c = idx % 7 of a particle.  Column 6 is 1.  Any other column is
mu[c] + sigma[c] * z, with

    h1, h2 = splitmix64(seed ^ splitmix64(2 idx)), splitmix64(seed ^ splitmix64(2 idx + 1))      (uint64, wrapping)
    u1 = (float64(h1 >> 11) + 1) * (1 / 9007199254740993.0)        the literal rounds to 2^53: u1 in (0, 1]
    u2 = float64(h2 >> 11) * (1 / 9007199254740992.0)              u2 in [0, 1)
    r  = sqrt(-2 ln u1),   z = r cos(6.283185307179586 u2)         all in float64

Every step but `log` and `cos` is exact or correctly rounded on both sides, so the kernel may differ from this by the
error of those two functions alone (tests/test_gpu_synthetic.py says by how much).
"""

import numpy as np

_U64 = np.uint64


def splitmix64(x):
    """One step of splitmix64 on a uint64 array (arithmetic modulo 2^64)."""
    x = np.asarray(x, dtype=_U64)
    with np.errstate(over="ignore"):
        x = x + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
    return x ^ (x >> _U64(31))


def fill_gaussian_reference(batch, n, mu, sigma, seed):
    """
    (particles, r): both float64 of shape (*batch, n, 7).  `particles` is the beam of
    `ParticleBeam.synthetic(batch, n, mu, sigma, seed=seed, dtype=float64)` before its final rounding to the dtype;
    `r` is sqrt(-2 ln u1) of every scalar (0 in column 6), the scale of the error bound.
    """
    batch = tuple(batch)
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    assert mu.shape == sigma.shape == (6,)
    total = int(np.prod(batch, dtype=np.int64)) * n * 7
    idx = np.arange(total, dtype=_U64)
    seed = _U64(int(seed) % (1 << 64))
    h1 = splitmix64(seed ^ splitmix64(idx * _U64(2)))
    h2 = splitmix64(seed ^ splitmix64(idx * _U64(2) + _U64(1)))
    u1 = ((h1 >> _U64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = (h2 >> _U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    r = np.sqrt(-2.0 * np.log(u1)).reshape(*batch, n, 7)
    z = r * np.cos(6.283185307179586 * u2).reshape(*batch, n, 7)
    particles = np.ones((*batch, n, 7), dtype=np.float64)
    particles[..., :6] = mu + sigma * z[..., :6]
    r[..., 6] = 0.0
    return particles, r
