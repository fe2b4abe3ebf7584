"""
`k_fill_gaussian_rows` and `k_transform_particles` (lynx_amd/csrc/lynx_device.hpp) restated in numpy.

The normals are those of tests/synthetic_reference.py: `fill_gaussian_reference` with mu = 0 and sigma = 1 returns
0 + 1 * z = z itself (both steps exact) and r = sqrt(-2 ln u1) of every scalar, so nothing of the generator is
repeated here.  Column c < 6 of a particle of sample b, with that sample's row (m[0..5], then L00, L10, L11, L20, ... L55):

    s = L[c][0] z_0;   s = s + L[c][j] z_j  for j = 1 ... c;   x_c = m[c] + s          (float64, in this order)

and column 6 is 1.  The rescale is, in the beam's dtype and in this order,

    out[c] = (in[c] - old_mu[c]) / old_sigma[c] * new_sigma[c] + new_mu[c]              (c < 6; column 6 is 1)

with rows (old_mu[6], old_sigma[6], new_sigma[6], new_mu[6]).
"""

import numpy as np

from .synthetic_reference import fill_gaussian_reference

TRIL = np.tril_indices(6)  # the order of the factor inside a row


def rows_of(mean, factor):
    """(B, 27) rows from means (B, 6) and lower-triangular factors (B, 6, 6)."""
    mean, factor = np.asarray(mean, dtype=np.float64), np.asarray(factor, dtype=np.float64)
    return np.concatenate([mean.reshape(-1, 6), factor.reshape(-1, 6, 6)[:, TRIL[0], TRIL[1]]], axis=-1)


def fill_gaussian_rows_reference(batch, n, rows, seed):
    """
    (particles, scale): float64 of shapes (*batch, n, 7) and (*batch, n, 6).  `particles` is the beam before its final
    rounding to the dtype; `scale` is |m_c| + sum_{j <= c} |L_cj| r_j, what the error bound of the float64 kernel is a
    multiple of.
    """
    batch = tuple(batch)
    rows = np.asarray(rows, dtype=np.float64).reshape(*batch, 27)
    z, r = fill_gaussian_reference(batch, n, np.zeros(6), np.ones(6), seed)
    particles = np.ones((*batch, n, 7), dtype=np.float64)
    scale = np.empty((*batch, n, 6), dtype=np.float64)
    k = 6
    for c in range(6):
        L = rows[..., None, k:k + c + 1]  # L[c][0..c], one per sample
        k += c + 1
        s = L[..., 0] * z[..., 0]
        for j in range(1, c + 1):
            s = s + L[..., j] * z[..., j]
        particles[..., c] = rows[..., None, c] + s
        scale[..., c] = np.abs(rows[..., None, c]) + np.sum(np.abs(L) * r[..., :c + 1], axis=-1)
    return particles, scale


def transform_reference(particles, rows):
    """`particles` (*batch, n, 7) rescaled with `rows` (*batch, 24), all in the dtype of `particles`."""
    particles = np.asarray(particles)
    rows = np.asarray(rows, dtype=particles.dtype)[..., None, :]
    out = np.ones_like(particles)
    with np.errstate(all="ignore"):
        out[..., :6] = (particles[..., :6] - rows[..., 0:6]) / rows[..., 6:12] * rows[..., 12:18] + rows[..., 18:24]
    return out
