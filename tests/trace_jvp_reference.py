"""
A NumPy restatement of the forward-mode sweep of the beam trace (lynx_amd/csrc/lynx_trace_jvp.hpp), tests only:

    mu_dot[0] = 0, C_dot[0] = 0
    for k = 1 .. S:
      Mdot = sum over the direction's entries at element k - 1 of weight . dM_{k-1}/d(parameter or energy)
      mu_dot[k] = M mu_dot[k-1] + Mdot mu[k-1]
      C_dot[k]  = M C_dot[k-1] M^T + X + X^T,   X = Mdot C[k-1] M^T

with M the oracle's element maps and dM by CENTRAL DIFFERENCES of them -- and, beside it, the tangents by central differences
of the oracle's `element_track` chain itself, which is what both the restatement and the kernels are held to.  This module
holds no test and needs no GPU.

A direction is a list of entries (leaf, name, component or None, weight); name "energy" stands for the energy at that step.
Every sample's parameter is moved at once: the samples do not see each other.
"""

import numpy as np

from oracle import lynx_oracle as o

STEP = 1e-6  # relative; the finite-difference tests' `h = 1e-6 max(|x|, 1e-2)`
# A difference quotient's own rounding error: the two chains it subtracts each carry a few units of float64 rounding per map
# applied -- 8 eps is the allowance for the lattices of these tests (up to 12 elements; a product of k maps is good to about
# k eps / 2 on average) -- so the quotient is off by up to 2 . 8 eps max |value| / 2 h, whatever the size of the derivative.
ROUNDING = 8 * np.finfo(np.float64).eps


def steps_of(values):
    return STEP * np.maximum(np.abs(values), 1e-2)


class moved:
    """`with moved(spec, name, component, delta):` -- the parameter array of an oracle spec shifted in place, put back on exit."""

    def __init__(self, spec, name, component, delta):
        self.array, self.delta = spec[name], delta
        self.index = (Ellipsis,) if component is None else (Ellipsis, component)

    def __enter__(self):
        self.kept = self.array[self.index].copy()
        self.array[self.index] = self.kept + self.delta

    def __exit__(self, *exc):
        self.array[self.index] = self.kept


def tangent_map(spec, energy, name, component=None):
    """dM/d(parameter) (B, 7, 7) of one oracle element by central differences; name "energy": dM/d(energy)."""
    energy = np.asarray(energy, dtype=np.float64)
    if name == "energy":
        h = STEP * energy
        up = o.element_transfer_map(spec, energy + h, np.float64)
        down = o.element_transfer_map(spec, energy - h, np.float64)
    else:
        values = spec[name] if component is None else spec[name][..., component]
        h = steps_of(values)
        with moved(spec, name, component, h):
            up = o.element_transfer_map(spec, energy, np.float64)
        with moved(spec, name, component, -h):
            down = o.element_transfer_map(spec, energy, np.float64)
    return (up - down) / (2 * h)[..., None, None]


def sweep(specs, energy, mu0, cov0, direction):
    """The recursion above -> (mu (B, P, 7), cov (B, P, 7, 7), mu_dot, cov_dot) in float64."""
    mu, cov = [np.asarray(mu0, dtype=np.float64)], [np.asarray(cov0, dtype=np.float64)]
    mu_dot, cov_dot = [np.zeros_like(mu[0])], [np.zeros_like(cov[0])]
    T = lambda a: np.swapaxes(a, -1, -2)  # noqa: E731
    for k, spec in enumerate(specs):
        M = o.element_transfer_map(spec, np.asarray(energy, dtype=np.float64), np.float64)
        md = np.einsum("bij,bj->bi", M, mu_dot[-1])
        cd = M @ cov_dot[-1] @ T(M)
        here = [entry for entry in direction if entry[0] == k]
        if here:  # (a step without an entry takes no Mdot term at all)
            Mdot = sum(weight * tangent_map(spec, energy, name, component) for _, name, component, weight in here)
            md = md + np.einsum("bij,bj->bi", Mdot, mu[-1])
            X = Mdot @ cov[-1] @ T(M)
            cd = cd + X + T(X)
        mu.append(np.einsum("bij,bj->bi", M, mu[-1]))
        cov.append(M @ cov[-1] @ T(M))
        mu_dot.append(md)
        cov_dot.append(cd)
    return tuple(np.stack(a, axis=1) for a in (mu, cov, mu_dot, cov_dot))


def chain(specs, beam):
    beams = [beam]
    for spec in specs:
        beams.append(o.element_track(spec, beams[-1], np.float64))
    return beams


def parameter_moments(beams):
    """(mu (B, P, 7), cov (B, P, 7, 7)) of a chain of oracle ParameterBeams."""
    return np.stack([b["mu"] for b in beams], axis=1), np.stack([b["cov"] for b in beams], axis=1)


def particle_moments(beams):
    """... of a chain of oracle ParticleBeams: the mean and the BIASED covariance of the particles in float64, 7 wide."""
    mus, covs = [], []
    for b in beams:
        Q = np.asarray(b["particles"], dtype=np.float64)
        mean = Q.mean(axis=-2)
        d = Q - mean[..., None, :]
        mus.append(mean)
        covs.append(np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2])
    return np.stack(mus, axis=1), np.stack(covs, axis=1)


def chain_tangents(specs, make_beam, moments, energy, direction):
    """
    Central differences of the oracle's element-by-element chain along one direction: every entry's parameter moved by
    t . weight . its own step -> (mu_dot (B, P, 7), cov_dot (B, P, 7, 7), and per sample the rounding error of each of the two
    quotients, (B,) each: `ROUNDING` max |value| / h).  `make_beam(energy)` makes the incoming oracle beam,
    `moments` is `parameter_moments` or `particle_moments`.  A direction's entries share ONE parameter t: the steps of all
    of them scale with the first entry's.
    """
    energy = np.asarray(energy, dtype=np.float64)
    first = direction[0]
    if first[1] == "energy":
        h = STEP * energy
    else:
        values = specs[first[0]][first[1]]
        h = steps_of(values if first[2] is None else values[..., first[2]])

    def at(sign):
        shifts, e = [], energy
        for leaf, name, component, weight in direction:
            if name == "energy":
                e = energy + sign * h  # (one incoming energy: every leaf's entry is this one shift)
            else:
                shifts.append(moved(specs[leaf], name, component, sign * weight * h))
        done = []
        for k, shift in enumerate(shifts):  # (an element object placed several times: its array is moved once per place)
            if any(shift.array is other.array and shift.index == other.index for other in shifts[:k]):
                continue
            shift.__enter__()
            done.append(shift)
        try:
            return moments(chain(specs, make_beam(e)))
        finally:
            for shift in reversed(done):
                shift.__exit__()

    (mu_up, cov_up), (mu_down, cov_down) = at(+1.0), at(-1.0)
    noise = lambda values: ROUNDING * np.max(np.abs(values).reshape(len(h), -1), axis=1) / h  # noqa: E731
    return ((mu_up - mu_down) / (2 * h)[:, None, None], (cov_up - cov_down) / (2 * h)[:, None, None, None],
            noise(mu_up[..., :6]), noise(cov_up))


def distance(got, ref, noise=None):
    """
    max |g - r| / (|r| + 1e-3 max |r|), the maximum taken per sample over one direction's whole array: an
    entry a thousand times smaller than the array's largest is measured against that largest one.  `noise` (B,): what of
    |g - r| is the reference's own rounding error (`chain_tangents`), taken off before the quotient -- it is absolute, eps
    |value| / h, and does not shrink with the derivative: where the derivative is 1e-6 of the value over the step it is
    all there is to see.
    """
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    per_sample = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, *([1] * (ref.ndim - 1)))  # noqa: E731
    top = per_sample(np.max(np.abs(ref).reshape(ref.shape[0], -1), axis=1))
    off = np.abs(got - ref) if noise is None else np.maximum(np.abs(got - ref) - per_sample(noise), 0.0)
    return float(np.max(off / (np.abs(ref) + 1e-3 * top + 1e-300)))
