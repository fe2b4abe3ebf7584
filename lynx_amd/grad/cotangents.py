"""
Cotangents on the host, pure NumPy: the rules that turn cotangents of named beam properties into cotangents of mean,
covariance and energy (`_walk_properties`, `property_cotangents`, `trace_property_cotangents`), their assembly in the order
they came (`_MomentCotangents`), the readings of BPMs, the packing into moment records (`_record_cotangents`), and the one
batch rule (`batch_size`, `over_batch`).  Nothing here knows the runtime.
"""

from __future__ import annotations

import math

import numpy as np

from .. import _ffi, config
from ..particles.beam import ELECTRON_MASS_EV
from ..particles.particle_beam import ParticleBeam, _tri
from ..trace import ParticleBeamTrace

_COORDINATES = ("x", "xp", "y", "yp", "s", "p")
# the properties a moment target may name, in the order of their codes: bit k of a point's mask in lynx_moments_along_loss
MOMENT_PROPERTIES = (*("mu_" + c for c in _COORDINATES), *("sigma_" + c for c in _COORDINATES), "sigma_xxp", "sigma_yyp",
                     "emittance_x", "emittance_y", "normalized_emittance_x", "normalized_emittance_y", "beta_x", "beta_y",
                     "alpha_x", "alpha_y", "energy")
_ENERGY_PROPERTIES = ("normalized_emittance_x", "normalized_emittance_y", "energy")  # what adds into the energy's cotangent


def batch_size(batch_shape) -> int:
    """The samples of a batch: B of every `[B]...` array a library call takes."""
    return int(np.prod(batch_shape, dtype=np.int64))


def broadcast_or_refuse(value: np.ndarray, shape, what: str, to: str) -> np.ndarray:
    """`value` broadcast to `shape`, or the ValueError every cotangent and target that does not fit is refused with."""
    try:
        return np.broadcast_to(value, shape)
    except ValueError:
        raise ValueError(f"track_along_vjp: {what} has shape {value.shape}, which does not broadcast to {to}") from None


def over_batch(value, batch_shape, what: str) -> np.ndarray:
    """`value` (a scalar, or whatever broadcasts to the batch) as (B,) float64 of its own; refused by value, naming `what`."""
    batch_shape = tuple(batch_shape)
    spread = broadcast_or_refuse(np.asarray(value, dtype=np.float64), batch_shape, what, f"the batch {batch_shape}")
    return np.ascontiguousarray(spread).reshape(-1)


def _walk_properties(named: dict, shape, what: str, per_plane=(), whole=()):
    """
    The one walk over `{property name: cotangent}` of the three rule functions: each cotangent broadcast to `shape` as
    float64, as ("mu" | "sigma", coordinate, bar) for `mu_<c>` and `sigma_<c>`, ("cross", 0 | 2, bar) for `sigma_xxp` and
    `sigma_yyp`, (name, 0 | 2, bar) for `<name>_x`, `<name>_y` of a name in `per_plane`, (name, None, bar) for one in `whole`.
    """
    for name, bar in named.items():
        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), shape)
        kind, _, coord = name.partition("_")
        head, _, plane = name.rpartition("_")
        if kind in ("mu", "sigma") and coord in _COORDINATES:
            yield kind, _COORDINATES.index(coord), bar
        elif name in ("sigma_xxp", "sigma_yyp"):
            yield "cross", 0 if name == "sigma_xxp" else 2, bar
        elif head in per_plane and plane in ("x", "y"):
            yield head, 0 if plane == "x" else 2, bar
        elif name in whole:
            yield name, None, bar
        else:
            raise KeyError(f"no cotangent rule for {what} property {name!r}")


def property_cotangents(outgoing, named: dict):
    """
    Cotangents of named beam properties -> (mu_bar, cov_bar).  `mu_<c>`: the mean itself;
    `sigma_<c>` = sqrt(cov_cc n / (n - ddof)) (particle_beam.py:736-823, `config.std_ddof`), so
    d sigma / d cov_cc = n / (n - ddof) / (2 sigma); `sigma_xxp`, `sigma_yyp`: cov_01, cov_23.
    Of a ParameterBeam, 7 wide: `sigma_<c>` = sqrt(max(cov_cc, 1e-20)) (parameter_beam.py:371-417), 0 where clamped.
    """
    particles = isinstance(outgoing, ParticleBeam)
    batch, width = outgoing.batch_shape, 6 if particles else 7
    mu_bar, cov_bar = np.zeros((*batch, width)), np.zeros((*batch, width, width))
    for kind, c, bar in _walk_properties(named, batch, "beam"):
        if kind == "mu":
            mu_bar[..., c] += bar
        elif kind == "cross":
            cov_bar[..., c, c + 1] += bar
        elif particles:  # (by the beam's own property, in the beam's dtype)
            n, sigma = float(outgoing.num_particles), np.asarray(getattr(outgoing, "sigma_" + _COORDINATES[c]), dtype=np.float64)
            cov_bar[..., c, c] += bar * (n / (n - config.std_ddof)) / (2.0 * sigma)
        else:
            var = np.asarray(outgoing._cov, dtype=np.float64)[..., c, c]
            cov_bar[..., c, c] += np.where(var > 1e-20, bar / (2.0 * np.sqrt(np.maximum(var, 1e-20))), 0.0)
    return mu_bar, cov_bar


class _MomentCotangents:
    """
    What every reverse pass assembles first: the cotangents of mean and covariance, entry by entry, as float64 terms (*lead, k)
    and (*lead, k, k) in the order they came -- `lead` = (B,) behind a lattice, (B, P) for a trace.  Behind a lattice a cotangent
    is whatever `reshape` takes for the flattened batch (`cov_width`: k where the caller fixes it), for a trace whatever
    broadcasts to (*batch, P, k): the rules of `track_vjp` and of `track_along_vjp`.
    """

    def __init__(self, batch_shape, points: int | None = None, cov_width: int | None = None):
        self.batch_shape, self.cov_width, self.means, self.covariances = tuple(batch_shape), cov_width, [], []
        self.lead = (math.prod(self.batch_shape), *(() if points is None else (points,)))

    def _term(self, bar: np.ndarray, *tail) -> np.ndarray:
        if len(self.lead) == 1:
            return bar.reshape(*self.lead, *tail)
        return np.broadcast_to(bar, (*self.batch_shape, *self.lead[1:], *tail)).reshape(*self.lead, *tail)

    def add(self, mu_bar=None, cov_bar=None):  # (`cov_bar` not necessarily symmetric; None: no such cotangent)
        if mu_bar is not None:
            mu_bar = np.asarray(mu_bar, dtype=np.float64)
            self.means.append(self._term(mu_bar, -1 if len(self.lead) == 1 else mu_bar.shape[-1]))
        if cov_bar is not None:
            cov_bar = np.asarray(cov_bar, dtype=np.float64)
            k = self.cov_width or cov_bar.shape[-1]
            self.covariances.append(self._term(cov_bar, k, k))

    def summed(self):
        """(mb (*lead, 7), cb (*lead, 7, 7)), the caller's own: every term added into zeros, in the order it came."""
        mb, cb = np.zeros((*self.lead, 7)), np.zeros((*self.lead, 7, 7))
        for term in self.means:
            mb[..., : term.shape[-1]] += term
        for term in self.covariances:
            cb[..., : term.shape[-1], : term.shape[-1]] += term
        return mb, cb

    def chained(self):  # (mean's, covariance's): one term to the next, None for none; a single one AS IT CAME -- no copy, no `-0.0` lost
        return tuple(sum(terms[1:], terms[0]) if terms else None for terms in (self.means, self.covariances))


def _known_bpm(element, known: bool):
    if not known:
        raise KeyError(f"{element!r} is not an active BPM of this lattice")


def _reading_bar(bar, batch_shape) -> np.ndarray:  # (2, B): a BPM reads `stack([mu_x, mu_y])` of the beam entering it (bpm.py:48-54)
    return np.broadcast_to(np.asarray(bar, dtype=np.float64), (2, *batch_shape)).reshape(2, -1)


def _add_reading(mb: np.ndarray, bar, batch_shape, *point):  # ... into the mean's cotangent, at `point` of a trace
    bar = _reading_bar(bar, batch_shape)
    mb[(slice(None), *point, 0)] += bar[0]
    mb[(slice(None), *point, 2)] += bar[1]


_TRIANGLE = [(7 + n, int(i), int(j)) for n, (i, j) in enumerate(zip(*np.triu_indices(6)))]  # (slot of a record, i, j): `_tri`


def _record_cotangents(lead: tuple, mb, cb) -> np.ndarray:
    """
    Cotangents of mean (*lead, k) and covariance (*lead, 6|7, 6|7), entry by entry (None: none), as record cotangents
    (*lead, 36): [0..k) the mean's, [7..27] the upper triangle in `_tri`'s order, an off-diagonal entry counted once.  The only
    place that packs records -- slot by slot: at a batch of thousands a gather of the triangle costs three times as much (it
    wrote (G + G) * 0.5 on the diagonal: the bits of G for every finite G below half the largest float64).
    """
    rec = np.zeros((*lead, _ffi.MOMENT_STRIDE), dtype=np.float64)
    if mb is not None:
        rec[..., : mb.shape[-1]] = mb
    if cb is not None:
        slots, G = rec.reshape(-1, _ffi.MOMENT_STRIDE), cb.reshape(-1, *cb.shape[-2:])  # (views of two and three dimensions: indexed the fastest)
        for slot, i, j in _TRIANGLE:
            slots[:, slot] = G[:, i, i] if i == j else G[:, i, j] + G[:, j, i]
    return rec


def trace_property_cotangents(trace, named: dict):
    """
    Cotangents of named properties of a `BeamTrace`, each (*batch, P) (broadcastable: a scalar is the same weight at
    every point) -> (mu_bar (*batch, P, 7), cov_bar (*batch, P, 7, 7) entry by entry, energy_bar (*batch, P)), float64.
    The formulas are the ones the traces evaluate:
      ParticleBeamTrace   sigma_c = sqrt(cov_cc n / (n - ddof)) (`config.std_ddof`), sigma_xxp = cov_01 as it is;
      ParameterBeamTrace  sigma_c = sqrt(max(cov_cc, 1e-20)): derivative 0 where clamped;
      both                emittance = sqrt(max(sigma^2 sigma_p^2 - sigma_xxp^2, tiny)) (`Beam._emittance`, 0 where
                          clamped), beta = sigma^2 / emittance, alpha = -sigma_xxp / emittance,
                          normalized_emittance = emittance sqrt(gamma^2 - 1) -- which also depends on the energy there.
    """
    shape = (*trace.batch_shape, trace.num_points)
    mu_bar, cov_bar, energy_bar = np.zeros((*shape, 7)), np.zeros((*shape, 7, 7)), np.zeros(shape)
    if isinstance(trace, ParticleBeamTrace):
        rec = np.asarray(trace.records, dtype=np.float64)
        n = rec[..., 35]
        scale = n / (n - config.std_ddof)
        variance = lambda c: rec[..., _tri(c, c)]  # noqa: E731
        cross_of = lambda a: rec[..., _tri(a, a + 1)]  # noqa: E731
        floor = None
    else:
        cov = np.asarray(trace._cov, dtype=np.float64)
        scale = np.ones(shape)
        variance = lambda c: cov[..., c, c]  # noqa: E731
        cross_of = lambda a: cov[..., a, a + 1]  # noqa: E731
        floor = float(trace.dtype.type(1e-20))
    tiny = float(np.finfo(trace.dtype).tiny)

    def sigma_squared(c):
        """sigma_c^2 and its derivative with respect to cov_cc."""
        v = variance(c)
        if floor is None:
            return v * scale, scale
        return np.maximum(v, floor), (v > floor).astype(np.float64)

    # what a plane's properties are written in: s2 = sigma^2, p2 = sigma_p^2, the cross term
    plane_bars = {}

    def plane(a):
        if a not in plane_bars:
            plane_bars[a] = {"s2": np.zeros(shape), "p2": np.zeros(shape), "cross": np.zeros(shape)}
        return plane_bars[a]

    def emittance(a):
        s2, p2, cross = sigma_squared(a)[0], sigma_squared(a + 1)[0], cross_of(a)
        q = s2 * p2 - cross**2
        return np.sqrt(np.maximum(q, tiny)), q > tiny, s2, p2, cross

    def emittance_bar(a, bar):
        eps, free, s2, p2, cross = emittance(a)
        with np.errstate(all="ignore"):
            w = np.where(free, bar / (2.0 * eps), 0.0)
        acc = plane(a)
        acc["s2"] += w * p2
        acc["p2"] += w * s2
        acc["cross"] += -2.0 * w * cross

    for kind, a, bar in _walk_properties(named, shape, "trace", ("emittance", "normalized_emittance", "beta", "alpha"), ("energy",)):
        if kind == "energy":
            energy_bar += bar
        elif kind == "mu":
            mu_bar[..., a] += bar
        elif kind == "sigma":
            s2, ds2 = sigma_squared(a)
            with np.errstate(all="ignore"):
                cov_bar[..., a, a] += np.where(ds2 != 0, bar * ds2 / (2.0 * np.sqrt(s2)), 0.0)
        elif kind == "cross":
            plane(a)["cross"] += bar
        elif kind == "emittance":
            emittance_bar(a, bar)
        elif kind == "normalized_emittance":
            gamma = np.asarray(trace.energy, dtype=np.float64) / ELECTRON_MASS_EV
            moving = np.abs(gamma) > 0
            with np.errstate(all="ignore"):
                bg = np.where(moving, np.sqrt(1 - 1 / gamma**2) * gamma, 0.0)  # relativistic beta . gamma
                dbg = np.where(moving, gamma / np.sqrt(gamma**2 - 1), 0.0) / ELECTRON_MASS_EV
            emittance_bar(a, bar * bg)
            energy_bar += bar * emittance(a)[0] * dbg
        elif kind == "beta":
            eps, _, s2, _, _ = emittance(a)
            plane(a)["s2"] += bar / eps
            emittance_bar(a, -bar * s2 / eps**2)
        else:  # alpha
            eps, _, _, _, cross = emittance(a)
            plane(a)["cross"] += -bar / eps
            emittance_bar(a, bar * cross / eps**2)
    for a, acc in plane_bars.items():
        cov_bar[..., a, a] += acc["s2"] * sigma_squared(a)[1]
        cov_bar[..., a + 1, a + 1] += acc["p2"] * sigma_squared(a + 1)[1]
        cov_bar[..., a, a + 1] += acc["cross"]
    return mu_bar, cov_bar, energy_bar
