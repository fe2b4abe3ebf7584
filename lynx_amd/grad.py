"""
Reverse-mode gradients of the outgoing beam's moments with respect to element parameters
(BASELINE config 5).  The reference only claims differentiability
(`setup.py:14-17`; its tests still assert torch `grad_fn`, `tests/test_differentiable.py`) --
there is no `jax.grad` call to mirror, so the API is an explicit vector-Jacobian product:

    vjp = lynx_amd.grad.track_vjp(segment, beam)     # forward pass, fused moments
    out = vjp.outgoing                                # the tracked ParticleBeam
    g = vjp(mu_bar=..., cov_bar=...)                  # cotangents of mean (.., 6) and cov (.., 6, 6)
    g = vjp(mu_x=..., sigma_x=..., sigma_y=...)       # or of the beam properties a loss is written in
    g[segment.Q1]["k1"], g.energy                     # dL/dk1 (shape of k1), dL/dE_in

All arithmetic runs in the HIP kernels of `lynx_amd/csrc/lynx_grad.hpp`
(`lynx_track_particles_backward`).
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _ffi, engine
from .device import get_runtime
from .particles.particle_beam import ParticleBeam, _tri

# kinds whose parameter row is differentiated; the slot names come from the element's schema
DIFFERENTIABLE_KINDS = (_ffi.KIND_DRIFT, _ffi.KIND_QUADRUPOLE, _ffi.KIND_DIPOLE, _ffi.KIND_HCOR, _ffi.KIND_VCOR,
                        _ffi.KIND_CAVITY, _ffi.KIND_SOLENOID, _ffi.KIND_UNDULATOR)


def _unbroadcast(grad: np.ndarray, shape) -> np.ndarray:
    """Sum a batch-shaped gradient down to the shape of a parameter that was broadcast."""
    shape = tuple(shape)
    if grad.shape == shape:
        return grad
    while grad.ndim > len(shape):
        grad = grad.sum(axis=0)
    for ax, n in enumerate(shape):
        if n == 1 and grad.shape[ax] != 1:
            grad = grad.sum(axis=ax, keepdims=True)
    return grad.reshape(shape)


class Gradients:
    """
    dL/d(parameter) per element (`g[element]["k1"]`), `energy` = dL/d(incoming beam energy).
    The raw `[B][E][8]` result stays in HBM; an element's gradients are copied and shaped on
    first access.
    """

    # `moments=` of a pass with no incoming moments to differentiate, `mu` and `cov` are None: the survivors of a trace with
    # losses are no single set of particles, behind a cavity's kick a ParticleBeam's gradient is no function of them
    NO_INCOMING_MOMENTS = (None, None)

    def __init__(self, program, beam, raw_dev, energy_dev, particles=None, moments=None, chosen=None, screens=None, zeros=()):
        # what a pass may have besides `[B][E][8]` and the energy's, on the device: `particles`; `moments` = (mu, cov); `chosen`;
        # `screens` = (the trace's active screens, the parts of dL/d(misalignment), each `[B][screens][2]`: they are added, and
        # none is an exact zero);
        # `zeros`: (element, parameter names) whose gradient is an exact zero
        self._program, self._raw_dev, self._energy_dev = program, raw_dev, energy_dev
        self._particles_dev, self._moments, self._chosen_dev = particles, moments, chosen
        self._screens, self._screen_shifts_dev = ([], []) if screens is None else (list(screens[0]), list(screens[1]))
        self._batch_shape, self._energy_shape = tuple(beam.batch_shape), np.asarray(beam.energy).shape
        self._zeros, self._raw, self._cache = list(zeros), None, {}

    def _host(self):
        if self._raw is None:
            E = max(len(self._program.leaves), 1)
            self._raw = self._raw_dev.numpy().reshape(*self._batch_shape, E, 8)
        return self._raw

    @property
    def energy(self) -> np.ndarray:
        return _unbroadcast(self._energy_dev.numpy().reshape(self._batch_shape), self._energy_shape)

    @property
    def particles(self):
        """dL/d(incoming particles), (*batch, N, 7), device-resident; needs `wrt_particles=True`."""
        if self._particles_dev is None:
            raise KeyError("call the VJP with wrt_particles=True to get the gradient w.r.t. the incoming particles")
        return self._particles_dev

    @property
    def mu(self) -> np.ndarray:
        """
        dL/d(incoming mu), (*batch, 7) -- ParameterBeam VJPs only; None for the survivors of a trace with losses and for a
        ParticleBeam differentiated through cavities.
        """
        if self._moments is None:
            raise KeyError("the gradient w.r.t. mu exists for ParameterBeam VJPs only")
        return None if self._moments[0] is None else self._moments[0].numpy()

    @property
    def cov(self) -> np.ndarray:
        """dL/d(incoming cov), (*batch, 7, 7), entry by entry -- ParameterBeam VJPs only; None like `mu`."""
        if self._moments is None:
            raise KeyError("the gradient w.r.t. cov exists for ParameterBeam VJPs only")
        return None if self._moments[1] is None else self._moments[1].numpy()

    @property
    def chosen_particles(self) -> np.ndarray:
        """
        dL/d(incoming coordinates of the chosen particles), (*batch, K, 7), row j for `trajectory_indices[j]` (a repeated
        index has a row per repeat) -- `track_along_vjp(..., trajectories=)` only.
        """
        if self._chosen_dev is None:
            raise KeyError("the gradient w.r.t. chosen particles exists for track_along_vjp(..., trajectories=) only")
        return self._chosen_dev.numpy()

    def __contains__(self, element) -> bool:
        if any(el is element for el, _ in self._zeros) or any(el is element for el in self._screens):
            return True
        return any(el is element and el._kind in DIFFERENTIABLE_KINDS for el in self._program.leaves)

    def __getitem__(self, element) -> dict:
        if id(element) in self._cache:
            return self._cache[id(element)]
        from .accelerator.magnets import RBend

        for el, names in self._zeros:
            if el is element:
                return {n: np.zeros(np.asarray(getattr(element, n)).shape) for n in names}
        for k, el in enumerate(self._screens):
            if el is element:  # the image sees mu_x - misalignment[0], mu_y - misalignment[1]: minus the mu cotangent there
                shape = np.asarray(el.misalignment).shape
                if not self._screen_shifts_dev:
                    return {"misalignment": np.zeros(shape)}
                shifts = sum(part.numpy() for part in self._screen_shifts_dev).reshape(*self._batch_shape, len(self._screens), 2)
                self._cache[id(element)] = {"misalignment": _unbroadcast(np.ascontiguousarray(shifts[..., k, :]), shape)}
                return self._cache[id(element)]
        raw, total = self._host(), None
        for e, el in enumerate(self._program.leaves):
            if el is not element or el._kind not in DIFFERENTIABLE_KINDS:
                continue
            g = {n: raw[..., e, j] for j, n in enumerate(el._row_names())}
            out = {}
            if "misalignment_x" in g:
                mis = np.stack([g.pop("misalignment_x"), g.pop("misalignment_y")], axis=-1)
                out["misalignment"] = _unbroadcast(mis, np.asarray(el.misalignment).shape)
            if isinstance(el, RBend):  # e1 = e1_user + angle/2, e2 = e2_user + angle/2 (rbend.py:79-80)
                g["angle"] = g["angle"] + 0.5 * (g["e1"] + g["e2"])
            for n, v in g.items():
                out[n] = _unbroadcast(v, np.asarray(getattr(el, n)).shape)
            # the same element object may appear several times in the lattice
            total = out if total is None else {n: total[n] + out[n] for n in out}
        if total is None:
            raise KeyError(f"{element!r} has no differentiable parameters in this lattice")
        self._cache[id(element)] = total
        return total


_COORDINATES = ("x", "xp", "y", "yp", "s", "p")


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
    from . import config

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


def _p(array):  # a device array, or None, as a library call takes it
    return None if array is None else C.c_void_p(array.ptr)


class _Sweep:
    """What every sweep of the moment recursion is given besides its cotangents: lattice, incoming energy, outputs in HBM."""

    def __init__(self, rt, cache, program, beam):
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B = int(np.prod(batch_shape, dtype=np.int64))
        self.lat = engine._ready(cache, program, batch_shape, dtype, beam._energy._host)
        self.g_par, self.g_en = rt.empty((B, max(self.lat.E, 1), 8), dtype), rt.empty((B,), dtype)
        self.g_mu, self.g_cov = rt.empty((*batch_shape, 7), dtype), rt.empty((*batch_shape, 7, 7), dtype)
        self.e_in = beam._energy.broadcast_device(rt, batch_shape)


class TrackVJP:
    def __init__(self, segment, beam: ParticleBeam):
        if not isinstance(beam, ParticleBeam):
            raise TypeError("track_vjp needs a ParticleBeam")
        # active BPMs are read inside the streaming pass (observer steps); their readings are differentiable outputs
        items = engine.partition(segment.elements if hasattr(segment, "elements") else [segment], fuse_observers=True)
        if len(items) != 1 or not isinstance(items[0], engine.Program):
            raise NotImplementedError(
                f"track_vjp: a lattice with an active Screen or Aperture, or with more than {_ffi.MAX_OBSERVERS} active "
                "BPMs, is tracked in several passes -- differentiate the stretches one by one")
        self.program = items[0]
        beam = beam.materialized()  # the reverse pass indexes the incoming particles per sample
        self.beam = beam
        self.cache = engine.lattice_cache(segment)
        self.outgoing = engine.run_program_particles(self.cache, self.program, beam, moments=True)

    def __call__(self, mu_bar=None, cov_bar=None, wrt_particles: bool = False, readings: dict | None = None,
                 **properties) -> Gradients:
        """
        Cotangents of the outgoing beam's mean (`mu_bar`, (*batch, 6)) and covariance (`cov_bar`, (*batch, 6, 6)), of named
        beam properties (`sigma_x=...`), and -- `readings={bpm: bar}` -- of the readings of the lattice's active BPMs
        (`bar` shaped like `bpm.reading`: (2, *batch)).
        """
        rt = get_runtime()
        beam, program = self.beam, self.program
        batch_shape, dtype = beam.batch_shape, beam.dtype
        bars = _MomentCotangents(batch_shape, cov_width=6)
        if properties:  # (beside them a cotangent has their shape; alone a mean's is as wide as it comes)
            pm, pc = property_cotangents(self.outgoing, properties)
            bars.add(pm, pc)
            bars.add(None if mu_bar is None else np.asarray(mu_bar, dtype=np.float64).reshape(pm.shape),
                     None if cov_bar is None else np.asarray(cov_bar, dtype=np.float64).reshape(pc.shape))
        else:
            bars.add(mu_bar, cov_bar)
        B = bars.lead[0]
        lat = engine._ready(self.cache, program, batch_shape, dtype, beam._energy._host)
        # What differs from the sweeps of the moment recursion below, on purpose: this call is bound by the host (one per step
        # of an optimisation), so cotangents in and gradients out live in host memory the GPU reads and writes through ...
        g_rec = rt.to_device_result(_record_cotangents(bars.lead, *bars.chained()))
        g_par = rt.empty_result((B, max(lat.E, 1), 8), dtype)
        g_en = rt.empty_result((B,), dtype)
        g_p = rt.empty((*batch_shape, beam.num_particles, 7), dtype) if wrt_particles else None
        fwd = self.outgoing._moments.device(rt)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        g_obs = None  # ... and the kernel reads the BPMs inside the pass: their cotangents go to its table [B][observers][2]
        if readings:
            obs_bar = np.zeros((B, len(program.observers), 2), dtype=np.float64)
            known = {id(element): k for k, (_, element) in enumerate(program.observers)}
            for element, bar in readings.items():
                _known_bpm(element, id(element) in known)
                obs_bar[:, known[id(element)], :] += _reading_bar(bar, batch_shape).T
            g_obs = rt.to_device_result(obs_bar)
        rt.check(rt.lib.lynx_track_particles_backward(
            rt.ctx, lat.handle, beam.num_particles, _p(e_in), _p(beam._particles.device(rt)), _p(fwd), _p(g_rec), _p(g_par),
            _p(g_en), _p(g_p), _p(g_obs)))
        return Gradients(program, beam, g_par, g_en, particles=g_p)


class ChainedGradients:
    """Gradients of a lattice that was differentiated stretch by stretch (a ParameterBeam through active BPMs)."""

    def __init__(self, parts: list):
        self._parts = parts  # in lattice order

    @property
    def energy(self) -> np.ndarray:
        return sum(part.energy for part in self._parts)

    @property
    def mu(self) -> np.ndarray:
        return self._parts[0].mu

    @property
    def cov(self) -> np.ndarray:
        return self._parts[0].cov

    def __contains__(self, element) -> bool:
        return any(element in part for part in self._parts)

    def __getitem__(self, element) -> dict:
        total = None
        for part in self._parts:
            if element in part:
                got = part[element]
                total = got if total is None else {n: total[n] + got[n] for n in got}
        if total is None:
            raise KeyError(f"{element!r} has no differentiable parameters in this lattice")
        return total


class MomentsVJP:
    """
    Vector-Jacobian product of `Segment.track` on a `ParameterBeam` (lynx_track_moments_backward).  An active BPM cuts
    the lattice in stretches (it is a host-side step of `track`, bpm.py:48-58): each stretch is differentiated by the
    kernel, and (mu_bar, cov_bar) -- plus the cotangent of the BPM's reading, which is (mu_x, mu_y) of the beam at that
    point -- is handed from a stretch to the one in front of it.
    """

    def __init__(self, segment, beam):
        items = engine.partition(segment.elements if hasattr(segment, "elements") else [segment])
        for item in items:
            if not isinstance(item, engine.Program) and not getattr(item, "_fusable_observer", False):
                raise NotImplementedError("track_vjp: lattices with an active Screen or Aperture are not differentiated")
        self.cache = engine.lattice_cache(segment)
        self.stretches = []  # (Program, beam entering it) / (BPM, None), in lattice order
        for k, item in enumerate(items):
            if isinstance(item, engine.Program):
                if any(el._kind == _ffi.KIND_CAVITY for el in item.leaves) and any(isinstance(i, engine.Program) for i in items[k + 1:]):
                    raise NotImplementedError(
                        "track_vjp: a cavity in front of an active BPM (the energy cotangent does not cross stretches yet)")
                self.stretches.append((item, beam))
                beam = engine.run_program_parameters(self.cache, item, beam)
            else:
                item._observe(beam)
                self.stretches.append((item, None))
                beam = beam._shallow_copy()
        self.program = items[0] if len(items) == 1 else None
        self.beam = self.stretches[0][1] if self.stretches else beam
        self.outgoing = beam

    def _stretch(self, program, beam, mb, cb) -> Gradients:
        rt = get_runtime()
        sweep = _Sweep(rt, self.cache, program, beam)
        # named, so that both uploads stay allocated until the call has been enqueued
        mb_dev, cb_dev = rt.to_device(mb.astype(beam.dtype)), rt.to_device(cb.astype(beam.dtype))
        rt.check(rt.lib.lynx_track_moments_backward(
            rt.ctx, sweep.lat.handle, _p(sweep.e_in), _p(beam._mu_d.device(rt)), _p(beam._cov_d.device(rt)),
            _p(mb_dev), _p(cb_dev), _p(sweep.g_par), _p(sweep.g_en), _p(sweep.g_mu), _p(sweep.g_cov)))
        return Gradients(program, beam, sweep.g_par, sweep.g_en, moments=(sweep.g_mu, sweep.g_cov))

    def __call__(self, mu_bar=None, cov_bar=None, readings: dict | None = None, **properties):
        """
        `mu_bar` (*batch, <=7), `cov_bar` (*batch, 6|7, 6|7): cotangents entry by entry; `readings={bpm: bar}`: cotangents
        of the readings of active BPMs, shaped like `bpm.reading` -- (2, *batch).
        """
        batch_shape = self.outgoing.batch_shape
        bars = _MomentCotangents(batch_shape)
        if properties:
            bars.add(*property_cotangents(self.outgoing, properties))
        bars.add(mu_bar, cov_bar)
        mb, cb = bars.summed()
        readings = dict(readings or {})
        for element in readings:
            _known_bpm(element, any(element is item for item, beam in self.stretches if beam is None))
        parts = []
        for item, beam in reversed(self.stretches):
            if beam is None:  # an active BPM cuts the lattice here: its reading joins what the stretch in front is given
                for element, bar in readings.items():
                    if element is item:
                        _add_reading(mb, bar, batch_shape)
                continue
            part = self._stretch(item, beam, mb, cb)
            parts.insert(0, part)
            mb = np.asarray(part.mu, dtype=np.float64).reshape(*bars.lead, 7)
            cb = np.asarray(part.cov, dtype=np.float64).reshape(*bars.lead, 7, 7)  # (what the stretch in front is given)
        if not parts:
            raise ValueError("track_vjp: the lattice has no element to differentiate")
        return parts[0] if len(parts) == 1 else ChainedGradients(parts)


# -------------------------------------------------------------------------------------------
# gradients of the beam ALONG the lattice (Segment.track_along)
# -------------------------------------------------------------------------------------------

MAX_TRACE_LEAVES = 256  # lynx_track_*_along_backward: k_build_bwd deals the steps of a program to its 256 threads
MAX_TRACE_LOSS_APERTURES = 15  # lynx_track_particles_along_backward_losses: 16 survivor sets
MAX_TRACE_CAVITY_LEAVES = 64  # lynx_track_particles_along_backward_cavities: k_track_bwd parks the states of 16 groups of 4 steps


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
    from . import config
    from .trace import ParticleBeamTrace

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
            gamma = np.asarray(trace.energy, dtype=np.float64) / engine.ELECTRON_MASS_EV
            moving = np.abs(gamma) > 0
            with np.errstate(all="ignore"):
                bg = np.where(moving, np.sqrt(1 - 1 / gamma**2) * gamma, 0.0)  # relativistic beta . gamma
                dbg = np.where(moving, gamma / np.sqrt(gamma**2 - 1), 0.0) / engine.ELECTRON_MASS_EV
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


def _refuse_moments(cavity: str):
    raise NotImplementedError(
        f"track_along_vjp: active Cavity {cavity!r} -- the moments of a ParticleBeam are not "
        "closed under a cavity's kick; a ParameterBeam of the same lattice is differentiated, and so is this beam by a "
        "second pass over its particles: track_along_vjp(..., cavities=True)")


def _trace_mode(segment, beam, trajectories, losses, screens, cavities):
    """
    Every refusal of `track_along_vjp` by value, before anything touches the GPU -> (mode, the trace's program, the leaf
    elements, the chosen particles or None, the name of the active cavity that stops this beam's moment cotangents or None).
    """
    from .particles.parameter_beam import ParameterBeam

    if not isinstance(beam, (ParameterBeam, ParticleBeam)):
        raise TypeError(f"track_along_vjp needs a ParticleBeam or a ParameterBeam, not {type(beam)}")
    for name, flag in (("losses", losses), ("screens", screens), ("cavities", cavities)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"track_along_vjp: {name} is True or False, not {flag!r}")
    if cavities and (trajectories is not None or losses):
        raise NotImplementedError(
            "track_along_vjp: cavities=True together with " + ("trajectories=" if trajectories is not None else "losses=True")
            + " -- the second pass over the particles differentiates the moments of the whole beam alone; ask for one of "
            "the two")
    particles = isinstance(beam, ParticleBeam)
    if screens and particles:
        raise TypeError(
            "track_along_vjp: screens=True with a ParticleBeam -- its screen image is a histogram of counts, a step "
            "function of the magnets whose gradient is zero almost everywhere; a ParameterBeam of the same moments "
            "(its image is a smooth density) is differentiated")
    if losses and trajectories is not None:
        raise NotImplementedError(
            "track_along_vjp: losses=True together with trajectories= -- the trajectories of a trace with losses are "
            "not differentiated; ask for one of the two")
    chosen = None if trajectories is None else engine.chosen_particles(trajectories, beam)
    leaves = list(segment._leaves() if hasattr(segment, "_leaves") else [segment])
    # (raises for an active Screen -- and, without `losses`, for an active Aperture --, naming it)
    program = engine._trace_plan(segment, leaves, bool(losses), True) if screens else engine._trace_plan(segment, leaves, bool(losses))
    B = int(np.prod(beam.batch_shape, dtype=np.int64))
    if screens and program.screens and B > _ffi.MAX_IMAGE_BATCH:  # (as lynx_gaussian_images_along refuses it)
        raise _ffi.LynxError(
            f"track_along_vjp: screens=True with a batch of {B} samples, more than {_ffi.MAX_IMAGE_BATCH} -- "
            "lynx_gaussian_images_along takes a sample per row of its launch grid (bad argument); trace the batch in parts")
    # survivors: a ParticleBeam and an active aperture; anything else with `losses` is the plain problem (nobody is lost)
    if not particles:
        mode = "moments"
    elif losses and len(program.apertures) > 0:
        mode = "survivors"
    else:
        mode = "kicks" if cavities else "particles" if chosen is None else "trajectories"
        program = engine._trace_plan(segment, leaves)
    if mode == "survivors" and len(program.apertures) > MAX_TRACE_LOSS_APERTURES:
        raise NotImplementedError(
            f"track_along_vjp: {len(program.apertures)} active apertures, more than {MAX_TRACE_LOSS_APERTURES} (the "
            f"first one beyond is {program.apertures[MAX_TRACE_LOSS_APERTURES][1].name!r}) -- differentiate the "
            "lattice in stretches")
    if len(leaves) > MAX_TRACE_LEAVES:
        raise NotImplementedError(
            f"track_along_vjp: {len(leaves)} leaf elements, more than {MAX_TRACE_LEAVES} (the first one beyond is "
            f"{leaves[MAX_TRACE_LEAVES].name!r}) -- differentiate the lattice in stretches")
    if mode == "kicks" and len(leaves) > MAX_TRACE_CAVITY_LEAVES:
        raise NotImplementedError(
            f"track_along_vjp: cavities=True with {len(leaves)} leaf elements, more than {MAX_TRACE_CAVITY_LEAVES} (the first "
            f"one beyond is {leaves[MAX_TRACE_CAVITY_LEAVES].name!r}) -- differentiate the lattice in stretches")
    # the first active cavity in front of a ParticleBeam: no moment cotangent passes it but through the kicks
    cavities_at = [first for kind, first, _ in program.steps if kind == _ffi.STEP_CAVITY] if particles and mode != "kicks" else []
    cavity = leaves[cavities_at[0]].name if cavities_at else None
    if cavity is not None and chosen is None:
        _refuse_moments(cavity)
    return mode, program, leaves, chosen, cavity


def _screen_of(key, program, leaves) -> int:
    """The ordinal among the trace's active screens of what `key` means: the `Screen` itself, or whatever `trace.image_at`
    takes (a name, the index of the point it observes) -- with that method's errors."""
    from .trace import screen_ordinal

    points = [step for step, _ in program.screens]
    if getattr(key, "_swallows_beam", False):  # the Screen element itself
        found = [k for k, (_, el) in enumerate(program.screens) if el is key]
        if not found:
            raise KeyError(f"{key!r} is not an active screen of this trace (screens at {points})")
        return found[0]
    return screen_ordinal([el.name for el in leaves], points, key)


class _TargetLayout:
    """Where the targets lie in what is uploaded: `offsets` per active screen (-1: no target), the `cells` of one row, the
    scalars between two samples' rows (`stride`, 0: one row shared by the batch) and the host array itself."""

    def __init__(self, offsets, cells, stride, host):
        self.offsets, self.cells, self.stride, self.host = offsets, cells, stride, host


class ImageTargets:
    """
    Target images of active screens, `{screen: target}` -- a key is whatever `trace.image_at` takes or the `Screen` itself, a
    target is `(nx, ny)` or `(*batch, nx, ny)` of that screen's image.  Given to `track_along_vjp(..., image_targets=)` they
    are uploaded ONCE, in the layout `lynx_gaussian_images_along_mse` reads, and stay on the device: the same object serves
    every pass of a tuning loop.  All targets `(nx, ny)`: one row shared by the batch.
    """

    def __init__(self, targets: dict):
        if not isinstance(targets, dict):
            raise TypeError(f"ImageTargets: a dict {{screen: target image}}, not {type(targets)}")
        self._given = [(key, np.array(target)) for key, target in targets.items()]  # (copies: the upload is made once)
        self._remembered = None  # (what the layout depends on, the layout, the device array or None)

    def _layout(self, program, leaves, beam) -> _TargetLayout:
        """The targets against one trace's screens and one beam, refused by value; nothing touches the GPU."""
        dtype, batch_shape = np.dtype(beam.dtype), tuple(beam.batch_shape)
        shapes = [tuple(len(v) for v in engine._pixel_positions(el, dtype)) for _, el in program.screens]
        key = (tuple(id(el) for _, el in program.screens), tuple(shapes), batch_shape, dtype.str)
        if self._remembered is not None and self._remembered[0] == key:
            return self._remembered[1]
        B = int(np.prod(batch_shape, dtype=np.int64))
        named = {}
        for given, target in self._given:
            k = _screen_of(given, program, leaves)
            name, shape = program.screens[k][1].name, shapes[k]
            if k in named:
                raise ValueError(f"track_along_vjp: screen {name!r} is given two target images")
            fits = target.shape == shape
            if not fits and target.ndim > 2:
                try:
                    fits = np.broadcast_shapes(target.shape, (*batch_shape, *shape)) == (*batch_shape, *shape)
                except ValueError:
                    fits = False
            if not fits:
                raise ValueError(f"track_along_vjp: the target image of screen {name!r} has shape {target.shape}, which is neither "
                                 f"its image's {shape} (nx, ny) nor broadcasts to {(*batch_shape, *shape)} (*batch, nx, ny)")
            named[k] = target
        shared = all(target.ndim == 2 for target in named.values())
        offsets, first = [], 0
        for k, shape in enumerate(shapes):
            offsets.append(first if k in named else -1)
            first += shape[0] * shape[1] if k in named else 0
        host = np.zeros((1 if shared else B, max(first, 1)), dtype=dtype)
        for k, target in named.items():
            cells = shapes[k][0] * shapes[k][1]
            rows = target.reshape(1, cells) if shared else np.broadcast_to(target, (*batch_shape, *shapes[k])).reshape(B, cells)
            host[:, offsets[k]:offsets[k] + cells] = rows
        layout = _TargetLayout(offsets, first, 0 if shared else max(first, 1), host)
        self._remembered = (key, layout, None)
        return layout

    def _device(self, rt, layout):
        key, remembered, dev = self._remembered
        assert remembered is layout
        if dev is None:
            dev = rt.to_device(layout.host)
            self._remembered = (key, layout, dev)
        return dev


# the properties a moment target may name, in the order of their codes: bit k of a point's mask in lynx_moments_along_loss
MOMENT_PROPERTIES = (*("mu_" + c for c in _COORDINATES), *("sigma_" + c for c in _COORDINATES), "sigma_xxp", "sigma_yyp",
                     "emittance_x", "emittance_y", "normalized_emittance_x", "normalized_emittance_y", "beta_x", "beta_y",
                     "alpha_x", "alpha_y", "energy")
_ENERGY_PROPERTIES = ("normalized_emittance_x", "normalized_emittance_y", "energy")  # what adds into the energy's cotangent


class _MomentLayout:
    """Where the moment targets lie in what is uploaded: `terms` [(point, name)] in (point, code) order, `points` [(point,
    mask)], `first` the ordinal of each point's first term, the scalars between two samples' rows (`stride`, 0: one row set
    shared by the batch) and the host rows (1 | B, T, 2) float64 of (target, weight)."""

    def __init__(self, terms, stride, host):
        self.terms, self.stride, self.host = terms, stride, host
        self.points, self.first = [], []
        for t, (point, name) in enumerate(terms):
            if not self.points or self.points[-1][0] != point:
                self.points.append([point, 0])
                self.first.append(t)
            self.points[-1][1] |= 1 << MOMENT_PROPERTIES.index(name)
        self.energy = any(name in _ENERGY_PROPERTIES for _, name in terms)  # a term adds into the energy's cotangent
        self.moments = any(name != "energy" for _, name in terms)  # a term adds into the moments' cotangents
        self.arguments = (len(self.points), (C.c_int32 * (2 * len(self.points)))(*(v for pair in self.points for v in pair)))


class MomentTargets:
    """
    Target values of beam properties at points of a trace, `{point: {property: target}}` -- a point is whatever
    `trace.index_of` takes (an element's name: the point behind it; or a point index, negative from the end), a property one
    of `MOMENT_PROPERTIES`, a target a scalar (one for the batch) or an array broadcastable to (*batch,).  `weights` has the
    same nesting and the same shapes; a missing weight is 1.  Given to `track_along_vjp(..., moment_targets=)` the loss is

        sum over the terms of weight (value - target)^2

    with the terms ordered by (point index, the property's place in `MOMENT_PROPERTIES`): `terms`, the list of (point index,
    name), once a layout exists.  The (target, weight) rows are uploaded ONCE, in the layout lynx_moments_along_loss reads,
    and stay on the device: the same object serves every pass of a tuning loop.  All targets and weights scalars: one row set
    shared by the batch.
    """

    def __init__(self, targets: dict, weights: dict | None = None):
        for what, given in (("targets", targets), ("weights", {} if weights is None else weights)):
            if not isinstance(given, dict) or not all(isinstance(named, dict) for named in given.values()):
                raise TypeError(f"MomentTargets: {what} is a dict {{point: {{property: value}}}}, not {given!r}")
            for named in given.values():
                for name in named:
                    if name not in MOMENT_PROPERTIES:
                        raise KeyError(f"no cotangent rule for trace property {name!r}")
        # (copies: the upload is made once)
        self._given = [[(point, {name: np.array(value, dtype=np.float64) for name, value in named.items()}) for point, named in given.items()]
                       for given in (targets, weights or {})]
        if not any(named for _, named in self._given[0]):
            raise ValueError("MomentTargets: no target is given")
        self._remembered = None  # (what the layout depends on, the layout, the device array or None)

    @property
    def terms(self) -> list:
        if self._remembered is None:
            raise ValueError("MomentTargets: the terms are known once the targets have met a trace -- pass them to track_along_vjp")
        return list(self._remembered[1].terms)

    def _layout(self, names, batch_shape) -> _MomentLayout:
        """The targets against the points of one trace (`names` of its elements) and one batch, refused by value; nothing
        touches the GPU."""
        from .trace import point_index

        batch_shape = tuple(batch_shape)
        key = (tuple(names), batch_shape)
        if self._remembered is not None and self._remembered[0] == key:
            return self._remembered[1]
        B = int(np.prod(batch_shape, dtype=np.int64))
        found = [{}, {}]  # (point, code) -> value, of the targets and of the weights
        for what, given, values in (("target", self._given[0], found[0]), ("weight", self._given[1], found[1])):
            for point, named in given:
                k = point_index(names, point)
                for name, value in named.items():
                    if (k, MOMENT_PROPERTIES.index(name)) in values:
                        raise ValueError(f"track_along_vjp: {name!r} at point {k} is given two {what}s")
                    try:
                        np.broadcast_to(value, batch_shape)
                    except ValueError:
                        raise ValueError(f"track_along_vjp: the {what} of {name!r} at point {k} has shape {value.shape}, which "
                                         f"does not broadcast to the batch {batch_shape}") from None
                    values[(k, MOMENT_PROPERTIES.index(name))] = value
        for k, code in found[1]:
            if (k, code) not in found[0]:
                raise ValueError(f"track_along_vjp: a weight of {MOMENT_PROPERTIES[code]!r} at point {k}, which has no target")
        order = sorted(found[0])
        shared = all(value.ndim == 0 for values in found for value in values.values())
        host = np.ones((1 if shared else B, len(order), 2))
        for column, values in enumerate(found):
            for t, term in enumerate(order):
                if term in values:
                    host[:, t, column] = values[term] if shared else np.broadcast_to(values[term], batch_shape).reshape(B)
        layout = _MomentLayout([(k, MOMENT_PROPERTIES[code]) for k, code in order], 0 if shared else 2 * len(order), host)
        self._remembered = (key, layout, None)
        return layout

    def _device(self, rt, layout):
        key, remembered, dev = self._remembered
        assert remembered is layout
        if dev is None:
            dev = rt.to_device(layout.host)
            self._remembered = (key, layout, dev)
        return dev


class TrackAlongVJP:
    """
    Vector-Jacobian product of `Segment.track_along`: gradients of any function of the beam moments and the energy at
    EVERY point of the lattice (lynx_track_moments_along_backward / lynx_track_particles_along_backward).  Without a
    kicking cavity every element is an affine map, so a ParticleBeam's mean and covariance obey the ParameterBeam's
    recursion: one reverse sweep of that recursion over the forward trace serves both beam classes, and no particle is
    tracked a second time.

    With `trajectories=` (the selection rules of `track_along`) the forward trace also keeps the coordinates of the chosen
    particles at every point, and the call takes `trajectories_bar`: cotangents of those coordinates
    (lynx_track_particles_along_backward_trajectories).  A single trajectory is differentiable through a cavity's kick, so
    a ParticleBeam on a lattice with an active cavity is accepted then -- for `trajectories_bar` and `energy_bar`; a
    moment cotangent is still refused, by the call.

    With `cavities=True` a ParticleBeam's moment cotangents pass active cavities: the reverse call is a second pass over the
    particles (lynx_track_particles_along_backward_cavities), the sweep of `track_vjp` with the moment cotangent of every
    point given to every particle at that point; at most 64 leaf elements, `wrt_particles=True` in the call.
    """

    def __init__(self, segment, beam, trajectories=None, losses=False, screens=False, cavities=False, image_targets=None,
                 moment_targets=None):
        targets = image_targets is not None
        if targets and not isinstance(image_targets, (dict, ImageTargets)):
            raise TypeError(f"track_along_vjp: image_targets is a dict {{screen: target image}} or an ImageTargets, not {type(image_targets)}")
        if moment_targets is not None and not isinstance(moment_targets, (dict, MomentTargets)):
            raise TypeError("track_along_vjp: moment_targets is a dict {point: {property: target}} or a MomentTargets, not "
                            f"{type(moment_targets)}")
        # the mode, decided once: "moments" (a ParameterBeam's sweep), "particles", "trajectories", "survivors" or "kicks"
        # (image targets need the screens in the trace's plan, and a ParticleBeam is refused as `screens=True` refuses it)
        self.mode, self.program, self.leaves, self.chosen, self._cavity = _trace_mode(
            segment, beam, trajectories, losses, True if targets and isinstance(screens, (bool, np.bool_)) else screens, cavities)
        self.segment, self.beam = segment, beam
        self._screens = bool(screens)  # (of "moments": the forward trace makes images, the call takes their cotangents)
        self._targets = self._image_loss = self._shots = None
        if targets:  # every refusal by value, before anything touches the GPU
            self._targets = image_targets if isinstance(image_targets, ImageTargets) else ImageTargets(image_targets)
            layout = self._targets._layout(self.program, self.leaves, beam)
        self._moment_targets = self._moment_layout = self._moment_loss = None
        if moment_targets is not None:
            self._moment_targets = moment_targets if isinstance(moment_targets, MomentTargets) else MomentTargets(moment_targets)
            self._moment_layout = self._moment_targets._layout([el.name for el in self.leaves], beam.batch_shape)
        # (a keyword is given only where it says something; apertures are identity steps of a ParameterBeam's trace; with
        # image targets alone the screens are points of the trace and no image is made)
        plain = {**({"losses": True} if losses and self.mode == "moments" else {}),
                 **({"screens": True} if screens else {"screens": "points"} if targets else {})}
        options = {"survivors": {"losses": "particles"}, "trajectories": {"trajectories": self.chosen}}.get(self.mode, plain)
        if self._moment_layout is not None:  # (the moment loss reads the energies where the trace wrote them)
            options = {**options, "keep_energy": True}
        self.trace = engine.track_along(segment, self.leaves, beam, keep_outgoing=True, keep_device=True, **options)
        self._set_records = self._survivor_set_records() if self.mode == "survivors" else None
        if targets:
            self._image_loss = self._evaluate_image_loss(layout)
        if self._moment_layout is not None:
            self._moment_loss = self._evaluate_moment_loss(self._moment_layout)

    def _moment_loss_arguments(self, rt, layout):
        """What lynx_moments_along_loss and its reverse half are given alike: sizes, the states of the trace, the terms, the rows."""
        from . import config

        beam, states = self.beam, self.trace._device
        B, P = int(np.prod(beam.batch_shape, dtype=np.int64)), self.trace.num_points
        return (rt.ctx, engine.dtype_code(beam.dtype), B, P, _p(states.get("records")), _p(states.get("mu")), _p(states.get("cov")),
                _p(states["energy"]), int(config.std_ddof), *layout.arguments, _p(self._moment_targets._device(rt, layout)), layout.stride)

    def _evaluate_moment_loss(self, layout):
        """
        The refusals that need the trace, then lynx_moments_along_loss right behind it, on its stream: the value of every term
        [B][T], the loss per target point [B][Q] and per sample [B], float64, all kept on the device -> (values, per point, loss).
        """
        if layout.moments and self._cavity is not None:  # (exactly where a moment cotangent is refused)
            _refuse_moments(self._cavity)
        if self.mode == "survivors":
            B, P = int(np.prod(self.beam.batch_shape, dtype=np.int64)), self.trace.num_points
            dead = np.asarray(self.trace.num_survivors).reshape(B, P) == 0
            for point, name in layout.terms:
                if name != "energy" and dead[:, point].any():  # (the energy is there at every point)
                    self._refuse_cotangent_on_nobody(np.arange(P) == point, dead, repr(name))
        rt = get_runtime()
        B, T, Q = int(np.prod(self.beam.batch_shape, dtype=np.int64)), len(layout.terms), len(layout.points)
        values, per_point, loss = rt.empty((B, T), np.float64), rt.empty((B, Q), np.float64), rt.empty((B,), np.float64)
        rt.check(rt.lib.lynx_moments_along_loss(*self._moment_loss_arguments(rt, layout), _p(values), _p(per_point), _p(loss)))
        return values, per_point, loss

    def _need_moment_loss(self, what):
        if self._moment_loss is None:
            raise ValueError(f"track_along_vjp: {what} needs moment targets -- pass moment_targets= to track_along_vjp")
        return self._moment_loss

    @property
    def moment_values(self) -> np.ndarray:
        """(*batch, T) float64: the value of every term of the moment loss, in the order of `MomentTargets.terms`."""
        values = self._need_moment_loss("moment_values")[0]
        return values.numpy().reshape(*self.beam.batch_shape, len(self._moment_layout.terms))

    @property
    def moment_loss(self) -> np.ndarray:
        """(*batch,) float64: the sum over the terms, in their order, of weight (value - target)^2."""
        return self._need_moment_loss("moment_loss")[2].numpy().reshape(self.beam.batch_shape)

    def moment_loss_of(self, point) -> np.ndarray:
        """The part of `moment_loss` that one point's terms make: by whatever `trace.index_of` takes."""
        per_point, layout = self._need_moment_loss("moment_loss_of")[1], self._moment_layout
        k = self.trace.index_of(point)
        found = [q for q, (at, _) in enumerate(layout.points) if at == k]
        if not found:
            raise KeyError(f"point {k} has no target in this call's moment_targets (targets at {[at for at, _ in layout.points]})")
        return np.ascontiguousarray(per_point.numpy().reshape(*self.beam.batch_shape, len(layout.points))[..., found[0]])

    def _moment_loss_cotangents(self, moment_loss_bar) -> np.ndarray:
        """`moment_loss_bar` as (B,) float64; refused by value."""
        if self._moment_loss is None:
            raise ValueError("track_along_vjp: moment_loss_bar needs the moment loss of the forward pass -- pass moment_targets= "
                             "to track_along_vjp")
        w, batch_shape = np.asarray(moment_loss_bar, dtype=np.float64), tuple(self.beam.batch_shape)
        try:
            return np.ascontiguousarray(np.broadcast_to(w, batch_shape)).reshape(-1)
        except ValueError:
            raise ValueError(f"track_along_vjp: moment_loss_bar has shape {w.shape}, which does not broadcast to the batch "
                             f"{batch_shape}") from None

    # what the launches below share: a cotangent buffer is uploaded where the host made one and zero-filled on the device where
    # the moment loss alone adds into it; then the loss's reverse half, in front of the sweep on the same stream
    def _zeros(self, rt, shape, dtype):
        zeros = rt.empty(shape, dtype)
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, _p(zeros), 0, int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize))
        return zeros

    def _points_shape(self, *tail):
        return (int(np.prod(self.beam.batch_shape, dtype=np.int64)), self.trace.num_points, *tail)

    def _record_buffer(self, rt, mb, cb):
        if mb is None:
            return self._zeros(rt, self._points_shape(_ffi.MOMENT_STRIDE), np.float64)
        return rt.to_device(_record_cotangents(mb.shape[:-1], mb, cb))

    def _moment_buffers(self, rt, mb, cb):
        dtype = self.beam.dtype
        if mb is None:
            return self._zeros(rt, self._points_shape(7), dtype), self._zeros(rt, self._points_shape(7, 7), dtype)
        return rt.to_device(mb.astype(dtype)), rt.to_device(cb.astype(dtype))

    def _add_moment_loss(self, rt, ml, eb_dev, rec_dev=None, mb_dev=None, cb_dev=None):
        if ml is None:
            return
        ml_dev = rt.to_device(ml)
        rt.check(rt.lib.lynx_moments_along_loss_backward(
            *self._moment_loss_arguments(rt, self._moment_layout), _p(ml_dev), _p(rec_dev), _p(mb_dev), _p(cb_dev), _p(eb_dev)))

    def _image_head(self, rt, *states):
        """
        What every image call begins with, (ctx, dtype, B, P, the named states of the trace), and the geometry of the trace's
        screens, looked up once per `TrackAlongVJP` -> (head, geometry).
        """
        beam = self.beam
        if self._shots is None:
            self._shots = engine._screen_geometry(self.segment, self.program, beam.batch_shape, beam.dtype, rt, False)
        return (rt.ctx, engine.dtype_code(beam.dtype), *self._points_shape(), *(_p(self.trace._device[s]) for s in states)), self._shots

    def _evaluate_image_loss(self, layout):
        """
        lynx_gaussian_images_along_mse right behind the trace, on its stream: the loss [B][K] and the six adjoint sums
        [B][K][6] of every screen with a target, float64, both kept on the device -> (loss, sums, which screens are named).
        """
        if not self.program.screens:  # (no active screen, and so no target: nothing to evaluate)
            return None, None, []
        rt = get_runtime()
        head, shots = self._image_head(rt, "mu", "cov")
        B, K = head[2], shots["count"]
        targets_dev = self._targets._device(rt, layout)
        loss, sums = rt.empty((B, K), np.float64), rt.empty((B, K, 6), np.float64)
        rt.check(rt.lib.lynx_gaussian_images_along_mse(
            *head, *shots["arguments"], (C.c_int64 * K)(*layout.offsets), _p(targets_dev), layout.stride, _p(loss), _p(sums)))
        return loss, sums, [offset >= 0 for offset in layout.offsets]

    @property
    def image_loss(self) -> dict:
        """{screen name: (*batch,) float64}: the mean squared difference of every named screen's image to its target."""
        if self._image_loss is None:
            raise ValueError("track_along_vjp: image_loss needs target images -- pass image_targets= to track_along_vjp")
        loss, _, named = self._image_loss
        if not any(named):
            return {}
        host = loss.numpy().reshape(*self.beam.batch_shape, len(named))
        return {el.name: np.ascontiguousarray(host[..., k]) for k, (_, el) in enumerate(self.program.screens) if named[k]}

    def image_loss_of(self, screen) -> np.ndarray:
        """`image_loss` of one screen: by whatever `trace.image_at` takes, or by the `Screen` itself."""
        if self._image_loss is None:
            raise ValueError("track_along_vjp: image_loss_of needs target images -- pass image_targets= to track_along_vjp")
        loss, _, named = self._image_loss
        k = _screen_of(screen, self.program, self.leaves)
        if not named[k]:
            raise KeyError(f"screen {self.program.screens[k][1].name!r} has no target image in this call's image_targets")
        return np.ascontiguousarray(loss.numpy().reshape(*self.beam.batch_shape, len(named))[..., k])

    def _image_loss_cotangents(self, image_loss_bar):
        """`image_loss_bar` as (B, K) of the beam's dtype, zeros for a screen without a target; refused by value."""
        if self._image_loss is None:
            raise ValueError("track_along_vjp: image_loss_bar needs the image loss of the forward pass -- pass image_targets= "
                             "to track_along_vjp")
        named, batch_shape = self._image_loss[2], self.beam.batch_shape
        B = int(np.prod(batch_shape, dtype=np.int64))
        bars = np.zeros((B, len(named)))

        def over_batch(bar, name):
            w = np.asarray(bar, dtype=np.float64)
            try:
                return np.broadcast_to(w, batch_shape).reshape(B)
            except ValueError:
                raise ValueError(f"track_along_vjp: image_loss_bar of screen {name!r} has shape {w.shape}, which does not "
                                 f"broadcast to the batch {tuple(batch_shape)}") from None

        if isinstance(image_loss_bar, dict):
            for key, bar in image_loss_bar.items():
                k = _screen_of(key, self.program, self.leaves)
                name = self.program.screens[k][1].name
                if not named[k]:
                    raise KeyError(f"screen {name!r} has no target image in this call's image_targets")
                bars[:, k] += over_batch(bar, name)
        else:
            for k, (_, el) in enumerate(self.program.screens):
                if named[k]:
                    bars[:, k] = over_batch(image_loss_bar, el.name)
        return bars.astype(self.beam.dtype)

    def _survivor_set_records(self):
        """
        The moment records of the INCOMING beam over the nested survivor sets, [B][A + 1][36] on the device
        (lynx_moments_by_loss): set j holds the particles alive behind the first j active apertures, by the `lost_at` the
        forward trace left on the device.  One more streaming pass over the incoming particles.
        """
        rt = get_runtime()
        beam, A = self.beam, len(self.program.apertures)
        B = int(np.prod(beam.batch_shape, dtype=np.int64))
        records = rt.empty((B, A + 1, _ffi.MOMENT_STRIDE), np.float64)
        rt.check(rt.lib.lynx_moments_by_loss(
            rt.ctx, engine.dtype_code(beam.dtype), B, beam.num_particles, _p(beam._particles.device(rt)),
            _ffi.TRACK_SHARED_INPUT if beam.is_shared else 0, A, _p(self.trace._device["lost_at"]), _p(records)))
        return records

    def _trajectory_cotangents(self, trajectories_bar) -> np.ndarray:
        """`trajectories_bar` as (B, P, K, 7) float64, refused by value."""
        if self.chosen is None:
            raise ValueError("track_along_vjp: trajectories_bar needs the trajectories of the forward trace -- pass "
                             "trajectories= (a number of particles or an array of particle indices) to track_along_vjp")
        batch_shape, P, K = self.beam.batch_shape, len(self.leaves) + 1, len(self.chosen)
        w = np.asarray(trajectories_bar, dtype=np.float64)
        want = (*batch_shape, P, K)
        k = w.shape[-1] if w.ndim else 0
        full = None
        if k in (6, 7):
            try:
                full = np.broadcast_to(w, (*want, k))
            except ValueError:
                pass
        if full is None:
            raise ValueError(f"track_along_vjp: trajectories_bar of shape {w.shape} does not broadcast to {(*want, 6)} "
                             f"or {(*want, 7)} (*batch, points, chosen particles, coordinates)")
        B = int(np.prod(batch_shape, dtype=np.int64))
        out = np.zeros((B, P, K, 7))
        out[..., :k] = full.reshape(B, P, K, k)
        return out

    def _cotangents(self, mu_bar, cov_bar, energy_bar, readings, properties):
        batch_shape, P = self.beam.batch_shape, self.trace.num_points
        bars = _MomentCotangents(batch_shape, P)
        eb = np.zeros(bars.lead)
        over_points = lambda bar: np.broadcast_to(np.asarray(bar, dtype=np.float64), (*batch_shape, P)).reshape(bars.lead)  # noqa: E731
        # a trace with losses: the points no particle of a sample reaches have no moments (NaN) and take no cotangent
        dead = np.asarray(self.trace.num_survivors).reshape(bars.lead) == 0 if self.mode == "survivors" else np.zeros(bars.lead, dtype=bool)
        if properties and dead.any():
            moments = {name: bar for name, bar in properties.items() if name != "energy"}  # (the energy is there at every point)
            for name, bar in moments.items():
                self._refuse_cotangent_on_nobody(over_points(bar), dead, repr(name))
            with np.errstate(all="ignore"):
                pm, pc, pe = trace_property_cotangents(self.trace, moments)
            nobody = dead.reshape(pe.shape)
            pm[nobody], pc[nobody], pe[nobody] = 0.0, 0.0, 0.0  # (0 x NaN of the rules above)
            bars.add(pm, pc)
            eb += pe.reshape(bars.lead)
            if "energy" in properties:
                eb += over_points(properties["energy"])
        elif properties:
            pm, pc, pe = trace_property_cotangents(self.trace, properties)
            bars.add(pm, pc)
            eb += pe.reshape(bars.lead)
        bars.add(mu_bar, cov_bar)
        mb, cb = bars.summed()
        if energy_bar is not None:
            eb += over_points(energy_bar)
        for element, bar in (readings or {}).items():
            points = [k for k, el in enumerate(self.leaves) if el is element and getattr(el, "_fusable_observer", False)]
            _known_bpm(element, bool(points))
            for k in points:  # an active BPM reads the beam that ENTERS it: point k of the trace
                _add_reading(mb, bar, batch_shape, k)
        if dead.any():  # (what nobody reaches stays zero: anything else was a cotangent of the moments of nobody)
            self._refuse_cotangent_on_nobody(np.abs(mb).sum(axis=-1) + np.abs(cb).sum(axis=(-1, -2)), dead, "the moments")
        return mb, cb, eb

    def _refuse_cotangent_on_nobody(self, bar, dead, what):
        """`bar` (B, P) must be zero where `dead`: the first offender is named by sample and point."""
        wrong = np.argwhere(dead & (bar != 0))
        if len(wrong):
            b, k = (int(v) for v in wrong[0])
            sample = tuple(int(v) for v in np.unravel_index(b, self.beam.batch_shape)) if self.beam.batch_shape else ()
            raise ValueError(
                f"track_along_vjp: a non-zero cotangent of {what} on sample {sample}, point {k}, which no particle reaches "
                f"(transmission 0 there): the moments of nobody have no gradient")

    def _image_cotangents(self, screen_images_bar):
        """
        `screen_images_bar` as one (B, cells) array of the beam's dtype in the layout of lynx_gaussian_images_along (screen
        after screen, zeros for a screen that is not named), refused by value; None for an empty dict.
        """
        if not self._screens:
            raise ValueError("track_along_vjp: screen_images_bar needs the screen images of the forward trace -- pass "
                             "screens=True to track_along_vjp")
        if not isinstance(screen_images_bar, dict):
            raise TypeError(f"track_along_vjp: screen_images_bar is a dict {{screen: cotangent of its image}}, not {type(screen_images_bar)}")
        trace, elements = self.trace, [el for _, el in self.program.screens]
        named = []  # (screen, cotangent broadcast to its image), checked before anything is allocated
        for key, bar in screen_images_bar.items():
            k = _screen_of(key, self.program, self.leaves)  # (KeyError for anything but an active screen of the trace)
            shape = trace.screen_images[k].shape
            w = np.asarray(bar)
            try:
                w = np.broadcast_to(w, shape)
            except ValueError:
                raise ValueError(f"track_along_vjp: screen_images_bar of screen {elements[k].name!r} has shape {w.shape}, which "
                                 f"does not broadcast to its image's {shape} (*batch, nx, ny)") from None
            named.append((k, w))
        if not named:
            return None
        B = int(np.prod(self.beam.batch_shape, dtype=np.int64))
        cells = [int(np.prod(image.shape[-2:])) for image in trace.screen_images]
        first = np.concatenate([[0], np.cumsum(cells)])
        # one pass per named screen, straight into what is uploaded: an ARES screen has 5e6 pixels per sample
        flat = np.zeros((B, int(first[-1])), dtype=self.beam.dtype)
        for k, w in named:
            flat[:, first[k]:first[k + 1]] += w.reshape(B, cells[k])
        return flat

    def __call__(self, mu_bar=None, cov_bar=None, energy_bar=None, readings: dict | None = None, trajectories_bar=None,
                 screen_images_bar: dict | None = None, wrt_particles: bool = False, image_loss_bar=None, moment_loss_bar=None,
                 **properties) -> Gradients:
        """
        `mu_bar` (*batch, P, 6|7), `cov_bar` (*batch, P, 6|7, 6|7) entry by entry, `energy_bar` (*batch, P): cotangents at
        every point; `properties`: cotangents (*batch, P) of any moment property of the trace and of `energy`;
        `readings={bpm: bar}`: of the readings of active BPMs, shaped like `bpm.reading` -- (2, *batch);
        `trajectories_bar` (broadcastable to (*batch, P, K, 6|7)): of the coordinates of the chosen particles at every point
        (`trajectories=` of `track_along_vjp`).  All of them in one reverse call; `Gradients.chosen_particles` is then the
        gradient w.r.t. the chosen incoming particles, and `mu`, `cov` exist if a moment cotangent was given.
        `screen_images_bar={screen: bar}` (`screens=True` of `track_along_vjp`): cotangents of the images of active screens,
        a key whatever `trace.image_at` takes or the `Screen` itself, a value broadcastable to that image (*batch, nx, ny);
        lynx_gaussian_images_along_backward reduces them on the device into the mu and cov cotangents at the screens' points,
        where the sweep picks them up, and `g[screen]["misalignment"]` is the gradient w.r.t. the screen's misalignment.
        `image_loss_bar` (`image_targets=` of `track_along_vjp`): cotangents of `image_loss` -- a scalar or (*batch,) for every
        screen with a target, or `{screen: bar}`; lynx_gaussian_images_along_mse_backward scales the sums the forward pass left
        on the device and adds them into the mu and cov cotangents at the screens' points, `g[screen]["misalignment"]` as above.
        `moment_loss_bar` (`moment_targets=` of `track_along_vjp`): the cotangent of `moment_loss`, a scalar or (*batch,);
        lynx_moments_along_loss_backward forms every term's bar from the states on the device and adds it into the cotangents
        the sweep reads.  Alone -- no other cotangent of a moment or of the energy in the call -- nothing with a point axis is
        made on the host: those cotangents are zero-filled on the device and the (*batch,) bars are the only upload.
        `wrt_particles=True` (`cavities=True` of `track_along_vjp`, a ParticleBeam): `Gradients.particles` (*batch, N, 7), the
        gradient w.r.t. every incoming particle, device-resident.
        """
        if wrt_particles and self.mode != "kicks":
            raise ValueError("track_along_vjp: wrt_particles=True needs the pass over the particles -- a ParticleBeam and "
                             "cavities=True of track_along_vjp (without a cavity g.mu and g.cov say the same)")
        wi = None if screen_images_bar is None else self._image_cotangents(screen_images_bar)
        lb = None if image_loss_bar is None else self._image_loss_cotangents(image_loss_bar)
        if lb is not None and not any(self._image_loss[2]):  # (no screen has a target: nothing to launch)
            lb = None
        ml = None if moment_loss_bar is None else self._moment_loss_cotangents(moment_loss_bar)
        with_moments = mu_bar is not None or cov_bar is not None or bool(readings) or any(name != "energy" for name in properties)
        # the moment loss as the call's only cotangent of a moment or of the energy: nothing with a point axis is made here
        alone = ml is not None and not with_moments and energy_bar is None and not properties
        wb = None  # (a trace with trajectories and no cotangent on them: zeros -- made on the device where the moment loss is alone)
        if trajectories_bar is not None or (self.chosen is not None and not alone):
            wb = self._trajectory_cotangents(np.zeros(7) if trajectories_bar is None else trajectories_bar)
        if with_moments and self._cavity is not None:
            _refuse_moments(self._cavity)
        mb, cb, eb = (None, None, None) if alone else self._cotangents(mu_bar, cov_bar, energy_bar, readings, properties)
        with_moments = with_moments or (ml is not None and self._moment_layout.moments)
        rt = get_runtime()
        sweep = _Sweep(rt, engine.trace_cache(self.segment), self.program, self.beam)
        # (an upload is named until its call has been enqueued, so that it stays allocated; no energy cotangent: no upload)
        eb_dev = rt.to_device(eb.astype(self.beam.dtype)) if eb is not None and np.any(eb) else None
        if eb_dev is None and ml is not None and self._moment_layout.energy:
            eb_dev = self._zeros(rt, self._points_shape(), self.beam.dtype)
        launch = getattr(self, "_launch_" + self.mode)  # (_launch_moments, _particles, _trajectories, _survivors, _kicks)
        results = launch(rt, sweep, mb, cb, eb_dev, wi=wi, lb=lb, wb=wb, ml=ml, with_moments=with_moments, wrt_particles=wrt_particles)
        return Gradients(self.program, self.beam, sweep.g_par, sweep.g_en, **results)

    # one method per mode, called alike (each names what it uses): the library call or calls -> `Gradients`' optional results
    def _launch_moments(self, rt, sweep, mb, cb, eb_dev, wi, lb, ml, **_):
        beam, states = self.beam, self.trace._device
        mb_dev, cb_dev = self._moment_buffers(rt, mb, cb)
        shifts = []  # the parts of dL/d(misalignment), one per image call: `Gradients` adds them
        if wi is not None:  # the images' cotangents go into mb_dev, cb_dev at the screens' points, on the same stream
            head, shots = self._image_head(rt, "mu", "cov")
            wi_dev = rt.to_device(np.ascontiguousarray(wi, dtype=beam.dtype))
            shifts.append(rt.empty((head[2], shots["count"], 2), beam.dtype))
            rt.check(rt.lib.lynx_gaussian_images_along_backward(
                *head, *shots["arguments"], _p(wi_dev), _p(mb_dev), _p(cb_dev), _p(shifts[-1])))
        if lb is not None:  # ... and so do the image losses' cotangents times the sums of the forward pass
            head, shots = self._image_head(rt, "cov")
            lb_dev = rt.to_device(np.ascontiguousarray(lb, dtype=beam.dtype))
            shifts.append(rt.empty((head[2], shots["count"], 2), beam.dtype))
            rt.check(rt.lib.lynx_gaussian_images_along_mse_backward(
                *head, shots["count"], shots["rows"], _p(self._image_loss[1]), _p(lb_dev), _p(mb_dev), _p(cb_dev), _p(shifts[-1])))
        self._add_moment_loss(rt, ml, eb_dev, mb_dev=mb_dev, cb_dev=cb_dev)
        rt.check(rt.lib.lynx_track_moments_along_backward(
            rt.ctx, sweep.lat.handle, _p(sweep.e_in), _p(states["mu"]), _p(states["cov"]), _p(mb_dev), _p(cb_dev), _p(eb_dev),
            _p(sweep.g_par), _p(sweep.g_en), _p(sweep.g_mu), _p(sweep.g_cov)))
        with_screens = self._screens or self._targets is not None
        return dict(moments=(sweep.g_mu, sweep.g_cov), screens=([el for _, el in self.program.screens], shifts) if with_screens else None)

    def _launch_particles(self, rt, sweep, mb, cb, eb_dev, ml, **_):
        rec_dev = self._record_buffer(rt, mb, cb)
        self._add_moment_loss(rt, ml, eb_dev, rec_dev=rec_dev)
        rt.check(rt.lib.lynx_track_particles_along_backward(
            rt.ctx, sweep.lat.handle, self.beam.num_particles, _p(sweep.e_in), _p(self.trace._device["records"]), _p(rec_dev),
            _p(eb_dev), _p(sweep.g_par), _p(sweep.g_en), _p(sweep.g_mu), _p(sweep.g_cov)))
        return dict(moments=(sweep.g_mu, sweep.g_cov))

    def _launch_trajectories(self, rt, sweep, mb, cb, eb_dev, wb, ml, with_moments, **_):
        beam, states, K = self.beam, self.trace._device, len(self.chosen)
        # without a moment cotangent the moment path does not run: no records in, no g.mu and g.cov out (a moment loss of
        # energies alone still adds into a record buffer, which the sweep is then not handed)
        rec_dev = self._record_buffer(rt, mb if with_moments else None, cb) if with_moments or ml is not None else None
        self._add_moment_loss(rt, ml, eb_dev, rec_dev=rec_dev)
        rec_dev = rec_dev if with_moments else None
        g_mu, g_cov = (sweep.g_mu, sweep.g_cov) if with_moments else (None, None)
        wb_dev = self._zeros(rt, self._points_shape(K, 7), np.float64) if wb is None else rt.to_device(wb)
        g_chosen = rt.empty((*beam.batch_shape, K, 7), beam.dtype)
        rt.check(rt.lib.lynx_track_particles_along_backward_trajectories(
            rt.ctx, sweep.lat.handle, beam.num_particles, _p(sweep.e_in), _p(states["records"]) if with_moments else None,
            _p(rec_dev), _p(eb_dev), _p(sweep.g_par), _p(sweep.g_en), _p(g_mu), _p(g_cov), K,
            _p(states["trajectories"]), _p(wb_dev), _p(g_chosen)))
        return dict(moments=(g_mu, g_cov) if with_moments else None, chosen=g_chosen)

    def _launch_kicks(self, rt, sweep, mb, cb, eb_dev, ml, wrt_particles, **_):
        beam = self.beam
        rec_dev = self._record_buffer(rt, mb, cb)
        self._add_moment_loss(rt, ml, eb_dev, rec_dev=rec_dev)
        g_p = rt.empty((*beam.batch_shape, beam.num_particles, 7), beam.dtype) if wrt_particles else None
        rt.check(rt.lib.lynx_track_particles_along_backward_cavities(
            rt.ctx, sweep.lat.handle, beam.num_particles, _p(sweep.e_in), _p(beam._particles.device(rt)),
            _ffi.TRACK_SHARED_INPUT if beam.is_shared else 0, _p(self.trace._device["records"]), _p(rec_dev), _p(eb_dev),
            _p(sweep.g_par), _p(sweep.g_en), _p(g_p)))
        return dict(particles=g_p, moments=Gradients.NO_INCOMING_MOMENTS)

    def _launch_survivors(self, rt, sweep, mb, cb, eb_dev, ml, **_):
        rec_dev = self._record_buffer(rt, mb, cb)
        self._add_moment_loss(rt, ml, eb_dev, rec_dev=rec_dev)
        A = len(self.program.apertures)
        at = (C.c_int32 * A)(*[step for step, _, _ in self.program.apertures])
        rt.check(rt.lib.lynx_track_particles_along_backward_losses(
            rt.ctx, sweep.lat.handle, self.beam.num_particles, _p(sweep.e_in), _p(self.trace._device["records"]), _p(rec_dev),
            _p(eb_dev), A, at, _p(self._set_records), _p(sweep.g_par), _p(sweep.g_en)))
        # the survivor set is held fixed: the limits that made it get gradient 0
        return dict(moments=Gradients.NO_INCOMING_MOMENTS, zeros=[(el, ("x_max", "y_max")) for _, el, _ in self.program.apertures])


def track_along_vjp(segment, beam, trajectories=None, losses=False, screens=False, cavities=False, image_targets=None,
                    moment_targets=None):
    """
    Forward pass of `segment.track_along(beam)` (the trace is `vjp.trace`; its states stay on the device); returns the
    callable vector-Jacobian product of the moments and energies at every point:

        vjp = lynx_amd.grad.track_along_vjp(segment, beam)
        g = vjp(beta_x=w_x, beta_y=w_y)          # cotangents (*batch, P) of any property of the trace, or
        g = vjp(mu_bar=..., cov_bar=..., energy_bar=..., readings={bpm: ...})
        g[segment.Q1]["k1"], g.energy, g.mu, g.cov

    `trajectories` (a ParticleBeam; `track_along`'s selection rules): the coordinates of the chosen particles at every point
    are differentiated as well --

        vjp = lynx_amd.grad.track_along_vjp(segment, beam, trajectories=[0, 17, 4])
        x = vjp.trace.trajectories[..., 0]       # (*batch, P, K)
        g = vjp(trajectories_bar=w)              # (*batch, P, K, 6|7), together with any cotangent above
        g[segment.HCOR1]["angle"], g.chosen_particles

    and an active cavity in front of a ParticleBeam is no obstacle to `trajectories_bar` and `energy_bar`.

    `losses=True` (a ParticleBeam): the forward pass is `segment.track_along(beam, losses=True)` -- active `Aperture`s remove
    particles, `vjp.trace` has `num_survivors`, `transmission`, `lost_in`, `lost_at` -- and every cotangent above is one of
    the SURVIVING beam at that point (a property's own count; a BPM reads the centroid of the particles alive in front of it):

        vjp = lynx_amd.grad.track_along_vjp(segment, beam, losses=True)
        k = vjp.trace.index_of("SCREEN")
        g = vjp(sigma_x=w, sigma_y=w)            # w (*batch, P), non-zero at point k: sizes of the collimated beam there
        g[segment.Q1]["k1"], g.energy

    The set of survivors is locally constant in the magnet settings and is HELD FIXED: the transmission is a step function
    and has no gradient, the moments over the survivors have one almost everywhere, and that is what is returned
    (lynx_moments_by_loss, lynx_track_particles_along_backward_losses).  An `Aperture`'s own `x_max` and `y_max`
    therefore get gradient 0, and `g.mu`, `g.cov` are None: no single set of particles came in.  A non-zero cotangent on a
    point no particle of a sample reaches is a ValueError.  At most 15 active apertures; not together with
    `trajectories=`.  Without an active aperture, or with a ParameterBeam (apertures pass it unchanged), `losses=True` is
    the plain call.

    `screens=True` (a ParameterBeam): the forward pass is `segment.track_along(beam, screens=True)` -- every active `Screen`
    makes its image inside the trace (`vjp.trace.screens`, `screen_images`, `image_at`; the screen's `reading` is that image)
    -- and the call takes cotangents of the images, together with any cotangent above:

        vjp = lynx_amd.grad.track_along_vjp(segment, parameter_beam, screens=True)
        img = vjp.trace.image_at("SCREEN")                        # (*batch, nx, ny)
        g = vjp(screen_images_bar={"SCREEN": 2 * (img - target)})
        g[segment.Q1]["k1"], g.energy, g.mu, g.cov, g[segment.SCREEN]["misalignment"]

    The image is the bivariate-normal density of (mu_x - misalignment[0], mu_y - misalignment[1]) and cov_xx, cov_xy, cov_yy at
    the point the screen observes; its adjoint is a weighted sum over all pixels (lynx_gaussian_images_along_backward, on the
    device, into the cotangents of mu and cov there), and the gradient with respect to the screen's `misalignment` -- summed
    over the batch where it is shared -- comes with it (zero for a screen that got no cotangent).  Nothing is special-cased:
    a covariance with cov_xx cov_yy - cov_xy^2 <= 0 gives NaN images and NaN gradients, a beam so far off the screen that the
    image has underflowed to 0 gives gradient 0.  A ParticleBeam is a TypeError (its image is a histogram of counts);
    `losses=True` may be combined (apertures pass a ParameterBeam unchanged); at most 65535 samples.

    `image_targets=` (a ParameterBeam): the loss every user of the path above writes, the mean squared difference of a screen's
    image to a target image, evaluated on the device -- neither the image nor its cotangent is made, read back or uploaded:

        targets = lynx_amd.grad.ImageTargets({"SCREEN": target})   # uploaded once, reusable over a loop (or pass the dict)
        vjp = lynx_amd.grad.track_along_vjp(segment, parameter_beam, image_targets=targets)
        vjp.image_loss                                            # {name: (*batch,) float64}; vjp.image_loss_of("SCREEN")
        g = vjp(image_loss_bar=1.0 / peak**2, beta_x=...)         # a scalar or (*batch,) for every named screen, or {screen: bar}
        g[segment.Q1]["k1"], g.mu, g.cov, g[segment.SCREEN]["misalignment"]

    A key is whatever `trace.image_at` takes or the `Screen` itself, a target is (nx, ny) -- then one target serves the whole
    batch -- or (*batch, nx, ny) of that screen's image.  The forward pass is the moment trace with the active screens as identity
    steps (`vjp.trace.screens` lists them, `screen_images` is empty, `image_at` raises, the screens' `reading` is left alone);
    lynx_gaussian_images_along_mse forms the density per pixel with the forward kernel's expression, so the loss is that of the
    image `screens=True` would have shown, bit for bit, and keeps the loss and six adjoint sums per sample and screen on the
    device; the call scales them by `image_loss_bar` (lynx_gaussian_images_along_mse_backward) in front of the sweep.  A screen
    without a target gets misalignment gradient 0.  `screens=True` may be given as well: the images are made as above, and
    `screen_images_bar` and `image_loss_bar` may both be used in one call.  Refusals are those of `screens=True`.

    `moment_targets=` (both beam classes, every mode above): the loss nearly every tuning loop writes, a weighted sum of squared
    distances of named beam properties at named points to target values, evaluated on the device from the states the trace left
    there -- no cotangent array with a point axis is made on the host or uploaded:

        targets = lynx_amd.grad.MomentTargets({"M1": {"beta_x": 4.0, "beta_y": 2.0}, -1: {"alpha_x": 0.0}},
                                              weights={"M1": {"beta_x": 0.25}})      # uploaded once, reusable over a loop
        vjp = lynx_amd.grad.track_along_vjp(segment, beam, moment_targets=targets)   # (or pass the dict of targets)
        vjp.moment_loss                          # (*batch,) float64: sum of weight (value - target)^2 over `targets.terms`
        vjp.moment_values, vjp.moment_loss_of("M1")                                  # (*batch, T); one point's part
        g = vjp(moment_loss_bar=1.0)             # a scalar or (*batch,), alone or with any cotangent above
        g[segment.Q1]["k1"], g.energy

    A point is whatever `trace.index_of` takes, a property one of `MOMENT_PROPERTIES` (the 23 names `trace_property_cotangents`
    has a rule for), a target or weight a scalar or broadcastable to (*batch,); a missing weight is 1.  The value of a term is
    the float64 expression that `trace_property_cotangents` differentiates, formed from the device states -- NOT the trace's
    property rounded to the beam's dtype: of a ParticleBeam's record sigma_c^2 = rec[cov_cc] n / (n - ddof) with the record's
    own count n and `config.std_ddof` (a lone survivor's variance is the record's, not the 0 the trace shows), of a
    ParameterBeam sigma_c^2 = max(cov_cc, 1e-20) with derivative 0 where clamped; emittance = sqrt(max(sigma^2 sigma_p^2 -
    sigma_xxp^2, tiny)), derivative 0 where clamped, beta = sigma^2 / emittance, alpha = -sigma_xxp / emittance,
    normalized_emittance = emittance gamma sqrt(1 - 1 / gamma^2) (lynx_moments_along_loss, right behind the trace on its stream;
    lynx_moments_along_loss_backward in front of the sweep).  A target other than `energy` is refused where a moment cotangent is:
    on a ParticleBeam behind an active cavity without `cavities=True`, and with `losses=True` on a point no particle of some
    sample reaches.  May be given together with `image_targets=` and `screens=`.

    `cavities=True` (a ParticleBeam): active cavities are no obstacle to the moment cotangents.  Behind a cavity's kick the
    moments are not a function of the moments in front of it, so the reverse call takes a second pass over the particles
    (lynx_track_particles_along_backward_cavities: the sweep of `track_vjp`, which parks every 4th state and walks back
    through the kicks, with the moment cotangent of every point given to every particle at that point):

        vjp = lynx_amd.grad.track_along_vjp(segment, beam, cavities=True)
        g = vjp(sigma_x=w, sigma_y=w)            # or mu_bar, cov_bar, energy_bar, readings=, any property of the trace
        g[segment.Q1]["k1"], g[segment.CAV]["voltage"], g.energy
        g = vjp(sigma_x=w, wrt_particles=True)   # g.particles (*batch, N, 7), device-resident

    `g.mu` and `g.cov` are None (the gradient is no function of the incoming moments).  One call instead of one
    `track_vjp` per point on a prefix of the lattice.  At most 64 leaf elements; not together with `trajectories=` or
    `losses=True`.  A lattice without a cavity is accepted (the same gradients by another way), and with a ParameterBeam
    `cavities=True` is the plain call.
    """
    return TrackAlongVJP(segment, beam, trajectories, losses, screens, cavities, image_targets, moment_targets)


# -------------------------------------------------------------------------------------------
# forward mode: tangents of the beam ALONG the lattice
# -------------------------------------------------------------------------------------------

ENERGY_ROW = 8  # kGradParams: the row of a direction's entry that stands for the energy at that step


def _jvp_directions(leaves, wrt, cavities=False):
    """
    `wrt` of `track_along_jvp` against the leaf elements of a lattice, refused by value -> the directions in the CSR form
    lynx_track_*_along_forward reads: (dir_start (D + 1,) int32, dir_leaf (n,) int32, dir_row (n,) int32, dir_weight (n,)
    float64).  An item is `(element, "name")`, `(element, "misalignment", 0 | 1)` or the string "energy".  An element object
    that occurs several times has an entry per place; `RBend.angle` also feeds e1 and e2 with weight 1/2 (the rule of
    `Gradients.__getitem__`); "energy" is one entry per leaf.

    `cavities` (lynx_track_moments_along_forward_cavities): `voltage`, `phase` and `frequency` of a Cavity that is an active
    step of the trace's program are directions too, and a direction that holds the voltage or the phase of such a cavity gets
    one energy entry of weight 1 per leaf BEHIND the first of them -- the energy there, and with it every later map, moves
    with the direction; the device scales the entry by the energy's own tangent at that leaf.
    """
    from .accelerator.magnets import Cavity, RBend

    wrt = list(wrt)
    if not wrt:
        raise ValueError("track_along_jvp: wrt is empty -- name at least one (element, parameter) or 'energy'")
    start, entries = [0], []
    for item in wrt:
        if isinstance(item, str):
            if item != "energy":
                raise KeyError(f"track_along_jvp: {item!r} -- the only direction given by a string is 'energy'")
            entries += [(e, ENERGY_ROW, 1.0) for e in range(len(leaves))]
            start.append(len(entries))
            continue
        if not isinstance(item, tuple) or len(item) not in (2, 3) or not isinstance(item[1], str):
            raise TypeError(f"track_along_jvp: an item of wrt is (element, 'name'), (element, 'misalignment', 0 | 1) or 'energy', not {item!r}")
        element, name = item[0], item[1]
        places = [e for e, el in enumerate(leaves) if el is element]
        if not places:
            raise KeyError(f"track_along_jvp: {element!r} is not an element of this lattice")
        rows = element._row_names() if element._kind in DIFFERENTIABLE_KINDS else []
        vector = name + "_x" in rows
        if vector and (len(item) != 3 or item[2] not in (0, 1)):
            raise ValueError(f"track_along_jvp: {name!r} of {element!r} has two components -- name one: (element, {name!r}, 0 | 1)")
        if not vector and len(item) == 3 and name in rows:
            raise ValueError(f"track_along_jvp: {name!r} of {element!r} has one component, {item!r} names one of several")
        slot = name + ("_x", "_y")[item[2]] if vector else name
        if slot not in rows:
            raise KeyError(f"track_along_jvp: {type(element).__name__} {element.name!r} has no differentiable parameter {name!r} "
                           f"(it has {sorted(set(r.rsplit('_x', 1)[0].rsplit('_y', 1)[0] for r in rows))})")
        active = isinstance(element, Cavity) and cavities and not element.is_skippable  # (a cavity step of the trace's program)
        if isinstance(element, Cavity) and name != "length" and not active:
            raise NotImplementedError(f"track_along_jvp: {name!r} of Cavity {element.name!r} -- the energy behind a cavity, and with "
                                      "it every later map, depends on it; cavities are not differentiated in forward mode yet")
        feeds = [(rows.index(slot), 1.0)]
        if isinstance(element, RBend) and name == "angle":  # e1 = e1_user + angle/2, e2 = e2_user + angle/2 (rbend.py:79-80)
            feeds += [(rows.index("e1"), 0.5), (rows.index("e2"), 0.5)]
        entries += [(e, row, weight) for e in places for row, weight in feeds]
        if active and name in ("voltage", "phase"):
            entries += [(e, ENERGY_ROW, 1.0) for e in range(places[0] + 1, len(leaves))]
        start.append(len(entries))
    return (np.array(start, dtype=np.int32), np.array([e for e, _, _ in entries], dtype=np.int32),
            np.array([r for _, r, _ in entries], dtype=np.int32), np.array([w for _, _, w in entries], dtype=np.float64))


def _jvp_program(segment, beam, cavities=False):
    """Every refusal of `track_along_jvp` about the beam and the lattice, before anything touches the GPU -> (program, leaves)."""
    from .particles.parameter_beam import ParameterBeam

    if not isinstance(beam, (ParameterBeam, ParticleBeam)):
        raise TypeError(f"track_along_jvp needs a ParticleBeam or a ParameterBeam, not {type(beam)}")
    if not isinstance(cavities, (bool, np.bool_)):
        raise ValueError(f"track_along_jvp: cavities is True or False, not {cavities!r}")
    leaves = list(segment._leaves() if hasattr(segment, "_leaves") else [segment])
    program = engine._trace_plan(segment, leaves)  # (raises for an active Screen or Aperture, naming it)
    for kind, first, _ in program.steps:
        if kind == _ffi.STEP_CAVITY and cavities:
            if isinstance(beam, ParticleBeam):
                raise NotImplementedError(
                    f"track_along_jvp: active Cavity {leaves[first].name!r} with a ParticleBeam -- its moments are not closed "
                    "under a cavity's kick, and forward mode makes no pass over the particles; a ParameterBeam of the same "
                    "moments is differentiated (track_along_vjp(..., cavities=True) differentiates this beam in reverse mode)")
        elif kind == _ffi.STEP_CAVITY:
            raise NotImplementedError(
                f"track_along_jvp: active Cavity {leaves[first].name!r} -- behind a cavity the energy, and with it every later "
                "map, depends on the cavity's parameters, and a ParticleBeam's moments are not closed under its kick; "
                "forward-mode tangents through cavities are not offered yet (track_along_vjp differentiates such a lattice)")
    return program, leaves


class TrackAlongJVP:
    """
    Jacobian-vector products of `Segment.track_along` (lynx_track_moments_along_forward / lynx_track_particles_along_forward):
    the tangents of the beam's mean and covariance at EVERY point of the lattice along each direction of `wrt` -- the shape
    reverse mode does not have: few parameters, every output.  Without a kicking cavity every element is an affine map, so
    one forward sweep of the moment recursion over the trace's states serves both beam classes, and no particle is tracked
    a second time.  The sweep runs when the object is made; the tangents stay on the device until they are asked for.

    A parameter given per sample has its tangent per sample; one shared by the batch (shape (1,)) gives every sample the
    tangent with respect to the shared value.

    `cavities=True` (a ParameterBeam; lynx_track_moments_along_forward_cavities): active cavities are steps of the sweep -- the
    tangent of the cavity branch follows a gaining cavity's products, every map is differentiated at its own step's energy, and
    a direction carries the energy's tangent with it (`energy_dot`, per sample, direction and point).
    """

    def __init__(self, segment, beam, wrt, cavities=False):
        self.program, self.leaves = _jvp_program(segment, beam, cavities)
        self.wrt = list(wrt)
        self._directions = _jvp_directions(self.leaves, self.wrt, bool(cavities))
        # through cavity steps only where there is one: a lattice without takes the plain path, bit for bit
        self._kicks = bool(cavities) and any(kind == _ffi.STEP_CAVITY for kind, _, _ in self.program.steps)
        self.segment, self.beam = segment, beam
        self.trace = engine.track_along(segment, self.leaves, beam, keep_outgoing=True, keep_device=True)
        rt = get_runtime()
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B, D, P = int(np.prod(batch_shape, dtype=np.int64)), len(self.wrt), self.trace.num_points
        lat = engine._ready(engine.trace_cache(segment), self.program, batch_shape, dtype, beam._energy._host)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        self._mu_dot_dev, self._cov_dot_dev = rt.empty((B, D, P, 7), np.float64), rt.empty((B, D, P, 7, 7), np.float64)
        start, leaf, row, weight = self._directions
        as_ints = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        directions = (as_ints(start), as_ints(leaf), as_ints(row), weight.ctypes.data_as(C.POINTER(C.c_double)), D, len(leaf))
        states = self.trace._device
        self._energy_dot_dev = self._energy_dot = None
        if self._kicks:
            seed = np.array([1.0 if isinstance(item, str) else 0.0 for item in self.wrt])
            self._energy_dot_dev = rt.empty((B, D, P), np.float64)
            rt.check(rt.lib.lynx_track_moments_along_forward_cavities(
                rt.ctx, lat.handle, _p(e_in), _p(states["mu"]), _p(states["cov"]), *directions, _p(self._mu_dot_dev),
                _p(self._cov_dot_dev), seed.ctypes.data_as(C.POINTER(C.c_double)), _p(self._energy_dot_dev)))
        elif isinstance(beam, ParticleBeam):
            rt.check(rt.lib.lynx_track_particles_along_forward(
                rt.ctx, lat.handle, beam.num_particles, _p(e_in), _p(states["records"]), *directions, _p(self._mu_dot_dev),
                _p(self._cov_dot_dev)))
        else:
            rt.check(rt.lib.lynx_track_moments_along_forward(
                rt.ctx, lat.handle, _p(e_in), _p(states["mu"]), _p(states["cov"]), *directions, _p(self._mu_dot_dev),
                _p(self._cov_dot_dev)))
        self._mu_dot = self._cov_dot = None

    @property
    def mu_dot(self) -> np.ndarray:
        """(*batch, D, P, 7) float64: the tangent of the mean at every point along every direction; entry 6 is an exact zero."""
        if self._mu_dot is None:
            self._mu_dot = self._mu_dot_dev.numpy().reshape(*self.beam.batch_shape, len(self.wrt), self.trace.num_points, 7)
        return self._mu_dot

    @property
    def cov_dot(self) -> np.ndarray:
        """(*batch, D, P, 7, 7) float64: the tangent of the covariance (a ParticleBeam's: the biased one); row and column 6 are
        exact zeros."""
        if self._cov_dot is None:
            self._cov_dot = self._cov_dot_dev.numpy().reshape(*self.beam.batch_shape, len(self.wrt), self.trace.num_points, 7, 7)
        return self._cov_dot

    @property
    def energy_dot(self) -> np.ndarray:
        """(D,): the tangent of the energy at every point -- without a cavity the incoming one: 1 along "energy", 0 otherwise.
        Through cavity steps (`cavities=True` on a lattice that has one): (*batch, D, P) float64, read from the device."""
        if self._kicks:
            if self._energy_dot is None:
                self._energy_dot = self._energy_dot_dev.numpy().reshape(*self.beam.batch_shape, len(self.wrt), self.trace.num_points)
            return self._energy_dot
        return np.array([1.0 if isinstance(item, str) else 0.0 for item in self.wrt])

    def tangent(self, name: str) -> np.ndarray:
        """
        (*batch, D, P) float64: the tangent of a property of the trace -- any of the 23 names `trace_property_cotangents` has a
        rule for -- as the contraction of that rule's output for a unit cotangent with `mu_dot`, `cov_dot` and the energy's
        tangent: the formulas are the reverse pass's own.  "energy" is exact: 1 along the "energy" direction, 0 otherwise.
        """
        shape = (*self.beam.batch_shape, len(self.wrt), self.trace.num_points)
        energy_dot = self.energy_dot if self._kicks else self.energy_dot[:, None]
        if name == "energy":
            return np.broadcast_to(energy_dot, shape).copy()
        mu_bar, cov_bar, energy_bar = trace_property_cotangents(self.trace, {name: 1.0})
        out = np.einsum("...pi,...dpi->...dp", mu_bar, self.mu_dot) + np.einsum("...pij,...dpij->...dp", cov_bar, self.cov_dot)
        if name in _ENERGY_PROPERTIES:
            out = out + energy_bar[..., None, :] * energy_dot
        return out

    def reading_tangents(self, bpm) -> np.ndarray:
        """(*batch, D, 2) float64: the tangent of a BPM's reading, the centroid (x, y) of the beam ENTERING it (the rule of
        `_add_reading`); the BPM need not be active.  Of a BPM placed several times: at its first place."""
        points = [k for k, el in enumerate(self.leaves) if el is bpm]
        if not points:
            raise KeyError(f"{bpm!r} is not an element of this lattice")
        return np.ascontiguousarray(self.mu_dot[..., points[0], :][..., (0, 2)])


def track_along_jvp(segment, beam, wrt, cavities=False):
    """
    Forward pass of `segment.track_along(beam)` (the trace is `jvp.trace`) and, right behind it, the forward-mode sweep: the
    tangents of the moments at every point along every direction of `wrt`:

        jvp = lynx_amd.grad.track_along_jvp(segment, beam, [(segment.Q3, "k1"), (segment.Q1, "misalignment", 0), "energy"])
        jvp.mu_dot, jvp.cov_dot                  # (*batch, D, P, 7), (*batch, D, P, 7, 7) float64
        jvp.tangent("beta_x")                    # (*batch, D, P): how beta_x at every point moves with each of them
        jvp.reading_tangents(segment.BPM1)       # (*batch, D, 2)

    An item of `wrt` is `(element, "name")`, `(element, "misalignment", 0 | 1)` or "energy" (the incoming beam energy).  Both
    beam classes, both dtypes; the tangents are float64.  Refused before anything touches the GPU: a lattice with a Cavity
    that has voltage, an active Screen or Aperture, a parameter the element does not have, an element that is not in the
    lattice, an empty `wrt`.  The cost is one sweep per direction, each as long as ONE reverse sweep: where reverse mode
    needs a call per output (a BPM and plane, a point of a curve), this needs a direction per parameter.

    `cavities=True` (a ParameterBeam): a lattice with cavities that have voltage is differentiated, too -- a linac's response
    matrix.  `(cavity, "voltage" | "phase" | "frequency")` of such a cavity are directions; `jvp.energy_dot` is then
    (*batch, D, P), the tangent of the beam energy at every point.  A ParticleBeam on such a lattice is refused (its moments
    are not closed under the kick); a lattice without an active cavity takes the plain path for both beam classes.
    """
    return TrackAlongJVP(segment, beam, wrt, cavities)


class OrbitResponseMatrix:
    """`matrix` (*batch, 2 n_bpm, n_corr): d(reading)/d(angle), the x rows first, then y; `bpms`, `correctors` in the order of
    its rows and columns; `jvp`, the `TrackAlongJVP` it was read from."""

    def __init__(self, matrix, bpms, correctors, jvp):
        self.matrix, self.bpms, self.correctors, self.jvp = matrix, bpms, correctors, jvp


def orbit_response_matrix(segment, beam, bpms=None, correctors=None, cavities=False) -> OrbitResponseMatrix:
    """
    The orbit response matrix of a lattice, in ONE forward-mode call: d(reading of every BPM)/d(angle of every corrector),
    what orbit correction by pseudo-inverse starts from.  By default every BPM and every HorizontalCorrector /
    VerticalCorrector of the flattened lattice, in lattice order.  A BPM need not be active: its reading is the centroid of
    the beam entering it.  A BPM in front of a corrector reads an exact 0.  `cavities=True` (a ParameterBeam): through
    accelerating cavities, as `track_along_jvp` takes it -- the response behind a cavity is damped by its map, and the energy
    behind it sets every later one.
    """
    from .accelerator.diagnostics import BPM
    from .accelerator.magnets import HorizontalCorrector, VerticalCorrector

    leaves = list(segment._leaves() if hasattr(segment, "_leaves") else [segment])

    def unique(kinds):
        return list({id(el): el for el in leaves if isinstance(el, kinds)}.values())

    bpms = unique(BPM) if bpms is None else list(bpms)
    correctors = unique((HorizontalCorrector, VerticalCorrector)) if correctors is None else list(correctors)
    if not bpms or not correctors:
        raise ValueError(f"orbit_response_matrix: {len(bpms)} BPMs and {len(correctors)} correctors -- the matrix needs one of each")
    for bpm in bpms:
        if not any(el is bpm for el in leaves):
            raise KeyError(f"orbit_response_matrix: {bpm!r} is not an element of this lattice")
    jvp = track_along_jvp(segment, beam, [(corrector, "angle") for corrector in correctors], cavities)
    readings = np.stack([jvp.reading_tangents(bpm) for bpm in bpms], axis=-3)  # (*batch, n_bpm, D, 2)
    matrix = np.concatenate([readings[..., 0], readings[..., 1]], axis=-2)
    return OrbitResponseMatrix(np.ascontiguousarray(matrix), bpms, correctors, jvp)


def track_vjp(segment, beam):
    """Forward pass through `segment`; returns the callable vector-Jacobian product."""
    from .particles.parameter_beam import ParameterBeam

    if isinstance(beam, ParameterBeam):
        return MomentsVJP(segment, beam)
    return TrackVJP(segment, beam)
