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

    def __init__(self, program, raw_dev, energy_dev, batch_shape, energy_shape, particles_dev=None,
                 mu_dev=None, cov_dev=None, chosen_dev=None, survivors: bool = False, screens=(), screen_shifts_dev=None,
                 through_kicks: bool = False):
        self._program, self._raw_dev, self._energy_dev = program, raw_dev, energy_dev
        self._survivors = survivors  # of `track_along_vjp(..., losses=True)`: no single incoming set of particles
        # of `track_along_vjp(..., cavities=True)` on a ParticleBeam: behind a kick the gradient is no function of the
        # incoming moments -- `mu`, `cov` are None, `particles` (if asked for) is what there is
        self._through_kicks = through_kicks
        self._particles_dev = particles_dev
        self._mu_dev, self._cov_dev = mu_dev, cov_dev
        self._chosen_dev = chosen_dev
        # of `track_along_vjp(..., screens=True)`: the trace's active screens and dL/d(misalignment) [B][screens][2] on the
        # device (None: no image took a cotangent)
        self._screens, self._screen_shifts_dev = list(screens), screen_shifts_dev
        self._batch_shape, self._energy_shape = tuple(batch_shape), tuple(energy_shape)
        self._raw = None
        self._cache = {}

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
        if self._survivors or self._through_kicks:
            return None
        if self._mu_dev is None:
            raise KeyError("the gradient w.r.t. mu exists for ParameterBeam VJPs only")
        return self._mu_dev.numpy()

    @property
    def cov(self) -> np.ndarray:
        """dL/d(incoming cov), (*batch, 7, 7), entry by entry -- ParameterBeam VJPs only; None like `mu`."""
        if self._survivors or self._through_kicks:
            return None
        if self._cov_dev is None:
            raise KeyError("the gradient w.r.t. cov exists for ParameterBeam VJPs only")
        return self._cov_dev.numpy()

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
        if self._survivors and any(el is element for _, el, _ in self._program.apertures):
            return True
        if any(el is element for el in self._screens):
            return True
        return any(el is element and el._kind in DIFFERENTIABLE_KINDS for el in self._program.leaves)

    def __getitem__(self, element) -> dict:
        if id(element) in self._cache:
            return self._cache[id(element)]
        from .accelerator.magnets import RBend

        if self._survivors and any(el is element for _, el, _ in self._program.apertures):
            # the survivor set is held fixed: the limits that made it get gradient 0
            return {n: np.zeros(np.asarray(getattr(element, n)).shape) for n in ("x_max", "y_max")}
        for k, el in enumerate(self._screens):
            if el is element:  # the image sees mu_x - misalignment[0], mu_y - misalignment[1]: minus the mu cotangent there
                shape = np.asarray(el.misalignment).shape
                if self._screen_shifts_dev is None:
                    return {"misalignment": np.zeros(shape)}
                shifts = self._screen_shifts_dev.numpy().reshape(*self._batch_shape, len(self._screens), 2)
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


def property_cotangents(outgoing: ParticleBeam, named: dict):
    """
    Cotangents of named beam properties -> (mu_bar, cov_bar).  `mu_<c>`: the mean itself;
    `sigma_<c>` = sqrt(cov_cc n / (n - ddof)) (particle_beam.py:736-823, `config.std_ddof`), so
    d sigma / d cov_cc = n / (n - ddof) / (2 sigma); `sigma_xxp`, `sigma_yyp`: cov_01, cov_23.
    """
    from . import config

    batch = outgoing.batch_shape
    mu_bar, cov_bar = np.zeros((*batch, 6)), np.zeros((*batch, 6, 6))
    n = float(outgoing.num_particles)
    for name, bar in named.items():
        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), batch)
        kind, _, coord = name.partition("_")
        if kind == "mu" and coord in _COORDINATES:
            mu_bar[..., _COORDINATES.index(coord)] += bar
        elif kind == "sigma" and coord in _COORDINATES:
            c = _COORDINATES.index(coord)
            sigma = np.asarray(getattr(outgoing, name), dtype=np.float64)
            cov_bar[..., c, c] += bar * (n / (n - config.std_ddof)) / (2.0 * sigma)
        elif name in ("sigma_xxp", "sigma_yyp"):
            c = 0 if name == "sigma_xxp" else 2
            cov_bar[..., c, c + 1] += bar
        else:
            raise KeyError(f"no cotangent rule for beam property {name!r}")
    return mu_bar, cov_bar


def _reading_cotangents(program, readings: dict, batch_shape) -> np.ndarray | None:
    """
    `{bpm: cotangent of bpm.reading}` -> [B][observers][2] float64 in the order the program reads them.  A BPM's reading
    is `stack([mu_x, mu_y])` of the beam that enters it (bpm.py:48-54), shape (2, *batch): so is its cotangent.
    """
    if not readings:
        return None
    B = int(np.prod(batch_shape, dtype=np.int64))
    out = np.zeros((B, len(program.observers), 2), dtype=np.float64)
    known = {id(element): k for k, (_, element) in enumerate(program.observers)}
    for element, bar in readings.items():
        if id(element) not in known:
            raise KeyError(f"{element!r} is not an active BPM of this lattice")
        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), (2, *batch_shape))
        out[:, known[id(element)], 0] += bar[0].reshape(B)
        out[:, known[id(element)], 1] += bar[1].reshape(B)
    return out


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
        self.cache = segment.__dict__.setdefault("_lattice_cache", engine.LatticeCache())
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
        B = int(np.prod(batch_shape, dtype=np.int64))
        if properties:
            extra_mu, extra_cov = property_cotangents(self.outgoing, properties)
            mu_bar = extra_mu if mu_bar is None else extra_mu + np.asarray(mu_bar, dtype=np.float64).reshape(extra_mu.shape)
            cov_bar = extra_cov if cov_bar is None else extra_cov + np.asarray(cov_bar, dtype=np.float64).reshape(extra_cov.shape)
        rec = np.zeros((B, _ffi.MOMENT_STRIDE), dtype=np.float64)
        if mu_bar is not None:
            mu_bar = np.asarray(mu_bar, dtype=np.float64).reshape(B, -1)
            rec[:, : mu_bar.shape[1]] = mu_bar
        if cov_bar is not None:
            G = np.asarray(cov_bar, dtype=np.float64).reshape(B, 6, 6)
            for i in range(6):
                rec[:, _tri(i, i)] = G[:, i, i]
                for j in range(i + 1, 6):
                    rec[:, _tri(i, j)] = G[:, i, j] + G[:, j, i]
        lat = engine._ready(self.cache, program, batch_shape, dtype, beam._energy._host)
        E = lat.E
        # (cotangents in and gradients out: small ones live in host memory the GPU reads and writes through)
        g_rec = rt.to_device_result(rec)
        g_par = rt.empty_result((B, max(E, 1), 8), dtype)
        g_en = rt.empty_result((B,), dtype)
        g_p = rt.empty((*batch_shape, beam.num_particles, 7), dtype) if wrt_particles else None
        fwd = self.outgoing._moments.device(rt)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        obs_bar = _reading_cotangents(program, readings, batch_shape)
        g_obs = None if obs_bar is None else rt.to_device_result(obs_bar)  # (named: alive until the call has been enqueued)
        rt.check(rt.lib.lynx_track_particles_backward(
            rt.ctx, lat.handle, beam.num_particles, C.c_void_p(e_in.ptr), C.c_void_p(beam._particles.device(rt).ptr),
            C.c_void_p(fwd.ptr), C.c_void_p(g_rec.ptr), C.c_void_p(g_par.ptr), C.c_void_p(g_en.ptr),
            None if g_p is None else C.c_void_p(g_p.ptr), None if g_obs is None else C.c_void_p(g_obs.ptr)))
        return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, g_p)


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
        self.cache = segment.__dict__.setdefault("_lattice_cache", engine.LatticeCache())
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

    def _property_cotangents(self, named: dict):
        """`mu_<c>`: mu[c]; `sigma_<c>` = sqrt(max(cov_cc, 1e-20)) (parameter_beam.py:371-417); `sigma_xxp/yyp`: cov_01, cov_23."""
        out = self.outgoing
        batch = out.batch_shape
        mu_bar, cov_bar = np.zeros((*batch, 7)), np.zeros((*batch, 7, 7))
        for name, bar in named.items():
            bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), batch)
            kind, _, coord = name.partition("_")
            if kind == "mu" and coord in _COORDINATES:
                mu_bar[..., _COORDINATES.index(coord)] += bar
            elif kind == "sigma" and coord in _COORDINATES:
                c = _COORDINATES.index(coord)
                var = np.asarray(out._cov, dtype=np.float64)[..., c, c]
                cov_bar[..., c, c] += np.where(var > 1e-20, bar / (2.0 * np.sqrt(np.maximum(var, 1e-20))), 0.0)
            elif name in ("sigma_xxp", "sigma_yyp"):
                c = 0 if name == "sigma_xxp" else 2
                cov_bar[..., c, c + 1] += bar
            else:
                raise KeyError(f"no cotangent rule for beam property {name!r}")
        return mu_bar, cov_bar

    def _stretch(self, program, beam, mb, cb) -> Gradients:
        rt = get_runtime()
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B = int(np.prod(batch_shape, dtype=np.int64))
        lat = engine._ready(self.cache, program, batch_shape, dtype, beam._energy._host)
        g_par = rt.empty((B, max(lat.E, 1), 8), dtype)
        g_en = rt.empty((B,), dtype)
        g_mu = rt.empty((*batch_shape, 7), dtype)
        g_cov = rt.empty((*batch_shape, 7, 7), dtype)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        p = lambda a: C.c_void_p(a.ptr)  # noqa: E731
        # named, so that both uploads stay allocated until the call has been enqueued
        mb_dev, cb_dev = rt.to_device(mb.astype(dtype)), rt.to_device(cb.astype(dtype))
        rt.check(rt.lib.lynx_track_moments_backward(
            rt.ctx, lat.handle, p(e_in), p(beam._mu_d.device(rt)), p(beam._cov_d.device(rt)),
            p(mb_dev), p(cb_dev), p(g_par), p(g_en), p(g_mu), p(g_cov)))
        return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, mu_dev=g_mu, cov_dev=g_cov)

    def __call__(self, mu_bar=None, cov_bar=None, readings: dict | None = None, **properties):
        """
        `mu_bar` (*batch, <=7), `cov_bar` (*batch, 6|7, 6|7): cotangents entry by entry; `readings={bpm: bar}`: cotangents
        of the readings of active BPMs, shaped like `bpm.reading` -- (2, *batch).
        """
        batch_shape = self.outgoing.batch_shape
        B = int(np.prod(batch_shape, dtype=np.int64))
        mb, cb = np.zeros((B, 7)), np.zeros((B, 7, 7))
        if properties:
            pm, pc = self._property_cotangents(properties)
            mb += pm.reshape(B, 7)
            cb += pc.reshape(B, 7, 7)
        if mu_bar is not None:
            mu_bar = np.asarray(mu_bar, dtype=np.float64).reshape(B, -1)
            mb[:, : mu_bar.shape[1]] += mu_bar
        if cov_bar is not None:
            cov_bar = np.asarray(cov_bar, dtype=np.float64)
            k = cov_bar.shape[-1]
            cb[:, :k, :k] += cov_bar.reshape(B, k, k)
        readings = dict(readings or {})
        known = {id(item): item for item, beam in self.stretches if beam is None}
        for element in readings:
            if id(element) not in known:
                raise KeyError(f"{element!r} is not an active BPM of this lattice")
        parts = []
        for item, beam in reversed(self.stretches):
            if beam is None:  # an active BPM: its reading is (mu_x, mu_y) of the beam passing here
                for element, bar in readings.items():
                    if element is item:
                        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), (2, *batch_shape))
                        mb[:, 0] += bar[0].reshape(B)
                        mb[:, 2] += bar[1].reshape(B)
                continue
            part = self._stretch(item, beam, mb, cb)
            parts.insert(0, part)
            mb, cb = np.asarray(part.mu, dtype=np.float64).reshape(B, 7), np.asarray(part.cov, dtype=np.float64).reshape(B, 7, 7)
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

    for name, bar in named.items():
        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), shape)
        kind, _, coord = name.partition("_")
        if name == "energy":
            energy_bar += bar
        elif kind == "mu" and coord in _COORDINATES:
            mu_bar[..., _COORDINATES.index(coord)] += bar
        elif kind == "sigma" and coord in _COORDINATES:
            c = _COORDINATES.index(coord)
            s2, ds2 = sigma_squared(c)
            with np.errstate(all="ignore"):
                cov_bar[..., c, c] += np.where(ds2 != 0, bar * ds2 / (2.0 * np.sqrt(s2)), 0.0)
        elif name in ("sigma_xxp", "sigma_yyp"):
            plane(0 if name == "sigma_xxp" else 2)["cross"] += bar
        elif name in ("emittance_x", "emittance_y"):
            emittance_bar(0 if name.endswith("x") else 2, bar)
        elif name in ("normalized_emittance_x", "normalized_emittance_y"):
            a = 0 if name.endswith("x") else 2
            gamma = np.asarray(trace.energy, dtype=np.float64) / engine.ELECTRON_MASS_EV
            moving = np.abs(gamma) > 0
            with np.errstate(all="ignore"):
                bg = np.where(moving, np.sqrt(1 - 1 / gamma**2) * gamma, 0.0)  # relativistic beta . gamma
                dbg = np.where(moving, gamma / np.sqrt(gamma**2 - 1), 0.0) / engine.ELECTRON_MASS_EV
            emittance_bar(a, bar * bg)
            energy_bar += bar * emittance(a)[0] * dbg
        elif name in ("beta_x", "beta_y"):
            a = 0 if name.endswith("x") else 2
            eps, _, s2, _, _ = emittance(a)
            plane(a)["s2"] += bar / eps
            emittance_bar(a, -bar * s2 / eps**2)
        elif name in ("alpha_x", "alpha_y"):
            a = 0 if name.endswith("x") else 2
            eps, _, _, _, cross = emittance(a)
            plane(a)["cross"] += -bar / eps
            emittance_bar(a, bar * cross / eps**2)
        else:
            raise KeyError(f"no cotangent rule for trace property {name!r}")
    for a, acc in plane_bars.items():
        cov_bar[..., a, a] += acc["s2"] * sigma_squared(a)[1]
        cov_bar[..., a + 1, a + 1] += acc["p2"] * sigma_squared(a + 1)[1]
        cov_bar[..., a, a + 1] += acc["cross"]
    return mu_bar, cov_bar, energy_bar


def _record_cotangents(mb: np.ndarray, cb: np.ndarray) -> np.ndarray:
    """
    Cotangents of mean (B, P, 7) and covariance (B, P, 7, 7), entry by entry, as record cotangents (B, P, 36): [0..6] the
    mean's, [7..27] the upper triangle in the record's order (`_tri`), an off-diagonal entry counted once.
    """
    rec = np.zeros((*mb.shape[:2], _ffi.MOMENT_STRIDE), dtype=np.float64)
    rec[..., :7] = mb
    rows, cols = np.triu_indices(6)
    rec[..., 7:28] = (cb[..., rows, cols] + cb[..., cols, rows]) * np.where(rows == cols, 0.5, 1.0)
    return rec


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

    def __init__(self, segment, beam, trajectories=None, losses=False, screens=False, cavities=False):
        from .particles.parameter_beam import ParameterBeam

        if not isinstance(beam, (ParameterBeam, ParticleBeam)):
            raise TypeError(f"track_along_vjp needs a ParticleBeam or a ParameterBeam, not {type(beam)}")
        if not isinstance(losses, (bool, np.bool_)):
            raise ValueError(f"track_along_vjp: losses is True or False, not {losses!r}")
        if not isinstance(screens, (bool, np.bool_)):
            raise ValueError(f"track_along_vjp: screens is True or False, not {screens!r}")
        if not isinstance(cavities, (bool, np.bool_)):
            raise ValueError(f"track_along_vjp: cavities is True or False, not {cavities!r}")
        if cavities and (trajectories is not None or losses):
            raise NotImplementedError(
                "track_along_vjp: cavities=True together with " + ("trajectories=" if trajectories is not None else "losses=True")
                + " -- the second pass over the particles differentiates the moments of the whole beam alone; ask for one of "
                "the two")
        # the pass through the kicks: a ParticleBeam's (a ParameterBeam's recursion handles cavities as it is)
        self._through_kicks = bool(cavities) and isinstance(beam, ParticleBeam)
        if screens and isinstance(beam, ParticleBeam):
            raise TypeError(
                "track_along_vjp: screens=True with a ParticleBeam -- its screen image is a histogram of counts, a step "
                "function of the magnets whose gradient is zero almost everywhere; a ParameterBeam of the same moments "
                "(its image is a smooth density) is differentiated")
        self._screens = bool(screens)
        if losses and trajectories is not None:
            raise NotImplementedError(
                "track_along_vjp: losses=True together with trajectories= -- the trajectories of a trace with losses are "
                "not differentiated; ask for one of the two")
        # (by value, before anything touches the GPU; a ParameterBeam has no particles to choose: TypeError)
        self.chosen = None if trajectories is None else engine.chosen_particles(trajectories, beam)
        leaves = list(segment._leaves() if hasattr(segment, "_leaves") else [segment])
        # (raises for an active Screen -- and, without `losses`, for an active Aperture --, naming it, before anything
        # touches the GPU)
        self.program = engine._trace_plan(segment, leaves, bool(losses), True) if screens else engine._trace_plan(segment, leaves, bool(losses))
        B = int(np.prod(beam.batch_shape, dtype=np.int64))
        if screens and self.program.screens and B > _ffi.MAX_IMAGE_BATCH:  # (as lynx_gaussian_images_along refuses it)
            raise _ffi.LynxError(
                f"track_along_vjp: screens=True with a batch of {B} samples, more than {_ffi.MAX_IMAGE_BATCH} -- "
                "lynx_gaussian_images_along takes a sample per row of its launch grid (bad argument); trace the batch in parts")
        # the survivors' reverse pass: a ParticleBeam and at least one active aperture; anything else with `losses` is the
        # plain problem (apertures pass a ParameterBeam unchanged)
        self._sets = bool(losses) and isinstance(beam, ParticleBeam) and len(self.program.apertures) > 0
        if isinstance(beam, ParticleBeam) and not self._sets:
            losses = False  # (no active aperture: nobody is lost, the call is the plain one)
            self.program = engine._trace_plan(segment, leaves)
        if self._sets and len(self.program.apertures) > MAX_TRACE_LOSS_APERTURES:
            raise NotImplementedError(
                f"track_along_vjp: {len(self.program.apertures)} active apertures, more than {MAX_TRACE_LOSS_APERTURES} (the "
                f"first one beyond is {self.program.apertures[MAX_TRACE_LOSS_APERTURES][1].name!r}) -- differentiate the "
                "lattice in stretches")
        if len(leaves) > MAX_TRACE_LEAVES:
            raise NotImplementedError(
                f"track_along_vjp: {len(leaves)} leaf elements, more than {MAX_TRACE_LEAVES} (the first one beyond is "
                f"{leaves[MAX_TRACE_LEAVES].name!r}) -- differentiate the lattice in stretches")
        if self._through_kicks and len(leaves) > MAX_TRACE_CAVITY_LEAVES:
            raise NotImplementedError(
                f"track_along_vjp: cavities=True with {len(leaves)} leaf elements, more than {MAX_TRACE_CAVITY_LEAVES} (the first "
                f"one beyond is {leaves[MAX_TRACE_CAVITY_LEAVES].name!r}) -- differentiate the lattice in stretches")
        self._cavity = None  # the first active cavity in front of a ParticleBeam: no moment cotangent passes it
        if isinstance(beam, ParticleBeam) and not self._through_kicks:
            for kind, first, _ in self.program.steps:
                if kind == _ffi.STEP_CAVITY:
                    self._cavity = leaves[first].name
                    break
        if self._cavity is not None and self.chosen is None:
            self._refuse_moments()
        self.segment, self.beam, self.leaves = segment, beam, leaves
        self._set_records = None
        with_screens = {"screens": True} if screens else {}  # (a ParameterBeam's then; without it the call is the one it was)
        if self._sets:
            self.trace = engine.track_along(segment, leaves, beam, keep_outgoing=True, keep_device=True, losses="particles")
            self._set_records = self._survivor_set_records()
        elif losses:  # (a ParameterBeam: active apertures are identity steps of its trace)
            self.trace = engine.track_along(segment, leaves, beam, keep_outgoing=True, keep_device=True, losses=True, **with_screens)
        elif self.chosen is None:
            self.trace = engine.track_along(segment, leaves, beam, keep_outgoing=True, keep_device=True, **with_screens)
        else:
            self.trace = engine.track_along(segment, leaves, beam, keep_outgoing=True, keep_device=True, trajectories=self.chosen)

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
            rt.ctx, engine.dtype_code(beam.dtype), B, beam.num_particles, C.c_void_p(beam._particles.device(rt).ptr),
            _ffi.TRACK_SHARED_INPUT if beam.is_shared else 0, A, C.c_void_p(self.trace._device["lost_at"].ptr),
            C.c_void_p(records.ptr)))
        return records

    def _refuse_moments(self):
        raise NotImplementedError(
            f"track_along_vjp: active Cavity {self._cavity!r} -- the moments of a ParticleBeam are not "
            "closed under a cavity's kick; a ParameterBeam of the same lattice is differentiated, and so is this beam by a "
            "second pass over its particles: track_along_vjp(..., cavities=True)")

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
        batch_shape = self.beam.batch_shape
        P = self.trace.num_points
        B = int(np.prod(batch_shape, dtype=np.int64))
        mb, cb, eb = np.zeros((B, P, 7)), np.zeros((B, P, 7, 7)), np.zeros((B, P))
        # a trace with losses: the points no particle of a sample reaches have no moments (NaN) and take no cotangent
        dead = np.asarray(self.trace.num_survivors).reshape(B, P) == 0 if self._sets else np.zeros((B, P), dtype=bool)
        if properties and dead.any():
            for name, bar in properties.items():
                if name != "energy":
                    self._refuse_cotangent_on_nobody(np.broadcast_to(np.asarray(bar, dtype=np.float64), (*batch_shape, P)).reshape(B, P),
                                                     dead, repr(name))
            with np.errstate(all="ignore"):
                pm, pc, pe = trace_property_cotangents(self.trace, {n: v for n, v in properties.items() if n != "energy"})
            pm, pc, pe = pm.reshape(B, P, 7), pc.reshape(B, P, 7, 7), pe.reshape(B, P)
            pm[dead], pc[dead], pe[dead] = 0.0, 0.0, 0.0  # (0 x NaN of the rules above)
            mb += pm
            cb += pc
            eb += pe
            if "energy" in properties:
                eb += np.broadcast_to(np.asarray(properties["energy"], dtype=np.float64), (*batch_shape, P)).reshape(B, P)
        elif properties:
            pm, pc, pe = trace_property_cotangents(self.trace, properties)
            mb += pm.reshape(B, P, 7)
            cb += pc.reshape(B, P, 7, 7)
            eb += pe.reshape(B, P)
        if mu_bar is not None:
            mu_bar = np.asarray(mu_bar, dtype=np.float64)
            k = mu_bar.shape[-1]
            mb[..., :k] += np.broadcast_to(mu_bar, (*batch_shape, P, k)).reshape(B, P, k)
        if cov_bar is not None:
            cov_bar = np.asarray(cov_bar, dtype=np.float64)
            k = cov_bar.shape[-1]
            cb[..., :k, :k] += np.broadcast_to(cov_bar, (*batch_shape, P, k, k)).reshape(B, P, k, k)
        if energy_bar is not None:
            eb += np.broadcast_to(np.asarray(energy_bar, dtype=np.float64), (*batch_shape, P)).reshape(B, P)
        for element, bar in (readings or {}).items():
            points = [k for k, el in enumerate(self.leaves) if el is element and getattr(el, "_fusable_observer", False)]
            if not points:
                raise KeyError(f"{element!r} is not an active BPM of this lattice")
            bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), (2, *batch_shape))
            for k in points:  # an active BPM reads (mu_x, mu_y) of the beam that ENTERS it: point k (bpm.py:48-54)
                mb[:, k, 0] += bar[0].reshape(B)
                mb[:, k, 2] += bar[1].reshape(B)
        if dead.any():
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
        if not getattr(self, "_screens", False):
            raise ValueError("track_along_vjp: screen_images_bar needs the screen images of the forward trace -- pass "
                             "screens=True to track_along_vjp")
        if not isinstance(screen_images_bar, dict):
            raise TypeError(f"track_along_vjp: screen_images_bar is a dict {{screen: cotangent of its image}}, not {type(screen_images_bar)}")
        trace, elements = self.trace, [el for _, el in self.program.screens]
        named = []  # (screen, cotangent broadcast to its image), checked before anything is allocated
        for key, bar in screen_images_bar.items():
            if getattr(key, "_swallows_beam", False):  # the Screen element itself
                found = [k for k, el in enumerate(elements) if el is key]
                if not found:
                    raise KeyError(f"{key!r} is not an active screen of this trace (screens at {list(trace.screens)})")
                k = found[0]
            else:
                image = trace.image_at(key)  # (KeyError for anything but an active screen of the trace)
                k = next(n for n, own in enumerate(trace.screen_images) if own is image)
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
                 screen_images_bar: dict | None = None, wrt_particles: bool = False, **properties) -> Gradients:
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
        `wrt_particles=True` (`cavities=True` of `track_along_vjp`, a ParticleBeam): `Gradients.particles` (*batch, N, 7), the
        gradient w.r.t. every incoming particle, device-resident.
        """
        if wrt_particles and not getattr(self, "_through_kicks", False):
            raise ValueError("track_along_vjp: wrt_particles=True needs the pass over the particles -- a ParticleBeam and "
                             "cavities=True of track_along_vjp (without a cavity g.mu and g.cov say the same)")
        wi = None if screen_images_bar is None else self._image_cotangents(screen_images_bar)
        wb = None
        if trajectories_bar is not None:
            wb = self._trajectory_cotangents(trajectories_bar)
        elif self.chosen is not None:  # (the trace has trajectories: the same entry point, with no cotangent on them)
            wb = self._trajectory_cotangents(np.zeros(7))
        with_moments = (mu_bar is not None or cov_bar is not None or bool(readings)
                        or any(name != "energy" for name in properties))
        if with_moments and self._cavity is not None:
            self._refuse_moments()
        mb, cb, eb = self._cotangents(mu_bar, cov_bar, energy_bar, readings, properties)
        rt = get_runtime()
        beam, program = self.beam, self.program
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B, P = mb.shape[:2]
        cache = self.segment.__dict__.setdefault("_trace_cache", engine.LatticeCache())
        lat = engine._ready(cache, program, batch_shape, dtype, beam._energy._host)
        g_par = rt.empty((B, max(lat.E, 1), 8), dtype)
        g_en = rt.empty((B,), dtype)
        g_mu = rt.empty((*batch_shape, 7), dtype)
        g_cov = rt.empty((*batch_shape, 7, 7), dtype)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        p = lambda a: None if a is None else C.c_void_p(a.ptr)  # noqa: E731
        # named, so that the uploads stay allocated until the call has been enqueued
        eb_dev = rt.to_device(eb.astype(dtype)) if np.any(eb) else None
        states = self.trace._device
        if wb is not None:
            K = len(self.chosen)
            rec_dev = None
            if with_moments:
                rec_dev = rt.to_device(_record_cotangents(mb, cb))
            else:
                g_mu = g_cov = None
            wb_dev = rt.to_device(wb)
            g_chosen = rt.empty((*batch_shape, K, 7), dtype)
            rt.check(rt.lib.lynx_track_particles_along_backward_trajectories(
                rt.ctx, lat.handle, beam.num_particles, p(e_in), p(states["records"]) if with_moments else None, p(rec_dev),
                p(eb_dev), p(g_par), p(g_en), p(g_mu), p(g_cov), K, p(states["trajectories"]), p(wb_dev), p(g_chosen)))
            return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, mu_dev=g_mu, cov_dev=g_cov,
                             chosen_dev=g_chosen)
        if getattr(self, "_through_kicks", False):
            rec_dev = rt.to_device(_record_cotangents(mb, cb))
            g_p = rt.empty((*batch_shape, beam.num_particles, 7), dtype) if wrt_particles else None
            rt.check(rt.lib.lynx_track_particles_along_backward_cavities(
                rt.ctx, lat.handle, beam.num_particles, p(e_in), p(beam._particles.device(rt)),
                _ffi.TRACK_SHARED_INPUT if beam.is_shared else 0, p(states["records"]), p(rec_dev), p(eb_dev), p(g_par), p(g_en),
                p(g_p)))
            return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, particles_dev=g_p,
                             through_kicks=True)
        if self._sets:
            rec_dev = rt.to_device(_record_cotangents(mb, cb))
            A = len(program.apertures)
            at = (C.c_int32 * A)(*[step for step, _, _ in program.apertures])
            rt.check(rt.lib.lynx_track_particles_along_backward_losses(
                rt.ctx, lat.handle, beam.num_particles, p(e_in), p(states["records"]), p(rec_dev), p(eb_dev), A, at,
                p(self._set_records), p(g_par), p(g_en)))
            return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, survivors=True)
        if isinstance(beam, ParticleBeam):
            rec_dev = rt.to_device(_record_cotangents(mb, cb))
            rt.check(rt.lib.lynx_track_particles_along_backward(
                rt.ctx, lat.handle, beam.num_particles, p(e_in), p(states["records"]), p(rec_dev), p(eb_dev),
                p(g_par), p(g_en), p(g_mu), p(g_cov)))
        else:
            mb_dev, cb_dev = rt.to_device(mb.astype(dtype)), rt.to_device(cb.astype(dtype))
            shifts = None
            if wi is not None:  # the images' cotangents go into mb_dev, cb_dev at the screens' points, on the same stream
                shots = engine._screen_geometry(self.segment, program, batch_shape, dtype, rt, False)
                wi_dev = rt.to_device(np.ascontiguousarray(wi, dtype=dtype))
                shifts = rt.empty((B, shots["count"], 2), dtype)
                rt.check(rt.lib.lynx_gaussian_images_along_backward(
                    rt.ctx, engine.dtype_code(dtype), B, P, p(states["mu"]), p(states["cov"]), shots["count"], shots["rows"],
                    p(shots["grid"]), p(shots["misalignment"]), shots["stride"], p(wi_dev), p(mb_dev), p(cb_dev), p(shifts)))
            rt.check(rt.lib.lynx_track_moments_along_backward(
                rt.ctx, lat.handle, p(e_in), p(states["mu"]), p(states["cov"]), p(mb_dev), p(cb_dev), p(eb_dev),
                p(g_par), p(g_en), p(g_mu), p(g_cov)))
            if getattr(self, "_screens", False):
                return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, mu_dev=g_mu, cov_dev=g_cov,
                                 screens=[el for _, el in program.screens], screen_shifts_dev=shifts)
        return Gradients(program, g_par, g_en, batch_shape, np.asarray(beam.energy).shape, mu_dev=g_mu, cov_dev=g_cov)


def track_along_vjp(segment, beam, trajectories=None, losses=False, screens=False, cavities=False):
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
    return TrackAlongVJP(segment, beam, trajectories, losses, screens, cavities)


def track_vjp(segment, beam):
    """Forward pass through `segment`; returns the callable vector-Jacobian product."""
    from .particles.parameter_beam import ParameterBeam

    if isinstance(beam, ParameterBeam):
        return MomentsVJP(segment, beam)
    return TrackVJP(segment, beam)
