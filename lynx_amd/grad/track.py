"""
`track_vjp`: the vector-Jacobian product of `Segment.track` for both beam classes -- `TrackVJP` (a ParticleBeam: one call of
lynx_track_particles_backward, bound by the host) and `MomentsVJP` (a ParameterBeam: lynx_track_moments_backward per stretch
between active BPMs) --, and what every other pass of the package shares with them: `_p`, `leaves_of` and `_Sweep`.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi, device, engine
from ..particles.parameter_beam import ParameterBeam
from ..particles.particle_beam import ParticleBeam
from .cotangents import _known_bpm, _MomentCotangents, _add_reading, _reading_bar, _record_cotangents, batch_size, property_cotangents
from .gradients import ChainedGradients, Gradients


def _p(array):  # a device array, or None, as a library call takes it
    return None if array is None else C.c_void_p(array.ptr)


def leaves_of(segment) -> list:
    """The leaf elements of a lattice, in order: what a trace has a point behind each of; an element alone is its own lattice."""
    return list(segment._leaves() if hasattr(segment, "_leaves") else [segment])


class _Sweep:
    """What every sweep of the moment recursion is given besides its cotangents: lattice, incoming energy, outputs in HBM."""

    def __init__(self, rt, cache, program, beam):
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B = batch_size(batch_shape)
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
        rt = device.get_runtime()
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
        rt = device.get_runtime()
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


def track_vjp(segment, beam):
    """Forward pass through `segment`; returns the callable vector-Jacobian product."""
    if isinstance(beam, ParameterBeam):
        return MomentsVJP(segment, beam)
    return TrackVJP(segment, beam)
