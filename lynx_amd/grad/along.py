"""
`track_along_vjp`: the vector-Jacobian product of `Segment.track_along` in its five modes -- "moments" (a ParameterBeam's
sweep, with screen images and image targets), "particles", "trajectories", "survivors" (`losses=True`) and "kicks"
(`cavities=True`).  `_trace_mode` holds every refusal of the constructor by value; `TrackAlongVJP` makes the forward trace,
has the two losses of targets.py evaluated right behind it, assembles the call's cotangents and launches one sweep per call.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _ffi, device, engine
from ..particles.parameter_beam import ParameterBeam
from ..particles.particle_beam import ParticleBeam
from .cotangents import _add_reading, _known_bpm, _MomentCotangents, _record_cotangents, batch_size, broadcast_or_refuse, trace_property_cotangents
from .gradients import Gradients
from .targets import ImageLoss, ImageTargets, MomentLoss, MomentTargets, ScreenCalls, _screen_of, loss_of
from .track import _p, _Sweep, leaves_of

MAX_TRACE_LEAVES = 256  # lynx_track_*_along_backward: k_build_bwd deals the steps of a program to its 256 threads
MAX_TRACE_LOSS_APERTURES = 15  # lynx_track_particles_along_backward_losses: 16 survivor sets
MAX_TRACE_CAVITY_LEAVES = 64  # lynx_track_particles_along_backward_cavities: k_track_bwd parks the states of 16 groups of 4 steps


def _refuse_moments(cavity: str):
    raise NotImplementedError(
        f"track_along_vjp: active Cavity {cavity!r} -- the moments of a ParticleBeam are not "
        "closed under a cavity's kick; a ParameterBeam of the same lattice is differentiated, and so is this beam by a "
        "second pass over its particles: track_along_vjp(..., cavities=True)")


def _refuse_beyond(elements, limit, how_many):
    if len(elements) > limit:
        raise NotImplementedError(f"track_along_vjp: {how_many.format(len(elements))}, more than {limit} (the first one beyond is "
                                  f"{elements[limit].name!r}) -- differentiate the lattice in stretches")


def _trace_mode(segment, beam, trajectories, losses, screens, cavities):
    """
    Every refusal of `track_along_vjp` by value, before anything touches the GPU -> (mode, the trace's program, the leaf
    elements, the chosen particles or None, the name of the active cavity that stops this beam's moment cotangents or None).
    """
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
    leaves = leaves_of(segment)
    # (raises for an active Screen -- and, without `losses`, for an active Aperture --, naming it)
    program = engine._trace_plan(segment, leaves, bool(losses), True) if screens else engine._trace_plan(segment, leaves, bool(losses))
    B = batch_size(beam.batch_shape)
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
    if mode == "survivors":
        _refuse_beyond([el for _, el, _ in program.apertures], MAX_TRACE_LOSS_APERTURES, "{} active apertures")
    _refuse_beyond(leaves, MAX_TRACE_LEAVES, "{} leaf elements")
    if mode == "kicks":
        _refuse_beyond(leaves, MAX_TRACE_CAVITY_LEAVES, "cavities=True with {} leaf elements")
    # the first active cavity in front of a ParticleBeam: no moment cotangent passes it but through the kicks
    cavities_at = [first for kind, first, _ in program.steps if kind == _ffi.STEP_CAVITY] if particles and mode != "kicks" else []
    cavity = leaves[cavities_at[0]].name if cavities_at else None
    if cavity is not None and chosen is None:
        _refuse_moments(cavity)
    return mode, program, leaves, chosen, cavity


class TrackAlongVJP:
    """
    Vector-Jacobian product of `Segment.track_along`: gradients of any function of the beam moments and the energy at
    EVERY point of the lattice (lynx_track_moments_along_backward / lynx_track_particles_along_backward).  Without a
    kicking cavity every element is an affine map, so a ParticleBeam's mean and covariance obey the ParameterBeam's
    recursion: one reverse sweep of that recursion over the forward trace serves both beam classes, and no particle is
    tracked a second time.  What `trajectories=`, `losses=`, `screens=`, `cavities=` and the two kinds of targets add to
    that: `track_along_vjp`.
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
        self._targets = self._image_loss = self._moment_targets = self._moment_loss = None
        if targets:  # every refusal by value, before anything touches the GPU
            self._targets = image_targets if isinstance(image_targets, ImageTargets) else ImageTargets(image_targets)
            image_layout = self._targets._layout(self.program, self.leaves, beam)
        if moment_targets is not None:
            self._moment_targets = moment_targets if isinstance(moment_targets, MomentTargets) else MomentTargets(moment_targets)
            moment_layout = self._moment_targets._layout([el.name for el in self.leaves], beam.batch_shape)
        # (a keyword is given only where it says something; apertures are identity steps of a ParameterBeam's trace; with
        # image targets alone the screens are points of the trace and no image is made)
        plain = {**({"losses": True} if losses and self.mode == "moments" else {}),
                 **({"screens": True} if screens else {"screens": "points"} if targets else {})}
        options = {"survivors": {"losses": "particles"}, "trajectories": {"trajectories": self.chosen}}.get(self.mode, plain)
        if moment_targets is not None:  # (the moment loss reads the energies where the trace wrote them)
            options = {**options, "keep_energy": True}
        self.trace = engine.track_along(segment, self.leaves, beam, keep_outgoing=True, keep_device=True, **options)
        self._set_records = self._survivor_set_records() if self.mode == "survivors" else None
        # the image calls' shared head and the two losses, each evaluated right behind the trace, on its stream
        self._image_calls = ScreenCalls(segment, self.program, self.leaves, beam, self.trace)
        if targets:
            self._image_loss = ImageLoss(device.get_runtime(), self._targets, image_layout, self._image_calls)
        if moment_targets is not None:
            self._refuse_moment_targets(moment_layout)
            self._moment_loss = MomentLoss(device.get_runtime(), self._moment_targets, moment_layout, beam, self.trace)

    def _refuse_moment_targets(self, layout):
        """The refusals of moment targets that need the trace: exactly where a moment cotangent is refused."""
        if layout.moments and self._cavity is not None:
            _refuse_moments(self._cavity)
        if self.mode == "survivors":
            B, P = self._points_shape()
            dead = np.asarray(self.trace.num_survivors).reshape(B, P) == 0
            for point, name in layout.terms:
                if name != "energy" and dead[:, point].any():  # (the energy is there at every point)
                    self._refuse_cotangent_on_nobody(np.arange(P) == point, dead, repr(name))

    @property
    def image_loss(self) -> dict:
        """{screen name: (*batch,) float64}: the mean squared difference of every named screen's image to its target."""
        return loss_of(self._image_loss, "image_loss").values()

    def image_loss_of(self, screen) -> np.ndarray:
        """`image_loss` of one screen: by whatever `trace.image_at` takes, or by the `Screen` itself."""
        return loss_of(self._image_loss, "image_loss_of").of(screen)

    @property
    def moment_values(self) -> np.ndarray:
        """(*batch, T) float64: the value of every term of the moment loss, in the order of `MomentTargets.terms`."""
        return loss_of(self._moment_loss, "moment_values").values()

    @property
    def moment_loss(self) -> np.ndarray:
        """(*batch,) float64: the sum over the terms, in their order, of weight (value - target)^2."""
        return loss_of(self._moment_loss, "moment_loss").loss()

    def moment_loss_of(self, point) -> np.ndarray:
        """The part of `moment_loss` that one point's terms make: by whatever `trace.index_of` takes."""
        return loss_of(self._moment_loss, "moment_loss_of").of(point)

    def _points_shape(self, *tail):
        return (batch_size(self.beam.batch_shape), self.trace.num_points, *tail)

    def _survivor_set_records(self):
        """
        The moment records of the INCOMING beam over the nested survivor sets, [B][A + 1][36] on the device
        (lynx_moments_by_loss): set j holds the particles alive behind the first j active apertures, by the `lost_at` the
        forward trace left on the device.  One more streaming pass over the incoming particles.
        """
        rt = device.get_runtime()
        beam, A = self.beam, len(self.program.apertures)
        B = batch_size(beam.batch_shape)
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
        B = batch_size(batch_shape)
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
        trace, screens = self.trace, self._image_calls
        named = []  # (screen, cotangent broadcast to its image), checked before anything is allocated
        for key, bar in screen_images_bar.items():
            k = _screen_of(key, self.program, self.leaves)  # (KeyError for anything but an active screen of the trace)
            shape = trace.screen_images[k].shape
            named.append((k, broadcast_or_refuse(np.asarray(bar), shape, f"screen_images_bar of screen {screens.elements[k].name!r}",
                                                 f"its image's {shape} (*batch, nx, ny)")))
        if not named:
            return None
        B = batch_size(self.beam.batch_shape)
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
        What a keyword of `track_along_vjp` adds, as that function says it: `screen_images_bar={screen: bar}` (`screens=True`),
        a value broadcastable to that screen's image (*batch, nx, ny); `image_loss_bar` (`image_targets=`), a scalar or
        (*batch,) for every screen with a target, or `{screen: bar}`; `moment_loss_bar` (`moment_targets=`), a scalar or
        (*batch,) -- alone, with no other cotangent of a moment or of the energy in the call, nothing with a point axis is made
        on the host: those cotangents are zero-filled on the device and the (*batch,) bars are the only upload;
        `wrt_particles=True` (`cavities=True`, a ParticleBeam): `Gradients.particles` (*batch, N, 7), device-resident.
        """
        if wrt_particles and self.mode != "kicks":
            raise ValueError("track_along_vjp: wrt_particles=True needs the pass over the particles -- a ParticleBeam and "
                             "cavities=True of track_along_vjp (without a cavity g.mu and g.cov say the same)")
        wi = None if screen_images_bar is None else self._image_cotangents(screen_images_bar)
        lb = None if image_loss_bar is None else loss_of(self._image_loss, "image_loss_bar").cotangents(image_loss_bar)
        ml = None if moment_loss_bar is None else loss_of(self._moment_loss, "moment_loss_bar").cotangents(moment_loss_bar)
        with_moments = mu_bar is not None or cov_bar is not None or bool(readings) or any(name != "energy" for name in properties)
        # the moment loss as the call's only cotangent of a moment or of the energy: nothing with a point axis is made here
        alone = ml is not None and not with_moments and energy_bar is None and not properties
        wb = None  # (a trace with trajectories and no cotangent on them: zeros -- made on the device where the moment loss is alone)
        if trajectories_bar is not None or (self.chosen is not None and not alone):
            wb = self._trajectory_cotangents(np.zeros(7) if trajectories_bar is None else trajectories_bar)
        if with_moments and self._cavity is not None:
            _refuse_moments(self._cavity)
        mb, cb, eb = (None, None, None) if alone else self._cotangents(mu_bar, cov_bar, energy_bar, readings, properties)
        with_moments = with_moments or (ml is not None and self._moment_loss.layout.moments)
        rt = device.get_runtime()
        sweep = _Sweep(rt, engine.trace_cache(self.segment), self.program, self.beam)
        # (an upload is named until its call has been enqueued, so that it stays allocated; no energy cotangent: no upload)
        eb_dev = rt.to_device(eb.astype(self.beam.dtype)) if eb is not None and np.any(eb) else None
        if eb_dev is None and ml is not None and self._moment_loss.layout.energy:
            eb_dev = self._zeros(rt, self._points_shape(), self.beam.dtype)
        launch = getattr(self, "_launch_" + self.mode)  # (_launch_moments, _particles, _trajectories, _survivors, _kicks)
        results = launch(rt, sweep, mb, cb, eb_dev, wi=wi, lb=lb, wb=wb, ml=ml, with_moments=with_moments, wrt_particles=wrt_particles)
        return Gradients(self.program, self.beam, sweep.g_par, sweep.g_en, **results)

    # what the launches below share: a cotangent buffer is uploaded where the host made one and zero-filled on the device where
    # the moment loss alone adds into it; then the loss's reverse half, in front of the sweep on the same stream
    def _zeros(self, rt, shape, dtype):
        zeros = rt.empty(shape, dtype)
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, _p(zeros), 0, math.prod(shape) * np.dtype(dtype).itemsize))
        return zeros

    def _add_moment_loss(self, rt, ml, eb_dev, **buffers):
        if ml is not None:
            self._moment_loss.backward(rt, ml, eb_dev, **buffers)

    def _records_in(self, rt, mb, cb, eb_dev, ml):
        """What the four particle modes begin with: the record cotangents on the device, with the moment loss's added into them."""
        zeros = lambda: self._zeros(rt, self._points_shape(_ffi.MOMENT_STRIDE), np.float64)  # noqa: E731
        rec_dev = zeros() if mb is None else rt.to_device(_record_cotangents(mb.shape[:-1], mb, cb))
        self._add_moment_loss(rt, ml, eb_dev, rec_dev=rec_dev)
        return rec_dev

    # one method per mode, called alike (each names what it uses): the library call or calls -> `Gradients`' optional results
    def _launch_moments(self, rt, sweep, mb, cb, eb_dev, wi, lb, ml, **_):
        beam, states = self.beam, self.trace._device
        zeros = lambda *tail: self._zeros(rt, self._points_shape(*tail), beam.dtype)  # noqa: E731
        mb_dev, cb_dev = (zeros(7), zeros(7, 7)) if mb is None else (rt.to_device(mb.astype(beam.dtype)), rt.to_device(cb.astype(beam.dtype)))
        shifts = []  # the parts of dL/d(misalignment), one per image call: `Gradients` adds them
        if wi is not None:  # the images' cotangents go into mb_dev, cb_dev at the screens' points, on the same stream
            head, shots = self._image_calls.head(rt, "mu", "cov")
            wi_dev = rt.to_device(np.ascontiguousarray(wi, dtype=beam.dtype))
            shifts.append(rt.empty((head[2], shots["count"], 2), beam.dtype))
            rt.check(rt.lib.lynx_gaussian_images_along_backward(
                *head, *shots["arguments"], _p(wi_dev), _p(mb_dev), _p(cb_dev), _p(shifts[-1])))
        if lb is not None:  # ... and so do the image losses' cotangents times the sums of the forward pass
            shifts.append(self._image_loss.backward(rt, lb, mb_dev, cb_dev))
        self._add_moment_loss(rt, ml, eb_dev, mb_dev=mb_dev, cb_dev=cb_dev)
        rt.check(rt.lib.lynx_track_moments_along_backward(
            rt.ctx, sweep.lat.handle, _p(sweep.e_in), _p(states["mu"]), _p(states["cov"]), _p(mb_dev), _p(cb_dev), _p(eb_dev),
            _p(sweep.g_par), _p(sweep.g_en), _p(sweep.g_mu), _p(sweep.g_cov)))
        with_screens = self._screens or self._targets is not None
        return dict(moments=(sweep.g_mu, sweep.g_cov), screens=(self._image_calls.elements, shifts) if with_screens else None)

    def _launch_particles(self, rt, sweep, mb, cb, eb_dev, ml, **_):
        rec_dev = self._records_in(rt, mb, cb, eb_dev, ml)
        rt.check(rt.lib.lynx_track_particles_along_backward(
            rt.ctx, sweep.lat.handle, self.beam.num_particles, _p(sweep.e_in), _p(self.trace._device["records"]), _p(rec_dev),
            _p(eb_dev), _p(sweep.g_par), _p(sweep.g_en), _p(sweep.g_mu), _p(sweep.g_cov)))
        return dict(moments=(sweep.g_mu, sweep.g_cov))

    def _launch_trajectories(self, rt, sweep, mb, cb, eb_dev, wb, ml, with_moments, **_):
        beam, states, K = self.beam, self.trace._device, len(self.chosen)
        # without a moment cotangent the moment path does not run: no records in, no g.mu and g.cov out (a moment loss of
        # energies alone still adds into a record buffer, which the sweep is then not handed)
        rec_dev = self._records_in(rt, mb if with_moments else None, cb, eb_dev, ml) if with_moments or ml is not None else None
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
        rec_dev = self._records_in(rt, mb, cb, eb_dev, ml)
        g_p = rt.empty((*beam.batch_shape, beam.num_particles, 7), beam.dtype) if wrt_particles else None
        rt.check(rt.lib.lynx_track_particles_along_backward_cavities(
            rt.ctx, sweep.lat.handle, beam.num_particles, _p(sweep.e_in), _p(beam._particles.device(rt)),
            _ffi.TRACK_SHARED_INPUT if beam.is_shared else 0, _p(self.trace._device["records"]), _p(rec_dev), _p(eb_dev),
            _p(sweep.g_par), _p(sweep.g_en), _p(g_p)))
        return dict(particles=g_p, moments=Gradients.NO_INCOMING_MOMENTS)

    def _launch_survivors(self, rt, sweep, mb, cb, eb_dev, ml, **_):
        rec_dev = self._records_in(rt, mb, cb, eb_dev, ml)
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
