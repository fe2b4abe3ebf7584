"""
Host side of the hot path: turns a list of element objects into the flat lattice program
liblynxhip consumes (include/lynx_hip.h) and dispatches the kernels.

What stays on the host is exactly what the reference also decides in Python: the order of
elements, the partition of the lattice into maximal skippable runs and non-skippable
elements (`Segment.track`, lynx/accelerator/segment.py:340-356) and the whole-batch
`if any(...)` predicates (track_methods.py:101, quadrupole.py:75, dipole.py:119,
cavity.py:128,164,260,290).  All arithmetic on maps, moments and particles happens in the
HIP kernels; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _ffi, config
from .device import DeviceArray, Dual, dtype_code, get_runtime

ELECTRON_MASS_EV = 510998.95069  # cavity.py:20
_F64 = np.dtype(np.float64)

_LATE = None


def _late():
    """
    What the engine needs from modules that import the engine themselves, bound on first use.  (As `from ... import`
    statements inside `track` and friends they cost seven import-system look-ups per call -- a fifth of the host
    time of a ParameterBeam `track`, which is bound by the host's enqueue rate.)
    """
    global _LATE
    if _LATE is None:
        from types import SimpleNamespace

        from .accelerator.element import EPOCH, STRUCTURE
        from .accelerator.segment import Segment
        from .particles.beam import Beam
        from .particles.parameter_beam import ParameterBeam
        from .particles.particle_beam import ParticleBeam

        from .accelerator.segment import ElementList
        from .trace import BeamTrace

        _LATE = SimpleNamespace(EPOCH=EPOCH, STRUCTURE=STRUCTURE, Segment=Segment, Beam=Beam, BeamTrace=BeamTrace,
                                ParameterBeam=ParameterBeam, ParticleBeam=ParticleBeam, ElementList=ElementList)
    return _LATE


# -------------------------------------------------------------------------------------------
# program = what Segment.track iterates over
# -------------------------------------------------------------------------------------------


@dataclass
class Program:
    """A maximal stretch of the lattice one kernel launch can run: runs + active cavities."""

    leaves: list = field(default_factory=list)  # leaf elements in lattice order
    steps: list = field(default_factory=list)   # (kind, first, last) over `leaves`
    raw: bool = False  # runs take their first map as is (Element.track), see LYNX_STEP_FLAG_RAW
    observers: list = field(default_factory=list)  # (step index, element): active BPMs read inside the pass
    apertures: list = field(default_factory=list)  # (step index, element, elliptical): active apertures of a trace with losses
    screens: list = field(default_factory=list)  # (step index, element): active screens of a trace with screens

    def add_run_element(self, element, new_run: bool):
        idx = len(self.leaves)
        self.leaves.append(element)
        if new_run or not self.steps or self.steps[-1][0] != _ffi.STEP_RUN:
            self.steps.append([_ffi.STEP_RUN, idx, idx + 1])
        else:
            self.steps[-1][2] = idx + 1

    def add_cavity(self, element):
        idx = len(self.leaves)
        self.leaves.append(element)
        self.steps.append([_ffi.STEP_CAVITY, idx, idx + 1])

    def add_observer(self, element):
        """An active BPM as a one-element run step of its own (LYNX_STEP_FLAG_OBSERVE): the streaming kernel
        adds up x and y of the particles entering it -- `reading = stack([mu_x, mu_y])`, bpm.py:48-54 --
        instead of the pass being cut in two there."""
        idx = len(self.leaves)
        self.leaves.append(element)
        self.observers.append((len(self.steps), element))
        self.steps.append([_ffi.STEP_RUN, idx, idx + 1])


def partition(elements, fuse_observers: bool = False) -> list:
    """
    Mirror of the `todos` loop in segment.py:344-351, flattened over nested segments:
    returns a list of `Program` objects and host-side barrier elements (active screens and
    apertures; active BPMs too unless `fuse_observers`, the ParticleBeam case, where up to
    `_ffi.MAX_OBSERVERS` of them per program are read inside the streaming pass), in
    order.  A nested non-skippable Segment is tracked on its own by the reference, so it
    starts and ends a run; a nested skippable Segment's elements join the current run (the
    reference multiplies its pre-composed product instead: same map up to rounding).
    """
    Segment = _late().Segment

    out: list = []
    state = {"new_run": True}

    def current() -> Program:
        if not out or not isinstance(out[-1], Program):
            out.append(Program())
            state["new_run"] = True
        return out[-1]

    def room_for_observer() -> bool:
        """The program being filled reads fewer than MAX_OBSERVERS active BPMs so far (a new one reads none)."""
        return not (out and isinstance(out[-1], Program)) or len(out[-1].observers) < _ffi.MAX_OBSERVERS

    def walk(items):
        for el in items:
            if isinstance(el, Segment):
                if el.is_skippable:
                    walk(el.elements)
                else:
                    state["new_run"] = True
                    walk(el.elements)
                    state["new_run"] = True
            elif el.is_skippable:
                current().add_run_element(el, state["new_run"])
                state["new_run"] = False
            elif el._kind == _ffi.KIND_CAVITY:
                current().add_cavity(el)
                state["new_run"] = True
            elif fuse_observers and getattr(el, "_fusable_observer", False) and room_for_observer():
                current().add_observer(el)
                state["new_run"] = True
            elif getattr(el, "_host_barrier", False):
                out.append(el)
                state["new_run"] = True
            else:
                raise TypeError(f"element {el!r} cannot be tracked by lynx_amd")

    walk(elements)
    return out


# -------------------------------------------------------------------------------------------
# what an owner remembers
# -------------------------------------------------------------------------------------------

# Everything the engine keeps on an owner (a Segment, or an Element tracked on its own) between two calls.  The first four
# are memos of `_remembered` ({mode: (token, value)}), the last two the packed programs of `track` / `transfer_map` and of
# `track_along`.  `Element._transient` is made from this tuple: a twin (`broadcast`) takes none of them along.
OWNER_SLOTS = ("_plan", "_trace_plan", "_trace_limits", "_trace_screens", "_lattice_cache", "_trace_cache")


def _held(owner, slot: str, make):
    # through `__dict__`, never `setattr`: `Segment.__setattr__` bumps EPOCH and STRUCTURE, the very counters that say
    # whether what is remembered here still holds
    held = owner.__dict__.get(slot)
    if held is None:
        held = owner.__dict__[slot] = make()
    return held


def lattice_cache(owner) -> "LatticeCache":
    """The packed programs of `track` and `transfer_map` on this owner."""
    return _held(owner, "_lattice_cache", LatticeCache)


def trace_cache(owner) -> "LatticeCache":
    """The packed every-element-its-own-step programs of `track_along` on this owner."""
    return _held(owner, "_trace_cache", LatticeCache)


def _remembered(owner, slot: str, mode, token, make):
    """`make()`, remembered in `slot` of `owner` per `mode` for as long as `token` compares equal."""
    memos = _held(owner, slot, dict)
    memo = memos.get(mode)
    if memo is None or memo[0] != token:
        memo = memos[mode] = (token, make())
    return memo[1]


def plan(owner, elements, raw: bool, fuse_observers: bool = False) -> list:
    """
    `partition(elements)` remembered on `owner` for as long as no attribute that can change the
    partition has been written (global STRUCTURE counter) and the element list holds the same
    objects: a tracking loop then costs one C-level pass over the list instead of Python work
    per element, also when magnet strengths are rewritten between the calls.
    """
    late = _late()
    STRUCTURE, Segment = late.STRUCTURE, late.Segment

    def identities(items):
        ids = tuple(map(id, items))
        if any(issubclass(t, Segment) for t in set(map(type, items))):  # nested lists can change too
            ids = (ids, tuple(identities(el.elements) for el in items if isinstance(el, Segment)))
        return ids

    def make():
        items = partition(elements, fuse_observers)
        for item in items:
            if isinstance(item, Program):
                item.raw = raw
        return items

    # a Segment's own list says when it is changed in place (ElementList bumps STRUCTURE, and so do the lists of nested
    # segments): the list object itself stands for its contents; any other sequence is compared element by element
    ids = id(elements) if type(elements) is late.ElementList else identities(elements)
    return _remembered(owner, "_plan", fuse_observers, (STRUCTURE[0], raw, ids), make)


# -------------------------------------------------------------------------------------------
# packing
# -------------------------------------------------------------------------------------------


def _broadcast_param(value, batch_shape, dtype, what):
    arr = np.asarray(value, dtype=dtype)
    try:
        return np.broadcast_to(arr, batch_shape)
    except ValueError:
        raise AssertionError(
            f"Beam shape {tuple(batch_shape)} does not match element shape {arr.shape} ({what})"
        ) from None


class PackedLattice:
    """Device-resident lattice program + the host arrays it was packed from."""

    def __init__(self, program: Program, batch_shape, dtype):
        self.program = program
        self.batch_shape = tuple(batch_shape)
        self.dtype = np.dtype(dtype)
        self.B = int(np.prod(self.batch_shape, dtype=np.int64))
        leaves = program.leaves
        E, S = len(leaves), len(program.steps)
        self.elems = (_ffi.Elem * max(E, 1))()
        self.steps = (_ffi.Step * max(S, 1))()
        parts, offset = [], 0
        self.layout = []  # per element: (offset, scalars, batch stride) in the parameter pool
        for e, el in enumerate(leaves):
            block, stride = self._pack_element(el)
            self.elems[e] = _ffi.Elem(el._kind, 0, offset, stride)
            self.layout.append((offset, block.size, stride))
            if block.size:
                parts.append(block)
                offset += block.size
        self.pool = (np.concatenate(parts) if parts else np.zeros(1, dtype=self.dtype)).astype(self.dtype)
        for s, (kind, first, last) in enumerate(program.steps):
            self.steps[s] = _ffi.Step(kind, first, last, 0)
        self.E, self.S = E, S
        self.elem_flags = [0] * E
        self.step_flags = [0] * S
        self.has_cavity_step = any(k == _ffi.STEP_CAVITY for k, _, _ in program.steps)
        self.handle = None
        self.rt = None
        self._static = None
        self._has_cavity = False
        self._ready_epoch = None
        self.versions = tuple(el._version for el in leaves)

    def _pack_element(self, el):
        """The element's parameter rows as one pool block: (flat array, batch stride)."""
        rows = el._param_rows(self.dtype)
        n = _ffi.PARAMS_OF_KIND[el._kind]
        assert len(rows) == n, (el, len(rows), n)
        if n == 0:
            return np.zeros(0, dtype=self.dtype), 0
        if all(np.asarray(r).size == 1 for r in rows):  # shared by the whole batch
            return np.array([np.asarray(r, dtype=self.dtype).reshape(()) for r in rows], dtype=self.dtype), 0
        mat = np.stack([_broadcast_param(r, self.batch_shape, self.dtype, type(el).__name__).reshape(self.B)
                        for r in rows], axis=1)
        return np.ascontiguousarray(mat).reshape(-1), n

    def refresh(self, versions) -> bool:
        """
        Element parameters changed (`quad.k1 = ...`) but not the structure: rewrite the pool
        blocks of the changed elements in place (`lynx_lattice_update_params`).  False if a
        block changed its size or stride -- the caller then packs from scratch.
        """
        for e, (el, old, new) in enumerate(zip(self.program.leaves, self.versions, versions)):
            if old == new:
                continue
            block, stride = self._pack_element(el)
            offset, size, old_stride = self.layout[e]
            if block.size != size or stride != old_stride:
                return False
            if size:
                self.pool[offset:offset + size] = block
                if self.handle is not None:
                    self.rt.check(self.rt.lib.lynx_lattice_update_params(
                        self.handle, offset, size, self.pool[offset:offset + size].ctypes.data))
            if self._static is not None:  # whole-batch predicates of this element (tilt, misalignment, ...)
                self._static = list(self._static)
                self._static[e] = el._static_flags()
        self.versions = tuple(versions)
        return True

    # whole-batch predicates -----------------------------------------------------------------
    def evaluate_flags(self, energy_host=None):
        """
        Element and step flags the host decides: the parameter-only predicates of magnets (tilt,
        misalignment, thick dipole: `_static_flags`), `LYNX_STEP_FLAG_RAW` and the observer steps.  The
        cavity predicates depend on the beam energy on its way through the lattice and are evaluated on
        the device before every build (`k_cavity_flags`), so the energy never has to come back to the
        host for them.  What stays here of cavity.py:260 (`assert Ei > 0`) is the check of the INCOMING
        energy, when the host already holds it; a cavity that decelerates the beam through zero is not
        caught.  Returns (elem_flags, step_flags).
        """
        leaves = self.program.leaves
        if self._static is None:  # element versions are part of the cache key: these cannot change
            self._static = [el._static_flags() for el in leaves]
            self._has_cavity = any(el._kind == _ffi.KIND_CAVITY for el in leaves)
        base = _ffi.STEP_FLAG_RAW if self.program.raw else 0
        observed = {s for s, _ in self.program.observers}
        if self._has_cavity and energy_host is not None:
            assert np.all(np.asarray(energy_host) > 0), "Initial energy must be larger than 0"
        return self._static, [base | (_ffi.STEP_FLAG_OBSERVE if s in observed else 0) for s in range(self.S)]

    # device side ----------------------------------------------------------------------------
    def upload(self, rt, elem_flags, step_flags):
        for e, f in enumerate(elem_flags):
            self.elems[e].flags = f
        for s, f in enumerate(step_flags):
            self.steps[s].flags = f
        self.elem_flags, self.step_flags = list(elem_flags), list(step_flags)
        handle = C.c_void_p()
        rt.check(rt.lib.lynx_lattice_create(
            rt.ctx, dtype_code(self.dtype), self.B, self.E, self.elems, self.S, self.steps,
            self.pool.ctypes.data, self.pool.size, C.byref(handle)))
        self.handle, self.rt = handle, rt

    def set_flags(self, elem_flags, step_flags):
        if list(elem_flags) == self.elem_flags and list(step_flags) == self.step_flags:
            return
        ef = (C.c_int32 * max(self.E, 1))(*elem_flags)
        sf = (C.c_int32 * max(self.S, 1))(*step_flags)
        self.rt.check(self.rt.lib.lynx_lattice_set_flags(self.handle, ef, sf))
        self.elem_flags, self.step_flags = list(elem_flags), list(step_flags)

    def release(self):
        if self.handle is not None:
            if not self.rt.closed:
                self.rt.lib.lynx_lattice_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class LatticeCache:
    """
    Packed programs of one owner (a Segment or an Element).  Keyed by structure (which element
    objects, which steps, batch shape, dtype); a parameter change only rewrites the changed
    elements' blocks of the device-resident pool.
    """

    def __init__(self, capacity: int = 4):
        self.capacity = capacity
        self.entries: dict = {}
        self._last = None

    def get(self, program: Program, batch_shape, dtype) -> PackedLattice:
        EPOCH = _late().EPOCH
        shape_key = (tuple(batch_shape), np.dtype(dtype).str, program.raw)
        last = self._last
        if last is not None and last[0] is program and last[1] == EPOCH[0] and last[2] == shape_key:
            return last[3]
        leaves = program.leaves
        key = (tuple(map(id, leaves)), tuple(tuple(s) for s in program.steps), shape_key)
        versions = tuple(el._version for el in leaves)
        hit = self.entries.get(key)
        if hit is not None and hit.versions != versions and not hit.refresh(versions):
            self.entries.pop(key).release()
            hit = None
        if hit is None:
            if len(self.entries) >= self.capacity:
                self.entries.pop(next(iter(self.entries))).release()
            hit = PackedLattice(program, batch_shape, dtype)
            self.entries[key] = hit
        self._last = (program, EPOCH[0], shape_key, hit)
        return hit


def _ready(cache: LatticeCache, program: Program, batch_shape, dtype, energy_host) -> PackedLattice:
    lat = cache.get(program, batch_shape, dtype)
    # nothing an element holds has been written since this lattice's flags were last evaluated (EPOCH), and it has no
    # cavity whose `assert Ei > 0` would have to look at THIS beam's energy: it is ready as it stands
    epoch = _late().EPOCH[0]
    if lat._ready_epoch == epoch and not lat._has_cavity and lat.handle is not None:
        return lat
    elem_flags, step_flags = lat.evaluate_flags(energy_host)
    if lat.handle is None:
        lat.upload(get_runtime(), elem_flags, step_flags)
    else:
        lat.set_flags(elem_flags, step_flags)
    lat._ready_epoch = epoch
    return lat


# -------------------------------------------------------------------------------------------
# dispatch
# -------------------------------------------------------------------------------------------


def _ptr(x):
    return None if x is None else C.c_void_p(x.ptr)


def _outgoing_particles(incoming, particles: Dual, energy: Dual | None, moments: Dual | None):
    """
    The ParticleBeam that leaves a pass `incoming` entered.  `energy` None: no cavity was passed, the beam goes on with
    the incoming beam's own energy object (and whatever device copies it holds).  The charges go on as they are, except
    those of a lazily broadcast beam, which are stored once for all samples: the outgoing beam has particles per sample,
    so it is handed the charges per sample too.
    """
    charges = incoming._charges
    if charges is not None and incoming.is_shared:
        charges = np.ascontiguousarray(incoming.particle_charges)
    # (`_from_raw` spelled out here and in `run_program_parameters`, the two beams a `track` call makes: the classmethod's
    # argument forwarding costs 0.6 us of a call that is bound by the host, see `_late`)
    out = object.__new__(_late().ParticleBeam)
    out._init_raw(particles, incoming._energy if energy is None else energy, charges, incoming.dtype, moments)
    return out


def run_program_particles(cache, program: Program, beam, moments: bool | None = None):
    """One pass of the streaming kernel: ParticleBeam -> ParticleBeam (`lynx_track_particles_new`)."""
    rt = get_runtime()
    dtype = beam.dtype
    batch_shape = beam.batch_shape
    lat = _ready(cache, program, batch_shape, dtype, beam._energy._host)  # no read-back: None if it lives in HBM only
    p_in = beam._particles.device(rt)  # (N, 7)-like storage when the beam is shared by the batch
    e_in = beam._energy.broadcast_device(rt, batch_shape)
    want_moments = config.fused_moments if moments is None else moments
    flags = ((0 if not want_moments else _ffi.TRACK_COVARIANCE if config.fused_covariance else _ffi.TRACK_MOMENTS)
             | (_ffi.TRACK_SHARED_INPUT if beam.is_shared else 0)
             | (0 if config.merge_steps else _ffi.TRACK_SEQUENTIAL_STEPS))
    n = beam.num_particles
    # the outgoing beam's blocks come from the library's pool inside the call: one crossing of the C boundary per
    # `track` instead of one per array (a small call is bound by the host's enqueue rate)
    blocks = (C.c_void_p * 4)()
    status = rt.lib.lynx_track_particles_new(rt.ctx, lat.handle, n, e_in.ptr, p_in.ptr, flags,
                                             1 if lat.has_cavity_step else 0, blocks)
    if status:
        rt.check(status)
    adopt = DeviceArray.adopt
    p_out = adopt(rt, blocks[0], (*batch_shape, n, 7), dtype)
    e_out = adopt(rt, blocks[1], batch_shape, dtype) if blocks[1] else None
    mom = adopt(rt, blocks[2], (*batch_shape, _ffi.MOMENT_STRIDE), _F64) if blocks[2] else None
    if blocks[3]:
        obs = adopt(rt, blocks[3], (lat.B, len(program.observers), 2), _F64)
        for k, (_, element) in enumerate(program.observers):
            element._reading_from(obs, k, batch_shape, dtype)  # read back only if somebody looks at it
    return _outgoing_particles(beam, Dual(dev=p_out), None if e_out is None else Dual(dev=e_out),
                               None if mom is None else Dual(dev=mom))


def run_program_parameters(cache, program: Program, beam):
    """ParameterBeam -> ParameterBeam (lynx_track_moments)."""
    rt = get_runtime()
    dtype = beam.dtype
    batch_shape = beam.batch_shape
    lat = _ready(cache, program, batch_shape, dtype, beam._energy._host)
    mu_in = beam._mu_d.device(rt)
    cov_in = beam._cov_d.device(rt)
    mu_out = rt.empty_result(mu_in.shape, dtype)
    cov_out = rt.empty_result(cov_in.shape, dtype)
    e_in = beam._energy.broadcast_device(rt, batch_shape)
    e_out = rt.empty(batch_shape, dtype) if lat.has_cavity_step else None
    rt.check(rt.lib.lynx_track_moments(rt.ctx, lat.handle, _ptr(e_in), _ptr(mu_in), _ptr(cov_in),
                                       _ptr(mu_out), _ptr(cov_out), _ptr(e_out)))
    out = object.__new__(_late().ParameterBeam)  # (`_from_raw` spelled out, as in `_outgoing_particles`)
    out._init_raw(Dual(dev=mu_out), Dual(dev=cov_out), Dual(dev=e_out) if e_out is not None else beam._energy, beam.total_charge, dtype)
    return out


def track(owner, elements, incoming, raw: bool = False):
    """`Segment.track` (raw=False) / `Element.track` (raw=True) for both beam types."""
    late = _late()
    Beam, ParameterBeam, ParticleBeam = late.Beam, late.ParameterBeam, late.ParticleBeam
    if incoming is Beam.empty:
        for el in elements:
            if getattr(el, "_host_barrier", False):
                el._observe(incoming)
        return incoming
    if not isinstance(incoming, (ParameterBeam, ParticleBeam)):
        raise TypeError(f"Parameter incoming is of invalid type {type(incoming)}")
    cache = lattice_cache(owner)
    beam = incoming
    for item in plan(owner, elements, raw, fuse_observers=isinstance(incoming, ParticleBeam)):
        if isinstance(item, Program):
            if isinstance(beam, ParticleBeam):
                beam = run_program_particles(cache, item, beam)
            else:
                beam = run_program_parameters(cache, item, beam)
        else:  # host-side barrier: active BPM (bpm.py:48-58) or active Screen (screen.py:126-141)
            item._observe(beam)
            if getattr(item, "_swallows_beam", False):
                beam = Beam.empty
            elif hasattr(item, "_transform"):  # active Aperture (aperture.py:69-108)
                beam = item._transform(beam)
            elif beam is not Beam.empty:
                beam = beam._shallow_copy()
        if beam is Beam.empty:  # everything behind an active screen sees the empty beam
            seen = False
            for later in elements:
                if later is item:
                    seen = True
                elif seen and getattr(later, "_host_barrier", False):
                    later._observe(beam)
            return beam
    return beam


# -------------------------------------------------------------------------------------------
# the beam along the lattice (Segment.track_along)
# -------------------------------------------------------------------------------------------


def trace_program(leaves, losses: bool = False, screens: bool = False) -> Program:
    """
    The lattice with every leaf element a step of its own, as the loop of the reference's `plot_twiss` tracks it
    (`element.track(beam)`: the element's OWN map, taken as it is -- LYNX_STEP_FLAG_RAW; an active cavity by
    `Cavity._track_beam`).  An active BPM is an identity element whose reading comes from the trace, so the observer
    limit of `Segment.track` does not apply; an active Screen has no place inside one streaming pass, and neither has
    an active Aperture unless the trace carries particle losses: with `losses` it is an identity step of its own, like an
    inactive one, and `program.apertures` remembers its step index and its shape (the kernel clears the particles
    outside it from every later point, `lynx_track_particles_along_losses`).  With `screens` an active Screen is an
    identity step of its own as well, `program.screens` remembers its step index, and the pass makes its image of the beam
    entering it (`lynx_track_particles_along_screens`, `lynx_gaussian_images_along`).
    """
    program = Program(raw=True)
    for el in leaves:
        if el.is_skippable or getattr(el, "_fusable_observer", False):
            program.add_run_element(el, True)
        elif el._kind == _ffi.KIND_CAVITY:
            program.add_cavity(el)
        elif losses and hasattr(el, "_transform"):  # active Aperture
            assert el.shape in ["rectangular", "elliptical"], f"Unknown aperture shape {el.shape}"
            program.apertures.append((len(program.steps), el, el.shape == "elliptical"))
            program.add_run_element(el, True)
        elif screens and getattr(el, "_swallows_beam", False):  # active Screen
            program.screens.append((len(program.steps), el))
            program.add_run_element(el, True)
        else:
            hint = (" (pass losses=True to have the trace carry the particle losses)" if hasattr(el, "_transform")
                    else " (pass screens=True to have the trace make the screen images)" if getattr(el, "_swallows_beam", False) else "")
            raise NotImplementedError(
                f"track_along: active {type(el).__name__} {el.name!r} -- a lattice with an active Screen or Aperture is "
                f"not traced in one pass; trace the stretches on either side of it{hint}")
    return program


def _trace_plan(owner, leaves, losses: bool = False, screens: bool = False) -> Program:
    """`trace_program` remembered on `owner` like `plan` remembers the partition of `track`, per (losses, screens) mode."""
    mode = (bool(losses), bool(screens))
    token = (_late().STRUCTURE[0], tuple(map(id, leaves)))
    return _remembered(owner, "_trace_plan", mode, token, lambda: trace_program(leaves, *mode))


def _aperture_limits(owner, program: Program, batch_shape, dtype, rt):
    """
    x_max, y_max of the program's active apertures on the device: ([B or 1][A][2] array, scalars between two samples --
    0 when every limit is shared by the batch).  Remembered on `owner` until a limit is written.
    """
    elements = [el for _, el, _ in program.apertures]

    def make():
        B = int(np.prod(batch_shape, dtype=np.int64))
        values = []
        for el in elements:
            assert np.all(el.x_max >= 0) and np.all(el.y_max >= 0)  # aperture.py:74-76
            values += [np.asarray(el.x_max, dtype=dtype), np.asarray(el.y_max, dtype=dtype)]
        shared = all(v.size == 1 for v in values)
        rows = [v.reshape(1) if shared else _broadcast_param(v, batch_shape, dtype, "Aperture").reshape(B) for v in values]
        host = np.ascontiguousarray(np.stack(rows, axis=1).reshape(-1, len(elements), 2)) if rows else np.zeros((1, 1, 2), dtype=dtype)
        return rt.to_device(host), 0 if shared else 2 * len(elements)

    token = (id(program), tuple(batch_shape), np.dtype(dtype).str, tuple(el._version for el in elements))
    return _remembered(owner, "_trace_limits", None, token, make)


def _aperture_arguments(owner, program: Program, batch_shape, dtype, rt):
    """The program's active apertures as both entry points take them: number, host pairs (step, elliptical), limits, stride."""
    A = len(program.apertures)
    limits, stride = _aperture_limits(owner, program, batch_shape, dtype, rt) if A else (None, 0)
    pairs = (C.c_int32 * max(2 * A, 1))(*[v for step, _, elliptical in program.apertures for v in (step, int(elliptical))])
    return A, pairs, _ptr(limits), stride


def _pixel_positions(screen, dtype):
    """xs, ys: where a ParameterBeam's image is evaluated -- the very expressions of `Screen.reading`, on the host alone."""
    e = screen.extent.astype(dtype)
    pitch = (screen.pixel_size * screen.binning).astype(dtype)
    return np.arange(e[0], e[1], pitch[0], dtype=dtype), np.arange(e[2], e[3], pitch[1], dtype=dtype)


def _screen_geometry(owner, program: Program, batch_shape, dtype, rt, particles: bool):
    """
    What the device needs to know about the program's active screens, remembered on `owner` until a screen setting or a
    misalignment is written: the host rows [K][3] (step -- which is the point the screen observes --, then the image's
    two sizes), the pixel grid on the device, the misalignments [B or 1][K][2] and the scalars between two samples of
    them (0: shared by the batch), the image shapes and the cells of one sample's images.  For a ParticleBeam the grid is
    every screen's `pixel_bin_edges` in the lattice's dtype (x edges, then y edges) and an image is (ny, nx); for a
    ParameterBeam it is the pixel positions `Screen.reading` evaluates the density at (xs, then ys), an image (len(xs),
    len(ys)).  "arguments" is (count, rows, grid, misalignments, stride) as the library takes them.
    """
    def make():
        B = int(np.prod(batch_shape, dtype=np.int64))
        rows, grid, shapes, shifts = [], [], [], []
        for (step, el) in program.screens:
            if particles:
                xe, ye = (np.ascontiguousarray(e.astype(dtype)) for e in el.pixel_bin_edges)
                nx, ny = len(xe) - 1, len(ye) - 1
                shapes.append((ny, nx))
                grid += [xe, ye]
            else:
                xs, ys = _pixel_positions(el, dtype)
                nx, ny = len(xs), len(ys)
                shapes.append((nx, ny))
                grid += [xs, ys]
            assert nx >= 1 and ny >= 1, f"Screen {el.name!r} has no pixels"
            rows += [step, nx, ny]
            shifts.append(np.asarray(el.misalignment, dtype=dtype))
        shared = all(v.size == 2 for v in shifts)
        shifts = [v.reshape(1, 2) if shared else _broadcast_param(v, (*batch_shape, 2), dtype, "Screen").reshape(B, 2) for v in shifts]
        geometry = {
            "rows": (C.c_int32 * len(rows))(*rows), "count": len(program.screens), "shapes": shapes,
            "cells": int(sum(a * b for a, b in shapes)),
            "grid": rt.to_device(np.ascontiguousarray(np.concatenate(grid))),
            "misalignment": rt.to_device(np.ascontiguousarray(np.stack(shifts, axis=1))),
            "stride": 0 if shared else 2 * len(program.screens),
        }
        # the screen argument group of every entry point that takes one, in the order they all take it
        geometry["arguments"] = (geometry["count"], geometry["rows"], _ptr(geometry["grid"]), _ptr(geometry["misalignment"]), geometry["stride"])
        return geometry

    token = (tuple((step, id(el), el._version) for step, el in program.screens), tuple(batch_shape), np.dtype(dtype).str, bool(particles))
    return _remembered(owner, "_trace_screens", None, token, make)


def _screen_images(flat, geometry, batch_shape, dtype):
    """One array per screen out of the [B][cells] the device wrote, in the dtype `Screen.reading` returns."""
    images, first = [], 0
    for shape in geometry["shapes"]:
        cells = shape[0] * shape[1]
        images.append(np.ascontiguousarray(flat[:, first:first + cells]).reshape(*batch_shape, *shape).astype(dtype, copy=False))
        first += cells
    return images


def chosen_particles(trajectories, incoming) -> np.ndarray:
    """
    `trajectories` of `track_along` as the (K,) int64 indices of the chosen particles: an int K is particles 0 .. K - 1,
    a 1-D integer array is taken as it is (any order, repeats allowed).  Everything else is refused here, on the host,
    by value -- the kernel relies on the indices.
    """
    late = _late()
    if isinstance(incoming, late.ParameterBeam):
        raise TypeError(
            "track_along: trajectories need particles and a ParameterBeam has none -- trace a ParticleBeam with its moments "
            "instead (ParticleBeam.make_linspaced or ParticleBeam.from_parameters), as the reference's "
            "plot_reference_particle_traces does")
    n = int(incoming.num_particles)
    what = f"track_along: trajectories={trajectories!r}"
    if isinstance(trajectories, (bool, np.bool_)):
        raise ValueError(f"{what}: a number of particles or an array of particle indices, not a bool")
    if isinstance(trajectories, (int, np.integer)):
        if trajectories < 1:
            raise ValueError(f"{what}: at least one particle")
        if trajectories > n:
            raise ValueError(f"{what}: the beam has {n} particles")
        return np.arange(int(trajectories), dtype=np.int64)
    chosen = np.asarray(trajectories)
    if chosen.ndim != 1:
        raise ValueError(f"{what}: a 1-D array of particle indices, not one of shape {chosen.shape}")
    if chosen.size == 0:
        raise ValueError(f"{what}: an empty selection")
    if chosen.dtype.kind not in "iu":
        raise ValueError(f"{what}: particle indices are integers, not {chosen.dtype.name}")
    outside = chosen[(chosen < 0) | (chosen >= n)]
    if outside.size:
        raise ValueError(f"{what}: index {int(outside[0])} is not a particle of a beam of {n} (0 <= index < {n})")
    return np.ascontiguousarray(chosen, dtype=np.int64)


# An argument group of `lynx_track_particles_along_trajectories`, the superset entry point, that the same call without
# trajectories would not hand over either: -1 for the list's length.  (The screen group ends with the image counts.)
_NO_APERTURES = (-1, None, None, 0)
_NO_SCREENS = (-1, None, None, None, 0, None)


def _trace_particles(*, owner, program: Program, lat, incoming, e_in, e_trace, lengths, names, keep_outgoing, rt, losses, chosen=None):
    """The ParticleBeam's trace: (trace, x and y of the centroid at every point, the device arrays a reverse pass reads)."""
    late = _late()
    dtype, batch_shape, P = incoming.dtype, incoming.batch_shape, lat.S + 1
    n, p_in = incoming.num_particles, incoming._particles.device(rt)
    p_out = rt.empty((*batch_shape, n, 7), dtype) if keep_outgoing else None
    records = rt.empty_result((lat.B, P, _ffi.MOMENT_STRIDE), _F64)
    common = (rt.ctx, lat.handle, n, _ptr(e_in), _ptr(p_in), _ptr(p_out), _ptr(e_trace), _ptr(records),
              _ffi.TRACK_SHARED_INPUT if incoming.is_shared else 0)
    lost_at = rt.empty((lat.B, n), np.int32) if losses == "particles" else None  # (4 B N bytes: device memory, read back once)
    # every argument group once: what it is when present, and its absent form
    paths = path_lost_in = shots = counts = None
    screens = _NO_SCREENS
    if chosen is not None:
        K = len(chosen)
        d_chosen = rt.to_device(chosen)  # (referenced until the call is enqueued)
        paths = rt.empty((lat.B, P, K, 7), dtype)
        path_lost_in = rt.empty((lat.B, K), np.int32) if losses else None
        particles = (K, _ptr(d_chosen), _ptr(paths), _ptr(path_lost_in))

    def aperture_group():  # (the screens entry takes the apertures too: there are none without `losses`)
        return _aperture_arguments(owner, program, batch_shape, dtype, rt) if losses or program.screens else _NO_APERTURES

    # (a first call uploads the limits and the pixel grid here, the limits first for chosen particles and last otherwise:
    # the order each of the two entry points that take both has always had)
    if chosen is not None:
        apertures = aperture_group()
    if program.screens:
        shots = _screen_geometry(owner, program, batch_shape, dtype, rt, True)
        counts = rt.empty((lat.B, shots["cells"]), np.int32)  # (zeroed by the call, on its stream)
        screens = (*shots["arguments"], _ptr(counts))
    if chosen is None:
        apertures = aperture_group()
    # the entry point that takes the groups present and no other: the trajectories entry, a superset of the other three, for chosen particles alone
    if chosen is not None:
        entry, groups = rt.lib.lynx_track_particles_along_trajectories, (*apertures, _ptr(lost_at), *screens, *particles)
    elif program.screens:
        entry, groups = rt.lib.lynx_track_particles_along_screens, (*apertures, _ptr(lost_at), *screens)
    elif losses:
        entry, groups = rt.lib.lynx_track_particles_along_losses, (*apertures, _ptr(lost_at))
    else:
        entry, groups = rt.lib.lynx_track_particles_along, ()
    rt.check(entry(*common, *groups))
    images = _screen_images(counts.numpy().reshape(lat.B, shots["cells"]), shots, batch_shape, dtype) if shots else []
    rec = records.numpy().reshape(*batch_shape, P, _ffi.MOMENT_STRIDE)
    energy = e_trace.numpy().reshape(*batch_shape, P)
    trace = late.BeamTrace.from_records(rec, energy, lengths, names, dtype,
                                        apertures=[step for step, _, _ in program.apertures],
                                        screens=[step for step, _ in program.screens], screen_images=images,
                                        trajectories=None if paths is None else paths.numpy().reshape(*batch_shape, P, len(chosen), 7),
                                        trajectory_indices=chosen,
                                        trajectory_lost_in=None if path_lost_in is None else path_lost_in.numpy().reshape(*batch_shape, len(chosen)))
    trace.num_particles = n
    if lost_at is not None:
        trace.lost_at = lost_at.numpy().reshape(*batch_shape, n)
    # a beam object has one particle count for all samples: with losses there is none to hand out
    if keep_outgoing and not (losses and not np.all(rec[..., -1, 35] == n)):
        e_out = Dual(np.ascontiguousarray(energy[..., -1])) if lat.has_cavity_step else None
        trace.outgoing = _outgoing_particles(incoming, Dual(dev=p_out), e_out, Dual(np.ascontiguousarray(rec[..., -1, :])))
    device = {"records": records} if paths is None else {"records": records, "trajectories": paths}
    if lost_at is not None:  # (what the reverse pass of a trace with losses makes its survivor sets from)
        device["lost_at"] = lost_at
    return trace, rec[..., :, (0, 2)].astype(dtype), device  # (mean x, y of the particles alive at every point)


def _trace_parameters(*, owner, program: Program, lat, incoming, e_in, e_trace, lengths, names, keep_outgoing, rt, make_images=True):
    """The ParameterBeam's trace: (trace, x and y of mu at every point, the device arrays a reverse pass reads).  Without
    `make_images` the active screens are points of the trace and nothing else: no image is made or read."""
    late = _late()
    dtype, batch_shape, P = incoming.dtype, incoming.batch_shape, lat.S + 1
    mu_t, cov_t = rt.empty((lat.B, P, 7), dtype), rt.empty((lat.B, P, 7, 7), dtype)
    rt.check(rt.lib.lynx_track_moments_along(
        rt.ctx, lat.handle, _ptr(e_in), _ptr(incoming._mu_d.device(rt)), _ptr(incoming._cov_d.device(rt)),
        _ptr(mu_t), _ptr(cov_t), _ptr(e_trace)))
    images = []
    if program.screens and make_images:  # from the trace arrays where the kernels wrote them, before they are read back
        shots = _screen_geometry(owner, program, batch_shape, dtype, rt, False)
        density = rt.empty((lat.B, shots["cells"]), dtype)
        rt.check(rt.lib.lynx_gaussian_images_along(
            rt.ctx, dtype_code(dtype), lat.B, P, _ptr(mu_t), _ptr(cov_t), *shots["arguments"], _ptr(density)))
        images = _screen_images(density.numpy().reshape(lat.B, shots["cells"]), shots, batch_shape, dtype)
    mu, cov = mu_t.numpy().reshape(*batch_shape, P, 7), cov_t.numpy().reshape(*batch_shape, P, 7, 7)
    energy = e_trace.numpy().reshape(*batch_shape, P)
    trace = late.BeamTrace.from_moments(mu, cov, energy, lengths, names, dtype,
                                        screens=[step for step, _ in program.screens], screen_images=images if make_images else None)
    if keep_outgoing:
        trace.outgoing = late.ParameterBeam._from_raw(
            Dual(np.ascontiguousarray(mu[..., -1, :])), Dual(np.ascontiguousarray(cov[..., -1, :, :])),
            Dual(np.ascontiguousarray(energy[..., -1])) if lat.has_cavity_step else incoming._energy, incoming.total_charge, dtype)
    return trace, mu[..., :, (0, 2)], {"mu": mu_t, "cov": cov_t}


def track_along(owner, leaves, incoming, keep_outgoing: bool = True, keep_device: bool = False, losses=False, screens: bool = False,
                trajectories=None, keep_energy: bool = False):
    """
    `Segment.track_along`: one launch sequence for the whole lattice (`lynx_track_particles_along` /
    `lynx_track_moments_along`).  The packed "every element its own step" lattice is cached on `owner` (its own
    LatticeCache: a parameter write between two calls rewrites that element's block only).  `keep_device`: the trace
    keeps the device arrays the kernels wrote (`trace._device`) -- what the reverse pass of `grad.track_along_vjp` reads;
    `keep_energy`: among them the energies at every point, where the call wrote them (what the moment loss reads).
    `losses` (True or "particles"): active apertures are part of the trace (`lynx_track_particles_along_losses`).
    `screens`: active screens are part of the trace and make their images inside it (`lynx_track_particles_along_screens`,
    with the apertures if `losses`; `lynx_gaussian_images_along` on the moment trace of a ParameterBeam).
    `screens="points"` (internal, a ParameterBeam: what `grad.track_along_vjp(..., image_targets=)` asks for): the active screens
    are identity steps and points of the trace, `trace.screens` lists them, and no image is made or read.
    `trajectories` (a number K of particles or a 1-D array of particle indices): the trace also holds the coordinates of
    those particles at every point (`lynx_track_particles_along_trajectories`: one more small kernel behind the same
    call's particle kernel); None: the call is the one it was.
    """
    late = _late()
    leaves = list(leaves)
    if not (losses is False or losses is True or losses == "particles"):
        raise ValueError(f"track_along: losses is False, True or 'particles', not {losses!r}")
    # (raises for an active Screen without `screens`, for an active Aperture without `losses`, before anything touches the GPU)
    program = _trace_plan(owner, leaves, bool(losses), bool(screens))
    if not isinstance(incoming, (late.ParameterBeam, late.ParticleBeam)):
        raise TypeError(f"Parameter incoming is of invalid type {type(incoming)}")
    points_only = isinstance(screens, str) and screens == "points"
    if points_only and not isinstance(incoming, late.ParameterBeam):
        raise TypeError('track_along: screens="points" is the trace of a ParameterBeam; a ParticleBeam\'s screens make their images')
    chosen = None if trajectories is None else chosen_particles(trajectories, incoming)
    rt = get_runtime()
    dtype, batch_shape = incoming.dtype, incoming.batch_shape
    lat = _ready(trace_cache(owner), program, batch_shape, dtype, incoming._energy._host)
    e_in = incoming._energy.broadcast_device(rt, batch_shape)
    e_trace = rt.empty_result((lat.B, lat.S + 1), dtype)
    made = dict(owner=owner, program=program, lat=lat, incoming=incoming, e_in=e_in, e_trace=e_trace, rt=rt, keep_outgoing=keep_outgoing,
                lengths=[getattr(el, "length", None) for el in leaves], names=[el.name for el in leaves])
    if isinstance(incoming, late.ParticleBeam):
        trace, centre, device = _trace_particles(**made, losses=losses, chosen=chosen)
    else:
        trace, centre, device = _trace_parameters(**made, make_images=not points_only)
    trace.total_charge = incoming.total_charge
    if keep_device:
        trace._device = {**device, "energy": e_trace} if keep_energy else device
    for k, el in enumerate(leaves):  # an active BPM reads the beam that ENTERS it: point k (bpm.py:48-54)
        if getattr(el, "_fusable_observer", False):
            el.reading = np.stack([centre[..., k, 0], centre[..., k, 1]]).astype(dtype)
    for (_, el), image in zip(program.screens, trace.screen_images):  # ... and so does an active screen
        el._reading_from_trace(image)
    return trace


def transfer_map(owner, elements, energy, dtype, raw: bool = False) -> np.ndarray:
    """`transfer_map(energy)` of a skippable element list -> host array (*batch, 7, 7)."""
    rt = get_runtime()
    dtype = np.dtype(dtype)
    energy = np.asarray(energy, dtype=dtype)
    items = plan(owner, elements, raw)
    if not items:
        return np.tile(np.eye(7, dtype=dtype), (*energy.shape, 1, 1))
    assert len(items) == 1 and isinstance(items[0], Program) and len(items[0].steps) == 1, (
        "transfer_map needs a skippable element list")
    return _composed_map(rt, lattice_cache(owner), items[0], energy, dtype)


def cavity_rmatrix(cavity, energy, dtype) -> np.ndarray:
    """`Cavity.transfer_map` = `_cavity_rmatrix` (cavity.py:248-325) whether or not it is on."""
    rt = get_runtime()
    dtype = np.dtype(dtype)
    energy = np.asarray(energy, dtype=dtype)
    program = Program(raw=True)
    program.add_run_element(cavity, True)
    return _composed_map(rt, lattice_cache(cavity), program, energy, dtype)


def _composed_map(rt, cache, program: Program, energy, dtype) -> np.ndarray:
    """The map of a program of one step at `energy` (`lynx_build_compose`) -> host array (*energy.shape, 7, 7)."""
    lat = _ready(cache, program, energy.shape, dtype, energy)
    e_in = rt.to_device(np.ascontiguousarray(energy))
    steps = rt.empty((lat.B, 1, _ffi.STEP_STRIDE), dtype)
    rt.check(rt.lib.lynx_build_compose(rt.ctx, lat.handle, _ptr(e_in), _ptr(steps), None))
    return steps.numpy()[:, 0, :49].reshape(*energy.shape, 7, 7)
