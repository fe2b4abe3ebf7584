"""
Forward mode: `track_along_jvp`, the tangents of the beam's moments at every point of a trace along a few directions, and
`orbit_response_matrix`, which reads the response of every BPM to every corrector from one such call.  `_jvp_directions` turns
`wrt` into the CSR form the library reads and `_jvp_program` refuses by value; `TrackAlongJVP` makes the trace and runs the
sweep (lynx_track_moments_along_forward, _forward_cavities, lynx_track_particles_along_forward).
"""

import ctypes as C

import numpy as np

from .. import _ffi, device, engine
from ..accelerator.diagnostics import BPM
from ..accelerator.magnets import Cavity, HorizontalCorrector, RBend, VerticalCorrector
from ..particles.parameter_beam import ParameterBeam
from ..particles.particle_beam import ParticleBeam
from .cotangents import _ENERGY_PROPERTIES, batch_size, trace_property_cotangents
from .gradients import DIFFERENTIABLE_KINDS
from .track import _p, leaves_of

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
    if not isinstance(beam, (ParameterBeam, ParticleBeam)):
        raise TypeError(f"track_along_jvp needs a ParticleBeam or a ParameterBeam, not {type(beam)}")
    if not isinstance(cavities, (bool, np.bool_)):
        raise ValueError(f"track_along_jvp: cavities is True or False, not {cavities!r}")
    leaves = leaves_of(segment)
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
        self._energy_seeds = np.array([1.0 if isinstance(item, str) else 0.0 for item in self.wrt])  # the incoming energy's tangent, per direction
        self.trace = engine.track_along(segment, self.leaves, beam, keep_outgoing=True, keep_device=True)
        rt = device.get_runtime()
        batch_shape, dtype = beam.batch_shape, beam.dtype
        B, D, P = batch_size(batch_shape), len(self.wrt), self.trace.num_points
        lat = engine._ready(engine.trace_cache(segment), self.program, batch_shape, dtype, beam._energy._host)
        e_in = beam._energy.broadcast_device(rt, batch_shape)
        self._mu_dot_dev, self._cov_dot_dev = rt.empty((B, D, P, 7), np.float64), rt.empty((B, D, P, 7, 7), np.float64)
        self._energy_dot_dev = rt.empty((B, D, P), np.float64) if self._kicks else None
        self._read_back = {}
        # one call, three entries: what they are given differs in the states of the trace in front and, through cavity steps
        # (a ParameterBeam: `_jvp_program`), in the energy's seeds and tangents behind
        start, leaf, row, weight = self._directions
        as_ints = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        as_doubles = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        states = self.trace._device
        if isinstance(beam, ParticleBeam):
            entry, given = rt.lib.lynx_track_particles_along_forward, (beam.num_particles, _p(e_in), _p(states["records"]))
        else:
            entry = rt.lib.lynx_track_moments_along_forward_cavities if self._kicks else rt.lib.lynx_track_moments_along_forward
            given = (_p(e_in), _p(states["mu"]), _p(states["cov"]))
        energies = (as_doubles(self._energy_seeds), _p(self._energy_dot_dev)) if self._kicks else ()
        rt.check(entry(rt.ctx, lat.handle, *given, as_ints(start), as_ints(leaf), as_ints(row), as_doubles(weight), D, len(leaf),
                       _p(self._mu_dot_dev), _p(self._cov_dot_dev), *energies))

    def _host(self, name, dev, *tail) -> np.ndarray:  # a tangent array (*batch, D, P, *tail), read from the device once
        if name not in self._read_back:
            self._read_back[name] = dev.numpy().reshape(*self.beam.batch_shape, len(self.wrt), self.trace.num_points, *tail)
        return self._read_back[name]

    @property
    def mu_dot(self) -> np.ndarray:
        """(*batch, D, P, 7) float64: the tangent of the mean at every point along every direction; entry 6 is an exact zero."""
        return self._host("mu_dot", self._mu_dot_dev, 7)

    @property
    def cov_dot(self) -> np.ndarray:
        """(*batch, D, P, 7, 7) float64: the tangent of the covariance (a ParticleBeam's: the biased one); row and column 6 are
        exact zeros."""
        return self._host("cov_dot", self._cov_dot_dev, 7, 7)

    @property
    def energy_dot(self) -> np.ndarray:
        """(D,): the tangent of the energy at every point -- without a cavity the incoming one: 1 along "energy", 0 otherwise.
        Through cavity steps (`cavities=True` on a lattice that has one): (*batch, D, P) float64, read from the device."""
        return self._host("energy_dot", self._energy_dot_dev) if self._kicks else self._energy_seeds.copy()

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
    leaves = leaves_of(segment)

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
