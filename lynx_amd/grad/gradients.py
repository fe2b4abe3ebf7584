"""
What a reverse pass hands back: `Gradients`, the raw `[B][E][8]` result of one library call shaped per element on first access,
`ChainedGradients` of a lattice differentiated stretch by stretch, and the kinds of element whose parameter row is
differentiated.  Nothing here launches anything; a device array is read when its gradient is asked for.
"""

import numpy as np

from .. import _ffi
from ..accelerator.magnets import RBend

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
