"""
Targets that live on the device and the two losses formed from them: `ImageTargets` and `MomentTargets` (each refuses by
value, lays its targets out as the library reads them and uploads them ONCE: `_DeviceTargets`), and `ImageLoss` and
`MomentLoss`, which `TrackAlongVJP` makes once its trace exists -- each owns the forward half's results on the device, what
the host reads of them, the validation of its `*_loss_bar` and the launch of its reverse half.  `ScreenCalls` is what every
image call of one `TrackAlongVJP` begins with.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import config, engine
from ..trace import point_index, screen_ordinal
from .cotangents import _ENERGY_PROPERTIES, MOMENT_PROPERTIES, batch_size, over_batch
from .track import _p


def _screen_of(key, program, leaves) -> int:
    """The ordinal among the trace's active screens of what `key` means: the `Screen` itself, or whatever `trace.image_at`
    takes (a name, the index of the point it observes) -- with that method's errors."""
    points = [step for step, _ in program.screens]
    if getattr(key, "_swallows_beam", False):  # the Screen element itself
        found = [k for k, (_, el) in enumerate(program.screens) if el is key]
        if not found:
            raise KeyError(f"{key!r} is not an active screen of this trace (screens at {points})")
        return found[0]
    return screen_ordinal([el.name for el in leaves], points, key)


class _DeviceTargets:
    """
    The memo of targets that are uploaded once: (what the layout depends on, the layout, the device array or None) of the last
    trace they met.  The same key gives the same layout object, and with it the same upload: the same targets serve every
    pass of a tuning loop.
    """

    _remembered = None

    def _remember(self, key, make):
        if self._remembered is None or self._remembered[0] != key:
            self._remembered = (key, make(), None)  # (a `make` that refuses leaves what was remembered)
        return self._remembered[1]

    def _device(self, rt, layout):
        key, remembered, dev = self._remembered
        assert remembered is layout
        if dev is None:
            dev = rt.to_device(layout.host)
            self._remembered = (key, layout, dev)
        return dev


class _TargetLayout:
    """Where the targets lie in what is uploaded: `offsets` per active screen (-1: no target), the `cells` of one row, the
    scalars between two samples' rows (`stride`, 0: one row shared by the batch) and the host array itself."""

    def __init__(self, offsets, cells, stride, host):
        self.offsets, self.cells, self.stride, self.host = offsets, cells, stride, host


class ImageTargets(_DeviceTargets):
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

    def _layout(self, program, leaves, beam) -> _TargetLayout:
        """The targets against one trace's screens and one beam, refused by value; nothing touches the GPU."""
        dtype, batch_shape = np.dtype(beam.dtype), tuple(beam.batch_shape)
        shapes = [tuple(len(v) for v in engine._pixel_positions(el, dtype)) for _, el in program.screens]
        key = (tuple(id(el) for _, el in program.screens), tuple(shapes), batch_shape, dtype.str)
        return self._remember(key, lambda: self._make(program, leaves, shapes, batch_shape, dtype))

    def _make(self, program, leaves, shapes, batch_shape, dtype) -> _TargetLayout:
        B = batch_size(batch_shape)
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
        return _TargetLayout(offsets, first, 0 if shared else max(first, 1), host)


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


class MomentTargets(_DeviceTargets):
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

    @property
    def terms(self) -> list:
        if self._remembered is None:
            raise ValueError("MomentTargets: the terms are known once the targets have met a trace -- pass them to track_along_vjp")
        return list(self._remembered[1].terms)

    def _layout(self, names, batch_shape) -> _MomentLayout:
        """The targets against the points of one trace (`names` of its elements) and one batch, refused by value; nothing
        touches the GPU."""
        batch_shape = tuple(batch_shape)
        return self._remember((tuple(names), batch_shape), lambda: self._make(names, batch_shape))

    def _make(self, names, batch_shape) -> _MomentLayout:
        found = [{}, {}]  # (point, code) -> (the value, the value over the batch), of the targets and of the weights
        for what, given, values in (("target", self._given[0], found[0]), ("weight", self._given[1], found[1])):
            for point, named in given:
                k = point_index(names, point)
                for name, value in named.items():
                    if (k, MOMENT_PROPERTIES.index(name)) in values:
                        raise ValueError(f"track_along_vjp: {name!r} at point {k} is given two {what}s")
                    values[(k, MOMENT_PROPERTIES.index(name))] = (value, over_batch(value, batch_shape, f"the {what} of {name!r} at point {k}"))
        for k, code in found[1]:
            if (k, code) not in found[0]:
                raise ValueError(f"track_along_vjp: a weight of {MOMENT_PROPERTIES[code]!r} at point {k}, which has no target")
        order = sorted(found[0])
        shared = all(value.ndim == 0 for values in found for value, _ in values.values())
        host = np.ones((1 if shared else batch_size(batch_shape), len(order), 2))
        for column, values in enumerate(found):
            for t, term in enumerate(order):
                if term in values:
                    host[:, t, column] = values[term][1][: len(host)]
        return _MomentLayout([(k, MOMENT_PROPERTIES[code]) for k, code in order], 0 if shared else 2 * len(order), host)


def loss_of(loss, what: str):
    """`loss`, the `ImageLoss` or `MomentLoss` that `what` (`image_loss`, `moment_loss_bar`, ...) reads -- or the ValueError of
    a `TrackAlongVJP` that was given no such targets."""
    if loss is None:
        raise ValueError(f"track_along_vjp: {what} needs {_NEEDS[what][0]} -- pass {_NEEDS[what][1]}= to track_along_vjp")
    return loss


_NEEDS = {  # what reads a loss: (what it needs, the keyword of track_along_vjp that gives it)
    "image_loss": ("target images", "image_targets"),
    "image_loss_of": ("target images", "image_targets"),
    "image_loss_bar": ("the image loss of the forward pass", "image_targets"),
    "moment_values": ("moment targets", "moment_targets"),
    "moment_loss": ("moment targets", "moment_targets"),
    "moment_loss_of": ("moment targets", "moment_targets"),
    "moment_loss_bar": ("the moment loss of the forward pass", "moment_targets"),
}


class ScreenCalls:
    """
    What the image calls of one `TrackAlongVJP` share: the trace's active screens, the arguments every such call begins with,
    and the geometry of the screens, looked up once -- by whichever call needs it first.
    """

    def __init__(self, segment, program, leaves, beam, trace):
        self.segment, self.program, self.leaves, self.beam, self.trace = segment, program, leaves, beam, trace
        self.elements = [el for _, el in program.screens]
        self._shots = None

    def head(self, rt, *states):
        """(ctx, dtype, B, P, the named states of the trace), and the geometry -> (head, geometry)."""
        beam = self.beam
        if self._shots is None:
            self._shots = engine._screen_geometry(self.segment, self.program, beam.batch_shape, beam.dtype, rt, False)
        return (rt.ctx, engine.dtype_code(beam.dtype), batch_size(beam.batch_shape), self.trace.num_points,
                *(_p(self.trace._device[s]) for s in states)), self._shots


class ImageLoss:
    """
    The image loss of one `TrackAlongVJP`.  lynx_gaussian_images_along_mse right behind the trace, on its stream: the loss
    [B][K] and the six adjoint sums [B][K][6] of every screen with a target, float64, both kept on the device (`loss`, `sums`;
    None without an active screen); `named`: which screens have a target.  What `values` and `of` hand out:
    `TrackAlongVJP.image_loss`, `image_loss_of`.
    """

    def __init__(self, rt, targets: ImageTargets, layout: _TargetLayout, screens: ScreenCalls):
        self.screens, self.named = screens, [offset >= 0 for offset in layout.offsets]
        self.loss = self.sums = None
        if not screens.elements:  # (no active screen, and so no target: nothing to evaluate)
            return
        head, shots = screens.head(rt, "mu", "cov")
        B, K = head[2], shots["count"]
        targets_dev = targets._device(rt, layout)
        self.loss, self.sums = rt.empty((B, K), np.float64), rt.empty((B, K, 6), np.float64)
        rt.check(rt.lib.lynx_gaussian_images_along_mse(
            *head, *shots["arguments"], (C.c_int64 * K)(*layout.offsets), _p(targets_dev), layout.stride, _p(self.loss), _p(self.sums)))

    def _host(self) -> np.ndarray:
        return self.loss.numpy().reshape(*self.screens.beam.batch_shape, len(self.named))

    def _named(self, key) -> int:
        k = _screen_of(key, self.screens.program, self.screens.leaves)
        if not self.named[k]:
            raise KeyError(f"screen {self.screens.elements[k].name!r} has no target image in this call's image_targets")
        return k

    def values(self) -> dict:
        if not any(self.named):
            return {}
        host = self._host()
        return {el.name: np.ascontiguousarray(host[..., k]) for k, el in enumerate(self.screens.elements) if self.named[k]}

    def of(self, screen) -> np.ndarray:
        k = self._named(screen)
        return np.ascontiguousarray(self._host()[..., k])

    def cotangents(self, image_loss_bar):
        """`image_loss_bar` as (B, K) of the beam's dtype, zeros for a screen without a target; refused by value.  None where
        no screen has a target: nothing to launch."""
        beam, elements = self.screens.beam, self.screens.elements
        bars = np.zeros((batch_size(beam.batch_shape), len(self.named)))
        if isinstance(image_loss_bar, dict):
            for key, bar in image_loss_bar.items():
                k = self._named(key)
                bars[:, k] += over_batch(bar, beam.batch_shape, f"image_loss_bar of screen {elements[k].name!r}")
        else:
            for k, el in enumerate(elements):
                if self.named[k]:
                    bars[:, k] = over_batch(image_loss_bar, beam.batch_shape, f"image_loss_bar of screen {el.name!r}")
        return bars.astype(beam.dtype) if any(self.named) else None

    def backward(self, rt, lb, mb_dev, cb_dev):
        """lynx_gaussian_images_along_mse_backward: `lb` times the sums of the forward pass, added into the mu and cov
        cotangents at the screens' points -> this call's part of dL/d(misalignment), [B][K][2] on the device."""
        dtype = self.screens.beam.dtype
        head, shots = self.screens.head(rt, "cov")
        lb_dev = rt.to_device(np.ascontiguousarray(lb, dtype=dtype))
        shifts = rt.empty((head[2], shots["count"], 2), dtype)
        rt.check(rt.lib.lynx_gaussian_images_along_mse_backward(
            *head, shots["count"], shots["rows"], _p(self.sums), _p(lb_dev), _p(mb_dev), _p(cb_dev), _p(shifts)))
        return shifts


class MomentLoss:
    """
    The moment loss of one `TrackAlongVJP`.  lynx_moments_along_loss right behind the trace, on its stream (`forward`): the
    value of every term [B][T], the loss per target point [B][Q] and per sample [B], float64, all kept on the device.  What
    `values`, `loss` and `of` hand out: `TrackAlongVJP.moment_values`, `moment_loss`, `moment_loss_of`.
    """

    def __init__(self, rt, targets: MomentTargets, layout: _MomentLayout, beam, trace):
        self.targets, self.layout, self.beam, self.trace = targets, layout, beam, trace
        self.forward(rt)

    def arguments(self, rt):
        """What lynx_moments_along_loss and its reverse half are given alike: sizes, the states of the trace, the terms, the rows."""
        beam, states, layout = self.beam, self.trace._device, self.layout
        return (rt.ctx, engine.dtype_code(beam.dtype), batch_size(beam.batch_shape), self.trace.num_points, _p(states.get("records")),
                _p(states.get("mu")), _p(states.get("cov")), _p(states["energy"]), int(config.std_ddof), *layout.arguments,
                _p(self.targets._device(rt, layout)), layout.stride)

    def forward(self, rt):
        B, T, Q = batch_size(self.beam.batch_shape), len(self.layout.terms), len(self.layout.points)
        self._values, self._per_point, self._loss = rt.empty((B, T), np.float64), rt.empty((B, Q), np.float64), rt.empty((B,), np.float64)
        rt.check(rt.lib.lynx_moments_along_loss(*self.arguments(rt), _p(self._values), _p(self._per_point), _p(self._loss)))

    def values(self) -> np.ndarray:
        return self._values.numpy().reshape(*self.beam.batch_shape, len(self.layout.terms))

    def loss(self) -> np.ndarray:
        return self._loss.numpy().reshape(self.beam.batch_shape)

    def of(self, point) -> np.ndarray:
        points = self.layout.points
        k = self.trace.index_of(point)
        found = [q for q, (at, _) in enumerate(points) if at == k]
        if not found:
            raise KeyError(f"point {k} has no target in this call's moment_targets (targets at {[at for at, _ in points]})")
        return np.ascontiguousarray(self._per_point.numpy().reshape(*self.beam.batch_shape, len(points))[..., found[0]])

    def cotangents(self, moment_loss_bar) -> np.ndarray:
        """`moment_loss_bar` as (B,) float64; refused by value."""
        return over_batch(moment_loss_bar, self.beam.batch_shape, "moment_loss_bar")

    def backward(self, rt, ml, eb_dev, rec_dev=None, mb_dev=None, cb_dev=None):
        """lynx_moments_along_loss_backward: every term's bar, formed from the states on the device, added into the cotangents
        the sweep reads -- the records' of a ParticleBeam, the moments' of a ParameterBeam, the energy's."""
        ml_dev = rt.to_device(ml)
        rt.check(rt.lib.lynx_moments_along_loss_backward(
            *self.arguments(rt), _p(ml_dev), _p(rec_dev), _p(mb_dev), _p(cb_dev), _p(eb_dev)))
