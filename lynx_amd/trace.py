"""
`BeamTrace`: the beam ALONG a lattice -- its moments and energy at the entrance (point 0) and behind every leaf element
(point k), for every batch sample; what `Segment.track_along` returns.

The reference holds this data in the loop of `Segment.plot_twiss` / `plot_twiss_over_lattice` (lynx/accelerator/
segment.py: `element.track(beam)` element by element, `beta_x`, `beta_y` of every intermediate beam) and in
`plot_reference_particle_traces` -- whose lines are the coordinates of single particles at every point, which no moment
holds: `track_along(..., trajectories=...)` brings those along (`ParticleBeamTrace.trajectories`); the plots themselves
are out of scope.  One deliberate departure: `plot_twiss` skips
elements of zero length altogether (it does not track through them); here every element is tracked and has a point,
and `where_length_changes()` gives the reference's subset.

Every moment property a beam has is here too, shaped (*batch, P): the formulas are the beam classes' own
(`ParticleBeam._std` with `LYNX_STD_DDOF`, `ParameterBeam._sigma`, the Twiss properties of `particles/beam.py`), applied
to all points at once.
"""

from __future__ import annotations

import numpy as np

from . import config
from .particles.beam import Beam
from .particles.parameter_beam import ParameterBeam
from .particles.particle_beam import ParticleBeam, _tri

_MOMENTS = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
            "sigma_p", "sigma_xxp", "sigma_yyp")
_DERIVED = ("emittance_x", "emittance_y", "normalized_emittance_x", "normalized_emittance_y", "beta_x", "beta_y",
            "alpha_x", "alpha_y")


def _cumulative_s(lengths, batch_shape, dtype) -> np.ndarray:
    """(P, *batch): 0, then the running sum of the elements' lengths (each broadcast over the batch)."""
    s = np.zeros((len(lengths) + 1, *batch_shape), dtype=dtype)
    for k, length in enumerate(lengths):
        length = np.asarray(0.0 if length is None else length, dtype=dtype)
        if length.size == 1:  # (an element without a length of its own carries [0.] whatever the batch)
            length = length.reshape(())
        s[k + 1] = s[k] + np.broadcast_to(length, batch_shape)
    return s


def screen_ordinal(names, screens, name_or_index) -> int:
    """
    The ordinal in `screens` (the points the active screens observe) of the screen that a name -- the element so named -- or
    a point index (negative from the end; there are len(names) + 1 points) means; KeyError if no active screen stands there.
    """
    if isinstance(name_or_index, str):
        if name_or_index not in names:
            raise KeyError(f"no element named {name_or_index!r} in this trace")
        k = names.index(name_or_index)
    else:
        k, points = int(name_or_index), len(names) + 1
        if not -points <= k < points:
            raise IndexError(f"point {k} of a trace of {points}")
        k %= points
    if k not in screens:
        raise KeyError(f"{name_or_index!r}: no active screen of this trace observes point {k} (screens at {list(screens)})")
    return list(screens).index(k)


def point_index(names, name_or_index) -> int:
    """`BeamTrace.index_of` on the element names alone (there are len(names) + 1 points): what is known before a trace exists."""
    if isinstance(name_or_index, str):
        if name_or_index not in names:
            raise KeyError(f"no element named {name_or_index!r} in this trace")
        return list(names).index(name_or_index) + 1
    k, points = int(name_or_index), len(names) + 1
    if not -points <= k < points:
        raise IndexError(f"point {k} of a trace of {points}")
    return k % points


class BeamTrace(Beam):
    """
    :ivar s: position of every point, (P, *batch) -- cumulative `length`, per sample because lengths are batched; a
        zero-length element's point has the `s` of the one before it.
    :ivar names: the P - 1 element names; point k lies behind `names[k - 1]`.
    :ivar mu: (*batch, P, 6), :ivar cov: (*batch, P, 6, 6), :ivar energy: (*batch, P).
    :ivar outgoing: the tracked beam (None if it was not kept); its moments are the last point's.

    A particle trace made with `losses` (active apertures inside the trace) also says who is left: `num_survivors`,
    `transmission`, `apertures`, `lost_in`, `lost_at` (see `ParticleBeamTrace`); they are None for a ParameterBeam.

    A trace made with `screens` (active screens inside the trace) holds their images: `screens`, the points the screens
    observe in lattice order -- a screen sees the beam that ENTERS it, so screen element k (`names[k]`) observes point k --
    and `screen_images`, one array per screen in the layout and dtype of `Screen.reading` (a list: resolutions differ);
    `image_at` finds one of them.  Both lists are empty for a trace without screens.
    """

    outgoing = None
    num_particles = None
    total_charge = None
    num_survivors = None
    transmission = None
    apertures = None
    lost_in = None
    lost_at = None
    trajectories = None
    trajectory_indices = None
    trajectory_lost_in = None
    screens = ()
    screen_images = ()
    _images_made = True

    def _set_screens(self, screens, screen_images):
        self.screens = [int(k) for k in screens]
        self._images_made = screen_images is not None  # (None: the screens are points of the trace, their images were not made)
        self.screen_images = list(screen_images) if self._images_made else []
        assert not self._images_made or len(self.screens) == len(self.screen_images), (self.screens, len(self.screen_images))
        assert all(0 <= k < self.num_points - 1 for k in self.screens), self.screens  # (a screen is an element: never the last point)

    def _set_common(self, energy, lengths, names, dtype, batch_shape):
        self.dtype = np.dtype(dtype)
        self.batch_shape = tuple(batch_shape)
        self._energy_trace = np.asarray(energy, dtype=self.dtype)
        self.names = list(names)
        self._lengths = [np.asarray(0.0 if length is None else length, dtype=self.dtype) for length in lengths]
        self.s = _cumulative_s(self._lengths, self.batch_shape, self.dtype)
        assert len(self.names) == len(self._lengths) == self.num_points - 1

    @staticmethod
    def from_records(records, energy, lengths, names, dtype=np.float32, apertures=(), screens=(), screen_images=(),
                     trajectories=None, trajectory_indices=None, trajectory_lost_in=None) -> "BeamTrace":
        """
        A particle trace from host arrays: `records` (*batch, P, 36) float64 moment records (layout of
        LYNX_MOMENT_STRIDE, include/lynx_hip.h; whole covariance triangle), `energy` (*batch, P), `lengths` the P - 1
        element lengths (each broadcastable to the batch), `names` the P - 1 element names.  Slot 35 of a record is the
        number of particles ITS moments were taken over: it may differ from point to point and from sample to sample
        (a trace with losses); `apertures`: the indices (into `names`) of the elements that removed particles.
        `screens`: the indices (into `names`) of the active screens, which are the points they observe; `screen_images`:
        their images, (*batch, ny, nx) each.  `trajectories`: (*batch, P, K, 7), the coordinates of K chosen particles
        at every point, with `trajectory_indices` (K,) and, for a trace with losses, `trajectory_lost_in` (*batch, K).
        """
        trace = ParticleBeamTrace.__new__(ParticleBeamTrace)
        trace.records = np.asarray(records, dtype=np.float64)
        assert trace.records.ndim >= 2 and trace.records.shape[-1] == 36, trace.records.shape
        trace._set_common(energy, lengths, names, dtype, trace.records.shape[:-2])
        entering = trace.records[..., 0, 35]  # nobody is lost in front of point 0
        trace.num_particles = int(entering.max()) if entering.size else 0
        trace._aperture_elements = [int(k) for k in apertures]
        assert all(0 <= k < trace.num_points - 1 for k in trace._aperture_elements), trace._aperture_elements
        trace._set_screens(screens, screen_images)
        if trajectories is not None:
            trace.trajectories = np.asarray(trajectories, dtype=trace.dtype)
            K = trace.trajectories.shape[-2]
            assert trace.trajectories.shape == (*trace.batch_shape, trace.num_points, K, 7), trace.trajectories.shape
            trace.trajectory_indices = (np.arange(K, dtype=np.int64) if trajectory_indices is None
                                        else np.asarray(trajectory_indices, dtype=np.int64))
            assert trace.trajectory_indices.shape == (K,), trace.trajectory_indices.shape
            if trajectory_lost_in is not None:
                trace.trajectory_lost_in = np.asarray(trajectory_lost_in, dtype=np.int32)
                assert trace.trajectory_lost_in.shape == (*trace.batch_shape, K), trace.trajectory_lost_in.shape
        return trace

    @staticmethod
    def from_moments(mu, cov, energy, lengths, names, dtype=np.float32, screens=(), screen_images=()) -> "BeamTrace":
        """A ParameterBeam trace: `mu` (*batch, P, 7), `cov` (*batch, P, 7, 7), the rest as for `from_records` (a
        ParameterBeam's screen image is (*batch, len(xs), len(ys)), as `Screen.reading` returns it)."""
        trace = ParameterBeamTrace.__new__(ParameterBeamTrace)
        trace._mu = np.asarray(mu, dtype=dtype)
        trace._cov = np.asarray(cov, dtype=dtype)
        trace._set_common(energy, lengths, names, dtype, trace._mu.shape[:-2])
        trace._set_screens(screens, screen_images)
        return trace

    @property
    def energy(self) -> np.ndarray:
        return self._energy_trace

    @property
    def num_points(self) -> int:
        return int(self._energy_trace.shape[-1])

    def __len__(self) -> int:
        return self.num_points

    def where_length_changes(self) -> np.ndarray:
        """
        (P,) bool: point 0 and the points behind elements whose length is not zero -- the points the reference's
        `plot_twiss` has (it passes over `length == 0` elements without tracking through them).
        """
        return np.array([True] + [bool(np.any(length != 0)) for length in self._lengths])

    def index_of(self, name_or_index) -> int:
        """Point index: an int as it is (negative from the end); a name -> the point behind the first element so named."""
        return point_index(self.names, name_or_index)

    def image_at(self, name_or_index) -> np.ndarray:
        """
        The image of one active screen: by the screen's name, or by the index of the point it observes (an int as
        `index_of` takes it, negative from the end).  A name resolves to the element so named and an index to a point;
        KeyError if no active screen of this trace stands there.
        """
        n = self.screen_at(name_or_index)
        if not self._images_made:
            raise KeyError(f"{name_or_index!r}: the images of this trace were not made (its screens are points of the trace alone); "
                           "pass screens=True to have them made")
        return self.screen_images[n]

    def screen_at(self, name_or_index) -> int:
        """Which of `screens` (its ordinal) a name or a point index means, by the rules and with the errors of `image_at`."""
        return screen_ordinal(self.names, self.screens, name_or_index)

    def at(self, name_or_index) -> dict:
        """Everything known about one point: `s`, `name` (None for point 0), `energy`, `mu`, `cov` and every moment --
        and, for a trace with trajectories, `trajectories`: the chosen particles there, (*batch, K, 7)."""
        k = self.index_of(name_or_index)
        out = {"index": k, "name": self.names[k - 1] if k else None, "s": self.s[k], "energy": self.energy[..., k],
               "mu": self.mu[..., k, :], "cov": self.cov[..., k, :, :]}
        for key in _MOMENTS + _DERIVED:
            out[key] = getattr(self, key)[..., k]
        if self.trajectories is not None:
            out["trajectories"] = self.trajectories[..., k, :, :]
        return out

    def __repr__(self) -> str:
        return f"{type(self).__name__}(points={self.num_points}, batch={self.batch_shape}, dtype={self.dtype.name})"


class ParticleBeamTrace(BeamTrace):
    """
    Trace of a `ParticleBeam`: one float64 moment record per sample and point (`records`, (*batch, P, 36)).  Every
    moment of a point is taken over the particles alive there (slot 35 of its record); a point nobody reaches has count
    0 and NaN moments.

    :ivar num_particles: the incoming N.
    :ivar lost_at: (*batch, N) int32, the ordinal in `apertures` of the aperture that removed each particle, -1 for a
        survivor (`losses="particles"`; else None).
    :ivar trajectories: (*batch, P, K, 7) in the beam's dtype, the coordinates of chosen particle j at point k -- point 0
        is the incoming particle (`trajectories=`; else None).  With `losses` a particle removed by the aperture that is
        element k still has its coordinates at point k (it entered the aperture there) and is NaN in all seven columns
        from point k + 1 on.
    :ivar trajectory_indices: (K,) int64, which particles those are.
    :ivar trajectory_lost_in: (*batch, K) int32, `lost_at[..., trajectory_indices]` -- with `losses=True` as well, without
        the (*batch, N) array of `losses="particles"` (None without `losses`).
    """

    _aperture_elements = ()

    def moment_record(self, covariance: bool = False) -> np.ndarray:
        return self.records

    @property
    def num_survivors(self) -> np.ndarray:
        """(*batch, P) int64: the particles alive at every point."""
        return self.records[..., 35].astype(np.int64)

    @property
    def transmission(self) -> np.ndarray:
        """(*batch, P): `num_survivors / num_particles`."""
        return self.num_survivors / self.num_particles

    @property
    def apertures(self) -> list:
        """Names of the active apertures of the trace, in lattice order."""
        return [self.names[k] for k in self._aperture_elements]

    @property
    def lost_in(self) -> np.ndarray:
        """(*batch, A) int64: the particles each aperture removed -- the drop of `num_survivors` across its point."""
        alive = self.num_survivors
        k = np.asarray(self._aperture_elements, dtype=np.int64)
        return alive[..., k] - alive[..., k + 1]

    # the ParticleBeam's own read-out of a record (LYNX_STD_DDOF and all), on (*batch, P) records -- with each record's
    # own count, and a single particle having no spread: where one particle is left of many, the difference of sums the
    # record holds is rounding noise of either sign instead of the 0 it stands for (sigma: NaN unbiased, 0 biased)
    _mean = ParticleBeam._mean

    def _central(self, i: int, j: int) -> np.ndarray:
        value = self.records[..., _tri(i, j)]
        return np.where((self.records[..., 35] == 1) & np.isfinite(value), 0.0, value)  # (a NaN stays one)

    def _std(self, c: int) -> np.ndarray:
        n = self.records[..., 35]
        with np.errstate(all="ignore"):
            return np.sqrt(self._central(c, c) * (n / (n - config.std_ddof))).astype(self.dtype)

    def _cov(self, i: int, j: int) -> np.ndarray:
        return self._central(i, j).astype(self.dtype)

    @property
    def mu(self) -> np.ndarray:
        return self.records[..., :6].astype(self.dtype)

    @property
    def cov(self) -> np.ndarray:
        """Biased 6 x 6 covariance of the particles at every point, (*batch, P, 6, 6)."""
        out = np.empty((*self.records.shape[:-1], 6, 6), dtype=self.dtype)
        for i in range(6):
            for j in range(i, 6):
                out[..., i, j] = out[..., j, i] = self._central(i, j)
        return out


class ParameterBeamTrace(BeamTrace):
    """Trace of a `ParameterBeam`: `mu` and `cov` as the kernels wrote them."""

    _sigma = ParameterBeam._sigma

    @property
    def mu(self) -> np.ndarray:
        return self._mu[..., :6]

    @property
    def cov(self) -> np.ndarray:
        return self._cov[..., :6, :6]


for _key in _MOMENTS:
    setattr(ParticleBeamTrace, _key, getattr(ParticleBeam, _key))
    setattr(ParameterBeamTrace, _key, getattr(ParameterBeam, _key))
