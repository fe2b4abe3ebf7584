"""
`Segment.track_along(..., trajectories=...)` on the GPU: the coordinates of chosen particles at every point.

Three references.  (1) What the product already computes, bit for bit: the incoming particles (point 0), `outgoing` of the
same call (last point), and `outgoing` of `track_along` on the first k leaves (point k) -- this is what holds
k_trace_trajectories to the streaming kernel's arithmetic.  (2) The oracle's element-by-element chain of
`tests/test_gpu_trace.py` (`chain`: a float32 active cavity by the kernels' form of the kick, the rule
`tests/test_gpu_parity.py` documents), every point of every chosen particle, column by column under `rel_err` at TOL_P --
the measure and tolerance of the particle parity tests.  (3) The same call without `trajectories`: nothing else of the
trace moves.

Sizes: a tile of the trajectory kernel is 128 chosen particles in float32 and 64 in float64, so K = 1, 63, 64, 65, 127,
128, 129, 130 puts both dtypes below, on and above a tile boundary and into a second workgroup per sample; N = 1, 63, 64,
1000 are the beam sizes of the neighbouring trace tests at which the particle kernel changes path.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice, rel_err
from .test_gpu_parity import TOL_P
from .test_gpu_trace import SIGMA, chain, mixed_desc
from .test_gpu_trace_screens import SCREEN_A, SCREEN_B

pytestmark = pytest.mark.gpu

KS = [1, 63, 64, 65, 127, 128, 129, 130]
CAVITY = 10  # its place in mixed_desc: point CAVITY + 1 lies directly behind it


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    raw = np.dtype(f"u{a.dtype.itemsize}")
    return np.array_equal(a.view(raw), b.view(raw))


def selection(K, n, seed=0):
    """K indices into a beam of n: random with repeats, the first three descending with a repeat (n - 1, n - 1, 0)."""
    idx = np.random.default_rng(100 + K + seed).integers(0, n, K)
    idx[:3] = [n - 1, n - 1, 0][:K]
    return idx


def assert_against_chain(paths, idx, beams, dtype):
    """Every point of every chosen particle against the oracle's particles there: rel_err per column at TOL_P."""
    worst = 0.0
    assert paths.shape[-3] == len(beams)
    for k, beam in enumerate(beams):
        for c in range(7):
            err = rel_err(paths[..., k, :, c], beam["particles"][..., idx, c])
            worst = max(worst, err)
            assert err < TOL_P[np.dtype(dtype).type], (k, c, err)
    return worst


@pytest.fixture(scope="module")
def mixed(lx):
    """The lattice of every element kind, its beam, its plain trace and the oracle's chain, once per (dtype, shape, n, shared)."""
    made = {}

    def get(dtype, shape, n, shared=False):
        key = (np.dtype(dtype).name, shape, n, shared)
        if key not in made:
            desc = mixed_desc(shape, np.random.default_rng(21))
            elements, specs = make_lattice(desc, dtype, lx)
            energy = np.full(shape, 1e8, dtype=dtype)
            if shared:
                one = o.gaussian_particles((1,), n, seed=3 + n, dtype=dtype, sigma=SIGMA)
                beam = lx.ParticleBeam(one, np.array([1e8], dtype=dtype), dtype=dtype).broadcast(shape)
                assert beam.is_shared
                P = np.ascontiguousarray(np.broadcast_to(one[0], (*shape, n, 7)))
            else:
                P = o.gaussian_particles(shape, n, seed=3 + n, dtype=dtype, sigma=SIGMA)
                beam = lx.ParticleBeam(P, energy, dtype=dtype)
            segment = lx.Segment(elements)
            plain = segment.track_along(beam)
            readings = [np.array(el.reading) for el in elements if getattr(el, "reading", None) is not None]
            beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
            made[key] = dict(desc=desc, elements=elements, segment=segment, beam=beam, P=P, plain=plain, readings=readings,
                             beams=beams, out=np.asarray(plain.outgoing.particles))
        return made[key]

    return get


def check_mixed(case, dtype, shape, n, Ks):
    segment, beam, P, plain = case["segment"], case["beam"], case["P"], case["plain"]
    points = len(case["desc"]) + 1
    worst = 0.0
    for K in Ks:
        idx = selection(K, n)
        trace = segment.track_along(beam, trajectories=idx)
        paths = trace.trajectories
        # (1) fails without the feature
        assert paths is not None and paths.shape == (*shape, points, K, 7) and paths.dtype == np.dtype(dtype)
        assert trace.trajectory_indices.dtype == np.int64 and np.array_equal(trace.trajectory_indices, idx)
        assert trace.trajectory_lost_in is None
        assert same_bits(trace.at(5)["trajectories"], paths[..., 5, :, :])
        # (2) bit for bit: the incoming particles, and the outgoing ones of this call and of the call without trajectories
        assert same_bits(paths[..., 0, :, :], P[..., idx, :]), K
        assert same_bits(paths[..., -1, :, :], np.asarray(trace.outgoing.particles)[..., idx, :]), K
        assert same_bits(paths[..., -1, :, :], case["out"][..., idx, :]), K
        # (4) the rest of the trace does not move
        assert np.array_equal(trace.records, plain.records) and same_bits(trace.energy, plain.energy)
        assert same_bits(np.asarray(trace.outgoing.particles), case["out"])
        now = [np.array(el.reading) for el in case["elements"] if getattr(el, "reading", None) is not None]
        assert len(now) == len(case["readings"]) == 2 and all(same_bits(a, b) for a, b in zip(now, case["readings"]))
        # (3) the oracle
        worst = max(worst, assert_against_chain(paths, idx, case["beams"], dtype))
    print(f"trajectories: worst rel_err against the chain {worst:.2e}")


@pytest.mark.parametrize("n", [1, 63, 64, 1000])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chosen_particles_at_every_point_of_every_element_kind(lx, mixed, dtype, shape, n):
    check_mixed(mixed(dtype, shape, n), dtype, shape, n, KS)


@pytest.mark.parametrize("n", [64, 1000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_shared_incoming_beam(lx, mixed, dtype, n):
    check_mixed(mixed(dtype, (3,), n, shared=True), dtype, (3,), n, [1, 65, 129])


@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_point_k_is_the_outgoing_beam_of_the_first_k_leaves(lx, mixed, dtype, shape):
    n = 1000
    case = mixed(dtype, shape, n)
    idx = selection(129, n)
    paths = case["segment"].track_along(case["beam"], trajectories=idx).trajectories
    for k in (3, CAVITY + 1, len(case["desc"]) - 1):
        head = lx.Segment(case["elements"][:k]).track_along(case["beam"])
        assert head.num_points == k + 1
        assert same_bits(paths[..., k, :, :], np.asarray(head.outgoing.particles)[..., idx, :]), k
    assert case["desc"][CAVITY][0] == "cavity"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_number_of_particles_and_a_trace_without_outgoing(lx, mixed, dtype):
    n, shape = 1000, (3,)
    case = mixed(dtype, shape, n)
    counted = case["segment"].track_along(case["beam"], trajectories=130)
    listed = case["segment"].track_along(case["beam"], trajectories=np.arange(130), keep_outgoing=False)
    assert counted.trajectory_indices.tolist() == list(range(130)) and listed.outgoing is None
    assert same_bits(counted.trajectories, listed.trajectories)
    assert same_bits(counted.trajectories[..., -1, :, :], case["out"][..., :130, :])
    assert np.array_equal(listed.records, case["plain"].records)
    whole = case["segment"].track_along(case["beam"], trajectories=n)  # every particle: eight workgroups per sample in float32
    assert same_bits(whole.trajectories[..., -1, :, :], case["out"]) and same_bits(whole.trajectories[..., 0, :, :], case["P"])


# ---------------------------------------------------------------------------------------------
# losses and screens
# ---------------------------------------------------------------------------------------------


def collimated(lx, dtype, shape, apertures, screens):
    """A drift, a collimator (elliptical, batched x_max), an active BPM, a screen, a quadrupole, a second collimator
    (rectangular, batched x_max), a second screen; the limits at about one sigma of SIGMA's beam."""
    B = int(np.prod(shape))
    f = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    ramp = lambda a, b: np.linspace(a, b, B).reshape(shape).astype(dtype)  # noqa: E731
    zero = np.zeros((*shape, 2), dtype=dtype)
    return [
        lx.Drift(f(0.5), dtype=dtype),
        lx.Aperture(x_max=ramp(0.9e-4, 1.3e-4), y_max=f(1.2e-4), shape="elliptical", is_active=apertures, name="COL1", dtype=dtype),
        lx.BPM(is_active=True, name="BPM1"),
        lx.Screen(**SCREEN_A, misalignment=zero, is_active=screens, name="SCR1", dtype=dtype),
        lx.Quadrupole(f(0.2), k1=f(4.0), dtype=dtype),
        lx.Drift(f(1.0), dtype=dtype),
        lx.Aperture(x_max=ramp(0.5e-4, 0.7e-4), y_max=f(0.8e-4), shape="rectangular", is_active=apertures, name="COL2", dtype=dtype),
        lx.Drift(f(0.3), dtype=dtype),
        lx.Screen(**SCREEN_B, misalignment=zero, is_active=screens, name="SCR2", dtype=dtype),
        lx.Drift(f(0.2), dtype=dtype),
    ]


def gaussian_beam(lx, dtype, shape, n=1000):
    P = o.gaussian_particles(shape, n, seed=11, dtype=dtype, sigma=SIGMA)
    return P, lx.ParticleBeam(P, np.full(shape, 1e8, dtype=dtype), dtype=dtype)


@pytest.mark.parametrize("screens", [False, True])
@pytest.mark.parametrize("losses", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_rest_of_the_trace_does_not_move(lx, dtype, losses, screens):
    shape, n = (3,), 1000
    elements = collimated(lx, dtype, shape, apertures=losses, screens=screens)
    segment = lx.Segment(elements)
    P, beam = gaussian_beam(lx, dtype, shape, n)
    mode = dict(losses="particles" if losses else False, screens=screens)
    plain = segment.track_along(beam, **mode)
    reading = np.array(elements[2].reading)
    idx = selection(129, n)
    trace = segment.track_along(beam, trajectories=idx, **mode)
    assert trace.trajectories.shape == (*shape, len(elements) + 1, 129, 7)
    assert np.array_equal(trace.records, plain.records, equal_nan=True) and same_bits(trace.energy, plain.energy)
    assert np.array_equal(trace.num_survivors, plain.num_survivors) and same_bits(np.array(elements[2].reading), reading)
    assert trace.screens == plain.screens and len(trace.screen_images) == (2 if screens else 0)
    for got, want in zip(trace.screen_images, plain.screen_images):
        assert same_bits(got, want) and got.sum() > 0
    if losses:
        assert same_bits(trace.lost_at, plain.lost_at) and (plain.lost_at >= 0).any() and trace.outgoing is None
        assert same_bits(trace.trajectory_lost_in, plain.lost_at[..., idx])
    else:
        assert trace.lost_at is None and trace.trajectory_lost_in is None
        assert same_bits(np.asarray(trace.outgoing.particles), np.asarray(plain.outgoing.particles))
        assert same_bits(trace.trajectories[..., -1, :, :], np.asarray(plain.outgoing.particles)[..., idx, :])
    assert same_bits(trace.trajectories[..., 0, :, :], P[..., idx, :])


@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_lost_particle_has_its_trajectory_up_to_the_aperture_that_removed_it(lx, dtype, shape):
    n = 1000
    elements = collimated(lx, dtype, shape, apertures=True, screens=False)
    segment = lx.Segment(elements)
    P, beam = gaussian_beam(lx, dtype, shape, n)
    points = len(elements) + 1
    full = segment.track_along(beam, losses="particles")
    # the inputs: each collimator removes some particles of every sample and leaves some
    assert full.apertures == ["COL1", "COL2"] and np.all(full.lost_in > 0) and np.all(full.num_survivors[..., -1] > 0)
    open_segment = lx.Segment(collimated(lx, dtype, shape, apertures=False, screens=False))
    where = np.array([1, 6])  # the collimators' places in the lattice: the points at which they test the particles
    for selected in (selection(129, n), n):
        trace = segment.track_along(beam, losses=True, trajectories=selected)
        idx = trace.trajectory_indices
        paths, lost_in = trace.trajectories, trace.trajectory_lost_in
        assert trace.lost_at is None and lost_in.shape == (*shape, len(idx)) and lost_in.dtype == np.int32
        assert same_bits(lost_in, full.lost_at[..., idx])
        assert np.array_equal(trace.records, full.records, equal_nan=True)
        finite = np.isfinite(paths)
        assert np.array_equal(finite.all(axis=-1), finite.any(axis=-1))  # all seven columns or none
        last = np.where(lost_in >= 0, where[np.maximum(lost_in, 0)], points - 1)  # the last point a particle has coordinates at
        want = np.arange(points).reshape((1,) * len(shape) + (points, 1)) <= last[..., None, :]
        assert np.array_equal(finite.all(axis=-1), want)
        assert np.isnan(paths[~finite]).all()
        # a survivor: the trajectory through the same lattice with the collimators inactive, bit for bit -- and so is a lost
        # particle as far as it got
        free = open_segment.track_along(beam, trajectories=selected).trajectories
        assert np.isfinite(free).all()
        assert same_bits(np.where(finite, paths, 0), np.where(finite, free, 0))
        survivor = lost_in < 0
        assert survivor.any() and (~survivor).any()
        assert same_bits(paths.swapaxes(-3, -2)[survivor], free.swapaxes(-3, -2)[survivor])
        if isinstance(selected, int):  # every particle: the rows with coordinates are the survivors of every point
            assert np.array_equal(finite.all(axis=-1).sum(axis=-1), trace.num_survivors)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resolution_gives_a_point_per_split_element(lx, dtype):
    shape = (2,)
    f = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(0.45), dtype=dtype), lx.Quadrupole(f(0.2), k1=f(3.0), dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                          lx.Quadrupole(f(0.2), k1=f(-3.0), dtype=dtype), lx.Drift(f(0.25), dtype=dtype)])
    P, beam = gaussian_beam(lx, dtype, shape, 64)
    pieces = segment.split(0.1)
    assert len(pieces) > len(segment.elements)
    trace = segment.track_along(beam, resolution=0.1, trajectories=3)
    assert trace.num_points == len(pieces) + 1 and trace.trajectories.shape == (*shape, len(pieces) + 1, 3, 7)
    s = np.asarray(trace.s, dtype=np.float64)
    assert np.all(np.diff(s, axis=0) >= 0) and np.allclose(s[-1], 1.6, rtol=1e-6) and np.all(s[0] == 0)
    assert same_bits(trace.trajectories[..., -1, :, :], np.asarray(trace.outgoing.particles)[..., :3, :])
    assert same_bits(trace.trajectories[..., 0, :, :], P[..., :3, :])
    # x moves from point to point: these are trajectories, not one point repeated
    assert np.all(np.abs(np.diff(trace.trajectories[..., :, :, 0], axis=-2)).max(axis=-2) > 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_parameter_write_between_two_calls_is_seen(lx, mixed, dtype):
    shape, n = (3,), 64
    desc = mixed_desc(shape, np.random.default_rng(21))
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    P, beam = gaussian_beam(lx, dtype, shape, n)
    idx = selection(65, n)
    before = segment.track_along(beam, trajectories=idx).trajectories
    assert desc[2][0] == "quadrupole"
    k1 = np.asarray([1.5, -2.5, 0.5], dtype=dtype)
    elements[2].k1 = k1
    after = segment.track_along(beam, trajectories=idx).trajectories
    fresh_desc = [(kind, dict(kw, k1=k1) if k == 2 else kw) for k, (kind, kw) in enumerate(desc)]
    fresh_elements, specs = make_lattice(fresh_desc, dtype, lx)
    fresh = lx.Segment(fresh_elements).track_along(beam, trajectories=idx).trajectories
    assert same_bits(after, fresh) and not same_bits(after, before)
    assert same_bits(after[..., :3, :, :], before[..., :3, :, :])  # in front of the quadrupole nothing changed
    beams, _ = chain(specs, o.particle_beam(P, np.full(shape, 1e8, dtype=dtype), dtype), dtype)
    assert_against_chain(after, idx, beams, dtype)
