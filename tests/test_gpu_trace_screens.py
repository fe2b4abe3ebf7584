"""
`Segment.track_along(..., screens=True)` on the GPU: active screens inside the beam trace.

A ParticleBeam's image is the reference's (screen.py:196-213): `flipud(histogramdd((x - misalignment_x, y), pixel_bin_edges).T)`
of the particles that ENTER the screen and are alive there -- `o.screen_reading_particles` of those particles, the
misalignment taken off x in the lattice's dtype first.  Where the particles come from the product itself (the outgoing
particles of the same trace, or of the plain trace of the prefix: a particle's coordinates at a point depend on itself and
the steps in front of it alone) the comparison is exact.  Against the oracle's own chain a particle may fall into the
neighbouring pixel if it lies within the particle tolerance of an edge: the float64 chain says which particles those are,
and sum |image - ref| <= 2 x (their number) is asserted (EDGE below).

Screens: effective 20 x 12 (40 x 24 at binning 2) with square pixels of sigma / 4 and a misalignment per sample, and an odd
33 x 17 with pixels of sigma / 5 by sigma / 4.5 and a shared misalignment; both extents cut the beam (2.5 and 1.5 sigma;
3.3 and 1.9 sigma).
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice
from .test_gpu_parity import TOL_P
from .test_gpu_trace import SIGMA, chain, upcast
from .test_gpu_trace_losses import EDGE as LOSSES_EDGE
from .test_gpu_trace_losses import criterion

pytestmark = pytest.mark.gpu

SCREEN_A = dict(resolution=(40, 24), pixel_size=(1.25e-5, 1.25e-5), binning=2)
SCREEN_B = dict(resolution=(33, 17), pixel_size=(2e-5, 2.2e-5), binning=1)
SHAPE_A, SHAPE_B = (12, 20), (17, 33)  # (ny, nx)
MIS_B = np.array([2e-5, -1e-5])
SIZES = [1, 63, 64, 127, 128, 129, 255, 256, 257, 1000, 70_001]  # tiles: 256 float32 / 128 float64 particles

# A particle is ON AN EDGE if the float64 chain puts x - misalignment_x or y within EDGE * sigma (of that coordinate, at that
# point, per sample) of a bin edge: EDGE is the particle tolerance of the plain-trace tests.  Pixels of sigma / 5 make that
# 2 EDGE / (1 / 5) = 1e-3 of the particles per axis in float32, 2e-3 in all: the inputs are held to at most 1 % of n per
# sample and screen, and to none at all for n <= 1000 (seeds searched on the host with the oracle alone; two particles of
# 1000 are expected on an edge per sample and screen, so the case of 1000 particles has one sample).
EDGE = TOL_P
ORACLE_CASES = [(257, (3,)), (1000, (1,)), (70_001, (3,))]
SEEDS = {257: 28, 1000: 41, 70_001: 0}


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


def mis_a(shape):
    return np.random.default_rng(8).normal(0, 3e-5, (*shape, 2))


def make_screen(lx, geometry, misalignment, dtype, name, is_active=True):
    return lx.Screen(**geometry, misalignment=np.asarray(misalignment, dtype=dtype), is_active=is_active, name=name, dtype=dtype)


def shifted(particles, misalignment, dtype):
    """`Screen._observe`: x less the x misalignment, in the dtype (the y misalignment goes to x', which no image sees)."""
    out = np.array(particles, dtype=dtype)
    out[..., 0] = out[..., 0] - np.asarray(misalignment, dtype=dtype)[..., None, 0]
    return out


def oracle_image(particles, misalignment, geometry, dtype, alive=None):
    """The reference's image; with `alive` (*batch, N) of every sample's own survivors."""
    P = shifted(particles, misalignment, dtype)
    if alive is None:
        return o.screen_reading_particles(P, **geometry, dtype=dtype)
    batch = P.shape[:-2]
    nx, ny = (int(r / geometry["binning"]) for r in geometry["resolution"])
    out = np.zeros((*batch, ny, nx), dtype=dtype)
    for b in np.ndindex(*batch):
        if alive[b].any():
            out[b] = o.screen_reading_particles(P[b][alive[b]], **geometry, dtype=dtype)
    return out


def optics(lx, shape, dtype):
    """Drift, quadrupole with a strength per sample, [screen A], corrector, drift, [screen B]: the four magnets."""
    f = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    k1 = np.linspace(-4.0, 5.0, int(np.prod(shape))).reshape(shape).astype(dtype)
    return [lx.Drift(f(0.6), dtype=dtype), lx.Quadrupole(f(0.2), k1=k1, dtype=dtype),
            lx.HorizontalCorrector(f(0.1), angle=f(3e-5), dtype=dtype), lx.Drift(f(0.8), dtype=dtype)]


def two_screen_lattice(lx, shape, dtype, is_active=True):
    d1, q, h, d2 = optics(lx, shape, dtype)
    a = make_screen(lx, SCREEN_A, mis_a(shape), dtype, "SCREEN_A", is_active)
    b = make_screen(lx, SCREEN_B, MIS_B, dtype, "SCREEN_B", is_active)
    return [d1, q, a, h, d2, b], a, b


def beam_of(lx, shape, n, dtype, seed=None):
    P = o.gaussian_particles(shape, n, seed=11 + n if seed is None else seed, dtype=dtype, sigma=SIGMA)
    return P, lx.ParticleBeam(P, np.full(shape, 1e8, dtype=dtype), dtype=dtype)


# ---------------------------------------------------------------------------------------------
# 1. exact, at every tile boundary
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_images_are_exact_at_every_tile_boundary(lx, dtype, shape, n):
    elements, a, b = two_screen_lattice(lx, shape, dtype)
    P, beam = beam_of(lx, shape, n, dtype)
    trace = lx.Segment(elements).track_along(beam, screens=True)
    assert trace.screens == [2, 5] and len(trace.screen_images) == 2
    image_a, image_b = trace.image_at("SCREEN_A"), trace.image_at("SCREEN_B")
    assert image_a.shape == (*shape, *SHAPE_A) and image_b.shape == (*shape, *SHAPE_B)
    assert image_a.dtype == image_b.dtype == np.dtype(dtype)
    # the last element is a screen and an identity: the outgoing particles of this very call entered it
    entering_b = np.asarray(trace.outgoing.particles)
    want_b = oracle_image(entering_b, MIS_B, SCREEN_B, dtype)
    assert np.array_equal(image_b, want_b), (int(np.abs(image_b - want_b).sum()), image_b.sum(), want_b.sum())
    # screen A: the outgoing particles of the plain trace of what stands in front of it
    entering_a = np.asarray(lx.Segment(elements[:2]).track_along(beam).outgoing.particles)
    want_a = oracle_image(entering_a, mis_a(shape), SCREEN_A, dtype)
    assert np.array_equal(image_a, want_a), (int(np.abs(image_a - want_a).sum()), image_a.sum(), want_a.sum())
    if n >= 1000:  # the extents cut the beam, and most of it is seen
        assert np.all(image_b.sum(axis=(-2, -1)) < n) and np.all(image_b.sum(axis=(-2, -1)) > 0.3 * n)
        assert np.all(image_a.sum(axis=(-2, -1)) < n) and np.all(image_a.sum(axis=(-2, -1)) > 0.3 * n)


# ---------------------------------------------------------------------------------------------
# 2. the bin rule
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_values_on_bin_edges_go_where_numpy_puts_them(lx, dtype):
    res, px, binning = (200, 120), (3.5e-6, 2.5e-6), 2
    P = o.gaussian_particles((3,), 5000, seed=1, dtype=dtype, mu=[5e-5, 0, -3e-5, 0, 0, 0], sigma=[1.2e-4, 1e-5, 0.9e-4, 1e-5, 1e-5, 1e-3])
    edges = o.screen_bin_edges(res, px, binning, dtype)
    for b in range(3):  # every edge of both axes, the first and the last included, in every sample; and values just outside
        P[b, :101, 0] = edges[0]
        P[b, 101:162, 2] = edges[1]
        P[b, 162, 0], P[b, 163, 0] = np.nextafter(edges[0][-1], dtype(1)), np.nextafter(edges[0][0], dtype(-1))
        P[b, 164, 2], P[b, 165, 2] = np.nextafter(edges[1][-1], dtype(1)), np.nextafter(edges[1][0], dtype(-1))
        P[b, 166, 0], P[b, 167, 2], P[b, 168, 0] = np.nan, np.inf, -np.inf
    kw = dict(resolution=res, pixel_size=px, binning=binning, misalignment=np.zeros((3, 2)), is_active=True, dtype=dtype)
    f = lambda v: np.full(3, v, dtype=dtype)  # noqa: E731
    first = lx.Screen(**kw, name="FIRST")
    beam = lx.ParticleBeam(P, f(1e8), dtype=dtype)
    trace = lx.Segment([first, lx.Drift(f(1.0), dtype=dtype)]).track_along(beam, screens=True)
    image = trace.image_at("FIRST")
    with np.errstate(all="ignore"):
        ref = o.screen_reading_particles(P, res, px, binning, dtype)
    assert image.shape == (3, 60, 100) == ref.shape and trace.screens == [0]
    assert np.array_equal(image, ref), int(np.abs(image - ref).sum())
    # ... and where the screen read-out of `Screen.track` puts them
    alone = lx.Screen(**kw, name="ALONE")
    assert alone.track(beam) is lx.Beam.empty
    assert np.array_equal(image, alone.reading)
    assert 0 < image.sum() < 3 * 5000


# ---------------------------------------------------------------------------------------------
# 3. with losses
# ---------------------------------------------------------------------------------------------


def collimated_lattice(lx, shape, dtype, active=True):
    """Drift, rectangular aperture (sample 0 lets nobody through), quadrupole, drift, screen A, elliptical aperture, drift,
    screen B.  `active`: apertures and screens in the beam; else all of them are identity elements."""
    d1, q, h, d2 = optics(lx, shape, dtype)
    B = int(np.prod(shape))
    x_max = (np.linspace(0.0, 1.2e-4, B)).reshape(shape).astype(dtype)  # (0.6 .. 1.2 sigma behind the first sample)
    first = lx.Aperture(x_max=x_max, y_max=np.asarray([1.5e-4], dtype=dtype), shape="rectangular", is_active=active, name="AP_RECT", dtype=dtype)
    second = lx.Aperture(x_max=np.asarray([1.3e-4], dtype=dtype), y_max=np.asarray([1.1e-4], dtype=dtype), shape="elliptical",
                         is_active=active, name="AP_ELL", dtype=dtype)
    a = make_screen(lx, SCREEN_A, mis_a(shape), dtype, "SCREEN_A", active)
    b = make_screen(lx, SCREEN_B, MIS_B, dtype, "SCREEN_B", active)
    return [d1, first, q, d2, a, second, h, b]


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_screen_behind_a_collimator_shows_the_collimated_beam(lx, dtype, shape, n):
    elements = collimated_lattice(lx, shape, dtype)
    P, beam = beam_of(lx, shape, n, dtype)
    trace = lx.Segment(elements).track_along(beam, losses="particles", screens=True)
    assert trace.screens == [4, 7] and trace.apertures == ["AP_RECT", "AP_ELL"]
    killer = np.array([1, 5, len(elements)])[trace.lost_at]  # the element that removed the particle (-1: beyond the end)
    opened = collimated_lattice(lx, shape, dtype, active=False)  # the same steps, nobody lost, nothing observed
    first_sample = (0,) * len(shape)
    for k, misalignment, geometry in ((4, mis_a(shape), SCREEN_A), (7, MIS_B, SCREEN_B)):
        entering = np.asarray(lx.Segment(opened[:k]).track_along(beam).outgoing.particles)
        alive = killer >= k  # aperture j clears its particles from point j + 1 on
        want = oracle_image(entering, misalignment, geometry, dtype, alive)
        image = trace.image_at(k)
        assert image.dtype == np.dtype(dtype) and np.array_equal(image, want), (k, int(np.abs(image - want).sum()))
        seen = image.sum(axis=(-2, -1))
        assert np.array_equal(seen, want.sum(axis=(-2, -1))) and np.all(seen <= trace.num_survivors[..., k])
        assert np.array_equal(alive.sum(axis=-1), trace.num_survivors[..., k])
        # nobody passes the first aperture of the first sample: an image of zeros, no exception
        assert trace.num_survivors[first_sample][k] == 0 and not image[first_sample].any()
    assert trace.image_at(4).sum(axis=(-2, -1)).reshape(-1)[-1] > 0  # (the widest sample does see particles)
    # losses=True (no `lost_at`) makes the same images
    counted = lx.Segment(elements).track_along(beam, losses=True, screens=True)
    assert counted.lost_at is None
    for got, want in zip(counted.screen_images, trace.screen_images):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# 4. against the oracle alone
# ---------------------------------------------------------------------------------------------


def oracle_case(shape, n, dtype):
    """The lattice of test 1 as the oracle's chain sees it (a screen is a marker), the particles entering both screens on
    the lattice-dtype and on the float64 chain."""
    f = lambda v: np.full(shape, v)  # noqa: E731
    k1 = np.linspace(-4.0, 5.0, int(np.prod(shape))).reshape(shape)
    desc = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=k1)), ("marker", {}),
            ("hcor", dict(length=f(0.1), angle=f(3e-5))), ("drift", dict(length=f(0.8))), ("marker", {})]
    P = o.gaussian_particles(shape, n, seed=SEEDS[n], dtype=dtype, sigma=SIGMA)
    energy = np.full(shape, 1e8, dtype=dtype)
    _, specs = make_lattice(desc, dtype)
    beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    beams64 = beams
    if np.dtype(dtype) == np.float32:  # the float32 lattice's own numbers in float64
        _, specs64 = make_lattice(upcast(desc), np.float64)
        beams64, _ = chain(specs64, o.particle_beam(P.astype(np.float64), energy.astype(np.float64), np.float64), np.float64)
    return desc, P, energy, beams, beams64


def on_an_edge(particles64, misalignment, geometry, dtype):
    """(*batch, N) bool: x - misalignment_x or y of the float64 chain within EDGE sigma of one of the screen's edges."""
    dtype = np.dtype(dtype).type
    mis = np.asarray(np.asarray(misalignment, dtype=dtype), dtype=np.float64)
    x = particles64[..., 0] - mis[..., None, 0]
    y = particles64[..., 2]
    out = np.zeros(x.shape, dtype=bool)
    for v, edges in zip((x, y), o.screen_bin_edges(**geometry, dtype=dtype)):
        delta = EDGE[dtype] * v.std(axis=-1, keepdims=True)
        nearest = np.abs(v[..., None] - edges.astype(np.float64)).min(axis=-1)
        out |= nearest <= delta
    return out


@pytest.mark.parametrize("n,shape", ORACLE_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_images_against_the_oracles_chain(lx, dtype, n, shape):
    desc, P, energy, beams, beams64 = oracle_case(shape, n, dtype)
    cases = [(2, "SCREEN_A", mis_a(shape), SCREEN_A), (5, "SCREEN_B", MIS_B, SCREEN_B)]
    # the condition on the inputs, from the oracle alone
    edge_counts = [on_an_edge(beams64[k]["particles"], mis, geometry, dtype).sum(axis=-1) for k, _, mis, geometry in cases]
    print(f"on an edge, per screen and sample: {[c.tolist() for c in edge_counts]} of n = {n}")
    for count in edge_counts:
        assert np.all(count == 0) if n <= 1000 else np.all(count <= 0.01 * n), edge_counts
    elements, _ = make_lattice(desc, dtype, lx)
    for k, name, mis, geometry in cases:
        elements[k] = make_screen(lx, geometry, mis, dtype, name)
    trace = lx.Segment(elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype), screens=True)
    for (k, name, mis, geometry), count in zip(cases, edge_counts):
        ref = oracle_image(beams[k]["particles"], mis, geometry, dtype)
        differ = np.abs(trace.image_at(name).astype(np.float64) - ref).sum(axis=(-2, -1))
        print(f"{name}: sum |image - ref| per sample {differ.tolist()}, on an edge {count.tolist()}")
        assert np.all(differ <= 2 * count), (name, differ, count)


# ---------------------------------------------------------------------------------------------
# 5. screens perturb nothing
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_screens_change_no_bit_of_the_trace_and_images_repeat(lx, dtype, n):
    shape = (3,)
    P, beam = beam_of(lx, shape, n, dtype)
    # without losses
    watched = lx.Segment(two_screen_lattice(lx, shape, dtype)[0]).track_along(beam, screens=True)
    idle = lx.Segment(two_screen_lattice(lx, shape, dtype, is_active=False)[0]).track_along(beam)
    assert np.array_equal(watched.records, idle.records) and np.array_equal(watched.energy, idle.energy)
    assert np.array_equal(np.asarray(watched.outgoing.particles), np.asarray(idle.outgoing.particles))
    assert idle.screens == [] and watched.lost_at is None
    # with losses
    elements = collimated_lattice(lx, shape, dtype)
    unwatched = collimated_lattice(lx, shape, dtype)
    for el in unwatched:
        if isinstance(el, lx.Screen):
            el.is_active = False
    segment = lx.Segment(elements)
    clipped = segment.track_along(beam, losses="particles", screens=True)
    plain = lx.Segment(unwatched).track_along(beam, losses="particles")
    assert np.array_equal(clipped.records, plain.records, equal_nan=True) and np.array_equal(clipped.energy, plain.energy)
    assert np.array_equal(clipped.lost_at, plain.lost_at) and np.array_equal(clipped.num_survivors, plain.num_survivors)
    assert clipped.outgoing is None and plain.outgoing is None and (plain.lost_at >= 0).any()
    # ... and with apertures that lose nobody the particles come out, the same bits
    for lattice in (elements, unwatched):
        for el in lattice:
            if isinstance(el, lx.Aperture):
                el.x_max, el.y_max = np.array([np.inf], dtype=dtype), np.array([np.inf], dtype=dtype)
    wide, wide_plain = segment.track_along(beam, losses="particles", screens=True), lx.Segment(unwatched).track_along(beam, losses="particles")
    assert np.array_equal(wide.records, wide_plain.records) and np.all(wide.lost_at == -1) and np.all(wide_plain.lost_at == -1)
    assert np.array_equal(np.asarray(wide.outgoing.particles), np.asarray(wide_plain.outgoing.particles))
    # a second identical call: identical images (integer adds, no order)
    again = segment.track_along(beam, losses="particles", screens=True)
    for first, second in zip(wide.screen_images, again.screen_images):
        assert np.array_equal(first, second) and first.sum() > 0
    # a misalignment written between two traces is seen
    elements[4].misalignment = np.asarray(mis_a(shape) + 1e-4, dtype=dtype)
    moved = segment.track_along(beam, losses="particles", screens=True)
    assert not np.array_equal(moved.image_at("SCREEN_A"), again.image_at("SCREEN_A"))
    assert np.array_equal(moved.image_at("SCREEN_B"), again.image_at("SCREEN_B"))


# ---------------------------------------------------------------------------------------------
# 6. ParameterBeam
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameter_beam_images_at_two_screens(lx, dtype, shape):
    full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-5), mu_y=full(-1e-5), sigma_x=full(1e-4), sigma_xp=full(1e-5),
                                            sigma_y=full(1e-4), sigma_yp=full(1e-5), sigma_s=full(1e-5), sigma_p=full(1e-3),
                                            energy=full(1e8), dtype=dtype)
    elements, a, b = two_screen_lattice(lx, shape, dtype)
    trace = lx.Segment(elements).track_along(beam, screens=True)
    assert trace.screens == [2, 5]
    tol = 2e-4 if dtype == np.float32 else 1e-10  # (of test_parameter_beam_gaussian_image)
    for k, mis, geometry in ((2, mis_a(shape), SCREEN_A), (5, MIS_B, SCREEN_B)):
        mu = np.array(trace._mu[..., k, :], dtype=dtype)
        mis = np.asarray(mis, dtype=dtype)
        mu[..., 0] = mu[..., 0] - mis[..., 0]
        mu[..., 2] = mu[..., 2] - mis[..., 1]
        ref = o.screen_reading_parameters(mu, trace._cov[..., k, :, :], **geometry, dtype=dtype)
        image = trace.image_at(k)
        assert image.shape == ref.shape and image.dtype == np.dtype(dtype) and image.shape[:-2] == shape
        assert np.max(np.abs(image - ref)) <= tol * ref.max() and ref.max() > 0
    assert a.reading is trace.image_at("SCREEN_A") and b.reading is trace.image_at("SCREEN_B")
    # active apertures, with losses=True, change nothing
    collimated = lx.Segment(collimated_lattice(lx, shape, dtype)).track_along(beam, losses=True, screens=True)
    opened = collimated_lattice(lx, shape, dtype)
    for el in opened:
        if isinstance(el, lx.Aperture):
            el.is_active = False
    free = lx.Segment(opened).track_along(beam, screens=True)
    assert collimated.screens == free.screens == [4, 7] and collimated.num_survivors is None
    for got, want in zip(collimated.screen_images, free.screen_images):
        assert np.array_equal(got, want) and got.max() > 0
    assert np.array_equal(collimated._mu, free._mu) and np.array_equal(collimated._cov, free._cov)


# ---------------------------------------------------------------------------------------------
# 7. the elements
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_screens_read_their_images_from_the_trace(lx, dtype):
    shape = (3,)
    elements, a, b = two_screen_lattice(lx, shape, dtype)
    idle = make_screen(lx, SCREEN_B, MIS_B, dtype, "IDLE", is_active=False)
    segment = lx.Segment([elements[0], lx.Segment(elements[1:4]), idle, *elements[4:]])  # (a nested segment is opened up)
    P, beam = beam_of(lx, shape, 1000, dtype)
    with pytest.raises(NotImplementedError, match="SCREEN_A"):
        segment.track_along(beam)
    with pytest.raises(NotImplementedError, match="SCREEN_A"):
        segment.track_along(beam, losses=True)
    trace = segment.track_along(beam, screens=True)
    assert trace.screens == [2, 6] and trace.names[2] == "SCREEN_A" and trace.names[6] == "SCREEN_B"
    assert a.reading is trace.image_at("SCREEN_A") and b.reading is trace.image_at("SCREEN_B")
    assert a.reading is trace.screen_images[0] and a.get_read_beam() is None and b.get_read_beam() is None
    with pytest.raises(KeyError):
        trace.image_at("IDLE")
    assert idle.reading.shape == SHAPE_B and not idle.reading.any()  # an inactive screen keeps its zeros
    # `resolution=` passes the keyword on to the split lattice
    fine = segment.track_along(beam, resolution=0.25, screens=True)
    assert len(fine.screens) == 2 and fine.num_points > trace.num_points
    assert np.array_equal(fine.image_at("SCREEN_B").sum(axis=(-2, -1)) > 0, np.ones(shape, dtype=bool))
    # no active screen: no images, and otherwise the plain result
    a.is_active = b.is_active = False
    nothing, plain = segment.track_along(beam, screens=True), segment.track_along(beam)
    assert nothing.screens == [] and nothing.screen_images == []
    assert np.array_equal(nothing.records, plain.records)
    assert np.array_equal(np.asarray(nothing.outgoing.particles), np.asarray(plain.outgoing.particles))
    # `Segment.track` keeps the reference's semantics: an active screen swallows the beam
    a.is_active = True
    assert segment.track(beam) is lx.Beam.empty


# ---------------------------------------------------------------------------------------------
# 8. the modes alternating on one context
# ---------------------------------------------------------------------------------------------


def expected_losses(lx, elements, beam, dtype):
    """
    `lost_at` of a lattice's active apertures and the particles on an edge, both (*batch, N), from `criterion` of
    tests/test_gpu_trace_losses.py on the particles that enter each aperture: the outgoing particles of the plain trace of
    what stands in front of it, apertures and screens switched off (the product's own numbers, as in test 3 above).
    """
    steps = [k for k, el in enumerate(elements) if isinstance(el, lx.Aperture) and el.is_active]
    limits = [(np.asarray(elements[k].x_max, dtype=dtype), np.asarray(elements[k].y_max, dtype=dtype), elements[k].shape) for k in steps]
    switchable = [el for el in elements if isinstance(el, (lx.Aperture, lx.Screen))]
    active = [el.is_active for el in switchable]
    for el in switchable:
        el.is_active = False
    entering = [np.asarray(lx.Segment(elements[:k]).track_along(beam).outgoing.particles) for k in steps]
    for el, was in zip(switchable, active):
        el.is_active = was
    alive = np.ones(entering[0].shape[:-1], dtype=bool)
    lost_at = np.full(alive.shape, -1, dtype=np.int32)
    on_edge = np.zeros(alive.shape, dtype=bool)
    for ordinal, (P, (x_max, y_max, shape)) in enumerate(zip(entering, limits)):
        crit = criterion(P.astype(np.float64), x_max, y_max, shape)
        with np.errstate(all="ignore"):
            keep = np.all(crit <= 1.0, axis=0)
            on_edge |= alive & np.any(np.abs(crit - 1.0) <= LOSSES_EDGE[np.dtype(dtype).type], axis=0)
        lost_at[alive & ~keep] = ordinal
        alive &= keep
    return steps, lost_at, on_edge


def assert_survivors(lx, trace, elements, beam, dtype):
    """The trace's `lost_at` and its counts at every point against `expected_losses`."""
    steps, lost_at, on_edge = expected_losses(lx, elements, beam, dtype)
    differ = (trace.lost_at != lost_at) & ~on_edge
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:5])
    where = np.array(steps + [len(elements)])  # the element that removed the particle (-1: beyond the end)
    # the trace's own survivor set: exactly; the criterion's: but for the particles on an edge
    for killer, slack in ((where[trace.lost_at], 0), (where[lost_at], on_edge.sum(axis=-1))):
        for k in range(len(elements) + 1):
            count = (killer >= k).sum(axis=-1)  # aperture j clears its particles from point j + 1 on
            assert np.all(np.abs(trace.num_survivors[..., k] - count) <= slack), (k, trace.num_survivors[..., k], count, slack)


def same_trace(got, want):
    assert np.array_equal(got.records, want.records, equal_nan=True) and np.array_equal(got.energy, want.energy)
    assert (got.lost_at is None) == (want.lost_at is None) and (got.outgoing is None) == (want.outgoing is None)
    if want.lost_at is not None:
        assert np.array_equal(got.lost_at, want.lost_at) and np.array_equal(got.num_survivors, want.num_survivors)
    if want.outgoing is not None:
        assert np.array_equal(np.asarray(got.outgoing.particles), np.asarray(want.outgoing.particles))
    assert got.screens == want.screens and len(got.screen_images) == len(want.screen_images)
    for a, b in zip(got.screen_images, want.screen_images):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_modes_alternate_on_one_context(lx, dtype):
    """
    losses, losses + screens, screens, plain, losses again, losses on a second lattice of the same length, then every mode
    once more, on ONE context: the step plan of a call is uploaded when it differs from the one on the device, and every
    mode reads the same buffer.  n = 257: a full float32 tile and a masked one; two full float64 tiles and a masked one.
    """
    shape, n = (2,), 257
    P, beam = beam_of(lx, shape, n, dtype)
    elements = collimated_lattice(lx, shape, dtype)
    segment = lx.Segment(elements)

    def switch(elements, apertures, screens):
        for el in elements:
            if isinstance(el, lx.Aperture):
                el.is_active = apertures
            if isinstance(el, lx.Screen):
                el.is_active = screens

    def run(mode):
        switch(elements, "losses" in mode, "screens" in mode)
        return segment.track_along(beam, losses="particles" if "losses" in mode else False, screens="screens" in mode)

    modes = [("losses",), ("losses", "screens"), ("screens",), ()]
    first = {mode: run(mode) for mode in modes}
    same_trace(run(("losses",)), first["losses",])
    # a second lattice with as many elements and the collimators elsewhere (steps 2 and 6, not 1 and 5), its screens idle
    d1, rect, q, d2, a, ell, h, b = collimated_lattice(lx, shape, dtype)
    moved = [d1, q, rect, a, d2, h, ell, b]
    switch(moved, True, False)
    other = lx.Segment(moved).track_along(beam, losses="particles")
    assert other.apertures == ["AP_RECT", "AP_ELL"] and other.num_points == first["losses",].num_points
    # every mode once more: the bits of its first call
    for mode in modes[1:] + modes[:1]:
        same_trace(run(mode), first[mode])
    # what the modes owe each other
    assert np.array_equal(first["losses", "screens"].records, first["losses",].records, equal_nan=True)
    assert np.array_equal(first["losses", "screens"].lost_at, first["losses",].lost_at)
    assert np.array_equal(first["screens",].records, first[()].records) and np.all(first[()].records[..., 35] == n)
    assert first["screens",].image_at("SCREEN_B").sum() > first["losses", "screens"].image_at("SCREEN_B").sum() > 0
    # the survivors of both lattices are their own: nobody is lost in front of point 3 of the second lattice, and both
    # agree with the criterion on the particles entering their own apertures
    assert np.all(first["losses",].num_survivors[..., 2] < n) and np.all(other.num_survivors[..., :3] == n)
    assert np.all(other.num_survivors[..., 3] < n)
    switch(elements, True, False)
    assert_survivors(lx, first["losses",], elements, beam, dtype)
    assert_survivors(lx, other, moved, beam, dtype)
