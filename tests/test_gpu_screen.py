"""
Screen read-out on the GPU (lynx_histogram2d, lynx_gaussian_image) against the oracle
(numpy.histogramdd / bivariate normal density), and the swallow-the-beam semantics of an
active screen inside a Segment (reference tests/test_screen.py, screen.py:126-216).
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()
    return lynx_amd


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_particle_beam_histogram_is_exact(lx, dtype):
    res, px, binning = (200, 120), (3.5e-6, 2.5e-6), 2
    P = o.gaussian_particles((3,), 50_000, seed=1, dtype=dtype, mu=[5e-5, 0, -3e-5, 0, 0, 0],
                             sigma=[1.2e-4, 1e-5, 0.9e-4, 1e-5, 1e-5, 1e-3])
    edges = o.screen_bin_edges(res, px, binning, dtype)
    P[0, :50, 0] = edges[0][np.arange(50) % len(edges[0])]   # values exactly on bin edges (the first 50 of each axis)
    P[0, :50, 2] = edges[1][np.arange(50) % len(edges[1])]
    screen = lx.Screen(resolution=res, pixel_size=px, binning=binning, is_active=True, dtype=dtype,
                       misalignment=np.zeros((3, 2)))
    out = screen.track(lx.ParticleBeam(P, np.full(3, 1e8), dtype=dtype))
    assert out is lx.Beam.empty
    image = screen.reading
    ref = o.screen_reading_particles(P, res, px, binning, dtype)
    assert image.shape == (3, 60, 100) == ref.shape
    assert np.array_equal(image, ref)  # integer counts, bit-exact bin assignment
    assert 0 < image.sum() <= 3 * 50_000
    assert screen.reading is image  # cached (screen.py:145-146)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameter_beam_gaussian_image(lx, dtype):
    res, px, binning = (160, 96), (2e-5, 2e-5), 4
    beam = lx.ParameterBeam.from_parameters(mu_x=np.array([1e-4, -2e-4]), mu_y=np.array([5e-5, 0.0]),
                                            sigma_x=np.array([2e-4, 3e-4]), sigma_y=np.array([1e-4, 2e-4]),
                                            dtype=dtype)
    screen = lx.Screen(resolution=res, pixel_size=px, binning=binning, is_active=True, dtype=dtype,
                       misalignment=np.zeros((2, 2)))
    assert screen.track(beam) is lx.Beam.empty
    image = screen.reading
    ref = o.screen_reading_parameters(beam._mu, beam._cov, res, px, binning, dtype)
    assert image.shape == ref.shape == (2, 40, 24)
    assert np.max(np.abs(image - ref)) <= (2e-4 if dtype == np.float32 else 1e-10) * ref.max()


def test_active_screen_inside_a_segment(lx):
    """reference tests/test_screen.py / tests/test_speed.py: ARES-style use."""
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    screen = lx.Screen(resolution=(64, 64), pixel_size=(2e-5, 2e-5), is_active=True, name="SCR")
    bpm = lx.BPM(name="B", is_active=True)
    seg = lx.Segment([lx.Drift(f(1.0)), lx.Quadrupole(f(0.2), k1=f(2.0)), screen, lx.Drift(f(1.0)), bpm])
    beam = lx.ParticleBeam.from_parameters(num_particles=20_000, sigma_x=f(1e-4), sigma_y=f(1e-4), seed=3)
    assert seg.track(beam) is lx.Beam.empty and bpm.reading is None  # the BPM behind the screen sees no beam
    assert screen.reading.shape == (1, 64, 64) and screen.reading.sum() > 10_000
    screen.is_active = False
    out = seg.track(beam)
    assert out is not lx.Beam.empty and bpm.reading.shape == (2, 1)
    empty = lx.Screen(resolution=(8, 6), is_active=True)
    assert np.array_equal(empty.reading, np.zeros((6, 8)))


# ---------------------------------------------------------------------------------------------
# The stand-alone read-out (lynx_histogram2d, lynx_gaussian_image) at its edges
# ---------------------------------------------------------------------------------------------

SMALL = dict(resolution=(40, 24), pixel_size=(5e-6, 7e-6), binning=2)  # 20 x 12 bins of 10 x 14 um: +-100 um by +-84 um
TOL_IMAGE = {np.float32: 2e-4, np.float64: 1e-10}  # of the peak (test_parameter_beam_gaussian_image)


def read(lx, geometry, beam, dtype, misalignment=None):
    """`Screen.reading` of a fresh active screen the beam was tracked into."""
    screen = lx.Screen(**geometry, misalignment=misalignment, is_active=True, dtype=dtype)
    assert screen.track(beam) is lx.Beam.empty
    return screen.reading


def particle_beam(lx, P, dtype):
    return lx.ParticleBeam(P, np.full(P.shape[:-2], 1e8, dtype=dtype), dtype=dtype)


def gaussian_beam(lx, batch, dtype, rho, mu_x=None, seed=0):
    """ParameterBeam from an explicit mu and cov: sigma_x != sigma_y, both distinct per sample, cov[x, y] = rho sigma_x sigma_y."""
    B = int(np.prod(batch))
    rng = np.random.default_rng(seed)
    sx, sy = np.linspace(2e-4, 4e-4, B).reshape(batch), np.linspace(1.5e-4, 0.9e-4, B).reshape(batch)
    mu = np.zeros((*batch, 7))
    mu[..., 0], mu[..., 2], mu[..., 6] = rng.normal(0, 1e-4, batch) if mu_x is None else mu_x, rng.normal(0, 5e-5, batch), 1.0
    cov = np.zeros((*batch, 7, 7))
    for c, s in enumerate([sx, 1e-5, sy, 1e-5, 1e-5, 1e-3]):
        cov[..., c, c] = np.asarray(s) ** 2
    cov[..., 0, 2] = cov[..., 2, 0] = np.asarray(rho).reshape(batch) * sx * sy
    return lx.ParameterBeam(mu, cov, np.full(batch, 1e8), dtype=dtype)


def assert_gaussian_image(image, ref, dtype):
    """Every sample within the file's tolerance of ITS OWN peak."""
    assert image.shape == ref.shape and image.dtype == np.dtype(dtype)
    peak = ref.max(axis=(-2, -1), keepdims=True)
    assert np.all(peak > 0) and np.all(np.abs(image - ref) <= TOL_IMAGE[dtype] * peak), float(np.max(np.abs(image - ref) / peak))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [(1,), (3,), (2, 2)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1025, 4097])
def test_histogram_at_every_workgroup_and_chunk_boundary(lx, dtype, batch, n):
    P = o.gaussian_particles(batch, n, seed=n, dtype=dtype, mu=[2e-5, 0, -1e-5, 0, 0, 0], sigma=[6e-5, 1e-5, 5e-5, 1e-5, 1e-5, 1e-3])
    image = read(lx, SMALL, particle_beam(lx, P, dtype), dtype)
    ref = o.screen_reading_particles(P, **SMALL, dtype=dtype)
    assert image.shape == (*batch, 12, 20) == ref.shape and image.dtype == np.dtype(dtype)
    assert np.array_equal(image, ref), int(np.abs(image - ref).sum())
    assert n == 1 or np.all(image.sum(axis=(-2, -1)) > 0.5 * n)
    assert n < 1000 or np.all(image.sum(axis=(-2, -1)) < n)  # (the screen cuts the beam)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_histogram_of_a_batch_with_one_chunk_per_sample(lx, dtype):
    """2100 samples are more than 8 x 256 compute units: every sample is one workgroup's, whatever its particle count."""
    geometry = dict(resolution=(16, 12), pixel_size=(2e-5, 2e-5), binning=1)
    P = o.gaussian_particles((2100,), 300, seed=6, dtype=dtype, sigma=[8e-5, 1e-5, 7e-5, 1e-5, 1e-5, 1e-3])
    P[..., 0] += np.linspace(-1e-4, 1e-4, 2100, dtype=dtype)[:, None]  # (no two samples alike)
    image = read(lx, geometry, particle_beam(lx, P, dtype), dtype)
    ref = o.screen_reading_particles(P, **geometry, dtype=dtype)
    assert image.shape == (2100, 12, 16) and np.array_equal(image, ref)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_particles_outside_the_screen_and_non_finite_ones_are_not_counted(lx, dtype):
    ex, ey = o.screen_bin_edges(**SMALL, dtype=dtype)
    up, down = dtype(np.inf), dtype(-np.inf)
    specials = [ex[0], ex[-1], np.nextafter(ex[0], down), np.nextafter(ex[-1], up), np.nextafter(ex[0], up), np.nextafter(ex[-1], down),
                dtype(-1.0), dtype(1.0), dtype(1e30), dtype(np.nan), up, down, ex[7], dtype(0)]
    specials_y = [ey[0], ey[-1], np.nextafter(ey[0], down), np.nextafter(ey[-1], up), np.nextafter(ey[0], up), np.nextafter(ey[-1], down),
                  dtype(-1.0), dtype(1.0), dtype(1e30), dtype(np.nan), up, down, ey[5], dtype(0)]
    P = o.gaussian_particles((2,), 600, seed=2, dtype=dtype, sigma=[6e-5, 1e-5, 5e-5, 1e-5, 1e-5, 1e-3])
    k = len(specials)
    P[0, :k, 0], P[0, k:2 * k, 2] = specials, specials_y           # in x alone, in y alone,
    P[1, :k, 0], P[1, :k, 2] = specials, specials_y[::-1]          # and both at once
    P[1, k:2 * k, 0], P[1, k:2 * k, 2] = specials, specials_y      # (a corner of the screen: on the first and last edge of both)
    image = read(lx, SMALL, particle_beam(lx, P, dtype), dtype)
    with np.errstate(all="ignore"):
        ref = o.screen_reading_particles(P, **SMALL, dtype=dtype)
        x, y = P[..., 0], P[..., 2]
        inside = (x >= ex[0]) & (x <= ex[-1]) & (y >= ey[0]) & (y <= ey[-1])
    assert np.array_equal(image, ref), int(np.abs(image - ref).sum())
    assert np.array_equal(image.sum(axis=(-2, -1)), inside.sum(axis=-1)) and np.all(inside.sum(axis=-1) < 600 - 8)
    # the corners: (first x edge, first y edge) is the bottom left pixel, (last, last) the top right one
    only = np.ones((1, 2, 7), dtype=dtype)
    only[0, :, 0], only[0, :, 2] = [ex[0], ex[-1]], [ey[0], ey[-1]]
    corners = read(lx, SMALL, particle_beam(lx, only, dtype), dtype)[0]
    assert corners[-1, 0] == 1 and corners[0, -1] == 1 and corners.sum() == 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_resolution_the_binning_does_not_divide(lx, dtype):
    """(10, 7) at binning 2: 5 x 3 bins for the histogram (int(3.5) = 3), 5 x 4 pixels from `arange` for the density -- as in
    the reference (screen.py:107-120 and 160-170)."""
    geometry = dict(resolution=(10, 7), pixel_size=(2e-5, 3e-5), binning=2)
    P = o.gaussian_particles((3,), 1000, seed=5, dtype=dtype, sigma=[6e-5, 1e-5, 6e-5, 1e-5, 1e-5, 1e-3])
    image = read(lx, geometry, particle_beam(lx, P, dtype), dtype)
    assert image.shape == (3, 3, 5) and np.array_equal(image, o.screen_reading_particles(P, **geometry, dtype=dtype))
    assert np.all(image.sum(axis=(-2, -1)) > 500)
    beam = gaussian_beam(lx, (3,), dtype, rho=[0.5, -0.5, 0.0])
    image = read(lx, geometry, beam, dtype)
    assert image.shape == (3, 5, 4)
    assert_gaussian_image(image, o.screen_reading_parameters(beam._mu, beam._cov, **geometry, dtype=dtype), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_screen_of_one_pixel(lx, dtype):
    geometry = dict(resolution=(1, 1), pixel_size=(1e-4, 8e-5), binning=1)
    P = o.gaussian_particles((3,), 500, seed=8, dtype=dtype, sigma=[6e-5, 1e-5, 6e-5, 1e-5, 1e-5, 1e-3])
    image = read(lx, geometry, particle_beam(lx, P, dtype), dtype)
    inside = (np.abs(P[..., 0]) <= dtype(5e-5)) & (np.abs(P[..., 2]) <= dtype(4e-5))
    assert image.shape == (3, 1, 1) and np.array_equal(image, o.screen_reading_particles(P, **geometry, dtype=dtype))
    assert np.array_equal(image[:, 0, 0], inside.sum(axis=-1)) and np.all(image > 0) and np.all(image < 500)
    beam = gaussian_beam(lx, (3,), dtype, rho=[0.5, -0.5, 0.0])
    image = read(lx, geometry, beam, dtype)
    assert image.shape == (3, 1, 1)
    assert_gaussian_image(image, o.screen_reading_parameters(beam._mu, beam._cov, **geometry, dtype=dtype), dtype)


def test_the_ares_camera_and_a_screen_too_large_for_the_edge_table(lx):
    """(2448 + 2040 + 2) float64 edges are 35.9 KB of the 64 KB table; (5000 + 4000 + 2) are 72 KB: refused before any launch."""
    dtype = np.float64
    ares = dict(resolution=(2448, 2040), pixel_size=(3.3198e-6, 2.4469e-6), binning=1)
    P = o.gaussian_particles((1,), 5000, seed=12, dtype=dtype, sigma=[2e-3, 1e-5, 1.5e-3, 1e-5, 1e-5, 1e-3])
    beam = particle_beam(lx, P, dtype)
    ref = o.screen_reading_particles(P, **ares, dtype=dtype)
    image = read(lx, ares, beam, dtype)
    assert image.shape == (1, 2040, 2448) and np.array_equal(image, ref) and 0.5 * 5000 < image.sum() < 5000
    huge = lx.Screen(resolution=(5000, 4000), pixel_size=(1e-6, 1e-6), binning=1, is_active=True, dtype=dtype)
    assert huge.track(beam) is lx.Beam.empty
    with pytest.raises(RuntimeError, match="too large for the edge table"):
        huge.reading
    assert np.array_equal(read(lx, ares, beam, dtype), ref)  # the context goes on working


# ---------------------------------------------------------------------------------------------
# Misalignment on the stand-alone path (`Screen._observe`)
# ---------------------------------------------------------------------------------------------


def misalignments(batch):
    """(*batch, 2): a misalignment per sample, both components at least 15 um (1.5 bins of SMALL) and no two alike."""
    B = int(np.prod(batch))
    return np.stack([[-3e-5, 2e-5, 4e-5, -1.5e-5][:B], [5e-5, -2e-5, 3e-5, -4e-5][:B]], axis=-1).reshape(*batch, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [(3,), (2, 2)])
def test_misalignment_of_a_particle_beam(lx, dtype, batch):
    """The reference takes the x misalignment off x and the y misalignment off x' (screen.py:134-135): kept as it is."""
    P = o.gaussian_particles(batch, 3000, seed=21, dtype=dtype, mu=[2e-5, 0, -1e-5, 0, 0, 0], sigma=[6e-5, 1e-5, 5e-5, 1e-5, 1e-5, 1e-3])
    mis = misalignments(batch).astype(dtype)
    beam = particle_beam(lx, P.copy(), dtype)
    image = read(lx, SMALL, beam, dtype, misalignment=mis)
    moved = P.copy()
    moved[..., 0] -= mis[..., None, 0]
    moved[..., 1] -= mis[..., None, 1]
    ref = o.screen_reading_particles(moved, **SMALL, dtype=dtype)
    assert np.array_equal(image, ref), int(np.abs(image - ref).sum())
    assert np.array_equal(np.asarray(beam.particles), P)  # the incoming beam is untouched
    # what the test can tell apart: no shift at all, the shift of another sample, and y shifted as well
    in_y = moved.copy()
    in_y[..., 2] -= mis[..., None, 1]
    rolled = P.copy()
    rolled[..., 0] -= np.roll(mis.reshape(-1, 2), 1, axis=0).reshape(mis.shape)[..., None, 0]
    for other in (P, in_y, rolled):
        differs = np.abs(o.screen_reading_particles(other, **SMALL, dtype=dtype) - ref).sum(axis=(-2, -1))
        assert np.all(differs > 0), differs
    # one misalignment for all samples
    shared = np.array([2.5e-5, -4e-5], dtype=dtype)
    moved = P.copy()
    moved[..., 0] -= shared[0]
    moved[..., 1] -= shared[1]
    assert np.array_equal(read(lx, SMALL, beam, dtype, misalignment=shared), o.screen_reading_particles(moved, **SMALL, dtype=dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [(3,), (2, 2)])
def test_misalignment_of_a_parameter_beam(lx, dtype, batch):
    B = int(np.prod(batch))
    beam = gaussian_beam(lx, batch, dtype, rho=np.linspace(-0.6, 0.6, B))
    mu_before = beam._mu.copy()
    mis = misalignments(batch).astype(dtype)
    geometry = dict(resolution=(160, 96), pixel_size=(2e-5, 2e-5), binning=4)
    image = read(lx, geometry, beam, dtype, misalignment=mis)
    mu = mu_before.copy()
    mu[..., 0] -= mis[..., 0]
    mu[..., 2] -= mis[..., 1]
    assert_gaussian_image(image, o.screen_reading_parameters(mu, beam._cov, **geometry, dtype=dtype), dtype)
    assert np.array_equal(beam._mu, mu_before)  # the incoming beam is untouched
    for other in (mu_before, mu - np.array([0, 0, 1, 0, 0, 0, 0], dtype) * mis[..., 1:2], mu + np.array([0, 0, 2, 0, 0, 0, 0], dtype) * mis[..., 1:2]):
        away = o.screen_reading_parameters(other, beam._cov, **geometry, dtype=dtype)  # no shift; y shifted twice; y the other way
        peak = away.max(axis=(-2, -1), keepdims=True)
        assert np.all(np.max(np.abs(image - away) / peak, axis=(-2, -1)) > 100 * TOL_IMAGE[dtype])


# ---------------------------------------------------------------------------------------------
# The Gaussian image of a correlated beam
# ---------------------------------------------------------------------------------------------

RHO = {(3,): [0.9, -0.9, 0.99], (2, 2): [0.9, -0.9, 0.99, -0.99]}
FINE = dict(resolution=(160, 96), pixel_size=(2e-5, 2e-5), binning=2)  # 80 x 48 pixels of 40 um: +-1.6 mm by +-0.96 mm


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [(3,), (2, 2)])
def test_gaussian_image_of_a_correlated_beam(lx, dtype, batch):
    beam = gaussian_beam(lx, batch, dtype, rho=RHO[batch])
    image = read(lx, FINE, beam, dtype)
    ref = o.screen_reading_parameters(beam._mu, beam._cov, **FINE, dtype=dtype)
    assert image.shape == (*batch, 80, 48)
    assert_gaussian_image(image, ref, dtype)
    # a kernel that ignored cov[x, y] (in det or in the quadratic form) is far away
    plain = np.array(beam._cov)
    plain[..., 0, 2] = plain[..., 2, 0] = 0
    uncorrelated = o.screen_reading_parameters(beam._mu, plain, **FINE, dtype=dtype)
    peak = ref.max(axis=(-2, -1))
    assert np.all(np.abs(ref - uncorrelated).max(axis=(-2, -1)) > 100 * TOL_IMAGE[dtype] * peak)
    assert np.all(np.abs(image - uncorrelated).max(axis=(-2, -1)) > 100 * TOL_IMAGE[dtype] * peak)
    # ... and one with the wrong sign of the cross term gives the mirror image
    mirrored = np.array(beam._cov)
    mirrored[..., 0, 2] = mirrored[..., 2, 0] = -mirrored[..., 0, 2]
    wrong = o.screen_reading_parameters(beam._mu, mirrored, **FINE, dtype=dtype)
    assert np.all(np.abs(image - wrong).max(axis=(-2, -1)) > 100 * TOL_IMAGE[dtype] * peak)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gaussian_image_of_a_beam_far_off_the_screen(lx, dtype):
    """The mean 50 sigma_x beyond the right edge: exp(-1250) and less, a finite number (zero) in every pixel."""
    batch = (3,)
    sx = np.linspace(2e-4, 4e-4, 3)
    inside = gaussian_beam(lx, batch, dtype, rho=RHO[batch], mu_x=np.zeros(3))
    beam = gaussian_beam(lx, batch, dtype, rho=RHO[batch], mu_x=1.6e-3 + 50 * sx)
    peak = read(lx, FINE, inside, dtype).max(axis=(-2, -1))
    image = read(lx, FINE, beam, dtype)
    assert image.shape == (3, 80, 48) and np.all(np.isfinite(image)) and np.all(image >= 0)
    assert np.all(peak > 0) and np.all(image.max(axis=(-2, -1)) < TOL_IMAGE[dtype] * peak)


# ---------------------------------------------------------------------------------------------
# Behind coupling optics, and the two kernels that make one image
# ---------------------------------------------------------------------------------------------

COUPLED_SEED = 8  # no particle of the oracle's float64 chain within the edge margin of a bin edge (searched on the host)
COUPLED_SCREEN = dict(resolution=(6, 4), pixel_size=(1.7e-5, 7.5e-5), binning=1)  # pixels of one sigma: +-3 by +-2 sigma
COUPLED_GRID = dict(resolution=(40, 24), pixel_size=(5e-6, 2e-5), binning=2)  # 20 x 12 pixels of 0.4 sigma
COUPLED_SIGMA = [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]


def coupled_optics():
    f = lambda v: np.array([v])  # noqa: E731
    return [("drift", dict(length=f(0.5))), ("quadrupole", dict(length=f(0.2), k1=f(3.0), tilt=f(0.4))),
            ("solenoid", dict(length=f(0.3), k=f(2.0))), ("drift", dict(length=f(0.4)))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_particle_beam_image_behind_coupling_optics(lx, dtype):
    from .test_gpu_trace import upcast
    from .test_gpu_trace_screens import on_an_edge

    desc = coupled_optics()
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles((1,), 5000, seed=COUPLED_SEED, dtype=dtype, sigma=COUPLED_SIGMA)
    energy = np.array([1e8], dtype=dtype)
    arriving = o.segment_track(specs, o.particle_beam(P, energy, dtype), dtype)["particles"]
    arriving64 = arriving
    if dtype == np.float32:  # the float32 lattice's own numbers in float64 say who is on an edge
        _, specs64 = make_lattice(upcast(desc), np.float64)
        arriving64 = o.segment_track(specs64, o.particle_beam(P.astype(np.float64), energy.astype(np.float64), np.float64), np.float64)["particles"]
    assert on_an_edge(arriving64, np.zeros(2), COUPLED_SCREEN, dtype).sum() == 0  # the condition on the input
    rho = np.corrcoef(arriving64[0, :, 0], arriving64[0, :, 2])[0, 1]
    assert abs(rho) > 0.1  # (the optics do couple x and y)
    screen = lx.Screen(**COUPLED_SCREEN, is_active=True, dtype=dtype, name="SCR")
    assert lx.Segment([*elements, screen]).track(lx.ParticleBeam(P, energy, dtype=dtype)) is lx.Beam.empty
    ref = o.screen_reading_particles(arriving, **COUPLED_SCREEN, dtype=dtype)
    assert np.array_equal(screen.reading, ref), int(np.abs(screen.reading - ref).sum())
    assert 0.9 * 5000 < ref.sum() < 5000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameter_beam_image_behind_coupling_optics(lx, dtype):
    elements, specs = make_lattice(coupled_optics(), dtype, lx)
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    kw = dict(mu_x=f(3e-5), mu_y=f(-2e-5), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1.5e-4), sigma_yp=f(2e-5), sigma_s=f(1e-5),
              sigma_p=f(1e-3), energy=f(1e8))
    screen = lx.Screen(**COUPLED_GRID, is_active=True, dtype=dtype, name="SCR")
    assert lx.Segment([*elements, screen]).track(lx.ParameterBeam.from_parameters(**kw, dtype=dtype)) is lx.Beam.empty
    arriving = o.segment_track(specs, o.parameter_beam_from_parameters(dtype=dtype, **kw), dtype)
    cov = np.asarray(arriving["cov"], dtype=np.float64)
    assert abs(cov[0, 0, 2] / np.sqrt(cov[0, 0, 0] * cov[0, 2, 2])) > 0.1
    assert_gaussian_image(screen.reading, o.screen_reading_parameters(arriving["mu"], arriving["cov"], **COUPLED_GRID, dtype=dtype), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_image_from_two_kernels(lx, dtype):
    """`Screen.reading` behind `Segment.track` (lynx_histogram2d, lynx_gaussian_image) and the image made inside
    `track_along(screens=True)`: bit for bit for particles, within the Gaussian tolerance for a ParameterBeam."""
    batch = (3,)
    f = lambda v: np.full(batch, v, dtype=dtype)  # noqa: E731
    k1 = np.array([4.0, -3.0, 0.5], dtype=dtype)

    def lattice():
        screen = lx.Screen(**SMALL, is_active=True, dtype=dtype, name="SCR")
        return lx.Segment([lx.Drift(f(0.5), dtype=dtype), lx.Quadrupole(f(0.2), k1=k1, dtype=dtype), lx.Drift(f(0.3), dtype=dtype), screen]), screen

    P = o.gaussian_particles(batch, 4097, seed=31, dtype=dtype, sigma=[6e-5, 1e-5, 5e-5, 1e-5, 1e-5, 1e-3])
    particles = particle_beam(lx, P, dtype)
    moments = lx.ParameterBeam.from_parameters(mu_x=f(2e-5), mu_y=f(-1e-5), sigma_x=f(6e-5), sigma_xp=f(1e-5), sigma_y=f(5e-5),
                                               sigma_yp=f(1e-5), sigma_s=f(1e-5), sigma_p=f(1e-3), energy=f(1e8), dtype=dtype)
    for beam in (particles, moments):
        segment, screen = lattice()
        assert segment.track(beam) is lx.Beam.empty
        alone = screen.reading
        segment, screen = lattice()
        inside = segment.track_along(beam, screens=True).image_at("SCR")
        assert alone.shape == inside.shape and alone.dtype == inside.dtype == np.dtype(dtype) and alone.max() > 0
        if beam is particles:
            assert np.array_equal(alone, inside) and np.all(alone.sum(axis=(-2, -1)) > 2000)
        else:
            assert_gaussian_image(alone, inside.astype(np.float64).astype(dtype), dtype)
