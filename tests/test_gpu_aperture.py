"""
Active `Aperture` on the GPU (lynx_aperture_mask / lynx_aperture_compact) against the oracle's
mask (reference lynx/accelerator/aperture.py:69-108): which particles survive, their order,
the lost ones, and the behaviour inside a Segment.  The reference has no test for this element.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()
    return lynx_amd


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", ["rectangular", "elliptical"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 50_001])
def test_single_sample_loses_particles_in_order(lx, dtype, shape, n):
    P = o.gaussian_particles((1,), n, seed=n, dtype=dtype, sigma=[1e-3, 1e-4, 2e-3, 1e-4, 1e-5, 1e-3])
    P[0, 0, 0] = 1e-3  # exactly on the rectangular limit: lost (strict inequality, aperture.py:79)
    charges = np.arange(n, dtype=dtype)[None] * 1e-15
    aperture = lx.Aperture(x_max=np.array([1e-3], dtype), y_max=np.array([1.5e-3], dtype), shape=shape, dtype=dtype)
    beam = lx.ParticleBeam(P, np.array([1e8], dtype), particle_charges=charges, dtype=dtype)
    keep = o.aperture_mask(P, np.array([1e-3], dtype), np.array([1.5e-3], dtype), shape)[0]
    out = aperture.track(beam)
    if keep.sum() == 0:
        assert out is lx.Beam.empty
        return
    assert out.num_particles == keep.sum() and out.batch_shape == (1,)
    assert np.array_equal(np.asarray(out.particles)[0], P[0][keep])          # survivors, original order
    assert np.array_equal(np.asarray(aperture.lost_particles), P[0][~keep])   # the rest, original order
    assert np.array_equal(out.particle_charges[0], charges[0][keep])
    assert np.array_equal(aperture.lost_particle_charges, charges[0][~keep])
    assert np.array_equal(out.energy, beam.energy)
    assert np.isclose(out.total_charge[0], charges[0][keep].sum())


def test_parameter_beam_and_inactive_aperture_pass_through(lx):
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    beam = lx.ParameterBeam.from_parameters(sigma_x=f(1e-2))
    assert lx.Aperture(x_max=f(1e-6), y_max=f(1e-6)).track(beam) is beam  # aperture.py:70-72
    pbeam = lx.ParticleBeam.from_parameters(num_particles=1000, sigma_x=f(1e-2), seed=0)
    assert lx.Aperture(x_max=f(1e-6), y_max=f(1e-6), is_active=False).track(pbeam) is pbeam


def test_batches_are_accepted_as_long_as_nothing_is_lost(lx):
    f = lambda v: np.full((2, 3), v, dtype=np.float32)  # noqa: E731
    beam = lx.ParticleBeam.from_parameters(num_particles=5000, sigma_x=np.array([1e-4], np.float32), seed=1).broadcast((2, 3))
    wide = lx.Aperture(x_max=f(np.inf), y_max=f(np.inf))
    out = wide.track(beam)
    assert np.array_equal(np.asarray(out.particles), np.asarray(beam.particles)) and wide.lost_particles.shape == (0, 7)
    narrow = lx.Aperture(x_max=f(1e-4), y_max=f(1.0))
    with pytest.raises(NotImplementedError, match="particles lost in a batch"):
        narrow.track(beam)


def test_aperture_inside_a_segment(lx):
    """ARES-style stretch: infinite active apertures (as in ARESlatticeStage3v1_9.json) and a real one."""
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    P = o.gaussian_particles((1,), 20_000, seed=4, dtype=np.float32, sigma=[2e-4, 1e-5, 2e-4, 1e-5, 1e-5, 1e-3])
    beam = lx.ParticleBeam(P, f(1e8))
    inf = np.array([np.inf], np.float32)
    collimator = lx.Aperture(x_max=f(3e-4), y_max=f(3e-4), shape="elliptical", name="COL")
    seg = lx.Segment([lx.Aperture(x_max=inf, y_max=inf, name="ARLISLHG1"), lx.Drift(f(0.5)),
                      lx.Quadrupole(f(0.122), k1=f(4.2)), collimator, lx.Drift(f(0.3)),
                      lx.Solenoid(f(0.09), k=f(0.0)), lx.Screen(is_active=False), lx.Drift(f(0.2))])
    assert not seg.is_skippable
    out = seg.track(beam)
    # oracle: track to the collimator, clip, track on
    head = o.segment_track([o.Drift(f(0.5)), o.Quadrupole(f(0.122), k1=f(4.2))], o.particle_beam(P, f(1e8)), np.float32)
    keep = o.aperture_mask(head["particles"], f(3e-4), f(3e-4), "elliptical")[0]
    tail = o.segment_track([o.Drift(f(0.3)), o.Solenoid(f(0.09), k=f(0.0)), o.Drift(f(0.2))],
                           o.particle_beam(head["particles"][:, keep], f(1e8)), np.float32)
    got = np.asarray(out.particles)
    assert 0 < keep.sum() < 20_000 and got.shape == tail["particles"].shape
    assert np.allclose(got, tail["particles"], rtol=2e-5, atol=1e-9)
    assert collimator.lost_particles.shape == (20_000 - keep.sum(), 7)
    assert np.isclose(out.sigma_x[0], tail["particles"][0, :, 0].std(ddof=1), rtol=1e-4)
    # a ParameterBeam goes through the same lattice untouched by the apertures
    pout = seg.track(lx.ParameterBeam.from_parameters(sigma_x=f(2e-4)))
    assert pout.sigma_x.shape == (1,)


# ---------------------------------------------------------------------------------------------
# Masks built on purpose: the compaction at every chunk and thread boundary
# ---------------------------------------------------------------------------------------------

CHUNK = 1024  # kApertureChunk: 256 threads x 4 consecutive particles
X_MAX, Y_MAX = 1e-3, 1.5e-3
PATTERN_SIZES = [1, 4, 5, 1023, 1024, 1025, 2048, 2049, 4097]


def _thread_ramp(i):
    """The thread that owns particles 4t ... 4t + 3 keeps the first min(t % 5, 4) of them."""
    return (i % 4) < np.minimum((i // 4) % 5, 4)


PATTERNS = {
    "first_only_kept": lambda i: i == 0,
    "last_only_kept": lambda i: i == len(i) - 1,
    "last_only_lost": lambda i: i != len(i) - 1,
    "alternating": lambda i: i % 2 == 0,
    "chunk0_lost_chunk1_kept": lambda i: i >= CHUNK,  # (every chunk but the first is kept)
    "thread_ramp": _thread_ramp,
}


def pattern(name, n):
    return PATTERNS[name](np.arange(n))


# a pattern that keeps nobody or everybody at some N is `Beam.empty` / the nothing-lost case: asserted once each, below
PATTERN_CASES = [(name, n) for name in PATTERNS for n in PATTERN_SIZES if 0 < pattern(name, n).sum() < n]


def tagged_beam(lx, keep, dtype):
    """
    One sample whose particle i has x = 0 if keep[i], else 2 x_max; y = 0; x', y', s and delta carry tags made of i
    (exact in float32 up to 2^24 / 4), the charge is i x 1e-15: order, content and charges of whatever comes out can be
    compared bit by bit.
    """
    n = len(keep)
    i = np.arange(n)
    P = np.ones((1, n, 7), dtype=dtype)
    P[0, :, 0] = np.where(keep, 0.0, 2 * X_MAX)
    P[0, :, 1], P[0, :, 2], P[0, :, 3], P[0, :, 4], P[0, :, 5] = i, 0.0, -i, i + 0.25, 4 * i + 1
    charges = (i * 1e-15).astype(dtype)[None]
    return P, charges, lx.ParticleBeam(P, np.array([1e8], dtype), particle_charges=charges, dtype=dtype)


def make_aperture(lx, dtype, shape, x_max=X_MAX, y_max=Y_MAX, **kw):
    return lx.Aperture(x_max=np.array([x_max], dtype), y_max=np.array([y_max], dtype), shape=shape, dtype=dtype, **kw)


def assert_split(lx, aperture, out, P, charges, keep):
    assert out is not lx.Beam.empty and out.num_particles == keep.sum() and out.batch_shape == (1,)
    assert np.array_equal(np.asarray(out.particles)[0], P[0][keep])
    assert np.array_equal(np.asarray(aperture.lost_particles), P[0][~keep])
    assert np.array_equal(out.particle_charges[0], charges[0][keep])
    assert np.array_equal(aperture.lost_particle_charges, charges[0][~keep])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,n", PATTERN_CASES)
def test_masks_built_on_purpose_are_compacted_in_order(lx, dtype, name, n):
    keep = pattern(name, n)
    P, charges, beam = tagged_beam(lx, keep, dtype)
    assert np.array_equal(o.aperture_mask(P, [X_MAX], [Y_MAX], "rectangular")[0], keep)  # (the helper does what it says)
    aperture = make_aperture(lx, dtype, "rectangular")
    assert_split(lx, aperture, aperture.track(beam), P, charges, keep)


def test_the_cases_cover_every_pattern_and_size():
    assert len(PATTERN_CASES) == 43  # 6 x 9, less the 6 at N = 1, chunk0 at 4 ... 1024 (4) and thread_ramp at 4: empty or total
    assert all(any(n == size for _, n in PATTERN_CASES) for size in PATTERN_SIZES[1:])
    assert pattern("thread_ramp", 24).tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", ["rectangular", "elliptical"])
def test_nobody_kept_and_nobody_lost(lx, dtype, shape):
    n = 1025
    P, charges, beam = tagged_beam(lx, np.zeros(n, dtype=bool), dtype)
    aperture = make_aperture(lx, dtype, shape)
    assert aperture.track(beam) is lx.Beam.empty
    assert np.array_equal(np.asarray(aperture.lost_particles), P[0]) and np.array_equal(aperture.lost_particle_charges, charges[0])
    P, charges, beam = tagged_beam(lx, np.ones(n, dtype=bool), dtype)
    out = aperture.track(beam)
    assert np.array_equal(np.asarray(out.particles), P) and np.array_equal(out.particle_charges, charges)
    assert aperture.lost_particles.shape == (0, 7) and aperture.lost_particle_charges.shape == (0,)
    # x_max = 0: nobody fits, not even x = 0 (a strict inequality; 0 / 0 in the ellipse)
    closed = make_aperture(lx, dtype, shape, x_max=0.0)
    assert not o.aperture_mask(P, [0.0], [Y_MAX], shape).any()
    assert closed.track(beam) is lx.Beam.empty
    assert np.array_equal(np.asarray(closed.lost_particles), P[0]) and np.array_equal(closed.lost_particle_charges, charges[0])


def test_lost_particles_are_those_of_the_last_active_track(lx):
    dtype = np.float32
    aperture = make_aperture(lx, dtype, "rectangular")
    P1, charges1, beam1 = tagged_beam(lx, pattern("alternating", 1025), dtype)
    P2, charges2, beam2 = tagged_beam(lx, pattern("thread_ramp", 37), dtype)
    P2[..., 5] += 0.5
    beam2 = lx.ParticleBeam(P2, np.array([1e8], dtype), particle_charges=charges2, dtype=dtype)
    assert_split(lx, aperture, aperture.track(beam1), P1, charges1, pattern("alternating", 1025))
    assert_split(lx, aperture, aperture.track(beam2), P2, charges2, pattern("thread_ramp", 37))
    aperture.is_active = False  # an inactive aperture passes the beam on and leaves what it holds alone
    held, held_charges = aperture.lost_particles, aperture.lost_particle_charges
    assert aperture.track(beam1) is beam1
    assert aperture.lost_particles is held and aperture.lost_particle_charges is held_charges
    assert np.array_equal(np.asarray(held), P2[0][~pattern("thread_ramp", 37)])


# ---------------------------------------------------------------------------------------------
# Limits per sample
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch", [(3,), (2, 3)])
def test_limits_per_sample_lose_nobody_only_if_indexed_right(lx, dtype, batch):
    """
    Sample b is one unit beam scaled by s_b in x (ascending) and t_b in y (descending); its limits are 1 % above its own
    largest |x| and |y|.  The limits of ANY other sample, and its own with x_max and y_max exchanged, lose particles (checked
    here with the oracle's mask), so the beam comes back whole only if the kernel reads x_max[b] and y_max[b].
    """
    n, B = 1500, int(np.prod(batch))
    unit = o.gaussian_particles((1,), n, seed=3, dtype=np.float64, sigma=np.ones(6))[0]
    s = (1e-4 * 1.5 ** np.arange(B)).reshape(batch)
    t = (1.2e-4 * 1.5 ** np.arange(B)[::-1]).reshape(batch)
    P = np.ones((*batch, n, 7), dtype=dtype)
    P[..., :6] = unit[:, :6]
    P[..., 0] = (unit[:, 0] * s[..., None]).astype(dtype)
    P[..., 2] = (unit[:, 2] * t[..., None]).astype(dtype)
    x_max = (1.01 * np.abs(P[..., 0]).max(axis=-1)).astype(dtype)
    y_max = (1.01 * np.abs(P[..., 2]).max(axis=-1)).astype(dtype)
    assert o.aperture_mask(P, x_max, y_max).all()
    assert not o.aperture_mask(P, y_max, x_max).all(axis=-1).any()  # exchanged: every sample loses somebody
    flat, fx, fy = P.reshape(B, n, 7), x_max.reshape(B), y_max.reshape(B)
    for b in range(B):
        for other in range(B):
            if other != b:
                assert not o.aperture_mask(flat[b], fx[other], fy[other]).all(), (b, other)
    beam = lx.ParticleBeam(P, np.full(batch, 1e8, dtype), dtype=dtype)
    aperture = lx.Aperture(x_max=x_max, y_max=y_max, dtype=dtype)
    out = aperture.track(beam)
    assert np.array_equal(np.asarray(out.particles), P) and out.batch_shape == batch
    assert aperture.lost_particles.shape == (0, 7) and aperture.lost_particle_charges.shape == (0,)
    # the same with one limit for all samples (stride 0), wide enough for the widest
    shared = lx.Aperture(x_max=np.array([x_max.max()], dtype), y_max=np.array([y_max.max()], dtype), dtype=dtype)
    out = shared.track(beam)
    assert np.array_equal(np.asarray(out.particles), P) and shared.lost_particles.shape == (0, 7)
    # ... and x_max per sample next to a single y_max
    mixed = lx.Aperture(x_max=x_max, y_max=np.array([y_max.max()], dtype), dtype=dtype)
    assert np.array_equal(np.asarray(mixed.track(beam).particles), P) and mixed.lost_particles.shape == (0, 7)
    with pytest.raises(NotImplementedError, match="particles lost in a batch"):
        lx.Aperture(x_max=y_max, y_max=x_max, dtype=dtype).track(beam)


# ---------------------------------------------------------------------------------------------
# lynx_aperture_mask through the C ABI: what the Python layer never looks at for a batch
# ---------------------------------------------------------------------------------------------


def mask_through_the_c_abi(P, x_max, y_max, shape):
    """(mask, counts, offsets, totals) of lynx_aperture_mask; limits of size 1 go in with stride 0, else one per sample."""
    import ctypes as C

    from lynx_amd.device import dtype_code, get_runtime

    rt = get_runtime()
    dtype = P.dtype
    batch, n = P.shape[:-2], P.shape[-2]
    B = int(np.prod(batch))
    x_max, y_max = np.asarray(x_max, dtype=dtype).reshape(-1), np.asarray(y_max, dtype=dtype).reshape(-1)
    assert x_max.size == y_max.size and x_max.size in (1, B)
    chunks = (n + CHUNK - 1) // CHUNK
    mask, counts = rt.empty((*batch, n), np.uint8), rt.empty((B, chunks), np.int32)
    offsets, totals = rt.empty((B, chunks), np.int64), rt.empty((B,), np.int64)
    particles, x_dev, y_dev = rt.to_device(np.ascontiguousarray(P)), rt.to_device(x_max), rt.to_device(y_max)
    ptr = lambda a: C.c_void_p(a.ptr)  # noqa: E731
    rt.check(rt.lib.lynx_aperture_mask(rt.ctx, dtype_code(dtype), B, n, ptr(particles), ptr(x_dev), ptr(y_dev),
                                       int(x_max.size != 1), int(shape == "elliptical"), ptr(mask), ptr(counts), ptr(offsets),
                                       ptr(totals)))
    return mask.numpy().astype(bool), counts.numpy(), offsets.numpy(), totals.numpy()


def assert_mask_and_counts(P, x_max, y_max, shape):
    """The mask is the oracle's in the same dtype, exactly; counts, offsets and totals are that mask's.  Returns the mask."""
    got, counts, offsets, totals = mask_through_the_c_abi(P, x_max, y_max, shape)
    batch, n = P.shape[:-2], P.shape[-2]
    limits = [np.asarray(v, dtype=P.dtype) for v in (x_max, y_max)]
    keep = o.aperture_mask(P, *[v.reshape(batch) if v.size > 1 else v.reshape(()) for v in limits], shape)
    assert got.shape == keep.shape == (*batch, n)
    assert np.array_equal(got, keep), (int((got != keep).sum()), np.argwhere(got != keep)[:5])
    flat = keep.reshape(-1, n)
    chunks = (n + CHUNK - 1) // CHUNK
    padded = np.zeros((len(flat), chunks * CHUNK), dtype=np.int64)
    padded[:, :n] = flat
    per_chunk = padded.reshape(len(flat), chunks, CHUNK).sum(axis=-1)
    assert np.array_equal(totals, flat.sum(axis=-1))
    assert np.array_equal(counts, per_chunk)
    assert np.array_equal(offsets, np.cumsum(per_chunk, axis=-1) - per_chunk)
    return keep


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", ["rectangular", "elliptical"])
@pytest.mark.parametrize("n", [1000, 2500])
def test_counts_offsets_and_totals_of_a_batch_that_loses_particles(lx, dtype, shape, n):
    P = o.gaussian_particles((3,), n, seed=n + 1, dtype=dtype, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-5, 1e-3])
    x_max, y_max = np.array([0.5e-3, 1e-3, 2.5e-3], dtype), np.array([3e-3, 1.2e-3, 0.7e-3], dtype)
    keep = assert_mask_and_counts(P, x_max, y_max, shape)
    survivors = keep.sum(axis=-1)
    assert np.all(survivors > 0) and np.all(survivors < n) and len(set(survivors.tolist())) == 3
    # the limits of another sample, or x_max and y_max exchanged, give another mask
    assert not np.array_equal(keep, o.aperture_mask(P, x_max[[0, 0, 0]], y_max, shape))
    assert not np.array_equal(keep, o.aperture_mask(P, y_max, x_max, shape))
    assert_mask_and_counts(P, x_max[1:2], y_max[1:2], shape)  # one limit for all (stride 0)
    assert_mask_and_counts(P.reshape(1, 3, n, 7), x_max, y_max, shape)  # a batch of two dimensions is its flat form


# ---------------------------------------------------------------------------------------------
# Edges of the comparison.  liblynxhip is built with -ffp-contract=off and float32 division is correctly rounded, so
# x x / (xm xm) + y y / (ym ym) <= 1 rounds as numpy's does: an inequality below is a finding about the kernel.
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", ["rectangular", "elliptical"])
def test_non_finite_coordinates_and_particles_on_the_limit(lx, dtype, shape):
    xm, ym = dtype(X_MAX), dtype(Y_MAX)
    rows = {
        "inside": (0.5 * xm, 0.5 * ym), "x nan": (np.nan, 0), "y nan": (0, np.nan), "x +inf": (np.inf, 0), "x -inf": (-np.inf, 0),
        "y +inf": (0, np.inf), "y -inf": (0, -np.inf), "both nan": (np.nan, np.nan),
        "on +x_max": (xm, 0), "on -x_max": (-xm, 0), "on +y_max": (0, ym), "on -y_max": (0, -ym),
        "below +x_max": (np.nextafter(xm, dtype(0)), 0), "above -x_max": (-np.nextafter(xm, dtype(0)), 0),
        "above +x_max": (np.nextafter(xm, dtype(1)), 0), "above +y_max": (0, np.nextafter(ym, dtype(1))),
        "corner": (np.nextafter(xm, dtype(0)), np.nextafter(ym, dtype(0))), "origin": (0, 0),
    }
    P = np.ones((1, len(rows), 7), dtype=dtype)
    P[0, :, 1], P[0, :, 3:6] = np.arange(len(rows)), 0.0
    P[0, :, 0], P[0, :, 2] = [r[0] for r in rows.values()], [r[1] for r in rows.values()]
    keep = dict(zip(rows, assert_mask_and_counts(P, [xm], [ym], shape)[0]))
    assert keep["inside"] and keep["origin"] and keep["below +x_max"] and keep["above -x_max"]
    assert not any(keep[name] for name in rows if "nan" in name or "inf" in name)
    assert not keep["above +x_max"] and not keep["above +y_max"]
    on_the_limit = [keep[name] for name in rows if name.startswith("on ")]
    # the rectangle is open (aperture.py:78-82), the ellipse closed (aperture.py:83-86)
    assert on_the_limit == [shape == "elliptical"] * 4 and keep["corner"] == (shape == "rectangular")
    # ... and through the element: the survivors and the lost ones, NaN for NaN
    aperture = make_aperture(lx, dtype, shape)
    out = aperture.track(lx.ParticleBeam(P, np.array([1e8], dtype), dtype=dtype))
    mask = np.array(list(keep.values()))
    assert np.array_equal(np.asarray(out.particles)[0], P[0][mask])
    assert np.array_equal(np.asarray(aperture.lost_particles), P[0][~mask], equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_ellipse_with_an_infinite_half_axis(lx, dtype):
    ym = dtype(Y_MAX)
    P = o.gaussian_particles((1,), 1030, seed=9, dtype=dtype, sigma=[1.0, 1e-4, 1e-3, 1e-4, 1e-5, 1e-3])
    P[0, :6, 0] = [np.inf, -np.inf, np.nan, 1e15, 0.0, 0.0]
    P[0, :6, 2] = [0.0, 0.0, 0.0, 0.0, ym, np.nextafter(ym, dtype(1))]
    keep = assert_mask_and_counts(P, [np.inf], [ym], "elliptical")[0]
    assert keep[:6].tolist() == [False, False, False, True, True, False]  # (inf / inf is NaN; finite / inf is 0)
    assert np.array_equal(keep[6:], np.abs(P[0, 6:, 2]) <= ym) and 0 < keep[6:].sum() < 1024
    # inf for both: everybody finite is kept
    assert np.array_equal(assert_mask_and_counts(P, [np.inf], [np.inf], "elliptical")[0], np.isfinite(P[0, :, 0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", ["rectangular", "elliptical"])
def test_points_within_an_ulp_of_the_ellipse(lx, dtype, shape):
    xm, ym = dtype(X_MAX), dtype(Y_MAX)
    t = np.linspace(0.0, 2 * np.pi, 4096, endpoint=False)
    x, y = (float(xm) * np.cos(t)).astype(dtype), (float(ym) * np.sin(t)).astype(dtype)
    P = np.ones((1, 3 * 4096, 7), dtype=dtype)
    P[0, :, 1:6] = 0.0
    P[0, :, 0] = np.concatenate([x, np.nextafter(x, dtype(np.inf)), np.nextafter(x, dtype(-np.inf))])
    P[0, :, 2] = np.concatenate([y, y, y])
    keep = assert_mask_and_counts(P, [xm], [ym], shape)[0]
    if shape == "elliptical":  # the rounding decides: hundreds are kept and hundreds lost, on the curve and an ulp off it
        for group in keep.reshape(3, 4096):
            assert 200 < group.sum() < 4096 - 200
