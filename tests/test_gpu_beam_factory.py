"""
The device beam factory on the GPU: `lynx_fill_gaussian_rows` / `k_fill_gaussian_rows` behind
`ParticleBeam.from_parameters(on_device=True)`, `from_twiss(on_device=True)` and `from_parameter_beam`, and
`lynx_transform_particles` / `k_transform_particles` behind `transformed_to(on_device=True)`.

The generator IS the formula of tests/beam_factory_reference.py, scalar by scalar (tests/test_beam_factory_host.py shows
that the formula is a sound generator).  It differs from the restatement only in `log` and `cos` of every normal: by
tests/test_gpu_synthetic.py's derivation a single term m + L z is within 16 x 2^-53 (|m| + |L| r), r = sqrt(-2 ln u1);
every further product-and-add L_cj z_j rounds once more on each side, one more ulp each, so column c is within
(16 + 2 c) x 2^-53 (|m_c| + sum_{j <= c} |L_cj| r_j).  float32: the float64 value rounded once, so within one spacing of
float32(ref), and different at all only where the float64 value lies within ~1e-14 of a rounding boundary.
Measured on an MI355X: the largest float64 ratio |got - ref| / (2^-53 (|m_c| + sum |L_cj| r_j)) over all cases below is
3.96 (in column 5, of the 26 allowed there; 2.24 of 16 in column 0; 2.8 % of the scalars differ at all), and no float32
value differs from float32(ref).

The rescale is four IEEE operations in the dtype, in the order of the host path: bit for bit what `transformed_to()` gives.

Tiles: a wave writes 64 x 4 = 256 particles in float32 and 64 x 2 = 128 in float64, so 127 ... 129 and 255 ... 257 sit on
the edges of the first tile, (2, 3) x 1000 has tiles that straddle two samples (1000 is no multiple of 128), and
(3,) x 350 003 = 1 050 009 particles are more than the 1024 workgroups x 4 waves x 256 = 1 048 576 particles the capped
grid covers at once (float64: x 128 = 524 288): the tile loop goes round a second time (float64: a third).
"""

import functools

import numpy as np
import pytest

from .beam_factory_reference import fill_gaussian_rows_reference, rows_of, transform_reference
from .test_gpu_parity import TOL_MOM

pytestmark = pytest.mark.gpu

SEED = 11
CASES = [((1,), 1), ((1,), 37), ((1,), 127), ((1,), 128), ((1,), 129), ((1,), 255), ((1,), 256), ((1,), 257),
         ((1,), 4097), ((2, 3), 1000), ((3,), 350_003)]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()
    return lynx_amd


def parameters(batch, dtype):
    """Per-sample means, sigmas and correlations that all differ, as arrays of shape `batch` in the dtype."""
    b = np.arange(int(np.prod(batch)), dtype=np.float64).reshape(batch)
    p = dict(mu_x=3e-4 * (1 + b), mu_xp=-2e-5 * (1 + 0.5 * b), mu_y=-1e-4 * (1 + b), mu_yp=4e-6 * (b - 2.5),
             sigma_x=1e-4 * (1 + 0.3 * b), sigma_xp=1e-5 * (1 + 0.2 * b), sigma_y=2e-4 / (1 + b),
             sigma_yp=2e-5 * (1 + 0.1 * b), sigma_s=1e-5 * (1 + b), sigma_p=1e-3 * (1 + 0.5 * b))
    p["cor_x"] = (0.8 - 0.3 * b) * p["sigma_x"] * p["sigma_xp"]
    p["cor_y"] = (-0.6 + 0.25 * b) * p["sigma_y"] * p["sigma_yp"]
    p["cor_s"] = (0.3 + 0.1 * b) * p["sigma_s"] * p["sigma_p"]
    return {k: v.astype(dtype) for k, v in p.items()}


def rows_of_parameters(lx, p):
    """What from_parameters(on_device=True) uploads: mean and covariance in float64 from the arguments as the dtype holds them."""
    q = {k: np.asarray(v, dtype=np.float64).reshape(-1) for k, v in p.items()}
    B = len(q["mu_x"])
    mean = np.stack([q["mu_x"], q["mu_xp"], q["mu_y"], q["mu_yp"], np.zeros(B), np.zeros(B)], axis=-1)
    cov = np.zeros((B, 6, 6))
    for at, (s, sp, cor) in ((0, ("sigma_x", "sigma_xp", "cor_x")), (2, ("sigma_y", "sigma_yp", "cor_y")),
                             (4, ("sigma_s", "sigma_p", "cor_s"))):
        cov[:, at, at], cov[:, at + 1, at + 1] = q[s] ** 2, q[sp] ** 2
        cov[:, at, at + 1] = cov[:, at + 1, at] = q[cor]
    from lynx_amd.particles.particle_beam import covariance_factor

    return rows_of(mean, covariance_factor(cov))


@functools.lru_cache(maxsize=4)
def _reference(batch, n, rows_bytes, seed):
    ref, scale = fill_gaussian_rows_reference(batch, n, np.frombuffer(rows_bytes, dtype=np.float64), seed)
    ref.setflags(write=False)
    scale.setflags(write=False)
    return ref, scale


def reference(batch, n, rows, seed):
    """The restatement, computed once per (shape, rows, seed) and read by whoever needs it again."""
    return _reference(tuple(batch), n, np.ascontiguousarray(rows, dtype=np.float64).tobytes(), seed)


def assert_is_the_formula(got, batch, n, dtype, rows, seed=SEED):
    ref, scale = reference(batch, n, rows, seed)
    assert got.shape == ref.shape and got.dtype == np.dtype(dtype)
    assert np.all(got[..., 6] == 1)
    if np.dtype(dtype) == np.float64:
        ratio = np.abs(got[..., :6] - ref[..., :6]) / (2.0**-53 * scale)
        print(f"float64 {batch} x {n}: largest |got - ref| per column = {np.round(ratio.max(axis=tuple(range(ratio.ndim - 1))), 3)}"
              f" x 2^-53 (|m| + sum |L| r); {np.count_nonzero(ratio)} of {ratio.size} differ")
        assert np.all(ratio <= 16.0 + 2.0 * np.arange(6)), float(ratio.max())
    else:
        ref32 = ref.astype(np.float32)
        differ = got != ref32
        print(f"float32 {batch} x {n}: {np.count_nonzero(differ)} of {differ.size} differ from float32(ref)")
        assert np.all(np.abs(got - ref32) <= np.spacing(np.abs(ref32)))
        assert np.count_nonzero(differ) <= 1e-4 * differ.size
    return ref


@pytest.mark.parametrize("batch,n", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_from_parameters_is_the_formula(lx, dtype, batch, n):
    p = parameters(batch, dtype)
    energy = np.full(batch, 1.3e8)
    make = lambda: lx.ParticleBeam.from_parameters(num_particles=n, **p, energy=energy, dtype=dtype, seed=SEED,  # noqa: E731
                                                   on_device=True)
    beam = make()
    assert isinstance(beam.particles, lx.device.DeviceArray)
    assert beam.batch_shape == batch and beam.num_particles == n and beam.dtype == np.dtype(dtype)
    assert beam.energy.shape == batch and np.all(beam.energy == dtype(1.3e8)) and beam.energy.dtype == np.dtype(dtype)
    assert beam._charges is None and beam._zero_charge_shape == batch and np.all(beam.total_charge == 0)
    got = np.asarray(beam.particles)
    ref = assert_is_the_formula(got, batch, n, dtype, rows_of_parameters(lx, p))
    assert np.array_equal(np.asarray(make().particles), got)  # the same call twice: the same bits
    if n > 1:  # the GPU moment pass on these particles against numpy on the restatement (rounded to the dtype)
        stored = ref.astype(dtype).astype(np.float64)
        tol = TOL_MOM[dtype]
        for c, name in enumerate(("x", "xp", "y", "yp")):
            mean, std = stored[..., c].mean(axis=-1), stored[..., c].std(axis=-1, ddof=1)
            assert np.all(np.abs(np.asarray(getattr(beam, "mu_" + name), np.float64) - mean) <= tol * (np.abs(mean) + std))
            assert np.all(np.abs(np.asarray(getattr(beam, "sigma_" + name), np.float64) - std) <= tol * std)


def coupled_parameter_beam(lx, batch, dtype):
    """A ParameterBeam whose samples have full 6 x 6 covariances (x-y coupling and every other pair) and their own means."""
    B = int(np.prod(batch))
    A = np.random.default_rng(3).standard_normal((B, 6, 6))
    scale = np.array([2e-4, 3e-5, 1e-4, 2e-5, 1e-5, 1e-3])
    mu, cov = np.zeros((B, 7)), np.zeros((B, 7, 7))
    mu[:, :6] = np.random.default_rng(4).standard_normal((B, 6)) * scale
    mu[:, 6] = 1.0
    cov[:, :6, :6] = (A @ A.transpose(0, 2, 1)) * np.outer(scale, scale)
    return lx.ParameterBeam(mu.reshape(*batch, 7), cov.reshape(*batch, 7, 7), energy=np.full(batch, 2e8),
                            total_charge=np.full(batch, 1e-9), dtype=dtype)


@pytest.mark.parametrize("batch,n", [((1,), 257), ((2, 3), 1000)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_from_parameter_beam_is_the_formula(lx, dtype, batch, n):
    from lynx_amd.particles.particle_beam import covariance_factor

    pb = coupled_parameter_beam(lx, batch, dtype)
    beam = lx.ParticleBeam.from_parameter_beam(pb, n, seed=SEED)
    assert isinstance(beam.particles, lx.device.DeviceArray)
    assert beam.batch_shape == batch and beam.num_particles == n and beam.dtype == np.dtype(dtype)
    assert np.array_equal(beam.energy, pb.energy)
    assert np.allclose(beam.total_charge, 1e-9, rtol=1e-5) and beam.particle_charges.shape == (*batch, n)
    mu, cov = np.asarray(pb._mu, np.float64), np.asarray(pb._cov, np.float64)
    L = covariance_factor(cov[..., :6, :6])
    assert np.count_nonzero(L) == int(np.prod(batch)) * 21  # the general factor: nothing of the triangle is zero
    assert_is_the_formula(np.asarray(beam.particles), batch, n, dtype, rows_of(mu[..., :6], L))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sample_does_not_depend_on_the_batch_behind_it(lx, dtype):
    """The counter is the flat index: sample 0 of three is the single sample of the same row and seed, and no other is."""
    p = parameters((3,), dtype)
    three = np.asarray(lx.ParticleBeam.from_parameters(num_particles=4097, **p, dtype=dtype, seed=SEED, on_device=True).particles)
    one = np.asarray(lx.ParticleBeam.from_parameters(num_particles=4097, **{k: v[:1] for k, v in p.items()}, dtype=dtype,
                                                     seed=SEED, on_device=True).particles)
    assert np.array_equal(three[0], one[0])
    # the same row for all three samples: no sample repeats another, in any scalar of the six coordinates
    same = {k: np.repeat(v[:1], 3) for k, v in p.items()}
    three = np.asarray(lx.ParticleBeam.from_parameters(num_particles=4097, **same, dtype=dtype, seed=SEED, on_device=True).particles)
    assert np.array_equal(three[0], one[0])
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.any(three[a, :, :6] == three[b, :, :6])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_seed_above_2_63_arrives_whole(lx, dtype):
    seed = 2**63 + 5
    p = parameters((2,), dtype)
    got = np.asarray(lx.ParticleBeam.from_parameters(num_particles=1000, **p, dtype=dtype, seed=seed, on_device=True).particles)
    rows = rows_of_parameters(lx, p)
    assert_is_the_formula(got, (2,), 1000, dtype, rows, seed=seed)
    for other in (5, 2**63, 2**63 + 4):  # the top bit and the low bits both count
        ref = fill_gaussian_rows_reference((2,), 1000, rows, other)[0].astype(dtype)
        assert not np.any(got[..., :6] == ref[..., :6])
    # no seed: a seed is drawn, and two calls draw two
    a, b = (np.asarray(lx.ParticleBeam.from_parameters(num_particles=1000, **p, dtype=dtype, on_device=True).particles)
            for _ in range(2))
    assert not np.any(a[..., :6] == b[..., :6])


@pytest.mark.parametrize("batch,n", [((2, 3), 1000), ((1,), 257)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_diagonal_factor_gives_the_bits_of_synthetic(lx, dtype, batch, n):
    mu = np.array([3e-4, -2e-5, -1e-4, 4e-6, 0.0, 0.0]).astype(dtype).astype(np.float64)
    sigma = np.array([1e-4, 1e-7, 1e-3, 1e-5, 1e-6, 3e-4]).astype(dtype).astype(np.float64)
    full = lambda v: np.full(batch, v)  # noqa: E731
    new = lx.ParticleBeam.from_parameters(
        num_particles=n, mu_x=full(mu[0]), mu_xp=full(mu[1]), mu_y=full(mu[2]), mu_yp=full(mu[3]), sigma_x=full(sigma[0]),
        sigma_xp=full(sigma[1]), sigma_y=full(sigma[2]), sigma_yp=full(sigma[3]), sigma_s=full(sigma[4]),
        sigma_p=full(sigma[5]), dtype=dtype, seed=SEED, on_device=True)
    old = lx.ParticleBeam.synthetic(batch, n, mu=mu, sigma=sigma, seed=SEED, dtype=dtype)
    assert np.array_equal(np.asarray(new.particles), np.asarray(old.particles))


def twiss_standard_errors(beta, alpha, emittance, n):
    """
    Standard errors of (beta, alpha, emittance) estimated from n particles of a Gaussian plane, by the delta method:
    with a, b, c = var(x), cov(x, x'), var(x') = beta eps, -alpha eps, (1 + alpha^2) eps / beta and eps^2 = a c - b^2,
    the estimates (a^, b^, c^) have the Wishart covariance V = [[2 a^2, 2 a b, 2 b^2], [2 a b, a c + b^2, 2 b c],
    [2 b^2, 2 b c, 2 c^2]] / n, and a function f of them the variance grad f^T V grad f:
        eps = sqrt(a c - b^2):  grad = (c, -2 b, a) / (2 eps)
        beta = a / eps:         grad = (1 / eps - a c / (2 eps^3),  a b / eps^3,  -a^2 / (2 eps^3))
        alpha = -b / eps:       grad = (b c / (2 eps^3),  -1 / eps - b^2 / eps^3,  a b / (2 eps^3))
    For alpha = 0 these come to eps / sqrt(n), beta / sqrt(n) and 1 / sqrt(n): 0.3 % at the 100 000 particles below.
    """
    a, b, c, e = beta * emittance, -alpha * emittance, (1 + alpha**2) * emittance / beta, emittance
    V = np.array([[2 * a * a, 2 * a * b, 2 * b * b], [2 * a * b, a * c + b * b, 2 * b * c], [2 * b * b, 2 * b * c, 2 * c * c]]) / n
    grads = {"beta": np.array([1 / e - a * c / (2 * e**3), a * b / e**3, -a * a / (2 * e**3)]),
             "alpha": np.array([b * c / (2 * e**3), -1 / e - b * b / e**3, a * b / (2 * e**3)]),
             "emittance": np.array([c, -2 * b, a]) / (2 * e)}
    return {k: float(np.sqrt(g @ V @ g)) for k, g in grads.items()}


# the Twiss values of tests/test_beam_factory_host.py's two samples and one with alpha = 0 in x
TWISS = dict(beta_x=[61.475, 5.9, 10.0], alpha_x=[-1.2124, 3.556, 0.0], emittance_x=[3.5e-9, 2e-8, 1e-8],
             beta_y=[74.9, 0.7, 3.0], alpha_y=[1.0, -0.4, 0.5], emittance_y=[2.3e-9, 1e-8, 5e-9])


@pytest.mark.parametrize("dtype", DTYPES)
def test_from_twiss_gives_the_twiss_values_asked_for(lx, dtype):
    n = 100_000
    args = {k: np.array(v, dtype=dtype) for k, v in TWISS.items()}
    beam = lx.ParticleBeam.from_twiss(num_particles=n, **args, sigma_s=np.array([1e-5, 8e-6, 0.0], dtype=dtype),
                                      sigma_p=np.array([2e-3, 1e-3, 5e-4], dtype=dtype),
                                      cor_s=np.array([0.6 * 1e-5 * 2e-3, -0.9 * 8e-6 * 1e-3, 0.0], dtype=dtype),
                                      energy=np.full(3, 1e8, dtype=dtype), dtype=dtype, seed=SEED, on_device=True)
    assert isinstance(beam.particles, lx.device.DeviceArray) and beam.batch_shape == (3,) and beam.num_particles == n
    for plane in "xy":
        for b in range(3):
            asked = {k: float(args[f"{k}_{plane}"][b]) for k in ("beta", "alpha", "emittance")}
            se = twiss_standard_errors(asked["beta"], asked["alpha"], asked["emittance"], n)
            for k in asked:
                got = float(getattr(beam, f"{k}_{plane}")[b])
                print(f"{np.dtype(dtype)} sample {b} {k}_{plane}: {(got - asked[k]) / se[k]:+.2f} standard errors")
                assert abs(got - asked[k]) <= 5.0 * se[k], (k, plane, b, got, asked[k], se[k])
    assert np.all(np.asarray(beam.particles)[2, :, 4] == 0)  # sigma_s = 0: a beam, not a NaN


# ---- transformed_to(on_device=True) ----------------------------------------------------------------------------------

def targets(batch, dtype):
    """New means and sigmas, every one per sample."""
    b = np.arange(int(np.prod(batch)), dtype=np.float64).reshape(batch)
    t = dict(mu_x=-2e-4 * (1 + b), mu_xp=3e-5 / (1 + b), mu_y=1e-4 * (b - 1.5), mu_yp=-5e-6 * (1 + 0.5 * b),
             sigma_x=3e-4 * (1 + 0.2 * b), sigma_xp=2e-5 / (1 + 0.3 * b), sigma_y=5e-5 * (1 + b), sigma_yp=1e-5 * (1 + 0.1 * b),
             sigma_s=2e-5 * (1 + 0.4 * b), sigma_p=3e-3 / (1 + b), energy=1.2e8 * (1 + 0.1 * b))
    return {k: v.astype(dtype) for k, v in t.items()}


def assert_same_rescale(lx, beam, dtype, finite=True, **t):
    """on_device=True against the host path of the same beam, bit for bit; the result has the moments asked for."""
    host = beam.transformed_to(**t)
    dev = beam.transformed_to(**t, on_device=True)
    assert isinstance(dev.particles, lx.device.DeviceArray) and dev.dtype == np.dtype(dtype)
    want, got = np.asarray(host.particles), np.asarray(dev.particles)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    assert np.all(got[..., 6] == 1)
    assert np.array_equal(dev.energy, host.energy) and dev.energy.dtype == host.energy.dtype
    assert np.array_equal(dev.particle_charges, host.particle_charges)
    if finite and beam.num_particles > 1:
        tol = TOL_MOM[dtype]
        for name in ("x", "xp", "y", "yp", "s", "p"):
            sigma = np.asarray(getattr(dev, "sigma_" + name), np.float64)
            if "sigma_" + name in t:
                assert np.all(np.abs(sigma - t["sigma_" + name]) <= tol * np.abs(t["sigma_" + name])), name
            if "mu_" + name in t:
                mu = np.asarray(getattr(dev, "mu_" + name), np.float64)
                assert np.all(np.abs(mu - t["mu_" + name]) <= tol * (np.abs(t["mu_" + name]) + sigma)), name
    return dev


def source_beam(lx, batch, n, dtype, total_charge=None):
    beam = lx.ParticleBeam.from_parameters(num_particles=n, **parameters(batch, dtype), energy=np.full(batch, 1e8),
                                           total_charge=total_charge, dtype=dtype, seed=5)
    assert not beam._particles.on_device  # a host beam: the device path uploads it
    return beam


@pytest.mark.parametrize("batch,n", [((1,), 2), ((1,), 37), ((1,), 257), ((1,), 4097), ((2, 3), 1000), ((3,), 350_003)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_transformed_to_on_device_is_the_host_path(lx, dtype, batch, n):
    beam = source_beam(lx, batch, n, dtype, total_charge=np.full(batch, 2e-10) if n == 37 else None)
    assert_same_rescale(lx, beam, dtype, **targets(batch, dtype))
    t = targets(batch, dtype)  # a few arguments only, a new total charge: the others are the beam's own
    assert_same_rescale(lx, beam, dtype, sigma_x=t["sigma_x"], mu_yp=t["mu_yp"], total_charge=np.full(batch, 1e-9, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_device_path_matches_the_reference_expression(lx, dtype):
    """... and both are the expression of tests/beam_factory_reference.py on the rows the host path forms."""
    batch, n = (2, 3), 1000
    beam, t = source_beam(lx, batch, n, dtype), targets(batch, dtype)
    zeros = np.zeros(batch, dtype)
    names = ("x", "xp", "y", "yp", "s", "p")
    rows = np.stack([beam.mu_x, beam.mu_xp, beam.mu_y, beam.mu_yp, zeros, zeros]
                    + [getattr(beam, "sigma_" + k) for k in names] + [t["sigma_" + k] for k in names]
                    + [t["mu_x"], t["mu_xp"], t["mu_y"], t["mu_yp"], zeros, zeros], axis=-1)
    got = np.asarray(beam.transformed_to(**t, on_device=True).particles)
    assert np.array_equal(got, transform_reference(np.asarray(beam.particles), rows))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_beam_left_on_the_device_by_track(lx, dtype):
    batch, n = (2,), 4097
    f = lambda v: np.full(batch, v, dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(0.5)), lx.Quadrupole(f(0.2), k1=np.array([4.2, -3.0], dtype=dtype)), lx.Drift(f(0.3))])
    out = segment.track(source_beam(lx, batch, n, dtype))
    assert out._particles.on_device and out._particles._host is None
    dev = assert_same_rescale(lx, out, dtype, **targets(batch, dtype))
    # ... and what it made can be tracked again without having seen the host
    assert dev._particles._host is None
    again = segment.track(lx.ParticleBeam(np.asarray(dev.particles), dev.energy, dtype=dtype))
    assert np.array_equal(np.asarray(segment.track(dev).particles), np.asarray(again.particles))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_shared_beam_goes_in_with_stride_0(lx, dtype):
    shared = source_beam(lx, (1,), 4097, dtype).broadcast((3,))
    assert shared.is_shared and shared.batch_shape == (3,)
    dev = assert_same_rescale(lx, shared, dtype, **targets((3,), dtype))
    got = np.asarray(dev.particles)
    assert not dev.is_shared and got.shape == (3, 4097, 7)
    assert not np.any(got[0, :, :6] == got[1, :, :6])  # three targets: three different beams
    # a shared beam whose tiles straddle the samples: 1000 is no multiple of 128
    assert_same_rescale(lx, source_beam(lx, (1,), 1000, dtype).broadcast((2, 3)), dtype, **targets((2, 3), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_entry_point_in_place_and_what_it_refuses(lx, dtype):
    """include/lynx_hip.h: `d_p_out` may be `d_p_in` unless the stride is 0; a stride is 0 or N * 7."""
    import ctypes as C

    from lynx_amd.device import dtype_code

    rt = lx.device.get_runtime()
    batch, n = (2, 3), 1000
    beam, t = source_beam(lx, batch, n, dtype), targets(batch, dtype)
    want = np.asarray(beam.transformed_to(**t).particles)
    rows = np.concatenate([np.stack([beam.mu_x, beam.mu_xp, beam.mu_y, beam.mu_yp, np.zeros(batch, dtype), np.zeros(batch, dtype)], -1),
                           np.stack([getattr(beam, "sigma_" + k) for k in ("x", "xp", "y", "yp", "s", "p")], -1),
                           np.stack([t["sigma_" + k] for k in ("x", "xp", "y", "yp", "s", "p")], -1),
                           np.stack([t["mu_x"], t["mu_xp"], t["mu_y"], t["mu_yp"], np.zeros(batch, dtype), np.zeros(batch, dtype)], -1)], -1)
    p, d_rows = rt.to_device(np.asarray(beam.particles)), rt.to_device(rows)
    call = lambda src, stride, dst: rt.lib.lynx_transform_particles(  # noqa: E731
        rt.ctx, dtype_code(dtype), 6, n, C.c_void_p(src), stride, C.c_void_p(d_rows.ptr), C.c_void_p(dst))
    for stride in (7, n * 7 - 1, -n * 7):
        with pytest.raises(lx._ffi.LynxError, match="stride"):
            rt.check(call(p.ptr, stride, p.ptr))
    with pytest.raises(lx._ffi.LynxError, match="in place"):
        rt.check(call(p.ptr, 0, p.ptr))
    with pytest.raises(lx._ffi.LynxError):
        rt.check(call(None, n * 7, p.ptr))
    assert np.array_equal(p.numpy(), np.asarray(beam.particles))  # nothing was written by a refused call
    rt.check(call(p.ptr, n * 7, p.ptr))
    assert np.array_equal(p.numpy(), want)


@pytest.mark.filterwarnings("ignore:(divide by zero|invalid value) encountered:RuntimeWarning")  # (the host path's division)
@pytest.mark.parametrize("dtype", DTYPES)
def test_division_by_a_zero_sigma_is_the_host_paths(lx, dtype):
    """sigma_s = 0 in the incoming beam: 0 / 0 and c / 0, NaN and inf in the same places on both paths."""
    P = np.array(np.asarray(source_beam(lx, (2,), 257, dtype).particles))
    P[0, :, 4], P[1, :, 4] = 0.0, 1e-3
    beam = lx.ParticleBeam(P, np.full(2, 1e8), dtype=dtype)
    assert np.all(beam.sigma_s == 0)
    dev = assert_same_rescale(lx, beam, dtype, finite=False, **targets((2,), dtype))
    got = np.asarray(dev.particles)
    assert np.all(np.isnan(got[0, :, 4])) and np.all(np.isinf(got[1, :, 4])) and np.all(np.isfinite(got[..., [0, 1, 2, 3, 5, 6]]))
