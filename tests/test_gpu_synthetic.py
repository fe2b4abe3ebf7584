"""
`ParticleBeam.synthetic` on the GPU (`lynx_fill_gaussian` / `k_fill_gaussian`) IS the formula of
tests/synthetic_reference.py, scalar by scalar -- tests/test_synthetic_host.py shows that the formula is a sound Gaussian
generator.  The synthetic beam is the input of the benchmark, of every full-size parity test and of the speed scripts, all
of which compare GPU against oracle on the same particles: none of them would see a generator that ignored `mu`,
correlated two coordinates or repeated itself across the batch.

The kernel differs from the restatement only in `log` and `cos` (every other step is exact or correctly rounded on both
sides).  With z = r cos(t), r = sqrt(-2 ln u1):
  * device and host `log` within 2 and 1 ulp: ln u1 off by <= 3 ulp, r by <= 1.5 ulp + 2 roundings of sqrt = 2.5 ulp;
  * device and host `cos` within 2 and 1 ulp of |cos| <= 1: 3 ulp of r after the product, which rounds once more on
    both sides: 2 more half-ulps;
  * sigma z and mu + sigma z round once each on both sides: <= 1 ulp of (|mu| + sigma r) each;
in all < 9 ulp of (|mu_c| + sigma_c r), an ulp being at most 2^-52 of the value: 16 x 2^-53 x (|mu_c| + sigma_c r) with
little room for anything else.  Measured on an MI355X: the largest |got - ref| / (2^-53 (|mu_c| + sigma_c r)) over all
cases below is 3.42 (of the 16 allowed; 1.7 % of the scalars differ at all), and no float32 value differs from float32(ref).
"""

import functools

import numpy as np
import pytest

from .test_gpu_parity import TOL_MOM
from .synthetic_reference import fill_gaussian_reference

pytestmark = pytest.mark.gpu

MU = np.array([3e-4, -2e-5, -1e-4, 4e-6, 2e-6, 1e-3])
SIGMA = np.array([1e-4, 1e-7, 1e-3, 1e-5, 1e-6, 3e-4])  # spans 1e-7 ... 1e-3
SEED = 11
# (3,) x 100 003 is 2 100 063 scalars: more than the 8192 x 256 = 2 097 152 threads of the capped grid, so the
# grid-stride loop goes round a second time for the last 2911 of them
CASES = [((1,), 1), ((1,), 37), ((1,), 4097), ((2, 3), 1000), ((3,), 100_003)]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()
    return lynx_amd


@functools.lru_cache(maxsize=None)
def reference(batch, n, seed=SEED):
    P, r = fill_gaussian_reference(batch, n, MU, SIGMA, seed)
    P.setflags(write=False)
    r.setflags(write=False)
    return P, r


def synthetic(lx, batch, n, dtype, seed=SEED):
    return lx.ParticleBeam.synthetic(batch, n, mu=MU, sigma=SIGMA, energy=1.3e8, seed=seed, dtype=dtype)


def assert_is_the_formula(got, batch, n, dtype, seed=SEED):
    ref, r = reference(batch, n, seed)
    assert got.shape == ref.shape and got.dtype == np.dtype(dtype)
    assert np.all(got[..., 6] == 1)
    if np.dtype(dtype) == np.float64:
        scale = 2.0**-53 * (np.abs(MU) + SIGMA * r[..., :6])
        ratio = np.abs(got[..., :6] - ref[..., :6]) / scale
        print(f"float64 {batch} x {n}: largest |got - ref| = {ratio.max():.3f} x 2^-53 (|mu| + sigma r); "
              f"{np.count_nonzero(ratio)} of {ratio.size} differ")
        assert np.all(ratio <= 16.0), (float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
    else:
        ref32 = ref.astype(np.float32)
        differ = got != ref32
        print(f"float32 {batch} x {n}: {np.count_nonzero(differ)} of {differ.size} differ from float32(ref)")
        # a difference needs the float64 value within ~1e-14 (relative) of a float32 rounding boundary
        assert np.all(np.abs(got - ref32) <= np.spacing(np.abs(ref32)))
        assert np.count_nonzero(differ) <= 1e-4 * differ.size


@pytest.mark.parametrize("batch,n", CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_kernel_is_the_formula(lx, dtype, batch, n):
    beam = synthetic(lx, batch, n, dtype)
    assert beam.batch_shape == batch and beam.num_particles == n and beam.dtype == np.dtype(dtype)
    assert beam.energy.shape == batch and np.all(beam.energy == dtype(1.3e8)) and beam.energy.dtype == np.dtype(dtype)
    got = np.asarray(beam.particles)
    assert_is_the_formula(got, batch, n, dtype)
    # the same call twice: the same bits
    assert np.array_equal(np.asarray(synthetic(lx, batch, n, dtype).particles), got)
    if n > 1:  # the GPU moment pass on these particles against numpy on the restatement (rounded to the dtype)
        stored = reference(batch, n)[0].astype(dtype).astype(np.float64)
        mean, std = stored[..., 0].mean(axis=-1), stored[..., 0].std(axis=-1, ddof=1)
        tol = TOL_MOM[dtype]
        assert np.all(np.abs(np.asarray(beam.mu_x, dtype=np.float64) - mean) <= tol * (np.abs(mean) + std))
        assert np.all(np.abs(np.asarray(beam.sigma_x, dtype=np.float64) - std) <= tol * std)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_sample_does_not_depend_on_the_batch_behind_it(lx, dtype):
    """The counter is the flat index: sample 0 of three is the single sample of the same size and seed, and no other is."""
    three = np.asarray(synthetic(lx, (3,), 4097, dtype).particles)
    one = np.asarray(synthetic(lx, (1,), 4097, dtype).particles)
    assert np.array_equal(three[0], one[0])
    for a, b in ((0, 1), (0, 2), (1, 2)):  # no sample repeats another, in any scalar of the six coordinates
        assert not np.any(three[a, :, :6] == three[b, :, :6])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_seed_above_2_63_arrives_whole(lx, dtype):
    seed = 2**63 + 5
    got = np.asarray(synthetic(lx, (2,), 1000, dtype, seed=seed).particles)
    assert_is_the_formula(got, (2,), 1000, dtype, seed=seed)
    for other in (5, 2**63, 2**63 + 4):  # the top bit and the low bits both count
        assert not np.any(got[..., :6] == reference((2,), 1000, other)[0].astype(dtype)[..., :6])
