"""
`helpers.covariance_distances` -- the check the GPU suite holds every producer of a moment record to, on all 36 entries of
the covariance -- without a GPU: that it BITES, and that the inputs of the GPU tests let it.

The oracle's own chain on `mixed_desc` plays the kernel: its covariance at every point is corrupted the ways a kernel
could get one wrong (a triangle slot routed to another's place, an entry mis-scaled, a shift correction left out), and the
worst distance must then exceed TOL_MOM[float32], the widest tolerance any GPU test compares at.  Uncorrupted, the
oracle's float32 chain stays within that tolerance of its float64 chain on every entry, so the tolerance is attainable.

The condition on the inputs, from the oracle alone: every off-diagonal |correlation| >= 0.1 -- a dropped entry is then
1000 tolerances away, one scaled by 1 + 1e-3 more than one -- at some point of a trace in every sample; for the
`Segment.track` cases, whose only point is the end, at the end in every sample.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import OFF_DIAGONAL, biased_covariance, correlations, covariance_distances, make_lattice
from .test_gpu_covariance import BIG_N, BIG_SHAPE, SHAPES, TILE_EDGES, shared_case, track_case
from .test_gpu_parity import TOL_MOM
from .test_gpu_trace import chain, every_element_kind_case, two_tiles_per_wave_case, upcast

TOL = TOL_MOM[np.float32]  # the widest tolerance a GPU test compares a covariance at
MIN_CORRELATION = 0.1
TRIANGLE = [(i, j) for i in range(6) for j in range(i, 6)]


def chain_of(desc, P, energy, dtype):
    _, specs = make_lattice(desc, dtype)
    with np.errstate(all="ignore"):
        beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    return beams


@pytest.fixture(scope="module")
def oracle_chain():
    """`mixed_desc` (3,), n = 1000: the float64 chain of the float32 lattice's numbers, and the float32 chain."""
    desc, P, energy = every_element_kind_case(np.float32, (3,), 1000)
    beams32 = chain_of(desc, P, energy, np.float32)[:-1]  # (without the point behind the dead cavity)
    beams64 = chain_of(upcast(desc), P.astype(np.float64), energy.astype(np.float64), np.float64)[:-1]
    particles = np.stack([b["particles"] for b in beams64], axis=-3)  # (B, points, N, 7)
    return particles, np.stack([b["particles"] for b in beams32], axis=-3)


def set_entry(cov, slot, value):
    i, j = slot
    cov[..., i, j] = value
    cov[..., j, i] = value


def test_an_uncorrupted_covariance_passes_and_float32_can_hold_every_entry(oracle_chain):
    p64, p32 = oracle_chain
    assert covariance_distances(biased_covariance(p64), p64)[0] == 0.0
    worst, where = covariance_distances(biased_covariance(p32), p64)
    print(f"the oracle's float32 chain against its float64 chain: worst of 36 entries {worst:.2e} at (i, j, (sample, point)) {where}")
    assert worst <= TOL, (worst, where)
    with pytest.raises(AssertionError, match="NaN pattern"):
        bad = biased_covariance(p64)
        bad[1, 2, 3, 4] = np.nan
        covariance_distances(bad, p64)


@pytest.mark.parametrize("slot", OFF_DIAGONAL)
def test_two_triangle_slots_swapped(oracle_chain, slot):
    """Slot (i, j) and the next slot of the record's triangle trade places (a wrong `tri_row` / `tri_col`, a butterfly
    level that routes a cell to the neighbouring lane)."""
    p64, _ = oracle_chain
    cov = biased_covariance(p64)
    other = TRIANGLE[(TRIANGLE.index(slot) + 1) % len(TRIANGLE)]
    a, b = cov[..., slot[0], slot[1]].copy(), cov[..., other[0], other[1]].copy()
    set_entry(cov, slot, b)
    set_entry(cov, other, a)
    worst, where = covariance_distances(cov, p64)
    assert worst > TOL and (where[0], where[1]) in (slot, slot[::-1], other, other[::-1]), (slot, other, worst, where)


@pytest.mark.parametrize("slot", TRIANGLE)
def test_one_entry_scaled_by_a_thousandth(oracle_chain, slot):
    p64, _ = oracle_chain
    cov = biased_covariance(p64)
    set_entry(cov, slot, cov[..., slot[0], slot[1]] * (1 + 1e-3))
    worst, where = covariance_distances(cov, p64)
    assert worst > TOL and (where[0], where[1]) in (slot, slot[::-1]), (slot, worst, where)


@pytest.mark.parametrize("slot", [(0, 1), (0, 2), (1, 3), (2, 3), (0, 0), (3, 3)])
def test_one_entry_left_uncentred(oracle_chain, slot):
    """S_ij / n without - S_i S_j / n^2: the transverse centroid is kicked by the correctors and the misaligned magnets
    to the size of the beam itself, so mu_i mu_j is of the order of sigma_i sigma_j in the transverse slots."""
    p64, _ = oracle_chain
    cov = biased_covariance(p64)
    mean = p64[..., :6].mean(axis=-2)
    set_entry(cov, slot, cov[..., slot[0], slot[1]] + mean[..., slot[0]] * mean[..., slot[1]])
    worst, where = covariance_distances(cov, p64)
    assert worst > TOL and (where[0], where[1]) in (slot, slot[::-1]), (slot, worst, where)


def test_one_entry_dropped(oracle_chain):
    """Every off-diagonal entry set to 0 in turn: |correlation| itself is the distance, >= 0.1 somewhere."""
    p64, _ = oracle_chain
    for slot in OFF_DIAGONAL:
        cov = biased_covariance(p64)
        set_entry(cov, slot, 0.0)
        worst, where = covariance_distances(cov, p64)
        assert worst >= MIN_CORRELATION and (where[0], where[1]) in (slot, slot[::-1]), (slot, worst, where)


def test_survivors_one_left_and_nobody_left():
    """`alive`: each sample's own survivor set; one survivor has no spread -- 0 exactly, and any other number fails;
    nobody left is NaN everywhere, and a number there fails."""
    P = o.gaussian_particles((3,), 50, seed=1, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    alive = np.ones((3, 50), dtype=bool)
    alive[0, 10:] = False
    alive[1, :] = False
    alive[1, 7] = True
    alive[2, :] = False
    ref = biased_covariance(P, alive)
    assert np.allclose(ref[0], np.cov(P[0, :10, :6].T, bias=True), rtol=1e-12, atol=0.0)
    assert np.all(ref[1] == 0.0) and np.isnan(ref[2]).all()
    assert covariance_distances(ref, P, alive=alive)[0] == 0.0
    noisy = ref.copy()
    noisy[1, 0, 1] = noisy[1, 1, 0] = 1e-30
    assert covariance_distances(noisy, P, alive=alive)[0] > 1.0
    number = ref.copy()
    number[2] = 0.0
    with pytest.raises(AssertionError, match="NaN pattern"):
        covariance_distances(number, P, alive=alive)


# ---------------------------------------------------------------------------------------------
# the condition on the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------


def assert_correlated_somewhere(beams, what):
    """Every off-diagonal slot >= MIN_CORRELATION at some point, in every sample."""
    best = np.max(np.stack([correlations(b["particles"]) for b in beams]), axis=0)  # (*batch, 15)
    worst = float(best.min())
    print(f"{what}: smallest over samples and slots of the largest |correlation| along the lattice {worst:.3f}")
    assert worst >= MIN_CORRELATION, (what, worst, OFF_DIAGONAL[int(np.argmin(best.min(axis=tuple(range(best.ndim - 1)))))])


@pytest.mark.parametrize("n", [63, 64, 1000, 70_001])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
def test_the_mixed_lattice_of_the_trace_tests_correlates_every_slot(shape, n):
    desc, P, energy = every_element_kind_case(np.float64, shape, n)
    assert_correlated_somewhere(chain_of(desc, P, energy, np.float64), f"mixed_desc {shape} n={n}")


@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257])
def test_the_mixed_lattice_at_the_tile_edges_of_the_plain_trace(n):
    desc, P, energy = every_element_kind_case(np.float64, (3,), n)
    assert_correlated_somewhere(chain_of(desc, P, energy, np.float64), f"mixed_desc (3,) n={n}")


@pytest.mark.parametrize("dtype,shared", [(np.float64, False), (np.float32, True)])
def test_the_six_element_lattice_correlates_every_slot_in_all_300_samples(dtype, shared):
    desc, P, energy = two_tiles_per_wave_case(dtype, shared)
    P = np.ascontiguousarray(np.broadcast_to(P, (*energy.shape, *P.shape[-2:])))
    assert_correlated_somewhere(chain_of(desc, P, energy, dtype), f"coupled_desc (300,) n={P.shape[-2]} shared={shared}")


def assert_correlated_at_the_end(particles, what):
    """Every off-diagonal slot >= MIN_CORRELATION at the end of the lattice, in every sample of the case."""
    rho = correlations(particles)
    print(f"{what}: smallest |correlation| over samples and slots, at the end {float(rho.min()):.3f}")
    assert rho.min() >= MIN_CORRELATION, (what, float(rho.min()), np.argwhere(rho < MIN_CORRELATION)[:5])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_track_cases_correlate_every_slot_at_the_end_in_every_sample(shape):
    for n in TILE_EDGES[1:]:  # (one particle has no spread)
        for dtype in (np.float32, np.float64):
            _, P, _, ref = track_case(dtype, shape, n, "mixed")
            assert_correlated_at_the_end(ref, f"track, mixed {np.dtype(dtype).name} {shape} n={n}")
            assert correlations(P).min() >= MIN_CORRELATION  # (the beam a host-particles case reads)


def test_the_big_and_the_shared_track_cases_correlate_every_slot_at_the_end_in_every_sample():
    for dtype in (np.float32, np.float64):
        _, _, _, ref = track_case(dtype, BIG_SHAPE, BIG_N, "coupled")
        assert_correlated_at_the_end(ref, f"track, coupled {np.dtype(dtype).name} {BIG_SHAPE} n={BIG_N}")
        _, _, _, ref = shared_case(dtype)
        assert_correlated_at_the_end(ref, f"track, coupled, shared beam {np.dtype(dtype).name}")


@pytest.mark.parametrize("n", [129, 257, 1000])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
def test_the_coupled_lattice_of_the_losses_tests_correlates_every_slot_of_the_survivors(shape, n):
    """Variant "c" of tests/test_gpu_trace_losses.py: the condition holds for the SURVIVORS at some point, in every sample.
    (Variants "a" and "b" have neither tilt nor dipole: their cross-plane entries are compared all the same, as noise.)"""
    from .test_gpu_trace_losses import expectation, mixed_case

    desc, P, energy = mixed_case(np.float64, shape, n, "c")
    beams, _, lost_at, on_edge, _, apertures = expectation(desc, P, energy, np.float64)
    assert not on_edge.any()
    killer = np.array(apertures + [len(desc)])[lost_at]
    best = 0.0
    for k, beam in enumerate(beams):
        best = np.maximum(best, correlations(beam["particles"], killer >= k))
    print(f"losses, coupled {shape} n={n}: smallest over samples and slots of the largest |correlation| {float(best.min()):.3f}; "
          f"survivors {(lost_at < 0).sum(axis=-1).tolist()}")
    assert best.min() >= MIN_CORRELATION and np.all((lost_at < 0).sum(axis=-1) >= 2)
