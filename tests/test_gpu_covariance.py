"""
The WHOLE 6 x 6 covariance out of `Segment.track` and `lynx_moments`, every one of the 36 entries against numpy.

Two producers: the tracking kernel's epilogue with `config.fused_covariance = True` (LYNX_TRACK_COVARIANCE: `full_cov` in
`plan_track`, the instantiations `launch_direct_m<T, 1|2|3, true>` and `launch_units_inst<2|3, true, 1|2>`), and the extra
pass behind `ParticleBeam.covariance()` (`lynx_moments(..., covariance=1)`: the same streaming kernel with S = 0).  Each
record is compared two ways with `helpers.covariance_distances` (|d cov_ij| / (sigma_i sigma_j), all 36 entries):

  * with the biased float64 numpy covariance of the ORACLE chain's outgoing particles (maps and reduction together), and
  * with that of the call's OWN outgoing particles (the reduction alone),

both at TOL_MOM[dtype]; the float64 forms both at 1e-9 as well, the bound of `test_fused_covariance_switch`.

The lattices couple the planes (tests/test_gpu_trace.py: `mixed_desc`, `coupled_desc`) and the incoming beam is correlated
in all 15 slots (`correlated_particles`).  A `Segment.track` call has one point, its end, so the condition on the inputs --
asserted from the oracle alone in tests/test_covariance_check_host.py -- is that every off-diagonal slot has
|correlation| >= 0.1 AT THE END, in every sample of every case with a spread (n > 1): the lattices are chosen for it
(TRACK_LATTICE_SEED, `conditioned_coupled_desc`).  A swapped, dropped or mis-scaled slot is then a thousand tolerances
away from passing, in whichever sample it happens.

Which kernel a call takes is decided by `plan_track` (lynx_hip.hip) from the shapes and the knobs; the arithmetic below is
for 256 CUs (4 * cus = 1024 workgroups is the small-job threshold).  A case that must reach the structured step loop
insists with LYNX_TRACK_UNITS=2, which is an error if the plan says otherwise -- a different CU count is noticed there.
"""

import functools

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import biased_covariance, correlations, covariance_distances, make_lattice, tri_slot
from .test_gpu_parity import TOL_MOM
from .test_gpu_trace import correlated_particles, coupled_desc, mixed_desc

pytestmark = pytest.mark.gpu

TOL_F64_REDUCTION = 1e-9  # test_fused_covariance_switch's
SHAPES = [(3,), (2, 2)]
TILE_EDGES = [1, 63, 64, 255, 256, 257, 1000, 2049]  # a wave; 256 u particles per workgroup tile, u = 1: 1, 2, 4, 9 tiles
# B ceil(N / (256 u)) >= 4 * 256 for u = 2 (114 * 17) AND u = 4 (114 * 9): the plan keeps two / four particles per lane
# instead of falling back to one (the loop under "small jobs" in plan_track); 114 * 8193 * 6 = 5.6e6 oracle steps a chain
BIG_SHAPE, BIG_N = (114,), 8193
# the covariance entries of the property-set record (slots 7, 8, 13, 18, 19, 22, 25, 27: test_fused_moments_equal_separate_pass)
HAVE_IJ = [(0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (3, 3), (4, 4), (5, 5)]
HAVE = [tri_slot(i, j) for i, j in HAVE_IJ]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


# `mixed_desc` per batch shape for the track cases: with these seeds every off-diagonal slot has |correlation| >= 0.1 at the
# END of the lattice in EVERY sample, for every n of TILE_EDGES with a spread (searched over seeds 0 .. 59 with the oracle;
# seed 21, the trace tests', leaves samples with a slot near 0 at the end)
TRACK_LATTICE_SEED = {(3,): 3, (2, 2): 25}
POOL = 8  # samples drawn per sample kept, for the batches of the six-element lattice


@functools.lru_cache(maxsize=None)
def conditioned_coupled_desc(shape):
    """
    `coupled_desc` for a batch in which EVERY sample meets the condition at the end: of random samples about one in four
    does (some slot of 15 is near 0 at any one point), so POOL times as many are drawn, a probe beam of 1024 correlated
    particles is tracked through them with the oracle (POOL * B * 1024 * 6 steps: 5.6e6 for B = 114), and the B samples
    whose smallest |correlation| at the end is largest are kept, in the order they were drawn.
    """
    B = int(np.prod(shape))
    pool = coupled_desc((POOL * B,), np.random.default_rng(22))
    _, specs = make_lattice(pool, np.float64)
    probe = correlated_particles((POOL * B,), 1024, seed=1, dtype=np.float64)
    end = o.segment_track(specs, o.particle_beam(probe, np.full(POOL * B, 1e8), np.float64), np.float64, kick="product")
    keep = np.sort(np.argsort(-correlations(end["particles"]).min(axis=-1), kind="stable")[:B])
    return [(kind, {k: np.asarray(v)[keep].reshape(*shape, *np.shape(v)[1:]) for k, v in kw.items()}) for kind, kw in pool]


def track_desc(lattice, shape):
    """"mixed": `mixed_desc` without the dead cavity, its two active BPMs kept; "coupled": the six elements, no BPM."""
    if lattice == "mixed":
        return mixed_desc(shape, np.random.default_rng(TRACK_LATTICE_SEED[shape]))
    return conditioned_coupled_desc(shape)


@functools.lru_cache(maxsize=None)
def track_case(dtype, shape, n, lattice):
    """(desc, P, energy, outgoing particles of the oracle's chain): computed once per case, shared, never written to."""
    desc = track_desc(lattice, shape)
    P = correlated_particles(shape, n, seed=7 + n, dtype=dtype)
    energy = np.full(shape, 1e8, dtype=dtype)
    _, specs = make_lattice(desc, dtype)
    ref = o.segment_track(specs, o.particle_beam(P, energy, dtype), dtype, kick="product")  # (_particle_case's chain)
    for a in (P, energy, ref["particles"]):
        a.setflags(write=False)
    return desc, P, energy, ref["particles"]


@functools.lru_cache(maxsize=None)
def shared_case(dtype):
    """One incoming beam of 2049 particles for a batch of 5 lattices: (desc, the one beam, energy, the oracle's outgoing particles)."""
    shape, n = (5,), 2049
    desc = track_desc("coupled", shape)
    one = correlated_particles((1,), n, seed=11, dtype=dtype)
    energy = np.full(shape, 1e8, dtype=dtype)
    _, specs = make_lattice(desc, dtype)
    P = np.ascontiguousarray(np.broadcast_to(one, (*shape, n, 7)))
    ref = o.segment_track(specs, o.particle_beam(P, energy, dtype), dtype, kick="product")
    return desc, one, energy, ref["particles"]


def fused(lx, segment, beam):
    lx.config.fused_covariance = True
    try:
        return segment.track(beam)
    finally:
        lx.config.fused_covariance = False


def assert_whole_covariance(out, ref_particles, dtype, what):
    """Both comparisons of the module docstring for one tracked (or host-made) beam; returns the two worst distances."""
    dtype = np.dtype(dtype).type
    cov = out.covariance()
    rec = out.moment_record(covariance=True)
    assert np.all(rec[..., 34] == 1.0), what
    for i in range(6):  # covariance() is the record's triangle, mirrored
        for j in range(6):
            assert np.array_equal(cov[..., i, j], rec[..., tri_slot(i, j)], equal_nan=True), (what, i, j)
    assert np.all(rec[..., 35] == ref_particles.shape[-2]), what
    assert not np.isnan(cov[~np.isnan(biased_covariance(ref_particles))]).any(), what
    own = np.asarray(out.particles)
    d_ref, at_ref = covariance_distances(cov, ref_particles)
    d_own, at_own = covariance_distances(cov, own)
    print(f"{what}: worst covariance distance {d_ref:.2e} at {at_ref} (oracle chain), {d_own:.2e} at {at_own} (own particles)")
    assert d_ref <= TOL_MOM[dtype], (what, "oracle chain", d_ref, at_ref)
    assert d_own <= TOL_MOM[dtype], (what, "own particles", d_own, at_own)
    if dtype == np.float64:
        assert d_ref <= TOL_F64_REDUCTION, (what, "oracle chain, float64", d_ref, at_ref)
        assert d_own <= TOL_F64_REDUCTION, (what, "own particles, float64", d_own, at_own)
    means = np.abs(rec[..., :6] - own[..., :6].astype(np.float64).mean(axis=-2))
    sig = np.sqrt(np.einsum("...ii->...i", biased_covariance(own)))
    assert np.all(means <= TOL_MOM[dtype] * (np.abs(rec[..., :6]) + sig)), (what, "means")
    return d_ref, d_own


# ---------------------------------------------------------------------------------------------
# (a) config.fused_covariance = True: the epilogue of the tracking kernel
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", TILE_EDGES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_covariance_at_tile_edges(lx, dtype, shape, n):
    """
    Default knobs.  B ceil(N / 256) < 1024 at these shapes: one particle per lane, and the two active BPMs keep the call
    in the dense step loop.  float64: `launch_direct_m<double, 1, true>`, U = 1, per-particle accesses; float32:
    `launch_direct_m<float, 3, true>`, U = 1 (tiles per workgroup x U <= 32: float32 lane sums).
    """
    desc, P, energy, ref = track_case(dtype, shape, n, "mixed")
    elements, _ = make_lattice(desc, dtype, lx)
    out = fused(lx, lx.Segment(elements), lx.ParticleBeam(P, energy, dtype=dtype))
    assert_whole_covariance(out, ref, dtype, f"fused {np.dtype(dtype).name} {shape} n={n}")


SMALL_FORMS = [
    # float32 partial sums per iteration instead of lane sums: launch_direct_m<float, 2, true>, U = 1
    (np.float32, {"LYNX_MOM": "2"}),
    # float32 lane sums, asked for: launch_direct_m<float, 3, true>, U = 1 (what the default plan takes here as well)
    (np.float32, {"LYNX_MOM": "3"}),
    # the switches of the structured loop and its pair kernel must change nothing here: BPMs observe, U = 1
    (np.float32, {"LYNX_TRACK_UNITS": "0"}), (np.float32, {"LYNX_UNIT_PAIRS": "0"}),
    # asked for more particles per lane than the job has workgroups for: the plan falls back to U = 1 all the same
    (np.float32, {"LYNX_UNROLL": "4"}), (np.float64, {"LYNX_UNROLL": "2"}),
]


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("dtype,env", SMALL_FORMS, ids=[f"{np.dtype(d).name}-{'-'.join(f'{k}={v}' for k, v in e.items())}" for d, e in SMALL_FORMS])
def test_fused_covariance_forms_of_a_small_job(lx, monkeypatch, dtype, env, n):
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    shape = (2, 2)
    desc, P, energy, ref = track_case(dtype, shape, n, "mixed")
    elements, _ = make_lattice(desc, dtype, lx)
    out = fused(lx, lx.Segment(elements), lx.ParticleBeam(P, energy, dtype=dtype))
    assert_whole_covariance(out, ref, dtype, f"fused {np.dtype(dtype).name} {shape} n={n} {env}")


BIG_FORMS = [
    # S = 3 steps ([drift .. solenoid] run, cavity, drift), two particles per lane, run and cavity merged, 17 tiles in 9
    # workgroups of 2: 2 * 2 <= 32 -> lane sums: launch_units_inst<3, true, 1> (full_cov keeps it out of the pair kernel)
    (np.float32, {"LYNX_TRACK_UNITS": "2"}),
    (np.float32, {"LYNX_TRACK_UNITS": "1"}),  # (the default spelled out: the same plan without the insistence)
    # ... partial sums per iteration: launch_units_inst<2, true, 1>
    (np.float32, {"LYNX_TRACK_UNITS": "2", "LYNX_MOM": "2"}),
    # four particles per lane, two pairs: 114 * 9 >= 1024 keeps U = 4: launch_units_inst<3, true, 2> and <2, true, 2>
    (np.float32, {"LYNX_TRACK_UNITS": "2", "LYNX_UNROLL": "4", "LYNX_MOM": "3"}),
    (np.float32, {"LYNX_TRACK_UNITS": "2", "LYNX_UNROLL": "4", "LYNX_MOM": "2"}),
    # the pair kernel switched off / on: with the whole covariance no call takes it (track_particles_t: `!p.full_cov`)
    (np.float32, {"LYNX_TRACK_UNITS": "2", "LYNX_UNIT_PAIRS": "0"}), (np.float32, {"LYNX_UNIT_PAIRS": "1"}),
    # the dense step loop with U = 2, 4 and 1: launch_direct_m<float, 3, true> (U = 2, 1), <float, 2 | 3, true> (U = 4)
    (np.float32, {"LYNX_TRACK_UNITS": "0"}), (np.float32, {"LYNX_TRACK_UNITS": "0", "LYNX_UNROLL": "4", "LYNX_MOM": "2"}),
    (np.float32, {"LYNX_TRACK_UNITS": "0", "LYNX_UNROLL": "4", "LYNX_MOM": "3"}), (np.float32, {"LYNX_UNROLL": "1"}),
    (np.float32, {"LYNX_UNROLL": "2", "LYNX_MOM": "2", "LYNX_TRACK_UNITS": "0"}),
    # float64, N >= 1024 and 114 * 17 >= 1024: U = 2 survives the small-job fallback, so the wave-tile form does:
    # launch_direct_inst<double, 1, true, 2, true>
    (np.float64, {}),
    (np.float64, {"LYNX_UNROLL": "2"}),
    # ... one particle per lane, per-particle accesses: launch_direct_inst<double, 1, true, 1, false>
    (np.float64, {"LYNX_UNROLL": "1"}),
    (np.float64, {"LYNX_TRACK_UNITS": "0"}), (np.float64, {"LYNX_UNIT_PAIRS": "0"}),  # (float32 switches: nothing changes)
]


@pytest.mark.parametrize("dtype,env", BIG_FORMS, ids=[f"{np.dtype(d).name}-{'-'.join(f'{k}={v}' for k, v in e.items()) or 'default'}" for d, e in BIG_FORMS])
def test_fused_covariance_of_every_epilogue_form(lx, monkeypatch, dtype, env):
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    desc, P, energy, ref = track_case(dtype, BIG_SHAPE, BIG_N, "coupled")
    elements, _ = make_lattice(desc, dtype, lx)
    out = fused(lx, lx.Segment(elements), lx.ParticleBeam(P, energy, dtype=dtype))
    assert_whole_covariance(out, ref, dtype, f"fused {np.dtype(dtype).name} {BIG_SHAPE} n={BIG_N} {env}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_covariance_of_a_shared_beam_repeats_bit_for_bit(lx, dtype):
    """Three calls with one incoming beam shared by the batch (the fuzz file's pattern "three"): the same bits thrice."""
    desc, one, energy, ref = shared_case(dtype)
    shape = energy.shape
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    beam = lx.ParticleBeam(one, energy[:1], dtype=dtype).broadcast(shape)
    assert beam.is_shared
    outs = [fused(lx, segment, beam) for _ in range(3)]
    assert_whole_covariance(outs[0], ref, dtype, f"fused shared {np.dtype(dtype).name}")
    first = np.asarray(outs[0].particles)
    for k in (1, 2):
        assert np.array_equal(np.asarray(outs[k].particles), first), k
        assert np.array_equal(outs[k].moment_record(), outs[0].moment_record()), k
        assert np.array_equal(outs[k].covariance(), outs[0].covariance()), k


# ---------------------------------------------------------------------------------------------
# (b) config.fused_covariance = False: the property-set record, and the covariance pass behind covariance()
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", TILE_EDGES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_covariance_pass_behind_a_tracked_beam(lx, dtype, shape, n):
    """`lynx_moments(..., covariance=1)`: S = 0, no stores, per-particle loads (plan_track: a read-only pass)."""
    assert lx.config.fused_covariance is False
    desc, P, energy, ref = track_case(dtype, shape, n, "mixed")
    elements, _ = make_lattice(desc, dtype, lx)
    out = lx.Segment(elements).track(lx.ParticleBeam(P, energy, dtype=dtype))
    compact = out.moment_record().copy()
    assert np.all(compact[..., 34] == 0.0) and not np.isnan(compact[..., :7]).any() and not np.isnan(compact[..., HAVE]).any()
    assert np.isnan(np.delete(compact[..., 7:28], [h - 7 for h in HAVE], axis=-1)).all()  # the 13 other slots
    assert_whole_covariance(out, ref, dtype, f"pass {np.dtype(dtype).name} {shape} n={n}")
    # the 14 numbers both records hold: to 1e-6 (test_fused_moments_equal_separate_pass's), in the moments' own scales
    full = out.moment_record()
    sig = np.sqrt(np.stack([full[..., tri_slot(c, c)] for c in range(6)], axis=-1))
    assert np.all(np.abs(full[..., :6] - compact[..., :6]) <= 1e-6 * (np.abs(full[..., :6]) + sig))
    for i, j in HAVE_IJ:
        assert np.all(np.abs(full[..., tri_slot(i, j)] - compact[..., tri_slot(i, j)]) <= 1e-6 * sig[..., i] * sig[..., j]), (i, j)


@pytest.mark.parametrize("n", TILE_EDGES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_covariance_pass_of_a_beam_from_host_particles(lx, dtype, shape, n):
    """Nothing tracked: the pass reads what the host wrote; the reference is numpy on the same array."""
    _, P, energy, _ = track_case(dtype, shape, n, "mixed")
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    assert_whole_covariance(beam, P, dtype, f"pass, host particles {np.dtype(dtype).name} {shape} n={n}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_covariance_pass_of_many_workgroups_per_sample(lx, dtype):
    """The big shape: several workgroups per sample and a reduction of their records, behind the units / wave-tile kernel."""
    desc, P, energy, ref = track_case(dtype, BIG_SHAPE, BIG_N, "coupled")
    elements, _ = make_lattice(desc, dtype, lx)
    out = lx.Segment(elements).track(lx.ParticleBeam(P, energy, dtype=dtype))
    assert np.all(out.moment_record()[..., 34] == 0.0)
    assert_whole_covariance(out, ref, dtype, f"pass {np.dtype(dtype).name} {BIG_SHAPE} n={BIG_N}")
