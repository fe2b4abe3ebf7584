"""
Parity of the HIP path (through the C ABI, via the lynx_amd Python layer) with the oracle.

Tolerances (north_star: 1e-6 rel fp64 / 1e-4 rel fp32 on beam moments; "bit-exact for
indexing"): maps and particles are compared relative to the scale of the quantity,
fp32 <= 1e-4 (observed ~1e-6), fp64 <= 1e-10 (observed ~1e-14).  Index placement is checked
exactly through maps whose every entry is distinct.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import (MOMENT_KEYS, assert_parameter_beam, make_lattice, map_err, moment_distances, random_samples, rel_err,
                      singular_entry_voltage)

pytestmark = pytest.mark.gpu

TOL_MAP = {np.float32: 5e-5, np.float64: 1e-11}
TOL_P = {np.float32: 1e-4, np.float64: 1e-10}
TOL_MOM = {np.float32: 1e-4, np.float64: 1e-6}


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


def _particle_case(lx, desc, dtype, batch_shape, n, seed, energy=1e8, sigma=None, ddof=1):
    dtype = np.dtype(dtype).type
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles(batch_shape, n, seed=seed, dtype=dtype,
                             sigma=sigma or [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    e = np.full(batch_shape, energy, dtype=dtype)
    out = lx.Segment(elements).track(lx.ParticleBeam(P, e, dtype=dtype))
    # float32 behind an active cavity: the chain with the kernels' form of the kick (see _assert_moments)
    ref = o.segment_track(specs, o.particle_beam(P, e, dtype), dtype, kick="product")
    if dtype == np.float32 and any(kind == "cavity" for kind, _ in desc):
        # ... and the float64 chain next to it, for the moments the kick decides
        up = lambda v: np.asarray(np.asarray(v, dtype=np.float32), dtype=np.float64) if isinstance(v, (np.ndarray, list, float)) else v  # noqa: E731
        _, specs64 = make_lattice([(kind, {k: up(v) for k, v in kw.items()}) for kind, kw in desc], np.float64)
        ref["float64_chain"] = o.segment_track(specs64, o.particle_beam(P.astype(np.float64), e.astype(np.float64), np.float64), np.float64)
    return out, ref


def _assert_particles(out, ref, dtype):
    got = np.asarray(out.particles)
    assert got.shape == ref["particles"].shape
    for c in range(7):
        err = rel_err(got[..., c], ref["particles"][..., c])
        assert err < TOL_P[dtype], (c, err)
    assert rel_err(out.energy, ref["energy"]) < 1e-6


KICK_MOMENTS = ("mu_s", "mu_p", "sigma_s", "sigma_p")  # what the cavity kick decides
TOL_KICK_F64 = 1e-5  # float32 product against the float64 chain in those (measured: 1e-8 .. 3e-6)


def _assert_moments(out, ref, dtype):
    """
    Every beam moment within north_star's tolerance of the oracle's chain.  float32 lattices with an active cavity:
    `ref` is the chain with the kernels' form of the kick (o.segment_track(..., kick="product")) -- the reference
    subtracts two cosines (cavity.py:150-160) that agree to four or five digits on a short bunch, and its float32 mean
    of delta carries that cosine's rounding as a whole (2e-4 .. 5e-4 of |mu_p| + sigma_p on BASELINE config 5's beam),
    the kernels form cos(phi)(cos d - 1) - sin(phi) sin d (device_cavity_kick) -- and, when `_particle_case` hands the
    float64 chain over too, the moments the kick decides are also held within TOL_KICK_F64 of that chain.
    """
    d = moment_distances(out, o.beam_moments(ref, ddof=1))
    assert max(d.values()) <= TOL_MOM[dtype], d
    if "float64_chain" in ref:
        d64 = moment_distances(out, o.beam_moments(ref["float64_chain"], ddof=1))
        assert max(d64[key] for key in KICK_MOMENTS) <= TOL_KICK_F64, d64


# ---------------------------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------------------------

ELEMENT_CASES = [
    ("drift", dict(length=[0.3, 1.0, 0.0])),
    ("hcor", dict(length=[0.3, 0.1, 0.2], angle=[1e-4, 0.0, -2e-3])),
    ("vcor", dict(length=[0.3, 0.1, 0.2], angle=[3.142e-3, 0.0, -2e-3])),
    ("quadrupole", dict(length=[0.2, 0.1, 0.3], k1=[4.2, -4.2, 0.0])),
    ("quadrupole", dict(length=[0.5, 0.5, 0.5], k1=[1.0, 1.0, 1.0], tilt=[np.pi / 4, np.pi / 2, 0.0])),
    ("quadrupole", dict(length=[1.0, 1.0, 1.0], k1=[1.0, -2.0, 3.0],
                        misalignment=[[0.1, 0.1], [0.0, 0.0], [-1e-3, 2e-3]], tilt=[0.0, 0.3, 0.0])),
    ("dipole", dict(length=[0.5, 0.5, 1.0], angle=[0.1, 0.2, 0.0])),
    ("dipole", dict(length=[0.5, 0.0, 1.0], angle=[0.1, 0.01, -0.3], e1=[0.05, 0.0, 0.1], e2=[0.02, 0.0, -0.1],
                    tilt=[0.0, 0.2, np.pi / 2], fringe_integral=[0.3, 0.0, 0.5], gap=[0.02, 0.0, 0.03])),
    ("dipole", dict(length=[0.0, 0.0, 0.0], angle=[0.1, 0.01, -0.3])),
    ("rbend", dict(length=[0.5, 0.4, 1.0], angle=[0.1, 0.01, -0.3], e1=[0.0, 0.01, 0.0],
                   fringe_integral=[0.3, 0.0, 0.5], fringe_integral_exit=[0.1, 0.2, 0.5], gap=[0.02, 0.0, 0.03])),
    ("cavity", dict(length=[1.0377, 3.0441, 1.0], voltage=[0.01815975e9, 48198468.0, 1e6],
                    phase=[0.0, 30.0, -10.0], frequency=[1.3e9, 2.856e9, 1.3e9])),
    ("cavity", dict(length=[1.0, 1.0, 1.0], voltage=[0.0, 0.0, 0.0], phase=[0.0, 1.0, 2.0],
                    frequency=[1.3e9, 1.3e9, 1.3e9])),
    ("marker", dict()),
    ("bpm", dict()),
    ("solenoid", dict(length=[0.5, 0.3, 0.0], k=[2.0, 0.0, 1.0])),
    ("solenoid", dict(length=[0.5, 0.3, 0.2], k=[2.0, -1.5, 1.0], misalignment=[[1e-3, -2e-3], [0.0, 0.0], [1e-4, 0.0]])),
    ("undulator", dict(length=[0.25, 1.0, 0.0])),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", range(len(ELEMENT_CASES)))
def test_element_transfer_map(lx, case, dtype):
    kind, kw = ELEMENT_CASES[case]
    elements, specs = make_lattice([(kind, kw)], dtype, lx)
    energy = np.array([1e8, 6e6, 1.0732e8], dtype=dtype)
    got = elements[0].transfer_map(energy)
    ref = o.element_transfer_map(specs[0], energy, dtype)
    assert got.shape == (3, 7, 7)
    tol = TOL_MAP[dtype] * (10 if kind in ("dipole", "rbend", "cavity") else 1)
    assert map_err(got, ref) < tol, (kind, map_err(got, ref))


def test_custom_transfer_map_index_placement_is_exact(lx):
    """Every one of the 49 entries distinct: catches any row/column/transposition mix-up."""
    tm = (np.arange(49, dtype=np.float64).reshape(1, 7, 7) + 1) / 64.0
    el = lx.CustomTransferMap(tm, dtype=np.float64)
    assert np.array_equal(el.transfer_map(np.array([1e8])), tm)
    seg = lx.Segment([el])
    assert np.array_equal(seg.transfer_map(np.array([1e8])), tm)  # tm @ I is exact
    P = np.zeros((1, 7, 7))
    P[0] = np.eye(7)  # unit vectors: row n of the output is column n of tm
    out = seg.track(lx.ParticleBeam(P, np.array([1e8]), dtype=np.float64))
    assert np.array_equal(np.asarray(out.particles)[0], tm[0].T)


def test_kat3_custom_map_broadcast(lx):
    """reference tests/test_vectorized.py:371-392"""
    tm = np.array([[[1.0, 4.0e-02, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 1.0e-05], [0, 0, 1.0, 4.0e-02, 0, 0, 0],
                    [0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 0, 1.0, -4.6422e-07, 0], [0, 0, 0, 0, 0, 1.0, 0],
                    [0, 0, 0, 0, 0, 0, 1.0]]], dtype=np.float32)
    element = lx.CustomTransferMap(length=np.array([0.4]), transfer_map=tm)
    b = element.broadcast((3, 10))
    assert b.length.shape == (3, 10) and b._transfer_map.shape == (3, 10, 7, 7)
    got = b.transfer_map(np.full((3, 10), 1e8, dtype=np.float32))
    for i in range(3):
        for j in range(10):
            assert np.all(got[i, j] == tm[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kat2_composition_of_1051_maps(lx, dtype):
    """docs/examples/optimize_speed.ipynb:47-67, printed result :270 (fp32 torch, 5 digits)."""
    cell = [("quadrupole", dict(length=[0.1], k1=[4.2])), ("drift", dict(length=[0.2])),
            ("quadrupole", dict(length=[0.1], k1=[-4.2])), ("drift", dict(length=[0.2])), ("marker", dict()),
            ("quadrupole", dict(length=[0.1], k1=[0.0])), ("drift", dict(length=[0.2]))]
    desc = [("drift", dict(length=[0.3]))] + cell * 150
    elements, specs = make_lattice(desc, dtype, lx)
    energy = np.array([107315902.44394557], dtype=dtype)
    seg = lx.Segment(elements)
    got = seg.transfer_map(energy)
    ref = o.segment_transfer_map(specs, energy, dtype)
    assert map_err(got, ref) < (2e-4 if dtype == np.float32 else 1e-10)
    printed = {(0, 0): 1.3122, (0, 1): -3.4577, (1, 0): 0.18828, (1, 1): 0.26594, (2, 2): 0.30360,
               (2, 3): -3.2559, (3, 2): 0.18828, (3, 3): 1.2746, (4, 5): -3.0678e-3}
    for (i, j), v in printed.items():
        assert abs(got[0, i, j] - v) < 3e-4 * max(1.0, abs(v)) if (i, j) != (4, 5) else abs(got[0, i, j] - v) < 1e-6
    assert abs(float(seg.length[0]) - 135.2991) < 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_segment_transfer_map_batched_fodo(lx, dtype):
    B = 5
    scale = np.linspace(0.5, 1.5, B)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(32):
        desc += [("quadrupole", dict(length=f(0.2), k1=4.2 * scale)), ("drift", dict(length=f(0.5))),
                 ("quadrupole", dict(length=f(0.2), k1=-4.2 * scale)), ("drift", dict(length=f(0.5)))]
    elements, specs = make_lattice(desc, dtype, lx)
    energy = np.full(B, 1e8, dtype=dtype)
    got = lx.Segment(elements).transfer_map(energy)
    ref = o.segment_transfer_map(specs, energy, dtype)
    assert map_err(got, ref) < (5e-5 if dtype == np.float32 else 1e-10)


# ---------------------------------------------------------------------------------------------
# particles
# ---------------------------------------------------------------------------------------------

ARES = [("bpm", {}), ("drift", dict(length=[1.0])), ("bpm", {}), ("drift", dict(length=[1.0])),
        ("vcor", dict(length=[0.3], angle=[3.142e-3])), ("drift", dict(length=[0.2])),
        ("hcor", dict(length=[0.3], angle=[1e-4])), ("drift", dict(length=[7.0])),
        ("hcor", dict(length=[0.3], angle=[-1e-4])), ("drift", dict(length=[0.05])), ("bpm", {})]


@pytest.mark.parametrize("n", [1, 3, 255, 1000, 100_000])
def test_c2_ares_segment_particles(lx, n):
    """BASELINE config 2: the 11-element README segment, fp32, B = 1 (and ragged N)."""
    out, ref = _particle_case(lx, ARES, np.float32, (1,), n, seed=0,
                              sigma=[175e-9, 2e-7, 175e-9, 2e-7, 1e-6, 1e-6])
    _assert_particles(out, ref, np.float32)
    if n >= 1000:
        _assert_moments(out, ref, np.float32)


@pytest.mark.parametrize("dtype,n", [(np.float32, 100_000), (np.float64, 300_001), (np.float64, 1_000_000)])
def test_the_two_forms_of_the_moment_reduction_agree(lx, dtype, n, monkeypatch):
    """
    Beams of few samples with hundreds to thousands of workgroup records (BASELINE configs 2 and 3): by default ONE
    launch adds them up in two levels -- groups of rows, then the workgroup that draws the sample's last ticket adds the
    group records in group order (k_reduce_moments_ticket).  The same records through two launches (a level, then the
    final one: LYNX_REDUCE_TICKET=0): a different association of the same float64 sums -- the records agree to rounding,
    and with the oracle; and the default form gives the same bits every time it runs (the last arrival decides who adds,
    not in which order).
    """
    sigma = [175e-9, 2e-7, 175e-9, 2e-7, 1e-6, 1e-6]
    out, ref = _particle_case(lx, ARES, dtype, (1,), n, seed=5, sigma=sigma)
    ticket = out.moment_record().copy()
    _assert_moments(out, ref, dtype)
    for _ in range(3):
        again, _ = _particle_case(lx, ARES, dtype, (1,), n, seed=5, sigma=sigma)
        assert np.array_equal(again.moment_record(), ticket, equal_nan=True)
    have = ~np.isnan(ticket)
    for knob in ({"LYNX_REDUCE_TICKET": "0"},):
        for key, value in knob.items():
            monkeypatch.setenv(key, value)
        other, _ = _particle_case(lx, ARES, dtype, (1,), n, seed=5, sigma=sigma)
        rec = other.moment_record()
        assert np.array_equal(np.isnan(ticket), np.isnan(rec)), knob
        assert np.allclose(ticket[have], rec[have], rtol=1e-11, atol=1e-300), knob
        for key in knob:
            monkeypatch.delenv(key)


@pytest.mark.parametrize("dtype,n", [(np.float32, 4096), (np.float32, 4099), (np.float64, 2048), (np.float64, 2047)])
def test_fodo_scan_particles(lx, dtype, n):
    """BASELINE configs 3/4 in small: 128-element FODO, k1 scan over the batch; odd N takes
    the unaligned (scalar-access) kernel variant."""
    B = 6
    scale = 0.5 + np.arange(B) / (B - 1)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(32):
        desc += [("quadrupole", dict(length=f(0.2), k1=4.2 * scale)), ("drift", dict(length=f(0.5))),
                 ("quadrupole", dict(length=f(0.2), k1=-4.2 * scale)), ("drift", dict(length=f(0.5)))]
    out, ref = _particle_case(lx, desc, dtype, (B,), n, seed=2)
    got = np.asarray(out.particles)
    tol = 1e-4 if dtype == np.float32 else 1e-9
    _assert_moments(out, ref, dtype)
    for c in range(7):
        assert rel_err(got[..., c], ref["particles"][..., c]) < tol, c
    # and exactly consistent with the GPU's own composed map (isolates the streaming kernel)
    elements, _ = make_lattice(desc, dtype, lx)
    tm = lx.Segment(elements).transfer_map(np.full(B, 1e8, dtype=dtype))
    P = o.gaussian_particles((B,), n, seed=2, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    via_map = np.matmul(P.astype(np.float64), np.swapaxes(tm.astype(np.float64), -1, -2))
    for c in range(7):
        assert rel_err(got[..., c], via_map[..., c]) < (2e-6 if dtype == np.float32 else 1e-14), c


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_multidim_batch_and_mixed_elements(lx, dtype):
    shape = (3, 2)
    rng = np.random.default_rng(5)
    f = lambda v: np.full(shape, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))),
            ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, shape), tilt=rng.uniform(-1, 1, shape),
                                misalignment=rng.normal(0, 1e-4, (*shape, 2)))),
            ("marker", {}),
            ("dipole", dict(length=f(0.5), angle=rng.uniform(-0.2, 0.2, shape), e1=f(0.05), e2=f(0.02),
                            fringe_integral=f(0.4), gap=f(0.02), tilt=f(0.1))),
            ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, shape))),
            ("rbend", dict(length=f(0.3), angle=f(0.05))),
            ("vcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, shape))),
            ("drift", dict(length=f(0.4)))]
    out, ref = _particle_case(lx, desc, dtype, shape, 3000, seed=11)
    assert np.asarray(out.particles).shape == (3, 2, 3000, 7)
    _assert_particles(out, ref, dtype)
    _assert_moments(out, ref, dtype)
    assert out.mu_x.shape == shape and out.sigma_p.shape == shape and out.energy.shape == shape


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_c5_cavity_lattice_particles(lx, dtype):
    """BASELINE config 5 in small: [Drift, misaligned Quad, Drift, Cavity] x 8, E_in = 6 MeV."""
    B = 4
    rng = np.random.default_rng(3)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(8):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                                 frequency=f(1.3e9)))]
    out, ref = _particle_case(lx, desc, dtype, (B,), 2500, seed=3, energy=6e6,
                              sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    got = np.asarray(out.particles)
    # delta goes through cos(phi + eps) - cos(phi): against the chain with the kernels' form of the kick (float32), at
    # the suite's tolerance like every other coordinate
    tol = {np.float32: [1e-4] * 6 + [1e-6], np.float64: [1e-9] * 7}[dtype]
    for c in range(7):
        assert rel_err(got[..., c], ref["particles"][..., c]) < tol[c], (c, rel_err(got[..., c], ref["particles"][..., c]))
    assert rel_err(out.energy, ref["energy"]) < 1e-6
    assert np.all(out.energy > 6e6)


def _fodo_scan(B, cells=32):
    scale = 0.5 + np.arange(B) / (B - 1)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(cells):
        desc += [("quadrupole", dict(length=f(0.2), k1=4.2 * scale)), ("drift", dict(length=f(0.5))),
                 ("quadrupole", dict(length=f(0.2), k1=-4.2 * scale)), ("drift", dict(length=f(0.5)))]
    return desc


def _moment_distance(out, m):
    """Largest deviation of the product's moments from the moments `m`, in units of the tolerance
    scale `_assert_moments` uses (sigma for means and sigmas, sigma_a sigma_b for the correlations)."""
    worst = 0.0
    for key in ("x", "xp", "y", "yp", "s", "p"):
        sig = m["sigma_" + key]
        worst = max(worst, float(np.max(np.abs(getattr(out, "mu_" + key) - m["mu_" + key]) / (np.abs(m["mu_" + key]) + sig))))
        if np.all(sig > 0):
            worst = max(worst, float(np.max(np.abs(getattr(out, "sigma_" + key) - sig) / sig)))
    for key, a, b in (("sigma_xxp", "sigma_x", "sigma_xp"), ("sigma_yyp", "sigma_y", "sigma_yp")):
        worst = max(worst, float(np.max(np.abs(getattr(out, key) - m[key]) / (m[a] * m[b]))))
    return worst


def test_c4_shape_moments_match_the_reference_chain(lx):
    """
    BASELINE config 4's shape (128-element FODO, k1 scan over the batch, 100 000 particles, float32):
    the beam MOMENTS against the float32 oracle, which composes left to right like the reference
    (segment.py:334-335), at north_star's 1e-4 -- and, for the record, their distance to the float64
    oracle on the same float32 inputs.  Measured on MI355X (this test prints it): 6e-6 from the
    float32 chain, 3.6e-5 from float64; the float32 chain itself is 3.5e-5 from float64 -- what is
    left is the rounding of the element maps (float32 sin / cos / sqrt arguments), not the order of
    the products: the build multiplies in float64.
    """
    B, N = 16, 100_000
    out, ref = _particle_case(lx, _fodo_scan(B), np.float32, (B,), N, seed=2)
    _assert_moments(out, ref, np.float32)
    _, specs64 = make_lattice(_fodo_scan(B), np.float64)
    P = o.gaussian_particles((B,), N, seed=2, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    ref64 = o.segment_track(specs64, o.particle_beam(P.astype(np.float64), np.full(B, 1e8), np.float64), np.float64)
    d32 = _moment_distance(out, o.beam_moments(ref, ddof=1))
    d64 = _moment_distance(out, o.beam_moments(ref64, ddof=1))
    print(f"C4 shape: moments {d32:.2e} from the float32 reference chain, {d64:.2e} from float64")
    assert d32 < 1e-4 and d64 < 2e-4
    # the particles themselves, relative to the scale of each coordinate
    got = np.asarray(out.particles)
    for c in range(7):
        assert rel_err(got[..., c], ref["particles"][..., c]) < 1e-4, c


def test_the_bench_plan_of_config_4_against_the_oracle(lx, record_property):
    """
    The kernel / launch combination `bench.py`'s headline number runs on, end to end against the oracle: FODO k1
    scan, float32, B = 320 (>= 256: lanes = samples build; not a multiple of 64: a cut wave of samples), N = 100 000
    (wave tiles with a cut last tile; B N >= 512 k: build on the second stream into the ring of step tables, host-side
    build wait, moment reduction on the side stream), two-tile workgroups, default environment, beam generated in HBM
    like the bench's.  THREE consecutive `track` calls, so that the builds of calls two and three run underneath the
    previous streaming kernel and every step-table slot is used.  Oracle: `o.segment_track` on the k1 values of
    samples {0, 63, 64, 255, 319} and three drawn per run (seed recorded) -- moments at north_star's 1e-4, particles of
    every one of them at 1e-4 of the coordinate's scale -- and the moments of ALL 320 samples at 1e-4 (the oracle takes
    them 64 at a time; the three calls' records are the same bits).  (segment.py:329-342, element.py:83-92.)
    """
    B, N = 320, 100_000
    dtype = np.float32
    desc = _fodo_scan(B)
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    beam = lx.ParticleBeam.synthetic((B,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=2, dtype=dtype)
    outs = [segment.track(beam) for _ in range(3)]
    P = np.asarray(beam.particles)
    pick, _ = random_samples(B, 3, always=(0, 63, 64, 255, 319), record=record_property)
    sub = [(kind, {k: np.asarray(v)[pick] for k, v in kw.items()}) for kind, kw in desc]
    _, specs = make_lattice(sub, dtype)
    e = np.full(len(pick), 1e8, dtype=dtype)
    ref = o.segment_track(specs, o.particle_beam(P[pick], e, dtype), dtype)
    m = o.beam_moments(ref, ddof=1)
    records = [np.asarray(out.moment_record()) for out in outs]
    tracked = np.asarray(outs[-1].particles)
    for call, out in enumerate(outs):
        for key in ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p"):
            sig = m["sigma" + key[2:]]
            got = np.asarray(getattr(out, key))[pick]
            assert np.all(np.abs(got - m[key]) <= 1e-4 * (np.abs(m[key]) + sig)), (call, key)
        for key in ("sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p"):
            assert np.allclose(np.asarray(getattr(out, key))[pick], m[key], rtol=1e-4, atol=0), (call, key)
        for key, a, b in (("sigma_xxp", "sigma_x", "sigma_xp"), ("sigma_yyp", "sigma_y", "sigma_yp")):
            assert np.all(np.abs(np.asarray(getattr(out, key))[pick] - m[key]) <= 1e-4 * m[a] * m[b]), (call, key)
        assert np.array_equal(records[call], records[0], equal_nan=True), call  # same input, same plan: bit for bit
    for c in range(7):
        assert rel_err(tracked[pick][..., c], ref["particles"][..., c]) < 1e-4, c
    assert np.array_equal(tracked, np.asarray(outs[0].particles))
    assert np.all(records[0][:, 35] == N)
    got = {key: np.asarray(getattr(outs[0], key)) for key in MOMENT_KEYS}
    for lo in range(0, B, 64):
        chunk = list(range(lo, min(lo + 64, B)))
        _, specs = make_lattice(_subset(desc, chunk), dtype)
        mc = o.beam_moments(o.segment_track(specs, o.particle_beam(P[chunk], np.full(len(chunk), 1e8, dtype=dtype), dtype), dtype), ddof=1)
        d = moment_distances({key: got[key][chunk] for key in MOMENT_KEYS}, mc)
        assert max(d.values()) <= 1e-4, (lo, d)


def test_config_4_at_its_full_size_is_exactly_linear_and_matches_the_oracle(lx, record_property):
    """
    BASELINE config 4 as the bench runs it -- 1024 samples x 100 000 particles x 128-element FODO, float32, beam made
    in HBM -- is too large to run through the oracle whole.  Two checks that do not depend on the size:
    (1) drifts and quadrupoles without misalignment have no affine column, so the lattice is LINEAR, and scaling a
    beam by 2 is exact in binary floating point: the beam with twice the sigmas (same seed) must come out exactly
    twice as large -- every particle of every sample bit for bit, the means times 2, the second moments times 4 --
    whatever the launch plan, tile order and reduction tree did on the way (element.py:83-92: P T^T).
    (2) against `o.segment_track` on their k1 values: the moments of ALL 1024 samples at north_star's 1e-4 (the
    oracle takes them 128 at a time) -- the linearity of (1) cannot see a sample tracked with its neighbour's k1 --
    and the particles of the two ends of the scan and three samples drawn per run (seed recorded) at 1e-4 of each
    coordinate's scale.
    """
    B, N = 1024, 100_000
    dtype = np.float32
    desc = _fodo_scan(B)
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    sigma = np.array([1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    beam = lx.ParticleBeam.synthetic((B,), N, sigma=sigma, energy=1e8, seed=2, dtype=dtype)
    twice = lx.ParticleBeam.synthetic((B,), N, sigma=2 * sigma, energy=1e8, seed=2, dtype=dtype)
    pick, _ = random_samples(B, 3, always=(0, 1023), record=record_property)
    P_all = np.asarray(beam.particles)
    P = P_all[pick]
    P2 = np.asarray(twice.particles)[pick]
    assert np.array_equal(P2[..., :6], 2 * P[..., :6]) and np.all(P2[..., 6] == 1)
    out, out2 = segment.track(beam), segment.track(twice)
    a, b = np.asarray(out.particles), np.asarray(out2.particles)
    assert np.array_equal(b[..., :6], 2 * a[..., :6]) and np.array_equal(b[..., 6], a[..., 6])
    for key in ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p"):
        assert np.array_equal(np.asarray(getattr(out2, key)), 2 * np.asarray(getattr(out, key))), key
    for key in ("sigma_xxp", "sigma_yyp"):
        assert np.array_equal(np.asarray(getattr(out2, key)), 4 * np.asarray(getattr(out, key))), key
    assert np.all(np.asarray(out.moment_record())[:, 35] == N)
    sub = [(kind, {k: np.asarray(v)[pick] for k, v in kw.items()}) for kind, kw in desc]
    _, specs = make_lattice(sub, dtype)
    ref = o.segment_track(specs, o.particle_beam(P, np.full(len(pick), 1e8, dtype=dtype), dtype), dtype)
    for c in range(7):
        assert rel_err(a[pick][..., c], ref["particles"][..., c]) < 1e-4, c
    got = {key: np.asarray(getattr(out, key)) for key in MOMENT_KEYS}
    worst = 0.0
    for lo in range(0, B, 128):
        chunk = list(range(lo, lo + 128))
        _, specs = make_lattice(_subset(desc, chunk), dtype)
        m = o.beam_moments(o.segment_track(specs, o.particle_beam(P_all[chunk], np.full(128, 1e8, dtype=dtype), dtype), dtype), ddof=1)
        d = moment_distances({key: got[key][chunk] for key in MOMENT_KEYS}, m)
        assert max(d.values()) <= 1e-4, (lo, d)
        worst = max(worst, max(d.values()))
    print(f"config 4 at its full size: all 1024 samples' moments within {worst:.1e} of the float32 oracle")


def test_config_5_at_its_full_size_structured_equals_dense_and_matches_the_oracle_on_three_samples(lx, monkeypatch):
    """
    BASELINE config 5 at its full size -- 4096 environments x 10 000 particles x [Drift, misaligned Quadrupole,
    Drift, Cavity] x 8, float32 -- through the structured step loop (k_track_units, insisted on) and through the dense
    one: every particle, every energy and every moment record of the two bit for bit (lynx_units.hpp: skipped terms
    are exact zeros); and environments 0, 2047 and 4095 against `o.segment_track`: moments at north_star's 1e-4,
    particle coordinates at 1e-4 of their scale, delta behind eight cavities included, against the chain with the
    kernels' form of the kick (o.segment_track(..., kick="product"); with the reference's form delta was 6e-5 .. 1.6e-4 away: the
    float32 cosines of eight kicks, the float32 oracle itself is 4e-5 .. 1e-4 away from the float64 one there:
    scripts/gpu/r3_c5_particles.py).  (cavity.py:97-246, quadrupole.py:66-80.)
    """
    B, N = 4096, 10_000
    dtype = np.float32
    rng = np.random.default_rng(4)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(8):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    # (sigma_s = 1e-4 as in test_c5_shape_moments: with the bench's 1e-5 the float32 cosines of eight kicks are worth
    # more than 1e-4 of sigma_s in the oracle as in the kernel)
    beam = lx.ParticleBeam.synthetic((B,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3], energy=6e6, seed=2, dtype=dtype)
    outs = {}
    for units in ("2", "0"):
        monkeypatch.setenv("LYNX_TRACK_UNITS", units)
        out = segment.track(beam)
        outs[units] = (np.asarray(out.particles), np.asarray(out.energy), np.asarray(out.moment_record()), out)
    for k in range(3):
        assert _same_bits(outs["2"][k], outs["0"][k]), k
    out = outs["2"][3]
    pick = [0, 2047, 4095]
    P = np.asarray(beam.particles)[pick]
    sub = [(kind, {k: np.asarray(v)[pick] for k, v in kw.items()}) for kind, kw in desc]
    _, specs = make_lattice(sub, dtype)
    ref = o.segment_track(specs, o.particle_beam(P, np.full(len(pick), 6e6, dtype=dtype), dtype), dtype, kick="product")
    m = o.beam_moments(ref, ddof=1)
    got = outs["2"][0][pick]
    for c in range(7):
        assert rel_err(got[..., c], ref["particles"][..., c]) < 1e-4, c
    assert rel_err(outs["2"][1][pick], ref["energy"]) < 1e-6
    for key in ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p"):
        sig = m["sigma" + key[2:]]
        assert np.all(np.abs(np.asarray(getattr(out, key))[pick] - m[key]) <= 1e-4 * (np.abs(m[key]) + sig)), key
    for key in ("sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p"):
        assert np.allclose(np.asarray(getattr(out, key))[pick], m[key], rtol=1e-4, atol=0), key
    assert np.all(outs["2"][2][:, 35] == N)


def _bench_workload(lx, name, dtype):
    """Lattice (description and product `Segment`) and incoming beam of `bench.py --workload <name>`, exactly as the
    bench makes them on one GPU: `bench.describe`, `bench.BEAM_SIGMA`, seed 2, the lattice's seed 3."""
    import bench

    batch, particles, cells, _, _ = bench.WORKLOADS[name]
    ids = np.arange(batch)
    desc = bench.describe(name, ids, cells, dtype, seed=3)
    segment = bench.build_segment(lx, name, ids, cells, dtype, seed=3)
    beam = lx.ParticleBeam.synthetic((batch,), particles, sigma=bench.BEAM_SIGMA, energy=bench.beam_energy(name), seed=2, dtype=dtype)
    return desc, segment, beam, bench.beam_energy(name)


def _subset(desc, pick, cast=None):
    """The lattice description cut to the samples `pick` (optionally with every array cast to another dtype)."""
    out = []
    for kind, kw in desc:
        sub = {k: np.asarray(v)[pick] for k, v in kw.items()}
        out.append((kind, {k: (v.astype(cast) if cast else v) for k, v in sub.items()}))
    return out


def test_config_5_on_the_bench_beam_product_oracle32_oracle64_distances(lx):
    """
    `bench.py --workload c5` times [Drift, misaligned Quadrupole, Drift, Cavity] x 8 on a beam with sigma_s = 1e-5; the
    other config-5 tests use sigma_s = 1e-4.  This one runs EXACTLY the benched input -- `bench.describe("c5")`,
    `bench.BEAM_SIGMA`, 4096 x 10 000 particles, default environment (structured step loop, lanes build, merged pairs)
    -- and compares, for ALL 4096 environments (the oracles take them 128 at a time, ~20 s), every beam moment of the
    product with the float32 oracle and with the float64 oracle (float32 parameters and particles cast up), next to the
    distance between the two oracles; units: north_star's tolerance scale (helpers.moment_distances' scales).

    What decides the size of these numbers is the kick, cavity.py:150-160:
        delta_out = delta_in E b0 / (E_out b1) + V b0 / (E_out b1) (cos(-s b0 k + phi) - cos(phi)).
    With sigma_s = 1e-5 the phase s b0 k is ~3e-4 rad, so cos(phi + eps) - cos(phi) ~ sin(phi) eps + eps^2/2 is a
    difference of two numbers of order one that agree to 4-5 digits: each float32 cosine carries an absolute error of
    ~6e-8 (half an ulp at 1), i.e. ~1e-3 of the difference, and because all particles of a sample sit within 3e-4 rad
    of each other that error is COMMON to them -- it moves mu_p as a whole, by up to 6e-8 V b0/(E_out b1) per cavity
    against a scale |mu_p| + sigma_p ~ 5e-5.  The reference's float32 chain (the float32 oracle) is therefore up to
    5.0e-4 away from its float64 chain in mu_p on this input, 9 % of the environments beyond 1e-4 -- and so is every
    float32 evaluation that subtracts two cosines, with whatever cosine (NumPy's, XLA's, this library's polynomial until
    late in round 4: up to 4.3e-4 from the float32 oracle, 5.9e-4 from the float64 one).  The kernels now form the
    difference as cos(phi)(cos d - 1) - sin(phi) sin d (device_cavity_kick: relative error 1e-7, same instruction
    count), and with that the product is ON the float64 chain -- mu_p 2e-8, sigma_p 1e-6, mu_s 2e-7 -- in every
    environment; its distance from the float32 chain is that chain's own distance from float64.

    Asserted, per environment and per moment: within 1e-4 of the float32 chain with the kernels' form of the kick
    (o.segment_track(..., kick="product")), and for the moments the kick decides (mu_s, mu_p, sigma_s, sigma_p) within
    1e-5 of the float64 chain.  The reference-form float32 chain is computed next to them and its distances printed.
    """
    dtype = np.float32
    desc, segment, beam, energy = _bench_workload(lx, "c5", dtype)
    B, N = beam.batch_shape[0], beam.num_particles
    assert (B, N, len(desc)) == (4096, 10_000, 32)
    out = segment.track(beam)
    got_all = {key: np.asarray(getattr(out, key), dtype=np.float64) for key in MOMENT_KEYS}
    P_all = np.asarray(beam.particles)
    tracked_all = np.asarray(out.particles)
    energy_all = np.asarray(out.energy)
    worst = {key: np.zeros(4) for key in MOMENT_KEYS}  # product-oracle32, product-oracle64, oracle32-oracle64, product-kick32
    for lo in range(0, B, 128):
        pick = list(range(lo, lo + 128))
        P = P_all[pick]
        _, specs32 = make_lattice(_subset(desc, pick), dtype)
        _, specs64 = make_lattice(_subset(desc, pick, cast=np.float64), np.float64)
        e = np.full(len(pick), energy, dtype=dtype)
        ref32 = o.segment_track(specs32, o.particle_beam(P, e, dtype), dtype)
        kick32 = o.segment_track(specs32, o.particle_beam(P, e, dtype), dtype, kick="product")
        ref64 = o.segment_track(specs64, o.particle_beam(P.astype(np.float64), e.astype(np.float64), np.float64), np.float64)
        m32, m64, mk = o.beam_moments(ref32, ddof=1), o.beam_moments(ref64, ddof=1), o.beam_moments(kick32, ddof=1)
        for key in MOMENT_KEYS:
            if key.startswith("mu_"):
                scale = np.abs(m64[key]) + m64["sigma" + key[2:]]
            elif key in ("sigma_xxp", "sigma_yyp"):
                scale = m64["sigma_x"] * m64["sigma_xp"] if key == "sigma_xxp" else m64["sigma_y"] * m64["sigma_yp"]
            else:
                scale = m64[key]
            r32 = np.asarray(m32[key], dtype=np.float64)
            d_p32 = np.abs(got_all[key][pick] - r32) / scale
            d_p64 = np.abs(got_all[key][pick] - m64[key]) / scale
            d_3264 = np.abs(r32 - m64[key]) / scale
            d_pk = np.abs(got_all[key][pick] - np.asarray(mk[key], dtype=np.float64)) / scale
            assert np.all(d_pk <= 1e-4), (key, lo, float(np.max(d_pk)))
            if key in KICK_MOMENTS:
                assert np.all(d_p64 <= TOL_KICK_F64), (key, lo, float(np.max(d_p64)))
            worst[key] = np.maximum(worst[key], [d_p32.max(), d_p64.max(), d_3264.max(), d_pk.max()])
        if lo % 1024 == 0:  # the particles of a stretch of samples, and their energies
            for c in range(7):
                err = rel_err(tracked_all[pick][..., c], kick32["particles"][..., c])
                assert err < 1e-4, (lo, c, err)
            assert rel_err(energy_all[pick], kick32["energy"]) < 1e-6
    print("config 5 on the bench beam (sigma_s = 1e-5), all 4096 environments: worst distance per moment")
    print(f"{'moment':>10} {'product-oracle32':>18} {'product-oracle64':>18} {'oracle32-oracle64':>18} {'product-kick32':>18}")
    for key in MOMENT_KEYS:
        print(f"{key:>10} {worst[key][0]:18.2e} {worst[key][1]:18.2e} {worst[key][2]:18.2e} {worst[key][3]:18.2e}")
    assert np.all(np.asarray(out.moment_record())[:, 35] == N)


def test_config_4_angle_scan_at_its_full_size_against_the_oracle_and_sample_by_sample(lx, record_property):
    """
    BASELINE config 4 is a "k1/angle scan"; `bench.py --workload c4a` is its corrector-angle variant (SURVEY.md section
    8d): the 128-element FODO with a horizontal and a vertical corrector in place of the drifts of every cell, k1 fixed,
    the two angles scanned over the 1024 samples.  A corrector's angle sits in the AFFINE column of its map
    (horizontal_corrector.py:52-67: [1, 6] = angle; vertical_corrector.py:52-66: [3, 6]), which the k1 scan never fills
    -- and the x2 linearity trick of the k1 test does not hold here (the affine column does not scale with the beam).
    At the full size, default environment (lanes build, wave tiles, reduction on the side stream):
    (1) three samples drawn at random per run (seed recorded) plus the ends of the scan against `o.segment_track`:
        particles at 1e-4 of each coordinate's scale, moments at north_star's 1e-4 (means are ~ sigma here);
    (2) sample independence and the batch-index <-> output-index mapping: 256 samples in a random ORDER as a batch of
        their own (same builder, same kernels) must give, bit for bit, the particles those samples got inside the
        1024-sample batch (segment.py:329-342, element.py:83-92).
    """
    import bench

    dtype = np.float32
    desc, segment, beam, energy = _bench_workload(lx, "c4a", dtype)
    B, N = beam.batch_shape[0], beam.num_particles
    assert (B, N, len(desc)) == (1024, 100_000, 128)
    out = segment.track(beam)
    tracked = np.asarray(out.particles)
    pick, seed = random_samples(B, 3, always=(0, 1023), record=record_property)
    P = np.asarray(beam.particles)
    _, specs = make_lattice(_subset(desc, pick), dtype)
    ref = o.segment_track(specs, o.particle_beam(P[pick], np.full(len(pick), energy, dtype=dtype), dtype), dtype)
    m = o.beam_moments(ref, ddof=1)
    for c in range(7):
        err = rel_err(tracked[pick][..., c], ref["particles"][..., c])
        assert err < 1e-4, (c, err)
    got = {key: np.asarray(getattr(out, key))[pick] for key in m if hasattr(out, key)}
    d = moment_distances(got, m)
    print("config 4, angle scan, samples", pick, {k: f"{v:.1e}" for k, v in d.items()})
    assert max(d.values()) <= 1e-4, d
    # the orbit does depend on the sample: the scan is not a copy of one sample
    assert np.ptp(np.asarray(out.mu_x)) > np.max(np.asarray(out.sigma_x))  # ends of the scan: -1.1e-4 and +1.1e-4 m
    assert np.all(np.asarray(out.moment_record())[:, 35] == N)
    # (2) 256 samples in random order, as their own batch
    order = np.random.default_rng(seed).permutation(B)[:256]
    sub = bench.build_segment(lx, "c4a", order, 32, dtype, seed=3)
    alone = sub.track(lx.ParticleBeam(P[order], np.full(256, energy, dtype=dtype), dtype=dtype))
    assert np.array_equal(np.asarray(alone.particles), tracked[order])
    rec_a, rec_b = np.asarray(alone.moment_record()), np.asarray(out.moment_record())[order]
    have = ~np.isnan(rec_b)
    assert np.array_equal(np.isnan(rec_a), ~have) and np.allclose(rec_a[have], rec_b[have], rtol=1e-9, atol=1e-30)


@pytest.mark.parametrize("name", ["c3", "c3big"])
def test_config_3_at_its_full_size_directly_against_the_oracle(lx, name):
    """
    BASELINE config 3 as worded (128-element FODO, 1 M particles, float64, batch 1) and at the 8 M particles the
    roofline figure is quoted on (`bench.py --workload c3 / c3big`: same lattice, same beam recipe): every particle of
    the outgoing beam against `o.segment_track` at 1e-10 of the coordinate's scale, the moments at north_star's 1e-6
    (segment.py:329-342: one composed map; element.py:83-92: particles @ tm^T) -- the oracle is one matmul here, so
    the direct comparison is affordable at the full size.
    """
    dtype = np.float64
    desc, segment, beam, energy = _bench_workload(lx, name, dtype)
    N = beam.num_particles
    assert (beam.batch_shape, len(desc)) == ((1,), 128) and N == (1_000_000 if name == "c3" else 8_000_000)
    out = segment.track(beam)
    P = np.asarray(beam.particles)
    _, specs = make_lattice(desc, dtype)
    ref = o.segment_track(specs, o.particle_beam(P, np.full(1, energy), dtype), dtype)
    got = np.asarray(out.particles)
    for c in range(7):
        err = rel_err(got[..., c], ref["particles"][..., c])
        assert err < 1e-10, (c, err)
    _assert_moments(out, ref, np.float64)
    d = moment_distances(out, o.beam_moments(ref, ddof=1))
    print(f"{name}: moments within {max(d.values()):.1e} of the float64 oracle")
    assert np.asarray(out.moment_record())[0, 35] == N


def test_c4_shape_composed_map_is_the_exact_product_of_its_float32_element_maps(lx):
    """The float32 build multiplies in float64: the composed map equals the float64 product of the
    GPU's own float32 element maps to float32 rounding, whatever the association.  (Against the
    oracle's chain the distance is set by the element maps -- float32 sin / cos of the device vs
    NumPy's, amplified over 128 elements -- not by the products.)"""
    B = 16
    desc = _fodo_scan(B)
    elements, specs = make_lattice(desc, np.float32, lx)
    energy = np.full(B, 1e8, dtype=np.float32)
    got = lx.Segment(elements).transfer_map(energy).astype(np.float64)
    exact = np.broadcast_to(np.eye(7), (B, 7, 7)).copy()
    for el in elements[:4]:  # one FODO cell; the lattice repeats it 32 times
        exact = np.matmul(el.transfer_map(energy).astype(np.float64), exact)
    cell = exact.copy()
    for _ in range(31):
        exact = np.matmul(cell, exact)
    assert map_err(got, exact) < 2e-7
    chain = o.segment_transfer_map(specs, energy, np.float32)
    print(f"C4 shape: composed map {map_err(got, chain):.2e} from the float32 reference chain")
    assert map_err(got, chain) < 5e-4


def test_c5_shape_moments(lx):
    """
    BASELINE config 5's shape ([Drift, misaligned Quad, Drift, Cavity] x 8 at 6 MeV, 10 000 particles,
    float32): every beam moment within north_star's 1e-4 of the reference's chain in float32 or in float64
    (_assert_moments).  mu_p and sigma_p pass through eight cavity kicks cos(phi + eps) - cos(phi) (cavity.py:150-160):
    evaluated in float32 as two cosines -- the reference's form -- the mean of delta is 2e-4 of its scale away from the
    float64 chain even on this 0.1 mm bunch; the kernel forms the difference without the cancellation.  Asserted: every
    moment within 1e-4 of the float32 chain with the kernels' form (kick="product"), within 1e-4 of the float64 chain as
    a whole and within 1e-5 of it in the moments the kick decides.  The distances are printed.
    """
    B, N = 16, 10_000
    rng = np.random.default_rng(3)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(8):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                                 frequency=f(1.3e9)))]
    sigma = [1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3]
    out, ref = _particle_case(lx, desc, np.float32, (B,), N, seed=3, energy=6e6, sigma=sigma)
    _assert_moments(out, ref, np.float32)
    _, ref_specs32 = make_lattice(desc, np.float32)
    _, specs64 = make_lattice([(k, {a: np.asarray(v, dtype=np.float32).astype(np.float64) for a, v in kw.items()})
                               for k, kw in desc], np.float64)
    P = o.gaussian_particles((B,), N, seed=3, dtype=np.float32, sigma=sigma)
    ref64 = o.segment_track(specs64, o.particle_beam(P.astype(np.float64), np.full(B, 6e6), np.float64), np.float64)
    d32 = _moment_distance(out, o.beam_moments(ref, ddof=1))
    d64 = _moment_distance(out, o.beam_moments(ref64, ddof=1))
    dref = _moment_distance(out, o.beam_moments(o.segment_track(ref_specs32, o.particle_beam(P, np.full(B, 6e6, np.float32), np.float32),
                                                                np.float32), ddof=1))
    print(f"C5 shape: moments {d32:.2e} from the float32 product-kick chain, {d64:.2e} from float64, "
          f"{dref:.2e} from the float32 reference-kick chain")
    assert d64 < 1e-4 and d32 < 1e-4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_c1_ares_segment_parameter_beam(lx, dtype):
    """
    BASELINE config 1: the 11-element README segment (README.md:34-48, angles of docs/examples/simple.ipynb)
    x `ParameterBeam.from_parameters()` defaults (parameter_beam.py:97-113), batch 1 -- mu and cov
    against `Segment.track` of the oracle (segment.py:340-356, element.py:71-82) at north_star's
    tolerances, entry by entry relative to sigma_i sigma_j.
    """
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    segment = lx.Segment([
        lx.BPM(name="BPM1SMATCH"), lx.Drift(f(1.0), dtype=dtype), lx.BPM(name="BPM6SMATCH"), lx.Drift(f(1.0), dtype=dtype),
        lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), name="V7SMATCH", dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(1e-4), name="H10SMATCH", dtype=dtype), lx.Drift(f(7.0), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), name="H12SMATCH", dtype=dtype), lx.Drift(f(0.05), dtype=dtype),
        lx.BPM(name="BPM13SMATCH")])
    specs = [o.BPM(), o.Drift(f(1.0)), o.BPM(), o.Drift(f(1.0)), o.VerticalCorrector(f(0.3), f(3.142e-3)), o.Drift(f(0.2)),
             o.HorizontalCorrector(f(0.3), f(1e-4)), o.Drift(f(7.0)), o.HorizontalCorrector(f(0.3), f(-1e-4)),
             o.Drift(f(0.05)), o.BPM()]
    assert len(segment.elements) == 11 and segment.is_skippable
    beam = lx.ParameterBeam.from_parameters(dtype=dtype)
    assert beam._mu.shape == (1, 7) and beam.energy.shape == (1,) and beam.energy[0] == 1e8
    out = segment.track(beam)
    ref = o.segment_track(specs, o.parameter_beam_from_parameters(dtype=dtype), dtype)
    tol = TOL_MOM[dtype]
    sig = np.sqrt(np.diagonal(ref["cov"], axis1=-2, axis2=-1)[..., :6].astype(np.float64))
    assert np.all(np.abs(out._mu[..., :6] - ref["mu"][..., :6]) <= tol * (np.abs(ref["mu"][..., :6]) + sig))
    assert np.array_equal(out._mu[..., 6], ref["mu"][..., 6])
    for i in range(6):
        for j in range(6):
            assert np.all(np.abs(out._cov[..., i, j] - ref["cov"][..., i, j]) <= tol * sig[..., i] * sig[..., j]), (i, j)
    assert np.array_equal(out._cov[..., 6, :], ref["cov"][..., 6, :])
    m = o.beam_moments(ref)
    for key in ("sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p"):
        assert np.allclose(getattr(out, key), m[key], rtol=tol, atol=0), key
    assert np.allclose(out.mu_y, m["mu_y"], rtol=tol) and np.allclose(out.mu_x, m["mu_x"], rtol=tol, atol=tol * 1e-6)
    assert np.array_equal(out.energy, beam.energy) and np.array_equal(out.total_charge, beam.total_charge)
    # the same lattice as one map: transfer_map(energy) agrees with what track applied
    tm = segment.transfer_map(beam.energy)
    assert map_err(tm, o.segment_transfer_map(specs, beam.energy, dtype)) < TOL_MAP[dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 70, 300])
def test_lanes_build_agrees_with_the_workgroup_build(lx, dtype, B, monkeypatch):
    """
    The two builders of the step table -- one workgroup per sample (small batches) and lanes = samples
    (large batches: k_build_pieces / k_pair_products / k_emit_steps) -- on the same lattice: every element
    kind, tilt, misalignment, cavities between runs, a run longer than a piece, a batch that is not a
    multiple of 64.  Same float64 accumulation, different association: float32 results agree to the
    last bit or two, float64 to ~1e-15; both agree with the oracle.
    """
    rng = np.random.default_rng(17)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))),
            ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B), tilt=rng.uniform(-1, 1, B),
                                misalignment=rng.normal(0, 1e-4, (B, 2)))),
            ("marker", {}),
            ("dipole", dict(length=f(0.5), angle=rng.uniform(-0.2, 0.2, B), e1=f(0.05), e2=f(0.02),
                            fringe_integral=f(0.4), gap=f(0.02), tilt=f(0.1))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                            frequency=f(1.3e9)))]
    for _ in range(5):  # a 20-element run: three pieces of 8, 8, 4
        desc += [("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B))), ("drift", dict(length=f(0.5))),
                 ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, B))), ("solenoid", dict(length=f(0.1), k=f(0.5)))]
    desc += [("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=f(2.0), frequency=f(1.3e9))),
             ("rbend", dict(length=f(0.3), angle=f(0.05))), ("vcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, B)))]
    results = {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        out, ref = _particle_case(lx, desc, dtype, (B,), 700, seed=8, energy=6e6, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
        results[name] = (np.asarray(out.particles), np.asarray(out.energy), out.moment_record().copy())
        got = np.asarray(out.particles)
        tol = {np.float32: [1e-4] * 6 + [1e-6], np.float64: [1e-9] * 7}[dtype]  # (float32: the product-kick chain)
        for c in range(7):
            assert rel_err(got[..., c], ref["particles"][..., c]) < tol[c], (name, c)
        assert rel_err(out.energy, ref["energy"]) < 1e-6
    a, b = results["workgroup"], results["lanes"]
    close = 2e-6 if dtype == np.float32 else 1e-12
    for c in range(7):
        assert rel_err(b[0][..., c], a[0][..., c]) < close, c
    assert np.array_equal(a[1], b[1])
    # a skippable lattice as ONE composed map, through both builders
    skippable = [d for d in desc if d[0] != "cavity"]
    energy = np.full(B, 1e8, dtype=dtype)
    maps = {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        maps[name] = lx.Segment(make_lattice(skippable, dtype, lx)[0]).transfer_map(energy)
    assert map_err(maps["lanes"], maps["workgroup"]) < (1e-6 if dtype == np.float32 else 1e-13)


def test_lanes_build_spreads_nan_like_the_reference(lx, monkeypatch):
    """A switched-off cavity inside a run carries the reference's NaN (cavity.py:269); the product with the
    rest of the run and with eye(7) must spread it the same way in both builders."""
    desc = [("drift", dict(length=[0.5] * 3)),
            ("cavity", dict(length=[1.0] * 3, voltage=[0.0, 0.0, 0.0], phase=[0.0] * 3, frequency=[1.3e9] * 3)),
            ("quadrupole", dict(length=[0.2] * 3, k1=[1.0, -2.0, 3.0]))]
    energy = np.array([1e8, 6e6, 1.0732e8], dtype=np.float32)
    maps = {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        elements, specs = make_lattice(desc, np.float32, lx)
        maps[name] = lx.Segment(elements).transfer_map(energy)
    ref = o.segment_transfer_map(specs, energy, np.float32)
    assert np.array_equal(np.isnan(maps["lanes"]), np.isnan(ref)) and np.array_equal(np.isnan(maps["workgroup"]), np.isnan(ref))
    assert np.isnan(ref).any()


def test_cavity_mixed_zero_voltage_batch_matches_reference_nan(lx):
    """reference tests/test_vectorized.py:423-439: no error; V = 0 rows carry the reference's NaN."""
    desc = [("cavity", dict(length=[3.0441] * 3, voltage=[0.0, 48198468.0, 0.0], phase=[48198468.0] * 3,
                            frequency=[2.8560e09] * 3))]
    out, ref = _particle_case(lx, desc, np.float32, (3,), 500, seed=1, sigma=[1e-5, 2e-7, 175e-9, 2e-7, 1e-6, 1e-6])
    got = np.asarray(out.particles)
    assert np.array_equal(np.isnan(got), np.isnan(ref["particles"]))
    assert np.isnan(got[0, :, 0]).all() and not np.isnan(got[1]).any()


# ---------------------------------------------------------------------------------------------
# ParameterBeam
# ---------------------------------------------------------------------------------------------


def test_kat1_parameter_beam_drift(lx):
    """try_batched.ipynb: from_twiss -> sigma_x etc, then Drift([1, 2])."""
    beam = lx.ParameterBeam.from_twiss(
        beta_x=np.array([61.47503078, 99.0]), alpha_x=np.array([-1.21242463, -0.9]),
        emittance_x=np.array([7.1971891e-13, 5e-13]), beta_y=np.array([35.41897281, 60.0]),
        alpha_y=np.array([0.66554622, 0.5]), emittance_y=np.array([3.5866484e-15, 1e-15]),
        energy=np.array([150e6, 14.6e9]))
    assert np.allclose(beam.sigma_x, [6.6517e-06, 7.0356e-06], rtol=1e-4)
    assert np.allclose(beam.relativistic_gamma, [293.5427, 28571.4863], rtol=1e-6)
    out = lx.Drift(length=np.array([1.0, 2.0])).track(beam)
    assert np.allclose(out.sigma_x, [6.7837e-06, 7.1650e-06], rtol=1e-4)
    assert np.allclose(out.sigma_y, [3.4987e-07, 2.4100e-07], rtol=1e-4)
    assert np.allclose(out.sigma_xp, beam.sigma_xp) and np.allclose(out.sigma_yp, beam.sigma_yp)


def _same_bits(a, b):
    """bit-identical up to the sign of zero; NaNs in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), 0, a) + 0.0, np.where(np.isnan(b), 0, b) + 0.0)


def test_lanes_build_with_a_wide_pair_tree_agrees_with_the_workgroup_build(lx, monkeypatch):
    """
    A run of 300 elements is 38 pieces of 8: the first level of the pair tree has 19 products -- more than the
    one-launch form of the tree takes (k_pair_levels: at most 16 per level), so the levels are launched one by one
    (k_pair_products).  Same table as the workgroup build to rounding, and the oracle's particles.
    """
    B, n = 256, 600
    rng = np.random.default_rng(31)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for k in range(150):
        desc += [("drift", dict(length=f(0.05))), ("quadrupole", dict(length=f(0.02), k1=rng.uniform(-2, 2, B)))]
    results = {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        out, ref = _particle_case(lx, desc, np.float32, (B,), n, seed=3, energy=1e8)
        results[name] = np.asarray(out.particles)
        _assert_particles(out, ref, np.float32)
    for c in range(7):
        assert rel_err(results["lanes"][..., c], results["workgroup"][..., c]) < 2e-6, c


@pytest.mark.parametrize("case", ["uncoupled", "dispersive", "coupled", "nan_map", "sequential"])
def test_structured_units_equal_the_dense_step_loop_bit_for_bit(lx, monkeypatch, case):
    """
    Multi-step float32 programs are walked as units whose maps hold only the entries that are not structurally zero
    (lynx_units.hpp: 16 for [drift, quadrupole, corrector, cavity] runs, 24 with untilted dipoles); LYNX_TRACK_UNITS=0
    keeps the dense 7x7 step loop.  On finite beams the two must agree bit for bit (a skipped term adds +-0: signed
    zeros aside) -- particles, energy and moment records -- for every class: uncoupled, dispersive, a tilted quadrupole
    (the numeric check sends every sample to the dense form), a zero-voltage cavity row (NaN in the map: that sample
    dense, cavity.py:269), and with every step on its own.  (track_methods.py:86-98, quadrupole.py:75-79, cavity.py:311-323.)
    """
    B, N = 6, 90_000  # large enough for two particles per lane, the form large beams get
    rng = np.random.default_rng(21)
    f = lambda v: np.full(B, v)  # noqa: E731
    volts = rng.uniform(5e6, 2e7, B)
    if case == "nan_map":
        volts[2] = 0.0
    cell = lambda: [("drift", dict(length=f(0.3))),  # noqa: E731
                    ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)),
                                        **({"tilt": rng.uniform(-0.5, 0.5, B)} if case == "coupled" else {}))),
                    ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, B))),
                    *([("dipole", dict(length=f(0.4), angle=rng.uniform(-0.1, 0.1, B), e1=f(0.02), e2=f(0.01)))] if case == "dispersive" else []),
                    ("drift", dict(length=f(0.3))),
                    ("cavity", dict(length=f(1.0377), voltage=volts, phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    desc = cell() + cell() + cell() + [("drift", dict(length=f(0.2))), ("vcor", dict(length=f(0.1), angle=f(1e-4)))]
    elements, _ = make_lattice(desc, np.float32, lx)
    segment = lx.Segment(elements)
    P = o.gaussian_particles((B,), N, seed=5, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    beam = lx.ParticleBeam(P, np.full(B, 6e6, np.float32), dtype=np.float32)
    if case == "sequential":
        monkeypatch.setattr(lx.config, "merge_steps", False)
    outs = {}
    for units in ("2", "0"):  # 2 = the structured loop or an error
        monkeypatch.setenv("LYNX_TRACK_UNITS", units)
        out = segment.track(beam)
        outs["1" if units == "2" else "0"] = (np.asarray(out.particles), np.asarray(out.energy), np.asarray(out.moment_record()))
    for k in range(3):
        assert _same_bits(outs["1"][k], outs["0"][k]), (case, k)
    if case != "nan_map":
        assert np.all(np.isfinite(outs["1"][0]))
    else:
        assert np.all(np.isnan(outs["1"][0][2, :, :4])) and np.all(np.isfinite(outs["1"][0][[0, 1, 3, 4, 5]]))


@pytest.mark.parametrize("case", ["every_sample", "no_voltage", "not_finite", "wide_kick", "no_moments"])
def test_the_kernel_for_lattices_of_pairs_equals_the_general_one_bit_for_bit(lx, monkeypatch, case):
    """
    A float32 lattice all of whose units are merged [run, cavity] pairs of class U -- BASELINE config 5's [Drift, misaligned
    Quadrupole, Drift, Cavity] cells -- is streamed by a kernel of its own (k_track_unit_pairs, lynx_units.hpp; insisted on
    with LYNX_UNIT_PAIRS=2): the same functions in the same order without the descriptor's branches.  Same bits as the
    general kernel (LYNX_UNIT_PAIRS=0) and as the dense step loop (LYNX_TRACK_UNITS=0) -- particles, energy, moment record --
    when every sample has the form; when one sample's cavities have no voltage (no kick and a NaN map, cavity.py:269:
    that sample dense, unit by unit); when a tile holds a non-finite particle or one that overflows on the way (the tile
    again, densely); when kicks leave the short form's range (|k s| > 0.25 rad: the tile again with the complete
    difference of cosines); and without fused moments.  (A lattice with a tilted quadrupole is not proposed as class U
    by the host and never reaches this kernel: test_structured_units_equal_the_dense_step_loop_bit_for_bit[coupled].)
    """
    B, N = 6, 90_001  # ragged; large enough for two particles per lane, the form large beams get
    rng = np.random.default_rng(31)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for k in range(4):
        volts = rng.uniform(5e6, 2e7, B)
        if case == "no_voltage":
            volts[3] = 0.0
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=volts, phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    elements, specs = make_lattice(desc, np.float32, lx)
    segment = lx.Segment(elements)
    sigma_s = 5e-3 if case == "wide_kick" else 1e-4  # k = 27.2 rad/m at 1.3 GHz: |k s| > 0.25 beyond 9.2 mm
    P = o.gaussian_particles((B,), N, seed=7, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, sigma_s, 1e-3])
    if case == "not_finite":
        P[0, 17, 2] = np.inf
        P[2, 40_000, 1] = np.nan
        P[4, 123, 0] = P[4, 123, 1] = 3e38  # finite going in, overflows in the first quadrupole's product
    if case == "wide_kick":
        assert (np.abs(P[..., 4]) * 2 * np.pi * 1.3e9 / 299792458.0 > 0.25).any(axis=1).all()
    beam = lx.ParticleBeam(P, np.full(B, 6e6, np.float32), dtype=np.float32)
    if case == "no_moments":
        monkeypatch.setattr(lx.config, "fused_moments", False)
    outs = {}
    for name, env in (("pairs", {"LYNX_UNIT_PAIRS": "2", "LYNX_TRACK_UNITS": "2"}), ("general", {"LYNX_UNIT_PAIRS": "0", "LYNX_TRACK_UNITS": "2"}),
                      ("dense", {"LYNX_TRACK_UNITS": "0"})):
        for key in ("LYNX_UNIT_PAIRS", "LYNX_TRACK_UNITS"):
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        out = segment.track(beam)
        outs[name] = [np.asarray(out.particles), np.asarray(out.energy)] + ([] if case == "no_moments" else [np.asarray(out.moment_record())])
    for other in ("general", "dense"):
        for k in range(len(outs["pairs"])):
            assert _same_bits(outs["pairs"][k], outs[other][k]), (case, other, k)
    got = outs["pairs"][0]
    ref = o.segment_track(specs, o.particle_beam(P, np.full(B, 6e6, np.float32), np.float32), np.float32)["particles"]
    # the reference's NaN pattern (a NaN map, a non-finite particle); where a finite particle OVERFLOWS on the way, inf - inf
    # or not depends on the order of the sums inside numpy's float32 matmul: that one is compared among the kernels only
    same = np.isnan(got) == np.isnan(ref)
    if case == "not_finite":
        same[4, 123] = True
    assert same.all()
    if case in ("every_sample", "wide_kick", "no_moments"):
        assert np.all(np.isfinite(got))
        # and the oracle's numbers, on the float32 chain or the float64 one (the kick: DESIGN section 2, deviation (v))
        ref64 = o.segment_track(specs, o.particle_beam(P.astype(np.float64), np.full(B, 6e6), np.float64), np.float64)["particles"]
        for c in range(6):
            assert min(rel_err(got[..., c], ref[..., c]), rel_err(got[..., c], ref64[..., c])) < (2e-4 if case == "wide_kick" else 1e-4), (case, c)


def test_structured_units_spread_a_non_finite_particle_like_the_dense_chain(lx, monkeypatch):
    """
    0 * inf = NaN: in the reference's `particles @ tm^T` (element.py:85) an infinite y makes every coordinate of that
    particle NaN, zero entries of the map or not.  The structured step loop skips those entries, so a wave that holds
    a non-finite value -- going in, or coming out after an overflow on the way -- redoes its tile with the dense form:
    the outcome must be the dense loop's, for the particle itself and for everybody else.
    """
    B, N = 2, 270_000
    rng = np.random.default_rng(22)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(3):
        desc += [("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    elements, specs = make_lattice(desc, np.float32, lx)
    segment = lx.Segment(elements)
    P = o.gaussian_particles((B,), N, seed=6, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    P[0, 17, 2] = np.inf        # y of one particle
    P[1, 4000, 1] = np.nan      # x' of another
    P[1, 123, 0] = 3e38         # finite going in, overflows in the first quadrupole's product
    P[1, 123, 1] = 3e38
    beam = lx.ParticleBeam(P, np.full(B, 6e6, np.float32), dtype=np.float32)
    outs = {}
    for units in ("2", "0"):
        monkeypatch.setenv("LYNX_TRACK_UNITS", units)
        outs["1" if units == "2" else "0"] = np.asarray(segment.track(beam).particles)
    assert _same_bits(outs["1"], outs["0"])
    ref = o.segment_track(specs, o.particle_beam(P, np.full(B, 6e6, np.float32), np.float32), np.float32)["particles"]
    assert np.array_equal(np.isnan(outs["1"]), np.isnan(ref))           # the reference's NaN pattern
    assert np.all(np.isnan(outs["1"][0, 17, :6])) and np.all(np.isnan(outs["1"][1, 4000, :6]))
    assert np.isfinite(outs["1"][0, 16]).all() and np.isfinite(outs["1"][1, 4001]).all()


def test_energy_not_above_zero_at_a_cavity_is_the_references_assertion(lx):
    """
    cavity.py:260 (`assert torch.all(Ei > 0)`) for energies the host never sees: the check runs on the device while
    the cavities' whole-batch predicates are evaluated (k_cavity_flags) and surfaces as AssertionError at the next
    read-back or sync.  (a) a beam whose energy exists in HBM only -- the output of an earlier program -- and is
    negative; (b) one sample of a batch decelerated through zero by the first cavity of the SAME program;
    (c) the incoming energy of a host-resident beam is still refused at once.
    """
    from lynx_amd.device import get_runtime

    dtype = np.float32
    f = lambda *v: np.asarray(v, dtype=dtype)  # noqa: E731
    P = o.gaussian_particles((2,), 4096, seed=4, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    brake = lx.Cavity(f(1.0, 1.0), voltage=f(2e7, 2e7), phase=f(0.0, 180.0), frequency=f(1.3e9, 1.3e9), dtype=dtype)
    boost = lx.Cavity(f(1.0, 1.0), voltage=f(1e7, 1e7), phase=f(0.0, 0.0), frequency=f(1.3e9, 1.3e9), dtype=dtype)
    beam = lx.ParticleBeam(P, f(6e6, 6e6), dtype=dtype)
    # (a) sample 1 leaves the first segment with 6 MeV - 20 MeV < 0 (the batch moves on: sample 0 gains)
    mid = lx.Segment([lx.Drift(f(0.1, 0.1), dtype=dtype), brake]).track(beam)
    assert mid._energy._host is None  # lives in HBM only: nothing was read back
    out = lx.Segment([lx.Drift(f(0.1, 0.1), dtype=dtype), boost]).track(mid)  # enqueued without complaint ...
    with pytest.raises(AssertionError, match="Initial energy must be larger than 0"):
        np.asarray(out.particles)  # ... and refused when the result is looked at
    get_runtime().sync()  # the flag was consumed: the runtime is usable again
    # (b) both cavities in one program
    out = lx.Segment([brake, lx.Drift(f(0.1, 0.1), dtype=dtype), boost]).track(beam)
    with pytest.raises(AssertionError, match="Initial energy must be larger than 0"):
        get_runtime().sync()
    # a healthy program afterwards is not affected
    good = lx.Segment([boost, lx.Drift(f(0.1, 0.1), dtype=dtype), boost]).track(beam)
    assert np.allclose(good.energy, 6e6 + 2e7)
    # (c) host-resident incoming energy: at once, as before
    with pytest.raises(AssertionError, match="Initial energy must be larger than 0"):
        lx.Segment([boost]).track(lx.ParticleBeam(P, f(6e6, -1.0), dtype=dtype))
    # ParameterBeam path, same rule
    pb = lx.ParameterBeam.from_parameters(energy=f(6e6, 6e6), dtype=dtype)
    pmid = lx.Segment([brake]).track(pb)
    pout = lx.Segment([boost]).track(pmid)
    with pytest.raises(AssertionError, match="Initial energy must be larger than 0"):
        np.asarray(pout._mu)


def test_kat4_cavity_bmad_twiss(lx):
    """reference tests/test_compare_ocelot.py:627-654 (Bmad-confirmed Twiss after the cavity)."""
    beam = lx.ParameterBeam.from_twiss(
        beta_x=np.array([5.91253677]), alpha_x=np.array([3.55631308]), emittance_x=np.array([3.494768647122823e-09]),
        beta_y=np.array([5.91253677]), alpha_y=np.array([3.55631308]), emittance_y=np.array([3.497810737006068e-09]),
        energy=np.array([6e6]), dtype=np.float64)
    cavity = lx.Cavity(length=np.array([1.0377]), voltage=np.array([0.01815975e9]), frequency=np.array([1.3e9]),
                       phase=np.array([0.0]), dtype=np.float64)
    out = cavity.track(beam)
    assert np.isclose(out.beta_x, 0.23847352510683092, rtol=1e-6)
    assert np.isclose(out.alpha_x, -1.0160687592932345, rtol=1e-6)
    assert np.isclose(out.beta_y, 0.23847352512430994, rtol=1e-6)
    assert np.isclose(out.alpha_y, -1.0160687593664295, rtol=1e-6)
    assert np.isclose(out.energy, 6e6 + 0.01815975e9)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameter_beam_through_mixed_lattice(lx, dtype):
    B = 7
    rng = np.random.default_rng(9)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                            frequency=f(1.3e9))),
            ("drift", dict(length=f(0.4))), ("hcor", dict(length=f(0.1), angle=f(1e-4))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=f(0.0), frequency=f(1.3e9))),
            ("dipole", dict(length=f(0.5), angle=f(0.1)))]
    elements, specs = make_lattice(desc, dtype, lx)
    kw = dict(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), sigma_s=f(1e-5),
              sigma_p=f(1e-3), mu_x=rng.normal(0, 1e-4, B), energy=f(6e6))
    kw = {k: np.asarray(v, dtype=dtype) for k, v in kw.items()}
    beam = lx.ParameterBeam.from_parameters(**kw, dtype=dtype)
    ref_in = o.parameter_beam_from_parameters(dtype=dtype, **kw)
    out = lx.Segment(elements).track(beam)
    ref = o.segment_track(specs, ref_in, dtype, kick="product")  # (float32 behind an active cavity: _assert_moments)
    # north_star's tolerances, entry by entry.  Measured on MI355X (scripts/gpu/r3_pb_study.py, float32): product vs
    # float32 oracle 2.8e-5 (mu) / 4.0e-6 (cov), float32 oracle vs float64 oracle 7.9e-7 / 3.1e-5 -- nothing in
    # cavity.py:134-140, 202-218 cancels in float32 on this lattice.
    assert_parameter_beam(out, ref, 1e-4 if dtype == np.float32 else 1e-9)
    assert rel_err(out.energy, ref["energy"]) < 1e-6


def test_parameter_beam_lanes_path_agrees_with_the_workgroup_path(lx, monkeypatch):
    """
    float32 ParameterBeam batches of >= 256 samples go lanes = samples (lanes build + k_apply_moments_lanes),
    smaller ones one workgroup per sample (k_track_moments): the same lattice with cavities through both, and
    against the oracle (element.py:71-82, cavity.py:134-140, 202-218).
    """
    B = 300
    rng = np.random.default_rng(12)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B), tilt=rng.uniform(-1, 1, B))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9))),
            ("drift", dict(length=f(0.4))), ("hcor", dict(length=f(0.1), angle=f(1e-4))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=f(0.0), frequency=f(1.3e9))),
            ("dipole", dict(length=f(0.5), angle=f(0.1)))]
    for _ in range(3):
        desc += [("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B))), ("drift", dict(length=f(0.5))), ("vcor", dict(length=f(0.1), angle=f(1e-4)))]
    dtype = np.float32
    kw = dict(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), sigma_s=f(1e-5), sigma_p=f(1e-3),
              mu_x=rng.normal(0, 1e-4, B), energy=f(6e6))
    kw = {k: np.asarray(v, dtype=dtype) for k, v in kw.items()}
    outs = {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        elements, specs = make_lattice(desc, dtype, lx)
        out = lx.Segment(elements).track(lx.ParameterBeam.from_parameters(**kw, dtype=dtype))
        outs[name] = (np.array(out._mu), np.array(out._cov), np.array(out.energy))
    ref = o.segment_track(specs, o.parameter_beam_from_parameters(dtype=dtype, **kw), dtype)
    for name, (mu, cov, energy) in outs.items():
        # measured (scripts/gpu/r3_pb_study.py): 3.4e-5 (mu) / 5.5e-6 (cov) from the float32 oracle on either path
        assert_parameter_beam((mu, cov), ref, 1e-4, name)
        assert rel_err(energy, ref["energy"]) < 1e-6, name
    a, b = outs["workgroup"], outs["lanes"]
    assert rel_err(b[0], a[0]) < 1e-5 and np.array_equal(a[2], b[2])
    sc = np.sqrt(np.abs(np.einsum("bii,bjj->bij", a[1][..., :6, :6], a[1][..., :6, :6]))) + 1e-300
    assert np.max(np.abs(b[1][..., :6, :6] - a[1][..., :6, :6]) / sc) < 1e-4


def test_parameter_beam_huge_batch(lx):
    """reference tests/test_vectorized.py:298-321 in spirit: (3, 100000) settings at once."""
    shape = (3, 20_000)
    k1 = np.tile(np.linspace(-30.0, 30.0, shape[1]), (3, 1)).astype(np.float32)
    seg = lx.Segment([lx.Drift(np.full(shape, 0.2, np.float32)), lx.Quadrupole(np.full(shape, 0.122, np.float32), k1=k1),
                      lx.Drift(np.full(shape, 0.4, np.float32))])
    beam = lx.ParameterBeam.from_parameters(sigma_x=np.full(shape, 1e-4, np.float32))
    out = seg.track(beam)
    assert out.mu_x.shape == shape and out.sigma_x.shape == shape and out.energy.shape == shape
    specs = [o.Drift(np.full(shape, 0.2, np.float32)), o.Quadrupole(np.full(shape, 0.122, np.float32), k1=k1),
             o.Drift(np.full(shape, 0.4, np.float32))]
    ref = o.segment_track(specs, o.parameter_beam_from_parameters(sigma_x=np.full(shape, 1e-4, np.float32)), np.float32)
    assert np.allclose(out.sigma_x, o.beam_moments(ref)["sigma_x"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------
# moments, kernel variants, invariants
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moment_readout_of_existing_beam(lx, dtype):
    P = o.gaussian_particles((2, 2), 30_001, seed=4, dtype=dtype, mu=[1e-3, -1e-4, 2e-3, 0, 0, 1e-3],
                             sigma=[1e-6, 1e-7, 2e-6, 1e-7, 1e-5, 1e-4])
    beam = lx.ParticleBeam(P, np.full((2, 2), 1e8), dtype=dtype)
    _assert_moments(beam, o.particle_beam(P, np.full((2, 2), 1e8), dtype), dtype)
    # |mu| >> sigma: a naive fp32 sum of squares would have no correct digit here
    assert np.allclose(beam.sigma_x, 1e-6, rtol=2e-2)


def test_fused_moments_equal_separate_pass(lx):
    out, _ = _particle_case(lx, ARES, np.float32, (1,), 50_000, seed=0)
    fused = out.moment_record().copy()
    fresh = lx.ParticleBeam(np.asarray(out.particles), out.energy, dtype=np.float32)
    again = fresh.moment_record()
    assert np.allclose(fused[..., :28], again[..., :28], rtol=1e-9, atol=1e-30, equal_nan=True)
    assert fused[..., 35] == again[..., 35] == 50_000
    # the fused record carries what the reference's properties need; the rest of the covariance is NaN ...
    have = [7, 8, 13, 18, 19, 22, 25, 27]
    assert not np.isnan(fused[..., :7]).any() and not np.isnan(fused[..., have]).any()
    assert np.isnan(np.delete(fused[..., 7:28], [h - 7 for h in have], axis=-1)).all() and fused[0, 34] == 0.0
    # ... until somebody asks for it: one more pass, whole 6x6 matrix, same values where both exist
    cov = out.covariance()
    P = np.asarray(out.particles)[0, :, :6].astype(np.float64)
    want = np.cov(P.T, bias=True)
    s = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.max(np.abs(cov[0] - want) / s) < 1e-6
    full = out.moment_record()
    assert full[0, 34] == 1.0 and np.allclose(full[..., have], fused[..., have], rtol=1e-6)


def test_fused_covariance_switch(lx):
    """`config.fused_covariance`: the tracking kernel's epilogue accumulates all 21 products."""
    lx.config.fused_covariance = True
    try:
        out, ref = _particle_case(lx, ARES, np.float64, (1,), 20_000, seed=5)
    finally:
        lx.config.fused_covariance = False
    rec = out.moment_record()
    assert np.all(rec[..., 34] == 1.0) and not np.isnan(rec).any()
    P = ref["particles"][..., :6]
    for b in range(1):
        want = np.cov(P[b].T, bias=True)
        s = np.sqrt(np.outer(np.diag(want), np.diag(want)))
        assert np.max(np.abs(out.covariance()[b] - want) / s) < 1e-9


VARIANTS = [
    {"LYNX_XPOSE": "1"}, {"LYNX_XPOSE": "0"}, {"LYNX_ASYNC_BUILD": "1"}, {"LYNX_ASYNC_BUILD": "0"},
    {"LYNX_LANES_BUILD_MIN_BATCH": "1"}, {"LYNX_LANES_BUILD_MIN_BATCH": "1", "LYNX_PIECE": "3"},
    {"LYNX_LANES_BUILD_MIN_BATCH": "1", "LYNX_PIECE": "1"},  # two levels of pair products, in one launch (k_pair_levels)
    {"LYNX_LANES_BUILD_MIN_BATCH": "1", "LYNX_PIECE": "1", "LYNX_PAIR_LEVELS_FUSED": "0"},  # ... one launch per level
    {"LYNX_UNROLL": "1"}, {"LYNX_UNROLL": "2"}, {"LYNX_UNROLL": "4"}, {"LYNX_MOM": "2"}, {"LYNX_MOM": "3"},
    {"LYNX_MIN_TILES_PER_WG": "1"}, {"LYNX_MERGE_STEPS": "0"},
    {"LYNX_SIDE_REDUCE": "1"}, {"LYNX_ASYNC_BUILD": "1", "LYNX_BUILD_HOST_WAIT": "1"}, {"LYNX_BUILD_IN_TAIL": "0", "LYNX_ASYNC_BUILD": "1"},
    {"LYNX_SMALL_INLINE": "0"}, {"LYNX_SMALL_INLINE": "1"},
    {"LYNX_ALTERNATE_ORDER": "2", "LYNX_UNROLL": "1"}, {"LYNX_ALTERNATE_ORDER": "2", "LYNX_TRACK_UNITS": "0"}, {"LYNX_UNIT_PAIRS": "0"},
    {"LYNX_ONE_ROUND": "0"}, {"LYNX_ONE_ROUND": "1"},
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_kernel_variant_gives_the_default_answer(lx, dtype, monkeypatch):
    """
    The launch plan picks one of several forms of the same computation (wave tiles or per-particle
    accesses, particles per lane, moment accumulation mode, build on the second stream or in line,
    lanes or workgroup build, tile order ...).  Every knob, on a lattice with cavities
    and an active BPM, a ragged particle count and a batch: particles agree with the default plan to
    rounding (the forms differ in the association of the map products only), moments and the BPM
    reading to the moment tolerance.
    """
    B, n = 5, 6151
    rng = np.random.default_rng(23)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731

    def lattice():
        els = []
        for k in range(3):
            els += [lx.Drift(f(0.3), dtype=dtype), lx.Quadrupole(f(0.2), k1=(rng0.uniform(-4, 4, B)).astype(dtype), dtype=dtype),
                    lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=dtype), lx.Drift(f(0.4), dtype=dtype)]
            if k == 1:
                els.append(lx.BPM(is_active=True, name="bpm"))
            els.append(lx.Cavity(f(1.0377), voltage=f(1.2e7), phase=f(2.0), frequency=f(1.3e9), dtype=dtype))
        return lx.Segment(els)

    P = o.gaussian_particles((B,), n, seed=9, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    energy = np.full(B, 6e6, dtype=dtype)
    results = []
    for env in [{}] + VARIANTS:
        for key in {k for v in VARIANTS for k in v}:
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        rng0 = np.random.default_rng(23)
        seg = lattice()
        out = seg.track(lx.ParticleBeam(P, energy, dtype=dtype))
        results.append((env, np.asarray(out.particles), out.moment_record().copy(), seg.bpm.reading.copy(), np.asarray(out.energy)))
    _, p0, m0, r0, e0 = results[0]
    close = 5e-6 if dtype == np.float32 else 1e-12
    for env, p, m, r, e in results[1:]:
        for c in range(7):
            assert rel_err(p[..., c], p0[..., c]) < close, (env, c)
        assert np.array_equal(e, e0), env
        have = ~np.isnan(m0)
        assert np.array_equal(np.isnan(m), np.isnan(m0)), env
        assert np.allclose(m[have], m0[have], rtol=TOL_MOM[dtype] * 0.1, atol=1e-30), env
        assert np.allclose(r, r0, rtol=TOL_MOM[dtype], atol=1e-12), env
    # the pair tree in one launch or in one launch per level: the same products in the same order
    tree = [p for env, p, *_ in results if env.get("LYNX_PIECE") == "1"]
    assert len(tree) == 2 and np.array_equal(tree[0], tree[1])


def test_merged_pairs_agree_with_the_step_by_step_form_and_the_oracle(lx):
    desc = [("drift", dict(length=[0.6] * 3)), ("quadrupole", dict(length=[0.2] * 3, k1=[4.2, -1.0, 0.0])),
            ("cavity", dict(length=[1.0] * 3, voltage=[1e7] * 3, phase=[5.0] * 3, frequency=[1.3e9] * 3)),
            ("drift", dict(length=[0.4] * 3))]
    # 200 000 particles per sample: large enough for the two-particles-per-lane plan, the one that merges
    lx.config.merge_steps = False  # step by step
    try:
        a, _ = _particle_case(lx, desc, np.float32, (3,), 200_000, seed=8, energy=6e6)
        # default: the run in front of the cavity is applied together with it -- same algebra,
        # one rounding of the 7x7 product more in the build and one application less per particle
        lx.config.merge_steps = True
        c, ref = _particle_case(lx, desc, np.float32, (3,), 200_000, seed=8, energy=6e6)
    finally:
        lx.config.merge_steps = True
    got, seq = np.asarray(c.particles), np.asarray(a.particles)
    assert not np.array_equal(got, seq)
    for k in range(6):
        scale = np.max(np.abs(ref["particles"][..., k]))
        # delta: the merged form recovers the s that enters the cavity from the product's own components (a few
        # float32 roundings away from the step-by-step value), which can move the float32 cosine of the kick
        # by one ulp (6e-8 at cos ~ 1), times the kick's amplitude V beta0 / (E_out beta1) < 1
        assert np.max(np.abs(got[..., k] - seq[..., k])) < 5e-6 * scale + (1.2e-7 if k == 5 else 0.0), k
        assert np.max(np.abs(got[..., k] - ref["particles"][..., k])) < 1e-4 * scale, k  # the oracle's cos is NumPy's


@pytest.mark.parametrize("units", ["2", "0"])
def test_merged_pairs_with_an_ill_conditioned_cavity_block_take_the_rows_form(lx, monkeypatch, units):
    """
    The merged [run, cavity] form recovers the s and delta that enter the cavity from components 4, 5 of the product
    map's output with the inverse of the cavity's (s, delta) block.  At 1 MeV and 30 degrees off crest that block of the
    reference's map (cavity.py:311-323) is singular at V = 0.5247 MV, and next to that voltage the inverse amplifies
    the float32 rounding of M z by (|c44 c55| + |c45 c54|) / |det|: 5e4, 5e3, 5e2, 25 for samples 0-3 here (with the
    guard switched off sample 0 is 4e-4 of the delta scale away from the step-by-step form).  The build marks such
    samples (LYNX_DESC_ILL, per sample) and the kernels take the two from the run's rows instead -- the results must stay
    as close to the step-by-step form and to the oracle as everywhere else, in both step loops (units / dense).
    Sample 4 is well-conditioned and keeps the inverse form.
    """
    B, N, E = 5, 200_000, 1e6
    v0 = singular_entry_voltage(E, -30.0, 1.0, 1.3e9, 4e5, 6.5e5)
    volts = np.array([v0 * (1 + 1e-4), v0 * (1 - 1e-3), v0 * (1 + 1e-2), v0 * 1.2, 4e5])
    phases = np.array([-30.0, -30.0, -30.0, -30.0, 0.0])
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.5))), ("quadrupole", dict(length=f(0.2), k1=f(1.5))),
            ("cavity", dict(length=f(1.0), voltage=volts, phase=phases, frequency=f(1.3e9))),
            ("drift", dict(length=f(0.4))),
            ("cavity", dict(length=f(1.0), voltage=f(3e5), phase=f(0.0), frequency=f(1.3e9))), ("drift", dict(length=f(0.1)))]
    monkeypatch.setenv("LYNX_TRACK_UNITS", units)
    merged, ref = _particle_case(lx, desc, np.float32, (B,), N, seed=12, energy=E)
    monkeypatch.setattr(lx.config, "merge_steps", False)
    stepwise, _ = _particle_case(lx, desc, np.float32, (B,), N, seed=12, energy=E)
    got, seq = np.asarray(merged.particles), np.asarray(stepwise.particles)
    assert np.all(np.isfinite(got))
    assert not np.array_equal(got, seq)  # the merged form did run
    for b in range(B):
        for k in range(6):
            scale = np.max(np.abs(ref["particles"][b, :, k]))
            assert np.max(np.abs(got[b, :, k] - seq[b, :, k])) < 2e-5 * scale, (b, k)
            assert np.max(np.abs(got[b, :, k] - ref["particles"][b, :, k])) < 1e-4 * scale, (b, k)
    assert np.array_equal(merged.energy, stepwise.energy)


def test_relational_invariants_from_the_reference_suite(lx):
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    beam = lx.ParameterBeam.from_parameters(sigma_xp=f(2e-7), sigma_yp=f(2e-7))
    # tests/test_quadrupole.py:6-22: k1 = 0 quadrupole == drift
    quad, drift = lx.Quadrupole(length=f(1.0), k1=f(0.0)), lx.Drift(length=f(1.0))
    assert np.allclose(quad(beam).sigma_x, drift(beam).sigma_x)
    quad.k1 = f(1.0)
    assert not np.allclose(quad(beam).sigma_x, drift(beam).sigma_x)
    # tests/test_dipole.py:6-22: angle = 0 dipole == drift
    pbeam = lx.ParticleBeam.from_parameters(num_particles=10_000, sigma_xp=f(2e-7), sigma_yp=f(2e-7), seed=0)
    dip = lx.Dipole(length=f(1.0), angle=f(0.0))
    assert np.allclose(dip(pbeam).sigma_x, drift(pbeam).sigma_x)
    dip.angle = f(1.0)
    assert not np.allclose(dip(pbeam).sigma_x, drift(pbeam).sigma_x)
    # tests/test_quadrupole.py:77-98: tilt pi/4 == 5pi/4 != pi/2
    inc = lx.ParticleBeam.from_parameters(num_particles=20_000, energy=f(1e9), mu_x=f(1e-5), seed=1).broadcast((3,))
    seg = lx.Segment([lx.Quadrupole(length=np.full(3, 0.5, np.float32), k1=np.ones(3, np.float32),
                                    tilt=np.array([np.pi / 4, np.pi / 2, np.pi * 5 / 4], dtype=np.float32)),
                      lx.Drift(length=f(0.5)).broadcast((3,))])
    out = np.asarray(seg(inc).particles)
    assert np.allclose(out[0], out[2], atol=1e-9) and not np.allclose(out[0], out[1])
    # tests/test_dipole.py:25-45: equal batch entries -> equal outputs (bit-exact here)
    seg = lx.Segment([lx.Dipole(length=np.full(3, 0.5, np.float32), angle=np.array([0.1, 0.2, 0.1], np.float32)),
                      lx.Drift(length=f(0.5)).broadcast((3,))])
    out = np.asarray(seg(inc).particles)
    assert np.array_equal(out[0], out[2]) and not np.allclose(out[0], out[1])


def test_broadcast_then_track_equals_track(lx):
    """tests/test_vectorized.py:324-366 (the cavity case uses exact == there too)."""
    cavity = lx.Cavity(length=np.array([3.0441]), voltage=np.array([48198468.0]), phase=np.array([-0.0]),
                       frequency=np.array([2.8560e09]), name="k26_2d")
    incoming = lx.ParameterBeam.from_parameters(sigma_x=np.array([1e-4], np.float32), energy=np.array([1.07e8], np.float32))
    outgoing = cavity.track(incoming)
    b_out = cavity.broadcast((3, 10)).track(incoming.broadcast((3, 10)))
    for i in range(3):
        for j in range(10):
            assert np.all(b_out._mu[i, j] == outgoing._mu[0])
            assert np.all(b_out._cov[i, j] == outgoing._cov[0])


def test_merged_maps_equal_unmerged(lx):
    """tests/test_speed_optimizations.py:6-75,157-184"""
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    incoming = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), sigma_xp=f(1e-5), energy=f(1.07e8))
    seg = lx.Segment([lx.Drift(f(0.6)), lx.Quadrupole(f(0.2), k1=f(4.2), name="Q1"), lx.Drift(f(0.4)),
                      lx.HorizontalCorrector(f(0.1), angle=f(1e-4), name="HCOR_1"), lx.Drift(f(0.4))])
    merged = seg.transfer_maps_merged(incoming_beam=incoming)
    assert len(merged.elements) == 1
    a, b = seg.track(incoming), merged.track(incoming)
    for key in ("mu_x", "mu_xp", "sigma_x", "sigma_xp", "sigma_y", "sigma_s", "sigma_p", "energy"):
        assert np.allclose(getattr(a, key), getattr(b, key), rtol=1e-5), key
    part = seg.transfer_maps_merged(incoming_beam=incoming, except_for=["Q1", "HCOR_1"])
    assert [type(e).__name__ for e in part.elements] == ["Drift", "Quadrupole", "Drift", "HorizontalCorrector",
                                                        "CustomTransferMap"]
    assert np.allclose(seg.elements[2].transfer_map(incoming.energy), part.elements[2].transfer_map(incoming.energy))


def test_active_bpm_reads_the_beam_position(lx):
    """bpm.py:48-58"""
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    seg = lx.Segment([lx.Drift(f(1.0)), lx.HorizontalCorrector(f(0.1), angle=f(1e-3)), lx.Drift(f(1.0)),
                      lx.BPM(name="my_bpm"), lx.Drift(f(1.0))])
    for beam in (lx.ParticleBeam.from_parameters(num_particles=20_000, seed=2), lx.ParameterBeam.from_parameters()):
        seg.my_bpm.is_active = False
        ref_out = seg.track(beam)
        assert seg.my_bpm.reading is None
        seg.my_bpm.is_active = True
        out = seg.track(beam)
        assert seg.my_bpm.reading.shape == (2, 1)
        assert np.isclose(seg.my_bpm.reading[0, 0], 1e-3 * 1.0, rtol=2e-3)  # kick at the corrector's end, then 1 m
        assert np.allclose(out.mu_x, ref_out.mu_x, rtol=1e-5)
        seg.my_bpm.reading = None


@pytest.mark.parametrize("dtype,n", [(np.float32, 5000), (np.float32, 4097), (np.float64, 6000), (np.float64, 1001)])
def test_active_bpms_are_read_inside_the_streaming_pass(lx, dtype, n):
    """
    bpm.py:48-58 -- `reading = stack([mu_x, mu_y])` of the beam entering an active BPM.  For a ParticleBeam
    the BPMs are steps of ONE program (LYNX_STEP_FLAG_OBSERVE): no split of the pass, no host round trip;
    readings against the oracle's, for BPMs behind linear runs and behind a cavity, ragged particle counts,
    both dtypes (float64 takes the wave-tile kernel).
    """
    from lynx_amd import engine

    B = 3
    rng = np.random.default_rng(31)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k1 = rng.uniform(-4, 4, B).astype(dtype)
    ang = rng.normal(0, 1e-3, B).astype(dtype)
    volt = rng.uniform(5e6, 2e7, B).astype(dtype)
    els = [lx.Drift(f(0.5), dtype=dtype), lx.HorizontalCorrector(f(0.1), angle=ang, dtype=dtype), lx.BPM(is_active=True, name="b0"),
           lx.Quadrupole(f(0.2), k1=k1, dtype=dtype), lx.Drift(f(0.7), dtype=dtype), lx.BPM(is_active=True, name="b1"),
           lx.Cavity(f(1.0377), voltage=volt, phase=f(3.0), frequency=f(1.3e9), dtype=dtype), lx.BPM(is_active=True, name="b2"),
           lx.VerticalCorrector(f(0.1), angle=ang, dtype=dtype), lx.Drift(f(0.3), dtype=dtype), lx.BPM(name="idle"),
           lx.BPM(is_active=True, name="b3")]
    specs = [o.Drift(f(0.5)), o.HorizontalCorrector(f(0.1), ang), o.BPM(True), o.Quadrupole(f(0.2), k1=k1), o.Drift(f(0.7)), o.BPM(True),
             o.Cavity(f(1.0377), voltage=volt, phase=f(3.0), frequency=f(1.3e9)), o.BPM(True), o.VerticalCorrector(f(0.1), ang),
             o.Drift(f(0.3)), o.BPM(False), o.BPM(True)]
    seg = lx.Segment(els)
    P = o.gaussian_particles((B,), n, seed=6, dtype=dtype, mu=[2e-4, 0, -1e-4, 1e-5, 0, 0], sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    energy = np.full(B, 6e6, dtype=dtype)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    items = engine.plan(seg, seg.elements, False, fuse_observers=True)
    assert len(items) == 1 and len(items[0].observers) == 4  # one program: nothing splits the pass
    out = seg.track(beam)
    readings = []
    ref = o.segment_track(specs, o.particle_beam(P, energy, dtype), dtype, bpm_readings=readings, kick="product")
    assert len(readings) == 4
    tol = TOL_MOM[dtype]
    sig_x = float(np.std(P[..., 0])) + 1e-4
    for name, (_, want) in zip(("b0", "b1", "b2", "b3"), readings):
        got = getattr(seg, name).reading
        assert got.shape == (2, B) and got.dtype == np.dtype(dtype)
        assert np.all(np.abs(got - want) <= tol * (np.abs(want) + 3 * sig_x)), (name, got, want)
    assert seg.idle.reading is None
    got = np.asarray(out.particles)
    ptol = {np.float32: [1e-4] * 6 + [1e-6], np.float64: [1e-9] * 7}[dtype]
    for c in range(7):
        assert rel_err(got[..., c], ref["particles"][..., c]) < ptol[c], c
    _assert_moments(out, ref, dtype)
    # the same lattice seen by a ParameterBeam keeps the host-side reading (no particles to add up)
    pb = lx.ParameterBeam.from_parameters(mu_x=np.full(B, 2e-4, dtype), energy=energy, dtype=dtype)
    seg.track(pb)
    assert seg.b3.reading.shape == (2, B)


def test_more_active_bpms_than_one_program_reads(lx):
    """Beyond LYNX_MAX_OBSERVERS (8) active BPMs the pass is split on the host, as before; every reading is still right."""
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    els = []
    for k in range(11):
        els += [lx.Drift(f(0.3)), lx.HorizontalCorrector(f(0.1), angle=f(1e-4 * (k + 1))), lx.BPM(is_active=True, name=f"m{k}")]
    seg = lx.Segment(els)
    beam = lx.ParticleBeam.from_parameters(num_particles=30_000, sigma_x=f(1e-5), sigma_xp=f(1e-6), seed=4)
    seg.track(beam)
    x, xp = 0.0, 0.0
    for k in range(11):
        a = 1e-4 * (k + 1)
        x += xp * 0.3  # drift
        x += xp * 0.1 + 0.0  # corrector: drift part; the kick lands in x' only (horizontal_corrector.py:52-67)
        xp += a
        assert np.isclose(getattr(seg, f"m{k}").reading[0, 0], x, rtol=5e-3, atol=2e-7), (k, getattr(seg, f"m{k}").reading, x)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cavity_predicates_are_evaluated_on_the_device(lx, dtype):
    """
    cavity.py:128,164,290 -- `if any(...)` over the whole batch, with the energy each cavity sees being the
    result of the cavities before it.  `k_cavity_flags` leaves the bits in slot 62 of every step-table row;
    checked against the oracle's bookkeeping for: an accelerating pair, a decelerating cavity (no T5XX), a
    mixed batch where only one sample has voltage, and a switched-off cavity inside a run (BETA bit only,
    no step).  Then the energy leaves one program in HBM and enters the next without a read-back.
    """
    from lynx_amd import _ffi, engine
    from lynx_amd.device import get_runtime

    B = 3
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    cases = [
        (dict(voltage=f(1e7), phase=f(10.0)), _ffi.FLAG_CAV_BETA | _ffi.FLAG_CAV_GAIN | _ffi.FLAG_CAV_T5XX),
        (dict(voltage=f(1e7), phase=f(180.0)), _ffi.FLAG_CAV_BETA | _ffi.FLAG_CAV_GAIN),
        (dict(voltage=np.array([0.0, 1e7, 0.0], dtype=dtype), phase=f(10.0)), _ffi.FLAG_CAV_BETA | _ffi.FLAG_CAV_GAIN | _ffi.FLAG_CAV_T5XX),
        (dict(voltage=f(-2e8), phase=f(0.0)), _ffi.FLAG_CAV_BETA),  # E + dE < 0 on every sample: no gain step at all
    ]
    rt = get_runtime()
    for kw, want in cases:
        cav = lx.Cavity(f(1.0), frequency=f(1.3e9), dtype=dtype, **kw)
        seg = lx.Segment([lx.Drift(f(0.5), dtype=dtype), cav, lx.Drift(f(0.5), dtype=dtype)])
        program = engine.plan(seg, seg.elements, False)[0]
        lat = engine._ready(seg.__dict__.setdefault("_lattice_cache", engine.LatticeCache()), program, (B,), dtype, None)
        e_in = rt.to_device(f(1e8))
        steps = rt.empty((B, len(program.steps), _ffi.STEP_STRIDE), dtype)
        rt.check(rt.lib.lynx_build_compose(rt.ctx, lat.handle, engine._ptr(e_in), engine._ptr(steps), None))
        desc = steps.numpy()[:, :, 62].astype(np.int64)  # flags | kind << 16 (| pair bit)
        assert np.all(desc[:, 1] & 0xFFFF == want) and np.all(desc[:, 1] >> 16 == _ffi.STEP_CAVITY), (kw, desc)
        assert np.all(desc[:, 0] == 0) and np.all(desc[:, 2] == 0)
    # The predicates of all cavities are first evaluated side by side under the assumption that every batch gains
    # energy (k_cavity_flags_spec).  Here it does not hold: the first cavity would take every sample below zero, so
    # nobody moves on (cavity.py:128-130) and the second cavity sees the INCOMING energy -- the serial walk must take
    # over: second cavity BETA | GAIN | T5XX, and no complaint about its energy (the assumed one was negative).
    brake = lx.Cavity(f(1.0), frequency=f(1.3e9), voltage=f(-2e8), phase=f(0.0), dtype=dtype)
    boost = lx.Cavity(f(1.0), frequency=f(1.3e9), voltage=f(1e7), phase=f(10.0), dtype=dtype)
    seg = lx.Segment([brake, lx.Drift(f(0.5), dtype=dtype), boost])
    program = engine.plan(seg, seg.elements, False)[0]
    lat = engine._ready(seg.__dict__.setdefault("_lattice_cache", engine.LatticeCache()), program, (B,), dtype, None)
    e_in = rt.to_device(f(1e8))
    for _ in range(2):  # twice: the words the first kernel accumulates into must be clean again
        steps = rt.empty((B, len(program.steps), _ffi.STEP_STRIDE), dtype)
        rt.check(rt.lib.lynx_build_compose(rt.ctx, lat.handle, engine._ptr(e_in), engine._ptr(steps), None))
        table = steps.numpy()
        desc = table[:, :, 62].astype(np.int64)
        assert np.all(desc[:, 0] & 0xFFFF == _ffi.FLAG_CAV_BETA), desc
        assert np.all(desc[:, 2] & 0xFFFF == (_ffi.FLAG_CAV_BETA | _ffi.FLAG_CAV_GAIN | _ffi.FLAG_CAV_T5XX)), desc
        assert np.allclose(table[:, 2, 63], 1e8 + 1e7 * np.cos(np.deg2rad(10.0)), rtol=1e-6)  # outgoing energy
        rt.sync()  # would raise if the assumed (negative) energy had been reported
    # chained programs: the first one's outgoing energy stays in HBM, the second evaluates its predicates from it
    seg = lx.Segment([lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), dtype=dtype), lx.Drift(f(0.3), dtype=dtype)])
    P = o.gaussian_particles((B,), 2000, seed=1, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    first = seg.track(lx.ParticleBeam(P, f(6e6), dtype=dtype))
    assert first._energy._host is None  # lives in HBM
    second = seg.track(first)
    assert first._energy._host is None  # and tracking it did not read it back
    assert np.allclose(second.energy, 6e6 + 2e7, rtol=1e-6)
    ref1 = o.segment_track([o.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9)), o.Drift(f(0.3))],
                           o.particle_beam(P, f(6e6), dtype), dtype, kick="product")
    ref2 = o.segment_track([o.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9)), o.Drift(f(0.3))], ref1, dtype,
                           kick="product")
    _assert_moments(second, ref2, dtype)


def test_error_conventions(lx):
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    with pytest.raises(TypeError):
        lx.Drift(f(1.0)).track("not a beam")
    assert lx.Drift(f(1.0)).track(lx.Beam.empty) is lx.Beam.empty
    with pytest.raises(AssertionError):  # drift.py:45-47
        lx.Drift(np.ones(2, np.float32)).transfer_map(np.ones(3, np.float32))
    with pytest.raises(AssertionError):
        lx.Segment([lx.Drift(np.ones(2, np.float32))]).track(lx.ParameterBeam.from_parameters(sigma_x=np.ones(3, np.float32)))
    with pytest.raises(AssertionError):  # particle_beam.py:35-37
        lx.ParticleBeam(np.ones((1, 10, 6), np.float32), f(1e8))
    with pytest.raises(AssertionError):  # cavity.py:260
        lx.Cavity(f(1.0), voltage=f(1e6), frequency=f(1.3e9)).track(lx.ParameterBeam.from_parameters(energy=f(0.0)))
    # tests/test_tracking_lengthless_elements.py
    beam_in = lx.ParticleBeam.from_parameters(num_particles=100, seed=0)
    assert np.allclose(np.asarray(lx.Segment([lx.Marker(name="start")]).track(beam_in).particles), np.asarray(beam_in.particles))
    lx.Segment([lx.Cavity(f(0.1), voltage=f(1e6), name="C2"), lx.Marker(name="start"),
                lx.Cavity(f(0.1), voltage=f(1e6), name="C1")]).track(beam_in)


# ---------------------------------------------------------------------------------------------
# full-size properties (BASELINE sizes, checked through size-independent properties)
# ---------------------------------------------------------------------------------------------


def test_c3_size_round_trip_and_map_consistency(lx):
    """C3: 128-element FODO, 1 M particles, fp64.  track -> track through the inverse map
    returns the input; output moments == T Sigma T^T of the input moments."""
    dtype = np.float64
    f = lambda v: np.array([v])  # noqa: E731
    elements = []
    for _ in range(32):
        elements += [lx.Quadrupole(f(0.2), k1=f(4.2), dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                     lx.Quadrupole(f(0.2), k1=f(-4.2), dtype=dtype), lx.Drift(f(0.5), dtype=dtype)]
    seg = lx.Segment(elements)
    beam = lx.ParticleBeam.synthetic((1,), 1_000_000, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=1,
                                     dtype=dtype)
    out = seg.track(beam)
    tm = seg.transfer_map(np.array([1e8]))
    inv = lx.CustomTransferMap(np.linalg.inv(tm), dtype=dtype)
    back = inv.track(out)
    a, b = np.asarray(beam.particles), np.asarray(back.particles)
    assert np.max(np.abs(a - b) / (np.abs(a).max(axis=(0, 1)) + 1e-300)) < 1e-9
    rec_in, rec_out = beam.moment_record(covariance=True)[0], out.moment_record(covariance=True)[0]
    cov_in = np.zeros((6, 6))
    cov_out = np.zeros((6, 6))
    k = 7
    for i in range(6):
        for j in range(i, 6):
            cov_in[i, j] = cov_in[j, i] = rec_in[k]
            cov_out[i, j] = cov_out[j, i] = rec_out[k]
            k += 1
    pred = tm[0, :6, :6] @ cov_in @ tm[0, :6, :6].T
    s = np.sqrt(np.outer(np.diag(pred), np.diag(pred)))
    assert np.max(np.abs(cov_out - pred) / s) < 1e-9
    assert rec_out[35] == 1_000_000


def test_c4_shard_linearity_fp32(lx):
    """C4 per-GPU shard in small multiples: 32 samples x 100k x 128 elements, fp32.
    Linearity: track(2 P) == 2 track(P) exactly (power-of-two scaling commutes with fp32
    rounding), and sample b's result does not depend on its neighbours."""
    dtype = np.float32
    B, N = 32, 100_000
    scale = (0.5 + np.arange(B) / (B - 1)).astype(dtype)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    elements = []
    for _ in range(32):
        elements += [lx.Quadrupole(f(0.2), k1=4.2 * scale), lx.Drift(f(0.5)), lx.Quadrupole(f(0.2), k1=-4.2 * scale),
                     lx.Drift(f(0.5))]
    seg = lx.Segment(elements)
    beam = lx.ParticleBeam.synthetic((B,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=2, dtype=dtype)
    out = np.asarray(seg.track(beam).particles)
    P = np.asarray(beam.particles)
    P2 = P.copy()
    P2[..., :6] *= 2  # 7th coordinate multiplies zeros only (no correctors here)
    out2 = np.asarray(seg.track(lx.ParticleBeam(P2, np.full(B, 1e8, dtype), dtype=dtype)).particles)
    assert np.array_equal(out2[..., :6], 2 * out[..., :6])
    # sample 5 alone, through the same lattice row
    sub = lx.Segment([lx.Quadrupole(np.array([0.2], dtype), k1=4.2 * scale[5:6]) if i % 4 == 0 else
                      lx.Quadrupole(np.array([0.2], dtype), k1=-4.2 * scale[5:6]) if i % 4 == 2 else
                      lx.Drift(np.array([0.5], dtype)) for i in range(128)])
    alone = np.asarray(sub.track(lx.ParticleBeam(P[5:6], np.array([1e8], dtype), dtype=dtype)).particles)
    assert np.array_equal(alone[0], out[5])


@pytest.mark.parametrize("dtype,n", [(np.float32, 300_000), (np.float32, 70_001), (np.float64, 200_003)])
def test_tracking_in_place_through_the_c_abi(lx, dtype, n):
    """
    include/lynx_hip.h: `d_p_in` and `d_p_out` of lynx_track_particles may alias.  Wave tiles (every wave reads a
    tile, prefetches the next and writes the first back) and per-particle accesses, full and cut tiles: tracking
    a copy of the beam in place gives the bytes of the out-of-place call.
    """
    import ctypes as C

    from lynx_amd import _ffi, engine
    from lynx_amd.device import get_runtime

    rt = get_runtime()
    B = 3
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    seg = lx.Segment([lx.Drift(f(0.4), dtype=dtype), lx.Quadrupole(f(0.2), k1=np.asarray([4.0, -3.0, 0.5], dtype), dtype=dtype),
                      lx.Drift(f(0.7), dtype=dtype)])
    beam = lx.ParticleBeam.synthetic((B,), n, seed=4, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    expected = np.asarray(seg.track(beam).particles)
    program, = engine.plan(seg, seg.elements, False, fuse_observers=True)
    lat = engine._ready(seg.__dict__["_lattice_cache"], program, (B,), np.dtype(dtype), beam._energy._host)
    work = rt.to_device(np.asarray(beam.particles))
    e_in = beam._energy.broadcast_device(rt, (B,))
    mom = rt.empty((B, _ffi.MOMENT_STRIDE), np.float64)
    rt.check(rt.lib.lynx_track_particles(rt.ctx, lat.handle, n, C.c_void_p(e_in.ptr), C.c_void_p(work.ptr),
                                         C.c_void_p(work.ptr), None, C.c_void_p(mom.ptr), _ffi.TRACK_MOMENTS, None))
    assert np.array_equal(np.asarray(work), expected)


@pytest.mark.parametrize("overlap", ["0", "1"], ids=["main-stream", "communication-stream"])
def test_rccl_communicator_single_rank(lx, overlap, monkeypatch):
    """The RCCL path of lynx_amd.parallel at world_size 1 (the only size a 1-GPU box allows): the gather in line
    on the main stream, and on the communication stream (LYNX_GATHER_OVERLAP=1) with tracking going on around it --
    several gathers in flight, results read back afterwards."""
    from lynx_amd.device import get_runtime
    from lynx_amd.parallel import RcclCommunicator

    monkeypatch.setenv("LYNX_GATHER_OVERLAP", overlap)
    rt = get_runtime()
    comm = RcclCommunicator(1, 0, lambda uid: uid, rt)
    try:
        local = rt.to_device(np.arange(5 * 36, dtype=np.float64).reshape(5, 36))
        out = comm.all_gather(local)
        assert out.shape == (1, 5, 36)
        assert np.array_equal(np.asarray(out)[0], np.asarray(local))
        seg = lx.Segment([lx.Drift(np.full(4, 0.5, np.float32)), lx.Quadrupole(np.full(4, 0.2, np.float32), k1=np.full(4, 3.0, np.float32))])
        beam = lx.ParticleBeam.synthetic((4,), 50_000, seed=3)
        results = []
        for _ in range(4):  # the host runs ahead: gathers queue up behind the tracking they belong to
            beam = seg.track(beam)
            results.append((beam, comm.all_gather(beam._moments.device(rt).reshape(4, 36))))
        for tracked, gathered in results:
            assert np.array_equal(np.asarray(gathered)[0], tracked.moment_record().reshape(4, 36), equal_nan=True)
    finally:
        comm.close()


def test_a_block_two_side_operations_touch_is_released_by_the_last_of_them(lx, monkeypatch):
    """
    The default multi-rank path: the side stream reduces the workgroups' records into the moment block, the RCCL gather
    behind it sends that same block.  `lynx_buf_free` of it while both are in flight must keep it out of the allocator
    until the LAST of the two has finished (round 3 gave it back with the first: two live arrays could then share a
    block while RCCL still read it).  Here: a queue of long streaming calls, so that the side stream's work of the last
    one is far from done when the host frees; the freed pointer must not come back from the allocator before
    `lynx_sync`, and afterwards it comes back exactly once.
    """
    from lynx_amd.device import get_runtime
    from lynx_amd.parallel import RcclCommunicator

    monkeypatch.setenv("LYNX_GATHER_OVERLAP", "1")
    monkeypatch.setenv("LYNX_SIDE_REDUCE", "1")
    rt = get_runtime()
    rt.sync()
    comm = RcclCommunicator(1, 0, lambda uid: uid, rt)
    try:
        B, N = 256, 200_000
        f = lambda v: np.full(B, v, np.float32)  # noqa: E731
        seg = lx.Segment([lx.Drift(f(0.5)), lx.Quadrupole(f(0.2), k1=f(3.0)), lx.Drift(f(0.4))])
        beam = lx.ParticleBeam.synthetic((B,), N, seed=5)
        nbytes = B * 36 * 8
        outs = [seg.track(beam) for _ in range(12)]  # 12 x 0.5 ms of streaming kernels: the host is milliseconds ahead
        last = outs[-1]
        mom = last._moments.device(rt)
        gathered = comm.all_gather(mom.reshape(B, 36))
        ptr = mom.ptr
        # (no read-back here: that would wait for the side stream)
        # free the moment block while its reduction AND its gather are queued on the side stream
        last._moments = None
        del mom, outs, last
        import gc

        gc.collect()
        taken = [rt.alloc(nbytes) for _ in range(8)]
        assert ptr not in taken, "a block still in flight on the side stream came back from the allocator"
        rt.sync()
        assert np.all(np.asarray(gathered)[0, :, 35] == N)  # the gather read a block nobody had overwritten
        again = [rt.alloc(nbytes) for _ in range(8)]
        assert len(set(taken + again)) == 16, "the allocator handed one block out twice"
        for p in taken + again:
            rt.free(p)
        rt.sync()
    finally:
        comm.close()


def test_particle_sharded_moments_merge_to_the_whole_beam(lx):
    """
    SURVEY.md section 8e, secondary partitioning: slices of one beam tracked separately (as the
    ranks of a particle-sharded run do) and merged with `merge_records` give the whole beam's
    record; the tracked particles of a slice are bit-identical to the same rows of the whole.
    """
    from lynx_amd.parallel import merge_records, shard_particles

    desc = []
    for _ in range(8):
        desc += [("quadrupole", dict(length=[0.2], k1=[4.2])), ("drift", dict(length=[0.5])),
                 ("quadrupole", dict(length=[0.2], k1=[-4.2])), ("drift", dict(length=[0.5]))]
    seg = lx.Segment(make_lattice(desc, np.float64, lx)[0])
    P = o.gaussian_particles((1,), 50_001, seed=12, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3],
                             mu=[2e-3, 0, -1e-3, 0, 0, 0])
    energy = np.full(1, 1e8)
    whole = seg.track(lx.ParticleBeam(P, energy, dtype=np.float64))
    parts, rows = [], []
    for r in range(3):
        a, b = shard_particles(P.shape[1], 3, r)
        out = seg.track(lx.ParticleBeam(P[:, a:b], energy, dtype=np.float64))
        parts.append(out.moment_record())
        rows.append(np.asarray(out.particles))
    assert np.array_equal(np.concatenate(rows, axis=1), np.asarray(whole.particles))
    merged, ref = merge_records(np.stack(parts)), whole.moment_record()
    assert merged[0, 35] == ref[0, 35] == 50_001
    np.testing.assert_allclose(merged[..., :7], ref[..., :7], rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(merged[..., 7:28], ref[..., 7:28], rtol=1e-9, atol=1e-24)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_track_methods_helpers(lx, dtype):
    """lynx/track_methods.py public functions: rotation_matrix, base_rmatrix, misalignment_matrix."""
    from lynx_amd import track_methods as tm

    rng = np.random.default_rng(21)
    ang = rng.uniform(-3, 3, (2, 3)).astype(dtype)
    assert map_err(tm.rotation_matrix(ang), o.rotation_matrix(ang)) < TOL_MAP[dtype]
    L, k1 = rng.uniform(0.1, 1, 5).astype(dtype), np.array([4.2, -4.2, 0.0, 1.0, -30.0], dtype)
    hx, tilt = rng.uniform(-0.5, 0.5, 5).astype(dtype), np.array([0, 0.3, 0, -1.0, 0.785], dtype)
    energy = np.array([1e8, 6e6, 2e7, 1e9, 1e8], dtype)
    got = tm.base_rmatrix(L, k1, hx, tilt, energy)
    ref = o.base_rmatrix(L, k1, hx, tilt, energy)
    assert map_err(got, ref) < TOL_MAP[dtype] * 10
    # energy defaults to 0 => beta = 0: the dispersion entries are 0/0 and inf - inf in the
    # reference too (track_methods.py:61-83); same NaN pattern, finite entries equal
    z = np.zeros_like(L)
    assert map_err(tm.base_rmatrix(L, k1, z), o.base_rmatrix(L, k1, z)) < TOL_MAP[dtype] * 10
    mis = rng.normal(0, 1e-3, (4, 2)).astype(dtype)
    (g_in, g_out), (r_in, r_out) = tm.misalignment_matrix(mis), o.misalignment_matrix(mis)
    assert np.array_equal(g_in, r_in) and np.array_equal(g_out, r_out)
    assert np.isclose(tm.REST_ENERGY, o.REST_ENERGY, rtol=1e-13)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lazily_broadcast_beam_tracks_like_the_repeated_one(lx, dtype):
    """
    `ParticleBeam.broadcast` of a single beam keeps one stored copy (LYNX_TRACK_SHARED_INPUT);
    every observable must equal what the reference's physical repeat (particle_beam.py:838-843)
    gives -- tracked particles and moments bit-for-bit.
    """
    shape = (3, 5)
    single = lx.ParticleBeam.from_parameters(num_particles=4099, sigma_x=np.array([1e-4], dtype), sigma_xp=np.array([1e-5], dtype),
                                             total_charge=np.array([1e-12], dtype), energy=np.array([6e6], dtype),
                                             seed=3, dtype=dtype)
    shared = single.broadcast(shape)
    lx.config.lazy_broadcast = False
    try:
        repeated = single.broadcast(shape)
    finally:
        lx.config.lazy_broadcast = True
    assert shared.is_shared and not repeated.is_shared
    assert shared.batch_shape == repeated.batch_shape == shape
    assert np.array_equal(np.asarray(shared.particles), np.asarray(repeated.particles))
    assert np.array_equal(shared.particle_charges, repeated.particle_charges)
    for name in ("mu_x", "sigma_x", "sigma_xxp", "energy", "total_charge", "emittance_x"):
        assert np.array_equal(getattr(shared, name), getattr(repeated, name)), name
    rng = np.random.default_rng(0)
    f = lambda v: np.full(shape, v, dtype)  # noqa: E731
    seg = lx.Segment([lx.Drift(f(0.3)), lx.Quadrupole(f(0.2), k1=rng.uniform(-5, 5, shape).astype(dtype)),
                      lx.Cavity(f(1.0377), voltage=rng.uniform(5e6, 2e7, shape).astype(dtype), phase=f(3.0), frequency=f(1.3e9)),
                      lx.Drift(f(0.4))])
    a, b = seg.track(shared), seg.track(repeated)
    assert not a.is_shared
    assert np.array_equal(np.asarray(a.particles), np.asarray(b.particles))
    assert np.array_equal(a.moment_record(), b.moment_record(), equal_nan=True)
    assert np.array_equal(a.particle_charges, b.particle_charges) and np.array_equal(a.energy, b.energy)
    # a single element, a write to a coordinate, the reverse pass and the screen all accept it
    assert np.array_equal(np.asarray(seg.elements[1].track(shared).particles), np.asarray(seg.elements[1].track(repeated).particles))
    w = shared.broadcast((1,)) if False else shared._shallow_copy()
    w.xs = np.asarray(w.xs) * 2
    assert not w.is_shared and np.array_equal(np.asarray(w.particles)[..., 0], 2 * np.asarray(repeated.particles)[..., 0])
    assert shared.is_shared  # the copy was written to, not the original


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lazily_broadcast_beam_through_wave_tiles(lx, dtype):
    """The same on the streaming kernel's wave-tile form (one composed map, enough particles for whole tiles plus
    a cut one): every sample reads the ONE stored beam (sample stride 0) and writes its own."""
    shape = (8,)
    single = lx.ParticleBeam.synthetic((1,), 150_001, seed=6, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3])
    shared = single.broadcast(shape)
    lx.config.lazy_broadcast = False
    try:
        repeated = single.broadcast(shape)
    finally:
        lx.config.lazy_broadcast = True
    assert shared.is_shared and not repeated.is_shared
    f = lambda v: np.full(shape, v, dtype)  # noqa: E731
    seg = lx.Segment([lx.Drift(f(0.3)), lx.Quadrupole(f(0.2), k1=np.linspace(-5, 5, 8).astype(dtype)), lx.Drift(f(0.4))])
    a, b = seg.track(shared), seg.track(repeated)
    assert not a.is_shared
    assert np.array_equal(np.asarray(a.particles), np.asarray(b.particles))
    assert np.array_equal(a.moment_record(), b.moment_record(), equal_nan=True)


@pytest.mark.parametrize("packed", [0, 1])
def test_device_phase_trig_accuracy(lx, packed):
    """
    The cavity kick's float32 cos/sin on the device (lynx_device.hpp: Cody-Waite + minimax up to
    |x| = 1000, library path beyond) against float64: within 2 ulp of the correctly rounded
    value and 1.2e-7 absolute -- the class of NumPy's float32 cos (the oracle's), so the choice of
    implementation does not show in the 1e-4 moment tolerance; special values as the library's.
    """
    import ctypes as C

    from lynx_amd.device import get_runtime

    rt = get_runtime()
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-1, 1, 200_000), rng.uniform(-30, 30, 200_000), rng.uniform(-1000, 1000, 200_000),
                        rng.uniform(-2e6, 2e6, 100_000), np.array([0.0, -0.0, 1000.0, -1000.0, 1000.0001, 841226.0]),
                        np.arange(-40, 41) * (np.pi / 4)]).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    xs = np.concatenate([x, special, special[:1]])  # odd length too
    d_x, d_s, d_c = rt.to_device(xs), rt.empty(xs.shape, np.float32), rt.empty(xs.shape, np.float32)
    rt.check(rt.lib.lynx_diag_phase_trig(rt.ctx, xs.size, C.c_void_p(d_x.ptr), packed, C.c_void_p(d_s.ptr), C.c_void_p(d_c.ptr)))
    s, c = d_s.numpy(), d_c.numpy()
    assert np.all(np.isnan(s[x.size:])) and np.all(np.isnan(c[x.size:]))
    x64 = x.astype(np.float64)
    for got, ref in ((c[: x.size], np.cos(x64)), (s[: x.size], np.sin(x64))):
        err = np.abs(got.astype(np.float64) - ref)
        assert err.max() < 1.2e-7, err.max()
        ulp = np.spacing(np.maximum(np.abs(ref), 1e-3).astype(np.float32)).astype(np.float64)  # relative, away from zeros
        assert (err / ulp).max() < 2.0, (err / ulp).max()
    # the forward kernels' cosine (one half-period polynomial): the kick is DKICK (cos(a) - cos(phi)), a difference
    # of numbers of order one, so what counts is the ABSOLUTE error: one float32 ulp of 1
    rt.check(rt.lib.lynx_diag_phase_trig(rt.ctx, xs.size, C.c_void_p(d_x.ptr), packed | 2, C.c_void_p(d_s.ptr), C.c_void_p(d_c.ptr)))
    c = d_c.numpy()
    assert np.all(np.isnan(c[x.size:]))
    err = np.abs(c[: x.size].astype(np.float64) - np.cos(x64))
    # up to pi/2 (no reduction: where cavity phases live) the polynomial's own 7.5e-8; beyond, the reduced argument
    # -- up to pi/2 in size -- is itself rounded to float32, which adds up to 6e-8 sin(r)
    assert err[np.abs(x64) <= np.pi / 2].max() < 8e-8, err[np.abs(x64) <= np.pi / 2].max()
    assert err.max() < 1.35e-7, err.max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("batch,cells", [(1, 3), (3, 3), (1, 40)])
def test_the_parameters_of_small_lattices_travel_in_the_kernel_arguments(lx, dtype, batch, cells, monkeypatch):
    """
    InlinePool (lynx_device.hpp): the parameter pool of a small lattice without cavities (up to 256 bytes, or up to
    1 KB) is passed to the one-workgroup-per-sample kernels by value; a parameter write then is a memcpy on the host,
    and the pool in HBM follows when a kernel that reads it from there is next launched.
    (batch, cells) = (1, 3): the small size; (3, 3): the large one; (1, 40): 160 elements, too many -- from memory.
    Same arithmetic as from memory (LYNX_INLINE_POOL=0): the same bits, for a ParticleBeam and a ParameterBeam; a
    parameter written between two calls reaches both forms, and the reverse pass -- which reads the parameters from
    HBM -- right behind a write.
    """
    import lynx_amd.grad as grad

    B = batch
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    rng = np.random.default_rng(31)
    k1 = rng.uniform(-4, 4, (cells, B)).astype(dtype)
    k1_new = rng.uniform(-4, 4, B).astype(dtype)

    def segment(first_k1):
        els = []
        for c in range(cells):
            els += [lx.Drift(f(0.3), dtype=dtype), lx.Quadrupole(f(0.2), k1=first_k1 if c == 0 else k1[c], dtype=dtype, name=f"Q{c}"),
                    lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=dtype), lx.Marker(name=f"M{c}")]
        return lx.Segment(els)

    P = o.gaussian_particles((B,), 3001, seed=7, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    energy = f(1e8)
    pbeam = lx.ParameterBeam.from_parameters(energy=energy, dtype=dtype) if B == 1 else None

    def results(seg):
        out = seg.track(lx.ParticleBeam(P, energy, dtype=dtype))
        res = [np.asarray(out.particles), out.moment_record().copy()]
        if pbeam is not None:
            pb = seg.track(pbeam)
            res += [np.asarray(pb._mu), np.asarray(pb._cov)]
        return res

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    seg = segment(k1[0])
    first = results(seg)
    seg.Q0.k1 = k1_new  # a write between two calls ...
    second = results(seg)
    assert not np.array_equal(first[0], second[0])
    assert same(second, results(segment(k1_new)))  # ... is what a new segment with that value gives
    vjp = grad.track_vjp(seg, lx.ParticleBeam(P, energy, dtype=dtype))  # the reverse pass right behind a write
    g = vjp(cov_bar=np.broadcast_to(np.eye(6), (B, 6, 6)).copy())
    seg.Q0.k1 = k1[0]
    seg.Q0.k1 = k1_new  # (two writes, none of them followed by a forward call)
    fresh = segment(k1_new)
    g_fresh = grad.track_vjp(fresh, lx.ParticleBeam(P, energy, dtype=dtype))(cov_bar=np.broadcast_to(np.eye(6), (B, 6, 6)).copy())
    assert np.array_equal(np.asarray(g[seg.Q0]["k1"]), np.asarray(g_fresh[fresh.Q0]["k1"]))
    g_again = grad.track_vjp(seg, lx.ParticleBeam(P, energy, dtype=dtype))(cov_bar=np.broadcast_to(np.eye(6), (B, 6, 6)).copy())
    assert np.array_equal(np.asarray(g[seg.Q0]["k1"]), np.asarray(g_again[seg.Q0]["k1"]))
    monkeypatch.setenv("LYNX_INLINE_POOL", "0")  # everything from memory: the same bits
    seg_mem = segment(k1[0])
    assert same(first, results(seg_mem))
    seg_mem.Q0.k1 = k1_new
    assert same(second, results(seg_mem))
    g_mem = grad.track_vjp(seg_mem, lx.ParticleBeam(P, energy, dtype=dtype))(cov_bar=np.broadcast_to(np.eye(6), (B, 6, 6)).copy())
    assert np.array_equal(np.asarray(g[seg.Q0]["k1"]), np.asarray(g_mem[seg_mem.Q0]["k1"]))
    # and against the oracle
    specs = []
    for c in range(cells):
        specs += [o.Drift(f(0.3)), o.Quadrupole(f(0.2), k1=k1_new if c == 0 else k1[c]), o.HorizontalCorrector(f(0.1), angle=f(1e-4)), o.Marker()]
    ref = o.segment_track(specs, o.particle_beam(P, energy, dtype), dtype)
    for c in range(7):
        assert rel_err(second[0][..., c], ref["particles"][..., c]) < TOL_P[np.dtype(dtype).type], c


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_results_live_in_host_memory_the_gpu_writes_through(lx, dtype, monkeypatch):
    """
    The moment records of a few samples, and a small ParameterBeam's outgoing mu and cov, are allocated in host memory
    the GPU writes through (lynx_buf_alloc_result): reading them back is a wait for the stream and a memcpy, no copy
    command (BASELINE config 2 with sigma_x read after every call: 55 -> 43 us).  Same kernels, same numbers
    (LYNX_HOST_VISIBLE_RECORDS=0: device memory): bit for bit -- read back, fed into the next `track` (a chain of two
    segments), and read by the reverse pass.
    """
    import lynx_amd.grad as grad

    B = 3
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    rng = np.random.default_rng(5)
    k1 = rng.uniform(-4, 4, B).astype(dtype)
    P = o.gaussian_particles((B,), 5000, seed=3, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])

    def everything():
        quad = lx.Quadrupole(f(0.2), k1=k1, dtype=dtype)
        first = lx.Segment([lx.Drift(f(0.4), dtype=dtype), quad, lx.Drift(f(0.3), dtype=dtype)])
        second = lx.Segment([lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=dtype), lx.Drift(f(0.7), dtype=dtype)])
        beam = lx.ParticleBeam(P, f(1e8), dtype=dtype)
        out = second.track(first.track(beam))
        pb = second.track(first.track(lx.ParameterBeam.from_parameters(energy=f(1e8), sigma_x=f(1e-4), dtype=dtype)))
        g = grad.track_vjp(first, beam)(cov_bar=np.broadcast_to(np.eye(6), (B, 6, 6)).copy())
        return [np.asarray(out.particles), out.moment_record().copy(), np.asarray(out.sigma_x), np.asarray(pb._mu), np.asarray(pb._cov),
                np.asarray(g[quad]["k1"]), np.asarray(g.energy)]

    through = everything()
    again = everything()
    monkeypatch.setenv("LYNX_HOST_VISIBLE_RECORDS", "0")
    device = everything()
    for a, b, c in zip(through, again, device):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)


@pytest.mark.parametrize("dtype,n", [(np.float32, 40_000), (np.float32, 40_003), (np.float64, 20_001)])
def test_the_order_the_workgroups_walk_the_batch_in_changes_nothing(lx, dtype, n, monkeypatch):
    """
    Long calls (256 MB of particles and more) walk the batch forwards and backwards in turn, so that a pass over the
    same incoming beam starts with what the previous one left in the Infinity Cache (TrackArgs::reversed).  The same
    workgroups write the same particles and the same records: bit for bit (LYNX_ALTERNATE_ORDER=2 reverses every call,
    whatever its size; 0 never does).
    """
    B = 7
    scale = 0.5 + np.arange(B) / (B - 1)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(4):
        desc += [("quadrupole", dict(length=f(0.2), k1=4.2 * scale)), ("drift", dict(length=f(0.5))),
                 ("quadrupole", dict(length=f(0.2), k1=-4.2 * scale)), ("drift", dict(length=f(0.5)))]
    results = []
    for order in ("0", "2"):
        monkeypatch.setenv("LYNX_ALTERNATE_ORDER", order)
        out, ref = _particle_case(lx, desc, dtype, (B,), n, seed=4)
        results.append((np.asarray(out.particles), out.moment_record().copy()))
    _assert_moments(out, ref, dtype)
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1], equal_nan=True)


def test_attribute_writes_between_tracks_take_effect(lx):
    """
    README.md:60 pattern (`segment.AREAMQZM2.k1 = ...`): values, whole-batch predicates (tilt,
    misalignment: LYNX_FLAG_*) and structure (cavity switched on, BPM activated) written between
    two `track` calls of the same Segment must all reach the device-resident lattice program.
    """
    f = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    quad = lx.Quadrupole(f(0.2), k1=f(1.0), dtype=np.float64, name="Q")
    cav = lx.Cavity(f(1.0), voltage=f(0.0), phase=f(0.0), frequency=f(1.3e9), dtype=np.float64, name="C")
    seg = lx.Segment([lx.Drift(f(0.5), dtype=np.float64), quad, lx.Drift(f(0.3), dtype=np.float64)])
    P = o.gaussian_particles((1,), 3000, seed=5, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    beam = lx.ParticleBeam(P, f(6e6), dtype=np.float64)

    def reference(**kw):
        specs = [o.Drift(f(0.5)), o.Quadrupole(f(0.2), **kw), o.Drift(f(0.3))]
        return o.segment_track(specs, o.particle_beam(P, f(6e6), np.float64), np.float64)["particles"]

    assert np.allclose(np.asarray(seg.track(beam).particles), reference(k1=f(1.0)), rtol=1e-12, atol=1e-18)
    seg.Q.k1 = f(-3.0)  # value
    assert np.allclose(np.asarray(seg.track(beam).particles), reference(k1=f(-3.0)), rtol=1e-12, atol=1e-18)
    seg.Q.tilt = f(0.4)  # predicate: any(tilt != 0) switches the rotation on
    assert np.allclose(np.asarray(seg.track(beam).particles), reference(k1=f(-3.0), tilt=f(0.4)), rtol=1e-11, atol=1e-17)
    seg.Q.misalignment = np.array([[1e-4, -2e-4]])
    got = np.asarray(seg.track(beam).particles)
    assert np.allclose(got, reference(k1=f(-3.0), tilt=f(0.4), misalignment=np.array([[1e-4, -2e-4]])), rtol=1e-11, atol=1e-17)
    seg.Q.tilt = f(0.0)  # and off again
    seg.Q.misalignment = np.zeros((1, 2))
    assert np.allclose(np.asarray(seg.track(beam).particles), reference(k1=f(-3.0)), rtol=1e-12, atol=1e-18)
    # structure: a cavity that is switched on becomes a step of its own
    seg2 = lx.Segment([lx.Drift(f(0.5), dtype=np.float64), cav, lx.Drift(f(0.3), dtype=np.float64)])
    cav.voltage = f(1e6)
    on_first = np.asarray(seg2.track(beam).particles)
    cav.voltage = f(2e6)
    specs = [o.Drift(f(0.5)), o.Cavity(f(1.0), voltage=f(2e6), phase=f(0.0), frequency=f(1.3e9)), o.Drift(f(0.3))]
    ref = o.segment_track(specs, o.particle_beam(P, f(6e6), np.float64), np.float64)
    out = seg2.track(beam)
    assert np.allclose(np.asarray(out.particles), ref["particles"], rtol=1e-9, atol=1e-15) and not np.allclose(on_first, ref["particles"])
    assert np.allclose(out.energy, ref["energy"])
