"""
`Segment.track_along` on the GPU against the oracle's element-by-element chain -- the loop of the reference's
`plot_twiss` with every element tracked: `beam = o.element_track(spec, beam, dtype)` (a float32 active cavity by
`o.cavity_track(..., kick="product")`, the rule `tests/test_gpu_parity.py` documents in `_assert_moments`) and
`o.beam_moments(beam, ddof=1)` at EVERY point.  Tolerances are the project's own (TOL_MOM, TOL_P, TOL_KICK_F64).
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import MOMENT_KEYS, assert_parameter_beam, covariance_distances, make_lattice, moment_distances, rel_err
from .test_gpu_parity import KICK_MOMENTS, TOL_KICK_F64, TOL_MOM, TOL_P

pytestmark = pytest.mark.gpu

SIGMA = [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


def chain(specs, beam, dtype):
    """The beams at points 0 .. E, and (element index, stack([mu_x, mu_y])) of the beam entering every active BPM."""
    dtype = np.dtype(dtype)
    beams, readings = [beam], []
    for k, spec in enumerate(specs):
        if spec["kind"] == "cavity" and not o.is_skippable(spec) and dtype == np.float32:
            beam = o.cavity_track(spec, beam, dtype, kick="product")
        else:
            if spec["kind"] == "bpm" and spec.get("is_active"):
                m = o.beam_moments(beam)
                readings.append((k, np.stack([m["mu_x"], m["mu_y"]])))
            beam = o.element_track(spec, beam, dtype)
        beams.append(beam)
    return beams, readings


def upcast(desc):
    """The float32 lattice's own numbers in float64 (the float64 chain of a float32 case)."""
    up = lambda v: np.asarray(np.asarray(v, dtype=np.float32), dtype=np.float64) if isinstance(v, (np.ndarray, list, float)) else v  # noqa: E731
    return [(kind, {k: up(v) for k, v in kw.items()}) for kind, kw in desc]


def point(trace, k):
    return {key: getattr(trace, key)[..., k] for key in MOMENT_KEYS}


def nan_aware_distances(got, ref):
    """`moment_distances` where a moment may be NaN (N = 1: the unbiased sigma): the NaN patterns must be equal, and a mean
    whose sigma is NaN is measured in its own size."""
    out = {}
    for key in MOMENT_KEYS:
        g, r = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (key, g, r)
        if key.startswith("mu_"):
            s = np.abs(r) + np.nan_to_num(np.asarray(ref["sigma" + key[2:]], dtype=np.float64)) + 1e-300
        elif key in ("sigma_xxp", "sigma_yyp"):
            a, b = ("sigma_x", "sigma_xp") if key == "sigma_xxp" else ("sigma_y", "sigma_yp")
            s = np.nan_to_num(np.asarray(ref[a] * ref[b], dtype=np.float64)) + 1e-300
        else:
            s = np.abs(r) + 1e-300
        d = np.abs(g - r) / s
        out[key] = float(np.nanmax(d)) if not np.all(np.isnan(d)) else 0.0
    return out


def assert_trace(trace, beams, dtype, beams64=None, first_kick=None, n=None, nan_points=()):
    """Every moment at every point within TOL_MOM of the chain; float32 behind an active cavity: the moments the kick
    decides also within TOL_KICK_F64 of the float64 chain.  Where the reference itself returns NaN (N = 1: the unbiased
    sigma; `nan_points`: behind a cavity without voltage, whose map has NaN entries) the NaN patterns must be equal and
    every other moment is held to the same tolerance.  And ALL 36 entries of the biased covariance at every point
    (`trace.cov`, `at(k)["cov"]`) within TOL_MOM of the float64 numpy covariance of the chain's particles there, in units of
    sigma_i sigma_j (`covariance_distances`: NaN patterns equal; one particle: 0 exactly)."""
    dtype = np.dtype(dtype).type
    assert trace.num_points == len(beams)
    worst, worst_cov, cov = 0.0, (0.0, None), trace.cov
    assert cov.shape == (*trace.batch_shape, len(beams), 6, 6)
    for k, beam in enumerate(beams):
        d_cov, where = covariance_distances(cov[..., k, :, :], beam["particles"])
        worst_cov = max(worst_cov, (d_cov, (k, *where)), key=lambda v: v[0])
        assert d_cov <= TOL_MOM[dtype], ("cov", k, d_cov, where)
        assert np.array_equal(trace.at(k)["cov"], cov[..., k, :, :], equal_nan=True), k
        ref = o.beam_moments(beam, ddof=1)
        d = nan_aware_distances(point(trace, k), ref) if (n == 1 or k in nan_points) else moment_distances(point(trace, k), ref)
        worst = max(worst, max(d.values()))
        assert max(d.values()) <= TOL_MOM[dtype], (k, d)
        assert rel_err(trace.energy[..., k], beam["energy"]) < 1e-6, k
        if beams64 is not None and first_kick is not None and k > first_kick and n != 1:
            d64 = moment_distances(point(trace, k), o.beam_moments(beams64[k], ddof=1))
            assert max(d64[key] for key in KICK_MOMENTS) <= TOL_KICK_F64, (k, d64)
    print(f"trace {np.dtype(dtype).name}: worst moment distance over {len(beams)} points {worst:.2e}; worst covariance distance {worst_cov[0]:.2e} "
          f"at (point, i, j, sample) {worst_cov[1]}")
    return worst


def mixed_desc(shape, rng, dead_cavity=False):
    """
    Every element kind of ELEMENT_CASES' families in one lattice, parameters batched over `shape`.  `dead_cavity`: a
    cavity without voltage comes last -- the reference's map of it has NaN entries (cavity.py:262-264: Ep = 0, r12 =
    Ei / Ep sin(0)), so x and y of everything behind it are NaN there and here; at the end of the lattice every other
    point keeps its numbers.
    """
    f = lambda v: np.full(shape, v)  # noqa: E731
    tm = np.broadcast_to(np.eye(7), (*shape, 7, 7)).copy()
    tm[..., :6, :6] += rng.normal(0, 1e-2, (*shape, 6, 6))
    tm[..., :6, 6] = rng.normal(0, 1e-5, (*shape, 6))
    return [
        ("bpm", dict(is_active=False)),
        ("drift", dict(length=f(0.6))),
        ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, shape), tilt=rng.uniform(-1, 1, shape),
                            misalignment=rng.normal(0, 1e-4, (*shape, 2)))),
        ("bpm", dict(is_active=True)),
        ("hcor", dict(length=f(0.1), angle=rng.uniform(1e-4, 2e-3, shape))),
        ("dipole", dict(length=f(0.5), angle=np.linspace(0.1, 0.2, int(np.prod(shape))).reshape(shape), e1=f(0.05), e2=f(0.02),
                        fringe_integral=f(0.4), gap=f(0.02), tilt=f(0.1))),
        ("marker", {}),
        ("rbend", dict(length=f(0.3), angle=f(0.05), fringe_integral=f(0.3), fringe_integral_exit=f(0.1), gap=f(0.02))),
        ("vcor", dict(length=f(0.1), angle=rng.uniform(-2e-3, -1e-4, shape))),
        ("solenoid", dict(length=f(0.3), k=rng.uniform(-2, 2, shape), misalignment=rng.normal(0, 1e-4, (*shape, 2)))),
        ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, shape), phase=rng.uniform(-10, 10, shape),
                        frequency=f(1.3e9))),
        ("undulator", dict(length=f(0.25))),
        ("custom", dict(transfer_map=tm, length=f(0.4))),
        ("bpm", dict(is_active=True)),
        ("drift", dict(length=f(0.4))),
    ] + ([("cavity", dict(length=f(1.0), voltage=f(0.0), phase=f(1.0), frequency=f(1.3e9)))] if dead_cavity else [])


def correlated_particles(shape, n, seed, dtype):
    """
    `o.gaussian_particles` of SIGMA with every pair of coordinates correlated on the way in: correlation matrix
    0.5 I + 0.5 v v^T, v = (+, -, +, +, -, +) -- |rho| = 0.5 in all 15 off-diagonal slots, signs mixed -- and the SIGMA
    of the plain beam.  A covariance check downstream then sees no slot that is sampling noise alone.
    """
    v = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0])
    L = np.linalg.cholesky(0.5 * np.eye(6) + 0.5 * np.outer(v, v))
    P = o.gaussian_particles(shape, n, seed=seed, dtype=np.float64, sigma=[1.0] * 6)
    P[..., :6] = (P[..., :6] @ L.T) * np.array(SIGMA)
    return P.astype(dtype)


def coupled_desc(shape, rng):
    """
    Six elements that couple every pair of coordinates in every sample: drift, tilted misaligned quadrupole (x-y), tilted
    dipole (dispersion in both planes, the s row), solenoid (x-y once more), gaining cavity (s-delta), drift.  The
    strengths keep away from 0, so that no sample of a large batch is an uncoupled one; tests/test_covariance_check_host.py
    asserts the correlations from the oracle alone.  No BPM: a float32 `Segment.track` walks it as units.
    """
    f = lambda v: np.full(shape, v)  # noqa: E731
    away = lambda lo, hi: rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)  # noqa: E731
    return [
        ("drift", dict(length=f(0.6))),
        ("quadrupole", dict(length=f(0.2), k1=away(2, 5), tilt=away(0.3, 1.0), misalignment=rng.normal(0, 1e-4, (*shape, 2)))),
        ("dipole", dict(length=f(0.5), angle=rng.uniform(0.1, 0.2, shape), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4),
                        gap=f(0.02), tilt=f(0.3))),
        ("solenoid", dict(length=f(0.3), k=away(0.8, 2.0))),
        ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, shape), phase=rng.uniform(-10, 10, shape),
                        frequency=f(1.3e9))),
        ("drift", dict(length=f(0.4))),
    ]


TWISS_KEYS = ("emittance", "beta", "alpha", "normalized_emittance")


def assert_twiss(trace, beams, beams64, dtype):
    """
    emittance, beta, alpha and the normalised emittance of both planes at every point against `o.beam_moments(ddof=1)` of
    the FLOAT64 chain.  The emittance is sqrt(sigma^2 sigma'^2 (1 - rho^2)) and cancels as |rho| -> 1, so the bounds follow
    from the record's own tolerance d on sigma, sigma' (relative) and the covariance (in sigma sigma'), to first order:
    eps^2 = sigma^2 sigma'^2 - c^2 moves by <= (4 + 2 |rho|) d sigma^2 sigma'^2, so eps by <= 3 d / (1 - rho^2)
    relative; beta = sigma^2 / eps by <= 2 d + 3 d / (1 - rho^2); alpha = -c / eps by <= d / sqrt(1 - rho^2) +
    3 |alpha| d / (1 - rho^2).  Asserted: relative error of eps, eps_n and beta <= 5 d / (1 - rho^2), absolute error of
    alpha <= 5 d (1 + |alpha|) / (1 - rho^2), rho the reference's own correlation at the point.  float64: d = TOL_MOM;
    float32: d = TOL_MOM plus the distance, in those three moments, of the oracle's float32 chain from its float64 chain
    at the point.  Points where the reference is NaN (one particle; behind the dead cavity) are left out, no others.
    """
    dtype = np.dtype(dtype).type
    worst = {key: 0.0 for key in TWISS_KEYS}
    compared = 0
    for k, beam64 in enumerate(beams64):
        with np.errstate(all="ignore"):
            ref = o.beam_moments(beam64, ddof=1)
            own = o.beam_moments(beams[k], ddof=1)
        for plane, cross in (("x", "sigma_xxp"), ("y", "sigma_yyp")):
            sa, sb, c = (np.asarray(ref[key], dtype=np.float64) for key in ("sigma_" + plane, "sigma_" + plane + "p", cross))
            delta = np.full(sa.shape, TOL_MOM[dtype])
            if dtype == np.float32:
                with np.errstate(all="ignore"):
                    delta = delta + np.maximum.reduce([np.abs(own["sigma_" + plane] - sa) / sa, np.abs(own["sigma_" + plane + "p"] - sb) / sb,
                                                       np.abs(own[cross] - c) / (sa * sb)])
            with np.errstate(all="ignore"):
                one_minus_rho2 = 1.0 - (c / (sa * sb)) ** 2
            for key in TWISS_KEYS:
                want = np.asarray(ref[f"{key}_{plane}"], dtype=np.float64)
                got = np.asarray(getattr(trace, f"{key}_{plane}")[..., k], dtype=np.float64)
                use = ~np.isnan(want)
                assert not np.isnan(got[use]).any(), (key, plane, k, got, want)
                if not use.any():
                    continue
                compared += int(use.sum())
                bound = 5 * delta / one_minus_rho2 * ((1 + np.abs(want)) if key == "alpha" else np.abs(want))
                err = np.abs(got - want)
                worst[key] = max(worst[key], float(np.max(err[use] / bound[use])))
                assert np.all(err[use] <= bound[use]), (key, plane, k, got, want, bound)
    print(f"twiss: worst error in units of its bound {({key: round(v, 4) for key, v in worst.items()})}; {compared} values compared")
    return compared


# `mixed_desc` per batch shape: with these seeds every off-diagonal slot of the covariance has |correlation| >= 0.1 at some
# point in every sample, for every n below (asserted from the oracle alone in tests/test_covariance_check_host.py)
LATTICE_SEED = {(3,): 21, (2, 2): 23}


def every_element_kind_case(dtype, shape, n):
    desc = mixed_desc(shape, np.random.default_rng(LATTICE_SEED[shape]), dead_cavity=True)
    P = o.gaussian_particles(shape, n, seed=3 + n, dtype=dtype, sigma=SIGMA)
    return desc, P, np.full(shape, 1e8, dtype=dtype)


@pytest.mark.parametrize("n", [1, 63, 64, 1000, 70_001])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_element_kind_at_every_point(lx, dtype, shape, n):
    """n = 70 001 is 274 tiles (float32) / 547 (float64); a batch of 3 or 4 caps the waves per sample at 1024 / 768, so
    there are as many waves as tiles (rounded up to 276 / 548), more than 256: those cases, of both shapes, take
    `k_trace_finalize<T, 1024>`; every other one takes `k_trace_finalize<T, 256>`."""
    every_element_kind(lx, dtype, shape, n)


@pytest.mark.parametrize("dtype,n", [(np.float32, 255), (np.float32, 256), (np.float32, 257),
                                     (np.float64, 127), (np.float64, 128), (np.float64, 129)])
def test_every_element_kind_at_the_tile_edges_of_the_plain_trace(lx, dtype, n):
    """A tile of `track_particles_along_t` is 64 U particles, U = 4 (float32) / 2 (float64): one particle short of a full
    tile, a full tile, and a second tile (a second wave) of one particle."""
    every_element_kind(lx, dtype, (3,), n)


def every_element_kind(lx, dtype, shape, n):
    desc, P, energy = every_element_kind_case(dtype, shape, n)
    elements, specs = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    trace = segment.track_along(lx.ParticleBeam(P, energy, dtype=dtype))
    beams, readings = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    beams64 = None
    if dtype == np.float32:
        _, specs64 = make_lattice(upcast(desc), np.float64)
        beams64, _ = chain(specs64, o.particle_beam(P.astype(np.float64), energy.astype(np.float64), np.float64), np.float64)
    first_kick = [k for k, (kind, kw) in enumerate(desc) if kind == "cavity" and np.any(kw["voltage"] != 0)][0]
    assert_trace(trace, beams, dtype, beams64, first_kick, n, nan_points=(len(desc),))
    compared = assert_twiss(trace, beams, beams if beams64 is None else beams64, dtype)
    assert compared == (0 if n == 1 else 8 * len(desc) * int(np.prod(shape)))  # (every point but the one behind the dead cavity)
    assert np.isnan(trace.mu_x[..., -1]).all() and not np.isnan(trace.records[..., :-1, :]).any()
    assert trace.s.shape == (len(desc) + 1, *shape) and trace.mu.shape == (*shape, len(desc) + 1, 6)
    assert trace.beta_x.shape == (*shape, len(desc) + 1) and trace.num_particles == n
    # the tracked beam: particles, energy, and its moments are the last point's record (no further pass)
    got = np.asarray(trace.outgoing.particles)
    for c in range(7):  # (x and y: NaN in both, see mixed_desc)
        assert rel_err(got[..., c], beams[-1]["particles"][..., c]) < TOL_P[dtype], c
    assert rel_err(trace.outgoing.energy, beams[-1]["energy"]) < 1e-6
    assert np.array_equal(trace.outgoing.moment_record(covariance=True), trace.records[..., -1, :], equal_nan=True)
    # an active BPM reads the beam that enters it
    assert len(readings) == 2
    sig_x = float(np.std(P[..., 0])) + 1e-4
    for k, want in readings:
        have = elements[k].reading
        assert have.shape == (2, *shape) and have.dtype == np.dtype(dtype)
        assert np.all(np.abs(have - want) <= TOL_MOM[dtype] * (np.abs(want) + 3 * sig_x)), (k, have, want)
    assert elements[0].reading is None


def two_tiles_per_wave_case(dtype, shared):
    shape, n = (300,), {np.float32: 4097, np.float64: 2049}[np.dtype(dtype).type]
    desc = coupled_desc(shape, np.random.default_rng(22))
    P = correlated_particles((1,) if shared else shape, n, seed=3 + n, dtype=dtype)
    return desc, P, np.full(shape, 1e8, dtype=dtype)


@pytest.mark.parametrize("dtype,shared", [(np.float32, False), (np.float64, False), (np.float32, True)])
def test_two_tiles_per_wave_and_waves_without_a_tile(lx, dtype, shared):
    """
    `track_particles_along_t` with 256 CUs and a batch of 300: the cap is ceil(256 * 12 / 300) = 11 waves per sample; n =
    4097 (float32, tiles of 256) / 2049 (float64, tiles of 128) is 17 tiles, so tiles_per_wave = ceil(17 / 11) = 2, nine
    waves own tiles -- the ninth one tile, of one particle -- and the launch is rounded up to 12 waves: three own none.
    That is the `first ? 0 : *cell` accumulation of `trace_deposit` over a wave's second tile, and the empty slabs in
    front of `k_trace_finalize<T, 256>`.  (Another CU count changes the cap: ceil(12 cus / 300) must stay in 9 .. 16 for
    two tiles per wave.)  The lattice couples every pair of coordinates; `shared`: one incoming beam for the batch.
    """
    desc, P, energy = two_tiles_per_wave_case(dtype, shared)
    shape, n = energy.shape, P.shape[-2]
    assert -(-n // (64 * (4 if dtype == np.float32 else 2))) == 17
    elements, specs = make_lattice(desc, dtype, lx)
    if shared:
        beam = lx.ParticleBeam(P, energy[:1], dtype=dtype).broadcast(shape)
        assert beam.is_shared
        P = np.ascontiguousarray(np.broadcast_to(P, (*shape, n, 7)))
    else:
        beam = lx.ParticleBeam(P, energy, dtype=dtype)
    trace = lx.Segment(elements).track_along(beam)
    beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    assert trace.num_points == 7 and trace.num_particles == n
    assert_trace(trace, beams, dtype)
    got = np.asarray(trace.outgoing.particles)
    for c in range(7):
        assert rel_err(got[..., c], beams[-1]["particles"][..., c]) < TOL_P[dtype], c
    assert np.array_equal(trace.outgoing.moment_record(covariance=True), trace.records[..., -1, :])


def test_a_centroid_that_moves_keeps_float32_variances(lx):
    """Correctors of 3 mrad and a 1 mm-misaligned quadrupole over 10 m: the centroid ends a centimetre -- a hundred of the
    incoming sigma_x -- from where it started; the sums of every point are taken about a reference point that moves with
    it (about a fixed one the float32 products x^2 ~ 1e-4 would carry the variance ~ 1e-8 in their last two digits)."""
    dtype, B = np.float32, 2
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(1.0))), ("hcor", dict(length=f(0.2), angle=f(3e-3))), ("drift", dict(length=f(2.0))),
            ("quadrupole", dict(length=f(0.3), k1=f(2.0), misalignment=np.tile([1e-3, -1e-3], (B, 1)))),
            ("drift", dict(length=f(2.5))), ("vcor", dict(length=f(0.2), angle=f(-3e-3))), ("drift", dict(length=f(2.0))),
            ("hcor", dict(length=f(0.2), angle=f(3e-3))), ("drift", dict(length=f(1.6)))]
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles((B,), 50_000, seed=8, dtype=dtype, sigma=SIGMA)
    energy = f(1e8).astype(dtype)
    trace = lx.Segment(elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype), keep_outgoing=False)
    beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    assert np.all(np.abs(trace.mu_x[..., -1]) > 90 * trace.sigma_x[..., 0])  # it did move
    assert np.isclose(np.asarray(trace.s[-1], dtype=np.float64), 10.0, rtol=1e-6).all()
    assert_trace(trace, beams, dtype)
    assert trace.outgoing is None


def test_fodo_128_elements_shared_beam_k1_scan(lx):
    """o.fodo_segment(32), float32, batch 8 with a k1_scale scan, 100 000 particles, one incoming beam shared by the
    batch.  The oracle's own float32 chain stays within 2.2e-5 (moments) / 2.1e-5 (beta, emittance) of its float64 chain
    on this lattice; beta_x, beta_y of the trace are held to 1e-4 relative against the float64 chain as well."""
    dtype, B, N = np.float32, 8, 100_000
    scale = np.linspace(0.6, 1.1, B).astype(dtype)
    specs = o.fodo_segment(32, dtype=dtype, batch_shape=(B,), k1_scale=scale)
    specs64 = o.fodo_segment(32, dtype=np.float64, batch_shape=(B,), k1_scale=scale.astype(np.float64))
    for s32, s64 in zip(specs, specs64):  # the float32 lattice's own numbers
        for key in ("length", "k1"):
            if s32.get(key) is not None:
                s64[key] = np.asarray(s32[key], dtype=np.float32).astype(np.float64)
    elements = [lx.Quadrupole(s["length"], k1=s["k1"], dtype=dtype) if s["kind"] == "quadrupole" else lx.Drift(s["length"], dtype=dtype)
                for s in specs]
    one = o.gaussian_particles((1,), N, seed=4, dtype=dtype, sigma=SIGMA)
    beam = lx.ParticleBeam(one, np.array([1e8], dtype=dtype), dtype=dtype).broadcast((B,))
    assert beam.is_shared
    trace = lx.Segment(elements).track_along(beam)
    P = np.ascontiguousarray(np.broadcast_to(one, (B, N, 7)))
    energy = np.full(B, 1e8, dtype=dtype)
    beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    beams64, _ = chain(specs64, o.particle_beam(P.astype(np.float64), energy.astype(np.float64), np.float64), np.float64)
    assert trace.num_points == 129
    assert_trace(trace, beams, dtype)
    worst = 0.0
    for k, b64 in enumerate(beams64):
        m = o.beam_moments(b64, ddof=1)
        for key in ("beta_x", "beta_y"):
            err = float(np.max(np.abs(getattr(trace, key)[:, k] / m[key] - 1.0)))
            worst = max(worst, err)
            assert err <= 1e-4, (key, k, err)
    print(f"fodo trace: worst relative difference of beta against the float64 chain {worst:.2e}")
    got = np.asarray(trace.outgoing.particles)
    for c in range(7):
        assert rel_err(got[..., c], beams[-1]["particles"][..., c]) < TOL_P[dtype], c


def test_three_hundred_elements_and_twelve_active_bpms(lx):
    """More steps than the workgroup build's table, the reverse pass (64) or the observer table (8) hold."""
    dtype, B = np.float64, 2
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for cell in range(72):
        desc += [("quadrupole", dict(length=f(0.2), k1=f(4.2) * np.array([1.0, 0.9]))), ("drift", dict(length=f(0.5))),
                 ("quadrupole", dict(length=f(0.2), k1=f(-4.2) * np.array([1.0, 0.9]))), ("drift", dict(length=f(0.5)))]
        if cell % 6 == 0:
            desc.append(("bpm", dict(is_active=True)))
    assert len(desc) == 300 and sum(kind == "bpm" for kind, _ in desc) == 12
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles((B,), 5000, seed=9, dtype=dtype, sigma=SIGMA, mu=[2e-4, 0, -1e-4, 0, 0, 0])
    energy = f(1e8)
    trace = lx.Segment(elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype))
    beams, readings = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    assert trace.num_points == 301 and len(readings) == 12
    assert_trace(trace, beams, dtype)
    for k, want in readings:
        assert np.all(np.abs(elements[k].reading - want) <= TOL_MOM[dtype] * (np.abs(want) + 3e-4)), k
    got = np.asarray(trace.outgoing.particles)
    for c in range(7):
        assert rel_err(got[..., c], beams[-1]["particles"][..., c]) < TOL_P[dtype], c


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameter_beam_trace_through_cavities(lx, dtype):
    B = 3
    rng = np.random.default_rng(9)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                            frequency=f(1.3e9))),
            ("bpm", dict(is_active=True)),
            ("drift", dict(length=f(0.4))), ("hcor", dict(length=f(0.1), angle=f(1e-4))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=f(0.0), frequency=f(1.3e9))),
            ("dipole", dict(length=f(0.5), angle=f(0.1)))]
    elements, specs = make_lattice(desc, dtype, lx)
    kw = dict(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), sigma_s=f(1e-5),
              sigma_p=f(1e-3), mu_x=rng.normal(0, 1e-4, B), energy=f(6e6))
    kw = {k: np.asarray(v, dtype=dtype) for k, v in kw.items()}
    trace = lx.Segment(elements).track_along(lx.ParameterBeam.from_parameters(**kw, dtype=dtype))
    beams, readings = chain(specs, o.parameter_beam_from_parameters(dtype=dtype, **kw), dtype)
    tol = 1e-4 if dtype == np.float32 else 1e-9  # (test_parameter_beam_through_mixed_lattice's)
    assert trace.num_points == len(beams)
    for k, ref in enumerate(beams):
        assert_parameter_beam((trace._mu[..., k, :], trace._cov[..., k, :, :]), ref, tol, f"point {k}")
        assert rel_err(trace.energy[..., k], ref["energy"]) < 1e-6, k
    assert_parameter_beam(trace.outgoing, beams[-1], tol, "outgoing")
    assert np.allclose(elements[3].reading, readings[0][1], rtol=tol, atol=tol * 1e-4)
    assert trace.sigma_x.shape == (B, len(beams)) and trace.beta_y.shape == (B, len(beams))


@pytest.mark.parametrize("B", [1, 64, 65])
def test_parameter_beam_trace_through_cavities_lanes_form(lx, B, monkeypatch):
    """
    The lattice and beam of `test_parameter_beam_trace_through_cavities`, float32, lanes = samples at any batch
    (LYNX_LANES_BUILD_MIN_BATCH=1: k_trace_moments_lanes, cavity branch included): one live lane, a full wave, a second
    wave of one live lane and 63 clamped ones.  Every point against the oracle chain, and the last point against
    `Segment.track` under the same knob (k_apply_moments_lanes: the same step function, moment_step_lanes).  The two are
    not the same bits, before the step function was shared or after: `track` composes [drift, quadrupole] and
    [drift, corrector] into one table row each, the trace keeps a row per element.  On the commit before the shared
    function, on an MI355X: mean 3.6e-12 / 1.5e-11 / 7.3e-12, covariance 5.2e-6 / 1.5e-5 / 6.7e-6 of sigma_i sigma_j at
    batch 1 / 64 / 65 -- so the limits are those of `test_parameter_beam_lanes_path_agrees_with_the_workgroup_path`.
    """
    monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", "1")
    dtype = np.float32
    rng = np.random.default_rng(9)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, B))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                            frequency=f(1.3e9))),
            ("bpm", dict(is_active=True)),
            ("drift", dict(length=f(0.4))), ("hcor", dict(length=f(0.1), angle=f(1e-4))),
            ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=f(0.0), frequency=f(1.3e9))),
            ("dipole", dict(length=f(0.5), angle=f(0.1)))]
    elements, specs = make_lattice(desc, dtype, lx)
    kw = dict(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), sigma_s=f(1e-5),
              sigma_p=f(1e-3), mu_x=rng.normal(0, 1e-4, B), energy=f(6e6))
    kw = {k: np.asarray(v, dtype=dtype) for k, v in kw.items()}
    segment = lx.Segment(elements)
    trace = segment.track_along(lx.ParameterBeam.from_parameters(**kw, dtype=dtype))
    beams, _ = chain(specs, o.parameter_beam_from_parameters(dtype=dtype, **kw), dtype)
    assert trace.num_points == len(beams) and trace.mu.shape == (B, len(beams), 6)
    for k, ref in enumerate(beams):
        assert_parameter_beam((trace._mu[..., k, :], trace._cov[..., k, :, :]), ref, 1e-4, f"point {k}")
        assert rel_err(trace.energy[..., k], ref["energy"]) < 1e-6, k
    out = segment.track(lx.ParameterBeam.from_parameters(**kw, dtype=dtype))
    mu, cov = np.array(out._mu), np.array(out._cov)
    last_mu, last_cov = np.asarray(trace._mu[..., -1, :]), np.asarray(trace._cov[..., -1, :, :])
    sc = np.sqrt(np.abs(np.einsum("bii,bjj->bij", cov[..., :6, :6], cov[..., :6, :6]))) + 1e-300
    d_mu, d_cov = rel_err(last_mu, mu), float(np.max(np.abs(last_cov[..., :6, :6] - cov[..., :6, :6]) / sc))
    print(f"lanes trace, batch {B}: last point against Segment.track: equal bits {np.array_equal(last_mu, mu)} (mu) "
          f"{np.array_equal(last_cov, cov)} (cov), distances {d_mu:.2e} (mu) {d_cov:.2e} (cov)")
    assert d_mu < 1e-5 and d_cov < 1e-4


@pytest.mark.parametrize("B", [3, 100_000])
def test_parameter_beam_trace_on_the_ares_segment(lx, B):
    """Batch 3: one wave per sample; batch 100 000: lanes = samples."""
    dtype = np.float32
    specs = o.ares_like_segment(dtype, (B,))
    specs[4]["angle"] = np.linspace(1e-3, 4e-3, B).astype(dtype)
    ctor = {"bpm": lambda s: lx.BPM(), "drift": lambda s: lx.Drift(s["length"], dtype=dtype),
            "vcor": lambda s: lx.VerticalCorrector(s["length"], angle=s["angle"], dtype=dtype),
            "hcor": lambda s: lx.HorizontalCorrector(s["length"], angle=s["angle"], dtype=dtype)}
    elements = [ctor[s["kind"]](s) for s in specs]
    kw = dict(sigma_x=np.full(B, 1e-4, dtype), sigma_xp=np.full(B, 1e-5, dtype), energy=np.full(B, 1e8, dtype))
    trace = lx.Segment(elements).track_along(lx.ParameterBeam.from_parameters(**kw, dtype=dtype))
    beams, _ = chain(specs, o.parameter_beam_from_parameters(dtype=dtype, **kw), dtype)
    assert trace.num_points == 12 and trace.mu.shape == (B, 12, 6)
    for k, ref in enumerate(beams):
        assert_parameter_beam((trace._mu[..., k, :], trace._cov[..., k, :, :]), ref, 1e-4, f"point {k}")
        assert np.array_equal(trace.energy[..., k], ref["energy"])


def _small_case(lx, dtype, seed=5, n=20_000, B=3):
    desc = mixed_desc((B,), np.random.default_rng(seed))
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles((B,), n, seed=seed, dtype=dtype, sigma=SIGMA)
    return desc, elements, specs, P, np.full(B, 1e8, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_last_point_is_segment_track_and_a_trace_repeats_bit_for_bit(lx, dtype):
    desc, elements, specs, P, energy = _small_case(lx, dtype)
    segment = lx.Segment(elements)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    first = segment.track_along(beam)
    again = segment.track_along(beam)
    assert np.array_equal(first.records, again.records, equal_nan=True) and np.array_equal(first.energy, again.energy)
    assert np.array_equal(np.asarray(first.outgoing.particles), np.asarray(again.outgoing.particles))
    out = segment.track(beam)  # composed runs: the same algebra, rounded differently
    other = lx.Segment([lx.Drift(np.full(3, 0.3, dtype), dtype=dtype)]).track(beam)
    assert other.sigma_x.shape == (3,)
    third = segment.track_along(beam)
    assert np.array_equal(first.records, third.records, equal_nan=True)
    d = moment_distances(point(first, -1), out, scale=point(first, -1))
    assert max(d.values()) <= TOL_MOM[dtype], d
    assert rel_err(first.energy[..., -1], out.energy) < 1e-6
    moments_only = segment.track_along(beam, keep_outgoing=False)
    assert moments_only.outgoing is None
    assert np.array_equal(first.records, moments_only.records, equal_nan=True)
    assert np.array_equal(first.energy, moments_only.energy)


def test_a_parameter_write_between_two_traces(lx):
    """The optimisation loop: trace, change a magnet, trace -- exactly the trace of a freshly built segment."""
    dtype = np.float32
    desc, elements, specs, P, energy = _small_case(lx, dtype)
    segment = lx.Segment(elements)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    before = segment.track_along(beam)
    new_k1 = np.array([1.5, -2.5, 3.5], dtype=dtype)
    elements[2].k1 = new_k1
    after = segment.track_along(beam)
    assert not np.array_equal(before.records, after.records)
    assert np.array_equal(before.records[..., :2, :], after.records[..., :2, :])  # nothing in front of the magnet moved
    desc[2][1]["k1"] = new_k1
    fresh_elements, _ = make_lattice(desc, dtype, lx)
    fresh = lx.Segment(fresh_elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype))
    assert np.array_equal(after.records, fresh.records, equal_nan=True)
    assert np.array_equal(np.asarray(after.outgoing.particles), np.asarray(fresh.outgoing.particles))


def test_a_trace_leaves_the_reverse_pass_alone(lx):
    """`grad.track_vjp` reads the forward call's step table; a trace in between writes caller memory and builds a table
    of its own -- the gradients before and after it are equal bit for bit."""
    dtype, B = np.float64, 2
    f = lambda v: np.full(B, v)  # noqa: E731
    quad = lx.Quadrupole(f(0.2), k1=np.array([4.2, -3.0]), dtype=dtype)
    cavity = lx.Cavity(f(1.0377), voltage=f(1.8e7), phase=f(3.0), frequency=f(1.3e9), dtype=dtype)
    segment = lx.Segment([lx.Drift(f(0.5), dtype=dtype), quad, lx.Drift(f(0.3), dtype=dtype), cavity, lx.Drift(f(0.4), dtype=dtype)])
    P = o.gaussian_particles((B,), 4000, seed=2, dtype=dtype, sigma=SIGMA)
    beam = lx.ParticleBeam(P, f(6e6), dtype=dtype)
    from lynx_amd import grad

    vjp = grad.track_vjp(segment, beam)
    one = np.ones(B)
    g0 = vjp(sigma_x=one, sigma_p=one)
    before = (g0[quad]["k1"].copy(), g0[cavity]["voltage"].copy(), np.array(g0.energy))
    trace = segment.track_along(beam)
    assert trace.num_points == 6
    g1 = vjp(sigma_x=one, sigma_p=one)
    after = (g1[quad]["k1"], g1[cavity]["voltage"], np.array(g1.energy))
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    again = grad.track_vjp(segment, beam)(sigma_x=one, sigma_p=one)
    assert np.array_equal(again[quad]["k1"], before[0]) and np.array_equal(np.array(again.energy), before[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_beam_without_batch_dimensions(lx, dtype):
    """Batch shape (): one beam, element parameters as 0-d arrays; every array of the trace loses the batch axes."""
    a = lambda v: np.asarray(v, dtype=dtype)  # noqa: E731
    desc = [("drift", dict(length=a(0.6))), ("quadrupole", dict(length=a(0.2), k1=a(3.1))), ("hcor", dict(length=a(0.1), angle=a(1e-3))),
            ("marker", {}), ("drift", dict(length=a(1.4)))]
    elements, specs = make_lattice(desc, dtype, lx)
    P = o.gaussian_particles((), 3000, seed=6, dtype=dtype, sigma=SIGMA)
    energy = a(1e8)
    trace = lx.Segment(elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype))
    beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
    assert trace.batch_shape == () and trace.s.shape == (6,) and trace.mu.shape == (6, 6) and trace.cov.shape == (6, 6, 6)
    assert trace.energy.shape == (6,) and trace.beta_x.shape == (6,)
    assert_trace(trace, beams, dtype)
    assert np.asarray(trace.outgoing.particles).shape == (3000, 7)
    pb = lx.ParameterBeam.from_parameters(sigma_x=a(1e-4), sigma_xp=a(1e-5), energy=a(1e8), dtype=dtype)
    ptrace = lx.Segment(elements).track_along(pb)
    pbeams, _ = chain(specs, o.parameter_beam_from_parameters(dtype=dtype, sigma_x=a(1e-4), sigma_xp=a(1e-5), energy=a(1e8)), dtype)
    assert ptrace.mu.shape == (6, 6) and ptrace.sigma_x.shape == (6,)
    for k, ref in enumerate(pbeams):
        assert_parameter_beam((ptrace._mu[..., k, :], ptrace._cov[..., k, :, :]), ref, 1e-4 if dtype == np.float32 else 1e-9, f"point {k}")
