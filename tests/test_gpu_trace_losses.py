"""
`Segment.track_along(..., losses=...)` on the GPU: active apertures inside the beam trace.

The expectation is built here from the oracle: `o.element_track` element by element on the float64 and on the
lattice-dtype chain (the chain of `tests/test_gpu_trace.py`; an aperture leaves the particle array alone),
`o.aperture_mask` on the lattice-dtype chain at every aperture, a boolean mask carried instead of compaction, moments
over the survivors.

Mask parity: a particle is ON THE EDGE of an aperture if the float64 chain puts its normalised criterion -- |x| / x_max,
|y| / y_max, or the ellipse sum -- within EDGE[dtype] of 1; `lost_at` must equal the oracle's for every particle that
is on no edge.  The inputs are held to: no edge particle at all for n <= 1000 and for float64, at most 1e-3 n per sample
and aperture above that -- asserted from the oracle alone, before the GPU result is looked at (the seeds of SEEDS were
picked so).  The moments are then compared with the oracle's moments over the survivor set `lost_at` gives, at the
tolerances of the plain trace (TOL_MOM, TOL_KICK_F64), and `num_survivors` with that set's counts, exactly; so are all
36 entries of the biased covariance at every point, with the float64 numpy covariance of that survivor set.
"""

import warnings

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import MOMENT_KEYS, biased_covariance, build, covariance_distances, criterion, make_lattice, moment_distances, rel_err
from .test_gpu_parity import KICK_MOMENTS, TOL_KICK_F64, TOL_MOM
from .test_gpu_trace import SIGMA, chain, correlated_particles, point, upcast

pytestmark = pytest.mark.gpu

EDGE = {np.float32: 1e-4, np.float64: 1e-9}
# gaussian_particles seeds per n for which the float32 cases with n <= 1000 have no particle on an edge (searched on the
# host with `expectation` alone: the condition is asserted in every case before the GPU result is looked at)
SEEDS = {1: 0, 63: 0, 64: 0, 127: 0, 128: 0, 129: 0, 255: 0, 256: 0, 257: 2, 1000: 5, 2049: 0, 70_001: 0}
SEEDS_COUPLED = {129: 0, 257: 0, 1000: 0}  # `correlated_particles` seeds of variant "c", searched the same way


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


# ---------------------------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------------------------


def expectation(desc, P, energy, dtype):
    """
    From the oracle alone: the beams of the lattice-dtype chain at every point (all N particles, lost ones carried along),
    those of the float64 chain of the same numbers, `lost_at` (*batch, N), the particles on an edge (*batch, N) bool, and
    the number of them per aperture and sample (A, *batch).
    """
    dtype = np.dtype(dtype)
    _, specs = build(desc, dtype)
    with np.errstate(all="ignore"):
        beams, _ = chain(specs, o.particle_beam(P, energy, dtype), dtype)
        beams64 = beams
        if dtype == np.float32:  # the float32 lattice's own numbers in float64
            _, specs64 = build(upcast(desc), np.float64)
            beams64, _ = chain(specs64, o.particle_beam(P.astype(np.float64), np.asarray(energy, dtype=np.float64), np.float64), np.float64)
    alive = np.ones(P.shape[:-1], dtype=bool)
    lost_at = np.full(P.shape[:-1], -1, dtype=np.int32)
    on_edge = np.zeros(P.shape[:-1], dtype=bool)
    per_aperture = []
    apertures = [k for k, (kind, kw) in enumerate(desc) if kind == "aperture" and kw.get("is_active", True)]
    for ordinal, k in enumerate(apertures):
        kw = desc[k][1]
        x_max, y_max = np.asarray(kw["x_max"], dtype=dtype), np.asarray(kw["y_max"], dtype=dtype)
        keep = o.aperture_mask(beams[k]["particles"], x_max, y_max, kw["shape"])
        crit = criterion(beams64[k]["particles"], x_max, y_max, kw["shape"])
        edge = alive & np.any(np.abs(crit - 1.0) <= EDGE[dtype.type], axis=0)
        per_aperture.append(edge.sum(axis=-1))
        on_edge |= edge
        lost_at[alive & ~keep] = ordinal
        alive &= keep
    return beams, beams64, lost_at, on_edge, np.array(per_aperture).reshape(len(apertures), *P.shape[:-2]), apertures


def survivor_moments(beam, alive):
    """`o.beam_moments(ddof=1)` of every sample's survivors (their number differs from sample to sample): key -> (*batch,)."""
    batch = alive.shape[:-1]
    out = {key: np.full(batch, np.nan) for key in MOMENT_KEYS}
    for b in np.ndindex(*batch):
        if alive[b].any():
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = o.beam_moments({"type": "particle", "particles": beam["particles"][b][alive[b]], "energy": beam["energy"][b]}, ddof=1)
            for key in MOMENT_KEYS:
                out[key][b] = m[key]
    return out


def sparse_distances(got, ref, alive):
    """
    `moment_distances` where a sample has one particle left, or none.  None: every moment is NaN in both.  One: the
    unbiased sigmas are NaN in both, and the scales a covariance is measured in (sigma_a sigma_b) are gone: a mean is
    measured in |mean|, and a correlation must be 0 exactly, as the oracle's is.  (The sums of a sample are taken about
    the median of the reference candidates that live longest -- particle floor(l n / 64), l = 0 .. 63: every particle of
    the samples of at most 64 that come here -- so a single survivor IS the reference point, and its sums are zeros.)
    Samples with two or more: the usual scales.
    """
    names = ["x", "xp", "y", "yp", "s", "p"]
    count = alive.sum(axis=-1)
    out = {}
    for key in MOMENT_KEYS:
        g, r = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (key, g, r, count)
        with np.errstate(all="ignore"):
            if key.startswith("mu_"):
                s = np.where(count == 1, np.abs(r), np.abs(r) + np.asarray(ref["sigma" + key[2:]], dtype=np.float64))
            elif key in ("sigma_xxp", "sigma_yyp"):
                a, b = (0, 1) if key == "sigma_xxp" else (2, 3)
                s = np.where(count == 1, 0.0, np.asarray(ref["sigma_" + names[a]] * ref["sigma_" + names[b]], dtype=np.float64))
            else:
                s = np.abs(r)
            d = np.abs(g - r) / (s + 1e-300)
        out[key] = float(np.nanmax(d)) if not np.all(np.isnan(d)) else 0.0
    return out


def assert_losses(trace, desc, P, energy, dtype, expected=None, overflows=(), patterns_only=()):
    """
    Everything the module docstring says, for one trace made with losses="particles"; returns the worst distance.
    `overflows`: (point, moment, sample) entries the float32 sums cannot hold while a particle is still ALIVE (the
    square of x = 1e30 is beyond the format): they must be inf or NaN and are not compared.
    `patterns_only`: points at which a particle that is not finite (or, in float32, whose square is not) is still ALIVE:
    there the counts are compared, and the NaN patterns of the moments and of the covariance with the oracle's, nothing else.
    """
    dtype = np.dtype(dtype).type
    n, batch = P.shape[-2], P.shape[:-2]
    beams, beams64, lost_at, on_edge, edge_counts, apertures = expected or expectation(desc, P, energy, dtype)
    # the condition on the inputs, from the oracle alone
    print(f"on an edge, per aperture and sample: {edge_counts.tolist()} of n = {n}")
    if n <= 1000 or dtype == np.float64:
        assert not on_edge.any(), edge_counts
    else:
        assert np.all(edge_counts <= 1e-3 * n), edge_counts
    # mask parity
    assert trace.lost_at.shape == (*batch, n) and trace.lost_at.dtype == np.int32
    differ = (trace.lost_at != lost_at) & ~on_edge
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:5])
    assert trace.apertures == [f"AP{k}" for k in apertures] and trace.num_particles == n
    # the survivor set the trace itself reports: counts exactly, moments at the plain trace's tolerances
    first_kick = next((k for k, (kind, kw) in enumerate(desc) if kind == "cavity" and np.any(kw["voltage"] != 0)), None)
    killer = np.array(apertures + [len(desc)])[trace.lost_at]  # element that removed the particle (-1 -> beyond the end)
    worst, worst_cov, cov = 0.0, (0.0, None), trace.cov
    assert trace.num_points == len(beams) and cov.shape == (*batch, len(beams), 6, 6)
    for k, beam in enumerate(beams):
        alive = killer >= k  # aperture j clears its particles from point j + 1 on
        count = alive.sum(axis=-1)
        assert np.array_equal(trace.num_survivors[..., k], count), (k, trace.num_survivors[..., k], count)
        # all 36 entries of the biased covariance of each sample's survivors (nobody left: NaN; one left: 0 exactly)
        got_cov, ref_cov = np.array(cov[..., k, :, :], dtype=np.float64), biased_covariance(beam["particles"], alive)
        if k in patterns_only:
            got, ref = point(trace, k), survivor_moments(beam, alive)
            for key in MOMENT_KEYS:
                assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), (k, key, got[key], ref[key])
            assert np.array_equal(np.isnan(got_cov), np.isnan(ref_cov)), (k, got_cov, ref_cov)
            continue
        for kk, key, b in overflows:  # (the variance of the same coordinate: the same rule as for the sigma below)
            if kk == k:
                c = ["x", "xp", "y", "yp", "s", "p"].index(key[len("sigma_"):])
                assert not np.isfinite(got_cov[b, c, c]), (k, key, b, got_cov[b, c, c])
                got_cov[b, c, c] = ref_cov[b, c, c]
        d_cov, where = covariance_distances(got_cov, ref_cov)
        worst_cov = max(worst_cov, (d_cov, (k, *where)), key=lambda v: v[0])
        assert d_cov <= TOL_MOM[dtype], ("cov", k, d_cov, where)
        assert np.array_equal(trace.at(k)["cov"], cov[..., k, :, :], equal_nan=True), k
        ref = survivor_moments(beam, alive)
        got = point(trace, k)
        for kk, key, b in overflows:
            if kk == k:
                assert not np.isfinite(got[key][b]), (k, key, b, got[key][b])
                got[key] = np.array(got[key], dtype=np.float64)
                got[key][b] = ref[key][b]
        sparse = bool(np.any(count <= 1))  # NaN in the reference itself: nobody left, or one particle's unbiased sigma
        d = sparse_distances(got, ref, alive) if sparse else moment_distances(got, ref)
        worst = max(worst, max(d.values()))
        assert max(d.values()) <= TOL_MOM[dtype], (k, d)
        assert rel_err(trace.energy[..., k], beam["energy"]) < 1e-6, k
        if dtype == np.float32 and first_kick is not None and k > first_kick and not sparse:
            d64 = moment_distances(got, survivor_moments(beams64[k], alive))
            assert max(d64[key] for key in KICK_MOMENTS) <= TOL_KICK_F64, (k, d64)
    assert np.array_equal(trace.transmission, trace.num_survivors / n)
    drops = [trace.num_survivors[..., k] - trace.num_survivors[..., k + 1] for k in apertures]
    assert np.array_equal(trace.lost_in, np.stack(drops, axis=-1)) and trace.lost_in.shape == (*batch, len(apertures))
    for ordinal in range(len(apertures)):
        assert np.array_equal(trace.lost_in[..., ordinal], (trace.lost_at == ordinal).sum(axis=-1))
    lost_any = bool((trace.lost_at >= 0).any())
    assert (trace.outgoing is None) == lost_any
    print(f"losses {np.dtype(dtype).name}: worst moment distance over {len(beams)} points {worst:.2e}; worst covariance distance {worst_cov[0]:.2e} at "
          f"(point, i, j, sample) {worst_cov[1]}; lost {(trace.lost_at >= 0).sum(axis=-1).tolist()} of {n}")
    return worst


# ---------------------------------------------------------------------------------------------
# shapes: tile boundaries of both dtypes, more than one wave, two batch shapes
# ---------------------------------------------------------------------------------------------


def mixed_desc(shape, energy, dtype, variant):
    """
    An aperture as first leaf, drift, quadrupole, active BPM, corrector, gaining cavity, an aperture with optics on
    either side, quadrupole, drift, an aperture as last leaf.  The apertures are sigma-sized where they stand (x_max =
    1 sigma_x, y_max = 1.5 sigma_y of the unclipped float64 chain there; per-sample limits 0.8 .. 1.2 of that).  Variant
    "a": rectangular shared, elliptical per sample, rectangular per sample; variant "b": elliptical per sample,
    rectangular shared, elliptical shared.  Variant "c": the apertures of "a" in optics that couple the planes (the
    quadrupole tilted, a tilted dipole behind the corrector), for a beam that comes in correlated (`mixed_case`): every
    off-diagonal slot of the survivors' covariance is then far from 0 somewhere (tests/test_covariance_check_host.py).
    """
    rng = np.random.default_rng(17)
    f = lambda v: np.full(shape, v)  # noqa: E731
    coupled = variant == "c"
    if coupled:  # the planes and the dispersion coupled in front of the second aperture: a tilted quadrupole and dipole
        variant, away = "a", lambda lo, hi: rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)  # noqa: E731
        first = dict(length=f(0.2), k1=away(2, 5), tilt=away(0.3, 1.0), misalignment=rng.normal(0, 2e-5, (*shape, 2)))
    else:
        first = dict(length=f(0.2), k1=rng.uniform(-5, 5, shape), misalignment=rng.normal(0, 2e-5, (*shape, 2)))
    optics = [
        ("aperture", None),
        ("drift", dict(length=f(0.6))),
        ("quadrupole", first),
        ("bpm", dict(is_active=True)),
        ("hcor", dict(length=f(0.1), angle=rng.uniform(1e-5, 5e-5, shape))),
    ] + ([("dipole", dict(length=f(0.5), angle=rng.uniform(0.1, 0.2, shape), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4),
                          gap=f(0.02), tilt=f(0.3)))] if coupled else []) + [
        ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, shape), phase=rng.uniform(-10, 10, shape), frequency=f(1.3e9))),
        ("aperture", None),
        ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-5, 5, shape))),
        ("drift", dict(length=f(0.8))),
        ("aperture", None),
    ]
    # the beam sizes where the apertures stand, from the float64 chain of a many-particle beam of the same distribution
    probe = o.gaussian_particles(shape, 20_000, seed=99, dtype=np.float64, sigma=SIGMA)
    _, specs64 = build(upcast([(kind, kw or {}) for kind, kw in optics]), np.float64)
    with np.errstate(all="ignore"):
        beams64, _ = chain(specs64, o.particle_beam(probe, np.asarray(energy, dtype=np.float64), np.float64), np.float64)
    shapes = {"a": ("rectangular", "elliptical", "rectangular"), "b": ("elliptical", "rectangular", "elliptical")}[variant]
    batched = {"a": (False, True, True), "b": (True, False, False)}[variant]
    spread = np.linspace(0.8, 1.2, int(np.prod(shape))).reshape(shape)
    desc, a = [], 0
    for k, (kind, kw) in enumerate(optics):
        if kind == "aperture":
            sx = beams64[k]["particles"][..., 0].std(axis=-1).mean()
            sy = beams64[k]["particles"][..., 2].std(axis=-1).mean()
            grow = 1.0 if shapes[a] == "rectangular" else 1.6  # (an ellipse of the same half axes keeps far fewer)
            x_max, y_max = (spread * sx * grow, spread * 1.5 * sy * grow) if batched[a] else (np.array([sx * grow]), np.array([1.5 * sy * grow]))
            kw = dict(x_max=np.asarray(x_max, dtype=dtype), y_max=np.asarray(y_max, dtype=dtype), shape=shapes[a])
            a += 1
        desc.append((kind, kw))
    return desc


def mixed_case(dtype, shape, n, variant):
    if variant == "c":
        P = correlated_particles(shape, n, seed=SEEDS_COUPLED[n], dtype=dtype)
    else:
        P = o.gaussian_particles(shape, n, seed=SEEDS[n], dtype=dtype, sigma=SIGMA)
    energy = np.full(shape, 1e8, dtype=dtype)
    desc = mixed_desc(shape, energy, dtype, variant)
    return desc, P, energy


def run_mixed(lx, dtype, shape, n, variant):
    desc, P, energy = mixed_case(dtype, shape, n, variant)
    expected = expectation(desc, P, energy, dtype)
    elements, _ = build(desc, dtype, lx)
    segment = lx.Segment([elements[0], lx.Segment(elements[1:5]), *elements[5:]])  # (a nested segment is opened up)
    trace = segment.track_along(lx.ParticleBeam(P, energy, dtype=dtype), losses="particles")
    assert_losses(trace, desc, P, energy, dtype, expected)
    # the active BPM reads the centroid of the survivors that enter it
    beams, _, _, _, _, apertures = expected
    alive = np.array(apertures + [len(desc)])[trace.lost_at] >= 3
    want = survivor_moments(beams[3], alive)
    have = elements[3].reading
    assert have.shape == (2, *shape) and have.dtype == np.dtype(dtype)
    sig_x = float(np.std(P[..., 0])) + 1e-4
    for c, key in enumerate(("mu_x", "mu_y")):
        assert np.array_equal(np.isnan(have[c]), np.isnan(want[key]))
        ok = np.abs(have[c] - want[key]) <= TOL_MOM[dtype] * (np.abs(want[key]) + 3 * sig_x)
        assert np.all(ok | np.isnan(want[key])), (key, have[c], want[key])
    # without `lost_at` the records are the same bits, and nothing is brought back
    counted = segment.track_along(lx.ParticleBeam(P, energy, dtype=dtype), losses=True)
    assert counted.lost_at is None and np.array_equal(counted.records, trace.records, equal_nan=True)
    assert np.array_equal(counted.num_survivors, trace.num_survivors)
    return trace


@pytest.mark.parametrize("n", [1, 63, 64, 127, 128, 129, 255, 256, 257, 1000, 70_001])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_losses_in_a_mixed_lattice_at_every_tile_boundary(lx, dtype, shape, n):
    run_mixed(lx, dtype, shape, n, "a")


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_other_shapes_and_sharing_of_the_limits(lx, dtype, shape, n):
    run_mixed(lx, dtype, shape, n, "b")


@pytest.mark.parametrize("n", [129, 257, 1000])
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_losses_in_optics_that_couple_every_pair_of_coordinates(lx, dtype, shape, n):
    """The survivors' x-y, dispersion and s-row covariances where they are far from 0: one particle past a tile edge of
    either dtype (129, 257), and several tiles."""
    run_mixed(lx, dtype, shape, n, "c")


# ---------------------------------------------------------------------------------------------
# crafted beams of a handful of explicit particles
# ---------------------------------------------------------------------------------------------


def crafted_lattice(B, x_max):
    """A drift of no length, one rectangular aperture (|x| < x_max per sample, |y| < 1 mm), two maps that multiply x by
    1e5 each, a drift."""
    f = lambda v: np.full(B, v)  # noqa: E731
    tm = np.broadcast_to(np.eye(7), (B, 7, 7)).copy()
    tm[..., 0, 0] = 1e5
    return [("drift", dict(length=f(0.0))),
            ("aperture", dict(x_max=np.asarray(x_max, dtype=np.float64), y_max=np.array([1e-3]), shape="rectangular")),
            ("custom", dict(transfer_map=tm, length=f(0.1))), ("custom", dict(transfer_map=tm.copy(), length=f(0.1))),
            ("drift", dict(length=f(1.0)))]


def crafted(dtype):
    """
    Four samples of six particles in front of one rectangular aperture (|x|, |y| < 1 mm; sample 0: x_max = 0), then two
    maps that multiply x by 1e5 each, then a drift.  Sample 0 loses everybody; sample 1 loses one particle, which sits at
    x = 1e30 and is inf / NaN in float32 two elements later; sample 2 keeps exactly one; sample 3 is sample 1 with the
    particle at 1e30 stored FIRST.  (In front of the aperture that particle is alive and part of the sums: float32 cannot
    hold the square of 1e30, so sigma_x of samples 1 and 3 is not finite at points 0 and 1 -- the plain trace's answer to
    such a beam too.  Behind the aperture nothing of it may be left.)
    """
    B, N = 4, 6
    rng = np.random.default_rng(3)
    P = np.ones((B, N, 7))
    P[:3, :, :6] = rng.normal(0, [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], (3, N, 6))
    P[1, 3, 0] = 1e30
    P[2, [0, 1, 3], 0] = [2e-3, -3e-3, 5e-3]  # outside in x
    P[2, [4, 5], 2] = [-2e-3, 1.5e-3]         # outside in y: particle 2 is the survivor
    P[3] = P[1][[3, 1, 2, 0, 4, 5]]           # the particle at 1e30 and the first one change places
    P = P.astype(dtype)
    return crafted_lattice(B, [0.0, 1e-3, 1e-3, 1e-3]), P, np.full(B, 1e8, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nobody_left_an_overflowing_lost_particle_and_a_single_survivor(lx, dtype):
    desc, P, energy = crafted(dtype)
    elements, _ = build(desc, dtype, lx)
    trace = lx.Segment(elements).track_along(lx.ParticleBeam(P, energy, dtype=dtype), losses="particles")
    overflows = [(k, "sigma_x", b) for k in (0, 1) for b in (1, 3)] if dtype == np.float32 else []
    assert_losses(trace, desc, P, energy, dtype, overflows=overflows)
    assert np.array_equal(trace.num_survivors, [[6, 6, 0, 0, 0, 0], [6, 6, 5, 5, 5, 5], [6, 6, 1, 1, 1, 1], [6, 6, 5, 5, 5, 5]])
    assert np.array_equal(trace.lost_at, [[0] * 6, [-1, -1, -1, 0, -1, -1], [0, 0, -1, 0, 0, 0], [0, -1, -1, -1, -1, -1]])
    assert np.array_equal(trace.lost_in, [[6], [1], [5], [1]]) and trace.outgoing is None
    # nobody left: count 0 and NaN from the point behind the aperture on -- in that sample alone
    assert np.isnan(trace.records[0, 2:, :28]).all() and not np.isnan(trace.records[0, :2]).any()
    assert np.isfinite(trace.records[1:, 2:]).all()  # (behind the aperture: no trace of the particle at 1e30)
    for key in ("mu_x", "sigma_y", "sigma_xxp", "beta_x"):
        assert np.isnan(getattr(trace, key)[0, 2:]).all() and np.isfinite(getattr(trace, key)[[1, 3], 2:]).all(), key
    if dtype == np.float32:  # the lost particle did overflow: it is the masking that kept it out of the sums
        with np.errstate(all="ignore"):
            gone = np.float32(1e30) * np.float32(1e5) * np.float32(1e5)
        assert np.isinf(gone)
    # one survivor: its coordinates are the means, the unbiased sigma of one particle is NaN
    assert np.isnan(trace.sigma_x[2, 2:]).all()
    assert abs(float(trace.mu_y[2, 2]) - float(P[2, 2, 2])) <= 1e-6 * abs(float(P[2, 2, 2]))
    # the other samples do not notice: the same trace with sample 0's aperture open gives them the same bits
    desc[1][1]["x_max"] = np.array([1e-3, 1e-3, 1e-3, 1e-3])
    opened, _ = build(desc, dtype, lx)
    other = lx.Segment(opened).track_along(lx.ParticleBeam(P, energy, dtype=dtype), losses="particles")
    assert np.array_equal(other.records[1:], trace.records[1:], equal_nan=True) and np.array_equal(other.lost_at[1:], trace.lost_at[1:])
    assert other.num_survivors[0, -1] > 0


# ---------------------------------------------------------------------------------------------
# nothing lost; ParameterBeam; screens
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_infinite_apertures_lose_nobody_and_a_trace_repeats_bit_for_bit(lx, dtype):
    B, n = 3, 1000
    desc, P, energy = mixed_case(dtype, (B,), n, "a")
    for kind, kw in desc:
        if kind == "aperture":
            kw["x_max"], kw["y_max"] = np.array([np.inf]), np.array([np.inf])
    elements, _ = build(desc, dtype, lx)
    segment = lx.Segment(elements)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    first = segment.track_along(beam, losses="particles")
    again = segment.track_along(beam, losses="particles")
    assert np.array_equal(first.records, again.records) and np.array_equal(first.lost_at, again.lost_at)
    assert np.array_equal(np.asarray(first.outgoing.particles), np.asarray(again.outgoing.particles))
    assert np.all(first.num_survivors == n) and np.all(first.lost_at == -1) and np.all(first.lost_in == 0)
    assert np.all(first.transmission == 1.0) and first.outgoing is not None
    # against the plain trace of the same lattice with the apertures switched off
    for el in elements:
        if isinstance(el, lx.Aperture):
            el.is_active = False
    plain = segment.track_along(beam)
    assert plain.num_points == first.num_points and np.array_equal(plain.energy, first.energy)
    for k in range(plain.num_points):
        d = moment_distances(point(first, k), point(plain, k))
        assert max(d.values()) <= TOL_MOM[dtype], (k, d)
    assert rel_err(np.asarray(first.outgoing.particles), np.asarray(plain.outgoing.particles)) <= 1e-6
    assert np.array_equal(first.outgoing.moment_record(covariance=True), first.records[..., -1, :])
    print(f"losses=True without losses against the plain trace: records bit for bit equal: "
          f"{np.array_equal(first.records, plain.records)}; particles: "
          f"{np.array_equal(np.asarray(first.outgoing.particles), np.asarray(plain.outgoing.particles))}")
    # a limit written between two traces is seen
    for el in elements:
        if isinstance(el, lx.Aperture):
            el.is_active = True
    elements[0].x_max = np.array([1e-4], dtype=dtype)
    clipped = segment.track_along(beam, losses=True)
    assert np.all(clipped.num_survivors[..., 1] < n) and np.all(clipped.num_survivors[..., 0] == n) and clipped.outgoing is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_parameter_beam_passes_active_apertures_unchanged(lx, dtype):
    B = 3
    desc, _, energy = mixed_case(dtype, (B,), 64, "a")
    elements, _ = build(desc, dtype, lx)
    segment = lx.Segment(elements)
    kw = dict(sigma_x=np.full(B, 1e-4), sigma_xp=np.full(B, 1e-5), sigma_y=np.full(B, 1e-4), sigma_yp=np.full(B, 1e-5),
              sigma_s=np.full(B, 1e-5), sigma_p=np.full(B, 1e-3), energy=np.full(B, 1e8))
    beam = lx.ParameterBeam.from_parameters(**{k: np.asarray(v, dtype=dtype) for k, v in kw.items()}, dtype=dtype)
    with pytest.raises(NotImplementedError, match="AP0"):
        segment.track_along(beam)
    through = segment.track_along(beam, losses=True)
    for name in ("num_survivors", "transmission", "apertures", "lost_in", "lost_at"):
        assert getattr(through, name) is None, name
    for el in elements:
        if isinstance(el, lx.Aperture):
            el.is_active = False
    off = segment.track_along(beam)
    assert np.array_equal(through._mu, off._mu) and np.array_equal(through._cov, off._cov)
    assert np.array_equal(through.energy, off.energy) and through.names == off.names
    assert np.array_equal(np.asarray(through.outgoing._mu), np.asarray(off.outgoing._mu))


def test_an_active_screen_is_still_refused_for_both_beam_classes(lx):
    dtype = np.float32
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), name="AP"), lx.Screen(is_active=True, name="SCR")])
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 64, seed=1, dtype=dtype, sigma=SIGMA), f(1e8), dtype=dtype)
    parameters = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), energy=f(1e8), dtype=dtype)
    for beam in (particles, parameters):
        for losses in (True, "particles"):
            with pytest.raises(NotImplementedError, match="SCR"):
                segment.track_along(beam, losses=losses)
