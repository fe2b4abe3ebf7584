"""
`lynx_amd.grad.track_along_vjp(..., cavities=True)` on the GPU (lynx_track_particles_along_backward_cavities): gradients of
a ParticleBeam's moments at EVERY point of a lattice with gaining cavities, by a second pass over the particles.
References: central differences of the oracle's particle chain in float64; the sum over the points of `track_vjp` on the
prefixes of the lattice (by linearity the same gradient, by a path that does not know of this one) at every size where
the kernel changes form; the moment sweep on a lattice without a cavity; the float64 pass of the same call for float32.
"""

import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import reverse_reference as rr
from .helpers import make_lattice
from .test_gpu_grad import PARAMS_TO_CHECK, _desc
from .test_gpu_trace_grad import _chain, _check_parameters, _particle_lattice, _particle_moments

pytestmark = pytest.mark.gpu

INVALID = -1  # LYNX_ERR_INVALID
SIGMA = [1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3]
MU = [1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _collect(g, desc, elements):
    """{(e, name): float64 array, "energy": ...} of every parameter of PARAMS_TO_CHECK the lattice gives."""
    out = {}
    for e, (kind, _) in enumerate(desc):
        if kind not in PARAMS_TO_CHECK or elements[e] not in g:
            continue
        got = g[elements[e]]
        for name in PARAMS_TO_CHECK[kind]:
            if name in got and getattr(elements[e], name, None) is not None:
                out[(e, name)] = np.asarray(got[name], dtype=np.float64)
    out["energy"] = np.asarray(g.energy, dtype=np.float64)
    return out


def _prefix_sum(lx, desc, elements, beam, w_mu, w_cov):
    """
    sum over the points p >= 1 that carry a cotangent of track_vjp(elements[:p])(mu_bar=w_mu[:, p], cov_bar=w_cov[:, p]),
    as `_collect` shapes it (point 0 is the incoming beam: no parameter reaches it).
    """
    total = {}
    for p in range(1, len(desc) + 1):
        if not (np.any(w_mu[:, p]) or np.any(w_cov[:, p])):
            continue
        g = lx.grad.track_vjp(lx.Segment(elements[:p]), beam)(mu_bar=w_mu[:, p], cov_bar=w_cov[:, p])
        for key, value in _collect(g, desc[:p], elements[:p]).items():
            total[key] = total.get(key, 0.0) + value
    return total


def _assert_close(got, ref, w_cov, what, rtol=2e-4):
    """`_worst_distance`'s rule of test_gpu_trace_grad (2e-4 scale + 1e-7 max|got|) on every parameter; the energy like test 1."""
    assert set(ref) <= set(got), (what, set(ref) - set(got))
    worst = 0.0
    for key, r in ref.items():
        g = got[key]
        assert np.shape(g) == np.shape(r), (what, key)
        if key == "energy":
            assert np.all(np.abs(g - r) <= rtol * np.abs(r) + 1e-12), (what, key, g, r)
            continue
        scale = np.maximum(np.abs(r), 1e-9 * np.max(np.abs(w_cov)))
        assert np.all(np.abs(g - r) <= rtol * scale + 1e-7 * np.max(np.abs(g))), (what, key, g, r)
        worst = max(worst, float(np.max(np.abs(g - r) / (np.abs(r) + 1e-3 * np.max(np.abs(r)) + 1e-300))))
    print(f"{what}: worst distance {worst:.1e} over {len(ref)} quantities")
    return worst


def _weights(B, P, seed, points=None):
    """Random cotangents of mean (B, P, 6) and covariance (B, P, 6, 6) at `points` (None: all of them)."""
    rng = np.random.default_rng(seed)
    w_mu, w_cov = rng.normal(size=(B, P, 6)), rng.normal(size=(B, P, 6, 6)) * 1e3
    if points is not None:
        keep = np.zeros(P, dtype=bool)
        keep[list(points)] = True
        w_mu[:, ~keep], w_cov[:, ~keep] = 0.0, 0.0
    return w_mu, w_cov


# ---- 1. finite differences ------------------------------------------------------------------------------------------------

def test_gradients_at_every_point_match_finite_differences_of_the_particle_chain_fp64(lx):
    """
    The nine-element lattice of test_gpu_grad (two gaining cavities, a tilted and misaligned quadrupole, a dipole with
    edges), B = 2, N = 400, random cotangents of mean, covariance (x 1e3) and energy (x 1e-10, relative to the unperturbed
    energy) at all ten points, against central differences of the oracle's particle chain.
    """
    rng = np.random.default_rng(23)
    B, N = 2, 400
    desc = _desc(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=SIGMA, mu=MU)
    energy = np.array([6e6, 8e6])
    w_mu = rng.normal(size=(B, P, 6))
    w_cov = rng.normal(size=(B, P, 6, 6)) * 1e3
    w_e = rng.normal(size=(B, P)) * 1e-10
    e_ref = np.stack([b["energy"] for b in _chain(specs, o.particle_beam(particles, energy, np.float64))], axis=-1)

    def loss(particles_, energy_):
        total = np.zeros(B)
        for k, b in enumerate(_chain(specs, o.particle_beam(particles_, energy_, np.float64))):
            mean, cov = _particle_moments(b)
            total += np.sum(w_mu[:, k] * mean, axis=-1) + np.sum(w_cov[:, k] * cov, axis=(-1, -2))
            total += w_e[:, k] * (b["energy"] - e_ref[:, k])
        return total

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), cavities=True)
    assert vjp.trace.num_points == P and np.allclose(vjp.trace.energy, e_ref, rtol=1e-12)
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    assert g.mu is None and g.cov is None

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss(particles, energy)
        apply(x0 - h)
        down = loss(particles, energy)
        apply(x0)
        return (up - down) / (2 * h)

    assert _check_parameters(desc, specs, elements, g, central, w_cov) > 50
    for bidx in range(B):
        h = 1e-6 * energy[bidx]
        ep, em = energy.copy(), energy.copy()
        ep[bidx] += h
        em[bidx] -= h
        ref = (loss(particles, ep)[bidx] - loss(particles, em)[bidx]) / (2 * h)
        assert abs(g.energy[bidx] - ref) <= 2e-4 * abs(ref) + 1e-12, (bidx, g.energy[bidx], ref)


# ---- 2. against track_vjp, point by point ----------------------------------------------------------------------------------

def _cavity(B, c):
    rng = np.random.default_rng([61, c])
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    return ("cavity", dict(length=f(1.0377), voltage=rr.f32(rng.uniform(2e6, 6e6, B)), phase=rr.f32(rng.uniform(-10, 10, B)),
                           frequency=f(1.3e9)))


def _short(B, layout):
    """`layout`: a string of d(rift), q(uadrupole, misaligned), h(corrector), c(avity) -- one element per letter."""
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    desc = []
    for k, letter in enumerate(layout):
        rng = np.random.default_rng([67, k])
        if letter == "d":
            desc.append(("drift", dict(length=f(0.3))))
        elif letter == "q":
            desc.append(("quadrupole", dict(length=f(0.1), k1=rr.f32((-1) ** k * rng.uniform(0.5, 2, B)),
                                            misalignment=rr.f32(rng.normal(0, 1e-3, (B, 2))))))
        elif letter == "h":
            desc.append(("hcor", dict(length=f(0.1), angle=rr.f32(rng.normal(0, 1e-3, B)))))
        else:
            desc.append(_cavity(B, k))
    return desc


# the parking group of 4: a cavity as first step, as last step, at u % 4 == 0 and at u % 4 == 3, two back to back
GROUP_LAYOUTS = {1: "c", 4: "cdqc", 5: "dqdcc", 8: "ccdqdhqc", 9: "dqdccdqdc"}


def _compare_with_prefixes(lx, desc, N, what, points=None, seed=0, shared=False, B=2):
    elements, _ = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    energy = rr.energies(B)
    if shared:
        one = rr.particles(1, N, seed=N)
        beam = lx.ParticleBeam(one, np.array([7e6]), dtype=np.float64).broadcast((B,))
        assert beam.is_shared
    else:
        beam = lx.ParticleBeam(rr.particles(B, N, seed=N), energy, dtype=np.float64)
    w_mu, w_cov = _weights(B, P, 4000 + seed + len(desc), points)
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, cavities=True)
    got = _collect(vjp(mu_bar=w_mu, cov_bar=w_cov), desc, elements)
    ref = _prefix_sum(lx, desc, elements, beam, w_mu, w_cov)
    assert len(ref) >= 2
    _assert_close(got, ref, w_cov, what)
    return vjp


@pytest.mark.parametrize("S", sorted(GROUP_LAYOUTS))
def test_the_sum_of_prefix_track_vjps_around_the_parking_group(lx, S):
    desc = _short(2, GROUP_LAYOUTS[S])
    assert len(desc) == S
    vjp = _compare_with_prefixes(lx, desc, 301, f"S = {S} ({GROUP_LAYOUTS[S]})")
    assert len(vjp.program.steps) == S  # every leaf a step of its own


@pytest.mark.parametrize("S", [58, 59, 64])
def test_the_sum_of_prefix_track_vjps_where_the_accumulator_stride_switches(lx, S):
    """float64: the per-wave sums take 64 entries per step up to 58 steps and the 57 in use beyond (bwd_acc_stride)."""
    desc = rr.gentle_cells(2, 16)[:S]
    cavities = [e for e, (kind, _) in enumerate(desc) if kind == "cavity"]
    points = sorted({1, 4, 5, S, *(e + 1 for e in cavities)})
    _compare_with_prefixes(lx, desc, 301, f"S = {S}", points=points)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_the_sum_of_prefix_track_vjps_on_partial_tiles(lx, N):
    """A tile is 256 particles in float64, 512 in float32 (two per lane); float32 against the float64 pass of the same call."""
    desc = _short(2, GROUP_LAYOUTS[5])
    _compare_with_prefixes(lx, desc, N, f"N = {N}, float64")
    w_mu, w_cov = _weights(2, 6, 4100 + N)
    out = {}
    for dtype in (np.float64, np.float32):
        elements, _ = make_lattice(desc, dtype, lx)
        beam = lx.ParticleBeam(rr.particles(2, N, seed=N).astype(dtype), rr.energies(2).astype(dtype), dtype=dtype)
        out[dtype] = _collect(lx.grad.track_along_vjp(lx.Segment(elements), beam, cavities=True)(mu_bar=w_mu, cov_bar=w_cov), desc, elements)
    _assert_fp32(out[np.float32], out[np.float64], w_cov, f"N = {N}, float32 against float64")


def test_several_tiles_per_workgroup_with_a_partial_last_tile_and_a_shared_beam(lx):
    """
    B = 300: track_backward_t's plan (reverse_reference.backward_geometry) gives every workgroup two tiles, the last
    workgroup one, and that one partial.  The beam is shared over the batch (LYNX_TRACK_SHARED_INPUT).
    """
    B = 300
    cus = lx.device.get_runtime().info()["compute_units"]
    cap = (24 * cus + B - 1) // B
    tiles = 2 * cap - 1
    N = tiles * 256 - 3
    _, chunks, per_wg = rr.backward_geometry(N, B, cus, 1)
    assert per_wg >= 2 and chunks * per_wg > tiles, (cus, chunks, per_wg)
    desc = _short(B, GROUP_LAYOUTS[5])
    _compare_with_prefixes(lx, desc, N, f"B = {B}, {tiles} tiles, {per_wg} per workgroup", points=[3, 5], shared=True, B=B)


def _seventeen_chunks(lx, N, lane_particles):
    """B = 2: every tile a workgroup of its own, and 17 of them -- k_reduce_tbar (from 16 chunks up) with a remainder behind its unrolled loop."""
    tiles, chunks, per_wg = rr.backward_geometry(N, 2, lx.device.get_runtime().info()["compute_units"], lane_particles)
    assert (tiles, chunks, per_wg) == (17, 17, 1)


def test_the_sum_of_prefix_track_vjps_at_seventeen_chunks(lx):
    _seventeen_chunks(lx, 4097, 1)
    _compare_with_prefixes(lx, _short(2, GROUP_LAYOUTS[5]), 4097, "N = 4097, 17 chunks, float64")


def test_a_shared_incoming_beam(lx):
    _compare_with_prefixes(lx, _short(3, GROUP_LAYOUTS[9]), 700, "shared beam", shared=True, B=3)


# ---- 3. no cavity: two implementations, one answer --------------------------------------------------------------------------

def test_without_a_cavity_the_pass_over_the_particles_is_the_moment_sweep(lx):
    rng = np.random.default_rng(42)
    B, N = 2, 400
    desc = _particle_lattice(B, rng)
    elements, _ = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    beam = lx.ParticleBeam(o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=SIGMA, mu=MU), np.array([6e6, 8e6]),
                           dtype=np.float64)
    w_mu, w_cov = _weights(B, P, 17)
    w_e = rng.normal(size=(B, P)) * 1e-10
    segment = lx.Segment(elements)
    sweep = lx.grad.track_along_vjp(segment, beam)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    again = lx.grad.track_along_vjp(segment, beam, cavities=True)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    reference = _collect(sweep, desc, elements)
    assert len(reference) > 15
    _assert_close(_collect(again, desc, elements), reference, w_cov, "no cavity")
    assert sweep.mu is not None and again.mu is None


# ---- 4. float32 against the float64 pass of the same call ------------------------------------------------------------------

def _assert_fp32(got, ref, w_cov, what):
    """3e-3 |ref| + floor, the floor of test_merged_pairs_reverse_pass_fp32: 1e-4 max(max|ref|, 1e-9 max|w_cov|)."""
    worst = 0.0
    for key, r in ref.items():
        g = got[key]
        assert g.shape == r.shape and np.all(np.isfinite(g)), (what, key)
        floor = 1e-4 * max(np.max(np.abs(r)), 1e-9 * np.max(np.abs(w_cov)))
        assert np.all(np.abs(g - r) <= 3e-3 * np.abs(r) + floor), (what, key, g, r)
        worst = max(worst, float(np.max(np.abs(g - r) / (3e-3 * np.abs(r) + floor))))
    print(f"{what}: worst distance {worst:.4f} of the bound")


def _both_dtypes(lx, B, N):
    """
    The lattice, beam and energies of test_merged_pairs_reverse_pass_fp32, cotangents at all ten points: the gradients of
    the call in both dtypes, and what they were made from: {dtype: (elements, beam)}, desc, w_mu, w_cov.
    """
    rng = np.random.default_rng(42)
    desc = _desc(B, rng)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=SIGMA, mu=MU)
    energy = rng.uniform(6e6, 8e6, B)
    w_mu, w_cov = _weights(B, P, 29)
    out, made = {}, {}
    for dtype in (np.float64, np.float32):
        elements, _ = make_lattice(desc, dtype, lx)
        beam = lx.ParticleBeam(particles.astype(dtype), energy.astype(dtype), dtype=dtype)
        out[dtype] = _collect(lx.grad.track_along_vjp(lx.Segment(elements), beam, cavities=True)(mu_bar=w_mu, cov_bar=w_cov), desc, elements)
        made[dtype] = (elements, beam)
    assert sum(v.size for v in out[np.float64].values()) > 50
    return out, made, desc, w_mu, w_cov


@pytest.mark.parametrize("B,N", [(2, 3000), (300, 256)], ids=["workgroup-build", "lanes-build"])
def test_float32_against_the_float64_pass(lx, B, N):
    out, _, _, _, w_cov = _both_dtypes(lx, B, N)
    _assert_fp32(out[np.float32], out[np.float64], w_cov, f"float32 against float64, B = {B}, N = {N}")


def test_float32_against_the_float64_pass_at_seventeen_chunks(lx):
    """
    N = 8193: 17 packed tiles.  The float32 sum of prefix `track_vjp` calls -- a float32 path that knows nothing of this
    one -- lies within the same bound of the float64 pass: the inputs allow float32 that much.
    """
    _seventeen_chunks(lx, 8193, 2)
    out, made, desc, w_mu, w_cov = _both_dtypes(lx, 2, 8193)
    _assert_fp32(out[np.float32], out[np.float64], w_cov, "float32 against float64, B = 2, N = 8193")
    elements, beam = made[np.float32]
    _assert_fp32(_prefix_sum(lx, desc, elements, beam, w_mu, w_cov), out[np.float64], w_cov, "float32 prefix track_vjps against float64, B = 2, N = 8193")


# ---- 5. the incoming particles -----------------------------------------------------------------------------------------------

def test_gradient_wrt_incoming_particles(lx):
    rng = np.random.default_rng(7)
    B, N = 2, 300
    desc = _desc(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=3, dtype=np.float64, sigma=SIGMA)
    energy = np.array([6e6, 8e6])
    w_mu = rng.normal(size=(B, P, 7))
    w_cov = rng.normal(size=(B, P, 6, 6)) * 1e3

    def loss(particles_):
        total = np.zeros(B)
        for k, b in enumerate(_chain(specs, o.particle_beam(particles_, energy, np.float64))):
            mean, cov = _particle_moments(b)
            total += np.sum(w_mu[:, k, :6] * mean, axis=-1) + np.sum(w_cov[:, k] * cov, axis=(-1, -2))
        return total

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), cavities=True)
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, wrt_particles=True)
    got = np.asarray(g.particles)
    assert got.shape == (B, N, 7)
    for b, n, c in [(0, 0, 0), (0, 17, 1), (1, 299, 2), (1, 5, 3), (0, 123, 4), (1, 200, 5), (0, 255, 5), (1, 256, 0)]:
        h = 1e-7
        up, down = particles.copy(), particles.copy()
        up[b, n, c] += h
        down[b, n, c] -= h
        ref = (loss(up)[b] - loss(down)[b]) / (2 * h)
        assert abs(got[b, n, c] - ref) <= 1e-4 * abs(ref) + 1e-6 * np.max(np.abs(got[b])), (b, n, c, got[b, n, c], ref)
    # a rigid shift of the beam: every particle moved by the same step
    for c in range(6):
        h = 1e-7
        up, down = particles.copy(), particles.copy()
        up[:, :, c] += h
        down[:, :, c] -= h
        ref = (loss(up) - loss(down)) / (2 * h)
        total = got[:, :, c].sum(axis=1)
        assert np.all(np.abs(total - ref) <= 1e-4 * np.abs(ref) + 1e-6 * np.max(np.abs(total))), (c, total, ref)
    # the 7th column carries mu_bar[..., 6] alone, every point's, 1 / N each (the 7th row of every map is e_7): without
    # it that column loses exactly this, and the other six keep their bits
    without = np.asarray(vjp(mu_bar=w_mu * [1, 1, 1, 1, 1, 1, 0], cov_bar=w_cov, wrt_particles=True).particles)
    assert np.array_equal(without[..., :6], got[..., :6])
    carried = w_mu[..., 6].sum(axis=1)[:, None] / N
    assert np.allclose(got[..., 6] - without[..., 6], carried, rtol=1e-9, atol=1e-12 * np.max(np.abs(got[..., 6])))
    only = np.asarray(vjp(mu_bar=w_mu * [0, 0, 0, 0, 0, 0, 1], wrt_particles=True).particles)
    assert np.all(only[..., :6] == 0) and np.allclose(only[..., 6], carried, rtol=1e-13, atol=0.0)
    with pytest.raises(KeyError):
        vjp(mu_bar=w_mu).particles
    with pytest.raises(ValueError, match="wrt_particles"):
        lx.grad.track_along_vjp(lx.Segment(elements[:3]), lx.ParticleBeam(particles, energy, dtype=np.float64))(
            mu_bar=w_mu[:, :4], wrt_particles=True)


# ---- 6. the rest of the contract ----------------------------------------------------------------------------------------------

def _bpm_line(lx):
    a = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    bpm = lx.BPM(is_active=True, name="BPM1")
    elements = [lx.Drift(a(1.0), dtype=np.float64), lx.VerticalCorrector(a(0.3), angle=a(3e-3), dtype=np.float64),
                lx.Quadrupole(a(0.2), k1=a(2.0), misalignment=np.array([[1e-4, -2e-4]]), dtype=np.float64),
                lx.Cavity(a(1.0377), voltage=a(1.5e7), phase=a(-5.0), frequency=a(1.3e9), dtype=np.float64, name="ACC"),
                lx.HorizontalCorrector(a(0.3), angle=a(1e-4), dtype=np.float64), lx.Drift(a(2.0), dtype=np.float64), bpm,
                lx.Drift(a(0.5), dtype=np.float64)]
    particles = o.gaussian_particles((1,), 2000, seed=21, dtype=np.float64, sigma=[1e-4, 2e-5, 1e-4, 2e-5, 1e-5, 1e-3],
                                     mu=[2e-4, 3e-5, -1e-4, 2e-5, 0.0, 0.0])
    return elements, bpm, lx.ParticleBeam(particles, a(2e7), dtype=np.float64), particles


def test_the_same_call_returns_the_same_bits_and_a_bpm_reads_the_centroid_in_front_of_it(lx):
    elements, bpm, beam, _ = _bpm_line(lx)
    segment = lx.Segment(elements)
    vjp = lx.grad.track_along_vjp(segment, beam, cavities=True)
    bar = np.array([[0.7], [-1.3]])
    got = vjp(readings={bpm: bar}, wrt_particles=True)
    weights = np.zeros((1, len(elements) + 1))
    weights[:, 6] = 1.0
    same = vjp(mu_x=weights * bar[0, 0], mu_y=weights * bar[1, 0], wrt_particles=True)
    ref = lx.grad.track_vjp(segment, beam)(readings={bpm: bar})  # (the BPM an observer step of the streaming pass)
    for element, name in ((elements[0], "length"), (elements[1], "angle"), (elements[2], "k1"), (elements[2], "misalignment"),
                          (elements[3], "voltage"), (elements[3], "phase"), (elements[4], "angle"), (elements[5], "length")):
        r = np.asarray(ref[element][name])
        assert np.all(r != 0), name
        assert np.allclose(got[element][name], r, rtol=2e-4, atol=0.0), (name, got[element][name], r)  # (two paths: the project's 2e-4)
        assert np.array_equal(same[element][name], got[element][name]), name
    assert np.all(np.asarray(got[elements[7]]["length"]) == 0)  # behind the BPM
    assert np.array_equal(np.asarray(same.particles), np.asarray(got.particles)) and np.array_equal(same.energy, got.energy)
    # a second vjp of the same problem: the same bits
    again = lx.grad.track_along_vjp(segment, beam, cavities=True)(readings={bpm: bar}, wrt_particles=True)
    assert np.array_equal(np.asarray(again.particles), np.asarray(got.particles))
    assert np.array_equal(again[elements[3]]["voltage"], got[elements[3]]["voltage"])
    with pytest.raises(KeyError):
        vjp(readings={lx.BPM(is_active=True): bar})


def test_property_cotangents_shapes_and_refusals(lx):
    elements, _, beam, particles = _bpm_line(lx)
    segment = lx.Segment(elements)
    vjp = lx.grad.track_along_vjp(segment, beam, cavities=True)
    g = vjp(sigma_x=1.0, beta_x=1.0, emittance_y=2.0)
    assert g.mu is None and g.cov is None
    k1 = g[elements[2]]["k1"]
    assert k1.shape == (1,) and np.isfinite(k1).all() and k1[0] != 0 and np.all(g[elements[3]]["voltage"] != 0)
    parts = vjp(sigma_x=1.0)[elements[2]]["k1"] + vjp(beta_x=1.0, emittance_y=2.0)[elements[2]]["k1"]
    assert np.allclose(parts, k1, rtol=1e-10)
    # d sigma_x / d k1 at the last point against a central difference of the tracked sigma_x
    last = np.zeros((1, len(elements) + 1))
    last[:, -1] = 1.0
    got = float(vjp(sigma_x=last)[elements[2]]["k1"][0])
    h = 1e-4
    values = []
    for sign in (1, -1):
        elements[2].k1 = np.array([2.0 + sign * h])
        values.append(float(segment.track(beam).sigma_x[0]))
    elements[2].k1 = np.array([2.0])
    assert np.isclose(got, (values[0] - values[1]) / (2 * h), rtol=1e-5), (got, values)
    # a ParameterBeam: the plain call
    mu = np.concatenate([particles[0, :, :6].mean(axis=0), [1.0]])[None]
    cov = np.zeros((1, 7, 7))
    cov[0, :6, :6] = np.cov(particles[0, :, :6].T, bias=True)
    pbeam = lx.ParameterBeam(mu, cov, np.array([2e7]), dtype=np.float64)
    plain, switched = lx.grad.track_along_vjp(segment, pbeam)(sigma_x=1.0), lx.grad.track_along_vjp(segment, pbeam, cavities=True)(sigma_x=1.0)
    assert np.array_equal(plain[elements[2]]["k1"], switched[elements[2]]["k1"]) and switched.mu is not None
    # refusals by value
    a = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    long = lx.Segment(elements[:4] + [lx.Drift(a(0.1), dtype=np.float64, name=f"D{k}") for k in range(61)])
    with pytest.raises(NotImplementedError, match="65 leaf elements, more than 64.*'D60'"):
        lx.grad.track_along_vjp(long, beam, cavities=True)
    with pytest.raises(NotImplementedError, match="trajectories="):
        lx.grad.track_along_vjp(segment, beam, trajectories=4, cavities=True)
    with pytest.raises(NotImplementedError, match="losses=True"):
        lx.grad.track_along_vjp(segment, beam, losses=True, cavities=True)
    with pytest.raises(NotImplementedError, match="ACC"):
        lx.grad.track_along_vjp(segment, beam)


def test_the_entry_point_refuses_before_it_launches(lx):
    from lynx_amd import _ffi, engine

    rt = lx.device.get_runtime()
    elements, _, beam, _ = _bpm_line(lx)
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, cavities=True)
    g = vjp(sigma_x=1.0)  # (the lattice is ready, the trace on the device)
    before = g[elements[2]]["k1"].copy()
    cache = vjp.segment.__dict__["_trace_cache"]
    lat = engine._ready(cache, vjp.program, beam.batch_shape, beam.dtype, beam._energy._host)
    P = vjp.trace.num_points
    e_in = beam._energy.broadcast_device(rt, beam.batch_shape)
    p_in = beam._particles.device(rt)
    rec = vjp.trace._device["records"]
    bar = rt.to_device(np.zeros((1, P, 36)))
    g_par, g_en = rt.empty((1, lat.E, 8), np.float64), rt.empty((1,), np.float64)
    p = lambda a: None if a is None else C.c_void_p(a.ptr)  # noqa: E731

    def call(n=beam.num_particles, energy=e_in, particles=p_in, flags=0, records=rec, cotangents=bar, params=g_par, grad_energy=g_en,
             grad_p=None, lattice=lat.handle):
        return rt.lib.lynx_track_particles_along_backward_cavities(
            rt.ctx, lattice, n, p(energy), p(particles), flags, p(records), p(cotangents), None, p(params), p(grad_energy),
            grad_p)

    assert call() == 0
    for kwargs in (dict(energy=None), dict(particles=None), dict(records=None), dict(cotangents=None), dict(params=None),
                   dict(grad_energy=None), dict(lattice=None), dict(n=0), dict(n=-3), dict(flags=_ffi.TRACK_MOMENTS),
                   dict(flags=_ffi.TRACK_SHARED_INPUT | _ffi.TRACK_COVARIANCE), dict(grad_p=C.c_void_p(p_in.ptr))):
        assert call(**kwargs) == INVALID, kwargs
        assert rt.lib.lynx_last_error(rt.ctx).decode().startswith("beam trace gradients with cavities: "), kwargs
    # more than 64 steps: a 65-leaf program, through the C ABI alone (Python refuses it by value)
    a = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    leaves = elements[:4] + [lx.Drift(a(0.1), dtype=np.float64) for _ in range(61)]
    long = lx.Segment(leaves)
    program = engine._trace_plan(long, leaves)
    lat65 = engine._ready(engine.LatticeCache(), program, beam.batch_shape, beam.dtype, beam._energy._host)
    assert call(lattice=lat65.handle) == INVALID
    message = rt.lib.lynx_last_error(rt.ctx).decode()
    assert message.startswith("beam trace gradients with cavities: 65 steps"), message
    assert np.array_equal(vjp(sigma_x=1.0)[elements[2]]["k1"], before)  # nothing was disturbed


# ---- 7. the example ---------------------------------------------------------------------------------------------------------

def test_match_beam_size_behind_cavity_example_converges(lx):
    """examples/match_beam_size_behind_cavity.py: Adam on two quadrupoles around a cavity until the beam sizes at two markers are the targets."""
    spec = importlib.util.spec_from_file_location(
        "match_beam_size_behind_cavity", pathlib.Path(__file__).resolve().parents[1] / "examples" / "match_beam_size_behind_cavity.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.accelerating_line(), example.incoming_beam()
    history = example.tune(segment, beam, steps=100)
    assert history[-1] < 0.05 * history[0], (history[0], history[-1])
    trace = segment.track_along(beam)
    for marker, (sigma_x, sigma_y) in example.TARGETS.items():
        k = trace.index_of(marker)
        assert abs(float(trace.sigma_x[0, k]) / sigma_x - 1) < 0.05, (marker, trace.sigma_x[0, k], sigma_x)
        assert abs(float(trace.sigma_y[0, k]) / sigma_y - 1) < 0.05, (marker, trace.sigma_y[0, k], sigma_y)
