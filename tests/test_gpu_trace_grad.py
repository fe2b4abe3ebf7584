"""
`lynx_amd.grad.track_along_vjp` on the GPU (lynx_track_moments_along_backward, lynx_track_particles_along_backward):
gradients of the moments and energies at EVERY point of a lattice against central differences of the oracle's
element-by-element chain in float64, against `track_vjp` where the two meet (a cotangent at the last point, the
reading of an active BPM), float32 against the float64 pass on a 128-element lattice, and the shapes.
"""

import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice
from .test_gpu_grad import PARAMS_TO_CHECK, _desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _chain(specs, beam):
    beams = [beam]
    for spec in specs:
        beams.append(o.element_track(spec, beams[-1], np.float64))
    return beams


def _particle_moments(beam):
    Q = beam["particles"][..., :6]
    mu = Q.mean(axis=-2)
    d = Q - mu[..., None, :]
    return mu, np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2]


def _check_parameters(desc, specs, elements, g, central, w_cov):
    """Every parameter of PARAMS_TO_CHECK at the tolerance of test_gpu_grad's finite-difference tests; returns how many."""
    checked = 0
    for e, (kind, _) in enumerate(desc):
        for name in PARAMS_TO_CHECK.get(kind, []):
            arr = specs[e][name]
            if arr is None:
                continue
            got = g[elements[e]][name]
            assert got.shape == arr.shape
            for idx in np.ndindex(arr.shape):
                def apply(x, arr=arr, idx=idx):
                    arr[idx] = x
                ref = central(apply, arr[idx])[idx[0]]
                scale = max(abs(ref), 1e-9 * np.max(np.abs(w_cov)))
                assert abs(got[idx] - ref) <= 2e-4 * scale + 1e-7 * np.max(np.abs(got)), (kind, e, name, idx, got[idx], ref)
                checked += 1
    return checked


def test_parameter_beam_gradients_at_every_point_match_finite_differences_fp64(lx):
    """
    The nine-element lattice of test_gpu_grad (two gaining cavities, a tilted and misaligned quadrupole, a dipole with
    edges), B = 2, random cotangents of mu, cov and the energy at ALL ten points, against central differences of the
    oracle chained with `element_track` element by element.  The loss takes the energy at a point relative to its
    unperturbed value (a constant: the gradient is the same) -- energies are 1e7, the moment terms 1e-3, and as written
    the differences of the sum would lose the moment terms' digits.
    """
    rng = np.random.default_rng(23)
    B = 2
    desc = _desc(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    A = rng.normal(size=(B, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3]
    cov = np.zeros((B, 7, 7))
    cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2)
    mu = np.concatenate([rng.normal(size=(B, 6)) * [1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3], np.ones((B, 1))], axis=-1)
    energy = np.array([6e6, 8e6])
    w_mu = rng.normal(size=(B, P, 7)) * [1, 1, 1, 1, 1, 1, 0]
    w_cov = np.zeros((B, P, 7, 7))
    w_cov[..., :6, :6] = rng.normal(size=(B, P, 6, 6)) * 1e3
    w_e = rng.normal(size=(B, P)) * 1e-10  # (the size of dL/dE through the maps: both paths count in what is compared)

    def energies(mu_, cov_, energy_):
        return np.stack([b["energy"] for b in _chain(specs, o.parameter_beam(mu_, cov_, energy_, np.float64))], axis=-1)

    e_ref = energies(mu, cov, energy)

    def loss(mu_, cov_, energy_):
        beams = _chain(specs, o.parameter_beam(mu_, cov_, energy_, np.float64))
        total = np.zeros(B)
        for k, b in enumerate(beams):
            total += np.sum(w_mu[:, k] * b["mu"], axis=-1) + np.sum(w_cov[:, k] * b["cov"], axis=(-1, -2))
            total += w_e[:, k] * (b["energy"] - e_ref[:, k])
        return total

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParameterBeam(mu, cov, energy, dtype=np.float64))
    assert vjp.trace.num_points == P and np.allclose(vjp.trace.energy, e_ref, rtol=1e-12)
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss(mu, cov, energy)
        apply(x0 - h)
        down = loss(mu, cov, energy)
        apply(x0)
        return (up - down) / (2 * h)

    assert _check_parameters(desc, specs, elements, g, central, w_cov) > 50
    for bidx in range(B):
        h = 1e-6 * energy[bidx]
        ep, em = energy.copy(), energy.copy()
        ep[bidx] += h
        em[bidx] -= h
        ref = (loss(mu, cov, ep)[bidx] - loss(mu, cov, em)[bidx]) / (2 * h)
        assert abs(g.energy[bidx] - ref) <= 2e-4 * abs(ref) + 1e-12, (bidx, g.energy[bidx], ref)
        for c in range(6):
            h = 1e-7
            mp, mm = mu.copy(), mu.copy()
            mp[bidx, c] += h
            mm[bidx, c] -= h
            ref = (loss(mp, cov, energy)[bidx] - loss(mm, cov, energy)[bidx]) / (2 * h)
            assert abs(g.mu[bidx, c] - ref) <= 1e-5 * abs(ref) + 1e-9 * np.max(np.abs(g.mu[bidx])), (bidx, c, g.mu[bidx, c], ref)
        for (r, c) in [(0, 0), (0, 1), (1, 0), (2, 3), (4, 4), (4, 5), (5, 4), (5, 5), (3, 5)]:
            h = 1e-12
            cp, cm = cov.copy(), cov.copy()
            cp[bidx, r, c] += h
            cm[bidx, r, c] -= h
            ref = (loss(mu, cp, energy)[bidx] - loss(mu, cm, energy)[bidx]) / (2 * h)
            assert abs(g.cov[bidx, r, c] - ref) <= 1e-4 * abs(ref) + 1e-7 * np.max(np.abs(g.cov[bidx])), (bidx, r, c, g.cov[bidx, r, c], ref)
    # the energy cotangents alone: E_k = E_in + the gains V cos(phi) of the cavities in front of point k
    only = vjp(energy_bar=w_e)
    assert np.allclose(only.energy, w_e.sum(axis=-1), rtol=1e-9, atol=0.0)
    for e in (3, 6):
        behind = w_e[:, e + 1:].sum(axis=-1)
        phi = np.deg2rad(specs[e]["phase"])
        assert np.allclose(only[elements[e]]["voltage"], behind * np.cos(phi), rtol=1e-9, atol=0.0)
        assert np.allclose(only[elements[e]]["phase"], -behind * specs[e]["voltage"] * np.sin(phi) * np.pi / 180, rtol=1e-9, atol=0.0)
    assert np.all(only[elements[1]]["k1"] == 0)


def _particle_lattice(B, rng):
    """test_gpu_grad's lattice without its two cavities, plus a corrector of zero length."""
    desc = [(kind, kw) for kind, kw in _desc(B, rng) if kind != "cavity"]
    desc.insert(4, ("hcor", dict(length=np.full(B, 0.0), angle=rng.normal(0, 1e-3, B))))
    return desc


def test_particle_beam_gradients_at_every_point_match_finite_differences_of_the_particle_chain_fp64(lx):
    """
    The reference is the PARTICLE chain: `element_track` on 400 particles per sample, element by element, the mean and the
    biased covariance of the particles at every point taken in float64.  The kernel never sees the particles again after
    the forward trace -- that it reproduces these differences is the closure of the moments under affine maps.
    """
    rng = np.random.default_rng(42)
    B, N = 2, 400
    desc = _particle_lattice(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6])
    w_mu = rng.normal(size=(B, P, 6))
    w_cov = rng.normal(size=(B, P, 6, 6)) * 1e3
    w_e = rng.normal(size=(B, P)) * 1e-10

    def loss(particles_, energy_):
        total = np.zeros(B)
        for k, b in enumerate(_chain(specs, o.particle_beam(particles_, energy_, np.float64))):
            mean, cov = _particle_moments(b)
            total += np.sum(w_mu[:, k] * mean, axis=-1) + np.sum(w_cov[:, k] * cov, axis=(-1, -2))
            total += w_e[:, k] * (b["energy"] - energy)  # (relative to the unperturbed energy, see the test above)
        return total

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64))
    assert vjp.trace.num_points == P
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss(particles, energy)
        apply(x0 - h)
        down = loss(particles, energy)
        apply(x0)
        return (up - down) / (2 * h)

    assert _check_parameters(desc, specs, elements, g, central, w_cov) > 40
    for bidx in range(B):
        h = 1e-6 * energy[bidx]
        ep, em = energy.copy(), energy.copy()
        ep[bidx] += h
        em[bidx] -= h
        ref = (loss(particles, ep)[bidx] - loss(particles, em)[bidx]) / (2 * h)
        assert abs(g.energy[bidx] - ref) <= 2e-4 * abs(ref) + 1e-12, (bidx, g.energy[bidx], ref)
        for c in range(6):  # the incoming mean: every particle moved by the same step
            h = 1e-7
            pp, pm = particles.copy(), particles.copy()
            pp[bidx, :, c] += h
            pm[bidx, :, c] -= h
            ref = (loss(pp, energy)[bidx] - loss(pm, energy)[bidx]) / (2 * h)
            assert abs(g.mu[bidx, c] - ref) <= 1e-5 * abs(ref) + 1e-9 * np.max(np.abs(g.mu[bidx])), (bidx, c, g.mu[bidx, c], ref)
    assert g.cov.shape == (B, 7, 7) and np.allclose(g.cov, np.swapaxes(g.cov, -1, -2), rtol=1e-12, atol=0.0)


def _worst_distance(desc, elements_a, g_a, elements_b, g_b, w_cov):
    """Both gradients within the finite-difference tests' tolerance of each other; the worst distance in units of it."""
    worst = 0.0
    for e, (kind, _) in enumerate(desc):
        for name in PARAMS_TO_CHECK.get(kind, []):
            if name not in g_b[elements_b[e]]:
                continue
            got, ref = np.asarray(g_a[elements_a[e]][name]), np.asarray(g_b[elements_b[e]][name])
            assert got.shape == ref.shape
            scale = np.maximum(np.abs(ref), 1e-9 * np.max(np.abs(w_cov)))
            assert np.all(np.abs(got - ref) <= 2e-4 * scale + 1e-7 * np.max(np.abs(got))), (kind, e, name, got, ref)
            worst = max(worst, float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.max(np.abs(ref)) + 1e-300))))
    return worst


@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_a_cotangent_at_the_last_point_is_track_vjp(lx, beam_type):
    """
    Cotangent at the LAST point only: `track_along_vjp` against `track_vjp` of the same segment and beam, float64.  The two
    differ by a chain of element maps against the composed map of a run: rounding.
    """
    rng = np.random.default_rng(5)
    B = 2
    desc = _desc(B, rng) if beam_type == "parameters" else _particle_lattice(B, rng)
    elements, _ = make_lattice(desc, np.float64, lx)
    segment = lx.Segment(elements)
    P = len(desc) + 1
    energy = np.array([6e6, 8e6])
    w_mu, w_cov = rng.normal(size=(B, 6)), rng.normal(size=(B, 6, 6)) * 1e3
    if beam_type == "parameters":
        A = rng.normal(size=(B, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3]
        cov = np.zeros((B, 7, 7))
        cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2)
        mu = np.concatenate([rng.normal(size=(B, 6)) * [1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3], np.ones((B, 1))], axis=-1)
        beam = lx.ParameterBeam(mu, cov, energy, dtype=np.float64)
    else:
        beam = lx.ParticleBeam(o.gaussian_particles((B,), 3000, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                                    mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3]), energy, dtype=np.float64)
    ref = lx.grad.track_vjp(segment, beam)(mu_bar=w_mu, cov_bar=w_cov)
    mu_bar, cov_bar = np.zeros((B, P, 6)), np.zeros((B, P, 6, 6))
    mu_bar[:, -1], cov_bar[:, -1] = w_mu, w_cov
    got = lx.grad.track_along_vjp(segment, beam)(mu_bar=mu_bar, cov_bar=cov_bar)
    worst = _worst_distance(desc, elements, got, elements, ref, w_cov)
    assert np.allclose(got.energy, ref.energy, rtol=2e-4, atol=1e-12)
    print(f"track_along_vjp against track_vjp, cotangent at the last point, {beam_type}: worst distance {worst:.1e}")
    if beam_type == "parameters":
        assert np.allclose(got.mu, ref.mu, rtol=1e-9, atol=1e-12 * np.max(np.abs(ref.mu)))
        assert np.allclose(got.cov, ref.cov, rtol=1e-9, atol=1e-12 * np.max(np.abs(ref.cov)))


@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_the_reading_of_an_active_bpm_is_the_centroid_in_front_of_it(lx, beam_type):
    """`readings={bpm: bar}` and a cotangent on mu_x, mu_y at the point in front of the BPM, against `track_vjp(readings=)`."""
    a = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    bpm = lx.BPM(is_active=True, name="BPM1")
    elements = [lx.Drift(a(1.0), dtype=np.float64), lx.VerticalCorrector(a(0.3), angle=a(3e-3), dtype=np.float64),
                lx.Quadrupole(a(0.2), k1=a(2.0), misalignment=np.array([[1e-4, -2e-4]]), dtype=np.float64),
                lx.HorizontalCorrector(a(0.3), angle=a(1e-4), dtype=np.float64), lx.Drift(a(2.0), dtype=np.float64), bpm,
                lx.Drift(a(0.5), dtype=np.float64)]
    segment = lx.Segment(elements)
    particles = o.gaussian_particles((1,), 2000, seed=21, dtype=np.float64, sigma=[1e-4, 2e-5, 1e-4, 2e-5, 1e-5, 1e-3],
                                     mu=[2e-4, 3e-5, -1e-4, 2e-5, 0.0, 0.0])
    energy = a(1e8)
    if beam_type == "parameters":
        Q = particles[0, :, :6]
        cov0 = np.zeros((1, 7, 7))
        cov0[0, :6, :6] = np.cov(Q.T, bias=True)
        beam = lx.ParameterBeam(np.concatenate([Q.mean(axis=0), [1.0]])[None], cov0, energy, dtype=np.float64)
    else:
        beam = lx.ParticleBeam(particles, energy, dtype=np.float64)
    bar = np.array([[0.7], [-1.3]])
    ref = lx.grad.track_vjp(segment, beam)(readings={bpm: bar})
    vjp = lx.grad.track_along_vjp(segment, beam)
    assert np.allclose(bpm.reading, np.stack([vjp.trace.mu_x[:, 5], vjp.trace.mu_y[:, 5]]), rtol=1e-12)
    got = vjp(readings={bpm: bar})
    weights = np.zeros((1, len(elements) + 1))
    weights[:, 5] = 1.0
    same = vjp(mu_x=weights * bar[0, 0], mu_y=weights * bar[1, 0])
    for element, name in ((elements[0], "length"), (elements[1], "angle"), (elements[2], "k1"), (elements[2], "misalignment"),
                          (elements[3], "angle"), (elements[4], "length")):
        r = np.asarray(ref[element][name])
        assert np.all(r != 0), name
        assert np.allclose(got[element][name], r, rtol=1e-7, atol=0.0), (name, got[element][name], r)
        assert np.array_equal(same[element][name], got[element][name]), name
    assert np.all(np.asarray(got[elements[6]]["length"]) == 0)  # behind the BPM
    with pytest.raises(KeyError):
        vjp(readings={lx.BPM(is_active=True): bar})


# distance max |g - r| / (|r| + 1e-3 max |r|) of the float32 gradient g from the float64 `track_along_vjp` r of the same
# input, per parameter name: twice what test_float32_against_the_float64_pass_on_128_elements measured on MI355X --
#                  particles (B = 64 x 100 000)     parameters (B = 300)
#     k1                     1.0e-03                      6.9e-03
#     length                 1.7e-03                      8.8e-03
#     energy                 0                            0          (beta does not depend on the energy in this lattice)
# Beyond 1e-3, and DESIGN.md ("Beam trace") says which sum cancels: the emittance, sigma^2 sigma'^2 - sigma_xx'^2, and with it
# C^-1 C in the sweep, (1 + alpha^2)-fold -- alpha reaches 15.5 here, the beam comes in with beta = 10 m where the channel's
# matched beta is below 2 m.  A ParameterBeam's float32 covariances carry that cancellation at every point of the forward
# trace already (beta_x of the float32 trace is 2.3e-4 from the float64 one; a ParticleBeam's records are float64 sums:
# 4.7e-5).  With the sweep itself in float32 these read 5.3e-3 / 4.1e-3 and 6.2e-3 / 9.2e-3.
TOL_TRACE_GRAD = {"particles": {"k1": 2.0e-3, "length": 3.4e-3, "energy": 0.0},
                  "parameters": {"k1": 1.4e-2, "length": 1.8e-2, "energy": 0.0}}


@pytest.mark.parametrize("beam_type", ["particles", "parameters"])
def test_float32_against_the_float64_pass_on_128_elements(lx, beam_type):
    """
    `o.fodo_segment(32)` with a k1 scan over the batch: B = 64 ParticleBeam of 100 000 shared particles, B = 300
    ParameterBeam (the lanes = samples build), cotangents beta_x = beta_y = 1 at every one of the 129 points.  The beam
    is the one of test_gpu_trace's test_fodo_128_elements_shared_beam_k1_scan.
    """
    B = 64 if beam_type == "particles" else 300
    scale = np.linspace(0.6, 1.1, B).astype(np.float32)
    specs = o.fodo_segment(32, dtype=np.float32, batch_shape=(B,), k1_scale=scale)
    sigma = np.array([1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    one = o.gaussian_particles((1,), 100_000, seed=4, dtype=np.float32, sigma=sigma)

    def gradients(dtype):
        cast = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)  # noqa: E731  (the float32 lattice's own numbers)
        elements = [lx.Quadrupole(cast(s["length"]), k1=cast(s["k1"]), dtype=dtype) if s["kind"] == "quadrupole"
                    else lx.Drift(cast(s["length"]), dtype=dtype) for s in specs]
        if beam_type == "particles":
            beam = lx.ParticleBeam(one.astype(dtype), np.array([1e8], dtype=dtype), dtype=dtype).broadcast((B,))
            assert beam.is_shared
        else:
            mu = np.zeros((B, 7), dtype=dtype)
            mu[:, 6] = 1
            cov = np.zeros((B, 7, 7), dtype=dtype)
            cov[:, range(6), range(6)] = (sigma**2).astype(np.float32).astype(dtype)
            beam = lx.ParameterBeam(mu, cov, np.full(B, 1e8, dtype=dtype), dtype=dtype)
        vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam)
        assert vjp.trace.num_points == 129
        g = vjp(beta_x=1.0, beta_y=1.0)
        out = {"k1": [], "length": [], "energy": [np.asarray(g.energy, dtype=np.float64)]}
        for el, s in zip(elements, specs):
            got = g[el]
            out["length"].append(np.asarray(got["length"], dtype=np.float64))
            if s["kind"] == "quadrupole":
                out["k1"].append(np.asarray(got["k1"], dtype=np.float64))
        return {name: np.stack(rows) for name, rows in out.items()}

    g32, g64 = gradients(np.float32), gradients(np.float64)
    measured = {}
    for name, ref in g64.items():
        got = g32[name]
        assert got.shape == ref.shape and np.all(np.isfinite(got)), name
        measured[name] = float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.max(np.abs(ref)) + 1e-300)))
    print(f"float32 track_along_vjp against float64, {beam_type}: " + ", ".join(f"{k} {v:.1e}" for k, v in measured.items()))
    for name, value in measured.items():
        assert value <= TOL_TRACE_GRAD[beam_type][name], (name, value)


def test_shapes_repeats_and_repeated_elements(lx):
    dtype = np.float64
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    rng = np.random.default_rng(2)
    particles = o.gaussian_particles((3,), 2000, seed=3, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    energy = np.array([1e8, 1.1e8, 1.2e8])
    beam = lx.ParticleBeam(particles, energy, dtype=dtype)

    def line(shape):
        full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
        return [lx.Quadrupole(full(0.2), k1=full(3.0), name="Q1", dtype=dtype), lx.Drift(full(0.5), dtype=dtype),
                lx.Quadrupole(full(0.2), k1=full(-3.0), name="Q2", dtype=dtype), lx.Drift(full(0.7), dtype=dtype)]

    # parameters of shape (1,) against a batch of 3: summed over the batch
    shared, batched = lx.Segment(line((1,))), lx.Segment(line((3,)))
    vjp = lx.grad.track_along_vjp(shared, beam)
    assert vjp.trace.mu.shape == (3, 5, 6)
    g1 = vjp(beta_x=1.0, sigma_y=2.0)
    g3 = lx.grad.track_along_vjp(batched, beam)(beta_x=1.0, sigma_y=2.0)
    assert g1[shared.Q1]["k1"].shape == (1,) and g3[batched.Q1]["k1"].shape == (3,)
    assert np.allclose(g1[shared.Q1]["k1"], g3[batched.Q1]["k1"].sum(), rtol=1e-12)
    assert np.allclose(g1[shared.elements[3]]["length"], g3[batched.elements[3]]["length"].sum(), rtol=1e-12)
    assert g1.energy.shape == (3,) and g1.mu.shape == (3, 7) and g1.cov.shape == (3, 7, 7)
    # a scalar property cotangent is the array of that value; a second call of the same vjp; the same bits twice
    again = vjp(beta_x=np.full((3, 5), 1.0), sigma_y=np.full((3, 5), 2.0))
    assert np.array_equal(again[shared.Q1]["k1"], g1[shared.Q1]["k1"]) and np.array_equal(again.energy, g1.energy)
    assert np.array_equal(again.cov, g1.cov)
    part_a, part_b = vjp(beta_x=1.0), vjp(sigma_y=2.0)
    assert not np.array_equal(part_a[shared.Q2]["k1"], g1[shared.Q2]["k1"])
    assert np.allclose(part_a[shared.Q2]["k1"] + part_b[shared.Q2]["k1"], g1[shared.Q2]["k1"], rtol=1e-10)
    # batch shape (2, 3)
    particles23 = o.gaussian_particles((2, 3), 1000, seed=5, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    k1 = rng.uniform(1, 4, size=(2, 3))
    w = rng.normal(size=(2, 3, 4))

    def grads(shape):
        seg = lx.Segment([lx.Quadrupole(np.full(shape, 0.2), k1=k1.reshape(shape), name="Q", dtype=dtype),
                          lx.Drift(np.full(shape, 0.5), dtype=dtype), lx.Marker(name="M")])
        b = lx.ParticleBeam(particles23.reshape(*shape, 1000, 7), np.full(shape, 1e8), dtype=dtype)
        g = lx.grad.track_along_vjp(seg, b)(sigma_x=w.reshape(*shape, 4), alpha_x=1.0)
        return g[seg.Q]["k1"], g.energy, g.mu
    k23, e23, m23 = grads((2, 3))
    k6, e6, m6 = grads((6,))
    assert k23.shape == (2, 3) and e23.shape == (2, 3) and m23.shape == (2, 3, 7)
    assert np.array_equal(k23.reshape(6), k6) and np.array_equal(e23.reshape(6), e6) and np.array_equal(m23.reshape(6, 7), m6)
    # the same element object twice in the lattice: its gradients are added up
    q, d = lx.Quadrupole(f(0.2), k1=f(3.0), dtype=dtype), lx.Drift(f(0.5), dtype=dtype)
    twice = lx.Segment([q, d, q, d])
    apart = lx.Segment([lx.Quadrupole(f(0.2), k1=f(3.0), dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                        lx.Quadrupole(f(0.2), k1=f(3.0), dtype=dtype), lx.Drift(f(0.5), dtype=dtype)])
    gt = lx.grad.track_along_vjp(twice, beam)(beta_y=1.0)
    ga = lx.grad.track_along_vjp(apart, beam)(beta_y=1.0)
    assert np.allclose(gt[q]["k1"], ga[apart.elements[0]]["k1"] + ga[apart.elements[2]]["k1"], rtol=1e-12)
    assert np.allclose(gt[d]["length"], ga[apart.elements[1]]["length"] + ga[apart.elements[3]]["length"], rtol=1e-12)
    # a ParameterBeam without cotangents of the energy, float32
    beam32 = lx.ParameterBeam.from_parameters(sigma_x=np.full(3, 1.75e-4, np.float32), sigma_xp=np.full(3, 3.7e-6, np.float32),
                                              energy=np.full(3, 1e8, np.float32))
    seg32 = lx.Segment([lx.Quadrupole(np.full(1, 0.2, np.float32), k1=np.full(1, 3.0, np.float32), name="Q"),
                        lx.Drift(np.full(1, 0.5, np.float32))])
    g32 = lx.grad.track_along_vjp(seg32, beam32)(sigma_x=1.0)
    assert g32[seg32.Q]["k1"].dtype == np.float32 and g32[seg32.Q]["k1"].shape == (1,) and np.all(np.isfinite(g32.cov))


def test_match_twiss_along_lattice_example_converges(lx):
    """examples/match_twiss_along_lattice.py: Adam on four quadrupoles until beta_x, beta_y at three markers are the targets."""
    spec = importlib.util.spec_from_file_location(
        "match_twiss_along_lattice", pathlib.Path(__file__).resolve().parents[1] / "examples" / "match_twiss_along_lattice.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.matching_line(), example.incoming_beam()
    history = example.tune(segment, beam)
    assert history[-1] < 0.05 * history[0], (history[0], history[-1])
    trace = segment.track_along(beam)
    for marker, (beta_x, beta_y) in example.TARGETS.items():
        k = trace.index_of(marker)
        assert abs(float(trace.beta_x[0, k]) / beta_x - 1) < 0.05, (marker, trace.beta_x[0, k], beta_x)
        assert abs(float(trace.beta_y[0, k]) / beta_y - 1) < 0.05, (marker, trace.beta_y[0, k], beta_y)
