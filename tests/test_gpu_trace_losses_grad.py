"""
`lynx_amd.grad.track_along_vjp(..., losses=True)` on the GPU (lynx_moments_by_loss,
lynx_track_particles_along_backward_losses): the moment records of the nested survivor sets against NumPy, the gradients of
the SURVIVING beam's moments at every point against central differences of the oracle's element-by-element particle chain
with the survivors of every point taken in float64, properties and BPM readings, the lattice that loses nobody against the
plain reverse pass, float32 against the float64 pass, shapes, a sample nobody survives in, and the example.

The finite differences need a condition on the inputs: the survivor sets are held fixed by the reverse pass, so EVERY
perturbed evaluation of the reference must have the unperturbed `lost_at` -- asserted inside the reference loss; the
seeds below were picked on the host, with the oracle alone, so that it holds.
"""

import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import build
from .test_gpu_parity import TOL_MOM
from .test_gpu_trace_grad import _check_parameters, _particle_lattice, _worst_distance
from .trace_grad_cases import _moments_of, _sized_apertures, _survivor_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _tri(i, j):
    return 7 + i * 6 - (i * (i - 1)) // 2 + (j - i)


# ---------------------------------------------------------------------------------------------
# 1. the set records
# ---------------------------------------------------------------------------------------------

SET_SIZES = (1, 63, 64, 65, 257, 4097)


def _lost_at(rng, B, n, A):
    """Sample 0 loses nobody, sample 1 everybody at the first aperture, the others at random -- without ordinal A // 2."""
    ordinals = [k for k in range(-1, A) if A == 1 or k != A // 2]
    lost_at = rng.choice(ordinals, size=(B, n)).astype(np.int32)
    lost_at[0], lost_at[1] = -1, 0
    return lost_at


def _set_reference(p, lost_at, A):
    """Two-pass mean and biased covariance of every set in float64: (counts (B, A + 1), mean (.., 6), cov (.., 6, 6))."""
    B, n = lost_at.shape
    q = np.broadcast_to(np.asarray(p, dtype=np.float64), (B, n, 7))[..., :6]
    counts, mean, cov = np.zeros((B, A + 1)), np.full((B, A + 1, 6), np.nan), np.full((B, A + 1, 6, 6), np.nan)
    for b in range(B):
        for j in range(A + 1):
            members = q[b][(lost_at[b] == -1) | (lost_at[b] >= j)]
            counts[b, j] = len(members)
            if len(members):
                mean[b, j] = members.mean(axis=0)
                d = members - mean[b, j]
                cov[b, j] = d.T @ d / len(members)
    return counts, mean, cov


def _set_records(lx, p, lost_at, A, shared):
    rt = lx.device.get_runtime()
    B, n = lost_at.shape
    d_p, d_lost = rt.to_device(np.ascontiguousarray(p)), rt.to_device(np.ascontiguousarray(lost_at))
    out = rt.empty((B, A + 1, 36), np.float64)
    rt.check(rt.lib.lynx_moments_by_loss(rt.ctx, 1 if p.dtype == np.float64 else 0, B, n, C.c_void_p(d_p.ptr),
                                         lx._ffi.TRACK_SHARED_INPUT if shared else 0, A, C.c_void_p(d_lost.ptr), C.c_void_p(out.ptr)))
    return out.numpy().reshape(B, A + 1, 36)


@pytest.mark.parametrize("A", [1, 3, 15])
@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "shared"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_records_of_the_nested_survivor_sets_against_numpy(lx, dtype, shared, A):
    B = 3
    worst = 0.0
    for n in SET_SIZES:
        rng = np.random.default_rng(1000 * A + n)
        p = o.gaussian_particles((1,) if shared else (B,), n, seed=n, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3],
                                 mu=[2e-4, 0.0, -1e-4, 1e-5, 0.0, 1e-3])
        p = p[0] if shared else p
        lost_at = _lost_at(rng, B, n, A)
        counts, mean, cov = _set_reference(p, lost_at, A)
        rec = _set_records(lx, p, lost_at, A, shared)
        assert np.array_equal(rec[..., 35], counts), (n, rec[..., 35], counts)
        assert np.all(rec[..., 34] == 1.0) and np.all(rec[..., 28:34] == 0.0)
        assert np.all(counts[0] == n) and np.all(counts[1, 1:] == 0) and counts[1, 0] == n
        # a set without particles: NaN moments; the others: finite
        nobody = counts == 0
        assert np.isnan(rec[nobody][:, :28]).all() and np.isfinite(rec[~nobody][:, :28]).all()
        for b in range(B):
            for j in range(A + 1):
                if counts[b, j] == 0:
                    continue
                got_mean = rec[b, j, :6]
                got_cov = np.array([[rec[b, j, _tri(min(r, c), max(r, c))] for c in range(6)] for r in range(6)])
                assert rec[b, j, 6] == 1.0
                if counts[b, j] == 1:
                    # one particle, and (a condition on the inputs) one of the 64 reference candidates of include/lynx_hip.h,
                    # particle floor(l n / 64): the only candidate in the innermost set, hence the reference point of its
                    # own sums -- its coordinates are the means, and the covariance is 0 exactly, as the oracle's is
                    member = int(np.flatnonzero((lost_at[b] == -1) | (lost_at[b] >= j))[0])
                    assert member in {(l * n) // 64 for l in range(64)}, (n, b, j, member)
                    assert np.all(np.abs(got_mean - mean[b, j]) <= TOL_MOM[dtype] * np.abs(mean[b, j])), (n, b, j)
                    assert np.all(got_cov == 0), (n, b, j)
                    continue
                sigma = np.sqrt(np.diag(cov[b, j]))
                d_mean = np.abs(got_mean - mean[b, j]) / (np.abs(mean[b, j]) + sigma)
                d_sigma = np.abs(np.sqrt(np.diag(got_cov)) - sigma) / sigma
                d_cov = np.abs(got_cov - cov[b, j]) / np.outer(sigma, sigma)
                here = max(d_mean.max(), d_sigma.max(), d_cov[~np.eye(6, dtype=bool)].max())
                assert here <= TOL_MOM[dtype], (n, b, j, counts[b, j], d_mean, d_sigma, d_cov)
                worst = max(worst, float(here))
        again = _set_records(lx, p, lost_at, A, shared)
        assert np.array_equal(again, rec, equal_nan=True), n
    print(f"set records, {np.dtype(dtype).name}, A = {A}, {'shared' if shared else 'per sample'}: worst distance {worst:.1e}")


def test_the_entry_points_refuse_bad_arguments_before_any_launch(lx):
    rt = lx.device.get_runtime()
    p = o.gaussian_particles((2,), 64, seed=1, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    d_p, d_lost, out = rt.to_device(p), rt.to_device(np.full((2, 64), -1, dtype=np.int32)), rt.empty((2, 17, 36), np.float64)
    ptr = lambda a: C.c_void_p(a.ptr)  # noqa: E731
    for args in ((1, 2, 64, ptr(d_p), 0, 16, ptr(d_lost), ptr(out)), (1, 2, 64, ptr(d_p), 0, 0, ptr(d_lost), ptr(out)),
                 (1, 2, 0, ptr(d_p), 0, 1, ptr(d_lost), ptr(out)), (1, 2, 64, None, 0, 1, ptr(d_lost), ptr(out)),
                 (1, 2, 64, ptr(d_p), 0, 1, None, ptr(out)), (1, 2, 64, ptr(d_p), 0, 1, ptr(d_lost), None)):
        assert rt.lib.lynx_moments_by_loss(rt.ctx, *args) != 0
        assert rt.lib.lynx_last_error(rt.ctx).decode().startswith("moments by loss: "), args
    # the reverse entry point, on the lattice of a trace with two apertures (steps 1 and 3)
    f = lambda v: np.array([v, v], dtype=np.float64)  # noqa: E731
    aperture = lambda name: lx.Aperture(x_max=f(1.0), y_max=f(1.0), is_active=True, name=name, dtype=np.float64)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(1.0), dtype=np.float64), aperture("A0"), lx.Quadrupole(f(0.2), k1=f(1.0), dtype=np.float64),
                          aperture("A1"), lx.Drift(f(1.0), dtype=np.float64)])
    beam = lx.ParticleBeam(p, f(1e8), dtype=np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, losses=True)
    lat = lx.engine._ready(segment._trace_cache, vjp.program, (2,), np.float64, beam._energy._host)
    e_in = beam._energy.broadcast_device(rt, (2,))
    bar, sets = rt.to_device(np.zeros((2, 6, 36))), rt.to_device(np.zeros((2, 17, 36)))
    g_par, g_en = rt.empty((2, 5, 8), np.float64), rt.empty((2,), np.float64)

    def call(steps, n=None):
        at = (C.c_int32 * max(len(steps), 1))(*steps)
        return rt.lib.lynx_track_particles_along_backward_losses(
            rt.ctx, lat.handle, 64, ptr(e_in), ptr(vjp.trace._device["records"]), ptr(bar), None, len(steps) if n is None else n, at,
            ptr(sets), ptr(g_par), ptr(g_en))

    assert call([1, 3]) == 0
    for steps, n in (([3, 1], None), ([1, 1], None), ([1, 2], None), ([0, 3], None), ([1, 5], None), ([1, 3], 16), ([1, 3], 0)):
        assert call(steps, n) != 0, (steps, n)
        assert rt.lib.lynx_last_error(rt.ctx).decode().startswith("beam trace gradients with losses: "), (steps, n)


# ---------------------------------------------------------------------------------------------
# the reference: the oracle's particle chain with the survivors of every point
# ---------------------------------------------------------------------------------------------


def _fd_case():
    """`_particle_lattice` with a rectangular aperture in front of the dipole and an elliptical one in front of the last quadrupole."""
    rng = np.random.default_rng(42)
    B, N = 2, 400
    plain = _particle_lattice(B, rng)
    particles = o.gaussian_particles((B,), N, seed=FD_SEED, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6])
    desc = _sized_apertures(plain, particles, energy, places=[3, 6], fractions=[1.4, 2.2])
    P = len(desc) + 1
    w_mu = rng.normal(size=(B, P, 6))
    w_cov = rng.normal(size=(B, P, 6, 6)) * 1e3
    w_e = rng.normal(size=(B, P)) * 1e-10
    return desc, particles, energy, w_mu, w_cov, w_e


FD_SEED = 9  # gaussian_particles seed of `_fd_case`: no survivor set moves under any step of the central differences


def _survivor_loss(desc, specs, particles, energy, energy_0, lost_at_0, w_mu, w_cov, w_e):
    """sum over the points of <w_mu, mean> + <w_cov, cov> of the particles alive there + w_e (E - E_0), per sample."""
    beams, masks, lost_at, _ = _survivor_chain(desc, specs, particles, energy)
    assert np.array_equal(lost_at, lost_at_0), "a survivor set moved under a finite-difference step: pick another seed"
    total = np.zeros(particles.shape[:-2])
    for k, b in enumerate(beams):
        mean, cov = _moments_of(b["particles"][..., :6], masks[k])
        total += np.sum(w_mu[:, k] * mean, axis=-1) + np.sum(w_cov[:, k] * cov, axis=(-1, -2))
        total += w_e[:, k] * (b["energy"] - energy_0)
    return total


def test_gradients_of_the_survivors_moments_match_finite_differences_of_the_particle_chain_fp64(lx):
    """
    B = 2, N = 400, a rectangular and an elliptical active aperture, random cotangents of mean, covariance and energy at
    ALL points; the reference is the central difference of the particle chain's loss over the survivors of every point.
    """
    desc, particles, energy, w_mu, w_cov, w_e = _fd_case()
    B, N = particles.shape[:2]
    elements, specs = build(desc, np.float64, lx)
    _, _, lost_at, margin = _survivor_chain(desc, specs, particles, energy)
    survive = (lost_at == -1).mean(axis=-1)
    print(f"survivors {survive.tolist()}, lost per aperture {[(lost_at == k).sum(axis=-1).tolist() for k in (0, 1)]}, "
          f"closest particle {margin:.1e} from an edge")
    assert np.all(survive >= 0.25) and np.all(survive <= 0.75), survive
    assert np.all((lost_at == 0).sum(axis=-1) > 0) and np.all((lost_at == 1).sum(axis=-1) > 0)

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), losses=True)
    assert vjp.trace.num_points == len(desc) + 1
    assert np.array_equal(vjp.trace.lost_at, lost_at)
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    assert g.mu is None and g.cov is None

    def loss(energy_):
        return _survivor_loss(desc, specs, particles, energy_, energy, lost_at, w_mu, w_cov, w_e)

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss(energy)
        apply(x0 - h)
        down = loss(energy)
        apply(x0)
        return (up - down) / (2 * h)

    assert _check_parameters(desc, specs, elements, g, central, w_cov) > 40
    for bidx in range(B):
        h = 1e-6 * energy[bidx]
        ep, em = energy.copy(), energy.copy()
        ep[bidx] += h
        em[bidx] -= h
        ref = (loss(ep)[bidx] - loss(em)[bidx]) / (2 * h)
        assert abs(g.energy[bidx] - ref) <= 2e-4 * abs(ref) + 1e-12, (bidx, g.energy[bidx], ref)
    # the survivor set is held fixed: the limits that made it get gradient 0
    for k, (kind, _) in enumerate(desc):
        if kind == "aperture":
            assert elements[k] in g and np.all(g[elements[k]]["x_max"] == 0) and g[elements[k]]["y_max"].shape == (B,)


# ---------------------------------------------------------------------------------------------
# 3. properties and readings
# ---------------------------------------------------------------------------------------------

PROPERTY_SEED = 21


def test_properties_and_bpm_readings_of_the_collimated_beam_fp64(lx):
    """
    One collimator, an active BPM behind it: `vjp(sigma_x=w, beta_y=w2, readings={bpm: r})` against central differences of
    the same properties of the oracle's survivors -- `ParticleBeam._std` with each point's own count and LYNX_STD_DDOF.
    """
    from lynx_amd import config

    rng = np.random.default_rng(8)
    B, N = 2, 400
    f = lambda v: np.full(B, v)  # noqa: E731
    plain = [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=np.array([3.0, -2.0]), misalignment=rng.normal(0, 1e-4, (B, 2)))),
             ("hcor", dict(length=f(0.1), angle=np.array([2e-4, -1e-4]))), ("drift", dict(length=f(0.5))),
             ("quadrupole", dict(length=f(0.3), k1=np.array([-2.5, 3.5]))), ("bpm", dict(is_active=True)), ("drift", dict(length=f(0.4)))]
    particles = o.gaussian_particles((B,), N, seed=PROPERTY_SEED, dtype=np.float64, sigma=[1e-4, 2e-5, 1e-4, 2e-5, 1e-5, 1e-3],
                                     mu=[2e-5, 3e-6, -1e-5, 2e-6, 0.0, 0.0])
    energy = np.array([1e8, 1.2e8])
    desc = _sized_apertures(plain, particles, energy, places=[3], fractions=[1.3])
    elements, specs = build(desc, np.float64, lx)
    P = len(desc) + 1
    bpm_at = next(k for k, (kind, _) in enumerate(desc) if kind == "bpm")
    _, _, lost_at, margin = _survivor_chain(desc, specs, particles, energy)
    print(f"survivors {(lost_at == -1).mean(axis=-1).tolist()}, closest particle {margin:.1e} from the edge")
    assert np.all((lost_at == 0).sum(axis=-1) > 0.2 * N)
    w, w2, r = rng.normal(size=(B, P)), rng.normal(size=(B, P)), rng.normal(size=(2, B))

    def loss():
        beams, masks, la, _ = _survivor_chain(desc, specs, particles, energy)
        assert np.array_equal(la, lost_at), "the survivor set moved under a finite-difference step: pick another seed"
        total = np.zeros(B)
        for k, b in enumerate(beams):
            n = masks[k].sum(axis=-1)
            mean, cov = _moments_of(b["particles"][..., :6], masks[k])
            unbias = n / (n - config.std_ddof)
            sigma_x = np.sqrt(cov[:, 0, 0] * unbias)
            s2, p2, cross = cov[:, 2, 2] * unbias, cov[:, 3, 3] * unbias, cov[:, 2, 3]
            beta_y = s2 / np.sqrt(s2 * p2 - cross**2)
            total += w[:, k] * sigma_x + w2[:, k] * beta_y
            if k == bpm_at:  # the BPM reads the centroid of the particles that enter it
                total += r[0] * mean[:, 0] + r[1] * mean[:, 2]
        return total

    bpm = elements[bpm_at]
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), losses=True)
    assert np.array_equal(vjp.trace.lost_at, lost_at)
    beams, masks, _, _ = _survivor_chain(desc, specs, particles, energy)
    centroid, _ = _moments_of(beams[bpm_at]["particles"][..., :6], masks[bpm_at])
    assert np.allclose(bpm.reading, np.stack([centroid[:, 0], centroid[:, 2]]), rtol=1e-9, atol=1e-15)
    g = vjp(sigma_x=w, beta_y=w2, readings={bpm: r})

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss()
        apply(x0 - h)
        down = loss()
        apply(x0)
        return (up - down) / (2 * h)

    # (`_check_parameters` floors the scale of a gradient at 1e-9 max |w_cov|: here the cotangents are of order 1)
    assert _check_parameters(desc, specs, elements, g, central, np.ones(1)) >= 16


# ---------------------------------------------------------------------------------------------
# 4. nothing lost
# ---------------------------------------------------------------------------------------------


def test_apertures_that_remove_nobody_give_the_plain_gradients_fp64(lx):
    desc, particles, energy, w_mu, w_cov, w_e = _fd_case()
    for kind, kw in desc:
        if kind == "aperture":
            kw["x_max"], kw["y_max"] = kw["x_max"] * 1e3, kw["y_max"] * 1e3
    elements, _ = build(desc, np.float64, lx)
    segment, beam = lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, losses=True)
    assert np.all(vjp.trace.lost_at == -1) and np.all(vjp.trace.transmission == 1.0)
    got = vjp(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    assert got.mu is None
    for el in elements:
        if isinstance(el, lx.Aperture):
            el.is_active = False
    ref = lx.grad.track_along_vjp(segment, beam)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    worst = _worst_distance(desc, elements, got, elements, ref, w_cov)
    assert np.allclose(got.energy, ref.energy, rtol=2e-4, atol=1e-12)
    print(f"losses=True with nobody lost against the plain track_along_vjp: worst distance {worst:.1e}")
    # ... and `losses=True` on the lattice without an active aperture IS the plain call
    same = lx.grad.track_along_vjp(segment, beam, losses=True)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    assert np.array_equal(same.energy, ref.energy) and np.array_equal(same.mu, ref.mu)
    assert np.array_equal(same[elements[1]]["k1"], ref[elements[1]]["k1"])


def test_a_parameter_beam_passes_the_apertures_and_takes_the_plain_call(lx):
    dtype = np.float64
    f = lambda v: np.array([v, 1.1 * v], dtype=dtype)  # noqa: E731
    elements = [lx.Drift(f(0.5), dtype=dtype), lx.Aperture(x_max=f(1e-5), y_max=f(1e-5), is_active=True, name="C", dtype=dtype),
                lx.Quadrupole(f(0.2), k1=f(3.0), name="Q", dtype=dtype), lx.Drift(f(0.7), dtype=dtype)]
    segment = lx.Segment(elements)
    beam = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), energy=f(1e8), dtype=dtype)
    with pytest.raises(NotImplementedError, match="'C'"):
        lx.grad.track_along_vjp(segment, beam)
    got = lx.grad.track_along_vjp(segment, beam, losses=True)(beta_x=1.0, sigma_y=2.0)
    elements[1].is_active = False
    ref = lx.grad.track_along_vjp(segment, beam)(beta_x=1.0, sigma_y=2.0)
    assert np.all(ref[segment.Q]["k1"] != 0)
    assert np.array_equal(got[segment.Q]["k1"], ref[segment.Q]["k1"]) and np.array_equal(got[elements[0]]["length"], ref[elements[0]]["length"])
    assert np.array_equal(got.energy, ref.energy) and np.array_equal(got.mu, ref.mu) and np.array_equal(got.cov, ref.cov)


# ---------------------------------------------------------------------------------------------
# 5. float32 against the float64 pass
# ---------------------------------------------------------------------------------------------

# distance max |g - r| / (|r| + 1e-3 max |r|) of the float32 gradient g from the float64 pass r of the same input, per
# parameter name, as TOL_TRACE_GRAD of test_gpu_trace_grad measures it: twice what
# test_float32_against_the_float64_pass_on_128_elements_with_two_collimators measured on MI355X --
#                  B = 2 x 1000 particles, 130 elements, two collimators (40 % of the particles lost)
#     k1                     3.9e-05
#     length                 4.4e-05
#     energy                 0          (beta does not depend on the energy in this lattice)
# (TOL_TRACE_GRAD's plain-trace figures, 1.0e-3 / 1.7e-3, are of another input: 64 k1 scales down to 0.6, 100 000 particles.)
TOL_LOSSES_GRAD = {"k1": 7.8e-5, "length": 8.8e-5, "energy": 0.0}
F32_SEED = 28
COLLIMATORS_AT = (41, 90)  # in front of these elements of the 128-element channel


def _f32_case():
    B, N = 2, 1000
    scale = np.array([0.7, 1.0], dtype=np.float32)
    specs32 = o.fodo_segment(32, dtype=np.float32, batch_shape=(B,), k1_scale=scale)
    plain = [("quadrupole", dict(length=np.asarray(s["length"], dtype=np.float64), k1=np.asarray(s["k1"], dtype=np.float64)))
             if s["kind"] == "quadrupole" else ("drift", dict(length=np.asarray(s["length"], dtype=np.float64))) for s in specs32]
    one = o.gaussian_particles((1,), N, seed=F32_SEED, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    particles = np.broadcast_to(one.astype(np.float64), (B, N, 7)).copy()
    energy = np.full(B, 1e8)
    desc = _sized_apertures(plain, particles, energy, places=list(COLLIMATORS_AT), fractions=[1.5, 1.8])
    for kind, kw in desc:  # the limits are numbers both dtypes hold
        if kind == "aperture":
            kw["x_max"], kw["y_max"] = (np.asarray(kw[n], dtype=np.float32).astype(np.float64) for n in ("x_max", "y_max"))
    return desc, one, particles, energy


def test_float32_against_the_float64_pass_on_128_elements_with_two_collimators(lx):
    """
    `o.fodo_segment(32)` with two k1 scales, two collimators, B = 2 x 1000 shared particles, cotangents beta_x = beta_y = 1
    at every point.  Every particle stays 1e-3 of the limit away from every edge in the float64 oracle chain, so both
    dtypes lose the same particles.
    """
    desc, one, particles, energy = _f32_case()
    B = len(energy)
    _, specs = build(desc, np.float64)
    _, _, lost_at, margin = _survivor_chain(desc, specs, particles, energy)
    print(f"survivors {(lost_at == -1).mean(axis=-1).tolist()}, closest particle {margin:.1e} from an edge")
    assert margin >= 1e-3, margin
    assert np.all((lost_at == 0).sum(axis=-1) > 0) and np.all((lost_at == 1).sum(axis=-1) > 0) and np.all((lost_at == -1).mean(axis=-1) > 0.25)

    def gradients(dtype):
        elements, _ = build(desc, dtype, lx)  # (every number of `desc` is one float32 holds)
        beam = lx.ParticleBeam(one.astype(dtype), np.array([1e8], dtype=dtype), dtype=dtype).broadcast((B,))
        assert beam.is_shared
        vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, losses=True)
        assert vjp.trace.num_points == 131
        g = vjp(beta_x=1.0, beta_y=1.0)
        out = {"k1": [], "length": [], "energy": [np.asarray(g.energy, dtype=np.float64)]}
        for el, (kind, _) in zip(elements, desc):
            if kind == "aperture":
                continue
            out["length"].append(np.asarray(g[el]["length"], dtype=np.float64))
            if kind == "quadrupole":
                out["k1"].append(np.asarray(g[el]["k1"], dtype=np.float64))
        return {name: np.stack(rows) for name, rows in out.items()}, vjp.trace.lost_at

    (g32, lost32), (g64, lost64) = gradients(np.float32), gradients(np.float64)
    assert np.array_equal(lost64, lost_at) and np.array_equal(lost32, lost64)
    measured = {}
    for name, ref in g64.items():
        got = g32[name]
        assert got.shape == ref.shape and np.all(np.isfinite(got)), name
        measured[name] = float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.max(np.abs(ref)) + 1e-300)))
    print("float32 track_along_vjp(losses=True) against float64: " + ", ".join(f"{k} {v:.1e}" for k, v in measured.items()))
    assert np.any(g64["k1"] != 0)
    for name, value in measured.items():
        assert value <= TOL_LOSSES_GRAD[name], (name, value)


# ---------------------------------------------------------------------------------------------
# 6. shapes and sparsity
# ---------------------------------------------------------------------------------------------


def test_batch_shapes_a_sample_nobody_survives_in_and_the_same_bits_twice(lx):
    dtype = np.float64
    shape, N = (2, 2), 300
    full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    particles = o.gaussian_particles(shape, N, seed=5, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    k1 = np.array([[3.0, 2.0], [1.0, 4.0]])
    second = full(1.5e-4)
    second[1, 0] = 0.0  # nobody passes |x| < 0: sample (1, 0) has no particle behind the second collimator

    def line(shp):
        r = lambda v: np.asarray(v, dtype=dtype).reshape(shp)  # noqa: E731
        return lx.Segment([lx.Quadrupole(r(full(0.2)), k1=r(k1), name="Q1", dtype=dtype), lx.Drift(r(full(0.5)), name="D1", dtype=dtype),
                           lx.Aperture(x_max=r(full(1.2e-4)), y_max=r(full(1.2e-4)), shape="elliptical", is_active=True, name="C1", dtype=dtype),
                           lx.Quadrupole(r(full(0.2)), k1=r(-k1), name="Q2", dtype=dtype), lx.Drift(r(full(0.5)), name="D2", dtype=dtype),
                           lx.Aperture(x_max=r(second), y_max=r(full(1.5e-4)), is_active=True, name="C2", dtype=dtype),
                           lx.Drift(r(full(0.7)), name="D3", dtype=dtype), lx.Marker(name="M")])

    def beam(shp):
        return lx.ParticleBeam(particles.reshape(*shp, N, 7), np.full(shp, 1e8), dtype=dtype)

    segment = line(shape)
    vjp = lx.grad.track_along_vjp(segment, beam(shape), losses=True)
    trace = vjp.trace
    P = trace.num_points
    assert P == 9 and trace.num_survivors.shape == (2, 2, P)
    assert np.all(trace.num_survivors[1, 0, 6:] == 0) and np.all(trace.num_survivors[1, 0, :6] > 0)
    reached = trace.num_survivors > 0
    assert np.all(reached[[0, 0, 1], [0, 1, 1]]) and np.all(trace.num_survivors[..., -1][[0, 0, 1], [0, 1, 1]] > 0.2 * N)
    rng = np.random.default_rng(6)
    w_mu = rng.normal(size=(2, 2, P, 6)) * reached[..., None]
    w_cov = rng.normal(size=(2, 2, P, 6, 6)) * 1e3 * reached[..., None, None]
    w_sigma = rng.normal(size=(2, 2, P)) * reached
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, sigma_x=w_sigma, energy_bar=1e-10)
    for name, param in (("Q1", "k1"), ("Q2", "k1"), ("D1", "length"), ("D2", "length"), ("D3", "length")):
        got = g[getattr(segment, name)][param]
        assert got.shape == (2, 2) and np.all(np.isfinite(got)), (name, got)
        assert np.all(got[[0, 0, 1], [0, 1, 1]] != 0), (name, got)
    assert g[segment.D3]["length"][1, 0] == 0  # behind the collimator nobody passes: no cotangent, no gradient
    assert g[segment.Q1]["k1"][1, 0] != 0 and g.energy.shape == (2, 2) and np.all(np.isfinite(g.energy))
    assert g.mu is None and g.cov is None
    # a cotangent where nobody is: refused, by sample and point
    bad = w_mu.copy()
    bad[1, 0, 7, 0] = 1.0
    with pytest.raises(ValueError, match=r"sample \(1, 0\), point 7"):
        vjp(mu_bar=bad)
    bad_sigma = w_sigma.copy()
    bad_sigma[1, 0, 6] = 0.5
    with pytest.raises(ValueError, match=r"'sigma_x'.*sample \(1, 0\), point 6"):
        vjp(sigma_x=bad_sigma)
    # the same call twice: the same bits
    again = vjp(mu_bar=w_mu, cov_bar=w_cov, sigma_x=w_sigma, energy_bar=1e-10)
    for name, param in (("Q1", "k1"), ("Q2", "k1"), ("D2", "length")):
        assert np.array_equal(again[getattr(segment, name)][param], g[getattr(segment, name)][param]), name
    assert np.array_equal(again.energy, g.energy)
    # batch (2, 2) is batch (4,)
    flat = line((4,))
    g4 = lx.grad.track_along_vjp(flat, beam((4,)), losses=True)(
        mu_bar=w_mu.reshape(4, P, 6), cov_bar=w_cov.reshape(4, P, 6, 6), sigma_x=w_sigma.reshape(4, P), energy_bar=1e-10)
    assert np.array_equal(g4[flat.Q2]["k1"], g[segment.Q2]["k1"].reshape(4)) and np.array_equal(g4.energy, g.energy.reshape(4))


# ---------------------------------------------------------------------------------------------
# 7. the example
# ---------------------------------------------------------------------------------------------


def test_tune_behind_collimator_example_converges(lx):
    """examples/tune_behind_collimator.py: Adam on two quadrupoles until the collimated beam has the target sizes at SCREEN."""
    spec = importlib.util.spec_from_file_location(
        "tune_behind_collimator", pathlib.Path(__file__).resolve().parents[1] / "examples" / "tune_behind_collimator.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.collimated_line(), example.incoming_beam(5000)
    history = example.tune(segment, beam, steps=80)
    assert history[-1][0] < 0.05 * history[0][0], (history[0], history[-1])
    trace = segment.track_along(beam, losses=True)
    k = trace.index_of("SCREEN")
    assert 0.3 < float(trace.transmission[0, k]) < 0.9
    assert abs(float(trace.sigma_x[0, k]) / example.TARGET[0] - 1) < 0.05, (trace.sigma_x[0, k], example.TARGET)
    assert abs(float(trace.sigma_y[0, k]) / example.TARGET[1] - 1) < 0.05, (trace.sigma_y[0, k], example.TARGET)
