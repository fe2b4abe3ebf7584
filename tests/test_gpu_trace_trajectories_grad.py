"""
`track_along_vjp(..., trajectories=)` / `vjp(trajectories_bar=)` on the GPU (k_trace_trajectories_bwd behind
lynx_track_particles_along_backward_trajectories).  The reference is always central differences of the oracle's float64
particle chain on the K chosen particles alone -- particles do not interact, so that chain is `o.element_track` element
by element -- never the code under test.
"""

import ctypes as C
import importlib.util
import pathlib
import re

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice
from .test_gpu_grad import PARAMS_TO_CHECK, _desc
from .test_gpu_trace_grad import _chain, _particle_lattice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _loss(specs, chosen, energy, w, w_e=None, e_ref=None):
    """sum over points, chosen particles and coordinates of w z, per sample; `w` (B, P, K, 6|7), `chosen` (B, K, 7)."""
    k = w.shape[-1]
    total = np.zeros(chosen.shape[0])
    for point, beam in enumerate(_chain(specs, o.particle_beam(chosen, energy, np.float64))):
        total += np.sum(w[:, point] * beam["particles"][..., :k], axis=(-1, -2))
        if w_e is not None:  # (relative to the unperturbed energy: see test_gpu_trace_grad)
            total += w_e[:, point] * (beam["energy"] - e_ref[:, point])
    return total


def _central(loss, apply, x0):
    h = 1e-6 * max(abs(x0), 1e-2)
    apply(x0 + h)
    up = loss()
    apply(x0 - h)
    down = loss()
    apply(x0)
    return (up - down) / (2 * h)


def _close(got, ref, what):
    """The project's finite-difference tolerance; entries below 1e-9 of the parameter's largest are compared absolutely."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    floor = 1e-9 * np.max(np.abs(ref))
    bound = 2e-4 * np.maximum(np.abs(ref), floor) + 1e-7 * np.max(np.abs(got))
    assert np.all(np.abs(got - ref) <= bound), (what, got, ref)


def _parameter_references(desc, specs, loss):
    """Central differences for every parameter of PARAMS_TO_CHECK of every element: {(element, name): array like the parameter}."""
    out = {}
    for e, (kind, _) in enumerate(desc):
        for name in PARAMS_TO_CHECK.get(kind, []):
            arr = specs[e][name]
            if arr is None:
                continue
            ref = np.zeros(arr.shape)
            for idx in np.ndindex(arr.shape):
                def apply(x, arr=arr, idx=idx):
                    arr[idx] = x
                ref[idx] = _central(loss, apply, arr[idx])[idx[0]]
            out[(e, name)] = ref
    return out


def _energy_reference(loss_of_energy, energy):
    ref = np.zeros(len(energy))
    for b in range(len(energy)):
        h = 1e-6 * energy[b]
        up, down = energy.copy(), energy.copy()
        up[b] += h
        down[b] -= h
        ref[b] = (loss_of_energy(up)[b] - loss_of_energy(down)[b]) / (2 * h)
    return ref


def _particle_reference(loss_of_particles, chosen, columns=7):
    ref = np.zeros((*chosen.shape[:2], 7))
    for b in range(chosen.shape[0]):
        for j in range(chosen.shape[1]):
            for c in range(columns):
                h = 1e-7
                up, down = chosen.copy(), chosen.copy()
                up[b, j, c] += h
                down[b, j, c] -= h
                ref[b, j, c] = (loss_of_particles(up)[b] - loss_of_particles(down)[b]) / (2 * h)
    return ref


def test_an_affine_lattice_matches_finite_differences_of_the_chosen_particles_chain_fp64(lx):
    """
    test_gpu_trace_grad's particle lattice (every kind, a corrector of zero length, batched parameters), B = 2, N = 200,
    five chosen particles, unordered and with a repeat, a random cotangent on all six coordinates at all points.
    """
    rng = np.random.default_rng(17)
    B, N, selection = 2, 200, [5, 0, 199, 5, 17]
    desc = _particle_lattice(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P, K = len(desc) + 1, len(selection)
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6])
    w = rng.normal(size=(B, P, K, 6))
    w[:, :, 3] = w[:, :, 0]  # (rows 0 and 3 are the same particle: equal cotangents on the two rows of the repeated index)
    chosen = particles[:, selection]

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), trajectories=selection)
    assert vjp.trace.trajectories.shape == (B, P, K, 7)
    reference_chain = np.stack([b["particles"] for b in _chain(specs, o.particle_beam(chosen, energy, np.float64))], axis=1)
    assert np.allclose(vjp.trace.trajectories, reference_chain, rtol=1e-9, atol=1e-15)
    g = vjp(trajectories_bar=w)

    for (e, name), ref in _parameter_references(desc, specs, lambda: _loss(specs, chosen, energy, w)).items():
        _close(g[elements[e]][name], ref, (desc[e][0], e, name))
    _close(g.energy, _energy_reference(lambda en: _loss(specs, chosen, en, w), energy), "energy")
    got = g.chosen_particles
    assert got.shape == (B, K, 7)
    _close(got, _particle_reference(lambda p: _loss(specs, p, energy, w), chosen), "chosen_particles")
    assert np.array_equal(got[:, 0], got[:, 3])  # the repeated index, equal cotangents: bit for bit
    with pytest.raises(KeyError):  # no moment cotangent in the call: the moment path did not run
        g.mu
    # a cotangent on the 7th column is accepted and lands on the 7th column
    w7 = np.concatenate([w, rng.normal(size=(B, P, K, 1))], axis=-1)
    g7 = vjp(trajectories_bar=w7)
    assert np.allclose(g7.chosen_particles[..., 6] - got[..., 6], w7[..., 6].sum(axis=1), rtol=1e-12)
    assert np.array_equal(g7.chosen_particles[..., :6], got[..., :6])


def test_a_particle_beam_is_differentiated_through_cavities_fp64(lx):
    """
    test_gpu_grad's nine-element lattice with its two gaining cavities, a ParticleBeam, K = 3: `trajectories_bar` and
    `energy_bar` only.  Voltage, phase, frequency, the magnets and the incoming energy against the chain's differences.
    """
    rng = np.random.default_rng(23)
    B, N, selection = 2, 40, [7, 0, 31]
    desc = _desc(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    P, K = len(desc) + 1, len(selection)
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6])
    w = rng.normal(size=(B, P, K, 6))
    w_e = rng.normal(size=(B, P)) * 1e-10
    chosen = particles[:, selection]
    e_ref = np.stack([b["energy"] for b in _chain(specs, o.particle_beam(chosen, energy, np.float64))], axis=-1)

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), trajectories=selection)
    assert np.allclose(vjp.trace.energy, e_ref, rtol=1e-12)
    g = vjp(trajectories_bar=w, energy_bar=w_e)

    loss = lambda p=chosen, en=energy: _loss(specs, p, en, w, w_e, e_ref)  # noqa: E731
    references = _parameter_references(desc, specs, loss)
    assert sum(name in ("voltage", "phase", "frequency") for _, name in references) == 6
    for (e, name), ref in references.items():
        _close(g[elements[e]][name], ref, (desc[e][0], e, name))
    _close(g.energy, _energy_reference(lambda en: loss(en=en), energy), "energy")
    _close(g.chosen_particles[..., :6], _particle_reference(lambda p: loss(p=p), chosen, columns=6)[..., :6], "chosen_particles")
    first = next(el for el, (kind, _) in zip(elements, desc) if kind == "cavity")
    with pytest.raises(NotImplementedError, match=re.escape(repr(first.name))):
        vjp(mu_bar=np.ones((B, P, 6)))


# distance max |g - r| / (|r| + 1e-3 max |r|) of the float32 gradient g from central differences r of the oracle's float64
# chain, per parameter name: twice what test_float32_on_128_elements measured on MI355X --
#     k1        1.3e-04
#     length    2.5e-04
#     energy    0          (x and y do not depend on the energy in a lattice of quadrupoles and drifts: g and r are zero)
# test_tile_edges has names this table has no figure for -- a corrector's `angle`, `chosen_particles`, and `energy`, which
# is not zero there (the cotangent is on s as well) -- and takes the largest limit of the table for them: they go through
# the same maps and the same sums as k1 and length do.  (Measured there, three elements: 2.5e-08 .. 6.7e-07.)
TOL_TRAJECTORY_GRAD = {"k1": 2.6e-4, "length": 5.0e-4, "energy": 0.0}


def _distance(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-3 * np.max(np.abs(ref)) + 1e-300)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("K", [1, 64, 65, 128, 129])
def test_tile_edges(lx, dtype, K):
    """
    K = 65 puts one particle into a lane's second slot, K = 129 one into the wave's second tile.  The cotangent is nonzero
    for the LAST chosen particle at the LAST point and for the first at point 0 only: every other row of `chosen_particles`
    is exactly zero, and the parameters see the last particle alone.
    """
    rng = np.random.default_rng(3)
    B, N = 2, 130
    desc = [("drift", dict(length=np.full(B, 0.7))), ("quadrupole", dict(length=np.full(B, 0.2), k1=np.array([3.0, -2.0]))),
            ("hcor", dict(length=np.full(B, 0.1), angle=np.array([1e-3, -5e-4])))]
    elements, _ = make_lattice(desc, dtype, lx)
    _, specs = make_lattice(desc, np.float64)  # (0.7, 0.2, 0.1 as float32 are not the float64 numbers:)
    for spec, (_, kw) in zip(specs, desc):
        for name, value in kw.items():
            spec[name][...] = np.asarray(value, dtype=dtype).astype(np.float64)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=4, dtype=dtype, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6], dtype=dtype)
    w = np.zeros((B, P, K, 6))
    w[:, -1, -1] = rng.normal(size=(B, 6))
    w[:, 0, 0] += rng.normal(size=(B, 6))
    g = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=dtype), trajectories=K)(trajectories_bar=w)

    chosen, energy64 = particles[:, :K].astype(np.float64), energy.astype(np.float64)
    references = _parameter_references(desc, specs, lambda: _loss(specs, chosen, energy64, w))
    references = {(desc[e][0], e, name): (g[elements[e]][name], ref) for (e, name), ref in references.items()}
    references["energy"] = (g.energy, _energy_reference(lambda en: _loss(specs, chosen, en, w), energy64))
    got = np.asarray(g.chosen_particles, dtype=np.float64)
    assert got.shape == (B, K, 7)
    edge = sorted({0, K - 1})
    # (the chain of the particles that carry a cotangent, with their cotangents)
    ref_rows = _particle_reference(lambda p: _loss(specs, p, energy64, w[:, :, edge]), chosen[:, edge])[..., :6]
    references["chosen_particles"] = (got[:, edge, :6], ref_rows)
    assert np.all(np.delete(got, edge, axis=1) == 0)
    for what, (value, ref) in references.items():
        if dtype == np.float64:
            _close(value, ref, what)
        else:
            name = what if isinstance(what, str) else what[2]
            measured = _distance(value, ref)
            print(f"tile edges, float32, K = {K}: {what} {measured:.1e}")
            limit = TOL_TRAJECTORY_GRAD.get(name) or max(TOL_TRAJECTORY_GRAD.values())
            assert measured <= limit, (what, measured, limit)


def test_the_two_paths_agree_fp64(lx):
    """
    Every particle chosen and trajectories_bar[..., k, j, :] = mu_bar[..., k, :] / N is the cotangent of the mean: the
    trajectory sweep against the moment sweep of the same object.  They differ by the order of float64 sums.
    """
    rng = np.random.default_rng(29)
    B, N = 2, 130
    desc = _particle_lattice(B, rng)
    elements, _ = make_lattice(desc, np.float64, lx)
    P = len(desc) + 1
    particles = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                     mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
    energy = np.array([6e6, 8e6])
    mu_bar = rng.normal(size=(B, P, 6))
    w = np.broadcast_to(mu_bar[:, :, None, :] / N, (B, P, N, 6))
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy, dtype=np.float64), trajectories=N)
    by_moments, by_particles, both = vjp(mu_bar=mu_bar), vjp(trajectories_bar=w), vjp(mu_bar=mu_bar, trajectories_bar=w)
    again = vjp(mu_bar=mu_bar, trajectories_bar=w)

    def every(g):
        rows = [np.asarray(g.energy, dtype=np.float64).ravel()]
        for element, (kind, _) in zip(elements, desc):
            rows += [np.asarray(g[element][name], dtype=np.float64).ravel() for name in PARAMS_TO_CHECK[kind]]
        return np.concatenate(rows)

    a, b, c = every(by_moments), every(by_particles), every(both)
    assert np.all(a != 0) or np.count_nonzero(a) > 40
    assert np.allclose(b, a, rtol=0.0, atol=1e-9 * np.max(np.abs(a)))
    assert np.allclose(c, a + b, rtol=0.0, atol=1e-12 * np.max(np.abs(a + b)))
    # dL/d(particle) = dL/d(mean) / N for every particle
    assert np.allclose(by_particles.chosen_particles, by_moments.mu[:, None, :] / N, rtol=0.0, atol=1e-9 * np.max(np.abs(by_moments.mu)) / N)
    assert np.array_equal(every(again), c) and np.array_equal(again.chosen_particles, both.chosen_particles)
    assert np.array_equal(again.mu, both.mu) and np.array_equal(again.cov, both.cov)


def test_float32_on_128_elements(lx):
    """
    `o.fodo_segment(32)`, B = 2 with a k1 scale, 8 of 64 particles, w = 1 on x and y at every point: the float32 lattice's
    gradients against central differences of the oracle's float64 chain (on the float32 lattice's own numbers).
    """
    B, N, selection = 2, 64, [3, 60, 17, 0, 41, 63, 8, 29]
    scale = np.array([0.7, 1.05], dtype=np.float32)
    specs32 = o.fodo_segment(32, dtype=np.float32, batch_shape=(B,), k1_scale=scale)
    elements = [lx.Quadrupole(s["length"], k1=s["k1"]) if s["kind"] == "quadrupole" else lx.Drift(s["length"]) for s in specs32]
    specs = [o.Quadrupole(s["length"].astype(np.float64), k1=s["k1"].astype(np.float64)) if s["kind"] == "quadrupole"
             else o.Drift(s["length"].astype(np.float64)) for s in specs32]  # (own arrays: the differences write into them)
    P, K = len(specs) + 1, len(selection)
    particles = o.gaussian_particles((B,), N, seed=4, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    energy = np.full(B, 1e8, dtype=np.float32)
    w = np.zeros((B, P, K, 6))
    w[..., 0] = w[..., 2] = 1.0
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParticleBeam(particles, energy), trajectories=selection)
    assert vjp.trace.num_points == 129 and vjp.trace.trajectories.dtype == np.float32
    g = vjp(trajectories_bar=w)

    # the loss is linear in the state at every point: the chain behind element e, started from the state that enters it
    chosen, energy64 = particles[:, selection].astype(np.float64), energy.astype(np.float64)
    states = _chain(specs, o.particle_beam(chosen, energy64, np.float64))

    def loss_from(e):
        total = np.zeros(B)
        beam = states[e]
        for point in range(e + 1, P):
            beam = o.element_track(specs[point - 1], beam, np.float64)
            total += np.sum(w[:, point] * beam["particles"][..., :6], axis=(-1, -2))
        return total

    got, ref = {"k1": [], "length": []}, {"k1": [], "length": []}
    for e, spec in enumerate(specs):
        for name in ("length", "k1") if spec["kind"] == "quadrupole" else ("length",):
            arr = spec[name]  # (the samples are independent: all of them are stepped at once)
            x0 = arr.copy()
            h = 1e-6 * np.maximum(np.abs(x0), 1e-2)
            arr[:] = x0 + h
            up = loss_from(e)
            arr[:] = x0 - h
            down = loss_from(e)
            arr[:] = x0
            ref[name].append((up - down) / (2 * h))
            got[name].append(np.asarray(g[elements[e]][name], dtype=np.float64))
    got["energy"] = [np.asarray(g.energy, dtype=np.float64)]
    ref["energy"] = [_energy_reference(lambda en: _loss(specs, chosen, en, w), energy64)]
    measured = {name: _distance(np.stack(got[name]), np.stack(ref[name])) for name in ref}
    print("float32 trajectory gradients against float64 differences, 128 elements: " + ", ".join(f"{k} {v:.1e}" for k, v in measured.items()))
    for name, value in measured.items():
        assert np.all(np.isfinite(np.stack(got[name]))), name
        assert value <= TOL_TRAJECTORY_GRAD[name], (name, value)


def test_the_entry_point_refuses_bad_arguments_and_leaves_no_trace(lx):
    """Each refusal is LYNX_ERR_INVALID with the entry point's prefix, before anything is launched; a valid call afterwards returns the same bits."""
    from lynx_amd import engine

    rt = lx.device.get_runtime()
    rng = np.random.default_rng(1)
    f = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(0.5), dtype=np.float64), lx.Quadrupole(f(0.2), k1=f(2.0), dtype=np.float64),
                          lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=np.float64)])
    beam = lx.ParticleBeam(o.gaussian_particles((1,), 50, seed=2, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]),
                           f(1e8), dtype=np.float64)
    K, P = 4, 4
    vjp = lx.grad.track_along_vjp(segment, beam, trajectories=K)
    w, mu_bar = rng.normal(size=(1, P, K, 6)), rng.normal(size=(1, P, 6))
    before = vjp(trajectories_bar=w, mu_bar=mu_bar)
    bits = (before[segment.elements[1]]["k1"], before.energy, before.chosen_particles, before.mu)

    lat = engine._ready(segment.__dict__["_trace_cache"], vjp.program, beam.batch_shape, np.float64, beam._energy._host)
    held = {"e_in": beam._energy.broadcast_device(rt, beam.batch_shape), "records": vjp.trace._device["records"],
            "rec_bar": rt.to_device(np.zeros((1, P, 36))), "g_par": rt.empty((1, 3, 8), np.float64), "g_en": rt.empty((1,), np.float64),
            "g_mu": rt.empty((1, 7), np.float64), "g_cov": rt.empty((1, 7, 7), np.float64), "paths": vjp.trace._device["trajectories"],
            "w": rt.to_device(np.zeros((1, P, K, 7))), "g_chosen": rt.empty((1, K, 7), np.float64)}
    order = ("e_in", "records", "rec_bar", None, "g_par", "g_en", "g_mu", "g_cov", "n_chosen", "paths", "w", "g_chosen")

    def call(handle=lat.handle, **changed):
        values = {name: C.c_void_p(array.ptr) for name, array in held.items()}
        values.update({"n_chosen": K, **changed})
        return rt.lib.lynx_track_particles_along_backward_trajectories(
            rt.ctx, handle, beam.num_particles, *[None if name is None else values[name] for name in order])

    def refused(**changed):
        assert call(**changed) == -1, changed  # LYNX_ERR_INVALID
        message = rt.lib.lynx_last_error(rt.ctx).decode()
        assert message.startswith("beam trace gradients with trajectories: "), message

    assert call() == 0, rt.lib.lynx_last_error(rt.ctx)  # (the arguments the refusals start from are valid)
    for name in ("e_in", "g_par", "g_en", "paths", "w", "g_chosen"):
        refused(**{name: None})
    refused(handle=None)
    refused(n_chosen=0)
    refused(n_chosen=-3)
    for name in ("records", "rec_bar", "g_mu", "g_cov"):  # the moment arguments: all four or none
        refused(**{name: None})
    refused(records=None, g_cov=None)
    assert call(records=None, rec_bar=None, g_mu=None, g_cov=None) == 0, rt.lib.lynx_last_error(rt.ctx)
    # more than 256 elements
    long_line = lx.Segment([lx.Drift(f(0.01), dtype=np.float64) for _ in range(257)])
    leaves = list(long_line._leaves())
    engine.track_along(long_line, leaves, beam, keep_device=True, trajectories=np.arange(K))
    long_lat = engine._ready(long_line.__dict__["_trace_cache"], engine._trace_plan(long_line, leaves), beam.batch_shape, np.float64,
                             beam._energy._host)
    refused(handle=long_lat.handle)
    rt.sync()

    after = vjp(trajectories_bar=w, mu_bar=mu_bar)
    for x, y in zip(bits, (after[segment.elements[1]]["k1"], after.energy, after.chosen_particles, after.mu)):
        assert np.array_equal(x, y)


def test_steer_halo_through_collimator_example(lx):
    """examples/steer_halo_through_collimator.py: particles are lost before, none after, and the clearance loss ends at 0."""
    spec = importlib.util.spec_from_file_location(
        "steer_halo_through_collimator", pathlib.Path(__file__).resolve().parents[1] / "examples" / "steer_halo_through_collimator.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.beamline(), example.incoming_beam()
    before = example.transmission(segment, beam)
    history = example.tune(segment, beam)
    assert before < 1.0 and history[0] > 0.0
    assert history[-1] == 0.0, history[-5:]
    assert example.transmission(segment, beam) == 1.0
    assert segment.COLLIMATOR.is_active
