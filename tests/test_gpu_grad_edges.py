"""
Reverse pass at the edges where the map builders' formulas cancel (lynx_amd/csrc/lynx_dual.hpp), end to end on the GPU:
quadrupoles at and near k1 = 0 (tilted, misaligned, broadcast), small-angle bends, an RBend (whose angle gradient goes
through grad.py's chain rule), solenoids at and near k = 0, an undulator and a weak off-crest cavity.  Every
differentiable parameter against central differences of the float64 oracle's loss, for both beam types, both dtypes,
the structured and the dense reverse kernel (LYNX_BWD_UNITS) and merged and step-wise pairs (LYNX_BWD_MERGE).
The CPU side of the same question, entry by entry against a 50-digit reference: tests/test_harness_dual_edges.py.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice

pytestmark = pytest.mark.gpu

B, N = 2, 2000
TOL = {np.float64: (2e-4, 1e-7), np.float32: (3e-3, 1e-5)}  # relative, floor (of the largest gradient of the lattice)


@pytest.fixture(scope="module")
def lx():
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _r(v):
    """float32-representable values, so that both dtypes and the float64 reference see the same lattice."""
    return np.asarray(np.asarray(v, dtype=np.float32), dtype=np.float64)


def _desc():
    f = lambda *v: _r(v)  # noqa: E731
    return [("drift", dict(length=f(0.3, 0.3))),
            ("quadrupole", dict(length=f(0.2, 0.2), k1=f(0.0, 1e-7))),
            ("drift", dict(length=f(0.25, 0.25))),
            ("quadrupole", dict(length=f(0.2, 0.2), k1=f(-1e-7, 1e-5), tilt=f(0.3, -0.2),
                                misalignment=_r([[1e-4, -2e-4], [3e-4, 1e-4]]))),
            ("quadrupole", dict(length=f(1.0, 1.0), k1=f(-1e-5, 1e-3), misalignment=_r([[2e-4, 5e-4], [-1e-4, 2e-4]]))),
            ("quadrupole", dict(length=f(0.1), k1=f(0.0))),  # broadcast over the batch
            ("dipole", dict(length=f(0.5, 0.5), angle=f(1e-4, -1e-3), e1=f(0.02, 0.02), e2=f(-0.01, -0.01),
                            fringe_integral=f(0.4, 0.4), fringe_integral_exit=f(0.3, 0.3), gap=f(0.02, 0.02),
                            tilt=f(0.1, 0.1))),
            ("rbend", dict(length=f(0.4, 0.4), angle=f(1e-3, 2e-4), e1=f(0.01, 0.01), e2=f(0.0, 0.0))),
            ("solenoid", dict(length=f(0.3, 0.3), k=f(0.0, 1e-3))),
            ("solenoid", dict(length=f(0.2, 0.2), k=f(1e-5, 0.0), misalignment=_r([[1e-4, 0.0], [0.0, -1e-4]]))),
            ("undulator", dict(length=f(0.8, 0.8))),
            ("hcor", dict(length=f(0.1, 0.1), angle=f(1e-4, -1e-4))),
            ("cavity", dict(length=f(1.0, 1.0), voltage=f(1e5, 5e4), phase=f(60.0, -45.0), frequency=f(1.3e9, 1.3e9))),
            ("drift", dict(length=f(0.4, 0.4)))]


PARAMS = {"drift": ["length"], "quadrupole": ["length", "k1", "tilt", "misalignment"], "hcor": ["length", "angle"],
          "dipole": ["length", "angle", "e1", "e2", "tilt", "fringe_integral", "fringe_integral_exit", "gap"],
          "rbend": ["length", "angle", "e1", "e2"], "solenoid": ["length", "k", "misalignment"],
          "undulator": ["length"], "cavity": ["length", "voltage", "phase", "frequency"]}
ENERGY = _r([1e8, 1.2e8])
# a divergent beam: sigma_x' ~ sigma_x, so that dM[0][1]/dk1 is not hidden behind M[0][0]
SIGMA = np.array([1e-4, 1e-4, 1e-4, 1e-4, 1e-5, 1e-3])
MU = np.array([2e-4, -1e-4, 1e-4, 2e-4, 1e-5, 1e-3])


def _beam_inputs():
    rng = np.random.default_rng(5)
    P = _r(o.gaussian_particles((B,), N, seed=17, dtype=np.float64, sigma=SIGMA, mu=MU))
    A = rng.normal(size=(B, 6, 6)) * SIGMA[:, None] * 0.5
    cov = np.zeros((B, 7, 7))
    cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2)
    cov = _r(cov)
    mu = _r(np.concatenate([MU + rng.normal(size=(B, 6)) * SIGMA * 0.1, np.ones((B, 1))], axis=-1))
    w_mu = rng.normal(size=(B, 6)) * 1e2
    w_cov = rng.normal(size=(B, 6, 6)) * 1e6
    return P, mu, cov, w_mu, w_cov


def _loss(specs, beam_type, inputs, energy):
    P, mu, cov, w_mu, w_cov = inputs
    if beam_type == "particle":
        out = o.segment_track(specs, o.particle_beam(P, energy, np.float64), np.float64)
        Q = out["particles"][..., :6]
        m = Q.mean(axis=-2)
        d = Q - m[..., None, :]
        c = np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2]
    else:
        out = o.segment_track(specs, o.parameter_beam(mu, cov, energy, np.float64), np.float64)
        m, c = out["mu"][..., :6], out["cov"][..., :6, :6]
    return np.sum(w_mu * m, axis=-1) + np.sum(w_cov * c, axis=(-1, -2))


_REFERENCE = {}


def _reference(beam_type):
    """{(element index, name): central differences of the float64 oracle's loss, shaped like the parameter}, energy."""
    if beam_type in _REFERENCE:
        return _REFERENCE[beam_type]
    desc = _desc()
    _, specs = make_lattice(desc, np.float64)
    inputs = _beam_inputs()
    ref = {}
    for e, (kind, _) in enumerate(desc):
        for name in PARAMS[kind]:
            arr = specs[e][name]
            if arr is None:  # left at its default in this element
                continue
            out = np.zeros(arr.shape)
            for idx in np.ndindex(arr.shape):
                x0 = arr[idx]
                h = 1e-6 * max(abs(x0), 1e-2)
                arr[idx] = x0 + h
                up = _loss(specs, beam_type, inputs, ENERGY)
                arr[idx] = x0 - h
                down = _loss(specs, beam_type, inputs, ENERGY)
                arr[idx] = x0
                d = (up - down) / (2 * h)
                out[idx] = d.sum() if arr.shape[0] == 1 else d[idx[0]]  # a broadcast parameter gathers every sample
            ref[(e, name)] = out
    g_e = np.zeros(B)
    for b in range(B):
        h = 1e-6 * ENERGY[b]
        ep, em = ENERGY.copy(), ENERGY.copy()
        ep[b] += h
        em[b] -= h
        g_e[b] = (_loss(specs, beam_type, inputs, ep)[b] - _loss(specs, beam_type, inputs, em)[b]) / (2 * h)
    _REFERENCE[beam_type] = ref, g_e
    return ref, g_e


@pytest.mark.parametrize("merge", ["1", "0"], ids=["merged", "stepwise"])
@pytest.mark.parametrize("units", ["1", "0"], ids=["structured", "dense"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("beam_type", ["particle", "parameter"])
def test_gradients_at_the_edges_match_finite_differences(lx, monkeypatch, beam_type, dtype, units, merge):
    monkeypatch.setenv("LYNX_BWD_UNITS", units)
    monkeypatch.setenv("LYNX_BWD_MERGE", merge)
    desc = _desc()
    elements, _ = make_lattice(desc, dtype, lx)
    P, mu, cov, w_mu, w_cov = _beam_inputs()
    if beam_type == "particle":
        beam = lx.ParticleBeam(P.astype(dtype), ENERGY.astype(dtype), dtype=dtype)
        g = lx.grad.track_vjp(lx.Segment(elements), beam)(mu_bar=w_mu, cov_bar=w_cov)
    else:
        beam = lx.ParameterBeam(mu.astype(dtype), cov.astype(dtype), ENERGY.astype(dtype), dtype=dtype)
        w_mu7, w_cov7 = np.zeros((B, 7)), np.zeros((B, 7, 7))
        w_mu7[:, :6], w_cov7[:, :6, :6] = w_mu, w_cov
        g = lx.grad.track_vjp(lx.Segment(elements), beam)(mu_bar=w_mu7, cov_bar=w_cov7)
    ref, ref_e = _reference(beam_type)
    rel, floor = TOL[dtype]
    gmax = max(float(np.max(np.abs(r))) for r in ref.values())
    bad = []
    for (e, name), r in ref.items():
        got = np.asarray(g[elements[e]][name], dtype=np.float64)
        assert got.shape == r.shape, (e, name, got.shape, r.shape)
        err = np.abs(got - r)
        if np.any(err > rel * np.abs(r) + floor * gmax):
            bad.append((desc[e][0], e, name, got.tolist(), r.tolist()))
    assert not bad, bad
    # dL/dE per eV, held like the parameters as E dL/dE (the loss's change for a relative change of the energy)
    err_e = np.abs(np.asarray(g.energy) - ref_e) * ENERGY
    assert np.all(err_e <= rel * np.abs(ref_e) * ENERGY + floor * gmax), (g.energy, ref_e)
    # the switched-off quadrupoles' k1 gradients stand well above the floor: a zero would fail
    for e, b in ((1, 0), (5, 0)):
        assert abs(ref[(e, "k1")][b]) > 10 * floor * gmax, (e, ref[(e, "k1")], gmax)


def test_tuning_starts_from_a_switched_off_lattice(lx):
    """
    The ARES EA lattice of examples/gradient_based_tuning.py as it is built, every magnet at 0: the three quadrupoles'
    gradients are the limit k1 -> 0 (not 0) and match finite differences of the float64 oracle at 1e-3, and a few Adam
    steps of its `tune()` move every quadrupole off 0.
    """
    import importlib.util
    import pathlib

    spec = importlib.util.spec_from_file_location(
        "gradient_based_tuning", pathlib.Path(__file__).resolve().parents[1] / "examples" / "gradient_based_tuning.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    f = example.f
    segment = example.ares_ea()
    beam = lx.ParticleBeam.from_parameters(num_particles=20_000, sigma_x=f(1.75e-4), sigma_xp=f(3.7e-6),
                                           sigma_y=f(1.75e-4), sigma_yp=f(3.7e-6), energy=f(1.07e8), seed=0)
    P = np.asarray(beam.particles, dtype=np.float64)
    quads = ("AREAMQZM1", "AREAMQZM2", "AREAMQZM3")
    bars = {"mu_x": 1.0, "sigma_x": 1.0, "mu_y": 1.0, "sigma_y": 1.0}
    g = lx.grad.track_vjp(segment, beam)(**bars)

    def loss(k1s):
        a = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
        specs = [o.Drift(a(0.17504)), o.Quadrupole(a(0.122), k1=a(k1s[0])), o.Drift(a(0.428)),
                 o.Quadrupole(a(0.122), k1=a(k1s[1])), o.Drift(a(0.204)), o.VerticalCorrector(a(0.02), a(0.0)),
                 o.Drift(a(0.204)), o.Quadrupole(a(0.122), k1=a(k1s[2])), o.Drift(a(0.179)),
                 o.HorizontalCorrector(a(0.02), a(0.0)), o.Drift(a(0.45))]
        m = o.beam_moments(o.segment_track(specs, o.particle_beam(P, np.array([1.07e8]), np.float64), np.float64))
        return sum(float(np.asarray(m[k])[0]) for k in bars)

    for q, name in enumerate(quads):
        got = float(g[getattr(segment, name)]["k1"][0])
        h = 1e-3
        k_up, k_down = [0.0] * 3, [0.0] * 3
        k_up[q], k_down[q] = h, -h
        ref = (loss(k_up) - loss(k_down)) / (2 * h)
        assert got != 0.0 and abs(got - ref) <= 1e-3 * abs(ref), (name, got, ref)

    example.tune(segment, beam, steps=3)
    for name in quads:
        assert float(getattr(segment, name).k1[0]) != 0.0, name
