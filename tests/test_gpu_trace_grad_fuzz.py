"""
Seeded random cases of `lynx_amd.grad.track_along_vjp` -- a ParameterBeam's sweep, a ParticleBeam's, with trajectories and with
losses -- and of `track_along_jvp` on the GPU, against references that do not come from the GPU: the along forms of
`reverse_reference.AffineReference` (analytic; tests/test_trace_grad_cases_host.py holds them to central differences of the
oracle's chain on the host).  The lattices of tests/trace_grad_cases.py have what the hand-made lattices of the other
along-family files lack: solenoids, undulators, RBends in reverse mode, thin dipoles, correctors of zero length, tilts and
misalignments in part of the batch, k1 = 0 in one sample, an element object placed twice, a nested Segment, parameters given as
(1,), batch shape (2, 2), and particle counts at a wave's edge.

Cavity cases (a line of drifts, quadrupoles and correctors with one to three gaining cavities) are held to central differences
of the oracle's element-by-element chain under the two-step condition of `reverse_reference.OracleCase`: a ParameterBeam through
`track_along_vjp` and through `track_along_jvp(cavities=True)`, 400 particles through `track_along_vjp(cavities=True)`.

Per affine case: the trace's moments at every point; every gradient of the reverse call, at the bounds of test_gpu_grad_sizes.py
(`Distances`: float64 as the project's finite-difference tests, float32 3e-3 |ref| + 1e-4 max |ref| against the float64
reference); the same bits twice; where forward mode applies, every direction's tangents, the BPMs' reading tangents, and the
adjoint identity between the two calls.  Every test prints its worst distance in units of its bound and where it was.

LYNX_TRACE_FUZZ_SEED=<seed> and `-k a07-` replay one case; a case that fails is a finding, not a draw to replace.
Measured on MI355X: see NOTES.md (the entry of this file).
"""

import time

import numpy as np
import pytest

from . import trace_grad_cases as tc
from . import trace_jvp_reference as jr
from .helpers import covariance_distances, make_lattice
from .test_gpu_grad_sizes import Distances
from .test_gpu_parity import TOL_MOM
from .test_gpu_trace_jvp import ADJOINT_CAP, TOL_RESTATEMENT
from .test_trace_jvp_host import TOL_FD

pytestmark = pytest.mark.gpu

# The analytic reference's own error: its map derivatives hold 30 digits (reverse_reference.DPS) of entries below 1e3, and a
# tangent is linear in them with coefficients (states, maps) below 1e2 -- below 1e-25 in all, where a tangent that is an exact
# zero (a thin dipole's tilt in the covariance) comes out of 30-digit arithmetic as 1e-47.  Taken off |got - ref| as
# `jr.distance` takes a quotient's rounding off.
REFERENCE_ERROR = 1e-24
CASES = tc.affine_cases()
CAVITY_CASES = tc.cavity_cases()


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


@pytest.fixture(autouse=True)
def _record_seed(record_property):
    print(f"test_gpu_trace_grad_fuzz: LYNX_TRACE_FUZZ_SEED={tc.SEED}")
    record_property("trace_fuzz_seed", tc.SEED)


def _beam(lx, case):
    dtype, shape = case["dtype"], case["shape"]
    energy = case["energy"].astype(dtype).reshape(shape)
    if case["mode"] == "parameters":
        return lx.ParameterBeam(case["mu"].reshape(*shape, 7).astype(dtype), case["cov"].reshape(*shape, 7, 7).astype(dtype), energy, dtype=dtype)
    return lx.ParticleBeam(case["particles"].reshape(*shape, case["N"], 7).astype(dtype), energy, dtype=dtype)


def _flat(a, tail):
    """(samples, *the last `tail` axes): a batch of shape (2, 2) is a batch of 4, a parameter given as (1,) stays one row."""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, *a.shape[a.ndim - tail:])


def _check_trace(case, trace, exact):
    """mu and cov at every point against the reference's states, in the measures of `moment_distances` and `covariance_distances`."""
    B, P, tol = case["B"], len(case["desc"]) + 1, TOL_MOM[case["dtype"]]
    mu, cov = np.asarray(trace.mu, dtype=np.float64).reshape(B, P, 6), np.asarray(trace.cov, dtype=np.float64).reshape(B, P, 6, 6)
    sigma = np.sqrt(np.einsum("bpii->bpi", exact["cov"]))
    with np.errstate(all="ignore"):
        d_mu = np.abs(mu - exact["mu"]) / (np.abs(exact["mu"]) + sigma)
    assert np.all(d_mu <= tol), (case["id"], "mu", float(np.max(d_mu)), np.unravel_index(int(np.argmax(d_mu)), d_mu.shape))
    d_cov, where = covariance_distances(cov.reshape(B * P, 6, 6), exact["cov"].reshape(B * P, 6, 6))
    assert d_cov <= tol, (case["id"], "cov", d_cov, where)
    if case["mode"] == "losses":
        assert np.array_equal(np.asarray(trace.lost_at).reshape(B, -1), case["lost_at"]), case["id"]
    return max(float(np.max(d_mu)), d_cov) / tol


def _reverse_call(lx, case, segment, elements):
    shape, P = case["shape"], len(case["desc"]) + 1
    k = case["w_mu"].shape[-1]
    options = {"trajectories": dict(trajectories=case.get("chosen")), "losses": dict(losses=True)}.get(case["mode"], {})
    vjp = lx.grad.track_along_vjp(segment, _beam(lx, case), **options)
    bars = dict(mu_bar=case["w_mu"].reshape(*shape, P, k), cov_bar=case["w_cov"].reshape(*shape, P, k, k),
                energy_bar=case["w_e"].reshape(*shape, P))
    if case["readings"]:
        bpms = [el for el, (kind, kw) in zip(elements, case["desc"]) if kind == "bpm" and kw.get("is_active")]
        bars["readings"] = {bpm: r.reshape(2, *shape) for bpm, r in zip(bpms, case["readings"])}
    if case["mode"] == "trajectories":
        bars["trajectories_bar"] = case["trajectories_bar"].reshape(*shape, P, len(case["chosen"]), 7)
    return vjp, bars


def _gradients(case, elements, g):
    """The call's gradients in the reference's keys, float64."""
    out = {"energy": np.asarray(g.energy, dtype=np.float64)}
    for key in case["exact"]["gradients"]:
        if isinstance(key, tuple):
            out[key] = np.asarray(g[elements[key[0]]][key[1]], dtype=np.float64)
    if case["mode"] == "losses":
        assert g.mu is None and g.cov is None, case["id"]
    else:
        out["mu"], out["cov"] = np.asarray(g.mu, dtype=np.float64), np.asarray(g.cov, dtype=np.float64)
    if case["mode"] == "trajectories":
        out["chosen_particles"] = np.asarray(g.chosen_particles, dtype=np.float64)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_random_affine_case_against_the_analytic_reference(lx, case):
    started = time.perf_counter()
    exact, dtype, shape, B = case["exact"], case["dtype"], case["shape"], case["B"]
    reference = exact["gradients"]
    segment, elements = tc.make_segment(case, lx)
    P = len(case["desc"]) + 1
    name_of = np.dtype(dtype).name

    # ---- reverse mode ------------------------------------------------------------------------------------------------------
    vjp, bars = _reverse_call(lx, case, segment, elements)
    assert vjp.trace.num_points == P
    trace_worst = _check_trace(case, vjp.trace, exact)
    g = vjp(**bars)
    got = _gradients(case, elements, g)
    d = Distances(dtype, case["w_cov"])
    for key, ref in reference.items():
        value = got[key]
        assert value.shape == ref.shape, (case["id"], key, value.shape, ref.shape)
        if key == "energy":
            d.add("energy", _flat(value, 0), _flat(ref, 0))
        elif key == "mu":
            d.add("mu", _flat(value, 1)[:, :6], _flat(ref, 1)[:, :6])
        elif key == "cov":
            value = _flat(value, 2)[:, :6, :6]
            if case["mode"] != "parameters":  # the particles fix the symmetric part of dL/d(biased covariance) alone
                value = (value + np.swapaxes(value, -1, -2)) / 2
            d.add("cov", value, _flat(ref, 2)[:, :6, :6])
        elif key == "chosen_particles":
            d.add("particles", _flat(value, 2), _flat(ref, 2))
        else:
            tail = value.ndim - (1 if key[0] in case["shared"] else len(shape))
            d.add(key, _flat(value, tail), _flat(ref, tail))
    for el, (kind, _) in zip(elements, case["desc"]):
        if kind == "aperture":  # the survivor sets are held fixed: the limits that made them get an exact 0
            zero = g[el]
            assert zero["x_max"].shape == shape and not zero["x_max"].any() and not zero["y_max"].any(), case["id"]
    d.done(f"{case['id']} reverse ({name_of}; trace {trace_worst:.2g} of TOL_MOM)", at_least=2)
    again = _gradients(case, elements, vjp(**bars))
    for key, value in got.items():
        assert np.array_equal(again[key], value, equal_nan=True), (case["id"], key, "a second call gave other bits")

    # ---- forward mode and the adjoint identity ----------------------------------------------------------------------------------
    if "tangents" not in exact:
        print(f"{case['id']}: {time.perf_counter() - started:.2f} s")
        return
    labels = [label for label, _, _ in exact["tangents"]]
    wrt = ["energy" if label == "energy" else (elements[label[0]], label[1]) if label[2] is None else (elements[label[0]], label[1], label[2])
           for label in labels]
    jvp = lx.grad.track_along_jvp(segment, _beam(lx, case), wrt)
    D = len(wrt)
    assert jvp.mu_dot.shape == (*shape, D, P, 7) and jvp.cov_dot.shape == (*shape, D, P, 7, 7)
    mu_dot, cov_dot = jvp.mu_dot.reshape(B, D, P, 7), jvp.cov_dot.reshape(B, D, P, 7, 7)
    assert not mu_dot[..., 6].any() and not cov_dot[..., 6, :].any() and not cov_dot[..., :, 6].any()  # exact zeros
    worst, where = 0.0, None
    for k, (label, ref_mu, ref_cov) in enumerate(exact["tangents"]):
        floor_mu, floor_cov = exact["floor_error"][k]  # (zero but in a sample whose quadrupole has k1 = 0: tc.floor_error)
        for what, value, ref, floor in (("mu_dot", mu_dot[:, k], ref_mu, floor_mu), ("cov_dot", cov_dot[:, k], ref_cov, floor_cov)):
            own = REFERENCE_ERROR + floor
            off = np.maximum(np.abs(value - ref) - own.reshape(-1, *([1] * (ref.ndim - 1))), 0.0)
            if dtype == np.float64:
                ratio = jr.distance(value, ref, own) / TOL_RESTATEMENT
                at = np.unravel_index(int(np.argmax(off)), ref.shape)
            else:
                bound = tc.float32_bound(ref, axis_from=1)
                with np.errstate(all="ignore"):
                    over = np.where(off <= bound, off / np.maximum(bound, 1e-300), np.inf)
                ratio, at = float(np.max(over)), np.unravel_index(int(np.argmax(off / np.maximum(bound, 1e-300))), ref.shape)
            if ratio > worst:
                worst, where = ratio, (label, what, tuple(int(v) for v in at), float(value[at]), float(ref[at]),
                                       float(np.max(np.abs(ref[at[0]]))))  # (where, got, reference, the sample's largest)
    print(f"{case['id']} forward ({name_of}): {D} directions, worst distance {worst:.3g} of its bound at {where}")
    assert worst <= 1.0, (case["id"], where, worst)
    for e, (el, (kind, _)) in enumerate(zip(elements, case["desc"])):
        if kind == "bpm":
            assert np.array_equal(jvp.reading_tangents(el), jvp.mu_dot[..., e, :][..., (0, 2)]), (case["id"], e)

    # <w, J v> = <J^T w, v> between the two calls; the readings and the energy's own cotangents are part of w
    k = case["w_mu"].shape[-1]
    terms_mu = case["w_mu"][:, None] * mu_dot[..., :k]
    terms_cov = case["w_cov"][:, None] * cov_dot[..., :k, :k]
    if case["readings"]:
        active = [e for e, (kind, kw) in enumerate(case["desc"]) if kind == "bpm" and kw.get("is_active")]
        for e, r in zip(active, case["readings"]):
            terms_mu[:, :, e, 0] += r[0][:, None] * mu_dot[:, :, e, 0]
            terms_mu[:, :, e, 2] += r[1][:, None] * mu_dot[:, :, e, 2]
    forward = terms_mu.sum(axis=(-1, -2)) + terms_cov.sum(axis=(-1, -2, -3))
    size = np.abs(terms_mu).sum(axis=(-1, -2)) + np.abs(terms_cov).sum(axis=(-1, -2, -3))
    worst, where = 0.0, None
    for k, label in enumerate(labels):
        if label == "energy":  # the energy at every point IS the incoming one: its tangent is 1 there
            fwd, sz, reverse = forward[:, k] + case["w_e"].sum(axis=-1), size[:, k] + np.abs(case["w_e"]).sum(axis=-1), _flat(got["energy"], 0)
        else:
            reverse = got[(label[0], label[1])]
            reverse = _flat(reverse if label[2] is None else reverse[..., label[2]], 0)
            fwd, sz = forward[:, k], size[:, k]
            if label[0] in case["shared"]:  # one value for the batch: the samples' tangents add up to its gradient
                fwd, sz = fwd.sum(keepdims=True), sz.sum(keepdims=True)
        assert reverse.shape == fwd.shape, (case["id"], label)
        if not sz.any():
            assert not reverse.any() and not fwd.any(), (case["id"], label)
            continue
        with np.errstate(all="ignore"):
            dist = float(np.max(np.where(sz > 0, np.abs(fwd - reverse) / sz, np.where(reverse == 0, 0.0, np.inf))))
        if dist > worst:
            worst, where = dist, label
    print(f"{case['id']} adjoint identity ({case['mode']}, {name_of}): worst |<w, J v> - <J^T w, v>| / sum |terms| = {worst:.2e} at {where}")
    assert worst <= ADJOINT_CAP[name_of], (case["id"], where, worst)
    print(f"{case['id']}: {time.perf_counter() - started:.2f} s")


def _cavity_gradients(case, elements, g):
    out = {"energy": np.asarray(g.energy, dtype=np.float64)}
    for q in case["quantities"]:
        if q != "energy":
            out[q[:2]] = np.asarray(g[elements[q[0]]][q[1]], dtype=np.float64)
    return out


@pytest.mark.parametrize("case", CAVITY_CASES, ids=[c["id"] for c in CAVITY_CASES])
def test_random_cavity_case_against_differences_of_the_oracle_chain(lx, case):
    """
    Eight quantities per case -- every cavity's voltage and phase, the energy, parameters of the magnets -- with cotangents of
    mu, cov and the energy at every point: (a) a ParameterBeam through `track_along_vjp`, (c) 400 particles through
    `track_along_vjp(cavities=True)`, both with `Distances.add_differences` (the float32 bound against the float64
    differences); (b) the ParameterBeam through `track_along_jvp(cavities=True)`: mu_dot, cov_dot and energy_dot at every point
    at TOL_FD, the quotient's own rounding taken off.
    """
    started = time.perf_counter()
    dtype, B, desc = case["dtype"], case["B"], case["desc"]
    elements, _ = make_lattice(desc, dtype, lx)
    segment = lx.Segment(elements)
    energy = case["energy"].astype(dtype)
    parameters = lx.ParameterBeam(case["mu"].astype(dtype), case["cov"].astype(dtype), energy, dtype=dtype)
    particles = lx.ParticleBeam(case["particles"].astype(dtype), energy, dtype=dtype)
    w_mu, w_cov, w_e = case["w_mu"], case["w_cov"], case["w_e"]
    name_of = np.dtype(dtype).name
    # a
    g = lx.grad.track_along_vjp(segment, parameters)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    d = Distances(dtype, w_cov)
    d.add_differences(_cavity_gradients(case, elements, g), case["parameters"].derivatives(case["quantities"], case["scales"]))
    d.done(f"{case['id']} a: ParameterBeam, track_along_vjp ({name_of})", at_least=B * tc.CHECKED_PER_CASE)
    # c
    g = lx.grad.track_along_vjp(segment, particles, cavities=True)(mu_bar=w_mu[..., :6], cov_bar=w_cov[..., :6, :6], energy_bar=w_e)
    assert g.mu is None and g.cov is None
    d = Distances(dtype, w_cov)
    d.add_differences(_cavity_gradients(case, elements, g), case["particle_chain"].derivatives(case["quantities"], case["scales"]))
    d.done(f"{case['id']} c: ParticleBeam, track_along_vjp(cavities=True) ({name_of})", at_least=B * tc.CHECKED_PER_CASE)
    # b
    wrt = ["energy" if q == "energy" else (elements[q[0]], *q[1:]) for q in case["quantities"]]
    jvp = lx.grad.track_along_jvp(segment, parameters, wrt, cavities=True)
    P, D = len(desc) + 1, len(wrt)
    assert jvp.mu_dot.shape == (B, D, P, 7) and jvp.cov_dot.shape == (B, D, P, 7, 7) and jvp.energy_dot.shape == (B, D, P)
    assert not jvp.mu_dot[..., 6].any() and not jvp.cov_dot[..., 6, :].any() and not jvp.cov_dot[..., :, 6].any()
    allowance = max(1.0, len(desc) / 12)
    worst, where = 0.0, None
    for k, q in enumerate(case["quantities"]):
        fd_mu, fd_cov, fd_energy, noise_mu, noise_cov, noise_energy = case["parameters"].tangents(q, allowance)
        for what, value, ref, noise in (("mu_dot", jvp.mu_dot[:, k], fd_mu, noise_mu), ("cov_dot", jvp.cov_dot[:, k], fd_cov, noise_cov),
                                        ("energy_dot", jvp.energy_dot[:, k], fd_energy, noise_energy)):
            dist = jr.distance(value, ref, noise)
            if dist > worst:
                worst, where = dist, (q, what)
    print(f"{case['id']} b: track_along_jvp(cavities=True) ({name_of}): {D} directions, worst distance {worst / TOL_FD:.3g} of its bound at {where}")
    assert worst <= TOL_FD, (case["id"], where, worst)
    print(f"{case['id']}: {time.perf_counter() - started:.2f} s")
