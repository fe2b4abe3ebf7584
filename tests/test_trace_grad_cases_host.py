"""
The references and the draws of tests/trace_grad_cases.py, without a GPU: the along forms of `AffineReference` against its
end-of-lattice forms, against central differences of the oracle's element-by-element chain (forward mode: every direction of
every case; reverse mode: two drawn parameters and the energy per case, under the two-step condition), the closure of the
moments under affine maps that the kernels rely on, and what the draws of the committed seed cover.
"""

import time

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import reverse_reference as rr
from . import trace_grad_cases as tc
from . import trace_jvp_reference as jr
from .helpers import build
from .test_trace_jvp_host import TOL_FD

_clock = {"start": None}


@pytest.fixture(scope="module", autouse=True)
def _timed():
    _clock["start"], _clock["drew"] = time.perf_counter(), tc.SEED not in tc.DRAW_SECONDS
    yield
    print(f"test_trace_grad_cases_host: {time.perf_counter() - _clock['start']:.1f} s with the draws")


@pytest.fixture(autouse=True)
def _record_seed(record_property):
    print(f"trace_grad_cases: LYNX_TRACE_FUZZ_SEED={tc.SEED}")
    record_property("trace_fuzz_seed", tc.SEED)


def _relative(got, ref):
    return float(np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) + 1e-300))


def test_the_along_forms_with_cotangents_at_the_last_point_are_the_end_of_lattice_forms():
    """1e-12 relative, key by key, on rr.affine_lattice(2): both beam classes, with both BPMs' reading weights."""
    B = 2
    desc, energy = rr.affine_lattice(B), rr.energies(B)
    reference = rr.AffineReference(desc, energy)
    P = len(desc) + 1
    particles = rr.particles(B, 300, seed=4)
    readings = rr.reading_weights(B)
    w_mu, w_cov = rr.cotangents(B, 31)
    along_mu, along_cov = np.zeros((B, P, 6)), np.zeros((B, P, 6, 6))
    along_mu[:, -1], along_cov[:, -1] = w_mu, w_cov
    old = reference.particle_gradients(particles, w_mu, w_cov, readings)
    new = reference.particle_gradients_along(particles, along_mu, along_cov, readings=readings)
    assert set(old) <= set(new) and len(old) > 40
    for key, ref in old.items():
        assert _relative(new[key], ref) <= 1e-12, (key, _relative(new[key], ref))
    assert _relative(new["mu"], old["particles"].sum(axis=1)) <= 1e-12  # every particle moved alike moves the mean
    mu, cov = rr.moments_of(particles)
    w_mu, w_cov = rr.cotangents(B, 32, size=7)
    along_mu, along_cov = np.zeros((B, P, 7)), np.zeros((B, P, 7, 7))
    along_mu[:, -1], along_cov[:, -1] = w_mu, w_cov
    old = reference.parameter_gradients(mu, cov, w_mu, w_cov, readings)
    new = reference.parameter_gradients_along(mu, cov, along_mu, along_cov, readings=readings)
    assert set(old) == set(new)
    for key, ref in old.items():
        assert _relative(new[key], ref) <= 1e-12, (key, _relative(new[key], ref))
    # the energy's cotangents: an affine lattice has the incoming energy at every point
    w_e = np.random.default_rng(3).normal(size=(B, P))
    with_e = reference.parameter_gradients_along(mu, cov, along_mu, along_cov, w_e, readings)
    assert np.allclose(with_e["energy"] - new["energy"], w_e.sum(axis=-1), rtol=1e-12, atol=0.0)


def _quotient_leaves_the_branch(case, label):
    """
    Whether a difference quotient along `label` leaves the branch of the map that the analytic derivative -- and the
    product, which selects the branch by a whole-batch flag as the modelled project does -- holds fixed: the length of a thin
    dipole, and a quadrupole's or solenoid's tilt or misalignment that is zero in EVERY sample (`if all(misalignment == 0):
    return R`: the parameter does not enter the map, its derivative is 0 by construction, and the quotient switches it on).
    """
    if label == "energy" or isinstance(label[0], tuple):
        return False
    kind, kw = case["desc"][label[0]]
    if kind in ("quadrupole", "solenoid") and label[1] in ("tilt", "misalignment"):
        return not np.any(kw[label[1]])
    return kind == "dipole" and label[1] == "length" and not np.any(kw["length"])


@pytest.mark.parametrize("i", range(tc.N_AFFINE))
def test_the_tangents_of_a_case_match_central_differences_of_the_oracle_chain(i):
    """
    `particle_tangents` on the case's particles and `parameter_tangents` on their moments, along every direction of the case,
    against `chain_tangents` (central differences of the oracle's chain, h = 1e-6) at TOL_FD with the quotient's own
    rounding taken off -- `ROUNDING` is the allowance for 12 elements and scales with the length of the lattice --, and
    against each other: the moment recursion reproduces what the particles do (1e-9 of a direction's largest entry).

    A thin dipole's `length` is left out: the analytic derivative holds the thin map fixed (the THICK flag is a whole-batch
    predicate of the lattice, not a function of the length), the quotient steps from length 0 to length h and crosses to
    the thick map -- measured on rr.affine_lattice(2), the two are 3e14 apart.  (The other raw outlier there, the thin
    dipole's tilt, has tangent zero and a quotient that is noise: the rounding taken off covers it.)
    """
    case = tc.affine_cases()[i]
    reference = case["exact"]["reference"]
    _, specs = build(case["desc"], np.float64)
    particles, energy = case["particles"], case["energy"]
    mu = particles.mean(axis=1)  # (the particles' own moments, not rounded to float32: the closure is exact)
    d = particles - mu[:, None, :]
    cov = np.einsum("bni,bnj->bij", d, d) / particles.shape[1]
    allowance = max(1.0, len(specs) / 12)
    make_particles = lambda e: o.particle_beam(particles, e, np.float64)  # noqa: E731
    make_moments = lambda e: o.parameter_beam(mu, cov, e, np.float64)  # noqa: E731
    worst, checked = 0.0, 0
    labelled = tc.directions_of(case, reference)
    smooth = [(label, direction) for label, direction in labelled[:-1] if not _quotient_leaves_the_branch(case, label)]
    if len({label[0] for label, _ in smooth}) >= 2:  # one direction with two items on different elements, weights 1 and 1/2
        (first, a), (last, b) = smooth[0], next(item for item in reversed(smooth) if item[0][0] != smooth[0][0][0])
        labelled.append(((first, last), a + [(leaf, name, component, 0.5 * weight) for leaf, name, component, weight in b]))
    for label, direction in labelled:
        by_particles = reference.particle_tangents(particles, direction)
        by_moments = reference.parameter_tangents(mu, cov, direction)
        for a, b in zip(by_particles, by_moments):
            top = np.max(np.abs(a).reshape(len(a), -1), axis=1).reshape(-1, *([1] * (a.ndim - 1)))
            assert np.all(np.abs(a - b) <= 1e-9 * top + 1e-300), (case["id"], label, "closure")
        assert not by_particles[0][..., 6].any() and not by_particles[1][..., 6, :].any() and not by_particles[1][..., :, 6].any()
        if _quotient_leaves_the_branch(case, label):
            continue
        for got, make_beam, moments in ((by_particles, make_particles, jr.particle_moments), (by_moments, make_moments, jr.parameter_moments)):
            fd_mu, fd_cov, noise_mu, noise_cov = jr.chain_tangents(specs, make_beam, moments, energy, direction)
            dist = (jr.distance(got[0], fd_mu, allowance * noise_mu), jr.distance(got[1], fd_cov, allowance * noise_cov))
            assert max(dist) <= TOL_FD, (case["id"], label, dist)
            worst = max(worst, *dist)
        checked += 1
    print(f"{case['id']}: {checked} directions, worst distance {worst:.1e} of the value (bound {TOL_FD:.0e})")
    assert checked >= 1  # (the energy at least)


@pytest.mark.parametrize("i", range(tc.N_AFFINE))
def test_two_gradients_and_the_energy_of_a_case_match_central_differences_of_the_along_loss(i):
    """
    `parameter_gradients_along` / `particle_gradients_along` (with the case's survivor sets, trajectory cotangents and
    readings) against central differences of `along_loss` under the two-step condition, at the float64 bounds of the
    project's finite-difference tests: 2e-4 max(|ref|, 1e-9 max |w_cov|) + 1e-7 max |got|; the energy 2e-4 |ref| + 1e-12.
    """
    case = tc.affine_cases()[i]
    rng = np.random.default_rng([tc.SEED, 5000 + i])
    _, specs = build(case["desc"], np.float64)
    gradients, shape = case["exact"]["gradients"], case["shape"]
    floor = 1e-9 * float(np.max(np.abs(case["w_cov"])))
    loss = lambda: tc.along_loss(case, specs, case["energy"])  # noqa: E731
    keys = [k for k in gradients if isinstance(k, tuple) and not _quotient_leaves_the_branch(case, (*k, None))]
    worst = 0.0
    for q in rng.permutation(len(keys))[:2]:
        e, name = keys[q]
        array = specs[e][name]
        for component in ((0, 1) if array.ndim == 2 else (None,)):
            index = () if component is None else (component,)
            values = array[(slice(None), *index)]
            fd = tc.two_step_difference(loss, array, index, np.maximum(np.abs(values), rr.FLOOR[name]), floor)
            fd = fd.sum(axis=0, keepdims=True) if e in case["shared"] else fd.reshape(shape)
            got = gradients[(e, name)][(Ellipsis, *index)]
            bound = 2e-4 * np.maximum(np.abs(fd), floor) + 1e-7 * np.max(np.abs(gradients[(e, name)]))
            assert np.all(np.abs(got - fd) <= bound), (case["id"], e, name, component, got, fd)
            worst = max(worst, float(np.max(np.abs(got - fd) / bound)))
    energy = case["energy"].copy()
    fd = tc.two_step_difference(lambda: tc.along_loss(case, specs, energy), energy, (), np.abs(energy), 1e-13).reshape(shape)
    got = gradients["energy"]
    assert np.all(np.abs(got - fd) <= 2e-4 * np.abs(fd) + 1e-12), (case["id"], "energy", got, fd)
    print(f"{case['id']}: worst distance {worst:.2g} of its bound")


def test_what_the_draws_cover_and_their_caps():
    cases = tc.affine_cases()
    assert [c["i"] for c in cases] == list(range(tc.N_AFFINE))
    for c in cases:  # at any seed
        assert 1 <= len(c["desc"]) <= tc.MAX_LEAVES and c["dtype"] == [np.float32, np.float64][c["i"] % 2], c["id"]
        assert tc.derivative_count(tc.reference_desc(c["desc"]), c["energy"]) <= tc.MAX_DERIVATIVES, c["id"]
        assert sum(kind == "bpm" and kw.get("is_active") for kind, kw in c["desc"]) <= 2, c["id"]
        if c["mode"] == "losses":
            kept = (c["lost_at"] == -1).mean(axis=-1)
            assert np.all(kept >= 0.1) and np.all(kept <= 0.9) and c["margin"] >= 1e-6 and c["N"] >= 257, c["id"]
            assert np.any((c["lost_at"] >= 0).any(axis=-1)), c["id"]  # somebody is lost in some sample
        for e in c["shared"]:  # a parameter set given as (1,): the leaf's rows are one row, and it has a row to share
            kind, kw = c["desc"][e]
            assert kind in rr.KIND and all(np.all(v == v[:1]) for v in kw.values() if isinstance(v, np.ndarray)), (c["id"], e)
        if c["twice"] is not None:
            assert c["desc"][c["twice"][0]][1] is c["desc"][c["twice"][1]][1] and (c["twice"][0] in c["shared"]) == (c["twice"][1] in c["shared"]), c["id"]
        if "tangents" in c["exact"]:  # what the k1 floor may take off a comparison stays an artefact's size (tc.floor_error)
            top = max(float(np.max(np.abs(t))) for _, mu_dot, cov_dot in c["exact"]["tangents"] for t in (mu_dot, cov_dot))
            assert all(float(np.max(f)) <= 1e-9 * top for pair in c["exact"]["floor_error"] for f in pair), c["id"]
        lengths = [kw["length"] for kind, kw in c["desc"] if kind == "dipole"]
        assert all(np.all(v == 0) for v in lengths) or all(np.all(v != 0) for v in lengths), c["id"]
    table = {mode: sum(c["mode"] == mode for c in cases) for mode in tc.MODES}
    redrawn = [c["id"] for c in cases if c["failures"]]
    print(f"seed {tc.SEED}: {table}; kinds {sorted({kind for c in cases for kind, _ in c['desc']})}; "
          f"redrawn for conditioning: {redrawn}; worst conditioning {max(c.get('conditioning', 0.0) for c in cases):.2g} of the "
          f"float32 bound (limit {tc.CONDITION}); derivatives {len(rr._derivative_cache)}")
    if tc.SEED != tc.DEFAULT_SEED:
        return
    assert {kind for c in cases for kind, _ in c["desc"]} == set(tc.KINDS) | {"aperture"}
    assert {(c["mode"], c["dtype"]) for c in cases} == {(m, t) for m in tc.MODES for t in (np.float32, np.float64)}
    assert {c["shape"] for c in cases} == set(tc.SHAPES)
    assert any(kind == "dipole" and not np.any(kw["length"]) for c in cases for kind, kw in c["desc"])  # a thin dipole
    assert any(c["shared"] for c in cases) and any(c["twice"] for c in cases) and any(c["nested"] for c in cases)
    particle_modes = [c for c in cases if c["mode"] != "parameters"]
    assert {1, 65} <= {c["N"] for c in particle_modes}
    assert 65 in {len(c["chosen"]) for c in cases if c["mode"] == "trajectories"}
    assert sum(c["dtype"] == np.float32 and len(c["desc"]) >= 8 for c in cases) >= 12
    # some samples only: a tilt, a misalignment, a corrector's length that is zero in part of the batch; k1 = 0 in one sample
    partly = lambda v: np.any(v == 0) and np.any(v != 0)  # noqa: E731
    for kind, name in (("quadrupole", "tilt"), ("quadrupole", "misalignment"), ("quadrupole", "k1"), ("solenoid", "misalignment"),
                       ("hcor", "length")):
        assert any(k == kind and name in kw and partly(kw[name]) for c in cases for k, kw in c["desc"]), (kind, name)
    # the caps: a cap that fails means narrower ranges, never a wider threshold
    assert len(redrawn) <= tc.N_AFFINE // 4, redrawn
    assert not any(c["stand_in"] for c in cases)


def test_the_cavity_cases_have_references_under_the_two_step_condition():
    """
    Every checked quantity of every cavity case has central differences of the along loss that agree with themselves at h and
    h / 4 -- of the ParameterBeam's chain and of the particles' --, and so have the tangents of the chain's moments; the draws
    hold what they are meant to: one to three gaining cavities, every cavity's voltage and phase and the energy among the eight.
    """
    cases = tc.cavity_cases()
    assert len(cases) == tc.N_CAVITY
    for c in cases:
        cavities = [e for e, (kind, _) in enumerate(c["desc"]) if kind == "cavity"]
        assert 4 <= len(c["desc"]) <= 10 and 1 <= len(cavities) <= 3 and len(c["quantities"]) == tc.CHECKED_PER_CASE, c["id"]
        assert {(e, name) for e in cavities for name in ("voltage", "phase")} | {"energy"} <= set(c["quantities"]), c["id"]
        for beam in ("parameters", "particle_chain"):
            refs = c[beam].derivatives(c["quantities"], c["scales"])
            assert all(np.all(np.isfinite(r)) and r.shape == (c["B"],) for r in refs.values()), c["id"]
            assert all(np.any(refs[(e, name)] != 0) for e in cavities for name in ("voltage", "phase")), c["id"]
        for q in c["quantities"]:
            mu_dot, cov_dot, energy_dot, *_ = c["parameters"].tangents(q)
            assert mu_dot.shape == (c["B"], len(c["desc"]) + 1, 7) and np.all(np.isfinite(cov_dot)), (c["id"], q)
            if q == "energy":
                assert np.allclose(energy_dot, 1.0, rtol=1e-6)
            elif q[1] == "voltage":  # E behind the cavity moves by cos(phase) per volt
                phase = np.deg2rad(c["desc"][q[0]][1]["phase"])
                assert np.allclose(energy_dot[:, q[0] + 1], np.cos(phase), rtol=1e-6) and not energy_dot[:, :q[0] + 1].any(), (c["id"], q)
    if tc.SEED == tc.DEFAULT_SEED:
        assert {len([1 for kind, _ in c["desc"] if kind == "cavity"]) for c in cases} == {1, 2, 3}
        assert any("misalignment" in kw for c in cases for kind, kw in c["desc"] if kind == "quadrupole")


def test_the_whole_file_takes_less_than_three_minutes():
    elapsed, draws = time.perf_counter() - _clock["start"], tc.DRAW_SECONDS[tc.SEED]
    # (in a run of the whole suite the cases were drawn when the GPU file was imported: the draws are counted either way)
    inside = elapsed >= draws and _clock.get("drew")
    total = elapsed if inside else elapsed + draws
    print(f"test_trace_grad_cases_host: {total:.1f} s, of which {draws:.1f} s drawing the cases and their references "
          f"({'inside' if inside else 'before'} this file's tests)")
    assert total < 180.0, total
