"""
The references of tests/test_gpu_grad_sizes.py, checked on the host (tests/reverse_reference.py).

(1) The analytic reverse mode for affine lattices against central differences of the float64 oracle: every parameter of
    every element kind -- tilted and misaligned quadrupoles, a thick and a thin dipole with edges, an RBend, solenoid,
    undulator, correctors -- the energy, the readings of two active BPMs, every particle and every entry of an incoming
    ParameterBeam.  The differences come with their own error: the steps h and h/4 agree to 1e-5 of max(|ref|, scale)
    (TWO_STEP_AGREEMENT), the truncation error of the wider one is 16/15 of their distance, so the analytic value has to
    lie within 2e-5 of max(|ref|, scale) of it (the rest is the differences' rounding).

(2) The two-step condition itself for every differenced quantity of every case of the GPU tests.
"""

import numpy as np
import pytest

from . import reverse_reference as rr

WITHIN = 2e-5


def _all_parameters(desc):
    out = []
    for e, (kind, kw) in enumerate(desc):
        for name in rr.ROW.get(kind, ()):
            if name == "length" and not np.any(kw[name]):
                continue  # a thin dipole: any step away from length 0 makes it a thick one (dipole.py:119), another map
            if name is not None and kw.get(name) is not None:
                out += [(e, name, 0), (e, name, 1)] if name == "misalignment" else [(e, name)]
    return out


def _compare(analytic, differences, scales):
    assert len(differences) > 40
    for q, ref in differences.items():
        if q == "energy" or q[0] in ("mu", "cov"):
            got = analytic[q if q == "energy" else q[0]][(slice(None), *(() if q == "energy" else q[1:]))]
        elif q[0] == "particles":
            got = analytic["particles"][:, q[1], q[2]]
        else:
            got = analytic[q[:2]][(slice(None), *q[2:])]
        assert got.shape == ref.shape
        assert np.all(np.abs(got - ref) <= WITHIN * np.maximum(np.abs(ref), scales[q])), (q, got, ref)


@pytest.mark.parametrize("beam", ["particles", "parameters"])
def test_analytic_reverse_mode_against_oracle_differences(beam):
    B, N = 2, 7
    desc = rr.affine_lattice(B)
    energy = rr.energies(B)
    readings = rr.reading_weights(B)
    P = rr.particles(B, N)
    reference = rr.AffineReference(desc, energy)
    quantities = _all_parameters(desc) + ["energy"]
    assert {desc[q[0]][0] for q in quantities if q != "energy"} == set(rr.KIND)  # every kind
    if beam == "particles":
        w_mu, w_cov = rr.cotangents(B, 1)
        case = rr.OracleCase(desc, energy, w_mu, w_cov, particles=P, readings=readings)
        quantities += [("particles", n, c) for n in range(N) for c in range(6)]
        analytic = reference.particle_gradients(P, w_mu, w_cov, readings)
    else:
        w_mu, w_cov = rr.cotangents(B, 2, size=7)
        mu, cov = rr.moments_of(P)
        case = rr.OracleCase(desc, energy, w_mu, w_cov, mu=mu, cov=cov, readings=readings)
        quantities += [("mu", c) for c in range(6)] + [("cov", r, c) for r in range(6) for c in range(6)]
        analytic = reference.parameter_gradients(mu, cov, w_mu, w_cov, readings)
    scales = rr._scales(quantities, w_cov, N)
    _compare(analytic, case.derivatives(quantities, scales), scales)
    # the readings' weights did go in
    plain = (reference.particle_gradients(P, w_mu, w_cov) if beam == "particles" else reference.parameter_gradients(mu, cov, w_mu, w_cov))
    assert not np.allclose(plain[(0, "length")], analytic[(0, "length")], rtol=1e-3)


def test_analytic_reverse_mode_of_a_long_run_against_oracle_differences():
    """The palette lattice of the 40 KiB cases, 47 elements: a parameter of every palette entry, at its first and its last use."""
    B, E = 2, 47
    desc = rr.long_affine_lattice(B, E)
    energy = rr.energies(B)
    mu, cov = rr.moments_of(rr.particles(B, 50))
    w_mu, w_cov = rr.cotangents(B, 4, size=7)
    first_uses = {id(kw): e for e, (_, kw) in reversed(list(enumerate(desc)))}
    last_uses = {id(kw): e for e, (_, kw) in enumerate(desc)}
    chosen = set(first_uses.values()) | set(last_uses.values())
    quantities = [q for q in _all_parameters(desc) if q[0] in chosen] + ["energy"]
    scales = rr._scales(quantities, w_cov)
    case = rr.OracleCase(desc, energy, w_mu, w_cov, mu=mu, cov=cov)
    _compare(rr.AffineReference(desc, energy).parameter_gradients(mu, cov, w_mu, w_cov), case.derivatives(quantities, scales), scales)


# (2) -- `references` raises where a quantity finds no step at which its two differences agree

@pytest.mark.parametrize("N", rr.PARTICLE_COUNTS)
def test_two_step_condition_of_the_particle_count_cases(N):
    refs = rr.references(rr.class_u_case(N))
    assert all(np.all(np.isfinite(v)) for v in refs.values()) and len(refs) >= 8 + 6


@pytest.mark.parametrize("units,pairs", [(u, False) for u in (*rr.DENSE_UNITS, 58, 59)] +[(u, True) for u in sorted({*rr.DENSE_UNITS, *rr.STRUCTURED_UNITS})])
def test_two_step_condition_of_the_unit_count_cases(units, pairs):
    refs = rr.references(rr.units_case(units, pairs))
    assert all(np.all(np.isfinite(v)) for v in refs.values()) and len(refs) >= 2


@pytest.mark.parametrize("steps", rr.STEP_COUNTS)
def test_two_step_condition_of_the_step_count_cases(steps):
    case, scales = rr.steps_case(steps)
    refs = rr.references((case, scales))
    assert all(np.all(np.isfinite(v)) for v in refs.values()) and len(refs) > 25
    # the issue's probe: phases need a wider step than voltages and lengths
    print({q: case.steps_taken[q] for q in refs})


def test_the_lds_switch_and_the_launch_geometry_formulas():
    assert (rr.lds_switch(8), rr.lds_switch(4)) == (46, 98)  # E = 46 | 47 in float64, 98 | 99 in float32
    assert rr.backward_geometry(7 * 512 - 3, 1024, 256, 2) == (7, 4, 2)  # 256 CUs: four workgroups of 2, 2, 2 and 1 tiles
    assert rr.backward_geometry(17 * 256 - 3, 1, 256, 1) == (17, 17, 1)
    assert sum(kind == "quadrupole" for kind, _ in rr.long_affine_lattice(2, 99)) * 6 > 256  # one kind, more than 256 tasks
