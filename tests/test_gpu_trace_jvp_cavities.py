"""
`lynx_amd.grad.track_along_jvp(..., cavities=True)` and `orbit_response_matrix(..., cavities=True)` on the GPU
(lynx_track_moments_along_forward_cavities): the tangents of a ParameterBeam's moments and of the beam energy at EVERY point of
a lattice with accelerating cavities against central differences of the oracle's element-by-element chain in float64; the
adjoint identity against `track_along_vjp`; a linac's response matrix against its closed form; the shapes at which the kernels
can go wrong, against the NumPy restatement of tests/trace_jvp_cavities_reference.py; bit equality with the plain call on a
lattice without cavities; float32 against the float64 pass; what the entry point refuses and where it writes.
"""

import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import entry_calls as ec
from . import entry_footprint as fp
from . import trace_jvp_cavities_reference as cref
from . import trace_jvp_reference as ref
from .helpers import make_lattice
from .test_gpu_grad import _desc
from .test_gpu_trace_jvp import ADJOINT_CAP, TOL_RESTATEMENT, _beam, _wrt, fd_case
from .test_trace_jvp_host import TOL_FD, directions_to_check, incoming_moments

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


_case, _envs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _library(built_library):
    yield
    _envs.clear()
    _case.clear()


def cavity_case(lx, dtype=np.float64):
    """The nine-element lattice of test_gpu_grad._desc WITH its two cavities, B = 2, 6 and 8 MeV, every direction to check."""
    if dtype not in _case:
        rng = np.random.default_rng(23)
        B = 2
        desc = _desc(B, rng)
        elements, _ = make_lattice(desc, dtype, lx)
        _, specs64 = make_lattice(desc, np.float64)
        mu, cov = incoming_moments(B, rng)
        labelled = directions_to_check(desc, specs64)
        _case[dtype] = dict(desc=desc, elements=elements, specs=specs64, mu=mu, cov=cov, energy=np.array([6e6, 8e6]),
                            labelled=labelled, wrt=_wrt(elements, labelled))
    return _case[dtype]


def test_tangents_at_every_point_match_finite_differences_of_the_oracle_chain_through_cavities_fp64(lx):
    """
    mu_dot, cov_dot and energy_dot at all ten points, for every parameter of PARAMS_TO_CHECK of every element -- both
    cavities' length, voltage, phase and frequency among them -- and for "energy", against central differences of the oracle's
    chain of ParameterBeams at 2e-4 of the value (`ref.distance`, the quotient's own rounding taken off).  The same call twice
    gives the same bits; the 7th row and column are exact zeros.
    """
    case = cavity_case(lx)
    segment = lx.Segment(case["elements"])
    beam = _beam(lx, case, "parameters", np.float64)
    jvp = lx.grad.track_along_jvp(segment, beam, case["wrt"], cavities=True)
    B, D, P = 2, len(case["wrt"]), 10
    assert D == 29 and jvp.mu_dot.shape == (B, D, P, 7) and jvp.cov_dot.shape == (B, D, P, 7, 7) and jvp.energy_dot.shape == (B, D, P)
    assert jvp.mu_dot.dtype == jvp.cov_dot.dtype == jvp.energy_dot.dtype == np.float64
    make_beam = lambda e: o.parameter_beam(case["mu"], case["cov"], e, np.float64)  # noqa: E731
    worst, moved_energy = 0.0, 0
    for d, (label, direction) in enumerate(case["labelled"]):
        fd_mu, fd_cov, noise_mu, noise_cov = ref.chain_tangents(case["specs"], make_beam, ref.parameter_moments, case["energy"], direction)
        fd_e, _, noise_e, _ = ref.chain_tangents(case["specs"], make_beam, cref.energy_moments, case["energy"], direction)
        dist = [ref.distance(jvp.mu_dot[:, d], fd_mu, noise_mu), ref.distance(jvp.cov_dot[:, d], fd_cov, noise_cov)]
        if np.any(fd_e != 0):
            dist.append(ref.distance(jvp.energy_dot[:, d, :, None], fd_e, noise_e))
            moved_energy += 1
        else:
            assert not jvp.energy_dot[:, d].any(), label
        worst = max(worst, ref.distance(jvp.mu_dot[:, d], fd_mu), ref.distance(jvp.cov_dot[:, d], fd_cov))
        print(f"  {label}: " + ", ".join(f"{v:.1e}" for v in dist))
        assert max(dist) <= TOL_FD, (label, dist)
    print(f"track_along_jvp(cavities=True) against central differences of the oracle chain: {D} directions, worst distance "
          f"{worst:.1e} with the quotients' own rounding left in")
    assert moved_energy == 5  # two voltages, two phases, the incoming energy
    for tangents in (jvp.mu_dot[..., 6], jvp.cov_dot[..., 6, :], jvp.cov_dot[..., :, 6], jvp.mu_dot[:, :, 0], jvp.cov_dot[:, :, 0]):
        assert not tangents.any()  # exact zeros
    again = lx.grad.track_along_jvp(segment, beam, case["wrt"], cavities=True)
    assert again.mu_dot.tobytes() == jvp.mu_dot.tobytes() and again.cov_dot.tobytes() == jvp.cov_dot.tobytes()
    assert again.energy_dot.tobytes() == jvp.energy_dot.tobytes()
    assert np.array_equal(jvp.tangent("energy"), jvp.energy_dot)


# The worst distance |<w, J v> - <J^T w, v>| / sum |terms| measured on MI355X over every direction of the case above, the
# cotangents w_mu, w_cov and w_e (`energy_bar`) at all points (beside the table of tests/test_gpu_trace_jvp.py):
#                      parameters, through cavities
#     float64 lattice    1.97e-16
#     float32 lattice    6.59e-08
# asserted at ten times that, and never looser than ADJOINT_CAP of that file.
ADJOINT_MEASURED = {"float64": 1.97e-16, "float32": 6.59e-08}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_the_adjoint_identity_against_track_along_vjp_through_cavities(lx, dtype):
    """
    Random w_mu, w_cov, w_e at all points: sum_k <w_mu, mu_dot> + <w_cov, cov_dot> + w_e e_dot per sample and direction is the
    gradient `track_along_vjp(...)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)` has at that parameter; the reverse side is held
    to finite differences by test_gpu_trace_grad.py.
    """
    case = cavity_case(lx, dtype)
    elements, name_of = case["elements"], np.dtype(dtype).name
    segment = lx.Segment(elements)
    beam = _beam(lx, case, "parameters", dtype)
    rng = np.random.default_rng(77)
    B, P = 2, 10
    w_mu, w_cov, w_e = rng.normal(size=(B, P, 6)), rng.normal(size=(B, P, 6, 6)) * 1e3, rng.normal(size=(B, P)) * 1e-9
    jvp = lx.grad.track_along_jvp(segment, beam, case["wrt"], cavities=True)
    g = lx.grad.track_along_vjp(segment, beam)(mu_bar=w_mu, cov_bar=w_cov, energy_bar=w_e)
    terms_mu = w_mu[:, None] * jvp.mu_dot[..., :6]
    terms_cov = w_cov[:, None] * jvp.cov_dot[..., :6, :6]
    terms_e = w_e[:, None] * jvp.energy_dot
    forward = terms_mu.sum(axis=(-1, -2)) + terms_cov.sum(axis=(-1, -2, -3)) + terms_e.sum(axis=-1)
    size = np.abs(terms_mu).sum(axis=(-1, -2)) + np.abs(terms_cov).sum(axis=(-1, -2, -3)) + np.abs(terms_e).sum(axis=-1)
    worst, where = 0.0, None
    for d, (label, _) in enumerate(case["labelled"]):
        if label == "energy":
            reverse = np.asarray(g.energy, dtype=np.float64)
        else:
            e, name, component = label
            reverse = np.asarray(g[elements[e]][name], dtype=np.float64)
            reverse = reverse if component is None else reverse[:, component]
        assert reverse.shape == (B,) and size[:, d].all(), label
        dist = float(np.max(np.abs(forward[:, d] - reverse) / size[:, d]))
        if dist > worst:
            worst, where = dist, label
    print(f"adjoint identity through cavities, {name_of} lattice: worst |<w, J v> - <J^T w, v>| / sum |terms| = {worst:.2e} at {where}")
    bound = min(10 * ADJOINT_MEASURED[name_of], ADJOINT_CAP[name_of])
    assert worst <= bound, (where, worst, bound)


def test_the_response_matrix_of_a_line_with_two_cavities_is_its_closed_form(lx):
    """
    corrector - drift - cavity - drift - BPM - vcor - cavity - BPM, B = 2 with a voltage per sample, float64.  No element
    couples the transverse planes to (s, delta), so d(reading)/d(angle) is the first or third row of [the product of the
    oracle's maps between the corrector's exit and the BPM's entrance, each AT ITS OWN STEP'S ENERGY] times [the corrector's own
    part] -- to 1e-10, the tolerance of the closed form without cavities.  A BPM in front of a corrector reads an exact 0.
    """
    t, B = np.float64, 2
    f = lambda v: np.full(B, v, dtype=t)  # noqa: E731
    cavity = lambda v: ("cavity", dict(length=f(1.0377), voltage=np.array(v, dtype=t), phase=f(-8.0), frequency=f(1.3e9)))  # noqa: E731
    desc = [("hcor", dict(length=f(0.1), angle=f(2e-4))), ("drift", dict(length=f(0.5))), cavity([1.5e7, 2.5e7]), ("drift", dict(length=f(0.3))),
            ("bpm", {}), ("vcor", dict(length=f(0.2), angle=f(-1e-4))), cavity([2e7, 1e7]), ("bpm", {})]
    elements, specs = make_lattice(desc, t, lx)
    segment = lx.Segment(elements)
    energy = np.array([4e7, 6e7])
    beam = lx.ParameterBeam.from_parameters(mu_x=f(1e-4), mu_yp=f(-2e-5), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4),
                                            sigma_yp=f(1e-5), sigma_s=f(1e-4), sigma_p=f(1e-3), energy=energy, dtype=t)
    response = lx.grad.orbit_response_matrix(segment, beam, cavities=True)
    assert [el is elements[k] for el, k in zip(response.bpms, (4, 7))] == [True] * 2
    assert [el is elements[k] for el, k in zip(response.correctors, (0, 5))] == [True] * 2
    assert response.matrix.shape == (B, 4, 2) and response.matrix.dtype == np.float64
    energies, maps = [energy], []
    for spec in specs:
        maps.append(o.element_transfer_map(spec, energies[-1], t))
        gain = spec["voltage"] * np.cos(np.deg2rad(spec["phase"])) if spec["kind"] == "cavity" else 0.0
        energies.append(energies[-1] + gain)
    assert np.allclose(np.stack(energies, axis=1), np.asarray(response.jvp.trace.energy, dtype=t), rtol=1e-14)
    expected = np.zeros((B, 4, 2))
    for column, c in enumerate((0, 5)):
        unit, zero = dict(specs[c], angle=f(1.0)), dict(specs[c], angle=f(0.0))
        own = (o.element_transfer_map(unit, energies[c], t) - o.element_transfer_map(zero, energies[c], t))[:, :, 6]
        for row, p in enumerate((4, 7)):
            if p <= c:
                continue
            v = own
            for k in range(c + 1, p):
                v = np.einsum("bij,bj->bi", maps[k], v)
            expected[:, row, column], expected[:, 2 + row, column] = v[:, 0], v[:, 2]
    assert np.allclose(response.matrix, expected, rtol=1e-10, atol=1e-10), (response.matrix, expected)
    assert np.all(np.abs(expected[:, 0, 0]) > 0.1) and np.all(np.abs(expected[:, 3, 1]) > 0.1)
    # the cavities matter: the same product at the incoming energy is percent away
    flat = np.einsum("bij,bj->bi", o.element_transfer_map(specs[6], energy, t), own)[:, 2]
    assert np.all(np.abs(flat - expected[:, 3, 1]) > 1e-3 * np.abs(expected[:, 3, 1]))
    for row, column in [(0, 1), (2, 1), (2, 0), (3, 0)]:  # the BPM in front of the corrector, or the other plane
        assert np.all(response.matrix[:, row, column] == 0.0), (row, column, response.matrix[:, row, column])


def test_orbit_response_matrix_linac_example_corrects_the_orbit_in_one_step(lx):
    """examples/orbit_response_matrix_linac.py: with the matrix taken through the cavities the rms orbit at the BPMs falls to
    rounding level in one step -- the centroid's x, y are affine in the angles (no dipole), the least-squares step is exact and
    what is left is eps x the condition of the matrix, bounded here as the plain example's test bounds it, 1e-6 of the start; the
    matrix of the line with its cavities switched off leaves a residual far above that."""
    path = pathlib.Path(__file__).resolve().parents[1] / "examples" / "orbit_response_matrix_linac.py"
    spec = importlib.util.spec_from_file_location("orbit_response_matrix_linac", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    response, before, through, without = example.correct()
    print(f"linac orbit correction example: rms orbit {before:.3e} -> {through:.3e} through the cavities, {without:.3e} with them off")
    assert response.matrix.shape == (1, 4 * example.CELLS, 4 * example.CELLS)
    assert before > 1e-5 and through < 1e-6 * before, (before, through)
    assert without > 100 * through, (through, without)


# ---- shapes, against the restatement -------------------------------------------------------------------------------------------

def _tolerance(label, at_step, at_twice):
    """max(TOL_RESTATEMENT, 4 x the restatement's own differencing error), never looser than 1e-4: the restatement's dR comes
    from central differences whose error falls 4-fold from 2 STEP to STEP where truncation rules, and the T5xx formulas cancel."""
    own = max(ref.distance(a, b) for a, b in zip(at_step, at_twice))
    tol = max(TOL_RESTATEMENT, 4 * own)
    print(f"  {label}: tolerance {tol:.1e} ({'TOL_RESTATEMENT' if tol == TOL_RESTATEMENT else '4 x the differencing error'})")
    assert tol <= 1e-4, (label, own)
    return tol


def _held(jvp, d, specs, energy, mu, cov, direction, label):
    at_step = cref.sweep(specs, energy, mu, cov, direction)[3:]
    at_twice = cref.sweep(specs, energy, mu, cov, direction, step=2 * ref.STEP)[3:]
    tol = _tolerance(label, at_step[:2], at_twice[:2])
    dist = (ref.distance(jvp.mu_dot[:, d], at_step[0]), ref.distance(jvp.cov_dot[:, d], at_step[1]))
    assert max(dist) <= tol, (label, dist, tol)
    if at_step[2].any():
        assert ref.distance(jvp.energy_dot[:, d], at_step[2]) <= TOL_RESTATEMENT, label  # (no differencing in e_dot)
    else:
        assert not jvp.energy_dot[:, d].any(), label


def _against_restatement(lx, desc, wrt_of, directions, B, lx_desc=None, seed=5, energy=None):
    rng = np.random.default_rng(seed)
    _, specs = make_lattice(desc, np.float64)
    elements, _ = make_lattice(lx_desc or desc, np.float64, lx)
    mu, cov = incoming_moments(B, rng)
    energy = np.linspace(9e7, 1.1e8, B) if energy is None else energy
    wrt = wrt_of(elements)
    jvp = lx.grad.track_along_jvp(lx.Segment(elements), lx.ParameterBeam(mu, cov, energy, dtype=np.float64), wrt, cavities=True)
    assert jvp.mu_dot.shape == (B, len(wrt), len(desc) + 1, 7) and jvp.energy_dot.shape == (B, len(wrt), len(desc) + 1)
    for d, direction in enumerate(directions):
        _held(jvp, d, specs, energy, mu, cov, direction, (d, direction[0][:2]))
    return jvp


def _cavity(B, voltage=2e7, phase=-10.0, length=1.0377):
    f = lambda v: np.full(B, v)  # noqa: E731
    return ("cavity", dict(length=f(length), voltage=np.broadcast_to(np.asarray(voltage, dtype=np.float64), (B,)).copy(), phase=f(phase),
                           frequency=f(1.3e9)))


def test_one_sample_one_direction_one_cavity(lx):
    """B = 1, D = 1, E = 1: the lattice is one cavity, the direction its voltage."""
    jvp = _against_restatement(lx, [_cavity(1)], lambda el: [(el[0], "voltage")], [[(0, "voltage", None, 1.0)]], B=1)
    assert jvp.cov_dot.shape == (1, 1, 2, 7, 7) and np.any(jvp.cov_dot[0, 0, 1] != 0) and jvp.energy_dot[0, 0, 0] == 0.0
    assert jvp.energy_dot[0, 0, 1] == np.cos(np.deg2rad(-10.0))


def test_cavity_first_and_last_and_a_voltage_carried_through_a_second_cavity(lx):
    """cavity - quadrupole - drift - cavity, B = 3: the first element and the last are cavities; the first one's voltage and
    phase are carried through the second cavity (its map, coefficients and kick at an energy that moves); the last one's
    parameters reach the last point alone; the incoming energy passes both."""
    B = 3
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [_cavity(B, np.linspace(1e7, 3e7, B)), ("quadrupole", dict(length=f(0.2), k1=f(3.0))), ("drift", dict(length=f(0.5))),
            _cavity(B, 1.5e7, phase=12.0, length=1.0)]
    names = [(0, "voltage"), (0, "phase"), (0, "frequency"), (0, "length"), (3, "voltage"), (3, "phase"), (1, "k1")]
    jvp = _against_restatement(lx, desc, lambda el: [(el[e], name) for e, name in names] + ["energy"],
                               [[(e, name, None, 1.0)] for e, name in names] + [[(e, "energy", None, 1.0) for e in range(4)]], B=B)
    assert not jvp.cov_dot[:, 4, :4].any() and not jvp.energy_dot[:, 4, :4].any() and np.all(jvp.energy_dot[:, 4, 4] != 0)
    assert np.all(jvp.energy_dot[:, 0, 1:] == jvp.energy_dot[:, 0, 1:2]) and np.all(jvp.energy_dot[:, 7] == 1.0)


def test_one_direction_on_a_cavity_phase_and_a_quadrupole_behind_it(lx, monkeypatch):
    """A direction is a list of entries: the phase of a cavity (with its energy entries behind it) and the k1 of a quadrupole
    behind it as ONE direction -- the CSR of the two items merged, which `wrt` itself cannot say."""
    B = 2
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [_cavity(B, 2e7, phase=20.0), ("drift", dict(length=f(0.5))), ("quadrupole", dict(length=f(0.2), k1=f(-3.0))), ("drift", dict(length=f(0.4)))]
    own = lx.grad._jvp_directions

    def merged(leaves, wrt, cavities=False):
        start, leaf, row, weight = own(leaves, [(leaves[0], "phase"), (leaves[2], "k1")], cavities)
        return np.array([0, len(leaf)], dtype=np.int32), leaf, row, weight * np.where(row == 1, 0.5, 1.0)  # (k1 with weight 1/2)

    monkeypatch.setattr(lx.grad.jvp, "_jvp_directions", merged)  # (the module that holds `TrackAlongJVP`)
    _against_restatement(lx, desc, lambda el: [(el[0], "phase")], [[(0, "phase", None, 1.0), (2, "k1", None, 0.5)]], B=B)


def test_a_shared_voltage_beside_one_per_sample_and_a_cavity_placed_twice(lx):
    """A voltage shared by the batch (shape (1,), stride 0) beside one per sample; a cavity OBJECT placed twice is one direction
    with an entry per place, and the energy entries start behind the first place."""
    B = 3
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [_cavity(B, 2e7), ("drift", dict(length=f(0.5))), _cavity(B, np.linspace(1e7, 2e7, B), phase=5.0)]
    shared = ("cavity", dict(desc[0][1], voltage=np.array([2e7])))
    _against_restatement(lx, desc, lambda el: [(el[0], "voltage"), (el[2], "voltage"), (el[0], "phase")],
                         [[(0, "voltage", None, 1.0)], [(2, "voltage", None, 1.0)], [(0, "phase", None, 1.0)]], B=B,
                         lx_desc=[shared, desc[1], desc[2]])

    rng = np.random.default_rng(8)
    mu, cov = incoming_moments(B, rng)
    energy = np.full(B, 8e7)
    cav = lx.Cavity(f(1.0377), voltage=np.linspace(1e7, 2e7, B), phase=f(-10.0), frequency=f(1.3e9), dtype=np.float64)
    q = lx.Quadrupole(f(0.2), k1=f(3.0), dtype=np.float64)
    jvp = lx.grad.track_along_jvp(lx.Segment([cav, q, cav]), lx.ParameterBeam(mu, cov, energy, dtype=np.float64),
                                  [(cav, "voltage"), (cav, "phase")], cavities=True)
    specs = [o.Cavity(f(1.0377), np.linspace(1e7, 2e7, B), f(-10.0), f(1.3e9)), o.Quadrupole(f(0.2), k1=f(3.0)),
             o.Cavity(f(1.0377), np.linspace(1e7, 2e7, B), f(-10.0), f(1.3e9))]
    for d, name in enumerate(("voltage", "phase")):
        _held(jvp, d, specs, energy, mu, cov, [(0, name, None, 1.0), (2, name, None, 1.0)], ("placed twice", name))
    assert np.all(jvp.energy_dot[:, 0, 3] == 2 * jvp.energy_dot[:, 0, 1])


def test_seventy_directions_through_cavities(lx):
    """D = 70 over a six-element line with two cavities, B = 3: equal directions give equal bits wherever they sit."""
    B = 3
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = [("quadrupole", dict(length=f(0.2), k1=f(4.2))), _cavity(B), ("drift", dict(length=f(0.5))), ("quadrupole", dict(length=f(0.2), k1=f(-4.2))),
            _cavity(B, 1e7, phase=8.0), ("drift", dict(length=f(0.5)))]
    kinds = [lambda el: (el[1], "voltage"), lambda el: (el[4], "phase"), lambda el: "energy", lambda el: (el[0], "k1"), lambda el: (el[5], "length")]
    entries = [[(1, "voltage", None, 1.0)], [(4, "phase", None, 1.0)], [(e, "energy", None, 1.0) for e in range(6)],
               [(0, "k1", None, 1.0)], [(5, "length", None, 1.0)]]
    jvp = _against_restatement(lx, desc, lambda el: [kinds[d % 5](el) for d in range(70)], entries, B=B)
    for d in range(5, 70):
        for a in (jvp.mu_dot, jvp.cov_dot, jvp.energy_dot):
            assert a[:, d].tobytes() == a[:, d % 5].tobytes(), d


@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_without_a_cavity_the_keyword_changes_no_bit(lx, beam_type):
    """`cavities=True` on the cavity-free lattice of tests/test_gpu_trace_jvp.py takes the existing path: mu_dot and cov_dot
    byte for byte those of the plain call, for both beam classes; energy_dot keeps its shape (D,)."""
    case = fd_case(lx)
    segment = lx.Segment(case["elements"])
    plain = lx.grad.track_along_jvp(segment, _beam(lx, case, beam_type, np.float64), case["wrt"])
    keyword = lx.grad.track_along_jvp(segment, _beam(lx, case, beam_type, np.float64), case["wrt"], cavities=True)
    assert keyword.mu_dot.tobytes() == plain.mu_dot.tobytes() and keyword.cov_dot.tobytes() == plain.cov_dot.tobytes()
    assert keyword.energy_dot.shape == (len(case["wrt"]),) and np.array_equal(keyword.energy_dot, plain.energy_dot)
    assert np.any(plain.cov_dot != 0)


# distance max |g - r| / (|r| + 1e-3 max |r|) of the float32 lattice's tangents g from the float64 pass r of
# the same input, the maximum per sample over a direction's whole curve, as test_float32_against_the_float64_pass measured it
# on MI355X over the three directions; asserted at twice that and never looser than 1e-2:
#     sigma_x 2.4e-06   beta_x 8.2e-06   mu_dot[..., 0] 2.6e-06   energy 0 (voltage and phase are float32 numbers: the same walk)
# The incoming beam is MATCHED to the cell (the periodic solution of quadrupole - drift - quadrupole - drift at k1 = 4.2 without the
# cavities: beta_x 3.29 m, alpha_x -1.37, beta_y 2.14 m, alpha_y 0.93; emittance 3e-9 m).  "Float32 Twiss values of a ParameterBeam
# are as good as the beam is matched" (DESIGN.md section 2): the tangent of beta_x contracts C_dot with -(beta / 2 eps) C^-1, a sum
# that cancels (1 + alpha^2)-fold, and along a cavity's voltage or phase it cancels once more -- adiabatic damping scales C and
# leaves beta alone, what moves beta is the cavity's focusing, 1/15 of it.  With the round 100 um x 10 urad beam of
# tests/test_gpu_trace_jvp.py on this line (alpha up to 20) beta_x along the phase was 0.46 away on MI355X, and float64 tangents
# whose states and C_dot are merely ROUNDED to float32 are already 4e-2 away: no property of the kernels.
MATCHED, EMITTANCE = ((3.29, -1.37), (2.14, 0.93)), 3e-9
F32_MEASURED = {"sigma_x": 2.4e-06, "beta_x": 8.2e-06, "mu_x": 2.6e-06, "energy": 0.0}


def test_float32_against_the_float64_pass_through_cavities(lx):
    """A 16-element FODO line with two cavities of 20 MV on 100 MeV, B = 2 with k1 scaled 1 and 0.8: one cavity's voltage, its
    phase and the k1 of the quadrupole in front of it; `tangent("sigma_x")`, `tangent("beta_x")`, `mu_dot[..., 0]` and
    `tangent("energy")`.  cov_dot[4][4], [4][5], [5][4] are NOT held in float32: the reference's T5xx formulas cancel there
    (DESIGN.md section 2); the finite-difference test above holds them in float64."""
    B = 2
    specs = o.fodo_segment(4, dtype=np.float32, batch_shape=(B,), k1_scale=np.array([1.0, 0.8], dtype=np.float32))
    sigma = np.array([1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])

    def tangents(dtype):
        cast = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)  # noqa: E731  (the float32 lattice's own numbers)
        full = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
        elements = [lx.Quadrupole(cast(s["length"]), k1=cast(s["k1"]), dtype=dtype) if s["kind"] == "quadrupole"
                    else lx.Drift(cast(s["length"]), dtype=dtype) for s in specs]
        for place in (5, 13):  # a drift of each of two cells becomes a cavity
            elements[place] = lx.Cavity(full(1.0), voltage=full(2e7), phase=full(-10.0), frequency=full(1.3e9), dtype=dtype)
        mu = np.zeros((B, 7), dtype=dtype)
        mu[:, :6] = np.array([1e-4, -1e-5, 5e-5, 2e-5, 1e-5, 1e-4], dtype=np.float32).astype(dtype)
        mu[:, 6] = 1
        cov = np.zeros((B, 7, 7), dtype=dtype)
        cov[:, range(6), range(6)] = (sigma**2).astype(np.float32).astype(dtype)
        for a, (beta, alpha) in ((0, MATCHED[0]), (2, MATCHED[1])):
            block = EMITTANCE * np.array([[beta, -alpha], [-alpha, (1 + alpha**2) / beta]])
            cov[:, a:a + 2, a:a + 2] = block.astype(np.float32).astype(dtype)
        beam = lx.ParameterBeam(mu, cov, np.full(B, 1e8, dtype=dtype), dtype=dtype)
        jvp = lx.grad.track_along_jvp(lx.Segment(elements), beam, [(elements[5], "voltage"), (elements[5], "phase"), (elements[4], "k1")],
                                      cavities=True)
        return dict(sigma_x=jvp.tangent("sigma_x"), beta_x=jvp.tangent("beta_x"), mu_x=jvp.mu_dot[..., 0], energy=jvp.tangent("energy"))

    t32, t64 = tangents(np.float32), tangents(np.float64)
    measured = {}
    for name, r in t64.items():
        g = t32[name]
        assert g.shape == r.shape == (B, 3, 17) and np.all(np.isfinite(g)), name
        moving = [d for d in range(3) if r[:, d].any()]  # (the energy does not move with k1)
        assert len(moving) == (2 if name == "energy" else 3), (name, moving)
        measured[name] = max(ref.distance(g[:, d], r[:, d]) for d in moving)
        assert all(not g[:, d].any() for d in range(3) if d not in moving), name
    print("float32 track_along_jvp(cavities=True) against float64: " + ", ".join(f"{k} {v:.1e}" for k, v in measured.items()))
    for name, value in measured.items():
        assert value <= min(2 * F32_MEASURED[name], 1e-2), (name, value)


# ---- the C entry point: what it refuses, where it writes -----------------------------------------------------------------------

ENTRY = "lynx_track_moments_along_forward_cavities"
# the "cavity" lattice of tests/entry_calls.py (inactive aperture, drift, ACTIVE cavity, quadrupole): the drift's length; the
# cavity's voltage with the energy behind it; the quadrupole's k1 twice on its leaf, its length and the cavity's phase in front
# of them, handed over out of order; the incoming energy at every leaf; a direction without entries
DIRECTIONS = dict(start=[0, 1, 3, 8, 12, 12], leaf=[1, 2, 3, 3, 3, 3, 2, 3, 0, 1, 2, 3], row=[0, 1, 8, 1, 0, 1, 2, 8, 8, 8, 8, 8],
                  weight=[1.0, 1.0, 1.0, 0.5, 2.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], seed=[0.0, 0.0, 0.0, 1.0, 0.0])


def env_of(shape, dtype):
    key = (shape, np.dtype(dtype))
    if key not in _envs:
        _envs[key] = ec.make_env(shape, dtype)
    return _envs[key]


def _call(env, pointer, directions=DIRECTIONS, **change):
    rt = env.rt
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    doubles = lambda v: (C.c_double * max(len(v), 1))(*v)  # noqa: E731
    d = dict(start=ints(directions["start"]), leaf=ints(directions["leaf"]), row=ints(directions["row"]), weight=doubles(directions["weight"]),
             seed=doubles(directions["seed"]), count=len(directions["start"]) - 1, entries=len(directions["leaf"]), lat=env.lat.handle,
             e_in=pointer("e_in"), mu_tr=pointer("mu_tr"), cov_tr=pointer("cov_tr"), mu_dot=pointer("mu_dot"), cov_dot=pointer("cov_dot"),
             e_dot=pointer("e_dot"))
    d.update(change)
    return rt.lib.lynx_track_moments_along_forward_cavities(
        rt.ctx, d["lat"], d["e_in"], d["mu_tr"], d["cov_tr"], d["start"], d["leaf"], d["row"], d["weight"], d["count"], d["entries"],
        d["mu_dot"], d["cov_dot"], d["seed"], d["e_dot"])


def _arrays(env, D=5):
    s, t = env.shape, env.dtype
    return [ec.Array("e_in", t, (s.B,), "in"), ec.Array("mu_tr", t, (s.B, s.P, 7), "in"), ec.Array("cov_tr", t, (s.B, s.P, 49), "in"),
            ec.Array("mu_dot", ec.F64, (s.B, D, s.P, 7), "out"), ec.Array("cov_dot", ec.F64, (s.B, D, s.P, 49), "out"),
            ec.Array("e_dot", ec.F64, (s.B, D, s.P), "out")]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_the_entry_point_writes_all_of_its_tangents_and_nothing_else(lx, dtype):
    """The checks of test_gpu_entry_footprint.py (tests/entry_footprint.py) for the new entry: every array of the call in ONE
    block between guards, the call over a block of 0x00 and of 0xFF; nothing outside d_mu_dot, d_cov_dot and d_energy_dot
    changes, every byte of the three is written whatever was there, and the bytes are those of the call into blocks of their
    own."""
    for row in ((1, 1, 1, 1, 1), (3, 65, 5, 3, 3)):
        env = env_of(ec.Shape(*row, "cavity"), dtype)
        rt, arrays = env.rt, _arrays(env)
        arena = fp.plan_arena(arrays)
        fp.check_plan(arena)
        base = rt.alloc(arena.nbytes)
        try:
            pointer = lambda name: C.c_void_p(base + arena.regions[name].start) if name in arena.regions else None  # noqa: E731
            runs = []
            for value in (0x00, 0xFF):
                rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(base), value, arena.nbytes))
                before = np.full(arena.nbytes, value, dtype=np.uint8)
                for a in arrays:
                    if a.role == "in":
                        host = np.ascontiguousarray(env.host[a.name]).reshape(a.shape)
                        arena.view(before, a.name)[...] = host
                        rt.check(rt.lib.lynx_buf_h2d(rt.ctx, pointer(a.name), host.ctypes.data, host.nbytes))
                assert _call(env, pointer) == 0, rt.lib.lynx_last_error(rt.ctx).decode()
                after = np.empty(arena.nbytes, dtype=np.uint8)
                rt.check(rt.lib.lynx_buf_d2h(rt.ctx, after.ctypes.data, C.c_void_p(base), after.nbytes))
                fp.nothing_else_written(arena, before, after)
                runs.append(after)
            fp.outputs_identical(arena, runs[0], runs[1])
            own = {a.name: rt.empty(a.shape, a.dtype) for a in arrays if a.role == "out"}
            ordinary = lambda name: C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
            assert _call(env, ordinary) == 0, rt.lib.lynx_last_error(rt.ctx).decode()
            for name, block in own.items():
                fp.same_as(arena, runs[1], name, block.numpy())
            mu_dot, cov_dot, e_dot = (arena.view(runs[1], name) for name in ("mu_dot", "cov_dot", "e_dot"))
            assert np.any(mu_dot[:, :4] != 0) and np.any(cov_dot[:, :4] != 0)
            for block in (mu_dot, cov_dot, e_dot):  # the direction without entries
                assert not block[:, 4].view(np.uint64).any()
            # the energy's tangent: cos(0) behind the cavity (point 3 on) along its voltage, 1 everywhere along the energy
            assert np.all(e_dot[:, 1, :3] == 0) and np.all(e_dot[:, 1, 3:] == 1.0) and np.all(e_dot[:, 3] == 1.0) and not e_dot[:, 0].any()
        finally:
            rt.sync()
            rt.free(base)


def test_what_the_entry_point_refuses(lx):
    """LYNX_ERR_INVALID before anything is launched, the message starting "beam trace tangents: "."""
    from lynx_amd import engine

    env = env_of(ec.Shape(3, 65, 5, 3, 3, "cavity"), np.float64)
    rt = env.rt
    own = {a.name: rt.empty(a.shape, a.dtype) for a in _arrays(env) if a.role == "out"}
    pointer = lambda name: C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
    assert _call(env, pointer) == 0, rt.lib.lynx_last_error(rt.ctx).decode()

    def refused(expect, directions=DIRECTIONS, **change):
        assert _call(env, pointer, directions, **change) == -1, expect
        message = rt.lib.lynx_last_error(rt.ctx).decode()
        assert message.startswith("beam trace tangents: ") and expect in message, (expect, message)

    for name in ("mu_dot", "cov_dot", "e_dot", "e_in", "weight", "mu_tr", "cov_tr", "seed", "start"):
        refused("null argument", **{name: None})
    refused("n_directions must be > 0", count=0)
    refused("leaf 4 out of range", dict(DIRECTIONS, leaf=[4] + DIRECTIONS["leaf"][1:]))
    refused("leaf -1 out of range", dict(DIRECTIONS, leaf=[-1] + DIRECTIONS["leaf"][1:]))
    refused("row 9 out of range", dict(DIRECTIONS, row=[9] + DIRECTIONS["row"][1:]))
    refused("has no parameter row 1", dict(DIRECTIONS, row=[1] + DIRECTIONS["row"][1:]))  # a drift has its length alone
    refused("has no parameter row 0", dict(DIRECTIONS, leaf=[0] + DIRECTIONS["leaf"][1:]))  # an aperture has none
    refused("dir_start", dict(DIRECTIONS, start=[0, 1, 3, 8, 12, 11]))
    refused("dir_start", dict(DIRECTIONS, start=[0, 3, 1, 8, 12, 12]))
    # voltage, phase, frequency of a cavity that is not a cavity step (no voltage: a drift-like element of a run); its length passes
    t = np.float64
    f = lambda v: np.full(3, v, dtype=t)  # noqa: E731
    leaves = [lx.Drift(f(0.7), dtype=t), lx.Cavity(f(1.0), voltage=f(0.0), phase=f(0.0), frequency=f(1.3e9), dtype=t),
              lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), dtype=t)]
    cache = engine.LatticeCache()
    idle = engine._ready(cache, engine.trace_program(leaves), (3,), t, env.host["e_in"])
    for row in (1, 2, 3):
        refused("not a cavity step", dict(start=[0, 1], leaf=[1], row=[row], weight=[1.0], seed=[0.0]), lat=idle.handle)
    refused("row 9 out of range", dict(start=[0, 1], leaf=[1], row=[9], weight=[1.0], seed=[0.0]), lat=idle.handle)
