"""
`lynx_amd.grad.track_along_jvp` and `orbit_response_matrix` on the GPU (lynx_track_moments_along_forward,
lynx_track_particles_along_forward): the tangents of the moments at EVERY point of a lattice against central differences of
the oracle's element-by-element chain in float64; the adjoint identity <w, J v> = <J^T w, v> against `track_along_vjp`, which is
pinned to finite differences itself; the response matrix against its closed form; the shapes at which the kernels can go
wrong, against the NumPy restatement of tests/trace_jvp_reference.py; float32 against the float64 pass; what the two entry
points refuse and where they write.
"""

import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import entry_calls as ec
from . import entry_footprint as fp
from . import trace_jvp_reference as ref
from .helpers import make_lattice
from .test_trace_jvp_host import TOL_FD, directions_to_check, incoming_moments, lattice_without_cavities

pytestmark = pytest.mark.gpu

# The restatement's dM comes from central differences of the oracle's maps with h = 1e-6 of the parameter: good to eps / h =
# 2e-10 of a map's entries per element, and the largest lattice here has 300 elements in a stable FODO channel (an error made
# at one element is carried on with a gain of a few): 300 x 2e-10 x 10 < 1e-6, in the distance of `ref.distance`.
TOL_RESTATEMENT = 1e-6


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _wrt(elements, labelled):
    """`directions_to_check`'s labels as the `wrt` of track_along_jvp."""
    out = []
    for label, _ in labelled:
        if label == "energy":
            out.append("energy")
        else:
            e, name, component = label
            out.append((elements[e], name) if component is None else (elements[e], name, component))
    return out


_case = {}


def fd_case(lx, dtype=np.float64):
    """The nine-element lattice without its cavities, B = 2, its incoming moments and particles, every direction to check."""
    if dtype not in _case:
        rng = np.random.default_rng(23)
        B = 2
        desc = lattice_without_cavities(B, rng)
        elements, specs = make_lattice(desc, dtype, lx)
        _, specs64 = make_lattice(desc, np.float64)
        mu, cov = incoming_moments(B, rng)
        particles = o.gaussian_particles((B,), 400, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3],
                                         mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])
        labelled = directions_to_check(desc, specs64)
        _case[dtype] = dict(desc=desc, elements=elements, specs=specs64, mu=mu, cov=cov, particles=particles,
                            energy=np.array([6e6, 8e6]), labelled=labelled, wrt=_wrt(elements, labelled))
    return _case[dtype]


def _beam(lx, case, beam_type, dtype):
    if beam_type == "parameters":
        return lx.ParameterBeam(case["mu"].astype(dtype), case["cov"].astype(dtype), case["energy"].astype(dtype), dtype=dtype)
    return lx.ParticleBeam(case["particles"].astype(dtype), case["energy"].astype(dtype), dtype=dtype)


@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_tangents_at_every_point_match_finite_differences_of_the_oracle_chain_fp64(lx, beam_type):
    """
    mu_dot and cov_dot at all ten points, for every parameter of PARAMS_TO_CHECK of every element and for "energy", against
    central differences (h = 1e-6 max(|x|, 1e-2)) of the oracle's chain -- of ParameterBeams, and of 400 particles whose mean
    and biased covariance are taken in float64 -- at 2e-4 of the value (`ref.distance`, the quotient's own rounding taken off).
    The same call twice gives the same bits; the 7th row and column are exact zeros.
    """
    case = fd_case(lx)
    segment = lx.Segment(case["elements"])
    jvp = lx.grad.track_along_jvp(segment, _beam(lx, case, beam_type, np.float64), case["wrt"])
    B, D, P = 2, len(case["wrt"]), 10
    assert jvp.mu_dot.shape == (B, D, P, 7) and jvp.cov_dot.shape == (B, D, P, 7, 7) and jvp.trace.num_points == P
    assert jvp.mu_dot.dtype == np.float64 and jvp.cov_dot.dtype == np.float64 and jvp.wrt == case["wrt"]
    if beam_type == "parameters":
        make_beam, moments = (lambda e: o.parameter_beam(case["mu"], case["cov"], e, np.float64)), ref.parameter_moments
    else:
        make_beam, moments = (lambda e: o.particle_beam(case["particles"], e, np.float64)), ref.particle_moments
    worst = 0.0
    for d, (label, direction) in enumerate(case["labelled"]):
        fd_mu, fd_cov, noise_mu, noise_cov = ref.chain_tangents(case["specs"], make_beam, moments, case["energy"], direction)
        dist = (ref.distance(jvp.mu_dot[:, d], fd_mu, noise_mu), ref.distance(jvp.cov_dot[:, d], fd_cov, noise_cov))
        worst = max(worst, ref.distance(jvp.mu_dot[:, d], fd_mu), ref.distance(jvp.cov_dot[:, d], fd_cov))
        assert max(dist) <= TOL_FD, (label, dist)
    print(f"track_along_jvp against central differences of the oracle chain, {beam_type}: {D} directions, worst distance "
          f"{worst:.1e} with the quotients' own rounding left in")
    assert D > 20
    for tangents in (jvp.mu_dot[..., 6], jvp.cov_dot[..., 6, :], jvp.cov_dot[..., :, 6], jvp.mu_dot[:, :, 0], jvp.cov_dot[:, :, 0]):
        assert not tangents.any()  # exact zeros
    again = lx.grad.track_along_jvp(segment, _beam(lx, case, beam_type, np.float64), case["wrt"])
    assert again.mu_dot.tobytes() == jvp.mu_dot.tobytes() and again.cov_dot.tobytes() == jvp.cov_dot.tobytes()
    # the energy's own tangent is exact
    energy = jvp.tangent("energy")
    assert energy.shape == (B, D, P) and np.all(energy[:, -1] == 1.0) and not energy[:, :-1].any()


# The worst distance |<w, J v> - <J^T w, v>| / sum |terms| measured on MI355X over every direction of the case above (both
# sides are float64 sweeps over the same states; a float32 lattice's maps, dM and reverse pass are float32):
#                      parameters      particles
#     float64 lattice    1.41e-16        1.48e-16
#     float32 lattice    6.07e-08        4.42e-08
# asserted at ten times that, and never looser than 1e-8 (float64 lattice) and 1e-3 (float32 lattice).
ADJOINT_MEASURED = {("parameters", "float64"): 1.41e-16, ("particles", "float64"): 1.48e-16,
                    ("parameters", "float32"): 6.07e-08, ("particles", "float32"): 4.42e-08}
ADJOINT_CAP = {"float64": 1e-8, "float32": 1e-3}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_the_adjoint_identity_against_track_along_vjp(lx, beam_type, dtype):
    """
    Random w_mu, w_cov at all points: sum_k <w_mu, mu_dot> + <w_cov, cov_dot> per sample and direction is the gradient
    `track_along_vjp(...)(mu_bar=w_mu, cov_bar=w_cov)` has at that parameter -- <w, J v> = <J^T w, v>, the reverse side being
    held to finite differences by test_gpu_trace_grad.py.
    """
    case = fd_case(lx, dtype)
    elements, name_of = case["elements"], np.dtype(dtype).name
    segment = lx.Segment(elements)
    beam = _beam(lx, case, beam_type, dtype)
    rng = np.random.default_rng(77)
    B, P = 2, 10
    w_mu, w_cov = rng.normal(size=(B, P, 6)), rng.normal(size=(B, P, 6, 6)) * 1e3
    jvp = lx.grad.track_along_jvp(segment, beam, case["wrt"])
    g = lx.grad.track_along_vjp(segment, beam)(mu_bar=w_mu, cov_bar=w_cov)
    terms_mu = w_mu[:, None] * jvp.mu_dot[..., :6]
    terms_cov = w_cov[:, None] * jvp.cov_dot[..., :6, :6]
    forward = terms_mu.sum(axis=(-1, -2)) + terms_cov.sum(axis=(-1, -2, -3))
    size = np.abs(terms_mu).sum(axis=(-1, -2)) + np.abs(terms_cov).sum(axis=(-1, -2, -3))
    worst, where = 0.0, None
    for d, (label, _) in enumerate(case["labelled"]):
        if label == "energy":
            reverse = np.asarray(g.energy, dtype=np.float64)
        else:
            e, name, component = label
            reverse = np.asarray(g[elements[e]][name], dtype=np.float64)
            reverse = reverse if component is None else reverse[:, component]
        assert reverse.shape == (B,), label
        if not size[:, d].any():
            assert not reverse.any() and not forward[:, d].any(), label
            continue
        dist = float(np.max(np.abs(forward[:, d] - reverse) / size[:, d]))
        if dist > worst:
            worst, where = dist, label
    print(f"adjoint identity, {beam_type}, {name_of} lattice: worst |<w, J v> - <J^T w, v>| / sum |terms| = {worst:.2e} at {where}")
    bound = min(10 * ADJOINT_MEASURED[(beam_type, name_of)], ADJOINT_CAP[name_of])
    assert worst <= bound, (where, worst, bound)


def test_the_response_matrix_of_a_drift_quadrupole_line_is_its_closed_form(lx):
    """
    Two correctors and three BPMs, float64.  d(reading)/d(angle) is the first or third row of [the product of the oracle's maps
    between the corrector's exit and the BPM's entrance] times [the corrector's own part, d(its map's column 6)/d(angle)] --
    the oracle's thick corrector kicks at its exit, so its own part is the unit kick in x' (y') and nothing in x (y).  A BPM
    in front of a corrector reads an exact 0.
    """
    t = np.float64
    f = lambda v: np.array([v], dtype=t)  # noqa: E731
    desc = [("bpm", {}), ("hcor", dict(length=f(0.1), angle=f(2e-4))), ("drift", dict(length=f(0.5))),
            ("quadrupole", dict(length=f(0.2), k1=f(2.0))), ("bpm", {}), ("vcor", dict(length=f(0.2), angle=f(-1e-4))),
            ("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.2), k1=f(-3.0))), ("drift", dict(length=f(0.4))), ("bpm", {})]
    elements, specs = make_lattice(desc, t, lx)
    segment = lx.Segment(elements)
    energy = f(1e8)
    beam = lx.ParameterBeam.from_parameters(mu_x=f(1e-4), mu_yp=f(-2e-5), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4),
                                            sigma_yp=f(1e-5), energy=energy, dtype=t)
    response = lx.grad.orbit_response_matrix(segment, beam)
    assert [el is elements[k] for el, k in zip(response.bpms, (0, 4, 9))] == [True] * 3
    assert [el is elements[k] for el, k in zip(response.correctors, (1, 5))] == [True] * 2
    assert response.matrix.shape == (1, 6, 2) and response.matrix.dtype == np.float64
    maps = [o.element_transfer_map(spec, energy, t)[0] for spec in specs]
    expected = np.zeros((6, 2))
    for column, c in enumerate((1, 5)):
        unit = dict(specs[c], angle=f(1.0))
        own = (o.element_transfer_map(unit, energy, t)[0] - o.element_transfer_map(dict(specs[c], angle=f(0.0)), energy, t)[0])[:, 6]
        for row, p in enumerate((0, 4, 9)):
            if p <= c:
                continue
            between = np.eye(7)
            for k in range(c + 1, p):
                between = maps[k] @ between
            expected[row, column], expected[3 + row, column] = (between @ own)[0], (between @ own)[2]
    assert np.allclose(response.matrix[0], expected, rtol=1e-10, atol=1e-10), (response.matrix[0], expected)
    assert abs(expected[2, 0]) > 0.1 and abs(expected[5, 1]) > 0.1 and abs(expected[1, 0]) > 0.1
    in_front = [(0, 0), (0, 1), (1, 1), (3, 0), (3, 1), (4, 1)]  # (row, column): the BPM lies in front of the corrector
    for row, column in in_front:
        assert response.matrix[0, row, column] == 0.0, (row, column, response.matrix[0, row, column])
    # chosen BPMs and correctors, in the order given
    chosen = lx.grad.orbit_response_matrix(segment, beam, bpms=[elements[9], elements[4]], correctors=[elements[5]])
    assert chosen.matrix.shape == (1, 4, 1)
    assert np.array_equal(chosen.matrix[0, :, 0], response.matrix[0, [2, 1, 5, 4], 1])
    # a reading's tangent is mu_dot's x and y at the BPM's point
    assert np.array_equal(response.jvp.reading_tangents(elements[9]), response.jvp.mu_dot[:, :, 9][..., (0, 2)])
    with pytest.raises(KeyError):
        response.jvp.reading_tangents(lx.BPM(name="elsewhere"))


def test_orbit_response_matrix_example_corrects_the_orbit_in_one_step(lx):
    """examples/orbit_response_matrix.py: the rms orbit at the BPMs falls below 1e-6 of its starting value in float64."""
    path = pathlib.Path(__file__).resolve().parents[1] / "examples" / "orbit_response_matrix.py"
    spec = importlib.util.spec_from_file_location("orbit_response_matrix", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    response, before, after = example.correct(example.fodo_line(), example.incoming_beam())
    print(f"orbit correction example: rms orbit {before:.3e} -> {after:.3e}")
    assert response.matrix.shape == (1, 4 * example.CELLS, 4 * example.CELLS)
    assert before > 1e-5 and after < 1e-6 * before, (before, after)


def _against_restatement(lx, desc, wrt_of, directions, beam_type="parameters", B=None, dtype=np.float64, lx_desc=None, seed=5):
    """
    One lattice (`desc` for the oracle, `lx_desc` for the package where the shapes of the parameters differ), one beam, the
    directions `wrt_of(elements)` -- whose restatement entries are `directions` -- at TOL_RESTATEMENT; returns the TrackAlongJVP.
    """
    rng = np.random.default_rng(seed)
    _, specs = make_lattice(desc, np.float64)
    elements, _ = make_lattice(lx_desc or desc, dtype, lx)
    mu, cov = incoming_moments(B, rng)
    energy = np.linspace(9e7, 1.1e8, B)
    beam = lx.ParameterBeam(mu, cov, energy, dtype=dtype)
    wrt = wrt_of(elements)
    jvp = lx.grad.track_along_jvp(lx.Segment(elements), beam, wrt)
    assert jvp.mu_dot.shape == (B, len(wrt), len(desc) + 1, 7)
    for d, direction in enumerate(directions):
        _, _, mu_dot, cov_dot = ref.sweep(specs, energy, mu, cov, direction)
        dist = (ref.distance(jvp.mu_dot[:, d], mu_dot), ref.distance(jvp.cov_dot[:, d], cov_dot))
        assert max(dist) <= TOL_RESTATEMENT, (d, direction[:3], dist)
    return jvp


def _fodo(B, cells, k1=4.2):
    f = lambda v: np.full(B, v)  # noqa: E731
    return [item for _ in range(cells) for item in (("quadrupole", dict(length=f(0.2), k1=f(k1))), ("drift", dict(length=f(0.5))),
                                                    ("quadrupole", dict(length=f(0.2), k1=f(-k1))), ("drift", dict(length=f(0.5))))]


def test_one_sample_one_direction_one_element(lx):
    """B = 1, D = 1, E = 1: the direction's only entry is the first element and the last."""
    desc = [("quadrupole", dict(length=np.array([0.2]), k1=np.array([3.0])))]
    jvp = _against_restatement(lx, desc, lambda el: [(el[0], "k1")], [[(0, "k1", None, 1.0)]], B=1)
    assert jvp.cov_dot.shape == (1, 1, 2, 7, 7) and jvp.tangent("beta_x").shape == (1, 1, 2) and np.any(jvp.cov_dot[0, 0, 1] != 0)


def test_seventy_directions_first_and_last_element_and_equal_directions(lx):
    """
    D = 70 over an eight-element line, B = 3 (grid indexing beyond one wave's worth of directions): a direction whose only entry
    is the first element, one whose only entry is the last, the energy, and the same few again and again -- equal directions
    give equal bits wherever they sit.
    """
    B = 3
    desc = _fodo(B, 2)
    kinds = [lambda el: (el[0], "k1"), lambda el: (el[7], "length"), lambda el: "energy", lambda el: (el[2], "k1"), lambda el: (el[3], "length")]
    entries = [[(0, "k1", None, 1.0)], [(7, "length", None, 1.0)], [(e, "energy", None, 1.0) for e in range(8)],
               [(2, "k1", None, 1.0)], [(3, "length", None, 1.0)]]
    jvp = _against_restatement(lx, desc, lambda el: [kinds[d % 5](el) for d in range(70)], entries, B=B)
    assert jvp.mu_dot.shape == (B, 70, 9, 7)
    for d in range(5, 70):
        assert jvp.mu_dot[:, d].tobytes() == jvp.mu_dot[:, d % 5].tobytes() and jvp.cov_dot[:, d].tobytes() == jvp.cov_dot[:, d % 5].tobytes(), d
    assert not jvp.cov_dot[:, 1, :8].any() and np.all(np.abs(jvp.cov_dot[:, 1, 8]).max(axis=(-1, -2)) > 0)  # the last element alone
    assert np.all(np.abs(jvp.cov_dot[:, 0, 1]).max(axis=(-1, -2)) > 0)  # the first: from point 1 on


def test_entries_that_share_a_leaf_an_object_placed_three_times_and_shared_parameters(lx):
    """
    RBend.angle is three entries on ONE leaf (angle, and e1, e2 with weight 1/2: the oracle's RBend moves its pole faces with
    its angle); a quadrupole object placed three times is one direction of three entries; a parameter shared over the batch
    (shape (1,), stride 0) next to one per sample.
    """
    B = 3
    f = lambda v: np.full(B, v)  # noqa: E731
    one = lambda v: np.array([v])  # noqa: E731
    bend = dict(length=f(0.5), angle=np.linspace(0.05, 0.2, B), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4), gap=f(0.02))
    desc = [("drift", dict(length=f(0.3))), ("rbend", bend), ("drift", dict(length=f(0.4)))]
    _against_restatement(lx, desc, lambda el: [(el[1], "angle"), (el[1], "e1")], [[(1, "angle", None, 1.0)], [(1, "e1", None, 1.0)]], B=B)

    rng = np.random.default_rng(8)
    mu, cov = incoming_moments(B, rng)
    energy = np.full(B, 1e8)
    q = lx.Quadrupole(one(0.2), k1=one(3.0), dtype=np.float64)  # shared by the batch
    own = lx.Quadrupole(f(0.2), k1=np.linspace(-3.0, -1.0, B), dtype=np.float64)  # one per sample
    d = lx.Drift(f(0.5), dtype=np.float64)
    jvp = lx.grad.track_along_jvp(lx.Segment([q, d, own, q, d, q]), lx.ParameterBeam(mu, cov, energy, dtype=np.float64),
                                  [(q, "k1"), (own, "k1"), (d, "length")])
    specs = [o.Quadrupole(f(0.2), k1=f(3.0)), o.Drift(f(0.5)), o.Quadrupole(f(0.2), k1=np.linspace(-3.0, -1.0, B)),
             o.Quadrupole(f(0.2), k1=f(3.0)), o.Drift(f(0.5)), o.Quadrupole(f(0.2), k1=f(3.0))]
    for k, direction in enumerate(([(e, "k1", None, 1.0) for e in (0, 3, 5)], [(2, "k1", None, 1.0)], [(e, "length", None, 1.0) for e in (1, 4)])):
        _, _, mu_dot, cov_dot = ref.sweep(specs, energy, mu, cov, direction)
        dist = (ref.distance(jvp.mu_dot[:, k], mu_dot), ref.distance(jvp.cov_dot[:, k], cov_dot))
        assert max(dist) <= TOL_RESTATEMENT, (k, dist)


def test_three_hundred_elements(lx):
    """E = 300 at B = 2 (the table comes from the lanes = samples build), against the restatement: the first quadrupole, one
    in the middle, the last drift, and the energy with its 300 entries."""
    B = 2
    desc = _fodo(B, 75)
    entries = [[(0, "k1", None, 1.0)], [(150, "k1", None, 1.0)], [(299, "length", None, 1.0)], [(e, "energy", None, 1.0) for e in range(300)]]
    jvp = _against_restatement(lx, desc, lambda el: [(el[0], "k1"), (el[150], "k1"), (el[299], "length"), "energy"], entries, B=B)
    assert jvp.trace.num_points == 301


def test_a_direction_that_changes_no_map_gives_exact_zeros(lx):
    """`tilt` of a drift-like quadrupole (k1 = 0, untilted): no map depends on it, and every tangent is an exact zero -- next
    to a direction that is not."""
    one = lambda v: np.array([v])  # noqa: E731
    q0 = lx.Quadrupole(one(0.2), k1=one(0.0), dtype=np.float64)
    q1 = lx.Quadrupole(one(0.2), k1=one(2.0), dtype=np.float64)
    d = lx.Drift(one(0.5), dtype=np.float64)
    mu, cov = incoming_moments(2, np.random.default_rng(4))
    beam = lx.ParameterBeam(mu, cov, np.full(2, 1e8), dtype=np.float64)
    jvp = lx.grad.track_along_jvp(lx.Segment([q1, d, q0, d]), beam, [(q0, "tilt"), (q1, "k1")])
    assert not jvp.mu_dot[:, 0].any() and not jvp.cov_dot[:, 0].any()
    assert np.all(jvp.tangent("beta_x")[:, 0] == 0) and np.all(jvp.tangent("sigma_y")[:, 0] == 0)
    assert np.any(jvp.cov_dot[:, 1, 1:] != 0)


# distance max |g - r| / (|r| + 1e-3 max |r|) of the float32 lattice's tangents g from the float64 pass r of
# the same input -- the float64 pass being the one held to the oracle above --, the maximum per sample over a direction's whole
# curve: twice what test_float32_against_the_float64_pass measured on MI355X (the rule of TOL_C5_GRAD) --
#                      beta_x      sigma_x
#     parameters       2.6e-05     1.5e-06
#     particles        5.3e-06     5.8e-07
# A ParameterBeam's float32 trace carries the cancellation of the emittance in its states ("Beam trace"); a
# ParticleBeam's records are float64 sums.
TOL_JVP_F32 = {"parameters": {"beta_x": 5.2e-5, "sigma_x": 3.0e-6}, "particles": {"beta_x": 1.06e-5, "sigma_x": 1.16e-6}}


@pytest.mark.parametrize("beam_type", ["parameters", "particles"])
def test_float32_against_the_float64_pass(lx, beam_type):
    """A 16-element FODO line, B = 2 with k1 scaled 1 and 0.8, `tangent("beta_x")` and `tangent("sigma_x")` along the k1 of the
    first quadrupole and of the ninth element; a ParticleBeam of 2000 particles."""
    B = 2
    specs = o.fodo_segment(4, dtype=np.float32, batch_shape=(B,), k1_scale=np.array([1.0, 0.8], dtype=np.float32))
    sigma = np.array([1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    particles = o.gaussian_particles((B,), 2000, seed=4, dtype=np.float32, sigma=sigma)

    def tangents(dtype):
        cast = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)  # noqa: E731  (the float32 lattice's own numbers)
        elements = [lx.Quadrupole(cast(s["length"]), k1=cast(s["k1"]), dtype=dtype) if s["kind"] == "quadrupole"
                    else lx.Drift(cast(s["length"]), dtype=dtype) for s in specs]
        if beam_type == "particles":
            beam = lx.ParticleBeam(particles.astype(dtype), np.full(B, 1e8, dtype=dtype), dtype=dtype)
        else:
            mu = np.zeros((B, 7), dtype=dtype)
            mu[:, 6] = 1
            cov = np.zeros((B, 7, 7), dtype=dtype)
            cov[:, range(6), range(6)] = (sigma**2).astype(np.float32).astype(dtype)
            beam = lx.ParameterBeam(mu, cov, np.full(B, 1e8, dtype=dtype), dtype=dtype)
        jvp = lx.grad.track_along_jvp(lx.Segment(elements), beam, [(elements[0], "k1"), (elements[8], "k1")])
        return {name: jvp.tangent(name) for name in ("beta_x", "sigma_x")}

    t32, t64 = tangents(np.float32), tangents(np.float64)
    measured = {}
    for name, r in t64.items():
        g = t32[name]
        assert g.shape == r.shape == (B, 2, 17) and np.all(np.isfinite(g)), name
        measured[name] = max(ref.distance(g[:, d], r[:, d]) for d in range(2))
    print(f"float32 track_along_jvp against float64, {beam_type}: " + ", ".join(f"{k} {v:.1e}" for k, v in measured.items()))
    for name, value in measured.items():
        assert TOL_JVP_F32[beam_type][name] is not None and value <= TOL_JVP_F32[beam_type][name], (name, value)


# ---- the C entry points: what they refuse, where they write ------------------------------------------------------------------

MOMENTS, PARTICLES = "lynx_track_moments_along_forward", "lynx_track_particles_along_forward"
_envs = {}


def env_of(shape, dtype):
    key = (shape, np.dtype(dtype))
    if key not in _envs:
        _envs[key] = ec.make_env(shape, dtype)
    return _envs[key]


@pytest.fixture(scope="module", autouse=True)
def _library(built_library):
    yield
    _envs.clear()
    _case.clear()


# the marked lattice (inactive aperture, drift, marker, quadrupole, marker): the drift's length; the quadrupole's k1 twice on its
# leaf and its length; the energy at every leaf (three of them kinds without parameters); a direction without entries
DIRECTIONS = dict(start=[0, 1, 4, 9, 9], leaf=[1, 3, 3, 3, 0, 1, 2, 3, 4], row=[0, 1, 0, 1, 8, 8, 8, 8, 8],
                  weight=[1.0, 0.5, 2.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0])


def _call(env, entry, pointer, directions=DIRECTIONS, **change):
    rt, s = env.rt, env.shape
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    d = dict(start=ints(directions["start"]), leaf=ints(directions["leaf"]), row=ints(directions["row"]),
             weight=(C.c_double * max(len(directions["weight"]), 1))(*directions["weight"]),
             count=len(directions["start"]) - 1, entries=len(directions["leaf"]), lat=env.lat.handle,
             e_in=pointer("e_in"), mu_tr=pointer("mu_tr"), cov_tr=pointer("cov_tr"), records=pointer("records"),
             mu_dot=pointer("mu_dot"), cov_dot=pointer("cov_dot"), n=s.N)
    d.update(change)
    tail = (d["start"], d["leaf"], d["row"], d["weight"], d["count"], d["entries"], d["mu_dot"], d["cov_dot"])
    if entry == MOMENTS:
        return rt.lib.lynx_track_moments_along_forward(rt.ctx, d["lat"], d["e_in"], d["mu_tr"], d["cov_tr"], *tail)
    return rt.lib.lynx_track_particles_along_forward(rt.ctx, d["lat"], d["n"], d["e_in"], d["records"], *tail)


def _arrays(env, entry, D=4):
    s, t = env.shape, env.dtype
    states = [ec.Array("mu_tr", t, (s.B, s.P, 7), "in"), ec.Array("cov_tr", t, (s.B, s.P, 49), "in")] if entry == MOMENTS \
        else [ec.Array("records", ec.F64, (s.B, s.P, 36), "in")]
    return [ec.Array("e_in", t, (s.B,), "in"), *states, ec.Array("mu_dot", ec.F64, (s.B, D, s.P, 7), "out"),
            ec.Array("cov_dot", ec.F64, (s.B, D, s.P, 49), "out")]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("entry", [MOMENTS, PARTICLES])
def test_an_entry_point_writes_all_of_its_tangents_and_nothing_else(lx, entry, dtype):
    """The checks of test_gpu_entry_footprint.py (tests/entry_footprint.py) for the two new entries: every array of the call in
    ONE block between guards, the call over a block of 0x00 and of 0xFF; nothing outside d_mu_dot and d_cov_dot changes, every
    byte of the two is written whatever was there, and the bytes are those of the call into blocks of their own."""
    for row in ((1, 1, 1, 1, 1), (3, 65, 5, 3, 3)):
        env = env_of(ec.Shape(*row, "marked"), dtype)
        rt, arrays = env.rt, _arrays(env, entry)
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
                assert _call(env, entry, pointer) == 0, rt.lib.lynx_last_error(rt.ctx).decode()
                after = np.empty(arena.nbytes, dtype=np.uint8)
                rt.check(rt.lib.lynx_buf_d2h(rt.ctx, after.ctypes.data, C.c_void_p(base), after.nbytes))
                fp.nothing_else_written(arena, before, after)
                runs.append(after)
            fp.outputs_identical(arena, runs[0], runs[1])
            own = {a.name: rt.empty(a.shape, a.dtype) for a in arrays if a.role == "out"}
            ordinary = lambda name: C.c_void_p((own[name] if name in own else env.a[name]).ptr) if name in own or name in env.a else None  # noqa: E731
            assert _call(env, entry, ordinary) == 0, rt.lib.lynx_last_error(rt.ctx).decode()
            for name, block in own.items():
                fp.same_as(arena, runs[1], name, block.numpy())
            mu_dot, cov_dot = arena.view(runs[1], "mu_dot"), arena.view(runs[1], "cov_dot")
            assert np.any(mu_dot[:, :3] != 0) and (np.any(cov_dot[:, :3] != 0) or env.shape.N == 1)  # (one particle has no spread)
            assert not cov_dot[:, 3].view(np.uint64).any() and not mu_dot[:, 3].view(np.uint64).any()  # the direction without entries
        finally:
            rt.sync()
            rt.free(base)


@pytest.mark.parametrize("entry", [MOMENTS, PARTICLES])
def test_what_the_entry_points_refuse(lx, entry):
    """LYNX_ERR_INVALID before anything is launched, the message starting "beam trace tangents: "."""
    env = env_of(ec.Shape(3, 65, 5, 3, 3, "marked"), np.float64)
    rt = env.rt
    own = {a.name: rt.empty(a.shape, a.dtype) for a in _arrays(env, entry) if a.role == "out"}
    pointer = lambda name: C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
    assert _call(env, entry, pointer) == 0

    def refused(expect, directions=DIRECTIONS, **change):
        assert _call(env, entry, pointer, directions, **change) == -1, expect
        message = rt.lib.lynx_last_error(rt.ctx).decode()
        assert message.startswith("beam trace tangents: ") and expect in message, (expect, message)

    refused("null argument", mu_dot=None)
    refused("null argument", cov_dot=None)
    refused("null argument", e_in=None)
    refused("null argument", weight=None)
    refused("null argument", **({"mu_tr": None} if entry == MOMENTS else {"records": None}))
    refused("n_directions must be > 0", count=0)
    refused("leaf 5 out of range", dict(DIRECTIONS, leaf=[1, 3, 3, 3, 0, 1, 2, 3, 5]))
    refused("leaf -1 out of range", dict(DIRECTIONS, leaf=[-1, 3, 3, 3, 0, 1, 2, 3, 4]))
    refused("row 9 out of range", dict(DIRECTIONS, row=[9, 1, 0, 1, 8, 8, 8, 8, 8]))
    refused("has no parameter row 1", dict(DIRECTIONS, row=[1, 1, 0, 1, 8, 8, 8, 8, 8]))  # a drift has its length alone
    refused("has no parameter row 0", dict(DIRECTIONS, leaf=[2, 3, 3, 3, 0, 1, 2, 3, 4]))  # a marker has none
    refused("dir_start", dict(DIRECTIONS, start=[0, 1, 4, 9, 8]))
    refused("dir_start", dict(DIRECTIONS, start=[0, 4, 1, 9, 9]))
    if entry == PARTICLES:
        refused("n_particles must be > 0", n=0)
    cavity = env_of(ec.Shape(3, 65, 5, 3, 3, "cavity"), np.float64)
    assert _call(cavity, entry, pointer, dict(start=[0, 1], leaf=[1], row=[0], weight=[1.0])) == -1
    message = rt.lib.lynx_last_error(rt.ctx).decode()
    assert message.startswith("beam trace tangents: ") and "step 2 is a cavity step" in message, message
