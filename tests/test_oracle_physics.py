"""
A second anchor for the oracle, independent of the reference's code: textbook linear optics.

SURVEY.md section 8c: the reference's own tests hold no absolute numbers for dipoles, correctors, tilts,
misalignments or the cavity matrix ("parity unpinned" rows A1, A2, A6, A7, A9).  The oracle follows the
reference line by line; these tests check the same maps against closed forms every accelerator-optics text
derives (sector bend, thick quadrupole, thin edge wedge, Rosenzweig-Serafini cavity), so that a misreading of
the reference would have to coincide with a physics error to go unnoticed.  float64, CPU only.  At the end: the two
forms of the cavity kick's difference of cosines the oracle can compute (float32 and float64).
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

ENERGY = np.array([1.0e9, 6.0e6])  # ultra-relativistic and gamma ~ 12


def _gamma_beta(energy):
    gamma = energy / o.REST_ENERGY
    return gamma, np.sqrt(1.0 - 1.0 / gamma**2)


def _f(v):
    return np.full(ENERGY.shape, v, dtype=np.float64)


def test_drift_is_the_free_space_map():
    L = 1.7
    T = o.element_transfer_map(o.Drift(_f(L)), ENERGY, np.float64)
    gamma, beta = _gamma_beta(ENERGY)
    expect = np.tile(np.eye(7), (2, 1, 1))
    expect[:, 0, 1] = expect[:, 2, 3] = L
    expect[:, 4, 5] = -L / (beta**2 * gamma**2)  # path length vs. momentum: velocity term only
    assert np.allclose(T, expect, rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("k1", [4.2, -4.2])
def test_thick_quadrupole_closed_form(k1):
    L = 0.3
    T = o.element_transfer_map(o.Quadrupole(_f(L), k1=_f(k1)), ENERGY, np.float64)
    w = np.sqrt(abs(k1))
    foc = np.array([[np.cos(w * L), np.sin(w * L) / w], [-w * np.sin(w * L), np.cos(w * L)]])
    defoc = np.array([[np.cosh(w * L), np.sinh(w * L) / w], [w * np.sinh(w * L), np.cosh(w * L)]])
    xb, yb = (foc, defoc) if k1 > 0 else (defoc, foc)
    for b in range(2):
        assert np.allclose(T[b, :2, :2], xb, rtol=1e-12)
        assert np.allclose(T[b, 2:4, 2:4], yb, rtol=1e-12)
        assert np.isclose(np.linalg.det(T[b, :2, :2]), 1.0, rtol=1e-12)
        assert np.isclose(np.linalg.det(T[b, 2:4, 2:4]), 1.0, rtol=1e-12)
        assert np.allclose(T[b, :4, 4:6], 0.0) and np.allclose(T[b, :4, 6], 0.0)  # no dispersion, no kick


def test_sector_bend_closed_form():
    L, angle = 0.8, 0.25
    rho = L / angle
    T = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle)), ENERGY, np.float64)
    _, beta = _gamma_beta(ENERGY)
    c, s = np.cos(angle), np.sin(angle)
    for b in range(2):
        assert np.allclose(T[b, :2, :2], [[c, rho * s], [-s / rho, c]], rtol=1e-12)
        # a drift vertically -- up to the reference's k1 = 0 -> 1e-12 substitution (track_methods.py:67-68)
        assert np.allclose(T[b, 2:4, 2:4], [[1.0, L], [0.0, 1.0]], rtol=1e-12, atol=2e-12)
        # dispersion of a sector magnet: D = rho (1 - cos), D' = sin, per unit delta = dp/p / beta convention
        assert np.isclose(T[b, 0, 5], rho * (1 - c) / beta[b], rtol=1e-12)
        assert np.isclose(T[b, 1, 5], s / beta[b], rtol=1e-12)
        # symplectic partner terms of the path length
        assert np.isclose(T[b, 4, 0], s / beta[b], rtol=1e-12)
        assert np.isclose(T[b, 4, 1], rho * (1 - c) / beta[b], rtol=1e-12)


def test_dipole_edges_are_thin_wedges():
    L, angle, e1, e2 = 0.8, 0.25, 0.11, -0.07
    h = angle / L
    body = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle)), ENERGY, np.float64)
    full = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle), e1=_f(e1), e2=_f(e2)), ENERGY, np.float64)

    def wedge(e):  # horizontally defocusing by h tan e, vertically focusing by the same (no fringe integral)
        W = np.eye(7)
        W[1, 0] = h * np.tan(e)
        W[3, 2] = -h * np.tan(e)
        return W

    for b in range(2):
        assert np.allclose(full[b], wedge(e2) @ body[b] @ wedge(e1), rtol=1e-12, atol=1e-15)
        assert np.isclose(np.linalg.det(full[b, :2, :2]), 1.0, rtol=1e-12)
        assert np.isclose(np.linalg.det(full[b, 2:4, 2:4]), 1.0, rtol=1e-12)


def test_fringe_field_reduces_the_vertical_edge_angle():
    L, angle, e1, fint, gap = 0.8, 0.25, 0.11, 0.45, 0.03
    h = angle / L
    T0 = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle), e1=_f(e1)), ENERGY, np.float64)
    T1 = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle), e1=_f(e1), fringe_integral=_f(fint),
                                         fringe_integral_exit=_f(0.0), gap=_f(gap)), ENERGY, np.float64)
    # SLAC-75 / MAD: psi = K g h (1 + sin^2 e) / cos e ; vertical kick -h tan(e - psi); horizontal unchanged
    psi = fint * gap * h * (1 + np.sin(e1) ** 2) / np.cos(e1)
    W0, W1 = np.eye(7), np.eye(7)
    W0[1, 0] = W1[1, 0] = h * np.tan(e1)
    W0[3, 2] = -h * np.tan(e1)
    W1[3, 2] = -h * np.tan(e1 - psi)
    for b in range(2):
        assert np.allclose(T1[b], T0[b] @ np.linalg.inv(W0) @ W1, rtol=1e-11, atol=1e-14)


def test_rbend_is_a_sector_bend_with_half_angle_wedges():
    L, angle = 0.8, 0.25
    r = o.element_transfer_map(o.RBend(_f(L), angle=_f(angle)), ENERGY, np.float64)
    s = o.element_transfer_map(o.Dipole(_f(L), angle=_f(angle), e1=_f(angle / 2), e2=_f(angle / 2)), ENERGY, np.float64)
    assert np.array_equal(r, s)
    # the textbook property of a rectangular magnet: no horizontal focusing at all
    rho = L / angle
    for b in range(2):
        assert np.allclose(r[b, :2, :2], [[1.0, rho * np.sin(angle)], [0.0, 1.0]], rtol=1e-12, atol=5e-12)  # cancellation


def test_correctors_are_drifts_with_a_kick():
    L, angle = 0.1, 3e-4
    d = o.element_transfer_map(o.Drift(_f(L)), ENERGY, np.float64)
    h = o.element_transfer_map(o.HorizontalCorrector(_f(L), angle=_f(angle)), ENERGY, np.float64)
    v = o.element_transfer_map(o.VerticalCorrector(_f(L), angle=_f(angle)), ENERGY, np.float64)
    eh, ev = d.copy(), d.copy()
    eh[:, 1, 6] = angle
    ev[:, 3, 6] = angle
    assert np.array_equal(h, eh) and np.array_equal(v, ev)


def test_tilt_is_a_rotation_of_the_transverse_plane():
    L, k1, tilt = 0.3, 4.2, 0.3
    plain = o.element_transfer_map(o.Quadrupole(_f(L), k1=_f(k1)), ENERGY, np.float64)
    tilted = o.element_transfer_map(o.Quadrupole(_f(L), k1=_f(k1), tilt=_f(tilt)), ENERGY, np.float64)
    c, s = np.cos(tilt), np.sin(tilt)
    R = np.eye(7)  # (x, y) -> (x cos + y sin, -x sin + y cos), same for the slopes
    R[0, 0] = R[1, 1] = R[2, 2] = R[3, 3] = c
    R[0, 2] = R[1, 3] = s
    R[2, 0] = R[3, 1] = -s
    for b in range(2):
        assert np.allclose(tilted[b], R.T @ plain[b] @ R, rtol=1e-12, atol=1e-15)
    # a quadrupole rolled by 45 degrees is a skew quadrupole: no x-x focusing term of first order in k1 L
    skew = o.element_transfer_map(o.Quadrupole(_f(1e-3), k1=_f(k1), tilt=_f(np.pi / 4)), ENERGY, np.float64)
    assert np.all(np.abs(skew[:, 1, 0]) < 1e-8) and np.allclose(skew[:, 1, 2], -k1 * 1e-3, rtol=1e-5)


def test_misalignment_shifts_the_axis():
    L, k1 = 0.3, 4.2
    dx, dy = 2e-4, -1e-4
    mis = np.tile(np.array([dx, dy]), (2, 1))
    T = o.element_transfer_map(o.Quadrupole(_f(L), k1=_f(k1), misalignment=mis), ENERGY, np.float64)
    plain = o.element_transfer_map(o.Quadrupole(_f(L), k1=_f(k1)), ENERGY, np.float64)
    # a particle on the magnet's own axis, parallel to it, stays there
    z = np.array([dx, 0.0, dy, 0.0, 0.0, 0.0, 1.0])
    for b in range(2):
        out = T[b] @ z
        assert np.allclose(out[:4], [dx, 0.0, dy, 0.0], atol=1e-18)
        # and any other particle sees the plain magnet in shifted coordinates
        p = np.array([1e-3, 2e-4, -5e-4, 1e-4, 0.0, 0.0, 1.0])
        shifted = p - np.array([dx, 0, dy, 0, 0, 0, 0])
        assert np.allclose((T[b] @ p)[:4], (plain[b] @ shifted)[:4] + [dx, 0, dy, 0], rtol=1e-12, atol=1e-18)


def test_cavity_matrix_damps_adiabatically():
    """Rosenzweig-Serafini standing-wave cavity: the transverse 2x2 block has determinant E_i / E_f
    (adiabatic damping of the normalised emittance), equal in both planes; on crest the energy gain is V."""
    L, V, f = 1.0377, 2.0e7, 1.3e9
    for phase in (0.0, 12.0, -30.0):
        spec = o.Cavity(_f(L), voltage=_f(V), phase=_f(phase), frequency=_f(f))
        energy = np.array([1.0e8, 6.0e6])
        T = o.element_transfer_map(spec, energy, np.float64)
        e_out = energy + V * np.cos(np.deg2rad(phase))
        for b in range(2):
            assert np.isclose(np.linalg.det(T[b, :2, :2]), energy[b] / e_out[b], rtol=1e-10)
            assert np.array_equal(T[b, :2, :2], T[b, 2:4, 2:4])
            assert np.allclose(T[b, :4, 4:], 0.0) and np.allclose(T[b, 4:6, :4], 0.0)  # s, delta couple only with each other
        beam = o.particle_beam(np.zeros((2, 4, 7)) + np.array([0, 0, 0, 0, 0, 0, 1.0]), energy, np.float64)
        out = o.element_track(spec, beam, np.float64)
        assert np.allclose(out["energy"], e_out, rtol=1e-14)
        # the reference particle (s = 0, delta = 0) stays the reference particle
        assert np.allclose(out["particles"][..., :6], 0.0, atol=1e-18)


def test_cavity_off_crest_chirps_the_bunch():
    """A particle ahead of (behind) the reference sees a different phase: to first order
    delta_out - delta_in E_i/E_f ~ -(V k sin(phi) / E_f) s for a relativistic beam -- sign and size of the chirp."""
    L, V, f, phase = 1.0377, 2.0e7, 1.3e9, -20.0
    energy = np.array([1.0e9])
    spec = o.Cavity(np.array([L]), voltage=np.array([V]), phase=np.array([phase]), frequency=np.array([f]))
    s0 = 1e-5
    P = np.zeros((1, 2, 7))
    P[..., 6] = 1.0
    P[0, 1, 4] = s0
    out = o.element_track(spec, o.particle_beam(P, energy, np.float64), np.float64)
    k = 2 * np.pi * f / 299792458.0
    e_out = energy[0] + V * np.cos(np.deg2rad(phase))
    # cos(-s k + phi) - cos(phi) ~ s k sin(phi): with phi < 0 a particle at s > 0 loses energy relative to the reference
    expect = V * s0 * k * np.sin(np.deg2rad(phase)) / e_out
    got = out["particles"][0, 1, 5] - out["particles"][0, 0, 5]
    assert np.isclose(got, expect, rtol=1e-3), (got, expect)


# ---------------------------------------------------------------------------------------------------------------------
# The two forms of the cavity kick's difference of cosines (oracle: cos_difference, kick="reference" | "product")
# ---------------------------------------------------------------------------------------------------------------------


def test_the_two_forms_of_the_difference_of_cosines_agree_in_float64():
    """cos(phi) (cos d - 1) - sin(phi) sin d is cos(phi + d) - cos(phi): in float64 the forms agree to 1e-12 of the
    difference's size (helpers.rel_err: relative to the largest |difference| of the set -- the difference crosses zero,
    where the reference form's own rounding, 1e-16 absolute, is all there is), down to spreads of 1e-3 rad.  (Below that
    the reference form's rounding alone is 1e-12 of the difference.)"""
    from .helpers import rel_err

    rng = np.random.default_rng(11)
    for spread in (0.3, 1e-2, 1e-3):  # (C5: s beta0 k ~ 3e-4 for sigma_s = 1e-5)
        d = np.concatenate([rng.uniform(-spread, spread, 2000), [0.0, spread, -spread]])
        phi = np.deg2rad(rng.uniform(-30, 30, d.size))
        a, b = o.cos_difference(d, phi, "product"), o.cos_difference(d, phi, "reference")
        assert a.dtype == np.float64
        assert rel_err(a, b) <= 1e-12, (spread, rel_err(a, b))
    d = np.array([0.0, 0.25, -0.25, 0.2500001, 0.3, -1.0])
    phi = np.deg2rad(np.array([3.0, -7.0, 10.0, 0.5, -2.0, 1.0]))
    a, b = o.cos_difference(d, phi, "product"), o.cos_difference(d, phi, "reference")
    # above |d| = 0.25 the product subtracts the two cosines itself: the same bits
    big = np.abs(d) > o.COS_DIFFERENCE_SMALL
    assert big.any() and np.array_equal(a[big], b[big])


def _c5_like(B=16, N=10_000, sigma_s=1e-5):
    """Eight cells of [Drift, misaligned Quadrupole, Drift, Cavity] at 6 MeV, 1.3 GHz: BASELINE config 5's shape."""
    from .helpers import make_lattice

    rng = np.random.default_rng(3)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for _ in range(8):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                                 frequency=f(1.3e9)))]
    _, s32 = make_lattice(desc, np.float32)
    _, s64 = make_lattice([(k, {a: np.asarray(v, dtype=np.float32).astype(np.float64) for a, v in kw.items()})
                           for k, kw in desc], np.float64)
    P = o.gaussian_particles((B,), N, seed=3, dtype=np.float32, sigma=[1e-4, 1e-5, 1e-4, 1e-5, sigma_s, 1e-3])
    e = np.full(B, 6e6, dtype=np.float32)
    return s32, s64, P, e


@pytest.mark.parametrize("sigma_s", [1e-5, 1e-4])
def test_float32_product_kick_sits_on_the_float64_chain_and_the_reference_kick_does_not(sigma_s):
    """
    On a C5-like beam the float32 chain with the kernels' form of the kick is within 1e-6 of the float64 chain in mu_s,
    mu_p and sigma_p (measured: 4e-9 .. 9e-8, 2e-7 .. 7e-7), the moments the kick decides.  sigma_s is set by the
    float32 cavity MAP, not by the kick: it is the same under both forms (3e-6 from float64, measured).  The float32
    chain with the reference's form -- two cosines that agree to four or five digits, subtracted -- is 2e-4 away in
    mu_p: why a float32 rule built on it cannot be strict, and why the oracle computes the product's form.
    """
    from .helpers import moment_distances

    s32, s64, P, e = _c5_like(sigma_s=sigma_s)
    prod = o.segment_track(s32, o.particle_beam(P, e, np.float32), np.float32, kick="product")
    ref = o.segment_track(s32, o.particle_beam(P, e, np.float32), np.float32, kick="reference")
    r64 = o.segment_track(s64, o.particle_beam(P.astype(np.float64), e.astype(np.float64), np.float64), np.float64)
    m64 = o.beam_moments(r64)
    dp = moment_distances(o.beam_moments(prod), m64)
    dr = moment_distances(o.beam_moments(ref), m64)
    for key in ("mu_s", "mu_p", "sigma_p"):
        assert dp[key] <= 1e-6, (key, dp[key])
    assert dp["sigma_s"] <= 5e-6 and abs(dp["sigma_s"] - dr["sigma_s"]) <= 1e-7, (dp["sigma_s"], dr["sigma_s"])
    assert dr["mu_p"] >= 1e-4 > 100 * dp["mu_p"], (dr["mu_p"], dp["mu_p"])
    # only delta and s are touched by the form: the transverse coordinates are the same bits
    assert np.array_equal(prod["particles"][..., :4], ref["particles"][..., :4])
    assert np.array_equal(prod["energy"], ref["energy"])


def test_the_product_kick_form_covers_the_parameter_beam_and_leaves_float64_alone():
    s32, s64, _, e = _c5_like(B=4)
    pb32 = o.parameter_beam_from_parameters(np.float32, sigma_x=np.full(4, 1e-4), sigma_xp=np.full(4, 1e-5),
                                            mu_x=np.full(4, 1e-4), sigma_s=np.full(4, 1e-5), sigma_p=np.full(4, 1e-3),
                                            energy=np.full(4, 6e6))
    pb32["mu"][..., 4] = np.float32(2e-5)  # a bunch off the crest's reference point: the kick sees mu_s
    prod = o.segment_track(s32, pb32, np.float32, kick="product")
    ref = o.segment_track(s32, pb32, np.float32, kick="reference")
    pb64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in pb32.items()}
    r64 = o.segment_track(s64, pb64, np.float64)
    scale = np.abs(r64["mu"][..., 5]) + np.sqrt(r64["cov"][..., 5, 5])
    d_prod = np.max(np.abs(prod["mu"][..., 5] - r64["mu"][..., 5]) / scale)
    d_ref = np.max(np.abs(ref["mu"][..., 5] - r64["mu"][..., 5]) / scale)
    assert d_prod <= 1e-6 and d_ref > 10 * d_prod, (d_prod, d_ref)
    assert np.array_equal(prod["cov"], ref["cov"]) and np.array_equal(prod["mu"][..., :4], ref["mu"][..., :4])
    q64 = o.segment_track(s64, pb64, np.float64, kick="product")
    assert np.array_equal(q64["mu"], r64["mu"]) and np.array_equal(q64["cov"], r64["cov"])
    with pytest.raises(AssertionError):
        o.segment_track(s32, pb32, np.float32, kick="fast")
