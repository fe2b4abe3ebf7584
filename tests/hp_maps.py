"""
High-precision restatement of the per-element maps (lynx_amd/csrc/lynx_maps.hpp, oracle/lynx_oracle.py) in mpmath, as a
reference for the dual-number derivatives of the map builders (lynx_amd/csrc/lynx_dual.hpp).  CPU tests only.

The parameter rows and flags are the kernels' (`build_element`): drift [L], correctors [L, angle], quadrupole [L, k1,
tilt, mx, my], dipole [L, angle, e1, e2, tilt, fint, fintx, gap] (an RBend is a dipole whose e1, e2 carry angle/2, which
`rbend_map` adds), cavity [L, V, phase_deg, f], solenoid [L, k, mx, my], undulator [L].

The functions of k2 in base_rmatrix (track_methods.py:72-81) -- C = cos(sqrt(k2) L), S = sin(sqrt(k2) L)/sqrt(k2),
(1 - C)/k2 and (L - S)/k2 -- are written as the entire functions of k2 they are, so that k2 = 0 is a regular point: the
derivative at a quadrupole's k1 = 0 is the limit.  The reference's `k1 == 0 -> 1e-12` stays for dipoles, which never
carry k1.  Derivatives are `mp.diff` of these maps.
"""

from __future__ import annotations

import mpmath as mp

DPS = 50
REST_ENERGY = mp.mpf("510998.9506917531")  # lynx_maps.hpp: LYNX_REST_ENERGY
ELECTRON_MASS_EV = mp.mpf("510998.95069")  # LYNX_ELECTRON_MASS_EV
SPEED_OF_LIGHT = mp.mpf(299792458)

KIND_DRIFT, KIND_QUADRUPOLE, KIND_DIPOLE, KIND_HCOR, KIND_VCOR, KIND_CAVITY = 1, 2, 3, 4, 5, 6
KIND_SOLENOID, KIND_UNDULATOR = 11, 12
FLAG_TILT, FLAG_MISALIGNED, FLAG_THICK = 1, 2, 4
FLAG_CAV_BETA, FLAG_CAV_GAIN, FLAG_CAV_T5XX = 8, 16, 32


def _series(x, j):
    """sum_{m >= 0} (-x)^m / (2m + j)!, to the working precision (|x| < 1)."""
    total, term, m = mp.mpf(0), 1 / mp.factorial(j), 0
    eps = mp.mpf(10) ** (-mp.mp.dps - 5)
    while abs(term) > eps * abs(total) or m == 0:
        total += term
        m += 1
        term = term * (-x) / ((2 * m + j - 1) * (2 * m + j))
    return total


def cs(k2, L):
    """C, S, (1 - C)/k2, (L - S)/k2 as entire functions of k2."""
    x = k2 * L * L
    if abs(x) < 1:
        return _series(x, 0), L * _series(x, 1), L**2 * _series(x, 2), L**3 * _series(x, 3)
    if k2 > 0:
        a = mp.sqrt(k2)
        c, s = mp.cos(a * L), mp.sin(a * L) / a
    else:
        a = mp.sqrt(-k2)
        c, s = mp.cosh(a * L), mp.sinh(a * L) / a
    return c, s, (1 - c) / k2, (L - s) / k2


def eye():
    return mp.eye(7)


def _gamma_terms(energy, ones_at_zero):
    gamma = energy / REST_ENERGY
    igamma2 = (mp.mpf(1) if ones_at_zero else mp.mpf(0)) if gamma == 0 else 1 / gamma**2
    return igamma2, mp.sqrt(1 - igamma2)


def rotation(angle):
    cs_, sn = mp.cos(angle), mp.sin(angle)
    R = eye()
    R[0, 0], R[0, 2], R[1, 1], R[1, 3] = cs_, sn, cs_, sn
    R[2, 0], R[2, 2], R[3, 1], R[3, 3] = -sn, cs_, -sn, cs_
    return R


def misalign(R, mx, my):
    """R_exit . R . R_entry (track_methods.py:108-122)."""
    entry, exit_ = eye(), eye()
    entry[0, 6], entry[2, 6], exit_[0, 6], exit_[2, 6] = -mx, -my, mx, my
    return exit_ * R * entry


def base_rmatrix(L, k1, hx, energy):
    """track_methods.py:37-99 without the tilt; k1 as given (no substitution)."""
    igamma2, beta = _gamma_terms(energy, ones_at_zero=True)
    kx2, ky2 = k1 + hx**2, -k1
    cx, sx, dx_k, r56_k = cs(kx2, L)
    cy, sy, _, _ = cs(ky2, L)
    dx = hx * dx_k
    r56 = hx**2 * r56_k / beta**2 - L / beta**2 * igamma2
    R = eye()
    R[0, 0], R[0, 1], R[0, 5] = cx, sx, dx / beta
    R[1, 0], R[1, 1], R[1, 5] = -kx2 * sx, cx, sx * hx / beta
    R[2, 2], R[2, 3] = cy, sy
    R[3, 2], R[3, 3] = -ky2 * sy, cy
    R[4, 0], R[4, 1], R[4, 5] = sx * hx / beta, dx / beta, r56
    return R


def drift_like(L, energy, with_beta=True):
    igamma2, beta = _gamma_terms(energy, ones_at_zero=False)
    R = eye()
    R[0, 1], R[2, 3] = L, L
    R[4, 5] = -L / beta**2 * igamma2 if with_beta else L * igamma2
    return R


def dipole_edge(hx, e, fint, gap):
    phi = fint * hx * gap / mp.cos(e) * (1 + mp.sin(e) ** 2)
    R = eye()
    R[1, 0] = hx * mp.tan(e)
    R[3, 2] = -hx * mp.tan(e - phi)
    return R


def cavity(p, flags, energy):
    """cavity.py:248-325 and the coefficients of `_track_beam` (:97-246) in the kernels' slot order."""
    L, V, phase, f = p
    me = ELECTRON_MASS_EV
    phi = phase * mp.pi / 180
    cphi, sphi = mp.cos(phi), mp.sin(phi)
    dE = V * cphi
    Ei, Ef = energy / me, (energy + dE) / me
    Ep = (Ef - Ei) / L
    alpha = mp.sqrt(mp.mpf(1) / 8) / cphi * mp.log(Ef / Ei)
    ca, sa = mp.cos(alpha), mp.sin(alpha)
    r11 = ca - mp.sqrt(2) * cphi * sa
    r12 = mp.sqrt(8) * Ei / Ep * cphi * sa
    r21 = -Ep / Ef * (cphi / mp.sqrt(2) + mp.sqrt(mp.mpf(1) / 8) / cphi) * sa
    r22 = Ei / Ef * (ca + mp.sqrt(2) * cphi * sa)
    r56, beta0, beta1, r55 = mp.mpf(0), mp.mpf(1), mp.mpf(1), mp.mpf(0)
    k = 2 * mp.pi * f / SPEED_OF_LIGHT
    if flags & FLAG_CAV_BETA:
        beta0, beta1 = mp.sqrt(1 - 1 / Ei**2), mp.sqrt(1 - 1 / Ef**2)
        r56 = -L / (Ef**2 * Ei * beta1) * (Ef + Ei) / (beta1 + beta0)
        g0, g1 = Ei, Ef
        r55 = k * L * beta0 * V / me * sphi * (g0 * g1 * (beta0 * beta1 - 1) + 1) / (beta1 * g1 * (g0 - g1) ** 2)
    r66 = Ei / Ef * beta0 / beta1
    r65 = k * sphi * V / (Ef * beta1 * me)
    R = eye()
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = r11, r12, r21, r22
    R[2, 2], R[2, 3], R[3, 2], R[3, 3] = r11, r12, r21, r22
    R[4, 4], R[4, 5], R[5, 4], R[5, 5] = 1 + r55, r56, r65, r66

    tb0, tig2, tg0 = mp.mpf(1), mp.mpf(0), mp.mpf("1e10")
    if energy != 0:
        tg0 = energy / me
        tig2 = 1 / tg0**2
        tb0 = mp.sqrt(1 - tig2)
    coef = [mp.mpf(1), mp.mpf(0), mp.mpf(0), phi, cphi, mp.mpf(0), mp.mpf(0), mp.mpf(0)]
    if flags & FLAG_CAV_GAIN:
        T566, T556, T555 = mp.mpf("1.5") * L * tig2 / tb0**3, mp.mpf(0), mp.mpf(0)
        eout = energy + dE
        g1 = eout / me
        tb1 = mp.sqrt(1 - 1 / g1**2)
        dgamma = V / me
        if flags & FLAG_CAV_T5XX:
            b03, b13, g03, g13, dg = tb0**3, tb1**3, tg0**3, g1**3, tg0 - g1
            T566 = L * (b03 * g03 - b13 * g13) / (2 * tb0 * b13 * tg0 * dg * g13)
            T556 = tb0 * k * L * dgamma * tg0 * (b13 * g13 + tb0 * (tg0 - g13)) * sphi / (b13 * g13 * dg**2)
            T555 = tb0**2 * k**2 * L * dgamma / 2 * (
                dgamma * (2 * tg0 * g13 * (tb0 * b13 - 1) + tg0**2 + 3 * g1**2 - 2) / (b13 * g13 * dg**3) * sphi**2
                - (g1 * tg0 * (tb1 * tb0 - 1) + 1) / (tb1 * g1 * dg**2) * cphi)
        coef = [energy * tb0 / (eout * tb1), V * tb0 / (eout * tb1), tb0 * k, phi, cphi, T566, T556, T555]
    return R, coef


def element_map(kind, flags, p, energy):
    """(7x7 mp.matrix, 8 coefficients or None) of one element at mpf parameters `p` and beam energy `energy`."""
    p = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in p]
    energy = energy if isinstance(energy, mp.mpf) else mp.mpf(float(energy))
    if kind == KIND_DRIFT:
        return drift_like(p[0], energy), None
    if kind in (KIND_HCOR, KIND_VCOR):
        R = drift_like(p[0], energy)
        R[1 if kind == KIND_HCOR else 3, 6] = p[1]
        return R, None
    if kind == KIND_UNDULATOR:
        return drift_like(p[0], energy, with_beta=False), None
    if kind == KIND_QUADRUPOLE:
        L, k1, tilt, mx, my = p
        R = base_rmatrix(L, k1, mp.mpf(0), energy)
        if flags & FLAG_TILT:
            R = rotation(-tilt) * R * rotation(tilt)
        if flags & FLAG_MISALIGNED:
            R = misalign(R, mx, my)
        return R, None
    if kind == KIND_DIPOLE:
        L, angle, e1, e2, tilt, fint, fintx, gap = p
        hx = angle / L if flags & FLAG_THICK and L != 0 else mp.mpf(0)  # thin: every length of the batch is 0
        if flags & FLAG_THICK:
            R = base_rmatrix(L, mp.mpf("1e-12"), hx, energy)  # track_methods.py:67-68: a dipole's k1 is always 0
        else:
            R = eye()
            R[0, 1], R[2, 6], R[2, 3] = L, angle, L
        R = dipole_edge(hx, e2, fintx, gap) * R * dipole_edge(hx, e1, fint, gap)
        return rotation(-tilt) * R * rotation(tilt), None
    if kind == KIND_SOLENOID:
        L, k, mx, my = p
        c, s = mp.cos(L * k), mp.sin(L * k)
        s_k = L * _series((k * L) ** 2, 1) if abs(k * L) < 1 else s / k  # sin(kL)/k, entire in k
        gamma = energy / REST_ENERGY
        r56 = mp.mpf(0)
        if gamma != 0:
            r56 = -L / ((1 - 1 / gamma**2) * gamma**2)
        R = eye()
        R[0, 0], R[0, 1], R[0, 2], R[0, 3] = c * c, c * s_k, s * c, s * s_k
        R[1, 0], R[1, 1], R[1, 2], R[1, 3] = -k * s * c, c * c, -k * s * s, s * c
        R[2, 0], R[2, 1], R[2, 2], R[2, 3] = -s * c, -s * s_k, c * c, c * s_k
        R[3, 0], R[3, 1], R[3, 2], R[3, 3] = k * s * s, -s * c, -k * s * c, c * c
        R[4, 5] = r56
        if flags & FLAG_MISALIGNED:
            R = misalign(R, mx, my)
        return R, None
    if kind == KIND_CAVITY:
        return cavity(p, flags, energy)
    raise ValueError(kind)


def _flat(R, coef):
    out = [R[i, j] for i in range(7) for j in range(7)]
    return out + (list(coef) if coef is not None else [])


def values(kind, flags, p, energy, dps=DPS):
    """The 49 map entries (row-major) followed by the 8 coefficients (cavities), as Python floats."""
    with mp.workdps(dps):
        return [float(v) for v in _flat(*element_map(kind, flags, p, energy))]


def derivative(f, x0, dps=DPS):
    """
    d f / dx at x0 for a function `f(x) -> list of mpf`, entry by entry by `mp.diff` (its evaluations of `f` are shared
    between the entries: mp.diff samples every entry at the same points).
    """
    with mp.workdps(dps):
        cache = {}

        def at(x):
            key = mp.nstr(x, mp.mp.dps + 10)
            if key not in cache:
                cache[key] = f(x)
            return cache[key]

        x0 = mp.mpf(x0)
        n = len(at(x0))
        return [float(mp.diff(lambda x, i=i: at(x)[i], x0)) for i in range(n)]


def param_derivative(kind, flags, p, energy, seed, dps=DPS):
    """d(map entries, coefficients)/d p[seed] (seed == len(p): d/d energy) at the given point."""
    p = list(p)

    def f(x):
        q, e = list(p), energy
        if seed < len(p):
            q[seed] = x
        else:
            e = x
        return _flat(*element_map(kind, flags, q, e))

    return derivative(f, p[seed] if seed < len(p) else energy, dps)


def rbend_angle_derivative(flags, p, energy, dps=DPS):
    """d/d angle of an RBend whose dipole row is p (e1, e2 without the angle/2 of rbend.py:79-80)."""
    p = list(p)

    def f(a):
        q = list(p)
        q[1], q[2], q[3] = a, q[2] + a / 2, q[3] + a / 2
        return _flat(*element_map(KIND_DIPOLE, flags, q, energy))

    return derivative(f, p[1], dps)
