"""
A NumPy restatement of the forward-mode sweep of the beam trace THROUGH cavities (lynx_amd/csrc/lynx_trace_jvp.hpp,
lynx_track_moments_along_forward_cavities), tests only.  Per sample and direction, with E[k] the energy that enters step k and
e_dot[k] its tangent (e_dot[0] = 1 for the direction "energy", 0 otherwise):

    R[k]    = the step's row: its map M (7 x 7) and, for an active cavity, the 8 coefficients c0 .. c7 of its kick
    Rdot    = sum over the direction's entries at element k of weight . dR/d(parameter)  +  e_dot[k] . dR/dE
    mu_dot' = M mu_dot + Mdot mu,   C_dot' = M C_dot M^T + X + X^T,   X = Mdot C M^T
    a gaining cavity, behind it, with z, c the INCOMING state and z_dot, c_dot its tangents, a = -z4 c2 + c3:
      mu_dot'[5]  = z5_dot c0 + z5 c0_dot + c1_dot (cos a - c4) + c1 (-sin a . a_dot - c4_dot)
      mu_dot'[4] += d(c5 z5^2 + c6 z4 z5 + c7 z4^2)
      C_dot'[5][5] = C_dot[5][5];   C_dot'[4][4] = C_dot'[4][5] = C_dot'[5][4] = d(c5 c55^2 + c6 c45 c55 + c7 c44^2)
      e_dot[k+1]  = e_dot[k] + w cos(phi) for a voltage entry, - w V sin(phi) pi/180 for a phase entry
    everywhere else e_dot[k+1] = e_dot[k]

The rows and coefficients are written from cavity.py the way the oracle's `cavity_track` is; dR by CENTRAL DIFFERENCES at a
relative step (`STEP` of tests/trace_jvp_reference.py by default -- `sweep(..., step=2 * STEP)` measures the differencing's own
error).  A direction is a list of entries (leaf, name, component or None, weight) as in tests/trace_jvp_reference.py; the
energy entries a direction needs behind a cavity are NOT listed -- the restatement carries e_dot itself, which is what holds
the package's placement of those entries to account.  This module holds no test and needs no GPU.
"""

import numpy as np

from oracle import lynx_oracle as o

from . import trace_jvp_reference as ref

C0, C1, C2, C3, C4, T566, T556, T555 = range(8)


def is_cavity_step(spec) -> bool:
    return spec["kind"] == "cavity" and not o.is_skippable(spec)


def cavity_flags(spec, energy):
    """(gain, t5xx): the whole-batch predicates of cavity.py:128 and :164 at the spec's own values."""
    energy = np.asarray(energy, dtype=np.float64)
    delta = np.asarray(spec["voltage"], dtype=np.float64) * np.cos(np.deg2rad(np.asarray(spec["phase"], dtype=np.float64)))
    return bool(np.any(energy + delta > 0)), bool(np.any(delta > 0))


def cavity_coefficients(spec, energy, flags):
    """(B, 8) float64: c0 = E beta0 / (E' beta1), c1 = V beta0 / (E' beta1), c2 = beta0 k, c3 = phi, c4 = cos(phi), T566, T556,
    T555 (cavity.py:141-226) -- with the branch predicates `flags` held fixed, so that a moved parameter differentiates the
    formulas and never the branch."""
    f = lambda name: np.asarray(spec[name], dtype=np.float64)  # noqa: E731
    energy = np.asarray(energy, dtype=np.float64)
    length, voltage, phase, frequency, energy = np.broadcast_arrays(f("length"), f("voltage"), f("phase"), f("frequency"), energy)
    gain, t5xx = flags
    me = o.ELECTRON_MASS_EV
    g0 = energy / me
    igamma2 = 1 / g0**2
    beta0 = np.sqrt(1 - igamma2)
    phi = np.deg2rad(phase)
    k = 2 * np.pi * frequency / o.SPEED_OF_LIGHT
    out = np.zeros((*energy.shape, 8))
    out[..., C2], out[..., C3], out[..., C4] = beta0 * k, phi, np.cos(phi)
    out[..., T566] = 1.5 * length * igamma2 / beta0**3
    if not gain:
        return out
    e1 = energy + voltage * np.cos(phi)
    g1 = e1 / me
    beta1 = np.sqrt(1 - 1 / g1**2)
    out[..., C0], out[..., C1] = energy * beta0 / (e1 * beta1), voltage * beta0 / (e1 * beta1)
    if t5xx:
        dgamma = voltage / me
        out[..., T566] = length * (beta0**3 * g0**3 - beta1**3 * g1**3) / (2 * beta0 * beta1**3 * g0 * (g0 - g1) * g1**3)
        out[..., T556] = (beta0 * k * length * dgamma * g0 * (beta1**3 * g1**3 + beta0 * (g0 - g1**3)) * np.sin(phi)
                          / (beta1**3 * g1**3 * (g0 - g1) ** 2))
        out[..., T555] = beta0**2 * k**2 * length * dgamma / 2.0 * (
            dgamma * (2 * g0 * g1**3 * (beta0 * beta1**3 - 1) + g0**2 + 3 * g1**2 - 2) / (beta1**3 * g1**3 * (g0 - g1) ** 3) * np.sin(phi) ** 2
            - (g1 * g0 * (beta1 * beta0 - 1) + 1) / (beta1 * g1 * (g0 - g1) ** 2) * np.cos(phi))
    return out


def row(spec, energy, flags=None):
    """(M (B, 7, 7), c (B, 8)) of one element at the energy that enters it; c is zeros for anything but an active cavity."""
    energy = np.asarray(energy, dtype=np.float64)
    M = o.element_transfer_map(spec, energy, np.float64)
    if flags is None:
        return M, np.zeros((*energy.shape, 8))
    return M, cavity_coefficients(spec, energy, flags)


def tangent_row(spec, energy, name, component, flags, step):
    """d(row)/d(parameter) by central differences at the relative step `step`; name "energy": d(row)/dE."""
    energy = np.asarray(energy, dtype=np.float64)
    if name == "energy":
        h = step * energy
        up, down = row(spec, energy + h, flags), row(spec, energy - h, flags)
    else:
        values = spec[name] if component is None else spec[name][..., component]
        h = step * np.maximum(np.abs(values), 1e-2)
        with ref.moved(spec, name, component, h):
            up = row(spec, energy, flags)
        with ref.moved(spec, name, component, -h):
            down = row(spec, energy, flags)
    return (up[0] - down[0]) / (2 * h)[..., None, None], (up[1] - down[1]) / (2 * h)[..., None]


def sweep(specs, energy, mu0, cov0, direction, step=ref.STEP):
    """The recursion of the module's head -> (mu (B, P, 7), cov (B, P, 7, 7), E (B, P), mu_dot, cov_dot, e_dot (B, P))."""
    E = np.asarray(energy, dtype=np.float64).copy()
    mu, cov, energies = [np.asarray(mu0, dtype=np.float64)], [np.asarray(cov0, dtype=np.float64)], [E]
    mu_dot, cov_dot = [np.zeros_like(mu[0])], [np.zeros_like(cov[0])]
    e_dot = np.full(E.shape, 1.0 if any(name == "energy" for _, name, _, _ in direction) else 0.0)
    e_dots = [e_dot]
    T = lambda a: np.swapaxes(a, -1, -2)  # noqa: E731
    for k, spec in enumerate(specs):
        flags = cavity_flags(spec, E) if is_cavity_step(spec) else None
        M, c = row(spec, E, flags)
        z, C, zd, Cd = mu[-1], cov[-1], mu_dot[-1], cov_dot[-1]
        here = [entry for entry in direction if entry[0] == k and entry[1] != "energy"]
        Mdot, cdot = np.zeros_like(M), np.zeros_like(c)
        for _, name, component, weight in here:
            dM, dc = tangent_row(spec, E, name, component, flags, step)
            Mdot, cdot = Mdot + weight * dM, cdot + weight * dc
        if np.any(e_dot != 0):
            dM, dc = tangent_row(spec, E, "energy", None, flags, step)
            Mdot, cdot = Mdot + e_dot[:, None, None] * dM, cdot + e_dot[:, None] * dc
        md = np.einsum("bij,bj->bi", M, zd) + np.einsum("bij,bj->bi", Mdot, z)
        X = Mdot @ C @ T(M)
        cd = M @ Cd @ T(M) + X + T(X)
        z1, C1_ = np.einsum("bij,bj->bi", M, z), M @ C @ T(M)
        if flags is not None and flags[0]:  # a gaining cavity: the branch behind the linear step, on the INCOMING state
            a = -z[:, 4] * c[:, C2] + c[:, C3]
            a_dot = -zd[:, 4] * c[:, C2] - z[:, 4] * cdot[:, C2] + cdot[:, C3]
            z1[:, 5] = z[:, 5] * c[:, C0] + c[:, C1] * (np.cos(a) - c[:, C4])
            md[:, 5] = zd[:, 5] * c[:, C0] + z[:, 5] * cdot[:, C0] + cdot[:, C1] * (np.cos(a) - c[:, C4]) \
                + c[:, C1] * (-np.sin(a) * a_dot - cdot[:, C4])
            z1[:, 4] += c[:, T566] * z[:, 5] ** 2 + c[:, T556] * z[:, 4] * z[:, 5] + c[:, T555] * z[:, 4] ** 2
            md[:, 4] += cdot[:, T566] * z[:, 5] ** 2 + 2 * c[:, T566] * z[:, 5] * zd[:, 5] + cdot[:, T556] * z[:, 4] * z[:, 5] \
                + c[:, T556] * (zd[:, 4] * z[:, 5] + z[:, 4] * zd[:, 5]) + cdot[:, T555] * z[:, 4] ** 2 + 2 * c[:, T555] * z[:, 4] * zd[:, 4]
            c44, c45, c55, d44, d45, d55 = C[:, 4, 4], C[:, 4, 5], C[:, 5, 5], Cd[:, 4, 4], Cd[:, 4, 5], Cd[:, 5, 5]
            v = c[:, T566] * c55**2 + c[:, T556] * c45 * c55 + c[:, T555] * c44**2
            vd = cdot[:, T566] * c55**2 + 2 * c[:, T566] * c55 * d55 + cdot[:, T556] * c45 * c55 \
                + c[:, T556] * (d45 * c55 + c45 * d55) + cdot[:, T555] * c44**2 + 2 * c[:, T555] * c44 * d44
            C1_[:, 5, 5], cd[:, 5, 5] = c55, d55
            C1_[:, 4, 4] = C1_[:, 4, 5] = C1_[:, 5, 4] = v
            cd[:, 4, 4] = cd[:, 4, 5] = cd[:, 5, 4] = vd
            phi = c[:, C3]
            voltage = np.broadcast_to(np.asarray(spec["voltage"], dtype=np.float64), E.shape)
            for _, name, _, weight in here:
                if name == "voltage":
                    e_dot = e_dot + weight * np.cos(phi)
                elif name == "phase":
                    e_dot = e_dot - weight * voltage * np.sin(phi) * np.pi / 180
            E = E + voltage * np.cos(phi)
        mu.append(z1)
        cov.append(C1_)
        mu_dot.append(md)
        cov_dot.append(cd)
        energies.append(E)
        e_dots.append(e_dot)
    return tuple(np.stack(a, axis=1) for a in (mu, cov, energies, mu_dot, cov_dot, e_dots))


def energy_moments(beams):
    """For `ref.chain_tangents`: the energies of a chain of oracle beams in the place of the means, (B, P, 1)."""
    return np.stack([np.broadcast_to(b["energy"], beams[0]["energy"].shape) for b in beams], axis=1)[..., None], \
        np.stack([b["cov"] for b in beams], axis=1)
