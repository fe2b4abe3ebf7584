"""
References for the reverse passes that do not come from the GPU (float64 NumPy and tests/hp_maps.py).

(1) `AffineReference`: analytic reverse mode for lattices without an active cavity.  Every element is an affine map
    T_e (oracle.lynx_oracle.element_transfer_map, float64) at the one beam energy, so with the state z entering every
    element kept,

        particles       L = w_mu . mean + w_cov : (biased cov) of the outgoing beam (+ readings . (mean x, mean y) of the
                        beam entering an active BPM);   z_bar_out = (w_mu + (W + W^T)(z - mean)) / N,
                        T_bar_e = sum_n z_bar_after z_before^T,   z_bar_before = T_e^T z_bar_after
        ParameterBeam   mu' = T mu, C' = T C T^T:   T_bar_e = mu_bar' mu^T + C_bar' T C^T + C_bar'^T T C,
                        mu_bar = T^T mu_bar',  C_bar = T^T C_bar' T  (entry by entry)

    and dL/dtheta = <T_bar_e, dT_e/dtheta>, dL/dE = sum_e <T_bar_e, dT_e/dE> with dT_e/dtheta from
    hp_maps.param_derivative (an RBend's angle through rbend_angle_derivative).  No step size anywhere: every parameter of
    every element, and dL/dz_n of every particle.

(2) `OracleCase.derivatives`: central differences of the float64 oracle for lattices with active cavities.  Every
    differenced quantity is evaluated at two steps, h and h/4, which must agree to 1e-5 of max(|ref|, scale); if they
    do not, the quantity takes the next step of `RELATIVE_STEPS`, and an AssertionError if none of them serves.  That is a
    condition on the reference, not a tolerance on what is compared with it.

(3) The lattices, beams and cotangents of tests/test_gpu_grad_sizes.py, so that tests/test_reverse_reference_host.py can
    hold every one of their references to (2) without a GPU.
"""

from __future__ import annotations

import numpy as np

from oracle import lynx_oracle as o

from . import hp_maps as hp
from .trace_jvp_reference import chain as _chain

KIND = {"drift": hp.KIND_DRIFT, "quadrupole": hp.KIND_QUADRUPOLE, "dipole": hp.KIND_DIPOLE, "rbend": hp.KIND_DIPOLE,
        "hcor": hp.KIND_HCOR, "vcor": hp.KIND_VCOR, "solenoid": hp.KIND_SOLENOID, "undulator": hp.KIND_UNDULATOR}
# the kernels' parameter rows (hp_maps.py): name -> slot(s)
ROW = {"drift": ("length",), "undulator": ("length",), "hcor": ("length", "angle"), "vcor": ("length", "angle"),
       "quadrupole": ("length", "k1", "tilt", "misalignment", None),
       "dipole": ("length", "angle", "e1", "e2", "tilt", "fringe_integral", "fringe_integral_exit", "gap"),
       "solenoid": ("length", "k", "misalignment", None)}
ROW["rbend"] = ROW["dipole"]
DPS = 30  # decimal digits of the map derivatives (the comparison is in float64)

_derivative_cache: dict = {}


def _value(kw, name, b, B):
    v = kw.get(name)
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    return v.reshape(B, -1)[b] if v.ndim else np.array([float(v)])


def element_row(kind, kw, b, B):
    """(hp kind, flags, parameter row) of sample `b` of one described element; the flags are whole-batch predicates."""
    nonzero = lambda name: kw.get(name) is not None and bool(np.any(np.asarray(kw[name]) != 0))  # noqa: E731
    row, flags = [], 0
    names = ROW[kind]
    for slot, name in enumerate(names):
        if name is None:
            continue
        v = _value(kw, name, b, B)
        if name == "misalignment":
            row += [0.0, 0.0] if v is None else [float(v[0]), float(v[1])]
        else:
            row.append(0.0 if v is None else float(v[0]))
    if kind == "quadrupole":
        flags = (hp.FLAG_TILT if nonzero("tilt") else 0) | (hp.FLAG_MISALIGNED if nonzero("misalignment") else 0)
    elif kind == "solenoid":
        flags = hp.FLAG_MISALIGNED if nonzero("misalignment") else 0
    elif kind in ("dipole", "rbend"):
        flags = hp.FLAG_THICK if nonzero("length") else 0
        assert kw.get("fringe_integral_exit") is not None or kw.get("fringe_integral") is None, \
            "give fringe_integral_exit: left out it follows fringe_integral (dipole.py), which the row does not say"
    return KIND[kind], flags, row


def map_derivatives(kind, kw, b, B, energy):
    """{name: (7, 7) or (2, 7, 7)} of every parameter the description gives, and "energy", for sample `b`."""
    hk, flags, row = element_row(kind, kw, b, B)

    def d(seed):
        key = (kind == "rbend" and seed == 1, hk, flags, tuple(row), float(energy), seed)
        if key not in _derivative_cache:
            if key[0]:
                flat = hp.rbend_angle_derivative(flags, row, float(energy), DPS)
            else:
                p = list(row)
                if kind == "rbend":  # rbend.py:79-80
                    p[2], p[3] = p[2] + p[1] / 2, p[3] + p[1] / 2
                flat = hp.param_derivative(hk, flags, p, float(energy), seed, DPS)
            _derivative_cache[key] = np.array(flat[:49]).reshape(7, 7)
        return _derivative_cache[key]

    out, slot = {}, 0
    for name in ROW[kind]:
        if name is None:
            continue
        if name == "misalignment":
            if kw.get(name) is not None:
                out[name] = np.stack([d(slot), d(slot + 1)])
            slot += 2
            continue
        if kw.get(name) is not None:
            out[name] = d(slot)
        slot += 1
    out["energy"] = d(len(row))
    return out


class AffineReference:
    """
    desc: [(kind, kwargs)] with (B,)-shaped float64 parameters ((B, 2) misalignments), no active cavity; energy (B,).
    `gradients` of both beam classes: {(e, name): (B,) or (B, 2), "energy": (B,), ...}.
    """

    def __init__(self, desc, energy, single=False):
        """`single`: maps and their derivatives rounded through `f32` (and a ParameterBeam's states of the along forms at
        every point) -- what rounding its inputs to float32 does to a result, for the conditioning of a drawn float32 case."""
        from .helpers import make_lattice

        self.q = f32 if single else (lambda a: a)
        self.desc = desc
        self.energy = np.asarray(energy, dtype=np.float64)
        self.B = len(self.energy)
        _, self.specs = make_lattice(desc, np.float64)
        assert all(o.is_skippable(s) or s["kind"] == "bpm" for s in self.specs), "an active cavity: not an affine lattice"
        self.maps = [self.q(o.element_transfer_map(s, self.energy, np.float64)) for s in self.specs]
        self.active_bpms = [e for e, s in enumerate(self.specs) if s["kind"] == "bpm" and s.get("is_active")]
        self._dmaps = None

    def dmaps(self):
        if self._dmaps is None:
            self._dmaps = []
            for kind, kw in self.desc:
                if kind not in KIND:
                    self._dmaps.append(None)
                    continue
                per = [map_derivatives(kind, kw, b, self.B, self.energy[b]) for b in range(self.B)]
                self._dmaps.append({name: self.q(np.stack([p[name] for p in per])) for name in per[0]})
        return self._dmaps

    def _contract(self, tbars):
        out = {"energy": np.zeros(self.B)}
        for e, dm in enumerate(self.dmaps()):
            if dm is None:
                continue
            for name, D in dm.items():
                if name == "energy":
                    out["energy"] += np.einsum("bij,bij->b", tbars[e], D)
                elif D.ndim == 4:
                    out[(e, name)] = np.einsum("bij,bkij->bk", tbars[e], D)
                else:
                    out[(e, name)] = np.einsum("bij,bij->b", tbars[e], D)
        return out

    def _reading(self, readings, e):
        """(B, 2) weights of (mean x, mean y) of the beam entering element e; `readings`: (2, B) per active BPM, in lattice order."""
        if not readings or e not in self.active_bpms:
            return None
        return np.asarray(readings[self.active_bpms.index(e)], dtype=np.float64).reshape(2, self.B).T

    def particle_gradients(self, P, w_mu, w_cov, readings=None):
        """P (B, N, 7), w_mu (B, 6), w_cov (B, 6, 6); adds "particles": (B, N, 7)."""
        z = np.asarray(P, dtype=np.float64)
        N = z.shape[1]
        states = []
        for T in self.maps:
            states.append(z)
            z = z @ np.swapaxes(T, -1, -2)
        d = z[..., :6] - z[..., :6].mean(axis=1, keepdims=True)
        W = np.asarray(w_cov, dtype=np.float64)
        zbar = np.zeros_like(z)
        zbar[..., :6] = (np.asarray(w_mu, dtype=np.float64)[:, None, :] + d @ np.swapaxes(W + np.swapaxes(W, -1, -2), -1, -2)) / N
        tbars = [None] * len(self.maps)
        for e in range(len(self.maps) - 1, -1, -1):
            tbars[e] = np.einsum("bni,bnj->bij", zbar, states[e])
            zbar = zbar @ self.maps[e]
            r = self._reading(readings, e)
            if r is not None:
                zbar[..., 0] += r[:, None, 0] / N
                zbar[..., 2] += r[:, None, 1] / N
        out = self._contract(tbars)
        out["particles"] = zbar
        return out

    def parameter_gradients(self, mu, cov, w_mu, w_cov, readings=None):
        """mu (B, 7), cov (B, 7, 7), w_mu (B, 7), w_cov (B, 7, 7) entry by entry; adds "mu": (B, 7) and "cov": (B, 7, 7)."""
        m, C = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        states = []
        for T in self.maps:
            states.append((m, C))
            m, C = np.einsum("bij,bj->bi", T, m), T @ C @ np.swapaxes(T, -1, -2)
        mbar, Cbar = np.array(w_mu, dtype=np.float64), np.array(w_cov, dtype=np.float64)
        tbars = [None] * len(self.maps)
        for e in range(len(self.maps) - 1, -1, -1):
            T, (m, C) = self.maps[e], states[e]
            tbars[e] = (np.einsum("bi,bj->bij", mbar, m) + Cbar @ T @ np.swapaxes(C, -1, -2)
                        + np.swapaxes(Cbar, -1, -2) @ T @ C)
            mbar = np.einsum("bji,bj->bi", T, mbar)
            Cbar = np.swapaxes(T, -1, -2) @ Cbar @ T
            r = self._reading(readings, e)
            if r is not None:
                mbar[:, 0] += r[:, 0]
                mbar[:, 2] += r[:, 1]
        out = self._contract(tbars)
        out["mu"], out["cov"] = mbar, Cbar
        return out

    # ---- the along forms: a cotangent at EVERY point (P = elements + 1), and forward-mode tangents -------------------------

    def parameter_states(self, mu, cov):
        """([mu at the P points], [cov at the P points]) of the moment recursion (`single`: rounded at every point)."""
        m, C = self.q(np.asarray(mu, dtype=np.float64)), self.q(np.asarray(cov, dtype=np.float64))
        mus, covs = [m], [C]
        for T in self.maps:
            m, C = self.q(np.einsum("bij,bj->bi", T, m)), self.q(T @ C @ np.swapaxes(T, -1, -2))
            mus.append(m)
            covs.append(C)
        return mus, covs

    def particle_states(self, P):
        z = np.asarray(P, dtype=np.float64)
        states = [z]
        for T in self.maps:
            z = z @ np.swapaxes(T, -1, -2)
            states.append(z)
        return states

    def parameter_gradients_along(self, mu, cov, w_mu, w_cov, w_e=None, readings=None):
        """
        `parameter_gradients` with w_mu (B, P, 7), w_cov (B, P, 7, 7) and w_e (B, P) given at every point: the cotangent of
        point k joins the sweep when it passes point k.  The energy at every point is the incoming one, so "energy" takes
        w_e.sum(-1) besides the maps' term.
        """
        w_mu, w_cov = np.asarray(w_mu, dtype=np.float64), np.asarray(w_cov, dtype=np.float64)
        mus, covs = self.parameter_states(mu, cov)
        E = len(self.maps)
        mbar, Cbar = w_mu[:, E].copy(), w_cov[:, E].copy()
        tbars = [None] * E
        for e in range(E - 1, -1, -1):
            T, m, C = self.maps[e], mus[e], covs[e]
            tbars[e] = (np.einsum("bi,bj->bij", mbar, m) + Cbar @ T @ np.swapaxes(C, -1, -2)
                        + np.swapaxes(Cbar, -1, -2) @ T @ C)
            mbar = np.einsum("bji,bj->bi", T, mbar) + w_mu[:, e]
            Cbar = np.swapaxes(T, -1, -2) @ Cbar @ T + w_cov[:, e]
            r = self._reading(readings, e)
            if r is not None:
                mbar[:, 0] += r[:, 0]
                mbar[:, 2] += r[:, 1]
        out = self._contract(tbars)
        if w_e is not None:
            out["energy"] = out["energy"] + np.asarray(w_e, dtype=np.float64).sum(axis=-1)
        out["mu"], out["cov"] = mbar, Cbar
        return out

    def particle_gradients_along(self, P, w_mu, w_cov, w_e=None, readings=None, alive=None, trajectories_bar=None, chosen=None):
        """
        `particle_gradients` with w_mu (B, P, 6), w_cov (B, P, 6, 6), w_e (B, P) at every point.  `alive` (P, B, N) bool: the
        mean and biased covariance of a point are over the particles alive there, and its z_bar goes to those alone, with
        that point's count (an active BPM reads the centroid of the particles alive in front of it).  `trajectories_bar`
        (B, P, K, 7) with `chosen` (K,): row [:, k, j] is added to z_bar of particle chosen[j] at point k, repeats add.
        Adds "particles" (B, N, 7); "mu" (B, 7) and "cov" (B, 7, 7), the moment cotangents carried back to the incoming mean
        and biased covariance (not with `alive`: no single set came in; "cov" is the symmetric part -- the particles fix
        no more); "chosen_particles" (B, K, 7): row j is the cotangent of its own trajectory alone.
        """
        states = self.particle_states(P)
        B, N = states[0].shape[:2]
        E = len(self.maps)
        w_mu, w_cov = np.asarray(w_mu, dtype=np.float64), np.asarray(w_cov, dtype=np.float64)
        a_all = np.ones((E + 1, B, N), dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
        tb = None if trajectories_bar is None else np.asarray(trajectories_bar, dtype=np.float64)

        def injected(k):
            a = a_all[k][..., None].astype(np.float64)
            n = np.maximum(a_all[k].sum(axis=-1), 1)[:, None, None]
            q = states[k][..., :6]
            d = (q - (q * a).sum(axis=1, keepdims=True) / n) * a
            W = w_cov[:, k]
            zb = np.zeros((B, N, 7))
            zb[..., :6] = a * (w_mu[:, k][:, None, :] + d @ np.swapaxes(W + np.swapaxes(W, -1, -2), -1, -2)) / n
            if tb is not None:
                for j, p in enumerate(chosen):
                    zb[:, p] += tb[:, k, j]
            return zb, a[..., 0] / n[..., 0]

        zbar, _ = injected(E)
        tbars = [None] * E
        for e in range(E - 1, -1, -1):
            tbars[e] = np.einsum("bni,bnj->bij", zbar, states[e])
            here, share = injected(e)
            zbar = zbar @ self.maps[e] + here
            r = self._reading(readings, e)
            if r is not None:
                zbar[..., 0] += r[:, None, 0] * share
                zbar[..., 2] += r[:, None, 1] * share
        out = self._contract(tbars)
        if w_e is not None:
            out["energy"] = out["energy"] + np.asarray(w_e, dtype=np.float64).sum(axis=-1)
        out["particles"] = zbar
        if alive is None:
            mbar, Cbar = np.zeros((B, 7)), np.zeros((B, 7, 7))
            for k in range(E, -1, -1):
                if k < E:
                    T = self.maps[k]
                    mbar, Cbar = np.einsum("bji,bj->bi", T, mbar), np.swapaxes(T, -1, -2) @ Cbar @ T
                    r = self._reading(readings, k)
                    if r is not None:
                        mbar[:, 0] += r[:, 0]
                        mbar[:, 2] += r[:, 1]
                mbar[:, :6] += w_mu[:, k]
                Cbar[:, :6, :6] += w_cov[:, k]
            out["mu"], out["cov"] = mbar, (Cbar + np.swapaxes(Cbar, -1, -2)) / 2
        if tb is not None:
            rows = np.zeros((B, len(chosen), 7))
            for k in range(E, -1, -1):
                if k < E:
                    rows = rows @ self.maps[k]
                rows = rows + tb[:, k]
            out["chosen_particles"] = rows
        return out

    def _direction_maps(self, direction):
        """{leaf: Mdot (B, 7, 7)} of a direction [(leaf, name, component or None, weight)]; "energy": dM/dE of that leaf."""
        dmaps, out = self.dmaps(), {}
        for leaf, name, component, weight in direction:
            if dmaps[leaf] is None:
                continue  # (a kind without a row: its map does not depend on anything, the energy included)
            D = dmaps[leaf][name]
            D = D if component is None else D[:, component]
            out[leaf] = out.get(leaf, 0.0) + weight * D
        return out

    def parameter_tangents(self, mu, cov, direction):
        """(mu_dot (B, P, 7), cov_dot (B, P, 7, 7)) of the moment recursion along one direction."""
        mus, covs = self.parameter_states(mu, cov)
        mdots = self._direction_maps(direction)
        md, cd = np.zeros_like(mus[0]), np.zeros_like(covs[0])
        mu_dot, cov_dot = [md], [cd]
        for e, T in enumerate(self.maps):
            md, cd = np.einsum("bij,bj->bi", T, md), T @ cd @ np.swapaxes(T, -1, -2)
            if e in mdots:
                md = md + np.einsum("bij,bj->bi", mdots[e], mus[e])
                X = mdots[e] @ covs[e] @ np.swapaxes(T, -1, -2)
                cd = cd + X + np.swapaxes(X, -1, -2)
            mu_dot.append(md)
            cov_dot.append(cd)
        return np.stack(mu_dot, axis=1), np.stack(cov_dot, axis=1)

    def particle_tangents(self, P, direction):
        """
        ... of the PARTICLES: z_dot' = M z_dot + Mdot z per particle, the tangents of the mean and of the biased covariance
        taken from the particles -- not from the moment recursion, whose closure under affine maps is what the kernels use.
        A particle is carried as mean + deviation, so that z_dot - mean(z_dot) is never formed by a subtraction: along a
        direction that moves every particle alike (a corrector's angle, a misalignment) the covariance's tangent is the
        exact zero it is, not the rounding of N equal numbers' mean.
        """
        states = self.particle_states(P)
        mdots = self._direction_maps(direction)
        B, N = states[0].shape[:2]
        md, dd = np.zeros((B, 7)), np.zeros((B, N, 6))
        mu_dot, cov_dot = [], []
        for k in range(len(self.maps) + 1):
            if k:
                T = self.maps[k - 1]
                md, dd = np.einsum("bij,bj->bi", T, md), dd @ np.swapaxes(T[:, :6, :6], -1, -2)
                if k - 1 in mdots:
                    before = states[k - 1]
                    mean = before.mean(axis=1)
                    md = md + np.einsum("bij,bj->bi", mdots[k - 1], mean)
                    dd = dd + (before - mean[:, None, :])[..., :6] @ np.swapaxes(mdots[k - 1][:, :6, :6], -1, -2)
            d = (states[k] - states[k].mean(axis=1, keepdims=True))[..., :6]
            X = np.zeros((B, 7, 7))
            X[:, :6, :6] = np.einsum("bni,bnj->bij", dd, d) / N
            mu_dot.append(md)
            cov_dot.append(X + np.swapaxes(X, -1, -2))
        return np.stack(mu_dot, axis=1), np.stack(cov_dot, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's losses and their central differences
# ---------------------------------------------------------------------------------------------------------------------

def particle_loss(specs, P, energy, w_mu, w_cov, readings=None):
    """(B,): w_mu . mean + w_cov : biased cov of the tracked particles, + readings (in lattice order) . the BPMs' readings."""
    seen = []
    out = o.segment_track(specs, o.particle_beam(P, energy, np.float64), np.float64, bpm_readings=seen)
    Q = out["particles"][..., :6]
    mu = Q.mean(axis=-2)
    d = Q - mu[..., None, :]
    cov = np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2]
    loss = np.sum(w_mu * mu, axis=-1) + np.sum(w_cov * cov, axis=(-1, -2))
    for w, (_, reading) in zip(readings or [], seen):
        loss = loss + np.sum(np.asarray(w) * reading, axis=0)
    return loss


def parameter_loss(specs, mu, cov, energy, w_mu, w_cov, readings=None):
    """(B,): w_mu . mu + w_cov : cov (7 and 7 x 7, entry by entry) of the tracked ParameterBeam, + the BPMs' readings."""
    seen = []
    out = o.segment_track(specs, o.parameter_beam(mu, cov, energy, np.float64), np.float64, bpm_readings=seen)
    loss = np.sum(w_mu * out["mu"], axis=-1) + np.sum(w_cov * out["cov"], axis=(-1, -2))
    for w, (_, reading) in zip(readings or [], seen):
        loss = loss + np.sum(np.asarray(w) * reading, axis=0)
    return loss


# (the wide ones serve quantities the loss is all but linear in -- a misalignment behind 60 cavities, an entry of the
# incoming covariance -- whose small differences drown in the loss's rounding at a narrow step)
RELATIVE_STEPS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 3e-6, 1e-7)
TWO_STEP_AGREEMENT = 1e-5
# what a relative step refers to where the value itself is small
FLOOR = {"length": 1e-2, "k1": 1e-2, "tilt": 1e-2, "misalignment": 1e-3, "angle": 1e-3, "voltage": 1.0, "phase": 1.0,
         "frequency": 1.0, "e1": 1e-2, "e2": 1e-2, "fringe_integral": 1e-2, "fringe_integral_exit": 1e-2, "gap": 1e-2,
         "k": 1e-2, "particles": 1e-1, "mu": 1e-1, "cov": 1e-6, "direction": 1e1}


def chain_moments(beams):
    """(mu (B, P, k), cov (B, P, k, k), energy (B, P)) of a chain of oracle beams: a ParameterBeam's own (k = 7), the particles'
    mean and biased covariance (k = 6)."""
    mus, covs = [], []
    for b in beams:
        if "particles" in b:
            Q = b["particles"][..., :6]
            mean = Q.mean(axis=-2)
            d = Q - mean[..., None, :]
            mus.append(mean)
            covs.append(np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2])
        else:
            mus.append(b["mu"])
            covs.append(b["cov"])
    return np.stack(mus, axis=1), np.stack(covs, axis=1), np.stack([b["energy"] for b in beams], axis=1)


def _tile(value, K):
    value = np.asarray(value, dtype=np.float64)
    return np.tile(value, (K,) + (1,) * (value.ndim - 1))


class OracleCase:
    """
    One lattice (desc as for helpers.make_lattice, (B,)-shaped float64 parameters), one beam and one pair of cotangents:
    the loss of the float64 oracle and its central differences.  A quantity is named
        (e, name) / (e, name, component)    a parameter of element e
        "energy"                            the incoming energy
        ("particles", n, c)                 coordinate c of incoming particle n;   ("direction",): all particles along `direction`
        ("mu", c), ("cov", r, c)            the incoming ParameterBeam, entry by entry
    `derivatives(quantities, scales)` evaluates every (quantity, +-h, +-h/4) as one more sample of ONE batched oracle call
    per relative step: each quantity takes the first step of RELATIVE_STEPS at which its two differences agree to
    TWO_STEP_AGREEMENT of max(|ref|, scale), and none is an AssertionError.
    """

    def __init__(self, desc, energy, w_mu, w_cov, particles=None, mu=None, cov=None, direction=None, readings=None, w_e=None):
        """`w_mu` (B, P, k), `w_cov` (B, P, k, k) and `w_e` (B, P): the ALONG loss, the sum over the P points of the oracle's
        element-by-element chain of <w_mu, mu> + <w_cov, cov> + w_e (E - E_0), E_0 the unperturbed energy at the point."""
        self.desc, self.energy = desc, np.asarray(energy, dtype=np.float64)
        self.w_e = None if w_e is None else np.asarray(w_e, dtype=np.float64)
        self.B = len(self.energy)
        self.w_mu, self.w_cov = np.asarray(w_mu, dtype=np.float64), np.asarray(w_cov, dtype=np.float64)
        self.particles, self.mu, self.cov, self.direction = particles, mu, cov, direction
        self.readings = readings  # [(2, B)] per active BPM, in lattice order
        self.steps_taken = {}
        self._known = {}

    def _build(self, K):
        from .helpers import make_lattice

        desc = [(kind, {k: (_tile(v, K) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}) for kind, kw in self.desc]
        _, specs = make_lattice(desc, np.float64)
        arrays = {"energy": _tile(self.energy, K)}
        for name in ("particles", "mu", "cov"):
            if getattr(self, name) is not None:
                arrays[name] = _tile(getattr(self, name), K)
        w_mu, w_cov = _tile(self.w_mu, K), _tile(self.w_cov, K)
        readings = None if self.readings is None else [np.tile(np.asarray(r, dtype=np.float64), (1, K)) for r in self.readings]

        def beam():
            if self.particles is not None:
                return o.particle_beam(arrays["particles"], arrays["energy"], np.float64)
            return o.parameter_beam(arrays["mu"], arrays["cov"], arrays["energy"], np.float64)

        if self.w_mu.ndim == 3:
            assert self.readings is None and self.direction is None, "the along loss has neither readings nor a direction"
            w_e, e_0 = _tile(self.w_e, K), _tile(self.energies_along(), K)

            def along():
                mu, cov, energy = chain_moments(_chain(specs, beam()))
                return (np.sum(w_mu * mu, axis=(-1, -2)) + np.sum(w_cov * cov, axis=(-1, -2, -3)) + np.sum(w_e * (energy - e_0), axis=-1))

            return specs, arrays, along

        def loss():
            if self.particles is not None:
                return particle_loss(specs, arrays["particles"], arrays["energy"], w_mu, w_cov, readings)
            return parameter_loss(specs, arrays["mu"], arrays["cov"], arrays["energy"], w_mu, w_cov, readings)

        return specs, arrays, loss

    def loss(self):
        return self._build(1)[2]()

    def energies_along(self):
        """(B, P): the unperturbed energy at every point of the chain."""
        if "energies" not in self._known:
            from .helpers import make_lattice

            _, specs = make_lattice(self.desc, np.float64)
            incoming = (o.particle_beam(self.particles, self.energy, np.float64) if self.particles is not None
                        else o.parameter_beam(self.mu, self.cov, self.energy, np.float64))
            self._known["energies"] = chain_moments(_chain(specs, incoming))[2]
        return self._known["energies"]

    def tangents(self, q, allowance=1.0):
        """
        (mu_dot (B, P, k), cov_dot (B, P, k, k), energy_dot (B, P), and per array the quotient's own rounding (B,)): central
        differences of the chain's moments at every point along quantity q, at the first step of RELATIVE_STEPS whose two
        quotients (h and h / 4) agree to TWO_STEP_AGREEMENT of each array's largest entry, per sample.  The rounding is
        `allowance` x 8 eps max |value| / h (tests/trace_jvp_reference.py, ROUNDING), with h / 4: the narrower step's, the larger.
        """
        B, tried = self.B, []
        eps = 8 * np.finfo(np.float64).eps * allowance
        for rel in RELATIVE_STEPS:
            specs, arrays, _ = self._build(4)
            array, index, _, magnitude = self._target(specs, arrays, q)
            h = rel * magnitude
            for v, d in enumerate((h, -h, h / 4, -h / 4)):
                array[(slice(v * B, (v + 1) * B), *index)] += d
            incoming = (o.particle_beam(arrays["particles"], arrays["energy"], np.float64) if self.particles is not None
                        else o.parameter_beam(arrays["mu"], arrays["cov"], arrays["energy"], np.float64))
            values = chain_moments(_chain(specs, incoming))
            out, noise, worst = [], [], 0.0
            for a in values:
                rows = lambda v: a[v * B:(v + 1) * B]  # noqa: E731
                step = lambda s: s.reshape(-1, *([1] * (a.ndim - 1)))  # noqa: E731
                wide, narrow = (rows(0) - rows(1)) / step(2 * h), (rows(2) - rows(3)) / step(h / 2)
                top = np.max(np.abs(wide).reshape(B, -1), axis=1)
                noise.append(eps * np.max(np.abs(rows(0)).reshape(B, -1), axis=1) / (h / 4))
                gap = np.max(np.abs(wide - narrow).reshape(B, -1), axis=1)
                # (an array that does not move at all -- the energy along a magnet's parameter -- agrees with itself)
                worst = max(worst, float(np.max(np.where(gap <= noise[-1], 0.0, gap / np.maximum(top, 1e-300)))))
                out.append(wide)
            tried.append((rel, worst))
            if worst <= TWO_STEP_AGREEMENT:
                return (*out, *noise)
        raise AssertionError(("no step at which the oracle's central differences agree with themselves", q, tried))

    def forward(self):
        """The oracle's outgoing beam."""
        specs, arrays, _ = self._build(1)
        if self.particles is not None:
            return o.segment_track(specs, o.particle_beam(arrays["particles"], arrays["energy"], np.float64), np.float64)
        return o.segment_track(specs, o.parameter_beam(arrays["mu"], arrays["cov"], arrays["energy"], np.float64), np.float64)

    def _target(self, specs, arrays, q):
        """(array, index within a sample, direction or None, magnitude (B,)) of quantity q."""
        B = self.B
        if q == "energy":
            return arrays["energy"], (), None, np.abs(self.energy)
        if q == ("direction",):
            return arrays["particles"], (), self.direction, np.full(B, FLOOR["direction"])
        if q[0] in ("particles", "mu", "cov"):
            return arrays[q[0]], tuple(q[1:]), None, np.full(B, FLOOR[q[0]])
        e, name = q[0], q[1]
        index = tuple(q[2:])
        x0 = np.asarray(self.desc[e][1][name], dtype=np.float64)[(slice(None), *index)]
        return specs[e][name], index, None, np.maximum(np.abs(x0), FLOOR[name])

    def derivatives(self, quantities, scales):
        """{quantity: (B,)}; `scales`: {quantity: scale} or one number."""
        B = self.B
        pending = [q for q in quantities if q not in self._known]
        tried = {q: [] for q in pending}
        for rel in RELATIVE_STEPS:
            if not pending:
                break
            specs, arrays, loss = self._build(4 * len(pending))
            steps = []
            for j, q in enumerate(pending):
                array, index, direction, magnitude = self._target(specs, arrays, q)
                h = rel * magnitude
                steps.append(h)
                for v, d in enumerate((h, -h, h / 4, -h / 4)):
                    rows = slice((4 * j + v) * B, (4 * j + v + 1) * B)
                    if direction is None:
                        array[(rows, *index)] += d
                    else:
                        array[rows] += d.reshape(B, *([1] * (direction.ndim - 1))) * direction
            L = loss().reshape(4 * len(pending), B)
            left = []
            for j, q in enumerate(pending):
                h = steps[j]
                wide, narrow = (L[4 * j] - L[4 * j + 1]) / (2 * h), (L[4 * j + 2] - L[4 * j + 3]) / (h / 2)
                scale = scales[q] if isinstance(scales, dict) else scales
                distance = float(np.max(np.abs(wide - narrow) / np.maximum(np.abs(wide), scale)))
                tried[q].append((rel, distance))
                if distance <= TWO_STEP_AGREEMENT:
                    self._known[q], self.steps_taken[q] = wide, rel
                else:
                    left.append(q)
            pending = left
        assert not pending, ("no step at which the oracle's central differences agree with themselves",
                             {q: tried[q] for q in pending})
        return {q: self._known[q] for q in quantities}


# ---------------------------------------------------------------------------------------------------------------------
# the lattices, beams and cotangents of tests/test_gpu_grad_sizes.py (tests/test_reverse_reference_host.py holds their
# references to the two-step condition).  Every value is a float32 number held in float64, so that the float32 and
# the float64 kernels are given the same problem and share one reference.
# ---------------------------------------------------------------------------------------------------------------------

def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


BEAM_SIGMA = [1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3]
BEAM_MU = [1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3]


def particles(B, N, seed=9, dtype=np.float64):
    return f32(o.gaussian_particles((B,), N, seed=seed, dtype=np.float32, sigma=BEAM_SIGMA, mu=BEAM_MU)).astype(dtype)


def energies(B, seed=3):
    return f32(np.concatenate([[6e6, 8e6], np.random.default_rng(seed).uniform(6e6, 8e6, max(B - 2, 0))])[:B])


def cotangents(B, seed, size=6):
    """(w_mu (B, size), w_cov (B, size, size)): random weights on the six means and the 6 x 6 covariance (a 7th row and column: zero)."""
    rng = np.random.default_rng(seed)
    w_mu, w_cov = np.zeros((B, size)), np.zeros((B, size, size))
    w_mu[:, :6] = rng.normal(size=(B, 6))
    w_cov[:, :6, :6] = rng.normal(size=(B, 6, 6)) * 1e3
    return w_mu, w_cov


def moments_of(P):
    """(mu (B, 7), cov (B, 7, 7)) of a ParameterBeam with the particles' mean and biased covariance."""
    P = np.asarray(P, dtype=np.float64)
    mu = P.mean(axis=1)
    d = P - mu[:, None, :]
    return f32(mu), f32(np.einsum("bni,bnj->bij", d, d) / P.shape[1])


def reading_weights(B, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(2, B)), rng.normal(size=(2, B))]


def affine_lattice(B, seed=21):
    """Every differentiable kind without a cavity, two active BPMs: run, BPM, run, BPM, run -- 5 steps of a ParticleBeam's program."""
    rng = np.random.default_rng(seed)
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    u = lambda lo, hi, *shape: f32(rng.uniform(lo, hi, (B, *shape)))  # noqa: E731
    n = lambda s, *shape: f32(rng.normal(0, s, (B, *shape)))  # noqa: E731
    return [("drift", dict(length=f(0.6))),
            ("quadrupole", dict(length=f(0.2), k1=u(-5, 5), tilt=u(0.1, 0.5), misalignment=n(1e-3, 2))),
            ("hcor", dict(length=f(0.1), angle=n(1e-3))),
            ("dipole", dict(length=f(0.5), angle=u(0.05, 0.2), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4),
                            fringe_integral_exit=f(0.3), gap=f(0.02), tilt=f(0.1))),
            ("bpm", dict(is_active=True)),
            ("vcor", dict(length=f(0.1), angle=n(1e-3))),
            ("solenoid", dict(length=f(0.3), k=u(0.5, 2.0), misalignment=n(1e-3, 2))),
            ("undulator", dict(length=f(0.4))),
            ("rbend", dict(length=f(0.4), angle=u(0.05, 0.15), e1=f(0.03), e2=f(-0.02), fringe_integral=f(0.5),
                           fringe_integral_exit=f(0.45), gap=f(0.03), tilt=f(-0.2))),
            ("bpm", dict(is_active=True)),
            ("quadrupole", dict(length=f(0.3), k1=u(-5, 5))),
            ("dipole", dict(length=f(0.0), angle=u(0.01, 0.05), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4),
                            fringe_integral_exit=f(0.3), gap=f(0.02), tilt=f(0.3))),
            ("drift", dict(length=f(0.4)))]


def take_samples(desc, samples):
    """The description of the chosen samples alone (the whole-batch predicates must not change: every tilt etc. is non-zero)."""
    return [(kind, {k: (v[samples] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}) for kind, kw in desc]


def class_u_lattice(B, seed=43):
    """[drift, misaligned quadrupole, hcor, drift, cavity] x 3 + [quadrupole, drift]: every unit has class U."""
    rng = np.random.default_rng(seed)
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    desc = []
    for _ in range(3):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=f32(rng.uniform(-5, 5, B)), misalignment=f32(rng.normal(0, 1e-3, (B, 2))))),
                 ("hcor", dict(length=f(0.1), angle=f32(rng.normal(0, 1e-3, B)))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=f32(rng.uniform(5e6, 2e7, B)), phase=f32(rng.uniform(-10, 10, B)),
                                 frequency=f(1.3e9)))]
    return desc + [("quadrupole", dict(length=f(0.2), k1=f32(rng.uniform(-5, 5, B)))), ("drift", dict(length=f(0.4)))]


def gentle_cells(B, cells, tail=False, seed=53, quadrupole_every=1, outer_drifts=True):
    """
    `cells` of [drift, misaligned quadrupole, drift, cavity] (+ `tail`: one more [drift, quadrupole, drift]) at gentle
    settings -- 2 to 6 MV per cavity, |k1| <= 2 -- so that a float32 pass through 64 of them stays conditioned.  The draws
    of a cell do not depend on how many cells follow: a shorter lattice is the beginning of a longer one.
    `quadrupole_every=4, outer_drifts=False`: cells of [drift, cavity] with a quadrupole in front of every fourth cavity.
    """
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    desc = []
    for c in range(cells + (1 if tail else 0)):
        rng = np.random.default_rng([seed, c])
        # (focusing and defocusing in turn: with signs drawn at random 64 cells amplify a float32 rounding of the first ones
        # beyond the float32 bound -- measured: misalignments of cells 3 and 4 of 64 off by 4e-3 of their gradients)
        k1, mis = f32((-1) ** (c // quadrupole_every) * rng.uniform(0.5, 2, B)), f32(rng.normal(0, 1e-3, (B, 2)))
        volts, phase = f32(rng.uniform(2e6, 6e6, B)), f32(rng.uniform(-10, 10, B))
        desc.append(("drift", dict(length=f(0.3))))
        if c % quadrupole_every == quadrupole_every - 1:
            desc.append(("quadrupole", dict(length=f(0.1), k1=k1, misalignment=mis)))
            if outer_drifts:
                desc.append(("drift", dict(length=f(0.3))))
        if c < cells:
            desc.append(("cavity", dict(length=f(1.0377), voltage=volts, phase=phase, frequency=f(1.3e9))))
    return desc


def unit_lattice(B, units, pairs):
    """
    A lattice of `units` units of the particles' reverse pass: `pairs` -- the float32 pass in its merged form, a unit is a
    [run, cavity] pair -- `units` cells; otherwise a unit is a step, run and cavity in turn, and an odd count ends on a run.
    Returns (desc, element indices per unit).
    """
    if pairs:
        return gentle_cells(B, units), [list(range(4 * u, 4 * u + 4)) for u in range(units)]
    desc = gentle_cells(B, units // 2, tail=units % 2 == 1)
    return desc, [list(range(4 * (u // 2), 4 * (u // 2) + 3)) if u % 2 == 0 else [4 * (u // 2) + 3] for u in range(units)]


def steps_lattice(B, steps):
    """`steps` steps of run and cavity in turn: cells of [drift, cavity], a quadrupole in front of every fourth cavity."""
    return gentle_cells(B, steps // 2, tail=steps % 2 == 1, quadrupole_every=4, outer_drifts=False)


def step_elements(desc):
    """Element indices per step of the program: maximal runs of skippable elements, every cavity on its own."""
    steps, run = [], []
    for e, (kind, _) in enumerate(desc):
        if kind == "cavity":
            if run:
                steps.append(run)
            steps.append([e])
            run = []
        else:
            run.append(e)
    return steps + ([run] if run else [])


PALETTE_KINDS = ("drift", "hcor", "vcor", "dipole", "solenoid", "undulator", "rbend", "drift")


def long_affine_lattice(B, E, seed=77):
    """
    One run of E elements of mixed kinds, every second one a quadrupole (tilted and misaligned, plain, misaligned, tilted
    in turn; focusing and defocusing in turn).  The elements come from a palette of a few settings per sample, so that
    their map derivatives are evaluated once; a shorter lattice is the beginning of a longer one.
    """
    rng = np.random.default_rng(seed)
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    u = lambda lo, hi, *shape: f32(rng.uniform(lo, hi, (B, *shape)))  # noqa: E731
    quads = [dict(length=f(0.1), k1=u(1.0, 2.0), tilt=u(0.05, 0.2), misalignment=u(-1e-3, 1e-3, 2)),
             dict(length=f(0.1), k1=-u(1.0, 2.0)),
             dict(length=f(0.1), k1=u(1.0, 2.0), misalignment=u(-1e-3, 1e-3, 2)),
             dict(length=f(0.1), k1=-u(1.0, 2.0), tilt=u(0.05, 0.2))]
    others = {"drift": dict(length=f(0.2)), "hcor": dict(length=f(0.1), angle=u(-1e-3, 1e-3)),
              "vcor": dict(length=f(0.1), angle=u(-1e-3, 1e-3)),
              "dipole": dict(length=f(0.2), angle=u(0.01, 0.03), e1=f(0.05), e2=f(0.02), fringe_integral=f(0.4),
                             fringe_integral_exit=f(0.3), gap=f(0.02), tilt=f(0.1)),
              "solenoid": dict(length=f(0.1), k=u(0.2, 0.5), misalignment=u(-1e-3, 1e-3, 2)),
              "undulator": dict(length=f(0.2)),
              "rbend": dict(length=f(0.2), angle=u(0.01, 0.03), e1=f(0.03), e2=f(-0.02), fringe_integral=f(0.5),
                            fringe_integral_exit=f(0.45), gap=f(0.03), tilt=f(-0.2))}
    desc = []
    for e in range(E):
        if e % 2 == 0:
            desc.append(("quadrupole", quads[(e // 2) % 4]))
        else:
            kind = PALETTE_KINDS[(e // 2) % len(PALETTE_KINDS)]
            desc.append((kind, others[kind]))
    return desc


def lds_switch(itemsize, steps=1, limit=40 << 10):
    """
    The largest element count E of a program of `steps` steps at which k_build_bwd still keeps maps and prefix products in LDS:
    build_bwd_lds_fixed(S, E) + (2 E + S + 1) 49 sizeof(T) <= 40 KiB, build_bwd_lds_fixed = (2 (S + 1) + E + 4 . 98) sizeof(T)
    (lynx_grad.hpp, track_backward_t).
    """
    bytes_at = lambda E: ((2 * (steps + 1) + E + 4 * 98) + (2 * E + steps + 1) * 49) * itemsize  # noqa: E731
    E = 1
    while bytes_at(E + 1) <= limit:
        E += 1
    return E


def backward_geometry(N, B, compute_units, lane_particles):
    """(tiles, chunks, tiles_per_wg) of track_backward_t: a tile is 256 lanes of `lane_particles` particles; 24 workgroups per CU."""
    tiles = -(-N // (256 * lane_particles))
    chunks = max(1, min(tiles, (24 * compute_units + B - 1) // B))
    per_wg = -(-tiles // chunks)
    return tiles, -(-tiles // per_wg), per_wg


# ---- cases held to the oracle's differences: (OracleCase, {quantity: scale}) -------------------------------------------
# scales of the two-step condition -- a derivative below them counts as zero: a parameter's 1e-9 max|w_cov| (the floor
# of the parameter tolerance); the energy's 1e-13; a particle coordinate's 1e-1 / N (z_bar_out is (w_mu + 2 W d) / N, of
# order 1 / N), the directional derivative's 1e-8; 1e-2 for mu_bar (order 1) and 10 for cov_bar (order 1e3).

CHECKED = {"drift": [("length",)], "quadrupole": [("k1",), ("misalignment", 0), ("misalignment", 1)], "hcor": [("angle",)],
           "cavity": [("voltage",), ("phase",)]}
_cases: dict = {}


def _parameter_quantities(desc, elements):
    return [(e, *tail) for e in dict.fromkeys(elements) for tail in CHECKED.get(desc[e][0], [])]


def _scales(quantities, w_cov, N=1):
    out = {}
    for q in quantities:
        if q == "energy":
            out[q] = 1e-13
        elif q == ("direction",):
            out[q] = 1e-8
        elif q[0] == "particles":
            out[q] = 1e-1 / N
        elif q[0] == "mu":
            out[q] = 1e-2
        elif q[0] == "cov":
            out[q] = 10.0
        else:
            out[q] = 1e-9 * float(np.max(np.abs(w_cov)))
    return out


PARTICLE_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 1025)
PACKED_EDGES = (255, 256, 511, 512)


def class_u_case(N):
    """Axis A: the class-U cavity lattice, B = 2, N particles."""
    if ("u", N) not in _cases:
        B = 2
        desc = class_u_lattice(B)
        w_mu, w_cov = cotangents(B, 1000 + N)
        direction = np.random.default_rng(N).normal(size=(B, N, 7)) * [*BEAM_SIGMA, 0.0]
        case = OracleCase(desc, energies(B), w_mu, w_cov, particles=particles(B, N, seed=N), direction=direction)
        chosen = sorted({0, N - 1, *(n for n in PACKED_EDGES if n < N)})
        quantities = ([(0, "length"), (1, "k1"), (6, "misalignment", 1), (2, "angle"), (4, "voltage"), (9, "phase"), "energy",
                       ("direction",)] + [("particles", n, c) for n in chosen for c in range(6)])
        _cases[("u", N)] = (case, _scales(quantities, w_cov, N))
    return _cases[("u", N)]


DENSE_UNITS = (1, 2, 3, 4, 5, 8, 9, 63, 64)
STRUCTURED_UNITS = (1, 7, 8, 9, 15, 16, 17)
UNITS_N = 301


def units_case(units, pairs):
    """Axis B: `units` units (unit_lattice), B = 2, N = 301: first and last element, the elements of units 3, 4 and U - 1, the energy."""
    key = ("units", units, pairs)
    if key not in _cases:
        B = 2
        desc, members = unit_lattice(B, units, pairs)
        w_mu, w_cov = cotangents(B, 2000 + units)
        case = OracleCase(desc, energies(B), w_mu, w_cov, particles=particles(B, UNITS_N, seed=11))
        elements = [0, len(desc) - 1] + [e for u in (3, 4, units - 1) if 0 <= u < units for e in members[u]]
        quantities = _parameter_quantities(desc, elements) + ["energy"]
        _cases[key] = (case, _scales(quantities, w_cov))
    return _cases[key]


STEP_COUNTS = (255, 256, 257, 261)
COV_ENTRIES = [(0, 0), (0, 1), (1, 0), (2, 3), (4, 4), (4, 5), (5, 4), (5, 5), (3, 5)]


def steps_case(steps):
    """Axis D: a ParameterBeam through `steps` steps (steps_lattice), B = 2, float64."""
    key = ("steps", steps)
    if key not in _cases:
        B = 2
        desc = steps_lattice(B, steps)
        members = step_elements(desc)
        assert len(members) == steps
        # (one draw for all four lattices.  With a draw per lattice, sample 0 of the 261-step one had voltage gradients that
        # change sign along the last cavities, 1e-13 next to the neighbouring cases' 1e-10: measured float32 errors of 4e-3
        # to 1e-1 of such a value at steps 245 .. 259, below and above step 256 alike, and 1e-5 in sample 1)
        w_mu, w_cov = cotangents(B, 3257, size=7)
        mu, cov = moments_of(particles(B, 400, seed=13))
        case = OracleCase(desc, energies(B), w_mu, w_cov, mu=mu, cov=cov)
        cavities = [e for e, (kind, _) in enumerate(desc) if kind == "cavity"]
        quadrupoles = [e for e, (kind, _) in enumerate(desc) if kind == "quadrupole"]
        around = [e for s in (254, 255, 256, 257) if s < steps for e in members[s]]  # the steps around thread 255
        elements = [cavities[0], *around, cavities[-1], quadrupoles[0], quadrupoles[-1], 0]
        quantities = (_parameter_quantities(desc, elements) + ["energy"] + [("mu", c) for c in range(6)]
                      + [("cov", r, c) for r, c in COV_ENTRIES])
        _cases[key] = (case, _scales(quantities, w_cov))
    return _cases[key]


def references(case_and_scales):
    case, scales = case_and_scales
    return case.derivatives(list(scales), scales)


