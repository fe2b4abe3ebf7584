"""
The moment loss of `grad.track_along_vjp(..., moment_targets=)` restated in NumPy float64, for the host and the GPU tests:
the value of every term and the loss, by the formulas of the issue (include/lynx_hip.h, lynx_moments_along_loss), and for
everything compared its UNCANCELLED SIZE -- the sum of the absolute values of the terms added into it, the scale rounding
errors have.  q = s2 p2 - cross^2 is a difference, so every term that passes through eps = sqrt(max(q, tiny)) is multiplied
by kappa = (s2 p2 + cross^2) / max(q, tiny).

The cotangents are NOT restated: their reference is the host rule the library had before, `grad.trace_property_cotangents`
on a host-made trace, one call per property name, packed by `grad._record_cotangents` for the records form.
"""

import numpy as np

PROPERTIES = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p",
              "sigma_xxp", "sigma_yyp", "emittance_x", "emittance_y", "normalized_emittance_x", "normalized_emittance_y",
              "beta_x", "beta_y", "alpha_x", "alpha_y", "energy")
THROUGH_EPS = tuple(name for name in PROPERTIES if name.rpartition("_")[0] in ("emittance", "normalized_emittance", "beta", "alpha"))
ELECTRON_MASS_EV = 510998.95069


def tri(i, j):
    return 7 + i * 6 - (i * (i - 1)) // 2 + (j - i)


def values_of(dtype, energy, records=None, ddof=None, mu=None, cov=None):
    """
    {name: value (*lead,)} and {name: kappa (*lead,)} (1 for a value that does not pass through eps) of states shaped
    (*lead, 36) or (*lead, 7), (*lead, 7, 7), float64 throughout; `dtype` is the beam's (it sets the floor and `tiny`).
    """
    dtype = np.dtype(dtype)
    tiny = float(np.finfo(dtype).tiny)
    energy = np.asarray(energy, dtype=np.float64)
    with np.errstate(all="ignore"):
        if records is not None:
            rec = np.asarray(records, dtype=np.float64)
            n = rec[..., 35]
            scale = n / (n - ddof)
            mean = [rec[..., c] for c in range(6)]
            s2 = [rec[..., tri(c, c)] * scale for c in range(6)]
            cross = {0: rec[..., tri(0, 1)], 2: rec[..., tri(2, 3)]}
        else:
            mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
            floor = float(dtype.type(1e-20))
            mean = [mu[..., c] for c in range(6)]
            s2 = [np.maximum(cov[..., c, c], floor) for c in range(6)]
            cross = {0: cov[..., 0, 1], 2: cov[..., 2, 3]}
        gamma = energy / ELECTRON_MASS_EV
        bg = np.where(np.abs(gamma) > 0, np.sqrt(1 - 1 / gamma**2) * gamma, 0.0)
        values, kappa = {}, {}
        for c, coordinate in enumerate(("x", "xp", "y", "yp", "s", "p")):
            values["mu_" + coordinate] = mean[c]
            values["sigma_" + coordinate] = np.sqrt(s2[c])
        values["sigma_xxp"], values["sigma_yyp"], values["energy"] = cross[0], cross[2], energy
        for a, plane in ((0, "x"), (2, "y")):
            q = s2[a] * s2[a + 1] - cross[a] ** 2
            eps = np.sqrt(np.maximum(q, tiny))
            values["emittance_" + plane] = eps
            values["normalized_emittance_" + plane] = eps * bg
            values["beta_" + plane] = s2[a] / eps
            values["alpha_" + plane] = -cross[a] / eps
            for head in ("emittance_", "normalized_emittance_", "beta_", "alpha_"):
                kappa[head + plane] = (s2[a] * s2[a + 1] + cross[a] ** 2) / np.maximum(q, tiny)
    ones = np.ones(energy.shape)
    return values, {name: kappa.get(name, ones) for name in PROPERTIES}


def mask_of(names):
    return sum(1 << PROPERTIES.index(name) for name in names)


def terms_of(target_points):
    """[(point, name)] in (point, bit) order of [(point, mask)]."""
    return [(point, name) for point, mask in target_points for k, name in enumerate(PROPERTIES) if (mask >> k) & 1]


def loss_of(terms, rows, values, kappa):
    """
    `terms` [(point, name)], `rows` (B, T, 2) of (target, weight), `values`, `kappa` {name: (B, P)} -> a dict of
      value (B, T), value_size;  point_loss (B, Q), point_loss_size;  loss (B,), loss_size;  the bar of every term for
      loss_bar = 1: bar (B, T) = 2 w (value - target), bar_size = 2 |w| (|value| + |target|)
    with the sums taken in term order, a point's first and the points' after.
    """
    B = rows.shape[0]
    out = {key: np.zeros((B, len(terms))) for key in ("value", "value_size", "bar", "bar_size")}
    points = sorted({point for point, _ in terms})
    for key in ("point_loss", "point_loss_size"):
        out[key] = np.zeros((B, len(points)))
    with np.errstate(all="ignore"):
        for t, (point, name) in enumerate(terms):
            v, k = values[name][:, point], kappa[name][:, point]
            target, weight = rows[:, t, 0], rows[:, t, 1]
            out["value"][:, t], out["value_size"][:, t] = v, np.abs(v) * k
            out["bar"][:, t] = 2.0 * weight * (v - target)
            out["bar_size"][:, t] = 2.0 * np.abs(weight) * (np.abs(v) + np.abs(target))
            q = points.index(point)
            out["point_loss"][:, q] += weight * (v - target) ** 2
            out["point_loss_size"][:, q] += np.abs(weight) * (np.abs(v) * k + np.abs(target)) ** 2
    out["loss"], out["loss_size"] = np.zeros(B), np.zeros(B)
    for q in range(len(points)):
        out["loss"] += out["point_loss"][:, q]
        out["loss_size"] += out["point_loss_size"][:, q]
    return out


def cotangents_of(trace, terms, bars, bar_sizes, kappa):
    """
    The host rule on `trace` for the bars (B, T) of `terms`: (mu_bar, cov_bar, energy_bar) and their uncancelled sizes -- per
    property name one call of `grad.trace_property_cotangents` with the bars, one with |bars| sizes (the rule is linear in the
    bar: the absolute value of what it adds is what it adds for the absolute bar), times kappa for a name that passes through eps.
    """
    from lynx_amd import grad

    B, P = bars.shape[0], trace.num_points
    total = [np.zeros((B, P, 7)), np.zeros((B, P, 7, 7)), np.zeros((B, P))]
    size = [np.zeros((B, P, 7)), np.zeros((B, P, 7, 7)), np.zeros((B, P))]
    for name in PROPERTIES:
        at = [(t, point) for t, (point, term) in enumerate(terms) if term == name]
        if not at:
            continue
        bar, bar_size = np.zeros((B, P)), np.zeros((B, P))
        for t, point in at:
            bar[:, point], bar_size[:, point] = bars[:, t], bar_sizes[:, t]
        with np.errstate(all="ignore"):
            added = grad.trace_property_cotangents(trace, {name: bar})
            sized = grad.trace_property_cotangents(trace, {name: bar_size})
        k = kappa[name]
        for n, scale in enumerate((k[..., None], k[..., None, None], k)):
            total[n] += added[n].reshape(total[n].shape)
            with np.errstate(over="ignore"):  # (q == 0: kappa is 1 / tiny, and such a size says "anything finite")
                size[n] += np.abs(sized[n].reshape(size[n].shape)) * scale
    return total, size


def touched(target_points, B, P):
    """Boolean (B, P, 7), (B, P, 7, 7), (B, P): the entries the reverse call may add into (include/lynx_hip.h)."""
    mu, cov, energy = np.zeros((B, P, 7), bool), np.zeros((B, P, 7, 7), bool), np.zeros((B, P), bool)
    for point, mask in target_points:
        names = [name for k, name in enumerate(PROPERTIES) if (mask >> k) & 1]
        for name in names:
            head, _, tail = name.partition("_")
            if head == "mu":
                mu[:, point, ("x", "xp", "y", "yp", "s", "p").index(tail)] = True
            elif head == "sigma" and tail in ("x", "xp", "y", "yp", "s", "p"):
                c = ("x", "xp", "y", "yp", "s", "p").index(tail)
                cov[:, point, c, c] = True
            elif name in ("sigma_xxp", "sigma_yyp"):
                a = 0 if name == "sigma_xxp" else 2
                cov[:, point, a, a + 1] = True
            elif name in THROUGH_EPS:
                a = 0 if name.endswith("_x") else 2
                cov[:, point, a, a] = cov[:, point, a + 1, a + 1] = cov[:, point, a, a + 1] = True
            if name in ("energy", "normalized_emittance_x", "normalized_emittance_y"):
                energy[:, point] = True
    return mu, cov, energy


def touched_records(target_points, B, P):
    """`touched` as record slots (B, P, 36)."""
    mu, cov, energy = touched(target_points, B, P)
    rec = np.zeros((B, P, 36), bool)
    rec[..., :6] = mu[..., :6]
    for i in range(6):
        for j in range(i, 6):
            rec[..., tri(i, j)] = cov[..., i, j]
    return rec, energy
