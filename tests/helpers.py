"""Shared test helpers: one lattice description -> (lynx_amd elements, oracle specs)."""

import ctypes as C

import numpy as np

from oracle import lynx_oracle as o


def make_lattice(desc, dtype, lx=None):
    """
    desc: list of (kind, kwargs) with array-valued kwargs.  Returns (elements, specs);
    `elements` is None when the product package is not wanted (lx=None).
    """
    ctor_o = {"drift": o.Drift, "quadrupole": o.Quadrupole, "dipole": o.Dipole, "rbend": o.RBend,
              "hcor": o.HorizontalCorrector, "vcor": o.VerticalCorrector, "cavity": o.Cavity,
              "custom": o.CustomTransferMap, "bpm": o.BPM, "marker": o.Marker, "solenoid": o.Solenoid,
              "undulator": o.Undulator}
    specs, elements = [], []
    for kind, kw in desc:
        kw_t = {k: (np.asarray(v, dtype=dtype) if isinstance(v, (np.ndarray, list, float)) else v)
                for k, v in kw.items()}
        specs.append(ctor_o[kind](**kw_t))
        if lx is not None:
            ctor_x = {"drift": lx.Drift, "quadrupole": lx.Quadrupole, "dipole": lx.Dipole, "rbend": lx.RBend,
                      "hcor": lx.HorizontalCorrector, "vcor": lx.VerticalCorrector, "cavity": lx.Cavity,
                      "custom": lx.CustomTransferMap, "bpm": lx.BPM, "marker": lx.Marker, "solenoid": lx.Solenoid,
                      "undulator": lx.Undulator}
            if kind in ("bpm", "marker"):
                elements.append(ctor_x[kind](**kw_t))
            else:
                elements.append(ctor_x[kind](**kw_t, dtype=dtype))
    return (elements if lx is not None else None), specs


def _some(rng, shape, draw, p=0.5):
    """`draw(shape)` in a random subset of the samples, 0 in the others: a whole-batch any() that some samples take."""
    return np.where(rng.random(shape) < p, draw(shape), 0.0)


def criterion(particles, x_max, y_max, shape):
    """The normalised quantities whose distance from 1 says how close to the boundary a particle is: (k, *batch, N)."""
    x, y = particles[..., 0], particles[..., 2]
    xm, ym = np.asarray(x_max, dtype=np.float64)[..., None], np.asarray(y_max, dtype=np.float64)[..., None]
    with np.errstate(all="ignore"):
        if shape == "elliptical":
            return np.stack([x ** 2 / xm ** 2 + y ** 2 / ym ** 2])
        return np.stack([np.abs(x) / xm, np.abs(y) / ym])


def build(desc, dtype, lx=None):
    """`make_lattice` with ("aperture", dict(x_max, y_max, shape)) entries: identity markers in the oracle's chain."""
    plain = [("marker", {}) if kind == "aperture" else (kind, kw) for kind, kw in desc]
    elements, specs = make_lattice(plain, dtype, lx)
    for k, (kind, kw) in enumerate(desc):
        if kind == "aperture" and lx is not None:
            elements[k] = lx.Aperture(x_max=np.asarray(kw["x_max"], dtype=dtype), y_max=np.asarray(kw["y_max"], dtype=dtype),
                                      shape=kw["shape"], is_active=kw.get("is_active", True), name=f"AP{k}", dtype=dtype)
    return elements, specs


def rel_err(got, ref):
    """max |got-ref| / max|ref| per trailing coordinate (robust to zeros), NaN-aware."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), "NaN pattern differs"
    g, r = np.where(nan_g, 0.0, got), np.where(nan_r, 0.0, ref)
    scale = np.max(np.abs(r)) + 1e-300
    return float(np.max(np.abs(g - r)) / scale)


def map_err(got, ref):
    """
    Error of a 7x7 map (or a batch of them) entry-wise relative to the largest entry of its
    2x2-block row: maps hold entries of very different magnitude (R56 ~ 1e-6 next to 1).
    """
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), "NaN pattern differs"
    inf_g, inf_r = np.isinf(got), np.isinf(ref)
    assert np.array_equal(inf_g, inf_r) and np.array_equal(np.sign(got[inf_g]), np.sign(ref[inf_r])), "inf pattern differs"
    g, r = np.where(nan_g | inf_g, 0.0, got), np.where(nan_r | inf_r, 0.0, ref)
    denom = np.maximum(np.abs(r), 1e-3 * np.max(np.abs(r), axis=(-1, -2), keepdims=True)) + 1e-300
    return float(np.max(np.abs(g - r) / denom))


def harness_map(h, kind, flags, params, energy, dtype, want_coef=False):
    dtype = np.dtype(dtype)
    ct = C.c_float if dtype == np.float32 else C.c_double
    fn = h.harness_build_f32 if dtype == np.float32 else h.harness_build_f64
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, ct, C.c_void_p, C.c_void_p, C.c_int]
    fn.restype = None
    p = np.ascontiguousarray(np.asarray(params, dtype=dtype))
    if p.size == 0:
        p = np.zeros(1, dtype=dtype)
    M = np.zeros(49, dtype=dtype)
    coef = np.zeros(8, dtype=dtype)
    fn(kind, flags, p.ctypes.data, ct(float(energy)), M.ctypes.data, coef.ctypes.data, int(want_coef))
    return M.reshape(7, 7), coef


def assert_parameter_beam(out, ref, tol, what=""):
    """
    mu and the 6 x 6 covariance of a tracked ParameterBeam against the oracle's, ENTRY BY ENTRY at `tol`:
    |d mu_i| <= tol (|mu_i| + sigma_i),  |d cov_ij| <= tol max(sigma_i sigma_j, |cov_ij|).
    The second scale matters behind an active cavity: the reference overwrites cov[4,4] and cov[4,5] with a
    second-order quantity (cavity.py:207-218: T566 c55^2 + T556 c45 c55 + T555 c44^2, ~1e-21 for a micrometre bunch)
    and leaves the rest of the s row as it was, so the matrix is no longer positive semi-definite and sigma_s does
    not bound its own row -- there an entry is compared with its own size.  `out`: a beam or a (mu, cov) pair.
    """

    mu, cov = (out._mu, out._cov) if hasattr(out, "_mu") else out
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    rmu, rcov = np.asarray(ref["mu"], dtype=np.float64), np.asarray(ref["cov"], dtype=np.float64)
    assert np.array_equal(np.isnan(cov), np.isnan(rcov)) and np.array_equal(np.isnan(mu), np.isnan(rmu)), what
    sig = np.sqrt(np.abs(np.einsum("...ii->...i", rcov[..., :6, :6])))
    scale = np.maximum(sig[..., :, None] * sig[..., None, :], np.abs(rcov[..., :6, :6])) + 1e-300
    dmu = np.abs(mu[..., :6] - rmu[..., :6]) / (np.abs(rmu[..., :6]) + sig + 1e-300)
    dcov = np.abs(cov[..., :6, :6] - rcov[..., :6, :6]) / scale
    assert np.nanmax(dmu) <= tol, (what, "mu", float(np.nanmax(dmu)), np.unravel_index(np.nanargmax(dmu), dmu.shape))
    assert np.array_equal(mu[..., 6], rmu[..., 6], equal_nan=True), what  # (NaN patterns: asserted equal above)
    assert np.nanmax(dcov) <= tol, (what, "cov", float(np.nanmax(dcov)), np.unravel_index(np.nanargmax(dcov), dcov.shape))


def singular_entry_voltage(energy, phase, length, frequency, lo, hi):
    """The voltage in [lo, hi] at which the (s, delta) block of the reference's cavity map (cavity.py:311-323) is singular."""
    def det(v):
        a = lambda x: np.array([x], dtype=np.float64)  # noqa: E731
        m = o.element_transfer_map(o.Cavity(a(length), voltage=a(v), phase=a(phase), frequency=a(frequency)), a(energy), np.float64)[0]
        return m[4, 4] * m[5, 5] - m[4, 5] * m[5, 4]
    assert det(lo) * det(hi) < 0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if det(mid) * det(lo) > 0 else (lo, mid)
    return 0.5 * (lo + hi)


def random_samples(batch, count, always=(), record=None):
    """
    `count` sample indices of a batch drawn at random PER RUN (a k1-dependent error in samples nobody ever picks would
    otherwise pass for ever), plus the ones in `always`; the seed is printed -- and handed to `record`, pytest's
    `record_property` -- so that a failure can be replayed with LYNX_TEST_SAMPLE_SEED=<seed>.
    """
    import os

    seed = int(os.environ.get("LYNX_TEST_SAMPLE_SEED") or int.from_bytes(os.urandom(4), "little"))
    print(f"random_samples: LYNX_TEST_SAMPLE_SEED={seed}")
    if record is not None:
        record("sample_seed", seed)
    rng = np.random.default_rng(seed)
    drawn = rng.choice(batch, size=min(count, batch), replace=False)
    return sorted(set(int(i) for i in always) | set(int(i) for i in drawn)), seed


MOMENT_KEYS = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
               "sigma_p", "sigma_xxp", "sigma_yyp")


def tri_slot(i, j):
    """Slot of cov[i, j] = cov[j, i] in a moment record (include/lynx_hip.h: 6 means, 1, the 21 entries of the triangle)."""
    i, j = min(i, j), max(i, j)
    return 7 + i * 6 - (i * (i - 1)) // 2 + (j - i)


def biased_covariance(particles, alive=None):
    """
    (*batch, 6, 6) float64: the biased covariance of (*batch, N, 7) particles, by numpy in float64 from the stored values.
    `alive` (*batch, N) bool: over each sample's survivors alone (their number differs from sample to sample); a sample
    nobody is left in is NaN everywhere.
    """
    P = np.asarray(particles)
    batch = P.shape[:-2]
    out = np.full((*batch, 6, 6), np.nan)
    with np.errstate(all="ignore"):
        for b in np.ndindex(*batch):  # (sample by sample: a sample's float64 copy stays in the cache)
            q = (P[b] if alive is None else P[b][alive[b]])[:, :6].astype(np.float64)
            if len(q):
                q -= q.mean(axis=0)
                out[b] = q.T @ q / len(q)
    return out


OFF_DIAGONAL = [(i, j) for i in range(6) for j in range(i + 1, 6)]


def correlations(particles, alive=None):
    """(*batch, 15): |correlation| of the 15 off-diagonal slots of the particles' covariance (a slot that is NaN counts as 0)."""
    cov = biased_covariance(particles, alive)
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.einsum("...ii->...i", cov))
        rho = np.abs(cov / (sig[..., :, None] * sig[..., None, :]))
    return np.nan_to_num(np.stack([rho[..., i, j] for i, j in OFF_DIAGONAL], axis=-1))


def covariance_distances(got_cov, ref_particles_or_cov, alive=None):
    """
    EVERY entry (i, j) of a (*batch, 6, 6) covariance against the reference's: |got - ref| / (sigma_i sigma_j), the sigmas
    the reference's own -- the scale `moment_distances` measures sigma_xxp in.  The reference is a (*batch, 6, 6) covariance,
    or (*batch, N, 7) particles, whose biased float64 covariance `biased_covariance` takes (over `alive`, if given).  The
    NaN patterns must be equal.  Where the reference has no spread at all (one particle: sigma = 0) the covariance must be
    0 exactly.  Returns (worst distance, (i, j, sample)) -- `sample` the batch index of the worst entry -- so that a
    failure names the slot.
    """
    got = np.asarray(got_cov, dtype=np.float64)
    ref = np.asarray(ref_particles_or_cov)
    ref = biased_covariance(ref, alive) if ref.shape[-1] == 7 else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and got.shape[-2:] == (6, 6), (got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        *sample, i, j = (int(v) for v in np.argwhere(nan_g != nan_r)[0])
        raise AssertionError(f"NaN pattern differs: first at cov[{i}, {j}] of sample {tuple(sample)}: got {got[(*sample, i, j)]}, "
                             f"reference {ref[(*sample, i, j)]}")
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.einsum("...ii->...i", ref))
        scale = np.nan_to_num(sig[..., :, None] * sig[..., None, :]) + 1e-300
        d = np.where(nan_r, 0.0, np.abs(got - ref) / scale)
    d = np.where(np.isnan(d), np.inf, d)  # (an inf on one side only)
    if d.size == 0:
        return 0.0, (0, 0, ())
    *sample, i, j = (int(v) for v in np.unravel_index(np.argmax(d), d.shape))
    return float(d[(*sample, i, j)]), (i, j, tuple(sample))


def moment_distances(got, ref, scale=None):
    """
    Per beam moment, the largest distance over the samples between `got` and `ref` (dicts key -> array, or objects with
    those attributes) in units of north_star's tolerance scale: |mu| + sigma for a mean, sigma for a sigma,
    sigma_a sigma_b for a correlation; the scales are taken from `scale` (default `ref`).
    """
    get = lambda obj, key: np.asarray(obj[key] if isinstance(obj, dict) else getattr(obj, key), dtype=np.float64)  # noqa: E731
    scale = ref if scale is None else scale
    out = {}
    for key in MOMENT_KEYS:
        g, r = get(got, key), get(ref, key)
        if key.startswith("mu_"):
            s = np.abs(get(scale, key)) + get(scale, "sigma" + key[2:])
        elif key in ("sigma_xxp", "sigma_yyp"):
            a, b = ("sigma_x", "sigma_xp") if key == "sigma_xxp" else ("sigma_y", "sigma_yp")
            s = get(scale, a) * get(scale, b)
        else:
            s = get(scale, key)
        out[key] = float(np.max(np.abs(g - r) / s))
    return out
