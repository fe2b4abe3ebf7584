"""
Seeded random cases of the GPU paths against the oracle.

The library picks its kernel form from the shape of every call and from what ran before it (wave tiles or
per-particle accesses, particles per lane, structured units or the dense step loop, merged [run, cavity] pairs, the
lanes build, parameters in the kernel arguments, host-visible records, the short-call inline path, the step-table
slots, the reverse pass's reuse of the forward table).  The hand-picked shapes of the other files cover each of these
on purpose; here lattices, batch shapes, particle counts, beams, call patterns and launch-plan knobs are DRAWN, and
every result is held to the oracle at the suite's tolerances.

Case i depends on (seed, i) only: LYNX_FUZZ_SEED=<seed> and `-k c07-` replay one case.  Everything is drawn on the CPU
with a numpy Generator before anything reaches the GPU, and nothing is ever retried or shrunk: a case that fails is a
finding.
"""

import os

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import _some, assert_parameter_beam, make_lattice, rel_err
from .test_gpu_parity import KICK_MOMENTS, TOL_KICK_F64, TOL_MOM, TOL_P, VARIANTS

pytestmark = pytest.mark.gpu

DEFAULT_SEED = 20261016
SEED = int(os.environ.get("LYNX_FUZZ_SEED") or DEFAULT_SEED)
N_CASES = 48
N_PROGRAMS = 4
LONG_F32_CASE = 2  # the float32 case whose lattice has more than 64 elements
SHAPES = [(1,), (3,), (64,), (255,), (256,), (300,), (2, 3), (4, 16)]
COUNTS = [1, 63, 64, 255, 257, 1000, 2047, 2049, 4097, 70_001]
KINDS = ["drift", "quadrupole", "dipole", "rbend", "hcor", "vcor", "cavity", "custom", "bpm", "marker", "solenoid",
         "undulator"]
# (entry 13 was the pair of the fused build prologue's switch and LYNX_UNROLL=1 while that form existed: the half that is
# left keeps the place, so that every case draws the knob it always drew)
KNOBS = VARIANTS[:13] + [{"LYNX_UNROLL": "1"}] + VARIANTS[13:] + [{"LYNX_TRACK_UNITS": "0"}, {"LYNX_INLINE_POOL": "0"},
                                                                 {"LYNX_LANES_BUILD_MIN_BATCH": "1"}]
STEP_BUDGET = 6_000_000  # particle-element steps of the oracle per case (48 cases: < 3e8 in all)
TOL_PB = TOL_MOM  # a ParameterBeam's mu and cov are its moments
CONDITION_F32 = 5e-5  # float32 draws: the oracle's own float32 chain within this of float64 (see _float32_conditioned)


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


@pytest.fixture(autouse=True)
def _record_seed(record_property):
    print(f"test_gpu_fuzz: LYNX_FUZZ_SEED={SEED}")
    record_property("fuzz_seed", SEED)


# ---------------------------------------------------------------------------------------------------------------------
# drawing
# ---------------------------------------------------------------------------------------------------------------------


def _element(rng, kind, shape, drawn):
    """One element as (kind, keyword arguments), parameters per sample or broadcast (shape (1,))."""
    wide = rng.random() < 0.3 and kind not in ("drift", "solenoid")  # (the oracle's drift / solenoid want the beam's shape)
    s = (1,) if wide else shape
    u = lambda lo, hi: rng.uniform(lo, hi, s)  # noqa: E731
    if kind == "drift":
        return dict(length=np.where(rng.random(s) < 0.1, 0.0, u(0.0, 1.0)))
    if kind == "quadrupole":
        kw = dict(length=u(0.05, 0.3), k1=u(-5, 5))
        if rng.random() < 0.4:
            kw["tilt"] = _some(rng, s, lambda sh: rng.uniform(-0.5, 0.5, sh))
        if rng.random() < 0.4:
            kw["misalignment"] = _some(rng, (*s, 2), lambda sh: rng.normal(0, 1e-4, sh))
        return kw
    if kind in ("dipole", "rbend"):
        mode = rng.choice(["thick", "thin", "mixed"], p=[0.6, 0.2, 0.2]) if kind == "dipole" else "thick"
        length = {"thick": u(0.1, 0.6), "thin": np.zeros(s), "mixed": np.where(rng.random(s) < 0.5, 0.0, u(0.1, 0.6))}[mode]
        kw = dict(length=length, angle=u(-0.1, 0.1))
        if rng.random() < 0.5:
            kw.update(e1=u(-0.05, 0.05), e2=u(-0.05, 0.05))
        if rng.random() < 0.5:
            kw.update(fringe_integral=u(0.0, 0.5), gap=u(0.0, 0.03))
            if rng.random() < 0.5:
                kw["fringe_integral_exit"] = u(0.0, 0.5)
        if rng.random() < 0.4:
            kw["tilt"] = _some(rng, s, lambda sh: rng.uniform(-0.3, 0.3, sh))
        return kw
    if kind in ("hcor", "vcor"):
        return dict(length=u(0.0, 0.3), angle=rng.normal(0, 1e-3, s))
    if kind == "cavity":
        voltage = u(1e6, 2e7)
        if not wide and np.prod(s) > 1 and not drawn["cavity_off"] and rng.random() < 0.3:
            # switched off in a few samples of the batch: the reference's map is NaN there (cavity.py:262-264, Ep = 0),
            # those samples stay NaN from here on -- one such cavity per lattice, so that most samples keep numbers
            drawn["cavity_off"] = True
            off = rng.random(s) < 0.1
            off.flat[rng.integers(off.size)] = True
            voltage = np.where(off, 0.0, voltage)
        return dict(length=u(0.5, 1.5), voltage=voltage, phase=u(-20, 20), frequency=np.full(s, rng.choice([1.3e9, 2.856e9])))
    if kind == "custom":
        tm = np.broadcast_to(np.eye(7), (*s, 7, 7)).copy()
        tm[..., :6, :6] += rng.normal(0, 1e-2, (*s, 6, 6))
        tm[..., :6, 6] = rng.normal(0, 1e-5, (*s, 6))
        kw = dict(transfer_map=tm)
        if rng.random() < 0.5:
            kw["length"] = u(0.0, 1.0)
        return kw
    if kind == "bpm":
        on = drawn["active_bpms"] < 2 and rng.random() < 0.5
        drawn["active_bpms"] += on
        return dict(is_active=bool(on))
    if kind == "marker":
        return {}
    if kind == "solenoid":
        kw = dict(length=rng.uniform(0.05, 0.5, shape), k=rng.uniform(-2, 2, shape))
        if rng.random() < 0.4:
            kw["misalignment"] = _some(rng, (*shape, 2), lambda sh: rng.normal(0, 1e-4, sh))
        return kw
    if kind == "undulator":
        return dict(length=u(0.1, 1.0))
    raise ValueError(kind)


def _amplification(desc, shape, energy):
    """Largest entry of the float64 composed map, energy carried through the cavities (NaN samples left out)."""
    _, specs = make_lattice(desc, np.float64)
    e = np.broadcast_to(np.asarray(energy, np.float64), shape).copy()
    M = np.broadcast_to(np.eye(7), (*shape, 7, 7)).copy()
    with np.errstate(all="ignore"):
        for spec in specs:
            if spec["kind"] == "cavity":
                T = o.cavity_rmatrix(spec, e, np.float64)
                gain = np.broadcast_to(spec["voltage"] * np.cos(np.deg2rad(spec["phase"])), shape)
                e = e + gain
            else:
                T = o.element_transfer_map(spec, e, np.float64)
            M = np.matmul(T, M)
    return float(np.nanmax(np.abs(np.where(np.isfinite(M), M, 0.0))))


def _float32_conditioned(desc, shape, energies, sigma):
    """
    Whether float32 can be held to 1e-4 on this lattice at all: a ParameterBeam of the case's sizes through the oracle's
    float32 chain (the product's arithmetic) and its float64 chain, every mu and diagonal cov entry but cov[4,4] within
    CONDITION_F32 of its scale (NaN samples left out).  Random lattices exist on which the oracle's own float32 chain is
    1e-4 .. 1e-3 away from float64 in mu_s, mu_p or sigma_s with every map entry below 1e2: no float32 evaluation can
    be compared at 1e-4 there, so such a draw is drawn again, like one that amplifies too much.
    """
    kw = dict(sigma_x=sigma[0], sigma_xp=sigma[1], sigma_y=sigma[2], sigma_yp=sigma[3], sigma_s=sigma[4], sigma_p=sigma[5])
    out = []
    for dt in (np.float32, np.float64):
        _, specs = make_lattice(desc, dt)
        up = (lambda v: v) if dt == np.float32 else (lambda v: np.asarray(v, np.float32).astype(np.float64))
        if dt == np.float64:
            _, specs = make_lattice([(k, {a: (up(v) if isinstance(v, np.ndarray) else v) for a, v in kwd.items()})
                                     for k, kwd in desc], np.float64)
        pb = o.parameter_beam_from_parameters(dtype=dt, **{k: np.full(shape, v) for k, v in kw.items()},
                                              energy=np.asarray(np.asarray(energies, np.float32), dt))
        with np.errstate(all="ignore"):
            out.append(o.segment_track(specs, pb, dt, kick="product", compose="float64"))
    (r32, r64) = out
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.abs(np.einsum("...ii->...i", r64["cov"][..., :6, :6])))
        dmu = np.abs(r32["mu"][..., :6] - r64["mu"][..., :6]) / (np.abs(r64["mu"][..., :6]) + sig)
        dcov = np.abs(np.einsum("...ii->...i", r32["cov"][..., :6, :6] - r64["cov"][..., :6, :6])) / sig**2
        dcov[..., 4] = 0  # (cov[4,4] behind a cavity: the reference's cancelling second-order sum, _check_parameter)
    worst = max(np.nanmax(np.nan_to_num(dmu, nan=0.0)), np.nanmax(np.nan_to_num(dcov, nan=0.0)))
    return worst <= CONDITION_F32


def draw_case(seed, i):
    rng = np.random.default_rng([seed, i])
    dtype = [np.float32, np.float64][i % 2]
    shape = SHAPES[rng.integers(len(SHAPES))]
    B = int(np.prod(shape))
    long_f32 = i == LONG_F32_CASE  # (float32 past kBuildChunk and kMaxUnits = 64: one case always is)
    L = int(rng.integers(65, 71)) if long_f32 else int(rng.integers(1, 71))
    fits = [n for n in COUNTS if B * n * L <= STEP_BUDGET]
    while not fits:
        L = max(1, L // 2)
        fits = [n for n in COUNTS if B * n * L <= STEP_BUDGET]
    n = int(fits[rng.integers(len(fits))])
    energy = float(np.exp(rng.uniform(np.log(6e6), np.log(1e9))))
    energies = energy * rng.uniform(0.9, 1.1, shape)
    beam = rng.choice(["particle", "shared", "parameter"], p=[0.5, 0.2, 0.3])
    sigma = [1e-4, 1e-5, 1e-4, 1e-5, rng.choice([1e-5, 1e-4]), 1e-3]
    # a lattice whose float64 map amplifies more than this is drawn again: float32 comparisons would not mean anything.
    # A float32 ParameterBeam's covariance goes with the SQUARE of the map (T C T^T): there 1e2 (measured: entries
    # 1.3e-4 .. 2.4e-4 of their scale from the float64 chain at amplifications 139 and 246, float32 rounding of the maps)
    bound = 1e2 if beam == "parameter" and dtype == np.float32 else 1e3
    # Drawing always ends: long random lattices are seldom well conditioned, so every ten failed draws the lattice gets
    # shorter (the long float32 case keeps its length and narrows its kinds instead), after thirty the all-kinds prefix
    # is dropped, and after sixty a lattice of drifts and markers -- conditioned by construction -- stands in.
    kinds_of = KINDS
    for attempt in range(61):
        if attempt and attempt % 10 == 0:
            if long_f32:
                kinds_of = ["drift", "quadrupole", "hcor", "vcor", "marker", "bpm", "solenoid", "undulator"]
            else:
                L = max(1, L // 2)
        drawn = dict(active_bpms=0, cavity_off=False)
        kinds = [kinds_of[k] for k in rng.integers(len(kinds_of), size=L)]
        if i % 6 == 0 and attempt < 30:  # every kind in the lattice at least once
            kinds = (KINDS + kinds)[:max(L, len(KINDS))]
        if attempt == 60:
            kinds = ["drift" if k % 2 == 0 else "marker" for k in range(L)]
        desc = [(kind, _element(rng, kind, shape, drawn)) for kind in kinds]
        if _amplification(desc, shape, energies) <= bound and (
                dtype == np.float64 or _float32_conditioned(desc, shape, energies, sigma)):
            break
    else:
        raise AssertionError(f"case {i}: drifts and markers out of bounds")  # (cannot happen: see above)
    pattern = rng.choice(["one", "three", "write"])
    read_between = bool(rng.random() < 0.5)
    knob = KNOBS[rng.integers(len(KNOBS))] if rng.random() < 0.25 else None
    if beam == "shared":
        energies = np.full(shape, energy)
    mu = rng.normal(0, 1, 6) * np.array([1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-4])
    write = int(rng.integers(1 << 30))
    tag = "-".join(f"{k}={v}" for k, v in knob.items()) if knob else ""
    cid = (f"c{i:02d}-{'f32' if dtype == np.float32 else 'f64'}-B{'x'.join(map(str, shape))}-N{n}-E{len(desc)}-{beam}-"
           f"{pattern}{'-read' if read_between else ''}{'-' + tag if tag else ''}")
    return dict(id=cid, i=i, dtype=dtype, shape=shape, n=n, desc=desc, energies=energies, beam=beam, pattern=pattern,
                read_between=read_between, knob=knob, sigma=sigma, mu=mu, write_seed=write, bound=bound)


CASES = [draw_case(SEED, i) for i in range(N_CASES)]


def test_the_oracle_budget_and_the_coverage_of_the_draws():
    """
    What the oracle is asked to do (<= 3e8 particle-element steps in all, at any seed) and the lattices past 64 elements
    in both precisions (LONG_F32_CASE); at the committed seed, also what the draws cover.
    """
    steps = sum(int(np.prod(c["shape"])) * c["n"] * len(c["desc"]) * (2 if c["pattern"] == "write" else 1) for c in CASES)
    print(f"oracle: {steps:.3g} particle-element steps over {len(CASES)} cases")
    assert steps <= 3e8
    assert CASES[LONG_F32_CASE]["dtype"] == np.float32 and len(CASES[LONG_F32_CASE]["desc"]) > 64
    if SEED != DEFAULT_SEED:
        return
    assert max(len(c["desc"]) for c in CASES if c["dtype"] == np.float64) > 64
    assert {kind for c in CASES for kind, _ in c["desc"]} == set(KINDS)
    assert {c["beam"] for c in CASES} == {"particle", "shared", "parameter"}
    assert {c["pattern"] for c in CASES} == {"one", "three", "write"}
    assert sum(c["knob"] is not None for c in CASES) >= 4


# ---------------------------------------------------------------------------------------------------------------------
# checking
# ---------------------------------------------------------------------------------------------------------------------


def _has_cavity(desc):
    return any(kind == "cavity" and np.any(np.asarray(kw["voltage"]) != 0) for kind, kw in desc)


def _oracle(case, desc, P=None, pkw=None):
    """
    The chains a case is held to: the oracle with the product's arithmetic where the product deviates from a literal
    reading on purpose ((i) runs composed in float64, (v) the float32 kick's form) and, for float32
    with an active cavity, the float64 chain next to it.
    """
    dtype, shape = case["dtype"], case["shape"]
    _, specs = make_lattice(desc, dtype)
    e = np.asarray(case["energies"], dtype=dtype)
    readings = []
    if P is not None:
        beam = o.particle_beam(np.broadcast_to(P, (*shape, *P.shape[-2:])), e, dtype)
    else:
        beam = o.parameter_beam_from_parameters(dtype=dtype, **pkw, energy=e)
    ref = o.segment_track(specs, beam, dtype, bpm_readings=readings, kick="product", compose="float64")
    ref["readings"] = readings
    if dtype == np.float32 and _has_cavity(desc):
        up = lambda v: np.asarray(v, np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v  # noqa: E731
        _, specs64 = make_lattice([(kind, {k: up(v) for k, v in kw.items()}) for kind, kw in desc], np.float64)
        b64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in beam.items()}
        ref["float64_chain"] = o.segment_track(specs64, b64, np.float64)
    return ref


def _moment_check(out, ref, dtype, n, what):
    """All 14 moments at TOL_MOM (NaN patterns equal); float32 behind a cavity: the kick's moments against float64 too."""
    m = o.beam_moments(ref, ddof=1)
    keys = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
            "sigma_p", "sigma_xxp", "sigma_yyp")
    got = {k: np.asarray(getattr(out, k), dtype=np.float64) for k in keys}
    for k in keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(m[k])), (what, k, "NaN pattern")
    if n < 2:  # one particle: no spread to measure the means by, the sigmas are NaN (unbiased) on both sides
        for k in keys[:6]:
            assert rel_err(got[k], m[k]) <= TOL_P[dtype], (what, k)
        return

    def dist(vals, mm, k):
        if k.startswith("mu_"):
            s = np.abs(mm[k]) + mm["sigma" + k[2:]]
        elif k in ("sigma_xxp", "sigma_yyp"):
            s = mm["sigma_x"] * mm["sigma_xp"] if k == "sigma_xxp" else mm["sigma_y"] * mm["sigma_yp"]
        else:
            s = mm[k]
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(vals[k], dtype=np.float64) - np.asarray(mm[k], dtype=np.float64)) / s
        return float(np.nanmax(d)) if np.any(np.isfinite(d)) else 0.0

    d = {k: dist(got, m, k) for k in keys}
    assert max(d.values()) <= TOL_MOM[dtype], (what, d)
    if "float64_chain" in ref:
        # the moments the kick decides, against the float64 chain: within TOL_KICK_F64, or -- where float32 maps of a
        # random lattice (dipoles' R56, ...) put the oracle's own float32 chain farther away -- no farther than twice that
        m64 = o.beam_moments(ref["float64_chain"], ddof=1)
        for k in KICK_MOMENTS:
            d_gpu, d_own = dist(got, m64, k), dist(m, m64, k)
            assert d_gpu <= max(TOL_KICK_F64, 2 * d_own), (what, k, d_gpu, d_own)


def _check_particles(case, out, ref, elements, what):
    dtype = case["dtype"]
    got = np.asarray(out.particles)
    assert got.shape == ref["particles"].shape, what
    for c in range(7):
        err = rel_err(got[..., c], ref["particles"][..., c])
        assert err < TOL_P[dtype], (what, c, err)
    assert rel_err(out.energy, ref["energy"]) < 1e-6, what
    _moment_check(out, ref, dtype, case["n"], what)


def _check_readings(case, elements, desc, ref, what):
    dtype = case["dtype"]
    active = [e for e, (kind, kw) in enumerate(desc) if kind == "bpm" and kw.get("is_active")]
    assert len(ref["readings"]) == len(active), what  # (in lattice order; the oracle's index is list.index's)
    sig = np.array([case["sigma"][0], case["sigma"][2]])
    for e, (_, want) in zip(active, ref["readings"]):
        got = np.asarray(elements[e].reading, dtype=np.float64)
        assert got.shape == want.shape, (what, e)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, e)
        scale = np.abs(want) + sig.reshape(2, *([1] * (want.ndim - 1)))
        with np.errstate(invalid="ignore"):
            assert np.all(np.nan_to_num(np.abs(got - want) / scale) <= TOL_MOM[dtype]), (what, e, got, want)


def _check_parameter(case, out, ref, what):
    """
    mu and cov entry by entry (helpers.assert_parameter_beam).  float32 behind an active cavity: mu_s and mu_p also
    against the float64 chain (as for the particles' moments); and the covariance against the FLOAT64 chain, every entry
    within 1e-4 of its scale plus twice the oracle's own float32 distance there.  The reference overwrites the s row with
    T566 c55^2 + T556 c45 c55 + T555 c44^2 (cavity.py:207-218), which cancels: in float32 that entry is 2e-4 .. 2e-3 of
    itself away from float64 in the oracle as in the product, and the maps behind the cavity carry the difference into
    other entries.  An open finding, not a property of one chain or the other.
    """
    dtype = case["dtype"]
    mu, cov = np.asarray(out._mu, np.float64), np.asarray(out._cov, np.float64)
    if "float64_chain" in ref:
        r64, r32 = ref["float64_chain"], np.asarray(ref["cov"], np.float64)
        c64 = np.asarray(r64["cov"], np.float64)
        assert np.array_equal(np.isnan(cov), np.isnan(c64)), what
        sig = np.sqrt(np.abs(np.einsum("...ii->...i", c64[..., :6, :6])))
        scale = np.maximum(sig[..., :, None] * sig[..., None, :], np.abs(c64[..., :6, :6]))
        with np.errstate(invalid="ignore"):
            bad = np.abs(cov - c64)[..., :6, :6] > TOL_PB[dtype] * scale + 2 * np.abs(r32 - c64)[..., :6, :6]
        assert not np.any(bad), (what, "cov", [tuple(int(v) for v in i) for i in np.argwhere(bad)[:3]])
        sig32 = np.sqrt(np.abs(np.einsum("...ii->...i", r32[..., :6, :6])))
        with np.errstate(all="ignore"):
            d = np.nan_to_num(np.abs(mu[..., 4:6] - r64["mu"][..., 4:6]) / (np.abs(r64["mu"][..., 4:6]) + sig[..., 4:6]))
            d_own = np.nan_to_num(np.abs(ref["mu"][..., 4:6] - r64["mu"][..., 4:6]) / (np.abs(r64["mu"][..., 4:6]) + sig32[..., 4:6]))
        assert np.all(d <= np.maximum(TOL_KICK_F64, 2 * d_own)), (what, float(np.max(d)), float(np.max(d_own)))
        cov = r32  # (mu against the product chain below; the covariance was checked above)
    assert_parameter_beam((mu, cov), ref, TOL_PB[dtype], what)
    assert rel_err(out.energy, ref["energy"]) < 1e-6, what


def _written(case, desc):
    """The attribute write of the "write" pattern: (element index, name, new value) and the lattice after it."""
    rng = np.random.default_rng(case["write_seed"])
    shape = case["shape"]
    options = [(e, name) for e, (kind, kw) in enumerate(desc)
               for name in {"quadrupole": ["k1", "tilt"], "hcor": ["angle"], "vcor": ["angle"], "drift": ["length"],
                            "cavity": ["voltage", "phase"], "dipole": ["angle"], "solenoid": ["k"]}.get(kind, [])]
    if not options:
        return None, desc
    e, name = options[rng.integers(len(options))]
    kind, kw = desc[e]
    value = {"k1": lambda: rng.uniform(-5, 5, shape), "tilt": lambda: rng.uniform(-0.5, 0.5, shape),
             "angle": lambda: rng.normal(0, 1e-3, shape) if kind != "dipole" else rng.uniform(-0.1, 0.1, shape),
             "length": lambda: rng.uniform(0, 1, shape), "voltage": lambda: rng.uniform(1e6, 2e7, shape),
             "phase": lambda: rng.uniform(-20, 20, shape), "k": lambda: rng.uniform(-2, 2, shape)}[name]()
    if name in kw and np.size(kw[name]) == 1 and value.size > 1:  # a broadcast parameter stays broadcast
        value = value.reshape(-1)[:1]
    if name not in kw and np.size(kw.get("length", value)) == 1:
        value = value.reshape(-1)[:1]
    after = list(desc)
    after[e] = (kind, {**kw, name: value})
    if _amplification(after, shape, case["energies"]) > case["bound"] or (
            case["dtype"] == np.float32 and not _float32_conditioned(after, shape, case["energies"], case["sigma"])):
        return None, desc
    return (e, name, value), after


def _run(lx, case, what):
    """One pass of the case's call pattern on a fresh Segment: every result against the oracle."""
    dtype, shape, n = case["dtype"], case["shape"], case["n"]
    desc = case["desc"]
    elements, _ = make_lattice(desc, dtype, lx)
    seg = lx.Segment(elements)
    e = np.asarray(case["energies"], dtype=dtype)
    P = pkw = None
    if case["beam"] == "parameter":
        pkw = dict(mu_x=np.full(shape, case["mu"][0]), mu_y=np.full(shape, case["mu"][2]),
                   sigma_x=np.full(shape, case["sigma"][0]), sigma_xp=np.full(shape, case["sigma"][1]),
                   sigma_y=np.full(shape, case["sigma"][2]), sigma_yp=np.full(shape, case["sigma"][3]),
                   sigma_s=np.full(shape, case["sigma"][4]), sigma_p=np.full(shape, case["sigma"][5]))
        pkw = {k: v.astype(dtype) for k, v in pkw.items()}
        beam = lx.ParameterBeam.from_parameters(**pkw, energy=e, dtype=dtype)
    elif case["beam"] == "shared":
        P = o.gaussian_particles((1,), n, seed=case["i"], dtype=dtype, mu=case["mu"], sigma=case["sigma"])
        beam = lx.ParticleBeam(P, np.asarray(e.reshape(-1)[:1]), dtype=dtype).broadcast(shape)
        assert beam.is_shared
    else:
        P = o.gaussian_particles(shape, n, seed=case["i"], dtype=dtype, mu=case["mu"], sigma=case["sigma"])
        beam = lx.ParticleBeam(P, e, dtype=dtype)

    def check(out, lattice_desc, label):
        ref = _oracle(case, lattice_desc, P=P, pkw=pkw)
        if case["beam"] == "parameter":
            _check_parameter(case, out, ref, f"{what}/{label}")
        else:
            _check_particles(case, out, ref, elements, f"{what}/{label}")
        return ref

    def peek(out):
        if case["read_between"]:
            np.asarray(out.energy)  # the host waits: the next call may take the short-call inline path

    if case["pattern"] == "one":
        out = seg.track(beam)
        ref = check(out, desc, "one")
        if case["beam"] != "parameter":
            _check_readings(case, elements, desc, ref, what)
    elif case["pattern"] == "three":
        outs = []
        for _ in range(3):
            outs.append(seg.track(beam))
            peek(outs[-1])
        ref = check(outs[0], desc, "call 0")
        if case["beam"] != "parameter":
            _check_readings(case, elements, desc, ref, what)
            first = np.asarray(outs[0].particles)
            for k in (1, 2):  # same input, same lattice: the same bits
                assert np.array_equal(np.asarray(outs[k].particles), first, equal_nan=True), (what, k)
                assert np.array_equal(outs[k].moment_record(), outs[0].moment_record(), equal_nan=True), (what, k)
        else:
            for k in (1, 2):
                assert np.array_equal(np.asarray(outs[k]._mu), np.asarray(outs[0]._mu), equal_nan=True), (what, k)
                assert np.array_equal(np.asarray(outs[k]._cov), np.asarray(outs[0]._cov), equal_nan=True), (what, k)
    else:
        change, after = _written(case, desc)
        first = seg.track(beam)
        peek(first)
        if change is not None:
            idx, name, value = change
            setattr(elements[idx], name, np.asarray(value, dtype=dtype))
        second = seg.track(beam)
        check(first, desc, "before the write")
        check(second, after, "after the write")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_random_case_against_the_oracle(lx, monkeypatch, case):
    _run(lx, case, "default")
    if case["knob"]:
        for key, value in case["knob"].items():
            monkeypatch.setenv(key, value)
        _run(lx, case, f"knob {case['knob']}")


# ---------------------------------------------------------------------------------------------------------------------
# random call sequences through the reverse pass
# ---------------------------------------------------------------------------------------------------------------------

GRAD_PARAMS = {"drift": ["length"], "quadrupole": ["k1", "misalignment"], "hcor": ["angle"], "vcor": ["angle"],
               "cavity": ["voltage", "phase"], "dipole": ["angle"]}


def _grad_segment(rng, B):
    desc = []
    for _ in range(int(rng.integers(2, 6))):
        desc += [("drift", dict(length=rng.uniform(0.1, 0.6, B))),
                 ("quadrupole", dict(length=rng.uniform(0.05, 0.3, B), k1=rng.uniform(-5, 5, B),
                                     misalignment=rng.normal(0, 1e-4, (B, 2)))),
                 ("hcor", dict(length=rng.uniform(0.0, 0.2, B), angle=rng.normal(0, 1e-3, B)))]
        if rng.random() < 0.5:
            desc.append(("cavity", dict(length=rng.uniform(0.5, 1.5, B), voltage=rng.uniform(5e6, 2e7, B),
                                        phase=rng.uniform(-10, 10, B), frequency=np.full(B, 1.3e9))))
        if rng.random() < 0.3:
            desc.append(("dipole", dict(length=rng.uniform(0.2, 0.5, B), angle=rng.uniform(-0.1, 0.1, B))))
        if rng.random() < 0.3:
            desc.append(("vcor", dict(length=rng.uniform(0.0, 0.2, B), angle=rng.normal(0, 1e-3, B))))
    return desc


def draw_program(seed, j):
    rng = np.random.default_rng([seed, 1000 + j])
    dtype = [np.float32, np.float64][j % 2]
    B = int(rng.choice([1, 3, 64]))
    n = int(rng.choice([257, 1000, 2000, 4097] if B < 64 and dtype == np.float32 else [257, 1000]))
    segs = [_grad_segment(rng, B) for _ in range(3)]
    ops = list(rng.choice(["track", "vjp_now", "vjp_later", "backward", "write", "parameter", "read"], size=30,
                          p=[0.2, 0.2, 0.15, 0.15, 0.15, 0.1, 0.05]))
    ops[0] = "vjp_now"  # (at least one gradient whose forward and reverse halves saw the same parameters)
    ops += ["backward"] * 4  # (what is still pending after these runs at the end of the test)
    picks = rng.integers(0, 1 << 30, size=len(ops))
    cid = f"p{j}-{'f32' if dtype == np.float32 else 'f64'}-B{B}-N{n}-E{'.'.join(str(len(s)) for s in segs)}"
    return dict(id=cid, j=j, dtype=dtype, B=B, n=n, segs=segs, ops=ops, picks=picks)


PROGRAMS = [draw_program(SEED, j) for j in range(N_PROGRAMS)]


def _snapshot(elements, desc):
    return [{name: np.asarray(getattr(el, name)).copy() for name in GRAD_PARAMS.get(kind, []) + (["length"] if kind != "drift" else [])
             if getattr(el, name, None) is not None} for el, (kind, _) in zip(elements, desc)]


def _restore(elements, snap):
    for el, values in zip(elements, snap):
        for name, v in values.items():
            if not np.array_equal(np.asarray(getattr(el, name)), v):
                setattr(el, name, v)


def _desc_at(desc, snap):
    return [(kind, {**kw, **{k: np.asarray(v) for k, v in values.items()}}) for (kind, kw), values in zip(desc, snap)]


def _flat(g, elements, desc):
    out = [np.asarray(g.energy)]
    for el, (kind, _) in zip(elements, desc):
        out += [np.asarray(g[el][name]) for name in GRAD_PARAMS.get(kind, []) if getattr(el, name, None) is not None]
    return out


def _loss64(desc, P, energy, w_mu, w_cov):
    _, specs = make_lattice(desc, np.float64)
    out = o.segment_track(specs, o.particle_beam(P, energy, np.float64), np.float64)
    Q = out["particles"][..., :6]
    mu = Q.mean(axis=-2)
    d = Q - mu[..., None, :]
    cov = np.einsum("...ni,...nj->...ij", d, d) / Q.shape[-2]
    return np.sum(w_mu * mu, axis=-1) + np.sum(w_cov * cov, axis=(-1, -2))


@pytest.mark.parametrize("prog", PROGRAMS, ids=[p["id"] for p in PROGRAMS])
def test_random_call_sequence_through_the_reverse_pass(lx, monkeypatch, prog):
    """
    About 30 operations over three segments and two beams: forward tracks, track_vjp with its backward call at once or
    later, parameter writes, ParameterBeam tracks, read-backs.  Every forward result against the oracle; afterwards
    every gradient recomputed from the recorded parameter values with LYNX_BWD_REUSE_TABLE=0 -- bit for bit; float64
    with <= 2000 particles: two parameter gradients per program against central differences of the float64 oracle.
    """
    dtype, B, n = prog["dtype"], prog["B"], prog["n"]
    built = [make_lattice(desc, dtype, lx) for desc in prog["segs"]]
    segs = [lx.Segment(elements) for elements, _ in built]
    energies = [np.full(B, 6e6 * (1 + k), dtype=dtype) for k in range(2)]
    Ps = [o.gaussian_particles((B,), n, seed=100 * prog["j"] + k, dtype=dtype,
                               sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3], mu=[1e-4, 0, -1e-4, 0, 0, 0]) for k in range(2)]
    beams = [lx.ParticleBeam(P, e, dtype=dtype) for P, e in zip(Ps, energies)]
    forwards, grads, pending = [], [], []
    for op, pick in zip(prog["ops"], prog["picks"]):
        rng = np.random.default_rng(int(pick))
        s, b = int(rng.integers(3)), int(rng.integers(2))
        elements, desc = built[s][0], prog["segs"][s]
        if op == "track":
            forwards.append(("particle", s, b, _snapshot(elements, desc), segs[s].track(beams[b])))
        elif op == "parameter":
            pb = lx.ParameterBeam.from_parameters(sigma_x=np.full(B, 1e-4, dtype), sigma_xp=np.full(B, 1e-5, dtype),
                                                  mu_x=np.full(B, 1e-4, dtype), energy=energies[b], dtype=dtype)
            forwards.append(("parameter", s, b, _snapshot(elements, desc), segs[s].track(pb)))
        elif op in ("vjp_now", "vjp_later"):
            w_mu, w_cov = rng.normal(size=(B, 6)), rng.normal(size=(B, 6, 6)) * 1e3
            vjp = lx.grad.track_vjp(segs[s], beams[b])
            entry = dict(s=s, b=b, fwd=_snapshot(elements, desc), w_mu=w_mu, w_cov=w_cov, vjp=vjp)
            forwards.append(("particle", s, b, entry["fwd"], vjp.outgoing))
            if op == "vjp_now":
                entry["bwd"] = entry["fwd"]
                entry["g"] = _flat(vjp(mu_bar=w_mu, cov_bar=w_cov), elements, desc)
                grads.append(entry)
            else:
                pending.append(entry)
        elif op == "backward" and pending:
            entry = pending.pop(int(rng.integers(len(pending))))
            el2, desc2 = built[entry["s"]][0], prog["segs"][entry["s"]]
            entry["bwd"] = _snapshot(el2, desc2)
            entry["g"] = _flat(entry["vjp"](mu_bar=entry["w_mu"], cov_bar=entry["w_cov"]), el2, desc2)
            grads.append(entry)
        elif op == "write":
            options = [(e, name) for e, (kind, _) in enumerate(desc) for name in GRAD_PARAMS.get(kind, [])
                       if name not in ("misalignment", "length")]
            e, name = options[int(rng.integers(len(options)))]
            old = np.asarray(getattr(elements[e], name))
            setattr(elements[e], name, (old * rng.uniform(0.8, 1.2, old.shape)).astype(dtype))
        elif op == "read" and forwards:
            out = forwards[-1][-1]
            np.asarray(out.energy)
    # the backward halves still pending, in a seeded order
    rng = np.random.default_rng([SEED, 3000 + prog["j"]])
    for q in rng.permutation(len(pending)):
        entry = pending[q]
        el2, desc2 = built[entry["s"]][0], prog["segs"][entry["s"]]
        entry["bwd"] = _snapshot(el2, desc2)
        entry["g"] = _flat(entry["vjp"](mu_bar=entry["w_mu"], cov_bar=entry["w_cov"]), el2, desc2)
        grads.append(entry)
    pending.clear()
    # forward results against the oracle, at the parameters each call saw
    for kind, s, b, snap, out in forwards:
        desc = _desc_at(prog["segs"][s], snap)
        case = dict(dtype=dtype, shape=(B,), n=n, energies=energies[b], sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3])
        if kind == "particle":
            ref = _oracle(case, desc, P=Ps[b])
            _check_particles(case, out, ref, None, f"forward on segment {s}, beam {b}")
        else:
            pkw = dict(sigma_x=np.full(B, 1e-4, dtype), sigma_xp=np.full(B, 1e-5, dtype), mu_x=np.full(B, 1e-4, dtype))
            _check_parameter(case, out, _oracle(case, desc, pkw=pkw), f"ParameterBeam on segment {s}")
    # every gradient again, each reverse pass building its own table
    assert grads
    monkeypatch.setenv("LYNX_BWD_REUSE_TABLE", "0")
    for k, entry in enumerate(grads):
        elements, desc = built[entry["s"]][0], prog["segs"][entry["s"]]
        _restore(elements, entry["fwd"])
        vjp = lx.grad.track_vjp(segs[entry["s"]], beams[entry["b"]])
        _restore(elements, entry["bwd"])
        again = _flat(vjp(mu_bar=entry["w_mu"], cov_bar=entry["w_cov"]), elements, desc)
        for x, y in zip(entry["g"], again):
            assert np.array_equal(x, y, equal_nan=True), (k, entry["s"], entry["b"])
    # two parameter gradients against central differences of the float64 oracle
    if dtype != np.float64 or n > 2000:
        return
    rng = np.random.default_rng([SEED, 2000 + prog["j"]])
    same = [entry for entry in grads if all(np.array_equal(entry["fwd"][q][k], entry["bwd"][q][k])
                                            for q in range(len(entry["fwd"])) for k in entry["fwd"][q])]
    assert same
    entry = same[int(rng.integers(len(same)))]
    desc0 = _desc_at(prog["segs"][entry["s"]], entry["fwd"])
    elements = built[entry["s"]][0]
    names = [(e, name) for e, (kind, kw) in enumerate(desc0) for name in GRAD_PARAMS.get(kind, []) if name != "misalignment"]
    flat_index = {}
    pos = 1
    for e, (kind, _) in enumerate(desc0):
        for name in GRAD_PARAMS.get(kind, []):
            if getattr(elements[e], name, None) is not None:
                flat_index[(e, name)] = pos
                pos += 1
    P, energy = Ps[entry["b"]], energies[entry["b"]]
    for q in rng.choice(len(names), size=2, replace=False):
        e, name = names[q]
        bidx = int(rng.integers(B))
        x0 = float(np.asarray(desc0[e][1][name])[bidx])
        h = 1e-6 * max(abs(x0), 1e-2)
        loss = []
        for x in (x0 + h, x0 - h):
            kw = dict(desc0[e][1])
            kw[name] = np.asarray(kw[name], np.float64).copy()
            kw[name][bidx] = x
            d = list(desc0)
            d[e] = (desc0[e][0], kw)
            loss.append(_loss64(d, P, energy, entry["w_mu"], entry["w_cov"])[bidx])
        ref = (loss[0] - loss[1]) / (2 * h)
        got = float(entry["g"][flat_index[(e, name)]][bidx])
        scale = max(abs(ref), 1e-9 * np.max(np.abs(entry["w_cov"])))
        assert abs(got - ref) <= 2e-4 * scale + 1e-7 * np.max(np.abs(entry["g"][flat_index[(e, name)]])), (e, name, bidx, got, ref)
