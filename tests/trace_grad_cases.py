"""
Seeded random cases of the derivatives of the beam trace -- `track_along_vjp` in its modes and `track_along_jvp` -- with
references that do not come from the GPU: `reverse_reference.AffineReference` in its along forms (analytic, no step size).
This module holds no test and needs no GPU; tests/test_trace_grad_cases_host.py checks the references and the draws on the
host, tests/test_gpu_trace_grad_fuzz.py runs the cases.

Case i depends on (seed, i) only: LYNX_TRACE_FUZZ_SEED=<seed> and `-k a07-` replay one case.  Everything is drawn with a
NumPy Generator before anything reaches the GPU; nothing is retried or shrunk at run time.  What IS drawn again, here, from
the reference alone: a lattice whose float64 map amplifies beyond 1e2, a float32 lattice on which rounding the reference's
own maps and map derivatives to float32 moves a result by more than a tenth of the float32 bound (a condition on the inputs:
it leaves the product a factor of ten over the rounding of what it is given), and a losses case whose apertures keep less
than 10 % or more than 90 % of a sample or have a survivor within 1e-6 of an edge.

The schedule of a case is fixed by i: dtype i % 2, beam and mode (i // 2) % 4, batch shape (i // 8) % 4 -- every mode at
every batch shape in both precisions.  Lattice, parameters, structure (a parameter set given as (1,), an element object
placed twice, a nested Segment), particle counts, cotangents and directions are drawn.

Every value passes through `rr.f32`, so that the float32 lattice holds exactly the reference's numbers.
"""

import os
import time

import numpy as np

from oracle import lynx_oracle as o

from . import reverse_reference as rr
from . import trace_jvp_reference as jr
from .helpers import _some, build, criterion

DEFAULT_SEED = 20261021
SEED = int(os.environ.get("LYNX_TRACE_FUZZ_SEED") or DEFAULT_SEED)
N_AFFINE = 32
SHAPES = [(1,), (2,), (3,), (2, 2)]
MODES = ["parameters", "plain", "trajectories", "losses"]
KINDS = ["drift", "quadrupole", "dipole", "rbend", "hcor", "vcor", "solenoid", "undulator", "marker", "bpm", "custom"]
COUNTS = (1, 2, 63, 64, 65, 257, 400)
CHOSEN = (1, 3, 64, 65)
MAX_LEAVES = 16
MAX_DERIVATIVES = 300  # map derivatives per case (13 ms each at 30 digits: about 4 s)
AMPLIFICATION = 1e2  # no entry of the float64 composed map above this
CONDITION = 0.1  # of the float32 bound: how far rounding maps and derivatives to float32 may move a result


# ---------------------------------------------------------------------------------------------------------------------
# the survivors of a particle chain (from tests/test_gpu_trace_losses_grad.py, which imports them back)
# ---------------------------------------------------------------------------------------------------------------------


def _survivor_chain(desc, specs, particles, energy):
    """
    `element_track` element by element in float64 (an aperture is a marker there), `o.aperture_mask` on the particles
    that ENTER every active aperture: (beams at the P points, alive (P, *batch, N) bool, lost_at, the smallest distance of
    a particle still alive from an edge in the `criterion` measure).
    """
    beams = jr.chain(specs, o.particle_beam(particles, energy, np.float64))
    alive = np.ones(particles.shape[:-1], dtype=bool)
    lost_at = np.full(particles.shape[:-1], -1, dtype=np.int32)
    masks, margin, ordinal = [], np.inf, 0
    for k, (kind, kw) in enumerate(desc):
        masks.append(alive.copy())
        if kind == "aperture" and kw.get("is_active", True):
            keep = o.aperture_mask(beams[k]["particles"], kw["x_max"], kw["y_max"], kw["shape"])
            crit = criterion(beams[k]["particles"], kw["x_max"], kw["y_max"], kw["shape"])
            margin = min(margin, float(np.min(np.abs(crit - 1.0)[:, alive]))) if alive.any() else margin
            lost_at[alive & ~keep] = ordinal
            alive = alive & keep
            ordinal += 1
    masks.append(alive.copy())
    return beams, np.array(masks), lost_at, margin


def _moments_of(q, alive):
    """Mean (*batch, 6) and biased covariance (*batch, 6, 6) of the particles `alive` (*batch, N) marks, in float64."""
    w = alive[..., None].astype(np.float64)
    n = alive.sum(axis=-1)[..., None]
    mean = (q * w).sum(axis=-2) / n
    d = (q - mean[..., None, :]) * w
    return mean, np.einsum("...ni,...nj->...ij", d, d) / n[..., None]


def _sized_apertures(desc, particles, energy, places, fractions):
    """
    `desc` with an active aperture in front of each element `places` names (indices into `desc`), rectangular and
    elliptical in turn along the lattice; the limits of each are its fraction of `fractions` times the rms sizes of the
    particles still alive where it stands (the apertures in front of it sized, the ones behind it open).
    """
    out = list(desc)
    for place in sorted(places, reverse=True):
        out.insert(place, ("aperture", None))
    order = [k for k, (kind, _) in enumerate(out) if kind == "aperture"]
    for count, (k, fraction) in enumerate(zip(order, fractions)):
        so_far = [("marker", {}) if kw is None else (kind, kw) for kind, kw in out]
        _, specs = build(so_far, np.float64)
        beams, masks, _, _ = _survivor_chain(so_far, specs, particles, energy)
        _, cov = _moments_of(beams[k]["particles"][..., :6], masks[k])
        out[k] = ("aperture", dict(x_max=fraction * np.sqrt(cov[..., 0, 0]), y_max=fraction * np.sqrt(cov[..., 2, 2]),
                                   shape=("rectangular", "elliptical")[count % 2]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# drawing an affine lattice
# ---------------------------------------------------------------------------------------------------------------------


def _element(rng, kind, B, drawn):
    """One element's keyword arguments, every parameter (B,)-shaped ((B, 2) misalignments) and a float32 number."""
    u = lambda lo, hi, *tail: rr.f32(rng.uniform(lo, hi, (B, *tail)))  # noqa: E731
    if kind == "drift":
        return dict(length=u(0.1, 0.6))
    if kind == "quadrupole":
        k1 = u(1.0, 4.0) * rng.choice([-1.0, 1.0], B)
        if B > 1 and rng.random() < 0.3:
            k1[rng.integers(B)] = 0.0  # drift-like in ONE sample: the duals' series branch next to the closed form
        kw = dict(length=u(0.1, 0.3), k1=k1)
        if rng.random() < 0.5:  # whole-batch predicates that only some samples take
            kw["tilt"] = rr.f32(_some(rng, (B,), lambda sh: rng.uniform(0.05, 0.5, sh)))
        if rng.random() < 0.5:
            kw["misalignment"] = rr.f32(_some(rng, (B, 2), lambda sh: rng.normal(0, 1e-3, sh)))
        return kw
    if kind in ("dipole", "rbend"):
        thin = kind == "dipole" and drawn["thin"]
        return dict(length=np.zeros(B) if thin else u(0.2, 0.5), angle=u(0.01, 0.05) if thin else u(0.02, 0.2), e1=u(-0.05, 0.05),
                    e2=u(-0.05, 0.05), fringe_integral=u(0.3, 0.5), fringe_integral_exit=u(0.3, 0.5), gap=u(0.01, 0.03),
                    tilt=u(-0.3, 0.3))
    if kind in ("hcor", "vcor"):
        return dict(length=rr.f32(_some(rng, (B,), lambda sh: rng.uniform(0.05, 0.2, sh), p=0.7)), angle=rr.f32(rng.normal(0, 1e-3, B)))
    if kind == "solenoid":
        kw = dict(length=u(0.1, 0.3), k=u(0.2, 2.0))
        if rng.random() < 0.6:
            kw["misalignment"] = rr.f32(_some(rng, (B, 2), lambda sh: rng.normal(0, 1e-3, sh)))
        return kw
    if kind == "undulator":
        return dict(length=u(0.1, 0.4))
    if kind == "marker":
        return {}
    if kind == "bpm":
        on = drawn["active_bpms"] < 2 and rng.random() < 0.6
        drawn["active_bpms"] += on
        return dict(is_active=bool(on))
    if kind == "custom":  # no differentiable parameter: passed through
        tm = np.broadcast_to(np.eye(7), (B, 7, 7)).copy()
        tm[:, :6, :6] += rng.normal(0, 1e-2, (B, 6, 6))
        tm[:, :6, 6] = rng.normal(0, 1e-5, (B, 6))
        return dict(transfer_map=rr.f32(tm))
    raise ValueError(kind)


def _shared(kw):
    """The element's parameters with sample 0's values in every sample: what a parameter set given as (1,) means."""
    return {k: (np.repeat(v[:1], len(v), axis=0) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def derivative_count(desc, energy):
    """How many map derivatives `AffineReference.dmaps` evaluates for `desc`: equal rows (shared, placed twice) count once."""
    keys, B = set(), len(energy)
    for kind, kw in desc:
        if kind not in rr.KIND:
            continue
        for b in range(B):
            hk, flags, row = rr.element_row(kind, kw, b, B)
            slots, slot = [len(row)], 0
            for name in rr.ROW[kind]:
                if name is None:
                    continue
                width = 2 if name == "misalignment" else 1
                if kw.get(name) is not None:
                    slots += list(range(slot, slot + width))
                slot += width
            keys |= {(kind == "rbend" and s == 1, hk, flags, tuple(row), float(energy[b]), s) for s in slots}
    return len(keys)


def _draw_lattice(rng, i, B, L, attempt):
    """(desc of leaves, shared leaves, (first, second place) or None, (a, b) of the nested run or None)."""
    drawn = dict(active_bpms=0, thin=bool(rng.random() < 0.3))
    if attempt >= 60:  # the stand-in: conditioned by construction
        f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
        return [("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.1), k1=rr.f32(rng.uniform(0.5, 2.0, B)))),
                ("hcor", dict(length=f(0.1), angle=rr.f32(rng.normal(0, 1e-3, B))))], set(), None, None
    kinds = [KINDS[k] for k in rng.integers(len(KINDS), size=L)]
    if i % 4 == 0 and attempt < 30:  # every kind at least once
        kinds = (KINDS + kinds)[:max(L, len(KINDS))]
    desc = [(kind, _element(rng, kind, B, drawn)) for kind in kinds]
    shared, twice, nested = set(), None, None
    rows = [e for e, (kind, _) in enumerate(desc) if kind in rr.KIND]
    if rows and rng.random() < 0.3:
        e = int(rng.choice(rows))
        desc[e] = (desc[e][0], _shared(desc[e][1]))
        shared = {e}
    if rows and len(desc) < MAX_LEAVES and rng.random() < 0.3:
        e = int(rng.choice(rows))
        at = int(rng.integers(e + 1, len(desc) + 1))
        desc.insert(at, desc[e])  # the SAME description: one element object at two leaves
        twice = (e, at)
        shared = {s + (s >= at) for s in shared}  # (the leaves from `at` on move up)
        if e in shared:
            shared = {e, at}
    if len(desc) >= 2 and rng.random() < 0.3:
        a = int(rng.integers(0, len(desc) - 1))
        nested = (a, int(rng.integers(a + 1, len(desc) + 1)))
    return desc, shared, twice, nested


def _cut(desc, shared, twice, nested, length):
    """The first `length` leaves, with what is left of the structure."""
    desc = desc[:length]
    shared = {e for e in shared if e < length}
    twice = twice if twice is not None and twice[1] < length else None
    nested = None if nested is None or nested[0] >= length else (nested[0], min(nested[1], length))
    return desc, shared, twice, nested


def _amplification(maps):
    M = np.broadcast_to(np.eye(7), maps[0].shape).copy()
    for T in maps:
        M = T @ M
    return float(np.max(np.abs(M)))


# ---------------------------------------------------------------------------------------------------------------------
# a case's reference, in the product's keys
# ---------------------------------------------------------------------------------------------------------------------


def reference_desc(desc, floor=True):
    """
    The lattice as `AffineReference` takes it: an aperture is a marker of the chain, and a quadrupole's k1 = 0 is the 1e-12
    that the modelled project tracks with (track_methods.py:67-68: `k1[k1 == 0] = 1e-12`), and with it the oracle and the
    product -- hp_maps.py differentiates a quadrupole at the k1 it is given.  The difference shows where nothing else does:
    along the misalignment of such a sample the mean's tangent is 1e-12 L, not 0.
    """
    out = []
    for kind, kw in desc:
        if kind == "aperture":
            kind, kw = "marker", {}
        elif kind == "quadrupole" and np.any(kw["k1"] == 0) and floor:
            kw = {**kw, "k1": np.where(kw["k1"] == 0, 1e-12, kw["k1"])}
        out.append((kind, kw))
    return out


def floor_error(case, tangents):
    """
    [(mu (B,), cov (B,))] per direction: how far the floor moves the reference's tangents, per sample -- the largest entry of
    |tangent at k1 = 1e-12 - tangent at k1 = 0|.  It is the size of what the floor alone puts into a sample whose tangent is
    otherwise an exact zero (1e-12 L along a misalignment), an artefact of the model that float32 cannot follow -- the map's
    entry is 1 - 1e-14 -- and that the reference, which could be evaluated on either side of it, does not pin down: it is
    taken off |got - ref| like a reference's rounding.  Zero in every sample whose k1 is not 0.
    """
    B = case["B"]
    if not any(kind == "quadrupole" and np.any(kw["k1"] == 0) for kind, kw in case["desc"]):
        return [(np.zeros(B), np.zeros(B)) for _ in tangents]
    limit = rr.AffineReference(reference_desc(case["desc"], floor=False), case["energy"])
    out = []
    for (label, mu_dot, cov_dot), (_, direction) in zip(tangents, directions_of(case, limit)):
        if case["mode"] == "parameters":
            other = limit.parameter_tangents(case["mu"], case["cov"], direction)
        else:
            other = limit.particle_tangents(case["particles"], direction)
        out.append(tuple(np.max(np.abs(a - b).reshape(B, -1), axis=1) for a, b in zip((mu_dot, cov_dot), other)))
    return out


def combine(case, raw):
    """
    The host-side rules, applied to a reference {(e, name) | "energy" | ...: (B, ...)}: an element object placed at several
    leaves gets the sum over its places (under its first leaf), a parameter given as (1,) the sum over the samples, and
    every array the batch shape of the case.
    """
    shape, twice, shared = case["shape"], case["twice"], case["shared"]
    out = dict(raw)
    if twice is not None:
        for key in [k for k in out if isinstance(k, tuple) and k[0] == twice[1]]:
            out[(twice[0], key[1])] = out[(twice[0], key[1])] + out.pop(key)
    for key, value in out.items():
        if isinstance(key, tuple) and key[0] in shared:
            out[key] = value.sum(axis=0, keepdims=True)
        else:
            out[key] = value.reshape(*shape, *value.shape[1:])
    return out


def directions_of(case, reference):
    """[(label, [(leaf, name, component, weight)])]: every (element, parameter[, component]) that has a row, and "energy"."""
    twice, out = case["twice"], []
    for e, dm in enumerate(reference.dmaps()):
        if dm is None or (twice is not None and e == twice[1]):
            continue
        places = [e] if twice is None or e != twice[0] else list(twice)
        for name, D in dm.items():
            if name == "energy":
                continue
            for component in ((0, 1) if D.ndim == 4 else (None,)):
                out.append(((e, name, component), [(p, name, component, 1.0) for p in places]))
    out.append(("energy", [(e, "energy", None, 1.0) for e in range(len(case["desc"]))]))
    return out


def evaluate(case, single=False):
    """
    Everything the case's calls are held to, from `AffineReference` (`single`: its float32-rounded form): "gradients" in the
    product's keys (`combine`), "tangents" [(label, mu_dot, cov_dot)] where forward mode applies, "mu" and "cov" at every
    point (B, P, 6), (B, P, 6, 6), and the reference itself.
    """
    desc, energy, B = case["desc"], case["energy"], case["B"]
    reference = rr.AffineReference(reference_desc(desc), energy, single=single)
    out = {"reference": reference}
    if case["mode"] == "parameters":
        mu, cov = case["mu"], case["cov"]
        raw = reference.parameter_gradients_along(mu, cov, case["w_mu"], case["w_cov"], case["w_e"], case["readings"])
        mus, covs = reference.parameter_states(mu, cov)
        out["mu"], out["cov"] = np.stack(mus, axis=1)[..., :6], np.stack(covs, axis=1)[..., :6, :6]
    else:
        raw = reference.particle_gradients_along(case["particles"], case["w_mu"], case["w_cov"], case["w_e"], case["readings"],
                                                 alive=case.get("alive"), trajectories_bar=case.get("trajectories_bar"),
                                                 chosen=case.get("chosen"))
        del raw["particles"]
        states = reference.particle_states(case["particles"])
        alive = case.get("alive")
        moments = [_moments_of(z[..., :6], np.ones(z.shape[:-1], dtype=bool) if alive is None else alive[k]) for k, z in enumerate(states)]
        out["mu"], out["cov"] = np.stack([m for m, _ in moments], axis=1), np.stack([c for _, c in moments], axis=1)
    out["gradients"] = combine(case, raw)
    if case["mode"] in ("parameters", "plain"):
        out["tangents"] = []
        for label, direction in directions_of(case, reference):
            if case["mode"] == "parameters":
                out["tangents"].append((label, *reference.parameter_tangents(case["mu"], case["cov"], direction)))
            else:
                out["tangents"].append((label, *reference.particle_tangents(case["particles"], direction)))
        if not single:
            out["floor_error"] = floor_error(case, out["tangents"])
    return out


def float32_bound(ref, axis_from=0):
    """3e-3 |ref| + 1e-4 max |ref|, the maximum over the whole array (`axis_from` = 1: per sample)."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    top = ref.max() if axis_from == 0 else ref.reshape(len(ref), -1).max(axis=1).reshape(-1, *([1] * (ref.ndim - 1)))
    return 3e-3 * ref + 1e-4 * top


def _conditioned(case, exact):
    """Whether rounding maps, derivatives (and a ParameterBeam's states) to float32 moves every result <= CONDITION of its bound."""
    rounded = evaluate(case, single=True)
    worst = 0.0
    for key, ref in exact["gradients"].items():
        bound = float32_bound(ref)
        with np.errstate(all="ignore"):
            ratio = np.where(bound > 0, np.abs(rounded["gradients"][key] - ref) / bound, 0.0)
        worst = max(worst, float(np.max(ratio)) if ratio.size else 0.0)
    for (_, mu_dot, cov_dot), (_, mu_r, cov_r) in zip(exact.get("tangents", []), rounded.get("tangents", [])):
        for ref, got in ((mu_dot, mu_r), (cov_dot, cov_r)):
            bound = float32_bound(ref, axis_from=1)
            with np.errstate(all="ignore"):
                ratio = np.where(bound > 0, np.abs(got - ref) / bound, 0.0)
            worst = max(worst, float(np.max(ratio)))
    return worst <= CONDITION, worst


def _cotangents(rng, i, B, P, size):
    w_mu, w_cov = np.zeros((B, P, size)), np.zeros((B, P, size, size))
    w_mu[..., :6] = rng.normal(size=(B, P, 6))
    w_cov[..., :6, :6] = rng.normal(size=(B, P, 6, 6)) * 1e3
    w_e = rng.normal(size=(B, P)) * 1e-10
    if i % 3 == 0:  # at one point only: an interior one where there is one
        k = int(rng.integers(1, P - 1)) if P > 2 else P - 1
        keep = np.arange(P) == k
        w_mu, w_cov, w_e = w_mu * keep[None, :, None], w_cov * keep[None, :, None, None], w_e * keep[None, :]
    return w_mu, w_cov, w_e


def draw_affine_case(seed, i):
    rng = np.random.default_rng([seed, i])
    # (the two draws the coverage of the committed seed depends on come first)
    N = int(COUNTS[rng.integers(len(COUNTS))])
    L = int(rng.integers(1, MAX_LEAVES + 1))
    dtype = [np.float32, np.float64][i % 2]
    mode = MODES[(i // 2) % 4]
    shape = SHAPES[(i // 8) % 4]
    B = int(np.prod(shape))
    if mode == "losses":
        N, L = max(N, 257) if N >= 257 else (257, 400)[N % 2], min(max(L, 2), MAX_LEAVES - 3)
    if mode == "parameters":
        N = 400
    energy = rr.energies(B, seed=int(rng.integers(1 << 30)))
    particles = rr.particles(B, N, seed=int(rng.integers(1 << 30)))
    case = dict(i=i, dtype=dtype, mode=mode, shape=shape, B=B, N=N, energy=energy, particles=particles, failures=0, loss_redraws=0,
                stand_in=False)
    for attempt in range(61):
        if attempt and attempt % 10 == 0:
            L = max(1, L // 2)
        desc, shared, twice, nested = _draw_lattice(rng, i, B, L, attempt)
        while derivative_count(desc, energy) > MAX_DERIVATIVES:
            desc, shared, twice, nested = _cut(desc, shared, twice, nested, len(desc) - 1)
        case.update(stand_in=attempt >= 60, shared=shared, twice=twice, nested=nested)
        case.pop("alive", None)
        if _amplification(rr.AffineReference(desc, energy).maps) > AMPLIFICATION:
            case["failures"] += 1
            continue
        if mode == "losses":
            plain = desc
            for _ in range(30):
                A = int(rng.integers(1, 4))
                places = sorted(int(p) for p in rng.choice(np.arange(1, len(plain) + 1), size=min(A, len(plain)), replace=False))
                desc = _sized_apertures(plain, particles, energy, places, rr.f32(rng.uniform(1.2, 2.5, len(places))))
                for kind, kw in desc:
                    if kind == "aperture":
                        kw["x_max"], kw["y_max"] = rr.f32(kw["x_max"]), rr.f32(kw["y_max"])
                _, specs = build(desc, np.float64)
                _, alive, lost_at, margin = _survivor_chain(desc, specs, particles, energy)
                kept = (lost_at == -1).mean(axis=-1)
                if np.all(kept >= 0.1) and np.all(kept <= 0.9) and margin >= 1e-6:
                    break
                case["loss_redraws"] += 1
            else:
                raise AssertionError(f"case {i}: no apertures that keep 10 % to 90 % of every sample")
            # (the leaves behind an inserted aperture move up)
            moved_up = lambda e: e + sum(p <= e for p in places)  # noqa: E731
            case.update(shared={moved_up(e) for e in shared}, twice=None if twice is None else tuple(moved_up(e) for e in twice),
                        nested=None if nested is None else (moved_up(nested[0]), moved_up(nested[1] - 1) + 1),
                        alive=alive, lost_at=lost_at, margin=margin)
        case["desc"] = desc
        P = len(desc) + 1
        w_rng = np.random.default_rng([seed, i, attempt])
        case["w_mu"], case["w_cov"], case["w_e"] = _cotangents(w_rng, i, B, P, 7 if mode == "parameters" else 6)
        active = [e for e, (kind, kw) in enumerate(desc) if kind == "bpm" and kw.get("is_active")]
        case["readings"] = [w_rng.normal(size=(2, B)) for _ in active] or None
        if mode == "parameters":
            case["mu"], case["cov"] = rr.moments_of(particles)
        if mode == "trajectories":
            K = min(CHOSEN[(i // 8) % 4], N)
            chosen = w_rng.permutation(N)[:K]
            if K >= 2:
                chosen[-1] = chosen[0]  # one repeat
            case["chosen"], case["trajectories_bar"] = chosen.astype(np.int64), w_rng.normal(size=(B, P, K, 7)) / N
        exact = evaluate(case)
        if dtype == np.float32:
            ok, case["conditioning"] = _conditioned(case, exact)
            if not ok:
                case["failures"] += 1
                continue
        break
    else:
        raise AssertionError(f"case {i}: the stand-in line is not conditioned")  # (cannot happen)
    case["exact"] = exact
    tags = "".join(tag for tag, on in (("s", case["shared"]), ("t", case["twice"]), ("n", case["nested"])) if on)
    size = f"N{N}" + (f"K{len(case['chosen'])}" if mode == "trajectories" else "")
    case["id"] = (f"a{i:02d}-{'f32' if dtype == np.float32 else 'f64'}-B{'x'.join(map(str, shape))}-{mode}-"
                  f"{size if mode != 'parameters' else 'pb'}-E{len(case['desc'])}{'-' + tags if tags else ''}")
    return case


_drawn: dict = {}


DRAW_SECONDS: dict = {}  # seed -> what drawing the affine cases and their references took, whoever asked first


def affine_cases(seed=SEED):
    if seed not in _drawn:
        started = time.perf_counter()
        _drawn[seed] = [draw_affine_case(seed, i) for i in range(N_AFFINE)]
        DRAW_SECONDS[seed] = time.perf_counter() - started
    return _drawn[seed]


# ---------------------------------------------------------------------------------------------------------------------
# building a case's Segment
# ---------------------------------------------------------------------------------------------------------------------


def lattice_description(case, for_product):
    """`desc` with the case's batch shape; `for_product`: a shared leaf's parameters as (1,) arrays."""
    shape, out = case["shape"], []
    for e, (kind, kw) in enumerate(case["desc"]):
        new = {}
        for name, v in kw.items():
            if isinstance(v, np.ndarray):
                v = v[:1] if for_product and e in case["shared"] else v.reshape(*shape, *v.shape[1:])
            new[name] = v
        out.append((kind, new))
    return out


def make_segment(case, lx):
    """(Segment, leaf elements): the nested run wrapped in a Segment of its own, the twice-placed object reused."""
    elements, _ = build(lattice_description(case, True), case["dtype"], lx)
    if case["twice"] is not None:
        elements[case["twice"][1]] = elements[case["twice"][0]]
    top = list(elements)
    if case["nested"] is not None:
        a, b = case["nested"]
        top = top[:a] + [lx.Segment(top[a:b])] + top[b:]
    return lx.Segment(top), elements


# ---------------------------------------------------------------------------------------------------------------------
# the along loss of the oracle's element-by-element chain, and its central differences under the two-step condition
# ---------------------------------------------------------------------------------------------------------------------


def along_loss(case, specs, energy):
    """
    (B,): the sum over the points of <w_mu, mu> + <w_cov, cov> + w_e (E - E_0) of the oracle's chain -- of ParameterBeams, or of
    the particles' mean and biased covariance over the particles alive at the point (the survivor sets of the case, held
    fixed) --, plus the active BPMs' reading weights and the chosen particles' trajectory cotangents.
    """
    w_mu, w_cov, w_e, B = case["w_mu"], case["w_cov"], case["w_e"], case["B"]
    active = [e for e, (kind, kw) in enumerate(case["desc"]) if kind == "bpm" and kw.get("is_active")]
    total = np.zeros(B)
    if case["mode"] == "parameters":
        beams = jr.chain(specs, o.parameter_beam(case["mu"], case["cov"], energy, np.float64))
        moments = [(b["mu"], b["cov"]) for b in beams]
    else:
        beams = jr.chain(specs, o.particle_beam(case["particles"], energy, np.float64))
        alive = case.get("alive")
        moments = [_moments_of(b["particles"][..., :6], np.ones((B, case["N"]), dtype=bool) if alive is None else alive[k])
                   for k, b in enumerate(beams)]
    for k, (b, (mean, cov)) in enumerate(zip(beams, moments)):
        total += np.sum(w_mu[:, k] * mean, axis=-1) + np.sum(w_cov[:, k] * cov, axis=(-1, -2)) + w_e[:, k] * (b["energy"] - case["energy"])
        if k in active:
            r = case["readings"][active.index(k)]
            total += r[0] * mean[:, 0] + r[1] * mean[:, 2]
        if case.get("chosen") is not None:
            total += np.sum(case["trajectories_bar"][:, k] * b["particles"][:, case["chosen"]], axis=(-1, -2))
    return total


def two_step_difference(loss, array, index, magnitude, scale):
    """
    d loss / d array[:, *index] per sample, by central differences at h and h / 4 that agree to rr.TWO_STEP_AGREEMENT of
    max(|value|, scale) -- the condition of `OracleCase.derivatives`, over its steps; `array` is moved in place and put back.
    """
    at = (slice(None), *index)
    kept = array[at].copy()
    tried = []

    def quotient(h):
        array[at] = kept + h
        up = loss()
        array[at] = kept - h
        down = loss()
        array[at] = kept
        return (up - down) / (2 * h)

    for rel in rr.RELATIVE_STEPS:
        h = rel * magnitude
        wide, narrow = quotient(h), quotient(h / 4)
        distance = float(np.max(np.abs(wide - narrow) / np.maximum(np.abs(wide), scale)))
        tried.append((rel, distance))
        if distance <= rr.TWO_STEP_AGREEMENT:
            return wide
    raise AssertionError(("no step at which the oracle's central differences agree with themselves", tried))


# ---------------------------------------------------------------------------------------------------------------------
# cavity cases: a line of drifts, quadrupoles and correctors with one to three gaining cavities, B = 2
# ---------------------------------------------------------------------------------------------------------------------

N_CAVITY = 8
CAVITY_PARTICLES = 400
CHECKED_PER_CASE = 8
OTHERS = {"drift": [("length",)], "quadrupole": [("k1",), ("length",), ("misalignment", 0), ("misalignment", 1)],
          "hcor": [("angle",), ("length",)], "vcor": [("angle",), ("length",)]}


def draw_cavity_case(seed, j):
    """
    Case j: 4 to 10 leaves, cavities at the settings of `rr.gentle_cells` (2 to 6 MV, |phase| <= 10 degrees, |k1| <= 2), every
    second quadrupole misaligned.  One `rr.OracleCase` with the along loss per beam class -- a ParameterBeam of the particles'
    moments (passes a and b) and the 400 particles themselves (pass c) -- and the eight quantities that are checked: every
    cavity's voltage and phase, the energy, and parameters of the other elements drawn to make eight.
    """
    rng = np.random.default_rng([seed, 1000 + j])
    dtype, B = [np.float32, np.float64][j % 2], 2
    L, C = int(rng.integers(4, 11)), int(rng.integers(1, 4))
    f = lambda v: np.full(B, float(np.float32(v)))  # noqa: E731
    u = lambda lo, hi, *tail: rr.f32(rng.uniform(lo, hi, (B, *tail)))  # noqa: E731
    kinds = [str(k) for k in rng.choice(["drift", "quadrupole", "hcor", "vcor"], size=L, p=[0.35, 0.35, 0.15, 0.15])]
    for at in rng.choice(L, size=C, replace=False):
        kinds[int(at)] = "cavity"
    desc, quadrupoles = [], 0
    for kind in kinds:
        if kind == "drift":
            desc.append((kind, dict(length=u(0.1, 0.5))))
        elif kind == "quadrupole":
            kw = dict(length=f(0.1), k1=u(0.5, 2.0) * (-1.0) ** quadrupoles)
            if quadrupoles % 2 == 0:
                kw["misalignment"] = rr.f32(rng.normal(0, 1e-3, (B, 2)))
            quadrupoles += 1
            desc.append((kind, kw))
        elif kind == "cavity":
            desc.append((kind, dict(length=f(1.0377), voltage=u(2e6, 6e6), phase=u(-10, 10), frequency=f(1.3e9))))
        else:
            desc.append((kind, dict(length=u(0.05, 0.2), angle=rr.f32(rng.normal(0, 1e-3, B)))))
    cavities = [e for e, (kind, _) in enumerate(desc) if kind == "cavity"]
    quantities = [(e, name) for e in cavities for name in ("voltage", "phase")] + ["energy"]
    others = [(e, *tail) for e, (kind, kw) in enumerate(desc) for tail in OTHERS.get(kind, []) if tail[0] in kw]
    quantities += [others[int(q)] for q in rng.permutation(len(others))[:CHECKED_PER_CASE - len(quantities)]]
    P = L + 1
    energy, particles = rr.energies(B), rr.particles(B, CAVITY_PARTICLES, seed=int(rng.integers(1 << 30)))
    mu, cov = rr.moments_of(particles)
    w_mu, w_cov, w_e = _cotangents(rng, 1, B, P, 7)  # (at every point)
    scales = rr._scales(quantities, w_cov)
    return dict(id=f"k{j}-{'f32' if dtype == np.float32 else 'f64'}-E{L}-C{C}", j=j, dtype=dtype, B=B, desc=desc, energy=energy,
                particles=particles, mu=mu, cov=cov, w_mu=w_mu, w_cov=w_cov, w_e=w_e, quantities=quantities, scales=scales,
                parameters=rr.OracleCase(desc, energy, w_mu, w_cov, mu=mu, cov=cov, w_e=w_e),
                particle_chain=rr.OracleCase(desc, energy, w_mu[..., :6], w_cov[..., :6, :6], particles=particles, w_e=w_e))


def cavity_cases(seed=SEED):
    if ("cavity", seed) not in _drawn:
        _drawn[("cavity", seed)] = [draw_cavity_case(seed, j) for j in range(N_CAVITY)]
    return _drawn[("cavity", seed)]
