"""
The reverse passes -- `grad.track_vjp` on a ParticleBeam (lynx_track_particles_backward) and on a ParameterBeam
(lynx_track_moments_backward), both through k_build_bwd -- at the sizes where their kernels change form, against
references that do not come from the GPU (tests/reverse_reference.py; tests/test_reverse_reference_host.py checks those
on the host): the analytic reverse mode for affine lattices, and central differences of the float64 oracle, held to
their two-step condition, where cavities are active.

    A  particle count      N = 1 .. 1025 around the float64 tile (256), the float32 tile (512: a lane carries particles
                           tid and tid + 256) and the wave (64)
    B  unit count          k_track_bwd parks the state every 4 units, at most 64; k_track_bwd_units<8>, <16>, and the dense
                           kernel from 17 units on
    C  chunking            workgroups per sample, k_reduce_tbar (chunks >= 16: unrolled loop and remainder) and
                           k_reduce_tbar_rows (chunks < 16: four rows per wave, clamped), tiles_per_wg >= 2
    D  long lattices       k_build_bwd with maps and prefix products in LDS and in HBM, a kind of more than 256 tasks, and
                           more than 256 steps (a ParameterBeam: several steps per thread)

Cotangents: `mu_bar` and `cov_bar` (and BPM readings).  Sample 1 has other parameters than sample 0.  Tolerances are
the project's: float64 as test_gpu_grad.py's finite-difference tests, float32 3e-3 |ref| + 1e-4 max |ref| -- here
against the float64 reference instead of the float64 GPU pass.  Every test prints its worst distance in units of its bound.

Measured on MI355X, worst distance / bound per axis: see NOTES.md (the entry of this file).
"""

import numpy as np
import pytest

from . import reverse_reference as rr
from .helpers import assert_parameter_beam, make_lattice, random_samples

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
_affine: dict = {}


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def _affine_reference(B):
    if B not in _affine:
        desc = rr.affine_lattice(B)
        _affine[B] = (desc, rr.energies(B), rr.AffineReference(desc, rr.energies(B)))
    return _affine[B]


def _vjp(lx, desc, dtype, energy, particles=None, mu=None, cov=None):
    elements, _ = make_lattice(desc, dtype, lx)
    if particles is not None:
        beam = lx.ParticleBeam(np.asarray(particles, dtype=dtype), energy.astype(dtype), dtype=dtype)
    else:
        beam = lx.ParameterBeam(mu, cov, energy, dtype=dtype)
    return elements, lx.grad.track_vjp(lx.Segment(elements), beam)


def _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=None, mu=None, cov=None, readings=None, wrt_particles=False,
               vjp=None):
    """Every gradient of the call, in the keys of the references: (e, name), "energy", "particles" | "mu", "cov"."""
    elements, vjp = _vjp(lx, desc, dtype, energy, particles, mu, cov) if vjp is None else vjp
    kwargs = {}
    if readings is not None:
        bpms = [el for (kind, kw), el in zip(desc, elements) if kind == "bpm" and kw.get("is_active")]
        kwargs["readings"] = dict(zip(bpms, readings))
    if particles is not None and wrt_particles:
        kwargs["wrt_particles"] = True
    g = vjp(mu_bar=w_mu, cov_bar=w_cov, **kwargs)
    out = {"energy": np.asarray(g.energy, dtype=np.float64)}
    for e, (kind, kw) in enumerate(desc):
        for name in kw:
            if kind != "bpm" and isinstance(kw[name], np.ndarray):
                out[(e, name)] = np.asarray(g[elements[e]][name], dtype=np.float64)
    if particles is not None and wrt_particles:
        out["particles"] = np.asarray(g.particles, dtype=np.float64)
    if particles is None:
        out["mu"], out["cov"] = np.asarray(g.mu, dtype=np.float64), np.asarray(g.cov, dtype=np.float64)
    return out


class Distances:
    """|got - ref| against the project's bounds; keeps the worst distance in units of its bound and where it was."""

    def __init__(self, dtype, w_cov):
        self.single = np.dtype(dtype) == np.float32
        self.floor = 1e-9 * float(np.max(np.abs(w_cov)))
        self.worst, self.where, self.failures, self.count = 0.0, None, [], 0

    def bound(self, key, got, ref, got_all, ref_all):
        """got, ref: the compared entries; got_all, ref_all: the arrays the bounds take their maxima of."""
        if self.single:
            return 3e-3 * np.abs(ref) + 1e-4 * np.max(np.abs(ref_all))
        if key == "energy":  # test_gradients_match_finite_differences_fp64
            return 2e-4 * np.abs(ref) + 1e-12
        if key == "direction":  # test_gradient_wrt_incoming_particles: rtol 1e-5 (+ allclose's atol)
            return 1e-5 * np.abs(ref) + 1e-8
        per_sample = lambda a: np.max(np.abs(a).reshape(len(a), -1), axis=1).reshape(-1, *([1] * (got.ndim - 1)))  # noqa: E731
        if key == "particles":  # test_gradient_wrt_incoming_particles
            return 1e-4 * np.abs(ref) + 1e-6 * per_sample(got_all)
        if key == "mu":  # test_parameter_beam_gradients_match_finite_differences_fp64
            return 1e-5 * np.abs(ref) + 1e-9 * per_sample(got_all)
        if key == "cov":
            return 1e-4 * np.abs(ref) + 1e-7 * per_sample(got_all)
        return 2e-4 * np.maximum(np.abs(ref), self.floor) + 1e-7 * np.max(np.abs(got_all))

    def add(self, key, got, ref, got_all=None, ref_all=None):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        kind = key if isinstance(key, str) else "parameter"
        bound = self.bound(kind, got, ref, got if got_all is None else got_all, ref if ref_all is None else ref_all)
        with np.errstate(all="ignore"):
            ratio = np.where(np.abs(got - ref) <= bound, np.abs(got - ref) / np.maximum(bound, 1e-300), np.inf)
            ratio = np.where(np.isfinite(got), ratio, np.inf)
        self.count += got.size
        if ratio.size and float(np.max(ratio)) > self.worst:
            self.worst, self.where = float(np.max(ratio)), (key, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        if ratio.size and not np.all(np.isfinite(ratio)):
            at = np.unravel_index(int(np.argmax(np.abs(got - ref) / np.maximum(bound, 1e-300))), ratio.shape)
            self.failures.append((key, at, float(got[at]), float(ref[at]), float(np.broadcast_to(bound, got.shape)[at])))

    def add_all(self, got, ref, samples=slice(None)):
        """Every key of the reference (arrays over the batch) against the same key of `got`, at `samples` of got's batch."""
        part = {"particles": (Ellipsis, slice(6)), "mu": (Ellipsis, slice(6)), "cov": (Ellipsis, slice(6), slice(6))}
        for key, r in ref.items():
            g = got[key][samples]
            self.add(key, g[part.get(key, Ellipsis)], r[part.get(key, Ellipsis)])

    def add_differences(self, got, refs):
        """`refs`: {quantity: (B,)} of OracleCase.derivatives; the float32 bound's max |ref| is over a parameter's / the group's references."""
        groups = {}
        for q in refs:
            groups.setdefault(q if q == "energy" else q[:2] if isinstance(q[0], int) else q[0], []).append(q)
        for group, members in groups.items():
            ref_all = np.stack([refs[q] for q in members])
            for q in members:
                if q == "energy":
                    self.add("energy", got["energy"], refs[q])
                elif q == ("direction",):
                    self.add("direction", got["direction"], refs[q])
                elif isinstance(q[0], int):
                    self.add(q[:2], got[q[:2]][(slice(None), *q[2:])], refs[q], got[q[:2]], ref_all)
                else:
                    self.add(q[0], got[q[0]][(slice(None), *q[1:])], refs[q], got[q[0]][..., :6] if q[0] == "particles" else got[q[0]],
                             ref_all)

    def done(self, what, at_least=1):
        print(f"{what}: {self.count} values, worst distance {self.worst:.3g} of its bound at {self.where}")
        assert self.count >= at_least, (what, self.count)
        assert not self.failures, (what, self.failures[:8])


# ---- A. particle count -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", rr.PARTICLE_COUNTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_particle_count_affine_lattice(lx, dtype, N):
    """Every parameter of every kind, the energy, both BPM readings' cotangents and EVERY particle's cotangent, analytic reference."""
    B = 2
    desc, energy, reference = _affine_reference(B)
    P = rr.particles(B, N, seed=N)
    w_mu, w_cov = rr.cotangents(B, 100 + N)
    readings = rr.reading_weights(B)
    got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=P, readings=readings, wrt_particles=True)
    assert got["particles"].shape == (B, N, 7)
    d = Distances(dtype, w_cov)
    d.add_all(got, reference.particle_gradients(P, w_mu, w_cov, readings))
    d.done(f"A affine {np.dtype(dtype).name} N={N}", at_least=60 + 12 * N)


@pytest.mark.parametrize("N", rr.PARTICLE_COUNTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_particle_count_class_u_cavity_lattice(lx, monkeypatch, dtype, N):
    """
    [drift, misaligned quadrupole, hcor, drift, cavity] x 3 + [quadrupole, drift] -- in float32 the structured kernel over
    merged pairs: one parameter of each kind, the energy, the cotangents of particles 0, N - 1 and 255, 256, 511, 512 (the
    edges of a lane's two packed particles) where they exist, and the directional derivative over all particles, against
    the oracle's differences.
    """
    case, _ = rr.class_u_case(N)
    refs = rr.references(rr.class_u_case(N))

    def run():
        got = _gradients(lx, case.desc, dtype, case.energy, case.w_mu, case.w_cov, particles=case.particles, wrt_particles=True)
        got["direction"] = np.sum(got["particles"] * case.direction, axis=(1, 2))
        return got

    got = run()
    d = Distances(dtype, case.w_cov)
    d.add_differences(got, refs)
    d.done(f"A class U {np.dtype(dtype).name} N={N}", at_least=2 * (8 + 6))
    if dtype == np.float32 and N >= 64:  # the structured kernel did run: the dense one associates the sums differently
        monkeypatch.setenv("LYNX_BWD_UNITS", "0")
        dense = run()
        assert any(np.any(dense[key] != got[key]) for key in got)


# ---- B. unit count -----------------------------------------------------------------------------------------------------

def _units_run(lx, dtype, units, pairs):
    case, _ = rr.units_case(units, pairs)
    return case, _gradients(lx, case.desc, dtype, case.energy, case.w_mu, case.w_cov, particles=case.particles)


@pytest.mark.parametrize("units", rr.DENSE_UNITS)
@pytest.mark.parametrize("mode", ["fp64", "fp32-pairs", "fp32-steps"])
def test_unit_count_dense_walk(lx, monkeypatch, mode, units):
    """
    k_track_bwd (state parked every 4 units, at most 64): float64; float32 with LYNX_BWD_UNITS=0 over merged [run, cavity]
    pairs; float32 with LYNX_BWD_MERGE=0 as well, step by step.  First and last element, the elements of units 3, 4 and
    U - 1, the energy, against the oracle's differences.

    In float64 a unit is a step, and k_track_bwd's workgroup needs 44352 + 2048 S bytes of LDS (exchange buffer
    [4][21][66] and per-step sums [4][S][64] doubles): more than the 163840 there are from S = 59 on, where the call used
    to refuse ("LDS budget exceeded") although the header promised 64 steps.  From 59 steps on the sums are now kept at a
    stride of the 57 entries in use (bwd_acc_stride: 64 steps take 161088 bytes), so fp64-63 and fp64-64 run in that
    layout; test_float64_steps_across_the_layout_switch holds 58 | 59.
    """
    dtype = np.float64 if mode == "fp64" else np.float32
    if dtype == np.float32:
        monkeypatch.setenv("LYNX_BWD_UNITS", "0")
    if mode == "fp32-steps":
        monkeypatch.setenv("LYNX_BWD_MERGE", "0")
    pairs = mode == "fp32-pairs"
    case, got = _units_run(lx, dtype, units, pairs)
    d = Distances(dtype, case.w_cov)
    d.add_differences(got, rr.references(rr.units_case(units, pairs)))
    d.done(f"B dense {mode} U={units}", at_least=4)


@pytest.mark.parametrize("units", rr.STRUCTURED_UNITS)
def test_unit_count_structured_walk(lx, monkeypatch, units):
    """
    k_track_bwd_units<8> up to 8 units, <16> up to 16, the dense kernel beyond: float32, default knobs.  That the intended
    form was reached: up to 16 units the result differs from LYNX_BWD_UNITS=0 (another kernel associates the sums
    differently), at 17 it is that result bit for bit.
    """
    case, got = _units_run(lx, np.float32, units, True)
    d = Distances(np.float32, case.w_cov)
    d.add_differences(got, rr.references(rr.units_case(units, True)))
    d.done(f"B structured U={units}", at_least=4)
    monkeypatch.setenv("LYNX_BWD_UNITS", "0")
    _, dense = _units_run(lx, np.float32, units, True)
    same = all(np.array_equal(dense[key], got[key]) for key in got)
    assert same == (units > 16), (units, same)


@pytest.mark.parametrize("mode", ["fp64", "fp32-pairs", "fp32-steps"])
def test_65_units_are_refused(lx, monkeypatch, mode):
    """
    One unit more than k_track_bwd parks: the library's message names the limit of 64 -- the refusal comes before any
    scratch is asked for and before the first launch (track_backward_t) --, and the context goes on working: the pass
    before and the pass after give the same bits.
    """
    from lynx_amd import _ffi

    dtype = np.float64 if mode == "fp64" else np.float32
    if mode == "fp32-steps":
        monkeypatch.setenv("LYNX_BWD_MERGE", "0")
    pairs = mode == "fp32-pairs"
    works = 16  # (any size every mode walks)
    case, before = _units_run(lx, dtype, works, pairs)
    desc, _ = rr.unit_lattice(2, 65, pairs)
    with pytest.raises(_ffi.LynxError, match=r"parks at most 64"):
        _gradients(lx, desc, dtype, case.energy, case.w_mu, case.w_cov, particles=case.particles)
    _, after = _units_run(lx, dtype, works, pairs)
    assert all(np.array_equal(before[key], after[key]) for key in before)


@pytest.mark.parametrize("units", [58, 59])
def test_float64_steps_across_the_layout_switch(lx, units):
    """
    In float64 k_track_bwd keeps its per-step sums at a stride of 64 entries up to 58 steps -- the last count at which
    44352 + 2048 S bytes fit 163840 -- and of 57 from 59 on: both sides against the oracle's differences.
    """
    assert (4 * 21 * 66 + 4 * 58 * 64) * 8 <= 160 * 1024 < (4 * 21 * 66 + 4 * 59 * 64) * 8
    assert (4 * 21 * 66 + 4 * 64 * 57) * 8 <= 160 * 1024  # the 64 units fit at the narrow stride
    case, got = _units_run(lx, np.float64, units, False)
    d = Distances(np.float64, case.w_cov)
    d.add_differences(got, rr.references(rr.units_case(units, False)))
    d.done(f"B dense fp64 U={units}", at_least=4)


# ---- C. chunking -------------------------------------------------------------------------------------------------------

def _tile(dtype):
    return 256 * (2 if np.dtype(dtype) == np.float32 else 1)


@pytest.mark.parametrize("tiles", [15, 16, 17, 29, 33])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_chunks_of_one_sample(lx, dtype, tiles):
    """
    B = 1: one workgroup per tile, `tiles` partial sums per step -- k_reduce_tbar_rows below 16 (an odd count), k_reduce_tbar
    from 16 on: 16, 17 and 33 leave its unrolled loop 0, 1 and 1 chunks per wave for the remainder, 29 leaves 5.
    """
    desc, energy, _ = _affine_reference(2)
    desc, energy = rr.take_samples(desc, [1]), energy[[1]]
    N = tiles * _tile(dtype) - 3
    info = lx.device.get_runtime().info()
    assert rr.backward_geometry(N, 1, info["compute_units"], _tile(dtype) // 256) == (tiles, tiles, 1)
    P = rr.particles(1, N, seed=tiles)
    w_mu, w_cov = rr.cotangents(1, 200 + tiles)
    readings = [r[:, [1]] for r in rr.reading_weights(2)]
    got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=P, readings=readings, wrt_particles=True)
    d = Distances(dtype, w_cov)
    d.add_all(got, rr.AffineReference(desc, energy).particle_gradients(P, w_mu, w_cov, readings))
    d.done(f"C {np.dtype(dtype).name} tiles={tiles}", at_least=6 * N)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_fifteen_rows_of_partial_sums(lx, dtype):
    """B = 3 samples of 5 steps: 15 (sample, step) rows -- the last wave of k_reduce_tbar_rows takes rows 12, 13, 14 and a clamped one."""
    B, N = 3, 300
    desc, energy, reference = _affine_reference(B)
    P = rr.particles(B, N, seed=15)
    w_mu, w_cov = rr.cotangents(B, 215)
    readings = rr.reading_weights(B)
    vjp = _vjp(lx, desc, dtype, energy, particles=P)
    assert len(vjp[1].program.steps) == 5  # run, BPM, run, BPM, run
    got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=P, readings=readings, wrt_particles=True, vjp=vjp)
    d = Distances(dtype, w_cov)
    d.add_all(got, reference.particle_gradients(P, w_mu, w_cov, readings))
    d.done(f"C {np.dtype(dtype).name} 15 rows", at_least=6 * N * B)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_several_tiles_per_workgroup_and_a_short_last_one(lx, dtype, record_property):
    """
    B = 1024 samples of 7 tiles: more samples than 24 workgroups per CU can give a tile each, so a workgroup walks
    tiles_per_wg >= 2 tiles and the last one of a sample fewer.  First sample, last sample and a handful drawn per run.
    """
    B, tiles = 1024, 7
    N = tiles * _tile(dtype) - 3
    info = lx.device.get_runtime().info()
    _, chunks, per_wg = rr.backward_geometry(N, B, info["compute_units"], _tile(dtype) // 256)
    assert per_wg >= 2 and chunks * per_wg > tiles, (info["compute_units"], chunks, per_wg)  # what the case means to reach
    desc, energy = rr.affine_lattice(B), rr.energies(B)
    rng = np.random.default_rng(7)
    P = np.ones((B, N, 7), dtype=np.float32)
    P[..., :6] = rng.standard_normal((B, N, 6), dtype=np.float32) * np.float32(rr.BEAM_SIGMA) + np.float32(rr.BEAM_MU)
    w_mu, w_cov = rr.cotangents(B, 300)
    readings = rr.reading_weights(B)
    got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=P, readings=readings, wrt_particles=True)
    samples, _ = random_samples(B, 4, always=(0, B - 1), record=record_property)
    reference = rr.AffineReference(rr.take_samples(desc, samples), energy[samples]).particle_gradients(
        P[samples].astype(np.float64), w_mu[samples], w_cov[samples], [r[:, samples] for r in readings])
    d = Distances(dtype, w_cov[samples])
    d.add_all(got, reference, samples)
    d.done(f"C {np.dtype(dtype).name} B=1024", at_least=6 * N * len(samples))


# ---- D. long lattices through k_build_bwd ------------------------------------------------------------------------------

@pytest.mark.parametrize("beam", ["particles", "parameters"])
@pytest.mark.parametrize("side", ["lds", "hbm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_maps_in_lds_and_in_hbm(lx, dtype, side, beam):
    """
    One run of E elements of every kind, E the last count at which k_build_bwd keeps maps and prefix products in LDS
    (40 KiB) and the first at which they go to HBM; the float32 lattices have more than 256 tasks of one kind
    (quadrupoles), the kind-sorted task list's second round.  Every parameter, analytic reference.
    """
    itemsize = np.dtype(dtype).itemsize
    fixed = lambda S, E: (2 * (S + 1) + E + 4 * 98) * itemsize  # noqa: E731  build_bwd_lds_fixed
    E = rr.lds_switch(itemsize)
    assert fixed(1, E) + (2 * E + 2) * 49 * itemsize <= 40 * 1024 < fixed(1, E + 1) + (2 * (E + 1) + 2) * 49 * itemsize
    assert E == (98 if dtype == np.float32 else 46)
    E += side == "hbm"
    B = 2
    desc, energy = rr.long_affine_lattice(B, E), rr.energies(B)
    if dtype == np.float32:
        assert 6 * sum(kind == "quadrupole" for kind, _ in desc) > 256
    reference = rr.AffineReference(desc, energy)
    P = rr.particles(B, 257, seed=E)
    if beam == "particles":
        w_mu, w_cov = rr.cotangents(B, 400 + E)
        got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, particles=P, wrt_particles=True)
        ref = reference.particle_gradients(P, w_mu, w_cov)
    else:
        w_mu, w_cov = rr.cotangents(B, 400 + E, size=7)
        mu, cov = rr.moments_of(P)
        got = _gradients(lx, desc, dtype, energy, w_mu, w_cov, mu=mu, cov=cov)
        ref = reference.parameter_gradients(mu, cov, w_mu, w_cov)
    d = Distances(dtype, w_cov)
    d.add_all(got, ref)
    d.done(f"D {np.dtype(dtype).name} E={E} {beam}", at_least=3 * E)


@pytest.mark.parametrize("steps", rr.STEP_COUNTS)
def test_step_count_parameter_beam(lx, steps):
    """
    A ParameterBeam through `steps` steps of run and cavity in turn, float64: k_build_bwd deals the steps to its 256
    threads, several steps per thread beyond 256 (with `if (tid < S)` instead the step energies, every map built from them
    and the whole energy cotangent were wrong from step 256 on).  The forward result against the oracle first, so that a
    failure says which half is wrong; then the first cavity, the elements of steps 254 .. 257, the last cavity, quadrupoles,
    a drift, the energy and the incoming mu and cov against the oracle's differences.

    lynx_track_moments and the build of the reverse pass keep the whole step table in LDS next to the build's scratch: in
    float64 520 bytes per step next to 89376 (a small batch's chunks of 128 elements) or 45472 (chunks of 64) of 163840,
    which used to end at 138 (220) steps with "program needs 226080 B of LDS: split the lattice" -- no float64 program of
    more than 256 steps ever reached k_build_bwd.  Both now halve the chunk until the table fits (more compose rounds: 32
    elements for these lattices), so these cases run; test_step_count_parameter_beam_float32 holds the same lattices in
    float32 at a batch that always fitted, which is where the old `if (tid < S)` was measured.
    """
    case, _ = rr.steps_case(steps)
    vjp = _vjp(lx, case.desc, np.float64, case.energy, mu=case.mu, cov=case.cov)
    assert len(vjp[1].program.steps) == steps
    assert_parameter_beam(vjp[1].outgoing, case.forward(), 1e-9, f"forward, {steps} steps")
    got = _gradients(lx, case.desc, np.float64, case.energy, case.w_mu, case.w_cov, mu=case.mu, cov=case.cov, vjp=vjp)
    d = Distances(np.float64, case.w_cov)
    d.add_differences(got, rr.references(rr.steps_case(steps)))
    d.done(f"D steps={steps}", at_least=2 * 25)


@pytest.mark.parametrize("steps", rr.STEP_COUNTS)
def test_step_count_parameter_beam_float32(lx, steps):
    """
    The lattices and references of test_step_count_parameter_beam where the library does run more than 256 steps: float32
    (443 + 268 bytes of LDS per step less than float64) and a batch of more than half the compute units (the builds then
    take chunks of 64 elements).  The batch is the two samples of the case over and over; the first two and the last two
    are compared.  With `if (tid < S)` in k_build_bwd the cases of 257 and 261 steps fail and those of 255 and 256 pass;
    with the strided loops all four pass (measured on MI355X, NOTES.md).
    """
    case, _ = rr.steps_case(steps)
    times = lx.device.get_runtime().info()["compute_units"] // 4 + 1
    tile = lambda a: np.tile(a, (times,) + (1,) * (np.ndim(a) - 1))  # noqa: E731
    desc = [(kind, {k: tile(v) for k, v in kw.items()}) for kind, kw in case.desc]
    vjp = _vjp(lx, desc, np.float32, tile(case.energy), mu=tile(case.mu), cov=tile(case.cov))
    assert len(vjp[1].program.steps) == steps
    out, ref = vjp[1].outgoing, case.forward()
    # forward: the project's float32 bound, 1e-4, is asserted on lattices of up to about 20 steps (test_gpu_parity.py); a
    # rounding error per step adds up linearly at worst, so `steps` steps get steps / 20 of it
    for rows in (slice(0, 2), slice(-2, None)):
        assert_parameter_beam((np.asarray(out._mu)[rows], np.asarray(out._cov)[rows]), ref, 1e-4 * steps / 20,
                              f"forward, {steps} steps, float32")
    got = _gradients(lx, desc, np.float32, tile(case.energy), tile(case.w_mu), tile(case.w_cov), mu=tile(case.mu),
                     cov=tile(case.cov), vjp=vjp)
    d = Distances(np.float32, case.w_cov)
    refs = rr.references(rr.steps_case(steps))
    for rows in (slice(0, 2), slice(-2, None)):
        d.add_differences({key: value[rows] for key, value in got.items()}, refs)
    d.done(f"D steps={steps} float32", at_least=4 * 25)
