"""
The optimisation loop at the sizes where consecutive calls overlap: a parameter is written before every call and
nothing is read until the last call has returned.

lynx_hip.hip overlaps consecutive `track` calls (track_table, track_particles_t, reduce_moment_records): the map build
of call n + 1 runs on a second stream into a ring of kTableSlots step tables, it starts in the tail of an earlier
streaming kernel, the host or the main stream waits for it, the moment reduction runs on a third stream out of a ring
of kPartialRing record buffers, every other launch of 256 MiB walks the batch backwards, short calls go inline or to
the second stream by `main_idle`, and a reverse pass reads the table its forward call left.  With the same parameters in
every call none of that can be seen to go wrong; here every call has its own (tests/pipelined_cases.py, and
tests/test_pipelined_host.py for what the sequences tell apart and which side of every threshold a shape lies on).

Each sequence runs three ways on the same incoming beam:
  pipelined  all K calls issued, every outgoing beam held, nothing read or synchronised before the last call returned;
  serial     a fresh Segment, the same writes, `get_runtime().sync()` and a read-back after every call;
  recycling  as pipelined, but only each call's moment record (and energy) stays alive: the beam is dropped at once and
             the allocator hands call n's particle block to call n + 1 -- the shape of the real loop.
Pipelined and recycling equal serial BIT FOR BIT (the same kernels see the same numbers; only streams and slots differ:
every lattice has at most 32 elements, one chunk of the workgroup build whether or not it runs underneath a kernel --
build_shape / build_chunk), and serial is held to the oracle at the parameters each call saw.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import pipelined_cases as pc
from .helpers import make_lattice, random_samples, rel_err
from .test_gpu_fuzz import _check_parameter, _check_particles, _has_cavity, _loss64, _moment_check, _oracle
from .test_gpu_grad import PARAMS_TO_CHECK
from .test_gpu_parity import TOL_KICK_F64, TOL_MOM, TOL_P  # noqa: F401  (the rule of _check_particles / _moment_check)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


# ---------------------------------------------------------------------------------------------------------------------
# running a sequence
# ---------------------------------------------------------------------------------------------------------------------


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _where(a, b):
    """For a failure message: how many samples differ, and the first of them."""
    a, b = np.asarray(a), np.asarray(b)
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    rows = np.flatnonzero(bad.reshape(bad.shape[0], -1).any(axis=1)) if bad.ndim else np.flatnonzero(bad)
    return f"{len(rows)} of {bad.shape[0] if bad.ndim else 1} samples differ, first {rows[:4].tolist()}"


def _segment(lx, case, seed=11):
    c = pc.CASES[case]
    desc, _, _, bpm = pc.lattice(pc.LATTICE_OF[case], c["B"], seed=seed)
    elements, _ = make_lattice(desc, c["dtype"], lx)
    return lx.Segment(elements), elements, bpm


def _incoming(lx, case, seed=2):
    c = pc.CASES[case]
    return lx.ParticleBeam.synthetic((c["B"],), c["N"], sigma=pc.SIGMA, energy=c["energy"], seed=seed, dtype=c["dtype"])


def _apply(elements, writes, dtype):
    for e, name, value in writes:
        setattr(elements[e], name, np.asarray(value, dtype=dtype))


def _run(lx, case, beam, mode, particle_calls):
    """One sequence: {records: [K], energies: [K], particles: {call: array}, reading}."""
    c = pc.CASES[case]
    seg, elements, bpm = _segment(lx, case)
    rt = lx.device.get_runtime()
    rt.sync()  # every run starts on an idle context: the first short call goes inline
    res = dict(records=[], energies=[], particles={})

    def read(j, moments, energy, particles):
        res["records"].append(moments.host())
        res["energies"].append(np.array(energy.host()))
        if particles is not None and j in particle_calls:
            res["particles"][j] = particles.host()

    held = []
    for j, w in enumerate(pc.writes(case)):
        _apply(elements, w, c["dtype"])
        out = seg.track(beam)
        if mode == "serial":
            rt.sync()
            read(j, out._moments, out._energy, out._particles)
        elif mode == "pipelined":
            held.append((out._moments, out._energy, out._particles))
        else:  # recycling: the particle block goes back to the allocator while its kernel may still be running
            held.append((out._moments, out._energy, None))
        del out
    for j, (moments, energy, particles) in enumerate(held):
        read(j, moments, energy, particles)
    res["reading"] = None if bpm is None else np.array(elements[bpm].reading)
    return res


def _assert_runs_equal(got, ref, what, particles=True):
    for j, (a, b) in enumerate(zip(got["records"], ref["records"])):
        assert _same(a, b), (what, "moment record of call", j, _where(a, b))
    for j, (a, b) in enumerate(zip(got["energies"], ref["energies"])):
        assert _same(a, b), (what, "energy of call", j, _where(a, b))
    if particles:
        assert sorted(got["particles"]) == sorted(ref["particles"])
        for j in ref["particles"]:
            assert _same(got["particles"][j], ref["particles"][j]), (what, "particles of call", j, _where(got["particles"][j], ref["particles"][j]))
    if ref["reading"] is not None:
        assert _same(got["reading"], ref["reading"]), (what, "BPM reading after the last call")


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------


def _oracle_chain(descs, P, energy, dtype):
    """
    `descs` (one lattice after the other) on the particles P: the chain test_gpu_fuzz._oracle holds a case to -- the
    product's arithmetic where it deviates on purpose (runs composed in float64, the float32 kick's form) and, float32
    behind an active cavity, the float64 chain next to it (test_gpu_parity._particle_case).
    """
    readings = []
    ref = o.particle_beam(P, np.asarray(energy, dtype=dtype), dtype)
    for desc in descs:
        _, specs = make_lattice(desc, dtype)
        ref = o.segment_track(specs, ref, dtype, bpm_readings=readings, kick="product", compose="float64")
    ref["readings"] = readings
    if dtype == np.float32 and any(_has_cavity(desc) for desc in descs):
        up = lambda v: np.asarray(v, np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v  # noqa: E731
        r64 = o.particle_beam(P.astype(np.float64), np.asarray(energy, dtype=np.float64), np.float64)
        for desc in descs:
            _, specs64 = make_lattice([(kind, {k: up(v) for k, v in kw.items()}) for kind, kw in desc], np.float64)
            r64 = o.segment_track(specs64, r64, np.float64)
        ref["float64_chain"] = r64
    return ref


def _beam_like(lx, dtype, record, energy, particles=None):
    """What a read-back left of an outgoing beam (cut to some samples), as a beam the shared checks take."""
    from lynx_amd.device import Dual

    out = lx.ParticleBeam.__new__(lx.ParticleBeam)
    p = particles if particles is not None else np.zeros((*record.shape[:-1], 1, 7), dtype=dtype)
    out._init_raw(Dual(np.ascontiguousarray(p), owned=True), Dual(np.asarray(energy, dtype=dtype)), None, dtype,
                  moments=Dual(np.ascontiguousarray(record), owned=True))
    return out


def _check_call(lx, case, descs, P, pick, record, energy, particles, what):
    """
    One call's results on the samples `pick` against the oracle: moments, energy and (if read back) particles.
    `case`: a key of pipelined_cases.CASES, or a dict with its own dtype, N and energy.
    """
    c = pc.CASES[case] if isinstance(case, str) else case
    dtype = c["dtype"]
    e = np.full(len(pick), c["energy"], dtype=dtype)
    ref = _oracle_chain([pc.subset(desc, pick, dtype) for desc in descs], P[pick], e, dtype)
    fcase = dict(dtype=dtype, n=c["N"])
    out = _beam_like(lx, dtype, record[pick], energy[pick], None if particles is None else particles[pick])
    if particles is not None:
        _check_particles(fcase, out, ref, None, what)
    else:
        _moment_check(out, ref, dtype, c["N"], what)
        assert rel_err(out.energy, ref["energy"]) < 1e-6, what
    return ref


def _samples(case, record_property):
    """All samples where the oracle can afford them, else {0, 63, 64, B - 1} and three drawn (seed recorded)."""
    B = pc.CASES[case]["B"]
    if pc.oracle_steps(case) <= pc.ORACLE_BUDGET:
        return list(range(B))
    pick, _ = random_samples(B, 3, always=[b for b in (0, 63, 64, B - 1) if b < B], record=record_property)
    return pick


def _check_serial_against_the_oracle(lx, case, serial, P, pick, what):
    c = pc.CASES[case]
    ref = None
    for j, desc in enumerate(pc.described(case)):
        ref = _check_call(lx, case, [desc], P, pick, serial["records"][j], serial["energies"][j],
                          serial["particles"].get(j), f"{what}, call {j}")
    if serial["reading"] is not None:  # the active BPM after the last call (bpm.py:48-58: mu_x, mu_y of what enters it)
        (_, want), = ref["readings"]
        got = np.asarray(serial["reading"], dtype=np.float64)[:, pick]
        scale = np.abs(want) + np.array([pc.SIGMA[0], pc.SIGMA[2]])[:, None]
        assert np.all(np.abs(got - want) <= TOL_MOM[c["dtype"]] * scale), (what, "BPM reading")


# ---------------------------------------------------------------------------------------------------------------------
# the four default paths
# ---------------------------------------------------------------------------------------------------------------------

REACHES = {
    "short": "a half-million SHORT call (track_table: `t->short_call`, B N >= 512 Ki, below 128 MiB, no cavity): the first call goes "
             "inline (`inline_all`, `ctx->main_idle`), later ones build on the second stream, so do the two behind a flag write "
             "(lynx_lattice_set_flags waits for the main stream: idle again); the reduction stays in line (track_particles_t: `side`); "
             "the parameters travel in the kernel arguments (lynx_lattice_create: `prog_pool`; lynx_lattice_update_params rewrites "
             "`h_pool` between launches); the lattice has an observer step (k_reduce_observers)",
    "long": "134 MB per call (track_table: `long_kernel`): the host waits for the build (hipEventSynchronize(ev_built)), the build "
            "starts in the tail (`t->tail`, hipStreamWaitValue32), the reduction runs on the side stream (reduce_moment_records: "
            "`side`); lanes build (launch_build: `lanes`) of single-map wave tiles; parameter writes go through "
            "lynx_lattice_update_params's copy",
    "cavity": "cavity flags and the lanes build on `s_build` with their single scratch buffers (launch_cavity_flags, "
              "launch_build_lanes); the MAIN STREAM waits for the build (track_table: `lat->has_cavity` -> hipStreamWaitEvent); merged "
              "[run, cavity] pairs in the units / pair-form kernel (track_particles_t: `pair_form`); an energy out",
    "order": "268.8 MB per call (track_particles_t: `>= ((size_t)256 << 20)`): launches alternate walking the batch backwards "
             "(`p.a.reversed`, `long_calls`); the records go through a second reduction level (reduce_moment_records: "
             "`rows > kReduceStage`)",
}


@pytest.mark.parametrize("case", ["short", "long", "cavity", "order"])
def test_pipelined_and_recycling_calls_equal_serial_ones_and_the_oracle(lx, monkeypatch, record_property, case):
    """
    K calls (9; `order`: 6) with k1 of one quadrupole rewritten before each -- three wraps of the table ring, two of the
    record ring -- pipelined, serial and recycling (module docstring).  Pipelined and recycling against serial: every
    call's moment record and outgoing energy, pipelined also every call's particles (`order`: of the last two calls)
    and the active BPM's reading after the last call, bit for bit.  Serial against the oracle at the parameters each
    call saw, on samples {0, 63, 64, B - 1} and three drawn: moments, energy, particles (TOL_MOM, TOL_P, TOL_KICK_F64
    and the float64-chain rule of test_gpu_fuzz._moment_check).  What each case reaches, and the lines of lynx_hip.hip
    that decide it (REACHES, printed; test_pipelined_host.py holds the shapes to the thresholds):
    `cavity` also asks LYNX_TRACK_UNITS=2 / LYNX_UNIT_PAIRS=2 ("insist") for one more call: the shape does take the
    pair-form kernel.
    """
    print(f"{case}: {REACHES[case]}")
    c = pc.CASES[case]
    K = c["K"]
    particle_calls = {K - 2, K - 1} if case == "order" else set(range(K))
    beam = _incoming(lx, case)
    serial = _run(lx, case, beam, "serial", particle_calls)
    pipelined = _run(lx, case, beam, "pipelined", particle_calls)
    _assert_runs_equal(pipelined, serial, f"{case}: pipelined against serial")
    del pipelined
    recycling = _run(lx, case, beam, "recycling", set())
    _assert_runs_equal(recycling, serial, f"{case}: recycling against serial", particles=False)
    for j in range(1, K):  # (the sequence is one: no two consecutive calls gave the same record)
        assert not _same(serial["records"][j], serial["records"][j - 1]), j
    pick = _samples(case, record_property)
    _check_serial_against_the_oracle(lx, case, serial, np.asarray(beam.particles), pick, f"{case}: serial against the oracle")
    if case == "cavity":
        monkeypatch.setenv("LYNX_TRACK_UNITS", "2")
        monkeypatch.setenv("LYNX_UNIT_PAIRS", "2")
        seg, _, _ = _segment(lx, case)
        assert np.all(np.isfinite(np.asarray(seg.track(beam).energy)))


test_pipelined_and_recycling_calls_equal_serial_ones_and_the_oracle.__doc__ += "\n" + "\n".join(f"    {k}: {v}." for k, v in REACHES.items()) + "\n"


# ---------------------------------------------------------------------------------------------------------------------
# forced forms at a small size
# ---------------------------------------------------------------------------------------------------------------------

FORCED = {"LYNX_ASYNC_BUILD": "1", "LYNX_SIDE_REDUCE": "1"}
FORCED_SETS = [{}, {"LYNX_BUILD_HOST_WAIT": "1"}, {"LYNX_BUILD_IN_TAIL": "0"}, {"LYNX_LANES_BUILD_MIN_BATCH": "1"},
               {"LYNX_HOST_VISIBLE_RECORDS": "0"}]


@pytest.mark.parametrize("extra", FORCED_SETS, ids=lambda e: "+".join(f"{k[5:].lower()}={v}" for k, v in e.items()) or "async+side")
def test_forced_pipeline_forms_at_a_small_size(lx, monkeypatch, record_property, extra):
    """
    The `cavity` lattice at B = 5, N = 6151 (a cut wave of samples, a ragged particle count, far below the half million
    from which any of this is on by default), the same 9-call sequence, under LYNX_ASYNC_BUILD=1 LYNX_SIDE_REDUCE=1
    (track_table: `async`; track_particles_t: `side`) and one more knob: the host's wait for the build
    (LYNX_BUILD_HOST_WAIT=1), no start in the tail (LYNX_BUILD_IN_TAIL=0: the build then waits for its slot's
    ev_streamed alone), the lanes build with its single scratch buffers (LYNX_LANES_BUILD_MIN_BATCH=1), records in
    device memory (LYNX_HOST_VISIBLE_RECORDS=0: lynx_track_particles_new).  Pipelined against serial under the same
    knobs bit for bit (records, energies, particles of every call); serial against the oracle, ALL samples.
    """
    case = "small"
    for key, value in {**FORCED, **extra}.items():
        monkeypatch.setenv(key, value)
    calls = set(range(pc.CASES[case]["K"]))
    beam = _incoming(lx, case)
    serial = _run(lx, case, beam, "serial", calls)
    pipelined = _run(lx, case, beam, "pipelined", calls)
    _assert_runs_equal(pipelined, serial, f"{extra}: pipelined against serial")
    recycling = _run(lx, case, beam, "recycling", set())
    _assert_runs_equal(recycling, serial, f"{extra}: recycling against serial", particles=False)
    pick = _samples(case, record_property)
    assert len(pick) == pc.CASES[case]["B"]
    _check_serial_against_the_oracle(lx, case, serial, np.asarray(beam.particles), pick, f"{extra}: serial against the oracle")


# ---------------------------------------------------------------------------------------------------------------------
# a beam from two calls back
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,knobs", [("cavity", {}), ("small", {"LYNX_ASYNC_BUILD": "1"}),
                                        ("small", {"LYNX_ASYNC_BUILD": "1", "LYNX_BUILD_IN_TAIL": "0"})],
                         ids=["defaults", "small-async", "small-async-no-tail"])
def test_a_build_that_reads_the_energy_of_a_call_two_back_waits_for_its_kernel(lx, monkeypatch, record_property, case, knobs):
    """
    up = U.track(beam); x = A.track(beam); y = B.track(up), nothing read in between, U, A, B three cavity lattices and
    U's voltages different in every sample.  The build and k_cavity_flags of the third call read `up`'s energy on
    `s_build`, the first call's streaming kernel writes it on the main stream.  Before this test there was nothing
    between them: `main_wrote` named x's energy, `main_dirty` is not set by an asynchronous call, the slot's
    ev_streamed belonged to a call three back and the tail flag says that a kernel's last workgroups have been
    DISPATCHED.  track_table now remembers which energy buffer each ring slot's kernel wrote (`slot_wrote`,
    track_particles_t) and lets the build wait for that slot's ev_streamed.

    Before each triple U runs once at other voltages and the result is dropped, so that the block `up`'s energy takes
    holds other energies.  Three triples with different voltages; y's energy, particles and moment record equal the
    serial run (a sync after every call) bit for bit and match the oracle's U-then-B chain.  A race shows only when the
    timing allows: a pass does not prove the ordering right, a failure is a finding.
    """
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    c = pc.CASES[case]
    dtype, B = c["dtype"], c["B"]
    rt = lx.device.get_runtime()
    beam = _incoming(lx, case)
    cavities = [e for e, (kind, _) in enumerate(pc.lattice("cavity", B)[0]) if kind == "cavity"]
    factors = [1.0, 0.8, 1.15]

    def run(serial):
        lattices = [_segment(lx, case, seed=s) for s in (21, 22, 23)]
        (U, u_el, _), (A, _, _), (Bs, _, _) = lattices
        volts = [np.asarray(u_el[e].voltage, dtype=np.float64).copy() for e in cavities]
        rt.sync()
        out = []
        for factor in factors:
            for e, v in zip(cavities, volts):
                u_el[e].voltage = (0.37 * v[::-1]).astype(dtype)
            junk = U.track(beam)
            del junk
            for e, v in zip(cavities, volts):
                u_el[e].voltage = (factor * v).astype(dtype)
            up = U.track(beam)
            if serial:
                rt.sync()
            x = A.track(beam)
            if serial:
                rt.sync()
            y = Bs.track(up)
            if serial:
                rt.sync()
                out.append((y._moments.host(), np.array(y._energy.host()), y._particles.host()))
            else:
                out.append(y)
            del up, x, y
        if not serial:
            out = [(y._moments.host(), np.array(y._energy.host()), y._particles.host()) for y in out]
        return out

    serial, pipelined = run(True), run(False)
    for k, (s, p) in enumerate(zip(serial, pipelined)):
        for what, a, b in zip(("moment record", "energy", "particles"), p, s):
            assert _same(a, b), (what, "of y in triple", k, _where(a, b))
    P = np.asarray(beam.particles)
    pick = _samples(case, record_property)
    descs = [pc.lattice("cavity", B, seed=s)[0] for s in (21, 23)]
    for k, factor in enumerate(factors):
        u_desc = [(kind, {**kw, "voltage": (factor * np.asarray(kw["voltage"])).astype(dtype)} if kind == "cavity" else kw)
                  for kind, kw in descs[0]]
        record, energy, particles = serial[k]
        _check_call(lx, case, [u_desc, descs[1]], P, pick, record, energy, particles, f"y of triple {k}")
    assert not _same(serial[0][1], serial[1][1])  # (the triples are told apart by y's energy)


# ---------------------------------------------------------------------------------------------------------------------
# the reverse pass in the loop
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype,B,N", [(np.float32, 300, 2000), (np.float64, 2, 300_000)], ids=["fp32-lanes-build-pairs", "fp64"])
def test_the_reverse_pass_in_a_loop_that_rewrites_k1(lx, monkeypatch, record_property, dtype, B, N):
    """
    Six steps, each: write k1 of one quadrupole, vjp = track_vjp(seg, beam), g = vjp(cov_bar=w); the gradients are held
    and read after the last step.  600 000 particles per call in both shapes: the forward build runs on the second
    stream into the ring, and the reverse pass reads the table its forward call left (lynx_ctx::FwdTable) while the next
    step's build takes the next slot.  float32, B = 300: lanes build (a cut wave of samples), merged pairs.  The lattice is
    that of test_gpu_grad.test_the_reverse_pass_reads_the_table_of_its_forward_call.  Every gradient (energy and each
    of PARAMS_TO_CHECK) equals, bit for bit, the serial run made with LYNX_BWD_REUSE_TABLE=0 (every reverse pass builds
    its own table) and a sync after every step.  float64: at two of the steps d/dk1 of the written quadrupole, one drawn
    sample, against central differences of the float64 oracle (rule and tolerance of
    test_gpu_fuzz.test_random_call_sequence_through_the_reverse_pass: 2e-4 of scale).
    """
    K = 6
    assert B * N >= pc.HALF_MILLION
    rng = np.random.default_rng(47)
    f = lambda v: np.full(B, v)  # noqa: E731
    desc = []
    for cell in range(3):
        desc += [("drift", dict(length=f(0.3))),
                 ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B), misalignment=rng.normal(0, 1e-3, (B, 2)))),
                 ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-3, B))), ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    P = o.gaussian_particles((B,), N, seed=9, dtype=np.float64, sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3]).astype(dtype)
    energy = rng.uniform(6e6, 8e6, B).astype(dtype)
    w_cov = rng.normal(size=(B, 6, 6)) * 1e3
    values = pc.written_values(B, K).astype(dtype)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    rt = lx.device.get_runtime()
    names = [(e, name) for e, (kind, kw) in enumerate(desc) for name in PARAMS_TO_CHECK.get(kind, []) if name in kw]

    def flat(g, elements):
        return [np.asarray(g.energy)] + [np.asarray(g[elements[e]][name]) for e, name in names]

    def loop(serial):
        elements, _ = make_lattice(desc, dtype, lx)
        seg = lx.Segment(elements)
        rt.sync()
        out = []
        for j in range(K):
            elements[1].k1 = values[j]
            g = lx.grad.track_vjp(seg, beam)(cov_bar=w_cov)
            if serial:
                rt.sync()
                g = flat(g, elements)
            out.append(g)
        return out if serial else [flat(g, elements) for g in out]

    pipelined = loop(False)
    monkeypatch.setenv("LYNX_BWD_REUSE_TABLE", "0")
    serial = loop(True)
    monkeypatch.delenv("LYNX_BWD_REUSE_TABLE")
    for j in range(K):
        for (e, name), a, b in zip([(-1, "energy")] + names, pipelined[j], serial[j]):
            assert _same(a, b), ("step", j, "element", e, name, _where(a, b))
    assert not _same(serial[0][1 + names.index((1, "k1"))], serial[1][1 + names.index((1, "k1"))])
    if dtype != np.float64:
        return
    seed = 20261019
    record_property("finite_difference_seed", seed)
    rng = np.random.default_rng(seed)
    bidx = int(rng.integers(B))
    P64, e64 = P.astype(np.float64), energy.astype(np.float64)
    for j in sorted(rng.choice(K, size=2, replace=False)):
        got = float(pipelined[j][1 + names.index((1, "k1"))][bidx])
        x0 = float(values[j][bidx])
        h = 1e-6 * max(abs(x0), 1e-2)
        loss = []
        for x in (x0 + h, x0 - h):
            k1 = np.asarray(values[j], dtype=np.float64).copy()
            k1[bidx] = x
            d = list(desc)
            d[1] = ("quadrupole", {**desc[1][1], "k1": k1})
            loss.append(_loss64(d, P64, e64, np.zeros((B, 6)), w_cov)[bidx])
        ref = (loss[0] - loss[1]) / (2 * h)
        scale = max(abs(ref), 1e-9 * np.max(np.abs(w_cov)))
        assert abs(got - ref) <= 2e-4 * scale + 1e-7 * np.max(np.abs(pipelined[j][1 + names.index((1, "k1"))])), (int(j), bidx, got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# several entry points on one context
# ---------------------------------------------------------------------------------------------------------------------

def test_several_entry_points_share_one_context(lx, record_property):
    """
    Fourteen operations in a seeded fixed order, each with a k1 write in front of it, over the `short` lattice
    (N = 140 001, float64: short calls, inline or on the second stream by `main_idle`), the `cavity` lattice (B = 320,
    N = 2000, float32: 640 000 particles, lanes build and k_cavity_flags on `s_build`) and a 13-element lattice a
    ParameterBeam of B = 300 goes through (its lanes path -- lynx_track_moments -- shares `scratch_products` with the
    particle builds): `track` of particles, `track` of a ParameterBeam, `track_along` (which reads its records back: a
    wait in the middle of the sequence, after which the main stream is idle), `track_vjp` with its backward half at once
    (the reverse pass reads the forward call's table: lynx_ctx::FwdTable).  Pipelined -- everything held, read after the
    last operation -- equals serial -- fresh Segments, a sync and a read after every operation -- bit for bit, entry by
    entry; the forward results of serial against the oracle on all samples.  (The ParameterBeam comes in at 100 MeV: at
    6 MeV the oracle's own float32 chain is farther than 5e-5 from its float64 chain on this lattice, and no float32
    result can be held to 1e-4 there -- test_gpu_fuzz._float32_conditioned, asserted for every written value in
    test_pipelined_host.py.)
    """
    record_property("entry_order_seed", pc.ENTRY_ORDER_SEED)
    ops = pc.entry_order()
    rt = lx.device.get_runtime()
    descs = {key: pc.lattice(sh["lattice"], sh["B"])[0] for key, sh in pc.ENTRY_SHAPES.items()}
    values = {key: pc.written_values(sh["B"], len(ops), seed=31) for key, sh in pc.ENTRY_SHAPES.items()}
    w_cov = {key: np.random.default_rng(5).normal(size=(sh["B"], 6, 6)) * 1e3 for key, sh in pc.ENTRY_SHAPES.items()}
    beams, pkw = {}, None
    for key, sh in pc.ENTRY_SHAPES.items():
        if sh["N"] is not None:
            beams[key] = lx.ParticleBeam.synthetic((sh["B"],), sh["N"], sigma=pc.SIGMA, energy=sh["energy"], seed=4, dtype=sh["dtype"])
        else:
            pkw = {k: np.full(sh["B"], v, dtype=sh["dtype"]) for k, v in pc.ENTRY_PARAMETER_SIGMA.items()}
            beams[key] = lx.ParameterBeam.from_parameters(**pkw, energy=np.full(sh["B"], sh["energy"], dtype=sh["dtype"]), dtype=sh["dtype"])
    names = {key: [(e, name) for e, (kind, kw) in enumerate(descs[key]) for name in PARAMS_TO_CHECK.get(kind, []) if name in kw]
             for key in descs}

    def read(op, key, elements, out):
        if op == "track":
            return dict(record=out._moments.host(), energy=np.array(out._energy.host()), particles=out._particles.host())
        if op == "parameter":
            return dict(mu=np.asarray(out._mu), cov=np.asarray(out._cov), energy=np.asarray(out.energy))
        if op == "along":
            res = dict(mu=np.asarray(out.mu), cov=np.asarray(out.cov), energy=np.asarray(out.energy))
            if pc.ENTRY_SHAPES[key]["N"] is not None:
                res.update(record=np.asarray(out.outgoing.moment_record()), particles=np.asarray(out.outgoing.particles),
                           energy_out=np.asarray(out.outgoing.energy))
            else:
                res.update(mu_out=np.asarray(out.outgoing._mu), cov_out=np.asarray(out.outgoing._cov), energy_out=np.asarray(out.outgoing.energy))
            return res
        vjp, g = out
        res = dict(record=vjp.outgoing._moments.host(), energy=np.array(vjp.outgoing._energy.host()), g_energy=np.asarray(g.energy))
        res.update({f"g_{e}_{name}": np.asarray(g[elements[e]][name]) for e, name in names[key]})
        return res

    def sequence(serial):
        segs = {}
        for key, sh in pc.ENTRY_SHAPES.items():
            elements, _ = make_lattice(descs[key], sh["dtype"], lx)
            segs[key] = (lx.Segment(elements), elements)
        rt.sync()
        results = []
        for i, (op, key) in enumerate(ops):
            seg, elements = segs[key]
            elements[1].k1 = values[key][i].astype(pc.ENTRY_SHAPES[key]["dtype"])
            if op in ("track", "parameter"):
                out = seg.track(beams[key])
            elif op == "along":
                out = seg.track_along(beams[key])
            else:
                vjp = lx.grad.track_vjp(seg, beams[key])
                out = (vjp, vjp(cov_bar=w_cov[key]))
            if serial:
                rt.sync()
                out = read(op, key, elements, out)
            results.append(out)
        if not serial:
            results = [read(op, key, segs[key][1], out) for (op, key), out in zip(ops, results)]
        return results

    serial, pipelined = sequence(True), sequence(False)
    for i, ((op, key), s, p) in enumerate(zip(ops, serial, pipelined)):
        assert sorted(s) == sorted(p)
        for field in s:
            assert _same(p[field], s[field]), (i, op, key, field, _where(p[field], s[field]))
    # the forward results of serial against the oracle, at the k1 each operation saw
    host = {key: np.asarray(beam.particles) for key, beam in beams.items() if pc.ENTRY_SHAPES[key]["N"] is not None}
    for i, ((op, key), s) in enumerate(zip(ops, serial)):
        sh = pc.ENTRY_SHAPES[key]
        dtype, B = sh["dtype"], sh["B"]
        desc = list(descs[key])
        desc[1] = ("quadrupole", {**desc[1][1], "k1": values[key][i]})
        what = f"operation {i}: {op} on {key}"
        if sh["N"] is None:
            fcase = dict(dtype=dtype, shape=(B,), energies=np.full(B, sh["energy"], dtype=dtype))
            ref = _oracle(fcase, pc.subset(desc, slice(None), dtype), pkw=pkw)
            mu, cov, e = (s["mu"], s["cov"], s["energy"]) if op == "parameter" else (s["mu_out"], s["cov_out"], s["energy_out"])
            from lynx_amd.device import Dual

            out = lx.ParameterBeam.__new__(lx.ParameterBeam)
            out._init_raw(Dual(mu), Dual(cov), Dual(e), beams[key].total_charge, dtype)
            _check_parameter(fcase, out, ref, what)
        else:
            energy = s["energy_out"] if op == "along" else s["energy"]
            _check_call(lx, sh, [desc], host[key], list(range(B)), s["record"], energy, s.get("particles"), what)
