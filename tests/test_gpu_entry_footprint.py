"""
WHERE every entry point writes: all of its outputs, and nothing else.  Every array of one call lives in ONE block from
lynx_buf_alloc at an interior offset (tests/entry_footprint.py: 256-aligned, a guard of max(8 KiB, its own size) on both
sides, the last one inside the block), the call runs twice on identical inputs -- over a block of 0x00, then of 0xFF --, and the
whole block is read back.  Byte for byte:
  1. outside the `out` / `inout` extents nothing has changed: guards, inputs, the other arrays;
  2. the `out` extents of the two runs are equal: every byte is written, none depends on what was there; an `inout` array
     (d_mu_bar / d_cov_bar of the two image reverse calls) changes only at the entries the header names;
  3. the `out` bytes are those of the same call into blocks of their own (`rt.empty`: the ordinary path);
  4. a moment record's slots 28..33 are 0, slot 34 is the flag the call was asked for, slot 35 is N or the survivors' count.
An overrun lands in memory the test owns; no case can fault by what it checks.  The calls and their arrays come from
tests/entry_calls.py; the checker is tested without a GPU in test_entry_footprint_host.py.

Which form of a kernel a (shape, knob) pair reaches (lynx_hip.hip: plan_track, table_unit_records, build_shape / launch_build,
trace_wave_plan, track_backward_t), on an MI355X of 256 CUs:
  * lynx_track_particles, lynx_moments.  plan_track halves the particles per lane while B * ceil(N / (256 u)) < 4 CUs = 1024
    workgroups ("small jobs"): at every shape up to (3, 1025) u = 1 whatever LYNX_UNROLL says, so the wave-tile form (which
    needs u = 16 / sizeof(T)) and the structured step loop of float32 (u = 2 or 4) are out of reach there -- the small shapes
    run k_track_direct<u = 1, per-particle accesses>, one 256-particle tile per workgroup and 1 / 1 / 2 / 5 workgroups per
    sample for N = 63, 65 / 257 / 1025, with a ragged last tile every time; LYNX_MOM 2 / 3 picks the float32 moment mode (3 by
    default here: a lane sees one particle).  (114, 8193) is the smallest shape of the suite that keeps u: float32 u = 2 (its
    default for a program of several steps) and, where LYNX_UNROLL asks, u = 4 (114 * 9 = 1026 workgroups); float64 u = 2.
    There LYNX_XPOSE = 1 with LYNX_UNROLL = 4 (float32) / 2 (float64) is the wave-tile kernel with a cut last tile
    (8193 = 32 * 256 + 1) -- with any other LYNX_UNROLL plan_track clears xpose (u != 16 / sizeof(T)) and the call is the
    LYNX_XPOSE = 0 one, so those pairs are not run --, LYNX_XPOSE = 0 with LYNX_UNROLL 1 / 2 / 4 the per-particle forms.
    Float32 with u = 2 or 4 takes the structured step loop (LYNX_TRACK_UNITS = 2 insists, 0 keeps k_track_direct), and
    which kernel of it depends on the lattice:
      cavity lattice (units: aperture, [drift, cavity], quadrupole -- pair[] = 0, 1, 0): k_track_units, the general unit
        kernel, [run, cavity] merged (default) or step by step (LYNX_MERGE_STEPS = 0).  Not every unit is a pair, so
        k_track_unit_pairs is out of reach here and LYNX_UNIT_PAIRS changes nothing: not run on this lattice.
      pairs lattice (units: [drift, cavity], [quadrupole, cavity], both class U): k_track_unit_pairs by default
        (LYNX_UNIT_PAIRS = 2 insists: an error if the call takes another kernel), LYNX_UNIT_PAIRS = 0 the general unit kernel,
        LYNX_MERGE_STEPS = 0 four units of one step, LYNX_TRACK_UNITS = 0 the dense loop.
    An observer step keeps k_track_direct (table_unit_records: n_observers == 0).
  * the table builds.  B < 256 takes the workgroup build (k_build); LYNX_LANES_BUILD_MIN_BATCH = 1 the lanes = samples build
    (one piece of 8 elements here), with LYNX_PIECE = 1 one element per piece and a pair tree of two levels over the 4 / 5
    elements of these lattices.
  * the particle traces.  trace_wave_plan: one wave per tile of 64 * (16 / sizeof(T)) particles, rounded up to workgroups of
    four waves: N = 63, 65 one tile (cut), N = 257 two tiles in float32 (one whole, one of a single particle) and three in
    float64, N = 1025 five / nine; (114, 8193): 27 waves wanted, 33 / 65 tiles, two / three tiles per wave.
    k_trace_finalize<256> everywhere (waves <= 256).
  * lynx_track_particles_backward, on the marked, the cavity and the pairs lattice (every unit of all three is proposed as
    class U: identity, drift, untilted quadrupole, cavity).  float32: two particles per lane (LYNX_BWD_PAIRS = 0: one, and
    with it the dense kernel without merged pairs); the structured kernel k_track_bwd_units (LYNX_BWD_UNITS = 0: the dense
    k_track_bwd); on the cavity and the pairs lattice [run, cavity] merged into one unit (plan_bwd_units; LYNX_BWD_MERGE = 0:
    every step a unit) -- the marked lattice has no cavity, and LYNX_BWD_MERGE changes nothing there.  float64: the dense
    kernel, step by step, which these knobs leave alone.  The other reverse entries read none of the LYNX_BWD_* knobs and
    are not run under them.
  Knobs that choose among float32 kernels only (LYNX_MOM, LYNX_TRACK_UNITS, LYNX_UNIT_PAIRS, LYNX_MERGE_STEPS, LYNX_BWD_*) run in
  float32 only.

No output is compared under a mask.  The one candidate was the step table of lynx_build_compose, whose header line names 57
of a row's 64 slots ("per step: 49 map entries + 8 cavity coefficients"): every build form writes all 64 of every row, run
steps and cavity steps alike (measured over blocks of 0x00 and of 0xFF: no slot differs), so its rows are held to checks 2
and 3 whole.

Every writer invalidates the forward table: test_every_writer_over_the_forward_energy_... below.
"""

import ctypes as C

import numpy as np
import pytest

from . import entry_calls as ec
from . import entry_footprint as fp

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
# (batch, particles): N odd, so that a sample's particles do not start on 16 bytes; 257 and 1025 lie just behind a float32
# tile of 256 and of 256 x 4.  Image cells and chosen particles ride along: 1 x 1, 5 x 3, 67 x 3; one, or three with a repeat.
SMALL = [(1, 1, 1, 1, 1), (3, 63, 5, 3, 3), (3, 65, 67, 3, 3), (2, 257, 5, 3, 1), (3, 1025, 5, 3, 3)]
LARGE = (114, 8193, 5, 3, 1)  # test_gpu_covariance.py's shape: the smallest that keeps two and four particles per lane

# entry -> (the array of moment records, slot 34, what slot 35 counts)
RECORDS = {
    "lynx_track_particles": ("mom", 0, "N"), "lynx_track_particles[covariance]": ("copy", 1, "N"),
    "lynx_track_particles[shared input]": ("copy", 0, "N"), "lynx_track_particles[observer]": ("copy", 0, "N"),
    "lynx_moments": ("copy", 1, "N"), "lynx_moments[properties]": ("copy", 0, "N"), "lynx_moments_by_loss": ("sets_out", 1, "sets"),
    "lynx_track_particles_along": ("records_out", 1, "N"), "lynx_track_particles_along[moments only, shared input]": ("records_out", 1, "N"),
    "lynx_track_particles_along_losses": ("records_out", 1, "alive"), "lynx_track_particles_along_losses[shared limits]": ("records_out", 1, "alive"),
    "lynx_track_particles_along_screens": ("records_out", 1, "alive"), "lynx_track_particles_along_screens[two screens]": ("records_out", 1, "N"),
    "lynx_track_particles_along_trajectories": ("records_out", 1, "N"), "lynx_track_particles_along_trajectories[no p_out]": ("records_out", 1, "alive"),
}

_envs = {}


def env_of(shape, dtype):
    """The arrays and the lattice of one (shape, dtype), made once for the module."""
    key = (shape, np.dtype(dtype))
    if key not in _envs:
        # (the reverse entries' inputs: not for the lattices and the large shape that only forward calls run at)
        _envs[key] = ec.make_env(shape, dtype, prelude=shape.lattice not in ("observer", "empty") and shape.N < 4096)
    return _envs[key]


@pytest.fixture(scope="module", autouse=True)
def _library(built_library):
    yield
    _envs.clear()


def lattices_of(entry):
    if entry in ec.ONLY_OBSERVER:
        return ["observer"]
    out = ["marked"]
    if entry in ec.ADMIT_CAVITY:
        out.append("cavity")
    if entry in ec.ADMIT_PAIRS:
        out.append("pairs")
    if entry in ("lynx_track_particles", "lynx_track_particles[no moments]"):
        out.append("empty")  # n_steps == 0: accepted, and d_energy_out is the incoming energy
    return out


class ArenaCall:
    """One entry's call with every array inside one block."""

    def __init__(self, env, entry, alias=None):
        self.env, self.entry, self.rt = env, entry, env.rt
        self.call = ec.ALL_ENTRIES[entry][0]
        self.arrays = ec.entry_arrays(entry, env.shape, env.dtype)
        self.arena = fp.plan_arena(self.arrays, alias)
        fp.check_plan(self.arena)
        self.alias = alias or {}
        self.base = self.rt.alloc(self.arena.nbytes)
        self.partial = None
        if entry == "lynx_aperture_compact":  # "d_kept [total][7] survivors and d_lost [N - total][7] lost particles" of sample 0
            total, row = int(env.host["totals"][0]), 7 * env.dtype.itemsize
            self.partial = {"kept": total * row, "lost": (env.shape.N - total) * row}

    def pointer(self, name, offset=0):
        return C.c_void_p(self.base + self.arena.regions[name].start + offset)

    def fill(self, value):
        """The whole block `value`, then the inputs (and what an `inout` array holds before the call); returns the block
        as the host expects it to be."""
        rt, arena = self.rt, self.arena
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(self.base), value, arena.nbytes))
        before = np.full(arena.nbytes, value, dtype=np.uint8)
        for a in self.arrays:
            if a.role == "out" or a.name in self.alias:  # (an aliased output: its bytes are its input's)
                continue
            host = np.ascontiguousarray(self.env.host[a.name])
            assert (host.dtype, host.shape) == (a.dtype, a.shape), (a.name, host.dtype, host.shape)
            arena.view(before, a.name)[...] = host
            if host.nbytes:
                rt.check(rt.lib.lynx_buf_h2d(rt.ctx, self.pointer(a.name), host.ctypes.data, host.nbytes))
        return before

    def run(self):
        """The call; returns the whole block read back."""
        rt, env = self.rt, self.env
        a = ec.arguments(self.entry, self.pointer, env.shape)
        status = self.call(rt.lib, rt.ctx, env.lat.handle, env.code, a, env.shape)
        assert status == 0, (self.entry, rt.lib.lynx_last_error(rt.ctx).decode())
        after = np.empty(self.arena.nbytes, dtype=np.uint8)
        rt.check(rt.lib.lynx_buf_d2h(rt.ctx, after.ctypes.data, C.c_void_p(self.base), after.nbytes))
        return after

    def close(self):
        self.rt.sync()  # (the allocator tracks blocks in flight by their exact pointer: nothing of this one is, now)
        self.rt.free(self.base)


def ordinary(env, entry):
    """The same call into blocks of their own (what `rt.empty` hands out: recycled, not zeroed): name -> host array."""
    rt = env.rt
    arrays = ec.entry_arrays(entry, env.shape, env.dtype)
    for a in arrays:
        if a.role == "inout":
            host = np.ascontiguousarray(env.host[a.name])
            rt.check(rt.lib.lynx_buf_h2d(rt.ctx, C.c_void_p(env.a[a.name].ptr), host.ctypes.data, host.nbytes))
    args = ec.arguments(entry, lambda name: C.c_void_p(env.a[name].ptr), env.shape)
    status = ec.ALL_ENTRIES[entry][0](rt.lib, rt.ctx, env.lat.handle, env.code, args, env.shape)
    assert status == 0, (entry, rt.lib.lynx_last_error(rt.ctx).decode())
    return {a.name: env.a[a.name].numpy() for a in arrays if a.role != "in"}


def allowed_entries(env, entry, name):
    """Where an `inout` array may change: the named entries of the rows of the screens' points."""
    s = env.shape
    region_shape = ec.array_specs(s, env.dtype)[name][1]
    allowed = np.zeros(region_shape, dtype=bool)
    allowed[:, s.SCREEN[0], list(ec.INOUT[entry][name])] = True
    return allowed


def check_records(env, entry, out):
    if entry not in RECORDS:
        return
    name, flag, counting = RECORDS[entry]
    s = env.shape
    records = out[name].reshape(s.B, -1, 36)
    if counting == "N":
        counts = np.full(records.shape[:2], s.N)
    elif counting == "sets":  # set 0 is everyone, set 1 whoever the first aperture left
        counts = np.stack([np.full(s.B, s.N), (env.host["lost_at"] != 0).sum(axis=1)], axis=1)
    else:  # the aperture at step 0 tests who enters it: everyone at point 0, the survivors behind
        alive = (out["lost_out"] == -1).sum(axis=1)
        counts = np.concatenate([np.full((s.B, 1), s.N), np.repeat(alive[:, None], s.P - 1, axis=1)], axis=1)
    fp.moment_record_constants(records, counts=counts, whole_triangle=bool(flag))


def footprint(env, entry, alias=None):
    """Checks 1 .. 4 of the module's docstring for one call; returns its outputs by name."""
    job = ArenaCall(env, entry, alias)
    try:
        arena, runs = job.arena, []
        for value in (0x00, 0xFF):
            before = job.fill(value)
            after = job.run()
            fp.nothing_else_written(arena, before, after, job.partial)
            for name in ec.INOUT.get(entry, {}):
                fp.inout_changed_only(arena, before, after, name, allowed_entries(env, entry, name))
                assert not np.array_equal(arena.view(before, name), arena.view(after, name), equal_nan=True), f"{name}: nothing was added"
            runs.append(after)
        fp.outputs_identical(arena, runs[0], runs[1], job.partial)
        for name in ec.INOUT.get(entry, {}):  # the prior content is data: the same in both runs, so is the result
            fp.same_as(arena, runs[0], name, arena.view(runs[1], name))
        reference = ordinary(env, entry)  # (always out of place)
        for name, expected in reference.items():
            fp.same_as(arena, runs[1], name, expected, (job.partial or {}).get(name))
        out = {name: arena.view(runs[1], name).copy() for name in reference}
        check_records(env, entry, out)
        if env.shape.lattice == "empty" and "e_out" in out:  # a program without steps: the beam leaves as it came
            assert out["e_out"].tobytes() == env.host["e_in"].tobytes()
        assert any(block.view(np.uint8).any() for block in out.values()), "the call wrote nothing"
        return out
    finally:
        job.close()


def small_shapes(lattice):
    return [ec.Shape(*row, lattice) for row in SMALL]


def each_case(entry, dtype, shapes=None):
    """(env) for every shape and lattice the entry runs at; a failure says which."""
    for lattice in lattices_of(entry):
        for shape in shapes or small_shapes(lattice):
            if shape.lattice != lattice:
                shape = shape._replace(lattice=lattice)
            yield env_of(shape, dtype)


def at(env, knobs=None):
    s = env.shape
    return f"[B = {s.B}, N = {s.N}, {s.NX} x {s.NY} cells, {s.CHOSEN} chosen, {s.lattice} lattice, {env.dtype.name}{', ' + str(knobs) if knobs else ''}] "


def run_cases(cases, knobs=None):
    for env, entry, alias in cases:
        try:
            footprint(env, entry, alias)
        except AssertionError as failure:
            raise AssertionError(at(env, knobs) + entry + ": " + str(failure)) from None


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("entry", sorted(ec.ALL_ENTRIES))
def test_an_entry_point_writes_all_of_its_outputs_and_nothing_else(entry, dtype):
    run_cases((env, entry, None) for env in each_case(entry, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_track_particles_refuses_an_outgoing_energy_without_an_incoming_one_on_a_program_without_steps(dtype):
    """include/lynx_hip.h: d_energy_in may be NULL for a program without steps, unless d_energy_out is given (which is then a
    copy of it)."""
    env = env_of(ec.Shape(2, 65, 1, 1, 1, "empty"), dtype)
    rt, p = env.rt, lambda name: C.c_void_p(env.a[name].ptr)  # noqa: E731
    status = rt.lib.lynx_track_particles(rt.ctx, env.lat.handle, 65, None, p("p_in"), p("p_out"), p("e_out"), None, 0, None)
    assert (status, rt.lib.lynx_last_error(rt.ctx).decode()) == (-1, "energy_in required")
    rt.check(rt.lib.lynx_track_particles(rt.ctx, env.lat.handle, 65, None, p("p_in"), p("p_out"), None, None, 0, None))
    assert env.a["p_out"].numpy().tobytes() == env.host["p_in"].tobytes()


# ---- the other forms of the kernels --------------------------------------------------------------------------------------

FORWARD = ["lynx_track_particles", "lynx_track_particles[covariance]", "lynx_track_particles[shared input]", "lynx_track_particles[no moments]"]
BUILDERS = FORWARD + ["lynx_track_moments", "lynx_track_moments_along", "lynx_build_compose", "lynx_track_particles_along",
                      "lynx_track_particles_along_losses", "lynx_track_particles_along_trajectories", "lynx_track_particles_backward",
                      "lynx_track_moments_backward", "lynx_track_moments_along_backward", "lynx_track_particles_along_backward",
                      "lynx_track_particles_along_backward_cavities", "lynx_track_particles_along_backward_losses",
                      "lynx_track_particles_along_backward_trajectories"]
REVERSE = ["lynx_track_particles_backward"]  # (the one entry that reads the LYNX_BWD_* knobs: track_backward_t)
MOMENTS = FORWARD[:3] + ["lynx_moments", "lynx_moments[properties]"]
F32, F64 = np.float32, np.float64
# (knobs, the entries they reach at the small shapes, the dtype).  LYNX_MOM and the LYNX_BWD_* knobs choose among float32
# kernels only; LYNX_TRACK_UNITS, LYNX_UNIT_PAIRS and LYNX_MERGE_STEPS need two particles per lane: the large shape below.
KNOBS_SMALL = ([({"LYNX_MOM": m}, MOMENTS, F32) for m in "23"]
               + [(k, BUILDERS, t) for k in ({"LYNX_LANES_BUILD_MIN_BATCH": "1"}, {"LYNX_LANES_BUILD_MIN_BATCH": "1", "LYNX_PIECE": "1"}) for t in (F32, F64)]
               + [(k, REVERSE, F32) for k in ({"LYNX_BWD_UNITS": "0"}, {"LYNX_BWD_UNITS": "1"}, {"LYNX_BWD_PAIRS": "0"}, {"LYNX_BWD_MERGE": "0"})])
SMALL_FOR_KNOBS = [(3, 65, 5, 3, 3), (2, 257, 5, 3, 1)]


def knob_id(knobs):
    return ",".join(f"{key[5:]}={value}" for key, value in knobs.items())


@pytest.mark.parametrize("knobs, entries, dtype", KNOBS_SMALL, ids=[f"{knob_id(k)}-{np.dtype(t).name}" for k, _, t in KNOBS_SMALL])
def test_the_other_forms_of_a_kernel_write_the_same_footprint_at_the_small_shapes(knobs, entries, dtype, monkeypatch):
    """The arena run against the ordinary call under the same knobs (the forms differ in rounding, not in where they write)."""
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    for entry in entries:
        shapes = [ec.Shape(*row) for row in SMALL_FOR_KNOBS]
        run_cases(((env, entry, None) for env in each_case(entry, dtype, shapes) if env.shape.lattice != "empty"), knobs)


# (lattice, knobs, dtype) at (114, 8193): the pairs of the docstring that reach a form of their own
KNOBS_LARGE = ([("cavity", k, F32) for k in [{}] + [{"LYNX_XPOSE": "0", "LYNX_UNROLL": u} for u in "124"] + [{"LYNX_XPOSE": "1", "LYNX_UNROLL": "4"}]
                + [{"LYNX_MOM": "2"}, {"LYNX_MOM": "3"}, {"LYNX_TRACK_UNITS": "0"}, {"LYNX_TRACK_UNITS": "2"}, {"LYNX_MERGE_STEPS": "0"}]]
               + [("cavity", k, F64) for k in [{}] + [{"LYNX_XPOSE": "0", "LYNX_UNROLL": u} for u in "12"] + [{"LYNX_XPOSE": "1", "LYNX_UNROLL": "2"}]]
               + [("pairs", k, F32) for k in [{}, {"LYNX_UNIT_PAIRS": "2"}, {"LYNX_UNIT_PAIRS": "0"}, {"LYNX_MERGE_STEPS": "0"}, {"LYNX_TRACK_UNITS": "0"}]])


@pytest.mark.parametrize("lattice, knobs, dtype", KNOBS_LARGE,
                         ids=[f"{lattice}-{knob_id(k) or 'default'}-{np.dtype(t).name}" for lattice, k, t in KNOBS_LARGE])
def test_the_forms_that_keep_two_and_four_particles_per_lane_write_the_same_footprint(lattice, knobs, dtype, monkeypatch):
    """(114, 8193): lynx_track_particles under the plan knobs on the cavity lattice (the general unit kernel in float32) and on
    the lattice of nothing but [run, cavity] pairs (the kernel for that form; LYNX_UNIT_PAIRS = 2 insists on it)."""
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    env = env_of(ec.Shape(*LARGE, lattice), dtype)
    run_cases([(env, "lynx_track_particles", None)], knobs)
    if not knobs and lattice == "cavity":  # the trace reads none of these knobs: once; and the forward call on five steps without a cavity
        marked = env_of(ec.Shape(*LARGE, "marked"), dtype)
        run_cases([(env, "lynx_track_particles_along", None), (marked, "lynx_track_particles_along", None), (marked, "lynx_track_particles", None)])


# ---- in place ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("entry, alias", [("lynx_track_moments", {"mu_out": "mu_in", "cov_out": "cov_in"}),
                                          ("lynx_track_particles_along", {"p_out": "p_in"})],
                         ids=["lynx_track_moments", "lynx_track_particles_along"])
def test_a_call_in_place_gives_the_bytes_of_the_call_out_of_place_and_writes_nothing_else(entry, alias, dtype):
    """include/lynx_hip.h: "d_mu [B][7], d_cov [B][7][7] (in/out may alias)"; "d_p_out ... (may alias d_p_in unless that is shared)"."""
    for env in each_case(entry, dtype):
        try:
            footprint(env, entry, alias)
        except AssertionError as failure:
            raise AssertionError(at(env) + entry + " in place: " + str(failure)) from None


# ---- every writer invalidates the forward table ---------------------------------------------------------------------------

MUST_NOT_BE_SKIPPED = {("lynx_track_moments", "e_out"), ("lynx_buf_d2d", "copy")}


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_every_writer_over_the_forward_energy_makes_the_reverse_pass_build_its_own_table(dtype, monkeypatch, capsys):
    """
    The reverse pass of lynx_track_particles reuses the forward call's step table while nothing has written the forward
    call's incoming energy E since (lynx_ctx::FwdTable::written, fed by what every entry point declares as its outputs).
    For every entry, every `out` / `inout` array of at least B scalars and E laid over its first or its last B scalars:
    forward call on E, the entry (which overwrites E), reverse pass on E.  With LYNX_BWD_REUSE_TABLE = 1 the gradients are
    those of LYNX_BWD_REUSE_TABLE = 0, bit for bit; E no longer holds the forward call's energies; and the gradients differ
    from the stale table's -- where they happen not to, the combination proves nothing and is skipped (printed; at most one
    in ten, and never the two writers whose declaration NOTES.md found no test for).  The lattice has no cavity: whatever
    the entry leaves in E -- NaN, integers, zero -- reaches only igamma2 of the drifts and the quadrupole.
    """
    from lynx_amd import _ffi

    monkeypatch.setenv("LYNX_BWD_MERGE", "0")
    env = env_of(ec.Shape(3, 65, 5, 3, 3, "marked"), dtype)
    rt, s, es = env.rt, env.shape, env.dtype.itemsize
    p = lambda name: C.c_void_p(env.a[name].ptr)  # noqa: E731
    e1 = np.random.default_rng(61).uniform(6e6, 8e6, s.B).astype(env.dtype)
    flags = _ffi.TRACK_MOMENTS | _ffi.TRACK_SEQUENTIAL_STEPS
    own = {name: rt.empty(shape, t) for name, (t, shape) in dict(p_out=(env.dtype, (s.B, s.N, 7)), mom=(np.float64, (s.B, 36)),
                                                                 g_par=(env.dtype, (s.B, s.E, 8)), g_en=(env.dtype, (s.B,))).items()}
    q = lambda name: C.c_void_p(own[name].ptr)  # noqa: E731

    def sequence(job, energy, reuse, overwrite):
        monkeypatch.setenv("LYNX_BWD_REUSE_TABLE", reuse)
        job.fill(0x00)
        rt.check(rt.lib.lynx_buf_h2d(rt.ctx, energy, e1.ctypes.data, e1.nbytes))
        rt.check(rt.lib.lynx_track_particles(rt.ctx, env.lat.handle, s.N, energy, p("p_in"), q("p_out"), None, q("mom"), flags, None))
        if overwrite:
            a = ec.arguments(job.entry, job.pointer, s)
            status = job.call(rt.lib, rt.ctx, env.lat.handle, env.code, a, s)
            assert status == 0, rt.lib.lynx_last_error(rt.ctx).decode()
        rt.check(rt.lib.lynx_track_particles_backward(rt.ctx, env.lat.handle, s.N, energy, p("p_in"), q("mom"), p("g_mom"), q("g_par"),
                                                      q("g_en"), None, None))
        held = np.empty(s.B, dtype=env.dtype)
        rt.check(rt.lib.lynx_buf_d2h(rt.ctx, held.ctypes.data, energy, held.nbytes))
        return own["g_par"].numpy(), own["g_en"].numpy(), held

    combinations, skipped, failures = 0, [], []
    for entry in sorted(ec.ALL_ENTRIES):
        if "marked" not in lattices_of(entry):
            continue
        job = ArenaCall(env, entry)
        try:
            for a in job.arrays:
                extent = (job.partial or {}).get(a.name, ec.nbytes(a))
                if a.role == "in" or extent < s.B * es:
                    continue
                first, last = 0, (extent - s.B * es) // es * es
                if a.role == "inout":  # the entries the call adds to: the first one on, up to the last one
                    changed = np.flatnonzero(allowed_entries(env, entry, a.name).reshape(-1))
                    first, last = int(changed[0]) * es, (int(changed[-1]) + 1 - s.B) * es
                for placement, offset in (("first", first), ("last", last)):
                    combinations += 1
                    energy = job.pointer(a.name, offset)
                    stale = sequence(job, energy, "1", overwrite=False)
                    fresh = sequence(job, energy, "0", overwrite=True)
                    reused = sequence(job, energy, "1", overwrite=True)
                    what = f"{entry}: E over the {placement} {s.B} scalars of {a.name}"
                    if not np.array_equal(stale[2], e1):
                        failures.append(what + ": the forward and the reverse pass alone changed E")
                    elif np.array_equal(fresh[2], e1, equal_nan=False) or not np.array_equal(fresh[2].view(np.uint8), reused[2].view(np.uint8)):
                        failures.append(what + f": E holds {fresh[2]} / {reused[2]} behind the entry, {e1} in front of it")
                    elif not (np.array_equal(reused[0], fresh[0], equal_nan=True) and np.array_equal(reused[1], fresh[1], equal_nan=True)):
                        failures.append(what + ": the reverse pass read the stale table")
                    elif np.array_equal(fresh[0], stale[0], equal_nan=True):
                        skipped.append((entry, a.name, placement))
        finally:
            job.close()
    with capsys.disabled():
        print(f"\n{combinations} combinations, {len(skipped)} skipped (the gradients at the new E are those at the old one): {skipped}")
    assert not failures, "\n".join(failures)
    assert 10 * len(skipped) <= combinations, skipped
    assert not {(entry, name) for entry, name, _ in skipped} & MUST_NOT_BE_SKIPPED, skipped
    assert combinations >= 2 * len(ec.ALL_ENTRIES) - 8
