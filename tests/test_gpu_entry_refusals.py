"""
What the entry points that take device pointers refuse, beside the particle trace's three (test_gpu_trace_refusals.py), called
through the C ABI: one valid call, one refused call -- a null output or a count of 0 --, and the same valid call again.  The
refusal is LYNX_ERR_INVALID with the library's exact message, and the valid call afterwards returns the bytes it returned
before.  Every refused argument is caught by a host check in front of the entry's first launch (lynx_hip.hip: the `if` lines
at the head of each entry), so no case reaches a kernel with a bad pointer.

`lynx_buf_d2d` and `lynx_buf_memset` check nothing but their context -- zero bytes is a valid call that does nothing --: their
refused call is the one without a context, and the zero-byte call is asserted to leave the destination alone.

`lynx_track_moments` also refuses a batch above 2^31 - 1 ("batch too large"); `lynx_lattice_create` allocates a parameter pool
and, for every element, validates offsets against `batch`, but no per-sample memory when every element's batch stride is 0:
the case makes such a handle and never launches on it.

Lattice: an inactive aperture (an identity step, which the reverse pass with losses may name), a drift and a quadrupole, every
element a step of its own; batch 2, 64 particles, both dtypes.
"""

import ctypes as C

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .test_gpu_trace import SIGMA

pytestmark = pytest.mark.gpu

INVALID = -1  # LYNX_ERR_INVALID
B, N, S, E, NX, NY, CHOSEN, GRAD_PARAMS = 2, 64, 3, 3, 5, 3, 2, 8
P = S + 1
F64 = np.dtype(np.float64)


class Env:
    """The runtime, the lattice and every device array the calls name, for one dtype."""


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["float32", "float64"])
def env(built_library, request):
    import lynx_amd as lx
    from lynx_amd import _ffi, engine

    rt = lx.device.get_runtime()  # raises loudly without a GPU
    dtype = np.dtype(request.param)
    one = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    leaves = [lx.Aperture(x_max=one(1e-2), y_max=one(1e-2), is_active=False, name="AP", dtype=dtype),
              lx.Drift(np.full(B, 0.7, dtype=dtype), dtype=dtype),
              lx.Quadrupole(np.full(B, 0.2, dtype=dtype), k1=np.array([4.2, -3.0], dtype=dtype), dtype=dtype)]
    e = Env()
    e.rt, e.dtype, e.code, e.leaves = rt, dtype, _ffi.F64 if dtype == F64 else _ffi.F32, leaves
    e.cache = engine.LatticeCache()
    energy = np.full(B, 1e8, dtype=dtype)
    e.lat = engine._ready(e.cache, engine.trace_program(leaves), (B,), dtype, energy)
    assert e.lat.S == S and e.lat.E == E and e.lat.B == B
    particles = o.gaussian_particles((B,), N, seed=5, dtype=dtype, sigma=SIGMA)
    mu = particles.mean(axis=1)
    centred = particles - mu[:, None, :]
    cov = np.einsum("bni,bnj->bij", centred, centred) / N
    rng = np.random.default_rng(11)
    small = lambda *shape, t=dtype: (1e-3 * rng.standard_normal(shape)).astype(t)  # noqa: E731
    up, empty = rt.to_device, rt.empty
    e.a = dict(  # device arrays by name, kept alive for the module
        e_in=up(energy), p_in=up(particles), mu_in=up(mu.astype(dtype)), cov_in=up(cov.astype(dtype)),
        p_out=empty((B, N, 7), dtype), e_out=empty((B,), dtype), mom=empty((B, 36), F64),
        mu_out=empty((B, 7), dtype), cov_out=empty((B, 49), dtype),
        mu_tr=empty((B, P, 7), dtype), cov_tr=empty((B, P, 49), dtype), e_tr=empty((B, P), dtype),
        records=empty((B, P, 36), F64), lost_at=empty((B, N), np.int32), set_records=empty((B, 2, 36), F64),
        limits=up(np.full((1, 2), 1e-2, dtype=dtype)),
        chosen=up(np.array([0, 5], dtype=np.int64)), traj=empty((B, P, CHOSEN, 7), dtype),
        g_mom=up(small(B, 36, t=F64)), g_records=up(small(B, P, 36, t=F64)), traj_bar=up(small(B, P, CHOSEN, 7, t=F64)),
        mu_bar=up(small(B, 7)), cov_bar=up(small(B, 49)), mu_bar_tr=up(small(B, P, 7)), cov_bar_tr=up(small(B, P, 49)),
        g_params=empty((B, E, GRAD_PARAMS), dtype), g_e=empty((B,), dtype), g_p=empty((B, N, 7), dtype),
        g_mu=empty((B, 7), dtype), g_cov=empty((B, 49), dtype), g_chosen=empty((B, CHOSEN, 7), dtype),
        steps=empty((B, S, 64), dtype),
        xedges=up(np.linspace(-3e-4, 3e-4, NX + 1).astype(dtype)), yedges=up(np.linspace(-3e-4, 3e-4, NY + 1).astype(dtype)),
        hist=empty((B, NX * NY), np.int32),
        x_max=up(one(1e-4)), y_max=up(one(1e-4)), mask=empty((B, N), np.uint8), counts=empty((B, 1), np.int32),
        offsets=empty((B, 1), np.int64), totals=empty((B,), np.int64), kept=empty((N, 7), dtype), lost=empty((N, 7), dtype),
        xs=up(np.linspace(-3e-4, 3e-4, NX).astype(dtype)), ys=up(np.linspace(-3e-4, 3e-4, NY).astype(dtype)),
        image=empty((B, NX * NY), dtype),
        grid=up(np.concatenate([np.linspace(-3e-4, 3e-4, NX), np.linspace(-3e-4, 3e-4, NY)]).astype(dtype)),
        misalignment=up(np.zeros((1, 2), dtype=dtype)), images=empty((B, NX * NY), dtype), images_bar=up(small(B, NX * NY)),
        mu_bar_out=empty((B, P, 7), dtype), cov_bar_out=empty((B, P, 49), dtype), g_mis=empty((B, 1, 2), dtype),
        fill=empty((B, N, 7), dtype),
        gauss_rows=up(np.tile(np.concatenate([np.zeros(6), np.diag(SIGMA)[np.tril_indices(6)]]), (B, 1)).astype(F64)),
        transform_rows=up(np.tile(np.concatenate([np.zeros(6), SIGMA, 2 * np.asarray(SIGMA), np.full(6, 1e-5)]), (B, 1)).astype(dtype)),
        copy=empty((B, 36), F64), sets_out=empty((B, 2, 36), F64))
    lib, ctx, lat, p = rt.lib, rt.ctx, e.lat.handle, lambda name: C.c_void_p(e.a[name].ptr)  # noqa: E731
    # what the reverse passes read: the forward call's moment records, the trace's records, the trace with losses' lost_at and
    # survivor-set records, the chosen particles' trajectories
    rt.check(lib.lynx_track_particles(ctx, lat, N, p("e_in"), p("p_in"), p("p_out"), None, p("mom"), _ffi.TRACK_MOMENTS, None))
    rt.check(lib.lynx_track_particles_along(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0))
    rt.check(lib.lynx_track_particles_along_losses(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0, 1,
                                                   (C.c_int32 * 2)(0, 0), p("limits"), 0, p("lost_at")))
    rt.check(lib.lynx_moments_by_loss(ctx, e.code, B, N, p("p_in"), 0, 1, p("lost_at"), p("set_records")))
    rt.check(lib.lynx_track_particles_along_trajectories(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0,
                                                         -1, None, None, 0, None, -1, None, None, None, 0, None,
                                                         CHOSEN, p("chosen"), p("traj"), None))
    rt.check(lib.lynx_track_moments_along(ctx, lat, p("e_in"), p("mu_in"), p("cov_in"), p("mu_tr"), p("cov_tr"), p("e_tr")))
    rt.sync()
    e.keep = {name: e.a[name].numpy().tobytes() for name in ("mom", "records", "lost_at", "set_records", "traj", "mu_tr", "cov_tr")}
    return e


SCREEN = [2, NX, NY]  # a screen at point 2 of the trace
ints = lambda values: (C.c_int32 * len(values))(*values)  # noqa: E731
doubles = lambda values: (C.c_double * len(values))(*values)  # noqa: E731

# entry -> (the call from the named arguments, the arguments of a valid call, what it writes, the refused change, the message).
# An argument that names a device array of the fixture is passed as its pointer; None is a null pointer.
ENTRIES = {
    "lynx_track_particles": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles(ctx, lat, a["n"], a["e_in"], a["p_in"], a["p_out"], a["e_out"], a["mom"], 1, None),
        dict(n=N, e_in="e_in", p_in="p_in", p_out="p_out", e_out="e_out", mom="mom"), ["p_out", "e_out", "mom"],
        dict(n=0), "n_particles must be > 0"),
    "lynx_track_particles_backward": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles_backward(ctx, lat, N, a["e_in"], a["p_in"], a["mom"], a["g_mom"], a["g_params"],
                                                                         a["g_e"], a["g_p"], None),
        dict(e_in="e_in", p_in="p_in", mom="mom", g_mom="g_mom", g_params="g_params", g_e="g_e", g_p="g_p"), ["g_params", "g_e", "g_p"],
        dict(g_params=None), "null argument"),
    "lynx_track_moments": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_moments(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_out"], a["cov_out"], a["e_out"]),
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_out="mu_out", cov_out="cov_out", e_out="e_out"), ["mu_out", "cov_out", "e_out"],
        dict(mu_out=None), "null argument"),
    "lynx_track_moments_backward": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_moments_backward(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_bar"], a["cov_bar"],
                                                                       a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_bar="mu_bar", cov_bar="cov_bar", g_params="g_params", g_e="g_e", g_mu="g_mu",
             g_cov="g_cov"), ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_moments_along": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_moments_along(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_tr"], a["cov_tr"], a["e_tr"]),
        # (into blocks of the right sizes that nothing else of the module reads)
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_tr="mu_bar_out", cov_tr="cov_bar_out", e_tr="e_tr"),
        ["mu_bar_out", "cov_bar_out", "e_tr"],
        dict(mu_tr=None), "null argument"),
    "lynx_track_moments_along_backward": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_moments_along_backward(ctx, lat, a["e_in"], a["mu_tr"], a["cov_tr"], a["mu_bar_tr"],
                                                                             a["cov_bar_tr"], None, a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", mu_tr="mu_tr", cov_tr="cov_tr", mu_bar_tr="mu_bar_tr", cov_bar_tr="cov_bar_tr", g_params="g_params", g_e="g_e",
             g_mu="g_mu", g_cov="g_cov"), ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_particles_along_backward": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles_along_backward(ctx, lat, N, a["e_in"], a["records"], a["g_records"], None,
                                                                               a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", records="records", g_records="g_records", g_params="g_params", g_e="g_e", g_mu="g_mu", g_cov="g_cov"),
        ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_particles_along_backward_cavities": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles_along_backward_cavities(ctx, lat, N, a["e_in"], a["p_in"], 0, a["records"],
                                                                                        a["g_records"], None, a["g_params"], a["g_e"], a["g_p"]),
        dict(e_in="e_in", p_in="p_in", records="records", g_records="g_records", g_params="g_params", g_e="g_e", g_p="g_p"),
        ["g_params", "g_e", "g_p"],
        dict(g_params=None), "beam trace gradients with cavities: null argument"),
    "lynx_track_particles_along_backward_losses": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles_along_backward_losses(ctx, lat, N, a["e_in"], a["records"], a["g_records"], None, 1,
                                                                                      ints([0]), a["set_records"], a["g_params"], a["g_e"]),
        dict(e_in="e_in", records="records", g_records="g_records", set_records="set_records", g_params="g_params", g_e="g_e"),
        ["g_params", "g_e"],
        dict(g_params=None), "beam trace gradients with losses: null argument"),
    "lynx_track_particles_along_backward_trajectories": (
        lambda lib, ctx, lat, code, a: lib.lynx_track_particles_along_backward_trajectories(ctx, lat, N, a["e_in"], None, None, None, a["g_params"],
                                                                                            a["g_e"], None, None, CHOSEN, a["traj"], a["traj_bar"],
                                                                                            a["g_chosen"]),
        dict(e_in="e_in", g_params="g_params", g_e="g_e", traj="traj", traj_bar="traj_bar", g_chosen="g_chosen"),
        ["g_params", "g_e", "g_chosen"],
        dict(g_chosen=None), "beam trace gradients with trajectories: null argument"),
    "lynx_moments": (
        lambda lib, ctx, lat, code, a: lib.lynx_moments(ctx, code, B, N, a["p_in"], a["out"], 1),
        dict(p_in="p_in", out="copy"), ["copy"],
        dict(out=None), "null argument"),
    "lynx_moments_by_loss": (
        lambda lib, ctx, lat, code, a: lib.lynx_moments_by_loss(ctx, code, B, N, a["p_in"], 0, 1, a["lost_at"], a["out"]),
        dict(p_in="p_in", lost_at="lost_at", out="sets_out"), ["sets_out"],
        dict(out=None), "moments by loss: null argument"),
    "lynx_histogram2d": (
        lambda lib, ctx, lat, code, a: lib.lynx_histogram2d(ctx, code, B, N, a["p_in"], a["xedges"], a["yedges"], NX, NY, a["hist"]),
        dict(p_in="p_in", xedges="xedges", yedges="yedges", hist="hist"), ["hist"],
        dict(hist=None), "bad argument"),
    "lynx_aperture_mask": (
        lambda lib, ctx, lat, code, a: lib.lynx_aperture_mask(ctx, code, B, N, a["p_in"], a["x_max"], a["y_max"], 0, 0, a["mask"], a["counts"],
                                                              a["offsets"], a["totals"]),
        dict(p_in="p_in", x_max="x_max", y_max="y_max", mask="mask", counts="counts", offsets="offsets", totals="totals"),
        ["mask", "counts", "offsets", "totals"],
        dict(mask=None), "bad argument"),
    "lynx_aperture_compact": (  # (the first sample's particles, behind the valid lynx_aperture_mask call of the module's order)
        lambda lib, ctx, lat, code, a: (lib.lynx_aperture_mask(ctx, code, B, N, a["p_in"], a["x_max"], a["y_max"], 0, 0, a["mask"], a["counts"],
                                                               a["offsets"], a["totals"])
                                        or lib.lynx_aperture_compact(ctx, code, N, a["p_in"], a["mask"], a["offsets"], a["kept"], a["lost"])),
        dict(p_in="p_in", x_max="x_max", y_max="y_max", mask="mask", counts="counts", offsets="offsets", totals="totals", kept="kept",
             lost="lost"), ["kept", "lost"],
        dict(kept=None), "bad argument"),
    "lynx_gaussian_image": (
        lambda lib, ctx, lat, code, a: lib.lynx_gaussian_image(ctx, code, B, a["mu_in"], a["cov_in"], a["xs"], a["ys"], NX, NY, a["image"]),
        dict(mu_in="mu_in", cov_in="cov_in", xs="xs", ys="ys", image="image"), ["image"],
        dict(image=None), "bad argument"),
    "lynx_gaussian_images_along": (
        lambda lib, ctx, lat, code, a: lib.lynx_gaussian_images_along(ctx, code, B, P, a["mu_tr"], a["cov_tr"], 1, ints(SCREEN), a["grid"],
                                                                      a["misalignment"], 0, a["images"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", images="images"), ["images"],
        dict(images=None), "bad argument"),
    "lynx_gaussian_images_along_backward": (
        lambda lib, ctx, lat, code, a: lib.lynx_gaussian_images_along_backward(ctx, code, B, P, a["mu_tr"], a["cov_tr"], 1, ints(SCREEN), a["grid"],
                                                                               a["misalignment"], 0, a["images_bar"], a["mu_bar_out"],
                                                                               a["cov_bar_out"], a["g_mis"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", images_bar="images_bar", mu_bar_out="mu_bar_out",
             cov_bar_out="cov_bar_out", g_mis="g_mis"), ["mu_bar_out", "cov_bar_out", "g_mis"],
        dict(mu_bar_out=None), "image gradients along the trace: bad argument"),
    "lynx_fill_gaussian": (
        lambda lib, ctx, lat, code, a: lib.lynx_fill_gaussian(ctx, code, B, N, doubles([0.0] * 6), doubles(SIGMA), 7, a["fill"]),
        dict(fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_fill_gaussian_rows": (
        lambda lib, ctx, lat, code, a: lib.lynx_fill_gaussian_rows(ctx, code, B, N, a["gauss_rows"], 7, a["fill"]),
        dict(gauss_rows="gauss_rows", fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_transform_particles": (
        lambda lib, ctx, lat, code, a: lib.lynx_transform_particles(ctx, code, B, N, a["p_in"], N * 7, a["transform_rows"], a["fill"]),
        dict(p_in="p_in", transform_rows="transform_rows", fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_build_compose": (
        lambda lib, ctx, lat, code, a: lib.lynx_build_compose(ctx, lat, a["e_in"], a["steps"], a["e_out"]),
        dict(e_in="e_in", steps="steps", e_out="e_out"), ["steps", "e_out"],
        dict(steps=None), "null argument"),
}

def run(env, entry, change=None):
    """The entry's call with the valid arguments, `change` applied; its outputs are zeroed first.  Returns (status, bytes)."""
    call, valid, outputs, _, _ = ENTRIES[entry]
    rt = env.rt
    for name in outputs:
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(env.a[name].ptr), 0, env.a[name].nbytes))
    names = {**valid, **(change or {})}
    a = {key: None if name is None else name if not isinstance(name, str) else C.c_void_p(env.a[name].ptr) for key, name in names.items()}
    status = call(rt.lib, rt.ctx, env.lat.handle, env.code, a)
    message = rt.lib.lynx_last_error(rt.ctx).decode()
    return status, message, [env.a[name].numpy().tobytes() for name in outputs]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_refused_call_says_why_and_the_next_valid_call_returns_the_same_bytes(env, entry):
    _, _, _, change, expected = ENTRIES[entry]
    status, message, before = run(env, entry)
    assert status == 0, message
    status, message, _ = run(env, entry, change)
    assert (status, message) == (INVALID, expected)
    status, message, after = run(env, entry)
    assert status == 0, message
    assert after == before
    assert any(any(block) for block in before), "the valid call wrote nothing"
    # ... and nothing the reverse passes read has been written to
    assert {name: env.a[name].numpy().tobytes() for name in env.keep} == env.keep


def test_track_particles_new_refuses_an_empty_beam_and_hands_out_no_block(env):
    from lynx_amd import _ffi
    from lynx_amd.device import DeviceArray

    rt, a = env.rt, env.a
    results = []
    for n in (N, 0, N):
        blocks = (C.c_void_p * 4)()
        status = rt.lib.lynx_track_particles_new(rt.ctx, env.lat.handle, n, C.c_void_p(a["e_in"].ptr), C.c_void_p(a["p_in"].ptr),
                                                 _ffi.TRACK_MOMENTS, 1, blocks)
        message = rt.lib.lynx_last_error(rt.ctx).decode()
        if n == 0:
            assert (status, message) == (INVALID, "n_particles must be > 0") and not any(blocks)
            continue
        assert status == 0 and blocks[0] and blocks[1] and blocks[2] and not blocks[3], message
        held = [DeviceArray.adopt(rt, blocks[0], (B, N, 7), env.dtype), DeviceArray.adopt(rt, blocks[1], (B,), env.dtype),
                DeviceArray.adopt(rt, blocks[2], (B, 36), F64)]
        results.append([block.numpy().tobytes() for block in held])
    assert results[0] == results[1] and any(results[0][0])


@pytest.mark.parametrize("entry", ["lynx_buf_d2d", "lynx_buf_memset"])
def test_a_copy_or_fill_without_a_context_is_refused_and_of_zero_bytes_does_nothing(env, entry):
    rt, src, dst = env.rt, C.c_void_p(env.a["mom"].ptr), C.c_void_p(env.a["copy"].ptr)
    nbytes = env.a["copy"].nbytes
    call = ((lambda ctx, n: rt.lib.lynx_buf_d2d(ctx, dst, src, n)) if entry == "lynx_buf_d2d"
            else (lambda ctx, n: rt.lib.lynx_buf_memset(ctx, dst, 0x3c, n)))
    rt.check(rt.lib.lynx_buf_memset(rt.ctx, dst, 0, nbytes))
    rt.check(call(rt.ctx, nbytes))
    before = env.a["copy"].numpy().tobytes()
    assert before == (env.keep["mom"] if entry == "lynx_buf_d2d" else b"\x3c" * nbytes)
    assert call(None, nbytes) == INVALID and rt.lib.lynx_last_error(None).decode() == "null ctx"
    rt.check(rt.lib.lynx_buf_memset(rt.ctx, dst, 0, nbytes))
    assert call(rt.ctx, 0) == 0 and not any(env.a["copy"].numpy().tobytes())
    rt.check(call(rt.ctx, nbytes))
    assert env.a["copy"].numpy().tobytes() == before


def test_track_moments_refuses_a_batch_above_int32_before_it_touches_a_result(env):
    """A lattice handle of batch 2^31: one drift whose parameter is shared by the batch (batch stride 0) -- its pool is one
    scalar, and lynx_lattice_create allocates nothing per sample.  Nothing is ever launched on it."""
    from lynx_amd import _ffi

    rt, a = env.rt, env.a
    elems = (_ffi.Elem * 1)(_ffi.Elem(_ffi.KIND_DRIFT, 0, 0, 0))
    steps = (_ffi.Step * 1)(_ffi.Step(_ffi.STEP_RUN, 0, 1, 0))
    pool = np.array([0.5], dtype=env.dtype)
    handle = C.c_void_p()
    rt.check(rt.lib.lynx_lattice_create(rt.ctx, env.code, 1 << 31, 1, elems, 1, steps, pool.ctypes.data, 1, C.byref(handle)))
    try:
        p = lambda name: C.c_void_p(a[name].ptr)  # noqa: E731
        status = rt.lib.lynx_track_moments(rt.ctx, handle, p("e_in"), p("mu_in"), p("cov_in"), p("mu_out"), p("cov_out"), None)
        assert (status, rt.lib.lynx_last_error(rt.ctx).decode()) == (INVALID, "batch too large")
    finally:
        rt.lib.lynx_lattice_destroy(handle)
    status, message, _ = run(env, "lynx_track_moments")
    assert status == 0, message
