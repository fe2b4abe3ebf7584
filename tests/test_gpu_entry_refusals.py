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

from .entry_calls import ENTRIES, REFUSALS_SHAPE, arguments, make_env

pytestmark = pytest.mark.gpu

INVALID = -1  # LYNX_ERR_INVALID
B, N, NX, NY, CHOSEN = REFUSALS_SHAPE[:5]
S, E, P = REFUSALS_SHAPE.S, REFUSALS_SHAPE.E, REFUSALS_SHAPE.P
F64 = np.dtype(np.float64)


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["float32", "float64"])
def env(built_library, request):
    """The runtime, the lattice and every device array the calls name, for one dtype (entry_calls.make_env)."""
    return make_env(REFUSALS_SHAPE, request.param)


def run(env, entry, change=None):
    """The entry's call with the valid arguments, `change` applied; its outputs are zeroed first.  Returns (status, bytes)."""
    call, _, outputs, _, _ = ENTRIES[entry]
    rt = env.rt
    for name in outputs:
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(env.a[name].ptr), 0, env.a[name].nbytes))
    a = arguments(entry, lambda name: C.c_void_p(env.a[name].ptr), env.shape, change)
    status = call(rt.lib, rt.ctx, env.lat.handle, env.code, a, env.shape)
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
