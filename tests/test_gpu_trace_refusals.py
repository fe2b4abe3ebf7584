"""
What the three entry points of the particle trace refuse (`lynx_track_particles_along`, `_along_losses`, `_along_screens`,
called through the C ABI): every bad argument is answered with LYNX_ERR_INVALID and a message that names the entry's mode
before anything is launched, and the context goes on as if nothing had happened.

Lattice: an inactive aperture (step 0), a drift, an inactive screen (step 2) -- the steps a valid call with losses or
with screens may name --, batch 2, 64 particles, float32.
"""

import ctypes as C

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .test_gpu_trace import SIGMA

pytestmark = pytest.mark.gpu

INVALID = -1  # LYNX_ERR_INVALID
MODE = {"plain": "beam trace: ", "losses": "beam trace with losses: ", "screens": "beam trace with screens: "}
B, N, NX, NY = 2, 64, 5, 3


@pytest.fixture(scope="module")
def case(built_library):
    import lynx_amd as lx
    from lynx_amd import engine

    rt = lx.device.get_runtime()  # raises loudly without a GPU
    dtype = np.float32
    one = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Aperture(x_max=one(1e-4), y_max=one(1e-4), is_active=False, name="AP", dtype=dtype),
                          lx.Drift(np.full(B, 0.7, dtype=dtype), dtype=dtype),
                          lx.Screen(resolution=(NX, NY), pixel_size=(1e-4, 1e-4), is_active=False, name="SCR", dtype=dtype)])
    beam = lx.ParticleBeam(o.gaussian_particles((B,), N, seed=5, dtype=dtype, sigma=SIGMA), np.full(B, 1e8, dtype=dtype), dtype=dtype)
    plain = segment.track_along(beam)
    leaves = list(segment._leaves())
    lat = engine._ready(segment.__dict__["_trace_cache"], engine._trace_plan(segment, leaves), beam.batch_shape, dtype, beam._energy._host)
    assert lat.S == 3 and lat.B == B
    held = dict(  # (device arrays, kept alive for the module)
        e_in=beam._energy.broadcast_device(rt, beam.batch_shape), p_in=beam._particles.device(rt), p_out=rt.empty((B, N, 7), dtype),
        e_trace=rt.empty((B, 4), dtype), records=rt.empty((B, 4, 36), np.float64),
        limits=rt.to_device(np.full((2, 2), 1e-4, dtype=dtype)), lost_at=rt.empty((B, N), np.int32),
        edges=rt.to_device(np.concatenate([np.linspace(-2e-4, 2e-4, NX + 1), np.linspace(-2e-4, 2e-4, NY + 1)]).astype(dtype)),
        misalignment=rt.to_device(np.zeros((1, 2), dtype=dtype)), images=rt.empty((B, NX * NY), np.int32))
    return rt, lat, held, plain, segment  # (the segment keeps the lattice it packed)


def arguments(held):
    """Valid arguments of the three entries by name: the plain entry's, then the aperture list, then the screen list."""
    ptr = {name: C.c_void_p(array.ptr) for name, array in held.items()}
    return dict(n=N, e_in=ptr["e_in"], p_in=ptr["p_in"], p_out=ptr["p_out"], e_trace=ptr["e_trace"], records=ptr["records"], flags=0,
                n_apertures=1, apertures=[0, 0], limits=ptr["limits"], limit_stride=0, lost_at=ptr["lost_at"],
                n_screens=1, screens=[2, NX, NY], edges=ptr["edges"], misalignment=ptr["misalignment"], misalignment_stride=0,
                images=ptr["images"])


def call(rt, lat, entry, a):
    ints = lambda values: (C.c_int32 * max(len(values), 1))(*values)  # noqa: E731
    common = (rt.ctx, lat.handle, a["n"], a["e_in"], a["p_in"], a["p_out"], a["e_trace"], a["records"], a["flags"])
    apertures = (a["n_apertures"], ints(a["apertures"]), a["limits"], a["limit_stride"], a["lost_at"])
    screens = (a["n_screens"], ints(a["screens"]), a["edges"], a["misalignment"], a["misalignment_stride"], a["images"])
    if entry == "plain":
        return rt.lib.lynx_track_particles_along(*common)
    if entry == "losses":
        return rt.lib.lynx_track_particles_along_losses(*common, *apertures)
    return rt.lib.lynx_track_particles_along_screens(*common, *apertures, *screens)


EVERY, LISTS, SCREENS = ("plain", "losses", "screens"), ("losses", "screens"), ("screens",)
REFUSALS = {  # what is wrong -> (the entries it applies to, the arguments that say it)
    "a null output": (EVERY, dict(records=None)),
    "no particles": (EVERY, dict(n=0)),
    "a flag other than LYNX_TRACK_SHARED_INPUT": (EVERY, dict(flags=1)),
    "a shared beam in place": (EVERY, dict(flags=4, p_out="p_in")),
    "aperture steps not increasing": (LISTS, dict(n_apertures=2, apertures=[1, 0, 0, 1])),
    "the same aperture step twice": (LISTS, dict(n_apertures=2, apertures=[0, 0, 0, 1])),
    "an aperture step behind the program": (LISTS, dict(apertures=[3, 0])),
    "a limit stride that is neither 0 nor 2 A": (LISTS, dict(limit_stride=1)),
    "a screen on an aperture's step": (SCREENS, dict(screens=[0, NX, NY])),
    "a screen step behind the program": (SCREENS, dict(screens=[3, NX, NY])),
    "a screen with nx = 0": (SCREENS, dict(screens=[2, 0, NY])),
    "no screen": (SCREENS, dict(n_screens=0)),
}


@pytest.mark.parametrize("entry,wrong", [(entry, wrong) for wrong, (entries, _) in REFUSALS.items() for entry in entries])
def test_a_bad_argument_is_refused_by_name_and_the_context_goes_on(case, entry, wrong):
    rt, lat, held, plain, _ = case
    a = arguments(held)
    assert call(rt, lat, entry, a) == 0, rt.lib.lynx_last_error(rt.ctx)  # (the arguments the refusals start from are valid)
    change = dict(REFUSALS[wrong][1])
    if change.get("p_out") == "p_in":
        change["p_out"] = a["p_in"]
    status = call(rt, lat, entry, {**a, **change})
    message = rt.lib.lynx_last_error(rt.ctx).decode()
    assert status == INVALID and message.startswith(MODE[entry]), (status, message)
    # a valid plain call on the same context: the plain result
    rt.check(rt.lib.lynx_buf_memset(rt.ctx, a["records"], 0, held["records"].nbytes))
    assert call(rt, lat, "plain", a) == 0, rt.lib.lynx_last_error(rt.ctx)
    assert np.array_equal(held["records"].numpy(), plain.records.reshape(B, 4, 36))
    assert np.array_equal(held["p_out"].numpy(), np.asarray(plain.outgoing.particles).reshape(B, N, 7))
