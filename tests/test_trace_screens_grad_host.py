"""
`track_along_vjp(..., screens=True)` without a GPU: the numpy restatement of the image's adjoint
(tests/screen_grad_reference.py) against central differences of the oracle's image in float64, what the forward kernel's
float32 operations cost it (the base of the GPU tests' float32 tolerance), every refusal by exception type and by the name in
its message, the calls a reverse call makes, and the new C entry point being declared.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import screen_grad_reference as ref
from .test_gpu_trace_screens import SCREEN_A, SCREEN_B
from .reverse_host_fakes import no_gpu, recorded  # noqa: F401 (fixtures)

ROOT = Path(__file__).resolve().parent.parent
ENTRY = "lynx_gaussian_images_along_backward"


# ---------------------------------------------------------------------------------------------
# 1. the float64 restatement against the oracle
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("geometry", [SCREEN_A, SCREEN_B], ids=["A", "B"])
def test_the_restatement_is_the_derivative_of_the_oracles_image_fp64(geometry):
    """L = sum W image(mu, cov), W held fixed: d L by mu_x, mu_y, cov_xx, cov_yy and by cov_xy, cov_yx moved together,
    central differences with steps of 1e-9 in mu and 1e-14 in cov (variances are 1e-8), to 1e-6 relative."""
    beam, xs, ys, W = ref.mismatch_cotangent(geometry, np.float64)
    entries, sizes = ref.image_cotangents(*beam, xs, ys, W)
    mu, cov = np.zeros((1, 7)), np.zeros((1, 7, 7))
    mu[0, 0], mu[0, 2], mu[0, 6] = beam[0], beam[1], 1.0
    cov[0, 0, 0], cov[0, 0, 2], cov[0, 2, 0], cov[0, 2, 2] = beam[2], beam[3], beam[3], beam[4]
    cov[0, 1, 1] = cov[0, 3, 3] = 1e-10
    image = o.screen_reading_parameters(mu, cov, **geometry, dtype=np.float64)[0]
    assert image.shape == W.shape == (len(xs), len(ys))
    assert np.max(np.abs(image - ref.density(*beam, xs, ys)[0])) <= 1e-12 * image.max()  # (the restatement's image is the oracle's)
    where = {"mu_x": [(mu, (0, 0))], "mu_y": [(mu, (0, 2))], "cov_xx": [(cov, (0, 0, 0))], "cov_yy": [(cov, (0, 2, 2))],
             "cov_xy": [(cov, (0, 0, 2)), (cov, (0, 2, 0))]}
    for name in ref.ENTRIES:
        h = 1e-9 if name.startswith("mu") else 1e-14
        values = []
        for sign in (+1, -1):
            for array, index in where[name]:
                array[index] += sign * h
            values.append(float(np.sum(W * o.screen_reading_parameters(mu, cov, **geometry, dtype=np.float64)[0])))
            for array, index in where[name]:
                array[index] -= sign * h
        central = (values[0] - values[1]) / (2 * h)
        got = entries[name] * (2 if name == "cov_xy" else 1)  # (both symmetric entries moved: the sum of the two halves)
        print(f"{name}: restatement {got:.12e}, central difference {central:.12e}, relative {abs(got - central) / abs(central):.2e}")
        assert abs(got - central) <= 1e-6 * abs(central), (name, got, central)
        assert 0 < abs(entries[name]) <= sizes[name]
    mu_bar, cov_bar = ref.moment_cotangents(entries)
    assert cov_bar[0, 2] == cov_bar[2, 0] and np.count_nonzero(mu_bar) == 2 and np.count_nonzero(cov_bar) == 4


# ---------------------------------------------------------------------------------------------
# 2. the float32 restatement
# ---------------------------------------------------------------------------------------------


def float32_deviation(geometry, sample):
    """Per entry: |float32 restatement - float64 restatement| on the float32 inputs, relative to the uncancelled size."""
    beam, xs, ys, W = ref.mismatch_cotangent(geometry, np.float32, "float32", sample)
    beam = tuple(np.float32(v) for v in beam)
    exact, sizes = ref.image_cotangents(*beam, xs, ys, W)
    single, _ = ref.image_cotangents(*beam, xs, ys, W, "float32")
    return {name: abs(single[name] - exact[name]) / sizes[name] for name in ref.ENTRIES}


def test_what_the_float32_operations_cost_the_restatement():
    """Measured, printed and asserted with a small margin: `FLOAT32_RESTATEMENT_DEVIATION` is the base of the GPU tests'
    float32 tolerance."""
    screens = dict(ref.KERNEL_SCREENS, A=SCREEN_A, B=SCREEN_B)
    worst = {}
    for label, geometry in screens.items():
        worst[label] = max(max(float32_deviation(geometry, sample).values()) for sample in range(4))
        print(f"{label}: {worst[label]:.3e} (asserted: {ref.FLOAT32_RESTATEMENT_DEVIATION[label]:.3e})")
    assert set(worst) == set(ref.FLOAT32_RESTATEMENT_DEVIATION)
    for label, value in worst.items():
        asserted = ref.FLOAT32_RESTATEMENT_DEVIATION[label]
        assert asserted / 2 <= value <= asserted, (label, value, asserted)  # (the margin is small)


def test_the_float32_restatement_on_the_screen_of_65_chunks_stays_inside_the_gpu_tests_bound():
    """The GPU test of `SCREEN_OF_65_CHUNKS` (a batch of 2: samples 0 and 1) asserts 8 x the deviation of 612 x 511; the
    float32 restatement itself is well inside that on these inputs.  Measured: 2.17e-7 and 2.67e-7 of 2.24e-6."""
    from .test_gpu_trace_screens_grad import FLOAT32_FACTOR, LARGEST

    bound = FLOAT32_FACTOR * ref.FLOAT32_RESTATEMENT_DEVIATION[LARGEST]
    for sample in range(2):
        worst = max(float32_deviation(ref.SCREEN_OF_65_CHUNKS, sample).values())
        print(f"65 chunks, sample {sample}: {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound / 2, (sample, worst, bound)


# ---------------------------------------------------------------------------------------------
# 3. refusals, and the calls
# ---------------------------------------------------------------------------------------------

f = lambda v: np.array([v], dtype=np.float64)  # noqa: E731


def _lattice(lx, shared=True, batch=(1,)):
    mis = np.array([1e-5, -2e-5]) if shared else np.zeros((*batch, 2))
    first = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), misalignment=mis, is_active=True, name="SCR_FIRST", dtype=np.float64)
    idle = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), is_active=False, name="SCR_IDLE", dtype=np.float64)
    last = lx.Screen(resolution=(33, 17), pixel_size=(1e-4, 1e-4), misalignment=np.zeros((*batch, 2)), is_active=True, name="SCR_LAST",
                     dtype=np.float64)
    quad = lx.Quadrupole(f(0.2), k1=f(2.0), dtype=np.float64, name="Q")
    aperture = lx.Aperture(x_max=f(1e-3), y_max=f(2e-3), is_active=False, name="AP", dtype=np.float64)
    return lx.Segment([first, lx.Drift(f(1.0), dtype=np.float64), idle, quad, aperture, last]), first, idle, last, quad, aperture


def _parameters(lx, batch=(1,)):
    full = lambda v: np.full(batch, v)  # noqa: E731
    return lx.ParameterBeam.from_parameters(sigma_x=full(1e-4), sigma_y=full(1e-4), energy=full(1e8), dtype=np.float64)


def test_a_particle_beam_is_a_type_error_that_points_to_a_parameter_beam(no_gpu):
    import lynx_amd as lx

    segment = _lattice(lx)[0]
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1, dtype=np.float64), np.full((1,), 1e8), dtype=np.float64)
    with pytest.raises(TypeError, match="ParameterBeam") as info:
        lx.grad.track_along_vjp(segment, particles, screens=True)
    assert "ParticleBeam" in str(info.value) and "histogram" in str(info.value)
    with pytest.raises(TypeError):  # (with trajectories as well: no differentiable image of particles)
        lx.grad.track_along_vjp(segment, particles, screens=True, trajectories=3)
    with pytest.raises(ValueError, match="screens"):
        lx.grad.track_along_vjp(segment, _parameters(lx), screens="yes")


def test_trajectories_of_a_parameter_beam_stay_the_type_error_of_track_along(no_gpu):
    import lynx_amd as lx

    segment = _lattice(lx)[0]
    with pytest.raises(TypeError, match="ParameterBeam") as info:
        lx.grad.track_along_vjp(segment, _parameters(lx), screens=True, trajectories=3)
    with pytest.raises(TypeError) as forward:
        segment.track_along(_parameters(lx), screens=True, trajectories=3)
    assert str(info.value) == str(forward.value) and "trajectories" in str(info.value)


def test_without_screens_an_active_screen_is_refused_as_before(no_gpu):
    import lynx_amd as lx
    from lynx_amd import engine

    segment = _lattice(lx)[0]
    with pytest.raises(NotImplementedError) as plan:
        engine.trace_program(list(segment._leaves()))
    for kwargs in ({}, {"screens": False}, {"losses": True}):
        with pytest.raises(NotImplementedError, match="SCR_FIRST") as info:
            lx.grad.track_along_vjp(segment, _parameters(lx), **kwargs)
        assert str(info.value) == str(plan.value)


def test_a_batch_beyond_65535_is_refused_as_the_forward_entry_point_refuses_it(no_gpu):
    import lynx_amd as lx
    from lynx_amd import _ffi

    batch = (_ffi.MAX_IMAGE_BATCH + 1,)
    segment = _lattice(lx, batch=batch)[0]
    with pytest.raises(_ffi.LynxError, match="65536") as info:
        lx.grad.track_along_vjp(segment, _parameters(lx, batch), screens=True)
    assert "lynx_gaussian_images_along" in str(info.value) and "bad argument" in str(info.value)


def test_the_forward_pass_is_track_along_with_screens_and_one_reverse_call_takes_every_cotangent(recorded):
    lx, calls, forward = recorded
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    assert forward == [dict(keep_outgoing=True, keep_device=True, screens=True)]
    assert vjp.trace.screens == [0, 5] and vjp.trace.image_at("SCR_FIRST").shape == (2, 20, 12) and vjp.trace.image_at(5).shape == (2, 33, 17)
    g = vjp(mu_bar=np.ones((2, 7, 6)), sigma_x=1.0)  # no image cotangent: nothing new is launched
    assert calls == ["lynx_track_moments_along_backward"]
    assert first in g and last in g and idle not in g and quad in g
    assert np.array_equal(g[first]["misalignment"], np.zeros(2)) and np.array_equal(g[last]["misalignment"], np.zeros((2, 2)))
    del calls[:]
    assert vjp(screen_images_bar={}).mu.shape == (2, 7) and calls == ["lynx_track_moments_along_backward"]
    del calls[:]
    # a name, a point, the element; a scalar, an image of one sample, a whole cotangent; the same screen twice
    g = vjp(screen_images_bar={"SCR_FIRST": 1.0, 5: np.ones((33, 17)), first: np.ones((2, 20, 12)), -2: 2.0}, cov_bar=np.ones((2, 7, 6, 6)),
            energy_bar=np.ones((2, 7)))
    assert calls == [ENTRY, "lynx_track_moments_along_backward"]
    assert g[first]["misalignment"].shape == (2,) and g[last]["misalignment"].shape == (2, 2) and g.mu.shape == (2, 7)
    # with losses: the ParameterBeam's plain problem, apertures identity steps
    aperture.is_active = True
    with pytest.raises(NotImplementedError, match="AP"):
        lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    del calls[:]
    both = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), losses=True, screens=True)
    assert forward[-1] == dict(keep_outgoing=True, keep_device=True, losses=True, screens=True)
    both(screen_images_bar={last: 1.0})
    assert calls == [ENTRY, "lynx_track_moments_along_backward"]


def test_the_image_cotangents_are_laid_out_as_the_forward_entry_point_lays_out_the_images(recorded):
    lx, calls, _ = recorded
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    w_first = np.arange(2 * 20 * 12, dtype=np.float64).reshape(2, 20, 12)
    flat = vjp._image_cotangents({"SCR_FIRST": w_first, last: 0.5, 5: np.full((33, 17), 0.25)})
    assert flat.shape == (2, 20 * 12 + 33 * 17)
    assert np.array_equal(flat[:, :240], w_first.reshape(2, 240)) and np.all(flat[:, 240:] == 0.75)
    only = vjp._image_cotangents({last: 1.0})  # a screen that is not named gets no cotangent
    assert np.all(only[:, :240] == 0) and np.all(only[:, 240:] == 1) and vjp._image_cotangents({}) is None
    assert calls == []


def test_refusals_of_the_call_are_made_by_value_and_name_the_offender(recorded, no_gpu):
    lx, calls, _ = recorded
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    stranger = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), is_active=True, name="SCR_ELSEWHERE", dtype=np.float64)
    for key, named in (("SCR_IDLE", "SCR_IDLE"), ("Q", "Q"), ("NOBODY", "NOBODY"), (1, "1"), (idle, "SCR_IDLE"), (stranger, "SCR_ELSEWHERE")):
        with pytest.raises(KeyError, match=named):
            vjp(screen_images_bar={key: 1.0})
    for key in ("SCR_IDLE", "NOBODY", 1):  # ... as `image_at` raises it
        with pytest.raises(KeyError) as own:
            vjp.trace.image_at(key)
        with pytest.raises(KeyError) as info:
            vjp(screen_images_bar={key: 1.0})
        assert str(info.value) == str(own.value)
    for shape in [(2, 12, 20), (3, 20, 12), (20,), (2, 20, 13), (2, 2, 20, 12)]:
        with pytest.raises(ValueError, match="SCR_FIRST") as info:
            vjp(screen_images_bar={"SCR_FIRST": np.ones(shape), last: 1.0})
        assert str(shape) in str(info.value) and "(2, 20, 12)" in str(info.value)
    with pytest.raises(TypeError, match="dict"):
        vjp(screen_images_bar=np.ones((2, 20, 12)))
    # without screens=True there are no images to take a cotangent of
    first.is_active = last.is_active = False
    plain = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)))
    for bar in ({"SCR_FIRST": 1.0}, {}):
        with pytest.raises(ValueError, match="screens=True") as info:
            plain(screen_images_bar=bar)
        assert "screen_images_bar" in str(info.value)
    assert calls == []


def test_the_entry_point_is_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    assert ENTRY in _ffi.SIGNATURES and f"int {ENTRY}(" in header
    forward = _ffi.SIGNATURES["lynx_gaussian_images_along"][1]
    args = _ffi.SIGNATURES[ENTRY][1]
    assert args[:len(forward) - 1] == forward[:-1] and len(args) == len(forward) + 3  # (up to misalignment_stride as the forward call)
    names = lambda entry: [part.split()[-1].lstrip("*") for part in re.search(rf"int {entry}\((.*?)\);", header, re.S).group(1).split(",")]  # noqa: E731
    assert names(ENTRY)[:-4] == names("lynx_gaussian_images_along")[:-1]
    assert names(ENTRY)[-4:] == ["d_images_bar", "d_mu_bar", "d_cov_bar", "d_grad_misalignment"]
    flat = header.replace("\n * ", " ").replace("  ", " ")
    assert "image gradients along the trace: " in flat and "the same call returns the same bits" in flat
    assert int(re.search(r"#define LYNX_IMAGE_GRAD_CELLS (\d+)", header).group(1)) == _ffi.IMAGE_GRAD_CELLS
