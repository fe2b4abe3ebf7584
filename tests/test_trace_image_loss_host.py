"""
`track_along_vjp(..., image_targets=)` without a GPU: the numpy restatement of the image loss and its adjoint
(tests/image_loss_reference.py) against central differences of the oracle's image loss in float64, what the forward kernel's
float32 operations cost it (the base of the GPU tests' float32 tolerance), every refusal by exception type and by the name in
its message, the calls the constructor and a reverse call make, and the two new C entry points being declared.
"""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import image_loss_reference as il
from . import screen_grad_reference as ref
from .reverse_host_fakes import no_gpu, recorded  # noqa: F401 (fixtures)
from .test_gpu_trace_screens import SCREEN_A, SCREEN_B
from .test_trace_screens_grad_host import _lattice, _parameters

ROOT = Path(__file__).resolve().parent.parent
FORWARD, BACKWARD, SWEEP = "lynx_gaussian_images_along_mse", "lynx_gaussian_images_along_mse_backward", "lynx_track_moments_along_backward"


# ---------------------------------------------------------------------------------------------
# 1. the float64 restatement against the oracle
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("geometry", [SCREEN_A, SCREEN_B], ids=["A", "B"])
def test_the_restatement_is_the_derivative_of_the_oracles_image_loss_fp64(geometry):
    """L = mean (image(mu, cov) - T)^2: d L by mu_x, mu_y, cov_xx, cov_yy and by cov_xy, cov_yx moved together, central
    differences with steps of 1e-9 in mu and 1e-14 in cov (variances are 1e-8), to 1e-6 relative -- the method and the bar of
    test_the_restatement_is_the_derivative_of_the_oracles_image_fp64."""
    beam, xs, ys, target = il.mismatch_target(geometry, np.float64)
    loss, entries, loss_size, sizes = il.image_loss(*beam, xs, ys, target)
    mu, cov = np.zeros((1, 7)), np.zeros((1, 7, 7))
    mu[0, 0], mu[0, 2], mu[0, 6] = beam[0], beam[1], 1.0
    cov[0, 0, 0], cov[0, 0, 2], cov[0, 2, 0], cov[0, 2, 2] = beam[2], beam[3], beam[3], beam[4]
    cov[0, 1, 1] = cov[0, 3, 3] = 1e-10
    of_oracle = lambda: float(np.mean(np.square(o.screen_reading_parameters(mu, cov, **geometry, dtype=np.float64)[0] - target)))  # noqa: E731
    assert target.shape == (len(xs), len(ys))
    assert abs(loss - of_oracle()) <= 1e-12 * loss and 0 < loss <= loss_size  # (the restatement's loss is the oracle's)
    where = {"mu_x": [(mu, (0, 0))], "mu_y": [(mu, (0, 2))], "cov_xx": [(cov, (0, 0, 0))], "cov_yy": [(cov, (0, 2, 2))],
             "cov_xy": [(cov, (0, 0, 2)), (cov, (0, 2, 0))]}
    for name in ref.ENTRIES:
        h = 1e-9 if name.startswith("mu") else 1e-14
        values = []
        for sign in (+1, -1):
            for array, index in where[name]:
                array[index] += sign * h
            values.append(of_oracle())
            for array, index in where[name]:
                array[index] -= sign * h
        central = (values[0] - values[1]) / (2 * h)
        got = entries[name] * (2 if name == "cov_xy" else 1)  # (both symmetric entries moved: the sum of the two halves)
        print(f"{name}: restatement {got:.12e}, central difference {central:.12e}, relative {abs(got - central) / abs(central):.2e}")
        assert abs(got - central) <= 1e-6 * abs(central), (name, got, central)
        assert 0 < abs(entries[name]) <= sizes[name]


def test_the_loss_of_a_match_is_zero_and_its_sizes_are_not():
    beam, xs, ys, _ = il.mismatch_target(SCREEN_B, np.float64)
    target = ref.density(*beam, xs, ys)[0]
    loss, entries, loss_size, sizes = il.image_loss(*beam, xs, ys, target)
    assert loss == 0 and all(entries[name] == 0 for name in ref.ENTRIES)
    assert loss_size == float(np.mean(np.square(2 * target))) and all(sizes[name] > 0 for name in ref.ENTRIES)


# ---------------------------------------------------------------------------------------------
# 2. the float32 restatement
# ---------------------------------------------------------------------------------------------


def float32_deviation(geometry, sample):
    """|float32 restatement - float64 restatement| on the float32 inputs, relative to the uncancelled size for this loss:
    (the worst entry, the loss)."""
    beam, xs, ys, target = il.mismatch_target(geometry, np.float32, "float32", sample)
    beam = tuple(np.float32(v) for v in beam)
    loss, exact, loss_size, sizes = il.image_loss(*beam, xs, ys, target)
    loss32, single, _, _ = il.image_loss(*beam, xs, ys, target, "float32")
    return max(abs(single[name] - exact[name]) / sizes[name] for name in ref.ENTRIES), abs(loss32 - loss) / loss_size


def test_what_the_float32_operations_cost_the_restatement():
    """Measured, printed and asserted with a small margin: `FLOAT32_ENTRY_DEVIATION` and `FLOAT32_LOSS_DEVIATION` are the base
    of the GPU tests' float32 tolerance."""
    worst_entry, worst_loss = {}, {}
    for label, geometry in il.LOSS_SCREENS.items():
        measured = [float32_deviation(geometry, sample) for sample in range(4)]
        worst_entry[label], worst_loss[label] = max(m[0] for m in measured), max(m[1] for m in measured)
        print(f"{label}: entries {worst_entry[label]:.3e} (asserted: {il.FLOAT32_ENTRY_DEVIATION[label]:.3e}), "
              f"loss {worst_loss[label]:.3e} (asserted: {il.FLOAT32_LOSS_DEVIATION[label]:.3e})")
    for worst, constants in ((worst_entry, il.FLOAT32_ENTRY_DEVIATION), (worst_loss, il.FLOAT32_LOSS_DEVIATION)):
        assert set(worst) == set(constants)
        for label, value in worst.items():
            assert constants[label] / 2 <= value <= constants[label], (label, value, constants[label])  # (the margin is small)


def test_the_float32_restatement_on_the_screen_of_65_chunks_stays_inside_the_gpu_tests_bounds():
    """The GPU test of `ref.SCREEN_OF_65_CHUNKS` (a batch of 2: samples 0 and 1) asserts 8 x the deviations of 612 x 511; the
    float32 restatement itself is inside them on these inputs.  Measured: entries 1.09e-7 and 1.06e-7 of 6.76e-7, loss
    9.07e-8 and 5.73e-8 of 3.56e-7."""
    from .test_gpu_trace_screens_grad import FLOAT32_FACTOR, LARGEST

    bounds = FLOAT32_FACTOR * il.FLOAT32_ENTRY_DEVIATION[LARGEST], FLOAT32_FACTOR * il.FLOAT32_LOSS_DEVIATION[LARGEST]
    for sample in range(2):
        measured = float32_deviation(ref.SCREEN_OF_65_CHUNKS, sample)
        print(f"65 chunks, sample {sample}: entries {measured[0]:.3e} (bound {bounds[0]:.3e}), loss {measured[1]:.3e} (bound {bounds[1]:.3e})")
        assert measured[0] <= bounds[0] / 2 and measured[1] <= bounds[1] / 2, (sample, measured, bounds)


# ---------------------------------------------------------------------------------------------
# 3. refusals by value
# ---------------------------------------------------------------------------------------------


def test_a_particle_beam_is_the_type_error_of_screens(no_gpu):
    import lynx_amd as lx

    segment = _lattice(lx)[0]
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1, dtype=np.float64), np.full((1,), 1e8), dtype=np.float64)
    with pytest.raises(TypeError, match="ParameterBeam") as info:
        lx.grad.track_along_vjp(segment, particles, image_targets={"SCR_FIRST": np.zeros((20, 12))})
    with pytest.raises(TypeError) as screens:
        lx.grad.track_along_vjp(segment, particles, screens=True)
    assert str(info.value) == str(screens.value) and "histogram" in str(info.value)
    with pytest.raises(TypeError, match="image_targets"):
        lx.grad.track_along_vjp(segment, _parameters(lx), image_targets=np.zeros((20, 12)))


def test_an_unknown_key_is_the_key_error_of_image_at(recorded):
    lx, calls, _ = recorded
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    plain = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    del calls[:]
    stranger = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), is_active=True, name="SCR_ELSEWHERE", dtype=np.float64)
    for key, named in (("SCR_IDLE", "SCR_IDLE"), ("Q", "Q"), ("NOBODY", "NOBODY"), (1, "1"), (idle, "SCR_IDLE"), (stranger, "SCR_ELSEWHERE")):
        with pytest.raises(KeyError, match=named) as info:
            lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={key: np.zeros((20, 12))})
        if not hasattr(key, "name"):  # ... as `image_at` raises it
            with pytest.raises(KeyError) as own:
                plain.trace.image_at(key)
            assert str(info.value) == str(own.value)
    with pytest.raises(ValueError, match="SCR_FIRST"):  # one screen, two targets
        lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={"SCR_FIRST": np.zeros((20, 12)), 0: np.zeros((20, 12))})
    assert calls == []


def test_a_target_that_does_not_fit_names_the_screen_and_both_shapes(no_gpu):
    import lynx_amd as lx

    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    for shape in [(2, 12, 20), (3, 20, 12), (20,), (), (12, 20), (2, 20, 13), (2, 2, 20, 12)]:
        with pytest.raises(ValueError, match="SCR_FIRST") as info:
            lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={"SCR_FIRST": np.ones(shape), last: np.ones((33, 17))})
        assert str(shape) in str(info.value) and "(20, 12)" in str(info.value) and "(2, 20, 12)" in str(info.value)
    with pytest.raises(ValueError, match="SCR_LAST"):  # (through an ImageTargets as well)
        lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets=lx.grad.ImageTargets({last: np.ones((17, 33))}))


def test_image_loss_bar_without_targets_is_a_value_error(recorded, no_gpu):
    lx, calls, _ = recorded
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    with_images = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True)
    first.is_active = last.is_active = False
    plain = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)))
    for vjp in (with_images, plain):
        for bar in (1.0, {"SCR_FIRST": 1.0}, {}):
            with pytest.raises(ValueError, match="image_targets") as info:
                vjp(image_loss_bar=bar)
            assert "image_loss_bar" in str(info.value)
        with pytest.raises(ValueError, match="image_targets"):
            vjp.image_loss
    assert calls == []


def test_a_batch_of_65536_is_the_lynx_error_of_screens(no_gpu):
    import lynx_amd as lx
    from lynx_amd import _ffi

    batch = (_ffi.MAX_IMAGE_BATCH + 1,)
    segment = _lattice(lx, batch=batch)[0]
    with pytest.raises(_ffi.LynxError, match="65536") as info:
        lx.grad.track_along_vjp(segment, _parameters(lx, batch), image_targets={"SCR_FIRST": np.zeros((20, 12))})
    with pytest.raises(_ffi.LynxError) as screens:
        lx.grad.track_along_vjp(segment, _parameters(lx, batch), screens=True)
    assert str(info.value) == str(screens.value)


# ---------------------------------------------------------------------------------------------
# 4. the calls
# ---------------------------------------------------------------------------------------------


def arguments(rt_records, entry):
    found = [args for name, args in rt_records if name == entry]
    assert len(found) == 1, (entry, len(found))
    return found[0]


@pytest.fixture
def recorded_in_full(monkeypatch):
    """`recorded` with the fake library's full records: (lynx_amd, the runtime, the keyword arguments of every forward pass)."""
    import lynx_amd as lx

    from .reverse_host_fakes import fake_gpu

    from lynx_amd import engine

    rt, forward = fake_gpu(monkeypatch)
    fabricated = engine.track_along

    def track_along(owner, leaves, incoming, **kwargs):
        """The fabricated forward pass; asked for the screens as points alone, it hands out no images, as the real one."""
        trace = fabricated(owner, leaves, incoming, **kwargs)
        if kwargs.get("screens") == "points":
            trace._set_screens(trace.screens, None)
        return trace

    monkeypatch.setattr(engine, "track_along", track_along)
    return lx, rt, forward


def test_the_forward_pass_makes_no_image_and_the_loss_is_evaluated_right_behind_it(recorded_in_full):
    lx, rt, forward = recorded_in_full
    calls = rt.lib.calls
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    target = np.arange(33 * 17, dtype=np.float64).reshape(33, 17)
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={last: target})
    assert forward == [dict(keep_outgoing=True, keep_device=True, screens="points")]
    assert calls == [FORWARD] and "lynx_gaussian_images_along" not in calls
    args = arguments(rt.lib.records, FORWARD)
    # ctx, dtype, batch, n_points, mu, cov, n_screens, rows, grid, misalignment, stride, offsets, targets, target stride, loss, sums
    assert len(args) == 16 and args[2:4] == [2, 7] and args[6] == 2 and args[7] == {"ctypes": [0, 20, 12, 5, 33, 17]}
    assert args[4]["how"] == "forward:mu" and args[5]["how"] == "forward:cov"
    assert args[11] == {"ctypes": [-1, 0]}  # SCR_FIRST is not named; SCR_LAST's target starts the row
    assert args[12]["how"] == "to_device" and args[12]["shape"] == [1, 33 * 17] and args[13] == 0  # one row, shared: stride 0
    assert np.array_equal(args[12]["host"], target.reshape(1, -1)) and args[12]["dtype"] == np.dtype(np.float64).str
    assert (args[14]["shape"], args[14]["dtype"]) == ([2, 2], "<f8") and (args[15]["shape"], args[15]["dtype"]) == ([2, 2, 6], "<f8")
    assert set(vjp.image_loss) == {"SCR_LAST"} and vjp.image_loss["SCR_LAST"].shape == (2,) and vjp.image_loss["SCR_LAST"].dtype == np.float64
    assert np.array_equal(vjp.image_loss_of(5), vjp.image_loss["SCR_LAST"]) and np.array_equal(vjp.image_loss_of(last), vjp.image_loss_of("SCR_LAST"))
    with pytest.raises(KeyError, match="SCR_FIRST"):
        vjp.image_loss_of("SCR_FIRST")
    # the trace knows its screens and has no images
    assert vjp.trace.screens == [0, 5] and list(vjp.trace.screen_images) == []
    with pytest.raises(KeyError, match="screens=True") as info:
        vjp.trace.image_at("SCR_LAST")
    assert "not made" in str(info.value)
    with pytest.raises(KeyError, match="SCR_IDLE"):
        vjp.trace.image_at("SCR_IDLE")


def test_per_sample_targets_are_one_row_per_sample_screen_after_screen(recorded_in_full):
    lx, rt, forward = recorded_in_full
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    t_first = np.arange(2 * 20 * 12, dtype=np.float64).reshape(2, 20, 12)
    t_last = np.full((33, 17), 0.25)
    lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={"SCR_LAST": t_last, 0: t_first})
    args = arguments(rt.lib.records, FORWARD)
    assert args[11] == {"ctypes": [0, 240]} and args[13] == 240 + 561 and args[12]["shape"] == [2, 801]
    assert np.array_equal(args[12]["host"][:, :240], t_first.reshape(2, 240)) and np.all(args[12]["host"][:, 240:] == 0.25)


def test_a_call_with_image_loss_bar_is_one_launch_in_front_of_the_sweep(recorded_in_full):
    lx, rt, forward = recorded_in_full
    calls = rt.lib.calls
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={last: np.ones((33, 17))})
    del calls[:], rt.lib.records[:]
    g = vjp(mu_bar=np.ones((2, 7, 6)), sigma_x=1.0)  # no image_loss_bar: nothing new is launched
    assert calls == [SWEEP]
    assert first in g and last in g and np.array_equal(g[first]["misalignment"], np.zeros(2))
    del calls[:], rt.lib.records[:]
    g = vjp(image_loss_bar=np.array([0.5, 0.0]), beta_x=1.0)
    assert calls == [BACKWARD, SWEEP]
    args = arguments(rt.lib.records, BACKWARD)
    # ctx, dtype, batch, n_points, cov, n_screens, rows, sums, loss_bar, mu_bar, cov_bar, grad_misalignment
    assert len(args) == 12 and args[2:4] == [2, 7] and args[4]["how"] == "forward:cov" and args[5] == 2
    assert args[6] == {"ctypes": [0, 20, 12, 5, 33, 17]} and args[7]["shape"] == [2, 2, 6] and args[7]["how"] == "empty"
    assert np.array_equal(args[8]["host"], [[0.0, 0.5], [0.0, 0.0]])  # (zero for the screen without a target)
    assert args[9]["shape"] == [2, 7, 7] and args[10]["shape"] == [2, 7, 7, 7] and args[11]["shape"] == [2, 2, 2]
    sweep = arguments(rt.lib.records, SWEEP)
    assert sweep[5] == args[9] and sweep[6] == args[10]  # the sweep takes the arrays the loss's cotangents went into
    assert g[first]["misalignment"].shape == (2,) and g[last]["misalignment"].shape == (2, 2) and g.mu.shape == (2, 7)
    del calls[:]
    vjp(image_loss_bar={"SCR_LAST": 2.0})
    assert calls == [BACKWARD, SWEEP]
    with pytest.raises(KeyError, match="SCR_FIRST"):  # a screen without a target has no loss to take a cotangent of
        vjp(image_loss_bar={first: 1.0})
    with pytest.raises(ValueError, match="SCR_LAST"):
        vjp(image_loss_bar=np.ones(3))


def test_with_screens_as_well_the_images_are_made_and_both_cotangents_go_in_one_call(recorded_in_full):
    lx, rt, forward = recorded_in_full
    calls = rt.lib.calls
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    vjp = lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), screens=True, image_targets={last: np.ones((33, 17))})
    assert forward == [dict(keep_outgoing=True, keep_device=True, screens=True)] and calls == [FORWARD]
    assert vjp.trace.image_at("SCR_LAST").shape == (2, 33, 17)
    del calls[:]
    g = vjp(screen_images_bar={first: 1.0}, image_loss_bar=1.0)
    assert calls == ["lynx_gaussian_images_along_backward", BACKWARD, SWEEP]
    assert g[last]["misalignment"].shape == (2, 2)
    aperture.is_active = True  # `losses=True` may be combined
    lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), losses=True, image_targets={last: np.ones((33, 17))})
    assert forward[-1] == dict(keep_outgoing=True, keep_device=True, losses=True, screens="points")


def test_a_dict_is_uploaded_per_pass_and_image_targets_once(recorded_in_full):
    lx, rt, forward = recorded_in_full
    segment, first, idle, last, quad, aperture = _lattice(lx, batch=(2,))
    target = np.ones((33, 17))
    uploads = lambda: [a for a in rt.allocations if a.how == "to_device" and a.shape == (1, 561)]  # noqa: E731
    for _ in range(2):
        lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets={last: target})
    assert len(uploads()) == 2
    targets = lx.grad.ImageTargets({last: target})
    passes = [lx.grad.track_along_vjp(segment, _parameters(lx, (2,)), image_targets=targets) for _ in range(2)]
    assert len(uploads()) == 3
    sent = [args[12] for name, args in rt.lib.records if name == FORWARD]
    assert len(sent) == 4 and sent[2] == sent[3] and passes[0].image_loss.keys() == passes[1].image_loss.keys()


# ---------------------------------------------------------------------------------------------
# 5. the entries are declared
# ---------------------------------------------------------------------------------------------


def test_the_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for entry in (FORWARD, BACKWARD):
        assert entry in _ffi.SIGNATURES and f"int {entry}(" in header
    forward = _ffi.SIGNATURES["lynx_gaussian_images_along"][1]
    args = _ffi.SIGNATURES[FORWARD][1]
    assert args[:11] == forward[:11] and len(forward) == 12 and len(args) == 16  # (up to misalignment_stride as the forward call)
    assert len(_ffi.SIGNATURES[BACKWARD][1]) == 12
    names = lambda entry: [part.split()[-1].lstrip("*") for part in re.search(rf"int {entry}\((.*?)\);", header, re.S).group(1).split(",")]  # noqa: E731
    assert names(FORWARD)[:11] == names("lynx_gaussian_images_along")[:11]
    assert names(FORWARD)[11:] == ["target_offsets", "d_targets", "target_stride", "d_loss", "d_sums"]
    assert names(BACKWARD) == ["ctx", "dtype", "batch", "n_points", "d_cov_trace", "n_screens", "screens", "d_sums", "d_loss_bar", "d_mu_bar",
                               "d_cov_bar", "d_grad_misalignment"]
    flat = re.sub(r"\s+\*?\s*", " ", header)
    assert 'starts with "image loss along the trace: "' in flat and "the same call returns the same bits" in flat
