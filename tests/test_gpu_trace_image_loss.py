"""
`lynx_amd.grad.track_along_vjp(..., image_targets=)` on the GPU: the mean squared difference of a ParameterBeam's screen image
to a target image, evaluated on the device (lynx_gaussian_images_along_mse behind the moment trace,
lynx_gaussian_images_along_mse_backward in front of lynx_track_moments_along_backward).

The kernels alone through the public interface (a screen as the first element observes point 0: `g.mu`, `g.cov` are the
kernels' own mu_bar, cov_bar) against the float64 restatement of tests/image_loss_reference.py, the loss and every entry
relative to its UNCANCELLED SIZE FOR THIS LOSS (that file says what it is); against the existing path, `screens=True` with the
cotangent 2 (image - target) / n formed in numpy; the loss of the image itself, which is exactly zero; end to end against central
differences of the oracle's chain and image loss; the position and the neighbours of a screen; the C entries' refusals; the
example.

Tolerances of the kernels alone:
    float64  1e-10 of the uncancelled size (`TOL_IMAGE` of tests/test_gpu_screen.py, the project's float64 image tolerance);
    float32  8 x what the float32 restatement deviates from the float64 one on the same inputs -- the bases are
             `FLOAT32_ENTRY_DEVIATION[screen]` and `FLOAT32_LOSS_DEVIATION[screen]` of tests/image_loss_reference.py, measured
             and asserted by tests/test_trace_image_loss_host.py.  The factor and its reasons are those of `FLOAT32_FACTOR` of
             tests/test_gpu_trace_screens_grad.py: another order of operations, the device's log and division, and the
             kernel's products in float64.

Sizes: a batch of at most 4, and the cell counts at which the kernel changes form -- 1, 63 | 64 | 65 (a wave), 255 | 256 | 257 (a
round of the workgroup's threads), 33 x 17, one row and one column, 89 x 71 (three full workgroups of 2048 cells and a partly
filled fourth), and 612 x 511 once per dtype.
"""

import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import image_loss_reference as il
from . import screen_grad_reference as ref
from .entry_calls import ints
from .helpers import make_lattice
from .test_gpu_entry_refusals import INVALID, NX, NY, B, P, env  # noqa: F401 (`env` is a fixture)
from .test_gpu_screen import TOL_IMAGE
from .test_gpu_trace_grad import _chain
from .test_gpu_trace_screens import MIS_B, SCREEN_A, SCREEN_B, make_screen, mis_a, two_screen_lattice
from .test_gpu_trace_screens_grad import B6, DESC_6, FLOAT32_FACTOR, LARGEST, end_to_end_case, front

pytestmark = pytest.mark.gpu

SMALL = [label for label in il.LOSS_SCREENS if label != LARGEST]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


# ---------------------------------------------------------------------------------------------
# 6. the kernels alone
# ---------------------------------------------------------------------------------------------


def loss_case(lx, label, dtype, shape, shared_misalignment, shared_target):
    """[Screen, Drift], the beams and misalignments of `kernel_case` of tests/test_gpu_trace_screens_grad.py, and as the target
    the image of `mismatch_target`'s other beam -- one for the batch, or per sample a little brighter with every sample.
    Returns (segment, beam, screen, the targets (B, nx, ny) in the dtype, what was given as the target, the misalignment)."""
    geometry = il.LOSS_SCREENS[label]
    B = int(np.prod(shape))
    hx, hy = (geometry["resolution"][k] * geometry["pixel_size"][k] / 2 for k in (0, 1))
    mis = np.array([0.07 * hx, -0.05 * hy]) if shared_misalignment else np.random.default_rng(5).normal(0, 0.05, (*shape, 2)) * [hx, hy]
    mis = np.asarray(mis, dtype=dtype)
    mu, cov = np.zeros((B, 7)), np.zeros((B, 7, 7))
    shifts = np.broadcast_to(mis, (*shape, 2)).reshape(B, 2).astype(np.float64)
    for s in range(B):
        mx, my, a, b, c = ref.beam_on(geometry, rho=0.5 - 0.2 * s, scale=1.0 + 0.1 * s, shift=(0.05 * s, -0.03 * s))
        m = shifts[s]
        mu[s, 0], mu[s, 2], mu[s, 6] = mx + m[0], my + m[1], 1.0
        cov[s, 0, 0], cov[s, 0, 2], cov[s, 2, 0], cov[s, 2, 2] = a, b, b, c
        cov[s, 1, 1] = cov[s, 3, 3] = 1e-10
        cov[s, 0, 1] = cov[s, 1, 0] = 1e-6 * np.sqrt(a)  # (entries the image does not see)
    beam = lx.ParameterBeam(mu.reshape(*shape, 7).astype(dtype), cov.reshape(*shape, 7, 7).astype(dtype), np.full(shape, 1e8, dtype=dtype),
                            dtype=dtype)
    screen = make_screen(lx, geometry, mis, dtype, "SCREEN")
    segment = lx.Segment([screen, lx.Drift(np.full(shape, 0.5, dtype=dtype), dtype=dtype)])
    other = il.mismatch_target(geometry, dtype)[3]
    if shared_target:
        given, targets = other, np.stack([other] * B)
    else:
        targets = np.stack([(other * (1.0 + 0.05 * s)).astype(dtype) for s in range(B)])
        given = targets.reshape(*shape, *other.shape)
    return segment, beam, screen, targets, given, mis


def restated(vjp, geometry, dtype, targets, mis, shape):
    """Per sample the float64 restatement on the trace's own values (mu less the misalignment formed in the dtype)."""
    xs, ys = ref.pixel_grid(**geometry, dtype=dtype)
    B = int(np.prod(shape))
    mu, cov = np.asarray(vjp.trace._mu)[..., 0, :].reshape(B, 7), np.asarray(vjp.trace._cov)[..., 0, :, :].reshape(B, 7, 7)
    assert mu.dtype == np.dtype(dtype)
    shifts = np.broadcast_to(mis, (*shape, 2)).reshape(B, 2)
    return [il.image_loss(mu[s, 0] - shifts[s, 0], mu[s, 2] - shifts[s, 1], cov[s, 0, 0], cov[s, 0, 2], cov[s, 2, 2], xs, ys, targets[s])
            for s in range(B)]


def entries_of(g, B):
    g_mu, g_cov = np.asarray(g.mu).reshape(B, 7), np.asarray(g.cov).reshape(B, 7, 7)
    return g_mu, g_cov, [{"mu_x": g_mu[s, 0], "mu_y": g_mu[s, 2], "cov_xx": g_cov[s, 0, 0], "cov_yy": g_cov[s, 2, 2], "cov_xy": g_cov[s, 0, 2]}
                         for s in range(B)]


KERNEL_CASES = ([(label, (3,), False, False) for label in SMALL] + [(label, (2, 2), True, True) for label in SMALL]
                + [(LARGEST, (3,), False, False)])


@pytest.mark.parametrize("label, shape, shared_misalignment, shared_target", KERNEL_CASES,
                         ids=[f"{c[0]}-{'shared' if c[2] else 'own'}" for c in KERNEL_CASES])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_kernels_alone_against_the_restatement(lx, dtype, label, shape, shared_misalignment, shared_target):
    from lynx_amd import _ffi

    geometry = il.LOSS_SCREENS[label]
    segment, beam, screen, targets, given, mis = loss_case(lx, label, dtype, shape, shared_misalignment, shared_target)
    B = int(np.prod(shape))
    nx, ny = targets.shape[-2:]
    if label == LARGEST:
        assert nx * ny >= 3 * _ffi.IMAGE_GRAD_CELLS and (nx * ny) % _ffi.IMAGE_GRAD_CELLS
    else:
        assert (nx, ny) == tuple(int(n) for n in label.split("x")) if "x" in label else nx * ny == int(label)
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={screen: given})
    assert vjp.trace.screens == [0] and list(vjp.trace.screen_images) == []  # (no image was made)
    loss = vjp.image_loss_of("SCREEN")
    assert loss.shape == shape and loss.dtype == np.float64 and np.array_equal(loss, vjp.image_loss["SCREEN"])
    g = vjp(image_loss_bar=1.0)
    g_mu, g_cov, got = entries_of(g, B)
    assert g_mu.dtype == g_cov.dtype == np.dtype(dtype)
    if dtype == np.float64:
        tol_entry = tol_loss = TOL_IMAGE[np.float64]
    else:
        tol_entry, tol_loss = FLOAT32_FACTOR * il.FLOAT32_ENTRY_DEVIATION[label], FLOAT32_FACTOR * il.FLOAT32_LOSS_DEVIATION[label]
    want = restated(vjp, geometry, dtype, targets, mis, shape)
    worst = {"loss": 0.0, "entries": 0.0}
    for s, (ref_loss, entries, loss_size, sizes) in enumerate(want):
        distance = abs(loss.reshape(B)[s] - ref_loss) / loss_size
        worst["loss"] = max(worst["loss"], distance)
        print(f"{label} {np.dtype(dtype).name} sample {s} loss: {loss.reshape(B)[s]:.9e} ref {ref_loss:.9e} distance {distance:.2e} of the size")
        for name in ref.ENTRIES:
            distance = abs(float(got[s][name]) - entries[name]) / sizes[name]
            worst["entries"] = max(worst["entries"], distance)
            print(f"{label} {np.dtype(dtype).name} sample {s} {name}: {float(got[s][name]):.9e} ref {entries[name]:.9e} distance {distance:.2e} of the size")
    print(f"{label} {np.dtype(dtype).name}: worst loss {worst['loss']:.2e} (tolerance {tol_loss:.2e}), worst entry {worst['entries']:.2e} "
          f"(tolerance {tol_entry:.2e})")
    for s, (ref_loss, entries, loss_size, sizes) in enumerate(want):
        assert abs(loss.reshape(B)[s] - ref_loss) <= tol_loss * loss_size, (s, loss.reshape(B)[s], ref_loss, loss_size)
        for name in ref.ENTRIES:
            assert abs(float(got[s][name]) - entries[name]) <= tol_entry * sizes[name], (s, name, got[s][name], entries[name], sizes[name])
            assert entries[name] != 0
    assert np.array_equal(g_cov[:, 0, 2], g_cov[:, 2, 0])
    seen_mu, seen_cov = np.zeros(7, dtype=bool), np.zeros((7, 7), dtype=bool)
    seen_mu[[0, 2]] = True
    seen_cov[[0, 0, 2, 2], [0, 2, 0, 2]] = True
    assert np.all(g_mu[:, ~seen_mu] == 0) and np.all(g_cov[:, ~seen_cov] == 0)
    # the misalignment: minus the mu cotangent, summed over the batch where it is shared
    assert screen in g
    shift_bar = g[screen]["misalignment"]
    assert shift_bar.shape == np.asarray(screen.misalignment).shape
    per_sample = -g_mu[:, [0, 2]]
    if shared_misalignment:
        total = per_sample.astype(np.float64).sum(axis=0)
        assert np.all(np.abs(shift_bar - total) <= (1e-14 if dtype == np.float64 else 1e-6) * np.abs(per_sample).sum(axis=0))
    else:
        assert np.array_equal(shift_bar.reshape(B, 2), per_sample)
    for el in vjp.leaves[1:]:  # the drift behind the screen: nothing reaches it
        assert np.all(g[el]["length"] == 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_screen_of_65_chunks_against_the_restatement(lx, monkeypatch, dtype):
    """`ref.SCREEN_OF_65_CHUNKS` through the test above, a batch of 2: 64 lanes of the finishing kernel add one chunk each and
    lane 0 a second one.  The float32 bounds are those of 612 x 511."""
    from lynx_amd import _ffi

    label = "3x43691"
    assert -(-3 * 43691 // _ffi.IMAGE_GRAD_CELLS) == 65
    monkeypatch.setitem(il.LOSS_SCREENS, label, ref.SCREEN_OF_65_CHUNKS)
    monkeypatch.setitem(il.FLOAT32_ENTRY_DEVIATION, label, il.FLOAT32_ENTRY_DEVIATION[LARGEST])
    monkeypatch.setitem(il.FLOAT32_LOSS_DEVIATION, label, il.FLOAT32_LOSS_DEVIATION[LARGEST])
    test_the_kernels_alone_against_the_restatement(lx, dtype, label, (2,), False, False)


# ---------------------------------------------------------------------------------------------
# 7. agreement with the existing path
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("label", ["1", "65", "257", "561", "1x257", "89x71"])
def test_agreement_with_screens_and_a_cotangent_formed_in_numpy_fp64(lx, label):
    dtype, shape = np.float64, (3,)
    segment, beam, screen, targets, given, mis = loss_case(lx, label, dtype, shape, False, False)
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": given})
    g = vjp(image_loss_bar=1.0)
    existing = lx.grad.track_along_vjp(segment, beam, screens=True)
    image = np.asarray(existing.trace.image_at("SCREEN"), dtype=np.float64)
    n = image.shape[-2] * image.shape[-1]
    h = existing(screen_images_bar={"SCREEN": 2.0 * (image - targets) / n})
    loss, by_numpy = vjp.image_loss_of(screen), np.mean(np.square(image - targets), axis=(-2, -1))
    print(f"{label}: loss {loss}, of the downloaded image {by_numpy}")
    assert np.all(np.abs(loss - by_numpy) <= 1e-12 * by_numpy) and np.all(by_numpy > 0)
    _, _, got = entries_of(g, 3)
    _, _, want = entries_of(h, 3)
    sizes = [case[3] for case in restated(vjp, il.LOSS_SCREENS[label], dtype, targets, mis, shape)]
    for s in range(3):
        for name in ref.ENTRIES:
            assert abs(got[s][name] - want[s][name]) <= 1e-10 * sizes[s][name], (s, name, got[s][name], want[s][name], sizes[s][name])
            assert want[s][name] != 0
    assert np.all(np.abs(g[screen]["misalignment"] - h[screen]["misalignment"])
                  <= 1e-10 * np.array([[sizes[s]["mu_x"], sizes[s]["mu_y"]] for s in range(3)]))
    assert np.array_equal(g.energy, h.energy)  # (nothing reaches the energy: a screen and a drift)
    for el in vjp.leaves[1:]:
        assert np.array_equal(g[el]["length"], h[el]["length"])


# ---------------------------------------------------------------------------------------------
# 8. the loss of the image itself
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("label", SMALL)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_loss_of_the_image_itself_is_exactly_zero(lx, dtype, label):
    """The density is formed with the forward kernel's expression: against the image `track_along(screens=True)` shows, every
    difference is an exact zero, and so are the loss and the five entries."""
    shape = (3,)
    segment, beam, screen, _, _, _ = loss_case(lx, label, dtype, shape, False, False)
    image = np.array(segment.track_along(beam, screens=True).image_at("SCREEN"))
    assert image.dtype == np.dtype(dtype) and np.all(image.max(axis=(-2, -1)) > 0)
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": image})
    assert np.array_equal(vjp.image_loss_of("SCREEN"), np.zeros(shape))
    g = vjp(image_loss_bar=1.0)
    assert np.all(np.asarray(g.mu) == 0) and np.all(np.asarray(g.cov) == 0) and np.all(g[screen]["misalignment"] == 0)
    # ... and of another sample's image it is not
    rolled = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": np.roll(image, 1, axis=0)})
    assert np.all(rolled.image_loss_of("SCREEN") > 0)


# ---------------------------------------------------------------------------------------------
# 9. the same call twice
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype, label", [(np.float32, LARGEST), (np.float64, LARGEST), (np.float64, "89x71")])
def test_the_same_call_twice_returns_the_same_bits(lx, dtype, label):
    shape = (3,)
    k1 = np.linspace(-2.0, 3.0, 3).astype(dtype)
    full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    geometry = il.LOSS_SCREENS[label]
    quad, corrector = lx.Quadrupole(full(0.2), k1=k1, dtype=dtype), lx.HorizontalCorrector(full(0.1), angle=full(3e-5), dtype=dtype)
    screen = make_screen(lx, geometry, np.array([1e-4, -2e-4]), dtype, "SCREEN")
    elements = [lx.Drift(full(0.6), dtype=dtype), quad, corrector, lx.Drift(full(0.8), dtype=dtype), screen]
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-4), mu_y=full(-1e-4), sigma_x=full(1.2e-3), sigma_xp=full(1e-4), sigma_y=full(1e-3),
                                            sigma_yp=full(1e-4), sigma_s=full(1e-5), sigma_p=full(1e-3), energy=full(1e8), dtype=dtype)
    target = il.mismatch_target(geometry, dtype)[3]
    targets = lx.grad.ImageTargets({"SCREEN": target})
    passes = [lx.grad.track_along_vjp(lx.Segment(elements), beam, image_targets=targets) for _ in range(2)]
    assert np.array_equal(passes[0].image_loss_of("SCREEN"), passes[1].image_loss_of("SCREEN")) and np.all(passes[0].image_loss_of("SCREEN") > 0)
    first, second, third = passes[0](image_loss_bar=1e-9, sigma_x=1e3), passes[0](image_loss_bar=1e-9, sigma_x=1e3), passes[1](image_loss_bar=1e-9, sigma_x=1e3)
    for other in (second, third):
        assert np.array_equal(first.mu, other.mu) and np.array_equal(first.cov, other.cov) and np.array_equal(first.energy, other.energy)
        for el in elements:
            for name, value in first[el].items():
                assert np.array_equal(value, other[el][name]), (el.name, name)
    assert np.any(first.mu != 0) and np.all(np.isfinite(first.cov))
    assert np.all(first[quad]["k1"] != 0) and np.all(first[screen]["misalignment"] != 0)


# ---------------------------------------------------------------------------------------------
# 10. end to end, float64
# ---------------------------------------------------------------------------------------------


def test_end_to_end_against_central_differences_of_the_oracle_fp64(lx):
    """The two-screen lattice of tests/test_gpu_trace_screens.py with SCREEN_B alone named: L = sum over the samples of
    bar_b mean (image_b - target_b)^2 by k1, the corrector's angle, the lengths, the incoming energy and SCREEN_B's (shared)
    misalignment; the tolerances of that file's test of the same name.  A central difference is taken pixel by pixel and summed
    then."""
    dtype = np.float64
    elements, a, b, beam, mu, cov, energy, _, _ = end_to_end_case(lx, dtype)
    f = lambda v: np.full((B6,), v)  # noqa: E731
    desc = DESC_6(f, np.linspace(-4.0, 5.0, B6))
    _, specs = make_lattice(desc, dtype)
    shown = np.asarray(lx.Segment(elements).track_along(beam, screens=True).image_at("SCREEN_B"), dtype=np.float64)
    target = 1.2 * np.roll(shown, (-3, 2), axis=(-2, -1))
    bar = np.array([1.0, 0.5, 2.0])
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, image_targets={b: target})
    assert vjp.trace.screens == [2, 5] and list(vjp.image_loss) == ["SCREEN_B"]
    mis = np.asarray(MIS_B, dtype=dtype).copy()

    def images(mu_, cov_, energy_):
        at = _chain(specs, o.parameter_beam(mu_, cov_, energy_, np.float64))[5]
        seen = np.array(at["mu"])
        seen[:, 0] -= mis[0]
        seen[:, 2] -= mis[1]
        return o.screen_reading_parameters(seen, at["cov"], **SCREEN_B, dtype=dtype)

    n = target.shape[-2] * target.shape[-1]
    # (the images agree to 1e-10 of their peak, `TOL_IMAGE`; the difference to the target is a tenth of the peak and more where
    # it counts, so the loss agrees to 1e-8)
    assert np.all(np.abs(vjp.image_loss_of(5) - np.mean(np.square(images(mu, cov, energy) - target), axis=(-2, -1)))
                  <= 1e-8 * vjp.image_loss_of(5))

    def difference(up, down):
        """(B,): bar_b (mean (up_b - T_b)^2 - mean (down_b - T_b)^2), summed pixel by pixel."""
        return bar * np.sum((up - down) * (up + down - 2 * target), axis=(-2, -1)) / n

    g = vjp(image_loss_bar=bar)

    def central(apply, x0, h):
        apply(x0 + h)
        up = images(mu, cov, energy)
        apply(x0 - h)
        down = images(mu, cov, energy)
        apply(x0)
        return difference(up, down) / (2 * h)

    checked = 0
    for e, name in ((0, "length"), (1, "length"), (1, "k1"), (3, "length"), (3, "angle"), (4, "length")):
        arr = specs[e][name]
        got = g[elements[e]][name]
        assert got.shape == arr.shape
        for idx in np.ndindex(arr.shape):
            def apply(x, arr=arr, idx=idx):
                arr[idx] = x
            reference = central(apply, arr[idx], 1e-6 * max(abs(arr[idx]), 1e-2))[idx[0]]
            assert abs(got[idx] - reference) <= 2e-4 * abs(reference) + 1e-7 * np.max(np.abs(got)), (e, name, idx, got[idx], reference)
            assert reference != 0
            checked += 1
    assert checked == 18
    for s in range(B6):
        h = 1e-6 * energy[s]
        ep, em = energy.copy(), energy.copy()
        ep[s] += h
        em[s] -= h
        reference = difference(images(mu, cov, ep), images(mu, cov, em))[s] / (2 * h)
        assert abs(g.energy[s] - reference) <= 2e-4 * abs(reference) + 1e-12, (s, g.energy[s], reference)
    # the misalignments: SCREEN_B's is shared, so its gradient is the sum over the samples; SCREEN_A is not named
    got = g[b]["misalignment"]
    assert got.shape == (2,)
    for c in range(2):
        def apply(x, c=c):
            mis[c] = x
        reference = central(apply, mis[c], 1e-9).sum()
        assert abs(got[c] - reference) <= 1e-5 * abs(reference) + 1e-9 * np.max(np.abs(got)), (c, got[c], reference)
    assert a in g and g[a]["misalignment"].shape == (B6, 2) and np.all(g[a]["misalignment"] == 0)


# ---------------------------------------------------------------------------------------------
# 11. position and neighbours of a screen, and the cotangent
# ---------------------------------------------------------------------------------------------


def assert_k1_as_explicit(lx, segment, quad, beam, named, dtype=np.float64):
    """`named`: {screen name: (geometry, misalignment)}; the image loss call against the call with the restatement's moment
    cotangents given explicitly.  The target of a screen is 1.2 x its own image, rolled."""
    shown = lx.grad.track_along_vjp(segment, beam, screens=True).trace
    targets = {name: 1.2 * np.roll(np.asarray(shown.image_at(name), dtype=np.float64), (2, 1), axis=(-2, -1)) for name in named}
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets=targets)
    g = vjp(image_loss_bar=1.0)
    trace = vjp.trace
    Bn, Pn = trace._mu.shape[0], trace.num_points
    mu_bar, cov_bar = np.zeros((Bn, Pn, 7)), np.zeros((Bn, Pn, 7, 7))
    for name, (geometry, mis) in named.items():
        k = trace.names.index(name)
        xs, ys = ref.pixel_grid(**geometry, dtype=dtype)
        shifts = np.broadcast_to(np.asarray(mis, dtype=dtype), (Bn, 2))
        for s in range(Bn):
            m, c = trace._mu[s, k], trace._cov[s, k]
            loss, entries, _, _ = il.image_loss(m[0] - shifts[s, 0], m[2] - shifts[s, 1], c[0, 0], c[0, 2], c[2, 2], xs, ys, targets[name][s])
            assert abs(vjp.image_loss_of(name)[s] - loss) <= 1e-10 * loss
            mb, cb = ref.moment_cotangents(entries)
            mu_bar[s, k] += mb
            cov_bar[s, k] += cb
    explicit = vjp(mu_bar=mu_bar, cov_bar=cov_bar)
    got, want = g[quad]["k1"], explicit[quad]["k1"]
    print(f"k1 gradients {got} explicit {want}")
    assert np.all(want != 0) and np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    return vjp, g


def test_a_screen_as_the_last_element(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    last = make_screen(lx, SCREEN_B, MIS_B, np.float64, "LAST")
    vjp, g = assert_k1_as_explicit(lx, lx.Segment(elements + [last]), quad, beam, {"LAST": (SCREEN_B, MIS_B)})
    assert vjp.trace.screens == [3] and vjp.trace.num_points == 5


def test_two_screens_directly_after_each_other_both_named(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    one, two = make_screen(lx, SCREEN_A, mis_a(shape), np.float64, "ONE"), make_screen(lx, SCREEN_B, MIS_B, np.float64, "TWO")
    segment = lx.Segment(elements + [one, two, lx.Drift(np.full(shape, 0.3), dtype=np.float64)])
    vjp, g = assert_k1_as_explicit(lx, segment, quad, beam, {"ONE": (SCREEN_A, mis_a(shape)), "TWO": (SCREEN_B, MIS_B)})
    assert vjp.trace.screens == [3, 4] and set(vjp.image_loss) == {"ONE", "TWO"}
    assert np.all(g[one]["misalignment"] != 0) and np.all(g[two]["misalignment"] != 0)


def test_a_screen_inside_a_nested_segment(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    inner = make_screen(lx, SCREEN_B, MIS_B, np.float64, "INNER")
    segment = lx.Segment([elements[0], lx.Segment([elements[1], lx.Segment([elements[2], inner])]), lx.Drift(np.full(shape, 0.3), dtype=np.float64)])
    vjp, g = assert_k1_as_explicit(lx, segment, quad, beam, {"INNER": (SCREEN_B, MIS_B)})
    assert vjp.trace.screens == [3] and inner in g


def behind_the_front(lx, dtype, aperture=None):
    shape = (3,)
    elements, quad, beam = front(lx, shape, dtype)
    screen = make_screen(lx, SCREEN_B, MIS_B, dtype, "SCREEN")
    segment = lx.Segment([elements[0]] + ([aperture] if aperture is not None else []) + [elements[1], elements[2], screen])
    target = il.mismatch_target(SCREEN_B, dtype)[3]
    return segment, elements, quad, beam, screen, target


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_losses_with_an_active_aperture_change_no_bit(lx, dtype):
    aperture = lx.Aperture(x_max=np.asarray([5e-5], dtype=dtype), y_max=np.asarray([5e-5], dtype=dtype), is_active=True, name="AP", dtype=dtype)
    segment, elements, quad, beam, screen, target = behind_the_front(lx, dtype, aperture)
    with pytest.raises(NotImplementedError, match="AP"):
        lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": target})
    collimated = lx.grad.track_along_vjp(segment, beam, losses=True, image_targets={"SCREEN": target})
    with_losses = collimated(image_loss_bar=1e-9, sigma_y=1e10)
    assert aperture not in with_losses  # (a ParameterBeam: the plain problem)
    aperture.is_active = False
    free = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": target})
    assert np.array_equal(free.image_loss_of("SCREEN"), collimated.image_loss_of("SCREEN")) and np.all(free.image_loss_of("SCREEN") > 0)
    plain = free(image_loss_bar=1e-9, sigma_y=1e10)
    assert np.array_equal(plain.mu, with_losses.mu) and np.array_equal(plain.cov, with_losses.cov) and np.array_equal(plain.energy, with_losses.energy)
    for el in (elements[0], quad, elements[2]):
        for name, value in plain[el].items():
            assert np.array_equal(value, with_losses[el][name]), (el.name, name)
    assert np.array_equal(plain[screen]["misalignment"], with_losses[screen]["misalignment"]) and np.all(plain[quad]["k1"] != 0)


def test_a_cotangent_of_zero_for_one_sample_gives_that_sample_gradient_zero(lx):
    segment, elements, quad, beam, screen, target = behind_the_front(lx, np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": target})
    g, whole = vjp(image_loss_bar=np.array([2.0, 0.0, 0.5])), vjp(image_loss_bar=1.0)
    assert np.all(whole[quad]["k1"] != 0) and np.all(whole.mu[:, 0] != 0)
    assert g[quad]["k1"][1] == 0 and np.all(g.mu[1] == 0) and np.all(g.cov[1] == 0) and g.energy[1] == 0
    for s, factor in ((0, 2.0), (2, 0.5)):  # (a power of two: the same bits, scaled)
        assert g[quad]["k1"][s] == factor * whole[quad]["k1"][s] and np.array_equal(g.mu[s], factor * whole.mu[s])
    by_name = vjp(image_loss_bar={"SCREEN": np.array([2.0, 0.0, 0.5])})
    assert np.array_equal(by_name[quad]["k1"], g[quad]["k1"]) and np.array_equal(by_name[screen]["misalignment"], g[screen]["misalignment"])


def test_the_loss_and_a_twiss_cotangent_in_one_call_are_the_sum_of_two_calls(lx):
    segment, elements, quad, beam, screen, target = behind_the_front(lx, np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": target})
    scale = 1.0 / target.max() ** 2
    both, loss_only, twiss_only = vjp(image_loss_bar=scale, beta_x=1e-3), vjp(image_loss_bar=scale), vjp(beta_x=1e-3)
    print(f"k1 gradient: of the image loss {loss_only[quad]['k1']}, of beta_x {twiss_only[quad]['k1']}")
    assert np.all(loss_only[quad]["k1"] != 0) and np.all(twiss_only[quad]["k1"] != 0)
    for el, name in ((elements[0], "length"), (quad, "k1"), (quad, "length"), (elements[2], "length")):
        total = loss_only[el][name] + twiss_only[el][name]
        size = np.maximum(np.abs(loss_only[el][name]), np.abs(twiss_only[el][name]))
        assert np.all(np.abs(both[el][name] - total) <= 1e-12 * size), (el.name, name, both[el][name], total)
    for whole, halves in ((both.mu, loss_only.mu + twiss_only.mu), (both.cov, loss_only.cov + twiss_only.cov),
                          (both.energy, loss_only.energy + twiss_only.energy)):
        assert np.all(np.abs(whole - halves) <= 1e-12 * np.max(np.abs(whole)))
    assert np.array_equal(both[screen]["misalignment"], loss_only[screen]["misalignment"])


def test_with_screens_as_well_both_cotangents_are_taken_in_one_call(lx):
    segment, elements, quad, beam, screen, target = behind_the_front(lx, np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, screens=True, image_targets={"SCREEN": target})
    image = np.asarray(vjp.trace.image_at("SCREEN"), dtype=np.float64)
    assert screen.reading is vjp.trace.image_at("SCREEN")
    W = image - 1.2 * np.roll(image, (2, 1), axis=(-2, -1))
    both, loss_only, image_only = vjp(image_loss_bar=1.0, screen_images_bar={"SCREEN": W / image.max()}), vjp(image_loss_bar=1.0), vjp(
        screen_images_bar={"SCREEN": W / image.max()})
    for got, parts in ((both[quad]["k1"], loss_only[quad]["k1"] + image_only[quad]["k1"]),
                       (both[screen]["misalignment"], loss_only[screen]["misalignment"] + image_only[screen]["misalignment"])):
        assert np.all(parts != 0) and np.all(np.abs(got - parts) <= 1e-12 * np.abs(parts)), (got, parts)


# ---------------------------------------------------------------------------------------------
# 12. the C entries refuse
# ---------------------------------------------------------------------------------------------

SCREEN = [2, NX, NY]  # a screen at point 2 of the trace of tests/test_gpu_entry_refusals.py
PREFIX = "image loss along the trace: "
TOO_MANY_PIXELS = [2, 46341, 46341]  # 2 147 488 281 cells: beyond 2^31 - 2048


@pytest.fixture(scope="module")
def loss_arrays(env):
    rt, dtype = env.rt, env.dtype
    rng = np.random.default_rng(17)
    return dict(targets=rt.to_device(rng.uniform(0, 1e7, (B, NX * NY)).astype(dtype)), loss=rt.empty((B, 1), np.float64),
                sums=rt.empty((B, 1, 6), np.float64), loss_bar=rt.to_device(np.array([[1.0], [-0.5]], dtype=dtype)))


def forward_call(env, arrays, **change):
    a = dict(batch=B, screens=SCREEN, stride=0, offsets=[0], targets="targets", target_stride=NX * NY, loss="loss", sums="sums")
    a.update(change)
    p = lambda name, own=arrays: None if name is None else C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
    status = env.rt.lib.lynx_gaussian_images_along_mse(
        env.rt.ctx, env.code, a["batch"], P, p("mu_tr"), p("cov_tr"), 1, ints(a["screens"]), p("grid"), p("misalignment"), a["stride"],
        (C.c_int64 * 1)(*a["offsets"]), p(a["targets"]), a["target_stride"], p(a["loss"]), p(a["sums"]))
    return status, env.rt.lib.lynx_last_error(env.rt.ctx).decode()


def backward_call(env, arrays, **change):
    a = dict(batch=B, screens=SCREEN, sums="sums", mu_bar="mu_bar_out", g_mis="g_mis")
    a.update(change)
    p = lambda name, own=arrays: None if name is None else C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
    status = env.rt.lib.lynx_gaussian_images_along_mse_backward(
        env.rt.ctx, env.code, a["batch"], P, p("cov_tr"), 1, ints(a["screens"]), p(a["sums"]), p("loss_bar"), p(a["mu_bar"]), p("cov_bar_out"),
        p(a["g_mis"]))
    return status, env.rt.lib.lynx_last_error(env.rt.ctx).decode()


def zeroed(env, arrays, names):
    rt = env.rt
    for name in names:
        block = arrays[name] if name in arrays else env.a[name]
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(block.ptr), 0, block.nbytes))


def read(env, arrays, names):
    return [(arrays[name] if name in arrays else env.a[name]).numpy().tobytes() for name in names]


FORWARD_REFUSALS = {
    "a null loss": (dict(loss=None), "bad argument"),
    "null targets": (dict(targets=None), "bad argument"),
    "a batch of 65536": (dict(batch=65536), "bad argument"),
    "a misalignment stride of 1": (dict(stride=1), "the misalignments' sample stride is 0 or 2 * n_screens"),
    "a target stride below the cells": (dict(target_stride=NX * NY - 1), "the targets' sample stride is 0 or at least the cells the offsets name"),
    "an offset that pushes the cells beyond the stride": (dict(offsets=[1]), "the targets' sample stride is 0 or at least the cells the offsets name"),
    "a screen outside the trace": (dict(screens=[P, NX, NY]), "a screen's point lies inside the trace, and it has pixels"),
    "a screen without pixels": (dict(screens=[2, 0, NY]), "a screen's point lies inside the trace, and it has pixels"),
    "2^31 - 2048 pixels or more": (dict(screens=TOO_MANY_PIXELS), "a screen has fewer than 2^31 - 2048 pixels"),
    "an offset of -2": (dict(offsets=[-2]), "a target's offset is -1 (no target) or not negative"),
}
BACKWARD_REFUSALS = {
    "a null mu_bar": (dict(mu_bar=None), "bad argument"),
    "null sums": (dict(sums=None), "bad argument"),
    "a batch of 65536": (dict(batch=65536), "bad argument"),
    "a screen outside the trace": (dict(screens=[-1, NX, NY]), "a screen's point lies inside the trace, and it has pixels"),
    "2^31 - 2048 pixels or more": (dict(screens=TOO_MANY_PIXELS), "a screen has fewer than 2^31 - 2048 pixels"),
}


@pytest.mark.parametrize("case", sorted(FORWARD_REFUSALS))
def test_the_forward_entry_refuses_and_the_next_valid_call_returns_the_same_bytes(env, loss_arrays, case):
    change, expected = FORWARD_REFUSALS[case]
    outputs = ["loss", "sums"]
    zeroed(env, loss_arrays, outputs)
    status, message = forward_call(env, loss_arrays)
    assert status == 0, message
    before = read(env, loss_arrays, outputs)
    zeroed(env, loss_arrays, outputs)
    assert forward_call(env, loss_arrays, **change) == (INVALID, PREFIX + expected)
    assert not any(any(block) for block in read(env, loss_arrays, outputs))  # (refused before anything was launched)
    status, message = forward_call(env, loss_arrays)
    assert status == 0, message
    assert read(env, loss_arrays, outputs) == before and all(any(block) for block in before)
    assert {name: env.a[name].numpy().tobytes() for name in env.keep} == env.keep
    # a screen without a target: loss 0 and sums 0, and a shared target is sample 0's row
    assert forward_call(env, loss_arrays, offsets=[-1])[0] == 0 and not any(any(block) for block in read(env, loss_arrays, outputs))
    status, _ = forward_call(env, loss_arrays, target_stride=0)
    shared = np.frombuffer(read(env, loss_arrays, ["loss"])[0], dtype=np.float64)
    assert status == 0 and shared[0] == np.frombuffer(before[0], dtype=np.float64)[0] and shared[1] != np.frombuffer(before[0], dtype=np.float64)[1]


@pytest.mark.parametrize("case", sorted(BACKWARD_REFUSALS))
def test_the_reverse_entry_refuses_and_the_next_valid_call_returns_the_same_bytes(env, loss_arrays, case):
    change, expected = BACKWARD_REFUSALS[case]
    outputs = ["mu_bar_out", "cov_bar_out", "g_mis"]
    status, message = forward_call(env, loss_arrays)
    assert status == 0, message
    zeroed(env, loss_arrays, outputs)
    status, message = backward_call(env, loss_arrays)
    assert status == 0, message
    before = read(env, loss_arrays, outputs)
    zeroed(env, loss_arrays, outputs)
    assert backward_call(env, loss_arrays, **change) == (INVALID, PREFIX + expected)
    assert not any(any(block) for block in read(env, loss_arrays, outputs))
    status, message = backward_call(env, loss_arrays)
    assert status == 0, message
    assert read(env, loss_arrays, outputs) == before and all(any(block) for block in before)
    status, message = backward_call(env, loss_arrays, g_mis=None)  # (the misalignment gradient is optional)
    assert status == 0, message
    assert {name: env.a[name].numpy().tobytes() for name in env.keep} == env.keep


def test_65_screens_of_one_pixel_through_both_entries(env):
    """More screens than one launch of the reverse half takes (64): 65 screens of one pixel each on the four points of the
    trace of tests/test_gpu_entry_refusals.py, screens 63 and 64 on one point, misalignments per sample, every third screen
    without a target.  The loss, the reverse half's additions at every point and the misalignments' gradients against the
    restatement, under the bounds of the single pixel ("1") of the kernels' own test; a screen without a target is all zeros."""
    rt, dtype = env.rt, env.dtype
    K = 65
    rng = np.random.default_rng(65)
    points = [((k + 1) // 2) % P for k in range(K)]
    named = [k % 3 != 1 or k == 64 for k in range(K)]
    assert points[63] == points[64] and named[0] and named[63] and named[64] and not all(named)
    pixels = rng.uniform(-2e-4, 2e-4, (K, 2)).astype(dtype)  # a screen's grid: its one x, its one y
    mis = (1e-5 * rng.standard_normal((B, K, 2))).astype(dtype)
    bars = np.where(named, rng.uniform(0.5, 2.0, (B, K)) * rng.choice([-1.0, 1.0], (B, K)), 3.0).astype(dtype)  # (3: on nothing)
    mu, cov = env.host["mu_tr"].reshape(B, P, 7), env.host["cov_tr"].reshape(B, P, 7, 7)
    state = lambda s, k: (mu[s, points[k], 0] - mis[s, k, 0], mu[s, points[k], 2] - mis[s, k, 1],  # noqa: E731
                          cov[s, points[k], 0, 0], cov[s, points[k], 0, 2], cov[s, points[k], 2, 2])
    columns = {k: j for j, k in enumerate(reversed([k for k in range(K) if named[k]]))}  # (the targets in another order)
    targets = np.zeros((B, len(columns)), dtype=dtype)
    for k, j in columns.items():
        for s in range(B):
            targets[s, j] = rng.uniform(0.5, 1.5) * ref.density(*state(s, k), pixels[k, :1], pixels[k, 1:])[0][0, 0]
    assert np.all(targets > 0)
    if dtype == np.float64:
        tol_entry = tol_loss = TOL_IMAGE[np.float64]
    else:
        tol_entry, tol_loss = FLOAT32_FACTOR * il.FLOAT32_ENTRY_DEVIATION["1"], FLOAT32_FACTOR * il.FLOAT32_LOSS_DEVIATION["1"]
    want, worst32 = {}, 0.0
    for k, j in columns.items():
        for s in range(B):
            arguments = (*state(s, k), pixels[k, :1], pixels[k, 1:], targets[s, j].reshape(1, 1))
            want[s, k] = il.image_loss(*arguments)
            if dtype == np.float32:  # (the float32 restatement itself stays inside the bound on these inputs)
                loss32, single, _, _ = il.image_loss(*arguments, "float32")
                ref_loss, entries, loss_size, sizes = want[s, k]
                worst32 = max(worst32, abs(loss32 - ref_loss) / loss_size / tol_loss,
                              *(abs(single[name] - entries[name]) / sizes[name] / tol_entry for name in ref.ENTRIES))
    print(f"{np.dtype(dtype).name}: the float32 restatement is at most {worst32:.2f} of the bound away from the float64 one")
    assert worst32 <= 0.5

    own = dict(grid=rt.to_device(pixels.reshape(-1)), mis=rt.to_device(mis), targets=rt.to_device(targets), bars=rt.to_device(bars),
               loss=rt.empty((B, K), np.float64), sums=rt.empty((B, K, 6), np.float64), g_mis=rt.empty((B, K, 2), dtype))
    p = lambda name: C.c_void_p((own[name] if name in own else env.a[name]).ptr)  # noqa: E731
    rows = ints([v for k in range(K) for v in (points[k], 1, 1)])
    offsets = (C.c_int64 * K)(*[columns.get(k, -1) for k in range(K)])
    rt.check(rt.lib.lynx_gaussian_images_along_mse(rt.ctx, env.code, B, P, p("mu_tr"), p("cov_tr"), K, rows, p("grid"), p("mis"), 2 * K,
                                                   offsets, p("targets"), targets.shape[1], p("loss"), p("sums")))
    zeroed(env, own, ["mu_bar_out", "cov_bar_out"])
    rt.check(rt.lib.lynx_gaussian_images_along_mse_backward(rt.ctx, env.code, B, P, p("cov_tr"), K, rows, p("sums"), p("bars"),
                                                            p("mu_bar_out"), p("cov_bar_out"), p("g_mis")))
    loss, sums, g_mis = own["loss"].numpy(), own["sums"].numpy(), own["g_mis"].numpy().astype(np.float64)
    g_mu, g_cov = env.a["mu_bar_out"].numpy().reshape(B, P, 7), env.a["cov_bar_out"].numpy().reshape(B, P, 7, 7)
    at = {"mu_x": lambda s, q: g_mu[s, q, 0], "mu_y": lambda s, q: g_mu[s, q, 2], "cov_xx": lambda s, q: g_cov[s, q, 0, 0],
          "cov_yy": lambda s, q: g_cov[s, q, 2, 2], "cov_xy": lambda s, q: g_cov[s, q, 0, 2]}
    worst = {"loss": 0.0, "misalignment": 0.0, "entries": 0.0}
    for s in range(B):
        for k in range(K):
            if not named[k]:
                assert loss[s, k] == 0 and not sums[s, k].any() and not g_mis[s, k].any(), (s, k)
                continue
            ref_loss, entries, loss_size, sizes = want[s, k]
            worst["loss"] = max(worst["loss"], abs(loss[s, k] - ref_loss) / loss_size / tol_loss)
            for axis, name in enumerate(("mu_x", "mu_y")):
                assert entries[name] != 0
                distance = abs(g_mis[s, k, axis] + float(bars[s, k]) * entries[name]) / (abs(float(bars[s, k])) * sizes[name])
                worst["misalignment"] = max(worst["misalignment"], distance / tol_entry)
        for q in range(P):  # what the screens on a point add there, in their order
            here = [k for k in range(K) if named[k] and points[k] == q]
            assert len(here) > 1
            for name in ref.ENTRIES:
                total = sum(float(bars[s, k]) * want[s, k][1][name] for k in here)
                size = sum(abs(float(bars[s, k])) * want[s, k][3][name] for k in here)
                worst["entries"] = max(worst["entries"], abs(float(at[name](s, q)) - total) / size / tol_entry)
    print(f"{np.dtype(dtype).name}: worst distances in units of the bound {worst}")
    assert max(worst.values()) <= 1, worst
    assert np.array_equal(g_cov[..., 0, 2], g_cov[..., 2, 0]) and np.all(g_mis[:, [0, 63, 64]] != 0)
    seen_mu, seen_cov = np.zeros(7, dtype=bool), np.zeros((7, 7), dtype=bool)
    seen_mu[[0, 2]] = True
    seen_cov[[0, 0, 2, 2], [0, 2, 0, 2]] = True
    assert np.all(g_mu[..., ~seen_mu] == 0) and np.all(g_cov[..., ~seen_cov] == 0)
    assert {name: env.a[name].numpy().tobytes() for name in env.keep} == env.keep


# ---------------------------------------------------------------------------------------------
# 13. the example
# ---------------------------------------------------------------------------------------------


def test_match_screen_image_on_device_example_converges(lx):
    """examples/match_screen_image_on_device.py: the loss falls as test_match_screen_image_example_converges asks of
    match_screen_image.py, and the settings it ends at are a match by that example's own loss -- the image read back, the
    difference formed in numpy -- within the same factor."""
    examples = pathlib.Path(__file__).resolve().parents[1] / "examples"
    spec = importlib.util.spec_from_file_location("match_screen_image_on_device", examples / "match_screen_image_on_device.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.screen_line(), example.incoming_beam()
    target = example.target_image(segment, beam)
    assert target.shape[0] == 1 and target.size < 3000 and target.max() > 0
    by_numpy = lambda: float(np.mean(np.square((np.asarray(segment.track_along(beam, screens=True).image_at("SCREEN"), dtype=np.float64)  # noqa: E731
                                                - target) / target.max())))
    at_first = by_numpy()
    history = example.tune(segment, beam, target)
    print(f"loss {history[0]:.3e} -> {history[-1]:.3e}; by the existing example's loss {at_first:.3e} -> {by_numpy():.3e}; "
          f"settings {example.settings(segment)}")
    assert abs(history[0] - at_first) <= 1e-12 * at_first  # (the same loss: the same float32 image, float64 differences)
    assert history[-1] <= history[0] / 100, (history[0], history[-1])
    assert by_numpy() <= at_first / 100, (at_first, by_numpy())
