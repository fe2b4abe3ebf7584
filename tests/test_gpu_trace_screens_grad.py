"""
`lynx_amd.grad.track_along_vjp(..., screens=True)` on the GPU: gradients of a ParameterBeam's screen images
(lynx_gaussian_images_along_backward in front of lynx_track_moments_along_backward).

The kernel alone through the public interface (a screen as the first element observes point 0: `g.mu`, `g.cov` are the
kernel's own mu_bar, cov_bar) against the float64 restatement of tests/screen_grad_reference.py, entry by entry and
relative to every entry's UNCANCELLED SIZE (that file says what it is); end to end against central differences of the
oracle's chain and image; the position and the neighbours of a screen; float32 against float64; the example.

Tolerances of the kernel alone:
    float64  1e-10 of the uncancelled size (`TOL_IMAGE` of tests/test_gpu_screen.py, the project's float64 image tolerance);
    float32  8 x what the float32 restatement deviates from the float64 one on the same inputs -- the base is
             `FLOAT32_RESTATEMENT_DEVIATION[screen]` of tests/screen_grad_reference.py, measured and asserted by
             tests/test_trace_screens_grad_host.py (2.2e-7 on 612 x 511 cells ... 1.9e-6 on a single pixel), so the constant
             runs from 8 x 2.8e-7 = 2.2e-6 to 8 x 2.35e-6 = 1.9e-5.  The factor covers another order of operations, the
             device's log and division, and the kernel's products in float64.
"""

import importlib.util
import pathlib

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import screen_grad_reference as ref
from .helpers import make_lattice
from .test_gpu_screen import TOL_IMAGE
from .test_gpu_trace_grad import _chain
from .test_gpu_trace_screens import MIS_B, SCREEN_A, SCREEN_B, make_screen, mis_a, two_screen_lattice

pytestmark = pytest.mark.gpu

FLOAT32_FACTOR = 8
LARGEST = "612x511"


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


# ---------------------------------------------------------------------------------------------
# 4. the kernel alone
# ---------------------------------------------------------------------------------------------


def kernel_case(lx, label, dtype, shape, shared):
    """[Screen, Drift] and a correlated beam per sample that the screen's extent cuts; the screen's misalignment per sample
    or shared.  Returns (vjp, screen, W (*shape, nx, ny) float64, the misalignment as the screen holds it)."""
    geometry = ref.KERNEL_SCREENS[label]
    B = int(np.prod(shape))
    hx, hy = (geometry["resolution"][k] * geometry["pixel_size"][k] / 2 for k in (0, 1))
    mis = np.array([0.07 * hx, -0.05 * hy]) if shared else np.random.default_rng(5).normal(0, 0.05, (*shape, 2)) * [hx, hy]
    mis = np.asarray(mis, dtype=dtype)
    mu, cov = np.zeros((B, 7)), np.zeros((B, 7, 7))
    shifts = np.broadcast_to(mis, (*shape, 2)).reshape(B, 2).astype(np.float64)
    for s in range(B):
        mx, my, a, b, c = ref.beam_on(geometry, rho=0.5 - 0.2 * s, scale=1.0 + 0.1 * s, shift=(0.05 * s, -0.03 * s))  # (`mismatch_cotangent`'s)
        m = shifts[s]
        mu[s, 0], mu[s, 2], mu[s, 6] = mx + m[0], my + m[1], 1.0
        cov[s, 0, 0], cov[s, 0, 2], cov[s, 2, 0], cov[s, 2, 2] = a, b, b, c
        cov[s, 1, 1] = cov[s, 3, 3] = 1e-10
        cov[s, 0, 1] = cov[s, 1, 0] = 1e-6 * np.sqrt(a)  # (entries the image does not see)
    beam = lx.ParameterBeam(mu.reshape(*shape, 7).astype(dtype), cov.reshape(*shape, 7, 7).astype(dtype), np.full(shape, 1e8, dtype=dtype),
                            dtype=dtype)
    screen = make_screen(lx, geometry, mis, dtype, "SCREEN")
    vjp = lx.grad.track_along_vjp(lx.Segment([screen, lx.Drift(np.full(shape, 0.5, dtype=dtype), dtype=dtype)]), beam, screens=True)
    image = vjp.trace.image_at(0)
    other = np.stack([ref.density(*ref.beam_on(geometry, rho=-0.2, scale=1.3, shift=(0.15, -0.2)), *ref.pixel_grid(**geometry, dtype=dtype))[0]] * B)
    W = image.astype(np.float64) - other.reshape(image.shape)
    return vjp, screen, W, mis


def restated(vjp, geometry, dtype, W, mis, shape):
    """Per sample the float64 restatement on the trace's own values (mu less the misalignment formed in the dtype)."""
    xs, ys = ref.pixel_grid(**geometry, dtype=dtype)
    B = int(np.prod(shape))
    mu, cov = np.asarray(vjp.trace._mu)[..., 0, :].reshape(B, 7), np.asarray(vjp.trace._cov)[..., 0, :, :].reshape(B, 7, 7)
    assert mu.dtype == np.dtype(dtype)
    shifts = np.broadcast_to(mis, (*shape, 2)).reshape(B, 2)
    out = []
    for s in range(B):
        mx, my = mu[s, 0] - shifts[s, 0], mu[s, 2] - shifts[s, 1]
        Ws = np.asarray(W.reshape(B, *W.shape[-2:])[s], dtype=dtype)  # (as the call uploads it)
        out.append(ref.image_cotangents(mx, my, cov[s, 0, 0], cov[s, 0, 2], cov[s, 2, 2], xs, ys, Ws))
    return out


@pytest.mark.parametrize("shape, shared", [((3,), False), ((2, 2), True)], ids=["3-own", "2x2-shared"])
@pytest.mark.parametrize("label", list(ref.KERNEL_SCREENS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_kernel_alone_against_the_restatement(lx, dtype, label, shape, shared):
    from lynx_amd import _ffi

    geometry = ref.KERNEL_SCREENS[label]
    vjp, screen, W, mis = kernel_case(lx, label, dtype, shape, shared)
    nx, ny = vjp.trace.image_at(0).shape[-2:]  # (taken, not computed: `arange` in float32 may give a pixel more)
    assert W.shape == (*shape, nx, ny)
    if label == LARGEST:  # at least three workgroups per sample, the last one partly filled (612 x 511, or a pixel more)
        assert nx * ny >= 3 * _ffi.IMAGE_GRAD_CELLS and (nx * ny) % _ffi.IMAGE_GRAD_CELLS
    else:
        assert (nx, ny) == tuple(int(n) for n in label.split("x")) if "x" in label else nx * ny == int(label)
    g = vjp(screen_images_bar={screen: W})
    B = int(np.prod(shape))
    g_mu, g_cov = np.asarray(g.mu).reshape(B, 7), np.asarray(g.cov).reshape(B, 7, 7)
    assert g_mu.dtype == g_cov.dtype == np.dtype(dtype)
    tol = TOL_IMAGE[np.float64] if dtype == np.float64 else FLOAT32_FACTOR * ref.FLOAT32_RESTATEMENT_DEVIATION[label]
    worst = 0.0
    for s, (entries, sizes) in enumerate(restated(vjp, geometry, dtype, W, mis, shape)):
        got = {"mu_x": g_mu[s, 0], "mu_y": g_mu[s, 2], "cov_xx": g_cov[s, 0, 0], "cov_yy": g_cov[s, 2, 2], "cov_xy": g_cov[s, 0, 2]}
        for name in ref.ENTRIES:
            distance = abs(float(got[name]) - entries[name]) / sizes[name]
            worst = max(worst, distance)
            print(f"{label} {np.dtype(dtype).name} sample {s} {name}: {float(got[name]):.9e} ref {entries[name]:.9e} distance {distance:.2e} of the size")
        for name in ref.ENTRIES:
            assert abs(float(got[name]) - entries[name]) <= tol * sizes[name], (s, name, got[name], entries[name], sizes[name])
            assert entries[name] != 0
    print(f"{label} {np.dtype(dtype).name}: worst {worst:.2e}, tolerance {tol:.2e}")
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
    if shared:
        want = per_sample.astype(np.float64).sum(axis=0)
        assert np.all(np.abs(shift_bar - want) <= (1e-14 if dtype == np.float64 else 1e-6) * np.abs(per_sample).sum(axis=0))
    else:
        assert np.array_equal(shift_bar.reshape(B, 2), per_sample)
    for el in vjp.leaves[1:]:  # the drift behind the screen: nothing reaches it
        assert np.all(g[el]["length"] == 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_screen_of_65_chunks_against_the_restatement(lx, monkeypatch, dtype):
    """`ref.SCREEN_OF_65_CHUNKS` through the test above, a batch of 2: 64 lanes of the finishing kernel add one chunk each and
    lane 0 a second one.  The float32 bound is that of 612 x 511."""
    from lynx_amd import _ffi

    label = "3x43691"
    assert -(-3 * 43691 // _ffi.IMAGE_GRAD_CELLS) == 65
    monkeypatch.setitem(ref.KERNEL_SCREENS, label, ref.SCREEN_OF_65_CHUNKS)
    monkeypatch.setitem(ref.FLOAT32_RESTATEMENT_DEVIATION, label, ref.FLOAT32_RESTATEMENT_DEVIATION[LARGEST])
    test_the_kernel_alone_against_the_restatement(lx, dtype, label, (2,), False)


# ---------------------------------------------------------------------------------------------
# 5. the same call twice
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_same_call_twice_returns_the_same_bits(lx, dtype):
    shape = (3,)
    geometry = ref.KERNEL_SCREENS[LARGEST]
    k1 = np.linspace(-2.0, 3.0, 3).astype(dtype)
    full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    quad, corrector = lx.Quadrupole(full(0.2), k1=k1, dtype=dtype), lx.HorizontalCorrector(full(0.1), angle=full(3e-5), dtype=dtype)
    screen = make_screen(lx, geometry, np.array([1e-4, -2e-4]), dtype, "SCREEN")
    elements = [lx.Drift(full(0.6), dtype=dtype), quad, corrector, lx.Drift(full(0.8), dtype=dtype), screen]
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-4), mu_y=full(-1e-4), sigma_x=full(1.2e-3), sigma_xp=full(1e-4), sigma_y=full(1e-3),
                                            sigma_yp=full(1e-4), sigma_s=full(1e-5), sigma_p=full(1e-3), energy=full(1e8), dtype=dtype)
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, screens=True)
    image = vjp.trace.image_at("SCREEN")
    assert image.shape[-2] * image.shape[-1] >= 3 * lx._ffi.IMAGE_GRAD_CELLS
    W = image.astype(np.float64) - np.roll(image.astype(np.float64), 7, axis=-2) * 1.1
    first, second = vjp(screen_images_bar={"SCREEN": W}, sigma_x=1e3), vjp(screen_images_bar={"SCREEN": W}, sigma_x=1e3)
    assert np.array_equal(first.mu, second.mu) and np.array_equal(first.cov, second.cov) and np.array_equal(first.energy, second.energy)
    assert np.any(first.mu != 0) and np.all(np.isfinite(first.cov))
    for el in elements:
        for name, value in first[el].items():
            assert np.array_equal(value, second[el][name]), (el.name, name)
    assert np.all(first[quad]["k1"] != 0) and np.all(first[screen]["misalignment"] != 0)


# ---------------------------------------------------------------------------------------------
# 6. end to end, float64
# ---------------------------------------------------------------------------------------------

B6 = 3
DESC_6 = lambda f, k1: [("drift", dict(length=f(0.6))), ("quadrupole", dict(length=f(0.2), k1=k1)), ("marker", {}),  # noqa: E731
                        ("hcor", dict(length=f(0.1), angle=f(3e-5))), ("drift", dict(length=f(0.8))), ("marker", {})]


def end_to_end_case(lx, dtype):
    """The two-screen lattice of tests/test_gpu_trace_screens.py, B = 3, a correlated incoming beam, and cotangents of both
    images (mismatch with a shifted, resized image), of mu and of cov at all seven points."""
    shape = (B6,)
    rng = np.random.default_rng(31)
    elements, a, b = two_screen_lattice(lx, shape, dtype)
    A = rng.normal(size=(B6, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]
    cov = np.zeros((B6, 7, 7))
    cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2) / 3
    mu = np.concatenate([rng.normal(size=(B6, 6)) * [2e-5, 2e-6, 2e-5, 2e-6, 1e-5, 1e-4], np.ones((B6, 1))], axis=-1)
    # (the float32 lattice's own numbers in both dtypes)
    mu, cov = mu.astype(np.float32).astype(np.float64), cov.astype(np.float32).astype(np.float64)
    energy = np.full(shape, 1e8)
    # (sized so that the moments' share of the k1 gradients is within a factor of 100 of the images': the test asserts it)
    w_mu = rng.normal(size=(B6, 7, 7)) * [1, 1, 1, 1, 1, 1, 0] * 1e14
    w_cov = np.zeros((B6, 7, 7, 7))
    w_cov[..., :6, :6] = rng.normal(size=(B6, 7, 6, 6)) * 1e18
    beam = lx.ParameterBeam(mu.astype(dtype), cov.astype(dtype), energy.astype(dtype), dtype=dtype)
    return elements, a, b, beam, mu, cov, energy, w_mu, w_cov


def image_weights(image, axis_shift):
    image = np.asarray(image, dtype=np.float64)
    return image - 1.2 * np.roll(image, axis_shift, axis=(-2, -1))


def test_end_to_end_against_central_differences_of_the_oracle_fp64(lx):
    dtype = np.float64
    elements, a, b, beam, mu, cov, energy, w_mu, w_cov = end_to_end_case(lx, dtype)
    f = lambda v: np.full((B6,), v)  # noqa: E731
    k1 = np.linspace(-4.0, 5.0, B6)
    desc = DESC_6(f, k1)
    _, specs = make_lattice(desc, dtype)
    vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, screens=True)
    assert vjp.trace.screens == [2, 5] and a.reading is vjp.trace.image_at("SCREEN_A") and b.reading is vjp.trace.image_at(5)
    W = {2: image_weights(vjp.trace.image_at(2), (2, -1)), 5: image_weights(vjp.trace.image_at(5), (-3, 2))}
    screens = {2: (np.asarray(mis_a((B6,)), dtype=dtype), SCREEN_A), 5: (np.asarray(MIS_B, dtype=dtype), SCREEN_B)}

    def terms(mu_, cov_, energy_):
        """Every term of the loss, (B, terms): the loss is their sum.  A central difference is taken term by term and summed
        then -- the loss is 1e15 and its derivative by the energy 0.03 per eV: the difference of two sums would be rounding."""
        beams = _chain(specs, o.parameter_beam(mu_, cov_, energy_, np.float64))
        out = []
        for k, at in enumerate(beams):
            out += [w_mu[:, k] * at["mu"], (w_cov[:, k] * at["cov"]).reshape(B6, 49)]
        for k, (mis, geometry) in screens.items():
            seen = np.array(beams[k]["mu"])
            seen[:, 0] -= np.broadcast_to(mis, (B6, 2))[:, 0]
            seen[:, 2] -= np.broadcast_to(mis, (B6, 2))[:, 1]
            out.append((W[k] * o.screen_reading_parameters(seen, beams[k]["cov"], **geometry, dtype=dtype)).reshape(B6, -1))
        return np.concatenate(out, axis=-1)

    def difference(up, down):
        return np.sum(up - down, axis=-1)

    g = vjp(screen_images_bar={"SCREEN_A": W[2], b: W[5]}, mu_bar=w_mu, cov_bar=w_cov)
    # the two parts are of one size: both count in what is compared
    parts = [vjp(screen_images_bar={2: W[2], 5: W[5]}), vjp(mu_bar=w_mu, cov_bar=w_cov)]
    ratio = np.abs(parts[0][elements[1]]["k1"]) / np.abs(parts[1][elements[1]]["k1"])
    print(f"k1 gradient, images / moments: {ratio}")
    assert np.all(ratio > 1e-2) and np.all(ratio < 1e2)

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = terms(mu, cov, energy)
        apply(x0 - h)
        down = terms(mu, cov, energy)
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
            reference = central(apply, arr[idx])[idx[0]]
            scale = max(abs(reference), 1e-9 * np.max(np.abs(w_cov)))
            assert abs(got[idx] - reference) <= 2e-4 * scale + 1e-7 * np.max(np.abs(got)), (e, name, idx, got[idx], reference)
            checked += 1
    assert checked == 18
    for s in range(B6):
        h = 1e-6 * energy[s]
        ep, em = energy.copy(), energy.copy()
        ep[s] += h
        em[s] -= h
        reference = difference(terms(mu, cov, ep), terms(mu, cov, em))[s] / (2 * h)
        assert abs(g.energy[s] - reference) <= 2e-4 * abs(reference) + 1e-12, (s, g.energy[s], reference)
        for c in range(6):
            h = 1e-9
            mp, mm = mu.copy(), mu.copy()
            mp[s, c] += h
            mm[s, c] -= h
            reference = difference(terms(mp, cov, energy), terms(mm, cov, energy))[s] / (2 * h)
            assert abs(g.mu[s, c] - reference) <= 1e-5 * abs(reference) + 1e-9 * np.max(np.abs(g.mu[s])), (s, c, g.mu[s, c], reference)
        # An off-diagonal entry moves together with its mirror image, and the sum of the two gradients is compared: an image
        # is a function of a SYMMETRIC covariance -- what one entry of an asymmetric one would do to it is a convention (the
        # oracle inverts the 2 x 2 block as it stands, the kernel splits the xy cotangent evenly), their sum is not.
        for (r, c) in [(0, 0), (0, 1), (0, 2), (2, 2), (2, 3), (1, 3), (0, 3), (1, 2), (4, 5), (5, 5)]:
            h = 1e-14
            cp, cm = cov.copy(), cov.copy()
            for (i, j) in {(r, c), (c, r)}:
                cp[s, i, j] += h
                cm[s, i, j] -= h
            reference = difference(terms(mu, cp, energy), terms(mu, cm, energy))[s] / (2 * h)
            got = g.cov[s, r, c] + (g.cov[s, c, r] if r != c else 0.0)
            assert abs(got - reference) <= 1e-4 * abs(reference) + 1e-7 * np.max(np.abs(g.cov[s])), (s, r, c, got, reference)
    # the misalignments: the image sees mu less the misalignment
    for k, screen in ((2, a), (5, b)):
        mis, _ = screens[k]
        got = g[screen]["misalignment"]
        assert got.shape == mis.shape
        for idx in np.ndindex(mis.shape):
            def apply(x, mis=mis, idx=idx):
                mis[idx] = x
            h = 1e-9
            apply(mis[idx] + h)
            up = terms(mu, cov, energy)
            apply(mis[idx] - 2 * h)
            down = terms(mu, cov, energy)
            apply(mis[idx] + h)
            reference = difference(up, down) / (2 * h)
            reference = reference[idx[0]] if mis.ndim == 2 else reference.sum()
            assert abs(got[idx] - reference) <= 1e-5 * abs(reference) + 1e-9 * np.max(np.abs(got)), (k, idx, got[idx], reference)
    # a screen that is not named gets no cotangent: the same as zeros
    named, zeros = vjp(screen_images_bar={"SCREEN_A": W[2]}), vjp(screen_images_bar={"SCREEN_A": W[2], "SCREEN_B": 0.0})
    assert np.array_equal(named.mu, zeros.mu) and np.array_equal(named.cov, zeros.cov) and np.array_equal(named.energy, zeros.energy)
    for el in elements:
        for name, value in named[el].items():
            assert np.array_equal(value, zeros[el][name])
    assert np.all(named[b]["misalignment"] == 0) and np.all(named[a]["misalignment"] != 0)
    # images only + moments only = the combined call
    for el, name in ((elements[0], "length"), (elements[1], "k1"), (elements[3], "angle"), (elements[4], "length")):
        total = parts[0][el][name] + parts[1][el][name]
        scale = np.maximum(np.abs(parts[0][el][name]), np.abs(parts[1][el][name]))
        assert np.all(np.abs(g[el][name] - total) <= 1e-12 * scale), (name, g[el][name], total)
    for whole, halves in ((g.mu, parts[0].mu + parts[1].mu), (g.cov, parts[0].cov + parts[1].cov), (g.energy, parts[0].energy + parts[1].energy)):
        assert np.all(np.abs(whole - halves) <= 1e-12 * np.max(np.abs(whole)))


# ---------------------------------------------------------------------------------------------
# 7. position and neighbours of a screen
# ---------------------------------------------------------------------------------------------


def explicit_cotangents(vjp, k, geometry, mis, W, dtype):
    """The restatement's mu_bar, cov_bar of the screen at point k as `mu_bar=`, `cov_bar=` of the whole trace."""
    trace = vjp.trace
    B, P = trace._mu.shape[0], trace.num_points
    xs, ys = ref.pixel_grid(**geometry, dtype=dtype)
    mu_bar, cov_bar = np.zeros((B, P, 7)), np.zeros((B, P, 7, 7))
    shifts = np.broadcast_to(np.asarray(mis, dtype=dtype), (B, 2))
    for s in range(B):
        m, c = trace._mu[s, k], trace._cov[s, k]
        entries, _ = ref.image_cotangents(m[0] - shifts[s, 0], m[2] - shifts[s, 1], c[0, 0], c[0, 2], c[2, 2], xs, ys, W[s])
        mu_bar[s, k], cov_bar[s, k] = ref.moment_cotangents(entries)
    return mu_bar, cov_bar


def front(lx, shape, dtype):
    full = lambda v: np.full(shape, v, dtype=dtype)  # noqa: E731
    quad = lx.Quadrupole(full(0.2), k1=np.linspace(-3.0, 4.0, int(np.prod(shape))).reshape(shape).astype(dtype), dtype=dtype, name="Q")
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-5), mu_y=full(-1e-5), sigma_x=full(1e-4), sigma_xp=full(1e-5), sigma_y=full(1e-4),
                                            sigma_yp=full(1e-5), sigma_s=full(1e-5), sigma_p=full(1e-3), energy=full(1e8), dtype=dtype)
    return [lx.Drift(full(0.6), dtype=dtype), quad, lx.Drift(full(0.5), dtype=dtype)], quad, beam


def assert_k1_as_explicit(lx, segment, quad, beam, bars, dtype=np.float64):
    """`bars`: {screen name: (geometry, misalignment, roll)}; the image call against the call with explicit moment cotangents."""
    vjp = lx.grad.track_along_vjp(segment, beam, screens=True)
    W = {name: image_weights(vjp.trace.image_at(name), roll) for name, (_, _, roll) in bars.items()}
    g = vjp(screen_images_bar=W)
    mu_bar, cov_bar = 0.0, 0.0
    for name, (geometry, mis, _) in bars.items():
        mb, cb = explicit_cotangents(vjp, vjp.trace.names.index(name), geometry, mis, W[name], dtype)
        mu_bar, cov_bar = mu_bar + mb, cov_bar + cb
    explicit = vjp(mu_bar=mu_bar, cov_bar=cov_bar)
    got, want = g[quad]["k1"], explicit[quad]["k1"]
    print(f"k1 gradients {got} explicit {want}")
    assert np.all(want != 0) and np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    return vjp, g


def test_a_screen_as_the_last_element(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    last = make_screen(lx, SCREEN_B, MIS_B, np.float64, "LAST")
    vjp, g = assert_k1_as_explicit(lx, lx.Segment(elements + [last]), quad, beam, {"LAST": (SCREEN_B, MIS_B, (2, 1))})
    assert vjp.trace.screens == [3] and vjp.trace.num_points == 5


def test_two_screens_directly_after_each_other(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    one, two = make_screen(lx, SCREEN_A, mis_a(shape), np.float64, "ONE"), make_screen(lx, SCREEN_B, MIS_B, np.float64, "TWO")
    segment = lx.Segment(elements + [one, two, lx.Drift(np.full(shape, 0.3), dtype=np.float64)])
    vjp, g = assert_k1_as_explicit(lx, segment, quad, beam, {"ONE": (SCREEN_A, mis_a(shape), (1, -1)), "TWO": (SCREEN_B, MIS_B, (2, 1))})
    assert vjp.trace.screens == [3, 4]
    assert np.all(g[one]["misalignment"] != 0) and np.all(g[two]["misalignment"] != 0)


def test_a_screen_inside_a_nested_segment(lx):
    shape = (3,)
    elements, quad, beam = front(lx, shape, np.float64)
    inner = make_screen(lx, SCREEN_B, MIS_B, np.float64, "INNER")
    segment = lx.Segment([elements[0], lx.Segment([elements[1], lx.Segment([elements[2], inner])]), lx.Drift(np.full(shape, 0.3), dtype=np.float64)])
    vjp, g = assert_k1_as_explicit(lx, segment, quad, beam, {"INNER": (SCREEN_B, MIS_B, (2, 1))})
    assert vjp.trace.screens == [3] and inner in g


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_losses_with_an_active_aperture_change_no_bit(lx, dtype):
    shape = (3,)
    elements, quad, beam = front(lx, shape, dtype)
    aperture = lx.Aperture(x_max=np.asarray([5e-5], dtype=dtype), y_max=np.asarray([5e-5], dtype=dtype), is_active=True, name="AP", dtype=dtype)
    screen = make_screen(lx, SCREEN_B, MIS_B, dtype, "SCREEN")
    segment = lx.Segment([elements[0], aperture, elements[1], elements[2], screen])
    with pytest.raises(NotImplementedError, match="AP"):
        lx.grad.track_along_vjp(segment, beam, screens=True)
    collimated = lx.grad.track_along_vjp(segment, beam, losses=True, screens=True)
    W = image_weights(collimated.trace.image_at("SCREEN"), (2, 1))
    with_losses = collimated(screen_images_bar={"SCREEN": W}, sigma_y=1e10)
    assert aperture not in with_losses  # (a ParameterBeam: the plain problem)
    aperture.is_active = False
    free = lx.grad.track_along_vjp(segment, beam, screens=True)
    assert np.array_equal(free.trace.image_at("SCREEN"), collimated.trace.image_at("SCREEN"))
    plain = free(screen_images_bar={"SCREEN": W}, sigma_y=1e10)
    assert np.array_equal(plain.mu, with_losses.mu) and np.array_equal(plain.cov, with_losses.cov) and np.array_equal(plain.energy, with_losses.energy)
    for el in (elements[0], quad, elements[2]):
        for name, value in plain[el].items():
            assert np.array_equal(value, with_losses[el][name]), (el.name, name)
    assert np.array_equal(plain[screen]["misalignment"], with_losses[screen]["misalignment"]) and np.all(plain[quad]["k1"] != 0)


# ---------------------------------------------------------------------------------------------
# 8. float32 end to end
# ---------------------------------------------------------------------------------------------

# Distance max |g - r| / max |r| of the float32 gradient g from the float64 `track_along_vjp(..., screens=True)` r of the same
# input (the lattice and cotangents of test 6), per kind of parameter, relative to the largest gradient of that kind: twice
# what test_float32_against_the_float64_pass measured on MI355X.  Never above 5e-3 (the largest entry of `TOL_TRACE_GRAD` of
# tests/test_gpu_trace_grad.py, a 128-element lattice, is 1.8e-2): more on a four-magnet lattice means something is wrong.
#     measured:  k1 8.0e-6, length 8.2e-6, angle 2.4e-6, energy 4.1e-7, mu 4.7e-6, cov 2.3e-6, misalignment 2.8e-6
# (a ParameterBeam's float32 trace of six elements, float64 sums in the image kernel: float32 rounding and little more)
TOL_SCREEN_GRAD = {"k1": 1.6e-5, "length": 1.7e-5, "angle": 4.8e-6, "energy": 8.2e-7, "mu": 9.4e-6, "cov": 4.6e-6, "misalignment": 5.7e-6}
assert max(TOL_SCREEN_GRAD.values()) <= 5e-3


def test_float32_against_the_float64_pass(lx):
    def gradients(dtype):
        elements, a, b, beam, mu, cov, energy, w_mu, w_cov = end_to_end_case(lx, dtype)
        vjp = lx.grad.track_along_vjp(lx.Segment(elements), beam, screens=True)
        images = {k: np.asarray(vjp.trace.image_at(k), dtype=np.float64) for k in (2, 5)}
        return elements, a, b, vjp, images, w_mu, w_cov

    # the float64 pass makes the cotangents; both passes take the same ones
    elements64, a64, b64, vjp64, images64, w_mu, w_cov = gradients(np.float64)
    W = {2: image_weights(images64[2], (2, -1)), 5: image_weights(images64[5], (-3, 2))}
    elements32, a32, b32, vjp32, images32, _, _ = gradients(np.float32)
    for k in (2, 5):
        assert np.max(np.abs(images32[k] - images64[k])) <= 2e-4 * images64[k].max()  # (`TOL_IMAGE` of float32)

    def collect(vjp, elements, a, b):
        g = vjp(screen_images_bar={2: W[2], 5: W[5]}, mu_bar=w_mu, cov_bar=w_cov)
        f64 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
        return {"k1": f64(g[elements[1]]["k1"]), "length": np.stack([f64(g[elements[e]]["length"]) for e in (0, 1, 3, 4)]),
                "angle": f64(g[elements[3]]["angle"]), "energy": f64(g.energy), "mu": f64(g.mu)[..., :6], "cov": f64(g.cov)[..., :6, :6],
                "misalignment": np.concatenate([f64(g[a]["misalignment"]).reshape(-1), f64(g[b]["misalignment"]).reshape(-1)])}

    g32, g64 = collect(vjp32, elements32, a32, b32), collect(vjp64, elements64, a64, b64)
    measured = {}
    for name, want in g64.items():
        got = g32[name]
        assert got.shape == want.shape and np.all(np.isfinite(got)), name
        measured[name] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("float32 track_along_vjp(screens=True) against float64: " + ", ".join(f"{k} {v:.2e}" for k, v in measured.items()))
    for name, value in measured.items():
        assert value <= TOL_SCREEN_GRAD[name], (name, value)


# ---------------------------------------------------------------------------------------------
# 9. the example
# ---------------------------------------------------------------------------------------------


def test_match_screen_image_example_converges(lx):
    """examples/match_screen_image.py: Adam on two quadrupoles and a corrector until the image on a 60 x 40 screen is the target."""
    spec = importlib.util.spec_from_file_location(
        "match_screen_image", pathlib.Path(__file__).resolve().parents[1] / "examples" / "match_screen_image.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.screen_line(), example.incoming_beam()
    target = example.target_image(segment, beam)
    assert target.shape[0] == 1 and target.size < 3000 and target.max() > 0
    history = example.tune(segment, beam, target)
    print(f"loss {history[0]:.3e} -> {history[-1]:.3e}")
    assert history[-1] <= history[0] / 100, (history[0], history[-1])
