"""
The adjoint of a ParameterBeam's screen image, restated in numpy -- the reference of the tests of
`track_along_vjp(..., screens=True)` (lynx_gaussian_images_along_backward).

The image of one sample on one screen is the bivariate-normal density I of (mx, my) = (mu_x - misalignment_x, mu_y -
misalignment_y) and a, b, c = cov_xx, cov_xy, cov_yy on the pixel grid xs, ys, stored flipped in x (row nx - 1 - i).  With W
the cotangent of the image in that layout, det = a c - b^2, dx = xs[i] - mx, dy = ys[j] - my, ux = (c dx - b dy) / det and
uy = (a dy - b dx) / det, six sums over the pixels

    S0, Sx, Sy, Sxx, Sxy, Syy = sum W I {1, ux, uy, ux^2, ux uy, uy^2}

give the five entries

    mu_x: Sx, mu_y: Sy, cov_xx: (Sxx - c/det S0) / 2, cov_yy: (Syy - a/det S0) / 2, cov_xy: (Sxy + b/det S0) / 2

where cov_xy is what EACH of cov_bar[0][2] and cov_bar[2][0] gets: their sum is the derivative by the covariance b.

Every entry comes with its UNCANCELLED SIZE: the same expression with every pixel's term replaced by its absolute value
(for mu_x that is sum |W I ux|; for cov_xx it is (sum |W I ux^2| + |c/det| sum |W I|) / 2) -- what an error of a sum is
measured against, since the signed sums may cancel to anything.

`mode="float32"` evaluates the restatement with the forward kernel's float32 operations: the grid, mx, my, a, b, c and W in
float32, det, dx, dy, the Mahalanobis form and log p in float32, exp in double and rounded to float32 (the image the caller
saw), ux, uy and every product in float32, the sums in double, and the five entries formed in double from the sums.
"""

import numpy as np

ENTRIES = ("mu_x", "mu_y", "cov_xx", "cov_yy", "cov_xy")
ARES_BINNING_4 = dict(resolution=(2448, 2040), pixel_size=(3.3198e-6, 2.4469e-6), binning=4)  # 612 x 511 pixels


def pixel_grid(resolution, pixel_size, binning, dtype):
    """xs, ys as `Screen.reading` and `oracle.screen_reading_parameters` make them, in `dtype`."""
    dtype = np.dtype(dtype)
    resolution, pixel_size = np.asarray(resolution, dtype), np.asarray(pixel_size, dtype)
    half = resolution * pixel_size / 2
    step = pixel_size * np.asarray(binning, dtype)
    return np.arange(-half[0], half[0], step[0], dtype=dtype), np.arange(-half[1], half[1], step[1], dtype=dtype)


def density(mx, my, a, b, c, xs, ys, mode="float64"):
    """The image [nx][ny] of one sample, flipped in x, and the (unflipped) dx [nx][1], dy [1][ny] it was made from."""
    T = np.float32 if mode == "float32" else np.float64
    mx, my, a, b, c = (T(v) for v in (mx, my, a, b, c))
    xs, ys = np.asarray(xs, dtype=T), np.asarray(ys, dtype=T)
    det = a * c - b * b
    dx, dy = xs[:, None] - mx, ys[None, :] - my
    with np.errstate(all="ignore"):
        maha = (c * dx * dx - T(2) * b * dx * dy + a * dy * dy) / det
        logp = T(-0.5) * maha - T(1.8378770664093453) - T(0.5) * T(np.log(np.float64(det)))  # (the log rounded correctly)
        image = np.exp(logp.astype(np.float64)).astype(T)
    return image[::-1], dx, dy


def image_cotangents(mx, my, a, b, c, xs, ys, W, mode="float64"):
    """
    One sample, one screen; W [nx][ny] in the image's layout.  Returns (entries, sizes): two dicts over ENTRIES, float64 --
    `misalignment_bar` is (-entries["mu_x"], -entries["mu_y"]).
    """
    T = np.float32 if mode == "float32" else np.float64
    image, dx, dy = density(mx, my, a, b, c, xs, ys, mode)
    a, b, c = T(a), T(b), T(c)
    det = a * c - b * b
    W = np.asarray(W, dtype=T)[::-1]  # (back to the order of xs)
    wi = W * image[::-1]
    ux, uy = (c * dx - b * dy) / det, (a * dy - b * dx) / det
    terms = [wi, wi * ux, wi * uy, wi * ux * ux, wi * ux * uy, wi * uy * uy]
    assert all(t.dtype == T for t in terms)
    S0, Sx, Sy, Sxx, Sxy, Syy = (float(np.sum(t, dtype=np.float64)) for t in terms)
    A0, Ax, Ay, Axx, Axy, Ayy = (float(np.sum(np.abs(t), dtype=np.float64)) for t in terms)
    a, b, c = float(a), float(b), float(c)
    det = a * c - b * b
    entries = {"mu_x": Sx, "mu_y": Sy, "cov_xx": 0.5 * (Sxx - c / det * S0), "cov_yy": 0.5 * (Syy - a / det * S0),
               "cov_xy": 0.5 * (Sxy + b / det * S0)}
    sizes = {"mu_x": Ax, "mu_y": Ay, "cov_xx": 0.5 * (Axx + abs(c / det) * A0), "cov_yy": 0.5 * (Ayy + abs(a / det) * A0),
             "cov_xy": 0.5 * (Axy + abs(b / det) * A0)}
    return entries, sizes


def moment_cotangents(entries):
    """The five entries as mu_bar (7,) and cov_bar (7, 7) at the screen's point."""
    mu_bar, cov_bar = np.zeros(7), np.zeros((7, 7))
    mu_bar[0], mu_bar[2] = entries["mu_x"], entries["mu_y"]
    cov_bar[0, 0], cov_bar[2, 2] = entries["cov_xx"], entries["cov_yy"]
    cov_bar[0, 2] = cov_bar[2, 0] = entries["cov_xy"]
    return mu_bar, cov_bar


def beam_on(geometry, rho=0.5, scale=1.0, shift=(0.0, 0.0)):
    """
    mx, my, a, b, c of a correlated beam that the screen's extent cuts: sigma_x = 0.4, sigma_y = 0.5 of the half extents
    (times `scale`), correlation `rho`, centred at (0.1, -0.1) + `shift` of the half extents.
    """
    hx = geometry["resolution"][0] * geometry["pixel_size"][0] / 2
    hy = geometry["resolution"][1] * geometry["pixel_size"][1] / 2
    sx, sy = 0.4 * hx * scale, 0.5 * hy * scale
    return (0.1 + shift[0]) * hx, (-0.1 + shift[1]) * hy, sx * sx, rho * sx * sy, sy * sy


def mismatch_cotangent(geometry, dtype, mode="float64", sample=0):
    """
    The test input of one sample: (beam, xs, ys, W) with W = I - (the image of a shifted, resized beam of another
    correlation), the cotangent of half a squared image difference -- signed, so that the sums cancel.  `sample` varies
    the beam: a little larger, a little further out and less correlated with every sample.
    """
    xs, ys = pixel_grid(**geometry, dtype=dtype)
    beam = beam_on(geometry, rho=0.5 - 0.2 * sample, scale=1.0 + 0.1 * sample, shift=(0.05 * sample, -0.03 * sample))
    other = beam_on(geometry, rho=-0.2, scale=1.3, shift=(0.15, -0.2))
    W = density(*beam, xs, ys, mode)[0].astype(np.float64) - density(*other, xs, ys, mode)[0].astype(np.float64)
    return beam, xs, ys, W


# The screens the kernel is run on alone, by the number of cells of their images.  A pixel of 2^-16 m makes `arange` exact
# in both dtypes: the image has exactly `resolution` pixels.  One workgroup sums 2048 cells (`_ffi.IMAGE_GRAD_CELLS`), one
# wave 64 cells at a time: 1, 63 | 64 | 65, 255 | 256 | 257 cells sit on either side of a wave and of a round of the
# workgroup's 256 threads, 33 x 17 is odd in both directions, 1 x 257 and 257 x 1 have one row and one column, and
# 612 x 511 = 312 732 cells are 153 workgroups per sample, the last of them partly filled.
_PIXEL = 2.0 ** -16
KERNEL_SCREENS = {
    "1": dict(resolution=(1, 1), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "63": dict(resolution=(9, 7), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "64": dict(resolution=(8, 8), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "65": dict(resolution=(13, 5), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "255": dict(resolution=(17, 15), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "256": dict(resolution=(16, 16), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "257": dict(resolution=(257, 1), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "561": dict(resolution=(33, 17), pixel_size=(2e-5, 2.2e-5), binning=1),
    "1x257": dict(resolution=(1, 257), pixel_size=(_PIXEL, _PIXEL), binning=1),
    "257x1": dict(resolution=(514, 2), pixel_size=(_PIXEL, _PIXEL), binning=2),
    "612x511": ARES_BINNING_4,
}

# A screen of exactly 65 workgroups, 3 x 43 691 = 64 x 2048 + 1 = 131 073 cells: the finishing kernels' lane l adds the chunks
# l, l + 64, ..., so here lane 0 alone makes a second trip.  It is run apart from KERNEL_SCREENS, a batch of 2 once per dtype,
# under the float32 bounds of 612 x 511 (the large screen next to it); tests/test_trace_screens_grad_host.py and
# tests/test_trace_image_loss_host.py check that the float32 restatement itself stays inside them on this screen.
SCREEN_OF_65_CHUNKS = dict(resolution=(3, 43691), pixel_size=(_PIXEL, _PIXEL), binning=1)

# What tests/test_trace_screens_grad_host.py measures and asserts for the float32 restatement against the float64 one on
# the float32 inputs: the worst entry relative to its uncancelled size, over samples 0 .. 3 of `mismatch_cotangent`, per
# screen ("A", "B": the two screens of tests/test_gpu_trace_screens.py).  Measured (numpy; log det rounded correctly):
#   1: 1.88e-6, 63: 8.34e-7, 64: 5.35e-7, 65: 4.20e-7, 255: 5.51e-7, 256: 5.26e-7, 257: 8.34e-7, 561: 7.07e-7,
#   1x257: 9.99e-7, 257x1: 8.31e-7, 612x511: 2.22e-7, A: 3.60e-7, B: 7.07e-7
# -- mostly the rounding of log p, which is about 17 (an ulp of 1.9e-6) and common to a whole image; the pixels' own errors
# average out on the large images.  Asserted: the measured value and a margin of a quarter.
FLOAT32_RESTATEMENT_DEVIATION = {
    "1": 2.35e-6, "63": 1.05e-6, "64": 6.7e-7, "65": 5.3e-7, "255": 6.9e-7, "256": 6.6e-7, "257": 1.05e-6, "561": 8.9e-7,
    "1x257": 1.25e-6, "257x1": 1.04e-6, "612x511": 2.8e-7, "A": 4.5e-7, "B": 8.9e-7,
}
