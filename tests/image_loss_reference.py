"""
The mean squared difference of a ParameterBeam's screen image to a target image and its adjoint, restated in numpy -- the
reference of the tests of `track_along_vjp(..., image_targets=)` (lynx_gaussian_images_along_mse and its reverse half).

For one sample and one screen of n = nx ny pixels, with I the image of tests/screen_grad_reference.py (`density`) and T the
target in the image's layout,

    loss = mean (I - T)^2,      W = d loss / d I = 2 (I - T) / n,

and the five entries are those of `screen_grad_reference.image_cotangents` for that W.

Every value comes with its UNCANCELLED SIZE FOR THIS LOSS: the same sums with |I - T| replaced by |I| + |T| and every pixel's
term by its absolute value; for the loss that is mean (|I| + |T|)^2.  Near a match I - T cancels, and the rounding error of a
float32 I does not shrink with it: the error of an entry is of the order of eps sum |I| |I u|, whatever is left of the
difference, so an error measured against sum |W I u| would grow without bound as the loss goes to zero.

`mode="float32"` evaluates I, and the products of `image_cotangents`, with the forward kernel's float32 operations; I - T, W
and the loss are formed in float64 from the float32 I and T, as the kernel forms them.
"""

import numpy as np

from . import screen_grad_reference as ref


def image_loss(mx, my, a, b, c, xs, ys, target, mode="float64"):
    """
    One sample, one screen; `target` [nx][ny] in the image's layout.  Returns (loss, entries, loss_size, sizes): the loss and
    its size as floats, `entries` and `sizes` dicts over `ref.ENTRIES`, all float64 -- the gradient with respect to the
    screen's misalignment is (-entries["mu_x"], -entries["mu_y"]).
    """
    image = ref.density(mx, my, a, b, c, xs, ys, mode)[0].astype(np.float64)
    target = np.asarray(target, dtype=np.float64)
    assert image.shape == target.shape, (image.shape, target.shape)
    n = image.size
    residual = image - target
    whole = np.abs(image) + np.abs(target)
    entries, _ = ref.image_cotangents(mx, my, a, b, c, xs, ys, 2.0 * residual / n, mode)
    _, sizes = ref.image_cotangents(mx, my, a, b, c, xs, ys, 2.0 * whole / n, mode)
    return float(np.mean(np.square(residual))), entries, float(np.mean(np.square(whole))), sizes


def mismatch_target(geometry, dtype, mode="float64", sample=0):
    """The beam of `ref.mismatch_cotangent` and the image of its `other` beam as the target: (beam, xs, ys, target in `dtype`)."""
    xs, ys = ref.pixel_grid(**geometry, dtype=dtype)
    beam = ref.beam_on(geometry, rho=0.5 - 0.2 * sample, scale=1.0 + 0.1 * sample, shift=(0.05 * sample, -0.03 * sample))
    other = ref.beam_on(geometry, rho=-0.2, scale=1.3, shift=(0.15, -0.2))
    return beam, xs, ys, ref.density(*other, xs, ys, mode)[0].astype(dtype)


# The screens the kernels are run on alone: those of `ref.KERNEL_SCREENS` and 89 x 71 = 6319 cells, three full workgroups of
# 2048 cells and a partly filled fourth.
LOSS_SCREENS = dict(ref.KERNEL_SCREENS, **{"89x71": dict(resolution=(89, 71), pixel_size=(2.0 ** -16, 2.0 ** -16), binning=1)})

# What tests/test_trace_image_loss_host.py measures and asserts for the float32 restatement against the float64 one on the
# float32 inputs, over samples 0 .. 3 of `mismatch_target`, per screen of `LOSS_SCREENS`: the worst entry and the loss,
# each relative to its uncancelled size for this loss.  Measured (numpy; log det rounded correctly):
#   entries  1: 1.95e-6, 63: 2.46e-7, 64: 1.61e-7, 65: 2.22e-7, 255: 3.32e-7, 256: 3.04e-7, 257: 3.21e-7, 561: 1.86e-7,
#            1x257: 4.92e-7, 257x1: 2.78e-7, 612x511: 6.76e-8, 89x71: 3.36e-7
#   loss     1: 9.13e-7, 63: 9.87e-8, 64: 9.92e-8, 65: 1.80e-7, 255: 2.76e-7, 256: 2.60e-7, 257: 6.25e-8, 561: 1.48e-7,
#            1x257: 3.01e-8, 257x1: 8.39e-8, 612x511: 3.56e-8, 89x71: 2.92e-7
# -- as in `ref.FLOAT32_RESTATEMENT_DEVIATION` mostly the rounding of log p, common to a whole image, here against a size that
# holds the target as well; it averages out on the large images.
# Asserted: the measured value and a margin of a quarter.
FLOAT32_ENTRY_DEVIATION = {
    "1": 2.44e-6, "63": 3.08e-7, "64": 2.01e-7, "65": 2.77e-7, "255": 4.14e-7, "256": 3.8e-7, "257": 4.01e-7, "561": 2.33e-7,
    "1x257": 6.16e-7, "257x1": 3.48e-7, "612x511": 8.45e-8, "89x71": 4.2e-7,
}
FLOAT32_LOSS_DEVIATION = {
    "1": 1.14e-6, "63": 1.23e-7, "64": 1.24e-7, "65": 2.25e-7, "255": 3.45e-7, "256": 3.25e-7, "257": 7.81e-8, "561": 1.84e-7,
    "1x257": 3.76e-8, "257x1": 1.05e-7, "612x511": 4.45e-8, "89x71": 3.65e-7,
}
