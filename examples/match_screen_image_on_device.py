"""
Matching a screen image without moving a pixel: the tuning of match_screen_image.py -- Adam on two quadrupoles and a
horizontal corrector until the image of a `ParameterBeam` on a screen is a given target image -- with the loss evaluated on
the device.  The target is uploaded once (`lynx_amd.grad.ImageTargets`) and stays there; every step is
`track_along_vjp(..., image_targets=targets)`, whose forward pass makes no image: one kernel forms the density per pixel, the
mean squared difference to the target and the six sums its gradient needs, and `vjp(image_loss_bar=...)` scales those sums and
sweeps them back to the magnets.  Per step a handful of numbers cross to the host -- the loss and the three gradients --
where match_screen_image.py reads an image back and uploads its cotangent.

    python examples/match_screen_image_on_device.py          # needs an MI355X and the built library
"""

import importlib.util
import pathlib

import numpy as np

import lynx_amd.grad as grad

# (the lattice, the beam, the knobs and the target of the example this one is a variant of)
_spec = importlib.util.spec_from_file_location("match_screen_image", pathlib.Path(__file__).with_name("match_screen_image.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
KNOBS, TARGET_SETTINGS = base.KNOBS, base.TARGET_SETTINGS
screen_line, incoming_beam, settings, apply, target_image = base.screen_line, base.incoming_beam, base.settings, base.apply, base.target_image


def tune(segment, beam, target, steps=200, lr=0.05):
    """Adam on the three knobs; returns the loss history (loss = mean squared image difference, in units of the target's peak)."""
    m, v, history = np.zeros(3), np.zeros(3), []
    peak = target.max()
    units = np.array([unit for _, _, unit in KNOBS])
    targets = grad.ImageTargets({"SCREEN": target})  # uploaded by the first pass, device-resident from then on
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam, image_targets=targets)
        history.append(float(vjp.image_loss_of("SCREEN")[0]) / peak**2)
        g = vjp(image_loss_bar=1.0 / peak**2)  # d (loss in units of the peak) / d (mean squared difference)
        gradient = np.array([float(g[getattr(segment, name)][parameter][0]) for name, parameter, _ in KNOBS]) * units
        m = 0.9 * m + 0.1 * gradient
        v = 0.999 * v + 0.001 * gradient**2
        update = lr * (m / (1 - 0.9**t)) / (np.sqrt(v / (1 - 0.999**t)) + 1e-30)
        now = settings(segment)
        apply(segment, {name: now[name] - delta * unit for (name, _, unit), delta in zip(KNOBS, update)})
    return history


if __name__ == "__main__":
    segment, beam = screen_line(), incoming_beam()
    target = target_image(segment, beam)
    history = tune(segment, beam, target)
    for t in range(0, len(history), 20):
        print(f"step {t:3d}  loss {history[t]:.4g}")
    print(f"loss {history[0]:.4g} -> {history[-1]:.4g} after {len(history)} Adam steps")
    for name, value in settings(segment).items():
        print(f"  {name} = {value:+.5g} (target {TARGET_SETTINGS[name]:+.5g})")
