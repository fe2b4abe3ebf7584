"""
Matching a screen image: Adam on two quadrupoles and a horizontal corrector until the image of a `ParameterBeam` on a screen
is a given target image -- the ARES tuning task, written as "make this picture look like that one".  The loss is the
mean squared difference of the two images, so its cotangent is an image, and `lynx_amd.grad.track_along_vjp(...,
screens=True)` takes it as it is: the forward pass makes the image inside the trace, one reverse call reduces the image
cotangent over all pixels on the device and sweeps it back to the magnets (the optimiser is written out in NumPy, as in
match_twiss_along_lattice.py).  The target is made by the same lattice at other settings.

    python examples/match_screen_image.py          # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

KNOBS = (("Q1", "k1", 1.0), ("Q2", "k1", 1.0), ("HCOR", "angle", 1e-4))  # element, parameter, the unit Adam steps in
TARGET_SETTINGS = {"Q1": 4.0, "Q2": -3.5, "HCOR": 1.5e-4}


def screen_line(resolution=(60, 40), pixel_size=(5e-5, 5e-5)):
    return lx.Segment([
        lx.Quadrupole(f(0.2), k1=f(2.0), name="Q1"), lx.Drift(f(0.4)),
        lx.Quadrupole(f(0.2), k1=f(-2.0), name="Q2"), lx.Drift(f(0.3)),
        lx.HorizontalCorrector(f(0.1), angle=f(0.0), name="HCOR"), lx.Drift(f(1.0)),
        lx.Screen(resolution=resolution, pixel_size=pixel_size, is_active=True, name="SCREEN"),
    ])


def incoming_beam():
    """Emittance 4 nm rad in both planes, beta = 10 m, alpha = 0."""
    return lx.ParameterBeam.from_parameters(sigma_x=f(2e-4), sigma_xp=f(2e-5), sigma_y=f(2e-4), sigma_yp=f(2e-5), sigma_s=f(8e-6),
                                            sigma_p=f(1e-3), energy=f(1e8))


def settings(segment):
    return {name: float(getattr(getattr(segment, name), parameter)[0]) for name, parameter, _ in KNOBS}


def apply(segment, values):
    for name, parameter, _ in KNOBS:
        setattr(getattr(segment, name), parameter, f(values[name]))


def target_image(segment, beam):
    """The image at TARGET_SETTINGS; the lattice comes back at the settings it had."""
    before = settings(segment)
    apply(segment, TARGET_SETTINGS)
    image = np.array(segment.track_along(beam, screens=True).image_at("SCREEN"), dtype=np.float64)
    apply(segment, before)
    return image


def tune(segment, beam, target, steps=200, lr=0.05):
    """Adam on the three knobs; returns the loss history (loss = mean squared image difference, in units of the target's peak)."""
    m, v, history = np.zeros(3), np.zeros(3), []
    peak = target.max()
    units = np.array([unit for _, _, unit in KNOBS])
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam, screens=True)
        residual = (np.asarray(vjp.trace.image_at("SCREEN"), dtype=np.float64) - target) / peak
        history.append(float(np.mean(np.square(residual))))
        g = vjp(screen_images_bar={"SCREEN": 2.0 * residual / (residual.size * peak)})  # d loss / d image
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
