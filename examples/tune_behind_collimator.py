"""
Tuning the COLLIMATED beam: Adam on two quadrupoles until `sigma_x` and `sigma_y` of the beam that survives a collimator
have given values at a marker behind it.  The collimator removes about 40 % of the particles, and which ones depends on
the quadrupoles in front of it; the loss is written in the moments of the survivors, so its gradient comes from
`lynx_amd.grad.track_along_vjp(..., losses=True)`: the set of survivors is held fixed (it is locally constant in the
strengths -- the transmission is a step function and has no gradient), the moments over it are smooth.  Every iteration
makes a new forward trace, and with it a new set (the optimiser is written out in NumPy, as in gradient_based_tuning.py).

    python examples/tune_behind_collimator.py          # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

QUADRUPOLES = ("Q1", "Q2")
# sigma_x, sigma_y in metres of the collimated beam at SCREEN: near what k1 = (3, -3.5) gives a beam that comes in with
# beta_x = beta_y = 5 m, alpha = 0 and 1 nm rad -- so the two quadrupoles can reach both values
TARGET = (4.5e-5, 3.3e-5)


def collimated_line():
    return lx.Segment([
        lx.Quadrupole(f(0.2), k1=f(1.5), name="Q1"), lx.Drift(f(0.5)),
        lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q2"), lx.Drift(f(0.5)),
        lx.Aperture(x_max=f(8e-5), y_max=f(8e-5), shape="rectangular", is_active=True, name="COLLIMATOR"),
        lx.Drift(f(1.0)), lx.Marker(name="SCREEN"),
    ])


def incoming_beam(num_particles=20_000):
    """Emittance 1 nm rad in both planes, beta = 5 m, alpha = 0."""
    return lx.ParticleBeam.from_parameters(num_particles=num_particles, sigma_x=f(7.0711e-5), sigma_xp=f(1.41421e-5),
                                           sigma_y=f(7.0711e-5), sigma_yp=f(1.41421e-5), sigma_s=f(8e-6), sigma_p=f(1e-3),
                                           energy=f(1e8), seed=0)


def tune(segment, beam, steps=100, lr=0.1, report=None):
    """
    Adam on the two strengths; returns the history of (loss, transmission, sigma_x, sigma_y) at SCREEN, the loss being
    half the summed squared relative distance of the two sizes from TARGET.
    """
    m, v, history = np.zeros(2), np.zeros(2), []
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam, losses=True)
        trace = vjp.trace
        k = trace.index_of("SCREEN")
        sizes = float(trace.sigma_x[0, k]), float(trace.sigma_y[0, k])
        residuals = [size / target - 1.0 for size, target in zip(sizes, TARGET)]
        history.append((0.5 * float(np.sum(np.square(residuals))), float(trace.transmission[0, k]), *sizes))
        if report is not None:
            report(t - 1, history[-1])
        bar_x, bar_y = np.zeros((1, trace.num_points)), np.zeros((1, trace.num_points))
        bar_x[0, k], bar_y[0, k] = residuals[0] / TARGET[0], residuals[1] / TARGET[1]  # d loss / d sigma at SCREEN
        g = vjp(sigma_x=bar_x, sigma_y=bar_y)
        gradient = np.array([float(g[getattr(segment, name)]["k1"][0]) for name in QUADRUPOLES])
        m = 0.9 * m + 0.1 * gradient
        v = 0.999 * v + 0.001 * gradient**2
        update = lr * (m / (1 - 0.9**t)) / (np.sqrt(v / (1 - 0.999**t)) + 1e-12)
        for name, delta in zip(QUADRUPOLES, update):
            quadrupole = getattr(segment, name)
            quadrupole.k1 = (quadrupole.k1 - delta).astype(np.float32)
    return history


if __name__ == "__main__":
    segment, beam = collimated_line(), incoming_beam(100_000)

    def show(t, row):
        loss, transmission, sigma_x, sigma_y = row
        print(f"step {t:3d}  loss {loss:.4g}  transmission {transmission:.4f}  sigma_x {sigma_x:.4g}  sigma_y {sigma_y:.4g}")

    history = tune(segment, beam, report=show)
    print(f"loss {history[0][0]:.4g} -> {history[-1][0]:.4g} after {len(history)} Adam steps; targets {TARGET}")
    for name in QUADRUPOLES:
        print(f"  {name}.k1 = {float(getattr(segment, name).k1[0]):+.5g}")
