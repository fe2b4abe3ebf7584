"""
Matching beam sizes AROUND an accelerating cavity: Adam on two quadrupoles, one in front of and one behind the cavity,
until `sigma_x` and `sigma_y` of a ParticleBeam at two markers -- M1 in front of the cavity, M2 behind it -- have given
values.  Behind the cavity's kick the moments of the particles are not a function of the moments in front of it, so the
gradient takes a second pass over the particles: `lynx_amd.grad.track_along_vjp(..., cavities=True)`, one call for the
cotangents at both markers (the optimiser is written out in NumPy, as in gradient_based_tuning.py).

    python examples/match_beam_size_behind_cavity.py      # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

QUADRUPOLES = ("Q1", "Q2")
# (sigma_x, sigma_y) in metres at each marker: what k1 = (2.5, -3.0) gives the beam of `incoming_beam` -- so the two
# quadrupoles can reach all four values
TARGETS = {"M1": (1.36572e-4, 2.74274e-4), "M2": (2.24569e-4, 1.18335e-4)}


def accelerating_line():
    return lx.Segment([
        lx.Quadrupole(f(0.2), k1=f(0.5), name="Q1"), lx.Drift(f(0.6)), lx.Marker(name="M1"),
        lx.Cavity(f(1.0377), voltage=f(2e7), phase=f(0.0), frequency=f(1.3e9), name="ACC"), lx.Drift(f(0.4)),
        lx.Quadrupole(f(0.2), k1=f(-0.5), name="Q2"), lx.Drift(f(1.2)), lx.Marker(name="M2"),
    ])


def incoming_beam(num_particles=20_000):
    """20 MeV, 0.2 mm and 50 urad in both planes: the cavity doubles the energy."""
    return lx.ParticleBeam.from_parameters(num_particles=num_particles, sigma_x=f(2e-4), sigma_xp=f(5e-5), sigma_y=f(2e-4),
                                           sigma_yp=f(5e-5), sigma_s=f(8e-6), sigma_p=f(1e-3), energy=f(2e7), seed=0)


def tune(segment, beam, steps=150, lr=0.1):
    """Adam on the two strengths; returns the loss history (loss = mean squared relative distance from the targets)."""
    m, v, history = np.zeros(2), np.zeros(2), []
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam, cavities=True)
        trace = vjp.trace
        bar_x, bar_y = np.zeros((1, trace.num_points)), np.zeros((1, trace.num_points))
        residuals = []
        for marker, (sigma_x, sigma_y) in TARGETS.items():
            k = trace.index_of(marker)
            rx, ry = float(trace.sigma_x[0, k]) / sigma_x - 1.0, float(trace.sigma_y[0, k]) / sigma_y - 1.0
            residuals += [rx, ry]
            bar_x[0, k], bar_y[0, k] = 2.0 * rx / (4 * sigma_x), 2.0 * ry / (4 * sigma_y)  # d loss / d sigma at this point
        history.append(float(np.mean(np.square(residuals))))
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
    segment, beam = accelerating_line(), incoming_beam(100_000)
    history = tune(segment, beam)
    for t in range(0, len(history), 10):
        print(f"step {t:3d}  loss {history[t]:.4g}")
    print(f"loss {history[0]:.4g} -> {history[-1]:.4g} after {len(history)} Adam steps")
    for name in QUADRUPOLES:
        print(f"  {name}.k1 = {float(getattr(segment, name).k1[0]):+.5g}")
    trace = segment.track_along(beam)
    for marker, (sigma_x, sigma_y) in TARGETS.items():
        k = trace.index_of(marker)
        print(f"  {marker}: sigma_x {float(trace.sigma_x[0, k]):.4e} (target {sigma_x:.4e}), "
              f"sigma_y {float(trace.sigma_y[0, k]):.4e} (target {sigma_y:.4e})")
