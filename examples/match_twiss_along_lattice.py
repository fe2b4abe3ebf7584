"""
Matching Twiss functions ALONG a beamline: Adam on the four quadrupoles of a short line until `beta_x` and `beta_y` at
three markers have given values.  The loss is written in properties of the beam at interior points of the lattice, so
its gradient comes from `lynx_amd.grad.track_along_vjp`: one pass over the particles for the trace, one reverse sweep
over the moments for all six cotangents (the optimiser is written out in NumPy, as in gradient_based_tuning.py).

    python examples/match_twiss_along_lattice.py          # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

QUADRUPOLES = ("Q1", "Q2", "Q3", "Q4")
# (beta_x, beta_y) in metres behind each marker: what k1 = (3, -3.5, 2.5, -2) gives a beam that comes in with
# beta_x = beta_y = 5 m, alpha = 0 -- so the four quadrupoles can reach all six values
TARGETS = {"M1": (1.7377, 7.5687), "M2": (1.9436, 7.6125), "M3": (4.7739, 4.9220)}


def matching_line():
    return lx.Segment([
        lx.Quadrupole(f(0.2), k1=f(1.5), name="Q1"), lx.Drift(f(0.5)),
        lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q2"), lx.Drift(f(0.5)), lx.Marker(name="M1"),
        lx.Quadrupole(f(0.2), k1=f(1.5), name="Q3"), lx.Drift(f(0.5)),
        lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q4"), lx.Drift(f(0.5)), lx.Marker(name="M2"),
        lx.Drift(f(1.0)), lx.Marker(name="M3"),
    ])


def incoming_beam(num_particles=20_000):
    """Emittance 1 nm rad in both planes, beta = 5 m, alpha = 0."""
    return lx.ParticleBeam.from_parameters(num_particles=num_particles, sigma_x=f(7.0711e-5), sigma_xp=f(1.41421e-5),
                                           sigma_y=f(7.0711e-5), sigma_yp=f(1.41421e-5), sigma_s=f(8e-6), sigma_p=f(1e-3),
                                           energy=f(1e8), seed=0)


def tune(segment, beam, steps=150, lr=0.1):
    """Adam on the four strengths; returns the loss history (loss = mean squared relative distance from the targets)."""
    m, v, history = np.zeros(4), np.zeros(4), []
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam)
        trace = vjp.trace
        bar_x, bar_y = np.zeros((1, trace.num_points)), np.zeros((1, trace.num_points))
        residuals = []
        for marker, (beta_x, beta_y) in TARGETS.items():
            k = trace.index_of(marker)
            rx, ry = float(trace.beta_x[0, k]) / beta_x - 1.0, float(trace.beta_y[0, k]) / beta_y - 1.0
            residuals += [rx, ry]
            bar_x[0, k], bar_y[0, k] = 2.0 * rx / (6 * beta_x), 2.0 * ry / (6 * beta_y)  # d loss / d beta at this point
        history.append(float(np.mean(np.square(residuals))))
        g = vjp(beta_x=bar_x, beta_y=bar_y)
        gradient = np.array([float(g[getattr(segment, name)]["k1"][0]) for name in QUADRUPOLES])
        m = 0.9 * m + 0.1 * gradient
        v = 0.999 * v + 0.001 * gradient**2
        update = lr * (m / (1 - 0.9**t)) / (np.sqrt(v / (1 - 0.999**t)) + 1e-12)
        for name, delta in zip(QUADRUPOLES, update):
            quadrupole = getattr(segment, name)
            quadrupole.k1 = (quadrupole.k1 - delta).astype(np.float32)
    return history


if __name__ == "__main__":
    segment, beam = matching_line(), incoming_beam(100_000)
    history = tune(segment, beam)
    for t in range(0, len(history), 10):
        print(f"step {t:3d}  loss {history[t]:.4g}")
    print(f"loss {history[0]:.4g} -> {history[-1]:.4g} after {len(history)} Adam steps")
    for name in QUADRUPOLES:
        print(f"  {name}.k1 = {float(getattr(segment, name).k1[0]):+.5g}")
    trace = segment.track_along(beam)
    for marker, (beta_x, beta_y) in TARGETS.items():
        k = trace.index_of(marker)
        print(f"  {marker}: beta_x {float(trace.beta_x[0, k]):.4f} (target {beta_x}), beta_y {float(trace.beta_y[0, k]):.4f} (target {beta_y})")
