"""
Steering a beam's halo through a collimator with gradients of single-particle trajectories.  `transmission` of
`track_along(losses=True)` is a step function of the magnets -- its gradient is zero -- so the loss is the usual
differentiable surrogate: the clearance of every particle to the collimator's limits at the point where it stands,

    loss = sum over particles of relu(|x| - c x_max)^2 + relu(|y| - c y_max)^2,

with the collimator switched off for the gradient (it is an identity step of the trace then).  The coordinates of the
particles at that point come from `track_along_vjp(..., trajectories=N)`, their cotangents go back in through
`trajectories_bar`, and Adam (written out in NumPy, as in gradient_based_tuning.py) moves two correctors and two
quadrupoles until no particle is outside c = 80 % of the limits.  Then the collimator is switched on again and
`track_along(losses=True)` counts what gets through, before and after.

    python examples/steer_halo_through_collimator.py          # needs an MI355X and the built library
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

MARGIN = 0.8  # c: the part of the collimator's half-widths the halo is steered into
# (element, parameter, Adam step): the angles are 1e-4 rad, the strengths 1 / m^2
KNOBS = (("HCOR", "angle", 2e-5), ("VCOR", "angle", 2e-5), ("Q1", "k1", 0.05), ("Q2", "k1", 0.05))


def beamline():
    return lx.Segment([
        lx.Drift(f(0.3), name="D1"),
        lx.HorizontalCorrector(f(0.1), angle=f(0.0), name="HCOR"),
        lx.VerticalCorrector(f(0.1), angle=f(0.0), name="VCOR"),
        lx.Quadrupole(f(0.2), k1=f(0.5), name="Q1"), lx.Drift(f(0.5), name="D2"),
        lx.Quadrupole(f(0.2), k1=f(-0.5), name="Q2"), lx.Drift(f(2.0), name="D3"),
        lx.Aperture(x_max=f(4e-4), y_max=f(4e-4), shape="rectangular", name="COLLIMATOR"),
        lx.Drift(f(1.0), name="D4"),
    ])


def incoming_beam(num_particles=256):
    """A small beam that comes in off the axis: part of it misses the collimator's opening."""
    rng = np.random.default_rng(11)
    particles = np.ones((1, num_particles, 7), dtype=np.float32)
    particles[0, :, :6] = rng.normal([3e-4, 2e-5, -2e-4, -1e-5, 0.0, 0.0], [6e-5, 1e-5, 6e-5, 1e-5, 1e-5, 1e-3],
                                     (num_particles, 6))
    return lx.ParticleBeam(particles, f(1e8))


def transmission(segment, beam) -> float:
    """The part of the beam behind the (active) collimator."""
    return float(segment.track_along(beam, losses=True).transmission[0, -1])


def clearance(segment, beam):
    """
    (loss, gradients per knob) with the collimator switched off: the forward trace with every particle's trajectory, the
    cotangent of x and y at the collimator's point, one reverse call.
    """
    collimator = segment.COLLIMATOR
    active, collimator.is_active = collimator.is_active, False
    try:
        vjp = grad.track_along_vjp(segment, beam, trajectories=beam.num_particles)
        trace = vjp.trace
        k = trace.index_of("COLLIMATOR")  # the point the collimator tests: the beam that ENTERS it
        bar = np.zeros(trace.trajectories.shape, dtype=np.float64)
        loss = 0.0
        for column, limit in ((0, float(collimator.x_max[0])), (2, float(collimator.y_max[0]))):
            position = trace.trajectories[0, k, :, column].astype(np.float64)
            outside = np.maximum(np.abs(position) - MARGIN * limit, 0.0)
            loss += float(np.sum(outside**2))
            bar[0, k, :, column] = 2.0 * outside * np.sign(position)
        if loss == 0.0:
            return loss, None
        g = vjp(trajectories_bar=bar)
        return loss, [float(g[getattr(segment, name)][parameter][0]) for name, parameter, _ in KNOBS]
    finally:
        collimator.is_active = active


def tune(segment, beam, steps=400):
    """Adam on the knobs until every particle clears the collimator; returns the loss history (its last entry is 0 then)."""
    m, v, history = np.zeros(len(KNOBS)), np.zeros(len(KNOBS)), []
    for t in range(1, steps + 1):
        loss, gradient = clearance(segment, beam)
        history.append(loss)
        if gradient is None:
            break
        gradient = np.asarray(gradient)
        m = 0.9 * m + 0.1 * gradient
        v = 0.999 * v + 0.001 * gradient**2
        update = (m / (1 - 0.9**t)) / (np.sqrt(v / (1 - 0.999**t)) + 1e-30)
        for (name, parameter, rate), delta in zip(KNOBS, update):
            element = getattr(segment, name)
            setattr(element, parameter, (getattr(element, parameter) - rate * delta).astype(np.float32))
    return history


if __name__ == "__main__":
    segment, beam = beamline(), incoming_beam()
    before = transmission(segment, beam)
    history = tune(segment, beam)
    for t in range(0, len(history), 10):
        print(f"step {t:3d}  clearance loss {history[t]:.4g}")
    print(f"clearance loss {history[0]:.4g} -> {history[-1]:.4g} after {len(history) - 1} Adam steps")
    for name, parameter, _ in KNOBS:
        print(f"  {name}.{parameter} = {float(getattr(getattr(segment, name), parameter)[0]):+.5g}")
    print(f"transmission through the collimator: {before:.4f} before, {transmission(segment, beam):.4f} after")
