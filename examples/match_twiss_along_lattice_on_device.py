"""
The tuning of match_twiss_along_lattice.py with the loss formed on the device: `beta_x` and `beta_y` at three markers are
`grad.MomentTargets`, uploaded once outside the loop; every step is one trace, `vjp.moment_loss` read back (eight bytes)
and `vjp(moment_loss_bar=1.0)` -- no cotangent with a point axis is made on the host or uploaded.  The weights 1 / (6
target^2) make the loss that example's mean squared relative distance from the targets.

    python examples/match_twiss_along_lattice_on_device.py          # needs an MI355X and the built library
"""

import importlib.util
import pathlib

import numpy as np

import lynx_amd.grad as grad

# (the existing example's line, beam and targets, from the file next to this one)
_spec = importlib.util.spec_from_file_location("match_twiss_along_lattice", pathlib.Path(__file__).with_name("match_twiss_along_lattice.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
QUADRUPOLES, TARGETS, matching_line, incoming_beam = base.QUADRUPOLES, base.TARGETS, base.matching_line, base.incoming_beam


def moment_targets():
    targets = {marker: {"beta_x": beta_x, "beta_y": beta_y} for marker, (beta_x, beta_y) in TARGETS.items()}
    weights = {marker: {name: 1.0 / (6 * value**2) for name, value in named.items()} for marker, named in targets.items()}
    return grad.MomentTargets(targets, weights)


def tune(segment, beam, steps=150, lr=0.1):
    """Adam on the four strengths; returns the loss history (loss = mean squared relative distance from the targets)."""
    targets = moment_targets()
    m, v, history = np.zeros(4), np.zeros(4), []
    for t in range(1, steps + 1):
        vjp = grad.track_along_vjp(segment, beam, moment_targets=targets)
        history.append(float(vjp.moment_loss[0]))
        g = vjp(moment_loss_bar=1.0)
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
