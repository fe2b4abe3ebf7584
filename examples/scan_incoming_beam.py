"""
64 incoming beams through ONE lattice in one pass: every sample of the batch gets its own Twiss values, made on the
device (`ParticleBeam.from_twiss(..., on_device=True)`: the particles never exist on the host), and
`Segment.track_along` gives `beta_x` and `sigma_x` of every sample at every element.  The beam behind the lattice is
then rescaled on the device to the size the next section wants (`transformed_to(..., on_device=True)`).

    python examples/scan_incoming_beam.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import lynx_amd as lx  # noqa: E402

B, N = 64, 100_000
f = lambda v: np.full(B, v, dtype=np.float32)  # noqa: E731

# a matching scan: beta_x and alpha_x of the incoming beam vary over the batch, the magnets do not
beta_x = np.linspace(2.0, 12.0, B).astype(np.float32)
alpha_x = np.linspace(-1.5, 1.5, B).astype(np.float32)
beam = lx.ParticleBeam.from_twiss(num_particles=N, beta_x=beta_x, alpha_x=alpha_x, emittance_x=f(2e-9), beta_y=f(4.0),
                                  alpha_y=f(0.3), emittance_y=f(1e-9), sigma_s=f(1e-5), sigma_p=f(1e-3), energy=f(1e8),
                                  seed=1, on_device=True)
print(f"incoming: {type(beam.particles).__name__} {beam.particles.shape}; beta_x of samples 0, 31, 63 as sampled:",
      np.round(beam.beta_x[[0, 31, 63]], 3))

cells = []
for c in range(4):
    cells += [lx.Quadrupole(f(0.2), k1=f(4.2), name=f"QF{c}"), lx.Drift(f(0.5), name=f"DA{c}"),
              lx.Quadrupole(f(0.2), k1=f(-4.2), name=f"QD{c}"), lx.Drift(f(0.5), name=f"DB{c}")]
segment = lx.Segment(cells)
trace = segment.track_along(beam)
worst = trace.beta_x.max(axis=-1)  # the largest beta_x along the channel, per incoming beam
best = int(worst.argmin())
print(f"{trace.num_points} points x {B} incoming beams; the beam that stays smallest is sample {best}: beta_x = {beta_x[best]:.2f} m,"
      f" alpha_x = {alpha_x[best]:.2f} in front, beta_x <= {worst[best]:.2f} m along the channel (worst sample: {worst.max():.2f} m)")

out = trace.outgoing
next_section = out.transformed_to(sigma_x=f(5e-5), sigma_y=f(5e-5), mu_x=f(0.0), mu_y=f(0.0), on_device=True)
print(f"behind the channel sigma_x = {1e6 * out.sigma_x.min():.1f} ... {1e6 * out.sigma_x.max():.1f} um;"
      f" rescaled on the device: {1e6 * next_section.sigma_x.min():.2f} ... {1e6 * next_section.sigma_x.max():.2f} um")
