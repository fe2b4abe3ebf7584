"""
How much beam gets through a collimator, and what it looks like behind it, over a batched quadrupole scan:
`Segment.track_along(beam, losses=True)` takes active apertures into the trace -- a lost particle is dropped from every
later point, nothing is compacted, so every one of the 16 magnet settings loses its own particles in the same pass.

    python examples/transmission_scan.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import lynx_amd as lx  # noqa: E402

B, N = 16, 200_000
dtype = np.float32
f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731

k1 = np.linspace(-6.0, 6.0, B).astype(dtype)  # the scan: one focusing strength per sample
segment = lx.Segment([
    lx.Drift(f(0.5), name="D1"),
    lx.Quadrupole(f(0.2), k1=k1, name="Q1"),
    lx.Drift(f(2.0), name="D2"),
    lx.Aperture(x_max=np.array([2e-4], dtype=dtype), y_max=np.array([2e-4], dtype=dtype), shape="elliptical", name="COLLIMATOR"),
    lx.Drift(f(1.0), name="D3"),
    lx.BPM(is_active=True, name="BPM"),
    lx.Drift(f(0.5), name="D4"),
])
one = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 5e-5, 1e-4, 5e-5, 1e-5, 1e-3], energy=1e8, seed=3, dtype=dtype)
beam = one.broadcast((B,))  # one incoming beam shared by the batch

trace = segment.track_along(beam, losses="particles")

behind = trace.index_of("COLLIMATOR")
print(f"{N} particles per setting, apertures in the trace: {trace.apertures}")
print(f"{'k1 [1/m^2]':>11} {'transmission':>13} {'lost':>8} {'sigma_x in [um]':>16} {'sigma_x behind [um]':>20} {'sigma_x at end [um]':>20}")
for b in range(B):
    print(f"{k1[b]:>11.2f} {trace.transmission[b, -1]:>13.4f} {int(trace.lost_in[b, 0]):>8d} {1e6 * trace.sigma_x[b, behind - 1]:>16.2f}"
          f" {1e6 * trace.sigma_x[b, behind]:>20.2f} {1e6 * trace.sigma_x[b, -1]:>20.2f}")
best = int(trace.transmission[:, -1].argmax())
print(f"\nbest transmission {trace.transmission[best, -1]:.4f} at k1 = {k1[best]:.2f}; the BPM behind the collimator reads the"
      f" survivors' centroid: x = {1e6 * segment.elements[5].reading[0, best]:.3f} um")
# which particles went: `lost_at` is 0 (the ordinal of COLLIMATOR in trace.apertures) for a lost particle, -1 for a survivor
lost = trace.lost_at[best] == 0
x_in = np.asarray(one.particles)[0, :, 0]
print(f"at that setting the lost particles entered with rms x = {1e6 * x_in[lost].std():.1f} um, the survivors with {1e6 * x_in[~lost].std():.1f} um")
print("trace.outgoing is", trace.outgoing, "-- a beam object has one particle count for all samples; the loss map says who is left")
