"""
Beta functions ALONG a lattice: `Segment.track_along` returns the beam's moments at the entrance and behind every
element from one pass over the particles -- the data behind the reference's `Segment.plot_twiss` (no plotting here:
the table is printed).

    python examples/twiss_along_lattice.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import lynx_amd as lx  # noqa: E402


def show(title, trace, every=1):
    print(f"\n{title}: {trace.num_points} points, {trace.num_particles or 'parameter'} particles")
    print(f"{'point':>5} {'behind':<12} {'s [m]':>8} {'beta_x [m]':>12} {'beta_y [m]':>12} {'sigma_x [um]':>13}")
    for k in range(0, trace.num_points, every):
        p = trace.at(k)
        print(f"{k:>5} {str(p['name'] or '(entrance)'):<12} {float(p['s'].flat[0]):>8.3f} {float(p['beta_x'].flat[0]):>12.4f}"
              f" {float(p['beta_y'].flat[0]):>12.4f} {1e6 * float(p['sigma_x'].flat[0]):>13.3f}")


f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731

# the ARES-like segment of the README
ares = lx.Segment([
    lx.BPM(name="BPM1"), lx.Drift(f(1.0), name="D1"), lx.BPM(name="BPM6"), lx.Drift(f(1.0), name="D2"),
    lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), name="V7"), lx.Drift(f(0.2), name="D3"),
    lx.HorizontalCorrector(f(0.3), angle=f(1e-4), name="H10"), lx.Drift(f(7.0), name="D4"),
    lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), name="H12"), lx.Drift(f(0.05), name="D5"), lx.BPM(name="BPM13")])
beam = lx.ParticleBeam.from_twiss(num_particles=100_000, beta_x=f(5.0), alpha_x=f(0.5), emittance_x=f(1e-9), beta_y=f(3.0),
                                  alpha_y=f(-0.3), emittance_y=f(1e-9), energy=f(1e8), seed=1)
trace = ares.track_along(beam)
show("ARES-like segment", trace)
print("points the reference's plot_twiss has (zero-length elements left out):", np.flatnonzero(trace.where_length_changes()).tolist())

# a 32-cell FODO channel, one sample of a k1 scan
cells = []
for c in range(32):
    cells += [lx.Quadrupole(f(0.2), k1=f(4.2), name=f"QF{c}"), lx.Drift(f(0.5), name=f"DA{c}"),
              lx.Quadrupole(f(0.2), k1=f(-4.2), name=f"QD{c}"), lx.Drift(f(0.5), name=f"DB{c}")]
fodo = lx.Segment(cells)
trace = fodo.track_along(beam, keep_outgoing=False)
show("32-cell FODO (every 8th point)", trace, every=8)
print(f"\nbeta_x along the channel: min {float(trace.beta_x.min()):.3f} m at point {int(trace.beta_x.argmin())},"
      f" max {float(trace.beta_x.max()):.3f} m at point {int(trace.beta_x.argmax())}")
