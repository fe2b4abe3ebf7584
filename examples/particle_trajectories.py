"""
Single-particle trajectories along a beamline -- the picture of the reference's `plot_reference_particle_traces`: ten
linspaced particles through a FODO cell with a collimator, the lattice split every 5 cm.
`Segment.track_along(beam, trajectories=K)` brings the coordinates of the chosen particles at every point back from the
same pass that makes the moments; with `losses=True` a particle the collimator removes has its trajectory up to the
collimator and NaN behind it, and `trajectory_lost_in` names the aperture.

    python examples/particle_trajectories.py
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import lynx_amd as lx  # noqa: E402

K = 10
dtype = np.float32
f = lambda v: np.array([v], dtype=dtype)  # noqa: E731

segment = lx.Segment([
    lx.Quadrupole(f(0.2), k1=f(4.2), name="QF"),
    lx.Drift(f(0.5), name="D1"),
    lx.Aperture(x_max=f(1.5e-4), y_max=f(1.5e-4), shape="elliptical", name="COLLIMATOR"),
    lx.Quadrupole(f(0.2), k1=f(-4.2), name="QD"),
    lx.Drift(f(0.5), name="D2"),
])
beam = lx.ParticleBeam.make_linspaced(num_particles=K, sigma_x=f(1.75e-4), sigma_xp=f(2e-5), sigma_y=f(1.75e-4), sigma_yp=f(2e-5),
                                      energy=f(1e8), dtype=dtype)

trace = segment.track_along(beam, resolution=0.05, losses=True, trajectories=K)

x = trace.trajectories[0, :, :, 0]  # (points, K)
print(f"{trace.num_points} points, particles {trace.trajectory_indices.tolist()}; x in um (nan: lost)")
print(f"{'s [m]':>6} " + " ".join(f"{'x' + str(j):>8}" for j in range(K)))
for k in range(trace.num_points):
    print(f"{float(trace.s[k, 0]):>6.2f} " + " ".join(f"{1e6 * x[k, j]:>8.2f}" for j in range(K)))
print()
for j, ordinal in enumerate(trace.trajectory_lost_in[0]):
    if ordinal < 0:
        print(f"particle {j}: reaches the end")
    else:
        name = trace.apertures[ordinal]
        k = trace.index_of(name) - 1  # it entered the aperture at the point in front of it
        print(f"particle {j}: lost in {name} at s = {float(trace.s[k, 0]):.2f} m, x = {1e6 * x[k, j]:.2f} um,"
              f" y = {1e6 * trace.trajectories[0, k, j, 2]:.2f} um")
print(f"survivors at the end: {int(trace.num_survivors[0, -1])} of {trace.num_particles}")
