"""
What a screen behind a collimator shows over a batched quadrupole scan: `Segment.track_along(beam, losses=True,
screens=True)` takes the active aperture AND the active screens into the trace.  Every one of the 16 magnet settings loses
its own particles at the collimator, and each screen makes its image of the particles that are alive where it stands --
in the same pass, with the beam going on behind it (inside the trace a screen is a diagnostic, not the end of the line).

    python examples/screen_scan.py
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
camera = dict(resolution=(240, 160), pixel_size=(1e-5, 1e-5), binning=4, dtype=dtype)  # 60 x 40 pixels of 40 um
segment = lx.Segment([
    lx.Drift(f(0.5), name="D1"),
    lx.Quadrupole(f(0.2), k1=k1, name="Q1"),
    lx.Drift(f(2.0), name="D2"),
    lx.Screen(**camera, is_active=True, name="SCREEN_BEFORE"),
    lx.Aperture(x_max=np.array([2e-4], dtype=dtype), y_max=np.array([2e-4], dtype=dtype), shape="elliptical", name="COLLIMATOR"),
    lx.Drift(f(1.0), name="D3"),
    lx.Screen(**camera, misalignment=np.array([1e-4, 0.0], dtype=dtype), is_active=True, name="SCREEN_BEHIND"),
    lx.Drift(f(0.5), name="D4"),
])
one = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 5e-5, 1e-4, 5e-5, 1e-5, 1e-3], energy=1e8, seed=3, dtype=dtype)
beam = one.broadcast((B,))  # one incoming beam shared by the batch

trace = segment.track_along(beam, losses=True, screens=True)

before, behind = trace.image_at("SCREEN_BEFORE"), trace.image_at("SCREEN_BEHIND")  # (B, 40, 60) each
at_screen = trace.index_of("SCREEN_BEHIND") - 1  # a screen observes the beam that ENTERS it
print(f"{N} particles per setting; screens at points {trace.screens}, apertures {trace.apertures}; images {before.shape}")
print(f"{'k1 [1/m^2]':>11} {'transmitted':>12} {'on SCREEN_BEFORE':>17} {'on SCREEN_BEHIND':>17} {'of the survivors':>17} {'brightest pixel':>16}")
for b in range(B):
    seen = behind[b].sum()
    print(f"{k1[b]:>11.2f} {trace.transmission[b, -1]:>12.4f} {int(before[b].sum()):>17d} {int(seen):>17d}"
          f" {seen / max(trace.num_survivors[b, at_screen], 1):>17.4f} {int(behind[b].max()):>16d}")
best = int(behind.max(axis=(-2, -1)).argmax())
row, col = np.unravel_index(int(behind[best].argmax()), behind[best].shape)
print(f"\nthe tightest spot behind the collimator is at k1 = {k1[best]:.2f}: {int(behind[best].max())} particles in pixel"
      f" (row {row}, column {col}) of {behind[best].shape}; the screen stands 100 um off the axis, so the spot is left of centre")
print("the screen elements hold the same arrays:", segment.elements[6].reading is behind)
