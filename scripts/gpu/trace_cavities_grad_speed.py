"""
`lynx_amd.grad.track_along_vjp(..., cavities=True)` -- forward trace + the reverse pass over the particles with a moment
cotangent injected at every point -- against
  (a) one `track_vjp` per point that carries a cotangent, on the prefix `Segment(leaves[:k])` of the lattice: what gave
      the same gradient before this call existed;
  (b) a single `track_vjp` of the whole lattice with the cotangent at its end: the same sweep without injections, so
      new / (b) is the price of the injection (plus the trace's forward pass against the plain one).
`sigma_x`, `sigma_y` cotangents at every point and at 3 points.  Same process, same input, warm.  HIP events on the
context's stream (lynx_timer_start / _stop) around each whole job, warm-up first, several repeats: median and spread; the
share of the reverse streaming kernel (k_track_bwd_inject) from lynx_profile_launches, with the cotangents as given and
with one at the last point alone (the sweep without injections).  float32 samples whose units all have class U take the
structured kernel in (a) and (b); LYNX_BWD_UNITS=0 in the environment sends them through k_track_bwd, the kernel the new
call is built from.

    python scripts/gpu/trace_cavities_grad_speed.py [--repeats 7] [--only c5|linac] [--what along|prefix|whole]

Prints one JSON line per (shape, set of points).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import bench  # noqa: E402
import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from trace_speed import gpu_ms, rt  # noqa: E402


def config5(B=4096, N=10_000, dtype=np.float32):
    """BASELINE config 5's lattice and beam: [Drift, misaligned Quadrupole, Drift, Cavity] x 8, 6 MeV."""
    segment = bench.build_segment(lx, "c5", np.arange(B), 8, dtype, 0)
    beam = lx.ParticleBeam.synthetic((B,), N, sigma=bench.BEAM_SIGMA, energy=bench.beam_energy("c5"), seed=2, dtype=dtype)
    return segment, beam


def linac(N=1_000_000, dtype=np.float64):
    """11 elements, one cavity, batch 1."""
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    segment = lx.Segment([
        lx.Drift(f(1.0), dtype=dtype), lx.Quadrupole(f(0.2), k1=f(2.0), dtype=dtype), lx.Drift(f(1.0), dtype=dtype),
        lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
        lx.Cavity(f(1.0377), voltage=f(2e7), phase=f(-5.0), frequency=f(1.3e9), dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
        lx.Quadrupole(f(0.2), k1=f(-2.0), dtype=dtype), lx.Drift(f(3.0), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), dtype=dtype), lx.Drift(f(0.05), dtype=dtype)])
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=2e7, seed=1, dtype=dtype)
    return segment, beam


def measure(name, segment, beam, points, repeats, what):
    leaves = list(segment._leaves())
    P = len(leaves) + 1
    w = np.zeros((*beam.batch_shape, P))
    w[..., points] = 1.0
    probe = grad.track_along_vjp(segment, beam, cavities=True)(sigma_x=w)
    differentiable = [el for el in leaves if el in probe]

    def along():
        g = grad.track_along_vjp(segment, beam, cavities=True)(sigma_x=w, sigma_y=w)
        return [g[el] for el in differentiable], g.energy

    res = {"shape": name, "elements": len(leaves), "batch": list(beam.batch_shape), "particles": beam.num_particles,
           "dtype": beam.dtype.name, "points": [int(k) for k in points]}
    if what in (None, "along"):
        res["track_along_vjp_cavities"] = gpu_ms(along, repeats)
        vjp = grad.track_along_vjp(segment, beam, cavities=True)

        def reverse():
            g = vjp(sigma_x=w, sigma_y=w)
            return [g[el] for el in differentiable], g.energy

        res["reverse_call_alone"] = gpu_ms(reverse, repeats)
        rt.sync()
        rt.profile_begin()
        for _ in range(repeats):
            reverse()
        rt.sync()
        rt.profile_end()
        kernel = np.sort(np.array(rt.profile_launches()))
        res["k_track_bwd_inject"] = {"median_ms": round(float(np.median(kernel)), 4), "min_ms": round(float(kernel[0]), 4),
                                     "max_ms": round(float(kernel[-1]), 4), "launches": len(kernel)}
        # the same kernel with a cotangent at the last point alone: the sweep without injections
        end = np.zeros_like(w)
        end[..., -1] = 1.0
        vjp(sigma_x=end, sigma_y=end)
        rt.sync()
        rt.profile_begin()
        for _ in range(repeats):
            vjp(sigma_x=end, sigma_y=end)
        rt.sync()
        rt.profile_end()
        kernel = np.sort(np.array(rt.profile_launches()))
        res["k_track_bwd_inject_end_only"] = {"median_ms": round(float(np.median(kernel)), 4), "min_ms": round(float(kernel[0]), 4),
                                              "max_ms": round(float(kernel[-1]), 4), "launches": len(kernel)}
    whole = beam.materialized()
    if what in (None, "prefix"):
        prefixes = [lx.Segment(leaves[:k]) for k in points if k >= 1]

        def prefix_loop():
            out = []
            for prefix in prefixes:
                g = grad.track_vjp(prefix, whole)(sigma_x=1.0, sigma_y=1.0)
                out.append([g[el] for el in prefix.elements if el in g])
            return out

        res["a_track_vjp_per_point"] = gpu_ms(prefix_loop, max(3, repeats // 2), warmup=1)
    if what in (None, "whole"):
        def end_only():
            g = grad.track_vjp(segment, whole)(sigma_x=1.0, sigma_y=1.0)
            return [g[el] for el in differentiable], g.energy

        res["b_track_vjp_at_the_end"] = gpu_ms(end_only, repeats)
    new = res.get("track_along_vjp_cavities", {}).get("median_ms")
    if new and "a_track_vjp_per_point" in res:
        res["a_over_new"] = round(res["a_track_vjp_per_point"]["median_ms"] / new, 2)
    if new and "b_track_vjp_at_the_end" in res:
        res["new_over_b"] = round(new / res["b_track_vjp_at_the_end"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("c5", "linac"))
    ap.add_argument("--what", choices=("along", "prefix", "whole"))
    args = ap.parse_args()
    shapes = []
    if args.only in (None, "c5"):
        shapes.append(("config 5: 4096 x 10000 x 32 elements, 8 cavities, float32", *config5(), [8, 20, 32]))
    if args.only in (None, "linac"):
        shapes.append(("linac: 1 x 1000000 x 11 elements, 1 cavity, float64", *linac(), [3, 7, 11]))
    for name, segment, beam, three in shapes:
        P = len(list(segment._leaves())) + 1
        measure(name, segment, beam, list(range(P)), args.repeats, args.what)
        measure(name, segment, beam, three, args.repeats, args.what)
