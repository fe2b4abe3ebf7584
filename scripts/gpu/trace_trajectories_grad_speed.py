"""
What the gradient of chosen particles' trajectories costs, against the only other way to get it: finite differences.

  64 samples x 128 elements (32 FODO cells, a k1 scan over the batch) x K = 128 chosen particles, float32 and float64.
  The beam IS the 128 particles (a halo set), so a finite-difference trace pays for nothing it does not need.

  reverse   one `vjp(trajectories_bar=w)` on an existing `track_along_vjp(segment, beam, trajectories=128)`: upload of the
            cotangents, k_trace_trajectories_bwd, k_build_bwd, read-back of every element's gradients;
  vjp       the same with the forward trace in it (what one optimiser step pays);
  forward   one `track_along(beam, trajectories=128)` with its trajectories read -- central differences need
            2 x (number of parameters) of them: 2 x 192 here (64 strengths, 128 lengths), every sample stepped at once.

HIP events on the context's stream (lynx_timer_start / _stop) around each whole job, warm-up first, median and spread of
`--repeats` runs, the jobs alternating in one process.

    python scripts/gpu/trace_trajectories_grad_speed.py [--repeats 7] [--dtype float32|float64]

Prints one JSON line per dtype.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from lynx_amd.device import get_runtime  # noqa: E402

rt = get_runtime()
B, CELLS, K = 64, 32, 128


def timed(job):
    ms = C.c_float()
    rt.check(rt.lib.lynx_timer_start(rt.ctx))
    job()
    rt.check(rt.lib.lynx_timer_stop(rt.ctx, C.byref(ms)))
    return ms.value


def summary(times):
    t = np.sort(np.array(times))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4)}


def lattice(dtype):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    elements = []
    for _ in range(CELLS):
        elements += [lx.Quadrupole(f(0.2), k1=k.copy(), dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                     lx.Quadrupole(f(0.2), k1=-k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype)]
    rng = np.random.default_rng(1)
    particles = np.ones((1, K, 7), dtype=dtype)
    particles[0, :, :6] = rng.normal(0.0, [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], (K, 6))
    beam = lx.ParticleBeam(particles, np.array([1e8], dtype=dtype), dtype=dtype).broadcast((B,))
    return lx.Segment(elements), beam


def measure(dtype, repeats):
    segment, beam = lattice(dtype)
    leaves = list(segment._leaves())
    P = len(leaves) + 1
    w = np.zeros((B, P, K, 6))
    w[..., 0] = w[..., 2] = 1.0
    held = grad.track_along_vjp(segment, beam, trajectories=K)

    def gradients(g):
        return [g[el] for el in leaves], g.energy, g.chosen_particles

    jobs = {
        "reverse": lambda: gradients(held(trajectories_bar=w)),
        "vjp": lambda: gradients(grad.track_along_vjp(segment, beam, trajectories=K)(trajectories_bar=w)),
        "forward": lambda: segment.track_along(beam, keep_outgoing=False, trajectories=K).trajectories,
    }
    for _ in range(2):
        for job in jobs.values():
            job()
    rt.sync()
    times = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, job in jobs.items():
            times[name].append(timed(job))
    parameters = sum(2 if isinstance(el, lx.Quadrupole) else 1 for el in leaves)
    res = {"shape": f"{B} x {len(leaves)} elements x K = {K}, {np.dtype(dtype).name}", "parameters": parameters}
    res.update({name: summary(t) for name, t in times.items()})
    res["finite_differences_ms"] = round(2 * parameters * res["forward"]["median_ms"], 2)
    res["finite_differences_over_vjp"] = round(res["finite_differences_ms"] / res["vjp"]["median_ms"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", choices=("float32", "float64"))
    args = ap.parse_args()
    for name in ("float32", "float64"):
        if args.dtype in (None, name):
            measure(np.dtype(name).type, args.repeats)
