"""
What the trajectories of ten particles cost a beam trace, and what they cost before there was a way to ask for them.

  fodo   64 x 100 000 x 128 FODO, float32, one incoming beam shared by the batch: `track_along(beam, trajectories=10)`
         against the plain `track_along(beam)` of the same segment -- the default call, which takes the path it took
         before -- and against the element loop `for el in leaves: beam = el.track(beam)` that reads ten particles of
         every intermediate beam back, ALTERNATING in one process.
  ares   1 x 1 000 000 x 11 ARES-like, float64: the same three.

HIP events on the context's stream (lynx_timer_start / _stop) around each whole job -- launches, read-back of the
records, the properties read from them and the trajectories -- warm-up first, median and spread of `--repeats` runs.

    python scripts/gpu/trace_trajectories_speed.py [--repeats 7] [--only fodo|ares]

Prints one JSON line per shape.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import lynx_amd as lx  # noqa: E402
from lynx_amd.device import get_runtime  # noqa: E402

rt = get_runtime()
KEYS = ("mu_x", "mu_y", "sigma_x", "sigma_y", "beta_x", "beta_y")
K = 10


def timed(job):
    ms = C.c_float()
    rt.check(rt.lib.lynx_timer_start(rt.ctx))
    job()
    rt.check(rt.lib.lynx_timer_stop(rt.ctx, C.byref(ms)))
    return ms.value


def summary(times):
    t = np.sort(np.array(times))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4)}


def alternating(jobs, repeats, warmup=2, slow=()):
    """Every job `repeats` times, one after the other in turn: {name: median, min, max}.  The jobs named in `slow` (the
    element loop: seconds per run at the large shape) take part in one warm-up round and in the first three rounds."""
    for round_ in range(warmup):
        for name, job in jobs.items():
            if name not in slow or round_ == 0:
                job()
    rt.sync()
    times = {name: [] for name in jobs}
    for round_ in range(repeats):
        for name, job in jobs.items():
            if name not in slow or round_ < 3:
                times[name].append(timed(job))
    return {name: summary(t) for name, t in times.items()}


def fodo(B=64, N=100_000, cells=32, dtype=np.float32):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    elements = []
    for _ in range(cells):
        elements += [lx.Quadrupole(f(0.2), k1=k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                     lx.Quadrupole(f(0.2), k1=-k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype)]
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=1, dtype=dtype)
    return lx.Segment(elements), beam.broadcast((B,))


def ares(N=1_000_000, dtype=np.float64):
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    segment = lx.Segment([
        lx.BPM(), lx.Drift(f(1.0), dtype=dtype), lx.BPM(), lx.Drift(f(1.0), dtype=dtype),
        lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(1e-4), dtype=dtype), lx.Drift(f(7.0), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), dtype=dtype), lx.Drift(f(0.05), dtype=dtype), lx.BPM()])
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[175e-9, 2e-7, 175e-9, 2e-7, 1e-6, 1e-6], energy=1e8, seed=1, dtype=dtype)
    return segment, beam


def read(trace):
    return [getattr(trace, key) for key in KEYS], trace.trajectories


def measure(name, shape, segment, beam, repeats):
    leaves = list(segment._leaves())

    def loop():
        """What there was: a launch and a read-back of the whole particle array per element, ten particles kept."""
        b, out = beam, [np.array(np.asarray(beam.particles)[..., :K, :])]
        for el in leaves:
            b = el.track(b)
            out.append(np.array(np.asarray(b.particles)[..., :K, :]))  # (a copy: the whole array is let go)
        return np.stack(out, axis=-3)

    jobs = {
        "trajectories": lambda: read(segment.track_along(beam, keep_outgoing=False, trajectories=K)),
        "plain": lambda: read(segment.track_along(beam, keep_outgoing=False)),
        "element_loop": loop,
    }
    res = {"shape": shape, "elements": len(leaves), "chosen": K}
    res.update(alternating(jobs, repeats, slow=("element_loop",)))
    res["trajectories_minus_plain_ms"] = round(res["trajectories"]["median_ms"] - res["plain"]["median_ms"], 4)
    res["trajectories_over_plain"] = round(res["trajectories"]["median_ms"] / res["plain"]["median_ms"], 3)
    res["loop_over_trajectories"] = round(res["element_loop"]["median_ms"] / res["trajectories"]["median_ms"], 2)
    got = segment.track_along(beam, keep_outgoing=False, trajectories=K).trajectories
    res["same_as_loop"] = bool(np.allclose(got, loop(), rtol=1e-4 if got.dtype == np.float32 else 1e-10, atol=0))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fodo", "ares"))
    args = ap.parse_args()
    if args.only in (None, "fodo"):
        measure("fodo", "fodo 64 x 100000 x 128 float32, shared incoming beam", *fodo(), args.repeats)
    if args.only in (None, "ares"):
        measure("ares", "ares-like 1 x 1000000 x 11 float64", *ares(), args.repeats)
