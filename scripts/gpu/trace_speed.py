"""
`Segment.track_along` against the only way the same data could be had before it: the loop of the reference's
`plot_twiss`, `for el in leaves: beam = el.track(beam)` with the moment properties read at every point -- same
process, same input, warm.  HIP events on the context's stream (lynx_timer_start / _stop) around each whole job,
warm-up first, several repeats: median and spread.  Next to them `segment.track` with one record read, so that a
reader sees what the P records cost over the one.

    python scripts/gpu/trace_speed.py [--repeats 7] [--only fodo|ares] [--once]

Prints one JSON line per shape.  `--once`: one warm trace per shape and nothing else (for a profiler run).
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


def gpu_ms(job, repeats, warmup=2):
    for _ in range(warmup):
        job()
    rt.sync()
    times = []
    for _ in range(repeats):
        ms = C.c_float()
        rt.check(rt.lib.lynx_timer_start(rt.ctx))
        job()
        rt.check(rt.lib.lynx_timer_stop(rt.ctx, C.byref(ms)))
        times.append(ms.value)
    t = np.sort(np.array(times))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4)}


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


def measure(name, segment, beam, repeats, once):
    leaves = list(segment._leaves())

    def trace():
        t = segment.track_along(beam, keep_outgoing=False)
        return [getattr(t, key) for key in KEYS]

    def trace_keeping():
        t = segment.track_along(beam)
        return [getattr(t, key) for key in KEYS]

    def loop():
        b, out = beam, []
        for el in leaves:
            b = el.track(b)
            out.append([getattr(b, key) for key in KEYS])
        return out

    def track():
        return segment.track(beam).sigma_x

    if once:
        trace()
        trace()
        rt.sync()
        return
    res = {"shape": name, "elements": len(leaves), "batch": list(beam.batch_shape), "particles": beam.num_particles,
           "dtype": beam.dtype.name,
           "trace_moments_only": gpu_ms(trace, repeats), "trace_with_outgoing": gpu_ms(trace_keeping, repeats),
           "element_loop": gpu_ms(loop, max(3, repeats // 2), warmup=1), "segment_track": gpu_ms(track, repeats)}
    res["loop_over_trace"] = round(res["element_loop"]["median_ms"] / res["trace_with_outgoing"]["median_ms"], 2)
    res["trace_over_track"] = round(res["trace_with_outgoing"]["median_ms"] / res["segment_track"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fodo", "ares"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.only in (None, "fodo"):
        measure("fodo 64 x 100000 x 128 float32, shared incoming beam", *fodo(), args.repeats, args.once)
    if args.only in (None, "ares"):
        measure("ares-like 1 x 1000000 float64", *ares(), args.repeats, args.once)
