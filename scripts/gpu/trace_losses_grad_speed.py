"""
What the gradients of the SURVIVING beam's moments cost: `track_along_vjp(segment, beam, losses=True)` and its call next
to the same two on the same lattice with the collimators switched off (the plain `track_along_vjp`).

  fodo   64 x 100 000 x 128 FODO, float32, one incoming beam shared by the batch, two collimators (behind cells 9 and
         25), cotangents sigma_x = sigma_y = 1 at every point: three survivor sets per sample.
  ares   1 x 1 000 000 x 11 ARES-like, float64, one collimator, the same cotangents: two sets.

Each job is the whole step an optimiser pays: forward trace, (losses: the set records, one more read of the incoming
beam,) cotangent rules, reverse call, every element's gradients read.  The two jobs ALTERNATE in one process; HIP events on
the context's stream (lynx_timer_start / _stop) around each whole job, warm-up first, median and spread of `--repeats`.

    python scripts/gpu/trace_losses_grad_speed.py [--repeats 7] [--only fodo|ares]

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
import lynx_amd.grad as grad  # noqa: E402
from lynx_amd.device import get_runtime  # noqa: E402

rt = get_runtime()


def timed(job):
    ms = C.c_float()
    rt.check(rt.lib.lynx_timer_start(rt.ctx))
    job()
    rt.check(rt.lib.lynx_timer_stop(rt.ctx, C.byref(ms)))
    return ms.value


def summary(times):
    t = np.sort(np.array(times))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4)}


def alternating(jobs, repeats, warmup=2):
    """Every job `repeats` times, one after the other in turn: {name: median, min, max}."""
    for _ in range(warmup):
        for job in jobs.values():
            job()
    rt.sync()
    times = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, job in jobs.items():
            times[name].append(timed(job))
    return {name: summary(t) for name, t in times.items()}


def fodo(B=64, N=100_000, cells=32, dtype=np.float32):
    """Two segments over the same magnets: the collimators active in one, inactive in the other (130 elements each)."""
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    with_losses, plain = [], []
    for cell in range(cells):
        magnets = [lx.Quadrupole(f(0.2), k1=k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                   lx.Quadrupole(f(0.2), k1=-k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype)]
        with_losses += magnets
        plain += magnets
        if cell in (8, 24):
            limits = dict(x_max=np.array([1.5e-4], dtype=dtype), y_max=np.array([1.5e-4], dtype=dtype), dtype=dtype)
            with_losses.append(lx.Aperture(**limits, shape="elliptical" if cell == 24 else "rectangular", name=f"COL{cell}"))
            plain.append(lx.Aperture(**limits, is_active=False, name=f"COL{cell}"))
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=1, dtype=dtype)
    return lx.Segment(with_losses), lx.Segment(plain), beam.broadcast((B,))


def ares(N=1_000_000, dtype=np.float64):
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731

    def line(active):
        return lx.Segment([
            lx.BPM(), lx.Drift(f(1.0), dtype=dtype),
            lx.Aperture(x_max=f(3e-7), y_max=f(3e-7), is_active=active, name="COL", dtype=dtype),
            lx.Drift(f(1.0), dtype=dtype),
            lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
            lx.HorizontalCorrector(f(0.3), angle=f(1e-4), dtype=dtype), lx.Drift(f(7.0), dtype=dtype),
            lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), dtype=dtype), lx.Drift(f(0.05), dtype=dtype), lx.BPM()])

    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[175e-9, 2e-7, 175e-9, 2e-7, 1e-6, 1e-6], energy=1e8, seed=1, dtype=dtype)
    return line(True), line(False), beam


def step(segment, beam, losses):
    """Forward and reverse, every differentiable element's gradients and the energy's read."""
    g = grad.track_along_vjp(segment, beam, losses=losses)(sigma_x=1.0, sigma_y=1.0)
    return [g[el] for el in segment._leaves() if el in g], g.energy


def measure(shape, with_losses, plain, beam, repeats):
    jobs = {"losses": lambda: step(with_losses, beam, True), "plain": lambda: step(plain, beam, False)}
    res = {"shape": shape, "elements": len(list(plain._leaves()))}
    res.update(alternating(jobs, repeats))
    res["losses_over_plain"] = round(res["losses"]["median_ms"] / res["plain"]["median_ms"], 3)
    trace = with_losses.track_along(beam, keep_outgoing=False, losses=True)
    res["transmission_min_max"] = [round(float(trace.transmission[..., -1].min()), 4), round(float(trace.transmission[..., -1].max()), 4)]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fodo", "ares"))
    args = ap.parse_args()
    if args.only in (None, "fodo"):
        measure("fodo 64 x 100000 x 128 float32, shared incoming beam, two collimators", *fodo(), args.repeats)
    if args.only in (None, "ares"):
        measure("ares-like 1 x 1000000 x 11 float64, one collimator", *ares(), args.repeats)
