"""
What screen images cost a beam trace, and what they cost before the trace made them.

  fodo   64 x 100 000 x 128 FODO, float32, one incoming beam shared by the batch, two collimators (behind cells 9 and
         25) and two screens of 256 x 256 pixels (behind cells 16 and 32; 128 images, 33.5 MB of int32):
         `track_along(beam, losses=True, screens=True)` against `track_along(beam, losses=True)` of the same lattice with
         the screens inactive (two segments over the same magnets), ALTERNATING in one process; a third leg has the same
         screens with 4 x 4 pixels of 250 um -- every add of a wave lands in a handful of cells: the contended case.
  ares   1 x 1 000 000 x 11 ARES-like, float64, one screen at the end with the ARES camera's effective resolution
         (2448 x 2040 pixels of 3.3198 x 2.4469 um): `track_along(beam, screens=True)` plus the image against
         `Segment.track` up to the screen plus `screen.reading`, with the screen aligned and misaligned.

HIP events on the context's stream (lynx_timer_start / _stop) around each whole job -- launches, read-back of the
records, the properties read from them and the images -- warm-up first, median and spread of `--repeats` runs.

    python scripts/gpu/trace_screens_speed.py [--repeats 7] [--only fodo|ares] [--once]

Prints one JSON line per shape.  `--once`: one warm trace of each kind per shape and nothing else (for a profiler run).
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


def fodo(B=64, N=100_000, cells=32, dtype=np.float32, pixels=256, pitch=4e-6, screens_active=True):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    camera = dict(resolution=(pixels, pixels), pixel_size=(pitch, pitch), binning=1, dtype=dtype)  # +- 0.5 mm
    elements = []
    for cell in range(cells):
        elements += [lx.Quadrupole(f(0.2), k1=k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype),
                     lx.Quadrupole(f(0.2), k1=-k, dtype=dtype), lx.Drift(f(0.5), dtype=dtype)]
        if cell in (8, 24):  # (the collimators of trace_losses_speed.py, active in every lattice)
            limits = dict(x_max=np.array([1.5e-4], dtype=dtype), y_max=np.array([1.5e-4], dtype=dtype), dtype=dtype)
            elements.append(lx.Aperture(**limits, shape="elliptical" if cell == 24 else "rectangular", name=f"COL{cell}"))
        if cell in (15, 31):  # (132 elements: one screen has a shared misalignment, the other one per sample)
            shift = np.array([2e-5, 0.0], dtype=dtype) if cell == 15 else (np.linspace(-1e-4, 1e-4, B)[:, None] * np.array([1.0, 0.0])).astype(dtype)
            elements.append(lx.Screen(**camera, misalignment=shift, is_active=screens_active, name=f"SCR{cell}"))
    return lx.Segment(elements)


def fodo_beam(B=64, N=100_000, dtype=np.float32):
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], energy=1e8, seed=1, dtype=dtype)
    return beam.broadcast((B,))


def ares(N=1_000_000, dtype=np.float64, misalignment=(0.0, 0.0)):
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    screen = lx.Screen(resolution=(2448, 2040), pixel_size=(3.3198e-6, 2.4469e-6), binning=1,
                       misalignment=np.array([misalignment], dtype=dtype), is_active=True, name="SCREEN", dtype=dtype)
    segment = lx.Segment([
        lx.BPM(), lx.Drift(f(1.0), dtype=dtype), lx.BPM(), lx.Drift(f(1.0), dtype=dtype),
        lx.VerticalCorrector(f(0.3), angle=f(3.142e-3), dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(1e-4), dtype=dtype), lx.Drift(f(7.0), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=f(-1e-4), dtype=dtype), lx.Drift(f(0.05), dtype=dtype), screen])
    beam = lx.ParticleBeam.synthetic((1,), N, sigma=[175e-6, 2e-7, 175e-6, 2e-7, 1e-6, 1e-6], energy=1e8, seed=1, dtype=dtype)
    return segment, screen, beam


def read(trace):
    return [getattr(trace, key) for key in KEYS] + list(trace.screen_images)


def measure_fodo(repeats, once):
    watched, idle, coarse, beam = fodo(), fodo(screens_active=False), fodo(pixels=4, pitch=2.5e-4), fodo_beam()
    jobs = {
        "screens": lambda: read(watched.track_along(beam, keep_outgoing=False, losses=True, screens=True)),
        "losses": lambda: read(idle.track_along(beam, keep_outgoing=False, losses=True)),
        "screens_4x4": lambda: read(coarse.track_along(beam, keep_outgoing=False, losses=True, screens=True)),
    }
    if once:
        for job in list(jobs.values()) * 2:  # (each kind twice: the second of each is warm)
            job()
        rt.sync()
        return
    res = {"shape": "fodo 64 x 100000 x 128 float32, shared incoming beam, two collimators, two screens of 256 x 256",
           "elements": len(list(idle._leaves()))}
    res.update(alternating(jobs, repeats))
    res["screens_over_losses"] = round(res["screens"]["median_ms"] / res["losses"]["median_ms"], 3)
    res["screens_4x4_over_losses"] = round(res["screens_4x4"]["median_ms"] / res["losses"]["median_ms"], 3)
    trace = watched.track_along(beam, keep_outgoing=False, losses=True, screens=True)
    res["image_megabytes"] = round(sum(im.size for im in trace.screen_images) * 4 / 1e6, 1)
    res["seen_fraction_min_max"] = [[round(float((im.sum(axis=(-2, -1)) / trace.num_survivors[..., k]).min()), 4),
                                     round(float((im.sum(axis=(-2, -1)) / trace.num_survivors[..., k]).max()), 4)]
                                    for k, im in zip(trace.screens, trace.screen_images)]
    res["brightest_pixel_max"] = [int(im.max()) for im in trace.screen_images]
    print(json.dumps(res), flush=True)


def measure_ares(repeats, once):
    res = {"shape": "ares-like 1 x 1000000 x 11 float64, one screen of 2448 x 2040 at the end"}
    for label, shift in (("aligned", (0.0, 0.0)), ("misaligned", (5e-5, -3e-5))):
        segment, screen, beam = ares(misalignment=shift)

        def trace_job():
            return read(segment.track_along(beam, keep_outgoing=False, screens=True))

        def track_job():
            out = segment.track(beam)  # (Beam.empty: the screen swallows the beam and renders it on read)
            return out, screen.reading

        if once:
            trace_job()
            trace_job()
            rt.sync()
            continue
        got = alternating({"trace": trace_job, "track_and_reading": track_job}, repeats)
        image = segment.track_along(beam, keep_outgoing=False, screens=True).image_at("SCREEN")
        segment.track(beam)
        got["same_image"] = bool(np.array_equal(image, screen.reading))
        got["track_over_trace"] = round(got["track_and_reading"]["median_ms"] / got["trace"]["median_ms"], 2)
        got["seen_fraction"] = round(float(image.sum()) / beam.num_particles, 4)
        res[label] = got
    if not once:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fodo", "ares"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.only in (None, "fodo"):
        measure_fodo(args.repeats, args.once)
    if args.only in (None, "ares"):
        measure_ares(args.repeats, args.once)
