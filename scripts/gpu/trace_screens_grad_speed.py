"""
What the gradient of a screen image costs: `track_along_vjp(segment, parameter_beam, screens=True)` and one reverse call with
a mean-squared-error cotangent on the image, against the nearest thing that could be done without it --
`track_along(beam, screens=True)` for the image plus `track_along_vjp` with a `cov_bar` on the same lattice with the screen
inactive (the adjoint of the density itself then still had to be written by hand, on the host).

  ares1   64 samples x the 13-element ARES experimental area, float32, its screen at binning 1 (2448 x 2040 pixels)
  ares4   the same at binning 4 (612 x 511)
  many    1024 samples x the same lattice with a screen of 612 x 511

Call timing: HIP events on the context's stream (lynx_timer_start / _stop) around each whole job -- forward launches, the
read-back of the images, the cotangent formed in numpy, its upload, the reverse launches, the gradients read --, the two
jobs ALTERNATING in one process, warm-up first, median and spread of `--repeats` runs.

Kernel timing: the same events around lynx_gaussian_images_along_backward alone (its reduction and finishing kernels, the
cotangent already on the device), the bytes of `d_images_bar` it reads, that rate, and the plain-copy rate of the same run
(`Runtime.copy_bandwidth`, read + write bytes, best launch shape) beside it.

    python scripts/gpu/trace_screens_grad_speed.py [--repeats 5] [--only ares1|ares4|many]

Prints one JSON line per case.
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
from lynx_amd import engine  # noqa: E402
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


def alternating(jobs, repeats, warmup=1):
    for _ in range(warmup):
        for job in jobs.values():
            job()
    rt.sync()
    times = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, job in jobs.items():
            times[name].append(timed(job))
    return {name: summary(t) for name, t in times.items()}


def ares(B, binning, active, dtype=np.float32, k1=(10.0, -9.0, 6.0)):
    """The ARES experimental area: three quadrupoles, two correctors, the screen at its end; the strengths scanned over the batch."""
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    scan = np.linspace(0.9, 1.1, B).astype(dtype)
    drift = lambda length: lx.Drift(f(length), dtype=dtype)  # noqa: E731
    quad = lambda k, name: lx.Quadrupole(f(0.122), k1=(k * scan).astype(dtype), name=name, dtype=dtype)  # noqa: E731
    screen = lx.Screen(resolution=(2448, 2040), pixel_size=(3.3198e-6, 2.4469e-6), binning=binning, misalignment=np.zeros(2, dtype=dtype),
                       is_active=active, name="SCREEN", dtype=dtype)
    return lx.Segment([
        lx.Marker(name="AREASOLA1"), drift(0.17504), quad(k1[0], "Q1"), drift(0.428), quad(k1[1], "Q2"), drift(0.204),
        lx.VerticalCorrector(f(0.02), angle=f(1e-4), name="CV", dtype=dtype), drift(0.204), quad(k1[2], "Q3"), drift(0.179),
        lx.HorizontalCorrector(f(0.02), angle=f(-1e-4), name="CH", dtype=dtype), drift(0.45), screen])


def beam_of(B, dtype=np.float32):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    return lx.ParameterBeam.from_parameters(sigma_x=f(175e-6), sigma_xp=f(2e-6), sigma_y=f(175e-6), sigma_yp=f(2e-6), sigma_s=f(1e-6),
                                            sigma_p=f(1e-6), energy=f(1e8), dtype=dtype)


def measure(label, B, binning, repeats):
    dtype = np.float32
    watched, idle, elsewhere, beam = ares(B, binning, True), ares(B, binning, False), ares(1, binning, True, k1=(9.0, -8.0, 6.5)), beam_of(B)
    target = np.asarray(elsewhere.track_along(beam_of(1), screens=True).image_at("SCREEN"))  # (1, nx, ny): one target for all samples
    P = len(list(watched._leaves())) + 1
    cov_bar = np.zeros((B, P, 6, 6))
    cov_bar[:, -1, 0, 0] = cov_bar[:, -1, 2, 2] = 1.0

    def new():
        vjp = grad.track_along_vjp(watched, beam, screens=True)
        image = vjp.trace.image_at("SCREEN")
        g = vjp(screen_images_bar={"SCREEN": (image - target) * dtype(2.0 / image[0].size)})
        return g[watched.Q1]["k1"], g[watched.CH]["angle"], g.mu

    def before():
        image = watched.track_along(beam, screens=True).image_at("SCREEN")
        g = grad.track_along_vjp(idle, beam)(cov_bar=cov_bar)
        return image, g[idle.Q1]["k1"], g[idle.CH]["angle"], g.mu

    res = {"case": label, "shape": f"{B} samples x 13 elements float32, screen at binning {binning}"}
    res.update(alternating({"image_gradient": new, "image_and_cov_bar_gradient": before}, repeats))
    res["new_over_before"] = round(res["image_gradient"]["median_ms"] / res["image_and_cov_bar_gradient"]["median_ms"], 3)
    # the kernel alone
    vjp = grad.track_along_vjp(watched, beam, screens=True)
    image = vjp.trace.image_at("SCREEN")
    res["pixels"] = [int(n) for n in image.shape[-2:]]
    shots = engine._screen_geometry(watched, vjp.program, beam.batch_shape, dtype, rt, False)
    w_dev = rt.to_device(np.ascontiguousarray(((image - target) * dtype(2.0 / image[0].size)).reshape(B, -1), dtype=dtype))
    mb, cb, shifts = rt.to_device(np.zeros((B, P, 7), dtype)), rt.to_device(np.zeros((B, P, 7, 7), dtype)), rt.empty((B, 1, 2), dtype)
    states = vjp.trace._device
    p = lambda a: C.c_void_p(a.ptr)  # noqa: E731

    def kernel():
        rt.check(rt.lib.lynx_gaussian_images_along_backward(
            rt.ctx, engine.dtype_code(dtype), B, P, p(states["mu"]), p(states["cov"]), shots["count"], shots["rows"], p(shots["grid"]),
            p(shots["misalignment"]), shots["stride"], p(w_dev), p(mb), p(cb), p(shifts)))

    kernel()
    rt.sync()
    res["kernel"] = summary([timed(kernel) for _ in range(max(repeats, 5))])
    nbytes = B * shots["cells"] * 4
    res["images_bar_megabytes"] = round(nbytes / 1e6, 1)
    res["kernel_read_gb_per_s"] = round(nbytes / (res["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
    res["plain_copy_gb_per_s_read_plus_write"] = round(max(rt.copy_bandwidth(min(nbytes, 1 << 30)).values()), 1)
    print(json.dumps(res), flush=True)


CASES = {"ares1": (64, 1), "ares4": (64, 4), "many": (1024, 4)}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=tuple(CASES))
    args = ap.parse_args()
    for label, (B, binning) in CASES.items():
        if args.only in (None, label):
            measure(label, B, binning, args.repeats)
