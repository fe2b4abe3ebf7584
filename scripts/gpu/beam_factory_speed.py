"""
What making a beam on the device costs.

  generator  `lynx_fill_gaussian_rows` (one mean and one covariance factor per sample) against `lynx_fill_gaussian`
             (`ParticleBeam.synthetic`: one mu and sigma for all, no correlations) writing the same array, in the order
             synthetic, rows, synthetic; then the two Python calls `ParticleBeam.synthetic` and
             `from_parameters(on_device=True)`; and the best plain-copy rate of the same job for the bytes written.
             64 x 100 000 in float32 and float64, 1024 x 100 000 in float32.
  rescale    `lynx_transform_particles` against `lynx_diag_copy` of the same bytes (one read, one write), in the order copy,
             rescale, copy; then `transformed_to(on_device=True)`.  64 x 100 000 float32 and 1 x 1 000 000 float64.
  host       wall time until the beam is in HBM: `from_twiss` and `transformed_to` on the host path against
             `on_device=True`, 64 x 100 000 float32.  (The host path at 1024 samples is not run.)

Allowed between two legs of the same thing is the larger of their spread and 3 % of their mean; `outside_by` says by how
much of that allowance the new kernel's median lies beyond the slower leg (negative: inside or faster).

Every step is a process of its own under its own `timeout`; the first one that fails ends the run.

    python scripts/gpu/beam_factory_speed.py [--repeats 9]

Prints one JSON line per step.
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

# step -> (seconds allowed, arguments)
STEPS = {
    "generator_f32_64": (120, dict(kind="generator", B=64, N=100_000, dtype="float32")),
    "generator_f64_64": (120, dict(kind="generator", B=64, N=100_000, dtype="float64")),
    "generator_f32_1024": (240, dict(kind="generator", B=1024, N=100_000, dtype="float32")),
    "rescale_f32_64": (120, dict(kind="rescale", B=64, N=100_000, dtype="float32")),
    "rescale_f64_1": (120, dict(kind="rescale", B=1, N=1_000_000, dtype="float64")),
    "host_f32_64": (300, dict(kind="host", B=64, N=100_000, dtype="float32")),
}


def summary(times):
    t = np.sort(np.array(times))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4)}


def verdict(first, new, last):
    """The project's rule: allowed is the larger of the spread of the two reference legs and 3 % of their mean."""
    a, b = first["median_ms"], last["median_ms"]
    allowed = max(abs(a - b), 0.03 * 0.5 * (a + b))
    return {"allowed_ms": round(allowed, 4), "outside_by": round((new["median_ms"] - max(a, b)) / allowed, 2),
            "new_over_reference": round(new["median_ms"] / (0.5 * (a + b)), 3)}


def twiss_arguments(B, dtype):
    s = np.linspace(0.0, 1.0, B)
    return dict(beta_x=(5.0 + 60.0 * s).astype(dtype), alpha_x=(-1.2 + 4.0 * s).astype(dtype),
                emittance_x=(3.5e-9 * (1 + 4 * s)).astype(dtype), beta_y=(75.0 - 70.0 * s).astype(dtype),
                alpha_y=(1.0 - 1.4 * s).astype(dtype), emittance_y=(2.3e-9 * (1 + 3 * s)).astype(dtype),
                sigma_s=(1e-5 * (1 + s)).astype(dtype), sigma_p=(2e-3 / (1 + s)).astype(dtype),
                cor_s=(0.6 * 1e-5 * 2e-3 * np.ones(B)).astype(dtype), energy=np.full(B, 1e8, dtype=dtype))


def run_step(kind, B, N, dtype, repeats):
    import lynx_amd as lx
    from lynx_amd.device import dtype_code, get_runtime
    from lynx_amd.particles.particle_beam import gaussian_rows

    rt = get_runtime()
    dtype = np.dtype(dtype)
    code, nbytes = dtype_code(dtype), B * N * 7 * dtype.itemsize

    def timed(job, n=repeats, warmup=2, launches=1):
        """HIP events around `launches` calls back to back (what lynx_diag_copy does with its `repeats`), per call."""
        out = []
        for i in range(warmup + n):
            rt.timer_start()
            for _ in range(launches):
                job()
            ms = rt.timer_stop()
            if i >= warmup:
                out.append(ms / launches)
        return summary(out)

    def wall(job, n=3):
        out = []
        for _ in range(n):
            rt.sync()
            t0 = time.perf_counter()
            job()
            rt.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return summary(out)

    res = {"step": kind, "shape": f"{B} x {N} {dtype}", "bytes": nbytes}
    tw = twiss_arguments(B, dtype.type)
    if kind == "generator":
        mu = np.array([3e-4, -2e-5, -1e-4, 4e-6, 0.0, 0.0])
        sigma = np.array([1e-4, 1e-5, 2e-4, 2e-5, 1e-5, 1e-3])
        dbl = C.c_double * 6
        arr = rt.empty((B, N, 7), dtype)
        probe = lx.ParticleBeam.from_twiss(num_particles=1, **tw, dtype=dtype, seed=1, on_device=True)  # (shapes checked)
        assert probe.batch_shape == (B,)
        s = np.linspace(0.0, 1.0, B)
        cov = np.zeros((B, 6, 6))
        for at in (0, 2, 4):
            cov[:, at, at], cov[:, at + 1, at + 1] = (sigma[at] * (1 + s)) ** 2, (sigma[at + 1] / (1 + s)) ** 2
            cov[:, at, at + 1] = cov[:, at + 1, at] = (0.8 - 1.6 * s) * sigma[at] * sigma[at + 1]
        d_rows = rt.to_device(gaussian_rows(np.tile(mu, (B, 1)) * (1 + s[:, None]), cov))
        old = lambda: rt.check(rt.lib.lynx_fill_gaussian(rt.ctx, code, B, N, dbl(*mu), dbl(*sigma), C.c_uint64(1),  # noqa: E731
                                                         C.c_void_p(arr.ptr)))
        new = lambda: rt.check(rt.lib.lynx_fill_gaussian_rows(rt.ctx, code, B, N, C.c_void_p(d_rows.ptr), C.c_uint64(1),  # noqa: E731
                                                              C.c_void_p(arr.ptr)))
        res["synthetic_first"], res["rows"], res["synthetic_last"] = (timed(job, launches=3) for job in (old, new, old))
        res.update(verdict(res["synthetic_first"], res["rows"], res["synthetic_last"]))
        del arr
        res["python_synthetic"] = timed(lambda: lx.ParticleBeam.synthetic((B,), N, mu=mu, sigma=sigma, seed=1, dtype=dtype))
        res["python_from_twiss_on_device"] = timed(
            lambda: lx.ParticleBeam.from_twiss(num_particles=N, **tw, dtype=dtype, seed=1, on_device=True))
        copy = rt.copy_bandwidth(min(nbytes, 1 << 30))
        best = max(copy.values())
        res["best_copy_GBps"] = round(best, 1)  # (read + write: the copy writes half of that)
        res["rows_write_GBps"] = round(nbytes / (res["rows"]["median_ms"] * 1e-3) / 1e9, 1)
        res["rows_write_over_copy_write_rate"] = round(res["rows_write_GBps"] / (0.5 * best), 3)
    elif kind == "rescale":
        beam = lx.ParticleBeam.synthetic((B,), N, sigma=[1e-4, 1e-5, 2e-4, 2e-5, 1e-5, 1e-3], seed=1, dtype=dtype)
        src, dst = beam._particles.device(rt), rt.empty((B, N, 7), dtype)
        rows = np.tile(np.array([0.0] * 6 + [1e-4, 1e-5, 2e-4, 2e-5, 1e-5, 1e-3] + [2e-4] * 6 + [1e-5] * 6, dtype=dtype), (B, 1))
        d_rows = rt.to_device(rows)
        ms = C.c_float()

        def copy():
            """The best launch shape of Runtime.copy_bandwidth's five, each timed `repeats` times over 10 launches."""
            legs = []
            for vpt in (1, 4, 0, 101, 104):
                times = []
                for _ in range(repeats):
                    rt.check(rt.lib.lynx_diag_copy(rt.ctx, C.c_void_p(dst.ptr), C.c_void_p(src.ptr), nbytes // 16 * 16, 10,
                                                   vpt, C.byref(ms)))
                    times.append(ms.value)
                legs.append(summary(times))
            return min(legs, key=lambda leg: leg["median_ms"])

        new = lambda: rt.check(rt.lib.lynx_transform_particles(  # noqa: E731
            rt.ctx, code, B, N, C.c_void_p(src.ptr), N * 7, C.c_void_p(d_rows.ptr), C.c_void_p(dst.ptr)))
        res["copy_first"], res["rescale"], res["copy_last"] = copy(), timed(new, launches=10), copy()
        res.update(verdict(res["copy_first"], res["rescale"], res["copy_last"]))
        res["rescale_GBps"] = round(2 * nbytes / (res["rescale"]["median_ms"] * 1e-3) / 1e9, 1)
        del dst
        beam.sigma_x  # (the moment record: made once, as a tuning loop has it from the tracking call)
        target = dict(sigma_x=np.full(B, 2e-4, dtype=dtype), mu_x=np.full(B, 1e-5, dtype=dtype))
        res["python_transformed_to_on_device"] = timed(lambda: beam.transformed_to(**target, on_device=True))
    else:
        res["from_twiss_host"] = wall(
            lambda: lx.ParticleBeam.from_twiss(num_particles=N, **tw, dtype=dtype, seed=1)._particles.device(rt))
        res["from_twiss_on_device"] = wall(
            lambda: lx.ParticleBeam.from_twiss(num_particles=N, **tw, dtype=dtype, seed=1, on_device=True))
        beam = lx.ParticleBeam.from_twiss(num_particles=N, **tw, dtype=dtype, seed=1, on_device=True)
        beam.sigma_x
        target = dict(sigma_x=np.full(B, 2e-4, dtype=dtype), mu_x=np.full(B, 1e-5, dtype=dtype))

        def host():
            beam._particles._host = None  # (a beam that lives in HBM only, as a tracking call leaves it)
            beam.transformed_to(**target)._particles.device(rt)

        res["transformed_to_host"] = wall(host)
        beam._particles._host = None
        res["transformed_to_on_device"] = wall(lambda: beam.transformed_to(**target, on_device=True))
        res["from_twiss_host_over_device"] = round(res["from_twiss_host"]["median_ms"] / res["from_twiss_on_device"]["median_ms"], 1)
        res["transformed_to_host_over_device"] = round(
            res["transformed_to_host"]["median_ms"] / res["transformed_to_on_device"]["median_ms"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step", choices=tuple(STEPS))
    ap.add_argument("--only", nargs="*", choices=tuple(STEPS))
    args = ap.parse_args()
    if args.step:
        run_step(repeats=args.repeats, **STEPS[args.step][1])
        sys.exit(0)
    for name in (args.only or STEPS):  # this process never opens the GPU: each step is a child under its own time limit
        limit = STEPS[name][0]
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", name,
                               "--repeats", str(args.repeats)])
        if done.returncode != 0:
            sys.exit(f"step {name} ended with status {done.returncode}: nothing more is started")
