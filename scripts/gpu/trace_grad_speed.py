"""
`lynx_amd.grad.track_along_vjp` -- forward trace + reverse sweep, with `beta_x`, `beta_y` cotangents at every point --
against the only way the same gradient could be had before it: one `track_vjp` per point on a prefix of the lattice,
`Segment(leaves[:k])` for every point k (P forward passes over the particles, P reverse passes, P map builds), with
cotangents on the six moments beta is written in.  Same process, same input, warm.  HIP events on the context's stream
(lynx_timer_start / _stop) around each whole job, warm-up first, several repeats: median and spread.

    python scripts/gpu/trace_grad_speed.py [--repeats 7] [--only fodo|ares|scan] [--what along|prefix] [--once]

`scan` is the README's ARES `ParameterBeam` scan, 300 000 settings x 11 elements, float32 (no prefix loop: `--what along`).

Prints one JSON line per shape.  `--once`: one warm `track_along_vjp` job per shape and nothing else (for a profiler run).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from trace_speed import ares, fodo, gpu_ms, rt  # noqa: E402

BETA_MOMENTS = ("sigma_x", "sigma_xp", "sigma_xxp", "sigma_y", "sigma_yp", "sigma_yyp")


def measure(name, segment, beam, repeats, what, once):
    leaves = list(segment._leaves())
    probe = grad.track_along_vjp(segment, beam)(beta_x=1.0)
    differentiable = [el for el in leaves if el in probe]

    def along():
        g = grad.track_along_vjp(segment, beam)(beta_x=1.0, beta_y=1.0)
        return [g[el] for el in differentiable], g.energy

    if once:
        along()
        along()
        rt.sync()
        return
    res = {"shape": name, "elements": len(leaves), "batch": list(beam.batch_shape), "particles": getattr(beam, "num_particles", None),
           "dtype": beam.dtype.name}
    if what in (None, "along"):
        res["track_along_vjp"] = gpu_ms(along, repeats)
    if what in (None, "prefix"):
        prefixes = [lx.Segment(leaves[:k]) for k in range(1, len(leaves) + 1)]
        bars = {key: 1.0 for key in BETA_MOMENTS}
        whole = beam.materialized()  # (track_vjp indexes the particles per sample: made once, outside the timed job)

        def prefix_loop():
            out = []
            for prefix in prefixes:
                g = grad.track_vjp(prefix, whole)(**bars)
                out.append([g[el] for el in prefix.elements if el in g])
            return out

        res["prefix_loop_of_track_vjp"] = gpu_ms(prefix_loop, max(3, repeats // 2), warmup=1)
    if "track_along_vjp" in res and "prefix_loop_of_track_vjp" in res:
        res["prefix_over_along"] = round(res["prefix_loop_of_track_vjp"]["median_ms"] / res["track_along_vjp"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


def ares_scan(B=300_000, dtype=np.float32):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    angle = np.linspace(-1e-3, 1e-3, B).astype(dtype)
    segment = lx.Segment([
        lx.BPM(), lx.Drift(f(1.0), dtype=dtype), lx.BPM(), lx.Drift(f(1.0), dtype=dtype),
        lx.VerticalCorrector(f(0.3), angle=angle, dtype=dtype), lx.Drift(f(0.2), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=-angle, dtype=dtype), lx.Drift(f(7.0), dtype=dtype),
        lx.HorizontalCorrector(f(0.3), angle=angle, dtype=dtype), lx.Drift(f(0.05), dtype=dtype), lx.BPM()])
    beam = lx.ParameterBeam.from_parameters(sigma_x=f(1.75e-4), sigma_xp=f(3.7e-6), sigma_y=f(1.75e-4), sigma_yp=f(3.7e-6),
                                            energy=f(1e8), dtype=dtype)
    return segment, beam


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fodo", "ares", "scan"))
    ap.add_argument("--what", choices=("along", "prefix"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.only in (None, "fodo"):
        measure("fodo 64 x 100000 x 128 float32, shared incoming beam", *fodo(), args.repeats, args.what, args.once)
    if args.only in (None, "ares"):
        measure("ares-like 1 x 1000000 float64", *ares(), args.repeats, args.what, args.once)
    if args.only == "scan":
        measure("ares-like ParameterBeam scan 300000 x 11 float32", *ares_scan(), args.repeats, "along", args.once)
