"""
`lynx_amd.grad.track_along_jvp` -- forward trace + one forward-mode sweep per direction -- against the way the same numbers
were had before it: one `track_along_vjp` reverse call per OUTPUT, each with its own cotangent assembly and its own
k_build_bwd.  A 128-element FODO line (24 cells; 16 correctors and 16 BPMs in the first 16 of them), a ParameterBeam, B = 64:

  response   the orbit response matrix, 32 readings x 16 correctors: `orbit_response_matrix` (16 directions) against 32 reverse
             calls (a BPM and a plane each) behind one forward trace
  curves     d beta_x, d beta_y at all 129 points along the k1 of 8 quadrupoles: `tangent("beta_x")`, `tangent("beta_y")` of one
             call with 8 directions against 258 reverse calls (a property and a point each) behind one forward trace

Same process, same input, warm; the two ways ALTERNATE, HIP events on the context's stream (lynx_timer_start / _stop) around
each whole job; the median of 7.

    python scripts/gpu/trace_jvp_speed.py [--repeats 7] [--only response|curves] [--dtype float32|float64]

Prints one JSON line per job.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from trace_speed import rt  # noqa: E402


def line(B=64, dtype=np.float32):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    elements = []
    for cell in range(24):
        elements.append(lx.Quadrupole(f(0.2), k1=k, name=f"QF{cell}", dtype=dtype))
        if cell < 16:
            corrector = lx.HorizontalCorrector if cell % 2 == 0 else lx.VerticalCorrector
            elements.append(corrector(f(0.05), angle=f(0.0), name=f"C{cell}", dtype=dtype))
        elements += [lx.Drift(f(0.45 if cell < 16 else 0.5), dtype=dtype), lx.Quadrupole(f(0.2), k1=-k, name=f"QD{cell}", dtype=dtype),
                     lx.Drift(f(0.5), dtype=dtype)]
        if cell < 16:
            elements.append(lx.BPM(name=f"BPM{cell}"))
    beam = lx.ParameterBeam.from_parameters(mu_x=f(1e-4), mu_y=f(-1e-4), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4),
                                            sigma_yp=f(1e-5), energy=f(1e8), dtype=dtype)
    segment = lx.Segment(elements)
    assert len(list(segment._leaves())) == 128
    return segment, beam


def alternate(jobs, repeats, warmup=1):
    """{name: median, min, max in ms} of jobs run in turn, `repeats` rounds."""
    for _ in range(warmup):
        for job in jobs.values():
            job()
    rt.sync()
    times = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, job in jobs.items():
            ms = C.c_float()
            rt.check(rt.lib.lynx_timer_start(rt.ctx))
            job()
            rt.check(rt.lib.lynx_timer_stop(rt.ctx, C.byref(ms)))
            times[name].append(ms.value)
    return {name: {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(min(t)), 3), "max_ms": round(float(max(t)), 3)}
            for name, t in times.items()}


def response(segment, beam, repeats):
    leaves = list(segment._leaves())
    bpms = [el for el in leaves if isinstance(el, lx.BPM)]
    correctors = [el for el in leaves if isinstance(el, (lx.HorizontalCorrector, lx.VerticalCorrector))]
    P = len(leaves) + 1

    def forward_mode():
        return grad.orbit_response_matrix(segment, beam).matrix

    def reverse_mode():
        vjp = grad.track_along_vjp(segment, beam)
        rows = []
        for name in ("mu_x", "mu_y"):
            for bpm in bpms:
                weights = np.zeros(P)
                weights[leaves.index(bpm)] = 1.0
                g = vjp(**{name: weights})
                rows.append(np.stack([np.asarray(g[c]["angle"], dtype=np.float64) for c in correctors], axis=-1))
        return np.stack(rows, axis=-2)

    a, b = forward_mode(), reverse_mode()
    worst = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    out = alternate({"orbit_response_matrix": forward_mode, "reverse_call_per_reading": reverse_mode}, repeats)
    return {"job": "response", "readings": 2 * len(bpms), "correctors": len(correctors), "largest_difference": worst, **out,
            "reverse_over_forward": round(out["reverse_call_per_reading"]["median_ms"] / out["orbit_response_matrix"]["median_ms"], 2)}


def curves(segment, beam, repeats):
    leaves = list(segment._leaves())
    quadrupoles = [el for el in leaves if isinstance(el, lx.Quadrupole)][:16:2]
    P = len(leaves) + 1

    def forward_mode():
        jvp = grad.track_along_jvp(segment, beam, [(q, "k1") for q in quadrupoles])
        return np.stack([jvp.tangent("beta_x"), jvp.tangent("beta_y")])

    def reverse_mode():
        vjp = grad.track_along_vjp(segment, beam)
        out = np.zeros((2, *beam.batch_shape, len(quadrupoles), P))
        for i, name in enumerate(("beta_x", "beta_y")):
            for k in range(P):
                weights = np.zeros(P)
                weights[k] = 1.0
                g = vjp(**{name: weights})
                out[i, ..., k] = np.stack([np.asarray(g[q]["k1"], dtype=np.float64) for q in quadrupoles], axis=-1)
        return out

    a, b = forward_mode(), reverse_mode()
    worst = float(np.max(np.abs(a - b) / (np.abs(b) + 1e-3 * np.max(np.abs(b)))))
    out = alternate({"track_along_jvp": forward_mode, "reverse_call_per_output": reverse_mode}, repeats)
    return {"job": "curves", "directions": len(quadrupoles), "outputs": 2 * P, "largest_distance": worst, **out,
            "reverse_over_forward": round(out["reverse_call_per_output"]["median_ms"] / out["track_along_jvp"]["median_ms"], 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("response", "curves"))
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    segment, beam = line(dtype=np.dtype(args.dtype).type)
    shape = {"elements": 128, "batch": list(beam.batch_shape), "dtype": beam.dtype.name}
    if args.only in (None, "response"):
        print(json.dumps({**shape, **response(segment, beam, args.repeats)}), flush=True)
    if args.only in (None, "curves"):
        print(json.dumps({**shape, **curves(segment, beam, args.repeats)}), flush=True)
