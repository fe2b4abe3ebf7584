"""
`lynx_amd.grad.orbit_response_matrix(..., cavities=True)` -- forward trace, the energy tangents, the entries' tangent rows and
one forward-mode sweep per corrector THROUGH the cavities -- against the way the same matrix was had before it, one
`track_along_vjp` reverse call per reading, and against the plain forward-mode call on the same line with its cavities switched
off (drifts in their places): what walking through the cavities costs.  A 128-element FODO line (26 cells; 16 correctors, 8
BPMs and 8 cavities of 10 MV in the first 16 of them), a ParameterBeam of 100 MeV, B = 64: the 16 x 16 response matrix.

Same process, same input, warm; the three ways ALTERNATE, HIP events on the context's stream (lynx_timer_start / _stop) around
each whole job; the median of 7.

    python scripts/gpu/trace_jvp_cavities_speed.py [--repeats 7] [--dtype float32|float64]

Prints one JSON line.
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
from trace_jvp_speed import alternate  # noqa: E402


def line(B=64, dtype=np.float32, cavities=True):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    k = (4.2 * np.linspace(0.6, 1.1, B)).astype(dtype)
    elements = []
    for cell in range(26):
        elements.append(lx.Quadrupole(f(0.2), k1=k, name=f"QF{cell}", dtype=dtype))
        if cell < 16:
            corrector = lx.HorizontalCorrector if cell % 2 == 0 else lx.VerticalCorrector
            elements.append(corrector(f(0.05), angle=f(0.0), name=f"C{cell}", dtype=dtype))
        elements += [lx.Drift(f(0.45 if cell < 16 else 0.5), dtype=dtype), lx.Quadrupole(f(0.2), k1=-k, name=f"QD{cell}", dtype=dtype)]
        if cell < 16 and cell % 2 == 0 and cavities:
            elements.append(lx.Cavity(f(0.5), voltage=f(1e7), phase=f(-5.0), frequency=f(1.3e9), name=f"ACC{cell}", dtype=dtype))
        else:
            elements.append(lx.Drift(f(0.5), dtype=dtype))
        if cell < 16 and cell % 2 == 1:
            elements.append(lx.BPM(name=f"BPM{cell}"))
    beam = lx.ParameterBeam.from_parameters(mu_x=f(1e-4), mu_y=f(-1e-4), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4),
                                            sigma_yp=f(1e-5), energy=f(1e8), dtype=dtype)
    segment = lx.Segment(elements)
    assert len(list(segment._leaves())) == 128
    return segment, beam


def response(dtype, repeats):
    segment, beam = line(dtype=dtype)
    without, _ = line(dtype=dtype, cavities=False)
    leaves = list(segment._leaves())
    bpms = [el for el in leaves if isinstance(el, lx.BPM)]
    correctors = [el for el in leaves if isinstance(el, (lx.HorizontalCorrector, lx.VerticalCorrector))]
    P = len(leaves) + 1

    def through_cavities():
        return grad.orbit_response_matrix(segment, beam, cavities=True).matrix

    def cavities_off():
        return grad.orbit_response_matrix(without, beam).matrix

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

    a, b = through_cavities(), reverse_mode()
    worst = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    out = alternate({"through_cavities": through_cavities, "cavities_off_plain_call": cavities_off, "reverse_call_per_reading": reverse_mode}, repeats)
    median = lambda name: out[name]["median_ms"]  # noqa: E731
    return {"job": "response", "elements": 128, "cavities": 8, "batch": list(beam.batch_shape), "dtype": beam.dtype.name,
            "readings": 2 * len(bpms), "correctors": len(correctors), "largest_difference_from_reverse_mode": worst, **out,
            "reverse_over_forward": round(median("reverse_call_per_reading") / median("through_cavities"), 2),
            "through_over_plain": round(median("through_cavities") / median("cavities_off_plain_call"), 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    print(json.dumps(response(np.dtype(args.dtype).type, args.repeats)), flush=True)
