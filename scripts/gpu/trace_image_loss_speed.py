"""
What the image loss on the device saves: `track_along_vjp(segment, parameter_beam, image_targets=targets)` and one reverse call
with `image_loss_bar` -- no image made, read back or uploaded, the targets resident on the device -- against the existing
call of the same job, `track_along_vjp(..., screens=True)` with the cotangent 2 (img - target) / n formed in numpy.

  ares1   64 samples x the 13-element ARES experimental area, float32, its screen at binning 1 (2448 x 2040 pixels)
  ares4   the same at binning 4 (612 x 511)
  many    1024 samples x the same lattice with a screen of 612 x 511
  own     ares1 with a target per sample: the target is a read of 1.28 GB (new call and forward entry alone)

Call timing: HIP events on the context's stream (lynx_timer_start / _stop) around each whole job -- forward launches, the
reverse launches, the gradients and the loss read; for the existing call also the read-back of the images, the cotangent
formed in numpy and its upload --, the two jobs ALTERNATING in one process, warm-up first, median and spread of `--repeats`
runs (the method of trace_screens_grad_speed.py, whose lattice and beam these are).

Kernel timing: the same events around lynx_gaussian_images_along_mse alone (its reduction and finishing kernels, the targets
already on the device) and, in the same job, around lynx_gaussian_images_along_backward alone: both evaluate the same float64
`exp` per pixel on the same pixels.  For a target per sample, the bytes of `d_targets` read, that rate, and the plain-copy rate
of the same run (`Runtime.copy_bandwidth`, read + write bytes, best launch shape) beside it.

    python scripts/gpu/trace_image_loss_speed.py [--repeats 3] [--only ares1|ares4|many|own]

Prints one JSON line per case.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import lynx_amd.grad as grad  # noqa: E402
from lynx_amd import engine  # noqa: E402
from trace_screens_grad_speed import alternating, ares, beam_of, rt, summary, timed  # noqa: E402


def measure(label, B, binning, repeats, own_targets=False):
    dtype = np.float32
    watched, elsewhere, beam = ares(B, binning, True), ares(1, binning, True, k1=(9.0, -8.0, 6.5)), beam_of(B)
    target = np.asarray(elsewhere.track_along(beam_of(1), screens=True).image_at("SCREEN"))[0]  # (nx, ny): one target for all samples
    given = np.broadcast_to(target, (B, *target.shape)) if own_targets else target
    targets = grad.ImageTargets({"SCREEN": given})  # (uploaded by the warm-up pass, resident from then on)
    P = len(list(watched._leaves())) + 1

    def new():
        vjp = grad.track_along_vjp(watched, beam, image_targets=targets)
        g = vjp(image_loss_bar=1.0)
        return vjp.image_loss_of("SCREEN"), g[watched.Q1]["k1"], g[watched.CH]["angle"], g.mu

    def existing():
        vjp = grad.track_along_vjp(watched, beam, screens=True)
        image = vjp.trace.image_at("SCREEN")
        g = vjp(screen_images_bar={"SCREEN": (image - target) * dtype(2.0 / image[0].size)})
        return g[watched.Q1]["k1"], g[watched.CH]["angle"], g.mu

    res = {"case": label, "shape": f"{B} samples x 13 elements float32, screen at binning {binning}",
           "targets": "one per sample" if own_targets else "one, shared by the batch"}
    jobs = {"image_loss_on_device": new} if own_targets else {"image_loss_on_device": new, "screens_and_numpy_cotangent": existing}
    res.update(alternating(jobs, repeats))
    if not own_targets:
        old, now = res["screens_and_numpy_cotangent"], res["image_loss_on_device"]
        res["existing_over_new"] = round(old["median_ms"] / now["median_ms"], 1)
        res["existing_spread_ms"] = round(old["max_ms"] - old["min_ms"], 4)
        res["saved_ms"] = round(old["median_ms"] - now["median_ms"], 4)
    # the forward entry alone, and the existing adjoint alone in the same job
    vjp = grad.track_along_vjp(watched, beam, image_targets=targets)
    shots = engine._screen_geometry(watched, vjp.program, beam.batch_shape, dtype, rt, False)
    res["pixels"] = [int(n) for n in shots["shapes"][0]]
    layout = targets._layout(vjp.program, vjp.leaves, beam)
    t_dev = targets._device(rt, layout)
    states = vjp.trace._device
    loss, sums = rt.empty((B, 1), np.float64), rt.empty((B, 1, 6), np.float64)
    p = lambda a: C.c_void_p(a.ptr)  # noqa: E731

    def forward_entry():
        rt.check(rt.lib.lynx_gaussian_images_along_mse(
            rt.ctx, engine.dtype_code(dtype), B, P, p(states["mu"]), p(states["cov"]), shots["count"], shots["rows"], p(shots["grid"]),
            p(shots["misalignment"]), shots["stride"], (C.c_int64 * 1)(*layout.offsets), p(t_dev), layout.stride, p(loss), p(sums)))

    forward_entry()
    rt.sync()
    res["forward_entry"] = summary([timed(forward_entry) for _ in range(max(repeats, 5))])
    res["pixels_per_second"] = float(f"{B * shots['cells'] / (res['forward_entry']['median_ms'] * 1e-3):.3g}")
    if own_targets:
        nbytes = B * shots["cells"] * 4
        res["targets_megabytes"] = round(nbytes / 1e6, 1)
        res["forward_entry_read_gb_per_s"] = round(nbytes / (res["forward_entry"]["median_ms"] * 1e-3) / 1e9, 1)
        res["plain_copy_gb_per_s_read_plus_write"] = round(max(rt.copy_bandwidth(min(nbytes, 1 << 30)).values()), 1)
    else:
        w_dev = rt.to_device(np.ones((B, shots["cells"]), dtype=dtype))
        mb, cb, shifts = rt.to_device(np.zeros((B, P, 7), dtype)), rt.to_device(np.zeros((B, P, 7, 7), dtype)), rt.empty((B, 1, 2), dtype)

        def adjoint_entry():
            rt.check(rt.lib.lynx_gaussian_images_along_backward(
                rt.ctx, engine.dtype_code(dtype), B, P, p(states["mu"]), p(states["cov"]), shots["count"], shots["rows"], p(shots["grid"]),
                p(shots["misalignment"]), shots["stride"], p(w_dev), p(mb), p(cb), p(shifts)))

        adjoint_entry()
        rt.sync()
        res["existing_adjoint_entry"] = summary([timed(adjoint_entry) for _ in range(max(repeats, 5))])
        res["forward_over_adjoint"] = round(res["forward_entry"]["median_ms"] / res["existing_adjoint_entry"]["median_ms"], 3)
    print(json.dumps(res), flush=True)


CASES = {"ares1": (64, 1, False), "ares4": (64, 4, False), "many": (1024, 4, False), "own": (64, 1, True)}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=tuple(CASES))
    args = ap.parse_args()
    for label, (B, binning, own) in CASES.items():
        if args.only in (None, label):
            measure(label, B, binning, args.repeats, own)
