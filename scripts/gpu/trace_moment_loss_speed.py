"""
What a step of a tuning loop on a trace costs with the loss formed on the device, `track_along_vjp(..., moment_targets=)`,
against the existing way of the same loss: the trace read back, 2 w (value - target) formed in numpy for every point and
passed as the properties' cotangents.  Forward + reverse of one step, gradients and loss read back, at four shapes:

  a   64 x 100 000 x 128 FODO, float32 ParticleBeam (one incoming beam shared by the batch): sigma_x, sigma_y at all 129 points
  b   1 x 1 000 000 x 11 ARES-like, float64 ParticleBeam: sigma_x, sigma_y behind its three markers
  c   the 13-element ARES experimental area, float32 ParameterBeam, 300 000 settings: beta_x, beta_y at two points
  d   config 5's lattice, 4096 x 10 000 x 32, float32 ParticleBeam through its cavities (cavities=True): sigma_x, sigma_y at 3 points

The legs run in one process in the order existing, new, existing, each after its own warm-up; HIP events on the context's
stream around each whole step (lynx_timer_start / _stop), median and spread of `--repeats` steps.  The condition: the new call
is not slower than the existing one beyond the larger of the spread between the two existing legs and 3 % of their mean.  The
new kernels' own times are those of lynx_profile_launches around the forward call and the reverse call alone.

    python scripts/gpu/trace_moment_loss_speed.py [--repeats 7] [--only a|b|c|d]

Prints one JSON line per shape.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from trace_speed import ares, fodo, gpu_ms, rt  # noqa: E402


def ares_area(B=300_000, dtype=np.float32):
    from trace_screens_grad_speed import ares as area, beam_of

    return area(B, 1, False, dtype), beam_of(B, dtype)


def config5():
    from trace_cavities_grad_speed import config5 as lattice

    return lattice()


def step_jobs(segment, beam, names, points, keywords):
    """(the existing step, the new step, the MomentTargets): targets 0.9 of the values of a first trace, weights 1 / target^2."""
    leaves = list(segment._leaves())
    first = grad.track_along_vjp(segment, beam, **keywords)
    trace = first.trace
    points = [trace.index_of(k) for k in points]
    B, P = int(np.prod(beam.batch_shape)), trace.num_points
    target = {name: 0.9 * np.asarray(getattr(trace, name), dtype=np.float64)[..., points] for name in names}  # (*batch, Q)
    weight = {name: 1.0 / target[name] ** 2 for name in names}
    probe = first(**{name: 1.0 for name in names})
    differentiable = [el for el in leaves if el in probe]
    targets = grad.MomentTargets({k: {name: target[name][..., q] for name in names} for q, k in enumerate(points)},
                                 {k: {name: weight[name][..., q] for name in names} for q, k in enumerate(points)})

    def existing():
        vjp = grad.track_along_vjp(segment, beam, **keywords)
        bars, loss = {}, np.zeros(beam.batch_shape)
        for name in names:
            value = np.asarray(getattr(vjp.trace, name), dtype=np.float64)[..., points]
            bar = np.zeros((*beam.batch_shape, P))
            bar[..., points] = 2.0 * weight[name] * (value - target[name])
            bars[name] = bar
            loss = loss + np.sum(weight[name] * (value - target[name]) ** 2, axis=-1)
        g = vjp(**bars)
        return loss, [g[el] for el in differentiable], g.energy

    def new():
        vjp = grad.track_along_vjp(segment, beam, moment_targets=targets, **keywords)
        loss = vjp.moment_loss
        g = vjp(moment_loss_bar=1.0)
        return loss, [g[el] for el in differentiable], g.energy

    return existing, new, targets, differentiable, B


def kernel_times(segment, beam, targets, keywords, repeats):
    """Milliseconds of the new kernels' launches: (forward call: its chunks and the finish, reverse call: its chunks), medians."""
    def profiled(job):
        rt.sync()
        rt.profile_begin()
        job()
        rt.sync()
        rt.profile_end()
        return rt.profile_launches()

    forward, reverse = [], []
    vjp = grad.track_along_vjp(segment, beam, moment_targets=targets, **keywords)
    loss = vjp._moment_loss  # (the `MomentLoss` of lynx_amd/grad/targets.py: both halves' arguments, the forward half's launch)
    for _ in range(repeats):
        forward.append(sum(profiled(lambda: loss.forward(rt))))
        ml = rt.to_device(np.ones(int(np.prod(beam.batch_shape))))
        args = loss.arguments(rt)
        B, P = vjp._points_shape()
        states = vjp.trace._device
        if "records" in states:
            buffers = (rt.empty((B, P, 36), np.float64), None, None)
        else:
            buffers = (None, rt.empty((B, P, 7), beam.dtype), rt.empty((B, P, 7, 7), beam.dtype))
        energy_bar = rt.empty((B, P), beam.dtype)
        for block in (*buffers, energy_bar):
            if block is not None:
                rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(block.ptr), 0, block.nbytes))
        p = lambda a: None if a is None else C.c_void_p(a.ptr)  # noqa: E731
        reverse.append(sum(profiled(lambda: rt.check(rt.lib.lynx_moments_along_loss_backward(
            *args, p(ml), *(p(b) for b in buffers), p(energy_bar))))))
    return round(float(np.median(forward)), 4), round(float(np.median(reverse)), 4)


def measure(label, segment, beam, names, points, repeats, **keywords):
    existing, new, targets, differentiable, B = step_jobs(segment, beam, names, points, keywords)
    res = {"shape": label, "batch": list(beam.batch_shape), "elements": len(list(segment._leaves())), "dtype": beam.dtype.name,
           "properties": list(names), "target_points": len(points), "differentiable_elements": len(differentiable)}
    res["existing_1"] = gpu_ms(existing, repeats)
    res["new"] = gpu_ms(new, repeats)
    res["existing_2"] = gpu_ms(existing, repeats)
    a, b, n = res["existing_1"]["median_ms"], res["existing_2"]["median_ms"], res["new"]["median_ms"]
    mean = 0.5 * (a + b)
    res["allowance_ms"] = round(max(abs(a - b), 0.03 * mean), 4)
    res["existing_over_new"] = round(mean / n, 3)
    res["not_slower"] = bool(n <= mean + res["allowance_ms"])
    # the same loss and the same gradients, at the sizes timed (float32: the trace's property is rounded, the device's value is not)
    loss_old, grads_old, energy_old = existing()
    loss_new, grads_new, energy_new = new()
    res["loss_relative_difference"] = float(np.max(np.abs(loss_new - loss_old) / np.abs(loss_old)))
    worst = 0.0
    for g_old, g_new in zip(grads_old, grads_new):
        for name in g_old:
            scale = np.max(np.abs(g_old[name]))
            if scale > 0:
                worst = max(worst, float(np.max(np.abs(np.asarray(g_new[name], dtype=np.float64) - g_old[name])) / scale))
    res["gradient_relative_difference"] = worst
    res["forward_kernels_ms"], res["reverse_kernels_ms"] = kernel_times(segment, beam, targets, keywords, repeats)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("a", "b", "c", "d"))
    args = ap.parse_args()
    if args.only in (None, "a"):
        segment, beam = fodo()
        measure("a: fodo 64 x 100000 x 128 float32, shared incoming beam, all 129 points", segment, beam, ("sigma_x", "sigma_y"),
                list(range(129)), args.repeats)
    if args.only in (None, "b"):
        segment, beam = ares()
        measure("b: ares-like 1 x 1000000 x 11 float64, three markers", segment, beam, ("sigma_x", "sigma_y"), [1, 3, 11], args.repeats)
    if args.only in (None, "c"):
        segment, beam = ares_area()
        measure("c: ARES area, 13 elements, ParameterBeam, 300000 settings float32, two points", segment, beam, ("beta_x", "beta_y"),
                ["Q3", -1], args.repeats)
    if args.only in (None, "d"):
        segment, beam = config5()
        measure("d: config 5, 4096 x 10000 x 32 float32, cavities=True, three points", segment, beam, ("sigma_x", "sigma_y"),
                [8, 16, 32], args.repeats, cavities=True)
