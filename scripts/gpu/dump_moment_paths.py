"""
Every path of the 7 x 7 moment recursion -- forward in both forms, and the reverse sweeps of `track_vjp` and
`track_along_vjp` (plain, with losses, with trajectories) -- once each on seeded inputs, every returned array written to
DIR/<case>.npz.  Two builds of the library (LYNX_HIP_LIBRARY picks one) are compared array by array with
`np.array_equal(..., equal_nan=True)`: in the spirit of `bench.py --dump-outputs`, for the kernels bench.py does not time.

    python scripts/gpu/dump_moment_paths.py DIR
    python scripts/gpu/dump_moment_paths.py --compare DIR_A DIR_B
"""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(dir_a, dir_b):
    names, differing = sorted(p.name for p in Path(dir_a).glob("*.npz")), []
    assert names and names == sorted(p.name for p in Path(dir_b).glob("*.npz")), "the two directories hold different cases"
    arrays = 0
    for name in names:
        a, b = np.load(Path(dir_a) / name), np.load(Path(dir_b) / name)
        assert sorted(a.files) == sorted(b.files), name
        arrays += len(a.files)
        differing += [f"{name}:{key}" for key in a.files if not np.array_equal(a[key], b[key], equal_nan=True)]
    print(f"{len(names)} cases, {arrays} arrays, {len(differing)} differ" + "".join(f"\n  {d}" for d in differing))
    return 1 if differing else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402

out_dir = Path(sys.argv[1])
out_dir.mkdir(parents=True, exist_ok=True)
rt = lx.device.get_runtime()
SIGMA = [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]


def cavities(B, dtype):
    """Eight elements, two active cavities (tests/test_gpu_trace.py), the BPM inactive (track_vjp: one stretch), and its beam."""
    rng = np.random.default_rng(9)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    u = lambda lo, hi: rng.uniform(lo, hi, B).astype(dtype)  # noqa: E731
    cavity = lambda phase: lx.Cavity(f(1.0377), voltage=u(5e6, 2e7), phase=phase, frequency=f(1.3e9), dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(0.6), dtype=dtype), lx.Quadrupole(f(0.2), k1=u(-5, 5), dtype=dtype), cavity(u(-10, 10)),
                          lx.BPM(is_active=False), lx.Drift(f(0.4), dtype=dtype), lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=dtype),
                          cavity(f(0.0)), lx.Dipole(f(0.5), angle=f(0.1), dtype=dtype)])
    beam = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(1e-4), sigma_yp=f(1e-5), sigma_s=f(1e-5),
                                            sigma_p=f(1e-3), mu_x=rng.normal(0, 1e-4, B).astype(dtype), energy=f(6e6), dtype=dtype)
    return segment, beam


def affine(B, dtype):
    """A cavity-free lattice of mixed kinds and 1000 particles per sample."""
    rng = np.random.default_rng(4)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    u = lambda lo, hi: rng.uniform(lo, hi, B).astype(dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(0.6), dtype=dtype), lx.Quadrupole(f(0.2), k1=u(-5, 5), tilt=u(-1, 1), dtype=dtype),
                          lx.HorizontalCorrector(f(0.1), angle=u(1e-4, 2e-3), dtype=dtype), lx.Dipole(f(0.5), angle=u(0.1, 0.2), dtype=dtype),
                          lx.VerticalCorrector(f(0.1), angle=u(-2e-3, -1e-4), dtype=dtype), lx.Solenoid(f(0.3), k=u(-2, 2), dtype=dtype),
                          lx.Drift(f(0.4), dtype=dtype)])
    return segment, lx.ParticleBeam.synthetic((B,), 1000, sigma=SIGMA, energy=1e8, seed=3, dtype=dtype)


def collimated(dtype):
    """Drift, aperture, quadrupole, aperture, drift; batch 2, 64 particles: each aperture takes some particles, not all."""
    f = lambda v: np.full(2, v, dtype=dtype)  # noqa: E731
    aperture = lambda name, limit: lx.Aperture(x_max=f(limit), y_max=f(limit), is_active=True, name=name, dtype=dtype)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(1.0), dtype=dtype), aperture("A0", 1.5e-4), lx.Quadrupole(f(0.2), k1=f(1.0), dtype=dtype),
                          aperture("A1", 1.0e-4), lx.Drift(f(1.0), dtype=dtype)])
    return segment, lx.ParticleBeam.synthetic((2,), 64, sigma=SIGMA, energy=1e8, seed=1, dtype=dtype)


def gradients(g, segment):
    out = {f"{k}.{name}": v for k, el in enumerate(segment._leaves()) if el in g for name, v in g[el].items()}
    out["energy"] = g.energy
    for name in ("mu", "cov", "chosen_particles"):
        try:
            if getattr(g, name) is not None:
                out[name] = getattr(g, name)
        except KeyError:
            pass
    return out


def save(case, arrays):
    np.savez(out_dir / f"{case}.npz", **{k: np.asarray(v) for k, v in arrays.items()})
    print(case, len(arrays), "arrays", flush=True)


for dtype in (np.float32, np.float64):
    name, rng = np.dtype(dtype).name, np.random.default_rng(17)
    segment, beam = cavities(3, dtype)
    save(f"a_track_vjp_{name}", gradients(grad.track_vjp(segment, beam)(mu_bar=rng.normal(size=(3, 7)), cov_bar=rng.normal(size=(3, 7, 7))), segment))
    save(f"b_along_vjp_parameter_beam_{name}",
         gradients(grad.track_along_vjp(segment, beam)(mu_bar=rng.normal(size=(3, 9, 7)), cov_bar=rng.normal(size=(3, 9, 7, 7))), segment))
    segment, beam = affine(3, dtype)
    mu_bar, cov_bar = rng.normal(size=(3, 8, 6)), rng.normal(size=(3, 8, 6, 6))
    save(f"c_along_vjp_particles_{name}", gradients(grad.track_along_vjp(segment, beam)(mu_bar=mu_bar, cov_bar=cov_bar), segment))
    vjp = grad.track_along_vjp(segment, beam, trajectories=4)
    save(f"e_along_vjp_trajectories_{name}", gradients(vjp(trajectories_bar=rng.normal(size=(3, 8, 4, 6)), mu_bar=mu_bar), segment))
    segment, beam = collimated(dtype)
    vjp = grad.track_along_vjp(segment, beam, losses=True)
    alive = np.asarray(vjp.trace.num_survivors)
    assert np.all((0 < alive[:, -1]) & (alive[:, -1] < alive[:, 2]) & (alive[:, 2] < 64)), alive
    save(f"d_along_vjp_losses_{name}",
         {**gradients(vjp(mu_bar=rng.normal(size=(2, 6, 6)), cov_bar=rng.normal(size=(2, 6, 6, 6))), segment), "num_survivors": alive})
    for B in (1, 3, 65):
        for min_batch in ("1", "1000000") if dtype == np.float32 else ("",):
            os.environ["LYNX_LANES_BUILD_MIN_BATCH"] = min_batch
            rt.reload_knobs()
            segment, beam = cavities(B, dtype)
            out, trace = segment.track(beam), segment.track_along(beam)
            save(f"f_forward_{name}_batch{B}_lanes_from_{min_batch or 'default'}",
                 {"mu": out._mu, "cov": out._cov, "energy": out.energy, "trace_mu": trace._mu, "trace_cov": trace._cov, "trace_energy": trace.energy})
    os.environ.pop("LYNX_LANES_BUILD_MIN_BATCH", None)
    rt.reload_knobs()
