"""
Every path of the 7 x 7 moment recursion -- forward in both forms, and the reverse sweeps of `track_vjp` and
`track_along_vjp` (plain, with losses, with trajectories) --, and every branch of the reverse pass over the particles
(`track_vjp` of a ParticleBeam under each of its knobs, pool sizes and chunk plans; `track_along_vjp` with cavities and with
screens), once each on seeded inputs, every returned array written to DIR/<case>.npz.  Two builds of the library (LYNX_HIP_LIBRARY picks one) are compared array by array with
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
    for name in ("mu", "cov", "chosen_particles", "particles"):
        try:
            if getattr(g, name) is not None:
                out[name] = getattr(g, name)
        except (KeyError, AttributeError):  # (AttributeError: ChainedGradients has `mu` and `cov` alone)
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


# ---- the reverse pass over the particles: every branch of track_backward_t, and the trace's passes that share its host code ----

from oracle import lynx_oracle as o  # noqa: E402
from tests.helpers import make_lattice  # noqa: E402
from tests.test_gpu_grad import _desc  # noqa: E402

BEAM = dict(sigma=[1e-3, 1e-4, 1e-3, 1e-4, 1e-3, 1e-3], mu=[1e-3, -1e-4, 5e-4, 2e-4, 1e-4, 1e-3])


def knobs(**values):
    """LYNX_<NAME>=value for these knobs and no other of the reverse pass."""
    for name in ("BWD_PAIRS", "BWD_UNITS", "BWD_MERGE", "BWD_REUSE_TABLE", "INLINE_POOL"):
        os.environ.pop(f"LYNX_{name}", None)
    os.environ.update({f"LYNX_{name}": str(value) for name, value in values.items()})
    rt.reload_knobs()


def beam_of(B, N, dtype):
    energy = np.random.default_rng(5).uniform(6e6, 8e6, B)
    return lx.ParticleBeam(o.gaussian_particles((B,), N, seed=9, dtype=np.float64, **BEAM).astype(dtype), energy.astype(dtype), dtype=dtype)


def nine(B, N, dtype):
    """The nine-element lattice of tests/test_gpu_grad.py (two gaining cavities, a tilted quadrupole, a dipole) and a beam."""
    return lx.Segment(make_lattice(_desc(B, np.random.default_rng(42)), dtype, lx)[0]), beam_of(B, N, dtype)


def plain_cells(B, N, cells, dtype=np.float32):
    """Cells of [drift, quadrupole, corrector, cavity]: every unit of class U -- the dense kernel runs one workgroup per sample."""
    rng = np.random.default_rng(8)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    elements = []
    for c in range(cells):
        elements += [lx.Drift(f(0.3), dtype=dtype), lx.Quadrupole(f(0.1), k1=((-1) ** c * rng.uniform(0.5, 2, B)).astype(dtype), dtype=dtype),
                     lx.HorizontalCorrector(f(0.1), angle=rng.normal(0, 1e-3, B).astype(dtype), dtype=dtype),
                     lx.Cavity(f(1.0377), voltage=rng.uniform(2e6, 6e6, B).astype(dtype), phase=rng.uniform(-10, 10, B).astype(dtype),
                               frequency=f(1.3e9), dtype=dtype)]
    return lx.Segment(elements), beam_of(B, N, dtype)


def pooled(B, dtype):
    """Three cavity-free cells (tests/test_gpu_parity.py): B = 1 fits the 256 B parameter pool, B = 3 needs the 1 KB one."""
    rng = np.random.default_rng(31)
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    elements = []
    for c in range(3):
        elements += [lx.Drift(f(0.3), dtype=dtype), lx.Quadrupole(f(0.2), k1=rng.uniform(-4, 4, B).astype(dtype), dtype=dtype),
                     lx.HorizontalCorrector(f(0.1), angle=f(1e-4), dtype=dtype), lx.Marker(name=f"M{c}")]
    return lx.Segment(elements), beam_of(B, 3001, dtype)


def track_vjp_case(case, segment, beam, **call):
    rng, B = np.random.default_rng(71), beam.batch_shape[0]
    g = grad.track_vjp(segment, beam)(mu_bar=rng.normal(size=(B, 6)), cov_bar=rng.normal(size=(B, 6, 6)) * 1e3, wrt_particles=True, **call)
    save(case, gradients(g, segment))


track_vjp_case("g_track_vjp_particles_float64", *nine(3, 3000, np.float64))
knobs(BWD_PAIRS=0)
track_vjp_case("g_track_vjp_particles_float32_one_per_lane", *nine(3, 3000, np.float32))
for units in (0, 1, 2):
    for merge in (0, 1):
        knobs(BWD_UNITS=units, BWD_MERGE=merge)
        track_vjp_case(f"g_track_vjp_particles_float32_units{units}_merge{merge}", *nine(3, 3000, np.float32))
        track_vjp_case(f"g_track_vjp_class_u_ten_cells_units{units}_merge{merge}", *plain_cells(3, 3000, 10))
for reuse in (0, 1):
    knobs(BWD_REUSE_TABLE=reuse)
    track_vjp_case(f"g_track_vjp_particles_float32_reuse_table{reuse}", *nine(3, 3000, np.float32))
    for inline in (0, 1):
        knobs(BWD_REUSE_TABLE=reuse, INLINE_POOL=inline)
        for B in (1, 3):
            for dtype in (np.float32, np.float64):
                track_vjp_case(f"g_track_vjp_pool_batch{B}_{np.dtype(dtype).name}_inline{inline}_reuse_table{reuse}", *pooled(B, dtype))
knobs()
f64 = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
bpm = lx.BPM(is_active=True, name="BPM1")
with_bpm = lx.Segment([lx.Drift(f64(1.0), dtype=np.float64), lx.Quadrupole(f64(0.2), k1=f64(2.0), dtype=np.float64),
                       lx.Cavity(f64(1.0377), voltage=f64(1.5e7), phase=f64(-5.0), frequency=f64(1.3e9), dtype=np.float64),
                       lx.Drift(f64(2.0), dtype=np.float64), bpm, lx.Drift(f64(0.5), dtype=np.float64)])
track_vjp_case("g_track_vjp_bpm_readings", with_bpm, beam_of(1, 2000, np.float64), readings={bpm: np.array([[0.7], [-1.3]])})
for dtype in (np.float32, np.float64):
    name = np.dtype(dtype).name
    track_vjp_case(f"g_track_vjp_sixteen_chunks_and_more_{name}", *nine(2, 9000, dtype))
    track_vjp_case(f"g_track_vjp_few_chunks_{name}", *nine(300, 700, dtype))
track_vjp_case("g_track_vjp_class_u_one_workgroup_per_sample", *plain_cells(2, 3000, 2))

for dtype, N in ((np.float64, 4097), (np.float32, 8193)):  # 17 chunks
    rng = np.random.default_rng(73)
    segment, beam = nine(2, N, dtype)
    g = grad.track_along_vjp(segment, beam, cavities=True)(mu_bar=rng.normal(size=(2, 10, 6)), cov_bar=rng.normal(size=(2, 10, 6, 6)) * 1e3,
                                                           wrt_particles=True)
    save(f"h_along_vjp_cavities_{np.dtype(dtype).name}_{N}", gradients(g, segment))
for dtype in (np.float32, np.float64):
    full = lambda v: np.full(3, v, dtype=dtype)  # noqa: E731
    screen = lx.Screen(resolution=(40, 24), pixel_size=(1.25e-5, 1.25e-5), binning=2, misalignment=np.array([1e-5, -2e-5], dtype=dtype),
                       is_active=True, name="SCREEN", dtype=dtype)
    segment = lx.Segment([lx.Drift(full(0.6), dtype=dtype), lx.Quadrupole(full(0.2), k1=np.linspace(-2.0, 3.0, 3).astype(dtype), dtype=dtype),
                          lx.HorizontalCorrector(full(0.1), angle=full(3e-5), dtype=dtype), lx.Drift(full(0.8), dtype=dtype), screen])
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-5), mu_y=full(-1e-5), sigma_x=full(1e-4), sigma_xp=full(1e-5), sigma_y=full(1e-4),
                                            sigma_yp=full(1e-5), sigma_s=full(1e-5), sigma_p=full(1e-3), energy=full(1e8), dtype=dtype)
    vjp = grad.track_along_vjp(segment, beam, screens=True)
    image = np.asarray(vjp.trace.image_at("SCREEN"), dtype=np.float64)
    save(f"i_along_vjp_screens_parameter_beam_{np.dtype(dtype).name}",
         {**gradients(vjp(screen_images_bar={"SCREEN": image - 1.1 * np.roll(image, 3, axis=-2)}, sigma_x=1e3), segment), "image": image})


# ---- what the Python layer of the reverse passes adds: named properties through each VJP class, `readings=` across two
# ---- stretches of a ParameterBeam lattice, an RBend (e1, e2 folded into angle), a parameter of shape (1,) under the batch ----

def mixed(dtype, B=3):
    f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
    bpm = lx.BPM(is_active=True, name="BPM_MIXED")
    segment = lx.Segment([lx.Drift(f(0.6), dtype=dtype), lx.Quadrupole(f(0.2), k1=np.linspace(-3.0, 4.0, B).astype(dtype), dtype=dtype),
                          lx.RBend(f(0.5), angle=np.linspace(0.1, 0.2, B).astype(dtype), e1=f(0.01), dtype=dtype), bpm,
                          lx.HorizontalCorrector(f(0.1), angle=np.array([2e-4], dtype=dtype), dtype=dtype), lx.Drift(f(0.4), dtype=dtype)])
    particles = lx.ParticleBeam.synthetic((B,), 1000, sigma=SIGMA, energy=1e8, seed=6, dtype=dtype)
    parameters = lx.ParameterBeam.from_parameters(mu_x=np.linspace(-1e-5, 2e-5, B).astype(dtype), sigma_x=f(1e-4), sigma_xp=f(1e-5), sigma_y=f(2e-4),
                                                  sigma_yp=f(1e-5), sigma_s=f(1e-5), sigma_p=f(1e-3), energy=f(1e8), dtype=dtype)
    return segment, bpm, particles, parameters


for dtype in (np.float32, np.float64):
    name, rng = np.dtype(dtype).name, np.random.default_rng(79)
    segment, bpm, particles, parameters = mixed(dtype)
    named = dict(sigma_x=rng.normal(size=3), sigma_p=rng.normal(size=3), mu_y=rng.normal(size=3), sigma_xxp=rng.normal(size=3) * 1e3, sigma_yyp=2e3)
    reading = {bpm: rng.normal(size=(2, 3))}
    save(f"j_track_vjp_particles_properties_{name}", gradients(grad.track_vjp(segment, particles)(readings=reading, **named), segment))
    save(f"j_track_vjp_parameter_beam_two_stretches_{name}",
         gradients(grad.track_vjp(segment, parameters)(mu_bar=rng.normal(size=(3, 6)), readings=reading, **named), segment))
    along = dict(beta_x=rng.normal(size=(3, 7)), sigma_y=rng.normal(size=(3, 7)), normalized_emittance_y=1e6, alpha_x=0.5, energy=rng.normal(size=(3, 7)) * 1e-8)
    save(f"j_along_vjp_particles_properties_{name}", gradients(grad.track_along_vjp(segment, particles)(readings=reading, **along), segment))
    save(f"j_along_vjp_parameter_beam_properties_{name}", gradients(grad.track_along_vjp(segment, parameters)(readings=reading, **along), segment))
