"""
One table of calls through the C ABI, shared by the tests that ask WHAT an entry point refuses (test_gpu_entry_refusals.py) and
WHERE it writes (test_gpu_entry_footprint.py, test_entry_footprint_host.py): per entry the call from named arguments, the
arguments of a valid call, and the arrays it names -- each stated as (name, dtype, shape, role), role `in`, `out` or `inout`
(read and added to: d_mu_bar / d_cov_bar of the two image reverse calls, include/lynx_hip.h).  Everything is a function of a
`Shape`: batch, particles, image cells, chosen particles and the lattice.

Lattices, every element a step of its own (the trace's program):
  plain     an inactive aperture (an identity step), a drift, a quadrupole                        S = 3
  marked    ... with a marker behind the drift and one behind the quadrupole (two more identity   S = 5
            steps: where a particle trace may hold screens beside the aperture at step 0)
  cavity    inactive aperture, drift, ACTIVE cavity, quadrupole; 1e8 eV in, 1e7 V on crest:        S = 4
            every sample gains energy
  pairs     drift, active cavity, quadrupole, active cavity: nothing but [run, cavity] pairs, the form     S = 4
            lynx_track_particles and its reverse pass walk as merged units of class U in float32 (no identity
            step: the forward call and lynx_track_particles_backward only)
  observer  drift, active BPM, quadrupole as lynx_track_particles runs them: run, observer, run    S = 3
  empty     no element, no step: what lynx_track_particles accepts and lynx_moments runs            S = 0

This module holds no test and needs no GPU to be imported; `make_env` does.
"""

import ctypes as C
import math
from collections import namedtuple

import numpy as np

from .test_gpu_trace import SIGMA

F64 = np.dtype(np.float64)
I32, I64, U8 = np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.uint8)
GRAD_PARAMS = 8
STEPS_OF = {"plain": 3, "marked": 5, "cavity": 4, "pairs": 4, "observer": 3, "empty": 0}

Array = namedtuple("Array", "name dtype shape role")


class Shape(namedtuple("Shape", "B N NX NY CHOSEN lattice", defaults=("plain",))):
    """Batch, particles per sample, image cells nx x ny, chosen particles, and the lattice's name."""

    __slots__ = ()
    S = property(lambda self: STEPS_OF[self.lattice])
    E = property(lambda self: STEPS_OF[self.lattice])  # every element is a step
    P = property(lambda self: STEPS_OF[self.lattice] + 1)
    CELLS = property(lambda self: self.NX * self.NY)
    SCREEN = property(lambda self: [2, self.NX, self.NY])  # a screen at point 2 of the trace
    SCREENS = property(lambda self: [2, self.NX, self.NY, 4, self.NY, self.NX])  # ... and one at point 4, transposed (marked lattice)
    BLOCKS = property(lambda self: -(-self.N // 1024))  # lynx_aperture_mask: counts / offsets per 1024 particles

    @property
    def indices(self):
        """The chosen particles: any order, the last one chosen twice from three on."""
        if self.CHOSEN == 2:
            return [0, min(5, self.N - 1)]
        return [self.N - 1, 0, self.N - 1, self.N // 2][: self.CHOSEN]


REFUSALS_SHAPE = Shape(2, 64, 5, 3, 2)

ints = lambda values: (C.c_int32 * len(values))(*values)  # noqa: E731
longs = lambda values: (C.c_int64 * len(values))(*values)  # noqa: E731
doubles = lambda values: (C.c_double * len(values))(*values)  # noqa: E731


def array_specs(s, dtype):
    """name -> (dtype, shape) of every device array the calls name, for one shape and lattice dtype."""
    B, N, P, E, K, cells = s.B, s.N, s.P, max(s.E, 1), s.CHOSEN, s.CELLS
    t = np.dtype(dtype)
    return dict(
        e_in=(t, (B,)), p_in=(t, (B, N, 7)), p_shared=(t, (N, 7)), mu_in=(t, (B, 7)), cov_in=(t, (B, 49)),
        p_out=(t, (B, N, 7)), e_out=(t, (B,)), mom=(F64, (B, 36)), obs=(F64, (B, 1, 2)),
        mu_out=(t, (B, 7)), cov_out=(t, (B, 49)),
        mu_tr=(t, (B, P, 7)), cov_tr=(t, (B, P, 49)), e_tr=(t, (B, P)),
        records=(F64, (B, P, 36)), lost_at=(I32, (B, N)), set_records=(F64, (B, 2, 36)),
        limits=(t, (1, 2)), limits_tight=(t, (B, 1, 2)),
        chosen=(I64, (K,)), traj=(t, (B, P, K, 7)),
        g_mom=(F64, (B, 36)), g_records=(F64, (B, P, 36)), traj_bar=(F64, (B, P, K, 7)),
        mu_bar=(t, (B, 7)), cov_bar=(t, (B, 49)), mu_bar_tr=(t, (B, P, 7)), cov_bar_tr=(t, (B, P, 49)),
        g_params=(t, (B, E, GRAD_PARAMS)), g_e=(t, (B,)), g_p=(t, (B, N, 7)),
        g_mu=(t, (B, 7)), g_cov=(t, (B, 49)), g_chosen=(t, (B, K, 7)),
        steps=(t, (B, max(s.S, 1), 64)),
        xedges=(t, (s.NX + 1,)), yedges=(t, (s.NY + 1,)), hist=(I32, (B, cells)),
        x_max=(t, (1,)), y_max=(t, (1,)), mask=(U8, (B, N)), counts=(I32, (B, s.BLOCKS)),
        offsets=(I64, (B, s.BLOCKS)), totals=(I64, (B,)), kept=(t, (N, 7)), lost=(t, (N, 7)),
        xs=(t, (s.NX,)), ys=(t, (s.NY,)), image=(t, (B, cells)),
        grid=(t, (s.NX + s.NY,)), grid2=(t, (2 * (s.NX + s.NY),)),
        misalignment=(t, (1, 2)), misalignment2=(t, (B, 2, 2)),
        images=(t, (B, cells)), images2=(t, (B, 2 * cells)), images_bar=(t, (B, cells)),
        mu_bar_out=(t, (B, P, 7)), cov_bar_out=(t, (B, P, 49)), g_mis=(t, (B, 1, 2)),
        fill=(t, (B, N, 7)), gauss_rows=(F64, (B, 27)), transform_rows=(t, (B, 24)),
        copy=(F64, (B, 36)), sets_out=(F64, (B, 2, 36)),
        # the entries the refusals' table lacks
        e_tr_out=(t, (B, P)), records_out=(F64, (B, P, 36)), lost_out=(I32, (B, N)),
        edges=(t, (s.NX + s.NY + 2,)), edges2=(t, (2 * (s.NX + s.NY + 2),)),
        pimages=(I32, (B, cells)), pimages2=(I32, (B, 2 * cells)),
        traj_out=(t, (B, P, K, 7)), traj_lost=(I32, (B, K)),
        targets=(t, (B, cells)), loss=(F64, (B, 1)), sums=(F64, (B, 1, 6)), sums_out=(F64, (B, 1, 6)), loss_bar=(t, (B, 1)))


# what the module's prelude of forward calls writes and the reverse entries read (`Env.keep`)
DERIVED = ("mom", "records", "lost_at", "set_records", "traj", "mu_tr", "cov_tr", "sums", "mask", "counts", "offsets", "totals")


def host_inputs(s, dtype):
    """name -> host array of every array that a call READS and no call of the prelude writes."""
    from oracle import lynx_oracle as o

    B, N, P, K = s.B, s.N, s.P, s.CHOSEN
    t = np.dtype(dtype)
    one = lambda v: np.array([v], dtype=t)  # noqa: E731
    particles = o.gaussian_particles((B,), N, seed=5, dtype=t, sigma=SIGMA)
    rng = np.random.default_rng(11)
    small = lambda *shape, t=t: (1e-3 * rng.standard_normal(shape)).astype(t)  # noqa: E731
    # the beam's own mean and biased covariance; a beam of a particle or two has none worth an image: a round one then
    mu = particles.mean(axis=1).astype(np.float64)
    centred = particles - particles.mean(axis=1)[:, None, :]
    cov = np.einsum("bni,bnj->bij", centred, centred).astype(np.float64) / N
    if N < 8:
        cov[:, :6, :6] = np.diag(np.square(SIGMA))
        cov[:, 0, 2] = cov[:, 2, 0] = 0.25 * SIGMA[0] * SIGMA[2]
    line = lambda n: np.linspace(-3e-4, 3e-4, n)  # noqa: E731
    edges = np.concatenate([line(s.NX + 1), line(s.NY + 1)])
    grid = np.concatenate([line(s.NX), line(s.NY)])
    edges2 = np.concatenate([edges, line(s.NY + 1), line(s.NX + 1)])  # the second screen: ny x nx pixels
    grid2 = np.concatenate([grid, line(s.NY), line(s.NX)])
    return dict(
        e_in=np.full(B, 1e8, dtype=t), p_in=particles, p_shared=np.ascontiguousarray(particles[0]),
        mu_in=mu.astype(t), cov_in=cov.reshape(B, 49).astype(t),
        limits=np.full((1, 2), 1e-2, dtype=t),
        limits_tight=np.tile(np.array([1.5 * SIGMA[0], 2.0 * SIGMA[2]], dtype=t), (B, 1, 1)),
        chosen=np.array(s.indices, dtype=np.int64),
        g_mom=small(B, 36, t=F64), g_records=small(B, P, 36, t=F64), traj_bar=small(B, P, K, 7, t=F64),
        mu_bar=small(B, 7), cov_bar=small(B, 49), mu_bar_tr=small(B, P, 7), cov_bar_tr=small(B, P, 49),
        xedges=line(s.NX + 1).astype(t), yedges=line(s.NY + 1).astype(t),
        x_max=one(1e-4), y_max=one(1e-4),
        xs=line(s.NX).astype(t), ys=line(s.NY).astype(t),
        grid=grid.astype(t), grid2=grid2.astype(t), edges=edges.astype(t), edges2=edges2.astype(t),
        images_bar=small(B, s.CELLS),
        misalignment=np.zeros((1, 2), dtype=t), misalignment2=(1e-5 * rng.standard_normal((B, 2, 2))).astype(t),
        gauss_rows=np.tile(np.concatenate([np.zeros(6), np.diag(SIGMA)[np.tril_indices(6)]]), (B, 1)).astype(F64),
        transform_rows=np.tile(np.concatenate([np.zeros(6), SIGMA, 2 * np.asarray(SIGMA), np.full(6, 1e-5)]), (B, 1)).astype(t),
        targets=np.abs(1e3 * rng.standard_normal((B, s.CELLS))).astype(t), loss_bar=small(B, 1),
        # what an `inout` array holds before the call: data, the same finite values in every run
        mu_bar_out=small(B, P, 7), cov_bar_out=small(B, P, 49))


def leaves_of(lx, s, dtype):
    """The lattice `s.lattice` as leaf elements (None for the empty program)."""
    t, B = np.dtype(dtype), s.B
    one = lambda v: np.array([v], dtype=t)  # noqa: E731
    aperture = lambda: lx.Aperture(x_max=one(1e-2), y_max=one(1e-2), is_active=False, name="AP", dtype=t)  # noqa: E731
    drift = lambda: lx.Drift(np.full(B, 0.7, dtype=t), dtype=t)  # noqa: E731
    quadrupole = lambda: lx.Quadrupole(np.full(B, 0.2, dtype=t), k1=np.linspace(4.2, -3.0, B).astype(t), dtype=t)  # noqa: E731
    if s.lattice == "plain":
        return [aperture(), drift(), quadrupole()]
    if s.lattice == "marked":
        return [aperture(), drift(), lx.Marker(name="M1"), quadrupole(), lx.Marker(name="M2")]
    if s.lattice == "cavity":
        f = lambda v: np.full(B, v, dtype=t)  # noqa: E731
        return [aperture(), drift(), lx.Cavity(f(1.0377), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), dtype=t), quadrupole()]
    if s.lattice == "pairs":
        f = lambda v: np.full(B, v, dtype=t)  # noqa: E731
        cavity = lambda: lx.Cavity(f(1.0377), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), dtype=t)  # noqa: E731
        return [drift(), cavity(), quadrupole(), cavity()]
    if s.lattice == "observer":
        return [drift(), lx.BPM(is_active=True, name="bpm"), quadrupole()]
    assert s.lattice == "empty", s.lattice
    return None


class EmptyLattice:
    """A handle of no elements and no steps, made through lynx_lattice_create itself."""

    S = E = 0

    def __init__(self, rt, code, B, dtype):
        from lynx_amd import _ffi

        self.rt, self.B, self.handle = rt, B, C.c_void_p()
        pool = np.zeros(1, dtype=dtype)
        rt.check(rt.lib.lynx_lattice_create(rt.ctx, code, B, 0, (_ffi.Elem * 1)(), 0, (_ffi.Step * 1)(), pool.ctypes.data, 1,
                                            C.byref(self.handle)))

    def __del__(self):
        try:
            if not self.rt.closed:
                self.rt.lib.lynx_lattice_destroy(self.handle)
        except Exception:
            pass


class Env:
    """The runtime, the lattice, every device array the calls name (`a`) and the host copy of every input (`host`), for
    one shape and dtype."""


def make_env(s, dtype, prelude=True):
    """Every array in a block of its own (`rt.to_device`, `rt.empty`: the ordinary path), and the prelude of forward calls
    whose results the reverse entries read."""
    import lynx_amd as lx
    from lynx_amd import _ffi, engine

    rt = lx.device.get_runtime()  # raises loudly without a GPU
    dtype = np.dtype(dtype)
    e = Env()
    e.rt, e.dtype, e.code, e.shape = rt, dtype, _ffi.F64 if dtype == F64 else _ffi.F32, s
    e.leaves = leaves_of(lx, s, dtype)
    e.host = host_inputs(s, dtype)
    if s.lattice == "empty":
        e.lat = EmptyLattice(rt, e.code, s.B, dtype)
    else:
        e.cache = engine.LatticeCache()
        if s.lattice == "observer":
            e.seg = lx.Segment(e.leaves)
            program, = engine.plan(e.seg, e.seg.elements, False, fuse_observers=True)
        else:
            program = engine.trace_program(e.leaves)
        e.lat = engine._ready(e.cache, program, (s.B,), dtype, e.host["e_in"])
    assert e.lat.S == s.S and e.lat.E == s.E and e.lat.B == s.B
    e.a = {name: rt.to_device(e.host[name]) if name in e.host else rt.empty(shape, t) for name, (t, shape) in array_specs(s, dtype).items()}
    e.keep = {}
    if not prelude:
        return e
    lib, ctx, lat, p, N, B = rt.lib, rt.ctx, e.lat.handle, lambda name: C.c_void_p(e.a[name].ptr), s.N, s.B  # noqa: E731
    # what the reverse passes read: the forward call's moment records, the trace's records, the trace with losses' lost_at and
    # survivor-set records, the chosen particles' trajectories, the ParameterBeam's trace, the image loss's sums, the mask
    rt.check(lib.lynx_track_particles(ctx, lat, N, p("e_in"), p("p_in"), p("p_out"), None, p("mom"), _ffi.TRACK_MOMENTS, None))
    if s.lattice == "pairs":  # (no identity step for an aperture or a screen: the forward call and its reverse pass only)
        e.host["mom"] = e.a["mom"].numpy()
        return e
    rt.check(lib.lynx_track_particles_along(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0))
    rt.check(lib.lynx_track_particles_along_losses(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0, 1,
                                                   ints([0, 0]), p("limits"), 0, p("lost_at")))
    rt.check(lib.lynx_moments_by_loss(ctx, e.code, B, N, p("p_in"), 0, 1, p("lost_at"), p("set_records")))
    rt.check(lib.lynx_track_particles_along_trajectories(ctx, lat, N, p("e_in"), p("p_in"), None, p("e_tr"), p("records"), 0,
                                                         -1, None, None, 0, None, -1, None, None, None, 0, None,
                                                         s.CHOSEN, p("chosen"), p("traj"), None))
    rt.check(lib.lynx_track_moments_along(ctx, lat, p("e_in"), p("mu_in"), p("cov_in"), p("mu_tr"), p("cov_tr"), p("e_tr")))
    rt.check(lib.lynx_gaussian_images_along_mse(ctx, e.code, B, s.P, p("mu_tr"), p("cov_tr"), 1, ints(s.SCREEN), p("grid"),
                                                p("misalignment"), 0, longs([0]), p("targets"), s.CELLS, p("loss"), p("sums")))
    rt.check(lib.lynx_aperture_mask(ctx, e.code, B, N, p("p_in"), p("x_max"), p("y_max"), 0, 0, p("mask"), p("counts"),
                                    p("offsets"), p("totals")))
    rt.sync()
    for name in DERIVED:
        e.host[name] = e.a[name].numpy()
    e.keep = {name: e.host[name].tobytes() for name in ("mom", "records", "lost_at", "set_records", "traj", "mu_tr", "cov_tr")}
    return e


# entry -> (the call from the named arguments and the shape, the arguments of a valid call, what it writes, the refused
# change, the message).  An argument that names a device array is passed as its pointer; None is a null pointer.
ENTRIES = {
    "lynx_track_particles": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles(ctx, lat, a["n"], a["e_in"], a["p_in"], a["p_out"], a["e_out"], a["mom"], 1, None),
        dict(n="N", e_in="e_in", p_in="p_in", p_out="p_out", e_out="e_out", mom="mom"), ["p_out", "e_out", "mom"],
        dict(n=0), "n_particles must be > 0"),
    "lynx_track_particles_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_backward(ctx, lat, s.N, a["e_in"], a["p_in"], a["mom"], a["g_mom"], a["g_params"],
                                                                            a["g_e"], a["g_p"], None),
        dict(e_in="e_in", p_in="p_in", mom="mom", g_mom="g_mom", g_params="g_params", g_e="g_e", g_p="g_p"), ["g_params", "g_e", "g_p"],
        dict(g_params=None), "null argument"),
    "lynx_track_moments": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_moments(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_out"], a["cov_out"], a["e_out"]),
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_out="mu_out", cov_out="cov_out", e_out="e_out"), ["mu_out", "cov_out", "e_out"],
        dict(mu_out=None), "null argument"),
    "lynx_track_moments_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_moments_backward(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_bar"], a["cov_bar"],
                                                                          a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_bar="mu_bar", cov_bar="cov_bar", g_params="g_params", g_e="g_e", g_mu="g_mu",
             g_cov="g_cov"), ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_moments_along": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_moments_along(ctx, lat, a["e_in"], a["mu_in"], a["cov_in"], a["mu_tr"], a["cov_tr"], a["e_tr"]),
        # (into blocks of the right sizes that nothing else reads)
        dict(e_in="e_in", mu_in="mu_in", cov_in="cov_in", mu_tr="mu_bar_out", cov_tr="cov_bar_out", e_tr="e_tr"),
        ["mu_bar_out", "cov_bar_out", "e_tr"],
        dict(mu_tr=None), "null argument"),
    "lynx_track_moments_along_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_moments_along_backward(ctx, lat, a["e_in"], a["mu_tr"], a["cov_tr"], a["mu_bar_tr"],
                                                                                a["cov_bar_tr"], None, a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", mu_tr="mu_tr", cov_tr="cov_tr", mu_bar_tr="mu_bar_tr", cov_bar_tr="cov_bar_tr", g_params="g_params", g_e="g_e",
             g_mu="g_mu", g_cov="g_cov"), ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_particles_along_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_backward(ctx, lat, s.N, a["e_in"], a["records"], a["g_records"], None,
                                                                                  a["g_params"], a["g_e"], a["g_mu"], a["g_cov"]),
        dict(e_in="e_in", records="records", g_records="g_records", g_params="g_params", g_e="g_e", g_mu="g_mu", g_cov="g_cov"),
        ["g_params", "g_e", "g_mu", "g_cov"],
        dict(g_params=None), "null argument"),
    "lynx_track_particles_along_backward_cavities": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_backward_cavities(ctx, lat, s.N, a["e_in"], a["p_in"], 0, a["records"],
                                                                                           a["g_records"], None, a["g_params"], a["g_e"], a["g_p"]),
        dict(e_in="e_in", p_in="p_in", records="records", g_records="g_records", g_params="g_params", g_e="g_e", g_p="g_p"),
        ["g_params", "g_e", "g_p"],
        dict(g_params=None), "beam trace gradients with cavities: null argument"),
    "lynx_track_particles_along_backward_losses": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_backward_losses(ctx, lat, s.N, a["e_in"], a["records"], a["g_records"], None, 1,
                                                                                         ints([0]), a["set_records"], a["g_params"], a["g_e"]),
        dict(e_in="e_in", records="records", g_records="g_records", set_records="set_records", g_params="g_params", g_e="g_e"),
        ["g_params", "g_e"],
        dict(g_params=None), "beam trace gradients with losses: null argument"),
    "lynx_track_particles_along_backward_trajectories": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_backward_trajectories(ctx, lat, s.N, a["e_in"], None, None, None, a["g_params"],
                                                                                               a["g_e"], None, None, s.CHOSEN, a["traj"], a["traj_bar"],
                                                                                               a["g_chosen"]),
        dict(e_in="e_in", g_params="g_params", g_e="g_e", traj="traj", traj_bar="traj_bar", g_chosen="g_chosen"),
        ["g_params", "g_e", "g_chosen"],
        dict(g_chosen=None), "beam trace gradients with trajectories: null argument"),
    "lynx_moments": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_moments(ctx, code, s.B, s.N, a["p_in"], a["out"], 1),
        dict(p_in="p_in", out="copy"), ["copy"],
        dict(out=None), "null argument"),
    "lynx_moments_by_loss": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_moments_by_loss(ctx, code, s.B, s.N, a["p_in"], 0, 1, a["lost_at"], a["out"]),
        dict(p_in="p_in", lost_at="lost_at", out="sets_out"), ["sets_out"],
        dict(out=None), "moments by loss: null argument"),
    "lynx_histogram2d": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_histogram2d(ctx, code, s.B, s.N, a["p_in"], a["xedges"], a["yedges"], s.NX, s.NY, a["hist"]),
        dict(p_in="p_in", xedges="xedges", yedges="yedges", hist="hist"), ["hist"],
        dict(hist=None), "bad argument"),
    "lynx_aperture_mask": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_aperture_mask(ctx, code, s.B, s.N, a["p_in"], a["x_max"], a["y_max"], 0, 0, a["mask"], a["counts"],
                                                                 a["offsets"], a["totals"]),
        dict(p_in="p_in", x_max="x_max", y_max="y_max", mask="mask", counts="counts", offsets="offsets", totals="totals"),
        ["mask", "counts", "offsets", "totals"],
        dict(mask=None), "bad argument"),
    "lynx_aperture_compact": (  # (the first sample's particles, behind the valid lynx_aperture_mask call of the module's order)
        lambda lib, ctx, lat, code, a, s: (lib.lynx_aperture_mask(ctx, code, s.B, s.N, a["p_in"], a["x_max"], a["y_max"], 0, 0, a["mask"],
                                                                  a["counts"], a["offsets"], a["totals"])
                                           or lib.lynx_aperture_compact(ctx, code, s.N, a["p_in"], a["mask"], a["offsets"], a["kept"], a["lost"])),
        dict(p_in="p_in", x_max="x_max", y_max="y_max", mask="mask", counts="counts", offsets="offsets", totals="totals", kept="kept",
             lost="lost"), ["kept", "lost"],
        dict(kept=None), "bad argument"),
    "lynx_gaussian_image": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_image(ctx, code, s.B, a["mu_in"], a["cov_in"], a["xs"], a["ys"], s.NX, s.NY, a["image"]),
        dict(mu_in="mu_in", cov_in="cov_in", xs="xs", ys="ys", image="image"), ["image"],
        dict(image=None), "bad argument"),
    "lynx_gaussian_images_along": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along(ctx, code, s.B, s.P, a["mu_tr"], a["cov_tr"], 1, ints(s.SCREEN), a["grid"],
                                                                         a["misalignment"], 0, a["images"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", images="images"), ["images"],
        dict(images=None), "bad argument"),
    "lynx_gaussian_images_along_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along_backward(ctx, code, s.B, s.P, a["mu_tr"], a["cov_tr"], 1, ints(s.SCREEN),
                                                                                  a["grid"], a["misalignment"], 0, a["images_bar"], a["mu_bar_out"],
                                                                                  a["cov_bar_out"], a["g_mis"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", images_bar="images_bar", mu_bar_out="mu_bar_out",
             cov_bar_out="cov_bar_out", g_mis="g_mis"), ["mu_bar_out", "cov_bar_out", "g_mis"],
        dict(mu_bar_out=None), "image gradients along the trace: bad argument"),
    "lynx_fill_gaussian": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_fill_gaussian(ctx, code, s.B, s.N, doubles([0.0] * 6), doubles(SIGMA), 7, a["fill"]),
        dict(fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_fill_gaussian_rows": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_fill_gaussian_rows(ctx, code, s.B, s.N, a["gauss_rows"], 7, a["fill"]),
        dict(gauss_rows="gauss_rows", fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_transform_particles": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_transform_particles(ctx, code, s.B, s.N, a["p_in"], s.N * 7, a["transform_rows"], a["fill"]),
        dict(p_in="p_in", transform_rows="transform_rows", fill="fill"), ["fill"],
        dict(fill=None), "bad argument"),
    "lynx_build_compose": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_build_compose(ctx, lat, a["e_in"], a["steps"], a["e_out"]),
        dict(e_in="e_in", steps="steps", e_out="e_out"), ["steps", "e_out"],
        dict(steps=None), "null argument"),
}

def _along(lib, ctx, lat, a, s, flags=0, apertures=None, limit_stride=0, screens=None, mis_stride=0, chosen=False):
    """lynx_track_particles_along_trajectories, the superset of the four particle traces, from the named arguments."""
    return lib.lynx_track_particles_along_trajectories(
        ctx, lat, s.N, a["e_in"], a["p_in"], a.get("p_out"), a["e_tr"], a["records"], flags,
        -1 if apertures is None else len(apertures) // 2, None if apertures is None else ints(apertures), a.get("limits"), limit_stride,
        a.get("lost_at"), -1 if screens is None else len(screens) // 3, None if screens is None else ints(screens), a.get("edges"),
        a.get("misalignment"), mis_stride, a.get("images"), s.CHOSEN, a["chosen"], a["traj"], a.get("traj_lost"))


# ... and the entries that table lacks, with the variants of a call that take another path: (call, arguments, what it
# writes).  A name in square brackets says what differs from the entry's first row.
MORE_ENTRIES = {
    "lynx_track_particles[covariance]": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_out"], a["mom"], 16, None),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_out="e_out", mom="copy"), ["p_out", "e_out", "copy"]),
    "lynx_track_particles[shared input]": (  # LYNX_TRACK_SHARED_INPUT: d_p_in [N][7], sample stride 0
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_out"], a["mom"], 1 | 4, None),
        dict(e_in="e_in", p_in="p_shared", p_out="p_out", e_out="e_out", mom="copy"), ["p_out", "e_out", "copy"]),
    "lynx_track_particles[no moments]": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_out"], None, 0, None),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_out="e_out"), ["p_out", "e_out"]),
    "lynx_track_particles[observer]": (  # an active BPM inside the pass: d_observations
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_out"], a["mom"], 1, a["obs"]),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_out="e_out", mom="copy", obs="obs"), ["p_out", "e_out", "copy", "obs"]),
    "lynx_moments[properties]": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_moments(ctx, code, s.B, s.N, a["p_in"], a["out"], 0),
        dict(p_in="p_in", out="copy"), ["copy"]),
    "lynx_transform_particles[shared input]": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_transform_particles(ctx, code, s.B, s.N, a["p_in"], 0, a["transform_rows"], a["fill"]),
        dict(p_in="p_shared", transform_rows="transform_rows", fill="fill"), ["fill"]),
    "lynx_track_particles_along": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_tr"], a["records"], 0),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_tr="e_tr_out", records="records_out"), ["p_out", "e_tr_out", "records_out"]),
    "lynx_track_particles_along[moments only, shared input]": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along(ctx, lat, s.N, a["e_in"], a["p_in"], None, a["e_tr"], a["records"], 4),
        dict(e_in="e_in", p_in="p_shared", e_tr="e_tr_out", records="records_out"), ["e_tr_out", "records_out"]),
    "lynx_track_particles_along_losses": (  # one aperture at step 0, limits per sample (limit_stride 2) that remove particles
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_losses(ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_tr"], a["records"],
                                                                                0, 1, ints([0, 0]), a["limits"], 2, a["lost_at"]),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_tr="e_tr_out", records="records_out", limits="limits_tight", lost_at="lost_out"),
        ["p_out", "e_tr_out", "records_out", "lost_out"]),
    "lynx_track_particles_along_losses[shared limits]": (  # limit_stride 0, an elliptical aperture, no d_p_out
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_losses(ctx, lat, s.N, a["e_in"], a["p_in"], None, a["e_tr"], a["records"],
                                                                                0, 1, ints([0, 1]), a["limits"], 0, a["lost_at"]),
        dict(e_in="e_in", p_in="p_in", e_tr="e_tr_out", records="records_out", limits="limits", lost_at="lost_out"),
        ["e_tr_out", "records_out", "lost_out"]),
    "lynx_track_particles_along_screens": (  # (marked lattice) the aperture at step 0, one screen at step 2, shared misalignment
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_screens(
            ctx, lat, s.N, a["e_in"], a["p_in"], a["p_out"], a["e_tr"], a["records"], 0, 1, ints([0, 0]), a["limits"], 2, a["lost_at"],
            1, ints(s.SCREEN), a["edges"], a["misalignment"], 0, a["images"]),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_tr="e_tr_out", records="records_out", limits="limits_tight", lost_at="lost_out",
             edges="edges", misalignment="misalignment", images="pimages"),
        ["p_out", "e_tr_out", "records_out", "lost_out", "pimages"]),
    "lynx_track_particles_along_screens[two screens]": (  # screens at steps 2 and 4, misalignment per sample, shared limits and beam
        lambda lib, ctx, lat, code, a, s: lib.lynx_track_particles_along_screens(
            ctx, lat, s.N, a["e_in"], a["p_in"], None, a["e_tr"], a["records"], 4, 1, ints([0, 0]), a["limits"], 0, None,
            2, ints(s.SCREENS), a["edges"], a["misalignment"], 4, a["images"]),
        dict(e_in="e_in", p_in="p_shared", e_tr="e_tr_out", records="records_out", limits="limits",
             edges="edges2", misalignment="misalignment2", images="pimages2"),
        ["e_tr_out", "records_out", "pimages2"]),
    "lynx_track_particles_along_trajectories": (
        lambda lib, ctx, lat, code, a, s: _along(lib, ctx, lat, a, s),
        dict(e_in="e_in", p_in="p_in", p_out="p_out", e_tr="e_tr_out", records="records_out", chosen="chosen", traj="traj_out"),
        ["p_out", "e_tr_out", "records_out", "traj_out"]),
    "lynx_track_particles_along_trajectories[no p_out]": (  # ... and with an aperture: d_trajectory_lost_in
        lambda lib, ctx, lat, code, a, s: _along(lib, ctx, lat, a, s, apertures=[0, 0], limit_stride=2),
        dict(e_in="e_in", p_in="p_in", e_tr="e_tr_out", records="records_out", limits="limits_tight", lost_at="lost_out", chosen="chosen",
             traj="traj_out", traj_lost="traj_lost"),
        ["e_tr_out", "records_out", "lost_out", "traj_out", "traj_lost"]),
    "lynx_gaussian_images_along[two screens]": (  # points 2 and 4, misalignment per sample
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along(ctx, code, s.B, s.P, a["mu_tr"], a["cov_tr"], 2, ints(s.SCREENS), a["grid"],
                                                                         a["misalignment"], 4, a["images"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid2", misalignment="misalignment2", images="images2"), ["images2"]),
    "lynx_gaussian_images_along_mse": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along_mse(ctx, code, s.B, s.P, a["mu_tr"], a["cov_tr"], 1, ints(s.SCREEN), a["grid"],
                                                                             a["misalignment"], 0, longs([0]), a["targets"], s.CELLS, a["loss"],
                                                                             a["sums"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", targets="targets", loss="loss", sums="sums_out"),
        ["loss", "sums_out"]),
    "lynx_gaussian_images_along_mse[shared target]": (  # target_stride 0: the first sample's row for everyone
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along_mse(ctx, code, s.B, s.P, a["mu_tr"], a["cov_tr"], 1, ints(s.SCREEN), a["grid"],
                                                                             a["misalignment"], 0, longs([0]), a["targets"], 0, a["loss"], a["sums"]),
        dict(mu_tr="mu_tr", cov_tr="cov_tr", grid="grid", misalignment="misalignment", targets="targets", loss="loss", sums="sums_out"),
        ["loss", "sums_out"]),
    "lynx_gaussian_images_along_mse_backward": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_gaussian_images_along_mse_backward(ctx, code, s.B, s.P, a["cov_tr"], 1, ints(s.SCREEN), a["sums"],
                                                                                      a["loss_bar"], a["mu_bar_out"], a["cov_bar_out"], a["g_mis"]),
        dict(cov_tr="cov_tr", sums="sums", loss_bar="loss_bar", mu_bar_out="mu_bar_out", cov_bar_out="cov_bar_out", g_mis="g_mis"),
        ["mu_bar_out", "cov_bar_out", "g_mis"]),
    "lynx_buf_d2d": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_buf_d2d(ctx, a["dst"], a["src"], s.B * 36 * 8),
        dict(dst="copy", src="mom"), ["copy"]),
    "lynx_buf_memset": (
        lambda lib, ctx, lat, code, a, s: lib.lynx_buf_memset(ctx, a["dst"], 0x3c, s.B * 36 * 8),
        dict(dst="copy"), ["copy"]),
}
ALL_ENTRIES = {**{name: row[:3] for name, row in ENTRIES.items()}, **MORE_ENTRIES}

# arrays a call writes beside the outputs the refusals compare (the mask call in front of lynx_aperture_compact)
ALSO_WRITTEN = {"lynx_aperture_compact": ["mask", "counts", "offsets", "totals"]}
# read and added to (include/lynx_hip.h: "d_mu_bar [B][n_points][7], read and written: at each screen's point, entries 0 and 2
# are added to", "d_cov_bar ...: entries [0][0], [2][2], [0][2] and [2][0] are added to"; "ADDED into d_mu_bar ... and d_cov_bar
# ... at the screens' points"): array -> the entries of a point's row that may change
INOUT = {"lynx_gaussian_images_along_backward": {"mu_bar_out": (0, 2), "cov_bar_out": (0, 16, 2, 14)},
         "lynx_gaussian_images_along_mse_backward": {"mu_bar_out": (0, 2), "cov_bar_out": (0, 16, 2, 14)}}
# entries whose header comment admits a cavity step
ADMIT_CAVITY = ("lynx_track_particles", "lynx_track_particles_backward", "lynx_track_particles[covariance]", "lynx_track_particles[shared input]",
                "lynx_track_particles[no moments]", "lynx_track_moments", "lynx_track_moments_along", "lynx_build_compose",
                "lynx_track_particles_along", "lynx_track_particles_along[moments only, shared input]",
                "lynx_track_particles_along_losses", "lynx_track_particles_along_trajectories",
                "lynx_track_particles_along_trajectories[no p_out]", "lynx_track_particles_along_backward_cavities")
NEED_MARKED = ("lynx_track_particles_along_screens", "lynx_track_particles_along_screens[two screens]",
               "lynx_gaussian_images_along[two screens]")
ONLY_OBSERVER = ("lynx_track_particles[observer]",)
# ... and the ones that run on a lattice of nothing but [run, cavity] pairs as well
ADMIT_PAIRS = ("lynx_track_particles", "lynx_track_particles[covariance]", "lynx_track_particles[shared input]",
               "lynx_track_particles[no moments]", "lynx_track_particles_backward")


def entry_arrays(entry, s, dtype):
    """The arrays `entry` names at shape `s`: [Array(name, dtype, shape, role)], in the order of its arguments."""
    _, valid, outputs = ALL_ENTRIES[entry]
    specs = array_specs(s, dtype)
    written = list(outputs) + ALSO_WRITTEN.get(entry, [])
    out = []
    for name in dict.fromkeys(v for v in valid.values() if isinstance(v, str) and v in specs):
        role = "inout" if name in INOUT.get(entry, {}) else "out" if name in written else "in"
        out.append(Array(name, specs[name][0], specs[name][1], role))
    assert {a.name for a in out if a.role != "in"} == set(written), entry
    return out


def nbytes(array):
    return math.prod(array.shape) * array.dtype.itemsize


def arguments(entry, pointer_of, s, change=None):
    """The named arguments of `entry`'s call: `pointer_of(name)` for a device array, "N" for the particle count, None for NULL."""
    valid = ALL_ENTRIES[entry][1]
    names = {**valid, **(change or {})}
    return {key: None if name is None else s.N if name == "N" else name if not isinstance(name, str) else pointer_of(name)
            for key, name in names.items()}
