"""
The wave-tile forms of k_track_direct at their edges: a tile whose waves are whole, cut and absent, and a prefetch that
finds nothing.

Lattice: drift, quadrupole (k1 per sample), drift, horizontal corrector -- one run, no cavity, no active BPM: the single
map of `one_run`.  Batch B = 2 x the device's compute units (512 on an MI355X of 256), N = 2 tiles + 1 wave + 3 particles:
    float32 (P = 4: a wave tile is 256 particles, a workgroup tile 1024)   N = 2 * 1024 + 256 + 3 = 2307
    float64 (P = 2: 128 and 512)                                           N = 2 *  512 + 128 + 3 = 1155
Which form a case reaches (lynx_hip.hip: plan_track), with LYNX_XPOSE = 1:
  * B * ceil(N / (256 P)) = 3 B >= 4 CUs, so the plan keeps u = P and with it the wave tiles: k_track_direct<T, MOM, FULL, P, true>
    -- float32 the wave tiles in registers, float64 the wave tiles resident in LDS; float32 moments in mode 3 (a lane sees
    at most 12 particles), float64 in mode 1.
  * default ("one round"): min_tpw = 2 gives 2 chunks, 2 B workgroups lie between 3 and 12 CUs' worth, the cap of 3 per CU makes
    it ONE workgroup of three tiles per sample.  Its tiles 0 and 1 are whole and leave as tiles; in tile 2 wave 0 is whole
    (a tile, fetched one iteration ahead), wave 1 is cut to 3 particles (per-particle accesses, clamped addresses, nothing
    prefetched for it), waves 2 and 3 lie past the end and leave the loop.
  * LYNX_ONE_ROUND = 0: two workgroups of two tiles.  The second starts on the cut tile (the prologue's fetch is the one that
    finds wave 1 cut and waves 2, 3 absent) and its second tile lies wholly past the end: the prefetch of iteration 0 finds
    nothing for any wave, and iteration 1 leaves the loop.
  * LYNX_XPOSE = 0, what the bits are compared with: the strided form, float32 u = 4 (three tiles of 1024), float64 u = 1
    (five tiles of 256), one workgroup per sample.
Both forms apply the same apply_step to the same table, so the particles must be equal bit for bit; the moment sums differ
in their order and are held to the oracle alone.

The outputs of every call lie in ONE lynx_buf_alloc block with a guard of 64 KiB (more than two workgroup tiles) in front of
and behind each; the block is filled with 0xA5 before the call and read back whole: nothing is written behind particle
N - 1 of the last sample, nor anywhere else outside the outputs -- and a call without d_p_out writes no particle at all.
"""

import ctypes as C

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import covariance_distances, make_lattice, moment_distances, rel_err, tri_slot
from .test_gpu_parity import TOL_MOM, TOL_P

pytestmark = pytest.mark.gpu

N_OF = {np.float32: 2 * 1024 + 256 + 3, np.float64: 2 * 512 + 128 + 3}
GUARD, FILL = 64 << 10, 0xA5
TRACK_MOMENTS, TRACK_COVARIANCE = 1, 16
KNOBS = ("LYNX_XPOSE", "LYNX_ONE_ROUND", "LYNX_UNROLL", "LYNX_MOM", "LYNX_MIN_TILES_PER_WG")

_cases = {}


class Case:
    """Lattice handle, inputs on the device, the oracle's outgoing beam, and the block the outputs go to -- per dtype, once."""

    def __init__(self, lx, dtype):
        from lynx_amd import engine

        self.rt = rt = lx.device.get_runtime()
        self.dtype, self.N = np.dtype(dtype), N_OF[dtype]
        self.B = B = 2 * rt.info()["compute_units"]
        f = lambda v: np.full(B, v, dtype=dtype)  # noqa: E731
        desc = [("drift", dict(length=f(0.7))), ("quadrupole", dict(length=f(0.2), k1=np.linspace(4.2, -3.0, B).astype(dtype))),
                ("drift", dict(length=f(0.4))), ("hcor", dict(length=f(0.1), angle=f(1e-4)))]
        elements, specs = make_lattice(desc, dtype, lx)
        self.host_p = o.gaussian_particles((B,), self.N, seed=31, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
        self.host_e = np.full(B, 1e8, dtype=dtype)
        self.ref = o.segment_track(specs, o.particle_beam(self.host_p, self.host_e, dtype), dtype)
        self.ref_moments = o.beam_moments(self.ref, ddof=1)
        self.segment = lx.Segment(elements)
        self.cache = engine.LatticeCache()
        program, = engine.plan(self.segment, self.segment.elements, False, fuse_observers=True)
        self.lat = engine._ready(self.cache, program, (B,), self.dtype, self.host_e)
        assert self.lat.S == 1, self.lat.S  # the single map
        self.p_in, self.e_in = rt.to_device(self.host_p), rt.to_device(self.host_e)
        # [guard] p_out [guard] e_out [guard] mom [guard], every array on 256 bytes
        up = lambda n: -(-n // 256) * 256  # noqa: E731
        self.spans, cursor = {}, GUARD
        for name, nbytes in (("p_out", self.host_p.nbytes), ("e_out", self.host_e.nbytes), ("mom", B * 36 * 8)):
            self.spans[name] = (cursor, cursor + nbytes)
            cursor = up(cursor + nbytes + GUARD)
        self.nbytes = cursor
        self.base = rt.alloc(self.nbytes)

    def close(self):
        self.rt.sync()
        self.rt.free(self.base)

    def run(self, flags, store=True):
        """One lynx_track_particles call into the block; returns {name: array}, after the check that nothing else was written."""
        rt, ptr = self.rt, lambda name: C.c_void_p(self.base + self.spans[name][0])  # noqa: E731
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(self.base), FILL, self.nbytes))
        rt.check(rt.lib.lynx_track_particles(rt.ctx, self.lat.handle, self.N, C.c_void_p(self.e_in.ptr), C.c_void_p(self.p_in.ptr),
                                             ptr("p_out") if store else None, ptr("e_out"), ptr("mom"), flags, None))
        block = np.empty(self.nbytes, dtype=np.uint8)
        rt.check(rt.lib.lynx_buf_d2h(rt.ctx, block.ctypes.data, C.c_void_p(self.base), block.nbytes))
        written = {name: span for name, span in self.spans.items() if store or name != "p_out"}
        cursor = 0
        for name, (start, stop) in sorted(written.items(), key=lambda item: item[1]) + [(None, (self.nbytes, self.nbytes))]:
            stray = np.flatnonzero(block[cursor:start] != FILL)
            if stray.size:
                last = self.spans["p_out"][1]
                raise AssertionError(f"{stray.size} byte(s) written outside the outputs; the first: block byte {cursor + stray[0]} "
                                     f"({cursor + stray[0] - last:+d} from the end of the last sample's particles)")
            cursor = stop
        view = lambda name, t, shape: block[slice(*self.spans[name])].view(t).reshape(shape)  # noqa: E731
        out = {"e_out": view("e_out", self.dtype, (self.B,)), "mom": view("mom", np.float64, (self.B, 36))}
        if store:
            out["p_out"] = view("p_out", self.dtype, (self.B, self.N, 7))
        return out


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    yield lynx_amd
    for case in _cases.values():
        case.close()
    _cases.clear()


def case_of(lx, dtype):
    if dtype not in _cases:
        _cases[dtype] = Case(lx, dtype)
    return _cases[dtype]


def knobs(monkeypatch, **values):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in values.items():
        monkeypatch.setenv(f"LYNX_{name}", str(value))


def moments_of(record):
    """The reference's properties from (B, 36) records, as ParticleBeam reads them (unbiased sigmas, biased products)."""
    n = record[:, 35]
    out = {f"mu_{c}": record[:, k] for k, c in enumerate(("x", "xp", "y", "yp", "s", "p"))}
    out.update({f"sigma_{c}": np.sqrt(record[:, tri_slot(k, k)] * (n / (n - 1))) for k, c in enumerate(("x", "xp", "y", "yp", "s", "p"))})
    out.update(sigma_xxp=record[:, tri_slot(0, 1)], sigma_yyp=record[:, tri_slot(2, 3)])
    return out


def check_against_the_oracle(case, out, what, dtype, whole_triangle):
    if "p_out" in out:
        for c in range(7):
            err = rel_err(out["p_out"][..., c], case.ref["particles"][..., c])
            assert err < TOL_P[dtype], (what, c, err)
    assert out["e_out"].tobytes() == case.host_e.tobytes(), what  # no cavity: the beam leaves with the energy it came with
    record = out["mom"]
    assert np.all(record[:, 35] == case.N) and np.all(record[:, 34] == (1.0 if whole_triangle else 0.0)), what
    d = moment_distances(moments_of(record), case.ref_moments)
    print(f"{what}: worst moment distance {max(d.values()):.2e}")
    assert max(d.values()) <= TOL_MOM[dtype], (what, d)
    if whole_triangle:
        cov = np.empty((case.B, 6, 6))
        for i in range(6):
            for j in range(6):
                cov[:, i, j] = record[:, tri_slot(i, j)]
        worst, at = covariance_distances(cov, case.ref["particles"])
        print(f"{what}: worst covariance distance {worst:.2e} at {at}")
        assert worst <= TOL_MOM[dtype], (what, worst, at)


ROUNDS = [{}, {"ONE_ROUND": 0}]  # one workgroup of three tiles | two of two: the second starts on the cut tile


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_tile_of_a_whole_a_cut_and_two_absent_waves_equals_the_strided_form_bit_for_bit(lx, dtype, monkeypatch):
    """Moments on, out of place (the module's docstring says which form each call reaches)."""
    case = case_of(lx, dtype)
    knobs(monkeypatch, XPOSE=0)
    strided = case.run(TRACK_MOMENTS)
    check_against_the_oracle(case, strided, "strided", dtype, False)
    for extra in ROUNDS:
        knobs(monkeypatch, XPOSE=1, **extra)
        tiles = case.run(TRACK_MOMENTS)
        what = f"wave tiles {extra}"
        check_against_the_oracle(case, tiles, what, dtype, False)
        differ = np.flatnonzero((tiles["p_out"].view(np.uint8) != strided["p_out"].view(np.uint8)).reshape(-1))
        assert differ.size == 0, (what, f"{differ.size} bytes differ from the strided form; the first in scalar {differ[0] // case.dtype.itemsize}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_whole_covariance_and_the_call_without_a_store_on_the_same_tiles(lx, dtype, monkeypatch):
    """LYNX_TRACK_COVARIANCE (the FULL sums) through the wave tiles, and lynx_track_particles with a null d_p_out: the same
    sums from the same particles in the same order -- the same record bit for bit -- and no particle written."""
    case = case_of(lx, dtype)
    for extra in ROUNDS:
        knobs(monkeypatch, XPOSE=1, **extra)
        full = case.run(TRACK_COVARIANCE)
        check_against_the_oracle(case, full, f"whole covariance {extra}", dtype, True)
        stored = case.run(TRACK_MOMENTS)
        unstored = case.run(TRACK_MOMENTS, store=False)
        check_against_the_oracle(case, unstored, f"no store {extra}", dtype, False)
        assert unstored["mom"].tobytes() == stored["mom"].tobytes(), extra
