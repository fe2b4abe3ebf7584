"""
The moment reduction (k_reduce_moments<FINAL>, k_reduce_moments_ticket) at the row counts where a level changes shape.

A sample's rows are the records of its streaming workgroups.  The read-only pass (lynx_moments: S = 0) under LYNX_UNROLL = 1,
LYNX_MIN_TILES_PER_WG = 1 and LYNX_ONE_ROUND = 0 gives one workgroup per tile of 256 particles (lynx_hip.hip, plan_track:
u = 1, so no wave tiles; min_tpw = 1; no cap of one round; chunks = min(tiles, ceil(512 CUs / B)) = tiles at every shape
here, asserted from `rt.info()["compute_units"]`): rows = ceil(N / 256), and a last row of N - 256 (rows - 1) particles.

reduce_moment_records then walks (kReduceStage = 70 rows staged per pass, 7 sets of 36 threads):
  rows <= 70   k_reduce_moments<true> alone: one workgroup per sample, one pass.
  rows >  70   rows_per_group = max(ceil(rows / 64), B <= 4 ? 32 : 1), groups = ceil(rows / rows_per_group) <= 64; by default one
               launch of k_reduce_moments_ticket (a group's rows, publish, ticket; the last arrival adds the group records in
               group order), with LYNX_REDUCE_TICKET = 0 k_reduce_moments<false> and then k_reduce_moments<true> over `groups` rows.
The cases (B, rows, N, dtype):
  (1, 70, 17 920)      the final kernel alone, the staging area full to its last row, every row whole.
  (1, 71, 17 921)      rows_per_group 32: groups of 32, 32 and 7 rows; the last row holds one particle.
  (1, 97, 24 700)      rows_per_group 32: 32, 32, 32 and a last group of a single row (of 124 particles).
  (1, 4482, 1 147 137) ceil(4482 / 64) = 71 rows per group -- one more than a stage, so every group makes a second pass of one
                       row --, ceil(4482 / 71) = 64 groups, the last of 4482 - 63 * 71 = 9 rows, the last row of one particle.
  (5, 71, 17 921)      rows_per_group max(2, 1) = 2: 36 groups, the last of one row of one particle.
  (5, 70, 17 920)      the final kernel alone, five workgroups.
  (1, 71, 17 921) in float32: the rows come from the float32 streaming kernel (the reduction itself is float64 throughout).

Per case, with the property set and with the whole covariance:
  * the default (ticket) form against the oracle within TOL_MOM (test_gpu_parity.py), every covariance entry included when asked for;
  * the default form three times more: the same bits;
  * LYNX_REDUCE_TICKET = 0: the same NaN pattern, and within rtol = 1e-11 (the bounds of
    test_the_two_forms_of_the_moment_reduction_agree; measured: equal bits in every case here -- with at most 64 groups the
    second level is one stage pass in both forms, the same sums in the same order);
  * slots 28..33 zero, slot 34 the flag asked for, slot 35 N (tests/entry_footprint.py: moment_record_constants).
"""

import ctypes as C

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import entry_footprint as fp
from .helpers import covariance_distances, moment_distances

pytestmark = pytest.mark.gpu

TOL_MOM = {np.float32: 1e-4, np.float64: 1e-6}  # test_gpu_parity.py
KNOBS = {"LYNX_UNROLL": "1", "LYNX_MIN_TILES_PER_WG": "1", "LYNX_ONE_ROUND": "0"}
# (B, rows, N, dtype)
CASES = [(1, 70, 17_920, np.float64), (1, 71, 17_921, np.float64), (1, 97, 24_700, np.float64), (1, 4482, 4481 * 256 + 1, np.float64),
         (5, 71, 17_921, np.float64), (5, 70, 17_920, np.float64), (1, 71, 17_921, np.float32)]


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


_beams = {}


@pytest.fixture(scope="module", autouse=True)
def _forget_the_beams():
    yield
    _beams.clear()


def beam_of(B, N, dtype):
    """The particles of one case and the oracle's moments of them, made once for both flags."""
    key = (B, N, np.dtype(dtype))
    if key not in _beams:
        P = o.gaussian_particles((B,), N, seed=11 + B, dtype=dtype, mu=[2e-4, -1e-5, 3e-4, 2e-5, 1e-5, -1e-3],
                                 sigma=[1e-4, 1e-5, 2e-4, 3e-5, 1e-5, 1e-3])
        energy = np.full(B, 1e8, dtype=dtype)
        _beams[key] = (P, energy, o.beam_moments(o.particle_beam(P, energy, dtype), ddof=1))
    return _beams[key]


@pytest.mark.parametrize("covariance", [False, True], ids=["properties", "covariance"])
@pytest.mark.parametrize("B, rows, N, dtype", CASES, ids=[f"B{B}-{rows}rows-{np.dtype(t).name}" for B, rows, _, t in CASES])
def test_the_levels_of_the_moment_reduction_at_the_row_counts_where_they_change_shape(lx, B, rows, N, dtype, covariance, monkeypatch):
    """See the module's docstring: the derivation of every case, and what is asserted."""
    from lynx_amd.device import dtype_code, get_runtime

    rt = get_runtime()
    cus = rt.info()["compute_units"]
    assert rows == -(-N // 256) and B * rows <= 512 * cus, (rows, N, cus)
    for key, value in KNOBS.items():
        monkeypatch.setenv(key, value)
    P, energy, ref = beam_of(B, N, dtype)
    beam = lx.ParticleBeam(P, energy, dtype=dtype)
    ticket = beam.moment_record(covariance=covariance).copy()
    d = moment_distances(beam, ref)
    print(f"B = {B}, {rows} rows, {np.dtype(dtype).name}, covariance = {covariance}: worst moment {max(d.values()):.2e}")
    assert max(d.values()) <= TOL_MOM[dtype], d
    if covariance:
        worst, where = covariance_distances(beam.covariance(), P)
        print(f"  worst covariance entry {worst:.2e} at {where}")
        assert worst <= TOL_MOM[dtype], (worst, where)
    fp.moment_record_constants(ticket, counts=np.full(B, N), whole_triangle=covariance)

    p = beam._particles.device(rt)
    rec = rt.empty((B, 36), np.float64)

    def again():
        rt.check(rt.lib.lynx_moments(rt.ctx, dtype_code(dtype), B, N, C.c_void_p(p.ptr), C.c_void_p(rec.ptr), 1 if covariance else 0))
        return rec.numpy()

    for _ in range(3):
        assert np.array_equal(again().view(np.uint64), ticket.view(np.uint64))
    monkeypatch.setenv("LYNX_REDUCE_TICKET", "0")
    levels = again()
    have = ~np.isnan(ticket)
    assert np.array_equal(np.isnan(levels), ~have)
    assert np.allclose(ticket[have], levels[have], rtol=1e-11, atol=1e-300)
    print(f"  two launches against one: worst relative difference {np.max(np.abs(levels[have] - ticket[have]) / (np.abs(ticket[have]) + 1e-300)):.2e}")
    fp.moment_record_constants(levels, counts=np.full(B, N), whole_triangle=covariance)
