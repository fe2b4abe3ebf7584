"""
Not-gpu companions of tests/test_gpu_pipelined.py: the call sequences there tell a kernel that took a neighbouring
call's table, records or energy from one that took its own, and every shape lies on the side of the launch plan's
thresholds it is meant to.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import pipelined_cases as pc
from .helpers import MOMENT_KEYS, make_lattice

CSRC = Path(__file__).resolve().parent.parent / "lynx_amd" / "csrc"
TOL_MOM = {np.float32: 1e-4, np.float64: 1e-6}  # tests/test_gpu_parity.py (a gpu module: not imported here)


def _per_sample_distances(a, b):
    """(14, B): |a - b| of every moment in units of the tolerance scale of helpers.moment_distances, taken from `a`."""
    out = []
    for key in MOMENT_KEYS:
        if key.startswith("mu_"):
            s = np.abs(a[key]) + a["sigma" + key[2:]]
        elif key in ("sigma_xxp", "sigma_yyp"):
            s = a["sigma_x"] * a["sigma_xp"] if key == "sigma_xxp" else a["sigma_y"] * a["sigma_yp"]
        else:
            s = a[key]
        out.append(np.abs(np.asarray(a[key], np.float64) - np.asarray(b[key], np.float64)) / np.asarray(s, np.float64))
    return np.stack(out)


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_consecutive_calls_of_a_sequence_are_told_apart_by_their_moments(case):
    """
    The oracle at N = 2000 on every sample of every call: the moments of call j differ from those of calls j - 1 and
    j + 1 by at least 100 TOL_MOM of their scale in at least one of the 14 moments.  A kernel that read the table of a
    neighbouring call (one slot of the ring off, or a slot rebuilt too early) then cannot pass the oracle comparison
    of test_gpu_pipelined.py at TOL_MOM.
    """
    c = pc.CASES[case]
    dtype, B, K = c["dtype"], c["B"], c["K"]
    P = o.gaussian_particles((B,), 2000, seed=3, dtype=dtype, sigma=pc.SIGMA)
    e = np.full(B, c["energy"], dtype=dtype)
    moments = []
    for desc in pc.described(case):
        _, specs = make_lattice(pc.subset(desc, slice(None), dtype), dtype)
        ref = o.segment_track(specs, o.particle_beam(P, e, dtype), dtype, kick="product", compose="float64")
        moments.append({k: np.asarray(v, np.float64) for k, v in o.beam_moments(ref, ddof=1).items()})
    assert all(np.all(np.isfinite(m[k])) for m in moments for k in MOMENT_KEYS)
    for j in range(1, K):
        for a, b in ((moments[j], moments[j - 1]), (moments[j - 1], moments[j])):
            d = _per_sample_distances(a, b).max(axis=0)
            assert np.all(d >= 100 * TOL_MOM[dtype]), (case, j, float(d.min()), int(d.argmin()))


def test_the_written_values_differ_by_order_one_and_never_repeat():
    for B, K in {(c["B"], c["K"]) for c in pc.CASES.values()}:
        v = pc.written_values(B, K)
        assert v.shape == (K, B) and np.all(np.abs(v) >= 1.0) and np.all(np.abs(v) <= 5.0)
        assert np.all(np.abs(np.diff(v, axis=0)) >= 2.0) and np.all(np.sign(v[1:]) == -np.sign(v[:-1]))
        for b in range(B):
            assert len(set(v[:, b])) == K


def test_the_mirrored_thresholds_are_the_sources():
    """Every constant of pipelined_cases.py next to the line that sets it: the line is still there, with that number."""
    for name, (file, text) in pc.SOURCE_LINES.items():
        assert text in (CSRC / file).read_text(), (name, file)
    assert pc.HALF_MILLION == 512 << 10 and pc.LONG_KERNEL_BYTES == 128 << 20 and pc.ALTERNATE_BYTES == 256 << 20
    assert (pc.TABLE_SLOTS, pc.PARTIAL_RING, pc.LANES_BUILD_MIN_BATCH, pc.REDUCE_STAGE, pc.INLINE_POOL_BYTES) == (3, 4, 256, 70, 1024)


def _pool_bytes(case):
    c = pc.CASES[case]
    desc, *_ = pc.lattice(pc.LATTICE_OF[case], c["B"])
    return sum(pc.PARAMS_OF_KIND[kind] for kind, _ in desc) * c["B"] * np.dtype(c["dtype"]).itemsize


def test_every_case_lies_on_its_side_of_the_thresholds():
    C = pc.CASES
    particles = {k: c["B"] * c["N"] for k, c in C.items()}
    # the machinery is on in the four default cases and off (forced by knobs) in the small one
    for case in ("short", "long", "cavity", "order"):
        assert particles[case] >= pc.HALF_MILLION, case
    assert particles["small"] < pc.HALF_MILLION
    # short: a short call -- below 128 MiB, no cavity -- whose parameters travel in the kernel arguments; few samples
    assert pc.particle_bytes("short") < pc.LONG_KERNEL_BYTES and _pool_bytes("short") <= pc.INLINE_POOL_BYTES
    assert C["short"]["B"] < pc.LANES_BUILD_MIN_BATCH and pc.lattice("short", 4)[3] is not None
    # long: the host waits for the build (>= 128 MiB, no cavity), no alternation (< 256 MiB), lanes build, parameter
    # writes through the copy (the pool does not fit the arguments).  320 samples are five WHOLE waves of the lanes build
    # (and a cut block of the 256-thread kernels); a cut wave of samples is what the small shape (B = 5) and the reverse
    # pass's B = 300 have.
    assert pc.LONG_KERNEL_BYTES <= pc.particle_bytes("long") < pc.ALTERNATE_BYTES
    assert C["long"]["B"] >= pc.LANES_BUILD_MIN_BATCH and C["long"]["B"] % 256 != 0 and _pool_bytes("long") > pc.INLINE_POOL_BYTES
    assert C["small"]["B"] % 64 != 0
    # cavity: the same shape with cavities (never a short call, the main stream waits for the build)
    assert (C["cavity"]["B"], C["cavity"]["N"]) == (C["long"]["B"], C["long"]["N"])
    assert any(kind == "cavity" for kind, _ in pc.lattice("cavity", 320)[0])
    # order: launches alternate (>= 256 MiB); workgroup build
    assert pc.particle_bytes("order") >= pc.ALTERNATE_BYTES and C["order"]["B"] < pc.LANES_BUILD_MIN_BATCH
    # K calls wrap the table ring three times and the record ring twice (order: twice and once)
    for case, c in C.items():
        wraps = (3, 2) if case != "order" else (2, 1)
        assert c["K"] // pc.TABLE_SLOTS >= wraps[0] and c["K"] // pc.PARTIAL_RING >= wraps[1], case
    # at most 32 elements: one chunk of the workgroup build whether or not it runs underneath a kernel (build_shape)
    for case, c in C.items():
        assert len(pc.lattice(pc.LATTICE_OF[case], c["B"])[0]) <= 32, case
    # which cases the oracle checks sample by sample
    assert pc.oracle_steps("small") <= pc.ORACLE_BUDGET
    for case in ("short", "long", "cavity", "order"):
        assert pc.oracle_steps(case) > pc.ORACLE_BUDGET, case


def test_the_parameter_beam_of_the_entry_point_sequence_is_within_reach_of_float32():
    """
    The float32 ParameterBeam lattice of test_several_entry_points_share_one_context at every value of k1 written to
    it: the oracle's float32 chain with the product's arithmetic (runs composed in float64, the kick's product form)
    stays within 5e-5 of its float64 chain in every mu and diagonal cov entry but cov[4, 4] -- the rule by which
    test_gpu_fuzz accepts a float32 lattice (`_float32_conditioned`, CONDITION_F32; a gpu module, so written out
    here).  At 6 MeV the same lattice is not: that is why the beam comes in at 100 MeV.
    """
    sh = pc.ENTRY_SHAPES["P"]
    B = sh["B"]
    ops = pc.entry_order()
    assert len(ops) == 14 and {op for op, _ in ops} == {"track", "parameter", "along", "vjp"}
    assert sorted(k for op, k in ops if op == "parameter") == ["P"] * 3 and all(op in ("parameter", "along") for op, k in ops if k == "P")
    desc, quad, _, _ = pc.lattice(sh["lattice"], B)
    assert len(desc) == 13 and B >= pc.LANES_BUILD_MIN_BATCH
    values = pc.written_values(B, len(ops), seed=31)

    def distance(energy, k1):
        d = list(desc)
        d[quad] = ("quadrupole", {**d[quad][1], "k1": k1})
        out = []
        for dt in (np.float32, np.float64):
            sub = pc.subset(pc.subset(d, slice(None), np.float32), slice(None), dt)  # (the float32 values, in both chains)
            _, specs = make_lattice(sub, dt)
            pb = o.parameter_beam_from_parameters(dtype=dt, **{k: np.full(B, v, dtype=dt) for k, v in pc.ENTRY_PARAMETER_SIGMA.items()},
                                                  energy=np.full(B, energy, dtype=dt))
            out.append(o.segment_track(specs, pb, dt, kick="product", compose="float64"))
        r32, r64 = out
        sig = np.sqrt(np.abs(np.einsum("...ii->...i", r64["cov"][..., :6, :6])))
        dmu = np.abs(r32["mu"][..., :6] - r64["mu"][..., :6]) / (np.abs(r64["mu"][..., :6]) + sig)
        dcov = np.abs(np.einsum("...ii->...i", r32["cov"][..., :6, :6] - r64["cov"][..., :6, :6])) / sig**2
        dcov[..., 4] = 0
        return max(float(dmu.max()), float(dcov.max()))

    used = [i for i, (_, key) in enumerate(ops) if key == "P"]
    assert all(distance(sh["energy"], values[i]) <= 5e-5 for i in used)
    assert any(distance(6e6, values[i]) > 5e-5 for i in used)
