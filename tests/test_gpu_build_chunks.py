"""
The workgroup build (k_build) on either side of each halving of its chunk.

launch_build keeps a sample's whole step table in LDS behind the build's scratch: build_scratch_bytes(chunk, sizeof(T)), then
[S][64] step rows and S + 1 energies.  While that is more than 160 KiB and the chunk longer than 8 elements, the chunk --
the number of elements built side by side and multiplied by one tree -- is halved (more compose rounds, less scratch).
No other test gets there: the trace hands a table beyond 64 KiB to the lanes build, and the 255 .. 261-step cases of the
suite are lynx_track_moments and k_build_bwd.  So lynx_build_compose directly, on a lattice of one-element runs (drifts)
alternating with active cavities: every element a step of its own, E = S >= 128 elements, and B = 2 samples, a batch that
leaves the GPU idle (2 B <= CUs, asserted): build_shape gives chunks of build_chunk(E, 128) = 128 elements.
  build_scratch_bytes(c, 8) = (c + c / 2 + 1 + c / 4 + 1 + 2) * 49 * 8:  89 376 B at c = 128, 45 472 B at c = 64;
  build_scratch_bytes(c, 4) adds c * 49 * 4 of staging:                 114 464 B at c = 128.
  float64: 89 376 + 520 S + 8 <= 163 840 up to S = 143: 143 steps keep chunks of 128, 144 take 64;
           45 472 + 520 S + 8 <= 163 840 up to S = 227: 227 steps keep chunks of 64, 228 take 32.
  float32: 114 464 + 260 S + 4 <= 163 840 up to S = 189: 189 steps keep chunks of 128, 190 take 64.
Asserted per case:
  * the table is the lanes build's (LYNX_LANES_BUILD_MIN_BATCH = 1) within test_gpu_parity.py's bound for "one map through
    both builders" (1e-6 float32, 1e-13 float64; the 49 map entries by map_err, the other slots of a row relative to the
    slot's largest value), and the two builds' energy_out are equal;
  * every step's map is the oracle's for that element at the energy the oracle's chain has there, within the bound of
    test_element_transfer_map (TOL_MAP, ten times that for a cavity), and energy_out is the chain's within 1e-6.
lynx_build_compose does not expose the merged form of [run, cavity] pairs (it always builds step by step), so that form has no
case here.
"""

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .helpers import make_lattice, map_err, rel_err

pytestmark = pytest.mark.gpu

TOL_MAP = {np.float32: 5e-5, np.float64: 1e-11}      # test_gpu_parity.py
SAME_TABLE = {np.float32: 1e-6, np.float64: 1e-13}   # test_gpu_parity.py: the lanes build against the workgroup build
CASES = [(np.float64, 143), (np.float64, 144), (np.float64, 227), (np.float64, 228), (np.float32, 189), (np.float32, 190)]
B = 2


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd

    lynx_amd.device.get_runtime()  # raises loudly without a GPU
    return lynx_amd


def alternating(S, dtype):
    rng = np.random.default_rng(S)
    desc = []
    for s in range(S):
        if s % 2 == 0:
            desc.append(("drift", dict(length=rng.uniform(0.1, 0.6, B))))
        else:
            desc.append(("cavity", dict(length=np.full(B, 1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B),
                                        frequency=np.full(B, 1.3e9))))
    return desc


@pytest.mark.parametrize("dtype, S", CASES, ids=[f"{np.dtype(t).name}-{S}steps" for t, S in CASES])
def test_the_workgroup_build_on_either_side_of_a_halving_of_its_chunk(lx, dtype, S, monkeypatch):
    """See the module's docstring: the derivation of the step counts, and what is asserted."""
    from lynx_amd import _ffi, engine
    from lynx_amd.device import get_runtime

    rt = get_runtime()
    assert 2 * B <= rt.info()["compute_units"] and S >= 128
    elements, specs = make_lattice(alternating(S, dtype), dtype, lx)
    seg = lx.Segment(elements)
    program = engine.plan(seg, seg.elements, False)[0]
    assert len(program.steps) == S == len(program.leaves)
    e_host = np.array([1e8, 6e7], dtype=dtype)
    lat = engine._ready(engine.lattice_cache(seg), program, (B,), dtype, e_host)
    e_in = rt.to_device(e_host)
    tables, energies = {}, {}
    for name, min_batch in (("workgroup", "1000000"), ("lanes", "1")):
        monkeypatch.setenv("LYNX_LANES_BUILD_MIN_BATCH", min_batch)
        steps, e_out = rt.empty((B, S, _ffi.STEP_STRIDE), dtype), rt.empty((B,), dtype)
        rt.check(rt.lib.lynx_build_compose(rt.ctx, lat.handle, engine._ptr(e_in), engine._ptr(steps), engine._ptr(e_out)))
        tables[name], energies[name] = steps.numpy(), e_out.numpy()
    got, other = tables["workgroup"], tables["lanes"]
    maps = got[:, :, :49].reshape(B, S, 7, 7)
    d = map_err(other[:, :, :49].reshape(B, S, 7, 7), maps)
    print(f"{np.dtype(dtype).name}, {S} steps: lanes build {d:.2e} from the workgroup build")
    assert d < SAME_TABLE[dtype], d
    for slot in range(49, _ffi.STEP_STRIDE):
        assert rel_err(other[:, :, slot], got[:, :, slot]) < SAME_TABLE[dtype], slot
    assert np.array_equal(energies["workgroup"], energies["lanes"])
    e, worst = e_host.copy(), {"drift": 0.0, "cavity": 0.0}
    for s, spec in enumerate(specs):
        kind = spec["kind"]
        err = map_err(maps[:, s], o.element_transfer_map(spec, e, dtype))
        worst[kind] = max(worst[kind], err)
        assert err < TOL_MAP[dtype] * (10 if kind == "cavity" else 1), (s, kind, err)
        if kind == "cavity":
            e = (e + spec["voltage"] * np.cos(np.deg2rad(spec["phase"]))).astype(dtype)
    print(f"  worst step against the oracle's chain: {worst}")
    assert rel_err(energies["workgroup"], e) < 1e-6
