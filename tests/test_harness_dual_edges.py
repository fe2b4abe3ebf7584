"""
The dual-number builders (lynx_amd/csrc/lynx_dual.hpp) that give k_build_bwd every dM/dtheta, against a 50-digit
restatement of the maps (tests/hp_maps.py) at the edges where the reference's formulas cancel: quadrupoles near and at
k1 = 0, bends of small angle, weak solenoids, weak and off-crest cavities.  Both instantiations (float, double) and both
builders the reverse pass uses (the dense `build_element` and the 16-entry `build_entries_u`), every parameter and the
beam energy.  The float32 duals are evaluated at the float32-rounded inputs and compared with the reference at those
same inputs.

Bar for each entry of one dM, with `scale` = the largest |exact| entry of that dM:
  Dual<double>  |got - exact| <= 1e-9 |exact| + 1e-12 scale
  Dual<float>   |got - exact| <= 1e-3 |exact| + 1e-5 scale
The cavity's T566 / T556 / T555 are held to measured bounds instead (CAVITY_T5XX_BOUNDS).
"""

import ctypes as C
import functools

import numpy as np
import pytest

from lynx_amd import _ffi
from oracle import lynx_oracle as o

from . import hp_maps as hp

UNIT_ENTRIES = (0, 1, 6, 7, 8, 13, 16, 17, 20, 23, 24, 27, 32, 33, 39, 40)  # lynx_unit_record.hpp: unit_entry_u
BARS = {np.float64: (1e-9, 1e-12), np.float32: (1e-3, 1e-5)}
NPARAMS = {_ffi.KIND_QUADRUPOLE: 5, _ffi.KIND_DIPOLE: 8, _ffi.KIND_SOLENOID: 4, _ffi.KIND_CAVITY: 4}
CAV = _ffi.FLAG_CAV_BETA | _ffi.FLAG_CAV_GAIN | _ffi.FLAG_CAV_T5XX

# d(T566, T556, T555)/dtheta on the cavity grid below: |got - exact| <= bound |exact|, the measured worst case (times
# two).  These three are the reference's formulas with (gamma0 - gamma1)^(1..3) in their denominators, whose numerators
# cancel to O((gamma0 - gamma1)^2 / gamma^2) of their terms: written as the reference writes them they lose that many
# digits in the value the forward pass uses and in the derivative alike (float32 4e10 of the entry at V/E = 1e-3 and 89
# degrees; float64 59).  Their weight in any loss is T5xx s^2 against the map's O(1) (cavity.py:219-226): the end-to-end
# gradients stay within tolerance (tests/test_gpu_grad_edges.py).  Not fixed here: DESIGN section 2.
CAVITY_T5XX_BOUNDS = {np.float32: 1e11, np.float64: 150.0}
# The cavity's map and its first five coefficients meet the bars above only where the energy gain is not small: with
# (E_out - E_in)/E below ~1e-3 (weak, or far off crest) Ep = (Ef - Ei)/L and log(Ef/Ei) lose digits in r11..r22 and
# their derivatives.  The bars there are the ones above times these factors (measured worst case, times two: float64
# 711, float32 1.1e5, both at 1e8 eV, 100 kV, 89 degrees, d/dphase).  Not fixed here: DESIGN section 2.
CAVITY_BAR_FACTORS = {np.float32: 2.2e5, np.float64: 1.5e3}

K1_GRID = (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3, 0.1, -0.1, 4.2, -4.2, 30.0, -30.0)
ANGLE_GRID = (0.0, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, 0.2)
SOLENOID_K_GRID = (0.0, 1e-6, 1e-4, 1e-2, 2.0)


def _cases():
    out = []
    for L in (0.05, 0.2, 1.0):
        for k1 in K1_GRID:
            out.append((f"quad-L{L}-k1{k1:g}", _ffi.KIND_QUADRUPOLE, 0, [L, k1, 0.0, 0.0, 0.0], 1e8))
    for k1 in K1_GRID:
        out.append((f"quad-tilt-mis-k1{k1:g}", _ffi.KIND_QUADRUPOLE, _ffi.FLAG_TILT | _ffi.FLAG_MISALIGNED,
                    [0.2, k1, 0.3, 1e-3, -2e-3], 6e6))
        out.append((f"quad-mis-k1{k1:g}", _ffi.KIND_QUADRUPOLE, _ffi.FLAG_MISALIGNED, [1.0, k1, 0.0, 2e-4, 5e-4], 1e9))
    for a in ANGLE_GRID:
        out.append((f"dipole-{a:g}", _ffi.KIND_DIPOLE, _ffi.FLAG_THICK, [0.5, a, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1e8))
        out.append((f"dipole-edges-{a:g}", _ffi.KIND_DIPOLE, _ffi.FLAG_THICK, [0.5, a, 0.05, -0.03, 0.2, 0.4, 0.3, 0.03],
                    6e6))
        out.append((f"dipole-thin-{a:g}", _ffi.KIND_DIPOLE, 0, [0.0, a, 0.05, -0.03, 0.2, 0.4, 0.3, 0.03], 1e8))
    for k in SOLENOID_K_GRID:
        out.append((f"solenoid-{k:g}", _ffi.KIND_SOLENOID, 0, [0.5, k, 0.0, 0.0], 6e6))
        out.append((f"solenoid-mis-{k:g}", _ffi.KIND_SOLENOID, _ffi.FLAG_MISALIGNED, [0.5, k, 1e-3, -2e-3], 1e8))
    for E, V, phase in ((6e6, 6e2, 0.0), (6e6, 6e3, 30.0), (1e8, 1e4, 10.0), (1e8, 1e5, 89.0), (1e9, 1e5, 20.0),
                        (1e9, 1e8, 45.0), (6e6, 1.8e7, 89.0), (1e8, -3e6, 20.0)):
        out.append((f"cavity-E{E:g}-V{V:g}-ph{phase:g}", _ffi.KIND_CAVITY, CAV, [1.0377, V, phase, 1.3e9], E))
    return out


CASES = _cases()


def _dense(h, dtype, kind, flags, p, energy, seed):
    f32 = dtype == np.float32
    fn = h.harness_build_dual_f32 if f32 else h.harness_build_dual_f64
    ct = C.c_float if f32 else C.c_double
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ct, C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    fn.restype = None
    p = np.ascontiguousarray(p, dtype=dtype)
    M, dM, c, dc = (np.zeros(n, dtype) for n in (49, 49, 8, 8))
    fn(kind, flags, p.ctypes.data, len(p), ct(energy), seed, M.ctypes.data, dM.ctypes.data, c.ctypes.data,
       dc.ctypes.data, int(kind == _ffi.KIND_CAVITY))
    return dM.astype(np.float64), dc.astype(np.float64)


def _entries_u(h, dtype, kind, flags, p, energy, seed):
    """dM of the 16-entry builder scattered into 49 (None if the kind does not take it)."""
    f32 = dtype == np.float32
    fn = h.harness_entries_u_dual_f32 if f32 else h.harness_entries_u_dual_f64
    ct = C.c_float if f32 else C.c_double
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ct, C.c_int] + [C.c_void_p] * 4
    fn.restype = C.c_int
    p = np.ascontiguousarray(p, dtype=dtype)
    m, dm, c, dc = (np.zeros(n, dtype) for n in (16, 16, 8, 8))
    if not fn(kind, flags, p.ctypes.data, len(p), ct(energy), seed, m.ctypes.data, dm.ctypes.data, c.ctypes.data,
              dc.ctypes.data):
        return None
    dM = np.zeros(49)
    dM[list(UNIT_ENTRIES)] = dm
    return dM, dc.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _exact(kind, flags, p, energy, seed):
    return np.array(hp.param_derivative(kind, flags, p, energy, seed))


def _check(got, exact, dtype, what, map_scale=0.0, factor=1.0):
    """`map_scale`: see SANDWICH_SEEDS; `factor`: CAVITY_BAR_FACTORS."""
    rel, floor = (factor * b for b in BARS[dtype])
    scale = float(np.max(np.abs(exact))) if exact.size else 0.0
    resolution = 4 * float(np.finfo(dtype).eps) * map_scale
    if scale == 0.0:
        assert np.all(np.abs(got) <= resolution), (what, got)
        return
    err = np.abs(got - exact)
    bad = err > rel * np.abs(exact) + floor * scale + resolution
    assert not np.any(bad), (what, [(int(q), float(got[q]), float(exact[q])) for q in np.flatnonzero(bad)[:6]], scale)


# Parameters that enter a map only through the tilt and misalignment sandwiches (quadrupole.py:66-80,
# track_methods.py:101-122): their dM is a difference of map entries -- the tilt's cx - cy, the misalignment's 1 - cx --
# which is k1 L^2 small on a weak quadrupole and exists in the builders only as the difference of two rounded map
# entries.  No evaluation of the reference's operations resolves it below the map's own rounding, so its floor is 4 ulp
# of the largest map entry (in absolute terms that is what the map itself carries: 2.4e-7 in float32).
SANDWICH_SEEDS = {_ffi.KIND_QUADRUPOLE: (2, 3, 4), _ffi.KIND_DIPOLE: (4,), _ffi.KIND_SOLENOID: (2, 3)}


def _map_scale(kind, seed, p, energy):
    if seed not in SANDWICH_SEEDS.get(kind, ()):
        return 0.0
    return float(np.max(np.abs(hp.values(kind, 0, p, energy)[:49])))


def _rounded(dtype, p, energy):
    return tuple(float(v) for v in np.asarray(p, dtype=dtype)), float(dtype(energy))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dual_map_derivatives_at_the_edges(host_harness, case, dtype):
    name, kind, flags, p, energy = case
    p, energy = _rounded(dtype, p, energy)
    # the forward pass builds a quadrupole at k1 = 0 as the one at 1e-12 (track_methods.py:67-68): the dual's derivative
    # is taken there, 1e-12 of the scale from the limit (which test_the_duals_give_the_limit_at_k1_zero holds it to)
    at = p if not (kind == _ffi.KIND_QUADRUPOLE and p[1] == 0.0) else (p[0], float(dtype(1e-12))) + p[2:]
    for seed in range(NPARAMS[kind] + 1):
        exact = _exact(kind, flags, at, energy, seed)
        builders = [("dense", _dense(host_harness, dtype, kind, flags, p, energy, seed))]
        u = _entries_u(host_harness, dtype, kind, flags, p, energy, seed)
        if u is not None:
            builders.append(("entries_u", u))
        map_scale = _map_scale(kind, seed, p, energy)
        for builder, (dM, dc) in builders:
            factor = CAVITY_BAR_FACTORS[dtype] if kind == _ffi.KIND_CAVITY else 1.0
            _check(dM, exact[:49], dtype, (name, builder, "map", seed), map_scale, factor)
            if kind == _ffi.KIND_CAVITY:
                _check(dc[:5], exact[49:54], dtype, (name, builder, "coef", seed), factor=factor)
                _check_t5xx(dc[5:], exact[54:], dtype, (name, builder, "T5xx", seed))


def _check_t5xx(got, exact, dtype, what):
    assert np.all(np.isfinite(got)), (what, got)
    err = np.abs(got - exact)
    assert np.all(err <= CAVITY_T5XX_BOUNDS[dtype] * np.abs(exact)), (what, got, exact)


RBEND_CASES = [(f"rbend-{a:g}-{'edges' if e else 'plain'}", a, e) for a in ANGLE_GRID for e in (False, True)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", RBEND_CASES, ids=[c[0] for c in RBEND_CASES])
def test_rbend_angle_derivative_through_the_edge_shift(host_harness, case, dtype):
    """An RBend's dM/dangle as grad.py assembles it: d/dangle + (d/de1 + d/de2) / 2 of the dipole row it becomes."""
    name, angle, edges = case
    row = [0.5, angle, 0.05, -0.03, 0.2, 0.4, 0.3, 0.03] if edges else [0.5, angle] + [0.0] * 6
    row, energy = _rounded(dtype, row, 1e8)
    shifted = list(row)
    shifted[2] = float(dtype(row[2] + dtype(row[1]) / dtype(2)))  # rbend.py:79-80, in the element's dtype
    shifted[3] = float(dtype(row[3] + dtype(row[1]) / dtype(2)))
    parts = [_dense(host_harness, dtype, _ffi.KIND_DIPOLE, _ffi.FLAG_THICK, shifted, energy, s)[0] for s in (1, 2, 3)]
    got = parts[0] + 0.5 * (parts[1] + parts[2])
    exact = np.array(hp.rbend_angle_derivative(_ffi.FLAG_THICK, row, energy))[:49]
    _check(got, exact, dtype, name)


# --- the reference itself, before it serves as one -------------------------------------------------------------------

GENERIC = [
    ("drift", {"kind": "drift", "length": 0.7}, _ffi.KIND_DRIFT, 0, [0.7], 1e8),
    ("hcor", {"kind": "hcor", "length": 0.3, "angle": 1e-3}, _ffi.KIND_HCOR, 0, [0.3, 1e-3], 6e6),
    ("vcor", {"kind": "vcor", "length": 0.3, "angle": -2e-3}, _ffi.KIND_VCOR, 0, [0.3, -2e-3], 1e8),
    ("quad", {"kind": "quadrupole", "length": 0.2, "k1": 4.2}, _ffi.KIND_QUADRUPOLE, 0, [0.2, 4.2, 0, 0, 0], 1e8),
    ("quad-tilt-mis", {"kind": "quadrupole", "length": 0.3, "k1": -3.1, "tilt": 0.4, "misalignment": [1e-3, -2e-3]},
     _ffi.KIND_QUADRUPOLE, _ffi.FLAG_TILT | _ffi.FLAG_MISALIGNED, [0.3, -3.1, 0.4, 1e-3, -2e-3], 6e6),
    ("quad-weak", {"kind": "quadrupole", "length": 0.2, "k1": 1e-3}, _ffi.KIND_QUADRUPOLE, 0, [0.2, 1e-3, 0, 0, 0], 1e8),
    ("dipole", {"kind": "dipole", "length": 0.5, "angle": 0.12, "e1": 0.05, "e2": 0.02, "tilt": 0.3,
                "fringe_integral": 0.4, "fringe_integral_exit": 0.2, "gap": 0.03},
     _ffi.KIND_DIPOLE, _ffi.FLAG_THICK, [0.5, 0.12, 0.05, 0.02, 0.3, 0.4, 0.2, 0.03], 1e8),
    ("dipole-thin", {"kind": "dipole", "length": 0.0, "angle": 0.02, "tilt": 0.1},
     _ffi.KIND_DIPOLE, 0, [0.0, 0.02, 0, 0, 0.1, 0, 0, 0], 1e8),
    ("cavity", {"kind": "cavity", "length": 1.0377, "voltage": 1.8e7, "phase": 5.0, "frequency": 1.3e9},
     _ffi.KIND_CAVITY, CAV, [1.0377, 1.8e7, 5.0, 1.3e9], 6e6),
    ("solenoid", {"kind": "solenoid", "length": 0.5, "k": 2.0, "misalignment": [1e-3, -2e-3]},
     _ffi.KIND_SOLENOID, _ffi.FLAG_MISALIGNED, [0.5, 2.0, 1e-3, -2e-3], 6e6),
    ("undulator", {"kind": "undulator", "length": 0.8}, _ffi.KIND_UNDULATOR, 0, [0.8], 6e6),
]


@pytest.mark.parametrize("case", GENERIC, ids=[c[0] for c in GENERIC])
def test_high_precision_maps_agree_with_the_oracle(host_harness, case):
    """hp_maps at generic points: every map entry within 1e-13 of the map's scale of the oracle's float64 map, every
    cavity coefficient within 1e-13 of its own size of the float64 builder's (the oracle forms them inside its track)."""
    _, spec, kind, flags, p, energy = case
    spec = {k: (np.array([v], dtype=np.float64) if k != "kind" and v is not None else v) for k, v in spec.items()}
    if "misalignment" in spec:
        spec["misalignment"] = spec["misalignment"].reshape(1, 2)
    ref = o.element_transfer_map(spec, np.array([energy]), np.float64)[0]
    got = np.array(hp.values(kind, flags, p, energy))
    assert np.max(np.abs(got[:49].reshape(7, 7) - ref)) <= 1e-13 * np.max(np.abs(ref)), (got[:49], ref)
    if kind == _ffi.KIND_CAVITY:
        from .helpers import harness_map

        _, c64 = harness_map(host_harness, kind, flags, np.array(p), energy, np.float64, True)
        assert np.all(np.abs(got[49:] - c64) <= 1e-13 * np.abs(c64) + 1e-300), (got[49:], c64)


def test_high_precision_quadrupole_derivative_at_k1_zero_is_the_limit():
    """d M[0][1] / d k1 = -L^3 / 6 at k1 = 0 (and d M[2][3] / d k1 = +L^3 / 6): the entire function, not the 1e-12."""
    L = 0.2
    d = hp.param_derivative(_ffi.KIND_QUADRUPOLE, 0, [L, 0.0, 0.0, 0.0, 0.0], 1e8, 1)
    assert abs(d[1] + L**3 / 6) <= 1e-15 and abs(d[2 * 7 + 3] - L**3 / 6) <= 1e-15
    assert abs(d[0] + L**2 / 2) <= 1e-15 and abs(d[7] + L) <= 1e-15  # d cos / d k1, d(-k1 S) / d k1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [0, _ffi.FLAG_TILT | _ffi.FLAG_MISALIGNED], ids=["plain", "tilt-mis"])
@pytest.mark.parametrize("L", [0.05, 0.2, 1.0])
def test_the_duals_give_the_limit_at_k1_zero(host_harness, L, flags, dtype):
    """A switched-off quadrupole: dM/dk1 of both builders is the limit k1 -> 0 of the continuous map (not 0)."""
    p, energy = _rounded(dtype, [L, 0.0, 0.3, 1e-3, -2e-3], 1e8)
    exact = np.array(hp.param_derivative(_ffi.KIND_QUADRUPOLE, flags, p, energy, 1))[:49]
    got = [_dense(host_harness, dtype, _ffi.KIND_QUADRUPOLE, flags, p, energy, 1)[0]]
    u = _entries_u(host_harness, dtype, _ffi.KIND_QUADRUPOLE, flags, p, energy, 1)
    got += [u[0]] if u is not None else []
    for dM in got:
        _check(dM, exact, dtype, ("k1 = 0", L, flags))
    if flags == 0:
        L = p[0]  # as rounded to the dtype
        assert abs(exact[1] + L**3 / 6) <= 1e-12 * L**3 and abs(exact[2 * 7 + 3] - L**3 / 6) <= 1e-12 * L**3
