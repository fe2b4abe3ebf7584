"""
`track_along_vjp(..., moment_targets=)` on the GPU (lynx_moments_along_loss, lynx_moments_along_loss_backward).

Through the C ABI: the two kernels alone on states the test uploads, against the numpy restatement of the values and the loss
(tests/moment_loss_reference.py) and against the host rule the library had before (`grad.trace_property_cotangents`), every
difference relative to the UNCANCELLED size of what is compared; the two clamps, gamma = 0, a record of two particles and a
zero cotangent; the same bytes twice, the footprint of both entries in the arena of tests/entry_footprint.py, and every
refusal with its text.  Through the public interface: every mode against the existing path (the trace read back, the bars
formed in numpy and passed as the properties' cotangents), central differences of the oracle's chain, the combinations with
other cotangents and with the image loss, the refusals at construction, and the example.

Shapes: the kernels have one thread per (sample, target point) in workgroups of 64, and the target points come 64 per launch;
B * Q is 1, 63, 64, 65 and 132 (two launches of 2 x 64 and 2 x 2 pairs, three workgroups), points 0 and P - 1 are targets, a
point has one term or all 23.

Worst ratios seen on an MI355X (difference / (tolerance x uncancelled size); the bound is 1): values and losses 0 in every
case (the restatement's bits); cotangents in float64 2.0e-4 of 1e-12 (both forms), in float32 0.48 of 2 x 2^-24 (mu, cov form,
and the energy's cotangents of the records form).  The public interface in float32, new against existing over existing against
float64, at its closest: kicks CAV.phase 4.1e-7 against 4.6e-7, survivors moment_loss 3.7e-7 against 4.5e-7.
"""

import ctypes as C
import importlib.util
import pathlib
from collections import namedtuple

import numpy as np
import pytest

from oracle import lynx_oracle as o

from . import entry_footprint as fp
from . import moment_loss_reference as ml
from .helpers import make_lattice
from .reverse_host_fakes import fabricated_energy, fabricated_moments, fabricated_records
from .test_gpu_grad import _desc
from .test_gpu_trace_grad import _chain, _check_parameters

pytestmark = pytest.mark.gpu

INVALID = -1
PREFIX = "moment loss along the trace: "
ALL = (1 << 23) - 1
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
FORMS = pytest.mark.parametrize("form", ["records", "moments"])
# the rounding of one add into an entry of the beam's dtype, and once more where the entry was not zero
TOL32 = 2 * 2.0**-24
TOL64 = 1e-12  # (the rtol of the float64 checks of tests/test_gpu_trace_grad.py for two ways to one number)


@pytest.fixture(scope="module")
def lx(built_library):
    import lynx_amd
    import lynx_amd.grad  # noqa: F401

    lynx_amd.device.get_runtime()
    return lynx_amd


def p(array):
    return None if array is None else C.c_void_p(array.ptr)


def ints(values):
    flat = [int(v) for pair in values for v in pair]
    return (C.c_int32 * len(flat))(*flat)


# ---------------------------------------------------------------------------------------------
# the cases of the C ABI tests
# ---------------------------------------------------------------------------------------------

# (B, P, the target points, ddof): B * Q = 1, 63, 64, 65, 132
SHAPES = [(1, 3, [2], 1), (9, 9, [0, 1, 2, 4, 5, 7, 8], 0), (8, 10, [0, 2, 3, 4, 6, 7, 8, 9], 1), (13, 7, [0, 1, 3, 5, 6], 1),
          (2, 66, list(range(66)), 0)]


def masks_for(points, rng):
    """All 23 terms at the first point, one term at the next ones (every property in turn), random sets behind."""
    masks = []
    for q, _ in enumerate(points):
        if q == 0:
            masks.append(ALL)
        elif q <= 23 and q % 2 == 1:
            masks.append(1 << ((q // 2 + 7 * (q // 2 % 3)) % 23))
        else:
            masks.append(int(rng.integers(1, ALL + 1)))
    return masks


class Case:
    """States, target points and rows of one call on the host and on the device, and the reference of everything it makes."""

    def __init__(self, lx, form, dtype, shape, shared, seed=0, records=None, mu=None, cov=None, energy=None, masks=None, rows=None,
                 loss_bar=None):
        from lynx_amd.trace import BeamTrace

        B, P, points, ddof = shape
        rng = np.random.default_rng(100 * seed + B)
        self.rt, self.form, self.dtype, self.B, self.P, self.ddof = lx.device.get_runtime(), form, np.dtype(dtype), B, P, ddof
        self.code = 1 if self.dtype == np.float64 else 0
        self.energy = np.asarray(fabricated_energy((B, P), seed) if energy is None else energy).astype(dtype)
        names, lengths = [f"E{k}" for k in range(P - 1)], [1.0] * (P - 1)
        if form == "records":
            self.records = fabricated_records((B,), P, seed + 1, count=256) if records is None else records
            self.trace = BeamTrace.from_records(self.records, self.energy, lengths, names, dtype)
            values, self.kappa = ml.values_of(dtype, self.energy, records=self.records, ddof=ddof)
            self.states = {"records": self.rt.to_device(self.records)}
        else:
            made = fabricated_moments((B,), (P,), dtype, seed + 2)
            self.mu, self.cov = (made[0] if mu is None else mu.astype(dtype)), (made[1] if cov is None else cov.astype(dtype))
            self.trace = BeamTrace.from_moments(self.mu, self.cov, self.energy, lengths, names, dtype)
            values, self.kappa = ml.values_of(dtype, self.energy, mu=self.mu, cov=self.cov)
            self.states = {"mu": self.rt.to_device(self.mu), "cov": self.rt.to_device(self.cov)}
        self.states["energy"] = self.rt.to_device(self.energy)
        self.target_points = list(zip(points, masks_for(points, rng) if masks is None else masks))
        self.terms = ml.terms_of(self.target_points)
        T, self.Q = len(self.terms), len(points)
        if rows is None:  # targets a tenth or so off the values, weights around 1 / target^2
            at = np.stack([values[name][:, point] for point, name in self.terms], axis=1)
            scale = np.where(at == 0, 1.0, np.abs(at))
            rows = np.stack([at + scale * rng.uniform(0.05, 0.2, (B, T)) * rng.choice([-1, 1], (B, T)), rng.uniform(0.5, 2.0, (B, T)) / scale**2], axis=-1)
            if shared:
                rows = rows[:1]
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        self.stride = 0 if self.rows.shape[0] == 1 and shared else 2 * T
        self.d_rows = self.rt.to_device(self.rows)
        self.loss_bar = rng.uniform(0.5, 2.0, B) * rng.choice([-1, 1], B) if loss_bar is None else np.asarray(loss_bar, dtype=np.float64)
        self.d_loss_bar = self.rt.to_device(self.loss_bar)
        self.expected = ml.loss_of(self.terms, np.broadcast_to(self.rows, (B, T, 2)), values, self.kappa)
        # what the reverse call adds, by the host rule (which reads `config.std_ddof`), and its uncancelled size
        from lynx_amd import config

        with pytest.MonkeyPatch.context() as patch:
            patch.setattr(config, "std_ddof", ddof)
            self.added, self.added_size = ml.cotangents_of(self.trace, self.terms, self.loss_bar[:, None] * self.expected["bar"],
                                                           np.abs(self.loss_bar[:, None]) * self.expected["bar_size"], self.kappa)

    def common(self, **change):
        a = dict(dtype=self.code, batch=self.B, n_points=self.P, records=self.states.get("records"), mu=self.states.get("mu"),
                 cov=self.states.get("cov"), energy=self.states["energy"], ddof=self.ddof, n=self.Q, points=self.target_points,
                 rows=self.d_rows, stride=self.stride)
        a.update(change)
        return (self.rt.ctx, a["dtype"], a["batch"], a["n_points"], p(a["records"]), p(a["mu"]), p(a["cov"]), p(a["energy"]), a["ddof"],
                a["n"], None if a["points"] is None else ints(a["points"]), p(a["rows"]), a["stride"])

    def forward(self, out=None, **change):
        """-> (status, message, values (B, T), point_loss (B, Q), loss (B,))."""
        rt, T = self.rt, len(self.terms)
        out = out or (rt.empty((self.B, T), np.float64), rt.empty((self.B, self.Q), np.float64), rt.empty((self.B,), np.float64))
        names = ("values", "point_loss", "loss")
        given = [change.pop(name, block) for name, block in zip(names, out)]
        status = rt.lib.lynx_moments_along_loss(*self.common(**change), *(p(block) for block in given))
        return (status, rt.lib.lynx_last_error(rt.ctx).decode(), *(block.numpy() for block in out))

    def priors(self, seed=3):
        """Host arrays the cotangent buffers hold before the call: nothing is zero."""
        rng = np.random.default_rng(seed)
        B, P = self.B, self.P
        if self.form == "records":
            return {"grad_trace": rng.normal(size=(B, P, 36)), "energy_bar": rng.normal(size=(B, P)).astype(self.dtype)}
        return {"mu_bar": rng.normal(size=(B, P, 7)).astype(self.dtype), "cov_bar": rng.normal(size=(B, P, 7, 7)).astype(self.dtype),
                "energy_bar": rng.normal(size=(B, P)).astype(self.dtype)}

    def backward(self, priors, **change):
        """-> (status, message, {name: the buffer after the call})."""
        rt = self.rt
        blocks = {name: rt.to_device(host) for name, host in priors.items()}
        given = {name: change.pop(name, blocks.get(name)) for name in ("grad_trace", "mu_bar", "cov_bar", "energy_bar")}
        loss_bar = change.pop("loss_bar", self.d_loss_bar)
        status = rt.lib.lynx_moments_along_loss_backward(*self.common(**change), p(loss_bar), p(given["grad_trace"]), p(given["mu_bar"]),
                                                         p(given["cov_bar"]), p(given["energy_bar"]))
        return status, rt.lib.lynx_last_error(rt.ctx).decode(), {name: block.numpy() for name, block in blocks.items()}

    def reference_after(self, priors):
        """{name: (the buffer the host rule gives, its uncancelled size, where the call may add)}."""
        from lynx_amd import grad

        (mu_bar, cov_bar, energy_bar), (mu_size, cov_size, energy_size) = self.added, self.added_size
        touched_mu, touched_cov, touched_energy = ml.touched(self.target_points, self.B, self.P)
        out = {"energy_bar": (priors["energy_bar"].astype(np.float64) + energy_bar, np.abs(priors["energy_bar"]) + energy_size, touched_energy)}
        if self.form == "records":
            lead = (self.B, self.P)
            out["grad_trace"] = (priors["grad_trace"] + grad._record_cotangents(lead, mu_bar, cov_bar),
                                 np.abs(priors["grad_trace"]) + grad._record_cotangents(lead, mu_size, cov_size),
                                 ml.touched_records(self.target_points, self.B, self.P)[0])
        else:
            out["mu_bar"] = (priors["mu_bar"].astype(np.float64) + mu_bar, np.abs(priors["mu_bar"]) + mu_size, touched_mu)
            out["cov_bar"] = (priors["cov_bar"].astype(np.float64) + cov_bar, np.abs(priors["cov_bar"]) + cov_size, touched_cov)
        return out


def worst_ratio(got, want, size, tolerance):
    """max |got - want| / (tolerance size) over the entries with a size; an entry of size 0 must be exact."""
    got, want, size = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(size, dtype=np.float64)
    assert got.shape == want.shape == size.shape, (got.shape, want.shape, size.shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), "a value is not finite"
    none = size == 0
    assert np.array_equal(got[none], want[none])
    return float(np.max(np.abs(got - want)[~none] / (tolerance * size[~none]), initial=0.0))


def check_backward(case, priors, after):
    """Every buffer against the host rule; an entry nothing is added into keeps its bytes.  Returns the worst ratio."""
    worst = 0.0
    for name, (want, size, touched) in case.reference_after(priors).items():
        have = after[name]
        assert have.dtype == priors[name].dtype and have.shape == priors[name].shape
        kept = ~touched
        assert have[kept].tobytes() == priors[name][kept].tobytes(), f"{name}: an entry nothing is added into has changed"
        tolerance = TOL64 if have.dtype == np.float64 else TOL32
        ratio = worst_ratio(have[touched], want[touched], size[touched], tolerance)
        assert ratio <= 1, (name, ratio)
        worst = max(worst, ratio)
    return worst


# ---------------------------------------------------------------------------------------------
# 6. the two kernels alone
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shared", [True, False], ids=["shared rows", "rows per sample"])
@DTYPES
@FORMS
def test_the_kernels_alone_against_the_restatement_and_the_host_rule(lx, form, dtype, shared):
    worst = {"values": 0.0, "loss": 0.0, "cotangents": 0.0}
    for seed, shape in enumerate(SHAPES):
        case = Case(lx, form, dtype, shape, shared, seed)
        status, message, values, point_loss, loss = case.forward()
        assert status == 0, message
        e = case.expected
        worst["values"] = max(worst["values"], worst_ratio(values, e["value"], e["value_size"], TOL64))
        worst["loss"] = max(worst["loss"], worst_ratio(point_loss, e["point_loss"], e["point_loss_size"], TOL64),
                            worst_ratio(loss, e["loss"], e["loss_size"], TOL64))
        priors = case.priors()
        status, message, after = case.backward(priors)
        assert status == 0, message
        worst["cotangents"] = max(worst["cotangents"], check_backward(case, priors, after))
        assert any(not np.array_equal(after[name], priors[name]) for name in priors)
    print(f"{form} {np.dtype(dtype).name} {'shared' if shared else 'per sample'}: worst ratios {worst}")
    assert worst["values"] <= 1 and worst["loss"] <= 1


# ---------------------------------------------------------------------------------------------
# 7. clamps and edges
# ---------------------------------------------------------------------------------------------


def bits(*names):
    return ml.mask_of(names)


@DTYPES
def test_a_variance_below_the_floor_gives_the_floors_square_root_and_no_derivative(lx, dtype):
    B, P = 2, 3
    mu, cov = fabricated_moments((B,), (P,), dtype, 4)
    cov[0, 1, 0, 0], cov[1, 1, 0, 0] = 1e-21, 0.0
    case = Case(lx, "moments", dtype, (B, P, [1], 0), False, mu=mu, cov=cov, masks=[bits("sigma_x", "mu_x")])
    status, message, values, _, _ = case.forward()
    assert status == 0, message
    floor = float(np.dtype(dtype).type(1e-20))
    assert np.all(np.abs(values[:, 1] - np.sqrt(floor)) <= 1e-15 * np.sqrt(floor)) and np.array_equal(values[:, 0], mu[:, 1, 0].astype(np.float64))
    priors = case.priors()
    status, message, after = case.backward(priors)
    assert status == 0, message
    assert np.array_equal(after["cov_bar"], priors["cov_bar"])  # clamped: the derivative is 0, and prior + 0 is the prior
    assert np.all(after["mu_bar"][:, 1, 0] != priors["mu_bar"][:, 1, 0]) and check_backward(case, priors, after) <= 1


@DTYPES
def test_a_plane_without_area_gives_no_derivative_through_the_emittance(lx, dtype):
    """cov = v v^T in the x plane with v = (2^-13, 2^-16): s2 p2 and cross^2 are both 2^-58 exactly, q = 0 <= tiny."""
    B, P = 2, 3
    mu, cov = fabricated_moments((B,), (P,), dtype, 5)
    cov[:, 2, 0, 0], cov[:, 2, 1, 1], cov[:, 2, 0, 1], cov[:, 2, 1, 0] = 2.0**-26, 2.0**-32, 2.0**-29, 2.0**-29
    tiny = float(np.finfo(dtype).tiny)
    weight = 1e-200 if np.dtype(dtype) == np.float64 else 1e-20  # (beta = s2 / sqrt(tiny) is 1e146 in float64: keep the bars finite)
    for names in (("emittance_x",), ("beta_x",), ("alpha_x",), ("emittance_x", "beta_x", "alpha_x")):
        rows = np.tile([[0.0, weight]], (1, len(names), 1))
        case = Case(lx, "moments", dtype, (B, P, [2], 0), True, mu=mu, cov=cov, masks=[bits(*names)], rows=rows)
        status, message, values, _, _ = case.forward()
        assert status == 0, message
        want = {"emittance_x": np.sqrt(tiny), "beta_x": 2.0**-26 / np.sqrt(tiny), "alpha_x": -(2.0**-29) / np.sqrt(tiny)}
        order = [name for name in ml.PROPERTIES if name in names]
        assert np.allclose(values, [[want[name] for name in order]] * B, rtol=1e-14, atol=0.0)
        priors = case.priors()
        status, message, after = case.backward(priors)
        assert status == 0, message
        if names == ("emittance_x",):  # everything goes through eps: zero bars, the three entries keep their values
            assert np.array_equal(after["cov_bar"], priors["cov_bar"])
        else:  # beta and alpha also depend on s2 and cross directly: only that part is added
            direct = np.zeros((B, 7, 7))
            for t, name in enumerate(order):
                bar = case.loss_bar * 2.0 * weight * want[name]
                if name == "beta_x":
                    direct[:, 0, 0] += bar / np.sqrt(tiny)
                elif name == "alpha_x":
                    direct[:, 0, 1] += -bar / np.sqrt(tiny)
            added = after["cov_bar"][:, 2].astype(np.float64) - priors["cov_bar"][:, 2].astype(np.float64)
            assert np.all(added[:, 1, 1] == 0) and np.all(direct[:, 0, 0] + direct[:, 0, 1] != 0)
            assert np.allclose(added, direct, rtol=1e-6 if np.dtype(dtype) == np.float32 else 1e-12, atol=0.0)
        assert check_backward(case, priors, after) <= 1  # ... which is what the host rule gives


@DTYPES
@FORMS
def test_at_gamma_zero_the_normalized_emittance_is_zero_and_has_no_derivative(lx, form, dtype):
    B, P = 2, 4
    energy = fabricated_energy((B, P), 6)
    energy[:, 3] = 0.0
    case = Case(lx, form, dtype, (B, P, [1, 3], 1), True, seed=6, energy=energy,
                masks=[bits("normalized_emittance_x", "normalized_emittance_y"), bits("normalized_emittance_x", "normalized_emittance_y")],
                rows=np.array([[[1e-7, 1.0], [2e-7, 1.0], [1e-7, 1.0], [2e-7, 1.0]]]))
    status, message, values, point_loss, _ = case.forward()
    assert status == 0, message
    assert np.all(values[:, 2:] == 0) and np.all(values[:, :2] > 0) and np.allclose(point_loss[:, 1], 1e-14 + 4e-14, rtol=1e-14)
    priors = case.priors()
    status, message, after = case.backward(priors)
    assert status == 0, message
    for name in priors:  # at the point of gamma = 0 every entry keeps its value; at the other point the covariance's move
        assert np.array_equal(after[name][:, 3], priors[name][:, 3])
        assert name in ("mu_bar", "energy_bar") or not np.array_equal(after[name][:, 1], priors[name][:, 1])
    assert check_backward(case, priors, after) <= 1


@DTYPES
def test_a_record_of_two_particles_and_of_one(lx, dtype):
    B, P = 2, 3
    records = fabricated_records((B,), P, 7, count=256)
    records[:, 1, 35] = 2.0
    case = Case(lx, "records", dtype, (B, P, [1, 2], 1), False, records=records, masks=[ALL, ALL])
    status, message, values, _, _ = case.forward()
    assert status == 0, message
    sigma_x = [t for t, term in enumerate(case.terms) if term == (1, "sigma_x")][0]
    assert np.allclose(values[:, sigma_x], np.sqrt(records[:, 1, 7] * 2.0), rtol=1e-15)  # n / (n - ddof) = 2
    assert worst_ratio(values, case.expected["value"], case.expected["value_size"], TOL64) <= 1
    priors = case.priors()
    status, message, after = case.backward(priors)
    assert status == 0, message
    assert check_backward(case, priors, after) <= 1
    # n - ddof == 0: what the host rule gives, inf or NaN, and no error
    records[:, 1, 35] = 1.0
    lone = Case.__new__(Case)
    lone.__dict__.update(case.__dict__)
    lone.states = {"records": case.rt.to_device(records), "energy": case.states["energy"]}
    status, message, values, _, loss = lone.forward()
    assert status == 0, message
    with np.errstate(all="ignore"):
        want, _ = ml.values_of(dtype, case.energy, records=records, ddof=1)
    expected = np.stack([want[name][:, point] for point, name in case.terms], axis=1)
    assert np.array_equal(np.isnan(values), np.isnan(expected)) and np.array_equal(np.isinf(values), np.isinf(expected))
    assert np.isinf(values[:, sigma_x]).all() and np.isnan(values).any() and not np.isfinite(loss).any()
    finite = np.isfinite(expected)
    assert np.allclose(values[finite], expected[finite], rtol=1e-12, atol=0.0)


@DTYPES
@FORMS
def test_a_loss_bar_of_zero_adds_exactly_zero_for_that_sample(lx, form, dtype):
    shape = (3, 5, [0, 2, 4], 1)
    case = Case(lx, form, dtype, shape, False, seed=8, masks=[ALL, bits("beta_y"), ALL], loss_bar=[1.5, 0.0, -2.0])
    priors = case.priors()
    status, message, after = case.backward(priors)
    assert status == 0, message
    for name in priors:
        assert after[name][1].tobytes() == priors[name][1].tobytes() and after[name][0].tobytes() != priors[name][0].tobytes()
    assert check_backward(case, priors, after) <= 1


# ---------------------------------------------------------------------------------------------
# 8. the same bytes twice, the footprint, the refusals
# ---------------------------------------------------------------------------------------------

Array = namedtuple("Array", "name dtype shape role")


def arena_arrays(case, entry):
    B, P, T, Q, t = case.B, case.P, len(case.terms), case.Q, case.dtype
    states = ([Array("records", np.float64, (B, P, 36), "in")] if case.form == "records"
              else [Array("mu", t, (B, P, 7), "in"), Array("cov", t, (B, P, 7, 7), "in")])
    shared = states + [Array("energy", t, (B, P), "in"), Array("rows", np.float64, case.rows.shape, "in")]
    if entry == "forward":
        return shared + [Array("values", np.float64, (B, T), "out"), Array("point_loss", np.float64, (B, Q), "out"),
                         Array("loss", np.float64, (B,), "out")]
    bars = ([Array("grad_trace", np.float64, (B, P, 36), "inout")] if case.form == "records"
            else [Array("mu_bar", t, (B, P, 7), "inout"), Array("cov_bar", t, (B, P, 7, 7), "inout")])
    return shared + [Array("loss_bar", np.float64, (B,), "in")] + bars + [Array("energy_bar", t, (B, P), "inout")]


def run_in_arena(case, entry, value, priors):
    """The call with every array inside one block filled with `value`: (the plan, the block before, the block after)."""
    rt = case.rt
    arrays = arena_arrays(case, entry)
    arena = fp.plan_arena(arrays)
    fp.check_plan(arena)
    host = {"records": getattr(case, "records", None), "mu": getattr(case, "mu", None), "cov": getattr(case, "cov", None),
            "energy": case.energy, "rows": case.rows, "loss_bar": case.loss_bar, **priors}
    base = rt.alloc(arena.nbytes)
    try:
        at = lambda name: C.c_void_p(base + arena.regions[name].start) if name in arena.regions else None  # noqa: E731
        rt.check(rt.lib.lynx_buf_memset(rt.ctx, C.c_void_p(base), value, arena.nbytes))
        before = np.full(arena.nbytes, value, dtype=np.uint8)
        for a in arrays:
            if a.role == "out":
                continue
            block = np.ascontiguousarray(host[a.name], dtype=a.dtype)
            assert block.shape == tuple(a.shape), (a.name, block.shape, a.shape)
            arena.view(before, a.name)[...] = block
            rt.check(rt.lib.lynx_buf_h2d(rt.ctx, at(a.name), block.ctypes.data, block.nbytes))
        common = (rt.ctx, case.code, case.B, case.P, at("records"), at("mu"), at("cov"), at("energy"), case.ddof, case.Q,
                  ints(case.target_points), at("rows"), case.stride)
        if entry == "forward":
            status = rt.lib.lynx_moments_along_loss(*common, at("values"), at("point_loss"), at("loss"))
        else:
            status = rt.lib.lynx_moments_along_loss_backward(*common, at("loss_bar"), at("grad_trace"), at("mu_bar"), at("cov_bar"), at("energy_bar"))
        assert status == 0, rt.lib.lynx_last_error(rt.ctx).decode()
        after = np.empty(arena.nbytes, dtype=np.uint8)
        rt.check(rt.lib.lynx_buf_d2h(rt.ctx, after.ctypes.data, C.c_void_p(base), after.nbytes))
        return arena, before, after
    finally:
        rt.sync()
        rt.free(base)


@DTYPES
@FORMS
def test_both_entries_write_their_outputs_and_nothing_else_and_the_same_bytes_twice(lx, form, dtype):
    case = Case(lx, form, dtype, (5, 13, [0, 3, 4, 12], 1), False, seed=9, masks=[ALL, bits("beta_x", "mu_y"), bits("energy"), ALL])
    # (small priors, so that every bar added moves its entry in float32 as well: d loss / d energy is 1e-8)
    priors = {name: (host * 1e-12).astype(host.dtype) for name, host in case.priors().items()}
    touched = case.reference_after(priors)
    for entry in ("forward", "backward"):
        runs = []
        for value in (0x00, 0xFF):
            arena, before, after = run_in_arena(case, entry, value, priors if entry == "backward" else {})
            fp.nothing_else_written(arena, before, after)
            if entry == "backward":
                for name in priors:
                    fp.inout_changed_only(arena, before, after, name, touched[name][2])
                    changed = arena.view(before, name) != arena.view(after, name)
                    assert np.array_equal(changed, touched[name][2]), f"{name}: a named entry did not change"
            runs.append(after)
        fp.outputs_identical(arena, runs[0], runs[1])
        for name in (priors if entry == "backward" else ()):  # the prior content is data: the same in both fills, so is the result
            fp.same_as(arena, runs[0], name, arena.view(runs[1], name))
        # ... and the same bytes as the call into blocks of their own
        if entry == "forward":
            status, message, values, point_loss, loss = case.forward()
            assert status == 0, message
            for name, block in (("values", values), ("point_loss", point_loss), ("loss", loss)):
                fp.same_as(arena, runs[1], name, block)
            assert values.any() and loss.all()
        else:
            status, message, own = case.backward(priors)
            assert status == 0, message
            for name, block in own.items():
                fp.same_as(arena, runs[1], name, block)


def refusals(case):
    """name -> (which entries, the change, the message behind the prefix); a pointer that is refused is never read."""
    both ={"records": case.states["energy"], "mu": case.states["energy"], "cov": case.states["energy"]}
    neither = {"records": None, "mu": None, "cov": None}
    half = dict(mu=None) if case.form == "moments" else dict(mu=case.states["energy"])
    states = "the states are records, or mu and cov, not both and not neither"
    T = len(case.terms)
    return {
        "a null energy trace": ("both", dict(energy=None), "bad argument"),
        "null rows": ("both", dict(rows=None), "bad argument"),
        "null target points": ("both", dict(points=None), "bad argument"),
        "a null loss": ("forward", dict(loss=None), "bad argument"),
        "null values": ("forward", dict(values=None), "bad argument"),
        "a null loss_bar": ("backward", dict(loss_bar=None), "bad argument"),
        "both state forms": ("both", both, states),
        "neither state form": ("both", neither, states),
        "half a state form": ("both", half, states),
        "a batch of 0": ("both", dict(batch=0), "bad argument"),
        "no points": ("both", dict(n_points=0), "bad argument"),
        "no target points": ("both", dict(n=0), "bad argument"),
        "a dtype of 2": ("both", dict(dtype=2), "the dtype is float32 or float64"),
        "a ddof of 2": ("both", dict(ddof=2), "ddof is 0 or 1"),
        "a ddof of -1": ("both", dict(ddof=-1), "ddof is 0 or 1"),
        "a point outside the trace": ("both", dict(points=[(0, 1), (case.P, 1)], n=2), "the target points lie inside the trace and increase"),
        "a negative point": ("both", dict(points=[(-1, 1), (2, 1)], n=2), "the target points lie inside the trace and increase"),
        "points that do not increase": ("both", dict(points=[(2, 1), (2, 2)], n=2), "the target points lie inside the trace and increase"),
        "a mask of 0": ("both", dict(points=[(0, 1), (2, 0)], n=2), "a property mask has bits 0 .. 22 and is not 0"),
        "a mask with bit 23": ("both", dict(points=[(0, 1), (2, 1 << 23)], n=2), "a property mask has bits 0 .. 22 and is not 0"),
        "a row stride of one row": ("both", dict(stride=2), "the rows' sample stride is 0 or 2 * the number of terms"),
        "a row stride of the terms": ("both", dict(stride=T), "the rows' sample stride is 0 or 2 * the number of terms"),
        "cotangents of the other form": ("backward", "swap", "the cotangents have the form of the states, records or mu and cov"),
        "no energy cotangents for an energy term": ("backward", dict(energy_bar=None),
                                                    "a term that depends on the energy needs the energy's cotangents"),
    }


@DTYPES
@FORMS
def test_every_refusal_carries_its_text_and_the_next_valid_call_returns_the_same_bytes(lx, form, dtype):
    case = Case(lx, form, dtype, (3, 6, [0, 2, 5], 1), False, seed=10, masks=[bits("beta_x"), ALL, bits("sigma_y", "energy")])
    assert len(case.terms) > 2
    priors = case.priors()
    cases = refusals(case)
    rt = case.rt
    status, message, *first = case.forward()
    assert status == 0, message
    status, message, first_after = case.backward(priors)
    assert status == 0, message
    for name, (entries, change, expected) in cases.items():
        if entries in ("both", "forward"):
            out = (rt.empty((case.B, len(case.terms)), np.float64), rt.empty((case.B, case.Q), np.float64), rt.empty((case.B,), np.float64))
            for block in out:
                rt.check(rt.lib.lynx_buf_memset(rt.ctx, p(block), 0, block.nbytes))
            status, message, *made = case.forward(out=out, **dict(change))
            assert (status, message) == (INVALID, PREFIX + expected), name
            assert not any(block.any() for block in made), name  # (refused before anything was launched)
            status, message, *again = case.forward()
            assert status == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(again, first)), (name, message)
        if entries in ("both", "backward"):
            if change == "swap":  # the cotangent buffers of the other state form
                wrong = rt.to_device(np.zeros((case.B, case.P, 49)))
                change = dict(grad_trace=None, mu_bar=wrong, cov_bar=wrong) if form == "records" else dict(grad_trace=wrong, mu_bar=None, cov_bar=None)
            status, message, after = case.backward(priors, **dict(change))
            assert (status, message) == (INVALID, PREFIX + expected), name
            assert all(after[key].tobytes() == priors[key].tobytes() for key in priors), name
            status, message, again = case.backward(priors)
            assert status == 0 and all(again[key].tobytes() == first_after[key].tobytes() for key in priors), (name, message)
    # a NULL energy cotangent is accepted where no term depends on the energy
    plain = Case(lx, form, dtype, (3, 6, [1], 1), True, seed=11, masks=[bits("beta_x", "sigma_p", "mu_s")])
    priors = {name: host for name, host in plain.priors().items() if name != "energy_bar"}
    status, message, after = plain.backward(priors, energy_bar=None)
    assert status == 0, message
    assert any(not np.array_equal(after[name], priors[name]) for name in priors)


# ---------------------------------------------------------------------------------------------
# 9. the public interface against the existing path, mode by mode
# ---------------------------------------------------------------------------------------------

MODES = ("moments", "particles", "trajectories", "survivors", "kicks")
B_PUBLIC = 3


def public_case(lx, mode, dtype):
    """(segment, beam, keywords, the elements whose gradients are compared) of one mode, the same numbers in either dtype."""
    a = lambda *v: np.array(v * (B_PUBLIC if len(v) == 1 else 1), dtype=dtype)  # noqa: E731 (one value: the same for every sample)
    quad = lambda name, k1: lx.Quadrupole(a(0.23), k1=a(*k1), name=name, dtype=dtype)  # noqa: E731
    drift = lambda name, length: lx.Drift(a(*length), name=name, dtype=dtype)  # noqa: E731
    q1, q2 = quad("Q1", (1.37, 1.61, 1.13)), quad("Q2", (-1.43, -1.21, -1.77))
    d1, d2 = drift("D1", (0.53, 0.47, 0.61)), drift("D2", (0.71, 0.67, 0.59))
    energy = a(1.07e8, 0.93e8, 1.21e8)
    if mode == "kicks":
        cavity = lx.Cavity(a(1.0377), voltage=a(1.3e7, 0.9e7, 1.1e7), phase=a(-7.0, 3.0, 11.0), frequency=a(1.3e9), name="CAV", dtype=dtype)
        elements, compared = [d1, cavity, q1, lx.Marker(name="M1"), d2, lx.Marker(name="M2")], [d1, cavity, q1]
    elif mode == "survivors":
        collimator = lx.Aperture(x_max=a(1.1e-4), y_max=a(1.3e-4), is_active=True, name="COL", dtype=dtype)
        elements, compared = [q1, d1, collimator, lx.Marker(name="M1"), q2, d2, lx.Marker(name="M2")], [q1, d1, q2, d2]
    else:
        elements, compared = [q1, d1, lx.Marker(name="M1"), q2, d2, lx.Marker(name="M2")], [q1, d1, q2, d2]
    if mode == "moments":
        full = lambda v: np.full((B_PUBLIC,), v, dtype=dtype)  # noqa: E731
        beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-5), mu_xp=full(-3e-6), sigma_x=full(1.1e-4), sigma_xp=full(1.3e-5), sigma_y=full(0.9e-4),
                                                sigma_yp=full(1.7e-5), sigma_s=full(8e-6), sigma_p=full(1e-3), energy=energy, dtype=dtype)
    else:
        particles = o.gaussian_particles((B_PUBLIC,), 256, seed=12, dtype=np.float64, sigma=[1.1e-4, 1.3e-5, 0.9e-4, 1.7e-5, 8e-6, 1e-3],
                                         mu=[2e-5, -3e-6, 1e-5, 2e-6, 0.0, 1e-4])
        beam = lx.ParticleBeam(particles.astype(dtype), energy, dtype=dtype)
    keywords = {"trajectories": {"trajectories": 3}, "survivors": {"losses": True}, "kicks": {"cavities": True}}.get(mode, {})
    return lx.Segment(elements), beam, keywords, compared


# a Twiss value, a size, a centroid, a cross term and (where the energy changes) a normalized emittance and the energy
PUBLIC_TARGETS = {"M1": {"beta_x": 2.0, "beta_y": 9.0, "mu_x": 0.0}, -1: {"sigma_x": 5e-5, "alpha_y": 0.3, "sigma_xxp": 0.0}}
PUBLIC_WEIGHTS = {"M1": {"beta_x": 0.25, "beta_y": 0.01, "mu_x": 1e9}, -1: {"sigma_x": np.array([3e8, 2e8, 1e8]), "alpha_y": 2.0, "sigma_xxp": 1e18}}
KICK_TARGETS = {**PUBLIC_TARGETS, "M2": {"normalized_emittance_x": 1e-7, "energy": 1.0e8}}
KICK_WEIGHTS = {**PUBLIC_WEIGHTS, "M2": {"normalized_emittance_x": 1e13, "energy": 1e-14}}


def existing_way(lx, vjp, targets, weights):
    """The parent's way to the same loss: the trace read back, 2 w (value - target) formed in numpy and passed as the
    properties' cotangents -> (gradients, the loss (*batch,))."""
    trace = vjp.trace
    shape = (*trace.batch_shape, trace.num_points)
    bars, loss = {}, np.zeros(trace.batch_shape)
    for point, named in targets.items():
        k = trace.index_of(point)
        for name, target in named.items():
            weight = np.asarray(weights.get(point, {}).get(name, 1.0), dtype=np.float64)
            value = np.asarray(getattr(trace, name), dtype=np.float64)[..., k]
            bars.setdefault(name, np.zeros(shape))[..., k] += 2.0 * weight * (value - target)
            loss = loss + weight * (value - target) ** 2
    return vjp(**bars), loss


def gradients_of(g, compared, mode):
    """{label: array} of everything the two ways are compared in."""
    out = {"energy": np.asarray(g.energy, dtype=np.float64)}
    for element in compared:
        for name, value in g[element].items():
            out[f"{element.name}.{name}"] = np.asarray(value, dtype=np.float64)
    if mode in ("moments", "particles", "trajectories"):
        out["mu"], out["cov"] = np.asarray(g.mu, dtype=np.float64), np.asarray(g.cov, dtype=np.float64)
    return out


def both_ways(lx, mode, dtype):
    segment, beam, keywords, compared = public_case(lx, mode, dtype)
    targets, weights = (KICK_TARGETS, KICK_WEIGHTS) if mode == "kicks" else (PUBLIC_TARGETS, PUBLIC_WEIGHTS)
    old, old_loss = existing_way(lx, lx.grad.track_along_vjp(segment, beam, **keywords), targets, weights)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets=lx.grad.MomentTargets(targets, weights), **keywords)
    new = vjp(moment_loss_bar=1.0)
    return gradients_of(old, compared, mode), old_loss, gradients_of(new, compared, mode), vjp


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_against_the_existing_path_fp64(lx, mode):
    old, old_loss, new, vjp = both_ways(lx, mode, np.float64)
    if mode == "survivors":
        assert np.all(vjp.trace.num_survivors[:, -1] < 256) and np.all(vjp.trace.num_survivors[:, -1] > 16)  # the collimator bites
    assert np.all(old["Q1.k1"] != 0) and np.all(old["D1.length"] != 0) and (mode != "kicks" or np.all(old["energy"] != 0))
    for label, ref in old.items():
        assert np.allclose(new[label], ref, rtol=1e-9, atol=1e-12 * np.max(np.abs(ref))), (mode, label, new[label], ref)
    assert np.allclose(vjp.moment_loss, old_loss, rtol=1e-9, atol=1e-12 * np.max(np.abs(old_loss))) and np.all(old_loss > 0)
    # the parts: the terms' values, the points' losses
    terms = vjp._moment_targets.terms
    assert vjp.moment_values.shape == (B_PUBLIC, len(terms)) and [name for _, name in terms[:3]] == ["mu_x", "beta_x", "beta_y"]
    for t, (k, name) in enumerate(terms):
        ref = np.asarray(getattr(vjp.trace, name), dtype=np.float64)[:, k]
        assert np.allclose(vjp.moment_values[:, t], ref, rtol=1e-12, atol=1e-12 * np.max(np.abs(ref))), (name, k)
    parts = sum(vjp.moment_loss_of(k) for k in sorted({k for k, _ in terms}))
    assert np.allclose(parts, vjp.moment_loss, rtol=1e-14)


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_in_float32_is_no_further_from_the_existing_path_than_that_is_from_float64(lx, mode):
    """Per parameter, scaled by max |float64 gradient|: |new float32 - existing float32| <= |existing float32 - existing float64|."""
    reference, loss64, _, _ = both_ways(lx, mode, np.float64)
    old, old_loss, new, vjp = both_ways(lx, mode, np.float32)
    report = []
    for label, ref64 in reference.items():
        scale = np.max(np.abs(ref64))
        if scale == 0:
            assert not np.any(new[label]) and not np.any(old[label])
            continue
        moved, allowed = np.max(np.abs(new[label] - old[label])) / scale, np.max(np.abs(old[label] - ref64)) / scale
        report.append((label, moved, allowed))
    moved, allowed = np.max(np.abs(vjp.moment_loss - old_loss) / np.abs(loss64)), np.max(np.abs(old_loss - loss64) / np.abs(loss64))
    report.append(("moment_loss", moved, allowed))
    for label, moved, allowed in report:
        print(f"{mode} {label}: new against existing float32 {moved:.2e}, existing float32 against float64 {allowed:.2e}")
    for label, moved, allowed in report:
        assert moved <= allowed, (mode, label, moved, allowed)


# ---------------------------------------------------------------------------------------------
# 10. end to end against central differences of the oracle's chain
# ---------------------------------------------------------------------------------------------


def test_the_gradient_of_the_loss_matches_finite_differences_of_the_oracles_chain_fp64(lx):
    """The lattice, the chain and the tolerances of test_parameter_beam_gradients_at_every_point_match_finite_differences_fp64;
    the loss is beta, alpha, sigma, the centroid and the normalized emittance at three of its ten points."""
    rng = np.random.default_rng(23)
    B = 2
    desc = _desc(B, rng)
    elements, specs = make_lattice(desc, np.float64, lx)
    A = rng.normal(size=(B, 6, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-4, 1e-3]
    cov = np.zeros((B, 7, 7))
    cov[:, :6, :6] = A @ np.swapaxes(A, -1, -2)
    mu = np.concatenate([rng.normal(size=(B, 6)) * [1e-3, 1e-4, 1e-3, 1e-4, 1e-4, 1e-3], np.ones((B, 1))], axis=-1)
    energy = np.array([6e6, 8e6])
    vjp0 = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParameterBeam(mu, cov, energy, dtype=np.float64))
    names = {3: ("beta_x", "alpha_y", "mu_xp"), 6: ("sigma_y", "emittance_x", "sigma_yyp"), 9: ("beta_y", "normalized_emittance_y", "alpha_x")}
    # targets and weights from the unperturbed trace: every term adds about 0.01 to the loss
    targets = {k: {name: 0.9 * np.asarray(getattr(vjp0.trace, name), dtype=np.float64)[:, k] for name in named} for k, named in names.items()}
    weights = {k: {name: 1.0 / np.maximum(np.abs(value), 1e-300) ** 2 for name, value in named.items()} for k, named in targets.items()}

    def loss(mu_, cov_, energy_):
        beams = _chain(specs, o.parameter_beam(mu_, cov_, energy_, np.float64))
        total = np.zeros(B)
        for k, named in targets.items():
            states = beams[k]
            values, _ = ml.values_of(np.float64, states["energy"], mu=states["mu"], cov=states["cov"])
            for name, target in named.items():
                total += weights[k][name] * (values[name] - target) ** 2
        return total

    vjp = lx.grad.track_along_vjp(lx.Segment(elements), lx.ParameterBeam(mu, cov, energy, dtype=np.float64),
                                  moment_targets=lx.grad.MomentTargets(targets, weights))
    assert np.allclose(vjp.moment_loss, loss(mu, cov, energy), rtol=1e-9) and np.all(vjp.moment_loss > 0.05)
    g = vjp(moment_loss_bar=1.0)

    def central(apply, x0):
        h = 1e-6 * max(abs(x0), 1e-2)
        apply(x0 + h)
        up = loss(mu, cov, energy)
        apply(x0 - h)
        down = loss(mu, cov, energy)
        apply(x0)
        return (up - down) / (2 * h)

    # (`_check_parameters` takes a floor for |ref| from the cotangents of cov: there are none here, and no floor)
    assert _check_parameters(desc, specs, elements, g, central, np.zeros(1)) > 50
    for bidx in range(B):
        h = 1e-6 * energy[bidx]
        ep, em = energy.copy(), energy.copy()
        ep[bidx] += h
        em[bidx] -= h
        ref = (loss(mu, cov, ep)[bidx] - loss(mu, cov, em)[bidx]) / (2 * h)
        assert abs(g.energy[bidx] - ref) <= 2e-4 * abs(ref) + 1e-12, (bidx, g.energy[bidx], ref)


# ---------------------------------------------------------------------------------------------
# 11. combinations and refusals at construction
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["moments", "particles"])
def test_with_another_cotangent_in_one_call_the_gradient_is_the_sum_of_the_two_calls(lx, mode):
    segment, beam, keywords, compared = public_case(lx, mode, np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets=lx.grad.MomentTargets(PUBLIC_TARGETS, PUBLIC_WEIGHTS), **keywords)
    w = np.zeros((B_PUBLIC, vjp.trace.num_points))
    w[:, 2], w[:, 5] = [0.3, -0.2, 0.5], [1.0, 0.7, -0.4]
    bar = np.array([0.5, -1.5, 2.0])
    one = gradients_of(vjp(moment_loss_bar=bar, beta_x=w, energy_bar=1e-9), compared, mode)
    first, second = gradients_of(vjp(moment_loss_bar=bar), compared, mode), gradients_of(vjp(beta_x=w, energy_bar=1e-9), compared, mode)
    for label in one:
        total = first[label] + second[label]
        assert np.allclose(one[label], total, rtol=1e-12, atol=1e-12 * np.max(np.abs(first[label]) + np.abs(second[label]))), label
    for label in ("Q1.k1", "D1.length", "Q2.k1", "cov"):  # (both parts count)
        assert np.any(first[label] != 0) and np.any(second[label] != 0), label


def test_with_the_image_loss_in_one_call_the_gradient_is_the_sum_of_the_two_calls(lx):
    dtype = np.float64
    a = lambda *v: np.array(v, dtype=dtype)  # noqa: E731
    screen = lx.Screen(resolution=(24, 16), pixel_size=(4e-5, 4e-5), misalignment=a(1e-5, -2e-5), is_active=True, name="SCREEN", dtype=dtype)
    quad, drift = lx.Quadrupole(a(0.23), k1=a(1.37, 1.61), name="Q1", dtype=dtype), lx.Drift(a(0.53, 0.47), name="D1", dtype=dtype)
    segment = lx.Segment([quad, drift, screen, lx.Marker(name="M1")])
    full = lambda v: np.full((2,), v, dtype=dtype)  # noqa: E731
    beam = lx.ParameterBeam.from_parameters(sigma_x=full(1.1e-4), sigma_xp=full(1.3e-5), sigma_y=full(0.9e-4), sigma_yp=full(1.7e-5),
                                            energy=full(1e8), dtype=dtype)
    target = np.asarray(segment.track_along(beam, screens=True).image_at("SCREEN"), dtype=dtype)[0] * 0.8
    vjp = lx.grad.track_along_vjp(segment, beam, image_targets={"SCREEN": target}, moment_targets={"M1": {"beta_x": 3.0, "sigma_y": 1e-4}})
    scale = 1.0 / np.max(target) ** 2
    one = vjp(image_loss_bar=scale, moment_loss_bar=1e-3)
    first, second = vjp(image_loss_bar=scale), vjp(moment_loss_bar=1e-3)
    assert np.all(vjp.image_loss_of("SCREEN") > 0) and np.all(vjp.moment_loss > 0)
    for read in (lambda g: g[quad]["k1"], lambda g: g[drift]["length"], lambda g: g.mu, lambda g: g.cov, lambda g: g[screen]["misalignment"]):
        total = np.asarray(read(first), dtype=np.float64) + np.asarray(read(second), dtype=np.float64)
        assert np.allclose(read(one), total, rtol=1e-12, atol=1e-12 * np.max(np.abs(total))) and np.any(read(first) != 0)
    assert np.any(second[quad]["k1"] != 0) and not np.any(second[screen]["misalignment"])


def test_behind_a_collimator_the_targets_are_the_survivors_values(lx):
    segment, beam, keywords, _ = public_case(lx, "survivors", np.float64)
    vjp = lx.grad.track_along_vjp(segment, beam, moment_targets={"M2": {"sigma_x": 5e-5, "mu_y": 0.0}}, **keywords)
    trace = vjp.trace
    k = trace.index_of("M2")
    assert np.all(trace.num_survivors[:, k] < 256)
    everyone = lx.Segment([el for el in segment.elements if el.name != "COL"]).track_along(beam)
    assert np.all(np.abs(np.asarray(trace.sigma_x)[:, k] / np.asarray(everyone.sigma_x)[:, k - 1] - 1) > 1e-3)  # (the collimated beam is another one)
    assert np.allclose(vjp.moment_values[:, 0], np.asarray(trace.mu_y, dtype=np.float64)[:, k], rtol=1e-12, atol=1e-18)
    assert np.allclose(vjp.moment_values[:, 1], np.asarray(trace.sigma_x, dtype=np.float64)[:, k], rtol=1e-12)


def test_the_refusals_at_construction_carry_the_texts_of_the_cotangents(lx):
    dtype = np.float32
    a = lambda *v: np.array(v, dtype=dtype)  # noqa: E731
    # a collimator nobody of sample 1 passes
    segment = lx.Segment([lx.Drift(a(0.5), name="D1"), lx.Aperture(x_max=a(1e-3, 1e-9), y_max=a(1e-3, 1e-9), is_active=True, name="COL"),
                          lx.Drift(a(0.5), name="D2")])
    particles = o.gaussian_particles((2,), 256, seed=13, dtype=np.float64, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]).astype(dtype)
    beam = lx.ParticleBeam(particles, a(1e8, 1e8))
    with pytest.raises(ValueError) as info:
        lx.grad.track_along_vjp(segment, beam, losses=True, moment_targets={-1: {"sigma_x": 1e-4}})
    vjp = lx.grad.track_along_vjp(segment, beam, losses=True, moment_targets={-1: {"energy": 1e8}, "D1": {"sigma_x": 1e-4}})
    assert np.array_equal(vjp.trace.num_survivors[:, -1] == 0, [False, True]) and np.all(np.isfinite(vjp.moment_loss))
    w = np.zeros((2, 4))
    w[1, 3] = 1.0
    with pytest.raises(ValueError) as of_call:
        vjp(sigma_x=w)
    assert str(info.value) == str(of_call.value) and "sample (1,), point 3, which no particle reaches" in str(info.value)
    # an active cavity in front of a ParticleBeam
    cavity = lx.Cavity(a(1.0377), voltage=a(1.3e7), phase=a(-7.0), frequency=a(1.3e9), name="CAV")
    line = lx.Segment([lx.Drift(a(0.5), name="D1"), cavity, lx.Drift(a(0.5), name="D2")])
    with pytest.raises(NotImplementedError) as info:
        lx.grad.track_along_vjp(line, beam, trajectories=2, moment_targets={-1: {"energy": 1.1e8, "sigma_x": 1e-4}})
    vjp = lx.grad.track_along_vjp(line, beam, trajectories=2, moment_targets={-1: {"energy": 1.1e8}})
    with pytest.raises(NotImplementedError) as of_call:
        vjp(sigma_x=1.0)
    assert str(info.value) == str(of_call.value) and "'CAV'" in str(info.value) and "cavities=True" in str(info.value)
    g = vjp(moment_loss_bar=1.0)  # the energy alone passes the cavity: d loss / d voltage = 2 (E - target) cos(phase)
    at_end = np.asarray(vjp.trace.energy, dtype=np.float64)[:, -1]
    assert np.allclose(g[cavity]["voltage"], np.sum(2 * (at_end - 1.1e8)) * np.cos(np.deg2rad(-7.0)), rtol=1e-5)
    assert np.allclose(vjp.moment_loss, (at_end - 1.1e8) ** 2, rtol=1e-12)


# ---------------------------------------------------------------------------------------------
# 12. the example
# ---------------------------------------------------------------------------------------------


def test_match_twiss_along_lattice_on_device_example_converges(lx):
    """examples/match_twiss_along_lattice_on_device.py in the form and step count of test_match_twiss_along_lattice_example_converges;
    at step 0 its loss is no further from the existing example's than that is from the existing example's loss in float64."""
    examples = pathlib.Path(__file__).resolve().parents[1] / "examples"
    spec = importlib.util.spec_from_file_location("match_twiss_along_lattice_on_device", examples / "match_twiss_along_lattice_on_device.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    segment, beam = example.matching_line(), example.incoming_beam()
    history = example.tune(segment, beam)
    assert len(history) == 150 and history[-1] < 0.05 * history[0], (history[0], history[-1])
    trace = segment.track_along(beam)
    for marker, (beta_x, beta_y) in example.TARGETS.items():
        k = trace.index_of(marker)
        assert abs(float(trace.beta_x[0, k]) / beta_x - 1) < 0.05, (marker, trace.beta_x[0, k], beta_x)
        assert abs(float(trace.beta_y[0, k]) / beta_y - 1) < 0.05, (marker, trace.beta_y[0, k], beta_y)

    def existing_loss(line, incoming):
        trace = line.track_along(incoming)
        residuals = []
        for marker, (beta_x, beta_y) in example.TARGETS.items():
            k = trace.index_of(marker)
            residuals += [float(trace.beta_x[0, k]) / beta_x - 1.0, float(trace.beta_y[0, k]) / beta_y - 1.0]
        return float(np.mean(np.square(residuals)))

    fresh = example.matching_line()
    existing = existing_loss(fresh, beam)
    wide = []
    for el in fresh.elements:  # the same line and beam in float64
        if isinstance(el, lx.Quadrupole):
            wide.append(lx.Quadrupole(np.asarray(el.length, dtype=np.float64), k1=np.asarray(el.k1, dtype=np.float64), name=el.name, dtype=np.float64))
        elif isinstance(el, lx.Drift):
            wide.append(lx.Drift(np.asarray(el.length, dtype=np.float64), name=el.name, dtype=np.float64))
        else:
            wide.append(lx.Marker(name=el.name))
    beam64 = lx.ParticleBeam(np.asarray(beam.particles, dtype=np.float64), np.asarray(beam.energy, dtype=np.float64), dtype=np.float64)
    in_float64 = existing_loss(lx.Segment(wide), beam64)
    print(f"step 0: on the device {history[0]:.9e}, existing {existing:.9e}, existing in float64 {in_float64:.9e}")
    assert abs(history[0] - existing) <= abs(existing - in_float64), (history[0], existing, in_float64)
