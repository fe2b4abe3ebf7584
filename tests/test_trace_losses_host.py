"""
Particle losses inside a beam trace, without a GPU: the plan (`engine.trace_program(leaves, losses=True)` makes active
apertures steps and remembers them, per mode), the read-out of records whose particle count differs from point to point
(`num_survivors`, `transmission`, `lost_in`, the sigmas under both `LYNX_STD_DDOF` values, a point nobody reaches), the
new C entry point being declared, and the default call still refusing an active aperture by name.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .test_trace_host import host_record

ROOT = Path(__file__).resolve().parent.parent

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731


def _lattice(lx):
    first = lx.Aperture(x_max=f(1e-3), y_max=f(2e-3), shape="elliptical", is_active=True, name="AP_FIRST")
    idle = lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=False, name="AP_IDLE")
    last = lx.Aperture(x_max=f(5e-4), y_max=f(5e-4), is_active=True, name="AP_LAST")
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9))
    leaves = [first, lx.Drift(f(1.0)), idle, lx.BPM(is_active=True), cavity, lx.Quadrupole(f(0.2), k1=f(2.0)), last]
    return leaves, first, idle, last


def test_the_plan_makes_active_apertures_steps_and_remembers_them():
    import lynx_amd as lx
    from lynx_amd import _ffi, engine

    leaves, first, idle, last = _lattice(lx)
    program = engine.trace_program(leaves, losses=True)
    assert program.raw and program.leaves == leaves and len(program.steps) == len(leaves)  # every leaf a step of its own
    assert [(step, el.name, elliptical) for step, el, elliptical in program.apertures] == [(0, "AP_FIRST", True), (6, "AP_LAST", False)]
    for step, _, _ in program.apertures:  # an identity step, like the inactive aperture's
        assert program.steps[step] == [_ffi.STEP_RUN, step, step + 1] and program.steps[2] == [_ffi.STEP_RUN, 2, 3]
    assert program.steps[4][0] == _ffi.STEP_CAVITY
    # without the mode nothing is remembered, and an active aperture is refused by name, with the hint
    with pytest.raises(NotImplementedError, match="AP_FIRST.*losses=True"):
        engine.trace_program(leaves)
    first.is_active = last.is_active = False
    assert engine.trace_program(leaves).apertures == [] and engine.trace_program(leaves, losses=True).apertures == []
    # an active screen stays refused in both modes (no hint: the mode does not help)
    screen = lx.Screen(is_active=True, name="SCR1")
    for losses in (False, True):
        with pytest.raises(NotImplementedError, match="SCR1") as info:
            engine.trace_program([lx.Drift(f(1.0)), screen], losses=losses)
        assert "losses=True" not in str(info.value)


def test_the_remembered_plan_is_kept_per_mode():
    import lynx_amd as lx
    from lynx_amd import engine

    leaves, first, idle, last = _lattice(lx)
    first.is_active = last.is_active = False
    owner = lx.Segment(leaves)
    plain = engine._trace_plan(owner, leaves)
    with_losses = engine._trace_plan(owner, leaves, True)
    assert plain is not with_losses
    assert engine._trace_plan(owner, leaves) is plain and engine._trace_plan(owner, leaves, True) is with_losses
    assert engine._trace_plan(owner, leaves, False) is plain
    last.is_active = True  # a structure write: both are planned again, and only one of them can be
    again = engine._trace_plan(owner, leaves, True)
    assert again is not with_losses and [el.name for _, el, _ in again.apertures] == ["AP_LAST"]
    assert engine._trace_plan(owner, leaves, True) is again
    with pytest.raises(NotImplementedError, match="AP_LAST"):
        engine._trace_plan(owner, leaves)
    last.shape = "elliptical"  # the remembered shape follows the element
    assert [e for _, _, e in engine._trace_plan(owner, leaves, True).apertures] == [True]


@pytest.fixture(scope="module")
def clipped():
    """Three points of a batch of two: 9 particles, an aperture (element 0) that keeps 5 / 1 of them, a second one
    (element 1) that keeps 2 / 0.  The records are the host's, over the survivors of each point."""
    rng = np.random.default_rng(5)
    P = np.ones((2, 9, 7))
    P[..., :6] = rng.normal(0, [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], (2, 9, 6))
    keep = [[9, 5, 2], [9, 1, 0]]
    records = np.zeros((2, 3, 36))
    for b in range(2):
        for k in range(3):
            n = keep[b][k]
            if n:
                records[b, k] = host_record(P[b, :n])
            else:  # what write_moment_record's divisions by a count of 0 give
                records[b, k] = np.nan
                records[b, k, 34], records[b, k, 35] = 1.0, 0.0
    energy = np.full((2, 3), 1e8)
    return P, keep, records, energy


def test_counts_that_differ_per_point_give_survivors_transmission_and_losses(clipped):
    from lynx_amd.trace import BeamTrace

    P, keep, records, energy = clipped
    trace = BeamTrace.from_records(records, energy, [None, None], ["AP_A", "AP_B"], np.float64, apertures=[0, 1])
    assert trace.num_particles == 9
    assert trace.num_survivors.dtype == np.int64 and np.array_equal(trace.num_survivors, keep)
    assert np.array_equal(trace.transmission, np.asarray(keep) / 9)
    assert trace.apertures == ["AP_A", "AP_B"]
    assert trace.lost_in.shape == (2, 2) and np.array_equal(trace.lost_in, [[4, 3], [8, 1]])
    assert trace.lost_at is None and trace.outgoing is None
    # only the second element is an aperture; none is
    one = BeamTrace.from_records(records, energy, [None, None], ["D", "AP_B"], np.float64, apertures=[1])
    assert one.apertures == ["AP_B"] and np.array_equal(one.lost_in, [[3], [1]])
    none = BeamTrace.from_records(records[:, :1], energy[:, :1], [], [], np.float64)
    assert none.apertures == [] and none.lost_in.shape == (2, 0) and np.array_equal(none.num_survivors, [[9], [9]])


@pytest.mark.parametrize("ddof", [1, 0])
def test_sigma_uses_each_points_own_count(clipped, ddof, monkeypatch):
    from lynx_amd import config
    from lynx_amd.trace import BeamTrace

    P, keep, records, energy = clipped
    monkeypatch.setattr(config, "std_ddof", ddof)
    records = records.copy()
    records[1, 1, 7], records[1, 1, 8] = 3e-21, -2e-22  # what float32 sums leave of var(x), cov(x, x') of ONE particle
    trace = BeamTrace.from_records(records, energy, [None, None], ["AP_A", "AP_B"], np.float64, apertures=[0, 1])
    for b in range(2):
        for k in range(3):
            n = keep[b][k]
            if n - ddof > 0:
                for c, key in enumerate(("sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s", "sigma_p")):
                    want = P[b, :n, c].std(ddof=ddof)
                    assert np.isclose(getattr(trace, key)[b, k], want, rtol=1e-12, atol=0.0), (key, b, k)
                assert np.isclose(trace.mu_x[b, k], P[b, :n, 0].mean(), rtol=1e-12, atol=1e-300)
    # one survivor: the unbiased sigma is NaN (0 / 0), the biased one 0; its mean is the particle
    assert np.isnan(trace.sigma_x[1, 1]) if ddof == 1 else trace.sigma_x[1, 1] == 0.0
    assert trace.mu_x[1, 1] == P[1, 0, 0] and trace.sigma_xxp[1, 1] == 0.0 and trace.cov[1, 1, 0, 0] == 0.0


def test_a_point_nobody_reaches_is_nan_and_no_exception(clipped):
    from lynx_amd.trace import BeamTrace

    P, keep, records, energy = clipped
    trace = BeamTrace.from_records(records, energy, [None, None], ["AP_A", "AP_B"], np.float32, apertures=[0, 1])
    for key in ("mu_x", "sigma_x", "sigma_p", "sigma_xxp", "beta_x", "emittance_y", "alpha_x"):
        got = getattr(trace, key)
        assert got.shape == (2, 3) and np.isnan(got[1, 2]), key
        assert not np.isnan(got[0]).any(), key  # the other sample is untouched
    assert np.isnan(trace.mu[1, 2]).all() and np.isnan(trace.cov[1, 2]).all() and not np.isnan(trace.cov[0]).any()
    assert trace.num_survivors[1, 2] == 0 and trace.transmission[1, 2] == 0.0
    point = trace.at(-1)
    assert np.isnan(point["sigma_x"][1]) and not np.isnan(point["sigma_x"][0])


def test_the_entry_point_is_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    name = "lynx_track_particles_along_losses"
    assert name in _ffi.SIGNATURES and f"int {name}(" in header
    # lynx_track_particles_along's arguments and five more
    assert _ffi.SIGNATURES[name][1][:9] == _ffi.SIGNATURES["lynx_track_particles_along"][1]
    assert len(_ffi.SIGNATURES[name][1]) == 14


def test_the_default_call_still_refuses_and_names_the_element(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    beam = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Segment([lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), name="AP1")]), lx.Drift(f(1.0))])
    with pytest.raises(NotImplementedError, match="AP1"):
        segment.track_along(beam)
    with pytest.raises(NotImplementedError, match="AP1"):
        segment.track_along(beam, losses=False)
    with pytest.raises(ValueError, match="losses"):
        segment.track_along(beam, losses="everything")
    screened = lx.Segment([lx.Drift(f(1.0)), lx.Screen(is_active=True, name="SCR7")])
    for losses in (True, "particles"):
        with pytest.raises(NotImplementedError, match="SCR7"):
            screened.track_along(beam, losses=losses)
