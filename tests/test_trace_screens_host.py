"""
Screen images inside a beam trace, without a GPU: the plan (`engine.trace_program(leaves, screens=True)` makes active
screens identity steps and remembers them, per (losses, screens) mode), the default call still refusing an active screen by
name before anything touches the GPU, `screens` / `screen_images` / `image_at` of both trace classes built from host
arrays, and the two new C entry points being declared.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

ROOT = Path(__file__).resolve().parent.parent

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731


def _lattice(lx):
    first = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), is_active=True, name="SCR_FIRST")
    idle = lx.Screen(resolution=(20, 12), pixel_size=(1e-4, 1e-4), is_active=False, name="SCR_IDLE")
    last = lx.Screen(resolution=(33, 17), pixel_size=(1e-4, 1e-4), is_active=True, name="SCR_LAST")
    aperture = lx.Aperture(x_max=f(1e-3), y_max=f(2e-3), is_active=True, name="AP")
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9))
    leaves = [first, lx.Drift(f(1.0)), idle, lx.BPM(is_active=True), cavity, aperture, lx.Quadrupole(f(0.2), k1=f(2.0)), last]
    return leaves, first, idle, last, aperture


def test_the_plan_makes_active_screens_identity_steps_and_remembers_them():
    import lynx_amd as lx
    from lynx_amd import _ffi, engine

    leaves, first, idle, last, aperture = _lattice(lx)
    program = engine.trace_program(leaves, losses=True, screens=True)
    assert program.raw and program.leaves == leaves and len(program.steps) == len(leaves)  # every leaf a step of its own
    assert [(step, el.name) for step, el in program.screens] == [(0, "SCR_FIRST"), (7, "SCR_LAST")]
    assert [(step, el.name) for step, el, _ in program.apertures] == [(5, "AP")]
    for step, _ in program.screens:  # an identity step, exactly like the inactive screen's
        assert program.steps[step] == [_ffi.STEP_RUN, step, step + 1] and program.steps[2] == [_ffi.STEP_RUN, 2, 3]
    assert program.steps[4][0] == _ffi.STEP_CAVITY
    # the two modes are independent: screens without losses still refuses the aperture, losses without screens the screen
    with pytest.raises(NotImplementedError, match="AP.*losses=True"):
        engine.trace_program(leaves, screens=True)
    with pytest.raises(NotImplementedError, match="SCR_FIRST") as info:
        engine.trace_program(leaves, losses=True)
    assert "losses=True" not in str(info.value)
    aperture.is_active = False
    assert [el.name for _, el in engine.trace_program(leaves, screens=True).screens] == ["SCR_FIRST", "SCR_LAST"]
    # nothing active: nothing is remembered, in any mode
    first.is_active = last.is_active = False
    for losses in (False, True):
        for screens in (False, True):
            assert engine.trace_program(leaves, losses, screens).screens == []


def test_the_remembered_plan_is_kept_per_mode():
    import lynx_amd as lx
    from lynx_amd import engine

    leaves, first, idle, last, aperture = _lattice(lx)
    first.is_active = last.is_active = aperture.is_active = False
    owner = lx.Segment(leaves)
    modes = [(False, False), (True, False), (False, True), (True, True)]
    plans = [engine._trace_plan(owner, leaves, *mode) for mode in modes]
    assert len({id(p) for p in plans}) == 4
    for mode, plan in zip(modes, plans):
        assert engine._trace_plan(owner, leaves, *mode) is plan
    assert engine._trace_plan(owner, leaves) is plans[0] and engine._trace_plan(owner, leaves, True) is plans[1]
    assert engine._trace_plan(owner, leaves, False, screens=True) is plans[2]
    last.is_active = True  # a structure write: every mode is planned again, and only two of them can be
    again = engine._trace_plan(owner, leaves, False, True)
    assert again is not plans[2] and [el.name for _, el in again.screens] == ["SCR_LAST"]
    assert engine._trace_plan(owner, leaves, False, True) is again
    assert [el.name for _, el in engine._trace_plan(owner, leaves, True, True).screens] == ["SCR_LAST"]
    for losses in (False, True):
        with pytest.raises(NotImplementedError, match="SCR_LAST"):
            engine._trace_plan(owner, leaves, losses)


def test_the_default_call_still_refuses_and_names_the_screen(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine, grad

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    particles = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    parameters = lx.ParameterBeam.from_parameters(sigma_x=f(1e-4), energy=f(1e8))
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Segment([lx.Screen(is_active=True, name="SCR7")]), lx.Drift(f(1.0))])
    for beam in (particles, parameters):
        for kw in ({}, {"screens": False}, {"losses": True}, {"losses": "particles", "screens": False}, {"resolution": 0.5}):
            with pytest.raises(NotImplementedError, match="SCR7") as info:
                segment.track_along(beam, **kw)
            assert "losses=True" not in str(info.value)
    # the gradient plans without screens and keeps refusing
    with pytest.raises(NotImplementedError, match="SCR7"):
        grad.track_along_vjp(segment, parameters)


def _records(batch, points, n=9):
    records = np.zeros((*batch, points, 36))
    records[..., 34], records[..., 35] = 1.0, n
    return records


def test_a_particle_trace_holds_its_screens_and_finds_their_images():
    from lynx_amd.trace import BeamTrace

    batch, names = (2,), ["D1", "SCR_A", "Q", "SCR_B"]
    image_a = np.arange(2 * 12 * 20, dtype=np.float32).reshape(2, 12, 20)
    image_b = np.arange(2 * 17 * 33, dtype=np.float32).reshape(2, 17, 33)
    trace = BeamTrace.from_records(_records(batch, 5), np.full((2, 5), 1e8), [None] * 4, names, np.float32,
                                   screens=[1, 3], screen_images=[image_a, image_b])
    assert trace.screens == [1, 3] and len(trace.screen_images) == 2
    assert trace.image_at("SCR_A") is image_a and trace.image_at("SCR_B") is image_b
    # a screen sees the beam ENTERING it: element k observes point k; an int is a point, negative from the end
    assert trace.image_at(1) is image_a and trace.image_at(3) is image_b and trace.image_at(-2) is image_b
    for elsewhere in ("D1", "Q", 0, 2, 4, -1, "NOBODY"):
        with pytest.raises(KeyError):
            trace.image_at(elsewhere)
    with pytest.raises(IndexError):
        trace.image_at(5)
    # together with apertures; and a trace without screens has none
    both = BeamTrace.from_records(_records(batch, 5), np.full((2, 5), 1e8), [None] * 4, names, np.float32, apertures=[0],
                                  screens=[3], screen_images=[image_b])
    assert both.apertures == ["D1"] and both.screens == [3] and both.image_at("SCR_B") is image_b
    none = BeamTrace.from_records(_records(batch, 5), np.full((2, 5), 1e8), [None] * 4, names, np.float32)
    assert none.screens == [] and none.screen_images == []
    with pytest.raises(KeyError):
        none.image_at("SCR_A")


def test_a_parameter_trace_holds_its_screens_too():
    from lynx_amd.trace import BeamTrace

    mu = np.zeros((3, 3, 7))
    mu[..., 6] = 1
    cov = np.broadcast_to(np.eye(7), (3, 3, 7, 7)).copy()
    image = np.ones((3, 20, 12))
    trace = BeamTrace.from_moments(mu, cov, np.full((3, 3), 1e8), [None, None], ["SCR", "D"], np.float64,
                                   screens=[0], screen_images=[image])
    assert trace.screens == [0] and trace.image_at("SCR") is image and trace.image_at(0) is image
    with pytest.raises(KeyError):
        trace.image_at("D")
    with pytest.raises(KeyError):
        trace.image_at(1)
    assert BeamTrace.from_moments(mu, cov, np.full((3, 3), 1e8), [None, None], ["SCR", "D"], np.float64).screens == []


def test_both_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for name in ("lynx_track_particles_along_screens", "lynx_gaussian_images_along"):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header
    # the arguments of the trace with losses, and six more for the screens
    with_screens = _ffi.SIGNATURES["lynx_track_particles_along_screens"][1]
    assert with_screens[:14] == _ffi.SIGNATURES["lynx_track_particles_along_losses"][1] and len(with_screens) == 20
    assert len(_ffi.SIGNATURES["lynx_gaussian_images_along"][1]) == 12
    # the existing read-out keeps its signature
    assert len(_ffi.SIGNATURES["lynx_gaussian_image"][1]) == 10 and len(_ffi.SIGNATURES["lynx_histogram2d"][1]) == 10
