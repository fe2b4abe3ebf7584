"""
Particle trajectories inside a beam trace, without a GPU: the C entry point being declared, every refusal of
`track_along(..., trajectories=...)` raised by value before a runtime exists, and `BeamTrace.from_records` carrying the
trajectories (`trajectories`, `trajectory_indices`, `trajectory_lost_in`, `at(k)["trajectories"]`).
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

from .test_trace_host import host_record

ROOT = Path(__file__).resolve().parent.parent
N = 16

f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731


def test_the_entry_point_is_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    name = "lynx_track_particles_along_trajectories"
    assert name in _ffi.SIGNATURES and f"int {name}(" in header
    # lynx_track_particles_along_screens' arguments and four more: n_chosen, d_indices, d_trajectories, d_trajectory_lost_in
    assert _ffi.SIGNATURES[name][1][:20] == _ffi.SIGNATURES["lynx_track_particles_along_screens"][1]
    assert len(_ffi.SIGNATURES[name][1]) == 24
    for argument in ("n_chosen", "d_indices", "d_trajectories", "d_trajectory_lost_in"):
        assert argument in header, argument


@pytest.fixture
def no_gpu(monkeypatch):
    from lynx_amd import device, engine

    def refuse(*args, **kwargs):
        raise AssertionError("track_along touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", refuse)
    monkeypatch.setattr(engine, "get_runtime", refuse)


@pytest.mark.parametrize("selection, named", [
    (True, "True"), (0, "0"), ([], r"\[\]"), ([1.5], "1.5"), (N + 1, str(N + 1)), ([N], str(N)), ([-1], "-1"),
    (np.int64(0), "0"), (np.array([0, 3, N + 4]), str(N + 4)), (np.zeros((2, 2), dtype=np.int64), r"\(2, 2\)"),
])
def test_a_bad_selection_is_a_value_error_that_names_the_value(no_gpu, selection, named):
    import lynx_amd as lx

    beam = lx.ParticleBeam(o.gaussian_particles((1,), N, seed=1), f(1e8))
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Quadrupole(f(0.2), k1=f(2.0))])
    with pytest.raises(ValueError, match=named) as info:
        segment.track_along(beam, trajectories=selection)
    assert "trajectories" in str(info.value)
    with pytest.raises(ValueError, match=named):  # ... through the split lattice too
        segment.track_along(beam, resolution=0.5, trajectories=selection)


def test_a_parameter_beam_is_a_type_error_that_says_what_to_do(no_gpu):
    import lynx_amd as lx

    beam = lx.ParameterBeam.from_parameters()
    segment = lx.Segment([lx.Drift(f(1.0))])
    with pytest.raises(TypeError, match="ParameterBeam") as info:
        segment.track_along(beam, trajectories=3)
    assert "make_linspaced" in str(info.value) and "from_parameters" in str(info.value)


def test_an_active_aperture_stays_refused_without_losses(no_gpu):
    import lynx_amd as lx

    beam = lx.ParticleBeam(o.gaussian_particles((1,), N, seed=1), f(1e8))
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), name="AP1")])
    with pytest.raises(NotImplementedError, match="AP1"):
        segment.track_along(beam, trajectories=3)


def test_the_selection_is_normalised_to_int64_indices():
    import lynx_amd as lx
    from lynx_amd import engine

    beam = lx.ParticleBeam(o.gaussian_particles((1,), N, seed=1), f(1e8))
    for selection, want in [(3, [0, 1, 2]), (N, list(range(N))), ([5, 5, 2], [5, 5, 2]), (np.array([N - 1, 0], dtype=np.uint8), [N - 1, 0]),
                            (np.int32(2), [0, 1]), ((4, 1), [4, 1])]:
        got = engine.chosen_particles(selection, beam)
        assert got.dtype == np.int64 and got.flags.c_contiguous and got.tolist() == want, selection


@pytest.fixture(scope="module")
def records():
    rng = np.random.default_rng(5)
    P = np.ones((2, 9, 7))
    P[..., :6] = rng.normal(0, [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3], (2, 9, 6))
    rec = np.stack([np.stack([host_record(P[b] * (1 + k)) for k in range(3)]) for b in range(2)])
    paths = np.stack([P[:, [7, 0, 7, 3]] * (1 + k) for k in range(3)], axis=1)  # (2, 3, 4, 7)
    return P, rec, np.full((2, 3), 1e8), paths


def test_from_records_carries_the_trajectories(records):
    from lynx_amd.trace import BeamTrace

    P, rec, energy, paths = records
    lost = np.array([[-1, 0, -1, 1], [0, -1, 0, -1]])
    trace = BeamTrace.from_records(rec, energy, [None, 1.0], ["A", "B"], np.float64, apertures=[0, 1], trajectories=paths,
                                   trajectory_indices=[7, 0, 7, 3], trajectory_lost_in=lost)
    assert trace.trajectories.shape == (2, 3, 4, 7) and trace.trajectories.dtype == np.float64
    assert np.array_equal(trace.trajectories, paths)
    assert trace.trajectory_indices.dtype == np.int64 and trace.trajectory_indices.tolist() == [7, 0, 7, 3]
    assert trace.trajectory_lost_in.dtype == np.int32 and np.array_equal(trace.trajectory_lost_in, lost)
    for k in (0, 1, 2, -1, "B"):
        got = trace.at(k)["trajectories"]
        assert got.shape == (2, 4, 7) and np.array_equal(got, paths[:, trace.index_of(k)])
    # the beam's dtype; the indices default to 0 .. K - 1; no losses: no `trajectory_lost_in`
    single = BeamTrace.from_records(rec, energy, [None, 1.0], ["A", "B"], np.float32, trajectories=paths)
    assert single.trajectories.dtype == np.float32 and np.array_equal(single.trajectories, paths.astype(np.float32))
    assert single.trajectory_indices.tolist() == [0, 1, 2, 3] and single.trajectory_lost_in is None
    with pytest.raises(AssertionError):  # one point short
        BeamTrace.from_records(rec, energy, [None, 1.0], ["A", "B"], np.float64, trajectories=paths[:, :2])


def test_a_trace_without_trajectories_has_none(records):
    from lynx_amd.trace import BeamTrace

    P, rec, energy, paths = records
    plain = BeamTrace.from_records(rec, energy, [None, 1.0], ["A", "B"], np.float64)
    moments = BeamTrace.from_moments(np.zeros((2, 3, 7)), np.zeros((2, 3, 7, 7)), energy, [None, 1.0], ["A", "B"], np.float64)
    for trace in (plain, moments):
        assert trace.trajectories is None and trace.trajectory_indices is None and trace.trajectory_lost_in is None
        assert "trajectories" not in trace.at(1)
