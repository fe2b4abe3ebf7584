"""
`BeamTrace` without a GPU: the derived quantities of a trace built from host records (`BeamTrace.from_records`) against the
oracle's element-by-element chain, the bookkeeping (`s`, `names`, `at`, the zero-length mask), the refusal of lattices
with an active Screen, and the two C entry points being declared.
"""

from pathlib import Path

import numpy as np
import pytest

from oracle import lynx_oracle as o

ROOT = Path(__file__).resolve().parent.parent

PROPERTIES = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
              "sigma_p", "sigma_xxp", "sigma_yyp", "emittance_x", "emittance_y", "normalized_emittance_x",
              "normalized_emittance_y", "beta_x", "beta_y", "alpha_x", "alpha_y")


def _tri(i, j):
    return 7 + i * 6 - (i * (i - 1)) // 2 + (j - i)


def host_record(particles):
    """(*batch, 36) float64 moment record of (*batch, N, 7) particles, layout of LYNX_MOMENT_STRIDE."""
    P = np.asarray(particles, dtype=np.float64)
    rec = np.zeros((*P.shape[:-2], 36))
    mean = P.mean(axis=-2)
    rec[..., :7] = mean
    d = P[..., :6] - mean[..., None, :6]
    for i in range(6):
        for j in range(i, 6):
            rec[..., _tri(i, j)] = (d[..., i] * d[..., j]).mean(axis=-1)
    rec[..., 34] = 1.0
    rec[..., 35] = P.shape[-2]
    return rec


def _chain(specs, beam, dtype):
    """The oracle's `plot_twiss` loop with every element tracked: the beams at points 0 .. E."""
    beams = [beam]
    for spec in specs:
        beams.append(o.element_track(spec, beams[-1], dtype))
    return beams


@pytest.fixture(scope="module")
def fodo_chain():
    dtype = np.float64
    B = 2
    specs = o.fodo_segment(8, dtype=dtype, batch_shape=(B,), k1_scale=np.array([1.0, 0.8]))
    specs.insert(5, o.Marker())  # a zero-length element: its point repeats the one before it
    particles = o.gaussian_particles((B,), 20_000, seed=11, dtype=dtype, sigma=[1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3])
    beams = _chain(specs, o.particle_beam(particles, np.full(B, 1e8), dtype), dtype)
    lengths = [spec.get("length") for spec in specs]
    names = [f"{spec['kind']}_{k}" for k, spec in enumerate(specs)]
    return specs, beams, lengths, names


@pytest.mark.parametrize("ddof", [1, 0])
def test_every_derived_property_of_a_trace_from_records_equals_the_oracles(fodo_chain, ddof, monkeypatch):
    from lynx_amd import config
    from lynx_amd.trace import BeamTrace

    specs, beams, lengths, names = fodo_chain
    monkeypatch.setattr(config, "std_ddof", ddof)
    records = np.stack([host_record(beam["particles"]) for beam in beams], axis=-2)  # (B, P, 36)
    energy = np.stack([beam["energy"] for beam in beams], axis=-1)
    trace = BeamTrace.from_records(records, energy, lengths, names, np.float64)
    P = len(specs) + 1
    assert trace.num_points == len(trace) == P and trace.num_particles == 20_000 and trace.batch_shape == (2,)
    assert trace.mu.shape == (2, P, 6) and trace.cov.shape == (2, P, 6, 6) and trace.energy.shape == (2, P)
    for k, beam in enumerate(beams):
        ref = o.beam_moments(beam, ddof=ddof)
        for key in PROPERTIES:
            got = getattr(trace, key)
            assert got.shape == (2, P), key
            assert np.allclose(got[:, k], ref[key], rtol=1e-12, atol=0.0), (key, k, got[:, k], ref[key])
        point = trace.at(k)
        assert point["index"] == k and point["name"] == (names[k - 1] if k else None)
        assert np.array_equal(point["beta_x"], trace.beta_x[:, k]) and np.array_equal(point["s"], trace.s[k])
        assert np.array_equal(point["cov"], trace.cov[:, k]) and np.array_equal(point["energy"], energy[:, k])


def test_positions_names_and_the_zero_length_mask(fodo_chain):
    from lynx_amd.trace import BeamTrace

    specs, beams, lengths, names = fodo_chain
    records = np.stack([host_record(beam["particles"]) for beam in beams], axis=-2)
    energy = np.stack([beam["energy"] for beam in beams], axis=-1)
    trace = BeamTrace.from_records(records, energy, lengths, names, np.float64)
    s = np.zeros((len(specs) + 1, 2))
    for k, length in enumerate(lengths):
        s[k + 1] = s[k] + (0.0 if length is None else length)
    assert trace.s.shape == s.shape and np.array_equal(trace.s, s)
    assert trace.names == names
    mask = trace.where_length_changes()
    assert mask.shape == (len(specs) + 1,) and mask.dtype == bool
    assert not mask[6] and mask.sum() == len(specs)  # the marker is element 6 (point 6); everything else has a length
    assert np.array_equal(trace.s[6], trace.s[5])
    # the reference's plot_twiss points: the marker's is left out, the positions stay monotonic
    assert np.all(np.diff(trace.s[mask], axis=0) > 0)
    assert trace.at("marker_5")["index"] == 6 and trace.at(-1)["index"] == len(specs)
    assert trace.index_of("quadrupole_0") == 1
    with pytest.raises(KeyError):
        trace.at("no such element")
    with pytest.raises(IndexError):
        trace.at(len(specs) + 1)


def test_a_parameter_beam_trace_reads_like_a_parameter_beam():
    from lynx_amd.trace import BeamTrace

    dtype = np.float32
    specs = o.ares_like_segment(dtype, (3,))
    beam = o.parameter_beam_from_parameters(dtype=dtype, sigma_x=np.full(3, 1e-4), sigma_xp=np.full(3, 1e-5),
                                            energy=np.full(3, 1e8))
    beams = _chain(specs, beam, dtype)
    trace = BeamTrace.from_moments(np.stack([b["mu"] for b in beams], axis=-2), np.stack([b["cov"] for b in beams], axis=-3),
                                   np.stack([b["energy"] for b in beams], axis=-1), [s.get("length") for s in specs],
                                   [s["kind"] for s in specs], dtype)
    for k, b in enumerate(beams):
        ref = o.beam_moments(b)
        for key in PROPERTIES:
            assert np.allclose(getattr(trace, key)[:, k], ref[key], rtol=1e-6, atol=0.0), (key, k)
    assert trace.mu.shape == (3, len(beams), 6) and trace.cov.shape == (3, len(beams), 6, 6)


def test_a_lattice_with_an_active_screen_is_refused_before_any_gpu_call(monkeypatch):
    import lynx_amd as lx
    from lynx_amd import device, engine

    def no_gpu(*args, **kwargs):
        raise AssertionError("track_along touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", no_gpu)
    monkeypatch.setattr(engine, "get_runtime", no_gpu)
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    segment = lx.Segment([lx.Drift(f(1.0)), lx.Segment([lx.Screen(is_active=True, name="SCR7")]), lx.Drift(f(1.0))])
    beam = lx.ParticleBeam(o.gaussian_particles((1,), 16, seed=1), f(1e8))
    with pytest.raises(NotImplementedError, match="SCR7"):
        segment.track_along(beam)
    with pytest.raises(NotImplementedError, match="AP1"):
        lx.Segment([lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=True, name="AP1")]).track_along(beam)


def test_both_entry_points_are_declared():
    from lynx_amd import _ffi

    header = (ROOT / "include" / "lynx_hip.h").read_text()
    for name in ("lynx_track_particles_along", "lynx_track_moments_along"):
        assert name in _ffi.SIGNATURES
        assert f"int {name}(" in header
