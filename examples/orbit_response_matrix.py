"""
Orbit correction from the orbit response matrix: a FODO line whose quadrupoles are misaligned steers the beam off axis;
`lynx_amd.grad.orbit_response_matrix` gives d(reading of every BPM)/d(angle of every corrector) in ONE forward-mode call
(`track_along_jvp`: one sweep per corrector over the states of one trace), the corrector settings come from its
pseudo-inverse, and -- the optics being linear in the angles -- one step brings the orbit at the BPMs back to zero.

    python examples/orbit_response_matrix.py          # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

CELLS = 4


def fodo_line(dtype=np.float64, seed=3):
    """CELLS x [QF, HCOR, VCOR, drift, BPM, QD, HCOR, VCOR, drift, BPM], every quadrupole misaligned by some 100 um."""
    f = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    rng = np.random.default_rng(seed)
    elements = []
    for cell in range(CELLS):
        for half, k1 in (("F", 4.2), ("D", -4.2)):
            tag = f"{cell}{half}"
            elements += [
                lx.Quadrupole(f(0.2), k1=f(k1), misalignment=rng.normal(0, 1e-4, (1, 2)).astype(dtype), name="Q" + tag, dtype=dtype),
                lx.HorizontalCorrector(f(0.05), angle=f(0.0), name="HC" + tag, dtype=dtype),
                lx.VerticalCorrector(f(0.05), angle=f(0.0), name="VC" + tag, dtype=dtype),
                lx.Drift(f(0.4), dtype=dtype), lx.BPM(name="BPM" + tag)]
    return lx.Segment(elements)


def incoming_beam(dtype=np.float64):
    one = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    return lx.ParameterBeam.from_parameters(sigma_x=one(1e-4), sigma_xp=one(1e-5), sigma_y=one(1e-4), sigma_yp=one(1e-5),
                                            energy=one(1e8), dtype=dtype)


def orbit(trace, segment, bpms) -> np.ndarray:
    """The readings of `bpms` from a trace, (2 n_bpm,): x first, then y -- the centroid of the beam entering each of them."""
    leaves = list(segment._leaves())
    points = [next(k for k, el in enumerate(leaves) if el is bpm) for bpm in bpms]
    mu = np.asarray(trace.mu, dtype=np.float64)[0]
    return np.concatenate([mu[points, 0], mu[points, 2]])


def correct(segment, beam):
    """One step of orbit correction; returns (the response matrix object, rms orbit before, rms orbit after)."""
    response = grad.orbit_response_matrix(segment, beam)
    before = orbit(response.jvp.trace, segment, response.bpms)
    angles = -np.linalg.pinv(response.matrix[0]) @ before
    for corrector, angle in zip(response.correctors, angles):
        corrector.angle = (np.asarray(corrector.angle, dtype=np.float64) + angle).astype(beam.dtype)
    after = orbit(segment.track_along(beam), segment, response.bpms)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))  # noqa: E731
    return response, rms(before), rms(after)


if __name__ == "__main__":
    segment, beam = fodo_line(), incoming_beam()
    response, before, after = correct(segment, beam)
    print(f"{len(response.bpms)} BPMs, {len(response.correctors)} correctors: response matrix {response.matrix.shape[1:]}")
    print(f"rms orbit at the BPMs {before:.3e} m -> {after:.3e} m with one step of pseudo-inverse correction")
    for corrector in response.correctors[:4]:
        print(f"  {corrector.name}.angle = {float(np.asarray(corrector.angle)[0]):+.4e} rad")
