"""
Orbit correction in a linac: a FODO line with two accelerating cavities whose misaligned quadrupoles steer the beam off axis.
`lynx_amd.grad.orbit_response_matrix(..., cavities=True)` takes d(reading of every BPM)/d(angle of every corrector) THROUGH the
cavities -- the response behind a cavity is damped by its map, and the energy behind it sets every later one -- and one step of
pseudo-inverse correction brings the orbit at the BPMs back to zero: the line has no dipole, so the centroid's x and y are
affine in the angles.  Beside it, the same step with the matrix of the same line with its cavities switched off, the best
forward mode had to offer before: it leaves a residual orbit.

    python examples/orbit_response_matrix_linac.py          # needs an MI355X and the built library
"""

import numpy as np

import lynx_amd as lx
import lynx_amd.grad as grad

CELLS = 4
VOLTAGE = 2e7  # per cavity, on a 50 MeV beam


def fodo_linac(dtype=np.float64, seed=3, voltage=VOLTAGE):
    """CELLS x [QF, HCOR, VCOR, drift, BPM, QD, HCOR, VCOR, drift, BPM] with a cavity behind the BPM of the first and of the
    third cell's QF half (`voltage=0`: a drift in its place); every quadrupole misaligned by some 100 um."""
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
            if half == "F" and cell in (0, 2) and voltage:
                elements.append(lx.Cavity(f(1.0377), voltage=f(voltage), phase=f(-5.0), frequency=f(1.3e9), name="ACC" + tag, dtype=dtype))
            elif half == "F" and cell in (0, 2):  # switched off: a drift of its length (the reference's cavity map at 0 V is NaN)
                elements.append(lx.Drift(f(1.0377), name="ACC" + tag, dtype=dtype))
    return lx.Segment(elements)


def incoming_beam(dtype=np.float64):
    one = lambda v: np.array([v], dtype=dtype)  # noqa: E731
    return lx.ParameterBeam.from_parameters(sigma_x=one(1e-4), sigma_xp=one(1e-5), sigma_y=one(1e-4), sigma_yp=one(1e-5),
                                            energy=one(5e7), dtype=dtype)


def orbit(trace, segment, bpms) -> np.ndarray:
    """The readings of `bpms` from a trace, (2 n_bpm,): x first, then y -- the centroid of the beam entering each of them."""
    leaves = list(segment._leaves())
    points = [next(k for k, el in enumerate(leaves) if el is bpm) for bpm in bpms]
    mu = np.asarray(trace.mu, dtype=np.float64)[0]
    return np.concatenate([mu[points, 0], mu[points, 2]])


def rms(v) -> float:
    return float(np.sqrt(np.mean(np.square(v))))


def corrected(segment, beam, response, matrix, before) -> float:
    """The rms orbit of `segment` with the angles `-pinv(matrix) before` on `response.correctors` (put back afterwards)."""
    angles = -np.linalg.pinv(matrix) @ before
    kept = [np.array(corrector.angle) for corrector in response.correctors]
    for corrector, angle in zip(response.correctors, angles):
        corrector.angle = (np.asarray(corrector.angle, dtype=np.float64) + angle).astype(beam.dtype)
    after = orbit(segment.track_along(beam), segment, response.bpms)
    for corrector, angle in zip(response.correctors, kept):
        corrector.angle = angle
    return rms(after)


def correct(dtype=np.float64):
    """-> (the response matrix object through the cavities, rms orbit before, after one step with that matrix, after one step
    with the matrix of the line with its cavities switched off)."""
    segment, beam = fodo_linac(dtype), incoming_beam(dtype)
    response = grad.orbit_response_matrix(segment, beam, cavities=True)
    before = orbit(response.jvp.trace, segment, response.bpms)
    off = grad.orbit_response_matrix(fodo_linac(dtype, voltage=0.0), beam)  # (no active cavity: the plain call)
    through = corrected(segment, beam, response, response.matrix[0], before)
    without = corrected(segment, beam, response, off.matrix[0], before)
    return response, rms(before), through, without


if __name__ == "__main__":
    response, before, through, without = correct()
    print(f"{len(response.bpms)} BPMs, {len(response.correctors)} correctors, 2 cavities of {VOLTAGE:.0e} V on 5e+07 eV: "
          f"response matrix {response.matrix.shape[1:]}")
    print(f"rms orbit at the BPMs {before:.3e} m")
    print(f"  -> {through:.3e} m with one step of the matrix taken through the cavities")
    print(f"  -> {without:.3e} m with one step of the matrix of the line with its cavities switched off")
