"""
The inputs of tests/test_gpu_trace_first_particle.py, without a GPU: for every case the beam and the lattice are built
and `expectation` -- the oracle alone -- must give what the GPU tests assume before they read a result: the edge rule,
the `lost_at` of the head, at least two survivors at every point of every sample, finite survivors.  A seed that stops
working fails here.
"""

import numpy as np
import pytest

from .test_gpu_trace_first_particle import CASES, SMALL, SMALL_IDS, alive_at, head_case, input_conditions, pattern_points
from .test_gpu_trace_losses import expectation


@pytest.mark.parametrize("kind,n,h", CASES, ids=[f"{kind}-n{n}-h{h}" for kind, n, h in CASES])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_inputs_of_every_head_case(dtype, kind, n, h):
    desc, P, energy = head_case(dtype, kind, n, h)
    expected = expectation(desc, P, energy, dtype)
    input_conditions(desc, P, kind, h, dtype, expected)
    # the head is alive exactly where the GPU test compares patterns alone, if it is not finite
    for k in pattern_points(kind):
        assert alive_at(desc, expected[2], expected[5], k)[..., :h].all()
    if kind == "overflow" and dtype == np.float32:  # float32 does lose it behind the aperture that removed it
        assert not np.isfinite(expected[0][-1]["particles"][..., :h, 0]).any()
        assert not alive_at(desc, expected[2], expected[5], 2)[..., :h].any()


@pytest.mark.parametrize("kind,n,h", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_inputs_of_the_shared_beam_and_of_the_gradients(dtype, kind, n, h):
    # the shared beam: per-sample limits of the first aperture
    desc, P, energy = head_case(dtype, kind, n, h)
    P = np.ascontiguousarray(np.broadcast_to(P[:1], P.shape))
    first = desc[0][1]
    x_max, y_max = (np.array([float(np.ravel(first[key])[0]), 1.0, 1.0], dtype=dtype) for key in ("x_max", "y_max"))
    desc[0] = ("aperture", dict(first, x_max=x_max, y_max=y_max))
    expected = expectation(desc, P, energy, dtype)
    if kind == "halo-1e3":
        assert np.all(expected[2][0, :h] == 0) and np.all(expected[2][1:, :h] >= 1)
        input_conditions(desc, P, kind, h, dtype, expected, head_lost_at=(0, 1, 2))
    else:
        input_conditions(desc, P, kind, h, dtype, expected)
    # the gradients: the cavity a drift, and the beam without its head
    desc, P, energy = head_case(dtype, kind, n, h)
    cavity = next(k for k, (what, _) in enumerate(desc) if what == "cavity")
    desc[cavity] = ("drift", dict(length=desc[cavity][1]["length"]))
    expected = expectation(desc, P, energy, dtype)
    input_conditions(desc, P, kind, h, dtype, expected)
    rest = np.ascontiguousarray(P[:, h:])
    expected_rest = expectation(desc, rest, energy, dtype)
    input_conditions(desc, rest, "core", 0, dtype, expected_rest)
    assert np.array_equal(expected[2][:, h:], expected_rest[2])
