"""
Every call of `lynx_amd.grad` against the transcripts in tests/golden/reverse_calls.npz (`track_vjp` and the five modes of
`track_along_vjp`) and tests/golden/target_calls.npz (`image_targets=`, `moment_targets=`, forward mode), without a GPU: the
keyword arguments of the forward trace, every library call with every argument (uploads by dtype, shape and bytes,
allocations by how they were made), everything `Gradients` and the loss and tangent objects hand out, and every refusal's
type and text.  Each transcript was made by tests/golden/make_reverse_calls.py on the commit before `lynx_amd.grad` was
last restructured: a pass that uploads another byte, allocates in another way or launches another entry point fails here.
"""

import numpy as np
import pytest

from .golden import make_reverse_calls as golden


@pytest.fixture(scope="module")
def recorded_files():
    return {path: golden.load(path) for path in (golden.PATH, golden.TARGET_PATH)}


def differences(want, got, want_arrays, got_arrays, where="", nan_equal=False):
    """Paths at which the two flattened trees differ; below "gradients" a NaN equals a NaN."""
    if isinstance(want, dict) and set(want) == {"array"} and isinstance(got, dict) and set(got) == {"array"}:
        a, b = want_arrays[want["array"]], got_arrays[got["array"]]
        if a.dtype != b.dtype or a.shape != b.shape:
            return [f"{where}: {a.dtype}{a.shape} became {b.dtype}{b.shape}"]
        if a.tobytes() == b.tobytes() or (nan_equal and np.array_equal(a, b, equal_nan=True)):
            return []
        return [f"{where}: {int(np.sum(a != b))} of {a.size} values differ"]
    if isinstance(want, dict) and isinstance(got, dict):
        if list(want) != list(got):
            return [f"{where}: keys {list(want)} became {list(got)}"]
        return [d for key in want for d in differences(want[key], got[key], want_arrays, got_arrays, f"{where}/{key}", nan_equal or key == "gradients")]
    if isinstance(want, list) and isinstance(got, list):
        if len(want) != len(got):
            names = lambda items: [item.get("entry", item.get("label")) if isinstance(item, dict) else item for item in items]  # noqa: E731
            return [f"{where}: {len(want)} items became {len(got)}: {names(want)} became {names(got)}"]
        return [d for k, (a, b) in enumerate(zip(want, got)) for d in differences(a, b, want_arrays, got_arrays, f"{where}[{k}]", nan_equal)]
    return [] if type(want) is type(got) and want == got else [f"{where}: {want!r} became {got!r}"]


def replayed(recorded, name):
    index, arrays = recorded
    got_arrays = []
    got = golden.flatten(golden.transcript(name), got_arrays)
    assert got["calls"] or "refusals" in name  # (the case reached the library)
    return differences(index[name], got, arrays, got_arrays)


def test_the_file_holds_these_cases_and_is_small(recorded_files):
    assert sorted(recorded_files[golden.PATH][0]) == sorted(golden.CASES)
    assert golden.PATH.stat().st_size < 100_000


@pytest.mark.parametrize("name", list(golden.CASES))
def test_the_calls_are_the_recorded_ones(recorded_files, name):
    found = replayed(recorded_files[golden.PATH], name)
    assert not found, "\n".join(found[:20])


def test_the_target_file_holds_these_cases_and_is_small(recorded_files):
    assert sorted(recorded_files[golden.TARGET_PATH][0]) == sorted(golden.TARGET_CASES)
    assert golden.TARGET_PATH.stat().st_size < 100_000


@pytest.mark.parametrize("name", list(golden.TARGET_CASES))
def test_the_target_calls_are_the_recorded_ones(recorded_files, name):
    found = replayed(recorded_files[golden.TARGET_PATH], name)
    assert not found, "\n".join(found[:20])
