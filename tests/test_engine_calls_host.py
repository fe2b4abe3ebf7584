"""
The forward host path of `lynx_amd/engine.py` against the transcript in tests/golden/engine_calls.npz, without a GPU:
for every call of `track`, `track_along` and `transfer_map` every library call with every argument (uploads by dtype,
shape and bytes, allocations by how they were made), what the caller sees of the result, and every refusal's type and
text.  The transcript was made by tests/golden/make_engine_calls.py on the commit before `engine.py` was last
restructured: a forward pass that uploads another byte, allocates in another way or calls another entry point fails here.
"""

import numpy as np
import pytest

from .golden import make_engine_calls as golden
from .golden.make_reverse_calls import PATH as REVERSE_PATH
from .test_reverse_calls_host import differences


@pytest.fixture(scope="module")
def recorded_file():
    return golden.load(golden.PATH)


def test_the_file_holds_these_cases_and_is_small(recorded_file):
    assert sorted(recorded_file[0]) == sorted(golden.CASES)
    assert golden.PATH.stat().st_size <= REVERSE_PATH.stat().st_size


@pytest.mark.parametrize("name", list(golden.CASES))
def test_the_calls_are_the_recorded_ones(recorded_file, name):
    index, arrays = recorded_file
    got_arrays = []
    got = golden.flatten(golden.transcript(name), got_arrays)
    assert any(event["calls"] for event in got["events"]) or name == "refusals"  # (the case reached the library)
    found = differences(index[name], got, arrays, got_arrays)
    assert not found, "\n".join(found[:20])


def test_a_twin_holds_nothing_the_engine_remembers_on_its_original():
    """`broadcast()` of an element that was tracked and traced: the twin has none of the six slots, the original all it had."""
    import lynx_amd as lx
    from lynx_amd import engine

    with pytest.MonkeyPatch.context() as monkeypatch:
        golden.fake_engine_gpu(monkeypatch)
        batch, dtype = (2,), np.float64
        beam = golden.particle_beam(lx, batch, dtype)
        segment = golden.diagnosed(lx, batch, dtype, True, True)
        segment.track_along(beam, losses=True, screens=True)
        segment.AP0.is_active = segment.AP1.is_active = segment.AP2.is_active = segment.SCR0.is_active = segment.SCR1.is_active = False
        segment.track(beam)
        assert set(engine.OWNER_SLOTS) <= set(segment.__dict__)
        held = {name: segment.__dict__[name] for name in engine.OWNER_SLOTS}
        twin = segment._twin()
        assert not set(engine.OWNER_SLOTS) & set(twin.__dict__)
        assert all(segment.__dict__[name] is value for name, value in held.items())
        quad = segment.Q
        quad.track(beam)
        lx.Segment([quad]).track_along(beam)  # (an element is the owner of `track` alone: a trace is remembered on its segment)
        before = dict(quad.__dict__)
        twin = quad.broadcast((3,))
        assert {"_plan", "_lattice_cache"} <= set(before) and not set(engine.OWNER_SLOTS) & set(twin.__dict__)
        assert all(quad.__dict__[name] is before[name] for name in engine.OWNER_SLOTS if name in before)


def test_the_named_slots_are_the_ones_written_on_the_owners():
    """Every `_` attribute an owner gains in the transcript's cases is one of `engine.OWNER_SLOTS`, and each of them is gained."""
    from lynx_amd import engine

    owners = []
    for name in golden.CASES:
        golden.transcript(name, owners)
    gained = {key for owner, before in owners for key in set(owner.__dict__) - before if key.startswith("_")}
    assert gained == set(engine.OWNER_SLOTS), sorted(gained ^ set(engine.OWNER_SLOTS))
