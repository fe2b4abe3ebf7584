"""
The checker of test_gpu_entry_footprint.py, checked without a GPU: the arena planner and the comparison functions of
tests/entry_footprint.py on numpy arrays that stand in for the read-back, with one planted fault per way a kernel can write
where it should not or leave unwritten what it should write.  Every fault must turn its check red with a message that names the
array and the byte; the clean stand-in must pass.  And the table of tests/entry_calls.py at the refusals' shape must state the
byte sizes that test's fixture allocated before the table took a shape.
"""

import numpy as np
import pytest

from . import entry_calls as ec
from . import entry_footprint as fp

SHAPES = [ec.Shape(1, 1, 1, 1, 1), ec.Shape(3, 63, 5, 3, 3), ec.Shape(3, 65, 67, 3, 3, "marked"), ec.Shape(2, 257, 5, 3, 1, "cavity"),
          ec.Shape(3, 1025, 5, 3, 3, "marked"), ec.Shape(3, 65, 5, 3, 1, "observer"), ec.Shape(2, 65, 1, 1, 1, "empty"),
          ec.Shape(3, 65, 5, 3, 3, "pairs")]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s.B}x{s.N}-{s.NX}x{s.NY}-{s.CHOSEN}-{s.lattice}")
def test_the_regions_are_disjoint_aligned_and_guarded(shape, dtype):
    for entry in ec.ALL_ENTRIES:
        arrays = ec.entry_arrays(entry, shape, dtype)
        arena = fp.plan_arena(arrays)
        fp.check_plan(arena)
        spans = sorted((r.start, r.stop, r.nbytes) for r in arena.regions.values())
        assert spans[0][0] >= max(8192, spans[0][2]) and arena.nbytes - spans[-1][1] >= max(8192, spans[-1][2])  # nothing against an end
        for (_, stop, size), (start, _, next_size) in zip(spans, spans[1:]):
            assert start - stop >= max(8192, size, next_size) and start % 256 == 0
        assert {r.name: r.nbytes for r in arena.regions.values()} == {a.name: ec.nbytes(a) for a in arrays}


def test_an_aliased_pair_is_one_region_that_the_call_writes():
    arrays = ec.entry_arrays("lynx_track_moments", ec.Shape(3, 63, 5, 3, 3), np.float32)
    arena = fp.plan_arena(arrays, alias={"mu_out": "mu_in", "cov_out": "cov_in"})
    fp.check_plan(arena)
    assert arena.regions["mu_out"].start == arena.regions["mu_in"].start and arena.regions["mu_in"].role == "out"
    assert arena.regions["cov_out"][1:4] == arena.regions["cov_in"][1:4] and arena.regions["e_in"].role == "in"


# ---- planted faults ----------------------------------------------------------------------------------------------------

ARRAYS = [ec.Array("p_in", np.float32, (3, 65, 7), "in"), ec.Array("p_out", np.float32, (3, 65, 7), "out"),
          ec.Array("mom", np.float64, (3, 36), "out"), ec.Array("mu_bar", np.float32, (3, 4, 7), "inout")]


def stand_in(fill):
    """(arena, the block before the call, the block after a correct call) over a prior content of `fill`."""
    arena = fp.plan_arena(ARRAYS)
    rng = np.random.default_rng(3)
    before = np.full(arena.nbytes, fill, dtype=np.uint8)
    for name in ("p_in", "mu_bar"):
        arena.view(before, name)[...] = rng.standard_normal(arena.regions[name].shape)
    after = before.copy()
    arena.view(after, "p_out")[...] = 2 * arena.view(before, "p_in")
    arena.view(after, "mom")[...] = np.arange(108).reshape(3, 36)
    arena.view(after, "mu_bar")[:, 2, [0, 2]] += 1.0
    return arena, before, after


ALLOWED = np.zeros((3, 4, 7), dtype=bool)
ALLOWED[:, 2, [0, 2]] = True


def all_checks(arena, runs):
    for before, after in runs:
        fp.nothing_else_written(arena, before, after)
        fp.inout_changed_only(arena, before, after, "mu_bar", ALLOWED)
    fp.outputs_identical(arena, runs[0][1], runs[1][1])


def test_a_correct_call_passes_every_check():
    arena, b0, a0 = stand_in(0x00)
    _, b1, a1 = stand_in(0xFF)
    all_checks(arena, [(b0, a0), (b1, a1)])


def plant(fault):
    arena, b0, a0 = stand_in(0x00)
    _, b1, a1 = stand_in(0xFF)
    out, src = arena.regions["p_out"], arena.regions["p_in"]
    if fault in ("1 B behind", "7168 B behind", "in front", "input"):
        at = {"1 B behind": out.stop, "7168 B behind": out.stop + 7167, "in front": out.start - 1, "input": src.start + 40}[fault]
        for block in (a0, a1):
            block[at] = 0x5A
    elif fault == "unwritten element":  # element 100 keeps what the block held
        a0[out.start + 400:out.start + 404] = b0[out.start + 400:out.start + 404]
        a1[out.start + 400:out.start + 404] = b1[out.start + 400:out.start + 404]
    elif fault == "prior + result":
        for before, after in ((b0, a0), (b1, a1)):
            prior = arena.view(before, "mom").view(np.uint64).copy()
            arena.view(after, "mom").view(np.uint64)[...] += prior
    elif fault == "inout elsewhere":
        for block in (a0, a1):
            arena.view(block, "mu_bar")[1, 2, 1] += 1.0
    return arena, [(b0, a0), (b1, a1)]


@pytest.mark.parametrize("fault, names", [
    ("1 B behind", ["1 B behind the last byte of p_out", f"byte {3 * 65 * 7 * 4} from its start"]),
    ("7168 B behind", ["7168 B behind the last byte of p_out"]),
    ("in front", ["1 B in front of p_out"]),
    ("input", ["p_in (in): byte 40 of", "element 10"]),
    ("unwritten element", ["p_out:", "byte 40", "element (0, 14, 2)"]),
    ("prior + result", ["mom:", "byte 0", "element (0, 0)"]),
    ("inout elsewhere", ["mu_bar:", "element (1, 2, 1)", f"byte {(1 * 28 + 2 * 7 + 1) * 4}"]),
])
def test_a_planted_fault_turns_the_check_red_and_the_message_names_the_array_and_the_byte(fault, names):
    arena, runs = plant(fault)
    with pytest.raises(AssertionError) as caught:
        all_checks(arena, runs)
    message = str(caught.value)
    for name in names:
        assert name in message, message


def test_the_constants_of_a_moment_record_are_checked():
    records = np.zeros((3, 36))
    records[:, 34], records[:, 35] = 1.0, 65.0
    fp.moment_record_constants(records, counts=[65, 65, 65], whole_triangle=True)
    for slot, value in ((30, 1e-300), (34, 0.5), (35, 64.0)):
        bad = records.copy()
        bad[1, slot] = value
        with pytest.raises(AssertionError):
            fp.moment_record_constants(bad, counts=[65, 65, 65], whole_triangle=True)
    bad = records.copy()
    bad[2, 28:34] = np.frombuffer(b"\xff" * 48, dtype=np.float64)  # what an unwritten slot of a block of ones holds
    with pytest.raises(AssertionError, match="reserved"):
        fp.moment_record_constants(bad)


# ---- the table at the refusals' shape ----------------------------------------------------------------------------------

def test_the_table_at_batch_2_and_64_particles_states_the_sizes_the_refusals_fixture_had():
    """The device arrays of tests/test_gpu_entry_refusals.py as its fixture made them while the table was bound to the
    constants B, N, S, NX, NY, CHOSEN = 2, 64, 3, 5, 3, 2: name -> bytes in float32 (float64: the lattice dtype's arrays double)."""
    B, N, P, E, NX, NY, CHOSEN = 2, 64, 4, 3, 5, 3, 2
    scalars = dict(  # name -> (scalars, bytes per scalar; 0: the lattice dtype)
        e_in=(B, 0), p_in=(B * N * 7, 0), mu_in=(B * 7, 0), cov_in=(B * 49, 0), p_out=(B * N * 7, 0), e_out=(B, 0), mom=(B * 36, 8),
        mu_out=(B * 7, 0), cov_out=(B * 49, 0), mu_tr=(B * P * 7, 0), cov_tr=(B * P * 49, 0), e_tr=(B * P, 0),
        records=(B * P * 36, 8), lost_at=(B * N, 4), set_records=(B * 2 * 36, 8), limits=(2, 0), chosen=(2, 8),
        traj=(B * P * CHOSEN * 7, 0), g_mom=(B * 36, 8), g_records=(B * P * 36, 8), traj_bar=(B * P * CHOSEN * 7, 8),
        mu_bar=(B * 7, 0), cov_bar=(B * 49, 0), mu_bar_tr=(B * P * 7, 0), cov_bar_tr=(B * P * 49, 0), g_params=(B * E * 8, 0),
        g_e=(B, 0), g_p=(B * N * 7, 0), g_mu=(B * 7, 0), g_cov=(B * 49, 0), g_chosen=(B * CHOSEN * 7, 0), steps=(B * 3 * 64, 0),
        xedges=(NX + 1, 0), yedges=(NY + 1, 0), hist=(B * NX * NY, 4), x_max=(1, 0), y_max=(1, 0), mask=(B * N, 1),
        counts=(B, 4), offsets=(B, 8), totals=(B, 8), kept=(N * 7, 0), lost=(N * 7, 0), xs=(NX, 0), ys=(NY, 0),
        image=(B * NX * NY, 0), grid=(NX + NY, 0), misalignment=(2, 0), images=(B * NX * NY, 0), images_bar=(B * NX * NY, 0),
        mu_bar_out=(B * P * 7, 0), cov_bar_out=(B * P * 49, 0), g_mis=(B * 2, 0), fill=(B * N * 7, 0), gauss_rows=(B * 27, 8),
        transform_rows=(B * 24, 0), copy=(B * 36, 8), sets_out=(B * 2 * 36, 8))
    for dtype in (np.float32, np.float64):
        specs = ec.array_specs(ec.REFUSALS_SHAPE, dtype)
        named = set()
        for entry in ec.ENTRIES:
            for a in ec.entry_arrays(entry, ec.REFUSALS_SHAPE, dtype):
                count, size = scalars[a.name]
                assert ec.nbytes(a) == count * (size or np.dtype(dtype).itemsize), (entry, a.name)
                assert (a.dtype, a.shape) == specs[a.name]
                named.add(a.name)
        assert named | {"limits", "chosen"} == set(scalars)  # (those two: read by the fixture's own forward calls only)
        for name, (count, size) in scalars.items():
            assert np.prod(specs[name][1]) * specs[name][0].itemsize == count * (size or np.dtype(dtype).itemsize), name
    assert len(ec.ENTRIES) == 22 and ec.REFUSALS_SHAPE[:5] == (2, 64, 5, 3, 2) and ec.REFUSALS_SHAPE.S == 3
    assert ec.arguments("lynx_track_particles", lambda name: name, ec.REFUSALS_SHAPE)["n"] == 64


def test_every_entry_states_a_role_for_every_array_it_names():
    for entry, (_, valid, outputs) in ec.ALL_ENTRIES.items():
        arrays = ec.entry_arrays(entry, ec.Shape(3, 65, 5, 3, 3, "marked"), np.float64)
        assert {a.role for a in arrays} <= {"in", "out", "inout"} and len({a.name for a in arrays}) == len(arrays)
        assert [a.name for a in arrays if a.role == "inout"] == list(ec.INOUT.get(entry, {}))
        assert set(outputs) <= {a.name for a in arrays if a.role != "in"}
