"""
The arena of test_gpu_entry_footprint.py and what is asserted of it, on plain numpy arrays (test_entry_footprint_host.py runs
all of this without a GPU): every array of one call at an interior offset of ONE block, each at a multiple of 256 B (the only
alignment the allocator hands out) and with a guard of at least max(8 KiB, its own size) on both sides -- a stray float32 wave
tile is 64 x 16 x 7 = 7168 B --, the last guard inside the block.  A store that misses its array lands in memory the test owns
and reads back.

The checks compare bytes, never values:
  nothing_else_written   outside the extents of the `out` / `inout` arrays the arena after the call is the arena before it
  outputs_identical      the `out` extents of two runs over different prior contents (0x00, 0xFF) are equal: every byte was
                         written, and none depends on what was there
  inout_changed_only     an `inout` array differs from its prior content at no entry but the ones the header names
A failure names the array and the byte offset.
"""

import math
from collections import namedtuple

import numpy as np

ALIGN = 256
MIN_GUARD = 8 << 10

Region = namedtuple("Region", "name start nbytes role dtype shape")
Region.stop = property(lambda self: self.start + self.nbytes)


class Arena(namedtuple("Arena", "regions nbytes")):
    """name -> Region, and the size of the block."""

    __slots__ = ()

    def extents(self, roles, partial=None):
        """[(start, stop, name)] of the regions with one of `roles`, sorted; `partial`: name -> the bytes of it the call
        is to write (lynx_aperture_compact's kept / lost rows), the rest of the region counts as outside."""
        spans = {(r.start, r.start + (partial or {}).get(r.name, r.nbytes), r.name) for r in self.regions.values() if r.role in roles}
        return sorted(spans)

    def view(self, block, name):
        """The array `name` out of the read-back `block` (uint8)."""
        r = self.regions[name]
        return block[r.start:r.stop].view(r.dtype).reshape(r.shape)


def guard_of(nbytes):
    return max(MIN_GUARD, nbytes)


def plan_arena(arrays, alias=None):
    """
    `arrays`: [(name, dtype, shape, role)].  `alias`: {name: the array whose bytes it shares} -- the aliased pair is one
    region of the stronger role (a call that may run in place: in = out).
    """
    alias = alias or {}
    regions, cursor, last_guard = {}, 0, 0
    for a in arrays:
        if a.name in alias:
            continue
        size = math.prod(a.shape) * np.dtype(a.dtype).itemsize
        guard = guard_of(size)
        start = -(-(cursor + max(guard, last_guard)) // ALIGN) * ALIGN
        regions[a.name] = Region(a.name, start, size, a.role, np.dtype(a.dtype), tuple(a.shape))
        cursor, last_guard = start + size, guard
    for a in arrays:
        if a.name in alias:
            base = regions[alias[a.name]]
            size = math.prod(a.shape) * np.dtype(a.dtype).itemsize
            assert size == base.nbytes and np.dtype(a.dtype) == base.dtype, (a.name, alias[a.name])
            role = "out" if "out" in (a.role, base.role) else base.role
            regions[alias[a.name]] = base._replace(role=role)
            regions[a.name] = base._replace(name=a.name, role=role)
    return Arena(regions, -(-(cursor + last_guard) // ALIGN) * ALIGN)


def check_plan(arena):
    """The regions are disjoint (aliases apart), 256-aligned and guarded as stated; nothing lies against the block's end."""
    spans = sorted({(r.start, r.stop) for r in arena.regions.values()})
    for start, stop in spans:
        assert start % ALIGN == 0, start
    edges = [(0, 0)] + spans + [(arena.nbytes, arena.nbytes)]
    for (_, before_stop), (start, stop), (after_start, _) in zip(edges, edges[1:], edges[2:]):
        need = guard_of(stop - start)
        assert start - before_stop >= need and after_start - stop >= need, (start, stop, need)


def _where(arena, offset):
    """A byte of the arena in words: inside which array, or how far behind / in front of the nearest one."""
    for r in arena.regions.values():
        if r.start <= offset < r.stop:
            k = offset - r.start
            return f"{r.name} ({r.role}): byte {k} of {r.nbytes} (element {k // r.dtype.itemsize})"
    behind = [(offset - r.stop, r) for r in arena.regions.values() if r.stop <= offset]
    front = [(r.start - offset, r) for r in arena.regions.values() if r.start > offset]
    parts = []
    if behind:
        d, r = min(behind, key=lambda x: x[0])
        parts.append(f"{d + 1} B behind the last byte of {r.name} (byte {r.nbytes + d} from its start)")
    if front:
        d, r = min(front, key=lambda x: x[0])
        parts.append(f"{d} B in front of {r.name}")
    return "guard: " + ", ".join(parts)


def nothing_else_written(arena, before, after, partial=None):
    """Outside the `out` / `inout` extents every byte of `after` is that of `before`: guards, inputs, the other arrays."""
    assert before.shape == after.shape == (arena.nbytes,)
    cursor = 0
    for start, stop, _ in arena.extents(("out", "inout"), partial) + [(arena.nbytes, arena.nbytes, None)]:
        if cursor < start and not np.array_equal(before[cursor:start], after[cursor:start]):  # (the detail only when it is needed)
            bad = cursor + np.flatnonzero(before[cursor:start] != after[cursor:start])
            raise AssertionError(f"{bad.size} byte(s) written outside the call's outputs; the first: arena byte {bad[0]}, "
                                 f"{_where(arena, int(bad[0]))}: {before[bad[0]]:#04x} -> {after[bad[0]]:#04x}")
        cursor = max(cursor, stop)


def outputs_identical(arena, first, second, partial=None):
    """The `out` extents of two runs are equal byte for byte."""
    for start, stop, name in arena.extents(("out",), partial):
        a, b = first[start:stop], second[start:stop]
        if np.array_equal(a, b):
            continue
        r, bad = arena.regions[name], np.flatnonzero(a != b)
        k = int(bad[0])
        elements = np.unique(bad // r.dtype.itemsize)
        index = np.unravel_index(int(elements[0]), r.shape)
        raise AssertionError(f"{name}: {elements.size} element(s) depend on what the block held before the call (unwritten, or "
                             f"added to); the first: byte {k}, element {tuple(int(i) for i in index)}: {a[k]:#04x} over zeros, "
                             f"{b[k]:#04x} over ones")


def inout_changed_only(arena, before, after, name, allowed):
    """`allowed`: boolean array of the region's shape, True at the entries the header says the call adds to."""
    r = arena.regions[name]
    changed = (before[r.start:r.stop] != after[r.start:r.stop]).reshape(-1, r.dtype.itemsize).any(axis=1).reshape(r.shape)
    bad = np.argwhere(changed & ~np.asarray(allowed, dtype=bool))
    assert bad.size == 0, (f"{name}: changed at {len(bad)} entr(ies) the header does not name; the first: element "
                           f"{tuple(int(i) for i in bad[0])}, byte {int(np.ravel_multi_index(tuple(bad[0]), r.shape)) * r.dtype.itemsize}")


def same_as(arena, block, name, expected, nbytes=None):
    """The array `name` of the arena holds the bytes of `expected` (the same call into blocks of its own)."""
    r = arena.regions[name]
    have = block[r.start:r.start + (r.nbytes if nbytes is None else nbytes)]
    want = np.ascontiguousarray(expected).view(np.uint8).reshape(-1)[: have.size]
    if np.array_equal(have, want):
        return
    bad = np.flatnonzero(have != want)
    raise AssertionError(f"{name}: differs from the call into separate blocks at {bad.size} byte(s); the first: byte {int(bad[0])}")


def moment_record_constants(records, counts=None, whole_triangle=None):
    """include/lynx_hip.h, LYNX_MOMENT_STRIDE: "[28..33] reserved (0), [34] 1 if the whole triangle was accumulated, 0 if only
    the property set was ..., [35] number of particles" (a trace with losses: the particles alive at that point)."""
    records = np.asarray(records).reshape(-1, 36)
    assert not records[:, 28:34].view(np.uint64).any(), f"record {int(np.argwhere(records[:, 28:34].view(np.uint64))[0][0])}: reserved slots 28..33 are not 0"
    flags = records[:, 34]
    assert np.all((flags == 0) | (flags == 1)), f"slot 34 holds {flags[(flags != 0) & (flags != 1)][:1]}"
    if whole_triangle is not None:
        assert np.all(flags == (1.0 if whole_triangle else 0.0)), flags
    if counts is not None:
        assert np.array_equal(records[:, 35], np.asarray(counts, dtype=np.float64).reshape(-1)), (records[:, 35], counts)
