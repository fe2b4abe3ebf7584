"""
What the host tests of the reverse and forward-mode passes (the package `lynx_amd/grad/`) share: a runtime, a library and
device arrays that exist on the host alone, and the two fixtures built on them.  The library records every call in full -- the entry point's name
and each argument by value --, an allocated output reads back as seeded random numbers, and the forward passes
(`engine.track_along`, `engine.run_program_particles`, `engine.run_program_parameters`) are fabricated on the host: what
the package does between its arguments and the C boundary is then a pure function, which tests/test_reverse_calls_host.py
holds to a transcript.

`fake_engine_gpu` leaves the forward passes as they are and replaces the runtime alone: the library then also plays the
entry points of `lynx_amd/engine.py` that hand something back (a lattice handle, the blocks of `lynx_track_particles_new`,
a read-back), so that tests/test_engine_calls_host.py holds the forward host path to a transcript in the same way.
"""

import ctypes as C

import numpy as np
import pytest

N = 16  # particles of a fabricated particle trace


class FakeArray:
    """
    What the calls need of a device array.  `how`: `empty`, `empty_result`, `to_device`, `to_device_result`, or `forward:
    <name>` for what a forward pass left on the device.  An upload keeps its host array; anything else reads back as
    multiples of 1/4 drawn from a generator seeded by the allocation's ordinal in its runtime.
    """

    fill = None  # what an array the library wrote reads back as, where seeded random numbers would not do

    def __init__(self, rt, how, shape, dtype, host=None):
        self.how, self.shape, self.dtype, self.host = how, tuple(int(n) for n in shape), np.dtype(dtype), host
        self.ordinal = len(rt.allocations)
        self.ptr = 4096 * (self.ordinal + 1)
        rt.allocations.append(self)

    def numpy(self):
        if self.host is not None:
            return self.host.copy()
        if self.fill is not None:
            return np.ascontiguousarray(self.fill, dtype=self.dtype).reshape(self.shape)
        return (np.random.default_rng(self.ordinal).integers(-8, 9, size=self.shape) / 4.0).astype(self.dtype)

    def __array__(self, dtype=None, copy=None):
        return self.numpy() if dtype is None else self.numpy().astype(dtype)

    def tag(self):
        tag = {"how": self.how, "shape": list(self.shape), "dtype": self.dtype.str}
        if self.host is not None:
            tag["host"] = self.host
        return tag


class FakeLibrary:
    """`calls`: the names of the entry points in the order they were asked for; `records`: (name, [argument, ...])."""

    def __init__(self, rt):
        self._rt, self.calls, self.records = rt, [], []

    def _argument(self, value):
        if value is None or isinstance(value, (bool, int, np.integer)):
            return None if value is None else int(value)
        if isinstance(value, C.c_void_p):
            if value.value is None:
                return None
            return self._rt.allocations[value.value // 4096 - 1].tag()
        if isinstance(value, C.Array):
            return {"ctypes": [int(v) for v in value]}
        if isinstance(value, dict):  # (what an entry point played below has already put by value)
            return value
        raise AssertionError(f"an argument of type {type(value)} crossed the C boundary")

    def __getattr__(self, name):
        def entry(*args):
            if name in self.UNRECORDED:
                return 0
            self.calls.append(name)
            played = getattr(type(self), "_play_" + name.removeprefix("lynx_"), None)
            self.records.append((name, [self._argument(a) for a in (args if played is None else played(self, *args))]))
            return 0
        return entry

    # ---- the entry points of the forward host path that hand something back: each returns the arguments to record ----

    UNRECORDED = ("lynx_lattice_destroy",)  # (a finaliser's call: when it comes is the garbage collector's matter)

    def _allocation(self, pointer):
        return self._rt.allocations[(pointer.value if isinstance(pointer, C.c_void_p) else pointer) // 4096 - 1]

    @staticmethod
    def _host_bytes(address, count, dtype):
        """`count` scalars the host holds at `address`, as the upload they are."""
        dtype = np.dtype(dtype)
        address = C.cast(address, C.c_void_p).value if isinstance(address, C._Pointer) else address
        return {"host": np.frombuffer(C.string_at(address, count * dtype.itemsize), dtype=dtype).copy()}

    @staticmethod
    def _structs(array, count):
        return {"structs": [[int(getattr(item, name)) for name, _ in item._fields_] for item in array[:count]]}

    def _play_lattice_create(self, ctx, code, B, E, elems, S, steps, pool, pool_size, handle):
        from lynx_amd import _ffi

        dtype = np.float32 if code == _ffi.F32 else np.float64
        lattice = FakeArray(self._rt, "lattice", (B,), dtype)
        lattice.S, lattice.step_flags = S, [int(step.flags) for step in steps[:S]]
        handle._obj.value = lattice.ptr
        return (ctx, code, B, E, self._structs(elems, E), S, self._structs(steps, S), self._host_bytes(pool, pool_size, dtype), pool_size)

    def _play_lattice_update_params(self, handle, offset, size, block):
        return handle, offset, size, self._host_bytes(block, size, self._allocation(handle).dtype)

    def _play_lattice_set_flags(self, handle, elem_flags, step_flags):
        lattice = self._allocation(handle)
        lattice.step_flags = [int(f) for f in step_flags[:lattice.S]]
        return handle, elem_flags, step_flags

    def _play_track_particles_new(self, ctx, handle, n, e_in, p_in, flags, with_energy, blocks):
        from lynx_amd import _ffi

        rt, lattice = self._rt, self._allocation(handle)
        B, dtype = lattice.shape[0], lattice.dtype
        observers = sum(1 for f in lattice.step_flags if f & _ffi.STEP_FLAG_OBSERVE)
        made = [FakeArray(rt, "library: particles", (B, n, 7), dtype),
                FakeArray(rt, "library: energy", (B,), dtype) if with_energy else None,
                FakeArray(rt, "library: moments", (B, _ffi.MOMENT_STRIDE), np.float64) if flags & (_ffi.TRACK_MOMENTS | _ffi.TRACK_COVARIANCE) else None,
                FakeArray(rt, "library: readings", (B, observers, 2), np.float64) if observers else None]
        if made[1] is not None:
            made[1].fill = fabricated_energy((B,), made[1].ordinal)
        if made[2] is not None:
            made[2].fill = fabricated_records((B,), 1, 3, count=n)
        for k, block in enumerate(made):
            blocks[k] = None if block is None else block.ptr
        return (ctx, handle, n, C.c_void_p(e_in), C.c_void_p(p_in), flags, with_energy,
                {"blocks": [None if block is None else block.tag() for block in made]})

    def _play_buf_d2h(self, ctx, host, pointer, nbytes):
        block = self._allocation(pointer)
        data = block.numpy().tobytes()
        assert len(data) == nbytes, (block.tag(), nbytes)
        C.memmove(host, data, nbytes)
        return ctx, {"read back": block.tag()}, nbytes

    def _play_particle_trace(self, *args):
        """e_trace and the moment records of the four `lynx_track_particles_along*`: plausible values, as `BeamTrace` wants them."""
        n, e_trace, records = args[2], self._allocation(args[6]), self._allocation(args[7])
        B, P = records.shape[0], records.shape[1]
        e_trace.fill = fabricated_energy((B, P), e_trace.ordinal)
        records.fill = fabricated_records((B,), P, 1, nobody=self._rt.nobody if len(args) > 9 and args[9] > 0 else (), count=n)
        return args

    _play_track_particles_along = _play_track_particles_along_losses = _play_particle_trace
    _play_track_particles_along_screens = _play_track_particles_along_trajectories = _play_particle_trace

    def _play_track_moments_along(self, *args):
        mu, cov, e_trace = (self._allocation(a) for a in args[5:8])
        B, P = mu.shape[0], mu.shape[1]
        mu.fill, cov.fill = fabricated_moments((B,), (P,), mu.dtype, 2)
        e_trace.fill = fabricated_energy((B, P), e_trace.ordinal)
        return args

    # ---- the forward-mode sweeps: the directions (CSR) and the energy seeds are host arrays the call reads in place ----

    def _directions(self, start, leaf, row, weight, n_directions, n_entries):
        return (self._host_bytes(start, n_directions + 1, np.int32), self._host_bytes(leaf, n_entries, np.int32),
                self._host_bytes(row, n_entries, np.int32), self._host_bytes(weight, n_entries, np.float64), n_directions, n_entries)

    def _play_track_moments_along_forward(self, *args):
        return (*args[:5], *self._directions(*args[5:11]), *args[11:])

    _play_track_particles_along_forward = _play_track_moments_along_forward

    def _play_track_moments_along_forward_cavities(self, *args):
        return (*args[:5], *self._directions(*args[5:11]), *args[11:13], self._host_bytes(args[13], args[9], np.float64), args[14])


class FakeRuntime:
    ctx = None
    closed = False

    def __init__(self, nobody=()):
        self.allocations = []
        self.nobody = tuple(nobody)  # the (flat sample, point) no particle of a trace with active apertures reaches
        self.lib = FakeLibrary(self)

    def free(self, ptr):
        pass

    def empty(self, shape, dtype):
        return FakeArray(self, "empty", shape, dtype)

    def empty_result(self, shape, dtype):
        return FakeArray(self, "empty_result", shape, dtype)

    def to_device(self, host):
        host = np.array(host)
        return FakeArray(self, "to_device", host.shape, host.dtype, host)

    def to_device_result(self, host):
        host = np.array(host)
        return FakeArray(self, "to_device_result", host.shape, host.dtype, host)

    def forward(self, name, shape, dtype=np.float64):
        return FakeArray(self, "forward:" + name, shape, dtype)

    def check(self, status):
        assert status == 0


def fabricated_records(batch, P, seed=0, nobody=(), count=N):
    """(*batch, P, 36) moment records of N particles drawn per sample and point, said to be of `count`; `nobody`: (flat
    sample, point) left empty."""
    rng = np.random.default_rng(seed)
    B = int(np.prod(batch, dtype=np.int64))
    rec = np.zeros((B, P, 36))
    rows, cols = np.triu_indices(6)
    for b in range(B):
        for k in range(P):
            z = rng.normal(size=(N, 6)) * [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3] + rng.normal(size=6) * 1e-5
            z[:, 1] += 0.05 * z[:, 0]
            z[:, 3] -= 0.03 * z[:, 2]
            d = z - z.mean(axis=0)
            rec[b, k, :6], rec[b, k, 6] = z.mean(axis=0), 1.0
            rec[b, k, 7:28] = (d.T @ d / N)[rows, cols]
            rec[b, k, 34], rec[b, k, 35] = 1.0, count
    for b, k in nobody:
        rec[b, k, :35], rec[b, k, 35] = np.nan, 0.0
    return rec.reshape(*batch, P, 36)


def fabricated_moments(batch, lead, dtype, seed):
    """mu (*batch, *lead, 7) and cov (*batch, *lead, 7, 7) of `fabricated_records`."""
    rec = fabricated_records(batch, int(np.prod(lead, dtype=np.int64)), seed).reshape(*batch, *lead, 36)
    mu, cov = np.zeros((*batch, *lead, 7)), np.zeros((*batch, *lead, 7, 7))
    rows, cols = np.triu_indices(6)
    mu[...] = rec[..., :7]
    cov[..., rows, cols] = rec[..., 7:28]
    cov[..., cols, rows] = rec[..., 7:28]
    return mu.astype(dtype), cov.astype(dtype)


def fabricated_energy(shape, seed):
    """Energies a cavity may meet: 10 MeV and a few steps of 0.25 MeV above it."""
    return 1e7 + 2.5e5 * np.random.default_rng(seed).integers(0, 9, size=shape)


def fake_engine_gpu(monkeypatch, nobody=()):
    """
    `lynx_amd` with the runtime replaced and nothing else, until `monkeypatch` is undone: `engine.track`, `track_along`,
    `transfer_map` and `cavity_rmatrix` run as they are, against a library that records.  Returns the runtime.
    """
    from lynx_amd import device, engine
    from lynx_amd.accelerator import diagnostics

    rt = FakeRuntime(nobody)
    for module in (device, engine, diagnostics):
        monkeypatch.setattr(module, "get_runtime", lambda: rt)
    return rt


def fake_gpu(monkeypatch, nobody=(), clamped=()):
    """
    `lynx_amd` with every way to the GPU replaced until `monkeypatch` is undone: returns (runtime, forward) -- `forward` the keyword arguments of every
    `engine.track_along`.  `nobody`: the (flat sample, point) no particle of a fabricated trace with losses reaches;
    `clamped`: the coordinates whose variance a fabricated outgoing ParameterBeam has at 1e-20 and below.
    """
    import lynx_amd as lx
    import lynx_amd.grad  # noqa: F401 (`import lynx_amd` does not import it)
    from lynx_amd import device, engine
    from lynx_amd.device import Dual
    from lynx_amd.trace import BeamTrace

    rt, forward = FakeRuntime(), []

    def track_along(owner, leaves, incoming, **kwargs):
        forward.append(kwargs)
        trace = fabricated_trace(owner, list(leaves), incoming, **kwargs)
        if kwargs.get("keep_energy"):  # (asked to keep the energies the real pass also leaves them on the device)
            B = int(np.prod(incoming.batch_shape, dtype=np.int64))
            trace._device["energy"] = rt.forward("energy", (B, trace.num_points), incoming.dtype)
        return trace

    def fabricated_trace(owner, leaves, incoming, **kwargs):
        batch, dtype = incoming.batch_shape, incoming.dtype
        B, P = int(np.prod(batch, dtype=np.int64)), len(leaves) + 1
        energy = np.broadcast_to(np.asarray(incoming.energy, dtype=np.float64)[..., None], (*batch, P)) * np.linspace(1.0, 1.5, P)
        lengths, names = [1.0] * (P - 1), [el.name for el in leaves]
        if isinstance(incoming, lx.ParticleBeam):
            chosen = kwargs.get("trajectories")
            losses = kwargs.get("losses", False)
            program = engine._trace_plan(owner, leaves, bool(losses))
            paths = None if chosen is None else np.zeros((*batch, P, len(chosen), 7))
            rec = fabricated_records(batch, P, 1, nobody if losses else ())
            trace = BeamTrace.from_records(rec, energy, lengths, names, dtype, apertures=[step for step, _, _ in program.apertures],
                                           trajectories=paths, trajectory_indices=chosen)
            trace._device = {"records": rt.forward("records", (B, P, 36))}
            if chosen is not None:
                trace._device["trajectories"] = rt.forward("trajectories", (B, P, len(chosen), 7), dtype)
            if losses == "particles":
                trace._device["lost_at"] = rt.forward("lost_at", (B, incoming.num_particles), np.int32)
            return trace
        program = engine._trace_plan(owner, leaves, bool(kwargs.get("losses")), bool(kwargs.get("screens")))
        shots = engine._screen_geometry(owner, program, batch, dtype, rt, False) if program.screens else {"shapes": []}
        mu, cov = fabricated_moments(batch, (P,), dtype, 2)
        trace = BeamTrace.from_moments(mu, cov, energy, lengths, names, dtype, screens=[step for step, _ in program.screens],
                                       screen_images=[np.zeros((*batch, *shape), dtype) for shape in shots["shapes"]])
        trace._device = {"mu": rt.forward("mu", (B, P, 7), dtype), "cov": rt.forward("cov", (B, P, 7, 7), dtype)}
        return trace

    def run_program_particles(cache, program, beam, moments=None):
        batch = beam.batch_shape
        rec = fabricated_records(batch, 1, 3).reshape(*batch, 36)
        record = rt.forward("moments", rec.shape)
        record.host = rec
        return lx.ParticleBeam._from_raw(Dual(dev=rt.forward("particles", (*batch, beam.num_particles, 7), beam.dtype)), beam._energy, None,
                                         beam.dtype, moments=Dual(dev=record))

    stretch = [0]

    def run_program_parameters(cache, program, beam):
        stretch[0] += 1
        mu, cov = fabricated_moments(beam.batch_shape, (), beam.dtype, 10 + stretch[0])
        for c in clamped:
            cov[..., c, c] = np.resize(np.array([1e-20, 1e-21, 0.0, 4e-8], dtype=cov.dtype), cov[..., c, c].shape)
        return lx.ParameterBeam._from_raw(Dual(mu), Dual(cov), beam._energy, beam.total_charge, beam.dtype)

    class Lattice:
        handle = None

        def __init__(self, program):
            self.E = len(program.leaves)

    def on_device(self, runtime=None):
        if self._dev is None:
            self._dev = rt.to_device(self._host)
        return self._dev

    patch = monkeypatch  # (the caller's own: whatever a test patches on top of this is undone in the right order)
    patch.setattr(engine, "track_along", track_along)
    patch.setattr(engine, "run_program_particles", run_program_particles)
    patch.setattr(engine, "run_program_parameters", run_program_parameters)
    patch.setattr(engine, "_ready", lambda cache, program, *a, **k: Lattice(program))
    patch.setattr(engine, "get_runtime", lambda: rt)
    patch.setattr(device, "get_runtime", lambda: rt)  # (`lynx_amd.grad` asks the module, every time)
    patch.setattr(Dual, "device", on_device)
    patch.setattr(Dual, "broadcast_device",
                  lambda self, runtime, shape: rt.to_device(np.ascontiguousarray(np.broadcast_to(self.host(), tuple(shape)))))
    return rt, forward


@pytest.fixture
def recorded(monkeypatch):
    """
    A vjp whose forward pass is fabricated on the host and whose reverse call goes to a library object that records it:
    (lynx_amd, the names of the entry points called so far, the keyword arguments of every `engine.track_along`).
    """
    import lynx_amd as lx

    rt, forward = fake_gpu(monkeypatch)
    return lx, rt.lib.calls, forward


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that asks for the GPU runtime fails the test."""
    from lynx_amd import device, engine

    def refuse(*args, **kwargs):
        raise AssertionError("track_along_vjp touched the GPU runtime")

    monkeypatch.setattr(device, "get_runtime", refuse)
    monkeypatch.setattr(engine, "get_runtime", refuse)
