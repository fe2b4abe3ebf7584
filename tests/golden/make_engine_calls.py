"""
A transcript of the forward host path (`lynx_amd/engine.py`), without a GPU: per case and per call of the public API
every library call with every argument by value, how every array was allocated, every uploaded byte
(tests/reverse_host_fakes.py: `fake_engine_gpu`), and what the caller sees -- the outgoing beam's fields and which of them
are the incoming beam's own objects, the trace's arrays, the elements' readings -- as the fake read-backs give them; for a
refusal the exception's type and text.  Only the public API and the fakes are used, so the script runs unchanged on any
commit's `engine.py`:

    python -m tests.golden.make_engine_calls        # writes tests/golden/engine_calls.npz

tests/test_engine_calls_host.py replays `CASES` and compares with that file byte for byte.  The file is made on the
commit BEFORE a change to `engine.py`, never with the code under test.
"""

from pathlib import Path

import numpy as np
import pytest

from tests.golden.make_reverse_calls import draw, flatten, full, load, save, spread  # noqa: F401 (`load`: for the test)
from tests.reverse_host_fakes import FakeArray, fake_engine_gpu

PATH = Path(__file__).resolve().parent / "engine_calls.npz"
SHAPES = (((2,), np.float64), ((2, 3), np.float32))
N = 5  # particles of every beam
CASES = {}


def case(name, **fake):
    def register(fn):
        CASES[name] = (fn, fake)
        return fn
    return register


# ---- what the caller sees ------------------------------------------------------------------------------------------------


def where(dual):
    return None if dual is None else ("host" if dual._host is not None else "") + ("device" if dual._dev is not None else "")


def seen(value):
    """A host-visible value as the transcript holds it (an array on the fake device is read back)."""
    return None if value is None else np.asarray(value)


def described(lx, beam, incoming=None):
    """A beam's fields, where they live before anybody looks, and which of them are `incoming`'s own objects."""
    if beam is None or beam is lx.Beam.empty:
        return None if beam is None else "Beam.empty"
    out = {"class": type(beam).__name__, "dtype": beam.dtype.str, "batch": list(beam.batch_shape), "is incoming": beam is incoming}
    if isinstance(beam, lx.ParticleBeam):
        fields = {"particles": beam._particles, "energy": beam._energy, "moments": beam._moments}
        out["where"] = {name: where(dual) for name, dual in fields.items()}
        out["shared"] = beam.is_shared
        out["charges"] = seen(beam._charges)
        out["moments"] = None if beam._moments is None else seen(beam._moments.host())
        out["particles"] = seen(beam.particles)
        own = ("_particles", "_energy", "_charges", "_moments")
    else:
        fields = {"mu": beam._mu_d, "cov": beam._cov_d, "energy": beam._energy}
        out["where"] = {name: where(dual) for name, dual in fields.items()}
        out["mu"], out["cov"], out["total_charge"] = seen(beam._mu_d.host()), seen(beam._cov_d.host()), seen(beam.total_charge)
        own = ("_mu_d", "_cov_d", "_energy", "total_charge")
    out["energy"] = seen(beam.energy)
    if incoming is not None and type(incoming) is type(beam):
        out["incoming's own"] = [name for name in own if getattr(beam, name) is not None and getattr(beam, name) is getattr(incoming, name)]
    return out


def plain(lx, value, incoming):
    """Whatever a trace holds, as dicts, lists, scalars and arrays."""
    if isinstance(value, lx.Beam):
        return described(lx, value, incoming)
    if isinstance(value, FakeArray):
        return value.tag()
    if isinstance(value, dict):
        return {str(key): plain(lx, item, incoming) for key, item in value.items()}
    if isinstance(value, (list, tuple)):
        return [plain(lx, item, incoming) for item in value]
    if isinstance(value, np.dtype):
        return value.str
    assert value is None or isinstance(value, (bool, int, float, str, np.ndarray, np.generic)), type(value)
    return value


def readings(lx, segment):
    """`reading` of every BPM, and of every Screen the beam a `track` parked on it or the image a trace left on it."""
    out = {}
    for el in segment._leaves() if isinstance(segment, lx.Segment) else [segment]:
        if isinstance(el, lx.BPM):
            out[el.name] = seen(el.reading)
        elif isinstance(el, lx.Screen):
            out[el.name] = {"read beam": described(lx, el.get_read_beam()), "image": seen(el._cached_reading)}
    return out


class Log:
    def __init__(self, lx, rt):
        self.lx, self.rt, self.events, self.owners = lx, rt, [], []

    def own(self, *owners):
        """These objects are handed to the engine as owners; what they hold now is theirs, not the engine's."""
        for owner in owners:
            self.owners.append((owner, set(owner.__dict__)))
        return owners[0] if len(owners) == 1 else owners

    def attempt(self, label, thunk, describe=lambda value: seen(value)):
        """Run `thunk`; record its library calls and allocations, and what it raised or `describe` of what it returned."""
        calls, made = len(self.rt.lib.records), len(self.rt.allocations)
        event = {"label": label}
        try:
            value = thunk()
        except Exception as error:  # noqa: BLE001 (the transcript is of whatever is raised)
            value = None
            event.update(raised=type(error).__name__, text=str(error))
        else:
            event["result"] = describe(value)
        event["calls"] = [{"entry": entry, "arguments": args} for entry, args in self.rt.lib.records[calls:]]
        event["allocations"] = [f"{a.how} {a.dtype.str} {list(a.shape)}" for a in self.rt.allocations[made:]]
        self.events.append(event)
        return value

    def track(self, label, owner, beam):
        lx = self.lx
        return self.attempt(label, lambda: owner.track(beam),
                            lambda out: {"outgoing": described(lx, out, beam), "readings": readings(lx, owner)})

    def trace(self, label, segment, beam, call=None, **kwargs):
        lx = self.lx
        call = call or (lambda: segment.track_along(beam, **kwargs))
        return self.attempt(label, call, lambda trace: {"class": type(trace).__name__, "readings": readings(lx, segment),
                                                        "trace": {key: plain(lx, item, beam) for key, item in sorted(vars(trace).items())}})


def transcript(name, owners=None):
    """The transcript of one case as a tree of dicts, lists, scalars and arrays; `owners`: a list that takes the case's
    (owner, the attributes it held before the engine saw it)."""
    import lynx_amd as lx

    fn, fake = CASES[name]
    switches = {key: getattr(lx.config, key) for key in ("fused_moments", "fused_covariance", "merge_steps")}
    with pytest.MonkeyPatch.context() as monkeypatch:
        log = Log(lx, fake_engine_gpu(monkeypatch, **fake))
        try:
            fn(lx, log)
        finally:
            for key, value in switches.items():
                setattr(lx.config, key, value)
    if owners is not None:
        owners.extend(log.owners)
    return {"events": log.events}


# ---- the cases -----------------------------------------------------------------------------------------------------------


def particle_beam(lx, batch, dtype, charges=False, seed=5):
    rng = np.random.default_rng(seed)
    particles = draw(rng, (*batch, N, 7)) * 1e-4
    particles[..., 6] = 1.0
    return lx.ParticleBeam(particles.astype(dtype), spread(batch, 6e6, 8e6, dtype), dtype=dtype,
                           particle_charges=(draw(rng, (*batch, N)) * 1e-12).astype(dtype) if charges else None)


def parameter_beam(lx, batch, dtype):
    return lx.ParameterBeam.from_parameters(mu_x=spread(batch, -1e-5, 2e-5, dtype), sigma_x=full(batch, 1e-4, dtype), sigma_xp=full(batch, 1e-5, dtype),
                                            sigma_y=full(batch, 2e-4, dtype), sigma_yp=full(batch, 1e-5, dtype), sigma_s=full(batch, 1e-5, dtype),
                                            sigma_p=full(batch, 1e-3, dtype), energy=spread(batch, 6e6, 8e6, dtype),
                                            total_charge=full(batch, 1e-10, dtype), dtype=dtype)


def parts(lx, batch, dtype):
    """Drift, quadrupole, active cavity, active BPM, quadrupole."""
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    return [lx.Drift(f(0.5), name="D0", dtype=dtype), lx.Quadrupole(f(0.2), k1=spread(batch, -3, 4, dtype), name="Q1", dtype=dtype),
            lx.Cavity(f(1.0), voltage=spread(batch, 1e7, 2e7, dtype), phase=f(3.0), frequency=f(1.3e9), name="CAV", dtype=dtype),
            lx.BPM(is_active=True, name="BPM"), lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q2", dtype=dtype)]


def track_particles(batch, dtype):
    def run(lx, log):
        segment = log.own(lx.Segment(parts(lx, batch, dtype), name="LINE"))
        beam = particle_beam(lx, batch, dtype)
        log.track("the defaults", segment, beam)
        for switch, value in (("fused_moments", False), ("fused_covariance", True), ("merge_steps", False)):
            before = getattr(lx.config, switch)
            setattr(lx.config, switch, value)
            log.track(f"config.{switch} = {value}", segment, beam)
            setattr(lx.config, switch, before)
        single = particle_beam(lx, (1,), dtype, charges=True, seed=6)
        log.track("a lazily broadcast shared beam with charges", segment, single.broadcast(batch))
        log.track("a beam of its own with charges", segment, particle_beam(lx, batch, dtype, charges=True))
        d0, q1, cav, bpm, q2 = parts(lx, batch, dtype)
        nested = log.own(lx.Segment([d0, lx.Segment([q1, cav], name="INNER"), lx.Segment([bpm], name="SKIPPED"), q2], name="NESTED"))
        log.track("a nested non-skippable segment", nested, beam)
        many = parts(lx, batch, dtype)
        many[1:2] = [lx.BPM(is_active=True, name=f"BPM{k}") for k in range(9)]  # (one more than a program reads inside the pass)
        log.track("nine active BPMs in a row", log.own(lx.Segment(many, name="MANY")), beam)
        log.track("Element.track", log.own(q1), beam)
        log.track("Element.track of the cavity", log.own(cav), beam)
        log.track("Beam.empty", segment, lx.Beam.empty)
    return run


for _batch, _dtype in SHAPES:
    case(f"track, ParticleBeam, {_batch} {np.dtype(_dtype).name}")(track_particles(_batch, _dtype))


def track_parameters(batch, dtype):
    def run(lx, log):
        beam = parameter_beam(lx, batch, dtype)
        d0, q1, cav, bpm, q2 = parts(lx, batch, dtype)
        log.track("with the cavity", log.own(lx.Segment([d0, q1, cav, bpm, q2], name="LINE")), beam)
        log.track("without the cavity", log.own(lx.Segment([d0, q1, bpm, q2], name="SHORT")), beam)
        screen = lx.Screen(resolution=(3, 2), pixel_size=(1e-4, 1e-4), misalignment=np.array([1e-5, -2e-5]), is_active=True, name="SCR", dtype=dtype)
        behind = lx.BPM(is_active=True, name="BEHIND")
        log.track("an active Screen in the middle", log.own(lx.Segment([d0, q1, screen, behind, q2], name="SCREENED")), beam)
        aperture = lx.Aperture(x_max=full(batch, 1e-3, dtype), y_max=full(batch, 1e-3, dtype), is_active=True, name="AP", dtype=dtype)
        log.track("an active Aperture in the middle", log.own(lx.Segment([d0, aperture, q2], name="CLIPPED")), beam)
        log.track("Element.track", log.own(q2), beam)
        log.track("Element.track of the cavity", log.own(cav), beam)
    return run


for _batch, _dtype in SHAPES:
    case(f"track, ParameterBeam, {_batch} {np.dtype(_dtype).name}")(track_parameters(_batch, _dtype))


def track_again(batch, dtype, make_beam):
    def run(lx, log):
        elements = parts(lx, batch, dtype)
        segment = log.own(lx.Segment(elements, name="LINE"))
        beam = make_beam(lx, batch, dtype)
        log.track("the first call", segment, beam)
        log.track("unchanged", segment, beam)
        elements[1].k1 = spread(batch, 1, 2, dtype)
        log.track("after quad.k1 = ...", segment, beam)
        elements[2].voltage = full(batch, 1.5e7, dtype)
        log.track("after cavity.voltage = ...", segment, beam)
        segment.elements.append(lx.Drift(full(batch, 0.3, dtype), name="D9", dtype=dtype))
        log.track("after segment.elements.append(...)", segment, beam)
        log.trace("track_along, the first call", segment, beam)
        elements[4].k1 = full(batch, -2.5, dtype)
        log.trace("track_along after quad.k1 = ...", segment, beam)
        log.track("track after that", segment, beam)
    return run


case("a second and a third call, ParticleBeam")(track_again((2,), np.float64, particle_beam))
case("a second and a third call, ParameterBeam")(track_again((2, 3), np.float32, parameter_beam))


def diagnosed(lx, batch, dtype, apertures, screens, per_sample=False):
    """Quadrupole, aperture, active cavity, active BPM, screen of 3 x 2 pixels, elliptical aperture, drift, screen of one pixel,
    aperture: three apertures and two screens, so that no stride of the one list is a stride of the other."""
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    rng = np.random.default_rng(31)
    limit = (lambda v: spread(batch, v, 2 * v, dtype)) if per_sample else (lambda v: np.array(v, dtype=dtype))
    shift = (lambda: draw(rng, (*batch, 2)) * 1e-5) if per_sample else (lambda: draw(rng, (2,)) * 1e-5)
    return lx.Segment([
        lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="Q", dtype=dtype),
        lx.Aperture(x_max=limit(1e-3), y_max=limit(2e-3), is_active=apertures, name="AP0", dtype=dtype),
        lx.Cavity(f(1.0), voltage=spread(batch, 1e7, 2e7, dtype), phase=f(3.0), frequency=f(1.3e9), name="CAV", dtype=dtype),
        lx.BPM(is_active=True, name="BPM"),
        lx.Screen(resolution=(3, 2), pixel_size=(1e-4, 1e-4), misalignment=shift(), is_active=screens, name="SCR0", dtype=dtype),
        lx.Aperture(x_max=limit(2e-3), y_max=limit(1e-3), shape="elliptical", is_active=apertures, name="AP1", dtype=dtype),
        lx.Drift(f(0.4), name="D", dtype=dtype),
        lx.Screen(resolution=(1, 1), pixel_size=(2e-4, 2e-4), misalignment=shift(), is_active=screens, name="SCR1", dtype=dtype),
        lx.Aperture(x_max=limit(3e-3), y_max=limit(3e-3), is_active=apertures, name="AP2", dtype=dtype)], name="DIAGNOSED")


def trace_particles(batch, dtype):
    def run(lx, log):
        beam = particle_beam(lx, batch, dtype)
        bare = log.own(diagnosed(lx, batch, dtype, False, False))
        log.trace("plain", bare, beam)
        log.trace("keep_outgoing=False", bare, beam, keep_outgoing=False)
        log.trace("keep_device=True", bare, beam, call=lambda: lx.engine.track_along(bare, bare._leaves(), beam, keep_device=True))
        log.trace("trajectories=2", bare, beam, trajectories=2)
        log.trace("losses=True, no active aperture", bare, beam, losses=True)
        log.trace("a shared beam with charges", bare, particle_beam(lx, (1,), dtype, charges=True, seed=6).broadcast(batch))
        log.trace("a beam of its own with charges", bare, particle_beam(lx, batch, dtype, charges=True))
        collimated = log.own(diagnosed(lx, batch, dtype, True, False))
        log.trace("losses=True", collimated, beam, losses=True)
        log.trace("losses='particles'", collimated, beam, losses="particles")
        log.trace("losses and trajectories", collimated, beam, losses=True, trajectories=np.array([3, 3]))
        screened = log.own(diagnosed(lx, batch, dtype, False, True))
        log.trace("screens=True", screened, beam, screens=True)
        log.trace("screens and trajectories", screened, beam, screens=True, trajectories=np.array([3, 3]))
        for label, per_sample in (("shared", False), ("per sample", True)):
            both = log.own(diagnosed(lx, batch, dtype, True, True, per_sample))
            log.trace(f"screens with losses, limits and misalignments {label}", both, beam, screens=True, losses=True)
            log.trace(f"the same call again, {label}", both, beam, screens=True, losses=True)
            log.trace(f"trajectories with losses and screens, {label}", both, beam, screens=True, losses="particles", trajectories=np.array([3, 3]),
                      call=lambda: lx.engine.track_along(both, both._leaves(), beam, keep_device=True, screens=True, losses="particles",
                                                         trajectories=np.array([3, 3])))
            both.AP1.x_max = both.AP1.x_max * 2
            log.trace(f"after a limit is rewritten, {label}", both, beam, screens=True, losses=True)
            both.SCR1.misalignment = both.SCR1.misalignment * 2
            log.trace(f"after a misalignment is rewritten, {label}", both, beam, screens=True, losses=True)
    return run


for _batch, _dtype in SHAPES:
    case(f"track_along, ParticleBeam, {_batch} {np.dtype(_dtype).name}")(trace_particles(_batch, _dtype))


@case("track_along, ParticleBeam, a sample loses everybody", nobody=((0, 9), (1, 8), (1, 9)))
def _(lx, log):
    batch, dtype = (2,), np.float64
    beam = particle_beam(lx, batch, dtype)
    both = log.own(diagnosed(lx, batch, dtype, True, True))
    log.trace("losses=True", both, beam, losses=True, screens=True)
    log.trace("losses='particles' and trajectories", both, beam, losses="particles", screens=True, trajectories=2)


def trace_parameters(batch, dtype):
    def run(lx, log):
        beam = parameter_beam(lx, batch, dtype)
        bare = log.own(diagnosed(lx, batch, dtype, False, False))
        log.trace("plain", bare, beam)
        log.trace("keep_outgoing=False", bare, beam, keep_outgoing=False)
        log.trace("keep_device=True", bare, beam, call=lambda: lx.engine.track_along(bare, bare._leaves(), beam, keep_device=True))
        for label, per_sample in (("shared", False), ("per sample", True)):
            both = log.own(diagnosed(lx, batch, dtype, True, True, per_sample))
            log.trace(f"screens=True and losses, misalignments {label}", both, beam, screens=True, losses=True)
            log.trace(f"the same call again, {label}", both, beam, screens=True, losses=True)
            log.trace(f"screens='points', {label}", both, beam, screens="points", losses=True)
            both.SCR0.misalignment = both.SCR0.misalignment * 2
            log.trace(f"after a misalignment is rewritten, {label}", both, beam, screens=True, losses=True)
        without = log.own(lx.Segment([el for el in parts(lx, batch, dtype) if el.name != "CAV"], name="SHORT"))
        log.trace("without a cavity", without, beam)
    return run


for _batch, _dtype in SHAPES:
    case(f"track_along, ParameterBeam, {_batch} {np.dtype(_dtype).name}")(trace_parameters(_batch, _dtype))


@case("transfer maps")
def _(lx, log):
    for batch, dtype in SHAPES:
        f = lambda v: full(batch, v, dtype)  # noqa: E731
        d0, q1, cav, bpm, q2 = parts(lx, batch, dtype)
        bpm.is_active = False
        energy = spread(batch, 6e6, 8e6, dtype)
        segment = log.own(lx.Segment([d0, q1, bpm, q2], name="SKIPPABLE"))
        log.attempt("a skippable segment", lambda: segment.transfer_map(energy))
        log.attempt("the same again", lambda: segment.transfer_map(energy))
        log.attempt("a segment with an active cavity", lambda: log.own(lx.Segment([d0, cav], name="NOT")).transfer_map(energy))
        log.attempt("an element", lambda: log.own(q1).transfer_map(energy))
        log.attempt("an empty list", lambda: log.own(lx.Segment([], name="EMPTY")).transfer_map(energy))
        log.attempt("Cavity.transfer_map, on", lambda: log.own(cav).transfer_map(energy))
        off = log.own(lx.Cavity(f(1.0), voltage=f(0.0), phase=f(0.0), frequency=f(1.3e9), name="OFF", dtype=dtype))
        log.attempt("Cavity.transfer_map, off", lambda: off.transfer_map(energy))
        log.attempt("an energy of another shape", lambda: q1.transfer_map(np.ones(5, dtype=dtype)))


@case("refusals")
def _(lx, log):
    batch, dtype = (2,), np.float64
    beam, moments = particle_beam(lx, batch, dtype), parameter_beam(lx, batch, dtype)
    segment = log.own(lx.Segment(parts(lx, batch, dtype), name="LINE"))
    both = log.own(diagnosed(lx, batch, dtype, True, True))
    log.attempt("track: an invalid incoming", lambda: segment.track(np.ones((2, N, 7))))
    log.attempt("track_along: an invalid incoming", lambda: segment.track_along(np.ones((2, N, 7))))
    log.attempt("an active Aperture without losses", lambda: both.track_along(beam, screens=True))
    log.attempt("an active Screen without screens", lambda: both.track_along(beam, losses=True))
    log.attempt("neither", lambda: both.track_along(moments))
    for bad in ("yes", 1, None):
        log.attempt(f"losses={bad!r}", lambda: both.track_along(beam, losses=bad, screens=True))
    log.attempt("screens='points' with a ParticleBeam", lambda: both.track_along(beam, losses=True, screens="points"))
    log.attempt("trajectories of a ParameterBeam", lambda: both.track_along(moments, losses=True, screens=True, trajectories=2))
    log.attempt("an index outside the beam", lambda: both.track_along(beam, losses=True, screens=True, trajectories=[N]))
    other = particle_beam(lx, (3,), dtype)
    log.attempt("track: a beam shape that does not match an element's", lambda: segment.track(other))
    log.attempt("track: the same, ParameterBeam", lambda: segment.track(parameter_beam(lx, (3,), dtype)))
    log.attempt("track_along: the same", lambda: segment.track_along(other))
    limits = lx.Aperture(x_max=spread(batch, 1e-3, 2e-3, dtype), y_max=np.array(1e-3, dtype=dtype), name="AP", dtype=dtype)
    log.attempt("track_along: an aperture's limits of another shape", lambda: log.own(lx.Segment([limits], name="A")).track_along(other, losses=True))
    shifted = lx.Screen(resolution=(3, 2), misalignment=np.zeros((*batch, 2)), is_active=True, name="SCR", dtype=dtype)
    log.attempt("track_along: a screen's misalignment of another shape", lambda: log.own(lx.Segment([shifted], name="B")).track_along(other, screens=True))
    log.attempt("track_along: the same, ParameterBeam", lambda: log.own(lx.Segment([shifted], name="C")).track_along(parameter_beam(lx, (3,), dtype), screens=True))
    log.attempt("a screen without pixels", lambda: log.own(lx.Segment([lx.Screen(resolution=(0, 2), is_active=True, name="NONE")], name="S")).track_along(beam, screens=True))
    log.attempt("an aperture of unknown shape", lambda: log.own(lx.Segment([lx.Aperture(shape="round", name="ROUND")], name="R")).track_along(beam, losses=True))


# ---- the file ------------------------------------------------------------------------------------------------------------


if __name__ == "__main__":
    arrays = []
    index = {name: flatten(transcript(name), arrays) for name in CASES}
    save(PATH, index, arrays)
    events = [event for entry in index.values() for event in entry["events"]]
    print(f"{len(CASES)} cases, {len(events)} events, {sum(len(e['calls']) for e in events)} library calls, "
          f"{sum('raised' in e for e in events)} refusals, {len(arrays)} arrays, {PATH.stat().st_size} bytes")
    for event in events:
        if "raised" in event:
            print(f"  {event['label']}: {event['raised']}: {event['text'][:150]}")
