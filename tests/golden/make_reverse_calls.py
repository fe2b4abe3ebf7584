"""
A transcript of every call `lynx_amd.grad` makes, without a GPU: per case the keyword arguments given to
`engine.track_along`, every library call with every argument by value (tests/reverse_host_fakes.py), everything
`Gradients` hands out, and for a refusal the exception's type and text.  Only the public API of `lynx_amd.grad` is used,
so the cases run unchanged on any commit's `lynx_amd.grad` -- given fakes that stand in for the runtime where that commit
asks for it: `fake_gpu` replaces `device.get_runtime`, and both files were made on commits whose `grad.py` bound a copy of
its own, with a `fake_gpu` that replaced `grad.get_runtime` as well:

    python -m tests.golden.make_reverse_calls reverse    # writes tests/golden/reverse_calls.npz: `CASES`
    python -m tests.golden.make_reverse_calls targets    # writes tests/golden/target_calls.npz: `TARGET_CASES`

`CASES` are `track_vjp` and the five modes of `track_along_vjp`; `TARGET_CASES` are `image_targets=`, `moment_targets=` and
forward mode (`track_along_jvp`, `orbit_response_matrix`), with what their objects hand out and every allocation in order.
tests/test_reverse_calls_host.py replays both and compares with the files byte for byte.  A file is made on the commit
BEFORE a change to `lynx_amd.grad`, never with the code under test.
"""

import json
from pathlib import Path

import numpy as np
import pytest

from tests.reverse_host_fakes import FakeArray, fake_gpu

PATH = Path(__file__).resolve().parent / "reverse_calls.npz"
TARGET_PATH = Path(__file__).resolve().parent / "target_calls.npz"
PROPERTIES = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
              "sigma_p", "sigma_xxp", "sigma_yyp", "emittance_x", "emittance_y", "normalized_emittance_x",
              "normalized_emittance_y", "beta_x", "beta_y", "alpha_x", "alpha_y")  # tests/test_trace_grad_host.py
BEAM_PROPERTIES = ("mu_y", "sigma_x", "sigma_p", "sigma_xxp", "sigma_yyp")
CASES, TARGET_CASES = {}, {}


def case(name, cases=CASES, **fake):
    def register(fn):
        cases[name] = (fn, fake)
        return fn
    return register


def target_case(name, **fake):
    return case(name, TARGET_CASES, **fake)


def handed_out(g, segment):
    """Everything a `Gradients` (or `ChainedGradients`) gives: per leaf element, and each property as array, None or error."""
    out = {}
    for k, el in enumerate(segment._leaves()):
        try:
            out[f"element {k}"] = {"contained": el in g, "values": dict(g[el])}
        except KeyError as error:
            out[f"element {k}"] = {"contained": el in g, "KeyError": str(error)}
    for name in ("energy", "mu", "cov", "particles", "chosen_particles"):
        try:
            value = getattr(g, name)
            out[name] = value.tag() if isinstance(value, FakeArray) else None if value is None else np.asarray(value)
        except (KeyError, AttributeError) as error:
            out[name] = {type(error).__name__: str(error)}
    return out


class Log:
    def __init__(self):
        self.events = []

    def attempt(self, label, thunk, segment=None):
        """Run `thunk`; record what it raised, or -- with `segment` -- what the Gradients it returned hand out."""
        try:
            value = thunk()
        except Exception as error:  # noqa: BLE001 (the transcript is of whatever is raised)
            self.events.append({"label": label, "raised": type(error).__name__, "text": str(error)})
            return None
        self.events.append({"label": label, "gradients": None if segment is None else handed_out(value, segment)})
        return value

    def value(self, label, thunk):
        """Run `thunk`; record what it raised or the value it returned: arrays, scalars, strings, lists and dicts of them."""
        try:
            self.events.append({"label": label, "value": thunk()})
        except Exception as error:  # noqa: BLE001
            self.events.append({"label": label, "raised": type(error).__name__, "text": str(error)})


def transcript(name):
    """The transcript of one case as a tree of dicts, lists, scalars and arrays."""
    import lynx_amd as lx

    fn, fake = CASES[name] if name in CASES else TARGET_CASES[name]
    log = Log()
    ddof = lx.config.std_ddof
    with pytest.MonkeyPatch.context() as monkeypatch:
        rt, forward = fake_gpu(monkeypatch, **fake)
        try:
            fn(lx, log)
        finally:
            lx.config.std_ddof = ddof
    out = {"forward": list(forward), "calls": [{"entry": entry, "arguments": args} for entry, args in rt.lib.records], "events": log.events}
    if name in TARGET_CASES:  # ... and every allocation in order: an upload made once shows as one
        out["allocations"] = [f"{a.how} {list(a.shape)} {a.dtype.str}" for a in rt.allocations]
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------


def draw(rng, shape):
    """Cotangents of few distinct values (multiples of 1/4 up to 2): they sum exactly and the file compresses."""
    return rng.integers(-8, 9, size=shape) / 4.0


def full(batch, value, dtype):
    return np.full(batch, value, dtype=dtype)


def spread(batch, lo, hi, dtype):
    return np.linspace(lo, hi, int(np.prod(batch))).reshape(batch).astype(dtype)


def particle_beam(lx, batch, dtype, energy=None):
    rng = np.random.default_rng(5)
    particles = draw(rng, (*batch, 16, 7)) * 1e-4
    particles[..., 6] = 1.0
    return lx.ParticleBeam(particles.astype(dtype), spread(batch, 6e6, 8e6, dtype) if energy is None else energy, dtype=dtype)


def parameter_beam(lx, batch, dtype):
    return lx.ParameterBeam.from_parameters(mu_x=spread(batch, -1e-5, 2e-5, dtype), sigma_x=full(batch, 1e-4, dtype), sigma_xp=full(batch, 1e-5, dtype),
                                            sigma_y=full(batch, 2e-4, dtype), sigma_yp=full(batch, 1e-5, dtype), sigma_s=full(batch, 1e-5, dtype),
                                            sigma_p=full(batch, 1e-3, dtype), energy=spread(batch, 6e6, 8e6, dtype), dtype=dtype)


def mixed_lattice(lx, batch, dtype, bpm_active=True):
    """A Quadrupole with misalignment, an RBend, an active BPM, a corrector whose angle has shape (1,) against the batch."""
    quad = lx.Quadrupole(full(batch, 0.2, dtype), k1=spread(batch, -3, 4, dtype), misalignment=np.stack([spread(batch, 1e-5, 3e-5, dtype)] * 2, axis=-1),
                         name="Q", dtype=dtype)
    bend = lx.RBend(full(batch, 0.5, dtype), angle=spread(batch, 0.1, 0.2, dtype), e1=full(batch, 0.01, dtype), name="RB", dtype=dtype)
    bpm = lx.BPM(is_active=bpm_active, name="BPM")
    corrector = lx.HorizontalCorrector(full(batch, 0.1, dtype), angle=np.array([1e-4], dtype=dtype), name="HC", dtype=dtype)
    return lx.Segment([lx.Drift(full(batch, 0.6, dtype), name="D0", dtype=dtype), quad, bend, bpm, corrector]), bpm


def track_vjp_particles(batch, dtype):
    def run(lx, log):
        rng = np.random.default_rng(21)
        segment, bpm = mixed_lattice(lx, batch, dtype)
        vjp = lx.grad.track_vjp(segment, particle_beam(lx, batch, dtype))
        mu_bar, cov_bar = draw(rng, (*batch, 6)), draw(rng, (*batch, 6, 6))
        named = {name: draw(rng, batch) for name in BEAM_PROPERTIES}
        log.attempt("mu_bar", lambda: vjp(mu_bar=mu_bar), segment)
        log.attempt("cov_bar", lambda: vjp(cov_bar=cov_bar), segment)
        for ddof in (0, 1):
            lx.config.std_ddof = ddof
            log.attempt(f"properties, ddof {ddof}", lambda: vjp(**named), segment)
            log.attempt(f"properties and both, ddof {ddof}", lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, sigma_x=1.5, mu_y=named["mu_y"]), segment)
        log.attempt("readings", lambda: vjp(readings={bpm: draw(rng, (2, *batch))}, mu_bar=mu_bar), segment)
        log.attempt("wrt_particles", lambda: vjp(cov_bar=cov_bar, wrt_particles=True), segment)
        log.attempt("an unknown property", lambda: vjp(beta_x=1.0))
        log.attempt("a reading of no BPM", lambda: vjp(readings={segment.Q: np.ones((2, *batch))}))
        shared = lx.grad.track_vjp(segment, particle_beam(lx, batch, dtype, energy=np.asarray(7e6, dtype=dtype)))
        log.attempt("an energy of shape ()", lambda: shared(mu_bar=mu_bar, sigma_p=named["sigma_p"]), segment)
        log.attempt("a ParameterBeam's class", lambda: lx.grad.TrackVJP(segment, parameter_beam(lx, batch, dtype)))
    return run


case("track_vjp, ParticleBeam, (3,) float64")(track_vjp_particles((3,), np.float64))
case("track_vjp, ParticleBeam, (2, 2) float32")(track_vjp_particles((2, 2), np.float32))


def track_vjp_parameters(batch, dtype, bpms):
    def run(lx, log):
        rng = np.random.default_rng(22)
        f = lambda v: full(batch, v, dtype)  # noqa: E731
        twice = lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="QQ", dtype=dtype)
        first, second = lx.BPM(is_active=bpms, name="BPM1"), lx.BPM(is_active=bpms, name="BPM2")
        segment = lx.Segment([lx.Drift(f(0.5), name="D0", dtype=dtype), twice, first, lx.RBend(f(0.5), angle=spread(batch, 0.1, 0.2, dtype), name="RB", dtype=dtype),
                              twice, second, lx.VerticalCorrector(f(0.1), angle=np.array([2e-4], dtype=dtype), name="VC", dtype=dtype)])
        vjp = lx.grad.track_vjp(segment, parameter_beam(lx, batch, dtype))
        readings = {first: draw(rng, (2, *batch)), second: draw(rng, (2, *batch))} if bpms else None
        for width in (6, 7):
            mu_bar, cov_bar = draw(rng, (*batch, width)), draw(rng, (*batch, width, width))
            log.attempt(f"mu_bar {width}", lambda: vjp(mu_bar=mu_bar, readings=readings), segment)
            log.attempt(f"cov_bar {width}", lambda: vjp(cov_bar=cov_bar), segment)
            log.attempt(f"both {width} and properties", lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, readings=readings, sigma_y=draw(rng, batch),
                                                                      sigma_x=2.0, mu_xp=-1.0, sigma_xxp=0.5, sigma_yyp=draw(rng, batch)), segment)
        log.attempt("an unknown property", lambda: vjp(emittance_x=1.0))
        log.attempt("a reading of no BPM", lambda: vjp(readings={twice: np.ones((2, *batch))}))
    return run


case("track_vjp, ParameterBeam, one stretch, (3,) float64")(track_vjp_parameters((3,), np.float64, False))
case("track_vjp, ParameterBeam, three stretches, (2, 2) float32", clamped=(0, 5))(track_vjp_parameters((2, 2), np.float32, True))
case("track_vjp, ParameterBeam, three stretches, (4,) float64", clamped=(2,))(track_vjp_parameters((4,), np.float64, True))


@case("track_vjp, ParameterBeam, refusals")
def _(lx, log):
    f = lambda v: np.array([v], dtype=np.float64)  # noqa: E731
    beam = parameter_beam(lx, (1,), np.float64)
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1", dtype=np.float64)
    drift = lx.Drift(f(1.0), name="D", dtype=np.float64)
    log.attempt("a cavity in front of a BPM", lambda: lx.grad.track_vjp(lx.Segment([cavity, lx.BPM(is_active=True, name="BPM"), drift]), beam))
    log.attempt("an active screen", lambda: lx.grad.track_vjp(lx.Segment([drift, lx.Screen(is_active=True, name="SCR")]), beam))
    only = lx.Segment([lx.BPM(is_active=True, name="BPM")])
    log.attempt("nothing to differentiate", lambda: lx.grad.track_vjp(only, beam)())


def odd_cotangents(lx, log, vjp, segment, lead, widths=(6, 7)):
    """Cotangents at the edge of what each class takes: raveled, of another width, a scalar, `-0.0` (the sign is uploaded or not).
    What the library is given is the matter: what `Gradients` hands out is in the other cases."""
    rng = np.random.default_rng(27)
    for width in widths:
        mu_bar, cov_bar = draw(rng, (*lead, width)), draw(rng, (*lead, width, width))
        mu_bar[..., 0], cov_bar[..., 1, 1], cov_bar[..., 0, 2] = -0.0, -0.0, -0.0
        log.attempt(f"mu_bar {width} wide with -0.0", lambda: vjp(mu_bar=mu_bar))
        log.attempt(f"cov_bar {width} wide with -0.0", lambda: vjp(cov_bar=cov_bar))
        log.attempt(f"both {width} wide with -0.0 and a property", lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, sigma_x=1.0))
        log.attempt(f"mu_bar {width} wide, raveled", lambda: vjp(mu_bar=mu_bar.ravel()))
        log.attempt(f"mu_bar {width} wide, raveled, and a property", lambda: vjp(mu_bar=mu_bar.ravel(), mu_x=1.0))
        log.attempt(f"cov_bar {width} wide, rows raveled", lambda: vjp(cov_bar=cov_bar.reshape(*lead, -1)))
        log.attempt(f"both {width} wide, the batch flattened", lambda: vjp(mu_bar=mu_bar.reshape(-1, *mu_bar.shape[-2:]), cov_bar=cov_bar.reshape(-1, *cov_bar.shape[-3:])))
    log.attempt("mu_bar a scalar", lambda: vjp(mu_bar=1.0))
    log.attempt("cov_bar a scalar", lambda: vjp(cov_bar=1.0))
    log.attempt("mu_bar a whole record wide", lambda: vjp(mu_bar=draw(rng, (*lead, 36))))


@case("odd cotangents, track_vjp")
def _(lx, log):
    for batch, dtype in (((3,), np.float64), ((2, 2), np.float32)):
        segment, bpm = mixed_lattice(lx, batch, dtype)
        odd_cotangents(lx, log, lx.grad.track_vjp(segment, particle_beam(lx, batch, dtype)), segment, batch)
        bpm.is_active = batch == (3,)  # (two stretches, then one)
        odd_cotangents(lx, log, lx.grad.track_vjp(segment, parameter_beam(lx, batch, dtype)), segment, batch)


@case("odd cotangents, track_along_vjp")
def _(lx, log):
    batch, dtype = (2, 2), np.float32
    segment, _ = mixed_lattice(lx, batch, dtype)
    odd_cotangents(lx, log, lx.grad.track_along_vjp(segment, particle_beam(lx, batch, dtype)), segment, (*batch, 6), widths=(6,))
    odd_cotangents(lx, log, lx.grad.track_along_vjp(segment, parameter_beam(lx, batch, dtype)), segment, (*batch, 6), widths=(7,))


def cotangent_calls(lx, log, vjp, segment, batch, bpm=None, width=6, **more):
    """Every kind of moment cotangent, with `energy_bar` absent, all zero (the energy pointer is None) and non-zero."""
    rng = np.random.default_rng(23)
    lead = (*batch, len(list(segment._leaves())) + 1)
    mu_bar, cov_bar = draw(rng, (*lead, width)), draw(rng, (*lead, width, width))
    readings = None if bpm is None else {bpm: draw(rng, (2, *batch))}
    for label, energy_bar in (("no", None), ("zero", np.zeros(lead)), ("non-zero", draw(rng, lead))):
        log.attempt(f"mu_bar, cov_bar, readings; {label} energy_bar",
                    lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, energy_bar=energy_bar, readings=readings, **more), segment)
    log.attempt("every property as a scalar", lambda: vjp(**{name: 0.5 + k for k, name in enumerate(PROPERTIES + ("energy",))}, **more), segment)
    arrays = {name: draw(rng, lead) for name in PROPERTIES + ("energy",)}
    log.attempt("every property as an array, with all the rest",
                lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, energy_bar=np.ones(lead), readings=readings, **arrays, **more), segment)
    log.attempt("nothing at all", lambda: vjp(**more), segment)
    log.attempt("an unknown property", lambda: vjp(sigma_xy=1.0))
    log.attempt("a reading of no BPM", lambda: vjp(readings={segment.Q: np.ones((2, *batch))}))


@case("track_along_vjp, ParameterBeam, (3,) float64")
def _(lx, log):
    segment, bpm = mixed_lattice(lx, (3,), np.float64)
    vjp = log.attempt("plain", lambda: lx.grad.track_along_vjp(segment, parameter_beam(lx, (3,), np.float64)))
    cotangent_calls(lx, log, vjp, segment, (3,), bpm, width=7)
    log.attempt("wrt_particles", lambda: vjp(mu_x=1.0, wrt_particles=True))
    log.attempt("screen_images_bar", lambda: vjp(screen_images_bar={}))
    log.attempt("trajectories_bar", lambda: vjp(trajectories_bar=np.ones(6)))


@case("track_along_vjp, ParameterBeam, losses and cavities, (2, 2) float32")
def _(lx, log):
    batch, dtype = (2, 2), np.float32
    segment, bpm = mixed_lattice(lx, batch, dtype)
    aperture = lx.Aperture(x_max=full(batch, 1e-3, dtype), y_max=full(batch, 1e-3, dtype), is_active=True, name="AP", dtype=dtype)
    cavity = lx.Cavity(full(batch, 1.0, dtype), voltage=full(batch, 1e7, dtype), phase=full(batch, 0.0, dtype), frequency=full(batch, 1.3e9, dtype), name="ACC1",
                       dtype=dtype)
    segment = lx.Segment([*segment.elements[1:4], aperture, cavity])  # (Q, RB, BPM, AP, ACC1)
    beam = parameter_beam(lx, batch, dtype)
    log.attempt("an active aperture without losses", lambda: lx.grad.track_along_vjp(segment, beam))
    log.attempt("losses and cavities", lambda: lx.grad.track_along_vjp(segment, beam, losses=True, cavities=True))
    vjp = log.attempt("losses", lambda: lx.grad.track_along_vjp(segment, beam, losses=True))
    cotangent_calls(lx, log, vjp, segment, batch, bpm)
    aperture.is_active = False
    vjp = log.attempt("cavities", lambda: lx.grad.track_along_vjp(segment, beam, cavities=True))
    cotangent_calls(lx, log, vjp, segment, batch, bpm)
    log.attempt("wrt_particles", lambda: vjp(mu_x=1.0, wrt_particles=True))


def screens_case(shared):
    def run(lx, log):
        batch, dtype = (2,), np.float64
        rng = np.random.default_rng(24)
        f = lambda v: full(batch, v, dtype)  # noqa: E731
        mis = np.array([1e-5, -2e-5]) if shared else draw(rng, (*batch, 2)) * 1e-5
        first = lx.Screen(resolution=(5, 4), pixel_size=(1e-4, 1e-4), misalignment=mis, is_active=True, name="SCR_FIRST", dtype=dtype)
        last = lx.Screen(resolution=(3, 2), pixel_size=(1e-4, 1e-4), misalignment=np.array([0.0, 1e-5]) if shared else np.zeros((*batch, 2)), is_active=True,
                         name="SCR_LAST", dtype=dtype)
        idle = lx.Screen(resolution=(5, 4), pixel_size=(1e-4, 1e-4), is_active=False, name="SCR_IDLE", dtype=dtype)
        quad = lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="Q", dtype=dtype)
        segment = lx.Segment([first, lx.Drift(f(1.0), name="D", dtype=dtype), idle, quad, last])
        beam = parameter_beam(lx, batch, dtype)
        log.attempt("an active screen without screens", lambda: lx.grad.track_along_vjp(segment, beam))
        log.attempt("a ParticleBeam", lambda: lx.grad.track_along_vjp(segment, particle_beam(lx, batch, dtype), screens=True))
        vjp = log.attempt("screens", lambda: lx.grad.track_along_vjp(segment, beam, screens=True))
        w_first, w_last = draw(rng, (*batch, 5, 4)), draw(rng, (3, 2))
        for label, energy_bar in (("zero", np.zeros((*batch, 6))), ("non-zero", draw(rng, (*batch, 6)))):
            log.attempt(f"both screens, one by element, one by name; {label} energy_bar",
                        lambda: vjp(screen_images_bar={first: w_first, "SCR_LAST": w_last}, energy_bar=energy_bar, sigma_x=1.0), segment)
            log.attempt(f"one screen not named; {label} energy_bar", lambda: vjp(screen_images_bar={4: w_last, last: 2.0}, energy_bar=energy_bar), segment)
        log.attempt("no image cotangent", lambda: vjp(mu_bar=draw(rng, (*batch, 6, 7)), screen_images_bar={}), segment)
        log.events.append({"label": "the layout of the image cotangents", "value": vjp._image_cotangents({"SCR_FIRST": w_first, last: 0.5})})
        log.attempt("an idle screen", lambda: vjp(screen_images_bar={"SCR_IDLE": 1.0}))
        log.attempt("an idle screen, by element", lambda: vjp(screen_images_bar={idle: 1.0}))
        log.attempt("a shape that does not broadcast", lambda: vjp(screen_images_bar={first: np.ones((4, 5))}))
        log.attempt("no dict", lambda: vjp(screen_images_bar=np.ones((2, 5, 4))))
        both = log.attempt("screens and losses", lambda: lx.grad.track_along_vjp(segment, beam, screens=True, losses=True))
        log.attempt("with losses", lambda: both(screen_images_bar={last: 1.0}), segment)
    return run


case("track_along_vjp, screens, misalignment shared")(screens_case(True))
case("track_along_vjp, screens, misalignment per sample")(screens_case(False))


@case("track_along_vjp, ParticleBeam, (3,) float64")
def _(lx, log):
    batch, dtype = (3,), np.float64
    segment, bpm = mixed_lattice(lx, batch, dtype)
    beam = particle_beam(lx, batch, dtype)
    vjp = log.attempt("plain", lambda: lx.grad.track_along_vjp(segment, beam))
    cotangent_calls(lx, log, vjp, segment, batch, bpm)
    log.attempt("a cotangent 7 wide, broadcast", lambda: vjp(mu_bar=np.ones((6, 7)), cov_bar=np.ones((6, 7, 7))), segment)
    log.attempt("wrt_particles", lambda: vjp(mu_x=1.0, wrt_particles=True))
    log.attempt("screen_images_bar", lambda: vjp(screen_images_bar={}))
    log.attempt("trajectories_bar", lambda: vjp(trajectories_bar=np.ones(6)))
    without = log.attempt("losses, no aperture", lambda: lx.grad.track_along_vjp(segment, beam, losses=True))
    cotangent_calls(lx, log, without, segment, batch, bpm)


@case("track_along_vjp, ParticleBeam, (2, 2) float32")
def _(lx, log):
    batch, dtype = (2, 2), np.float32
    segment, bpm = mixed_lattice(lx, batch, dtype)
    for ddof in (0, 1):
        lx.config.std_ddof = ddof
        vjp = log.attempt("plain", lambda: lx.grad.track_along_vjp(segment, particle_beam(lx, batch, dtype)))
        cotangent_calls(lx, log, vjp, segment, batch, bpm)


def collimated(lx, batch, dtype, apertures=2):
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    elements = [lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="Q", dtype=dtype)]
    for k in range(apertures):
        elements += [lx.Aperture(x_max=f(1e-3), y_max=f(2e-3), is_active=True, name=f"COL{k}", dtype=dtype), lx.Drift(f(0.1), name=f"D{k}", dtype=dtype)]
    bpm = lx.BPM(is_active=True, name="BPM")
    return lx.Segment((elements[:3] + [bpm] + elements[3:])[:5 if apertures == 2 else None]), bpm  # (Q, COL0, D0, BPM, COL1)


@case("track_along_vjp, losses, two apertures, nobody left at two points", nobody=((1, 5), (2, 2), (2, 3), (2, 4), (2, 5)))
def _(lx, log):
    batch, dtype = (3,), np.float64
    segment, bpm = collimated(lx, batch, dtype)
    vjp = log.attempt("losses", lambda: lx.grad.track_along_vjp(segment, particle_beam(lx, batch, dtype), losses=True))
    rng = np.random.default_rng(25)
    alive = np.ones((*batch, 6))
    alive[1, 5], alive[2, 2:] = 0.0, 0.0
    mu_bar, cov_bar = draw(rng, (*batch, 6, 6)) * alive[..., None], draw(rng, (*batch, 6, 6, 6)) * alive[..., None, None]
    for label, energy_bar in (("zero", np.zeros((*batch, 6))), ("non-zero", draw(rng, (*batch, 6)))):
        log.attempt(f"zero on the points nobody reaches; {label} energy_bar",
                    lambda: vjp(mu_bar=mu_bar, cov_bar=cov_bar, energy_bar=energy_bar, readings={bpm: draw(rng, (2, *batch)) * alive[:, 3]}), segment)
        log.attempt(f"every property, zero there; {label} energy_bar",
                    lambda: vjp(energy_bar=energy_bar, **{name: draw(rng, (*batch, 6)) * alive for name in PROPERTIES}, energy=1.0), segment)
    log.attempt("a property there", lambda: vjp(sigma_x=1.0))
    log.attempt("a property there, last sample alone", lambda: vjp(beta_y=(1.0 - alive) * [[0], [0], [1]]))
    log.attempt("a reading there", lambda: vjp(readings={bpm: np.ones((2, *batch))}))
    log.attempt("mu_bar there", lambda: vjp(mu_bar=np.ones(6)))
    log.attempt("cov_bar there", lambda: vjp(cov_bar=np.ones((6, 6))))
    log.attempt("energy there", lambda: vjp(energy=1.0, energy_bar=np.ones((*batch, 6))), segment)
    log.attempt("wrt_particles", lambda: vjp(wrt_particles=True))


@case("track_along_vjp, losses, (2, 2) float32, everybody somewhere")
def _(lx, log):
    batch, dtype = (2, 2), np.float32
    segment, bpm = collimated(lx, batch, dtype)
    vjp = log.attempt("losses", lambda: lx.grad.track_along_vjp(segment, particle_beam(lx, batch, dtype), losses=True))
    cotangent_calls(lx, log, vjp, segment, batch, bpm)


@case("track_along_vjp, trajectories")
def _(lx, log):
    batch, dtype = (2,), np.float64
    segment, bpm = mixed_lattice(lx, batch, dtype)
    beam = particle_beam(lx, batch, dtype)
    rng = np.random.default_rng(26)
    vjp = log.attempt("trajectories", lambda: lx.grad.track_along_vjp(segment, beam, trajectories=[3, 0, 3]))
    wb = draw(rng, (*batch, 6, 3, 6))
    for label, energy_bar in (("zero", np.zeros((*batch, 6))), ("non-zero", draw(rng, (*batch, 6)))):
        log.attempt(f"without a moment cotangent; {label} energy_bar", lambda: vjp(trajectories_bar=wb, energy_bar=energy_bar), segment)
        log.attempt(f"with a moment cotangent; {label} energy_bar",
                    lambda: vjp(trajectories_bar=wb[..., :1, :], energy_bar=energy_bar, mu_bar=draw(rng, (*batch, 6, 6)), sigma_y=2.0,
                                readings={bpm: np.ones((2, *batch))}), segment)
    log.attempt("moments alone", lambda: vjp(cov_bar=draw(rng, (*batch, 6, 6, 6))), segment)
    log.attempt("energy alone", lambda: vjp(energy=1.0), segment)
    log.attempt("a shape that does not broadcast", lambda: vjp(trajectories_bar=np.ones((2, 6, 3, 5))))
    log.attempt("wrt_particles", lambda: vjp(trajectories_bar=wb, wrt_particles=True))
    log.attempt("a number of particles", lambda: lx.grad.track_along_vjp(segment, beam, trajectories=2)(trajectories_bar=np.ones(7)), segment)
    for label, selection in (("True", True), ("0", 0), ("beyond", 17), ("negative", [-1])):
        log.attempt(f"a bad selection: {label}", lambda: lx.grad.track_along_vjp(segment, beam, trajectories=selection))
    log.attempt("a ParameterBeam", lambda: lx.grad.track_along_vjp(segment, parameter_beam(lx, batch, dtype), trajectories=2))


def with_cavity(lx, batch, dtype):
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    bpm = lx.BPM(is_active=True, name="BPM")
    return lx.Segment([lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="Q", dtype=dtype),
                       lx.Cavity(f(1.0377), voltage=spread(batch, 1e7, 2e7, dtype), phase=f(3.0), frequency=f(1.3e9), name="CAV1", dtype=dtype), bpm,
                       lx.RBend(f(0.5), angle=spread(batch, 0.1, 0.2, dtype), name="RB", dtype=dtype)]), bpm


@case("track_along_vjp, cavities")
def _(lx, log):
    for batch, dtype in (((3,), np.float64), ((2, 2), np.float32)):
        segment, bpm = with_cavity(lx, batch, dtype)
        beam = particle_beam(lx, batch, dtype)
        log.attempt("without the switch", lambda: lx.grad.track_along_vjp(segment, beam))
        vjp = log.attempt("cavities", lambda: lx.grad.track_along_vjp(segment, beam, cavities=True))
        cotangent_calls(lx, log, vjp, segment, batch, bpm)
        cotangent_calls(lx, log, vjp, segment, batch, bpm, wrt_particles=True)
        log.attempt("trajectories_bar", lambda: vjp(trajectories_bar=np.ones(6)))
        chosen = log.attempt("a cavity and trajectories", lambda: lx.grad.track_along_vjp(segment, beam, trajectories=2))
        log.attempt("a moment cotangent", lambda: chosen(mu_bar=np.ones((*batch, 5, 6)), trajectories_bar=np.ones(6)))
        log.attempt("a property", lambda: chosen(beta_x=1.0))
        log.attempt("a reading", lambda: chosen(readings={bpm: np.ones((2, *batch))}))
        log.attempt("trajectories and energy", lambda: chosen(trajectories_bar=np.ones(7), energy_bar=np.ones((*batch, 5)), energy=1.0), segment)


@case("track_along_vjp, refusals of the constructor")
def _(lx, log):
    f = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    beam = particle_beam(lx, (1,), np.float32)
    segment, _ = collimated(lx, (1,), np.float32, 1)
    make = lx.grad.track_along_vjp
    log.attempt("no beam", lambda: make(segment, np.ones((1, 16, 7))))
    for name in ("losses", "screens", "cavities"):
        for bad in ("yes", 1, None):
            log.attempt(f"{name}={bad!r}", lambda: make(segment, beam, **{name: bad}))
    log.attempt("cavities and trajectories", lambda: make(segment, beam, trajectories=[0, 1], cavities=True))
    log.attempt("cavities and losses", lambda: make(segment, beam, losses=True, cavities=True))
    log.attempt("losses and trajectories", lambda: make(segment, beam, losses=True, trajectories=4))
    log.attempt("screens and a ParticleBeam", lambda: make(segment, beam, screens=True, trajectories=4))
    log.attempt("an active aperture", lambda: make(segment, beam))
    log.attempt("sixteen apertures", lambda: make(collimated(lx, (1,), np.float32, 16)[0], beam, losses=True))
    long = lx.Segment([*segment.elements, *[lx.Drift(f(0.1), name=f"T{k}") for k in range(254)]])
    log.attempt("257 leaves", lambda: make(long, beam, losses=True))
    cavity = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="ACC1")
    log.attempt("a cavity", lambda: make(lx.Segment([lx.Drift(f(1.0), name="D"), cavity]), beam))
    log.attempt("a cavity with losses", lambda: make(lx.Segment([*segment.elements, cavity]), beam, losses=True))
    nested = lx.Segment([lx.Segment([lx.Drift(f(0.1), name=f"D{k}") for k in range(60)]), cavity, lx.Segment([lx.Drift(f(0.1), name=f"T{k}") for k in range(4)])])
    log.attempt("65 leaves with cavities", lambda: make(nested, beam, cavities=True))
    log.attempt("an active screen", lambda: make(lx.Segment([cavity, lx.Screen(is_active=True, name="SCR7")]), beam, cavities=True))
    many = parameter_beam(lx, (65536,), np.float32)
    screen = lx.Screen(resolution=(5, 4), pixel_size=(1e-4, 1e-4), is_active=True, name="SCR")
    log.attempt("65536 samples with screens", lambda: make(lx.Segment([lx.Drift(f(1.0), name="D"), screen]), many, screens=True))


# ---- the cases of target_calls.npz: image targets, moment targets, forward mode ---------------------------------------------


def screened(lx, batch, dtype):
    """(segment, first, last, quad): SCR_FIRST (5 x 4 pixels), D, Q, SCR_LAST (3 x 2) -- both screens active."""
    pixels = dict(pixel_size=(1e-4, 1e-4), is_active=True, dtype=dtype)
    first = lx.Screen(resolution=(5, 4), misalignment=np.array([1e-5, -2e-5]), name="SCR_FIRST", **pixels)
    last = lx.Screen(resolution=(3, 2), misalignment=np.zeros((*batch, 2)), name="SCR_LAST", **pixels)
    quad = lx.Quadrupole(full(batch, 0.2, dtype), k1=spread(batch, 1, 2, dtype), name="Q", dtype=dtype)
    return lx.Segment([first, lx.Drift(full(batch, 1.0, dtype), name="D", dtype=dtype), quad, last]), first, last, quad


def image_targets_case(batch, dtype):
    def run(lx, log):
        rng = np.random.default_rng(31)
        make = lx.grad.track_along_vjp
        segment, first, last, quad = screened(lx, batch, dtype)
        beam = parameter_beam(lx, batch, dtype)
        t_first, t_last, per_sample = draw(rng, (5, 4)), draw(rng, (3, 2)), draw(rng, (*batch, 5, 4))
        log.attempt("no dict", lambda: make(segment, beam, image_targets=[t_last]))
        log.attempt("ImageTargets of no dict", lambda: lx.grad.ImageTargets([t_last]))
        log.attempt("an unknown key", lambda: make(segment, beam, image_targets={"NOPE": t_last}))
        log.attempt("the quadrupole as a key", lambda: make(segment, beam, image_targets={quad: t_last}))
        log.attempt("a target that does not fit", lambda: make(segment, beam, image_targets={first: t_last}))
        log.attempt("a per-sample target that does not fit", lambda: make(segment, beam, image_targets={last: np.ones((5, 3, 2))}))
        log.attempt("two targets for one screen", lambda: make(segment, beam, image_targets={first: t_first, "SCR_FIRST": t_first}))
        log.attempt("a ParticleBeam", lambda: make(segment, particle_beam(lx, batch, dtype), image_targets={last: t_last}))
        without = log.attempt("screens alone", lambda: make(segment, beam, screens=True))
        log.attempt("image_loss_bar without targets", lambda: without(image_loss_bar=1.0))
        log.value("image_loss without targets", lambda: without.image_loss)
        log.value("image_loss_of without targets", lambda: without.image_loss_of(last))
        # two active screens, one with a target shared by the batch
        vjp = log.attempt("one shared target", lambda: make(segment, beam, image_targets={last: t_last}))
        log.value("image_loss", lambda: vjp.image_loss)
        log.value("image_loss_of, by element", lambda: vjp.image_loss_of(last))
        log.value("image_loss_of, by point", lambda: vjp.image_loss_of(3))
        log.value("image_loss_of a point without a screen", lambda: vjp.image_loss_of(4))
        log.value("image_loss_of a screen without a target", lambda: vjp.image_loss_of("SCR_FIRST"))
        log.value("image_loss_of no screen", lambda: vjp.image_loss_of("Q"))
        log.attempt("a scalar bar", lambda: vjp(image_loss_bar=0.5), segment)
        log.attempt("a bar over the batch, beside a property", lambda: vjp(image_loss_bar=draw(rng, batch), beta_x=1.0))
        log.attempt("a dict of bars, one screen named twice", lambda: vjp(image_loss_bar={last: 2.0, "SCR_LAST": draw(rng, batch)}, energy_bar=draw(rng, (*batch, 5))))
        log.attempt("an empty dict of bars", lambda: vjp(image_loss_bar={}, mu_bar=draw(rng, (*batch, 5, 7))))
        log.attempt("no bar", lambda: vjp(sigma_x=1.0), segment)
        log.attempt("a bar of a screen without a target", lambda: vjp(image_loss_bar={first: 1.0}))
        log.attempt("a bar that does not broadcast", lambda: vjp(image_loss_bar=np.ones(5)))
        log.attempt("a bar in a dict that does not broadcast", lambda: vjp(image_loss_bar={last: np.ones((7, 2))}))
        log.attempt("screen_images_bar without screens", lambda: vjp(screen_images_bar={last: 1.0}))
        # a target per sample beside a shared one: a row per sample
        both = log.attempt("a target per sample", lambda: make(segment, beam, image_targets={"SCR_LAST": t_last, 0: per_sample}))
        log.value("image_loss of both", lambda: both.image_loss)
        log.attempt("a dict of bars for both", lambda: both(image_loss_bar={first: draw(rng, batch), 3: 0.25}), segment)
        # a dict is uploaded per pass, an ImageTargets once
        for _ in range(2):
            again = log.attempt("a dict again", lambda: make(segment, beam, image_targets={last: t_last}))
            log.attempt("its bar", lambda: again(image_loss_bar=1.0))
        targets = lx.grad.ImageTargets({first: t_first})
        for _ in range(2):
            again = log.attempt("the same ImageTargets", lambda: make(segment, beam, image_targets=targets))
            log.attempt("its bar", lambda: again(image_loss_bar=1.0))
        # with the images as well: both cotangents in one call
        images = log.attempt("screens and targets", lambda: make(segment, beam, screens=True, image_targets=targets, losses=True))
        log.attempt("both cotangents", lambda: images(screen_images_bar={last: draw(rng, (3, 2))}, image_loss_bar=draw(rng, batch), alpha_y=0.5), segment)
        log.events.append({"label": "the layout of the image cotangents", "value": images._image_cotangents({"SCR_LAST": 0.5})})
        first.is_active = last.is_active = False
        idle = log.attempt("targets and no active screen", lambda: make(segment, beam, image_targets={}))
        log.value("image_loss of no screen", lambda: idle.image_loss)
        log.attempt("a bar of no screen", lambda: idle(image_loss_bar=1.0, mu_x=1.0))
    return run


target_case("image targets, (2,) float64")(image_targets_case((2,), np.float64))
target_case("image targets, (2, 3) float32")(image_targets_case((2, 3), np.float32))


def matched(lx, batch, dtype, mode):
    """(segment, beam, keywords of track_along_vjp) of a mode: Q1, D1, M1, Q2, M2, with an aperture or a cavity where the mode needs one."""
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    elements = [lx.Quadrupole(f(0.2), k1=spread(batch, 1, 2, dtype), name="Q1", dtype=dtype), lx.Drift(f(0.5), name="D1", dtype=dtype), lx.Marker(name="M1"),
                lx.Quadrupole(f(0.2), k1=f(-1.5), name="Q2", dtype=dtype), lx.Marker(name="M2")]
    if mode == "survivors":
        elements.insert(3, lx.Aperture(x_max=f(1e-3), y_max=f(1e-3), is_active=True, name="COL", dtype=dtype))
    if mode in ("kicks", "behind a cavity"):
        elements[1] = lx.Cavity(f(1.0), voltage=f(1e7), phase=f(0.0), frequency=f(1.3e9), name="CAV", dtype=dtype)
    beam = parameter_beam(lx, batch, dtype) if mode == "moments" else particle_beam(lx, batch, dtype)
    keywords = {"trajectories": {"trajectories": [2, 0]}, "behind a cavity": {"trajectories": [2, 0]}, "survivors": {"losses": True}, "kicks": {"cavities": True}}
    return lx.Segment(elements), beam, keywords.get(mode, {})


def moment_targets_case(batch, dtype, mode):
    def run(lx, log):
        rng = np.random.default_rng(32)
        segment, beam, keywords = matched(lx, batch, dtype, mode)
        P = len(segment.elements) + 1
        per_sample = batch != (2,)  # (a target and a weight per sample: a row set per sample)
        targets = lx.grad.MomentTargets({"M1": {"beta_x": 4.0 + draw(rng, batch) if per_sample else 4.0, "beta_y": 2.0}, -1: {"sigma_x": 1e-4, "energy": 1e8, "normalized_emittance_y": 1e-6}},
                                        weights={"M1": {"beta_y": 0.5 + np.abs(draw(rng, batch[-1:])) if per_sample else 0.25}, P - 1: {"energy": 1e-12}})
        log.value("terms before a trace", lambda: targets.terms)
        for _ in range(2):  # the same object in two passes: its rows are uploaded once
            vjp = log.attempt("the targets", lambda: lx.grad.track_along_vjp(segment, beam, moment_targets=targets, **keywords))
        log.value("terms", lambda: [list(term) for term in targets.terms])
        log.value("the same terms", lambda: vjp._moment_targets.terms == targets.terms)
        log.value("moment_values", lambda: vjp.moment_values)
        log.value("moment_loss", lambda: vjp.moment_loss)
        log.value("moment_loss_of M1", lambda: vjp.moment_loss_of("M1"))
        log.value("moment_loss_of the last point", lambda: vjp.moment_loss_of(-1))
        log.value("moment_loss_of a point without a target", lambda: vjp.moment_loss_of(0))
        log.value("moment_loss_of no point", lambda: vjp.moment_loss_of("M7"))
        more = {"wrt_particles": True} if mode == "kicks" else {"trajectories_bar": draw(rng, (*batch, P, 2, 6))} if mode == "trajectories" else {}
        log.attempt("the bar alone, a scalar", lambda: vjp(moment_loss_bar=1.0), segment)
        log.attempt("the bar alone, over the batch", lambda: vjp(moment_loss_bar=draw(rng, batch), **more))
        log.attempt("beside mu_bar", lambda: vjp(moment_loss_bar=2.0, mu_bar=draw(rng, (*batch, P, 6)), **more), segment)
        log.attempt("beside a property", lambda: vjp(moment_loss_bar=draw(rng, batch), beta_x=draw(rng, (*batch, P))))
        log.attempt("beside energy_bar", lambda: vjp(moment_loss_bar=0.5, energy_bar=draw(rng, (*batch, P))))
        log.attempt("beside the energy as a property", lambda: vjp(moment_loss_bar=0.5, energy=1.0))
        log.attempt("no bar", lambda: vjp(sigma_y=1.0))
        log.attempt("a bar that does not broadcast", lambda: vjp(moment_loss_bar=np.ones(5)))
        # terms of the energy alone, from a dict: no moment cotangent comes of them
        energies = log.attempt("energy alone", lambda: lx.grad.track_along_vjp(segment, beam, moment_targets={"M2": {"energy": 1.1e8}, 1: {"energy": 1e8}}, **keywords))
        log.value("its values", lambda: energies.moment_values)
        log.attempt("its bar", lambda: energies(moment_loss_bar=1.0), segment)
        log.attempt("its bar beside a property", lambda: energies(moment_loss_bar=1.0, sigma_x=draw(rng, (*batch, P))))
    return run


for _mode in ("moments", "particles", "trajectories", "survivors", "kicks"):
    target_case(f"moment targets, {_mode}, (2,) float32")(moment_targets_case((2,), np.float32, _mode))
target_case("moment targets, moments, (2, 3) float64")(moment_targets_case((2, 3), np.float64, "moments"))
target_case("moment targets, particles, (2, 3) float64")(moment_targets_case((2, 3), np.float64, "particles"))


@target_case("moment targets, refusals and the three together")
def _(lx, log):
    batch, dtype = (2,), np.float64
    make, Targets = lx.grad.track_along_vjp, lx.grad.MomentTargets
    segment, beam, _ = matched(lx, batch, dtype, "moments")
    log.attempt("no dict", lambda: make(segment, beam, moment_targets=[1.0]))
    log.attempt("MomentTargets of no dict", lambda: Targets([("M1", "beta_x", 1.0)]))
    log.attempt("a point without a dict", lambda: Targets({"M1": 1.0}))
    log.attempt("weights of no dict", lambda: Targets({"M1": {"beta_x": 1.0}}, weights=[1.0]))
    log.attempt("no target", lambda: Targets({"M1": {}}))
    log.attempt("an unknown property", lambda: make(segment, beam, moment_targets={"M1": {"beta_z": 1.0}}))
    log.attempt("an unknown property of a weight", lambda: Targets({"M1": {"beta_x": 1.0}}, weights={"M1": {"gamma": 1.0}}))
    log.attempt("a weight without a target", lambda: make(segment, beam, moment_targets=Targets({"M1": {"beta_x": 1.0}}, weights={"M2": {"beta_x": 1.0}})))
    log.attempt("a doubled target", lambda: make(segment, beam, moment_targets={"M1": {"beta_x": 1.0}, 3: {"beta_x": 2.0}}))
    log.attempt("a doubled weight", lambda: make(segment, beam, moment_targets=Targets({"M1": {"beta_x": 1.0}}, weights={"M1": {"beta_x": 1.0}, -3: {"beta_x": 2.0}})))
    log.attempt("a target that does not broadcast", lambda: make(segment, beam, moment_targets={"M1": {"beta_x": np.ones(3)}}))
    log.attempt("a weight that does not broadcast", lambda: make(segment, beam, moment_targets=Targets({"M1": {"beta_x": 1.0}}, weights={"M1": {"beta_x": np.ones((2, 2))}})))
    log.attempt("no such element", lambda: make(segment, beam, moment_targets={"M7": {"beta_x": 1.0}}))
    log.attempt("no such point", lambda: make(segment, beam, moment_targets={6: {"beta_x": 1.0}}))
    plain = log.attempt("no targets", lambda: make(segment, beam))
    log.attempt("moment_loss_bar without targets", lambda: plain(moment_loss_bar=1.0))
    for name in ("moment_values", "moment_loss"):
        log.value(f"{name} without targets", lambda: getattr(plain, name))
    log.value("moment_loss_of without targets", lambda: plain.moment_loss_of("M1"))
    # a ParticleBeam behind an active cavity: a moment's target is refused where its cotangent is, the energy's is not
    behind, particles, keywords = matched(lx, batch, dtype, "behind a cavity")
    log.attempt("a target behind a cavity", lambda: make(behind, particles, moment_targets={"M1": {"beta_x": 1.0}}))
    log.attempt("a target behind a cavity, with trajectories", lambda: make(behind, particles, moment_targets={-1: {"energy": 1.1e8, "beta_x": 1.0}}, **keywords))
    chosen = log.attempt("the energy behind a cavity, with trajectories", lambda: make(behind, particles, moment_targets={-1: {"energy": 1.1e8}}, **keywords))
    log.attempt("its bar alone", lambda: chosen(moment_loss_bar=1.0), behind)
    log.attempt("its bar beside the trajectories'", lambda: chosen(moment_loss_bar=1.0, trajectories_bar=np.ones(6)), behind)
    log.attempt("a property behind the cavity", lambda: chosen(moment_loss_bar=1.0, beta_x=1.0))
    # image targets, images and moment targets in one call
    rng = np.random.default_rng(33)
    screens, first, last, quad = screened(lx, batch, dtype)
    three = log.attempt("all three", lambda: make(screens, beam, screens=True, image_targets={last: draw(rng, (3, 2))}, moment_targets={"Q": {"beta_x": 3.0}}))
    log.attempt("all three bars", lambda: three(screen_images_bar={first: 1.0}, image_loss_bar=1.0, moment_loss_bar=1.0), screens)
    log.attempt("all three bars and a property", lambda: three(screen_images_bar={first: 1.0}, image_loss_bar=1.0, moment_loss_bar=1.0, alpha_x=draw(rng, (*batch, 5))))


@target_case("moment targets, losses, nobody left at a point", nobody=((1, 5), (1, 6)))
def _(lx, log):
    batch, dtype = (2,), np.float64
    segment, beam, keywords = matched(lx, batch, dtype, "survivors")
    make = lx.grad.track_along_vjp
    log.attempt("a target where nobody is", lambda: make(segment, beam, moment_targets={5: {"sigma_x": 1e-4}}, **keywords))
    log.attempt("a target where nobody is, behind one that is fine", lambda: make(segment, beam, moment_targets={2: {"mu_x": 0.0}, "M2": {"alpha_y": 0.0}}, **keywords))
    vjp = log.attempt("the energy there and a moment in front", lambda: make(segment, beam, moment_targets={5: {"energy": 1e8}, 4: {"sigma_x": 1e-4}}, **keywords))
    log.value("moment_values", lambda: vjp.moment_values)
    log.attempt("the bar", lambda: vjp(moment_loss_bar=np.array([1.0, -0.5])), segment)
    w = np.zeros((*batch, 7))
    w[1, 5] = 1.0
    log.attempt("a cotangent where nobody is", lambda: vjp(moment_loss_bar=1.0, sigma_x=w))


def forward_lattice(lx, batch, dtype):
    """(segment, quad, bend, bpm, corrector): Q, RB, BPM, HC, Q again, VC -- the quadrupole object placed twice."""
    f = lambda v: full(batch, v, dtype)  # noqa: E731
    mixed, bpm = mixed_lattice(lx, batch, dtype, bpm_active=False)
    _, quad, bend, _, corrector = mixed.elements
    return lx.Segment([quad, bend, bpm, corrector, quad, lx.VerticalCorrector(f(0.1), angle=f(1e-4), name="VC", dtype=dtype)]), quad, bend, bpm, corrector


def handed_out_forward(lx, log, jvp, bpm):
    for name in ("mu_dot", "cov_dot", "energy_dot"):
        log.value(name, lambda: getattr(jvp, name))
    for name in ("beta_x", "normalized_emittance_y", "energy", "sigma_p", "gamma"):
        log.value(f"the tangent of {name}", lambda: jvp.tangent(name))
    log.value("the tangents of a reading", lambda: jvp.reading_tangents(bpm))
    log.value("the tangents of no element's reading", lambda: jvp.reading_tangents(lx.BPM(name="OTHER")))


def forward_case(batch, dtype, particles):
    def run(lx, log):
        segment, quad, bend, bpm, corrector = forward_lattice(lx, batch, dtype)
        beam = particle_beam(lx, batch, dtype) if particles else parameter_beam(lx, batch, dtype)
        make, matrix = lx.grad.track_along_jvp, lx.grad.orbit_response_matrix
        wrt = [(quad, "k1"), (bend, "angle"), (quad, "misalignment", 1), "energy", (corrector, "angle")]
        jvp = log.attempt("five directions", lambda: make(segment, beam, wrt))
        handed_out_forward(lx, log, jvp, bpm)
        # `cavities=True` on a lattice without an active cavity is the plain call, for both beam classes
        same = log.attempt("cavities=True without a cavity", lambda: make(segment, beam, [(quad, "misalignment", 0), "energy"], cavities=True))
        log.value("energy_dot", lambda: same.energy_dot)
        log.value("the tangent of energy", lambda: same.tangent("energy"))

        def response(**given):
            found = matrix(segment, beam, **given)
            return {"matrix": found.matrix, "bpms": [el.name for el in found.bpms], "correctors": [el.name for el in found.correctors],
                    "directions": len(found.jvp.wrt)}

        log.value("the response matrix", response)
        log.value("the response matrix of given lists", lambda: response(bpms=[bpm, bpm], correctors=[segment.VC]))
        log.value("the response matrix, cavities=True", lambda: response(cavities=True))
        # every refusal of `wrt`
        other = lx.Drift(full(batch, 1.0, dtype), name="OTHER", dtype=dtype)
        for label, bad in (("empty", []), ("a string", ["k1"]), ("no tuple", [quad]), ("four items", [(quad, "k1", 0, 1)]), ("no name", [(quad, 1)]),
                           ("not of the lattice", [(other, "length")]), ("a vector without a component", [(quad, "misalignment")]),
                           ("a vector with component 2", [(quad, "misalignment", 2)]), ("a scalar with a component", [(quad, "k1", 0)]),
                           ("no such parameter", [(bend, "k1")]), ("a BPM's parameter", [(bpm, "angle")]), ("no such parameter, with a component", [(bend, "k7", 0)])):
            log.attempt(f"wrt: {label}", lambda: make(segment, beam, bad))
        log.attempt("no beam", lambda: make(segment, None, wrt))
        for bad in ("yes", 1, None):
            log.attempt(f"cavities={bad!r}", lambda: make(segment, beam, wrt, cavities=bad))
        drift = lx.Drift(full(batch, 1.0, dtype), name="D", dtype=dtype)
        log.attempt("an active screen", lambda: make(lx.Segment([drift, lx.Screen(is_active=True, name="SCR7")]), beam, [(drift, "length")]))
        aperture = lx.Aperture(x_max=full(batch, 1e-3, dtype), y_max=full(batch, 1e-3, dtype), is_active=True, name="AP1", dtype=dtype)
        log.attempt("an active aperture", lambda: make(lx.Segment([drift, aperture]), beam, [(drift, "length")], cavities=True))
        log.attempt("the response matrix without a BPM", lambda: matrix(lx.Segment([drift, corrector]), beam))
        log.attempt("the response matrix without a corrector", lambda: matrix(lx.Segment([drift, bpm]), beam))
        log.attempt("the response matrix of no lists", lambda: matrix(segment, beam, bpms=[], correctors=[]))
        log.attempt("the response matrix of another BPM", lambda: matrix(segment, beam, bpms=[lx.BPM(name="OTHER")]))
        log.attempt("the response matrix of another corrector", lambda: matrix(segment, beam, correctors=[lx.HorizontalCorrector(full(batch, 0.1, dtype), name="HC9", dtype=dtype)]))
    return run


target_case("forward mode, ParameterBeam, (2,) float64")(forward_case((2,), np.float64, False))
target_case("forward mode, ParticleBeam, (2, 3) float32")(forward_case((2, 3), np.float32, True))


@target_case("forward mode, cavities")
def _(lx, log):
    batch, dtype = (2,), np.float64
    segment, bpm = with_cavity(lx, batch, dtype)  # (Q, CAV1, BPM, RB)
    cavity, quad, bend = segment.CAV1, segment.Q, segment.RB
    idle = lx.Cavity(full(batch, 1.0, dtype), voltage=full(batch, 0.0, dtype), phase=full(batch, 0.0, dtype), frequency=full(batch, 1.3e9, dtype), name="IDLE", dtype=dtype)
    corrector = lx.HorizontalCorrector(full(batch, 0.1, dtype), angle=full(batch, 1e-4, dtype), name="HC", dtype=dtype)
    segment = lx.Segment([corrector, *segment.elements, idle])
    beam, particles = parameter_beam(lx, batch, dtype), particle_beam(lx, batch, dtype)
    make = lx.grad.track_along_jvp
    wrt = [(cavity, "voltage"), (quad, "k1"), (cavity, "phase"), "energy", (cavity, "frequency"), (cavity, "length"), (bend, "angle"), (idle, "length")]
    log.attempt("without the switch", lambda: make(segment, beam, wrt[1:2]))
    log.attempt("without the switch, a ParticleBeam", lambda: make(segment, particles, wrt[1:2]))
    log.attempt("a ParticleBeam", lambda: make(segment, particles, wrt[1:2], cavities=True))
    log.attempt("the voltage of a cavity without any", lambda: make(segment, beam, [(idle, "voltage")], cavities=True))
    cavity.voltage = full(batch, 0.0, dtype)
    log.attempt("the voltage of a cavity switched off, without the switch", lambda: make(segment, beam, [(cavity, "phase")]))
    cavity.voltage = spread(batch, 1e7, 2e7, dtype)
    jvp = log.attempt("through the cavity", lambda: make(segment, beam, wrt, cavities=True))
    handed_out_forward(lx, log, jvp, bpm)
    found = log.attempt("the response matrix", lambda: lx.grad.orbit_response_matrix(segment, beam, cavities=True))
    log.value("its matrix", lambda: found.matrix)
    log.value("its energy_dot", lambda: found.jvp.energy_dot)
    log.attempt("the response matrix without the switch", lambda: lx.grad.orbit_response_matrix(segment, beam))


# ---- the file ---------------------------------------------------------------------------------------------------------


def flatten(tree, arrays):
    """`tree` with every array replaced by {"array": its index in `arrays`} -- what JSON holds; equal arrays share an index."""
    if isinstance(tree, dict):
        return {str(key): flatten(value, arrays) for key, value in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [flatten(value, arrays) for value in tree]
    if isinstance(tree, (np.ndarray, np.generic)):
        value = np.ascontiguousarray(tree)
        for k, have in enumerate(arrays):
            if have.dtype == value.dtype and have.shape == value.shape and have.tobytes() == value.tobytes():
                return {"array": k}
        arrays.append(value)
        return {"array": len(arrays) - 1}
    assert tree is None or isinstance(tree, (bool, int, float, str)), type(tree)
    return tree


def save(path, index, arrays):
    """One JSON index and one block of bytes: a zip member per small array would cost more than the array."""
    layout = [[a.dtype.str, list(a.shape)] for a in arrays]
    np.savez_compressed(path, index=np.frombuffer(json.dumps({"cases": index, "arrays": layout}).encode(), dtype=np.uint8),
                        bytes=np.frombuffer(b"".join(a.tobytes() for a in arrays), dtype=np.uint8))


def load(path):
    """(index per case, arrays) as `flatten` made them."""
    with np.load(path) as file:
        held, block = json.loads(file["index"].tobytes().decode()), file["bytes"].tobytes()
    arrays, first = [], 0
    for dtype, shape in held["arrays"]:
        count = int(np.prod(shape, dtype=np.int64))
        arrays.append(np.frombuffer(block, dtype=dtype, count=count, offset=first).reshape(shape))
        first += count * np.dtype(dtype).itemsize
    return held["cases"], arrays


if __name__ == "__main__":
    import sys

    files = {"reverse": (PATH, CASES), "targets": (TARGET_PATH, TARGET_CASES)}
    if sys.argv[1:] not in (["reverse"], ["targets"]):
        sys.exit("usage: python -m tests.golden.make_reverse_calls reverse | targets")
    path, cases = files[sys.argv[1]]
    arrays = []
    index = {name: flatten(transcript(name), arrays) for name in cases}
    save(path, index, arrays)
    calls = sum(len(entry["calls"]) for entry in index.values())
    print(f"{len(cases)} cases, {calls} library calls, {len(arrays)} arrays, {path.stat().st_size} bytes")
