"""
A transcript of every reverse call `lynx_amd/grad.py` makes, without a GPU: per case the keyword arguments given to
`engine.track_along`, every library call with every argument by value (tests/reverse_host_fakes.py), everything
`Gradients` hands out, and for a refusal the exception's type and text.  Only the public API of `lynx_amd.grad` is used,
so the script runs unchanged on any commit's `grad.py`:

    python -m tests.golden.make_reverse_calls        # writes tests/golden/reverse_calls.npz

tests/test_reverse_calls_host.py replays `CASES` and compares with that file byte for byte.  The file is made on the
commit BEFORE a change to `grad.py`, never with the code under test.
"""

import json
from pathlib import Path

import numpy as np
import pytest

from tests.reverse_host_fakes import FakeArray, fake_gpu

PATH = Path(__file__).resolve().parent / "reverse_calls.npz"
PROPERTIES = ("mu_x", "mu_xp", "mu_y", "mu_yp", "mu_s", "mu_p", "sigma_x", "sigma_xp", "sigma_y", "sigma_yp", "sigma_s",
              "sigma_p", "sigma_xxp", "sigma_yyp", "emittance_x", "emittance_y", "normalized_emittance_x",
              "normalized_emittance_y", "beta_x", "beta_y", "alpha_x", "alpha_y")  # tests/test_trace_grad_host.py
BEAM_PROPERTIES = ("mu_y", "sigma_x", "sigma_p", "sigma_xxp", "sigma_yyp")
CASES = {}


def case(name, **fake):
    def register(fn):
        CASES[name] = (fn, fake)
        return fn
    return register


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


def transcript(name):
    """The transcript of one case as a tree of dicts, lists, scalars and arrays."""
    import lynx_amd as lx

    fn, fake = CASES[name]
    log = Log()
    ddof = lx.config.std_ddof
    with pytest.MonkeyPatch.context() as monkeypatch:
        rt, forward = fake_gpu(monkeypatch, **fake)
        try:
            fn(lx, log)
        finally:
            lx.config.std_ddof = ddof
    return {"forward": list(forward), "calls": [{"entry": entry, "arguments": args} for entry, args in rt.lib.records], "events": log.events}


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
    arrays = []
    index = {name: flatten(transcript(name), arrays) for name in CASES}
    save(PATH, index, arrays)
    calls = sum(len(entry["calls"]) for entry in index.values())
    print(f"{len(CASES)} cases, {calls} library calls, {len(arrays)} arrays, {PATH.stat().st_size} bytes")
