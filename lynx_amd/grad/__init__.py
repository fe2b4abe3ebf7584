"""
Gradients of the beam with respect to element parameters, the incoming energy and the incoming beam (SURVEY.md section 8f-1;
BASELINE config 5).  The reference only claims differentiability (`setup.py:14-17`; its tests still assert torch `grad_fn`,
`tests/test_differentiable.py`) -- there is no `jax.grad` call to mirror, so the API is explicit products with the Jacobian,
four entry functions:

    vjp = lynx_amd.grad.track_vjp(segment, beam)           # reverse mode of `segment.track`: forward pass, fused moments
    out = vjp.outgoing                                      # the tracked beam
    g = vjp(mu_bar=..., cov_bar=...)                        # cotangents of mean (.., 6) and cov (.., 6, 6)
    g = vjp(mu_x=..., sigma_x=..., sigma_y=...)             # or of the beam properties a loss is written in
    g[segment.Q1]["k1"], g.energy                           # dL/dk1 (shape of k1), dL/dE_in

    vjp = lynx_amd.grad.track_along_vjp(segment, beam)      # reverse mode of `segment.track_along`: the trace is `vjp.trace`
    g = vjp(beta_x=w_x, beta_y=w_y)                         # cotangents (*batch, P) at EVERY point of the lattice
    # ... with `trajectories=`, `losses=True`, `screens=True`, `cavities=True`, and the two losses formed on the device:
    vjp = lynx_amd.grad.track_along_vjp(segment, beam, moment_targets=lynx_amd.grad.MomentTargets({"M1": {"beta_x": 4.0}}))
    vjp.moment_loss, vjp(moment_loss_bar=1.0)               # (`image_targets=lynx_amd.grad.ImageTargets(...)` alike)

    jvp = lynx_amd.grad.track_along_jvp(segment, beam, [(segment.Q3, "k1"), "energy"])    # forward mode: few parameters,
    jvp.mu_dot, jvp.cov_dot, jvp.tangent("beta_x")                                        # every output

    orm = lynx_amd.grad.orbit_response_matrix(segment, beam)   # d(reading of every BPM)/d(angle of every corrector): `orm.matrix`

All arithmetic runs in the HIP kernels of `lynx_amd/csrc` (`lynx_grad.hpp`, `lynx_trace_grad.hpp`, `lynx_trace_jvp.hpp`,
`lynx_moment_loss.hpp`, ...).  The package, module by module, each importing only from those above it:

    gradients.py    what a reverse pass hands back: `Gradients`, `ChainedGradients`
    cotangents.py   the property rules and the assembly of cotangents on the host; pure NumPy
    track.py        `track_vjp` for both beam classes
    targets.py      `ImageTargets`, `MomentTargets` and the two losses formed from them on the device
    along.py        `track_along_vjp` and its five modes
    jvp.py          `track_along_jvp`, `orbit_response_matrix`

`import lynx_amd` does not import this package.

`lynx_amd.grad.get_runtime`, the name the old module had and callers replaced to stand in for the GPU, is kept as a property
of the package: it reads and replaces `device.get_runtime`, the one place the package asks.
"""

import sys
import types

from .. import device
from .along import MAX_TRACE_CAVITY_LEAVES, MAX_TRACE_LEAVES, MAX_TRACE_LOSS_APERTURES, TrackAlongVJP, track_along_vjp  # noqa: F401
from .cotangents import (MOMENT_PROPERTIES, _record_cotangents, _walk_properties, property_cotangents,  # noqa: F401
                         trace_property_cotangents)
from .gradients import DIFFERENTIABLE_KINDS, ChainedGradients, Gradients, _unbroadcast  # noqa: F401
from .jvp import ENERGY_ROW, OrbitResponseMatrix, TrackAlongJVP, _jvp_directions, orbit_response_matrix, track_along_jvp  # noqa: F401
from .targets import ImageTargets, MomentTargets  # noqa: F401
from .track import MomentsVJP, TrackVJP, track_vjp  # noqa: F401


class _Package(types.ModuleType):
    get_runtime = property(lambda package: device.get_runtime, lambda package, value: setattr(device, "get_runtime", value))


sys.modules[__name__].__class__ = _Package
