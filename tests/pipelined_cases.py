"""
The call sequences of tests/test_gpu_pipelined.py and tests/test_pipelined_host.py: the lattices, the values written
before every call, and the thresholds of the launch plan that decide which path a shape takes.

Every sequence is K calls on ONE Segment.  Before call j the k1 of one quadrupole is written with per-sample values
v_j (the `short` lattice: a corrector's angle too, and a tilt switched on at j = 4 and off at j = 6), so that no two
consecutive calls compute the same thing: a kernel that read a neighbour's step table, record buffer or energy gives
another answer (test_pipelined_host.py holds the oracle to that).
"""

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# the plan's thresholds, each with the line of lynx_amd/csrc/lynx_hip.hip that sets it (test_pipelined_host.py checks
# that the quoted text is still there)
# ---------------------------------------------------------------------------------------------------------------------

HALF_MILLION = 512 * 1024          # track_table: second stream, side reduction, short calls from here on
LONG_KERNEL_BYTES = 128 << 20      # track_table: below it a call without a cavity is a "short call"; from it the host waits for the build
ALTERNATE_BYTES = 256 << 20        # track_particles_t: every other launch of this size walks the batch backwards
TABLE_SLOTS = 3                    # lynx_ctx::kTableSlots
PARTIAL_RING = 4                   # lynx_ctx::kPartialRing
LANES_BUILD_MIN_BATCH = 256        # Knobs::lanes_build_min_batch
REDUCE_STAGE = 70                  # lynx_device.hpp kReduceStage: more rows per sample go through a second level
INLINE_POOL_BYTES = 1024           # lynx_device.hpp kInlinePoolLarge: a pool up to this travels in the kernel arguments

SOURCE_LINES = {
    "HALF_MILLION": ("lynx_hip.hip", "const bool half_million = B * N >= (int64_t)512 << 10;"),
    "HALF_MILLION (side reduction)": ("lynx_hip.hip", "knob(ctx->knobs.side_reduce, (B * N >= (int64_t)512 << 10 && !t.short_call) ? 1 : 0)"),
    "LONG_KERNEL_BYTES (short call)": ("lynx_hip.hip", "t->short_call = half_million && (size_t)B * N * 7 * sizeof(T) < ((size_t)128 << 20) && !lat->has_cavity;"),
    "LONG_KERNEL_BYTES (host wait)": ("lynx_hip.hip", "const bool long_kernel = (size_t)B * N * 7 * sizeof(T) >= ((size_t)128 << 20);"),
    "ALTERNATE_BYTES": ("lynx_hip.hip", "(ctx->knobs.alternate_order == 2 || (size_t)B * N * 7 * sizeof(T) >= ((size_t)256 << 20)))"),
    "TABLE_SLOTS": ("lynx_hip.hip", "static constexpr int kTableSlots = 3;"),
    "PARTIAL_RING": ("lynx_hip.hip", "static constexpr int kPartialRing = 4;"),
    "LANES_BUILD_MIN_BATCH": ("lynx_hip.hip", "int lanes_build_min_batch = 256;"),
    "REDUCE_STAGE": ("lynx_device.hpp", "constexpr int kReduceStage = 70;"),
    "INLINE_POOL_BYTES": ("lynx_device.hpp", "constexpr int kInlinePoolSmall = 256, kInlinePoolLarge = 1024;"),
}

PARAMS_OF_KIND = {"drift": 1, "quadrupole": 5, "hcor": 2, "cavity": 4, "bpm": 0}  # lynx_hip.hip params_of_kind
SIGMA = [1e-4, 1e-5, 1e-4, 1e-5, 1e-5, 1e-3]  # the incoming beams (bench.BEAM_SIGMA)
ORACLE_BUDGET = 3e7  # particle-element steps of the oracle per case up to which every sample's moments are checked

# id: dtype, B, N, calls, incoming energy
CASES = {
    "short": dict(dtype=np.float64, B=4, N=140_001, K=9, energy=1e8),
    "long": dict(dtype=np.float32, B=320, N=15_001, K=9, energy=1e8),
    "cavity": dict(dtype=np.float32, B=320, N=15_001, K=9, energy=6e6),
    "order": dict(dtype=np.float32, B=64, N=150_001, K=6, energy=1e8),
    "small": dict(dtype=np.float32, B=5, N=6151, K=9, energy=6e6),  # the cavity lattice, for the forced forms
}
LATTICE_OF = {"short": "short", "long": "fodo", "cavity": "cavity", "order": "fodo", "small": "cavity"}


def particle_bytes(case):
    c = CASES[case]
    return c["B"] * c["N"] * 7 * np.dtype(c["dtype"]).itemsize


def lattice(kind, B, seed=11):
    """(description, element index of the written quadrupole, of the written corrector or None, of the active BPM or None)."""
    rng = np.random.default_rng([seed, B])
    f = lambda v: np.full(B, v)  # noqa: E731
    if kind == "short":  # 3 x [drift, quad, hcor, drift] + one active BPM
        desc = []
        for _ in range(3):
            desc += [("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-4, 4, B))),
                     ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, B))), ("drift", dict(length=f(0.4)))]
        desc.insert(8, ("bpm", dict(is_active=True)))
        return desc, 1, 2, 8
    if kind == "fodo":  # 16-element FODO, k1 per sample, no misalignment
        k = 4.2 * (0.5 + np.arange(B) / max(B - 1, 1))
        desc = []
        for _ in range(4):
            desc += [("quadrupole", dict(length=f(0.2), k1=k)), ("drift", dict(length=f(0.5))),
                     ("quadrupole", dict(length=f(0.2), k1=-k)), ("drift", dict(length=f(0.5)))]
        return desc, 0, None, None
    if kind == "parameter":  # 3 x [drift, quad, hcor, drift] + a cavity: the 13 elements a ParameterBeam goes through
        desc = []
        for _ in range(3):
            desc += [("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.2), k1=rng.uniform(-4, 4, B))),
                     ("hcor", dict(length=f(0.1), angle=rng.normal(0, 1e-4, B))), ("drift", dict(length=f(0.4)))]
        desc.append(("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9))))
        return desc, 1, 2, None
    assert kind == "cavity"  # 8 x [drift, quad, drift, cavity]
    desc = []
    for _ in range(8):
        desc += [("drift", dict(length=f(0.3))), ("quadrupole", dict(length=f(0.1), k1=rng.uniform(-5, 5, B))),
                 ("drift", dict(length=f(0.3))),
                 ("cavity", dict(length=f(1.0377), voltage=rng.uniform(5e6, 2e7, B), phase=rng.uniform(-10, 10, B), frequency=f(1.3e9)))]
    return desc, 1, None, None


def written_values(B, K, seed=5):
    """
    (K, B) values of k1: the sign alternates from call to call, the magnitudes are K distinct levels in [1.2, 4.2] in a
    drawn order, each sample's scaled by its own factor in [1, 1.19] -- consecutive calls differ by more than 2 in every
    sample, and no two calls of a sample are equal.
    """
    rng = np.random.default_rng([seed, B, K])
    levels = rng.permutation(np.linspace(1.2, 4.2, K))
    factor = 1.0 + 0.19 * rng.random(B)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    return (sign * levels)[:, None] * factor[None, :]


def writes(case):
    """Per call j: the list of (element index, attribute, (B,) float64 value) written before it."""
    c = CASES[case]
    B, K = c["B"], c["K"]
    kind = LATTICE_OF[case]
    _, quad, hcor, _ = lattice(kind, B)
    v = written_values(B, K)
    rng = np.random.default_rng([7, B, K])
    angles = rng.uniform(1e-4, 5e-4, (K, B)) * np.where(np.arange(K) % 2 == 0, -1.0, 1.0)[:, None]
    tilt = rng.uniform(0.1, 0.5, B)
    out = []
    for j in range(K):
        w = [(quad, "k1", v[j])]
        if hcor is not None:
            w.append((hcor, "angle", angles[j]))
        if kind == "short" and j == 4:
            w.append((quad, "tilt", tilt))
        if kind == "short" and j == 6:
            w.append((quad, "tilt", np.zeros(B)))
        out.append(w)
    return out


def described(case):
    """The lattice of `case` as it stands at every call: a list of K descriptions (the writes accumulate)."""
    c = CASES[case]
    desc, *_ = lattice(LATTICE_OF[case], c["B"])
    out = []
    for w in writes(case):
        desc = list(desc)
        for e, name, value in w:
            kind, kw = desc[e]
            desc[e] = (kind, {**kw, name: value})
        out.append(desc)
    return out


def subset(desc, pick, dtype):
    """The description cut to the samples `pick`, every value rounded to `dtype` as the product's elements hold it."""
    out = []
    for kind, kw in desc:
        out.append((kind, {k: (np.asarray(np.asarray(v, dtype=dtype)[pick], dtype=dtype) if isinstance(v, np.ndarray) else v)
                           for k, v in kw.items()}))
    return out


def oracle_steps(case):
    c = CASES[case]
    return c["B"] * c["N"] * len(lattice(LATTICE_OF[case], c["B"])[0]) * c["K"]


# several entry points on one context (test_several_entry_points_share_one_context)
ENTRY_SHAPES = {
    "S": dict(lattice="short", dtype=np.float64, B=4, N=140_001, energy=1e8),    # a short call with an observer step
    "C": dict(lattice="cavity", dtype=np.float32, B=320, N=2000, energy=6e6),    # lanes build and cavity flags on s_build
    "P": dict(lattice="parameter", dtype=np.float32, B=300, N=None, energy=1e8),  # a ParameterBeam's lanes path
}
ENTRY_OPS = [("track", "S"), ("track", "C"), ("parameter", "P"), ("along", "S"), ("vjp", "C"), ("track", "S"),
             ("parameter", "P"), ("along", "P"), ("vjp", "S"), ("track", "C"), ("along", "C"), ("parameter", "P"),
             ("track", "C"), ("vjp", "C")]
ENTRY_ORDER_SEED = 20261019
ENTRY_PARAMETER_SIGMA = dict(sigma_x=1e-4, sigma_xp=1e-5, mu_x=1e-4)  # the ParameterBeam (the rest: from_parameters' defaults)


def entry_order():
    return [ENTRY_OPS[i] for i in np.random.default_rng(ENTRY_ORDER_SEED).permutation(len(ENTRY_OPS))]
