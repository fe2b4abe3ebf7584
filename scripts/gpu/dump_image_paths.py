"""
Every kernel of the screen images along a ParameterBeam's trace once on the inputs of their own tests
(tests/test_gpu_trace_image_loss.py `loss_case`, tests/test_gpu_trace_screens_grad.py `kernel_case`: every screen of
`LOSS_SCREENS` and the screen of 65 chunks, both dtypes, a batch of 3), and a lattice of 65 one-pixel screens (two launches of
the image loss's reverse half): the images, the loss, the six sums, mu_bar, cov_bar and the misalignments' gradients, written
to DIR/<case>.npz.  Two builds of the library (LYNX_HIP_LIBRARY picks one) are compared array by array, bit for bit.

    python scripts/gpu/dump_image_paths.py DIR
    python scripts/gpu/dump_image_paths.py --compare DIR_A DIR_B
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def compare(dir_a, dir_b):
    names, differing = sorted(p.name for p in Path(dir_a).glob("*.npz")), []
    assert names and names == sorted(p.name for p in Path(dir_b).glob("*.npz")), "the two directories hold different cases"
    arrays = 0
    for name in names:
        a, b = np.load(Path(dir_a) / name), np.load(Path(dir_b) / name)
        assert sorted(a.files) == sorted(b.files), name
        arrays += len(a.files)
        differing += [f"{name}:{key}" for key in a.files if not np.array_equal(a[key], b[key], equal_nan=True)]
    print(f"{len(names)} cases, {arrays} arrays, {len(differing)} differ" + "".join(f"\n  {d}" for d in differing))
    return 1 if differing else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

import lynx_amd as lx  # noqa: E402
import lynx_amd.grad as grad  # noqa: E402
from tests import image_loss_reference as il  # noqa: E402
from tests import screen_grad_reference as ref  # noqa: E402
from tests.test_gpu_trace_image_loss import loss_case  # noqa: E402
from tests.test_gpu_trace_screens_grad import kernel_case  # noqa: E402

out_dir = Path(sys.argv[1])
out_dir.mkdir(parents=True, exist_ok=True)
lx.device.get_runtime()
il.LOSS_SCREENS["3x43691"] = ref.SCREEN_OF_65_CHUNKS
ref.KERNEL_SCREENS.update(il.LOSS_SCREENS)  # (`kernel_case` looks its screens up there)


def save(case, **arrays):
    assert all(np.asarray(v).size for v in arrays.values()), case
    np.savez(out_dir / f"{case}.npz", **{k: np.asarray(v) for k, v in arrays.items()})


def gradients(g, screens):
    return dict(mu_bar=g.mu, cov_bar=g.cov, **{f"grad_misalignment_{k}": g[screen]["misalignment"] for k, screen in enumerate(screens)})


for dtype in (np.float32, np.float64):
    name = np.dtype(dtype).name
    for label in il.LOSS_SCREENS:
        segment, beam, screen, _, given, _ = loss_case(lx, label, dtype, (3,), False, False)
        vjp = grad.track_along_vjp(segment, beam, image_targets={screen: given})
        save(f"loss {label} {name}", images=segment.track_along(beam, screens=True).image_at("SCREEN"), loss=vjp.image_loss_of(screen),
             sums=vjp._image_loss.sums.numpy(), **gradients(vjp(image_loss_bar=np.array([1.0, -0.5, 2.0])), [screen]))
        vjp, screen, W, _ = kernel_case(lx, label, dtype, (3,), False)
        save(f"gradients {label} {name}", **gradients(vjp(screen_images_bar={screen: W}), [screen]))
    # 65 screens of one pixel behind a drift each; every third one without a target
    rng = np.random.default_rng(65)
    full = lambda v: np.full((3,), v, dtype=dtype)  # noqa: E731
    screens = [lx.Screen(resolution=(1, 1), pixel_size=(2.0 ** -14, 2.0 ** -14), binning=1, misalignment=(1e-5 * rng.standard_normal((3, 2))).astype(dtype),
                         is_active=True, name=f"S{k}", dtype=dtype) for k in range(65)]
    segment = lx.Segment([el for screen in screens for el in (lx.Drift(full(0.05), dtype=dtype), screen)])
    beam = lx.ParameterBeam.from_parameters(mu_x=full(2e-5), mu_y=full(-1e-5), sigma_x=full(1.2e-4), sigma_xp=full(1e-5), sigma_y=full(1e-4),
                                            sigma_yp=full(1e-5), sigma_s=full(1e-5), sigma_p=full(1e-3), energy=full(1e8), dtype=dtype)
    named = [screen for k, screen in enumerate(screens) if k % 3 != 1 or k == 64]
    vjp = grad.track_along_vjp(segment, beam, image_targets={screen: rng.uniform(1e6, 1e7, (3, 1, 1)).astype(dtype) for screen in named})
    bars = {screen: rng.uniform(0.5, 2.0, 3) for screen in named}
    save(f"65 screens {name}", loss=np.stack([vjp.image_loss_of(screen) for screen in named]), sums=vjp._image_loss.sums.numpy(),
         **gradients(vjp(image_loss_bar=bars), screens))
print(f"{len(list(out_dir.glob('*.npz')))} cases written to {out_dir}")
