"""Shared inputs and references of the frame-metric tests (tests/test_metrics.py, tests/test_hip_metrics*.py).

  * the loader of tests/golden/video_metrics.npz (tools/make_golden_metrics.py: the reference's own `ssim`, `img_psnr`,
    `calculate_ssim`, `calculate_psnr` on the stored planes), read once and never modified;
  * an fp64 numpy restatement of the two per-plane numbers with the separable window, for inputs the fixture does not hold
    (strided launches, the trainer's quantised frames).  tests/test_metrics.py holds it to the fixture.

Tolerances, each from the reference's functions and none from the kernel: per-plane SSIM 1e-10 absolute (an fp64 separable
evaluation is within 1.4e-13 of the reference's 2-D float64 result, fp32 arithmetic 2e-8 .. 5e-5 off, the exact u / 255 in place
of the float32 quotient 1e-9 .. 6e-9 off); PSNR 1e-5 dB (the reference squares and averages in float32: within 1e-7 dB of the
exact value on the shapes tried, rounding bound 6e-6 dB at 576 x 1024); the aggregates the same on `value` and `value_std`.
"""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_metrics.npz")
SSIM_TOL, PSNR_TOL = 1e-10, 1e-5
PAIRS = ["noise_11x11", "noise_12x75", "smooth_pm6_45x70", "const200_one201_64x96", "near_saturated_37x131", "smooth_96x160",
         "row_11x300", "column_300x11", "mixed_150x333", "generic_f32_40x52", "identical_33x47"]
LUT = np.arange(256, dtype=np.float32) / np.float32(255)          # the reference's to_tensor value of a byte
LUT.setflags(write=False)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for v in g.values():
        v.setflags(write=False)
    return g


def pair(name):
    """(a, b, ssim, psnr) of a fixture pair: the stored planes (uint8, or float32 for the generic pair) and the reference's numbers."""
    g = golden()
    return g[f"{name}__a"], g[f"{name}__b"], float(g[f"{name}__ssim"]), float(g[f"{name}__psnr"])


def as_f32(x):
    """The float32 plane the reference sees: a uint8 plane through the table, a float32 plane as it is."""
    return LUT[x] if x.dtype == np.uint8 else x


@functools.lru_cache(maxsize=None)
def window():
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return k / k.sum()


def _valid(x):
    """The 11 x 11 Gaussian mean of x (float64) on the windows inside the plane: rows, then columns."""
    k, (H, W) = window(), x.shape
    rows = sum(k[j] * x[:, j:W - 10 + j] for j in range(11))
    return sum(k[j] * rows[j:H - 10 + j] for j in range(11))


def plane_metrics(a, b):
    """(mean SSIM over the valid region, sum of squared differences) of one plane pair, float64 after the load."""
    x, y = as_f32(a).astype(np.float64), as_f32(b).astype(np.float64)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = _valid(x), _valid(y)
    s11, s22, s12 = _valid(x * x) - mu1 * mu1, _valid(y * y) - mu2 * mu2, _valid(x * y) - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return float(ssim_map.mean()), float(((x - y) ** 2).sum())


def psnr_of(sse, count):
    """calculate_psnr.py `img_psnr` from a summed squared error over `count` samples."""
    mse = sse / count
    return 100.0 if mse < 1e-10 else 20 * math.log10(1 / math.sqrt(mse))


def planes_metrics(a, b):
    """(N, 2) float64 of stacked planes (N, H, W)."""
    return np.array([plane_metrics(p, q) for p, q in zip(a, b)], np.float64).reshape(-1, 2)


def frame_scores(gt, gen):
    """ssim (B, T), psnr (B, T) of (B, T, 3, H, W) arrays through the restatement."""
    B, T, Cc, H, W = gt.shape
    m = planes_metrics(gt.reshape(-1, H, W), gen.reshape(-1, H, W)).reshape(B, T, Cc, 2)
    ssim = m[..., 0].mean(-1)
    psnr = np.array([[psnr_of(m[v, t, :, 1].sum(), Cc * H * W) for t in range(T)] for v in range(B)])
    return ssim, psnr
