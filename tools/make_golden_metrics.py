#!/usr/bin/env python
"""Generate tests/golden/video_metrics.npz: the REFERENCE's frame metrics (evaluation/FVD/calculate_ssim.py `ssim`,
`calculate_ssim`; evaluation/FVD/calculate_psnr.py `img_psnr`, `calculate_psnr`) on a set of plane pairs and one small video
pair — build container only; the reference is imported at run time (its root: oracle/_ref_import.py `REF_ROOT`).

SUBSTITUTED PRIMITIVES.  The reference's `ssim` calls two OpenCV functions and `cv2` is not installed in the build container, so
this script registers a stand-in module named `cv2` with exactly those two, and everything else is the reference's own code:

  * `getGaussianKernel(n, sigma)`: the (n, 1) float64 column k[i] = exp(-(i - (n - 1) / 2)^2 / (2 sigma^2)) / sum — OpenCV's
    formula for a kernel that is not one of its small fixed tables (n = 11 is not);
  * `filter2D(img, -1, k)`: `scipy.ndimage.correlate(img, k, mode="mirror")` — a correlation, float64 in and out, with OpenCV's
    default border BORDER_REFLECT_101 (`mirror` is scipy's name for it).  The reference crops the result by [5:-5, 5:-5], which
    removes every pixel the border mode touches.

`cal_4metrics.evaluate_video_metrics` itself is not imported (it pulls in the LPIPS / FVD networks); its SSIM and PSNR entries
are `calculate_ssim(gt, gen, only_final)` and `calculate_psnr(gt, gen, only_final)` on the concatenated clips, which is what is
recorded here for both values of the flag.

Content (loader: tests/metrics_fixtures.py): per pair `<name>__a`, `<name>__b` (uint8 planes u, standing for the float32 value
float32(u) / float32(255) of the reference's to_tensor; float32 for the one pair that is not uint8-derived), `<name>__ssim`
(float64, `ssim(a, b)`) and `<name>__psnr` (`img_psnr(a, b)`); the video pair `video__gt`, `video__gen` (uint8 (2, 3, 3, 16, 20)),
its per-frame `video__ssim`, `video__psnr` (2, 3) and `video__<metric>__{final,frames}__{value,std}`.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_metrics.py
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np  # noqa: E402

NAME = "video_metrics.npz"


def cv2_stand_in():
    import scipy.ndimage

    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(n, sigma):
        i = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        k = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (k / k.sum()).reshape(n, 1)

    def filter2D(img, ddepth, kernel):
        assert ddepth == -1 and img.dtype == np.float64
        return scipy.ndimage.correlate(img, kernel, mode="mirror")

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    return cv2


def to_unit(u):
    """uint8 -> the float32 of torchvision's to_tensor: float32(u) / float32(255)."""
    return u.astype(np.float32) / np.float32(255)


def smooth(rs, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fy, fx, ph = rs.uniform(0.02, 0.09, 2), rs.uniform(0.02, 0.09, 2), rs.uniform(0, 6.28, 2)
    return 127.5 + 60.0 * np.sin(fy[0] * y + fx[0] * x + ph[0]) + 50.0 * np.cos(fy[1] * y - fx[1] * x + ph[1])


def u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def plane_pairs():
    """name -> (a, b): uint8 planes, except `generic_f32` (float32 in [0, 1], not a multiple of 1/255)."""
    rs = np.random.RandomState(20261019)
    P = {}

    def noise(H, W):
        return rs.randint(0, 256, size=(H, W)).astype(np.uint8)

    P["noise_11x11"] = (noise(11, 11), noise(11, 11))                      # one valid pixel
    P["noise_12x75"] = (noise(12, 75), noise(12, 75))
    s = smooth(rs, 45, 70)
    P["smooth_pm6_45x70"] = (u8(s), u8(s + rs.randint(-6, 7, size=s.shape)))
    a = np.full((64, 96), 200, np.uint8)
    b = a.copy()
    b[31, 47] = 201
    P["const200_one201_64x96"] = (a, b)
    P["near_saturated_37x131"] = (rs.randint(250, 252, size=(37, 131)).astype(np.uint8),
                                  rs.randint(250, 252, size=(37, 131)).astype(np.uint8))
    s = smooth(rs, 96, 160)
    P["smooth_96x160"] = (u8(s), u8(s * 0.93 + 9.0 + 3.0 * np.sin(np.arange(160) * 0.4)[None, :]))
    s = smooth(rs, 11, 300)
    P["row_11x300"] = (u8(s + rs.randint(-20, 21, size=s.shape)), u8(s))                      # one valid row
    s = smooth(rs, 300, 11)
    P["column_300x11"] = (u8(s), u8(s + rs.randint(-20, 21, size=s.shape)))                   # one valid column
    s = smooth(rs, 150, 333)
    P["mixed_150x333"] = (u8(s + rs.randint(-12, 13, size=s.shape)), u8(0.8 * s + 30.0 + rs.randint(-12, 13, size=s.shape)))
    g = (smooth(rs, 40, 52) / 255.0).clip(0, 1)
    P["generic_f32_40x52"] = ((g + rs.uniform(-0.03, 0.03, g.shape)).clip(0, 1).astype(np.float32),
                              (g * 0.9 + rs.uniform(0.0, 0.08, g.shape)).clip(0, 1).astype(np.float32))
    s = u8(smooth(rs, 33, 47) + rs.randint(-30, 31, size=(33, 47)))
    P["identical_33x47"] = (s, s.copy())
    return P


def video_pair():
    rs = np.random.RandomState(7)
    gt = np.stack([np.stack([np.stack([u8(smooth(rs, 16, 20) + rs.randint(-10, 11, size=(16, 20))) for _ in range(3)])
                             for _ in range(3)]) for _ in range(2)])
    gen = u8(gt.astype(np.float64) * rs.uniform(0.7, 1.0, size=(2, 3, 1, 1, 1)) + rs.randint(-25, 26, size=gt.shape))
    return gt, gen


def main():
    import scipy
    import torch

    from _ref_import import REF_ROOT

    sys.dont_write_bytecode = True          # the reference tree is read-only
    assert "cv2" not in sys.modules
    sys.modules["cv2"] = cv2_stand_in()
    sys.path.insert(0, REF_ROOT)
    from evaluation.FVD.calculate_psnr import calculate_psnr, img_psnr  # type: ignore  (reference)
    from evaluation.FVD.calculate_ssim import calculate_ssim, ssim  # type: ignore  (reference)

    out = {}
    for name, (a, b) in plane_pairs().items():
        fa, fb = (a, b) if a.dtype == np.float32 else (to_unit(a), to_unit(b))
        out[f"{name}__a"], out[f"{name}__b"] = a, b
        out[f"{name}__ssim"] = np.array(ssim(fa, fb), np.float64)
        out[f"{name}__psnr"] = np.array(img_psnr(fa, fb), np.float64)
        print(f"{name:28s} {a.dtype}  ssim {float(out[f'{name}__ssim']):+.15f}  psnr {float(out[f'{name}__psnr']):.9f}")
    gt, gen = video_pair()
    tg, tn = torch.from_numpy(to_unit(gt)), torch.from_numpy(to_unit(gen))
    out["video__gt"], out["video__gen"] = gt, gen
    from evaluation.FVD.calculate_ssim import calculate_ssim_function  # type: ignore  (reference)

    out["video__ssim"] = np.array([[calculate_ssim_function(tg[v, t].numpy(), tn[v, t].numpy()) for t in range(3)] for v in range(2)])
    out["video__psnr"] = np.array([[img_psnr(tg[v, t].numpy(), tn[v, t].numpy()) for t in range(3)] for v in range(2)], np.float64)
    for metric, fn in (("ssim", calculate_ssim), ("psnr", calculate_psnr)):
        for tag, flag in (("final", True), ("frames", False)):
            r = fn(tg, tn, only_final=flag)
            out[f"video__{metric}__{tag}__value"] = np.array(r["value"], np.float64)
            out[f"video__{metric}__{tag}__std"] = np.array(r["value_std"], np.float64)
            print(metric, tag, r)
    versions = dict(numpy=np.__version__, scipy=scipy.__version__, torch=torch.__version__)
    path = os.path.join(ROOT, "tests", "golden", NAME)
    np.savez_compressed(path, _versions=np.array(repr(versions)), **out)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB)")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
