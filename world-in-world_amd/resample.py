"""PIL-exact 8-bit image resampling: the coefficient tables of Pillow's `ImagingResample` and a numpy restatement of its
two passes (no torch: the tables are built on the host for the kernels of csrc/resample.hip, and the restatement is what
their tests compare against).

`Image.resize` of an 8-bit image is integer arithmetic on uint8 with a fixed-point table (libImaging/Resample.c):

  * `precompute_coeffs`: per output index the window [xmin, xmin + n) of input samples and n normalised filter weights,
    computed in doubles;
  * `normalize_coeffs_8bpc`: weights -> int32, scaled by 2**22 (PRECISION_BITS) and rounded half away from zero by a C cast;
  * one pass per axis, horizontal first: out = clip8((2**21 + sum pixel * coeff) >> 22), the intermediate image is uint8;
    a pass whose side does not change is skipped (`need_horizontal` / `need_vertical`) — NOT run with its filter.

Everything below follows those functions operation for operation in Python floats (C doubles), so that the integer tables —
and with them every output byte — are Pillow's own.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # Resample.c: 8 bits for the result, 2 for the filter's overshoot, the rest is precision
MAX_TAPS = 64                        # the kernels' cap on ksize (include/wiw_resample.h); Lanczos-3 down to 1/10 of a side


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def table_ksize(in_size: int, out_size: int, filter: str) -> int:
    """Taps per output sample (the row length of `pil_tables(...)[0]`) without building the table."""
    filterscale = max(in_size / out_size, 1.0)
    return int(math.ceil(FILTERS[filter][1] * filterscale)) * 2 + 1


def supported(in_size: int, out_size: int, filter: str) -> bool:
    """Whether the kernels take this side: equal sides need no table; otherwise at most MAX_TAPS taps."""
    return in_size == out_size or (in_size > 0 and out_size > 0 and table_ksize(in_size, out_size, filter) <= MAX_TAPS)


@lru_cache(maxsize=64)
def pil_tables(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (coeffs int32 (out_size, ksize), bounds int32 (out_size, 2) = [xmin, n]) of one axis, as Pillow builds them
    (`precompute_coeffs` + `normalize_coeffs_8bpc`).  Cached per geometry; the arrays are read-only."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    if in_size <= 0 or out_size <= 0:
        raise ValueError("pil_tables: sizes must be positive")
    fn, fsupport = FILTERS[filter]
    filterscale = scale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)          # a C cast: truncation toward zero
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        for x, w in enumerate(k):
            coeffs[xx, x] = int(-0.5 + w * one) if w < 0 else int(0.5 + w * one)
        bounds[xx] = (xmin, n)
    coeffs.setflags(write=False)
    bounds.setflags(write=False)
    return coeffs, bounds


def _pass_last_axis(planes: np.ndarray, out_size: int, filter: str) -> np.ndarray:
    """One pass along the LAST axis of uint8 (..., in_size) -> uint8 (..., out_size)."""
    coeffs, bounds = pil_tables(planes.shape[-1], out_size, filter)
    in_size = planes.shape[-1]
    acc = np.full(planes.shape[:-1] + (out_size,), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for k in range(coeffs.shape[1]):
        live = bounds[:, 1] > k
        if not live.any():
            break
        idx = np.minimum(bounds[:, 0] + k, in_size - 1)          # taps past n carry a zero coefficient
        acc += planes[..., idx].astype(np.int64) * np.where(live, coeffs[:, k], 0).astype(np.int64)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)          # >> on a signed array is arithmetic


def resample_reference(planes: np.ndarray, out_w: int, out_h: int, filter: str) -> np.ndarray:
    """`Image.resize((out_w, out_h), filter)` of every plane of uint8 (N, H, W) -> uint8 (N, out_h, out_w): horizontal pass,
    uint8 intermediate, vertical pass; a pass whose side does not change is skipped."""
    planes = np.asarray(planes)
    if planes.dtype != np.uint8 or planes.ndim != 3:
        raise ValueError("resample_reference: uint8 (N, H, W) planes")
    _, H, W = planes.shape
    out = planes
    if out_w != W:
        out = _pass_last_axis(out, out_w, filter)
    if out_h != H:
        out = np.swapaxes(_pass_last_axis(np.swapaxes(out, 1, 2), out_h, filter), 1, 2)
    return np.ascontiguousarray(out)


def u8_to_unit_range_lut() -> np.ndarray:
    """fp32[256]: byte u -> 2 * (u / 255) - 1, by the numpy expression of `server.plumbing.preprocess_image` itself."""
    x = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    return 2.0 * x - 1.0
