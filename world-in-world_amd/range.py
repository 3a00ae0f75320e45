"""Value-range statistics of tensors: the numpy restatement of `wiw_range_stats` (include/wiw_range.h), the reader of the
kernel's result buffers, and the range probe that records them per activation tensor of a forward.

  * `reference_stats` — what the kernel computes, restated with numpy's own predicates (isnan / isinf / frexp on float64): the
    reference of tests/test_hip_range.py, and what the serving guard uses when it is handed host arrays;
  * `stats_records`   — the device buffers of `Hip.range_stats` -> the same records (copies them to the host: call it after
    the synchronisation the caller needs anyway);
  * `RangeProbe`      — set as `Hip.range_probe`: the operators called by `UNetHIP.forward`, `VAEHIP` and `CLIPVisionHIP` then
    record the statistics of the activation tensor they wrote, under the module path of the scope they run in.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
from typing import List, Optional

import numpy as np

BINS = 64          # WIW_RANGE_BINS: bin = clamp(floor(log2 |x|) + 32, 0, 63) over finite non-zero x
FIELDS = ("n_nan", "n_inf", "n_zero", "n_hot", "n_tiny", "absmax", "absmin")
# (largest finite value, smallest normal) of the storage types
_LIMITS = {"float16": (65504.0, 2.0 ** -14), "bfloat16": (float.fromhex("0x1.fep127"), 2.0 ** -126),
           "float32": (float(np.finfo(np.float32).max), 2.0 ** -126)}


def _dtype_name(dtype) -> str:
    name = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    if name not in _LIMITS:
        raise ValueError(f"range statistics are defined for float16, bfloat16 and float32, not {dtype}")
    return name


def finite_max(dtype) -> float:
    """Largest finite value of a storage type (torch or numpy dtype, or its name)."""
    return _LIMITS[_dtype_name(dtype)][0]


def thresholds(dtype):
    """(hot, tiny) of a storage type: half its largest finite value, and its smallest normal."""
    mx, tiny = _LIMITS[_dtype_name(dtype)]
    return float(np.float32(mx / 2.0)), tiny


def reference_stats(array, rows_per_segment: Optional[int] = None, hot: Optional[float] = None, tiny: Optional[float] = None,
                    hist: bool = True, dtype=None) -> List[dict]:
    """Per-segment statistics of a (rows, cols) array (a 1-D array is one row) of float16 / float32 values — bfloat16 values
    come as the float32 they convert to, with dtype="bfloat16" for the default thresholds: one record per group of
    rows_per_segment rows (default: all rows), each {n_nan, n_inf, n_zero, n_hot, n_tiny: int, absmax, absmin: float,
    hist: uint64 [64] or None} as include/wiw_range.h defines them."""
    if hasattr(array, "detach"):          # a host torch tensor
        array = array.detach().float().numpy() if "bfloat16" in str(array.dtype) else array.detach().numpy()
    a = np.asarray(array)
    d_hot, d_tiny = thresholds(dtype if dtype is not None else a.dtype)
    hot, tiny = d_hot if hot is None else hot, d_tiny if tiny is None else tiny
    if not (np.isfinite(hot) and hot >= 0 and np.isfinite(tiny) and tiny >= 0):
        raise ValueError("hot and tiny must be finite and not negative")
    a = a.reshape(1, -1) if a.ndim < 2 else a.reshape(a.shape[0], -1)
    rows = a.shape[0]
    rps = rows if rows_per_segment is None else int(rows_per_segment)
    if rows <= 0 or a.shape[1] <= 0 or rps <= 0 or rows % rps:
        raise ValueError(f"rows {rows}, cols {a.shape[1]}, rows_per_segment {rps}")
    out = []
    for s in range(rows // rps):
        with np.errstate(invalid="ignore"):          # widening a signalling NaN raises the flag
            x = np.abs(a[s * rps:(s + 1) * rps].astype(np.float64).ravel())          # exact for every storage type
        nan, inf = np.isnan(x), np.isinf(x)
        fin = x[~(nan | inf)]
        nz = fin[fin > 0]
        rec = {"n_nan": int(nan.sum()), "n_inf": int(inf.sum()), "n_zero": int((fin == 0).sum()),
               "n_hot": int((fin >= hot).sum()), "n_tiny": int((nz < tiny).sum()),
               "absmax": float(fin.max()) if fin.size else 0.0, "absmin": float(nz.min()) if nz.size else float("inf"), "hist": None}
        if hist:
            e = np.frexp(nz)[1].astype(np.int64) - 1          # |x| = m * 2^e', m in [0.5, 1): floor(log2 |x|) = e' - 1
            rec["hist"] = np.bincount(np.clip(e + 32, 0, BINS - 1), minlength=BINS).astype(np.uint64)
        out.append(rec)
    return out


class _Stats(C.Structure):          # WiwRangeStats
    _fields_ = [(n, C.c_uint64) for n in FIELDS[:5]] + [(n, C.c_float) for n in FIELDS[5:]]


_STATS_DTYPE = np.dtype([(n, np.uint64) for n in FIELDS[:5]] + [(n, np.float32) for n in FIELDS[5:]])
assert _STATS_DTYPE.itemsize == C.sizeof(_Stats) == 48


def stats_records(stats, hist=None) -> List[dict]:
    """The buffers `Hip.range_stats` returned -> records as `reference_stats` gives them.  Copies to the host."""
    raw = np.ascontiguousarray(stats.cpu().numpy() if hasattr(stats, "cpu") else stats).view(np.uint8).reshape(-1, 48)
    st = raw.view(_STATS_DTYPE).reshape(-1)
    bins = None
    if hist is not None:
        bins = np.ascontiguousarray(hist.cpu().numpy() if hasattr(hist, "cpu") else hist).view(np.uint64).reshape(-1, BINS)
    out = []
    for s, r in enumerate(st):
        rec = {n: int(r[n]) for n in FIELDS[:5]}
        rec["absmax"], rec["absmin"] = float(r["absmax"]), float(r["absmin"])
        rec["hist"] = bins[s].copy() if bins is not None else None
        out.append(rec)
    return out


def non_finite(rec: dict) -> int:
    return rec["n_nan"] + rec["n_inf"]


def scoped(root: Optional[str] = None):
    """Method decorator of the model classes (they hold their `Hip` as `self.hip`): with a probe attached the body runs under
    the scope `root`, or under the module path the method receives as its first argument; without one it just runs."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(self, *args, **kw):
            probe = self.hip.range_probe
            if probe is None:
                return fn(self, *args, **kw)
            with probe.scope(root if root is not None else (args[0] if args else kw["p"])):
                return fn(self, *args, **kw)
        return wrapper
    return deco


class RangeProbe:
    """Collects `wiw_range_stats` of the activation tensors a forward writes.  Attach with `hip.range_probe = probe`, run the
    forward EAGERLY (a probe set while a graph is being captured raises: its buffers would be read before any replay), then
    `probe.records()` once at the end — the only point that waits for the device.  The probed forward launches every kernel it
    launches without the probe, with the same arguments: its outputs are bit-identical."""

    def __init__(self):
        self._scope: List[str] = []
        self._pending = []                # (scope, family, ordinal, shape, dtype name, stats buffer, hist buffer)
        self._ordinals = {}
        self.entry_points = set()         # C entry points whose output was recorded (tests: the coverage rule)

    @contextlib.contextmanager
    def scope(self, path: str):
        """The module path (`mid_block.resnets.0`, ...) the operators inside run under."""
        self._scope.append(path)
        try:
            yield self
        finally:
            self._scope.pop()

    @property
    def current_scope(self) -> str:
        return self._scope[-1] if self._scope else ""

    def record(self, hip, family: str, t, *, rows=None, cols=None, ld=None, entry: Optional[str] = None) -> None:
        """Launch the statistics of `t` (the tensor an operator of `family` just wrote) on the operator's stream."""
        import torch
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("range probe: set while a graph is being captured; probe an eager forward "
                               "(SVDDenoiser(use_graph=False), --no-hip_graph)")
        if not self._scope:          # an operator called from outside the probed forwards (the Euler step, a test)
            return
        if entry is not None:
            self.entry_points.add(entry)
        scope = self.current_scope
        k = self._ordinals.get(scope, 0)
        self._ordinals[scope] = k + 1
        stats, hist = hip.range_stats(t, rows, cols, ld, hist=True)
        shape = tuple(t.shape) if rows is None else (int(rows), int(cols))
        self._pending.append((scope, family, k, shape, str(t.dtype).replace("torch.", ""), stats, hist))

    def records(self) -> List[dict]:
        """Every record so far, in launch order: {scope, family, ordinal, shape, dtype, headroom} + the statistics.
        headroom = largest finite value of the storage type / absmax: inf for a tensor without a non-zero finite element, and 0
        for one that holds an inf (it went past the largest finite value)."""
        out = []
        for scope, family, k, shape, dtype, stats, hist in self._pending:
            rec = stats_records(stats, hist)[0]
            headroom = 0.0 if rec["n_inf"] else finite_max(dtype) / rec["absmax"] if rec["absmax"] > 0 else float("inf")
            rec.update(scope=scope, family=family, ordinal=k, shape=shape, dtype=dtype, headroom=headroom)
            out.append(rec)
        return out
