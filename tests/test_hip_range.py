"""`wiw_range_stats` (csrc/range.hip) against `range.reference_stats` on the GPU, both libraries, the 16-bit type and fp32:
every count, absmax, absmin and all 64 bins EQUAL (the statistics are exact: counts, a max and a min of exactly converted
values), on the shapes at which the kernel takes another path — one element; a few; strided rows with NaN in the padding;
several segments; rows longer than a chunk at an odd leading dimension from an element-aligned base (scalar heads and tails);
many blocks per segment — with the special values at the first and last element, around chunk (4096) and block (8 chunks)
boundaries and in the tail.  Also: two runs give the same bytes, and a segment computed alone equals itself among four."""
import functools
import zlib

import numpy as np
import pytest
import torch

import wiw_amd  # noqa: F401
from wiw_amd.range import reference_stats, stats_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CHUNK, BLOCK = 4096, 8 * 4096          # elements of a unit / of a block's units in csrc/range.hip

# (rows, cols, ld, segments, element offset of the base)
SHAPES = {
    "1x1": (1, 1, 1, 1, 0),
    "3x5": (3, 5, 5, 1, 0),
    "257x320-ld384": (257, 320, 384, 1, 0),
    "64x1000-4seg": (64, 1000, 1000, 4, 0),
    "2x70001-odd-ld": (2, 70001, 70003, 1, 1),
    "2x70001-2seg": (2, 70001, 70003, 2, 3),
    "4096x1280": (4096, 1280, 1280, 1, 0),
    "96x700-ld701-4seg": (96, 700, 701, 4, 0),
}
#            qNaN    sNaN    -NaN    +inf    -inf    +0      -0      min sub  max sub  min nrm (tiny)  max finite  -hot
SPECIAL = {
    "fp16": [0x7e00, 0x7c01, 0xffff, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0x7bff, 0xf7ff],
    "bf16": [0x7fc0, 0x7f81, 0xffff, 0x7f80, 0xff80, 0x0000, 0x8000, 0x0001, 0x007f, 0x0080, 0x7f7f, 0xfeff],
    "f32": [0x7fc00000, 0x7f800001, 0xffffffff, 0x7f800000, 0xff800000, 0x0, 0x80000000, 0x1, 0x007fffff, 0x00800000, 0x7f7fffff,
            0xfeffffff],
}
_HIPS = {}


def hip_of(name):
    from wiw_amd.hip import Hip

    if name not in _HIPS:
        _HIPS[name] = Hip(torch.device(DEV), DTYPES[name])
    return _HIPS[name]


def to_float(bits, kind):
    if kind == "fp16":
        return bits.view(np.float16)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> (bit patterns [rows][ld] with NaN in the padding, reference records); made once per shape and element type."""
    rows, cols, ld, segments, _ = SHAPES[shape]
    rs = np.random.RandomState(zlib.crc32(f"{shape} {kind}".encode()))
    word = np.uint32 if kind == "f32" else np.uint16
    nbits = 32 if kind == "f32" else 16
    x = rs.randint(0, 1 << nbits, size=(rows, cols), dtype=np.uint64).astype(word)          # every pattern: NaNs, infs, subnormals
    ordinary = rs.rand(rows, cols) < 0.5                                                     # and half of them of moderate size
    one = {"fp16": 0x3c00, "bf16": 0x3f80, "f32": 0x3f800000}[kind]
    mant = {"fp16": 10, "bf16": 7, "f32": 23}[kind]
    mod = (one + (rs.randint(-12, 13, size=(rows, cols)) << mant) + rs.randint(0, 1 << mant, size=(rows, cols))).astype(word)
    mod |= (rs.randint(0, 2, size=(rows, cols)) << (nbits - 1)).astype(word)
    x = np.where(ordinary, mod, x)
    flat = x.reshape(-1)
    spots = [0, flat.size - 1]
    for edge in (CHUNK, BLOCK, 2 * BLOCK, cols, (rows // segments) * cols):
        spots += [edge - 1, edge, edge + 1]
    spots += list(range(max(flat.size - 9, 0), flat.size))                                   # the scalar tail
    special = SPECIAL[kind]
    for k, i in enumerate(dict.fromkeys(i for i in spots if 0 <= i < flat.size)):
        flat[i] = special[k % len(special)]
    full = np.full((rows, ld), {"f32": 0x7fc00000}.get(kind, 0x7fff), dtype=word)            # NaN in both 16-bit types
    full[:, :cols] = x
    ref = reference_stats(to_float(x, kind), rows_per_segment=rows // segments, dtype={"fp16": "float16", "bf16": "bfloat16",
                                                                                       "f32": "float32"}[kind])
    return full, ref


def on_device(full, kind, off):
    """The strided tensor on the device, its first element `off` elements into the allocation (element-aligned only)."""
    signed = full.view(np.int32 if kind == "f32" else np.int16).reshape(-1)
    buf = torch.empty(signed.size + off + 8, dtype=torch.from_numpy(signed[:1]).dtype, device=DEV)
    buf[off:off + signed.size] = torch.from_numpy(signed.copy()).to(DEV)
    return buf[off:].view({"f32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[kind])


def same(got, ref):
    return len(got) == len(ref) and all(np.array_equal(g[k], r[k]) for g, r in zip(got, ref) for k in r)


@pytest.mark.parametrize("lib", ["bf16", "fp16"])
@pytest.mark.parametrize("f32", [False, True], ids=["h16", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_reference(shape, f32, lib):
    hip = hip_of(lib)
    kind = "f32" if f32 else lib
    rows, cols, ld, segments, off = SHAPES[shape]
    full, ref = case(shape, kind)
    t = on_device(full, kind, off)
    assert t.data_ptr() % (4 if f32 else 2) == 0 and (off == 0 or t.data_ptr() % 16 != 0)
    rps = rows // segments
    stats, bins = hip.range_stats(t, rows, cols, ld, rps, f32=f32, hist=True)
    stats2, bins2 = hip.range_stats(t, rows, cols, ld, rps, f32=f32, hist=True)
    plain, none = hip.range_stats(t, rows, cols, ld, rps, f32=f32, hist=False)
    torch.cuda.synchronize()
    got = stats_records(stats, bins)
    for s, (g, r) in enumerate(zip(got, ref)):
        print(f"[range {lib} {kind} {shape}] segment {s}: " + ", ".join(f"{k} {g[k]} / {r[k]}" for k in r if k != "hist")
              + f", bins equal {np.array_equal(g['hist'], r['hist'])}")
    assert same(got, ref)
    assert sum(r["n_nan"] for r in ref) > 0 and sum(r["n_inf"] for r in ref) > 0 or rows * cols == 1
    assert torch.equal(stats, stats2) and torch.equal(bins, bins2)                     # two runs, the same bytes
    assert none is None and torch.equal(plain, stats)                                  # the histogram changes no other number
    if segments > 1:                                                                   # a segment alone = itself among the others
        s = segments - 2
        alone = hip.range_stats(t.reshape(-1)[s * rps * ld:], rps, cols, ld, rps, f32=f32, hist=True)
        torch.cuda.synchronize()
        assert torch.equal(alone[0][0], stats[s]) and torch.equal(alone[1][0], bins[s])


@pytest.mark.parametrize("lib", ["bf16", "fp16"])
def test_binding_defaults_and_refusals(lib):
    hip = hip_of(lib)
    x = torch.randn(6, 40, device=DEV)
    x[1, 3], x[4, 0] = float("nan"), float("inf")
    for t in (x, x.to(hip.dtype)):                                                     # 2-D: shape and row stride; one segment
        got = stats_records(*hip.range_stats(t, hist=True))
        assert same(got, reference_stats(t.cpu(), dtype=str(t.dtype).replace("torch.", "")))
    view = x[:, :33]                                                                   # a strided 2-D view: ld = 40
    assert same(stats_records(*hip.range_stats(view, rows_per_segment=2, hist=True)), reference_stats(view.cpu(), rows_per_segment=2))
    cube = torch.randn(3, 4, 5, device=DEV)                                            # contiguous, not 2-D: one row
    assert same(stats_records(*hip.range_stats(cube, hist=True)), reference_stats(cube.cpu().reshape(1, -1)))
    with pytest.raises(ValueError):
        hip.range_stats(x, rows_per_segment=4)
    with pytest.raises(RuntimeError, match="finite and not negative"):
        hip.range_stats(x, hot=-1.0)
    with pytest.raises(AssertionError):
        hip.range_stats(x.double())
