"""PIL-exact image resampling on the device (csrc/resample.hip, include/wiw_resample.h) against Pillow itself.  Every comparison
is for equality of bytes; both library builds.  Inputs and the PIL references are shared (tests/resample_fixtures.py)."""
import numpy as np
import pytest
import torch

import resample_fixtures as RF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_HIPS = {}

# (filter, H, W, ow, oh, planes)
CASES = [
    ("bicubic", 37, 53, 64, 64, 3),              # both sides up, odd sizes, three planes, a ragged 4-row group
    ("bicubic", 64, 128, 64, 48, 1),             # both sides down
    ("bicubic", 64, 128, 64, 64, 1),             # height kept: horizontal pass only
    ("bicubic", 48, 40, 40, 96, 1),              # width kept: vertical pass only
    ("lanczos", 100, 90, 64, 128, 1),
    ("bicubic", 576, 1024, 480, 480, 3),         # the served output resize: two column tiles, the second one partial
    ("lanczos", 600, 800, 1024, 576, 3),         # the served input resize
]


def hip_for(name):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    if name not in _HIPS:
        _HIPS[name] = Hip(torch.device(DEV), DTYPES[name])
    return _HIPS[name]


def _same(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = got != ref
    print(f"[resample] {what}: {int(bad.sum())} of {ref.size} bytes differ")
    assert got.shape == ref.shape and got.dtype == ref.dtype and not bad.any()


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[RF.case_id(c[:5]) for c in CASES])
def test_resample_u8_equals_pil(case, name):
    filt, H, W, ow, oh, N = case
    hip = hip_for(name)
    src = torch.from_numpy(RF.planes(H, W, N).copy()).to(DEV)
    got = hip.resample_u8(src, oh, ow, filt)
    torch.cuda.synchronize()
    _same(got, RF.pil_reference(filt, H, W, ow, oh, N), f"{RF.case_id(case[:5])} [{name}]")


def _frames():
    """fp32 (2, 3, 40, 72): a seeded normal scaled to overshoot [-1, 1], and every tie of the quantisation — the fp32 value
    (2k + 1) / 255 - 1, for which (x / 2 + 0.5) * 255 is k + 1/2 up to rounding — with its two fp32 neighbours."""
    g = torch.Generator().manual_seed(11)
    f = (torch.randn(2, 3, 40, 72, generator=g) * 0.8).reshape(-1)
    ties = ((2.0 * np.arange(255, dtype=np.float64) + 1.0) / 255.0 - 1.0).astype(np.float32)
    vals = np.concatenate([np.nextafter(ties, np.float32(-2)), ties, np.nextafter(ties, np.float32(2))])
    f[7:7 + vals.size] = torch.from_numpy(vals)
    return f.reshape(2, 3, 40, 72)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_frames_resample_u8_equals_quantise_then_pil(name):
    import wiw_amd  # noqa: F401
    from wiw_amd.vae import frames_to_uint8_device

    hip = hip_for(name)
    frames = _frames().to(DEV)
    T, C, H, W = frames.shape
    q = frames_to_uint8_device(frames).permute(0, 3, 1, 2).reshape(T * C, H, W).cpu().numpy()        # (T, H, W, 3) -> planes
    assert q.min() == 0 and q.max() == 255
    for ow, oh in ((48, 48), (72, 48), (48, 40), (72, 40)):          # both passes, vertical only, horizontal only, the copy
        got = hip.frames_resample_u8(frames.reshape(T * C, H, W), oh, ow, "bicubic")
        torch.cuda.synchronize()
        _same(got, RF.pil_resize(q, ow, oh, "bicubic"), f"frames 40x72 -> {ow}x{oh} [{name}]")


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_u8_to_f32_lut_all_values(name):
    """Bit-equal to the numpy expression of `plumbing.preprocess_image`, over all 256 bytes (n not a multiple of the block)."""
    hip = hip_for(name)
    u = np.concatenate([np.arange(256), np.arange(255, -1, -1), np.arange(0, 256, 3)]).astype(np.uint8)
    ref = 2.0 * (u.astype(np.float32) / 255.0) - 1.0
    got = hip.u8_to_f32_lut(torch.from_numpy(u).to(DEV))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_refused_geometry_raises(name):
    """More than 64 taps: the entry point refuses (no fallback inside the binding), and nothing was launched."""
    hip = hip_for(name)
    src = torch.zeros(1, 4, 1100, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="ksize_h <= 64"):
        hip.resample_u8(src, 4, 100, "lanczos")
    torch.cuda.synchronize()
