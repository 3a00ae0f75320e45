"""PIL-exact image resampling — CPU side.  Every comparison is for equality of bytes.

  * `resample.resample_reference` (numpy restatement of Pillow's ImagingResample) against `PIL.Image.resize`, both filters, and
    the pinned table geometry of the served output resize;
  * the two rounding identities the uint8 response rests on, over all 256 values;
  * `SVDWorker(device_resize=True)` against the default worker through a fake frontend whose two new methods are the numpy
    restatement: responses and written files byte-identical, and the fall-back past the kernels' tap cap;
  * include/wiw_resample.h against `hip.EXPORTS_RESAMPLE` and both libraries, the footprint-coverage rule for the header, and
    the argument refusals of its entry points (validated before any launch: no GPU needed).
"""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
from PIL import Image

import resample_fixtures as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wiw_resample.h")


# ------------------------------------------------------------------------------------------------ tables and the restatement
@pytest.mark.parametrize("case", RF.GEOMETRIES + RF.ONE_SIDED, ids=RF.case_id)
def test_reference_equals_pil(case):
    import wiw_amd  # noqa: F401
    from wiw_amd.resample import resample_reference

    filt, H, W, ow, oh = case
    src = RF.planes(H, W)
    got = resample_reference(src, ow, oh, filt)
    ref = RF.pil_reference(filt, H, W, ow, oh)
    assert got.dtype == np.uint8 and got.shape == ref.shape == (1, oh, ow)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ from PIL"
    assert ref.min() == 0 and ref.max() == 255          # the saturated bands reach the clamp


def test_rgb_image_resizes_plane_by_plane():
    """What lets the kernels work on planes: PIL resizes the bands of an RGB image independently."""
    a = RF.planes(37, 53, 3)
    rgb = np.asarray(Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0))).resize((64, 48), Image.LANCZOS))
    assert np.array_equal(rgb.transpose(2, 0, 1), RF.pil_resize(a, 64, 48, "lanczos"))


def test_pass_at_scale_one_is_the_identity():
    """Pillow skips a pass whose side does not change, and so do the kernels (a null table).  Nothing is lost: at scale 1 both
    filters sample ON the pixels, their integer taps are (.., 0, 2**22, 0, ..), and the pass would return its input."""
    import wiw_amd  # noqa: F401
    from wiw_amd.resample import _pass_last_axis, pil_tables

    a = RF.planes(64, 128)
    for filt, ksize in (("bicubic", 5), ("lanczos", 7)):
        coef, _ = pil_tables(128, 128, filt)
        assert coef.shape == (128, ksize) and (np.sort(coef, axis=1)[:, -1] == 1 << 22).all() and (coef.sum(1) == 1 << 22).all()
        assert np.array_equal(_pass_last_axis(a, 128, filt), a)


def test_served_table_is_pinned():
    """pil_tables(1024, 480, "bicubic"): scale 32/15, support 64/15 -> ksize 2 * 5 + 1; the windows by hand from
    xmin = int(center - support + 0.5), xmax = int(center + support + 0.5), center = (xx + 0.5) * 32 / 15."""
    import wiw_amd  # noqa: F401
    from wiw_amd.resample import MAX_TAPS, pil_tables, supported, table_ksize

    coef, bounds = pil_tables(1024, 480, "bicubic")
    assert coef.dtype == bounds.dtype == np.int32 and coef.shape == (480, 11) and bounds.shape == (480, 2)
    assert table_ksize(1024, 480, "bicubic") == 11
    assert bounds[:3].tolist() == [[0, 5], [0, 7], [1, 9]] and bounds[-3:].tolist() == [[1014, 9], [1017, 7], [1019, 5]]
    assert bounds[240].tolist() == [509, 8]              # center 513.07: int(509.3) = 509 .. int(517.83) = 517
    assert (bounds[:, 0] + bounds[:, 1] <= 1024).all() and (np.diff(bounds[:, 0]) >= 0).all()
    assert bounds[:, 1].max() == 9 and bounds[:, 1].min() == 5
    sums = coef.sum(1)                                   # normalised weights: 2**22 up to one rounding per tap
    assert (np.abs(sums - (1 << 22)) <= 5).all()
    for xx in range(480):
        assert not coef[xx, bounds[xx, 1]:].any()
    assert pil_tables(1024, 480, "bicubic")[0] is coef   # cached per geometry
    assert not coef.flags.writeable
    # the tap cap: Lanczos-3 down to 1/10 of a side is the last one served
    assert table_ksize(1000, 100, "lanczos") == 61 and supported(1000, 100, "lanczos")
    assert table_ksize(1100, 100, "lanczos") == 67 and not supported(1100, 100, "lanczos")
    assert supported(5000, 5000, "lanczos") and MAX_TAPS == 64
    with pytest.raises(ValueError):
        pil_tables(10, 10, "nearest")


def test_truncation_and_jpeg_rounding_are_identities():
    """`build_response` truncates clip(x, 0, 1) * 255 and `save_predict` rounds x * 255 + 0.5 with x = float32(u) / 255: both give
    u back for all 256 bytes, so the resized uint8 frames ARE the response."""
    import wiw_amd  # noqa: F401
    from wiw_amd.resample import u8_to_unit_range_lut

    u = np.arange(256, dtype=np.uint8)
    x = u.astype(np.float32) / 255.0
    assert np.array_equal((np.clip(x, 0, 1) * 255).astype(np.uint8), u)
    assert np.array_equal(np.clip(x * 255.0 + 0.5, 0, 255).astype(np.uint8), u)
    lut = u8_to_unit_range_lut()
    assert lut.dtype == np.float32 and lut.shape == (256,) and lut[0] == -1.0 and lut[255] == 1.0
    assert np.array_equal(lut.view(np.uint32), (2.0 * (np.asarray(u, dtype=np.float32) / 255.0) - 1.0).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the worker
class FakeDeviceFrontend:
    """`test_server.ToyFrontend` plus a CLIP branch that sees `clip_images`, and the two device-resize methods as the numpy
    restatement (what `vae.HIPFrontend` computes with the kernels)."""

    def __init__(self):
        self.calls = []

    def encode(self, images, image_noise, noise_aug_strength, clip_images=None):
        x = images + noise_aug_strength * image_noise
        B, _, H, W = x.shape
        lat = x.reshape(B, 3, H // 8, 8, W // 8, 8).mean((3, 5))
        lat = np.concatenate([lat, lat[:, :1]], 1).astype(np.float32)
        seen = images if clip_images is None else clip_images
        emb = np.stack([np.tile(np.asarray(c).mean((1, 2)), 342)[None, :1024] for c in seen]).astype(np.float32)
        return lat, emb

    def decode(self, latents):
        return np.clip(np.repeat(np.repeat(latents[:, :, :3], 8, axis=3), 8, axis=4) * 1.5, -1.2, 1.2).astype(np.float32)

    def encode_uint8(self, images_u8, image_noise, noise_aug_strength, size):
        from wiw_amd.resample import resample_reference, u8_to_unit_range_lut

        self.calls.append("encode_uint8")
        width, height = size
        lut = u8_to_unit_range_lut()
        x = np.stack([lut[im if im.shape[1:] == (height, width) else resample_reference(im, width, height, "lanczos")]
                      for im in images_u8])
        clip = [lut[im] for im in images_u8] if any(im.shape[1:] != (height, width) for im in images_u8) else None
        return self.encode(x, image_noise, noise_aug_strength, clip_images=clip)

    def decode_resized_uint8(self, latents, out_size, filter="bicubic"):
        from wiw_amd.resample import resample_reference

        self.calls.append("decode_resized_uint8")
        frames = self.decode(np.asarray(latents, dtype=np.float32))
        B, T, C, H, W = frames.shape
        u8 = (np.clip(frames / 2.0 + 0.5, 0.0, 1.0) * 255).round().astype(np.uint8)
        return resample_reference(u8.reshape(-1, H, W), out_size[0], out_size[1], filter).reshape(B, T, C, out_size[1], out_size[0])


def _workers(seed=3):
    import wiw_amd  # noqa: F401
    from wiw_amd.server.worker import SVDWorker
    from test_server import toy_denoise

    kw = dict(width=128, height=64, out_width=48, out_height=40, seed=seed)
    host, dev = FakeDeviceFrontend(), FakeDeviceFrontend()
    return SVDWorker(toy_denoise, host, **kw), SVDWorker(toy_denoise, dev, device_resize=True, **kw), host, dev


def _request(tmp, tag, image_hw, return_objects, b=2):
    acts = np.tile(np.array([[4, 1, 2, 1, 3, 1, 1, 2, 2, 1, 3, 3, 1, 1]], dtype=np.int64), (b, 1))
    dirs = [os.path.join(str(tmp), tag, f"PredA-{i}") for i in range(b)]
    req = {"b_action": acts, "save_dirs": dirs, "request_model_name": "igen"}
    if image_hw is not None:
        req["b_image"] = np.stack([RF.planes(*image_hw, N=3, seed=i) for i in range(b)])
    if return_objects:
        req["return_objects"] = [True] * b
    return req


def _files(dirs):
    out = {}
    for d in dirs:
        for f in sorted(os.listdir(d)):
            if f != "cond_rgb.png":
                out[(os.path.basename(d), f)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.mark.parametrize("return_objects", [True, False], ids=["objects", "files"])
@pytest.mark.parametrize("image_hw", [(64, 128), (50, 90), None], ids=["model-size", "other-size", "cond_rgb"])
def test_device_resize_worker_gives_the_bytes_of_the_default_worker(tmp_path, image_hw, return_objects):
    w_host, w_dev, fe_host, fe_dev = _workers()
    assert w_dev.device_resize and not w_host.device_resize
    outs = []
    for tag, w in (("host", w_host), ("dev", w_dev)):
        for k in range(2):                      # two requests: the persistent generator advances identically
            req = _request(tmp_path, f"{tag}{k}", image_hw, return_objects)
            if image_hw is None:                # no b_image: the worker loads <save_dir>/cond_rgb.png (of another size)
                for i, d in enumerate(req["save_dirs"]):
                    os.makedirs(d)
                    Image.fromarray(np.ascontiguousarray(RF.planes(72, 100, N=3, seed=5 + i).transpose(1, 2, 0))).save(
                        os.path.join(d, "cond_rgb.png"))
            outs.append((w(req), req["save_dirs"]))
    assert fe_dev.calls == ["encode_uint8", "decode_resized_uint8"] * 2 and fe_host.calls == []
    for (a, da), (b, db) in zip(outs[:2], outs[2:]):
        assert set(a) == set(b)
        if return_objects:
            assert a["pred_frames"].dtype == b["pred_frames"].dtype == np.uint8
            assert a["pred_frames"].shape == b["pred_frames"].shape == (2, 14, 3, 40, 48)
            assert np.array_equal(a["pred_frames"], b["pred_frames"])
            assert a["pred_frames"].std() > 0
        else:
            fa, fb = _files(da), _files(db)
            assert len(fa) == 2 * 15 and fa == fb           # 14 JPEGs + action_seq.json per candidate, byte for byte


def test_geometry_past_the_tap_cap_falls_back_to_the_host_path(tmp_path, caplog):
    """A b_image 13x as wide as the model: LANCZOS needs 2 * 39 + 1 = 79 taps > 64.  The request is served by the PIL path
    (one logged line, neither device method called) with the default worker's bytes; the next request takes the device path."""
    w_host, w_dev, _, fe_dev = _workers()
    ref = w_host(_request(tmp_path, "host", (64, 128 * 13), True))
    with caplog.at_level(logging.WARNING, logger="wiw_amd.server.worker"):
        got = w_dev(_request(tmp_path, "dev", (64, 128 * 13), True))
    assert fe_dev.calls == []
    assert len([r for r in caplog.records if "device_resize" in r.getMessage()]) == 1
    assert np.array_equal(got["pred_frames"], ref["pred_frames"])
    assert np.array_equal(w_dev(_request(tmp_path, "dev2", (50, 90), True))["pred_frames"],
                          w_host(_request(tmp_path, "host2", (50, 90), True))["pred_frames"])
    assert fe_dev.calls == ["encode_uint8", "decode_resized_uint8"]


def test_device_resize_is_off_by_default_and_needs_both_methods(caplog):
    import wiw_amd  # noqa: F401
    import serve_worker
    from wiw_amd.server.worker import SVDWorker
    from test_server import ToyFrontend, toy_denoise

    assert SVDWorker(toy_denoise, FakeDeviceFrontend()).device_resize is False
    with caplog.at_level(logging.WARNING, logger="wiw_amd.server.worker"):
        assert SVDWorker(toy_denoise, ToyFrontend(), device_resize=True).device_resize is False
    assert any("encode_uint8" in r.getMessage() for r in caplog.records)
    ap = serve_worker.arg_parser()
    assert ap.parse_args(["--port", "1"]).device_resize is False
    assert ap.parse_args(["--port", "1", "--device_resize"]).device_resize is True
    assert ap.parse_args(["--port", "1", "--no-device_resize"]).device_resize is False


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib_path():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import build

    return build(verbose=False)


def declared_symbols(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(wiw_[a-z0-9_]+)\s*\(", txt)))


def declared_arity(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(wiw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_header_and_binding_agree():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import SOURCES
    from wiw_amd.hip import EXPORTS, EXPORTS_CROSS_TRAIN, EXPORTS_RESAMPLE, EXPORTS_TRAIN_BATCH

    assert declared_symbols() == sorted(EXPORTS_RESAMPLE) == ["wiw_frames_resample_u8", "wiw_resample_u8",
                                                              "wiw_resample_u8_scratch_bytes", "wiw_u8_to_f32_lut"]
    assert not set(EXPORTS_RESAMPLE) & (set(EXPORTS) | set(EXPORTS_CROSS_TRAIN) | set(EXPORTS_TRAIN_BATCH))
    arity = declared_arity()
    for name, (res, args) in EXPORTS_RESAMPLE.items():
        assert len(args) == arity[name], name
        assert res is (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int)
    assert arity["wiw_resample_u8"] == arity["wiw_frames_resample_u8"] == 19 and arity["wiw_u8_to_f32_lut"] == 5
    # every `int wiw_*(` of the header is bound
    launching = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    assert launching == {"wiw_resample_u8", "wiw_frames_resample_u8", "wiw_u8_to_f32_lut"} and launching <= set(EXPORTS_RESAMPLE)
    # the first header and its table are as they were: the addition is a companion header, not a new ABI version
    main = declared_symbols(os.path.join(ROOT, "include", "wiw_svd.h"))
    assert main == sorted(EXPORTS) and len(main) == 67 and not set(main) & set(EXPORTS_RESAMPLE)
    assert re.search(r"#define WIW_ABI_VERSION 17\b", open(os.path.join(ROOT, "include", "wiw_svd.h")).read())
    assert "resample.hip" in SOURCES


@pytest.mark.parametrize("variant,code", [("bf16", 0), ("fp16", 1)])
def test_both_libraries_export_the_resample_header(lib_path, variant, code):
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS_RESAMPLE, load_library

    path = lib_path if variant == "bf16" else LIB_F16
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in wiw_resample.h but not exported by {os.path.basename(path)}"
    lib = load_library(path)
    assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code
    for name, (res, args) in EXPORTS_RESAMPLE.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_every_launching_entry_point_of_the_resample_header_has_a_footprint_case():
    """The rule of test_footprint_harness.py `test_every_launching_entry_point_has_a_footprint_case`, for this header."""
    import test_hip_resample_footprint as T

    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    missing = declared - covered - excluded
    assert not missing, f"entry points without a footprint case: {sorted(missing)}"
    assert not excluded
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 5


def test_argument_validation_without_gpu(lib_path):
    """Bad arguments return WIW_EINVAL (-1) with a message before anything is launched; the size query answers 0."""
    from wiw_amd.hip import load_library

    lib = load_library(lib_path)
    P = 4096          # a non-null, 4-byte aligned stand-in for a device pointer: refused calls never touch it

    def call(fn=lib.wiw_resample_u8, src=P, sps=64 * 128, srs=128, N=1, H=64, W=128, dst=P, dps=48 * 64, drs=64, oh=48, ow=64,
             ch=P, bh=P, kh=9, cv=P, bv=P, kv=7, scratch=P):
        return fn(None, src, sps, srs, N, H, W, dst, dps, drs, oh, ow, ch, bh, kh, cv, bv, kv, scratch)

    for fn in (lib.wiw_resample_u8, lib.wiw_frames_resample_u8):
        assert call(fn, src=None) == -1 and b"null" in lib.wiw_last_error()
        assert call(fn, dst=None) == -1 and b"null" in lib.wiw_last_error()
        assert call(fn, kh=65) == -1 and b"ksize_h <= 64" in lib.wiw_last_error()
        assert call(fn, kv=65) == -1 and b"ksize_v <= 64" in lib.wiw_last_error()
        assert call(fn, kh=0) == -1 and b"ksize_h" in lib.wiw_last_error()
        for bad in (dict(N=0), dict(H=0), dict(W=-1), dict(oh=0), dict(ow=0)):
            assert call(fn, **bad) == -1 and b"positive" in lib.wiw_last_error(), bad
        assert call(fn, srs=127) == -1 and b"row stride" in lib.wiw_last_error()
        assert call(fn, drs=63) == -1 and b"row stride" in lib.wiw_last_error()
        assert call(fn, sps=64 * 128 - 1) == -1 and b"plane stride" in lib.wiw_last_error()
        assert call(fn, dps=48 * 64 - 1) == -1 and b"plane stride" in lib.wiw_last_error()
        assert call(fn, bh=None) == -1 and b"come together" in lib.wiw_last_error()
        assert call(fn, ch=None, bh=None) == -1 and b"ow != W" in lib.wiw_last_error()
        assert call(fn, cv=None, bv=None) == -1 and b"oh != H" in lib.wiw_last_error()
        assert call(fn, scratch=None) == -1 and b"scratch" in lib.wiw_last_error()
        assert call(fn, ch=P + 2) == -1 and b"4-byte aligned" in lib.wiw_last_error()
        assert call(fn, N=1 << 30) == -1 and b"2^30 rows" in lib.wiw_last_error()
    assert call(lib.wiw_frames_resample_u8, src=P + 1) == -1 and b"4-byte aligned" in lib.wiw_last_error()
    lut = lib.wiw_u8_to_f32_lut
    assert lut(None, None, 8, P, P) == -1 and b"null" in lib.wiw_last_error()
    assert lut(None, P, 0, P, P) == -1 and b"positive" in lib.wiw_last_error()
    assert lut(None, P, 8, P + 2, P) == -1 and b"4-byte aligned" in lib.wiw_last_error()
    assert lut(None, P, 8, P, P + 1) == -1 and b"4-byte aligned" in lib.wiw_last_error()
    q = lib.wiw_resample_u8_scratch_bytes
    assert q(42, 576, 480) == 42 * 576 * 480 and q(0, 5, 5) == 0 and q(5, -1, 5) == 0 and q(5, 5, 0) == 0
    assert q(1 << 20, 1 << 10, 1 << 10) == 1 << 40          # 64-bit arithmetic
