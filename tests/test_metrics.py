"""Validation frame metrics (SSIM / PSNR as the reference logs them) — CPU side.

  * include/wiw_metrics.h against `hip.EXPORTS_METRICS` and both libraries, the footprint-coverage rule for the header, and the
    argument refusals of its entry points (validated before any launch: no GPU needed);
  * the fp64 numpy restatement of tests/metrics_fixtures.py against the fixture of the reference's own functions
    (tests/golden/video_metrics.npz, tools/make_golden_metrics.py), every pair, at the tolerances stated there;
  * `metrics.aggregate` / `metrics.evaluate_video_metrics` (both values of `only_final`) against the fixture's aggregations, the
    per-plane numbers coming from the restatement through a stand-in for `Hip.frame_metrics`.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import metrics_fixtures as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wiw_metrics.h")


# ------------------------------------------------------------------------------------------------ fixture and restatement
def test_fixture_holds_every_pair_the_tests_name():
    g = MF.golden()
    names = sorted({k.split("__")[0] for k in g if not k.startswith(("video", "_"))})
    assert names == sorted(MF.PAIRS) and len(MF.PAIRS) == 11
    shapes = {n: MF.pair(n)[0].shape for n in MF.PAIRS}
    assert {shapes[n] for n in MF.PAIRS} >= {(11, 11), (12, 75), (45, 70), (64, 96), (37, 131), (96, 160), (11, 300), (300, 11),
                                             (150, 333)}
    for n in MF.PAIRS:
        a, b, _, _ = MF.pair(n)
        assert a.shape == b.shape and a.dtype == b.dtype == (np.float32 if n.startswith("generic_f32") else np.uint8)
    a, b, s, p = MF.pair("identical_33x47")
    assert np.array_equal(a, b) and s == 1.0 and p == 100.0
    a, b, _, _ = MF.pair("const200_one201_64x96")
    assert (a == 200).all() and int((b != 200).sum()) == 1 and b.max() == 201
    a, b, _, _ = MF.pair("near_saturated_37x131")
    assert set(np.unique(a)) == set(np.unique(b)) == {250, 251}
    a, _, _, _ = MF.pair("generic_f32_40x52")
    assert 0 <= a.min() and a.max() <= 1 and not np.array_equal(np.rint(a * 255) / 255, a)
    assert g["video__gt"].shape == g["video__gen"].shape == (2, 3, 3, 16, 20) and g["video__gt"].dtype == np.uint8
    assert os.path.getsize(MF.GOLDEN) < (1 << 20)
    assert np.array_equal(MF.LUT.view(np.uint32), (np.arange(256, dtype=np.float32) / np.float32(255)).view(np.uint32))


@pytest.mark.parametrize("name", MF.PAIRS)
def test_restatement_equals_the_reference(name):
    a, b, ssim, psnr = MF.pair(name)
    got_ssim, sse = MF.plane_metrics(a, b)
    got_psnr = MF.psnr_of(sse, a.size)
    print(f"[metrics] {name}: |ssim - ref| = {abs(got_ssim - ssim):.3e}, |psnr - ref| = {abs(got_psnr - psnr):.3e} dB")
    assert abs(got_ssim - ssim) <= MF.SSIM_TOL
    assert abs(got_psnr - psnr) <= MF.PSNR_TOL


def test_shortcuts_miss_the_ssim_tolerance():
    """What the 1e-10 is for: the exact quotient u / 255 in double (instead of the float32 one) is outside it."""
    a, b, ssim, _ = MF.pair("smooth_pm6_45x70")
    x, y = a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = MF._valid(x), MF._valid(y)
    s11, s22, s12 = MF._valid(x * x) - mu1 * mu1, MF._valid(y * y) - mu2 * mu2, MF._valid(x * y) - mu1 * mu2
    m = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))).mean()
    assert abs(m - ssim) > MF.SSIM_TOL


class RestatementHip:
    """Stands in for `Hip` where only `frame_metrics` is used: the numpy restatement on host tensors."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def frame_metrics(self, a, b):
        self.calls.append((tuple(a.shape), a.dtype, b.dtype))
        return torch.from_numpy(MF.planes_metrics(a.numpy(), b.numpy()))


def _check_aggregates(got, metric, tag, tol):
    g = MF.golden()
    for key, stored in (("value", "value"), ("value_std", "std")):
        ref = g[f"video__{metric}__{tag}__{stored}"]
        d = np.abs(np.asarray(got[key]) - ref)
        print(f"[metrics] {metric} {tag} {key}: max |got - ref| = {d.max():.3e}")
        assert len(got[key]) == len(ref) == (1 if tag == "final" else 3) and (d <= tol).all()


@pytest.mark.parametrize("only_final", [True, False], ids=["final", "frames"])
def test_aggregation_follows_the_reference(only_final):
    import wiw_amd  # noqa: F401
    from wiw_amd.metrics import aggregate

    g, tag = MF.golden(), "final" if only_final else "frames"
    for metric, tol in (("ssim", MF.SSIM_TOL), ("psnr", MF.PSNR_TOL)):
        got = aggregate(g[f"video__{metric}"], only_final)
        assert set(got) == {"value", "value_std"} and all(isinstance(v, float) for v in got["value"] + got["value_std"])
        _check_aggregates(got, metric, tag, tol)


@pytest.mark.parametrize("form", ["f32", "u8", "list"])
@pytest.mark.parametrize("only_final", [True, False], ids=["final", "frames"])
def test_evaluate_video_metrics_on_the_restatement(only_final, form):
    import wiw_amd  # noqa: F401
    from wiw_amd.metrics import evaluate_video_metrics, frame_scores

    g, hip = MF.golden(), RestatementHip()
    gt, gen = g["video__gt"], g["video__gen"]
    if form == "f32":
        gt_in, gen_in = torch.from_numpy(MF.LUT[gt]), torch.from_numpy(MF.LUT[gen])
    elif form == "u8":
        gt_in, gen_in = torch.from_numpy(gt.copy()), torch.from_numpy(gen.copy())
    else:                                            # the reference's calling form: one (B, T, C, H, W) tensor per batch
        gt_in, gen_in = [torch.from_numpy(MF.LUT[gt[i:i + 1]]) for i in range(2)], [torch.from_numpy(gen[i:i + 1].copy()) for i in range(2)]
    got = evaluate_video_metrics(gt_in, gen_in, only_final=only_final, hip=hip)
    assert sorted(got) == ["psnr", "ssim"]                      # no lpips, no fvd
    assert hip.calls[0][0] == (18, 16, 20)
    for metric, tol in (("ssim", MF.SSIM_TOL), ("psnr", MF.PSNR_TOL)):
        _check_aggregates(got[metric], metric, "final" if only_final else "frames", tol)
    ssim, psnr = frame_scores(hip, torch.from_numpy(gt.copy()), torch.from_numpy(gen.copy()))
    assert ssim.shape == psnr.shape == (2, 3) and ssim.dtype == psnr.dtype == np.float64
    assert np.abs(ssim - g["video__ssim"]).max() <= MF.SSIM_TOL and np.abs(psnr - g["video__psnr"]).max() <= MF.PSNR_TOL


def test_identical_frames_score_100_db():
    import wiw_amd  # noqa: F401
    from wiw_amd.metrics import frame_scores

    x = torch.from_numpy(MF.golden()["video__gt"].copy())
    ssim, psnr = frame_scores(RestatementHip(), x, x.clone())
    assert (psnr == 100.0).all() and np.abs(ssim - 1.0).max() <= 1e-12


def test_validate_signature_keeps_frame_metrics_off_by_default():
    import inspect

    import wiw_amd  # noqa: F401
    from wiw_amd.train_unet import Trainer

    sig = inspect.signature(Trainer.validate)
    assert sig.parameters["frame_metrics"].default is False
    assert "val_kwargs" in inspect.signature(Trainer.fit).parameters


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
    from wiw_amd import hip as H
    from wiw_amd.build import SOURCES

    assert declared_symbols() == sorted(H.EXPORTS_METRICS) == ["wiw_frame_metrics", "wiw_frame_metrics_partials"]
    others = set(H.EXPORTS) | set(H.EXPORTS_CROSS_TRAIN) | set(H.EXPORTS_TRAIN_BATCH) | set(H.EXPORTS_RESAMPLE)
    assert not set(H.EXPORTS_METRICS) & others
    arity = declared_arity()
    for name, (res, args) in H.EXPORTS_METRICS.items():
        assert len(args) == arity[name], name
        assert res is (ctypes.c_int64 if name.endswith("_partials") else ctypes.c_int)
    assert arity == {"wiw_frame_metrics": 15, "wiw_frame_metrics_partials": 3}
    launching = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    assert launching == {"wiw_frame_metrics"}
    txt = open(HEADER).read()
    assert re.search(r"#define WIW_METRICS_F32 0\b", txt) and re.search(r"#define WIW_METRICS_U8 1\b", txt)
    assert (H.METRICS_F32, H.METRICS_U8) == (0, 1)
    # the first header and its table are as they were: the addition is a companion header, not a new ABI version
    main = declared_symbols(os.path.join(ROOT, "include", "wiw_svd.h"))
    assert main == sorted(H.EXPORTS) and len(main) == 67 and not set(main) & set(H.EXPORTS_METRICS)
    assert re.search(r"#define WIW_ABI_VERSION 17\b", open(os.path.join(ROOT, "include", "wiw_svd.h")).read())
    assert "metrics.hip" in SOURCES


@pytest.mark.parametrize("variant,code", [("bf16", 0), ("fp16", 1)])
def test_both_libraries_export_the_metrics_header(lib_path, variant, code):
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS_METRICS, load_library

    path = lib_path if variant == "bf16" else LIB_F16
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in wiw_metrics.h but not exported by {os.path.basename(path)}"
    lib = load_library(path)
    assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code
    for name, (res, args) in EXPORTS_METRICS.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_every_launching_entry_point_of_the_metrics_header_has_a_footprint_case():
    """The rule of test_footprint_harness.py `test_every_launching_entry_point_has_a_footprint_case`, for this header."""
    import test_hip_metrics_footprint as T

    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    missing = declared - covered - excluded
    assert not missing, f"entry points without a footprint case: {sorted(missing)}"
    assert not excluded
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 3


def test_argument_validation_without_gpu(lib_path):
    """Bad arguments return WIW_EINVAL (-1) with a message before anything is launched; the size query answers 0."""
    from wiw_amd.hip import METRICS_F32 as F, METRICS_U8 as U, load_library

    lib = load_library(lib_path)
    P = 4096          # a non-null, 8-byte aligned stand-in for a device pointer: refused calls never touch it

    def call(a=P, ak=F, aps=64 * 128, ars=128, b=P, bk=U, bps=64 * 128, brs=128, lut=P, N=2, H=64, W=128, partials=P, out=P):
        return lib.wiw_frame_metrics(None, a, ak, aps, ars, b, bk, bps, brs, lut, N, H, W, partials, out)

    for bad in (dict(a=None), dict(b=None), dict(partials=None), dict(out=None)):
        assert call(**bad) == -1 and b"null" in lib.wiw_last_error(), bad
    assert call(H=10) == -1 and b"at least 11" in lib.wiw_last_error()
    assert call(W=10, ars=128) == -1 and b"at least 11" in lib.wiw_last_error()
    assert call(N=0) == -1 and b"positive" in lib.wiw_last_error()
    assert call(lut=None) == -1 and b"lut" in lib.wiw_last_error()                      # b is uint8
    assert call(lut=None, ak=U, bk=F) == -1 and b"lut" in lib.wiw_last_error()
    for bad in (dict(ak=2), dict(bk=-1), dict(ak=7, bk=7)):
        assert call(**bad) == -1 and b"kind" in lib.wiw_last_error(), bad
    assert call(ars=127) == -1 and b"row stride" in lib.wiw_last_error()
    assert call(brs=127) == -1 and b"row stride" in lib.wiw_last_error()
    assert call(aps=64 * 128 - 1) == -1 and b"plane stride" in lib.wiw_last_error()
    assert call(bps=64 * 128 - 1) == -1 and b"plane stride" in lib.wiw_last_error()
    assert call(a=P + 2) == -1 and b"4-byte aligned" in lib.wiw_last_error()           # a is fp32
    assert call(b=P + 2, bk=F) == -1 and b"4-byte aligned" in lib.wiw_last_error()
    assert call(lut=P + 2) == -1 and b"4-byte aligned" in lib.wiw_last_error()
    assert call(partials=P + 4) == -1 and b"8-byte aligned" in lib.wiw_last_error()
    assert call(out=P + 4) == -1 and b"8-byte aligned" in lib.wiw_last_error()
    assert call(N=1 << 25, H=64) == -1 and b"2^30 rows" in lib.wiw_last_error()
    q = lib.wiw_frame_metrics_partials
    assert q(1, 11, 11) == 2 and q(3, 34, 42) == 6 and q(3, 35, 43) == 3 * 2 * 2 * 2          # 24 x 32 tiles of the valid region
    assert q(42, 576, 1024) == 2 * 42 * 24 * 32
    for bad in ((0, 64, 64), (-1, 64, 64), (1, 10, 64), (1, 64, 10), (1 << 25, 64, 64)):
        assert q(*bad) == 0, bad
    assert q(1, 1 << 30, 1 << 20) > 1 << 32          # 64-bit arithmetic
