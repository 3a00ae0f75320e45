"""Value-range statistics and the serving worker's finite guard — CPU side.

  * include/wiw_range.h against `hip.EXPORTS_RANGE` and both libraries, the footprint-coverage rule for the header, and the
    argument refusals of its entry points (validated before any launch: no GPU needed);
  * `range.reference_stats`, the numpy restatement the GPU tests hold the kernel to, on hand-made arrays;
  * `SVDWorker(finite_guard=...)` driven by a numpy denoiser and a numpy frontend: off / error (both stages) / fallback /
    double failure / containment behind a `Coalescer` / the start-up refusal.
"""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import wiw_amd  # noqa: F401
from test_server import ToyFrontend, make_request, toy_denoise
from wiw_amd.range import reference_stats, stats_records, thresholds
from wiw_amd.server.worker import Coalescer, NonFiniteOutput, SVDWorker, build_arg_parser, validate_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wiw_range.h")


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib_path():
    from wiw_amd.build import build

    return build(verbose=False)


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared_symbols(path=HEADER):
    return sorted(set(re.findall(r"\b(wiw_[a-z0-9_]+)\s*\(", _code(path))))


def declared_arity(path=HEADER):
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(wiw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _code(path))}


def test_header_and_binding_agree():
    from wiw_amd import hip as H
    from wiw_amd.build import SOURCES

    assert declared_symbols() == sorted(H.EXPORTS_RANGE) == ["wiw_range_stats", "wiw_range_stats_partials"]
    others = (set(H.EXPORTS) | set(H.EXPORTS_CROSS_TRAIN) | set(H.EXPORTS_TRAIN_BATCH) | set(H.EXPORTS_RESAMPLE)
              | set(H.EXPORTS_METRICS))
    assert not set(H.EXPORTS_RANGE) & others
    arity = declared_arity()
    for name, (res, args) in H.EXPORTS_RANGE.items():
        assert len(args) == arity[name], name
        assert res is (ctypes.c_int64 if name.endswith("_partials") else ctypes.c_int)
    assert arity == {"wiw_range_stats": 12, "wiw_range_stats_partials": 4}
    launching = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    assert launching == {"wiw_range_stats"}
    assert re.search(r"#define WIW_RANGE_BINS 64\b", open(HEADER).read()) and H.RANGE_BINS == 64
    # the struct of the header, field by field, and its two Python mirrors
    body = re.search(r"typedef struct WiwRangeStats \{(.*?)\} WiwRangeStats;", _code(), flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [("uint64_t", "n_nan"), ("uint64_t", "n_inf"), ("uint64_t", "n_zero"), ("uint64_t", "n_hot"),
                      ("uint64_t", "n_tiny"), ("float", "absmax"), ("float", "absmin")]
    assert [(n, t) for n, t in H.WiwRangeStats._fields_] == [(n, ctypes.c_uint64 if t == "uint64_t" else ctypes.c_float)
                                                             for t, n in fields]
    assert ctypes.sizeof(H.WiwRangeStats) == 48
    # the first header and its table are as they were: the addition is a companion header, not a new ABI version
    main = declared_symbols(os.path.join(ROOT, "include", "wiw_svd.h"))
    assert main == sorted(H.EXPORTS) and len(main) == 67 and not set(main) & set(H.EXPORTS_RANGE)
    assert re.search(r"#define WIW_ABI_VERSION 17\b", open(os.path.join(ROOT, "include", "wiw_svd.h")).read())
    assert "range.hip" in SOURCES
    assert '"wiw_range.h"' in open(os.path.join(ROOT, "world-in-world_amd", "build.py")).read()


@pytest.mark.parametrize("variant,code", [("bf16", 0), ("fp16", 1)])
def test_both_libraries_export_the_range_header(lib_path, variant, code):
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS_RANGE, load_library

    path = lib_path if variant == "bf16" else LIB_F16
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in wiw_range.h but not exported by {os.path.basename(path)}"
    lib = load_library(path)
    assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code
    for name, (res, args) in EXPORTS_RANGE.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_every_launching_entry_point_of_the_range_header_has_a_footprint_case():
    import test_hip_range_footprint as T

    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    assert not declared - covered - excluded, f"entry points without a footprint case: {sorted(declared - covered - excluded)}"
    assert not excluded
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 3


@pytest.mark.parametrize("variant", ["bf16", "fp16"])
def test_argument_validation_without_gpu(lib_path, variant):
    """Every refusal the header lists returns WIW_EINVAL (-1) with a message before anything is launched (null stream, no
    device); the size query answers 0 for the same sizes, and is positive and monotone in `rows` otherwise."""
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import load_library

    lib = load_library(lib_path if variant == "bf16" else LIB_F16)
    P = 4096          # a non-null, 8-byte aligned stand-in for a device pointer: refused calls never touch it

    def call(X=P, f32=0, rows=8, cols=16, ld=16, rps=4, hot=1.0, tiny=1e-5, partials=P, out=P, hist=None):
        return lib.wiw_range_stats(None, X, f32, rows, cols, ld, rps, hot, tiny, partials, out, hist)

    for bad in (dict(X=None), dict(partials=None), dict(out=None)):
        assert call(**bad) == -1 and b"null" in lib.wiw_last_error(), bad
    for bad in (dict(cols=0, ld=0), dict(cols=-3), dict(rows=0), dict(rows=-8)):
        assert call(**bad) == -1 and b"positive" in lib.wiw_last_error(), bad
    assert call(ld=15) == -1 and b"ld" in lib.wiw_last_error()
    for bad in (dict(rps=0), dict(rps=-4), dict(rps=3), dict(rps=16)):
        assert call(**bad) == -1 and b"rows_per_segment" in lib.wiw_last_error(), bad
    for bad in (dict(hot=-1.0), dict(hot=float("nan")), dict(hot=float("inf")), dict(tiny=-1e-9), dict(tiny=float("nan")),
                dict(tiny=float("inf")), dict(hot=float("-inf"))):
        assert call(**bad) == -1 and b"finite and not negative" in lib.wiw_last_error(), bad
    assert call(f32=2) == -1 and b"f32" in lib.wiw_last_error()
    assert call(X=P + 1) == -1 and b"element-aligned" in lib.wiw_last_error()
    assert call(X=P + 2, f32=1) == -1 and b"element-aligned" in lib.wiw_last_error()
    for bad in (dict(partials=P + 4), dict(out=P + 4), dict(hist=P + 4)):
        assert call(**bad) == -1 and b"8-byte aligned" in lib.wiw_last_error(), bad
    q = lib.wiw_range_stats_partials
    for bad in ((0, 16, 1, 0), (-1, 16, 1, 0), (8, 0, 4, 0), (8, -1, 4, 0), (8, 16, 0, 0), (8, 16, -2, 0), (8, 16, 3, 0)):
        assert q(*bad) == 0, bad
    for hist in (0, 1):
        sizes = [q(rows, 5000, 1, hist) for rows in (1, 2, 3, 64, 65, 1000, 1 << 20)]
        assert sizes[0] > 0 and sizes[0] % 8 == 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        sizes = [q(rows, 320, rows, hist) for rows in (1, 7, 8, 9, 4096, 258048)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert q(64, 100, 16, 1) > q(64, 100, 16, 0)
    assert q(1 << 34, 1 << 20, 1 << 34, 0) > 1 << 32          # 64-bit arithmetic


# ------------------------------------------------------------------------------------------------ reference_stats
def _bits32(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def _bits16(*words):
    return np.array(words, dtype=np.uint16).view(np.float16)


def test_reference_stats_counts_the_special_values_fp16():
    hot, tiny = thresholds("float16")
    assert (hot, tiny) == (32752.0, 2.0 ** -14)
    #            qNaN    sNaN    -qNaN   +inf    -inf    +0      -0      min sub  max sub  min nrm  65504   -32752  32736   1.0
    x = _bits16(0x7e00, 0x7c01, 0xfe00, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0x7bff, 0xf7ff, 0x77fe, 0x3c00)
    r = reference_stats(x)[0]
    assert (r["n_nan"], r["n_inf"], r["n_zero"]) == (3, 2, 2)
    assert r["n_hot"] == 2          # 65504 and |-32752| == hot (counts); 32736, the value below, does not
    assert r["n_tiny"] == 2         # the two subnormals; the smallest normal == tiny does not count
    assert r["absmax"] == 65504.0 and r["absmin"] == 2.0 ** -24
    h = r["hist"]
    assert h.dtype == np.uint64 and h.shape == (64,) and h.sum() == 7          # finite non-zero elements
    assert h[-24 + 32] == 1 and h[-15 + 32] == 1 and h[-14 + 32] == 1 and h[15 + 32] == 1 and h[14 + 32] == 2 and h[32] == 1


def test_reference_stats_counts_the_special_values_fp32():
    hot, tiny = thresholds("float32")
    assert hot == float(np.float32(np.finfo(np.float32).max / 2)) and tiny == 2.0 ** -126
    #            qNaN        sNaN        +inf        -inf        +0   -0          min sub     max sub     min normal  max finite
    x = _bits32(0x7fc00000, 0x7f800001, 0x7f800000, 0xff800000, 0x0, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff,
                np.float32(-hot).view(np.uint32), np.float32(3.0).view(np.uint32), np.float32(2.0 ** 40).view(np.uint32))
    r = reference_stats(x)[0]
    assert (r["n_nan"], r["n_inf"], r["n_zero"], r["n_hot"], r["n_tiny"]) == (2, 2, 2, 2, 2)
    assert r["absmax"] == float(np.finfo(np.float32).max) and r["absmin"] == 2.0 ** -149
    h = r["hist"]
    assert h.sum() == 7 and h[0] == 3          # both subnormals and 2^-126 are at or below bin 0 = 2^-32
    assert h[33] == 1 and h[63] == 3           # 3.0; 2^40, hot (just below 2^127) and the largest finite value clamp to the last bin
    # explicit thresholds: |x| == hot counts as hot, |x| == tiny does not count as tiny, zeros are never tiny
    r = reference_stats(np.array([[0.0, 0.5, -2.0, 1.0, 2.0, 4.0]], np.float32), hot=2.0, tiny=1.0, hist=False)[0]
    assert (r["n_zero"], r["n_hot"], r["n_tiny"], r["absmax"], r["absmin"], r["hist"]) == (1, 3, 1, 4.0, 0.5, None)


def test_reference_stats_segments_and_empty_segments():
    x = np.ones((6, 5), np.float32)
    x[2:4] = np.nan
    x[4, 1], x[5, 2] = np.inf, 0.0
    recs = reference_stats(x, rows_per_segment=2)
    assert [r["n_nan"] for r in recs] == [0, 10, 0] and [r["n_inf"] for r in recs] == [0, 0, 1]
    assert (recs[1]["absmax"], recs[1]["absmin"], int(recs[1]["hist"].sum())) == (0.0, float("inf"), 0)          # all NaN
    alone = reference_stats(x[:2])[0]          # a segment's numbers do not depend on the others
    assert all(np.array_equal(recs[0][k], alone[k]) for k in recs[0])
    assert (recs[2]["n_zero"], recs[2]["absmax"]) == (1, 1.0)
    zeros = reference_stats(np.zeros((1, 4), np.float16))[0]
    assert (zeros["n_zero"], zeros["absmax"], zeros["absmin"]) == (4, 0.0, float("inf"))
    for bad in (dict(rows_per_segment=4), dict(rows_per_segment=0), dict(hot=-1.0), dict(tiny=float("nan"))):
        with pytest.raises(ValueError):
            reference_stats(x, **bad)
    with pytest.raises(ValueError):
        reference_stats(np.zeros((2, 2), np.int32))


def test_stats_records_reads_the_c_struct():
    from wiw_amd.hip import WiwRangeStats

    raw = (WiwRangeStats * 2)(WiwRangeStats(1, 2, 3, 4, 1 << 40, 7.5, 0.25), WiwRangeStats(0, 0, 0, 0, 0, 0.0, float("inf")))
    buf = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(2, 48)
    hist = np.arange(128, dtype=np.int64).reshape(2, 64)
    a, b = stats_records(buf, hist)
    assert (a["n_nan"], a["n_inf"], a["n_zero"], a["n_hot"], a["n_tiny"], a["absmax"], a["absmin"]) == (1, 2, 3, 4, 1 << 40, 7.5, 0.25)
    assert (b["absmax"], b["absmin"]) == (0.0, float("inf")) and b["hist"].dtype == np.uint64 and b["hist"][63] == 127
    assert stats_records(buf)[0]["hist"] is None


# ------------------------------------------------------------------------------------------------ the guard, with fakes
POISON = 0          # the 'placeholder' action id in a candidate's first slot marks it for the poisoning denoiser


def poison_denoise(image_latents, image_embeddings, noise, actions, **kw):
    lat = toy_denoise(image_latents, image_embeddings, noise, actions, **kw)
    for i, a in enumerate(np.asarray(actions)):
        if a[0] == POISON:
            lat[i, 3, 1, 2, 5] = np.nan
    return lat


class RecordingFrontend(ToyFrontend):
    def __init__(self):
        self.encodes, self.decodes = [], []

    def encode(self, images, image_noise, noise_aug_strength):
        self.encodes.append((np.array(images), np.array(image_noise)))
        return super().encode(images, image_noise, noise_aug_strength)

    def decode(self, *args, **kw):
        self.decodes.append((args, kw))
        return super().decode(*args)


class InfFrontend(ToyFrontend):
    """The decoder overflows on candidate 0: finite latents in, one inf out."""

    def decode(self, latents):
        frames = super().decode(latents)
        frames[0, 13, 2, 7, 9] = -np.inf
        return frames


def worker(denoise=toy_denoise, frontend=None, **kw):
    return SVDWorker(denoise, frontend or ToyFrontend(), width=128, height=64, out_width=48, out_height=40, **kw)


def poisoned(req, *candidates):
    req = dict(req, b_action=req["b_action"].copy())
    for c in candidates:
        req["b_action"][c, 0] = POISON
    return req


def test_guard_off_changes_nothing(tmp_path):
    req = make_request(3, tmp=tmp_path)
    plain, fe = worker(), RecordingFrontend()
    off = worker(frontend=fe, finite_guard="off")
    a, b = plain(req), off(req)
    assert np.array_equal(a["pred_frames"], b["pred_frames"]) and a["save_dirs"] == b["save_dirs"]
    assert len(fe.decodes) == 1 and len(fe.decodes[0][0]) == 1 and fe.decodes[0][1] == {}          # decode(latents), as today
    assert off.guard_status() == {"mode": "off", "requests": 0, "candidates_checked": 0, "bad_latents": 0, "bad_frames": 0,
                                  "re_served": 0, "failed": 0}
    # a poisoned request goes through unnoticed: what the guard is for
    assert worker(poison_denoise)(poisoned(req, 1))["pred_frames"].shape == a["pred_frames"].shape
    # healthy requests under "error": the same bytes, and the counters say so
    err = worker(finite_guard="error")
    assert np.array_equal(err(req)["pred_frames"], a["pred_frames"])
    st = err.guard_status()
    assert (st["requests"], st["candidates_checked"], st["bad_latents"], st["bad_frames"], st["failed"]) == (1, 3, 0, 0, 0)
    with pytest.raises(ValueError):
        worker(finite_guard="maybe")
    with pytest.raises(ValueError):
        worker(finite_guard="fallback")


@pytest.mark.parametrize("return_objects", [True, False])
def test_guard_error_at_the_latents_stage(tmp_path, return_objects):
    req = poisoned(make_request(3, tmp=tmp_path, return_objects=return_objects), 1)
    w = worker(poison_denoise, finite_guard="error")
    with pytest.raises(NonFiniteOutput) as e:
        w(req)
    err = e.value
    assert isinstance(err, RuntimeError)
    assert err.indices == [1] and err.stage == "latents" and err.stages == ["latents"] and err.save_dirs == [req["save_dirs"][1]]
    assert err.counts[0]["latents"] == (1, 0) and err.counts[0]["frames"][0] > 0          # the NaN reaches the frames
    assert not any(os.path.exists(d) for d in req["save_dirs"])                            # nothing was written
    st = w.guard_status()
    assert (st["requests"], st["candidates_checked"], st["bad_latents"], st["bad_frames"], st["failed"]) == (1, 3, 1, 0, 1)


def test_guard_error_at_the_frames_stage(tmp_path):
    req = make_request(2, tmp=tmp_path, return_objects=False)
    w = worker(frontend=InfFrontend(), finite_guard="error")
    with pytest.raises(NonFiniteOutput) as e:
        w(req)
    assert e.value.indices == [0] and e.value.stage == "frames"
    assert e.value.counts[0] == {"latents": (0, 0), "frames": (0, 1)}
    assert not any(os.path.exists(d) for d in req["save_dirs"])
    assert w.guard_status()["bad_frames"] == 1


def fb_denoise(image_latents, image_embeddings, noise, actions, **kw):
    """The second chain of the fake: recognisably other frames."""
    return toy_denoise(image_latents, image_embeddings, noise, actions, **kw) * 0.5 + 0.25


def test_guard_fallback_serves_the_bad_candidates_from_the_same_draws(tmp_path):
    B, bad = 5, [1, 3]
    req = poisoned(make_request(B, tmp=tmp_path), *bad)
    req["b_image"] = np.random.RandomState(7).randint(0, 256, size=(B, 3, 64, 128), dtype=np.uint8)
    req["b_action"][:, 5] = np.arange(B) % 4 + 1          # every candidate its own actions
    fb_fe, seen = RecordingFrontend(), []

    def fb_recording(image_latents, image_embeddings, noise, actions, **kw):
        seen.append((np.array(noise), np.array(actions)))
        return fb_denoise(image_latents, image_embeddings, noise, actions, **kw)

    fb = worker(fb_recording, fb_fe, seed=99)
    fb_state = str(fb._rng.bit_generator.state)
    w = worker(poison_denoise, finite_guard="fallback", fallback=fb, seed=5)
    out = w(req)["pred_frames"]

    # the draws of this request, from a generator seeded alike
    rng = np.random.Generator(np.random.Philox(5))
    img_noise = rng.standard_normal((B, 3, 64, 128), dtype=np.float32)
    lat_noise = rng.standard_normal((B, 14, 4, 8, 16), dtype=np.float32)
    # the fallback chain saw exactly the bad candidates: images, actions and the slices of both draws
    assert len(fb_fe.encodes) == len(seen) == 1
    images = np.stack([2.0 * (im.astype(np.float32) / 255.0) - 1.0 for im in req["b_image"]])
    assert np.array_equal(fb_fe.encodes[0][0], images[bad]) and np.array_equal(fb_fe.encodes[0][1], img_noise[bad])
    assert np.array_equal(seen[0][0], lat_noise[bad]) and np.array_equal(seen[0][1], req["b_action"][bad])
    # its frames are where the bad candidates were, in order: what a worker on that chain answers for those draws
    draws = iter([img_noise[bad], lat_noise[bad]])
    alone = worker(fb_denoise, noise_fn=lambda shape: next(draws))
    sub = {k: (v if isinstance(v, str) else [v[i] for i in bad] if isinstance(v, list) else v[bad]) for k, v in req.items()}
    assert np.array_equal(out[bad], alone(sub)["pred_frames"])
    # the others are the first chain's bytes, untouched
    clean = worker(poison_denoise, seed=5)(req)["pred_frames"]
    good = [i for i in range(B) if i not in bad]
    assert np.array_equal(out[good], clean[good]) and not np.array_equal(out[bad], clean[bad])
    # neither generator moved beyond the request's own two draws
    ref = worker(seed=5)
    ref(make_request(B, tmp=tmp_path))
    assert str(w._rng.bit_generator.state) == str(ref._rng.bit_generator.state)
    assert str(fb._rng.bit_generator.state) == fb_state
    st = w.guard_status()
    assert (st["requests"], st["candidates_checked"], st["bad_latents"], st["re_served"], st["failed"]) == (1, B, 2, 2, 0)


def test_guard_fallback_writes_the_repaired_request(tmp_path):
    req = poisoned(make_request(2, tmp=tmp_path, return_objects=False), 0)
    w = worker(poison_denoise, finite_guard="fallback", fallback=worker(fb_denoise))
    assert w(req) == {"save_dirs": req["save_dirs"]}
    assert all(os.path.isfile(os.path.join(d, "13.jpg")) for d in req["save_dirs"])


def test_guard_fallback_that_fails_too_raises(tmp_path):
    req = poisoned(make_request(3, tmp=tmp_path, return_objects=False), 2)
    w = worker(poison_denoise, finite_guard="fallback", fallback=worker(poison_denoise))
    with pytest.raises(NonFiniteOutput, match="fallback chain too") as e:
        w(req)
    assert e.value.indices == [2] and e.value.stage == "latents" and e.value.save_dirs == [req["save_dirs"][2]]
    assert not any(os.path.exists(d) for d in req["save_dirs"])
    st = w.guard_status()
    assert (st["re_served"], st["failed"]) == (0, 1)


def test_only_the_poisoning_client_of_a_merged_batch_sees_the_error(tmp_path):
    calls = []
    base = worker(poison_denoise, finite_guard="error", noise_fn=lambda shape: np.zeros(shape, np.float32))

    def recording(req):
        calls.append(len(req["save_dirs"]))
        return base(req)

    co = Coalescer(recording, max_candidates=8, max_wait_s=0.5)
    good, bad = make_request(2, tmp=tmp_path / "g"), poisoned(make_request(2, tmp=tmp_path / "b"), 1)
    res = {}

    def run(name, req):
        try:
            res[name] = co.submit(req)
        except NonFiniteOutput as e:
            res[name] = e

    ts = [threading.Thread(target=run, args=("good", good)), threading.Thread(target=run, args=("bad", bad))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(30)
    co.close()
    assert calls[0] == 4 and sorted(calls[1:]) == [2, 2]          # merged, then one by one
    assert isinstance(res["bad"], NonFiniteOutput) and res["bad"].indices == [1] and res["bad"].save_dirs == [bad["save_dirs"][1]]
    alone = worker(noise_fn=lambda shape: np.zeros(shape, np.float32))(good)
    assert res["good"]["save_dirs"] == good["save_dirs"] and np.array_equal(res["good"]["pred_frames"], alone["pred_frames"])


def test_fallback_on_a_bfloat16_worker_is_refused_at_startup():
    ap = build_arg_parser()
    assert ap.parse_args([]).finite_guard == "off"
    with pytest.raises(SystemExit, match="nothing to fall back to"):
        validate_args(ap.parse_args(["--finite_guard", "fallback", "--weight_dtype", "bfloat16"]))
    validate_args(ap.parse_args(["--finite_guard", "fallback"]))                     # float16, the default
    validate_args(ap.parse_args(["--finite_guard", "error", "--weight_dtype", "bfloat16"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--finite_guard", "sometimes"])


# ------------------------------------------------------------------------------------------------ tools/fp16_headroom.py
def test_headroom_tool_summary_and_json_on_hand_made_records(capsys):
    import importlib.util
    import json

    from wiw_amd.range import finite_max

    spec = importlib.util.spec_from_file_location("fp16_headroom", os.path.join(ROOT, "tools", "fp16_headroom.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def record(scope, k, values, dtype="float16"):
        r = reference_stats(np.asarray(values, np.float32).reshape(1, -1), dtype=dtype)[0]
        headroom = 0.0 if r["n_inf"] else finite_max(dtype) / r["absmax"] if r["absmax"] > 0 else float("inf")
        r.update(scope=scope, family="gemm", ordinal=k, shape=(1, len(values)), dtype=dtype, headroom=headroom)
        return r

    records = [record("unet", 0, [1.0, -2.0, 0.0, 1e-6]), record("mid_block.resnets.0", 0, [40000.0, 3.0, -1.0, 2.0]),
               record("mid_block.resnets.0", 1, [np.inf, 65504.0, 1.0, 1.0]), record("mid_block.resnets.1", 0, [np.nan] * 4),
               record("up_blocks.0", 0, [0.0] * 4)]
    tool.summarise(records, top=3)
    out = capsys.readouterr().out.splitlines()
    table = out[2:5]                                                      # lowest headroom first: the inf, then 40000, then 2.0
    assert "mid_block.resnets.0#1" in table[0] and "mid_block.resnets.0#0" in table[1] and "unet#0" in table[2]
    assert table[1].split()[0] == f"{65504 / 40000:.4g}"
    bad = out[out.index(next(l for l in out if "with inf or NaN" in l)):]
    assert bad[0].startswith("[headroom] 2 tensor(s)") and "resnets.0#1" in bad[1] and "resnets.1#0" in bad[2]      # launch order
    assert any("tiny elements" in l and "5.0000% of 20" in l for l in out)           # 1e-6 is below fp16's smallest normal
    text = json.dumps(tool.to_json(records), allow_nan=False)                        # strict JSON: no Infinity / NaN token
    back = json.loads(text)
    assert back[3]["headroom"] is None and back[3]["absmin"] is None and back[4]["headroom"] is None
    assert back[2]["headroom"] == 0.0 and back[1]["shape"] == [1, 4] and len(back[0]["hist"]) == 64 and sum(back[0]["hist"]) == 3
