"""Prediction horizons of up to 32 frames, the part that needs no GPU: the unchanged CPU oracle against fixtures the REFERENCE
produced at num_frames = 25 (tools/make_golden_horizon.py), the additive ABI (two new symbols, version still 17), the new
entries' argument validation, `validate_args`, and the fine-tuning refusal."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import svd_oracle as O
import wiw_amd  # noqa: F401
from wiw_amd.config import UNetConfig
from wiw_amd.weights import random_state_dict

from horizon_fixtures import GOLDEN, load_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wiw_attn_temporal32_bf16", "wiw_temporal_attn_block32_bf16")


def _sd(cfg, seed):
    return {k: torch.from_numpy(v) for k, v in random_state_dict(cfg, int(seed)).items()}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_oracle_unet_tiny_t25(golden):
    """The gate of test_oracle_golden.test_unet_b1 at 25 frames."""
    g = golden("unet_tiny_t25.npz")
    cfg = UNetConfig.tiny(25)
    assert g["sample"].shape == (2, 25, 8, 16, 16) and g["action_ids"].shape == (1, 25, 25)
    np.testing.assert_array_equal(O.action_ids_idx_encode(g["actions"]), g["action_ids"])
    out = O.unet_forward(_sd(cfg, g["weight_seed"]), cfg.as_dict(), torch.from_numpy(g["sample"]), torch.tensor(float(g["timestep"])),
                         torch.from_numpy(g["ehs"]), torch.from_numpy(g["added_time_ids"]), torch.from_numpy(g["action_ids"]))
    assert _rel(out.numpy(), g["out"]) < 5e-5
    assert 1e-4 < _rel(g["out_ref_bf16"], g["out"]) < 0.2


def test_oracle_unet_full_width_t25():
    g = load_parts("unet_full_16x32_t25")
    cfg = UNetConfig(num_frames=25, action_input_channel=25)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        out = O.unet_forward(_sd(cfg, g["weight_seed"]), cfg.as_dict(), torch.from_numpy(g["sample"]), torch.tensor(float(g["timestep"])),
                             torch.from_numpy(g["ehs"]), torch.from_numpy(g["added_time_ids"]), torch.from_numpy(g["action_ids"]))
    assert _rel(out.numpy(), g["out"]) < 5e-5
    for name in ("bf16", "fp16"):
        assert 1e-5 < _rel(g[f"out_ref_{name}_weights_fp32_math"], g["out"]) < 0.2 and 1e-5 < _rel(g[f"out_ref_{name}"], g["out"]) < 0.2


def test_oracle_pipeline_loop_t25(golden):
    """The gate of test_oracle_golden.test_pipeline_loop on the 25-frame loop fixture."""
    g = golden("pipeline_tiny_t25.npz")
    cfg = UNetConfig.tiny(25)
    assert g["latent_noise"].shape == (1, 25, 4, 16, 16)
    lat = O.denoise(_sd(cfg, g["weight_seed"]), cfg.as_dict(), torch.from_numpy(g["image_latents"]), torch.from_numpy(g["image_embeddings"]),
                    torch.from_numpy(g["latent_noise"]), g["actions"], num_steps=int(g["num_steps"]))
    assert _rel(lat.numpy(), g["latents_out"]) < 1e-4


def test_served_width_loop_fixture_t25():
    """Shape and sanity of the served-width 10-step fixture (the oracle would need 20 served-width forwards: the GPU suite runs it)."""
    p = load_parts("pipeline_full_16x32_t25")
    assert int(p["num_frames"]) == 25 and int(p["num_steps"]) == 10 and int(p["weight_seed"]) == 4
    assert p["actions"].shape == (1, 25) and p["actions"][0, 0] == 4 and list(p["actions"][0, 1:9]) == [1, 2, 1, 3, 1, 2, 1, 3]
    assert p["latents_out"].shape == (1, 25, 4, 16, 32) and p["trajectory"].shape == (2, 25, 4, 16, 32) and list(p["trajectory_steps"]) == [5, 10]
    assert np.array_equal(p["trajectory"][-1], p["latents_out"][0])       # the last kept step IS the final latent
    for tag in ("_fp16_weights", "_bf16_weights"):
        assert 1e-6 < _rel(p["latents_out" + tag], p["latents_out"]) < 0.2


def test_no_horizon_fixture_file_is_larger_than_1_mib():
    files = [f for f in os.listdir(GOLDEN) if "_t25" in f]
    assert len(files) >= 4
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f


@pytest.fixture(scope="module")
def lib_path():
    from wiw_amd.build import build

    return build(verbose=False)


def test_new_symbols_in_header_binding_and_both_libraries(lib_path):
    import re

    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wiw_svd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in EXPORTS
    assert "#define WIW_ABI_VERSION 17" in txt
    for path, code in ((lib_path, 0), (LIB_F16, 1)):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), f"{name} not exported by {os.path.basename(path)}"
        lib.wiw_abi_version.restype = lib.wiw_dtype.restype = ctypes.c_int
        assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code


def test_new_entries_validate_before_launching(lib_path):
    """WIW_EINVAL (-1) + a message, with no GPU: T outside 1..32, null pointers, misaligned pointers / strides, operands >= 4 GiB;
    and T = 25 passes the T check (a null pointer at T = 25 is refused for the POINTER)."""
    from wiw_amd.hip import load_library

    lib = load_library(lib_path)
    err = lib.wiw_last_error
    P = 1 << 20   # a 16-byte-aligned, never dereferenced address
    un = lambda *a: lib.wiw_attn_temporal32_bf16(None, *a)          # noqa: E731   (QKV, ldqkv, O, ldo, batch, T, S, heads, scale)
    fu = lambda *a: lib.wiw_temporal_attn_block32_bf16(None, *a)    # noqa: E731   (X, W, fold, O, ldo, batch, T, S, heads, eps, scale)
    for T in (33, 0, -1):
        assert un(P, 192, P, 64, 1, T, 8, 1, 0.125) == -1 and b"1 <= T <= 32" in err()
        assert fu(P, P, P, P, 64, 1, T, 8, 1, 1e-5, 0.125) == -1 and b"1 <= T <= 32" in err()
    assert un(None, 192, P, 64, 1, 25, 8, 1, 0.125) == -1 and b"null" in err() and b"T <=" not in err()
    assert un(P, 192, None, 64, 1, 25, 8, 1, 0.125) == -1 and b"null" in err()
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        assert fu(*args, 64, 1, 25, 8, 1, 1e-5, 0.125) == -1 and b"null" in err() and b"T <=" not in err()
    assert un(P, 190, P, 64, 1, 25, 8, 1, 0.125) == -1 and b"misaligned" in err()          # ldqkv % 8
    assert un(P, 128, P, 64, 1, 25, 8, 1, 0.125) == -1 and b"misaligned" in err()          # ldqkv < 3C
    assert un(P, 192, P, 62, 1, 25, 8, 1, 0.125) == -1 and b"misaligned" in err()          # ldo % 4
    assert un(P + 8, 192, P, 64, 1, 25, 8, 1, 0.125) == -1 and b"aligned" in err()
    assert un(P, 3840, P, 1280, 1, 25, 1 << 30, 20, 0.125) == -1 and b"grid too large" in err()
    assert fu(P, P, P, P, 60, 1, 25, 8, 1, 1e-5, 0.125) == -1 and b"ldo" in err()
    assert fu(P + 8, P, P, P, 64, 1, 25, 8, 1, 1e-5, 0.125) == -1 and b"16-byte aligned" in err()
    assert fu(P, P, P, P + 4, 64, 1, 25, 8, 1, 1e-5, 0.125) == -1 and b"16-byte aligned" in err()
    assert fu(P, P, P, P, 320, 1, 25, 300000, 5, 1e-5, 0.125) == -1 and b"4 GiB" in err()   # 25 x 300 000 x 320 x 2 B = 4.8 GB
    assert fu(P, P, P, P, 1 << 20, 1, 25, 100, 1, 1e-5, 0.125) == -1 and b"O must be < 4 GiB" in err()
    assert un(P, 192, P, 64, 0, 25, 8, 1, 0.125) == -1 and b"bad sizes" in err()
    # the 16-slot entries keep their limits
    assert lib.wiw_attn_temporal_bf16(None, 1, 192, 1, 64, 1, 17, 8, 1, 0.125) == -1 and b"T <= 16" in err()
    assert lib.wiw_temporal_attn_block_bf16(None, P, P, P, P, 64, 1, 15, 8, 1, 1e-5, 0.125, P) == -1 and b"T <= 14" in err()


def _args(*argv):
    from wiw_amd.server.worker import build_arg_parser

    return build_arg_parser().parse_args(list(argv))


def test_validate_args_horizon():
    from wiw_amd.server.worker import MAX_NUM_FRAMES, validate_args

    assert MAX_NUM_FRAMES == 32
    validate_args(_args("--num_frames", "25", "--action_input_channel", "25"))
    validate_args(_args("--num_frames", "25", "--task_type", "manipulation", "--action_input_channel", "10"))
    validate_args(_args("--num_frames", "25", "--task_type", "manipulation", "--action_input_channel", "34"))
    validate_args(_args("--num_frames", "1", "--action_input_channel", "1"))
    validate_args(_args("--num_frames", "32", "--action_input_channel", "32", "--width", "448", "--height", "448"))
    for n in (33, 0, -3, 100):
        with pytest.raises(SystemExit, match="32"):
            validate_args(_args("--num_frames", str(n), "--action_input_channel", str(n)))
    with pytest.raises(SystemExit, match="num_frames"):
        validate_args(_args("--num_frames", "25", "--action_input_channel", "14"))
    # the clip is decoded whole: a (frames, size) whose widest decoder activation would reach 4 GiB is refused at start-up
    validate_args(_args("--num_frames", "28", "--action_input_channel", "28"))                   # 1024x576: 4.23e9 < 2^32
    with pytest.raises(SystemExit, match="4 GiB"):
        validate_args(_args("--num_frames", "29", "--action_input_channel", "29"))
    with pytest.raises(SystemExit, match="4 GiB"):
        validate_args(_args("--num_frames", "32", "--action_input_channel", "32"))


def test_unet_and_trainer_refuse_unbuilt_horizons():
    """UNetHIP serves 1..32 frames; fine-tuning stays at <= 16 (its temporal attention pads to 16 rows) and says so when BUILT."""
    from wiw_amd.train_unet import TRAIN_MAX_FRAMES, UNetTrain
    from wiw_amd.unet import MAX_NUM_FRAMES, UNetHIP

    assert (MAX_NUM_FRAMES, TRAIN_MAX_FRAMES) == (32, 16)
    with pytest.raises(ValueError, match="1 .. 32"):
        UNetHIP(UNetConfig.tiny(33), {}, "cpu")
    with pytest.raises(ValueError, match="at most 16"):
        UNetTrain(UNetConfig.tiny(17), {}, "cpu")
    with pytest.raises(ValueError, match="at most 16"):
        UNetTrain(UNetConfig.tiny(25), {}, "cpu")


def test_graph_pool_estimate_scales_with_frames():
    from wiw_amd.pipeline import SVDDenoiser

    class U:      # the estimate reads two attributes of the UNet
        res32_any = False

    est = {}
    for n in (14, 25):
        den = SVDDenoiser.__new__(SVDDenoiser)
        den.unet = U()
        den.unet.cfg = argparse.Namespace(num_frames=n)
        est[n] = den.graph_pool_estimate(1, 72, 128)
    assert est[14] == pytest.approx(6.2e9) and est[25] == pytest.approx(6.2e9 * 25 / 14)
