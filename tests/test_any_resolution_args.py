"""CPU-side checks of the any-resolution serving path: start-up validation of --width / --height, and the argument
validation of the frame-padded attention entries (no launch: the arguments are refused before any HIP call)."""
import pytest

import wiw_amd  # noqa: F401
from wiw_amd.server.worker import build_arg_parser, validate_args


@pytest.fixture(scope="module")
def libs():
    from wiw_amd.build import LIB_F16, build
    from wiw_amd.hip import load_library

    return [load_library(build(verbose=False)), load_library(LIB_F16)]


def test_validate_args_accepts_448_manipulation_and_refuses_other_sizes():
    ap = build_arg_parser()
    manip = "--task_type manipulation --action_input_channel 10"
    validate_args(ap.parse_args(f"{manip} --width 448 --height 448".split()))      # the deployed manipulation worker
    validate_args(ap.parse_args("--width 448 --height 448".split()))
    validate_args(ap.parse_args(f"{manip} --width 640 --height 384".split()))
    validate_args(ap.parse_args([]))                                                # 1024 x 576, the served default
    for bad in ("--width 450 --height 448", "--width 448 --height 450", "--width 448 --height 0", "--width 32 --height 448"):
        with pytest.raises(SystemExit, match="multiple of 64"):
            validate_args(ap.parse_args(f"{manip} {bad}".split()))


def test_padded_attention_entries_validate_without_gpu(libs):
    for lib in libs:
        # frame-padded transpose: Sv not a multiple of 8, Sv < S, misaligned columns, a too-small destination stride
        assert lib.wiw_transpose_framepad_bf16(None, 1, 960, 640, 2, 49, 52, 320, 1, 112) == -1
        assert b"multiple of 8" in lib.wiw_last_error()
        assert lib.wiw_transpose_framepad_bf16(None, 1, 960, 640, 2, 49, 48, 320, 1, 112) == -1
        assert b">= S" in lib.wiw_last_error()
        assert lib.wiw_transpose_framepad_bf16(None, 1, 960, 644, 2, 49, 56, 320, 1, 112) == -1
        assert b"multiples of 8" in lib.wiw_last_error()
        assert lib.wiw_transpose_framepad_bf16(None, 1, 960, 640, 2, 49, 56, 320, 1, 104) == -1
        assert b"smaller" in lib.wiw_last_error()
        assert lib.wiw_transpose_framepad_bf16(None, None, 960, 640, 2, 49, 56, 320, 1, 112) == -1
        assert b"null" in lib.wiw_last_error()
        # padded attention: (QK, ldqk, k_col_off, Vt, ldvt, O, ldo, frames, S, Sv, heads, zeros)
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 112, 1, 320, 2, 49, 52, 5, 1) == -1
        assert b"multiple of 8" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 112, 1, 320, 2, 49, 40, 5, 1) == -1
        assert b">= S" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 644, 320, 1, 112, 1, 320, 2, 49, 56, 5, 1) == -1
        assert b"misaligned" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 112, 1, 324, 2, 49, 56, 5, 1) == -1
        assert b"misaligned" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 104, 1, 320, 2, 49, 56, 5, 1) == -1
        assert b"smaller" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 112, 1, 320, 0, 49, 56, 5, 1) == -1
        assert b"bad sizes" in lib.wiw_last_error()
        assert lib.wiw_attn_spatial_ps_padded_bf16(None, 1, 640, 320, 1, 112, 1, 320, 2, 49, 56, 5, None) == -1
        assert b"null" in lib.wiw_last_error()
        # the existing entries keep their refusals
        assert lib.wiw_attn_spatial_ps_bf16(None, 1, 640, 320, 1, 98, 1, 320, 2, 49, 5, 1) == -1
        assert b"multiple of 8" in lib.wiw_last_error()
