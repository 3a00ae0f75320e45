"""WHERE the entry points of include/wiw_resample.h read and write — the rules and the harness of tests/test_hip_footprint.py
(tests/footprint.py) for the resampling header.  GPU only (the table itself imports without one).

Source and destination are STRIDED planes: rows with gap columns, and PAD rows between the planes (plane stride > rows x row
stride) that hold poison in the source and must keep their bytes in the destination; uint8 operands and the scratch at 1-byte
alignment (an odd address), fp32 frames and the int32 tables at 4 bytes and not 8; everything between poisoned guards.  Three
launches per case (surroundings zero, finite garbage, NaN): P1 independence, P2 containment, P3 inputs unchanged, and P4 —
the zero run against Pillow on the same bytes (`resample_fixtures.pil_resize`), exactly.
"""
import numpy as np
import pytest
import torch

import footprint as FP
import resample_fixtures as RF
from test_hip_footprint import DEV, F32, Env, ptr

U8, I32 = torch.uint8, torch.int32
PAD = 2             # pad rows after every plane
CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


def _tables(fp, tag, in_size, out_size, filt):
    """(coef ptr, bounds ptr, ksize) of one axis in arenas, or (None, None, 0) for an unchanged side."""
    import wiw_amd  # noqa: F401
    from wiw_amd.resample import pil_tables

    if in_size == out_size:
        return None, None, 0
    coef, bounds = pil_tables(in_size, out_size, filt)
    c = fp.inp(f"coef_{tag}", torch.from_numpy(coef.copy()), I32, gap=0, align=4)
    b = fp.inp(f"bounds_{tag}", torch.from_numpy(bounds.copy()), I32, gap=0, align=4)
    return ptr(c), ptr(b), coef.shape[1]


def _padded(fp, x, dtype):
    """(N, H, W) -> [N * (H + PAD)][W] rows, the PAD rows of every plane filled with this run's poison."""
    N, H, W = x.shape
    full = fp.poison(N * (H + PAD) * W, dtype).reshape(N, H + PAD, W).clone()
    full[:, :H] = x
    return full.reshape(N * (H + PAD), W)


def resample_case(entry, filt, H, W, ow, oh, N):
    def body(fp, E):
        src_u8 = RF.planes(H, W, N)
        if entry == "wiw_frames_resample_u8":
            # fp32 frames whose quantisation is src_u8: byte u -> the value 2 * u / 255 - 1 moved off the ties by the seeded jitter
            g = torch.Generator().manual_seed(5)
            jitter = (torch.rand(N, H, W, generator=g) - 0.5) * (0.9 * 2.0 / 255.0)
            x = torch.from_numpy(src_u8.astype(np.float32)) * (2.0 / 255.0) - 1.0 + jitter
            q = torch.clamp(x / 2.0 + 0.5, 0.0, 1.0).mul(255.0).round().to(torch.uint8).numpy()
            S = fp.inp("frames", _padded(fp, x, F32), F32, gap=1, align=4)
        else:
            q = src_u8
            S = fp.inp("src", _padded(fp, torch.from_numpy(src_u8.copy()), U8), U8, gap=3, align=1)
        D = fp.inout("dst", torch.zeros(N * (oh + PAD), ow, dtype=U8), U8, gap=5, align=1)
        ch, bh, kh = _tables(fp, "h", W, ow, filt)
        cv, bv, kv = _tables(fp, "v", H, oh, filt)
        scratch = None
        if ch is not None and cv is not None:
            nbytes = E.lib.wiw_resample_u8_scratch_bytes(N, H, ow)
            assert nbytes == N * H * ow
            scratch = fp.out("scratch", 1, nbytes, U8, gap=0, align=1, compare=False)
        E.ck(getattr(E.lib, entry)(E.stream(), ptr(S), (H + PAD) * S.ld, S.ld, N, H, W, ptr(D), (oh + PAD) * D.ld, D.ld, oh, ow,
                                   ch, bh, kh, cv, bv, kv, ptr(scratch)), entry)
        pad_rows = torch.arange(N * (oh + PAD)).reshape(N, oh + PAD)[:, oh:].reshape(-1)
        real_rows = torch.arange(N * (oh + PAD)).reshape(N, oh + PAD)[:, :oh].reshape(-1)
        fp.finally_check(lambda: D.untouched_in_window(rows=pad_rows.to(D.window().device)))

        def check(got, ref, what):
            same = torch.equal(got.cpu(), ref)
            print(f"[footprint P4 {E.name}] {what}: byte-identical = {same}")
            assert same, "differs from PIL"
        fp.expect(f"{entry} vs PIL", lambda: D.window()[real_rows.to(D.window().device)],
                  lambda: torch.from_numpy(RF.pil_resize(q, ow, oh, filt).reshape(N * oh, ow)), check)
    return body


def lut_case(n):
    def body(fp, E):
        import wiw_amd  # noqa: F401
        from wiw_amd.resample import u8_to_unit_range_lut

        u = torch.from_numpy(np.random.RandomState(2).randint(0, 256, size=n, dtype=np.uint8))
        u[:256] = torch.arange(256, dtype=torch.uint8)
        lut = torch.from_numpy(u8_to_unit_range_lut())
        S = fp.inp("src", u, U8, gap=0, align=1)
        L = fp.inp("lut", lut, F32, gap=0, align=4)
        D = fp.out("dst", 1, n, F32, gap=0, align=4)
        E.ck(E.lib.wiw_u8_to_f32_lut(E.stream(), ptr(S), n, ptr(L), ptr(D)), "u8_to_f32_lut")
        fp.expect("u8_to_f32_lut vs the host expression", D.window,
                  lambda: (2.0 * (u.numpy().astype(np.float32) / 255.0) - 1.0).reshape(1, n), lambda g, r, w: E.exact(g, torch.from_numpy(r), w))
    return body


R, F, L = "wiw_resample_u8", "wiw_frames_resample_u8", "wiw_u8_to_f32_lut"
add("resample_u8-both", [R], resample_case(R, "bicubic", 37, 53, 64, 64, 3))            # both passes: the scratch is used
add("resample_u8-h-only", [R], resample_case(R, "bicubic", 64, 128, 64, 64, 2))         # height kept
add("resample_u8-v-only", [R], resample_case(R, "lanczos", 48, 40, 40, 96, 2))          # width kept
add("frames_resample_u8-both", [F], resample_case(F, "bicubic", 37, 53, 64, 64, 3))
add("frames_resample_u8-v-only", [F], resample_case(F, "bicubic", 48, 40, 40, 96, 2))
add("frames_resample_u8-copy", [F], resample_case(F, "bicubic", 37, 53, 53, 37, 2))     # neither side changes: quantise and copy
add("u8_to_f32_lut", [L], lut_case(1001))

# Coverage: every `int wiw_*(` declaration of include/wiw_resample.h is in the table above or excluded here
# (tests/test_resample.py checks it without a GPU).
EXCLUDED = {}
COVERED = sorted({e for _, entries, _ in CASES for e in entries})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_footprint(case, name):
    cid, entries, body = case
    E = Env(name)
    try:
        FP.run_footprint(lambda fp: body(fp, E), device=DEV, sync=torch.cuda.synchronize)
    except RuntimeError as e:       # a device fault poisons the context: nothing more is launched on the GPU from this session
        if "illegal memory access" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in footprint case {cid} [{name}]: {e}", returncode=3)
        raise
