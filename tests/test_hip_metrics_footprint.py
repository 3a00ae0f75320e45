"""WHERE the entry points of include/wiw_metrics.h read and write — the rules and the harness of tests/test_hip_footprint.py
(tests/footprint.py) for the frame-metrics header.  GPU only (the table itself imports without one).

Both operands are STRIDED planes: rows with gap columns, and PAD rows between the planes (plane stride > rows x row stride) that
hold poison; uint8 operands at 1-byte alignment (an odd address), fp32 operands and the table at 4 bytes and not 8, `partials`
and `out` at 8 bytes and not 16; everything between poisoned guards.  Three launches per case (surroundings zero, finite garbage,
NaN): P1 independence, P2 containment (`out` is written in its N x 2 doubles only; `partials` is scratch: containment alone),
P3 inputs unchanged, and P4 — the zero run against the fp64 restatement of tests/metrics_fixtures.py at its tolerances.
"""
import numpy as np
import pytest
import torch

import footprint as FP
import metrics_fixtures as MF
from test_hip_footprint import DEV, F32, Env, ptr

U8, F64 = torch.uint8, torch.float64
PAD = 2             # pad rows after every plane
CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


def _padded(fp, x, dtype):
    """(N, H, W) -> [N * (H + PAD)][W] rows, the PAD rows of every plane filled with this run's poison."""
    N, H, W = x.shape
    full = fp.poison(N * (H + PAD) * W, dtype).reshape(N, H + PAD, W).clone()
    full[:, :H] = x
    return full.reshape(N * (H + PAD), W)


def _planes(N, H, W, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, size=(N, H, W)).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rs.randint(-14, 15, size=a.shape), 0, 255).astype(np.uint8)
    return a, b


def metrics_case(kinds, N, H, W):
    def body(fp, E):
        import wiw_amd  # noqa: F401
        from wiw_amd.hip import METRICS_F32, METRICS_U8

        a, b = _planes(N, H, W, H * 1000 + W)
        ops = []
        for tag, x, kind, gap in (("a", a, kinds[0], 3), ("b", b, kinds[1], 5)):
            if kind == "u8":
                S = fp.inp(tag, _padded(fp, torch.from_numpy(x.copy()), U8), U8, gap=gap, align=1)
            else:
                S = fp.inp(tag, _padded(fp, torch.from_numpy(MF.LUT[x]), F32), F32, gap=gap, align=4)
            ops += [ptr(S), METRICS_U8 if kind == "u8" else METRICS_F32, (H + PAD) * S.ld, S.ld]
        L = fp.inp("lut", torch.from_numpy(MF.LUT.copy()), F32, gap=0, align=4) if "u8" in kinds else None
        n = E.lib.wiw_frame_metrics_partials(N, H, W)
        assert n > 0 and n % (2 * N) == 0
        Pt = fp.out("partials", 1, n, F64, gap=0, align=8, compare=False)
        O = fp.out("out", N, 2, F64, gap=0, align=8)
        E.ck(E.lib.wiw_frame_metrics(E.stream(), *ops, ptr(L), N, H, W, ptr(Pt), ptr(O)), "wiw_frame_metrics")

        def check(got, ref, what):
            got = got.cpu().numpy()
            d_ssim = np.abs(got[:, 0] - ref[:, 0]).max()
            d_psnr = max(abs(MF.psnr_of(g, H * W) - MF.psnr_of(r, H * W)) for g, r in zip(got[:, 1], ref[:, 1]))
            print(f"[footprint P4 {E.name}] {what}: max |ssim - ref| = {d_ssim:.3e}, max |psnr - ref| = {d_psnr:.3e} dB")
            assert d_ssim <= MF.SSIM_TOL and d_psnr <= MF.PSNR_TOL
        fp.expect(f"frame_metrics {kinds} vs the fp64 restatement", O.window, lambda: MF.planes_metrics(a, b), check)
    return body


M = "wiw_frame_metrics"
add("frame_metrics-u8-u8", [M], metrics_case(("u8", "u8"), 3, 37, 53))             # 2 x 2 tiles, all partial; odd addresses
add("frame_metrics-f32-u8", [M], metrics_case(("f32", "u8"), 2, 61, 45))           # 3 x 2 tiles
add("frame_metrics-f32-f32", [M], metrics_case(("f32", "f32"), 2, 11, 80))         # one valid row; no table (lut = NULL)
add("frame_metrics-u8-f32-one-tile", [M], metrics_case(("u8", "f32"), 1, 34, 42))  # exactly one full tile

# Coverage: every `int wiw_*(` declaration of include/wiw_metrics.h is in the table above or excluded here
# (tests/test_metrics.py checks it without a GPU).
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
