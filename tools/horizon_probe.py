#!/usr/bin/env python
"""25-frame (SVD-XT horizon) serving numbers at 576x1024, one JSON line, ONE process, the variants alternated:
  * per precision (bf16; fp16 with the fp32 residual stream, the served default): ms per graphed UNet forward at B = 1 for
    T = 14, T = 25 as shipped (fused 32-slot temporal block at C <= 320, unfused chain above), T = 25 all fused and T = 25 all
    unfused — each leg timed twice, in two rounds, so the spread of a repeated leg is in the output; the 25-step rollout and one whole uint8 request at T = 25;
  * per launch, at the four level shapes of that forward (2 x 25 x S x C): wiw_temporal_attn_block32_bf16 against the unfused
    chain (LayerNorm + QKV GEMM + wiw_attn_temporal32_bf16), device events, rounds alternated, median us and TF/s on the
    algorithmic FLOPs (projection 2 M 3C C + attention core 4 B S heads T^2 64).
Random served-width weights (timing does not depend on them).  Usage: python tools/horizon_probe.py [--steps 25] [--rounds 7]
`--ab-only` keeps to the per-launch A/B (what a counter run under rocprofv3 --pmc wraps).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wiw_amd  # noqa: E402,F401
from wiw_amd import frontend as FE  # noqa: E402
from wiw_amd.config import UNetConfig  # noqa: E402
from wiw_amd.hip import Hip  # noqa: E402
from wiw_amd.pipeline import SVDDenoiser  # noqa: E402
from wiw_amd.server.worker import SVDWorker  # noqa: E402
from wiw_amd.unet import UNetHIP, pack_temporal_qkv  # noqa: E402
from wiw_amd.vae import HIPFrontend, VAEHIP  # noqa: E402
from wiw_amd.weights import random_state_dict  # noqa: E402

DEV = "cuda:0"
W, H = 1024, 576
LEVELS = ((9216, 5), (2304, 10), (576, 20), (144, 20))   # (sites, heads) of the four UNet levels at a 72x128 latent


def _inputs(T, B=1, seed=0):
    rs = np.random.RandomState(seed)
    h, w = H // 8, W // 8
    il = torch.from_numpy(rs.standard_normal((B, 4, h, w)).astype(np.float32))
    ie = torch.from_numpy(rs.standard_normal((B, 1, 1024)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((B, T, 4, h, w)).astype(np.float32))
    acts = np.tile(np.array([4] + [[1, 2, 1, 3][i % 4] for i in range(T - 1)], dtype=np.int64), (B, 1))
    return il, ie, noise, acts


def _timed(fn, reps):
    fn()                                   # warm-up: graph capture, allocator, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def forward_legs(dtype, res32, steps):
    """ms per graphed forward: T = 14, T = 25 (shipped, all fused, all unfused), then the same legs again (spread of a repeated leg)."""
    out, keep = {}, {}
    legs = (("t14", 14, None), ("t25", 25, None), ("t25_fused", 25, 1 << 30), ("t25_unfused", 25, 0))
    hip = Hip(torch.device(DEV), dtype)
    for name, T, fused in legs:
        cfg = UNetConfig(num_frames=T, action_input_channel=T)
        unet = UNetHIP(cfg, random_state_dict(cfg, 0), DEV, hip=hip, dtype=dtype, residual_fp32=res32)
        if fused is not None:                      # None: the shipped per-level dispatch (UNetHIP.FUSED32_MAX_C)
            unet.FUSED32_MAX_C = fused
        keep[name] = (unet, SVDDenoiser(unet, use_graph=True), _inputs(T))
    n = 6
    for rnd in (0, 1):
        for name, _, _ in legs:
            unet, den, (il, ie, noise, acts) = keep[name]
            out.setdefault(f"forward_ms_{name}", []).append(round(_timed(lambda: den.denoise(il, ie, noise, acts, num_steps=n), 2) / n, 2))
            assert den.graph_error is None, den.graph_error
    a, b = out["forward_ms_t14"]
    out["t14_repeat_spread"] = round(abs(a - b) / min(a, b), 4)
    unet, den, (il, ie, noise, acts) = keep["t25"]
    out[f"rollout_{steps}_ms_t25"] = round(_timed(lambda: den.denoise(il, ie, noise, acts, num_steps=steps), 1), 1)
    from serve_worker import _clip

    fe = HIPFrontend(VAEHIP(FE.vae_random_state_dict(1), DEV, hip=hip), _clip(None, True), dtype=dtype, device_io=True)

    def denoise(image_latents, image_embeddings, nz, actions, **kw):
        return den.denoise(torch.as_tensor(image_latents), torch.as_tensor(image_embeddings), torch.as_tensor(nz), actions, **kw)

    worker = SVDWorker(denoise, fe, width=W, height=H, out_width=480, out_height=480, num_frames=25, num_inference_steps=steps)
    rs = np.random.RandomState(1)
    req = {"b_action": _inputs(25)[3], "save_dirs": ["/tmp/horizon_probe"], "request_model_name": "igen",
           "b_image": rs.randint(0, 256, size=(1, 3, 480, 640), dtype=np.uint8), "return_objects": [True]}
    res = {}

    def run():
        res["pf"] = worker(req)["pred_frames"]
    out["request_ms_t25"] = round(_timed(run, 1), 1)
    assert res["pf"].shape == (1, 25, 3, 480, 480) and res["pf"].dtype == np.uint8
    del worker, fe, keep
    torch.cuda.empty_cache()
    return out


def kernel_ab(dtype, rounds, T=25, B=2):
    hip = Hip(torch.device(DEV), dtype)
    rows = []
    for S, heads in LEVELS:
        C, M = heads * 64, B * T * S
        g = torch.Generator().manual_seed(1)
        rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        x = (rn(M, C) * 1.5 + 0.3).to(DEV, dtype)
        wq, wk, wv = (rn(C, C) / math.sqrt(C) for _ in range(3))
        gamma, beta = 1 + 0.2 * rn(C), 0.2 * rn(C)
        wg, fold = (t.to(DEV) for t in pack_temporal_qkv(wq, wk, wv, gamma, beta, dtype=dtype))
        wqkv = torch.cat([wq, wk, wv]).to(DEV, dtype).contiguous()
        gd, bd = gamma.to(DEV), beta.to(DEV)
        o, a = torch.empty(M, C, dtype=dtype, device=DEV), torch.empty(M, C, dtype=dtype, device=DEV)
        qkv = torch.empty(M, 3 * C, dtype=dtype, device=DEV)

        def fused():
            hip.temporal_attn_block32(x, wg, fold, o, C, B, T, S, heads, 1e-5, 0.125)

        def chain():
            hip.layernorm(x, M, C, gd, bd, out=a)
            hip.gemm(a, wqkv, qkv, M=M, N=3 * C, K=C, C1=C)
            hip.attn_temporal32(qkv, 3 * C, o, C, B, T, S, heads, 0.125)

        def core():
            hip.attn_temporal32(qkv, 3 * C, o, C, B, T, S, heads, 0.125)

        us = {"fused": [], "chain": [], "attn32_alone": []}
        for fn in (fused, chain):
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in (("fused", fused), ("chain", chain), ("attn32_alone", core)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / 5)
        flops = 2.0 * M * 3 * C * C + 4.0 * B * S * heads * T * T * 64
        row = {"S": S, "heads": heads, "C": C, "rows": M}
        for name, v in us.items():
            med = float(np.median(v))
            row[f"{name}_us"] = round(med, 1)
            row[f"{name}_us_min"] = round(float(np.min(v)), 1)
            if name != "attn32_alone":
                row[f"{name}_tflops"] = round(flops / med / 1e6, 1)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ab-only", action="store_true")
    args = ap.parse_args()
    result = {"probe": "horizon", "width": W, "height": H, "latent": [H // 8, W // 8], "steps": args.steps,
              "device": torch.cuda.get_device_name(0)}
    variants = (("bf16", torch.bfloat16, False), ("fp16_res32", torch.float16, True))
    for name, dtype, _ in variants:
        result[f"temporal_block_ab_{name}"] = kernel_ab(dtype, args.rounds)
    if not args.ab_only:
        for name, dtype, res32 in variants:
            result[name] = forward_legs(dtype, res32, args.steps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
