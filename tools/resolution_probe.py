#!/usr/bin/env python
"""448x448 manipulation serving numbers (the reference deploys FTsvd/eval_inference.py --task_type=manipulation
--action_input_channel=10 --width=448 --height=448): one JSON line with, per precision (bf16; fp16 with the fp32 residual
stream, the served default),
  * ms per UNet forward under graph replay at B = 1 and B = 8 candidates (CFG doubles the batch: 2B x 14 frames of 56x56);
  * the 30-step rollout (the reference worker's step count) at B = 1;
  * one whole request, uint8 image in -> uint8 (1, 14, 3, 480, 480) frames out (VAE + CLIP on the HIP kernels).
Random served-width weights (timing does not depend on them).  Usage: python tools/resolution_probe.py [--steps 30]
"""
import argparse
import json
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
from wiw_amd.pipeline import SVDDenoiser  # noqa: E402
from wiw_amd.server.worker import SVDWorker  # noqa: E402
from wiw_amd.unet import UNetHIP  # noqa: E402
from wiw_amd.vae import HIPFrontend, VAEHIP  # noqa: E402
from wiw_amd.weights import random_state_dict  # noqa: E402

DEV = "cuda:0"
W = H = 448
T = 14


def _inputs(B, seed=0):
    rs = np.random.RandomState(seed)
    h, w = H // 8, W // 8
    il = torch.from_numpy(rs.standard_normal((B, 4, h, w)).astype(np.float32))
    ie = torch.from_numpy(rs.standard_normal((B, 1, 1024)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((B, T, 4, h, w)).astype(np.float32))
    acts = np.zeros((B, T, 8), np.float32)
    acts[..., :3] = rs.uniform([-0.3, -0.5, 0.6], [0.7, 0.5, 1.6], size=(B, T, 3))
    acts[..., 3:7] = rs.standard_normal((B, T, 4))
    acts[..., 7] = rs.uniform(0, 1, size=(B, T))
    return il, ie, noise, acts


def _timed(fn, reps):
    fn()                                   # warm-up: graph capture, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def probe(cfg, sd, clip, vae_sd, dtype, res32, steps):
    unet = UNetHIP(cfg, sd, DEV, dtype=dtype, residual_fp32=res32)
    den = SVDDenoiser(unet, use_graph=True)
    out = {}
    for B, n in ((1, 10), (8, 4)):       # the loop's per-step cost is one graphed UNet forward (+ a tiny Euler kernel)
        il, ie, noise, acts = _inputs(B)
        out[f"forward_ms_b{B}"] = round(_timed(lambda: den.denoise(il, ie, noise, acts, num_steps=n), 2) / n, 2)
    il, ie, noise, acts = _inputs(1)
    out[f"rollout_{steps}_ms"] = round(_timed(lambda: den.denoise(il, ie, noise, acts, num_steps=steps), 2), 1)
    assert den.graph_error is None, den.graph_error
    fe = HIPFrontend(VAEHIP(vae_sd, DEV, hip=unet.hip), clip, dtype=dtype, device_io=True)

    def denoise(image_latents, image_embeddings, nz, actions, **kw):
        return den.denoise(torch.as_tensor(image_latents), torch.as_tensor(image_embeddings), torch.as_tensor(nz), actions, **kw)

    worker = SVDWorker(denoise, fe, width=W, height=H, out_width=480, out_height=480, num_frames=T, num_inference_steps=steps,
                       task_type="manipulation")
    rs = np.random.RandomState(1)
    req = {"b_action": _inputs(1)[3], "save_dirs": ["/tmp/resolution_probe"], "request_model_name": "igen",
           "b_image": rs.randint(0, 256, size=(1, 3, 480, 640), dtype=np.uint8), "return_objects": [True]}
    res = {}

    def run():
        res["pf"] = worker(req)["pred_frames"]
    out["request_ms"] = round(_timed(run, 2), 1)
    pf = res["pf"]
    assert pf.shape == (1, T, 3, 480, 480) and pf.dtype == np.uint8
    del worker, fe, den, unet
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    from serve_worker import _clip

    cfg = UNetConfig(num_frames=T, action_input_channel=10, task_type="manipulation")
    sd = random_state_dict(cfg, 0)
    vae_sd = FE.vae_random_state_dict(1)
    clip = _clip(None, True)
    result = {"probe": "resolution", "width": W, "height": H, "task_type": "manipulation", "num_frames": T,
              "latent": [H // 8, W // 8], "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, dtype, res32 in (("bf16", torch.bfloat16, False), ("fp16_res32", torch.float16, True)):
        result[name] = probe(cfg, sd, clip, vae_sd, dtype, res32, args.steps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
