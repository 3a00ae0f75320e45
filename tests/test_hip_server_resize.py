"""`SVDWorker(device_resize=True)` on the HIP path: both image resizes of a request on the device (csrc/resample.hip behind
`HIPFrontend.encode_uint8` / `decode_resized_uint8`) against the default worker (PIL on the host) — the same request, the same
draws, the tiny geometry of test_hip_server.py `test_worker_end_to_end_matches_oracle_chain`.  Equality of bytes throughout."""
import os

import numpy as np
import pytest
import torch

import resample_fixtures as RF

pytestmark = pytest.mark.gpu

T, H, W = 4, 128, 256
_BUILT = {}


def _stack(dtype):
    """(denoise, frontend) of the tiny worker, built once per storage type."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    import wiw_amd  # noqa: F401
    from wiw_amd import frontend as FE
    from wiw_amd.config import UNetConfig
    from wiw_amd.pipeline import SVDDenoiser
    from wiw_amd.unet import UNetHIP
    from wiw_amd.vae import HIPFrontend, VAEHIP
    from wiw_amd.weights import random_state_dict

    if dtype not in _BUILT:
        cfg = UNetConfig.tiny(T)
        unet = UNetHIP(cfg, random_state_dict(cfg, 21), "cuda:0", dtype=dtype)
        den = SVDDenoiser(unet)
        vcfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
        torch.manual_seed(0)
        clip = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                                              num_attention_heads=2, image_size=224, patch_size=32,
                                                              projection_dim=1024, hidden_act="gelu")).eval()
        fe = HIPFrontend(VAEHIP(FE.vae_random_state_dict(22, **vcfg), "cuda:0", hip=unet.hip, **vcfg), clip, clip="hip")

        def denoise(il, ie, nz, act, **kw):
            return den.denoise(torch.as_tensor(il), torch.as_tensor(ie), torch.as_tensor(nz), act, **kw).cpu().numpy()
        _BUILT[dtype] = (denoise, fe)
    return _BUILT[dtype]


def _worker(dtype, device_resize, shapes):
    from wiw_amd.server.worker import SVDWorker

    denoise, fe = _stack(dtype)

    def noise_fn(shape):          # the k-th draw of a worker is a function of k alone; its shape is recorded
        shapes.append(tuple(shape))
        return np.random.RandomState(100 + len(shapes)).standard_normal(shape).astype(np.float32)
    return SVDWorker(denoise, fe, width=W, height=H, out_width=64, out_height=48, num_frames=T, num_inference_steps=2,
                     noise_fn=noise_fn, device_resize=device_resize)


def _files(dirs):
    return {(os.path.basename(d), f): open(os.path.join(d, f), "rb").read() for d in dirs for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("image_hw,return_objects", [((H, W), True), ((100, 180), False), ((100, 180), True)],
                         ids=["model-size-objects", "other-size-files", "other-size-objects"])
def test_device_resize_gives_the_host_path_bytes(tmp_path, dtype, image_hw, return_objects):
    outs, draws = {}, {}
    for mode in (False, True):
        shapes = draws.setdefault(mode, [])
        worker = _worker(dtype, mode, shapes)
        assert worker.device_resize is mode
        dirs = [str(tmp_path / f"{'dev' if mode else 'host'}" / f"PredA-{i}") for i in range(2)]
        req = {"b_action": np.array([[4, 2, 1, 3], [4, 1, 3, 3]], dtype=np.int64), "save_dirs": dirs, "request_model_name": "igen",
               "b_image": np.stack([RF.planes(*image_hw, N=3, seed=i) for i in range(2)])}
        if return_objects:
            req["return_objects"] = [True, True]
        outs[mode] = (worker(req), dirs)
    assert draws[True] == draws[False] == [(2, 3, H, W), (2, T, 4, H // 8, W // 8)]       # order and shapes of the draws
    (host, hd), (dev, dd) = outs[False], outs[True]
    if return_objects:
        a, b = host["pred_frames"], dev["pred_frames"]
        assert a.shape == b.shape == (2, T, 3, 48, 64) and a.dtype == b.dtype == np.uint8
        print(f"[server resize] {int((a != b).sum())} of {a.size} bytes differ; std {a.std():.1f}")
        assert np.array_equal(a, b) and a.std() > 0
    else:
        fa, fb = _files(hd), _files(dd)
        assert len(fa) == 2 * (T + 1) and fa == fb              # T JPEGs + action_seq.json per candidate


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_encode_uint8_is_bit_equal_to_encode_of_the_host_preprocessing(dtype):
    """Latents and embeddings of `encode_uint8` against `encode(preprocess_image(...), clip_images=image_to_array(...))`: the
    LANCZOS resize and the un-resized CLIP branch on the device, bit for bit."""
    from PIL import Image

    from wiw_amd.server import plumbing as P

    _, fe = _stack(dtype)
    planes = [RF.planes(100, 180, N=3, seed=7), RF.planes(100, 180, N=3, seed=8)]
    images = [Image.fromarray(np.ascontiguousarray(p.transpose(1, 2, 0))) for p in planes]
    noise = np.random.RandomState(4).standard_normal((2, 3, H, W)).astype(np.float32)
    x = np.stack([P.preprocess_image(im, W, H) for im in images])
    lat_ref, emb_ref = fe.encode(x, noise, 0.02, clip_images=[P.image_to_array(im) for im in images])
    lat, emb = fe.encode_uint8([P.image_to_u8_planes(im) for im in images], noise, 0.02, (W, H))
    assert np.array_equal(lat.view(np.uint32), lat_ref.view(np.uint32)) and np.array_equal(emb.view(np.uint32), emb_ref.view(np.uint32))
    assert np.isfinite(lat).all() and lat.std() > 0
