"""`SVDWorker(finite_guard=...)` end to end on the GPU, at the tiny geometry of tests/test_hip_server.py (UNetConfig.tiny(4),
128x256, 3 Euler steps, reduced VAE and CLIP, explicit noise draws), VAE / CLIP / denoiser all on the HIP kernels with device
tensors in between, as `serve_worker.build_worker` wires them: the statistics come from `wiw_range_stats`.

The overflowing checkpoints: weight and bias of ONE 3x3 convolution scaled by GAIN = 2^18, chosen on the CPU with the fp32
oracle (oracle/svd_oracle.py, oracle/vae_oracle.py; this request, these draws):
  * UNet `mid_block.resnets.0.spatial_res_block.conv1`: largest |w| = 0.0295 -> 7.7e3 after scaling (fp16 holds it; largest
    finite fp16 value 65504); the oracle's output of that convolution has absmax 1.0 .. 1.3 per candidate and forward
    unscaled, and 2.55e5 .. 3.44e5 scaled (smallest over the 6 forwards and 2 candidates: 254803.7): past 65504 in every
    candidate at every step, so the 16-bit `h` of `_res_block` holds an inf and the next GroupNorm spreads NaN over the
    candidate.  The oracle's own latents stay finite (absmax 2.53): bf16, with fp32's exponent range, serves it;
  * VAE `decoder.conv_in`: largest |w| = 0.167 -> 4.4e4; the oracle's output absmax is 8.8 / 8.5 per candidate unscaled and
    2.31e6 / 2.22e6 scaled; its frames stay finite.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H, W, B, STEPS = 4, 128, 256, 2, 3
GAIN = 2.0 ** 18
UNET_CONV = "mid_block.resnets.0.spatial_res_block.conv1"
VAE_CONV = "decoder.conv_in"
VCFG = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)


def scaled(sd, conv):
    out = dict(sd)
    for s in (".weight", ".bias"):
        out[conv + s] = (np.asarray(sd[conv + s], dtype=np.float32) * np.float32(GAIN)).astype(np.float32)
    assert np.abs(out[conv + ".weight"]).max() < 65504 / 1.4          # the scaled weights are fp16 values
    return out


@pytest.fixture(scope="module")
def env():
    """The weights, the request, and a factory of chains (denoise, frontend) per (dtype, unet weights, vae weights), each
    built once."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    import wiw_amd  # noqa: F401
    from wiw_amd import frontend as FE
    from wiw_amd.config import UNetConfig
    from wiw_amd.pipeline import SVDDenoiser
    from wiw_amd.server.worker import SVDWorker
    from wiw_amd.unet import UNetHIP
    from wiw_amd.vae import HIPFrontend, VAEHIP
    from wiw_amd.weights import random_state_dict

    cfg = UNetConfig.tiny(T)
    sds = {"healthy": random_state_dict(cfg, 21)}
    sds["overflow"] = scaled(sds["healthy"], UNET_CONV)
    vsds = {"healthy": FE.vae_random_state_dict(22, **VCFG)}
    vsds["overflow"] = scaled(vsds["healthy"], VAE_CONV)
    torch.manual_seed(0)
    clip = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                                          num_attention_heads=2, image_size=224, patch_size=32,
                                                          projection_dim=1024, hidden_act="gelu")).eval()
    chains = {}

    def chain(dtype, unet="healthy", vae="healthy"):
        key = (dtype, unet, vae)
        if key not in chains:
            # as served: fp16 carries the block-level fp32 residual stream, bf16 does not (server.worker.resolve_precision)
            net = UNetHIP(cfg, sds[unet], DEV, dtype=dtype, residual_fp32=dtype == torch.float16)
            den = SVDDenoiser(net, use_graph=False)
            fe = HIPFrontend(VAEHIP(vsds[vae], DEV, hip=net.hip, **VCFG), clip, dtype=dtype, device_io=True)

            def denoise(il, ie, nz, act, **kw):
                return den.denoise(torch.as_tensor(il), torch.as_tensor(ie), torch.as_tensor(nz), act, **kw)
            chains[key] = (denoise, fe, net.hip)
        return chains[key]

    def draws(nan_at=None):
        """noise_fn: the request's two draws, the same for every worker; nan_at: a candidate whose latent noise holds a NaN."""
        count = []

        def noise_fn(shape):
            x = np.random.RandomState(100 + len(count)).standard_normal(shape).astype(np.float32)
            if len(count) == 1 and nan_at is not None:
                x[nan_at, 0, 1, 3, 4] = np.nan          # frame 0: a turn re-derives later frames from their predecessor
            count.append(shape)
            return x
        return noise_fn

    def worker(ch, nan_at=None, **kw):
        return SVDWorker(ch[0], ch[1], width=W, height=H, out_width=64, out_height=48, num_frames=T, num_inference_steps=STEPS,
                         noise_fn=draws(nan_at), **kw)

    rs = np.random.RandomState(0)
    req = {"b_action": np.array([[4, 2, 1, 3], [4, 1, 3, 3]], dtype=np.int64), "save_dirs": ["unused-a", "unused-b"],
           "request_model_name": "igen", "b_image": rs.randint(0, 256, size=(B, 3, H, W), dtype=np.uint8),
           "return_objects": [True] * B}
    return dict(chain=chain, worker=worker, req=req)


class CountRangeCalls:
    """Counts `wiw_range_stats` calls on a bound library."""

    def __init__(self, hip):
        self.lib, self.n = hip.lib, 0

    def __enter__(self):
        self.real = self.lib.wiw_range_stats

        def counting(*a):
            self.n += 1
            return self.real(*a)
        self.lib.wiw_range_stats = counting
        return self

    def __exit__(self, *exc):
        self.lib.wiw_range_stats = self.real


@pytest.mark.parametrize("device_resize", [False, True], ids=["host-resize", "device-resize"])
def test_healthy_weights_error_gives_the_bytes_of_off(env, device_resize):
    ch = env["chain"](torch.float16)
    with CountRangeCalls(ch[2]) as c:
        off = env["worker"](ch, device_resize=device_resize)(env["req"])["pred_frames"]
        assert c.n == 0                                                   # "off" launches no statistics
        w = env["worker"](ch, finite_guard="error", device_resize=device_resize)
        err = w(env["req"])["pred_frames"]
        assert c.n == 1 + B                                               # the latents once, the frames per decoded clip
    assert off.shape == (B, T, 3, 48, 64) and off.std() > 0 and np.array_equal(off, err)
    st = w.guard_status()
    assert (st["requests"], st["candidates_checked"], st["bad_latents"], st["bad_frames"], st["re_served"], st["failed"]) \
        == (1, B, 0, 0, 0, 0)


def test_overflowing_unet_error_names_every_candidate_at_the_latents(env):
    from wiw_amd.server.worker import NonFiniteOutput

    w = env["worker"](env["chain"](torch.float16, unet="overflow"), finite_guard="error")
    with pytest.raises(NonFiniteOutput) as e:
        w(env["req"])
    print(f"[finite guard] {e.value}")
    assert e.value.indices == list(range(B)) and e.value.stage == "latents" and e.value.stages == ["latents"] * B
    assert all(sum(c["latents"]) > 0 for c in e.value.counts)
    assert w.guard_status()["bad_latents"] == B and w.guard_status()["failed"] == B


def test_overflowing_unet_fallback_answers_with_the_bf16_workers_bytes(env):
    fb = env["worker"](env["chain"](torch.bfloat16, unet="overflow"))
    w = env["worker"](env["chain"](torch.float16, unet="overflow"), finite_guard="fallback", fallback=fb)
    out = w(env["req"])["pred_frames"]
    bf16 = env["worker"](env["chain"](torch.bfloat16, unet="overflow"))(env["req"])["pred_frames"]          # the same draws
    assert out.std() > 0 and np.array_equal(out, bf16)
    st = w.guard_status()
    assert (st["candidates_checked"], st["bad_latents"], st["re_served"], st["failed"]) == (B, B, B, 0)


def test_nan_in_one_candidates_noise(env):
    from wiw_amd.server.worker import NonFiniteOutput

    w = env["worker"](env["chain"](torch.float16), nan_at=1, finite_guard="error")
    with pytest.raises(NonFiniteOutput) as e:
        w(env["req"])
    assert e.value.indices == [1] and e.value.stage == "latents"          # candidates do not mix: candidate 0 is clean
    fb = env["worker"](env["chain"](torch.bfloat16))
    w = env["worker"](env["chain"](torch.float16), nan_at=1, finite_guard="fallback", fallback=fb)
    with pytest.raises(NonFiniteOutput, match="fallback chain too") as e:          # the same draw: bf16 is NaN too
        w(env["req"])
    assert e.value.indices == [1] and w.guard_status()["failed"] == 1 and w.guard_status()["re_served"] == 0


def test_overflowing_vae_is_caught_at_the_frames(env):
    from wiw_amd.server.worker import NonFiniteOutput

    w = env["worker"](env["chain"](torch.float16, vae="overflow"), finite_guard="error")
    with pytest.raises(NonFiniteOutput) as e:
        w(env["req"])
    print(f"[finite guard] {e.value}")
    assert e.value.stage == "frames" and e.value.indices == list(range(B))
    assert all(c["latents"] == (0, 0) and sum(c["frames"]) > 0 for c in e.value.counts)
    # bf16 decodes the same latents: the fallback serves them
    fb = env["worker"](env["chain"](torch.bfloat16, vae="overflow"))
    w = env["worker"](env["chain"](torch.float16, vae="overflow"), finite_guard="fallback", fallback=fb)
    out = w(env["req"])["pred_frames"]
    assert np.array_equal(out, env["worker"](env["chain"](torch.bfloat16, vae="overflow"))(env["req"])["pred_frames"])
    assert w.guard_status()["bad_frames"] == B and w.guard_status()["re_served"] == B
