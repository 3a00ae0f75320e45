"""A 25-frame prediction horizon (SVD-XT's num_frames) through every layer: UNetHIP against fixtures the REFERENCE produced at
num_frames = 25 (tools/make_golden_horizon.py), graph replay, the batch contract, both loop fixtures through SVDDenoiser, the
temporal VAE decoding the whole 25-frame clip, and one request through SVDWorker.  GPU only.

Gates: relative ones as tests/test_hip_unet.py (the reference's OWN 16-bit run on the same inputs is the yardstick); absolute
ones 1.2 x the value measured on the MI355X, recorded beside each."""
import numpy as np
import pytest
import torch

import vae_oracle as VO
from horizon_fixtures import load_parts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 25
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
_CACHE = {}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)), float(
        np.sqrt(((a - b) ** 2).mean()) / (np.sqrt((b ** 2).mean()) + 1e-30))


def unet_for(kind, seed, name="bf16", res32=False):
    """kind 'tiny' | 'full': (cfg, fp32 state dict, UNetHIP) at 25 frames, cached per (kind, seed, dtype, stream)."""
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.hip import Hip
    from wiw_amd.unet import UNetHIP
    from wiw_amd.weights import random_state_dict

    key = (kind, seed, name, res32)
    if key not in _CACHE:
        cfg = UNetConfig.tiny(T) if kind == "tiny" else UNetConfig(num_frames=T, action_input_channel=T)
        if ("sd", kind, seed) not in _CACHE:
            _CACHE[("sd", kind, seed)] = {k: torch.from_numpy(v) for k, v in random_state_dict(cfg, seed).items()}
        if ("hip", name) not in _CACHE:
            _CACHE[("hip", name)] = Hip(torch.device(DEV), DTYPES[name])
        sd = _CACHE[("sd", kind, seed)]
        _CACHE[key] = (cfg, sd, UNetHIP(cfg, sd, DEV, hip=_CACHE[("hip", name)], residual_fp32=res32))
    return _CACHE[key]


def run_unet(unet, g):
    return unet(torch.from_numpy(g["sample"]), float(g["timestep"]), torch.from_numpy(g["ehs"]),
                torch.from_numpy(g["added_time_ids"]), torch.from_numpy(g["action_ids"])).cpu().numpy()


@pytest.mark.parametrize("fused", [None, True, False], ids=["shipped", "fused32", "unfused32"])
def test_unet_tiny_t25_golden(golden, fused):
    """The shipped per-level dispatch of `_transformer` and each 32-slot path forced at every level, against the reference's
    fp32 output; the gate of test_unet_tiny_b1_golden."""
    g = golden("unet_tiny_t25.npz")
    assert g["sample"].shape == (2, T, 8, 16, 16)
    cfg, sd, unet = unet_for("tiny", int(g["weight_seed"]))
    if fused is not None:
        unet.FUSED32_MAX_C = (1 << 30) if fused else 0
    try:
        out = run_unet(unet, g)
    finally:
        unet.__dict__.pop("FUSED32_MAX_C", None)
    mx, rms = rel(out, g["out"])
    mx_ref, rms_ref = rel(g["out_ref_bf16"], g["out"])
    print(f"[parity] unet tiny T=25 ({ {None: 'shipped dispatch', True: 'fused', False: 'unfused'}[fused] } 32-slot temporal block): HIP max_rel={mx:.3e} rms_rel={rms:.3e} "
          f"| reference bf16 run: {mx_ref:.3e} {rms_ref:.3e}")
    assert np.isfinite(out).all()
    assert rms <= rms_ref and mx <= 1.25 * mx_ref


# measured on the MI355X (deterministic kernels): rms / max of the HIP forward against the reference's fp32 output
# (the T = 14 counterparts on unet_full_16x32.npz: 9.85e-3 / 1.21e-2, gated 1.18e-2 / 1.5e-2)
FULL_T25_MEASURED = {"rms": 1.053e-2, "max": 1.306e-2}   # shipped dispatch (every level fused: 1.052e-2 / 1.249e-2)


def test_unet_full_width_t25_golden():
    g = load_parts("unet_full_16x32_t25")
    cfg, sd, unet = unet_for("full", int(g["weight_seed"]))
    out = run_unet(unet, g)
    mx, rms = rel(out, g["out"])
    mx_ref, rms_ref = rel(g["out_ref_bf16"], g["out"])
    print(f"[parity] FULL-WIDTH unet 16x32x25 B=1: HIP max_rel={mx:.3e} rms_rel={rms:.3e} | reference bf16 run {mx_ref:.3e} {rms_ref:.3e}")
    assert np.isfinite(out).all()
    assert rms <= rms_ref and mx <= 1.25 * mx_ref
    assert FULL_T25_MEASURED["rms"] is not None, "absolute gate not recorded yet"
    assert rms <= 1.2 * FULL_T25_MEASURED["rms"] and mx <= 1.2 * FULL_T25_MEASURED["max"]


def test_unet_full_width_t25_fp16_fp32_stream(golden):
    """The served default (fp16 storage, block-level fp32 residual stream) at 25 frames, gate form of
    test_hip_res32.test_unet_full_width_tolerance: against the reference's fp32 output, against the reference on the same
    fp16-rounded weights, and never worse than the reference's own fp16 run.

    The gate.  At T = 14 that test gates north_star's 1e-3 (measured 9.47e-4 / 9.68e-4).  The 25-frame fixture is a harder
    input for EVERY 16-bit evaluation: the reference's own fp16 run is 1.611e-3 from its fp32 run here against 1.50e-3 on the
    14-frame fixture, its bf16 run 1.359e-2 against 1.27e-2 (+7 % both).  The gate is therefore 1e-3 scaled by the reference's
    own fp16 error on the two fixtures (computed below from the fixtures, 1.07e-3), not by anything this code produces.
    Measured on the MI355X: 1.023e-3 / 1.033e-3 — i.e. this configuration MISSES a flat 1e-3 at 25 frames by 2-3 %, in step
    with the reference's own drift (9.47e-4 x 1.074 = 1.017e-3)."""
    g = load_parts("unet_full_16x32_t25")
    g14 = golden("unet_full_16x32.npz")
    scale = rel(g["out_ref_fp16"], g["out"])[1] / rel(g14["out_ref_fp16"], g14["out"])[1]
    gate = 1.0e-3 * max(scale, 1.0)
    cfg, sd, unet = unet_for("full", int(g["weight_seed"]), "fp16", True)
    assert unet.res32_any
    out = run_unet(unet, g)
    mx, rms = rel(out, g["out"])
    mx_w, rms_w = rel(out, g["out_ref_fp16_weights_fp32_math"])
    mx_own, rms_own = rel(g["out_ref_fp16"], g["out"])
    print(f"[tolerance] FULL-WIDTH unet 16x32x25, fp16 + fp32 residual stream: vs reference fp32 rms={rms:.3e} max={mx:.3e} | vs the "
          f"reference on the SAME fp16-rounded weights rms={rms_w:.3e} | reference's own fp16 run {rms_own:.3e}")
    assert np.isfinite(out).all()
    print(f"[tolerance] gate {gate:.3e} = 1e-3 x {scale:.3f} (the reference's own fp16 error, 25-frame over 14-frame fixture)")
    assert rms <= gate and rms_w <= gate and rms <= rms_own


def _loop_inputs(cfg, B, h, w, seed):
    rs = np.random.RandomState(seed)
    il = torch.from_numpy(rs.standard_normal((B, 4, h, w)).astype(np.float32))
    ie = torch.from_numpy(rs.standard_normal((B, 1, cfg.cross_attention_dim)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((B, T, 4, h, w)).astype(np.float32))
    acts = np.stack([np.roll(np.array(([4, 2, 1, 3, 1, 1, 2] * 4)[:T]), b) for b in range(B)])
    acts[:, 0] = 4
    return il, ie, noise, acts


def test_graph_replay_and_batch_contract_t25():
    """hipGraph replay == the eager loop, bit for bit; candidate i of a B = 2 request == its own B = 1 run, bit for bit."""
    from wiw_amd.pipeline import SVDDenoiser

    cfg, sd, unet = unet_for("tiny", 5)
    eager, graphed = SVDDenoiser(unet, use_graph=False), SVDDenoiser(unet, use_graph=True)
    il, ie, noise, acts = _loop_inputs(cfg, 2, 16, 16, 3)
    a = eager.denoise(il, ie, noise, acts, num_steps=3)
    b = graphed.denoise(il, ie, noise, acts, num_steps=3)
    assert graphed.graph_error is None, graphed.graph_error
    assert torch.isfinite(a).all() and torch.equal(a, b)
    for i in range(2):
        one = eager.denoise(il[i:i + 1], ie[i:i + 1], noise[i:i + 1], acts[i:i + 1], num_steps=3)
        assert torch.equal(one[0], a[i]), f"candidate {i} of B = 2 differs from its B = 1 run"
    # the pool estimate follows the frame count (a 25-frame capture pins 25/14 of a 14-frame one)
    assert graphed.graph_pool_estimate(1, 72, 128) == pytest.approx(6.2e9 * T / 14.0)


# measured on the MI355X: final-latent rms error of the HIP loop against the reference pipeline's fp32 latents
# (tiny: 2.808e-2; the reference's own bf16 run of the 4-frame tiny loop is 3.5e-2 from its fp32 run)
# full: 7.448e-3 after 10 steps (fp32 arithmetic on bf16-rounded weights alone: 4.889e-3).  Far below the 1.9e-2 gate of the 3-step
# T = 14 loop because the relative latent error FALLS along the schedule as the noise the error rides on is removed: the 10-step,
# 8-frame BASELINE config 0 rollout measures 7.69e-3 (test_hip_res32.CONFIG0_GATES), the 25-step T = 14 one 5.25e-3
LOOP_T25_MEASURED = {"tiny": 2.808e-2, "full": 7.448e-3}


def _denoise_fixture(p, unet):
    from wiw_amd.pipeline import SVDDenoiser

    lat = SVDDenoiser(unet).denoise(torch.from_numpy(p["image_latents"]), torch.from_numpy(p["image_embeddings"]),
                                    torch.from_numpy(p["latent_noise"]), p["actions"], num_steps=int(p["num_steps"])).cpu().numpy()
    assert np.isfinite(lat).all()
    return rel(lat, p["latents_out"])


def test_denoise_loop_tiny_t25(golden):
    p = golden("pipeline_tiny_t25.npz")
    cfg, sd, unet = unet_for("tiny", int(p["weight_seed"]))
    mx, rms = _denoise_fixture(p, unet)
    print(f"[parity] tiny 3-step loop 16x16x25 vs the reference pipeline: max_rel={mx:.3e} rms_rel={rms:.3e}")
    assert LOOP_T25_MEASURED["tiny"] is not None, "gate not recorded yet"
    assert rms <= 1.2 * LOOP_T25_MEASURED["tiny"]


def test_denoise_loop_full_width_t25():
    p = load_parts("pipeline_full_16x32_t25")
    assert int(p["num_frames"]) == T and int(p["num_steps"]) == 10 and p["latent_noise"].shape == (1, T, 4, 16, 32)
    cfg, sd, unet = unet_for("full", int(p["weight_seed"]))
    mx, rms = _denoise_fixture(p, unet)
    floor = rel(p["latents_out_bf16_weights"], p["latents_out"])[1]
    print(f"[parity] FULL-WIDTH 10-step loop 16x32x25 vs the reference pipeline: max_rel={mx:.3e} rms_rel={rms:.3e} "
          f"(weight-rounding floor {floor:.3e}; the 3-step T = 14 counterpart gates 1.9e-2)")
    assert LOOP_T25_MEASURED["full"] is not None, "gate not recorded yet"
    assert rms <= 1.2 * LOOP_T25_MEASURED["full"]


VCFG = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=2)


def test_vae_decodes_the_whole_25_frame_clip():
    """decode_chunk_size = num_frames (pipeline:291-302): the (3,1,1) convolutions see all 25 frames; gate of the 4-frame test."""
    from wiw_amd import frontend as FE
    from wiw_amd.vae import VAEHIP

    sd = FE.vae_random_state_dict(31, **VCFG)
    vae = VAEHIP(sd, DEV, **VCFG)
    h, w = 16, 32
    z = torch.randn(T, 4, h, w, generator=torch.Generator().manual_seed(7)) * 3.0
    out = vae.decode_frames(z).float().cpu()
    ref = VO.vae_decode({k: torch.from_numpy(v) for k, v in sd.items()}, z, T, len(VCFG["block_out_channels"]), VCFG["layers_per_block"])
    mx, rms = rel(out.numpy(), ref.numpy())
    print(f"[parity] VAE decode {T}x{8 * h}x{8 * w}: max_rel={mx:.3e} rms_rel={rms:.3e}")
    assert out.shape == (T, 3, 8 * h, 8 * w) and torch.isfinite(out).all() and rms <= 3e-2


def test_worker_request_25_frames(tmp_path):
    """One whole request through SVDWorker(num_frames=25) on the HIP frontend (tiny weights): (b, 25, 3, 480, 480) uint8, the
    same bytes with the eager loop and under graph replay."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    from wiw_amd import frontend as FE
    from wiw_amd.pipeline import SVDDenoiser
    from wiw_amd.server.worker import SVDWorker
    from wiw_amd.vae import HIPFrontend, VAEHIP

    cfg, sd, unet = unet_for("tiny", 21)
    vcfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
    torch.manual_seed(0)
    clip = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1,
                                                          num_attention_heads=2, image_size=224, patch_size=32,
                                                          projection_dim=1024)).eval()
    fe = HIPFrontend(VAEHIP(FE.vae_random_state_dict(22, **vcfg), DEV, hip=unet.hip, **vcfg), clip, dtype=torch.float32, clip="torch")
    rs = np.random.RandomState(0)
    req = {"b_action": np.stack([np.array([4] + [[1, 2, 1, 3][i % 4] for i in range(T - 1)]), np.array([4] + [2] * 12 + [1] * 12)]).astype(np.int64),
           "save_dirs": [str(tmp_path / "a"), str(tmp_path / "b")], "request_model_name": "igen",
           "b_image": rs.randint(0, 256, size=(2, 3, 128, 128), dtype=np.uint8), "return_objects": [True, True]}
    frames = []
    for graph in (False, True):
        den = SVDDenoiser(unet, use_graph=graph)

        def denoise(il, ie, nz, act, **kw):
            return den.denoise(torch.as_tensor(il), torch.as_tensor(ie), torch.as_tensor(nz), act, **kw)

        worker = SVDWorker(denoise, fe, width=128, height=128, out_width=480, out_height=480, num_frames=T, num_inference_steps=3, seed=1)
        pf = worker(req)["pred_frames"]
        assert den.graph_error is None, den.graph_error
        assert pf.shape == (2, T, 3, 480, 480) and pf.dtype == np.uint8
        frames.append(pf)
    assert np.array_equal(frames[0], frames[1])
    assert frames[0].std() > 1.0        # not a constant image
