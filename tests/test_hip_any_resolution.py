"""Any latent size: token counts that are not multiples of 8 (the 14x14 and 7x7 levels of a 448x448 output, the deployed
manipulation worker's geometry).  GPU only, both 16-bit libraries.

  * the kernels: wiw_attn_spatial_ps_padded_bf16 against fp32 attention on the same rounded operands, for S from 1 to 3129;
    wiw_transpose_framepad_bf16 exact, padding columns zero (on a NaN-poisoned output); the fused temporal block at the
    site tails of S = 49 and 196;
  * the tiny UNet with the 10-channel manipulation embedder at a 56x56 latent against the CPU oracle, and at 24x40
    (S = 960, 240, 60, 15) against the reference's own output (tests/golden/unet_tiny_tails_24x40.npz,
    tools/make_golden_tails.py);
  * the served width (320 .. 1280 channels) at 24x40 against the oracle, and one 448x448 forward (finite, bits repeat);
  * contracts at 56x56: graph replay == eager, run-to-run bits, candidate 0 of B = 2 == its B = 1 run; the 2-step loop
    against the oracle loop;
  * a whole SVDWorker request at width = height = 448, task_type 'manipulation', HIP denoiser and HIP frontend.

Tolerances: kernels as test_attn_spatial_prescaled_north_star_shape (max <= 2e-2 max|ref|, rms <= 8e-3); networks as
test_unet_with_manipulation_actions_on_the_hip_path (rms 1.8e-2 bf16 / 2.3e-3 fp16; loop 2.2e-2 / 2.7e-3).
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import svd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
NET_TOL = {torch.bfloat16: 1.8e-2, torch.float16: 2.3e-3}
LOOP_TOL = {torch.bfloat16: 2.2e-2, torch.float16: 2.7e-3}


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)), float(
        np.sqrt(((a - b) ** 2).mean()) / (np.sqrt((b ** 2).mean()) + 1e-30))


_HIPS = {}


def get_hip(dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    if dtype not in _HIPS:
        _HIPS[dtype] = Hip(torch.device(DEV), dtype)
    return _HIPS[dtype]


def _sdpa(q, k, v, heads):
    Bn, S, C = q.shape
    q, k, v = (t.reshape(Bn, S, heads, 64).transpose(1, 2) for t in (q, k, v))
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Bn, S, C)


# ----------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S", [1, 7, 9, 36, 45, 49, 180, 196, 200, 3129])
def test_transpose_framepad_exact(dtype, S):
    hip = get_hip(dtype)
    frames, Cn = 3, 320
    Sv = -(-S // 8) * 8
    x = rnd(frames * S, 3 * Cn, seed=S).to(dtype)
    xd = x.to(DEV)
    y = torch.full((Cn, frames * Sv), float("nan"), dtype=dtype, device=DEV)
    hip.transpose_framepad(xd, 3 * Cn, 2 * Cn, frames, S, Sv, Cn, y, frames * Sv)
    torch.cuda.synchronize()
    y = y.cpu().reshape(Cn, frames, Sv)
    want = x[:, 2 * Cn:].reshape(frames, S, Cn).permute(2, 0, 1)
    assert torch.equal(y[:, :, :S], want)
    assert torch.equal(y[:, :, S:], torch.zeros(Cn, frames, Sv - S, dtype=dtype))


# (S = 3129 with 20 heads x 3 frames is left out: the fp32 reference alone would hold 2.3 GB of scores)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,heads,frames", [(S, h, f) for S in (1, 7, 9, 36, 45, 49, 180, 196, 200, 3129) for h in (1, 5, 20)
                                            for f in (1, 3) if not (S == 3129 and h == 20 and f == 3)])
def test_attn_spatial_ps_padded(dtype, S, heads, frames):
    hip = get_hip(dtype)
    C = heads * 64
    Sv = -(-S // 8) * 8
    ps = math.log2(math.e) / 8.0
    q, k, v = (rnd(frames, S, C, seed=s, scale=sc) for s, sc in ((1, 1.5), (2, 1.5), (3, 1.0)))
    rd = lambda t: t.to(dtype).float()   # noqa: E731  (what the kernel sees)
    qs, k, v = rd(q * ps), rd(k), rd(v)
    qk = torch.cat([qs, k], -1).reshape(frames * S, 2 * C).to(DEV, dtype).contiguous()
    vd = v.reshape(frames * S, C).to(DEV, dtype).contiguous()
    vt = torch.full((C, frames * Sv), float("nan"), dtype=dtype, device=DEV)
    hip.transpose_framepad(vd, C, 0, frames, S, Sv, C, vt, frames * Sv)
    o = torch.full((frames * S, C), float("nan"), dtype=dtype, device=DEV)
    hip.attn_spatial_ps_padded(qk, 2 * C, C, vt, frames * Sv, o, C, frames, S, Sv, heads)
    torch.cuda.synchronize()
    out = o.float().cpu().reshape(frames, S, C)
    ref = _sdpa(qs / ps, k, v, heads)
    assert torch.isfinite(out).all(), "rows left unwritten or non-finite"
    mx, rms = rel(out.numpy(), ref.numpy())
    assert mx <= 2e-2 and rms <= 8e-3, f"S={S} heads={heads} frames={frames}: max_rel={mx:.3e} rms_rel={rms:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,heads", [(49, 20), (196, 20), (49, 2), (196, 10)])
def test_temporal_attn_block_site_tails(dtype, S, heads):
    from wiw_amd.unet import pack_temporal_qkv

    hip = get_hip(dtype)
    B, T = 2, 14
    C = heads * 64
    x = (rnd(B, T, S, C, seed=1) * 1.5 + 0.3).to(dtype).float()
    wq, wk, wv = (rnd(C, C, seed=s) / math.sqrt(C) for s in (2, 3, 4))
    gamma, beta = 1 + 0.2 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    wg, fold = pack_temporal_qkv(wq, wk, wv, gamma, beta, dtype=dtype)
    o = torch.full((B * T * S, C), float("nan"), dtype=dtype, device=DEV)
    hip.temporal_attn_block(x.reshape(-1, C).to(DEV, dtype).contiguous(), wg.to(DEV), fold.to(DEV), o, C, B, T, S, heads,
                            1e-5, 0.125)
    torch.cuda.synchronize()
    rd = lambda t: t.to(dtype).float()   # noqa: E731
    a = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    q, k, v = a @ rd(wq).t(), a @ rd(wk).t(), a @ rd(wv).t()
    perm = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, T, heads, 64).transpose(1, 2)   # noqa: E731
    ref = F.scaled_dot_product_attention(perm(q), perm(k), perm(v)).transpose(1, 2).reshape(B, S, T, C).permute(0, 2, 1, 3)
    out = o.float().cpu().reshape(B, T, S, C)
    assert torch.isfinite(out).all(), "rows left unwritten or non-finite"
    mx, rms = rel(out.numpy(), ref.numpy())
    print(f"[parity] temporal_attn_block S={S} heads={heads} {dtype}: max_rel={mx:.3e} rms_rel={rms:.3e}")
    assert mx <= 2e-2 and rms <= 8e-3


# ----------------------------------------------------------------------------------------------
# networks
# ----------------------------------------------------------------------------------------------
def manip_cfg(T=4):
    from wiw_amd.config import UNetConfig

    return UNetConfig(block_out_channels=(64, 128, 128, 128), num_attention_heads=(1, 2, 2, 2), num_frames=T,
                      action_input_channel=10, task_type="manipulation")


def manip_inputs(cfg, B, h, w, seed):
    """(sample, ehs, added_time_ids, 10-channel action ids) for B candidates with CFG doubling."""
    rs = np.random.RandomState(seed)
    T = cfg.num_frames
    sample = rs.standard_normal((2 * B, T, 8, h, w)).astype(np.float32)
    ehs = rs.standard_normal((2 * B, 1, cfg.cross_attention_dim)).astype(np.float32)
    ehs[:B] = 0
    sample[:B, :, 4:] = 0
    tids = np.tile(np.array([[6, 127, 0.02]], dtype=np.float32), (2 * B, 1))
    acts = _manip_actions(B, T, seed)
    return sample, ehs, tids, O.manip_action_ids(acts), acts


def _manip_actions(B, T, seed):
    rs = np.random.RandomState(seed + 1000)
    acts = np.zeros((B, T, 8), np.float32)
    acts[..., :3] = rs.uniform([-0.3, -0.5, 0.6], [0.7, 0.5, 1.6], size=(B, T, 3))
    acts[..., 3:7] = rs.standard_normal((B, T, 4))
    acts[..., 7] = rs.uniform(0, 1, size=(B, T))
    return acts


_NETS = {}


def tiny_manip(dtype):
    from wiw_amd.unet import UNetHIP
    from wiw_amd.weights import random_state_dict

    if dtype not in _NETS:
        cfg = manip_cfg()
        sd = random_state_dict(cfg, 6)
        _NETS[dtype] = (cfg, sd, UNetHIP(cfg, sd, DEV, dtype=dtype, hip=get_hip(dtype)))
    return _NETS[dtype]


def _call(unet, sample, t, ehs, tids, aid):
    return unet(torch.from_numpy(sample), t, torch.from_numpy(ehs), torch.from_numpy(tids), torch.from_numpy(aid))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_manip_unet_56x56_vs_oracle(dtype):
    """Levels 56x56, 28x28, 14x14, 7x7: S = 3136, 784, 196 (tail 4) and 49 (tail 1)."""
    cfg, sd, unet = tiny_manip(dtype)
    sample, ehs, tids, aid, _ = manip_inputs(cfg, 1, 56, 56, seed=3)
    t = 1.0640485
    out = _call(unet, sample, t, ehs, tids, aid).cpu().numpy()
    with torch.no_grad():
        ref = O.unet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, cfg.as_dict(), torch.from_numpy(sample),
                             torch.tensor(t), torch.from_numpy(ehs), torch.from_numpy(tids), torch.from_numpy(aid)).numpy()
    mx, rms = rel(out, ref)
    print(f"[parity] tiny manipulation UNet 56x56, {dtype}: max_rel={mx:.3e} rms_rel={rms:.3e}")
    assert np.isfinite(out).all() and rms <= NET_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_unet_tail_geometry_golden(dtype, golden):
    """The reference's own output at latent 24x40 (S = 960, 240, 60, 15: tails of 4 and 7)."""
    from wiw_amd.config import UNetConfig
    from wiw_amd.unet import UNetHIP
    from wiw_amd.weights import random_state_dict

    g = golden("unet_tiny_tails_24x40.npz")
    cfg = UNetConfig.tiny(4)
    unet = UNetHIP(cfg, random_state_dict(cfg, int(g["weight_seed"])), DEV, dtype=dtype, hip=get_hip(dtype))
    out = _call(unet, g["sample"], float(g["timestep"]), g["ehs"], g["added_time_ids"], g["action_ids"]).cpu().numpy()
    mx, rms = rel(out, g["out"])
    mx_ref, rms_ref = rel(g["out_ref_bf16"], g["out"])
    print(f"[parity] tiny UNet 24x40 vs reference, {dtype}: max_rel={mx:.3e} rms_rel={rms:.3e} | reference bf16 run "
          f"{mx_ref:.3e} {rms_ref:.3e}")
    assert np.isfinite(out).all() and rms <= NET_TOL[dtype] and rms <= rms_ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_contracts_at_56x56(dtype):
    """Graph replay == eager, run-to-run bits, candidate 0 of B = 2 == its B = 1 run (the batch-independence contract)."""
    from wiw_amd.pipeline import SVDDenoiser

    cfg, sd, unet = tiny_manip(dtype)
    rs = np.random.RandomState(9)
    T, h, w = cfg.num_frames, 56, 56
    il = torch.from_numpy(rs.standard_normal((2, 4, h, w)).astype(np.float32))
    ie = torch.from_numpy(rs.standard_normal((2, 1, cfg.cross_attention_dim)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((2, T, 4, h, w)).astype(np.float32))
    acts = _manip_actions(2, T, 9)
    eager, graphed = SVDDenoiser(unet, use_graph=False), SVDDenoiser(unet, use_graph=True)
    a = eager.denoise(il, ie, noise, acts, num_steps=2)
    b = graphed.denoise(il, ie, noise, acts, num_steps=2)
    assert graphed.graph_error is None, graphed.graph_error
    assert torch.equal(a, b), "graph replay differs from the eager loop at 56x56"
    assert torch.equal(a, eager.denoise(il, ie, noise, acts, num_steps=2)), "run-to-run bits differ"
    one = eager.denoise(il[:1], ie[:1], noise[:1], acts[:1], num_steps=2)
    assert torch.equal(a[:1], one), "candidate 0 of B = 2 differs from its B = 1 run"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_denoise_loop_56x56_vs_oracle(dtype):
    from wiw_amd.pipeline import SVDDenoiser

    cfg, sd, unet = tiny_manip(dtype)
    rs = np.random.RandomState(2)
    T, h, w = cfg.num_frames, 56, 56
    il = torch.from_numpy(rs.standard_normal((1, 4, h, w)).astype(np.float32))
    ie = torch.from_numpy(rs.standard_normal((1, 1, cfg.cross_attention_dim)).astype(np.float32))
    noise = torch.from_numpy(rs.standard_normal((1, T, 4, h, w)).astype(np.float32))
    acts = _manip_actions(1, T, 2)
    lat = SVDDenoiser(unet).denoise(il, ie, noise, acts, num_steps=2).cpu()
    with torch.no_grad():
        ref = O.denoise({k: torch.from_numpy(v) for k, v in sd.items()}, cfg.as_dict(), il, ie, noise, acts, num_steps=2)
    rms = float((lat - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"[parity] 2-step loop at 56x56, manipulation, {dtype}: rms_rel={rms:.3e}")
    assert torch.isfinite(lat).all() and rms <= LOOP_TOL[dtype]


def test_served_width_tail_geometry_and_448():
    """The served architecture (320/640/1280/1280 channels) at latent 24x40, 4 frames, against the oracle; then one forward
    at the 448x448 output's 56x56 latent (14 frames): finite and bit-identical on repeat."""
    from wiw_amd.config import UNetConfig
    from wiw_amd.unet import UNetHIP
    from wiw_amd.weights import random_state_dict

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cfg = UNetConfig(num_frames=4, action_input_channel=4)
    sd = random_state_dict(cfg, 8)
    unet = UNetHIP(cfg, sd, DEV, hip=get_hip(torch.bfloat16))
    sample, ehs, tids, _ = _nav_inputs(cfg, 1, 24, 40, seed=4)
    aid = O.action_ids_idx_encode(np.array([[4, 2, 1, 3]]))
    t = 1.0640485
    out = _call(unet, sample, t, ehs, tids, aid).cpu().numpy()
    with torch.no_grad():
        ref = O.unet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, cfg.as_dict(), torch.from_numpy(sample),
                             torch.tensor(t), torch.from_numpy(ehs), torch.from_numpy(tids), torch.from_numpy(aid)).numpy()
    mx, rms = rel(out, ref)
    print(f"[parity] served-width UNet 24x40x4 vs oracle: max_rel={mx:.3e} rms_rel={rms:.3e}")
    assert np.isfinite(out).all() and rms <= NET_TOL[torch.bfloat16]
    del unet, sd
    torch.cuda.empty_cache()
    cfg14 = UNetConfig()
    unet = UNetHIP(cfg14, random_state_dict(cfg14, 8), DEV, hip=get_hip(torch.bfloat16))
    sample, ehs, tids, _ = _nav_inputs(cfg14, 1, 56, 56, seed=5)
    aid = O.action_ids_idx_encode(np.array([[4, 2, 1, 3, 1, 2, 3, 1, 4, 2, 1, 3, 1, 2]]))
    a = _call(unet, sample, t, ehs, tids, aid).cpu()
    b = _call(unet, sample, t, ehs, tids, aid).cpu()
    assert a.shape == (2, 14, 4, 56, 56) and torch.isfinite(a).all() and torch.equal(a, b)
    del unet
    torch.cuda.empty_cache()


def _nav_inputs(cfg, B, h, w, seed):
    rs = np.random.RandomState(seed)
    T = cfg.num_frames
    sample = rs.standard_normal((2 * B, T, 8, h, w)).astype(np.float32)
    ehs = rs.standard_normal((2 * B, 1, cfg.cross_attention_dim)).astype(np.float32)
    ehs[:B] = 0
    sample[:B, :, 4:] = 0
    tids = np.tile(np.array([[6, 127, 0.02]], dtype=np.float32), (2 * B, 1))
    return sample, ehs, tids, None


# ----------------------------------------------------------------------------------------------
# a whole request at 448x448
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,psnr_gate", [(torch.bfloat16, 40.0), (torch.float16, 43.0)], ids=IDS)   # measured 45.8 / 48.5 dB
def test_worker_manipulation_448(tmp_path, dtype, psnr_gate):
    """wire request -> SVDWorker(width = height = 448, task_type 'manipulation') with the HIP denoiser and the HIP frontend
    (VAE + CLIP kernels), tiny weights -> uint8 (1, 14, 3, 480, 480); against the CPU chain (fp32 frontend + oracle loop)
    on the same noise draws."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    import vae_oracle as VO
    from wiw_amd import frontend as FE
    from wiw_amd.pipeline import SVDDenoiser
    from wiw_amd.server import plumbing as P
    from wiw_amd.server.worker import SVDWorker
    from wiw_amd.unet import UNetHIP
    from wiw_amd.vae import HIPFrontend, VAEHIP
    from wiw_amd.weights import random_state_dict

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    T, H, W = 14, 448, 448
    cfg = manip_cfg(T)
    sd = random_state_dict(cfg, 21)
    hip = get_hip(dtype)
    den = SVDDenoiser(UNetHIP(cfg, sd, DEV, dtype=dtype, hip=hip))
    vcfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
    vsd = FE.vae_random_state_dict(22, **vcfg)
    torch.manual_seed(0)
    clip = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1,
                                                          num_attention_heads=2, image_size=224, patch_size=32,
                                                          projection_dim=1024, hidden_act="gelu")).eval()
    fe = HIPFrontend(VAEHIP(vsd, DEV, hip=hip, **vcfg), clip, clip="hip")

    def denoise(il, ie, nz, act, **kw):
        return den.denoise(torch.as_tensor(il), torch.as_tensor(ie), torch.as_tensor(nz), act, **kw).cpu().numpy()

    draws = []

    def noise_fn(shape):
        rs = np.random.RandomState(100 + len(draws))
        draws.append(rs.standard_normal(shape).astype(np.float32))
        return draws[-1]

    worker = SVDWorker(denoise, fe, width=W, height=H, out_width=480, out_height=480, num_frames=T, num_inference_steps=2,
                       noise_fn=noise_fn, task_type="manipulation")
    rs = np.random.RandomState(0)
    acts = _manip_actions(1, T, 0)
    req = {"b_action": acts.tolist(), "save_dirs": [str(tmp_path / "a")], "request_model_name": "igen",
           "b_image": rs.randint(0, 256, size=(1, 3, 480, 640), dtype=np.uint8), "return_objects": [True]}
    P.validate_request(req, T, "manipulation")
    out = worker(req)
    pf = out["pred_frames"]
    assert pf.shape == (1, T, 3, 480, 480) and pf.dtype == np.uint8

    fe_cpu = VO.TorchFrontend(vsd, clip, device="cpu", vae_dtype=torch.float32, dtype=torch.float32, **vcfg)
    _, _, _, images = P.parse_request(req)
    x = np.stack([P.preprocess_image(im, W, H) for im in images])
    il, ie = fe_cpu.encode(x, draws[0], 0.02)
    with torch.no_grad():
        lat = O.denoise({k: torch.from_numpy(v) for k, v in sd.items()}, cfg.as_dict(), torch.from_numpy(il),
                        torch.from_numpy(ie), torch.from_numpy(draws[1]), acts, num_steps=2).numpy()
    frames = fe_cpu.decode(lat)
    ref = P.build_response(P.images_to_tensor([P.frames_to_pil(f) for f in frames], save_size=(480, 480)),
                           acts, req["save_dirs"], True)["pred_frames"]
    diff = np.abs(pf.astype(np.int32) - ref.astype(np.int32))
    mse = float((diff.astype(np.float64) ** 2).mean())
    psnr = 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))
    print(f"[parity] 448x448 manipulation request, {dtype}: mean|diff|={diff.mean():.3f} levels, max={diff.max()}, "
          f"PSNR={psnr:.1f} dB")
    assert psnr > psnr_gate
