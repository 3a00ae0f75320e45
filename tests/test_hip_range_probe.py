"""The range probe (`range.RangeProbe` as `Hip.range_probe`) on the GPU, at the tiny geometry of tests/test_hip_finite_guard.py:
a probed run computes the unprobed run's bytes; every launching entry point a probed run calls leaves a record or is excluded
with a reason; an overflowing checkpoint is located (the lowest-headroom record is the overflowing convolution's scope, with
n_inf > 0); a capture with the probe set is refused."""
import os
import re

import numpy as np
import pytest
import torch

from test_hip_finite_guard import B, DEV, H, T, UNET_CONV, VCFG, W, scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launching entry points a probed run calls that leave NO record, and why
EXCLUDED = {
    "wiw_range_stats": "the probe's own launches",
    "wiw_groupnorm_stats": "scratch only: per-block sums for the apply launch, whose output is recorded",
    "wiw_groupnorm_stats_f32in": "scratch only: per-block sums for the apply launch, whose output is recorded",
    "wiw_transpose_bf16": "a transpose of recorded data (V^T of a recorded q|k|v tensor)",
    "wiw_transpose_framepad_bf16": "a transpose of recorded data, zero-padded",
    "wiw_prep_unet_input": "the sampler's launch between forwards, not a forward's: `Hip.prep_unet_input` carries no probe hook",
    "wiw_emb_combine": "the sampler's time embedding between forwards: `Hip.emb_combine` carries no probe hook",
    "wiw_cfg_euler_step": "the sampler's fp32 latents, not an activation of a forward (the serving guard checks them)",
}


@pytest.fixture(scope="module")
def env():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    import wiw_amd  # noqa: F401
    from wiw_amd import frontend as FE
    from wiw_amd.config import UNetConfig
    from wiw_amd.weights import random_state_dict

    cfg = UNetConfig.tiny(T)
    sd = random_state_dict(cfg, 21)
    torch.manual_seed(0)
    clip = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                                          num_attention_heads=2, image_size=224, patch_size=32,
                                                          projection_dim=1024, hidden_act="gelu")).eval()
    rs = np.random.RandomState(3)
    h, w = H // 8, W // 8
    inputs = dict(images=rs.uniform(-1, 1, size=(B, 3, H, W)).astype(np.float32),
                  img_noise=rs.standard_normal((B, 3, H, W)).astype(np.float32),
                  noise=torch.from_numpy(rs.standard_normal((B, T, 4, h, w)).astype(np.float32)),
                  acts=np.array([[4, 2, 1, 3], [4, 1, 3, 3]], dtype=np.int64))
    return dict(cfg=cfg, sd=sd, vsd=FE.vae_random_state_dict(22, **VCFG), clip=clip, **inputs)


def build(env, sd):
    from wiw_amd.pipeline import SVDDenoiser
    from wiw_amd.unet import UNetHIP
    from wiw_amd.vae import HIPFrontend, VAEHIP

    net = UNetHIP(env["cfg"], sd, DEV, dtype=torch.float16, residual_fp32=True)
    fe = HIPFrontend(VAEHIP(env["vsd"], DEV, hip=net.hip, **VCFG), env["clip"], dtype=torch.float16, device_io=True)
    return net, SVDDenoiser(net, use_graph=False), fe


def run(env, den, fe, steps=2):
    """CLIP + VAE encode, `steps` Euler steps, VAE decode: every tensor that leaves a stage."""
    il, ie = fe.encode(env["images"], env["img_noise"], 0.02)
    lat = den.denoise(il, ie, env["noise"], env["acts"], num_steps=steps)
    frames = fe.vae.decode(lat)
    torch.cuda.synchronize()
    return il.clone(), ie.clone(), lat.clone(), frames


def test_probed_run_is_bit_identical_and_covers_what_it_launches(env):
    from wiw_amd import hip as HM
    from wiw_amd.range import RangeProbe

    net, den, fe = build(env, env["sd"])
    plain = run(env, den, fe)
    lib, called = net.hip.lib, []
    names = [n for table in (HM.EXPORTS, HM.EXPORTS_RESAMPLE, HM.EXPORTS_METRICS, HM.EXPORTS_RANGE) for n in table]
    real = {n: getattr(lib, n) for n in names}
    for n in names:
        setattr(lib, n, (lambda f, n: lambda *a: (called.append(n), f(*a))[1])(real[n], n))
    probe = RangeProbe()
    net.hip.range_probe = probe
    try:
        probed = run(env, den, fe)
        records = probe.records()
    finally:
        net.hip.range_probe = None
        for n in names:
            setattr(lib, n, real[n])
    for a, b, what in zip(plain, probed, ("image latents", "CLIP embeddings", "latents", "frames")):
        assert torch.equal(a, b), f"{what} differ with the probe attached"
    assert run(env, den, fe)[2].equal(plain[2])                                         # and it detaches cleanly
    # every record is complete and finite on healthy weights
    assert len(records) > 100 and all(r["n_nan"] + r["n_inf"] == 0 and r["headroom"] > 1 for r in records)
    scopes = {r["scope"] for r in records}
    assert {"unet", "mid_block.resnets.0", "down_blocks.0.attentions.0", "vae.decoder", "vae.encoder", "clip",
            "decoder.mid_block.resnets.0.spatial_res_block", "encoder.mid_block.attentions.0"} <= scopes, sorted(scopes)
    for r in records:
        assert r["hist"].sum() + r["n_zero"] == int(np.prod(r["shape"])) and r["dtype"] in ("float16", "float32")
    per_scope = {}
    for r in records[:200]:          # ordinals count up per scope, across forwards
        assert r["ordinal"] == per_scope.get(r["scope"], 0)
        per_scope[r["scope"]] = r["ordinal"] + 1
    # the coverage rule
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("wiw_svd.h", "wiw_resample.h", "wiw_metrics.h", "wiw_range.h"))
    launching = set(re.findall(r"^int\s+(wiw_\w+)\s*\(\s*void\s*\*\s*stream", headers, flags=re.M))
    assert {"wiw_gemm_bf16", "wiw_range_stats", "wiw_groupnorm_stats"} <= launching
    ran = set(called) & launching
    print(f"[range probe] {len(records)} records from {sorted(probe.entry_points)}; launched and excluded: {sorted(ran - probe.entry_points)}")
    assert probe.entry_points <= ran
    missing = ran - probe.entry_points - set(EXCLUDED)
    assert not missing, f"launching entry points of the probed run without a record or an exclusion: {sorted(missing)}"
    assert len(probe.entry_points) >= 10


def test_overflowing_checkpoint_is_located(env):
    from wiw_amd.range import RangeProbe

    net, den, fe = build(env, scaled(env["sd"], UNET_CONV))
    probe = RangeProbe()
    net.hip.range_probe = probe
    try:
        il, ie = fe.encode(env["images"], env["img_noise"], 0.02)
        den.denoise(il, ie, env["noise"], env["acts"], num_steps=1)
        records = probe.records()
    finally:
        net.hip.range_probe = None
    first = min(range(len(records)), key=lambda i: (records[i]["headroom"], i))
    r = records[first]
    print(f"[range probe] lowest headroom: {r['scope']}#{r['ordinal']} {r['family']} {r['shape']} absmax {r['absmax']} n_inf {r['n_inf']}")
    assert r["scope"] == "mid_block.resnets.0" and r["n_inf"] > 0 and r["headroom"] == 0.0 and r["family"] == "gemm"
    assert all(q["n_inf"] + q["n_nan"] == 0 for q in records[:first])                  # nothing before it is bad


def test_a_capture_with_the_probe_set_is_refused(env):
    from wiw_amd.pipeline import GraphedForward, SVDDenoiser, action_ids_idx_encode
    from wiw_amd.range import RangeProbe

    net, den, fe = build(env, env["sd"])
    il, ie = fe.encode(env["images"], env["img_noise"], 0.02)
    cond = net.prepare_request(ie, action_ids_idx_encode(env["acts"]), 0.02)
    net.hip.range_probe = RangeProbe()
    try:
        with pytest.raises(RuntimeError, match="range probe"):
            GraphedForward(net, cond, H // 8, W // 8)
        graphed = SVDDenoiser(net, use_graph=True)                                      # the sampler then runs that shape eagerly
        lat = graphed.denoise(il, ie, env["noise"], env["acts"], num_steps=1)
        assert not graphed._graphs and "range probe" in graphed.graph_error
    finally:
        net.hip.range_probe = None
    assert torch.equal(lat, den.denoise(il, ie, env["noise"], env["acts"], num_steps=1))
