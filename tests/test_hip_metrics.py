"""Per-plane SSIM / squared error on the device (csrc/metrics.hip, include/wiw_metrics.h) against the reference's own functions
(tests/golden/video_metrics.npz), both library builds.  Tolerances: tests/metrics_fixtures.py — SSIM 1e-10 absolute, PSNR 1e-5 dB,
the same on aggregates; none comes from the kernel.  Inputs and references are shared and never modified."""
import numpy as np
import pytest
import torch

import metrics_fixtures as MF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_HIPS = {}
# operand forms (a, b).  The pair that is not uint8-derived exists as fp32 only.
FORMS = [("f32", "f32"), ("f32", "u8"), ("u8", "u8")]
PAIR_FORMS = [(n, f) for n in MF.PAIRS for f in FORMS if MF.pair(n)[0].dtype == np.uint8 or f == ("f32", "f32")]


def hip_for(name):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    if name not in _HIPS:
        _HIPS[name] = Hip(torch.device(DEV), DTYPES[name])
    return _HIPS[name]


def operand(x, form):
    """A stored plane (or stack of planes) as the device tensor of one operand form."""
    if form == "u8":
        assert x.dtype == np.uint8
        return torch.from_numpy(x.copy()).to(DEV)
    return torch.from_numpy(np.array(MF.as_f32(x), np.float32)).to(DEV)


def strided(t, gap=3, pad=2):
    """The same planes (N, H, W) inside a larger allocation: `gap` unused columns per row, `pad` unused rows per plane, filled
    with a value that would show (255 / 7.5: outside [0, 1] for fp32)."""
    N, H, W = t.shape
    big = torch.full((N, H + pad, W + gap), 255 if t.dtype == torch.uint8 else 7.5, dtype=t.dtype, device=t.device)
    big[:, :H, :W] = t
    v = big[:, :H, :W]
    assert not v.is_contiguous() and v.stride() == ((H + pad) * (W + gap), W + gap, 1)
    return v


def check_pair(got, name, what):
    a, _, ssim, psnr = MF.pair(name)
    got = got.cpu().numpy()
    assert got.shape == (1, 2) and got.dtype == np.float64
    got_psnr = MF.psnr_of(float(got[0, 1]), a.size)
    print(f"[metrics] {what}: ssim {got[0, 0]:+.15f} (ref {ssim:+.15f}, diff {abs(got[0, 0] - ssim):.3e}), "
          f"psnr {got_psnr:.9f} dB (ref {psnr:.9f}, diff {abs(got_psnr - psnr):.3e})")
    assert abs(got[0, 0] - ssim) <= MF.SSIM_TOL
    assert abs(got_psnr - psnr) <= MF.PSNR_TOL
    return got


@pytest.mark.parametrize("lib", ["bf16", "fp16"])
@pytest.mark.parametrize("name,form", PAIR_FORMS, ids=[f"{n}-{fa}-{fb}" for n, (fa, fb) in PAIR_FORMS])
def test_fixture_pair(name, form, lib):
    hip = hip_for(lib)
    a, b, _, _ = MF.pair(name)
    ta, tb = operand(a[None], form[0]), operand(b[None], form[1])
    dense = hip.frame_metrics(ta, tb)
    gapped = hip.frame_metrics(strided(ta), strided(tb, gap=5, pad=1))
    torch.cuda.synchronize()
    d = check_pair(dense, name, f"{name} {form} [{lib}] dense")
    s = check_pair(gapped, name, f"{name} {form} [{lib}] strided")
    assert np.array_equal(d.view(np.uint64), s.view(np.uint64))          # the strides change addresses, not arithmetic


@pytest.mark.parametrize("lib", ["bf16", "fp16"])
@pytest.mark.parametrize("form", FORMS, ids=["f32-f32", "f32-u8", "u8-u8"])
def test_identical_pair_is_100_db_and_ssim_one(form, lib):
    hip = hip_for(lib)
    a, b, _, _ = MF.pair("identical_33x47")
    got = hip.frame_metrics(operand(a[None], form[0]), operand(b[None], form[1])).cpu().numpy()
    assert got[0, 1] == 0.0 and MF.psnr_of(float(got[0, 1]), a.size) == 100.0
    assert abs(got[0, 0] - 1.0) <= 1e-12


@pytest.mark.parametrize("lib", ["bf16", "fp16"])
def test_batch_equals_single_planes_and_repeats(lib):
    """Seven planes of 61 x 100 (2 x 3 tiles of the valid region, the last of each partial) in one launch, fp32 against uint8:
    bit-equal to the planes one at a time, to a second run, and within the tolerances of the restatement."""
    hip = hip_for(lib)
    rs = np.random.RandomState(5)
    base = rs.randint(0, 256, size=(7, 61, 100)).astype(np.uint8)
    other = np.clip(base.astype(np.int64) + rs.randint(-9, 10, size=base.shape), 0, 255).astype(np.uint8)
    a, b = operand(base, "f32"), operand(other, "u8")
    together = hip.frame_metrics(a, b)
    again = hip.frame_metrics(a, b)
    single = torch.cat([hip.frame_metrics(a[i:i + 1], b[i:i + 1]) for i in range(7)])
    tail = hip.frame_metrics(a[4:], b[4:])
    torch.cuda.synchronize()
    assert torch.equal(together.view(torch.int64), again.view(torch.int64))
    assert torch.equal(together.view(torch.int64), single.view(torch.int64))
    assert torch.equal(together[4:].view(torch.int64), tail.view(torch.int64))
    ref = MF.planes_metrics(base, other)
    got = together.cpu().numpy()
    d_ssim = np.abs(got[:, 0] - ref[:, 0]).max()
    d_psnr = max(abs(MF.psnr_of(g, 61 * 100) - MF.psnr_of(r, 61 * 100)) for g, r in zip(got[:, 1], ref[:, 1]))
    print(f"[metrics] 7 x 61 x 100 [{lib}]: max |ssim - restatement| = {d_ssim:.3e}, max |psnr - restatement| = {d_psnr:.3e} dB")
    assert d_ssim <= MF.SSIM_TOL and d_psnr <= MF.PSNR_TOL


def test_planes_below_the_window_are_refused():
    hip = hip_for("bf16")
    x = torch.zeros(1, 10, 64, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="at least 11"):
        hip.frame_metrics(x, x)
    torch.cuda.synchronize()


@pytest.mark.parametrize("only_final", [True, False], ids=["final", "frames"])
def test_evaluate_video_metrics_on_the_fixture_video(only_final):
    import wiw_amd  # noqa: F401
    from wiw_amd.metrics import evaluate_video_metrics, frame_scores

    hip, g = hip_for("bf16"), MF.golden()
    gt = torch.from_numpy(MF.LUT[g["video__gt"]])                      # fp32 on the host, as a data loader hands it over
    gen = torch.from_numpy(g["video__gen"].copy()).to(DEV)            # uint8 on the device, as the quantised decode is
    got = evaluate_video_metrics(gt, gen, only_final=only_final, hip=hip)
    assert sorted(got) == ["psnr", "ssim"]
    tag = "final" if only_final else "frames"
    for metric, tol in (("ssim", MF.SSIM_TOL), ("psnr", MF.PSNR_TOL)):
        for key, stored in (("value", "value"), ("value_std", "std")):
            ref = g[f"video__{metric}__{tag}__{stored}"]
            d = np.abs(np.asarray(got[metric][key]) - ref)
            print(f"[metrics] video {metric} {tag} {key}: max |got - ref| = {d.max():.3e}")
            assert len(got[metric][key]) == len(ref) and (d <= tol).all()
    ssim, psnr = frame_scores(hip, gt, gen)
    assert np.abs(ssim - g["video__ssim"]).max() <= MF.SSIM_TOL and np.abs(psnr - g["video__psnr"]).max() <= MF.PSNR_TOL


class FixedFrontend:
    """`decode` returns the same fp32 frames (1, T, 3, H, W) in about [-1.1, 1.1] whatever the latents are."""

    def __init__(self, T=4, H=24, W=40):
        rs = np.random.RandomState(9)
        y, x = np.mgrid[0:H, 0:W]
        base = np.sin(0.21 * y + 0.13 * x)[None, None, None] * rs.uniform(0.5, 1.0, size=(1, T, 3, 1, 1))
        self.frames = (base + rs.uniform(-0.15, 0.15, size=(1, T, 3, H, W))).astype(np.float32)
        self.calls = 0

    def decode(self, latents):
        self.calls += 1
        assert isinstance(latents, np.ndarray)
        return self.frames.copy()


def test_trainer_validate_frame_metrics(golden):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import Trainer, UNetTrain
    from wiw_amd.vae import frames_to_uint8_device
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_tiny.npz")
    cfg = UNetConfig.tiny(4)
    hip = hip_for("bf16")
    sd = random_state_dict(cfg, int(g["weight_seed"]))
    rs = np.random.RandomState(3)
    h, w = g["latents"].shape[-2:]
    fe = FixedFrontend()
    samples = [dict(image_latents=torch.from_numpy(rs.standard_normal((1, 4, h, w)).astype(np.float32)),
                    image_embeddings=torch.from_numpy(rs.standard_normal((1, 1, cfg.cross_attention_dim)).astype(np.float32)),
                    noise=torch.from_numpy(rs.standard_normal((1, 4, 4, h, w)).astype(np.float32)),
                    actions=np.array([[4, 1, 2, 3]]),
                    target_latents=torch.from_numpy(rs.standard_normal((1, 4, 4, h, w)).astype(np.float32)),
                    target_frames=torch.from_numpy(MF.LUT[rs.randint(0, 256, size=(1, 4, 3, 24, 40)).astype(np.uint8)]))
               for _ in range(2)]
    tr = Trainer(UNetTrain(cfg, sd, DEV, hip=hip), lr=1e-3)
    plain = tr.validate(samples, num_steps=2, frontend=fe)
    assert sorted(plain) == ["clips", "global_step", "latent_mse", "latent_psnr", "psnr", "weights"]          # today's record
    rich = tr.validate(samples, num_steps=2, frontend=fe, frame_metrics=True)
    assert sorted(rich) == sorted(list(plain) + ["ssim", "ssim_std", "frame_psnr", "frame_psnr_std"])
    assert all(rich[k] == plain[k] for k in plain) and fe.calls == 4
    # the new keys: the restatement on the same quantised frames (the quantisation is elementwise fp32: the host gives the same bytes)
    q = frames_to_uint8_device(torch.from_numpy(fe.frames[0])).permute(0, 3, 1, 2).numpy()[None]
    assert q.dtype == np.uint8 and q.shape == (1, 4, 3, 24, 40) and q.min() == 0 and q.max() == 255
    ssim, psnr = [], []
    for s in samples:
        fs, fp = MF.frame_scores(s["target_frames"].numpy(), q)
        ssim.append(fs.reshape(-1)); psnr.append(fp.reshape(-1))
    ssim, psnr = np.concatenate(ssim), np.concatenate(psnr)
    want = {"ssim": ssim.mean(), "ssim_std": ssim.std(), "frame_psnr": psnr.mean(), "frame_psnr_std": psnr.std()}
    for k, tol in (("ssim", MF.SSIM_TOL), ("ssim_std", MF.SSIM_TOL), ("frame_psnr", MF.PSNR_TOL), ("frame_psnr_std", MF.PSNR_TOL)):
        print(f"[metrics] validate {k}: {rich[k]:.12f} (restatement {want[k]:.12f}, diff {abs(rich[k] - want[k]):.3e})")
        assert abs(rich[k] - want[k]) <= tol
    assert want["ssim_std"] > 0 and want["frame_psnr_std"] > 0
