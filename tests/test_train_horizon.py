"""Fine-tuning at every served horizon (17 .. 32 frames, 25 = SVD-XT) — CPU side.

  * the two tapes' frame limits and `make_unet_train`'s choice between them;
  * `oracle/train_oracle.training_step` (unchanged, generic in T) against the reference's own `loss.backward()` at 25 and 17
    frames: tests/golden/train_step_horizon.npz, written by tools/make_golden_train_horizon.py.  Tolerances as
    tests/test_train_oracle.py (fp32 summation order only);
  * `train.batch_from_pixels` at 25 frames on a CPU stand-in for the HIP front end.
"""
import time

import numpy as np
import pytest
import torch

import svd_oracle as O
import train_oracle as TO

from test_train_any_size import _draws, _front

INPUTS = ("latents", "noise", "conditional_latents", "encoder_hidden_states")
NAME = "train_step_horizon.npz"
PREFIXES = ("t25__", "t17__", "full__")


def horizon_config(pre):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig

    t25 = UNetConfig.tiny(25)
    if pre == "t25__":
        return t25
    if pre == "t17__":
        return UNetConfig(block_out_channels=t25.block_out_channels, num_attention_heads=t25.num_attention_heads, num_frames=17,
                          action_input_channel=10, task_type="manipulation")
    return UNetConfig(num_frames=25, action_input_channel=25)


def horizon_inputs(g, pre):
    """The fp32 inputs of one scenario, re-drawn from the stored seed as tools/make_golden_train_tails.py `draw_inputs` draws
    them (RandomState's stream is frozen; values rounded to bf16) and checked against the stored checksums."""
    (h, w), T, ctx = (int(v) for v in g[f"{pre}latent_hw"]), int(g[f"{pre}num_frames"]), 1024
    rs = np.random.RandomState(int(g[f"{pre}input_seed"]))
    draw = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))  # noqa: E731
    inp = {"latents": draw(1, T, 4, h, w) * 0.8, "noise": draw(1, T, 4, h, w), "conditional_latents": draw(1, 4, h, w),
           "encoder_hidden_states": draw(1, 1, ctx)}
    inp = {k: v.to(torch.bfloat16).float() for k, v in inp.items()}
    sums = np.array([[float(inp[k].double().sum()), float(inp[k].double().pow(2).sum())] for k in INPUTS])
    assert np.array_equal(sums, g[f"{pre}input_checksums"]), "the re-drawn inputs are not the generator's"
    return inp


def is_dead(n):
    return ("transformer_blocks.0.norm2." in n) or (".attn2.to_q." in n) or (".attn2.to_k." in n) or n.startswith("add_embedding.")


def test_frame_limits_and_tape_choice():
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import TRAIN_MAX_FRAMES, UNetTrain, UNetTrain32, make_unet_train
    from wiw_amd.unet import MAX_NUM_FRAMES

    assert TRAIN_MAX_FRAMES == 16 and UNetTrain.MAX_FRAMES == 16 and UNetTrain32.MAX_FRAMES == MAX_NUM_FRAMES == 32
    with pytest.raises(ValueError, match="32"):
        UNetTrain32(UNetConfig.tiny(33), {}, "cpu")
    with pytest.raises(ValueError, match="32"):
        make_unet_train(UNetConfig.tiny(33), {}, "cpu")
    with pytest.raises(ValueError, match="at most 16.*UNetTrain32"):
        UNetTrain(UNetConfig.tiny(17), {}, "cpu")

    class NoHip:                      # the constructors need a Hip only for its dtype: nothing is launched on the CPU
        dtype = torch.bfloat16

    for n in (1, 14, 16):
        assert type(make_unet_train(UNetConfig.tiny(n), {}, "cpu", hip=NoHip())) is UNetTrain
    for n in (17, 25, 32):
        net = make_unet_train(UNetConfig.tiny(n), {}, "cpu", hip=NoHip())
        assert type(net) is UNetTrain32 and isinstance(net, UNetTrain) and net.cfg.num_frames == n
    assert type(UNetTrain32(UNetConfig.tiny(4), {}, "cpu", hip=NoHip())) is UNetTrain32       # 1 .. 32, not only 17 .. 32


def test_horizon_fixture_inputs_redraw_and_file_size(golden):
    import os

    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, NAME)) < (1 << 20)
    g = golden(NAME)
    for pre, T, hw, ch in (("t25__", 25, (16, 32), 25), ("t17__", 17, (16, 16), 10), ("full__", 25, (8, 16), 25)):
        x = horizon_inputs(g, pre)
        assert tuple(x["latents"].shape) == (1, T, 4, *hw) and tuple(g[f"{pre}model_pred"].shape) == (1, T, 4, *hw)
        assert tuple(g[f"{pre}action_ids"].shape) == (1, T, ch)
        cfg = horizon_config(pre)
        assert (cfg.num_frames, cfg.action_input_channel) == (T, ch)
    assert "t25__loss_ref_bf16" in g.files and "t17__loss_ref_bf16" in g.files and "full__loss_ref_bf16" not in g.files


@pytest.mark.parametrize("pre", PREFIXES)
def test_oracle_training_step_matches_reference_at_long_horizons(golden, pre):
    """The oracle's step against the reference's autograd at 25 frames (navigation, 25 action channels), 17 frames
    (manipulation, 10 channels) and at the served width with 25 frames: loss, prediction, every gradient norm, the stored
    gradients.  (The served-width step takes about ten seconds on eight CPU threads: it is checked in full.)"""
    import wiw_amd  # noqa: F401
    from wiw_amd.pipeline import manip_action_ids
    from wiw_amd.weights import random_state_dict

    g = golden(NAME)
    cfg = horizon_config(pre)
    sd = {k: torch.from_numpy(v) for k, v in random_state_dict(cfg, int(g["weight_seed"])).items()}
    torch.set_num_threads(8)
    ids = manip_action_ids(g[f"{pre}actions"]) if cfg.task_type == "manipulation" else O.action_ids_idx_encode(g[f"{pre}actions"])
    aid = torch.from_numpy(np.asarray(ids)).float()
    assert float((aid - torch.from_numpy(g[f"{pre}action_ids"])).abs().max()) <= 1e-5
    x = horizon_inputs(g, pre)
    t0 = time.perf_counter()
    loss, pred, grads = TO.training_step(
        sd, cfg.as_dict(), x["latents"], x["noise"], torch.from_numpy(g[f"{pre}sigmas"]), x["conditional_latents"],
        x["encoder_hidden_states"], float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]),
        dropout_prob=float(g["dropout_prob"]), random_p=torch.from_numpy(g["random_p"]))
    print(f"[horizon oracle {pre}] step in {time.perf_counter() - t0:.1f} s")
    ref_loss = float(g[f"{pre}loss"])
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    ref = torch.from_numpy(g[f"{pre}model_pred"])
    assert float((pred - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    names, norms = [str(n) for n in g[f"{pre}grad_names"]], g[f"{pre}grad_norms"]
    assert set(names) <= set(grads)
    med = float(np.median(norms[norms > 0]))
    worst, dead = 0.0, 0
    for n, nr in zip(names, norms):
        gn = 0.0 if grads[n] is None else float(grads[n].double().norm())
        if is_dead(n):
            assert gn == 0.0 and nr <= 1e-3 * med, (n, gn, nr)
            dead += 1
        else:
            assert nr > 0, n
            worst = max(worst, max(abs(gn - nr) - 1e-9, 0.0) / nr)
    print(f"[horizon oracle {pre}] {len(names)} gradient norms ({dead} dead), worst relative deviation of the live ones {worst:.2e}")
    assert dead == sum(is_dead(n) for n in sd) and dead >= 132 and worst <= 1e-3
    n_full = 0
    for key in g.files:
        if key.startswith(f"{pre}grad__") or key.startswith(f"{pre}grad8__"):
            name = key[len(pre):].split("__", 1)[1].replace("__", ".")
            r = torch.from_numpy(g[key])
            mine = grads[name] if key.startswith(f"{pre}grad__") else grads[name].reshape(grads[name].shape[0], -1)[:8, :r.shape[1]]
            assert float((mine.reshape(r.shape) - r).abs().max()) <= 2e-4 * float(r.abs().max()) + 1e-12, name
            n_full += 1
    assert n_full >= 15


def _poses(Tn, seed):
    from wiw_amd.pipeline import SCENE_BOUNDS

    rs = np.random.RandomState(seed)
    poses = np.zeros((1, Tn, 8), dtype=np.float32)
    poses[..., :3] = SCENE_BOUNDS[:3] + (SCENE_BOUNDS[3:] - SCENE_BOUNDS[:3]) * rs.uniform(0.1, 0.9, size=(1, Tn, 3))
    poses[..., 3:7] = rs.standard_normal((1, Tn, 4))
    poses[..., 7] = rs.choice([0.0, 1.0], size=(1, Tn))
    return poses


def test_batch_from_pixels_at_25_frames():
    """T = 25 through the host logic: the VAE sample of 25 frames, (1, 25) navigation ids -> the (1, 25, 25) cumulative matrix
    and the rotated noise; (1, 25, 8) poses -> 10 channels (or the positional 25 + 9) and the noise draw as it is."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.pipeline import action_encode_positional, action_ids_idx_encode, manip_action_ids, rotate_latent_noise

    g = torch.Generator().manual_seed(7)
    Tn, H, W = 25, 16, 128
    px = torch.tanh(torch.randn(1, Tn, 3, H, W, generator=g))
    past = torch.tanh(torch.randn(1, 1, 3, H, W, generator=g))
    d = _draws(g, Tn, H, W)
    front = _front((1, 3, H, W))
    m, lv = front.vae.encode_moments(px[0])
    lat = ((m + torch.exp(0.5 * lv) * d["vae_eps"]) * 0.18215)[None]
    assert tuple(lat.shape) == (1, Tn, 4, H // 8, W // 8)
    # navigation
    acts = np.array([[4] + [[1, 2, 1, 3][i % 4] for i in range(Tn - 1)]])
    st = T.batch_from_pixels(front, px, past, acts, dropout_prob=0.1, draws=d, action_input_channel=Tn)
    assert st.unet_input.shape == (1, Tn, 8, H // 8, W // 8) and st.target.shape == st.noisy.shape == (1, Tn, 4, H // 8, W // 8)
    assert st.ehs.shape == (1, 1, 1024) and st.added_time_ids.shape == (1, 3)
    assert st.action_ids.shape == (1, Tn, Tn) and torch.equal(st.action_ids, torch.from_numpy(action_ids_idx_encode(acts)))
    noise = rotate_latent_noise(d["latent_noise"], acts)
    assert not torch.equal(noise, d["latent_noise"])
    assert torch.allclose(st.target, lat, atol=1e-6) and torch.allclose(st.noisy, lat + 0.8 * noise, atol=1e-6)
    # manipulation: 10 channels, and the positional form at T + 9 = 34
    poses = _poses(Tn, 3)
    ids = manip_action_ids(poses)
    mp = T.batch_from_pixels(front, px, past, poses, dropout_prob=0.1, draws=d)
    assert mp.action_ids.shape == (1, Tn, 10) and torch.equal(mp.action_ids, torch.from_numpy(ids))
    assert torch.allclose(mp.noisy, lat + 0.8 * d["latent_noise"], atol=1e-6)                      # the draw itself: no rotation
    pos = T.batch_from_pixels(front, px, past, poses, dropout_prob=0.1, draws=d, action_input_channel=Tn + 9)
    assert pos.action_ids.shape == (1, Tn, Tn + 9) and torch.equal(pos.action_ids, torch.from_numpy(action_encode_positional(ids)))
    assert torch.equal(pos.noisy, mp.noisy)
    with pytest.raises(ValueError, match=r"10.*34|34.*10"):
        T.batch_from_pixels(front, px, past, poses, draws=d, action_input_channel=25)
