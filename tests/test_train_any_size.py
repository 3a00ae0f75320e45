"""Fine-tuning at every served latent size — CPU side.

  * the dispatch predicate of the training graph's spatial self-attention (`train_unet.attn_padded_rows`): which levels of a
    latent take the padded form (S % 16 != 0) and with which row stride;
  * `train.batch_from_pixels` with (1, T, 8) manipulation actions on a CPU stand-in for the HIP front end;
  * `oracle/train_oracle.training_step` against the reference's own `loss.backward()` at 24x40 (navigation) and 56x56
    (manipulation, 10 action channels): tests/golden/train_step_tails.npz, written by tools/make_golden_train_tails.py.
    Tolerances as tests/test_train_oracle.py (fp32 summation order only).
"""
import numpy as np
import pytest
import torch

import svd_oracle as O
import train_oracle as TO

INPUTS = ("latents", "noise", "conditional_latents", "encoder_hidden_states")


def tails_inputs(g, pre):
    """The fp32 inputs of one scenario, re-drawn from the stored seed exactly as tools/make_golden_train_tails.py `draw_inputs`
    draws them (RandomState's stream is frozen; values rounded to bf16) and checked against the stored checksums."""
    (h, w), T, ctx = (int(v) for v in g[f"{pre}latent_hw"]), 4, 1024
    rs = np.random.RandomState(int(g[f"{pre}input_seed"]))
    draw = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))  # noqa: E731
    inp = {"latents": draw(1, T, 4, h, w) * 0.8, "noise": draw(1, T, 4, h, w), "conditional_latents": draw(1, 4, h, w),
           "encoder_hidden_states": draw(1, 1, ctx)}
    inp = {k: v.to(torch.bfloat16).float() for k, v in inp.items()}
    sums = np.array([[float(inp[k].double().sum()), float(inp[k].double().pow(2).sum())] for k in INPUTS])
    assert np.array_equal(sums, g[f"{pre}input_checksums"]), "the re-drawn inputs are not the generator's"
    return inp


def tails_config(pre):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig

    tiny = UNetConfig.tiny(4)
    if pre == "nav__":
        return tiny
    if pre == "manip__":
        return UNetConfig(block_out_channels=tiny.block_out_channels, num_attention_heads=tiny.num_attention_heads, num_frames=4,
                          action_input_channel=10, task_type="manipulation")
    return UNetConfig(num_frames=4, action_input_channel=10, task_type="manipulation")


def test_attention_dispatch_predicate():
    import wiw_amd  # noqa: F401
    from wiw_amd.train_unet import attn_level_plan, attn_padded_rows

    assert attn_level_plan(72, 128) == [(9216, 0), (2304, 0), (576, 0), (144, 0)]          # 576 x 1024: today's launches everywhere
    assert attn_level_plan(32, 64) == [(2048, 0), (512, 0), (128, 0), (32, 0)]
    assert attn_level_plan(56, 56) == [(3136, 0), (784, 0), (196, 208), (49, 64)]          # 448 x 448: the two inner levels
    assert attn_level_plan(24, 40) == [(960, 0), (240, 0), (60, 64), (15, 16)]
    assert attn_level_plan(24, 24) == [(576, 0), (144, 0), (36, 48), (9, 16)]
    for S in range(1, 400):
        Sp = attn_padded_rows(S)
        assert (Sp == 0) == (S % 16 == 0)
        assert Sp == 0 or (Sp % 16 == 0 and S < Sp < S + 16)


def _front(embed_shape):
    import vae_oracle as VO
    from wiw_amd import frontend as FE

    cfg = dict(block_out_channels=(32, 32, 64, 64), layers_per_block=1)
    sd = {k: torch.from_numpy(v) for k, v in FE.vae_random_state_dict(3, **cfg).items()}

    class Vae:
        device, scaling_factor = torch.device("cpu"), 0.18215

        def encode_moments(self, x):
            return VO.vae_encode_moments(sd, x, len(cfg["block_out_channels"]), cfg["layers_per_block"])

    class Front:
        vae = Vae()

        def _embed(self, x, clip_images):
            assert x.shape == embed_shape and clip_images is None
            return torch.full((1, 1, 1024), 0.25)

    return Front()


def _draws(g, Tn, H, W):
    h, w = H // 8, W // 8
    return dict(vae_eps=torch.randn(Tn, 4, h, w, generator=g), cond_eps=torch.randn(1, 4, h, w, generator=g),
                pixel_noise=torch.randn(1, 3, H, W, generator=g), latent_noise=torch.randn(1, Tn, 4, h, w, generator=g), sigma=0.8,
                cond_sigma=0.05, random_p=torch.tensor([0.9]))


def test_batch_from_pixels_with_manipulation_actions():
    """(1, T, 8) poses: `manip_action_ids` (10 channels) or its positional form (T + 9), the noise draw UN-rotated — at a 7 x 7
    latent, whose width the navigation rotation would refuse; a channel count that is neither form is a ValueError."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.pipeline import SCENE_BOUNDS, action_encode_positional, manip_action_ids

    g = torch.Generator().manual_seed(1)
    Tn, H, W = 4, 56, 56
    px = torch.tanh(torch.randn(1, Tn, 3, H, W, generator=g))
    past = torch.tanh(torch.randn(1, 1, 3, H, W, generator=g))
    rs = np.random.RandomState(2)
    poses = np.zeros((1, Tn, 8), dtype=np.float32)
    poses[..., :3] = SCENE_BOUNDS[:3] + (SCENE_BOUNDS[3:] - SCENE_BOUNDS[:3]) * rs.uniform(0.1, 0.9, size=(1, Tn, 3))
    poses[..., 3:7] = rs.standard_normal((1, Tn, 4))
    poses[..., 7] = [1.0, 0.0, 1.0, 0.3]
    d = _draws(g, Tn, H, W)
    front = _front((1, 3, H, W))
    st = T.batch_from_pixels(front, px, past, poses, dropout_prob=0.1, draws=d)                     # default: 10 channels
    ids = manip_action_ids(poses)
    assert st.action_ids.shape == (1, Tn, 10) and torch.equal(st.action_ids, torch.from_numpy(ids))
    m, lv = front.vae.encode_moments(px[0])
    lat = ((m + torch.exp(0.5 * lv) * d["vae_eps"]) * 0.18215)[None]
    assert torch.allclose(st.target, lat, atol=1e-6)
    assert torch.allclose(st.noisy, lat + 0.8 * d["latent_noise"], atol=1e-6)                       # the draw itself: no rotation
    assert st.unet_input.shape == (1, Tn, 8, 7, 7)
    pos = T.batch_from_pixels(front, px, past, poses, dropout_prob=0.1, draws=d, action_input_channel=Tn + 9)
    assert pos.action_ids.shape == (1, Tn, Tn + 9) and torch.equal(pos.action_ids, torch.from_numpy(action_encode_positional(ids)))
    assert torch.equal(pos.noisy, st.noisy)
    as_list = T.batch_from_pixels(front, px, past, poses.tolist(), draws=d)                         # a nested list has rank 3 too
    assert torch.equal(as_list.action_ids, st.action_ids)
    for bad in (14, 9, 23):
        with pytest.raises(ValueError, match=r"10.*13|13.*10"):
            T.batch_from_pixels(front, px, past, poses, draws=d, action_input_channel=bad)


def test_batch_from_pixels_with_navigation_actions_is_unchanged():
    """Rank-2 actions: the cumulative id matrix and the rotated noise, whatever `action_input_channel` says."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.pipeline import action_ids_idx_encode, rotate_latent_noise

    g = torch.Generator().manual_seed(5)
    Tn, H, W = 4, 16, 128
    px = torch.tanh(torch.randn(1, Tn, 3, H, W, generator=g))
    past = torch.tanh(torch.randn(1, 1, 3, H, W, generator=g))
    acts = np.array([[4, 2, 3, 3]])
    d = _draws(g, Tn, H, W)
    front = _front((1, 3, H, W))
    for kw in ({}, {"action_input_channel": 4}):
        st = T.batch_from_pixels(front, px, past, acts, dropout_prob=0.1, draws=d, **kw)
        assert torch.equal(st.action_ids, torch.from_numpy(action_ids_idx_encode(acts)))
        noise = rotate_latent_noise(d["latent_noise"], acts)
        assert not torch.equal(noise, d["latent_noise"])
        assert torch.allclose(st.noisy, st.target + 0.8 * noise, atol=1e-6)
    flat = T.batch_from_pixels(front, px, past, [4, 2, 3, 3], dropout_prob=0.1, draws=d)           # (T,) ids, as before
    assert torch.equal(flat.noisy, st.noisy) and torch.equal(flat.action_ids, st.action_ids)


@pytest.mark.parametrize("pre", ["nav__", "manip__"])
def test_oracle_training_step_matches_reference_at_tail_sizes(golden, pre):
    """The oracle's step against the reference's autograd at levels of 60 / 15 and 196 / 49 tokens (and, for manip__, the
    10-channel action embedder): loss, prediction, every gradient norm, the stored gradients."""
    import wiw_amd  # noqa: F401
    from wiw_amd.pipeline import manip_action_ids
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_tails.npz")
    cfg = tails_config(pre)
    sd = {k: torch.from_numpy(v) for k, v in random_state_dict(cfg, int(g["weight_seed"])).items()}
    torch.set_num_threads(8)
    ids = O.action_ids_idx_encode(g[f"{pre}actions"]) if pre == "nav__" else manip_action_ids(g[f"{pre}actions"])
    aid = torch.from_numpy(np.asarray(ids)).float()
    assert float((aid - torch.from_numpy(g[f"{pre}action_ids"])).abs().max()) <= 1e-5
    x = tails_inputs(g, pre)
    loss, pred, grads = TO.training_step(
        sd, cfg.as_dict(), x["latents"], x["noise"], torch.from_numpy(g[f"{pre}sigmas"]), x["conditional_latents"],
        x["encoder_hidden_states"], float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]),
        dropout_prob=float(g["dropout_prob"]), random_p=torch.from_numpy(g["random_p"]))
    ref_loss = float(g[f"{pre}loss"])
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    ref = torch.from_numpy(g[f"{pre}model_pred"])
    assert float((pred - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    names, norms = [str(n) for n in g[f"{pre}grad_names"]], g[f"{pre}grad_norms"]
    assert set(names) <= set(grads)
    is_dead = lambda n: ("transformer_blocks.0.norm2." in n) or (".attn2.to_q." in n) or (".attn2.to_k." in n) or \
        n.startswith("add_embedding.")  # noqa: E731
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
    print(f"[tails oracle {pre}] {len(names)} gradient norms, worst relative deviation of the live ones {worst:.2e}")
    assert dead == 132 and worst <= 1e-3
    n_full = 0
    for key in g.files:
        if key.startswith(f"{pre}grad__") or key.startswith(f"{pre}grad8__"):
            name = key[len(pre):].split("__", 1)[1].replace("__", ".")
            r = torch.from_numpy(g[key])
            mine = grads[name] if key.startswith(f"{pre}grad__") else grads[name].reshape(grads[name].shape[0], -1)[:8, :r.shape[1]]
            assert float((mine.reshape(r.shape) - r).abs().max()) <= 2e-4 * float(r.abs().max()) + 1e-12, name
            n_full += 1
    assert n_full >= 15
