"""Scenarios, inputs and references of the batched fine-tuning step (several clips per step), shared by the generator of
tests/golden/train_step_batch.npz (tools/make_batch_golden.py) and by tests/test_train_batch.py / tests/test_hip_train_batch.py.

    name     network                                           latent, T   B   P   tape          reference
    tiny2    UNetConfig.tiny(4), navigation                    8x16, 4     2   1   UNetTrain     oracle, in the test
    nav3     UNetConfig.tiny(4), navigation                    24x40, 4    3   1   UNetTrain     oracle, in the test
    manip3   tiny, task_type manipulation, 10 channels         24x40, 4    3   1   UNetTrain     oracle, in the test
    h17      UNetConfig.tiny(17), navigation                   8x16, 17    2   1   UNetTrain32   oracle, in the test
    ctx3     UNetConfig.tiny(4), navigation                    8x16, 4     2   3   UNetTrain     oracle, in the test
    full2    served width (320/640/1280/1280), navigation      16x32, 4    2   1   UNetTrain     train_step_batch.npz

The reference of a batch is the MEAN over its samples of `oracle/train_oracle.training_step` run on each sample alone (the
oracle is pinned to the reference's `loss.backward()` by tests/test_train_oracle.py): loss = mean_b loss_b, every gradient the
mean of the B single-sample gradients — train_svd.py:946-951 with independent samples.

Sample b of a scenario is drawn from its own seed (`seed + b`) as tools/make_golden_train_tails.py `draw_inputs` draws
(RandomState's frozen stream, values rounded to bf16) and has its own sigma, noise_aug_strength, actions, conditioning tokens
and conditioning-dropout draw; with dropout_prob 0.1 a draw of 0.05 zeroes the sample's tokens, 0.25 its conditioning latents,
0.9 keeps both."""
import functools

import numpy as np
import torch

NAME = "train_step_batch.npz"
DROPOUT = 0.1
WEIGHT_SEED = 7
INPUTS = ("latents", "noise", "conditional_latents", "encoder_hidden_states")
# name: (h, w, T, B, P, input seed, sigmas, noise_aug_strengths, random_p, task)
SCENARIOS = {
    "tiny2": (8, 16, 4, 2, 1, 71, (1.7, 0.6), (0.043, 0.021), (0.05, 0.25), "navigation"),
    "nav3": (24, 40, 4, 3, 1, 74, (1.3, 0.45, 2.6), (0.043, 0.02, 0.061), (0.05, 0.25, 0.9), "navigation"),
    "manip3": (24, 40, 4, 3, 1, 78, (0.9, 2.1, 0.5), (0.031, 0.05, 0.017), (0.25, 0.9, 0.05), "manipulation"),
    "h17": (8, 16, 17, 2, 1, 82, (1.1, 0.7), (0.035, 0.05), (0.9, 0.05), "navigation"),
    "ctx3": (8, 16, 4, 2, 3, 85, (1.4, 0.8), (0.041, 0.027), (0.9, 0.9), "navigation"),
    "full2": (16, 32, 4, 2, 1, 88, (2.2, 0.7), (0.027, 0.052), (0.05, 0.25), "navigation"),
}
# one tensor per operator class (the list of oracle/make_train_golden.py `FULL`), and the tensors that are live only with
# more than one conditioning token (tests/ctx_fixtures.py `CTX_FULL`)
WATCH = ["conv_in.weight", "conv_out.bias", "time_embedding.linear_1.weight", "add_action_proj.proj.weight",
         "down_blocks.0.resnets.0.spatial_res_block.conv1.weight", "down_blocks.0.resnets.0.spatial_res_block.norm2.weight",
         "down_blocks.0.resnets.0.temporal_res_block.conv2.weight", "down_blocks.0.resnets.0.time_mixer.mix_factor",
         "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.weight",
         "down_blocks.1.attentions.0.transformer_blocks.0.norm3.bias",
         "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj.weight",
         "down_blocks.1.attentions.0.temporal_transformer_blocks.0.attn1.to_v.weight",
         "down_blocks.1.attentions.0.temporal_transformer_blocks.0.attn2.to_out.0.bias",
         "down_blocks.1.attentions.0.time_pos_embed.linear_2.weight",
         "up_blocks.1.resnets.0.spatial_res_block.conv_shortcut.weight", "up_blocks.0.upsamplers.0.conv.weight",
         "down_blocks.0.downsamplers.0.conv.weight", "mid_block.attentions.0.proj_out.weight"]
_BLK = "down_blocks.1.attentions.0."
WATCH_CTX = [_BLK + blk + t for blk in ("transformer_blocks.0.", "temporal_transformer_blocks.0.")
             for t in ("attn2.to_q.weight", "attn2.to_k.weight", "norm2.weight")]
FULL_ROWS_ABOVE = 4096      # fixture: larger gradients are stored as [:8, :512] of their (out, -1) view (`grad8__`)


def batch_config(name):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig

    T, task = SCENARIOS[name][2], SCENARIOS[name][9]
    tiny = UNetConfig.tiny(T)
    if name == "full2":
        return UNetConfig(num_frames=T, action_input_channel=T)
    if task == "manipulation":
        return UNetConfig(block_out_channels=tiny.block_out_channels, num_attention_heads=tiny.num_attention_heads, num_frames=T,
                          action_input_channel=10, task_type="manipulation")
    return tiny


def batch_weights(name):
    from wiw_amd.weights import random_state_dict

    return random_state_dict(batch_config(name), WEIGHT_SEED)


def is_dead(n, P=1):
    if P > 1:
        return n.startswith("add_embedding.")
    return ("transformer_blocks.0.norm2." in n) or (".attn2.to_q." in n) or (".attn2.to_k." in n) or n.startswith("add_embedding.")


def sample_inputs(name, b):
    """Sample b of a scenario: fp32 tensors leading with 1, bf16-representable, and its action ids (1, T, Ch)."""
    from wiw_amd.pipeline import SCENE_BOUNDS, action_ids_idx_encode, manip_action_ids

    h, w, T, _, P, seed, _, _, _, task = SCENARIOS[name]
    rs = np.random.RandomState(seed + b)
    draw = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))  # noqa: E731
    inp = {"latents": draw(1, T, 4, h, w) * 0.8, "noise": draw(1, T, 4, h, w), "conditional_latents": draw(1, 4, h, w),
           "encoder_hidden_states": draw(1, P, 1024)}
    inp = {k: v.to(torch.bfloat16).float() for k, v in inp.items()}
    if task == "manipulation":
        poses = np.zeros((1, T, 8), dtype=np.float32)
        lo, hi = SCENE_BOUNDS[:3], SCENE_BOUNDS[3:]
        poses[..., :3] = lo + (hi - lo) * rs.uniform(0.05, 0.95, size=(1, T, 3))
        q = rs.standard_normal((1, T, 4))
        poses[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        poses[..., 7] = rs.randint(0, 2, size=T).astype(np.float32)
        inp["action_ids"] = torch.from_numpy(manip_action_ids(poses)).float()
    else:
        inp["action_ids"] = torch.from_numpy(action_ids_idx_encode(rs.randint(1, 5, size=(1, T)))).float()
    return inp


def checksums(name):
    """[B][4][2]: sum and sum of squares of every input tensor of every sample (exact in float64 for 8-bit mantissas)."""
    B = SCENARIOS[name][3]
    return np.array([[[float(x[k].double().sum()), float(x[k].double().pow(2).sum())] for k in INPUTS]
                     for x in (sample_inputs(name, b) for b in range(B))])


def batch_step_inputs(name):
    """(batched StepInputs through `prepare_step` on the stacked tensors, [single-sample StepInputs])."""
    from wiw_amd import train as T

    _, _, _, B, _, _, sig, aug, rp, _ = SCENARIOS[name]
    xs = [sample_inputs(name, b) for b in range(B)]
    cat = lambda k: torch.cat([x[k] for x in xs])  # noqa: E731
    st = T.prepare_step(cat("latents"), cat("noise"), list(sig), cat("conditional_latents"), cat("encoder_hidden_states"), list(aug),
                        cat("action_ids"), dropout_prob=DROPOUT, random_p=torch.tensor(rp))
    singles = [T.prepare_step(x["latents"], x["noise"], sig[b], x["conditional_latents"], x["encoder_hidden_states"], aug[b],
                              x["action_ids"], dropout_prob=DROPOUT, random_p=torch.tensor([rp[b]])) for b, x in enumerate(xs)]
    return st, singles


@functools.lru_cache(maxsize=None)
def oracle_mean(name):
    """(loss, model_pred (B, T, 4, h, w), {parameter: mean gradient}, [per-sample losses]) of the scenario: the oracle once per sample on the CPU,
    averaged.  Computed once per process and shared; callers do not modify it."""
    import train_oracle as TO

    _, _, _, B, _, _, sig, aug, rp, _ = SCENARIOS[name]
    cfg = batch_config(name)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in batch_weights(name).items()}
    torch.set_num_threads(8)
    losses, preds, acc = [], [], {}
    for b in range(B):
        x = sample_inputs(name, b)
        loss, pred, grads = TO.training_step(sd, cfg.as_dict(), x["latents"], x["noise"], torch.tensor([sig[b]]),
                                             x["conditional_latents"], x["encoder_hidden_states"], aug[b], x["action_ids"],
                                             dropout_prob=DROPOUT, random_p=torch.tensor([rp[b]]))
        losses.append(float(loss))
        preds.append(pred)
        for k, g in grads.items():
            if g is not None:
                acc[k] = g.double() if k not in acc else acc[k] + g.double()
    return sum(losses) / B, torch.cat(preds), {k: (v / B).float() for k, v in acc.items()}, losses
