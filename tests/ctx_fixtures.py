"""Scenarios and inputs of tests/golden/train_step_ctx.npz (fine-tuning with 2 .. 8 conditioning tokens per sample), shared by
its generator (tools/make_golden_train_ctx.py) and its tests (tests/test_hip_train_ctx.py, tests/test_cross_attn_train_abi.py).

    prefix   network                                              latent, T   P   tape
    p3__     UNetConfig.tiny(4), navigation                       16x32, 4    3   UNetTrain
    p8__     tiny, task_type manipulation, 10 action channels     16x16, 17   8   UNetTrain32
    full__   served width (320/640/1280/1280), navigation         8x16, 4     2   UNetTrain

latents / noise / conditional_latents are drawn as tools/make_golden_train_tails.py `draw_inputs` draws them (RandomState's
frozen stream, rounded to bf16); the P conditioning tokens are N(0, 1) rounded to bf16 from their OWN seed (`ctx_tokens`)."""
import numpy as np
import torch

NAME = "train_step_ctx.npz"
PREFIXES = ("p3__", "p8__", "full__")
INPUTS = ("latents", "noise", "conditional_latents", "encoder_hidden_states")
# prefix: (latent h, w, frames, P, sigma, noise_aug_strength, input seed, token seed, also the reference's own bf16 run)
SCENARIOS = {"p3__": (16, 32, 4, 3, 1.4, 0.041, 51, 61, True),
             "p8__": (16, 16, 17, 8, 0.9, 0.033, 52, 62, True),
             "full__": (8, 16, 4, 2, 2.2, 0.027, 53, 63, False)}
# gradients stored in full next to `make_train_golden.FULL`: the newly live tensors of one spatial and one temporal block
_B = "down_blocks.1.attentions.0."
CTX_FULL = [_B + blk + t for blk in ("transformer_blocks.0.", "temporal_transformer_blocks.0.")
            for t in ("attn2.to_q.weight", "attn2.to_k.weight", "norm2.weight")]


def ctx_config(pre):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig

    tiny = UNetConfig.tiny(4)
    if pre == "p3__":
        return tiny
    if pre == "p8__":
        return UNetConfig(block_out_channels=tiny.block_out_channels, num_attention_heads=tiny.num_attention_heads, num_frames=17,
                          action_input_channel=10, task_type="manipulation")
    return UNetConfig(num_frames=4, action_input_channel=4)


def ctx_tokens(seed, P, dim=1024):
    """(1, P, dim) conditioning tokens: unit normal, bf16-representable."""
    rs = np.random.RandomState(int(seed))
    return torch.from_numpy(rs.standard_normal((1, P, dim)).astype(np.float32)).to(torch.bfloat16).float()


def draw_ctx_inputs(pre):
    h, w, T, P, _, _, seed, tok_seed, _ = SCENARIOS[pre]
    rs = np.random.RandomState(seed)
    draw = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))  # noqa: E731
    inp = {"latents": draw(1, T, 4, h, w) * 0.8, "noise": draw(1, T, 4, h, w), "conditional_latents": draw(1, 4, h, w)}
    inp = {k: v.to(torch.bfloat16).float() for k, v in inp.items()}
    inp["encoder_hidden_states"] = ctx_tokens(tok_seed, P)
    return inp


def checksums(inp):
    return np.array([[float(inp[k].double().sum()), float(inp[k].double().pow(2).sum())] for k in INPUTS])


def ctx_inputs(g, pre):
    """The fp32 inputs of one scenario, re-drawn and checked against the checksums the generator stored."""
    inp = draw_ctx_inputs(pre)
    assert int(g[f"{pre}input_seed"]) == SCENARIOS[pre][6] and int(g[f"{pre}token_seed"]) == SCENARIOS[pre][7]
    assert np.array_equal(checksums(inp), g[f"{pre}input_checksums"]), "the re-drawn inputs are not the generator's"
    return inp
