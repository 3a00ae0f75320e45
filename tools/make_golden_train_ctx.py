#!/usr/bin/env python
"""Generate tests/golden/train_step_ctx.npz: three fine-tuning steps of the REFERENCE UNet under `loss.backward()` with 2 .. 8
conditioning tokens per sample (`--num_past_obs P`, train_svd.py:359, 889-894) — build container only; imports the reference
through oracle/_ref_import.py; the step is tools/make_golden_train_tails.py `step` (train_svd.py:886-952) on
encoder_hidden_states (1, P, 1024).  Scenarios, seeds and the token draw: tests/ctx_fixtures.py.

Per scenario: loss, model_pred, every gradient norm (`grad_names` / `grad_norms`), and of one tensor per operator class
(`make_train_golden.FULL` + `ctx_fixtures.CTX_FULL`: attn2.to_q / attn2.to_k / norm2 of one spatial and one temporal block) the
gradient.  For the two tiny scenarios also the reference's OWN bf16 run: loss, prediction, gradient norms and the CTX_FULL
gradients (`gradb16__`), the yardstick of 16-bit storage on the newly live tensors.  Size devices as train_step_tails.npz.

The generator asserts, per transformer block, that the fp32 gradient norms of attn2.to_q, attn2.to_k and norm2.weight are
>= 1e-2, >= 1e-2 and >= 1e-3 of that block's attn2.to_v.weight: the newly live gradients are signal, not rounding.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_ctx.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctx_fixtures import CTX_FULL, NAME, SCENARIOS, checksums, ctx_config, draw_ctx_inputs  # noqa: E402
from make_golden_train_horizon import nav_actions, poses  # noqa: E402
from make_golden_train_tails import FULL_ROWS_ABOVE, bf16_bits, step  # noqa: E402


def stored(g):
    if g.numel() > FULL_ROWS_ABOVE:
        return "grad8__", g.reshape(g.shape[0], -1)[:8, :512].float().numpy().copy()
    return "grad__", g.float().numpy().copy()


def live_ratios(norms):
    """min over the transformer blocks of |to_q| / |to_v|, |to_k| / |to_v|, |norm2.weight| / |to_v| (asserted)."""
    worst = [np.inf, np.inf, np.inf]
    for k, nv in norms.items():
        if not k.endswith(".attn2.to_v.weight"):
            continue
        blk = k[: -len("attn2.to_v.weight")]
        r = [norms[blk + "attn2.to_q.weight"] / nv, norms[blk + "attn2.to_k.weight"] / nv, norms[blk + "norm2.weight"] / nv]
        assert r[0] >= 1e-2 and r[1] >= 1e-2 and r[2] >= 1e-3, (blk, r)
        worst = [min(a, b) for a, b in zip(worst, r)]
    return worst


def main():
    from _ref_import import import_reference
    import wiw_amd  # noqa: F401
    from make_golden import save
    from make_train_golden import FULL

    ns = import_reference()
    from utils.svd_utils import apply_conditioning_dropout  # type: ignore  (reference)

    torch.set_num_threads(8)
    out = {}
    for pre, (h, w, T, P, sigma, nas, seed, tok_seed, with_bf16) in SCENARIOS.items():
        cfg = ctx_config(pre)
        actions = poses(T, 29) if cfg.task_type == "manipulation" else nav_actions(T)
        inp = draw_ctx_inputs(pre)
        assert tuple(inp["encoder_hidden_states"].shape) == (1, P, cfg.cross_attention_dim)
        m, action_ids, loss, pred = step(ns, apply_conditioning_dropout, cfg, inp, actions, sigma, nas, torch.float32)
        names, norms = [], []
        for k, prm in m.named_parameters():
            g = prm.grad
            names.append(k)
            norms.append(0.0 if g is None else float(g.double().norm()))
            if k in FULL or k in CTX_FULL:
                kind, a = stored(g)
                out[f"{pre}{kind}" + k.replace(".", "__")] = a
        ratios = live_ratios(dict(zip(names, norms)))
        out.update({f"{pre}input_seed": np.array(seed), f"{pre}token_seed": np.array(tok_seed), f"{pre}latent_hw": np.array([h, w]),
                    f"{pre}num_frames": np.array(T), f"{pre}num_past_obs": np.array(P), f"{pre}input_checksums": checksums(inp),
                    f"{pre}live_ratios": np.array(ratios)})
        out.update({f"{pre}actions": actions, f"{pre}action_ids": action_ids.numpy(), f"{pre}sigmas": np.array([sigma], np.float32),
                    f"{pre}noise_aug_strength": np.array(nas), f"{pre}loss": np.array(loss), f"{pre}model_pred": pred.numpy(),
                    f"{pre}grad_names": np.array(names), f"{pre}grad_norms": np.array(norms)})
        print(pre, "loss", loss, "tensors", len(names), "min to_q/to_v, to_k/to_v, norm2/to_v:", ratios, flush=True)
        ref32 = {k: prm.grad.clone() for k, prm in m.named_parameters() if k in CTX_FULL}
        del m
        if with_bf16:
            mb, _, loss_b, pred_b = step(ns, apply_conditioning_dropout, cfg, inp, actions, sigma, nas, torch.bfloat16)
            nb = [0.0 if p.grad is None else float(p.grad.double().norm()) for _, p in mb.named_parameters()]
            out.update({f"{pre}loss_ref_bf16": np.array(loss_b), f"{pre}model_pred_ref_bf16_bits": bf16_bits(pred_b),
                        f"{pre}grad_norms_ref_bf16": np.array(nb)})
            devs = []
            for k, prm in mb.named_parameters():
                if k in CTX_FULL:
                    a, b = prm.grad.float(), ref32[k]
                    devs.append(float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()))
            out[f"{pre}ctx_full_ref_bf16_rms"] = np.array(devs)
            print(pre, "bf16 loss", loss_b, "rel rms of the CTX_FULL gradients, bf16 run vs fp32 run:", devs, flush=True)
    save(NAME, weight_seed=np.array(7), random_p=np.array([0.9], np.float32), dropout_prob=np.array(0.1), **out)
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", NAME))
    print("bytes", size)
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
