#!/usr/bin/env python
"""Generate tests/golden/train_step_horizon.npz: three fine-tuning steps of the REFERENCE UNet under `loss.backward()` at
prediction horizons of more than 16 frames (build container only; imports the reference through oracle/_ref_import.py; the
step formulas — train_svd.py:886-952, as oracle/make_train_golden.py states them — are those of
tools/make_golden_train_tails.py `step`, which this file calls).

    prefix   network                                              latent, T   levels S            actions
    t25__    UNetConfig.tiny(25)                                  16x32, 25   512, 128, 32, 8     navigation ids (1, 25)
    t17__    tiny, task_type manipulation, 10 action channels,    16x16, 17   256, 64, 16, 4      (1, 17, 8) poses in SCENE_BOUNDS
             num_frames 17
    full__   served width (320/640/1280/1280, 5/10/20/20 heads),  8x16, 25    128, 32, 8, 2       navigation ids (1, 25)
             navigation, num_frames 25 (25-channel action embedder)

Per scenario: loss, model_pred, every gradient norm (`grad_names` / `grad_norms`), and of one tensor per operator class
(`make_train_golden.FULL`) the gradient.  For the two tiny scenarios also the loss, prediction and gradient norms of the
reference's OWN bf16 run.  The size devices are those of train_step_tails.npz: inputs re-drawn from `{prefix}input_seed` by
`draw_inputs` and checked against `{prefix}input_checksums`, gradients above 4096 elements stored as `[:8, :512]` (`grad8__`),
the bf16 prediction as its bit pattern.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_horizon.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden_train_tails import FULL_ROWS_ABOVE, bf16_bits, checksums, draw_inputs, step  # noqa: E402

NAME = "train_step_horizon.npz"


def nav_actions(n):
    """[4] + cycle([1, 2, 1, 3]): forward steps and both turns (the turns rotate the latent noise)."""
    return np.array([[4] + [[1, 2, 1, 3][i % 4] for i in range(n - 1)]], dtype=np.int64)


def poses(n, seed):
    from wiw_amd.pipeline import SCENE_BOUNDS

    rs = np.random.RandomState(seed)
    p = np.zeros((1, n, 8), dtype=np.float32)
    lo, hi = SCENE_BOUNDS[:3], SCENE_BOUNDS[3:]
    p[..., :3] = lo + (hi - lo) * rs.uniform(0.05, 0.95, size=(1, n, 3))
    q = rs.standard_normal((1, n, 4))
    p[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    p[..., 7] = (np.arange(n) % 3 == 0).astype(np.float32)
    return p


def scenarios():
    from wiw_amd.config import UNetConfig

    t25 = UNetConfig.tiny(25)
    t17 = UNetConfig(block_out_channels=t25.block_out_channels, num_attention_heads=t25.num_attention_heads, num_frames=17,
                     action_input_channel=10, task_type="manipulation")
    full = UNetConfig(num_frames=25, action_input_channel=25)
    # prefix: (config, h, w, actions, sigma, noise_aug_strength, input seed, also the bf16 run)
    return {"t25__": (t25, 16, 32, nav_actions(25), 1.3, 0.037, 41, True),
            "t17__": (t17, 16, 16, poses(17, 29), 0.8, 0.045, 42, True),
            "full__": (full, 8, 16, nav_actions(25), 2.1, 0.028, 43, False)}


def main():
    from _ref_import import import_reference
    import wiw_amd  # noqa: F401
    from make_golden import save
    from make_train_golden import FULL

    ns = import_reference()
    from utils.svd_utils import apply_conditioning_dropout  # type: ignore  (reference)

    torch.set_num_threads(8)
    out = {}
    for pre, (cfg, h, w, actions, sigma, nas, seed, with_bf16) in scenarios().items():
        inp = draw_inputs(seed, cfg.num_frames, h, w, cfg.cross_attention_dim)
        m, action_ids, loss, pred = step(ns, apply_conditioning_dropout, cfg, inp, actions, sigma, nas, torch.float32)
        names, norms = [], []
        for k, prm in m.named_parameters():
            g = prm.grad
            names.append(k)
            norms.append(0.0 if g is None else float(g.double().norm()))
            if k in FULL:
                if g.numel() > FULL_ROWS_ABOVE:
                    out[f"{pre}grad8__" + k.replace(".", "__")] = g.reshape(g.shape[0], -1)[:8, :512].numpy().copy()
                else:
                    out[f"{pre}grad__" + k.replace(".", "__")] = g.numpy().copy()
        out.update({f"{pre}input_seed": np.array(seed), f"{pre}latent_hw": np.array([h, w]), f"{pre}num_frames": np.array(cfg.num_frames),
                    f"{pre}input_checksums": checksums(inp)})
        out.update({f"{pre}actions": actions, f"{pre}action_ids": action_ids.numpy(), f"{pre}sigmas": np.array([sigma], np.float32),
                    f"{pre}noise_aug_strength": np.array(nas), f"{pre}loss": np.array(loss), f"{pre}model_pred": pred.numpy(),
                    f"{pre}grad_names": np.array(names), f"{pre}grad_norms": np.array(norms)})
        print(pre, "loss", loss, "tensors", len(names), flush=True)
        del m
        if with_bf16:
            mb, _, loss_b, pred_b = step(ns, apply_conditioning_dropout, cfg, inp, actions, sigma, nas, torch.bfloat16)
            nb = [0.0 if p.grad is None else float(p.grad.double().norm()) for _, p in mb.named_parameters()]
            out.update({f"{pre}loss_ref_bf16": np.array(loss_b), f"{pre}model_pred_ref_bf16_bits": bf16_bits(pred_b),
                        f"{pre}grad_norms_ref_bf16": np.array(nb)})
            print(pre, "bf16 loss", loss_b, flush=True)
    save(NAME, weight_seed=np.array(7), random_p=np.array([0.9], np.float32), dropout_prob=np.array(0.1), **out)
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", NAME))
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
