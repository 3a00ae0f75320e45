#!/usr/bin/env python
"""Generate tests/golden/train_step_batch.npz: the batched fine-tuning step at the SERVED width (320/640/1280/1280, 4 frames,
16x32 latent, B = 2; scenario `full2` of tests/batch_fixtures.py).  The reference of a batch is the mean over its samples of
`oracle/train_oracle.training_step` (pinned to the reference's `loss.backward()` by tests/test_train_oracle.py) run on each
sample alone on the CPU, in fp32: loss = mean_b loss_b, every gradient the mean of the single-sample gradients.

Schema of tests/golden/train_step_tails.npz: the inputs are NOT stored but re-drawn from `full2__input_seed` (+ b for sample
b) by `batch_fixtures.sample_inputs` and checked against `full2__input_checksums`; stored are the loss, the per-sample losses,
the prediction, the norm of every gradient (`grad_names` / `grad_norms`) and, of the tensors of `batch_fixtures.WATCH`, the
gradient itself — whole (`grad__`) up to 4096 elements, else the first 512 columns of its first 8 rows (`grad8__`).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_batch_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np  # noqa: E402


def main():
    import batch_fixtures as BF

    pre, name = "full2__", "full2"
    loss, pred, grads, losses = BF.oracle_mean(name)
    sc = BF.SCENARIOS[name]
    out = {f"{pre}input_seed": np.array(sc[5]), f"{pre}latent_hw": np.array(sc[:2]), f"{pre}input_checksums": BF.checksums(name),
           f"{pre}sigmas": np.array(sc[6], np.float32), f"{pre}noise_aug_strength": np.array(sc[7]),
           f"{pre}random_p": np.array(sc[8], np.float32), f"{pre}loss": np.array(loss), f"{pre}sample_losses": np.array(losses),
           f"{pre}model_pred": pred.numpy()}
    names, norms = [], []
    for k in BF.batch_weights(name):
        g = grads.get(k)
        names.append(k)
        norms.append(0.0 if g is None else float(g.double().norm()))
        if k in BF.WATCH:
            if g.numel() > BF.FULL_ROWS_ABOVE:
                out[f"{pre}grad8__" + k.replace(".", "__")] = g.reshape(g.shape[0], -1)[:8, :512].numpy().copy()
            else:
                out[f"{pre}grad__" + k.replace(".", "__")] = g.numpy().copy()
    out.update({f"{pre}grad_names": np.array(names), f"{pre}grad_norms": np.array(norms)})
    path = os.path.join(ROOT, "tests", "golden", BF.NAME)
    np.savez_compressed(path, weight_seed=np.array(BF.WEIGHT_SEED), dropout_prob=np.array(BF.DROPOUT), **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), loss {loss}, per sample {losses}")


if __name__ == "__main__":
    main()
