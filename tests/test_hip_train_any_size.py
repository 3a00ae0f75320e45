"""Fine-tuning at every served latent size — GPU side (448 x 448 manipulation clips: a 56 x 56 latent, levels of 3136, 784, 196
and 49 tokens).  Both 16-bit libraries.

  * the padded self-attention helpers (`Hip.attn_padded` / `attn_padded_backward`: pad -> attn_small -> unpad, one-wave backward
    with Sp > S) against torch fp32 autograd at the tail classes of 8x8, 24x40 and 56x56 latents;
  * wiw_transpose_bf16 at row counts that are not multiples of 8 (the conv weight gradients of a 4 x 7 x 7-row level), and the
    convolution backward at that level against torch;
  * the whole training step against the reference's own `loss.backward()` (tests/golden/train_step_tails.npz, written by
    tools/make_golden_train_tails.py): tiny navigation network at 24x40, tiny manipulation network at 56x56, served width at 24x24;
  * `Trainer` on the tiny manipulation network at 56x56: steps, validation rollout with (1, T, 8) actions, save / resume.
"""
import os

import numpy as np
import pytest
import torch

from test_train_any_size import tails_config, tails_inputs

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _rel(a, b, scale=None):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    if scale is not None:                     # an identically-zero reference: errors relative to the given magnitude
        return float((a - b).abs().max() / scale), float((a - b).pow(2).mean().sqrt() / scale)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)), float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _poison(sizes, dtype):
    """Fill blocks of the sizes the code under test is about to allocate with NaN and free them: the caching allocator hands
    them out again, so a pad row that is read without ever having been written shows up as NaN."""
    blocks = [torch.full((int(n),), float("nan"), dtype=dt, device=DEV) for n in sizes for dt in (dtype, torch.float32) for _ in range(2)]
    torch.cuda.synchronize()
    del blocks


@DTYPES
@pytest.mark.parametrize("seqs,S,heads", [(2, 1, 1), (2, 4, 1), (2, 15, 2), (2, 24, 1), (3, 49, 20), (3, 60, 1), (2, 196, 2)])
def test_padded_attention_forward_and_backward(seqs, S, heads, dtype):
    """O, dQ, dK, dV of softmax(Q K^T / 8) V through the padded helpers against torch autograd on the same 16-bit-rounded q, k,
    v, dO: the kernel pair's tolerance (max 2e-2, rms 8e-3 relative, tests/test_hip_train.py `test_attention_backward`).
    Outputs have exactly seqs * S rows, are NaN-free on a poisoned allocator and repeat bit for bit.
    S = 1: the softmax over one key is identically 1, so the reference dQ and dK are exactly zero and a relative error does
    not exist; the kernel's dS = P (dP - D) cancels to fp32 round-off of dP there, so dQ / dK are measured against the magnitude
    of the cancelling terms, scale * max|dP| * max|K| (resp. max|Q|) — the same 2e-2 / 8e-3 of the quantity the kernel rounds."""
    import torch.nn.functional as F

    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV), dtype)
    r16 = lambda t: t.to(dtype).float()  # noqa: E731
    C, M, Sp = heads * 64, seqs * S, -(-S // 16) * 16
    qkv, dO = r16(_rnd(M, 3 * C, seed=1)), r16(_rnd(M, C, seed=2))
    leaf = qkv.clone().requires_grad_(True)

    def hd(t):
        return t.reshape(seqs, S, heads, 64).transpose(1, 2)

    o_ref = F.scaled_dot_product_attention(hd(leaf[:, :C]), hd(leaf[:, C:2 * C]), hd(leaf[:, 2 * C:])).transpose(1, 2).reshape(M, C)
    o_ref.backward(dO)
    qkv_d, dO_d = qkv.to(DEV, dtype), dO.to(DEV, dtype)
    sizes = [seqs * Sp * 3 * C, seqs * Sp * C, M * C, M * 3 * C, seqs * heads * Sp]
    _poison(sizes, dtype)
    O, saved = hip.attn_padded(qkv_d, seqs, S, heads, 0.125)
    _poison(sizes, dtype)
    dqkv = hip.attn_padded_backward(saved, dO_d)
    torch.cuda.synchronize()
    assert tuple(O.shape) == (M, C) and tuple(dqkv.shape) == (M, 3 * C)
    assert torch.isfinite(O.float()).all() and torch.isfinite(dqkv.float()).all()
    zero_scale = {}
    if S == 1:
        dP = (hd(dO) * hd(qkv[:, 2 * C:])).sum(-1).abs().max()
        zero_scale = {"dQ": float(0.125 * dP * qkv[:, C:2 * C].abs().max()), "dK": float(0.125 * dP * qkv[:, :C].abs().max())}
        assert float(leaf.grad[:, :2 * C].abs().max()) == 0.0
    mx, rms = _rel(O, o_ref)
    print(f"[any size {dtype}] padded attention {seqs}x{S}x{heads} (Sp {Sp}) O: max_rel={mx:.2e} rms={rms:.2e}")
    assert mx <= 2e-2 and rms <= 8e-3
    for name, sl in (("dQ", slice(0, C)), ("dK", slice(C, 2 * C)), ("dV", slice(2 * C, 3 * C))):
        mx, rms = _rel(dqkv[:, sl], leaf.grad[:, sl], zero_scale.get(name))
        print(f"[any size {dtype}] padded attention {seqs}x{S}x{heads} {name}: max_rel={mx:.2e} rms={rms:.2e}")
        assert mx <= 2e-2 and rms <= 8e-3, name
    O2, saved2 = hip.attn_padded(qkv_d, seqs, S, heads, 0.125)
    assert torch.equal(O, O2) and torch.equal(dqkv, hip.attn_padded_backward(saved2, dO_d))


@DTYPES
@pytest.mark.parametrize("rows,C,c0,ldx", [(196, 128, 0, 128), (60, 64, 64, 192), (686, 320, 0, 320), (1, 8, 8, 24), (71, 72, 0, 72)])
def test_transpose_with_any_row_count(rows, C, c0, ldx, dtype):
    """wiw_transpose_bf16 at row counts that are not multiples of 8 (196 = 4 x 7 x 7, 686 = 14 x 49: the dY^T operand of the conv
    weight-gradient GEMM at the 7 x 7 level): exact, the columns up to the next multiple of 8 zero, nothing beyond written."""
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV), dtype)
    X = _rnd(rows, ldx, seed=3).to(DEV, dtype)
    ldy = -(-rows // 64) * 64
    Y = torch.full((C, ldy), 7.0, dtype=dtype, device=DEV)
    hip.transpose(X, ldx, c0, rows, C, Y, ldy)
    r8 = -(-rows // 8) * 8
    assert torch.equal(Y[:, :rows], X[:, c0:c0 + C].t())
    assert float(Y[:, rows:r8].float().abs().max()) == 0.0 if r8 > rows else True
    assert bool((Y[:, r8:] == 7.0).all())
    with pytest.raises(RuntimeError):                              # a destination that cannot hold the zero columns
        hip.transpose(X, ldx, c0, rows, C, torch.empty(C, r8 - 8, dtype=dtype, device=DEV), r8 - 8)


@DTYPES
@pytest.mark.parametrize("temporal", [False, True], ids=["3x3", "t3"])
def test_conv_backward_at_the_7x7_level(temporal, dtype):
    """`train.conv_backward` at M = 4 x 7 x 7 = 196 rows (not a multiple of 8: today's assertion, and the transposes of the
    weight-gradient operands, refused it) against torch autograd: dx, dW, db."""
    import torch.nn.functional as F

    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV), dtype)
    r16 = lambda t: t.to(dtype).float()  # noqa: E731
    Tn, H, W, Cin, Cout = 4, 7, 7, 128, 64
    M, taps = Tn * H * W, 3 if temporal else 9
    x, dy = r16(_rnd(M, Cin, seed=1)), r16(_rnd(M, Cout, seed=2))
    w = r16(_rnd(Cout, Cin, *((3, 1, 1) if temporal else (3, 3)), seed=3) * (taps * Cin) ** -0.5)
    xr = x.reshape(Tn, H, W, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)      # (T, C, H, W)
    wr = w.clone().requires_grad_(True)
    if temporal:
        y = F.conv3d(xr.permute(1, 0, 2, 3)[None], wr, padding=(1, 0, 0))[0].permute(1, 0, 2, 3)
        Wk = w[:, :, :, 0, 0].permute(0, 2, 1).reshape(Cout, -1)
    else:
        y = F.conv2d(xr, wr, padding=1)
        Wk = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    y.backward(dy.reshape(Tn, H, W, Cout).permute(0, 3, 1, 2))
    T.clear_wgrad_plans()
    dx, dW, db = T.conv_backward(hip, x.to(DEV, dtype), Wk.to(DEV, dtype).contiguous(), dy.to(DEV, dtype), H, W, T=Tn, temporal=temporal)
    if temporal:
        dW_ref = wr.grad[:, :, :, 0, 0].permute(0, 2, 1).reshape(Cout, -1)
    else:
        dW_ref = wr.grad.permute(0, 2, 3, 1).reshape(Cout, -1)
    dx_ref = xr.grad.permute(0, 2, 3, 1).reshape(M, Cin)
    e = {"dx": _rel(dx, dx_ref), "dW": _rel(dW, dW_ref), "db": _rel(db, dy.sum(0))}
    print(f"[any size {dtype}] conv backward {'t3' if temporal else '3x3'} at 4x7x7: " + " ".join(f"{k} max={v[0]:.1e} rms={v[1]:.1e}" for k, v in e.items()))
    # dx is an fp32 sum of exact products rounded ONCE to 16 bits: unit round-off u = 2^-8 (bf16: 8 significant bits) / 2^-11
    # (fp16), so every element is within u of its value — rms <= u, and 4 u for the max leaves room for the fp32 summation
    # order; dW and db are fp32 sums over 196 rows of exact products of the same 16-bit operands: summation order only
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert e["dx"][1] <= eps and e["dx"][0] <= 4 * eps
    assert e["dW"][0] <= 1e-5 and e["db"][0] <= 1e-5
    T.clear_wgrad_plans()


# ---- the whole step against the reference -----------------------------------------------------------------------------
# (prediction rms, loss rel, gradient-norm median, 90th percentile, full-gradient median rms, worst): the tuples of
# tests/test_hip_train.py, unchanged — same networks, same operators, same dtypes
TINY_GATES = {torch.bfloat16: (4e-2, 1e-3, 7e-3, 2.6e-2, 0.11, 0.20), torch.float16: (5e-3, 1e-4, 7e-4, 3.3e-3, 1.5e-2, 2.3e-2)}
FULL_WIDTH_GATES = {torch.bfloat16: (3.5e-2, 1e-3, 8.5e-3, 1.2e-2, 3e-2, 8e-2), torch.float16: (4.5e-3, 2e-4, 5e-4, 1.1e-3, 4.5e-3, 8e-3)}
# measured on MI355X (profiles/r23c_gpu_suite_full.log), same order as the tuples; in brackets twice the deviation of the
# reference's own bf16 run from its fp32 run (the alternative bound of the first four statistics; never needed):
#   nav__   bf16 1.42e-2 [3.29e-2] | 1.5e-4 [1.7e-5] | 3.0e-3 [6.7e-3] | 9.1e-3 [2.1e-2] | 3.3e-2 | 8.1e-2
#           fp16 1.77e-3 | 2.1e-6 | 2.6e-4 | 9.1e-4 | 3.4e-3 | 7.4e-3
#   manip__ bf16 1.30e-2 [3.08e-2] | 5.3e-5 [8.6e-5] | 2.0e-3 [7.5e-3] | 7.9e-3 [2.4e-2] | 2.2e-2 | 6.7e-2
#           fp16 1.63e-3 | 1.3e-5 | 2.4e-4 | 9.6e-4 | 3.5e-3 | 8.5e-3
#   full__  bf16 1.19e-2 | 1.1e-4 | 5.6e-4 | 1.7e-3 | 1.6e-2 | 3.9e-2
#           fp16 1.48e-3 | 5.8e-6 | 1.3e-4 | 2.9e-4 | 1.9e-3 | 4.3e-3
# padded attention (7 shapes): bf16 max <= 4.8e-3, rms <= 3.2e-3; fp16 max <= 7.6e-4, rms <= 4.1e-4 (gate 2e-2 / 8e-3)
STAT_NAMES = ("prediction rms", "loss rel", "grad-norm median", "grad-norm 90%", "full-grad median rms", "full-grad worst rms")


def _is_dead(n):
    return ("transformer_blocks.0.norm2." in n) or (".attn2.to_q." in n) or (".attn2.to_k." in n) or n.startswith("add_embedding.")


def _norm_devs(names, norms, mine):
    dev = sorted((abs(mine[n] - nr) / max(nr, 1e-7) for n, nr in zip(names, norms) if not _is_dead(n)), reverse=True)
    return dev[len(dev) // 2], dev[len(dev) // 10]


def _reference_bf16_stats(g, pre):
    """What the REFERENCE's own bf16 run deviates from its fp32 run by, for the first four statistics (stored for the two tiny
    scenarios): the yardstick of 16-bit storage at this geometry that does not depend on the code under test."""
    if f"{pre}loss_ref_bf16" not in g.files:
        return None
    bits = np.ascontiguousarray(g[f"{pre}model_pred_ref_bf16_bits"]).view(np.int16)
    pred_b = torch.from_numpy(bits).view(torch.bfloat16).float()
    names = [str(n) for n in g[f"{pre}grad_names"]]
    med, p90 = _norm_devs(names, g[f"{pre}grad_norms"], dict(zip(names, g[f"{pre}grad_norms_ref_bf16"])))
    return (_rel(pred_b, torch.from_numpy(g[f"{pre}model_pred"]))[1],
            abs(float(g[f"{pre}loss_ref_bf16"]) - float(g[f"{pre}loss"])) / float(g[f"{pre}loss"]), med, p90)


def _step_against_reference(g, pre, dtype, gate, sd):
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import UNetTrain

    cfg = tails_config(pre)
    hip = Hip(torch.device(DEV), dtype)
    net = UNetTrain(cfg, sd, DEV, hip=hip)
    x = tails_inputs(g, pre)
    st = T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                        float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]),
                        dropout_prob=float(g["dropout_prob"]), random_p=torch.from_numpy(g["random_p"]))
    pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
    assert torch.isfinite(pred).all()
    stats = [_rel(pred, torch.from_numpy(g[f"{pre}model_pred"]))[1]]
    loss, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
    stats.append(abs(float(loss) - float(g[f"{pre}loss"])) / float(g[f"{pre}loss"]))
    grads = net.backward(dpred.reshape(pred.shape), loss_scale=1.0 if dtype == torch.bfloat16 else 2.0 ** 14)
    torch.cuda.synchronize()
    names, norms = [str(n) for n in g[f"{pre}grad_names"]], g[f"{pre}grad_norms"]
    # conditions, not measurements: every live parameter has a finite gradient of the master's shape, the dead classes none
    assert len(grads) == len(net.master) - 132
    mine = {}
    for n in names:
        if _is_dead(n):
            assert n not in grads, n
            continue
        assert n in grads, n
        assert tuple(grads[n].shape) == tuple(net.master[n].shape) and bool(torch.isfinite(grads[n]).all()), n
        mine[n] = float(grads[n].double().norm())
    stats += list(_norm_devs(names, norms, mine))
    full = []
    for key in g.files:
        if key.startswith(f"{pre}grad__") or key.startswith(f"{pre}grad8__"):
            name = key[len(pre):].split("__", 1)[1].replace("__", ".")
            r = torch.from_numpy(g[key])
            m = grads[name] if key.startswith(f"{pre}grad__") else grads[name].reshape(grads[name].shape[0], -1)[:8, :r.shape[1]]
            full.append((_rel(m.reshape(r.shape), r)[1], name))
    full.sort(reverse=True)
    assert len(full) >= 15
    stats += [full[len(full) // 2][0], full[0][0]]
    ref16 = _reference_bf16_stats(g, pre) if dtype == torch.bfloat16 else None
    print(f"[any size {pre} {dtype}] full gradients (rms rel error): " + ", ".join(f"{n.split('.')[-2]}.{n.split('.')[-1]} {e:.1e}" for e, n in full))
    failed = []
    for i, (nm, v, gt) in enumerate(zip(STAT_NAMES, stats, gate)):
        alt = 2.0 * ref16[i] if ref16 is not None and i < len(ref16) else None
        ok = v <= gt or (alt is not None and v <= alt)
        print(f"[any size {pre} {dtype}] {nm}: {v:.3e} (gate {gt:.1e}" + (f"; 2 x the reference's own bf16 run {alt:.3e}" if alt is not None else "") + f") {'ok' if ok else 'FAIL'}")
        if not ok:
            failed.append(nm)
    assert not failed, failed


@DTYPES
@pytest.mark.parametrize("pre", ["nav__", "manip__"])
def test_training_step_matches_reference_at_tail_sizes(golden, pre, dtype):
    """`prepare_step` -> `UNetTrain.forward` -> loss -> backward of the tiny network at 24x40 (levels of 960, 240, 60, 15 tokens)
    and, with the 10-channel manipulation embedder, at 56x56 (3136, 784, 196, 49) against the reference's `loss.backward()`.
    A statistic passes at its gate of `test_unet_training_step_matches_reference_gradients`, or (bf16) within twice what the
    reference's own bf16 run deviates from its fp32 run (factor 2: this tape also keeps its activation GRADIENTS in 16 bits)."""
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_tails.npz")
    _step_against_reference(g, pre, dtype, TINY_GATES[dtype], random_state_dict(tails_config(pre), int(g["weight_seed"])))


@pytest.fixture(scope="module")
def full_width_weights(golden):
    from wiw_amd.weights import random_state_dict

    return random_state_dict(tails_config("full__"), int(golden("train_step_tails.npz")["weight_seed"]))


@DTYPES
def test_served_width_training_step_matches_reference_at_tail_sizes(golden, full_width_weights, dtype):
    """The served width (320/640/1280/1280, 5/10/20/20 heads, 10 manipulation channels, 4 frames) at a 24x24 latent: levels of
    576, 144, 36 and 9 tokens, the padded attention at 20 heads; gates of `test_full_width_training_step_matches_reference_gradients`."""
    _step_against_reference(golden("train_step_tails.npz"), "full__", dtype, FULL_WIDTH_GATES[dtype], full_width_weights)


def test_trainer_on_manipulation_clips_at_56x56(golden, tmp_path):
    """`Trainer` with UNetConfig(task_type="manipulation", action_input_channel=10) at the deployed latent: three optimiser steps
    on one batch lower its loss; a validation rollout with (1, 4, 8) actions gives a finite PSNR; `save` writes a checkpoint the
    worker's loader resolves, and a fresh Trainer resumed from it repeats the fourth step bit for bit."""
    import serve_worker
    import wiw_amd  # noqa: F401
    from wiw_amd import checkpoint as C
    from wiw_amd import train as T
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import Trainer, UNetTrain
    from wiw_amd.weights import load_safetensors, random_state_dict, validate_state_dict

    g = golden("train_step_tails.npz")
    pre, cfg = "manip__", tails_config("manip__")
    hip = Hip(torch.device(DEV))
    sd = random_state_dict(cfg, int(g["weight_seed"]))
    x = tails_inputs(g, pre)
    st = T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                        float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]))
    a = Trainer(UNetTrain(cfg, sd, DEV, hip=hip), lr=1e-3)
    losses = [a.step(st), a.step(st), a.step(st)]
    print(f"[any size] Trainer at 56x56, manipulation: losses {losses}")
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
    sample = dict(image_latents=x["conditional_latents"], image_embeddings=x["encoder_hidden_states"], noise=x["noise"],
                  actions=g[f"{pre}actions"], target_latents=x["latents"])
    assert sample["actions"].shape == (1, 4, 8)
    val = a.validate([sample], num_steps=2)
    print(f"[any size] validation rollout: {val}")
    assert val["clips"] == 1 and np.isfinite(val["latent_psnr"]) and np.isfinite(val["latent_mse"])
    path = a.save(str(tmp_path), total_limit=1)
    served = serve_worker.resolve_unet_weights(path, "")
    assert served == os.path.join(path, C.UNET_FILE)
    validate_state_dict(cfg, load_safetensors(served))
    l4 = a.step(st)
    b = Trainer(UNetTrain(cfg, sd, DEV, hip=hip), lr=1e-3)
    b.load(C.resolve_resume(str(tmp_path), "latest"))
    assert b.steps == 3
    assert b.step(st) == l4
    for k in sd:
        assert torch.equal(a.net.master[k], b.net.master[k]) and torch.equal(a.m[k], b.m[k]) and torch.equal(a.v[k], b.v[k]), k
