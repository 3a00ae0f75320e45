"""Fine-tuning at every served horizon (17 .. 32 frames, 25 = SVD-XT) — GPU side.  Both 16-bit libraries.

  * the temporal self-attention of `UNetTrain32` — `wiw_attn_temporal32_bf16` forward on the (b, t, s) rows, row maps at
    Tp = 32 around the one-wave backward — through the tape's OWN forward call and backward closure, against torch fp32 autograd;
  * `UNetTrain32` at 4 frames on the 16-row tape's fixture (train_step_tiny.npz): the same operator;
  * the whole training step against the reference's own `loss.backward()` at 25 and 17 frames and at the served width with 25
    frames (tests/golden/train_step_horizon.npz, written by tools/make_golden_train_horizon.py);
  * bit-repeatability of forward + backward at 25 frames;
  * `Trainer` at 25 frames: steps, save / resume, and the checkpoint served by `UNetHIP`.
"""
import os

import numpy as np
import pytest
import torch

from test_hip_train_any_size import (FULL_WIDTH_GATES, STAT_NAMES, TINY_GATES, _is_dead, _norm_devs, _poison, _reference_bf16_stats,
                                     _rel, _rnd)
from test_train_horizon import NAME, horizon_config, horizon_inputs

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _attention_only_tape(hip, T):
    """A `UNetTrain32` without weights whose `linear` hands back its input: `self_attention(qkv, ...)` then runs the temporal
    attention of the tape on a q|k|v tensor the test owns, and leaves the attention's backward closure on the tape."""
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import Tape, UNetTrain32

    net = UNetTrain32(UNetConfig.tiny(T), {}, DEV, hip=hip)
    net.linear = lambda x, *a, **k: x
    net.tape, net.grads = Tape(hip), {}
    return net


@DTYPES
@pytest.mark.parametrize("T", [17, 24, 25, 31, 32])
def test_temporal_attention_of_the_32_slot_tape(T, dtype):
    """O and dQ, dK, dV of softmax(Q K^T / 8) V over the T frames of every site, for sites Ssp in {1, 9, 49}, heads in {1, 5} and
    batch in {1, 2} (batch * Ssp * heads is not always a multiple of the 4 waves of a workgroup), against torch autograd in fp32
    on the same 16-bit-rounded q, k, v and dO: the kernel pair's tolerance (max 2e-2, rms 8e-3 relative,
    tests/test_hip_train.py `test_attention_backward`).  The q|k|v tensor carries 64 NaN rows after its last frame — where frames
    T+1 .. 32 of the last clip would lie — and every buffer the closure allocates comes from a NaN-poisoned allocator: no NaN may
    reach O or d_qkv, the outputs have exactly M rows and repeat bit for bit."""
    import torch.nn.functional as F

    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV), dtype)
    r16 = lambda t: t.to(dtype).float()  # noqa: E731
    for Ssp in (1, 9, 49):
        for heads in (1, 5):
            for batch in (1, 2):
                C, M, nseq = heads * 64, batch * T * Ssp, batch * Ssp
                qkv, dO = r16(_rnd(M, 3 * C, seed=T + Ssp)), r16(_rnd(M, C, seed=100 + T + heads))
                leaf = qkv.clone().requires_grad_(True)

                def hd(t):                                                  # rows (b, t, s) -> (b, s, head, t, 64)
                    return t.reshape(batch, T, Ssp, heads, 64).permute(0, 2, 3, 1, 4)

                o_ref = F.scaled_dot_product_attention(hd(leaf[:, :C]), hd(leaf[:, C:2 * C]), hd(leaf[:, 2 * C:]))
                o_ref = o_ref.permute(0, 3, 1, 2, 4).reshape(M, C)
                o_ref.backward(dO)
                qkv_d = torch.full((M + 64, 3 * C), float("nan"), dtype=dtype, device=DEV)
                qkv_d[:M] = qkv.to(DEV, dtype)
                dO_d = dO.to(DEV, dtype)
                sizes = [nseq * 32 * 3 * C, nseq * 32 * C, M * C, M * 3 * C, nseq * heads * 32]

                def run():
                    net = _attention_only_tape(hip, T)
                    _poison(sizes, dtype)
                    o = net.self_attention(qkv_d, "attn1", M, batch, Ssp, heads, temporal_T=T)
                    assert len(net.tape.ops) == 1
                    net.tape.add(o, dO_d)
                    _poison(sizes, dtype)
                    net.tape.ops.pop()()
                    dq = net.tape.take(qkv_d)
                    torch.cuda.synchronize()
                    return o, dq
                O, dqkv = run()
                tag = f"[horizon {dtype}] temporal attention T={T} sites={Ssp} heads={heads} batch={batch}"
                assert tuple(O.shape) == (M, C) and tuple(dqkv.shape) == (M + 64, 3 * C), tag
                assert float(dqkv[M:].float().abs().max()) == 0.0, tag              # the tape pads a gradient to ITS tensor's rows
                dqkv = dqkv[:M]
                assert torch.isfinite(O.float()).all() and torch.isfinite(dqkv.float()).all(), tag
                mx, rms = _rel(O, o_ref)
                print(f"{tag} O: max_rel={mx:.2e} rms={rms:.2e}")
                assert mx <= 2e-2 and rms <= 8e-3, tag
                for name, sl in (("dQ", slice(0, C)), ("dK", slice(C, 2 * C)), ("dV", slice(2 * C, 3 * C))):
                    mx, rms = _rel(dqkv[:, sl], leaf.grad[:, sl])
                    print(f"{tag} {name}: max_rel={mx:.2e} rms={rms:.2e}")
                    assert mx <= 2e-2 and rms <= 8e-3, (tag, name)
                O2, dqkv2 = run()
                assert torch.equal(O, O2) and torch.equal(dqkv, dqkv2[:M]), tag


# ---- the whole step against the reference -----------------------------------------------------------------------------
# Gates: TINY_GATES / FULL_WIDTH_GATES of tests/test_hip_train_any_size.py (the project's gates for these networks and dtypes),
# and for bf16 alternatively twice the deviation of the reference's own bf16 run from its fp32 run.
# (the values measured on MI355X: MEASURED, below these tests)
def _step(g, pre, cfg, x, dtype, gate, sd, cls, tag):
    """The six statistics and the pass rule of tests/test_hip_train_any_size.py `_step_against_reference`, for any tape class,
    config and input set.  Returns the statistics."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV), dtype)
    net = cls(cfg, sd, DEV, hip=hip)
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
    assert set(names) <= set(net.master)
    dead = sum(_is_dead(n) for n in net.master)
    assert dead > 0 and len(grads) == len(net.master) - dead
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
    print(f"[horizon {tag} {dtype}] full gradients (rms rel error): " + ", ".join(f"{n.split('.')[-2]}.{n.split('.')[-1]} {e:.1e}" for e, n in full))
    failed = []
    for i, (nm, v, gt) in enumerate(zip(STAT_NAMES, stats, gate)):
        alt = 2.0 * ref16[i] if ref16 is not None and i < len(ref16) else None
        ok = v <= gt or (alt is not None and v <= alt)
        print(f"[horizon {tag} {dtype}] {nm}: {v:.3e} (gate {gt:.1e}" + (f"; 2 x the reference's own bf16 run {alt:.3e}" if alt is not None else "") + f") {'ok' if ok else 'FAIL'}")
        if not ok:
            failed.append(nm)
    assert not failed, failed
    return stats


@DTYPES
def test_32_slot_tape_is_the_16_row_tape_at_4_frames(golden, dtype):
    """`UNetTrain32` at T = 4 on the 16-row tape's own fixture (tests/golden/train_step_tiny.npz) at that tape's gates: the 32-slot
    temporal attention is the same operator."""
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain32
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_tiny.npz")
    cfg = UNetConfig.tiny(4)
    x = {k: torch.from_numpy(g[k]) for k in ("latents", "noise", "conditional_latents", "encoder_hidden_states")}
    _step(g, "", cfg, x, dtype, TINY_GATES[dtype], random_state_dict(cfg, int(g["weight_seed"])), UNetTrain32, "tiny T=4")


@DTYPES
@pytest.mark.parametrize("pre", ["t25__", "t17__"])
def test_training_step_matches_reference_at_long_horizons(golden, pre, dtype):
    """`prepare_step` -> `make_unet_train(...).forward` -> loss -> backward of the tiny network at 25 frames (16x32 latent: 512,
    128, 32 and 8 tokens, the padded spatial attention at 8 next to the 32-slot temporal one) and, with the 10-channel
    manipulation embedder, at 17 frames (one frame in the second 16-row fragment) against the reference's `loss.backward()`."""
    from wiw_amd.train_unet import UNetTrain32, make_unet_train
    from wiw_amd.weights import random_state_dict

    g = golden(NAME)
    cfg = horizon_config(pre)
    made = []

    def cls(*a, **k):
        made.append(make_unet_train(*a, **k))
        return made[-1]
    _step(g, pre, cfg, horizon_inputs(g, pre), dtype, TINY_GATES[dtype], random_state_dict(cfg, int(g["weight_seed"])), cls, pre)
    assert type(made[0]) is UNetTrain32


@pytest.fixture(scope="module")
def full_width_weights(golden):
    from wiw_amd.weights import random_state_dict

    return random_state_dict(horizon_config("full__"), int(golden(NAME)["weight_seed"]))


@DTYPES
def test_served_width_training_step_matches_reference_at_25_frames(golden, full_width_weights, dtype):
    """The served width (320/640/1280/1280, 5/10/20/20 heads, 25 navigation channels) at 25 frames on an 8x16 latent: the 32-slot
    temporal attention at 20 heads; gates of `test_full_width_training_step_matches_reference_gradients`."""
    from wiw_amd.train_unet import make_unet_train

    g = golden(NAME)
    _step(g, "full__", horizon_config("full__"), horizon_inputs(g, "full__"), dtype, FULL_WIDTH_GATES[dtype], full_width_weights,
          make_unet_train, "full__")


# MEASURED on MI355X (profiles/r24a_train_horizon_tests.log), same order as STAT_NAMES; in brackets twice the deviation of the
# reference's own bf16 run from its fp32 run (the alternative bound of the first four statistics; never needed):
#   tiny T=4 (UNetTrain32) bf16 1.39e-2 | 4.1e-5 | 2.2e-3 | 8.3e-3 | 3.8e-2 | 6.3e-2
#                          fp16 1.74e-3 | 4.5e-6 | 2.5e-4 | 1.0e-3 | 4.7e-3 | 8.0e-3
#   t25__  bf16 1.50e-2 [3.49e-2] | 4.6e-6 [1.5e-5] | 2.3e-3 [8.5e-3] | 8.4e-3 [2.8e-2] | 2.8e-2 | 6.8e-2
#          fp16 1.86e-3 | 4.1e-7 | 2.6e-4 | 1.1e-3 | 4.1e-3 | 8.7e-3
#   t17__  bf16 1.36e-2 [3.24e-2] | 6.2e-5 [2.8e-4] | 2.6e-3 [8.7e-3] | 7.7e-3 [2.3e-2] | 2.6e-2 | 6.6e-2
#          fp16 1.72e-3 | 4.1e-6 | 3.0e-4 | 1.2e-3 | 3.6e-3 | 8.8e-3
#   full__ bf16 1.27e-2 | 1.3e-4 | 1.6e-3 | 3.3e-3 | 1.6e-2 | 6.1e-2
#          fp16 1.57e-3 | 1.9e-5 | 6.0e-5 | 2.1e-4 | 1.9e-3 | 4.9e-3
# temporal attention of the 32-slot tape (60 shapes per dtype; O, dQ, dK, dV): bf16 max <= 6.3e-3, rms <= 2.9e-3; fp16 max <=
# 7.3e-4, rms <= 3.5e-4 (gate 2e-2 / 8e-3).  UNetHIP on the 25-frame checkpoint vs UNetTrain32.forward: rms 1.36e-2 (gate 4e-2).


@DTYPES
def test_step_at_25_frames_repeats_bit_for_bit(golden, dtype):
    """Two forward + backward runs of t25__ on one tape: identical predictions and gradients (fixed summation orders everywhere,
    the 32-slot attention and its backward included)."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import make_unet_train
    from wiw_amd.weights import random_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    hip = Hip(torch.device(DEV), dtype)
    net = make_unet_train(cfg, random_state_dict(cfg, int(g["weight_seed"])), DEV, hip=hip)
    x = horizon_inputs(g, pre)
    st = T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                        float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]))
    runs = []
    for _ in range(2):
        pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
        _, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
        grads = net.backward(dpred.reshape(pred.shape), loss_scale=1.0 if dtype == torch.bfloat16 else 2.0 ** 14)
        runs.append((pred.clone(), {k: v.clone() for k, v in grads.items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 1000
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


def test_trainer_at_25_frames_and_its_checkpoint_serves(golden, tmp_path):
    """`Trainer` on the tiny 25-frame network (modelled on `test_trainer_on_manipulation_clips_at_56x56`): two optimiser steps
    with finite losses; `save` writes a checkpoint the worker's loader resolves; a fresh Trainer resumed from it repeats the third
    step bit for bit; the checkpoint's UNet loads into `UNetHIP(UNetConfig.tiny(25))` without conversion, and one inference
    forward agrees with the training forward of the same weights.

    That last tolerance: both are bf16 evaluations of one function in different operator fusions.  The project gates the bf16
    training forward of this network at rms 4e-2 of the fp32 reference (TINY_GATES, prediction rms; measured ~1.4e-2), the
    inference forward at the reference's own bf16 deviation (~1.4e-2 here: t25__model_pred_ref_bf16_bits): two such errors apart
    stay within the one gate, 4e-2."""
    import serve_worker
    import wiw_amd  # noqa: F401
    from wiw_amd import checkpoint as C
    from wiw_amd import train as T
    from wiw_amd.config import UNetConfig
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import Trainer, UNetTrain32, make_unet_train
    from wiw_amd.unet import UNetHIP
    from wiw_amd.weights import load_safetensors, random_state_dict, validate_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    assert cfg == UNetConfig.tiny(25)
    hip = Hip(torch.device(DEV))
    sd = random_state_dict(cfg, int(g["weight_seed"]))
    x = horizon_inputs(g, pre)
    st = T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                        float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]))
    a = Trainer(make_unet_train(cfg, sd, DEV, hip=hip), lr=1e-3)
    assert type(a.net) is UNetTrain32
    losses = [a.step(st), a.step(st)]
    print(f"[horizon] Trainer at 25 frames: losses {losses}")
    assert all(np.isfinite(losses)) and a.steps == 2
    path = a.save(str(tmp_path), total_limit=1)
    served = serve_worker.resolve_unet_weights(path, "")
    assert served == os.path.join(path, C.UNET_FILE)
    weights = load_safetensors(served)
    validate_state_dict(cfg, weights)
    assert tuple(weights["add_action_proj.proj.weight"].shape)[1] == 25 * 12          # the 25-channel action embedder
    l3 = a.step(st)
    b = Trainer(make_unet_train(cfg, sd, DEV, hip=hip), lr=1e-3)
    b.load(C.resolve_resume(str(tmp_path), "latest"))
    assert b.steps == 2
    # the resumed weights, served: one inference forward against the training forward
    unet = UNetHIP(cfg, weights, DEV, hip=hip)
    served_out = unet(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids).float().cpu()
    train_out = b.net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids).float().cpu()
    mx, rms = _rel(served_out.reshape(train_out.shape), train_out)
    print(f"[horizon] UNetHIP on the 25-frame checkpoint vs UNetTrain32.forward: max_rel={mx:.2e} rms={rms:.2e}")
    assert torch.isfinite(served_out).all() and rms <= TINY_GATES[torch.bfloat16][0]
    assert b.step(st) == l3
    for k in sd:
        assert torch.equal(a.net.master[k], b.net.master[k]) and torch.equal(a.m[k], b.m[k]) and torch.equal(a.v[k], b.v[k]), k


def _t25(golden):
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.weights import random_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    x = horizon_inputs(g, pre)
    st = T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                        float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]))
    return g, cfg, random_state_dict(cfg, int(g["weight_seed"])), x, st


def test_gradient_accumulation_and_validation_rollout_at_25_frames(golden):
    """The rest of the loop at 25 frames.  Two micro-batches of the same sample under grad_accum = 2 give g/2 + g/2 = g exactly:
    the parameters of one plain step, bit for bit, and no update on the first micro-batch.  `validate` rolls the 25-frame clip
    out on `UNetHIP` with (1, 25) navigation actions and returns finite numbers."""
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import Trainer, make_unet_train

    g, cfg, sd, x, st = _t25(golden)
    hip = Hip(torch.device(DEV))
    one = make_unet_train(cfg, sd, DEV, hip=hip)
    Trainer(one, lr=1e-3).step(st)
    two = make_unet_train(cfg, sd, DEV, hip=hip)
    tr = Trainer(two, lr=1e-3, grad_accum=2)
    tr.step(st)
    key = "conv_in.weight"
    assert torch.equal(two.master[key].cpu(), torch.from_numpy(np.asarray(sd[key]))) and tr.steps == 0
    tr.step(st)
    assert tr.steps == 1
    assert max(float((two.master[k] - one.master[k]).abs().max()) for k in sd) == 0.0
    sample = dict(image_latents=x["conditional_latents"], image_embeddings=x["encoder_hidden_states"], noise=x["noise"],
                  actions=g["t25__actions"], target_latents=x["latents"])
    assert sample["actions"].shape == (1, 25)
    val = tr.validate([sample], num_steps=2)
    print(f"[horizon] validation rollout at 25 frames: {val}")
    assert val["clips"] == 1 and np.isfinite(val["latent_psnr"]) and np.isfinite(val["latent_mse"])


def test_sharded_adamw_single_rank_at_25_frames(golden):
    """`Trainer` + `parallel.ShardedAdamW` (the ZeRO-1 path; a one-rank `nccl` group, as
    `test_trainer_with_sharded_adamw_over_rccl_single_rank`) on the 25-frame tape: the flat layout holds the 300-column
    `add_action_proj`, the second step hands its buckets over during the backward — the 32-slot attention's closure included —
    and the parameters equal the single-process update bit for bit."""
    import socket

    import torch.distributed as dist

    from wiw_amd.hip import Hip
    from wiw_amd.parallel import ShardedAdamW
    from wiw_amd.train_unet import Trainer, make_unet_train

    g, cfg, sd, x, st = _t25(golden)
    hip = Hip(torch.device(DEV))
    solo = make_unet_train(cfg, sd, DEV, hip=hip)
    solo_tr = Trainer(solo, lr=1e-3)
    solo_tr.step(st)
    solo_tr.step(st)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        net = make_unet_train(cfg, sd, DEV, hip=hip)
        assert tuple(net.master["add_action_proj.proj.weight"].shape)[1] == 300
        opt = ShardedAdamW({k: tuple(v.shape) for k, v in net.master.items()}, torch.device(DEV),
                           lambda p, gr, m, v, step, lr, b1, b2, eps, wd: hip.adamw_step(p, gr, m, v, step, lr, b1, b2, eps, wd),
                           bucket_elems=1 << 20, lr=1e-3)
        tr = Trainer(net, lr=1e-3, optimizer=opt)
        tr.step(st)
        tr.step(st)
        assert opt.async_launched >= opt.n_buckets - 1, (opt.async_launched, opt.n_buckets)
        live = [k for k in sd if not torch.equal(solo.master[k].cpu(), torch.from_numpy(np.asarray(sd[k])))]
        assert len(live) > 1000
        diff = max(float((net.master[k] - solo.master[k]).abs().max()) for k in live)
        assert diff == 0.0, diff
    finally:
        dist.destroy_process_group()
