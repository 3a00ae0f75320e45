"""Activation checkpointing of the training tape (`gradient_checkpointing=True`) — GPU side.  Both 16-bit libraries.

The kernels on the tape repeat bit for bit, the recomputed closures run in the plain run's order against the plain run's gradient
map: the checkpointed step IS the plain step.  Nothing here has a tolerance of its own.

  * forward + backward with the keyword off and on: prediction and every gradient `torch.equal`, same key set — the 16-row tape
    (tiny, 14 frames, 16x32), the 32-slot tape (t25__), the padded spatial attention (24x40: levels of 60 and 15 tokens) and the
    manipulation embedder at 17 frames (t17__, 16x16);
  * the checkpointed t25__ step at the existing gates against the reference's own `loss.backward()`;
  * bytes held between forward and backward, off and on, at the served width (full__: 8x16 latent, 25 frames) and for the tiny
    network at 32x64x14;
  * `Trainer`: two optimiser steps under grad_accum = 2 (clipped bf16, fp16 with the dynamic loss scale, frozen weights under
    "new+temp_layer"), an evaluation forward and `validate` in between: masters, both moments and the losses equal;
  * the checkpointed step at 25 frames repeats bit for bit.
"""
import numpy as np
import pytest
import torch

from test_hip_train_any_size import TINY_GATES
from test_hip_train_horizon import _step
from test_train_any_size import tails_config, tails_inputs
from test_train_horizon import NAME, horizon_config, horizon_inputs

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _n_segments(cfg):
    """Every ResBlock and transformer call of `UNetTrain.forward`: 14 down, 3 mid, 21 up at the served depth."""
    n, L = len(cfg.block_out_channels), cfg.layers_per_block
    return (L * n + L * (n - 1)) + 3 + ((L + 1) * n + (L + 1) * (n - 1))


def _scale(dtype):
    return 1.0 if dtype == torch.bfloat16 else 2.0 ** 14


def _fixture_step(g, pre, x, dropout=False):
    from wiw_amd import train as T

    kw = dict(dropout_prob=float(g["dropout_prob"]), random_p=torch.from_numpy(g["random_p"])) if dropout else {}
    return T.prepare_step(x["latents"], x["noise"], float(g[f"{pre}sigmas"][0]), x["conditional_latents"], x["encoder_hidden_states"],
                          float(g[f"{pre}noise_aug_strength"]), torch.from_numpy(g[f"{pre}action_ids"]), **kw)


def _drawn_step(cfg, h, w, seed=11):
    """A navigation step of `cfg` at an h x w latent from seeded draws (values rounded to bf16, as the fixtures' inputs)."""
    from wiw_amd import train as T
    from wiw_amd.pipeline import action_ids_idx_encode

    Tn = cfg.num_frames
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16).float()  # noqa: E731
    x = dict(latents=r(1, Tn, 4, h, w) * 0.8, noise=r(1, Tn, 4, h, w), conditional_latents=r(1, 4, h, w),
             encoder_hidden_states=r(1, 1, cfg.cross_attention_dim))
    acts = np.array([[4] + [[1, 2, 1, 3][i % 4] for i in range(Tn - 1)]])
    st = T.prepare_step(x["latents"], x["noise"], 1.3, x["conditional_latents"], x["encoder_hidden_states"], 0.04,
                        torch.from_numpy(action_ids_idx_encode(acts)))
    return x, acts, st


def _forward_backward(net, st, dtype):
    from wiw_amd import train as T

    pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
    ops = [f.__name__ for f in net.tape.ops]
    _, dpred = T.TrainStep(net.hip).loss_and_grad(pred, st)
    grads = net.backward(dpred.reshape(pred.shape), loss_scale=_scale(dtype))
    torch.cuda.synchronize()
    assert len(net.tape.ops) == 0 and len(net.tape.g) == 0 and len(net.tape.keep) == 0
    return pred.clone(), {k: v.clone() for k, v in grads.items()}, ops


def _assert_same_step(a, b, tag):
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]), tag
    assert set(a[1]) == set(b[1]) and len(a[1]) > 1000, tag
    for k, v in a[1].items():
        assert v.dtype == b[1][k].dtype and torch.equal(v, b[1][k]), (tag, k)


def _off_and_on(cfg, sd, st, dtype, tag, cls=None):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import make_unet_train

    hip = Hip(torch.device(DEV), dtype)
    make = cls or make_unet_train
    off = make(cfg, sd, DEV, hip=hip)
    on = make(cfg, sd, DEV, hip=hip, gradient_checkpointing=True)
    assert off.gradient_checkpointing is False and on.gradient_checkpointing is True
    r_off, r_on = _forward_backward(off, st, dtype), _forward_backward(on, st, dtype)
    _assert_same_step(r_off, r_on, tag)
    # between forward and backward: one closure per segment, and the operators outside the segments as they were
    assert "recompute" not in r_off[2]
    assert r_on[2].count("recompute") == _n_segments(cfg), tag
    outside = [n for n in r_on[2] if n != "recompute"]
    assert len(outside) < len(r_off[2]) - 10 * _n_segments(cfg), tag
    print(f"[checkpoint {tag} {dtype}] closures on the tape after forward: {len(r_off[2])} plain, {len(r_on[2])} checkpointed "
          f"({_n_segments(cfg)} segments); {len(r_off[1])} gradients equal")
    return on, type(off)


@DTYPES
def test_checkpointed_step_is_the_plain_step_on_the_16_row_tape(dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain
    from wiw_amd.weights import random_state_dict

    cfg = UNetConfig.tiny(14)
    _, _, st = _drawn_step(cfg, 16, 32)
    _, cls = _off_and_on(cfg, random_state_dict(cfg, 5), st, dtype, "tiny 14 frames 16x32")
    assert cls is UNetTrain


@DTYPES
def test_checkpointed_step_is_the_plain_step_on_the_32_slot_tape(golden, dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.train_unet import UNetTrain32
    from wiw_amd.weights import random_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    st = _fixture_step(g, pre, horizon_inputs(g, pre), dropout=True)
    _, cls = _off_and_on(cfg, random_state_dict(cfg, int(g["weight_seed"])), st, dtype, pre)
    assert cls is UNetTrain32


@DTYPES
@pytest.mark.parametrize("pre", ["nav__", "t17__"])
def test_checkpointed_step_is_the_plain_step_with_padded_attention_and_manipulation(golden, pre, dtype):
    """nav__ of train_step_tails.npz: 24x40, levels of 960, 240, 60 and 15 tokens — the two inner ones through `Hip.attn_padded`,
    whose saved set is rebuilt by the recompute.  t17__ of train_step_horizon.npz: the 10-channel manipulation embedder at 16x16
    (8 tokens at the innermost level: padded too) on the 32-slot tape."""
    import wiw_amd  # noqa: F401
    from wiw_amd.train_unet import UNetTrain, UNetTrain32, attn_level_plan
    from wiw_amd.weights import random_state_dict

    if pre == "nav__":
        g = golden("train_step_tails.npz")
        cfg, x, want = tails_config(pre), tails_inputs(g, pre), UNetTrain
        assert [Sp for _, Sp in attn_level_plan(24, 40)] == [0, 0, 64, 16]
    else:
        g = golden(NAME)
        cfg, x, want = horizon_config(pre), horizon_inputs(g, pre), UNetTrain32
        assert cfg.task_type == "manipulation" and tuple(x["latents"].shape[-2:]) == (16, 16)
    st = _fixture_step(g, pre, x, dropout=True)
    _, cls = _off_and_on(cfg, random_state_dict(cfg, int(g["weight_seed"])), st, dtype, pre)
    assert cls is want


@DTYPES
def test_checkpointed_step_passes_the_reference_gates_at_25_frames(golden, dtype):
    """The checkpointed t25__ step against the reference's own `loss.backward()`: `_step` of tests/test_hip_train_horizon.py, its
    six statistics and TINY_GATES, unchanged."""
    from wiw_amd.train_unet import make_unet_train
    from wiw_amd.weights import random_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    made = []

    def cls(*a, **k):
        made.append(make_unet_train(*a, gradient_checkpointing=True, **k))
        return made[-1]
    _step(g, pre, cfg, horizon_inputs(g, pre), dtype, TINY_GATES[dtype], random_state_dict(cfg, int(g["weight_seed"])), cls,
          "t25__ checkpointed")
    assert made[0].gradient_checkpointing is True


@pytest.fixture(scope="module")
def full_width_weights(golden):
    from wiw_amd.weights import random_state_dict

    return random_state_dict(horizon_config("full__"), int(golden(NAME)["weight_seed"]))


def _held(net, st):
    """Bytes the forward leaves allocated: `memory_allocated` right after it minus right before it."""
    if getattr(net, "tape", None) is not None:
        net.tape.release()
    net._out = None
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    del pred
    return held


# bytes held after the forward, checkpointed / plain, MEASURED on MI355X (profiles/r25b_grad_checkpoint_tests.log):
#   full__        bf16 81.88 / 1313.02 MiB = 0.0624, fp16 80.89 / 1304.10 MiB = 0.0620
#   tiny 32x64x14 bf16 and fp16 126.98 / 2212.07 MiB = 0.0574
HELD_RATIO_MEASURED = {"full__": 0.0624, "tiny 32x64x14": 0.0574}


@DTYPES
@pytest.mark.parametrize("case", ["full__", "tiny 32x64x14"])
def test_checkpointing_holds_fewer_bytes_after_the_forward(golden, full_width_weights, case, dtype):
    """What stays allocated between forward and backward, keyword off and on, on ONE tape in one process (the keyword is
    configuration: `forward` reads it).  Checkpointed, the tape holds the block-boundary tensors and the operators outside the
    segments; plain, every operator's saved tensors."""
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import make_unet_train
    from wiw_amd.weights import random_state_dict

    hip = Hip(torch.device(DEV), dtype)
    if case == "full__":
        g = golden(NAME)
        cfg, sd = horizon_config("full__"), full_width_weights
        st = _fixture_step(g, "full__", horizon_inputs(g, "full__"))
    else:
        cfg = UNetConfig.tiny(14)
        sd = random_state_dict(cfg, 5)
        _, _, st = _drawn_step(cfg, 32, 64)
    net = make_unet_train(cfg, sd, DEV, hip=hip)
    held = {False: [], True: []}
    for mode in (False, True, False, True, False, True):              # the first pair warms up: buffers the library keeps
        net.gradient_checkpointing = mode
        held[mode].append(_held(net, st))
    net.tape.release()
    off, on = held[False][1:], held[True][1:]
    ratio = max(on) / min(off)
    print(f"[checkpoint {case} {dtype}] held after forward (MiB): plain {[round(v / 2 ** 20, 2) for v in off]}, checkpointed "
          f"{[round(v / 2 ** 20, 2) for v in on]}, ratio {ratio:.4f}")
    assert max(on) < min(off)
    if case in HELD_RATIO_MEASURED:                                   # the project's convention: 1.25 x the measured value
        assert ratio <= 1.25 * HELD_RATIO_MEASURED[case]


@pytest.mark.parametrize("setup", ["bf16 clipped", "fp16 dynamic scale", "bf16 new+temp_layer"])
def test_trainer_steps_are_the_plain_trainer_steps(setup):
    """Two optimiser steps of four micro-batches (grad_accum = 2, autotune off) on the tiny 14-frame network at 16x32, with an
    evaluation forward and a validation rollout between them: every master parameter, both moments, the losses and the loss scale
    equal with the keyword off and on.  Under "new+temp_layer" the frozen weights' weight-gradient GEMMs are skipped inside the
    recomputed segments as in the plain run: the same parameters move."""
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import Trainer, make_unet_train
    from wiw_amd.weights import random_state_dict

    dtype = torch.float16 if setup.startswith("fp16") else torch.bfloat16
    kw = {"bf16 clipped": dict(max_grad_norm=0.5), "fp16 dynamic scale": {}, "bf16 new+temp_layer": dict(train_param_type="new+temp_layer")}[setup]
    cfg = UNetConfig.tiny(14)
    sd = random_state_dict(cfg, 5)
    x, acts, st = _drawn_step(cfg, 16, 32)
    _, _, st2 = _drawn_step(cfg, 16, 32, seed=12)
    sample = dict(image_latents=x["conditional_latents"], image_embeddings=x["encoder_hidden_states"], noise=x["noise"], actions=acts,
                  target_latents=x["latents"])
    hip = Hip(torch.device(DEV), dtype)
    runs = {}
    for mode in (False, True):
        net = make_unet_train(cfg, sd, DEV, hip=hip, gradient_checkpointing=mode)
        tr = Trainer(net, lr=1e-3, grad_accum=2, autotune=False, **kw)
        losses = [tr.step(st), tr.step(st2)]
        # evaluation: a forward that no backward follows, then the served loop beside the tape it left
        net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
        left = net.tape
        assert len(left.ops) > 0
        val = tr.validate([sample], num_steps=2)
        assert val["clips"] == 1 and np.isfinite(val["latent_psnr"]) and np.isfinite(val["latent_mse"])
        losses += [tr.step(st2), tr.step(st)]
        assert len(left.ops) == 0 and len(left.g) == 0 and len(left.keep) == 0          # released by the next forward
        assert len(net.tape.ops) == 0 and len(net.tape.g) == 0 and len(net.tape.keep) == 0
        torch.cuda.synchronize()
        assert all(np.isfinite(losses))
        runs[mode] = (losses, tr.steps, tr.loss_scale, val, {k: v.clone() for k, v in net.master.items()},
                      {k: v.clone() for k, v in tr.m.items()}, {k: v.clone() for k, v in tr.v.items()}, tr.grad_norm)
    off, on = runs[False], runs[True]
    print(f"[checkpoint trainer {setup}] losses {on[0]}, optimiser steps {on[1]}, loss scale {on[2]}, grad norm {on[7]}")
    assert off[0] == on[0] and off[1] == on[1] and off[2] == on[2] and off[3] == on[3] and off[7] == on[7]
    assert on[1] >= 1
    moved = 0
    for k in sd:
        assert torch.equal(off[4][k], on[4][k]) and torch.equal(off[5][k], on[5][k]) and torch.equal(off[6][k], on[6][k]), k
        moved += not torch.equal(on[4][k].cpu(), torch.from_numpy(np.asarray(sd[k])).float())
    assert moved > 0
    if setup == "bf16 new+temp_layer":
        assert moved < len(sd) // 2


@DTYPES
def test_checkpointed_step_at_25_frames_repeats_bit_for_bit(golden, dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import make_unet_train
    from wiw_amd.weights import random_state_dict

    g, pre = golden(NAME), "t25__"
    cfg = horizon_config(pre)
    hip = Hip(torch.device(DEV), dtype)
    net = make_unet_train(cfg, random_state_dict(cfg, int(g["weight_seed"])), DEV, hip=hip, gradient_checkpointing=True)
    st = _fixture_step(g, pre, horizon_inputs(g, pre))
    a, b = _forward_backward(net, st, dtype), _forward_backward(net, st, dtype)
    _assert_same_step(a, b, "t25__ checkpointed, twice")
