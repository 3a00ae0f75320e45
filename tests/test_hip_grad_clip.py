"""Global-norm gradient clipping on the GPU: the sum-of-squares / finalise kernels against torch in float64, the AdamW
kernel with a device-side gradient scale against the plain one, and `Trainer(max_grad_norm=)` on the reference-pinned
fixtures (the reference's own global gradient norm is sqrt(sum(grad_norms^2)) of the fixture: tests/test_grad_clip.py)."""
import math
import os
import socket

import numpy as np
import pytest
import torch

DEV = "cuda:0"
N_REF_TINY, N_REF_FULL = 1.3216, 5.9572        # pinned by tests/test_grad_clip.py::test_reference_global_norm_anchors
# the per-tensor gradient-norm gates (90th percentile) of tests/test_hip_train.py: `tiny_gate[3]` in
# test_unet_training_step_matches_reference_gradients and `FULL_WIDTH_GATES[dtype][3]`
TINY_NORM_GATE = {torch.bfloat16: 2.6e-2, torch.float16: 3.3e-3}
FULL_NORM_GATE = {torch.bfloat16: 1.2e-2, torch.float16: 1.1e-3}


def _sum_bound(L: int) -> float:
    """fp32 pairwise summation inside a chunk of L elements: relative error <= about (log2(L) + 2) 2^-24 (the squares'
    rounding and the head / tail term included); the double-precision finalise adds nothing visible.  The tests assert
    against TWICE this.  For the library's L = 16384: 16 * 2^-24 = 9.5e-7, asserted 1.9e-6."""
    return (math.log2(L) + 2) * 2.0 ** -24


def _hip(dtype=torch.bfloat16):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    return Hip(torch.device(DEV), dtype)


def _check_against_float64(hip, tensors, what, max_norm=0.5):
    rec = hip.grad_sumsq(tensors, max_norm).tolist()
    ref = sum(float(t.double().pow(2).sum()) for t in tensors)
    L = hip.sumsq_chunk
    bound = 2 * _sum_bound(L)                                   # L = 16384: 2 * 9.5e-7
    rel = abs(rec[0] - ref) / ref
    rel_n = abs(rec[1] - math.sqrt(ref)) / math.sqrt(ref)
    print(f"[clip] {what}: sumsq rel err {rel:.2e}, norm rel err {rel_n:.2e} (L = {L}, asserted bound {bound:.2e})")
    assert rel <= bound and rel_n <= bound
    coef = np.float32(max_norm) / (np.float32(rec[1]) + np.float32(1e-6))
    assert rec[2] == float(min(np.float32(1.0), coef)) and rec[3] == 1.0
    return rec


@pytest.mark.gpu
def test_sumsq_kernel_against_float64():
    hip = _hip()
    gen = torch.Generator().manual_seed(0)
    # (a) one flat tensor: 5 whole chunks and a ragged one
    flat = torch.randn(5 * hip.sumsq_chunk + 777, generator=gen).to(DEV)
    _check_against_float64(hip, [flat], "one flat tensor")
    # (b) many tensors of awkward lengths carved out of one buffer at offsets that break 16-byte alignment
    buf = torch.randn(400000, generator=gen).to(DEV)
    tensors, off = [], 1
    for i, n in enumerate([1, 3, 4, 5, 1023, 100003, 1, 5, 3, 100003, 4, 1023]):
        tensors.append(buf[off:off + n])
        off += n + (i % 4)                                      # every residue of the address mod 16 occurs
    assert {t.data_ptr() % 16 for t in tensors} == {0, 4, 8, 12}
    rec = _check_against_float64(hip, tensors, "12 tensors, lengths 1..100003, misaligned")
    # each of them alone too (a single element, a head-only tensor, ...)
    for t in tensors[:6]:
        _check_against_float64(hip, [t], f"alone, n = {t.numel()}, address % 16 = {t.data_ptr() % 16}")
    # (c) bit-repeatable, and independent of the grid: the element -> partial mapping and the order inside a partial depend
    # on the table alone; blocks only decide which workgroup computes a partial
    assert hip.grad_sumsq(tensors, 0.5).tolist() == rec        # (the list changed back from the single tensors: one upload)
    uploads = hip.sumsq_table_uploads
    for blocks in (0, 0, 1, 7, 1000):
        again = hip.grad_sumsq(tensors, 0.5, blocks=blocks).tolist()
        assert [np.float32(x).tobytes() for x in again] == [np.float32(x).tobytes() for x in rec], (blocks, again, rec)
    assert hip.sumsq_table_uploads == uploads                  # same addresses and sizes: the table was not sent again
    hip.grad_sumsq(tensors[:5], 0.5)
    assert hip.sumsq_table_uploads == uploads + 1              # ... and a changed list goes up as ONE copy
    # (d) the two halves separately (the sharded optimiser's use): sum only, then the coefficient from a given sum
    half = hip.grad_sumsq(tensors)
    assert half.tolist()[0] == rec[0] and half.tolist()[1:] == [0.0, 0.0, 0.0]
    assert hip.clip_coef(half, 0.5).tolist() == rec
    # (e) a coefficient of exactly 1 below the threshold
    small = [t * 1e-4 for t in tensors]
    r = hip.grad_sumsq(small, 0.5).tolist()
    assert r[1] < 0.5 and r[2] == 1.0


@pytest.mark.gpu
def test_sumsq_of_the_tiny_unet_gradients(golden):
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_tiny.npz")
    cfg = UNetConfig.tiny(4)
    hip = _hip()
    net = UNetTrain(cfg, random_state_dict(cfg, int(g["weight_seed"])), DEV, hip=hip)
    st = _tiny_step(g)
    pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
    _, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
    grads = net.backward(dpred.reshape(pred.shape))
    tensors = [v.reshape(-1).contiguous() for v in grads.values()]
    assert len(tensors) > 1000 and min(t.numel() for t in tensors) == 1
    _check_against_float64(hip, tensors, f"the {len(tensors)} gradient tensors of the tiny UNet")


@pytest.mark.gpu
def test_sumsq_beyond_2_to_31_elements_is_exact():
    hip = _hip()
    n = 2 ** 31 + 12345                                         # 8.6 GB of fp32, an odd length
    x = torch.zeros(n, dtype=torch.float32, device=DEV)
    idx = torch.tensor([2 ** 31 + 1, 2 ** 31 + 4097, 2 ** 31 + 12000, n - 1, n - 2], device=DEV)
    x[idx] = 1.0
    rec = hip.grad_sumsq([x], 10.0).tolist()
    assert rec == [5.0, float(np.float32(math.sqrt(5.0))), 1.0, 1.0], rec
    del x
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_inputs_surface(bad):
    hip = _hip()
    gen = torch.Generator().manual_seed(1)
    tensors = [torch.randn(n, generator=gen).to(DEV) for n in (70001, 5, 1)]
    for t, i in ((0, 33333), (0, 70000), (1, 2), (2, 0)):       # the vector body, the scalar tail, a short tensor, a single element
        cur = [x.clone() for x in tensors]
        cur[t][i] = bad
        rec = hip.grad_sumsq(cur, 0.5).tolist()
        assert rec[3] == 0.0 and not math.isfinite(rec[0]) and not math.isfinite(rec[1]), (t, i, rec)
        assert not (0.0 < rec[2] <= 1.0) or rec[2] != rec[2], rec      # never a usable-looking coefficient: 0 (Inf) or NaN


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_adamw_with_a_device_scale_equals_the_plain_kernel(dtype):
    hip = _hip(dtype)
    n = 100003                                                  # odd: the vector body and the scalar tail
    for scale in (1.0, 0.3783, 0.0839):                         # 1, and the reference threshold's coefficients on the two fixtures
        gen = torch.Generator().manual_seed(7)
        p0 = torch.randn(n, generator=gen)
        s = torch.tensor([scale], dtype=torch.float32, device=DEV)
        a = [p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=dtype, device=DEV)]
        b = [t.clone() for t in a]
        for step in range(1, 6):
            gr = torch.randn(n, generator=gen).to(DEV)
            keep = gr.clone()
            hip.adamw_step(a[0], gr, a[1], a[2], step, 3e-3, beta1=0.9, beta2=0.95, weight_decay=0.05, p16=a[3], grad_scale=s)
            assert torch.equal(gr, keep)                        # the clipped gradient is never written
            pre = gr if scale == 1.0 else gr * s                # fp32 product, rounded: what the kernel must reproduce
            hip.adamw_step(b[0], pre, b[1], b[2], step, 3e-3, beta1=0.9, beta2=0.95, weight_decay=0.05, p16=b[3])
            for x, y, what in zip(a, b, ("p", "m", "v", "p16")):
                assert torch.equal(x, y), (scale, step, what, float((x.float() - y.float()).abs().max()))


# ----------------------------------------------------------------------------------------------------------------
# Trainer
# ----------------------------------------------------------------------------------------------------------------
def _tiny_step(g):
    from wiw_amd import train as T

    return T.prepare_step(torch.from_numpy(g["latents"]), torch.from_numpy(g["noise"]), float(g["sigmas"][0]),
                          torch.from_numpy(g["conditional_latents"]), torch.from_numpy(g["encoder_hidden_states"]),
                          float(g["noise_aug_strength"]), torch.from_numpy(g["action_ids"]))


def _tiny(g, dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain
    from wiw_amd.weights import random_state_dict

    cfg = UNetConfig.tiny(4)
    hip = _hip(dtype)
    sd = random_state_dict(cfg, int(g["weight_seed"]))
    return hip, sd, (lambda: UNetTrain(cfg, sd, DEV, hip=hip))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_trainer_clips_at_the_reference_threshold(golden, dtype):
    """`max_grad_norm = 0.5` (FTsvd/config/accelerate_deepspeed_o1_config.yaml) on the tiny fixture, one step: the norm the
    trainer reports against the reference's own backward, and the update against the plain AdamW kernel on the trainer's own
    gradients pre-multiplied in fp32 by 0.5 / (grad_norm + 1e-6).
    Measured on MI355X (printed below): grad_norm 1.320806 in bf16 (6.0e-4 from the reference), 1.321668 in fp16
    (5.2e-5)."""
    from wiw_amd.train_unet import Trainer

    g = golden("train_step_tiny.npz")
    hip, sd, make = _tiny(g, dtype)
    st = _tiny_step(g)
    lr = 1e-3
    net = make()
    tr = Trainer(net, lr=lr, weight_decay=0.0, max_grad_norm=0.5)
    tr.step(st)
    dev = abs(tr.grad_norm - N_REF_TINY) / N_REF_TINY
    print(f"[clip {dtype}] tiny fixture: Trainer.grad_norm {tr.grad_norm:.6f} vs the reference's {N_REF_TINY} (rel dev {dev:.2e}, "
          f"gate {TINY_NORM_GATE[dtype]:.1e}), coefficient {tr.clip_coef:.6f}")
    assert dev <= TINY_NORM_GATE[dtype]
    assert tr.clip_coef < 1.0 and abs(tr.clip_coef - 0.5 / (tr.grad_norm + 1e-6)) <= 1e-6
    # replay: the plain kernel on copies of the trainer's gradients, pre-multiplied in fp32 by the coefficient
    coef = np.float32(0.5) / (np.float32(tr.grad_norm) + np.float32(1e-6))          # fp32, as the finalise kernel computes it
    assert float(coef) == tr.clip_coef
    coef = torch.tensor([coef], dtype=torch.float32, device=DEV)
    moved = 0
    for name, gr in net.grads.items():
        if not tr.trainable(name):
            continue
        p = torch.from_numpy(np.asarray(sd[name])).to(DEV, torch.float32).reshape(-1).clone()
        p_start = p.clone()
        pre = gr.reshape(-1).contiguous().clone() * coef
        hip.adamw_step(p, pre, torch.zeros_like(p), torch.zeros_like(p), 1, lr, weight_decay=0.0)
        assert torch.equal(p, net.master[name].reshape(-1)), name
        assert float((p - p_start).abs().max()) <= 1.01 * lr, name
        moved += int(not torch.equal(p, p_start))
    assert moved > 1000
    dead = "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.weight"
    assert torch.equal(net.master[dead].cpu(), torch.from_numpy(np.asarray(sd[dead])))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_threshold_that_does_not_clip_changes_nothing(golden, dtype):
    """max_grad_norm = 2 N_ref: the coefficient is exactly 1 and two steps leave every parameter, both moments and the 16-bit
    operand copies bit-equal to a trainer built without the argument.
    The learning rate is the reference's (and the Trainer's default) 1e-5.  At the 1e-3 of
    test_trainer_steps_reduce_the_loss_and_follow_adamw one AdamW step moves every weight of the random-init toy network by
    1e-3 and the SECOND gradient's norm is 4.86 (bf16, measured), above 2 N_ref = 2.64: clipping with coefficient 0.544 is
    then the correct behaviour, not the no-op this test is about."""
    from wiw_amd.train_unet import Trainer

    g = golden("train_step_tiny.npz")
    hip, sd, make = _tiny(g, dtype)
    st = _tiny_step(g)
    plain_net, clip_net = make(), make()
    plain, clip = Trainer(plain_net, lr=1e-5), Trainer(clip_net, lr=1e-5, max_grad_norm=2 * N_REF_TINY)
    for i in range(2):
        plain.step(st)
        clip.step(st)
        print(f"[clip {dtype}] threshold {2 * N_REF_TINY:.4f}, step {i + 1}: grad_norm {clip.grad_norm:.6f}, coefficient {clip.clip_coef!r}")
        assert clip.clip_coef == 1.0 and plain.grad_norm is None
    for k in plain_net.master:
        assert torch.equal(plain_net.master[k], clip_net.master[k]), k
        assert torch.equal(plain.m[k], clip.m[k]) and torch.equal(plain.v[k], clip.v[k]), k
    assert set(plain_net._direct) == set(clip_net._direct) and len(plain_net._direct) > 100
    for k in plain_net._direct:
        assert torch.equal(plain_net._direct[k], clip_net._direct[k]), k
    assert plain.loss_scale == clip.loss_scale and plain.steps == clip.steps == 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_full_width_global_norm_matches_the_reference(golden, dtype):
    """The served width on tests/golden/train_step_full_32x64.npz, set up as
    test_full_width_training_step_matches_reference_gradients: the reported global norm against the reference's 5.9572."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import Trainer, UNetTrain
    from wiw_amd.weights import random_state_dict

    g = golden("train_step_full_32x64.npz")
    cfg = UNetConfig()
    hip = _hip(dtype)
    net = UNetTrain(cfg, random_state_dict(cfg, int(g["weight_seed"])), DEV, hip=hip)
    st = T.prepare_step(torch.from_numpy(g["latents"]), torch.from_numpy(g["noise"]), float(g["sigmas"][0]),
                        torch.from_numpy(g["conditional_latents"]), torch.from_numpy(g["encoder_hidden_states"]),
                        float(g["noise_aug_strength"]), torch.from_numpy(g["action_ids"]),
                        dropout_prob=float(g["dropout_prob"]), random_p=torch.from_numpy(g["random_p"]))
    tr = Trainer(net, lr=1e-5, max_grad_norm=0.5)
    tr.step(st)
    assert tr.steps == 1
    dev = abs(tr.grad_norm - N_REF_FULL) / N_REF_FULL
    print(f"[clip {dtype}] served width: Trainer.grad_norm {tr.grad_norm:.6f} vs the reference's {N_REF_FULL} (rel dev {dev:.2e}, "
          f"gate {FULL_NORM_GATE[dtype]:.1e}), coefficient {tr.clip_coef:.6f}, table uploads {hip.sumsq_table_uploads}")
    assert dev <= FULL_NORM_GATE[dtype]
    assert abs(tr.clip_coef - 0.5 / (tr.grad_norm + 1e-6)) <= 1e-6
    del tr, net
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_fp16_overflow_skips_the_window_with_clipping_on(golden):
    """A loss scale so large that the 16-bit activation gradients leave fp16's range (they become Inf in the data): the window
    is skipped, the scale halves, no parameter moves and the reported norm is non-finite — clipping never turns a non-finite
    step into a finite one."""
    from wiw_amd.train_unet import Trainer

    g = golden("train_step_tiny.npz")
    hip, sd, make = _tiny(g, torch.float16)
    st = _tiny_step(g)
    net = make()
    tr = Trainer(net, lr=1e-3, loss_scale=2.0 ** 30, max_grad_norm=0.5)
    tr.step(st)
    assert tr.steps == 0 and tr.loss_scale == 2.0 ** 29
    assert not math.isfinite(tr.grad_norm)
    for k, v in net.master.items():
        assert torch.equal(v.cpu(), torch.from_numpy(np.asarray(sd[k])).to(torch.float32)), k
    assert all(not bool(m.any()) for m in tr.m.values())
    # the same trainer recovers at a sane scale
    tr.loss_scale = 2.0 ** 14
    tr.step(st)
    assert tr.steps == 1 and math.isfinite(tr.grad_norm) and 0.0 < tr.clip_coef < 1.0


@pytest.mark.gpu
def test_clipping_sees_the_accumulated_mean_gradient(golden):
    """grad_accum = 2 on one GPU: the norm is taken once per window, over the MEAN gradient.  Two micro-batches of the same
    sample average to that sample's gradient exactly (g/2 + g/2), so the window equals one plain clipped step bit for bit."""
    from wiw_amd.train_unet import Trainer

    g = golden("train_step_tiny.npz")
    hip, sd, make = _tiny(g, torch.bfloat16)
    st = _tiny_step(g)
    one_net, two_net = make(), make()
    one, two = Trainer(one_net, lr=1e-3, max_grad_norm=0.5), Trainer(two_net, lr=1e-3, max_grad_norm=0.5, grad_accum=2)
    one.step(st)
    two.step(st)
    assert two.steps == 0 and two.grad_norm is None             # accumulating micro-batch: no norm, no update
    two.step(st)
    assert two.steps == 1 and two.grad_norm == one.grad_norm and two.clip_coef == one.clip_coef < 1.0
    for k in one_net.master:
        assert torch.equal(one_net.master[k], two_net.master[k]), k


@pytest.mark.gpu
def test_sharded_adamw_clips_over_rccl_single_rank(golden):
    """One-rank RCCL `ShardedAdamW(max_grad_norm=0.5)` under `Trainer` against the unsharded clipped trainer.  The two sum the
    squares in different orders (per-tensor chunks against chunks of the flat shard), so the coefficients may differ in the
    last bits: gated at twice the summation bound, the parameters at lr times that."""
    import torch.distributed as dist

    from wiw_amd.parallel import ShardedAdamW
    from wiw_amd.train_unet import Trainer

    g = golden("train_step_tiny.npz")
    hip, sd, make = _tiny(g, torch.bfloat16)
    st = _tiny_step(g)
    lr = 1e-3
    solo = make()
    solo_tr = Trainer(solo, lr=lr, max_grad_norm=0.5)
    solo_tr.step(st)
    solo_coef = solo_tr.clip_coef
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        net = make()
        opt = ShardedAdamW({k: tuple(v.shape) for k, v in net.master.items()}, torch.device(DEV),
                           lambda p, gr, m, v, step, lr, b1, b2, eps, wd, grad_scale: hip.adamw_step(
                               p, gr, m, v, step, lr, b1, b2, eps, wd, grad_scale=grad_scale),
                           bucket_elems=1 << 20, lr=lr, max_grad_norm=0.5, norm_ops=hip)
        tr = Trainer(net, lr=lr, optimizer=opt)
        tr.step(st)
        L = hip.sumsq_chunk
        bound = 2 * _sum_bound(L)                               # L = 16384: 2 * 9.5e-7 = 1.9e-6
        live = [k for k in sd if not torch.equal(solo.master[k].cpu(), torch.from_numpy(np.asarray(sd[k])).to(torch.float32))]
        assert len(live) > 1000
        dcoef = abs(tr.clip_coef - solo_coef) / solo_coef
        diff = max(float((net.master[k] - solo.master[k]).abs().max()) for k in live)
        print(f"[clip] one-rank RCCL: coefficient {tr.clip_coef!r} vs unsharded {solo_coef!r} (rel diff {dcoef:.2e}, gate {bound:.2e}); "
              f"largest parameter difference {diff:.3e} (gate {lr * bound:.3e})")
        assert dcoef <= bound
        assert diff <= lr * bound
    finally:
        dist.destroy_process_group()
