"""Fine-tuning several clips per step (`--per_gpu_batch_size B`) — GPU side, both 16-bit libraries.

  * `wiw_edm_loss_grad_batched` (include/wiw_train_batch.h): per-sample partials bit-equal to `wiw_edm_loss_grad` on that sample
    alone, the gradient the single-sample one times fp32(1 / B);
  * the whole batched step — `prepare_step` (B, ...) -> `UNetTrain.forward` -> loss -> backward — against the MEAN over the
    samples of `oracle/train_oracle.training_step` run on each sample alone on the CPU (tests/batch_fixtures.py `oracle_mean`;
    the oracle is pinned to the reference's `loss.backward()` by tests/test_train_oracle.py), scenarios of batch_fixtures:
    B = 2 at 8x16 (two dropout branches), B = 3 at 24x40 navigation and manipulation (padded attention; the 15-token level has
    60 rows per clip and 180 per batch: both sides of the 64-row padding), 17 frames (`UNetTrain32`), 3 conditioning tokens,
    and the served width against tests/golden/train_step_batch.npz (tools/make_batch_golden.py: the same oracle mean);
  * `gradient_checkpointing=True` at B = 2: the plain run's gradients bit for bit;
  * `Trainer.step` on a batch: mean of `last_sample_losses`, descent, bit-repeatable, save / resume.

Statistics and gates: STAT_NAMES / TINY_GATES / FULL_WIDTH_GATES of tests/test_hip_train_any_size.py, unchanged.  They were
measured on single-sample steps; a batched mean gradient has the same error sources per sample.

MEASURED on MI355X, same order as STAT_NAMES; every statistic is below its gate:
   tiny2   bf16 1.67e-02 | 5.68e-05 | 2.81e-03 | 1.15e-02 | 3.98e-02 | 6.75e-02
           fp16 2.09e-03 | 3.21e-05 | 3.38e-04 | 1.24e-03 | 4.80e-03 | 8.71e-03
   nav3    bf16 1.57e-02 | 3.58e-05 | 2.23e-03 | 9.63e-03 | 3.74e-02 | 6.16e-02
           fp16 1.96e-03 | 3.78e-06 | 2.15e-04 | 9.65e-04 | 3.36e-03 | 7.98e-03
   manip3  bf16 1.53e-02 | 1.87e-06 | 1.94e-03 | 8.82e-03 | 3.38e-02 | 1.04e-01
           fp16 1.89e-03 | 1.01e-05 | 2.77e-04 | 1.32e-03 | 4.85e-03 | 8.09e-03
   h17     bf16 1.47e-02 | 5.33e-05 | 2.59e-03 | 9.46e-03 | 3.72e-02 | 6.90e-02
           fp16 1.83e-03 | 5.81e-06 | 2.30e-04 | 9.88e-04 | 4.42e-03 | 9.01e-03
   ctx3    bf16 1.48e-02 | 1.33e-04 | 2.74e-03 | 8.79e-03 | 3.96e-02 | 6.69e-02
           fp16 1.81e-03 | 7.01e-06 | 2.76e-04 | 1.01e-03 | 4.45e-03 | 8.54e-03
   full2   bf16 1.38e-02 | 1.05e-04 | 7.09e-04 | 2.29e-03 | 1.91e-02 | 4.56e-02
           fp16 1.68e-03 | 9.35e-06 | 1.46e-04 | 3.34e-04 | 2.10e-03 | 5.51e-03
batched gradients against the host mean of the same samples run one by one through the B = 1 tape (rms rel over all 1304
tensors; information, not a gate):
   tiny2 bf16: median 2.39e-09 90% 8.08e-08 worst 4.88e-03
   tiny2 fp16: median 2.20e-03 90% 2.92e-03 worst 5.82e-02
   nav3 bf16: median 1.97e-02 90% 2.75e-02 worst 2.10e+00
   nav3 fp16: median 2.59e-03 90% 3.64e-03 worst 2.64e-02
   manip3 bf16: median 1.94e-02 90% 2.75e-02 worst 2.14e-01
   manip3 fp16: median 2.48e-03 90% 3.42e-03 worst 2.05e-02
"""
import os

import numpy as np
import pytest
import torch

import batch_fixtures as BF
from test_hip_train_any_size import FULL_WIDTH_GATES, STAT_NAMES, TINY_GATES, _rel

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ---- 1. the loss kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("n,nb", [(2048, 8), (2048, 3), (240, 1), (240, 2)])
def test_batched_loss_kernel_is_the_single_sample_kernel_per_sample(n, nb, B):
    """partial[b][.] carries the bits `wiw_edm_loss_grad` writes for sample b alone with the same n_partial (one pass and several
    grid-stride passes per block, a ragged last pass, blocks with nothing to do); grad is the single-sample gradient times
    fp32(1 / B): bit-equal for B = 1, 2, 4, within one ulp for B = 3.  A sample with sigma <= 0 turns NaN, its neighbours do not."""
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    hip = Hip(torch.device(DEV))
    lib, s = hip.lib, hip._stream()
    g = torch.Generator().manual_seed(100 * n + B)
    pred, noisy, target = (torch.randn(B, n, generator=g).to(DEV) for _ in range(3))
    sig = [0.37, 1.7, 4.2, 0.9][:B]
    sig_d = torch.tensor(sig, dtype=torch.float32, device=DEV)
    grad, part = torch.full((B, n), 7.0, device=DEV), torch.full((B, nb), 7.0, device=DEV)
    hip._ck(lib.wiw_edm_loss_grad_batched(s, pred.data_ptr(), noisy.data_ptr(), target.data_ptr(), n, B, sig_d.data_ptr(),
                                          grad.data_ptr(), part.data_ptr(), nb), "batched")
    inv_b = torch.tensor(1.0 / B, dtype=torch.float32, device=DEV)
    for b in range(B):
        g1, p1 = torch.empty(n, device=DEV), torch.empty(nb, device=DEV)
        hip._ck(lib.wiw_edm_loss_grad(s, pred[b].data_ptr(), noisy[b].data_ptr(), target[b].data_ptr(), n, sig[b], g1.data_ptr(),
                                      p1.data_ptr(), nb), "single")
        assert torch.equal(_bits(part[b]), _bits(p1)), f"partials of sample {b}"
        want = g1 * inv_b
        ulps = int((_bits(grad[b]).long() - _bits(want).long()).abs().max())
        print(f"[batch loss] n={n} nb={nb} B={B} sample {b}: gradient within {ulps} ulp of single x fp32(1/B)")
        assert ulps <= (1 if B == 3 else 0)
    # the wrapper: per-sample losses, the same numbers `edm_loss_grad` returns sample by sample
    losses, grad_w = hip.edm_loss_grad_batched(pred, noisy, target, sig)
    assert tuple(losses.shape) == (B,) and grad_w.shape == pred.shape
    for b in range(B):
        l1, _ = hip.edm_loss_grad(pred[b], noisy[b], target[b], sig[b])
        assert abs(float(losses[b]) - float(l1)) <= 1e-6 * abs(float(l1))
    if B >= 2:
        bad = sig_d.clone()
        bad[1] = 0.0
        hip._ck(lib.wiw_edm_loss_grad_batched(s, pred.data_ptr(), noisy.data_ptr(), target.data_ptr(), n, B, bad.data_ptr(),
                                              grad.data_ptr(), part.data_ptr(), nb), "batched")
        assert bool(torch.isnan(grad[1]).all()) and bool(torch.isnan(part[1]).all())
        assert bool(torch.isfinite(grad[0]).all()) and bool(torch.isfinite(part[0]).all())


# ---- 2 .. 7. the whole step against the oracle mean ----------------------------------------------------------------------
def _net(name, dtype, **kw):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip
    from wiw_amd.train_unet import UNetTrain, UNetTrain32, make_unet_train

    cfg, P = BF.batch_config(name), BF.SCENARIOS[name][4]
    hip = Hip(torch.device(DEV), dtype)
    net = make_unet_train(cfg, BF.batch_weights(name), DEV, hip=hip, num_past_obs=P, **kw)
    assert type(net) is (UNetTrain32 if cfg.num_frames > 16 else UNetTrain)
    return net, hip


def _grads(net, hip, st, dtype):
    from wiw_amd import train as T

    pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
    losses, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
    grads = net.backward(dpred.reshape(pred.shape), loss_scale=1.0 if dtype == torch.bfloat16 else 2.0 ** 14)
    torch.cuda.synchronize()
    return pred.clone(), losses.reshape(-1).tolist(), {k: v.clone() for k, v in grads.items()}


def _norm_devs(ref_norms, mine, P):
    dev = sorted((abs(mine[n] - nr) / max(nr, 1e-7) for n, nr in ref_norms.items() if not BF.is_dead(n, P)), reverse=True)
    return dev[len(dev) // 2], dev[len(dev) // 10]


def _batched_step(name, dtype, gate, ref_loss, ref_pred, ref_norms, ref_full, ref_losses, vs_singles=False):
    """ref_full: [(parameter, reference gradient or its [:8, :512] window, windowed?)]."""
    h, w, T, B, P = BF.SCENARIOS[name][:5]
    net, hip = _net(name, dtype)
    st, singles = BF.batch_step_inputs(name)
    assert st.batch == B and tuple(st.unet_input.shape) == (B, T, 8, h, w) and tuple(st.ehs.shape) == (B, P, 1024)
    pred, losses, grads = _grads(net, hip, st, dtype)
    assert tuple(pred.shape) == (B, T, 4, h, w) and torch.isfinite(pred).all() and len(losses) == B
    stats = [_rel(pred, ref_pred)[1], abs(sum(losses) / B - ref_loss) / ref_loss]
    print(f"[batch {name} {dtype}] per-sample losses {losses} (oracle {ref_losses})")
    n_dead = sum(BF.is_dead(n, P) for n in net.master)
    assert len(grads) == len(net.master) - n_dead and n_dead == (4 if P > 1 else 132)
    mine = {}
    for n in net.master:
        if BF.is_dead(n, P):
            assert n not in grads, n
            continue
        assert n in grads and tuple(grads[n].shape) == tuple(net.master[n].shape) and bool(torch.isfinite(grads[n]).all()), n
        mine[n] = float(grads[n].double().norm())
    stats += list(_norm_devs(ref_norms, mine, P))
    full = []
    for n, r, windowed in ref_full:
        m = grads[n].reshape(grads[n].shape[0], -1)[:8, :r.shape[1]] if windowed else grads[n]
        full.append((_rel(m.reshape(r.shape), r)[1], n))
    full.sort(reverse=True)
    assert len(full) >= 15
    stats += [full[len(full) // 2][0], full[0][0]]
    print(f"[batch {name} {dtype}] full gradients (rms rel error): " + ", ".join(f"{'.'.join(n.split('.')[-3:])} {e:.1e}" for e, n in full))
    if vs_singles:      # information, not a gate: the same samples one by one through the unchanged B = 1 tape, averaged on the host
        acc = {}
        for s1 in singles:
            _, _, g1 = _grads(net, hip, s1, dtype)
            for k, v in g1.items():
                acc[k] = v.double() if k not in acc else acc[k] + v.double()
        dev = sorted(_rel(grads[k], (v / B).float())[1] for k, v in acc.items())
        print(f"[batch {name} {dtype}] batched gradients vs the host mean of {B} single-sample runs of the B = 1 tape (rms rel, "
              f"{len(dev)} tensors): median {dev[len(dev) // 2]:.2e}, 90% {dev[(9 * len(dev)) // 10]:.2e}, worst {dev[-1]:.2e}")
    failed = []
    for nm, v, gt in zip(STAT_NAMES, stats, gate):
        ok = v <= gt
        print(f"[batch {name} {dtype}] {nm}: {v:.3e} (gate {gt:.1e}) {'ok' if ok else 'FAIL'}")
        if not ok:
            failed.append(nm)
    assert not failed, failed
    return grads


def _against_oracle(name, dtype, vs_singles=False):
    P = BF.SCENARIOS[name][4]
    loss, pred, g, losses = BF.oracle_mean(name)
    norms = {n: float(v.double().norm()) for n, v in g.items()}
    watch = BF.WATCH + (BF.WATCH_CTX if P > 1 else [])
    return _batched_step(name, dtype, TINY_GATES[dtype], loss, pred, norms, [(n, g[n], False) for n in watch], losses, vs_singles)


@DTYPES
def test_batch_of_two_matches_the_oracle_mean(dtype):
    """Case 2: UNetConfig.tiny(4), 8x16 latent, B = 2, navigation; the samples differ in sigma, noise_aug_strength, actions and
    tokens; sample 0 loses its tokens to the conditioning dropout, sample 1 its conditioning latents."""
    _against_oracle("tiny2", dtype, vs_singles=True)


@DTYPES
@pytest.mark.parametrize("name", ["nav3", "manip3"])
def test_batch_of_three_at_24x40_matches_the_oracle_mean(name, dtype):
    """Case 3: odd B; levels of 960 / 240 / 60 / 15 tokens — the padded attention with 12 sequences, and the innermost level with
    60 rows per clip (below the 64-row padding of the B = 1 tape) and 180 per batch (above it)."""
    _against_oracle(name, dtype, vs_singles=True)


@DTYPES
def test_batch_of_two_at_17_frames_matches_the_oracle_mean(dtype):
    """Case 4: `UNetTrain32` (temporal attention over 32 slots, seqs = B)."""
    _against_oracle("h17", dtype)


@DTYPES
def test_batch_of_two_with_three_tokens_matches_the_oracle_mean(dtype):
    """Case 5: num_past_obs = 3, different tokens per sample (K / V are (B, P, C), rows_per_item = M / B); the newly live
    attn2.to_q / attn2.to_k / norm2 gradients are in the full-gradient statistics and must be non-zero."""
    grads = _against_oracle("ctx3", dtype)
    for n in BF.WATCH_CTX:
        assert float(grads[n].abs().max()) > 0.0, n


def test_recompute_gives_the_same_gradients_for_a_batch():
    """Case 6: `gradient_checkpointing=True`, B = 2 (tiny2, bf16): prediction and gradients of the plain run bit for bit."""
    st, _ = BF.batch_step_inputs("tiny2")
    net, hip = _net("tiny2", torch.bfloat16)
    plain = _grads(net, hip, st, torch.bfloat16)
    net_ck, hip_ck = _net("tiny2", torch.bfloat16, gradient_checkpointing=True)
    ck = _grads(net_ck, hip_ck, st, torch.bfloat16)
    assert torch.equal(plain[0], ck[0]) and plain[1] == ck[1]
    assert set(plain[2]) == set(ck[2]) and len(plain[2]) == len(net.master) - 132
    for k, v in plain[2].items():
        assert torch.equal(v, ck[2][k]), k


@DTYPES
def test_served_width_batch_matches_the_oracle_mean(golden, dtype):
    """Case 7: 320 / 640 / 1280 / 1280 channels, 4 frames, 16x32 latent, B = 2, against tests/golden/train_step_batch.npz."""
    g, pre = golden(BF.NAME), "full2__"
    assert np.array_equal(BF.checksums("full2"), g[f"{pre}input_checksums"]), "the re-drawn inputs are not the generator's"
    norms = dict(zip((str(n) for n in g[f"{pre}grad_names"]), (float(v) for v in g[f"{pre}grad_norms"])))
    full = []
    for key in g.files:
        if key.startswith(f"{pre}grad__") or key.startswith(f"{pre}grad8__"):
            name = key[len(pre):].split("__", 1)[1].replace("__", ".")
            full.append((name, torch.from_numpy(g[key]), key.startswith(f"{pre}grad8__")))
    _batched_step("full2", dtype, FULL_WIDTH_GATES[dtype], float(g[f"{pre}loss"]), torch.from_numpy(g[f"{pre}model_pred"]), norms,
                  full, [float(v) for v in g[f"{pre}sample_losses"]])


# ---- 8. Trainer ----------------------------------------------------------------------------------------------------------
def test_trainer_on_a_batch_of_two(tmp_path):
    """`Trainer.step` on a B = 2 batch: the returned loss is the mean of `last_sample_losses`; three steps on one batch lower it;
    the same step from equal state gives bit-identical gradients; `save`, then a fresh `Trainer.load`, repeats the fourth
    step bit for bit."""
    import wiw_amd  # noqa: F401
    from wiw_amd import checkpoint as C
    from wiw_amd.train_unet import Trainer

    st, _ = BF.batch_step_inputs("tiny2")
    net_a, _ = _net("tiny2", torch.bfloat16)
    net_c, _ = _net("tiny2", torch.bfloat16)
    a, c = Trainer(net_a, lr=1e-3), Trainer(net_c, lr=1e-3)
    l1 = a.step(st)
    g_a = {k: v.clone() for k, v in a.net.grads.items()}
    assert len(a.last_sample_losses) == 2 and l1 == sum(a.last_sample_losses) / 2
    assert a.last_sample_losses[0] != a.last_sample_losses[1]
    assert c.step(st) == l1 and c.last_sample_losses == a.last_sample_losses
    assert set(g_a) == set(c.net.grads) and all(torch.equal(v, c.net.grads[k]) for k, v in g_a.items())
    losses = [l1, a.step(st), a.step(st)]
    print(f"[batch] Trainer, B = 2: losses {losses}")
    assert all(np.isfinite(losses)) and losses[2] < losses[0] and a.steps == 3
    path = a.save(str(tmp_path), total_limit=1)
    assert os.path.isdir(path)
    l4 = a.step(st)
    net_b, _ = _net("tiny2", torch.bfloat16)
    b = Trainer(net_b, lr=1e-3)
    b.load(C.resolve_resume(str(tmp_path), "latest"))
    assert b.steps == 3 and b.step(st) == l4 and b.last_sample_losses == a.last_sample_losses
    for k in a.net.master:
        assert torch.equal(a.net.master[k], b.net.master[k]) and torch.equal(a.m[k], b.m[k]) and torch.equal(a.v[k], b.v[k]), k
