"""Where one fine-tuning step goes, by OPERATOR (not by kernel): HIP-event time of every backward closure of the tape, summed
per operator kind, plus the linear / conv backward split into dx | weight-gradient | bias pieces, and a sweep of the
weight-gradient GEMM over orientation (dW vs dW^T) and split-K factors at the served shapes.  GPU box only.

`--max_grad_norm C` instead measures what global-norm gradient clipping costs: the whole `Trainer.step` (PH x PW x 14, default
576 x 1024) without and with the threshold, in one process on one box, in alternating blocks (off, on, off, on), plus the
norm kernels on their own (ms and GB/s over the trainer's own gradient tensors).

`--manip448` measures the fine-tuning step of the served network on a 448 x 448 x 14 manipulation clip (56 x 56 latent: levels of
3136, 784, 196 and 49 tokens, 10 action channels): forward / backward / whole `Trainer.step` ms, peak memory, the kernel-family
rows `Hip._timed` keeps, the GEMMs by mode, and every attention call by sequence length — the padded form (`attn_small` + the
one-wave backward at S = 196 and 49) and the one-wave backward at S = 784 next to the LDS-tiled S = 3136.

`--frames N` (1 .. 32) runs the same measurement at N frames on the tape `make_unet_train` picks (`UNetTrain` up to 16 frames,
`UNetTrain32` above): a PH x PW x N navigation clip, or with `--manip448` a 448 x 448 x N manipulation clip.  Its record also
carries `temporal_attention`: the GPU time between the first and the last launch of every temporal self-attention — forward
(the 32-slot kernel; on the 16-row tape re-ordering, V^T and `attn_small`) and backward closure (row maps, transposes, the two
one-wave kernels) — and its share of the step.

`--gradient_checkpointing` (with `--frames N` and / or `--manip448`) measures what activation checkpointing costs and saves: one
tape in one process, blocks of `--steps` steps without and with the keyword in alternation (off, on, off, on); per mode forward,
backward and whole `Trainer.step` ms and the peak GiB (`torch.cuda.max_memory_allocated`, reset per block), the checkpointed step
against `plain step + 1.15 x plain forward`; written to profiles/r25a_train_step_ckpt_<size>x<frames>_<dtype>.json.

`--num_past_obs P` (1 .. 8) measures the step of the served network on a PH x PW x 14 navigation clip with P conditioning tokens
per sample (`UNetTrain(num_past_obs=P)`): forward / backward / step ms, peak GiB and, above 1, the summed ms of the 32
cross-attentions — LayerNorm, to_q GEMM, forward kernel, backward kernels — with the backward's bytes/s against its minimum;
written to profiles/r26a_train_step_ctx_P<P>_<size>x14_<dtype>.json.

`--batch B` (with `--manip448` and / or `--frames N`, optionally `--gradient_checkpointing`) measures the step on batches of
1, 2, 4, ... and B clips (`train.collate` of clips that differ in noise level, actions and tokens) on ONE tape in one process:
per row ms per step, ms per clip, forward / backward ms, peak GiB, the kernel-family and GEMM-mode breakdown of one step, and
the ratio of ms per clip to the B = 1 row of the same run — which is the unchanged single-clip path; written to
profiles/r27a_train_step_batch_B<B>_<size>x<frames>_<dtype>[_ckpt].json."""
import argparse
import collections
import dataclasses
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wiw_amd  # noqa: F401,E402
from wiw_amd import train as T  # noqa: E402
from wiw_amd.config import UNetConfig  # noqa: E402
from wiw_amd.hip import EPI_OUT_F32  # noqa: E402
from wiw_amd.train_unet import UNetTrain, make_unet_train  # noqa: E402
from wiw_amd.weights import random_state_dict_torch  # noqa: E402

dev = torch.device("cuda:0")
H, W = int(os.environ.get("PH", 576)), int(os.environ.get("PW", 1024))


def step_by_operator():
    cfg = UNetConfig()
    net = UNetTrain(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev)
    gen = torch.Generator().manual_seed(0)
    Tn, h, w = 14, H // 8, W // 8
    lat, noise = torch.randn(1, Tn, 4, h, w, generator=gen) * 0.8, torch.randn(1, Tn, 4, h, w, generator=gen)
    st = T.prepare_step(lat, noise, 1.3, torch.randn(1, 4, h, w, generator=gen), torch.randn(1, 1, 1024, generator=gen), 0.04,
                        torch.zeros(1, Tn, 14))
    T.clear_wgrad_plans()
    T.set_wgrad_tuning(os.environ.get("TUNE", "0") == "1")
    frecs = []

    def fwrap(obj, name, label):
        f = getattr(obj, name)

        def g(*a, **k):
            if not frecs_on[0]:
                return f(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = f(*a, **k); e1.record()
            frecs.append((label, e0, e1))
            return out
        setattr(obj, name, g)
    frecs_on = [False]
    for nm in ("linear", "conv", "groupnorm", "layernorm", "geglu", "silu", "blend", "concat", "upsample2x", "cast16", "_add_rowvec",
               "host_sum"):
        fwrap(net, nm, "net." + nm)
    for nm in ("attn_spatial", "attn_small", "row_map", "transpose"):
        fwrap(net.hip, nm, "hip." + nm)
    for it in range(3):
        frecs_on[0] = it == 2
        torch.cuda.synchronize(); tf0 = time.perf_counter()
        pred = net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids)
        torch.cuda.synchronize(); tfw = time.perf_counter() - tf0
        frecs_on[0] = False
        loss, dpred = T.TrainStep(net.hip).loss_and_grad(pred, st)
        recs = []

        def wrap(f):
            def g():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                recs.append((f.__qualname__, a, b))
            return g
        if it == 2:
            net.tape.ops = [wrap(f) for f in net.tape.ops]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        net.backward(dpred.reshape(pred.shape))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    agg = collections.defaultdict(lambda: [0, 0.0])
    for q, a, b in recs:
        agg[q][0] += 1; agg[q][1] += a.elapsed_time(b)
    fagg = collections.defaultdict(lambda: [0, 0.0])
    for q, e0, e1 in frecs:
        fagg[q][0] += 1; fagg[q][1] += e0.elapsed_time(e1)
    print(f"forward wall {tfw*1e3:.1f} ms (with per-call events; hip.* calls nest inside net.* ones only for attention):")
    for q, (n, ms) in sorted(fagg.items(), key=lambda kv: -kv[1][1]):
        print(f"  {q:55s} {n:5d} calls    {ms:8.1f} ms")
    print(f"backward wall {dt*1e3:.1f} ms (with per-closure events); by operator:")
    for q, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"  {q:55s} {n:5d} closures {ms:8.1f} ms")
    print("plans:", {k: v for k, v in sorted(T.wgrad_plans().items())})
    T.set_wgrad_tuning(False)
    T.clear_wgrad_plans()
    del net
    torch.cuda.empty_cache()


def timeit(fn, n=5):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wgrad_sweep():
    from wiw_amd.hip import Hip
    hip = Hip(dev)
    M0 = 14 * (H // 8) * (W // 8)
    shapes = []
    for lvl, C in enumerate((320, 640, 1280)):
        M = M0 >> (2 * lvl)
        shapes += [(f"L{lvl} qkv", 3 * C, C, M), (f"L{lvl} out/proj", C, C, M), (f"L{lvl} ff1", 8 * C, C, M), (f"L{lvl} ff2", C, 4 * C, M),
                   (f"L{lvl} conv3x3", C, 9 * C, M), (f"L{lvl} conv_t", C, 3 * C, M)]
    shapes += [("L3 conv3x3", 1280, 11520, -(-(M0 >> 6) // 64) * 64), ("L3 res-t", 1280, 3840, -(-(M0 >> 6) // 64) * 64), ("up0 conv3x3 2560", 1280, 9 * 2560, M0 >> 4),
               ("up2 conv3x3 960", 320, 9 * 960, M0), ("up1 conv3x3 1920", 640, 9 * 1920, M0 >> 2), ("conv_out", 64, 2880, M0),
               ("L0 shortcut 640", 320, 640, M0)]
    print("weight-gradient GEMM dW[N,K] = dy^T x over Mrows (ms): auto split | best of sweep (orientation, split)")
    for name, N, K, M in shapes:
        dyT = torch.randn(N, M, device=dev).to(torch.bfloat16)
        xT = torch.randn(K, M, device=dev).to(torch.bfloat16)
        out = torch.empty(N, K, dtype=torch.float32, device=dev)
        outT = torch.empty(K, N, dtype=torch.float32, device=dev)
        f0, s0 = T.wgrad_plan(N, K, M)
        base = timeit(lambda: T._wgrad_run(hip, dyT, xT, N, K, M, f0, s0))
        res = []
        nk = M // 64
        cands = sorted({s for s in (1, 2, 3, 4, 6, 7, 8, 9, 12, 14, 16, 18, 21, 24, 28, 32, 36, 42, 48, 56, 63, 64, 72, 84, 96, 112, 126, 128)
                        if nk % s == 0 and nk // s >= 4})
        for flip in (0, 1):
            for s in cands:
                try:
                    if flip:
                        t = timeit(lambda: hip.gemm(xT, dyT, outT, M=K, N=N, K=M, C1=M, epilogue=EPI_OUT_F32, splitk=s), 3)
                    else:
                        t = timeit(lambda: hip.gemm(dyT, xT, out, M=N, N=K, K=M, C1=M, epilogue=EPI_OUT_F32, splitk=s), 3)
                    res.append((t, flip, s))
                except Exception as e:  # noqa: BLE001
                    res.append((1e9, flip, s))
        res.sort()
        # the row-major ("TN") kernel: no transposes; the NT numbers above exclude the two transposes it saves
        dy = dyT.t().contiguous(); x = xT.t().contiguous()
        ref = (dyT.float() @ xT.float().t())
        tn = []
        for sp in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384):
            if M // sp < 128:
                break
            t = timeit(lambda: hip.wgrad_tn(dy, x, M, N, K, sp), 3)
            tn.append((t, sp))
        tn.sort()
        err = float((hip.wgrad_tn(dy, x, M, N, K, tn[0][1]) - ref).abs().max() / ref.abs().max())
        def tr2():
            a_ = torch.empty(N, M, dtype=dy.dtype, device=dev); hip.transpose(dy, N, 0, M, N, a_, M)
            b_ = torch.empty(K, M, dtype=dy.dtype, device=dev); hip.transpose(x, K, 0, M, K, b_, M)
        t_tr = timeit(tr2, 3)
        print(f"      TN best: " + ", ".join(f"s={sp} {t:.3f}" for t, sp in tn[:3]) + f"   (max err vs fp32 {err:.1e}); the two transposes NT needs: {t_tr:.3f} ms")
        del dy, x, ref
        tf = 2.0 * N * K * M / 1e9
        print(f"  {name:14s} N={N:5d} K={K:5d} M={M:6d}: plan {'T' if f0 else 'N'}/s={s0:3d} {base:7.3f} ms ({tf/base:6.0f} TF/s) | best "
              + ", ".join(f"{'T' if f else 'N'}/s={s} {t:.3f}" for t, f, s in res[:4]))
        del dyT, xT, out, outT


def clip_cost(max_grad_norm: float, steps: int = 5, dtype=torch.bfloat16):
    import json
    import statistics

    from wiw_amd.train_unet import Trainer

    cfg = UNetConfig()
    net = UNetTrain(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev, dtype=dtype)
    gen = torch.Generator().manual_seed(100)
    Tn, h, w = 14, H // 8, W // 8
    lat, noise = torch.randn(1, Tn, 4, h, w, generator=gen) * 0.8, torch.randn(1, Tn, 4, h, w, generator=gen)
    st = T.prepare_step(lat, noise, 1.3, torch.randn(1, 4, h, w, generator=gen), torch.randn(1, 1, 1024, generator=gen), 0.04,
                        torch.zeros(1, Tn, 14))
    tr = Trainer(net, lr=1e-5, autotune=True)
    for _ in range(2):                                   # warm-up: weight-gradient plans, allocator
        tr.step(st)
    tr.max_grad_norm = max_grad_norm
    tr.step(st)                                          # ... and the norm's table / partial buffers
    torch.cuda.synchronize()
    blocks = []
    for setting in (None, max_grad_norm, None, max_grad_norm):
        tr.max_grad_norm = setting
        ms = []
        for _ in range(steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tr.step(st)
            torch.cuda.synchronize(); ms.append(1e3 * (time.perf_counter() - t0))
        blocks.append({"max_grad_norm": setting, "ms_per_step_median": round(statistics.median(ms), 2), "ms_per_step_all": [round(x, 1) for x in ms],
                       "grad_norm": tr.grad_norm if setting is not None else None})
    off = statistics.median(x for b in blocks if b["max_grad_norm"] is None for x in b["ms_per_step_all"])
    on = statistics.median(x for b in blocks if b["max_grad_norm"] is not None for x in b["ms_per_step_all"])
    # the norm kernels alone, over the gradient tensors the last step left (HIP events around 20 calls; the table is cached)
    flat = [g.reshape(-1).contiguous() for n, g in net.grads.items() if tr.trainable(n)]
    nbytes = 4.0 * sum(t.numel() for t in flat)
    up0 = net.hip.sumsq_table_uploads
    ms_norm = timeit(lambda: net.hip.grad_sumsq(flat, max_grad_norm), 20)
    print(json.dumps({"probe": "clip_cost", "size": f"{H}x{W}x{Tn}", "dtype": str(dtype), "blocks": blocks,
                      "ms_per_step_off": round(off, 2), "ms_per_step_on": round(on, 2), "on_over_off": round(on / off, 4),
                      "norm_tensors": len(flat), "norm_GB": round(nbytes / 1e9, 3), "norm_ms": round(ms_norm, 4),
                      "norm_GBps": round(nbytes / ms_norm / 1e6, 1), "table_uploads_in_21_calls": net.hip.sumsq_table_uploads - up0,
                      "table_uploads_total": net.hip.sumsq_table_uploads}))


def train_step_probe(Tn: int, manip448: bool, dtype=torch.bfloat16, steps: int = 5):
    """forward / backward / whole `Trainer.step` of the served network on a Tn-frame clip: 448 x 448 manipulation (10 action
    channels) or PH x PW navigation (Tn action channels)."""
    import json
    import statistics

    import numpy as np

    from wiw_amd.pipeline import SCENE_BOUNDS, action_ids_idx_encode, manip_action_ids
    from wiw_amd.train_unet import Trainer, attn_level_plan

    h, w = (56, 56) if manip448 else (H // 8, W // 8)
    if manip448:
        cfg = UNetConfig(num_frames=Tn, action_input_channel=10, task_type="manipulation")
    else:
        cfg = UNetConfig(num_frames=Tn, action_input_channel=Tn)
    net = make_unet_train(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev, dtype=dtype)
    hip = net.hip
    gen = torch.Generator().manual_seed(100)
    rs = np.random.RandomState(0)
    poses = np.zeros((1, Tn, 8), np.float32)
    poses[..., :3] = SCENE_BOUNDS[:3] + (SCENE_BOUNDS[3:] - SCENE_BOUNDS[:3]) * rs.uniform(0.1, 0.9, size=(1, Tn, 3))
    poses[..., 3:7] = rs.standard_normal((1, Tn, 4))
    poses[..., 7] = rs.choice([0.0, 1.0], size=(1, Tn))
    ids = manip_action_ids(poses) if manip448 else action_ids_idx_encode(np.array([[4] + [[1, 2, 1, 3][i % 4] for i in range(Tn - 1)]]))
    lat, noise = torch.randn(1, Tn, 4, h, w, generator=gen) * 0.8, torch.randn(1, Tn, 4, h, w, generator=gen)
    st = T.prepare_step(lat, noise, 1.3, torch.randn(1, 4, h, w, generator=gen), torch.randn(1, 1, 1024, generator=gen), 0.04,
                        torch.from_numpy(ids))
    T.clear_wgrad_plans()
    tr = Trainer(net, lr=1e-5, autotune=True)
    for _ in range(2):                                   # warm-up: weight-gradient plans, allocator
        tr.step(st)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    fwd, bwd, whole = [], [], []
    for _ in range(steps):
        ms, pred = wall(lambda: net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids))
        fwd.append(ms)
        loss, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
        bwd.append(wall(lambda: net.backward(dpred.reshape(pred.shape), tr.loss_scale))[0])
    for _ in range(steps):
        whole.append(wall(lambda: tr.step(st))[0])
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    # one more step with events: families, GEMM modes, every attention call by sequence length
    arecs = []

    def awrap(name, key):
        f = getattr(hip, name)

        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = f(*a, **k); e1.record()
            arecs.append((f"{name} {key(a, k)}", e0, e1))
            return out
        setattr(hip, name, g)
    awrap("attn_spatial", lambda a, k: f"S={a[8]}" + (" +lse" if k.get("lse") is not None else ""))
    awrap("attn_small", lambda a, k: f"S={a[8]} Sp={a[9]}")
    awrap("attn_backward", lambda a, k: f"S={a[4]} Sp={k.get('Sp') or a[4]}" + (" given lse" if k.get("lse") is not None else ""))
    # the temporal self-attentions as a whole: events around the forward's launches after the q|k|v GEMM, and around the
    # backward closure the call leaves on the tape
    trecs, in_temporal = [], [False]

    def timed(label, f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = f(*a, **k); e1.record()
            trecs.append((label, e0, e1))
            return out
        return g

    def fwd_only(name):
        f = getattr(hip, name)
        tf = timed("forward", f)
        setattr(hip, name, lambda *a, **k: (tf if in_temporal[0] else f)(*a, **k))
    for nm in ("attn_temporal32", "attn_small", "row_map", "transpose"):
        fwd_only(nm)
    self_attention = net.self_attention

    def sa(*a, temporal_T=0, **k):
        in_temporal[0] = bool(temporal_T)
        try:
            out = self_attention(*a, temporal_T=temporal_T, **k)
        finally:
            in_temporal[0] = False
        if temporal_T:
            net.tape.ops[-1] = timed("backward", net.tape.ops[-1])
        return out
    net.self_attention = sa
    hip.kernel_profile, hip.gemm_profile = [], []
    ms_prof, _ = wall(lambda: tr.step(st))
    net.self_attention = self_attention
    ta = collections.defaultdict(lambda: [0, 0.0])
    for key, e0, e1 in trecs:
        ta[key][0] += 1; ta[key][1] += e0.elapsed_time(e1)
    fam = collections.defaultdict(lambda: [0, 0.0])
    for e0, e1, family, _, _ in hip.kernel_profile:
        fam[family][0] += 1; fam[family][1] += e0.elapsed_time(e1)
    gm = collections.defaultdict(lambda: [0, 0.0])
    for e0, e1, _, mode, _ in hip.gemm_profile:
        gm[f"gemm mode {mode}"][0] += 1; gm[f"gemm mode {mode}"][1] += e0.elapsed_time(e1)
    at = collections.defaultdict(lambda: [0, 0.0])
    for key, e0, e1 in arecs:
        at[key][0] += 1; at[key][1] += e0.elapsed_time(e1)
    hip.kernel_profile = hip.gemm_profile = None
    step_ms = statistics.median(whole)
    rows = lambda d: {k: {"calls": n, "ms": round(ms, 3), "share_of_step": round(ms / step_ms, 4)}  # noqa: E731
                      for k, (n, ms) in sorted(d.items(), key=lambda kv: -kv[1][1])}
    ta_ms = sum(ms for _, ms in ta.values())
    print(json.dumps({"probe": "manip448_train_step" if manip448 else "train_step", "size": f"{8 * h}x{8 * w}x{Tn}", "latent": [h, w],
                      "dtype": str(dtype), "tape": type(net).__name__,
                      "temporal_attention": dict(rows(ta), total_ms=round(ta_ms, 3), share_of_step=round(ta_ms / step_ms, 4)),
                      "levels_S_Sp": attn_level_plan(h, w), "forward_ms": round(statistics.median(fwd), 2),
                      "backward_ms": round(statistics.median(bwd), 2), "step_ms": round(step_ms, 2),
                      "step_ms_all": [round(x, 1) for x in whole], "step_ms_with_events": round(ms_prof, 1),
                      "peak_GiB": round(peak, 2), "loss_scale": tr.loss_scale, "attention_calls": rows(at),
                      "kernel_families": rows(fam), "gemms": rows(gm), "wgrad_plans": len(T.wgrad_plans())}))


def _probe_clip(Tn: int, manip448: bool):
    """(cfg, latent (h, w), StepInputs) of the clip `train_step_probe` measures."""
    import numpy as np

    from wiw_amd.pipeline import SCENE_BOUNDS, action_ids_idx_encode, manip_action_ids

    h, w = (56, 56) if manip448 else (H // 8, W // 8)
    if manip448:
        cfg = UNetConfig(num_frames=Tn, action_input_channel=10, task_type="manipulation")
    else:
        cfg = UNetConfig(num_frames=Tn, action_input_channel=Tn)
    gen = torch.Generator().manual_seed(100)
    rs = np.random.RandomState(0)
    poses = np.zeros((1, Tn, 8), np.float32)
    poses[..., :3] = SCENE_BOUNDS[:3] + (SCENE_BOUNDS[3:] - SCENE_BOUNDS[:3]) * rs.uniform(0.1, 0.9, size=(1, Tn, 3))
    poses[..., 3:7] = rs.standard_normal((1, Tn, 4))
    poses[..., 7] = rs.choice([0.0, 1.0], size=(1, Tn))
    ids = manip_action_ids(poses) if manip448 else action_ids_idx_encode(np.array([[4] + [[1, 2, 1, 3][i % 4] for i in range(Tn - 1)]]))
    lat, noise = torch.randn(1, Tn, 4, h, w, generator=gen) * 0.8, torch.randn(1, Tn, 4, h, w, generator=gen)
    st = T.prepare_step(lat, noise, 1.3, torch.randn(1, 4, h, w, generator=gen), torch.randn(1, 1, 1024, generator=gen), 0.04,
                        torch.from_numpy(ids))
    return cfg, (h, w), st


def batch_probe(B: int, Tn: int, manip448: bool, dtype=torch.bfloat16, steps: int = 5, gradient_checkpointing: bool = False):
    """`--batch B`: rows for 1, 2, 4, ... and B clips per step on one tape (module docstring)."""
    import json
    import statistics

    from wiw_amd.train_unet import MAX_BATCH_ROWS, Trainer

    cfg, (h, w), st1 = _probe_clip(Tn, manip448)
    sizes = sorted({b for b in (1, 2, 4, 8, 16, 32, 64) if b < B} | {B})
    if B > 1 and B * Tn * h * w > MAX_BATCH_ROWS:
        raise SystemExit(f"--batch {B}: {B * Tn * h * w} rows, above MAX_BATCH_ROWS = {MAX_BATCH_ROWS}")
    gen = torch.Generator().manual_seed(200)
    clips = [st1]
    for b in range(1, B):                                 # the same clip geometry; own latents, noise level, tokens and actions
        lat, noise = torch.randn(1, Tn, 4, h, w, generator=gen) * 0.8, torch.randn(1, Tn, 4, h, w, generator=gen)
        clips.append(T.prepare_step(lat, noise, 0.5 + 0.4 * b, torch.randn(1, 4, h, w, generator=gen),
                                    torch.randn(1, 1, 1024, generator=gen), 0.02 + 0.01 * b, st1.action_ids.flip(1) if b % 2 else st1.action_ids))
    net = make_unet_train(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev, dtype=dtype,
                          gradient_checkpointing=gradient_checkpointing)
    hip = net.hip
    T.clear_wgrad_plans()
    tr = Trainer(net, lr=1e-5, autotune=True)

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    rows = []
    for b in sizes:
        st = T.collate(clips[:b])
        for _ in range(2):                                # warm-up: this row count's weight-gradient plans, allocator
            tr.step(st)
        net.grads = {}
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fwd, bwd, whole = [], [], []
        for _ in range(steps):
            ms, pred = wall(lambda: net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids))
            fwd.append(ms)
            loss, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
            bwd.append(wall(lambda: net.backward(dpred.reshape(pred.shape), tr.loss_scale))[0])
            del pred, dpred
        for _ in range(steps):
            whole.append(wall(lambda: tr.step(st))[0])
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        hip.kernel_profile, hip.gemm_profile = [], []
        ms_prof, _ = wall(lambda: tr.step(st))
        fam, gm = collections.defaultdict(lambda: [0, 0.0]), collections.defaultdict(lambda: [0, 0.0])
        for e0, e1, family, _, _ in hip.kernel_profile:
            fam[family][0] += 1; fam[family][1] += e0.elapsed_time(e1)
        for e0, e1, _, mode, _ in hip.gemm_profile:
            gm[f"gemm mode {mode}"][0] += 1; gm[f"gemm mode {mode}"][1] += e0.elapsed_time(e1)
        hip.kernel_profile = hip.gemm_profile = None
        step_ms = statistics.median(whole)
        table = lambda d: {k: {"calls": n, "ms": round(ms, 3), "ms_per_clip": round(ms / b, 3)}  # noqa: E731
                           for k, (n, ms) in sorted(d.items(), key=lambda kv: -kv[1][1])}
        rows.append({"batch": b, "rows_level0": b * Tn * h * w, "step_ms": round(step_ms, 2), "ms_per_clip": round(step_ms / b, 2),
                     "step_ms_all": [round(x, 1) for x in whole], "forward_ms": round(statistics.median(fwd), 2),
                     "backward_ms": round(statistics.median(bwd), 2), "peak_GiB": round(peak, 2),
                     "sample_losses": [round(x, 4) for x in tr.last_sample_losses], "step_ms_with_events": round(ms_prof, 1),
                     "kernel_families": table(fam), "gemms": table(gm)})
        rows[-1]["ms_per_clip_over_B1"] = round(rows[-1]["ms_per_clip"] / rows[0]["ms_per_clip"], 4)
        print(json.dumps({k: v for k, v in rows[-1].items() if k not in ("kernel_families", "gemms")}), flush=True)
    rec = {"probe": "train_step_batch", "size": f"{8 * h}x{8 * w}x{Tn}", "latent": [h, w], "dtype": str(dtype), "tape": type(net).__name__,
           "task": cfg.task_type, "gradient_checkpointing": gradient_checkpointing, "steps_per_row": steps, "loss_scale": tr.loss_scale,
           "wgrad_plans": len(T.wgrad_plans()), "rows": rows}
    print(json.dumps(rec))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       f"r27a_train_step_batch_B{B}_{8 * h}x{8 * w}x{Tn}_{'fp16' if dtype == torch.float16 else 'bf16'}"
                       f"{'_ckpt' if gradient_checkpointing else ''}.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def checkpoint_cost(Tn: int, manip448: bool, dtype=torch.bfloat16, steps: int = 5):
    """Activation checkpointing off / on / off / on on ONE tape (the keyword is configuration: `forward` reads it)."""
    import json
    import statistics

    from wiw_amd.train_unet import Trainer

    cfg, (h, w), st = _probe_clip(Tn, manip448)
    net = make_unet_train(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev, dtype=dtype)
    hip = net.hip
    T.clear_wgrad_plans()
    tr = Trainer(net, lr=1e-5, autotune=True)
    for mode in (False, False, True):                     # warm-up: weight-gradient plans, allocator, both modes
        net.gradient_checkpointing = mode
        tr.step(st)

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    blocks = []
    for mode in (False, True, False, True):
        net.gradient_checkpointing = mode
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fwd, bwd, whole, held = [], [], [], []
        for _ in range(steps):
            net.grads = {}                                # the last step's gradients: `forward` drops them, it does not hold them
            before = torch.cuda.memory_allocated()
            ms, pred = wall(lambda: net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids))
            fwd.append(ms)
            held.append((torch.cuda.memory_allocated() - before) / 2 ** 30)
            loss, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
            bwd.append(wall(lambda: net.backward(dpred.reshape(pred.shape), tr.loss_scale))[0])
            del pred, dpred
        for _ in range(steps):
            whole.append(wall(lambda: tr.step(st))[0])
        blocks.append({"gradient_checkpointing": mode, "forward_ms": round(statistics.median(fwd), 2),
                       "backward_ms": round(statistics.median(bwd), 2), "step_ms": round(statistics.median(whole), 2),
                       "step_ms_all": [round(x, 1) for x in whole], "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                       "held_after_forward_GiB": round(statistics.median(held), 2)})

    def mode_row(mode):
        bs = [b for b in blocks if b["gradient_checkpointing"] is mode]
        return {"forward_ms": round(statistics.median(b["forward_ms"] for b in bs), 2),
                "backward_ms": round(statistics.median(b["backward_ms"] for b in bs), 2),
                "step_ms": round(statistics.median(x for b in bs for x in b["step_ms_all"]), 2),
                "peak_GiB": max(b["peak_GiB"] for b in bs), "held_after_forward_GiB": max(b["held_after_forward_GiB"] for b in bs)}
    off, on = mode_row(False), mode_row(True)
    budget = off["step_ms"] + 1.15 * off["forward_ms"]
    rec = {"probe": "gradient_checkpointing", "size": f"{8 * h}x{8 * w}x{Tn}", "latent": [h, w], "dtype": str(dtype),
           "tape": type(net).__name__, "task": cfg.task_type, "steps_per_block": steps, "off": off, "on": on,
           "step_on_over_off": round(on["step_ms"] / off["step_ms"], 4), "peak_on_over_off": round(on["peak_GiB"] / off["peak_GiB"], 4),
           "budget_ms_plain_step_plus_1.15_plain_forward": round(budget, 2), "step_on_over_budget": round(on["step_ms"] / budget, 4),
           "weights_moments_grads_GiB": round(sum(v.numel() for v in net.master.values()) * (4 * 4 + 2) / 2 ** 30, 2),
           "loss_scale": tr.loss_scale, "blocks": blocks}
    print(json.dumps(rec))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       f"r25a_train_step_ckpt_{8 * h}x{8 * w}x{Tn}_{'fp16' if dtype == torch.float16 else 'bf16'}.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def past_obs_probe(P: int, dtype=torch.bfloat16, steps: int = 5):
    """`--num_past_obs P`: forward / backward / whole `Trainer.step` of the served network on a PH x PW x 14 navigation clip with
    P conditioning tokens, peak GiB, and — P > 1 — the 32 cross-attentions of the step by piece: the forward's LayerNorm(norm2),
    to_q GEMM and `cross_attn_fewkeys` launch, the backward kernels (`cross_attn_fewkeys_backward`: the streaming launch + the
    block sum) against their 3 x rows x C x 2-byte minimum, and the backward closures of norm2 / to_q.  P = 1 is the row every
    other measurement of this size has: the same tape, launch for launch."""
    import json
    import statistics

    from wiw_amd.train_unet import Trainer

    Tn = 14
    cfg, (h, w), st = _probe_clip(Tn, False)
    gen = torch.Generator().manual_seed(101)
    ehs = torch.randn(1, P, cfg.cross_attention_dim, generator=gen) if P > 1 else st.ehs
    net = make_unet_train(cfg, random_state_dict_torch(cfg, 0, dev, torch.float32), dev, dtype=dtype, num_past_obs=P)
    hip = net.hip
    T.clear_wgrad_plans()
    tr = Trainer(net, lr=1e-5, autotune=True)
    st = dataclasses.replace(st, ehs=ehs)
    for _ in range(2):                                   # warm-up: weight-gradient plans, allocator
        tr.step(st)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    fwd, bwd, whole = [], [], []
    for _ in range(steps):
        ms, pred = wall(lambda: net.forward(st.unet_input, st.timestep, st.ehs, st.added_time_ids, st.action_ids))
        fwd.append(ms)
        loss, dpred = T.TrainStep(hip).loss_and_grad(pred, st)
        bwd.append(wall(lambda: net.backward(dpred.reshape(pred.shape), tr.loss_scale))[0])
        del pred, dpred
    for _ in range(steps):
        whole.append(wall(lambda: tr.step(st))[0])
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    step_ms = statistics.median(whole)
    rec = {"probe": "train_step_past_obs", "size": f"{8 * h}x{8 * w}x{Tn}", "latent": [h, w], "dtype": str(dtype),
           "tape": type(net).__name__, "num_past_obs": P, "forward_ms": round(statistics.median(fwd), 2),
           "backward_ms": round(statistics.median(bwd), 2), "step_ms": round(step_ms, 2), "step_ms_all": [round(x, 1) for x in whole],
           "peak_GiB": round(peak, 2), "loss_scale": tr.loss_scale,
           "optimizer_tensors": len(Trainer.optimizer_shapes(net))}
    if P > 1:
        # one more step with events round the pieces of every cross-attention
        recs, inside = [], [False]

        def timed(label, f):
            def g(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = f(*a, **k); e1.record()
                recs.append((label, e0, e1))
                return out
            return g

        def piece(obj, name, label, pick):
            f = getattr(obj, name)
            tf = timed(label, f)

            def g(*a, **k):
                if not (inside[0] and pick(a)):
                    return f(*a, **k)
                out = tf(*a, **k)
                net.tape.ops[-1] = timed(label + " backward closure", net.tape.ops[-1])
                return out
            setattr(obj, name, g)
            return f
        ln = piece(net, "layernorm", "LayerNorm norm2", lambda a: a[1].endswith(".norm2"))
        lin = piece(net, "linear", "to_q GEMM", lambda a: a[1].endswith(".attn2.to_q"))
        kf, kb = hip.cross_attn_fewkeys, hip.cross_attn_fewkeys_backward
        hip.cross_attn_fewkeys = timed("forward kernel", kf)
        hip.cross_attn_fewkeys_backward = timed("backward kernels", kb)
        cross = net.cross_attention

        def ca(*a, **k):
            inside[0] = True
            try:
                return cross(*a, **k)
            finally:
                inside[0] = False
        net.cross_attention = ca
        hip.kernel_profile = []
        ms_prof, _ = wall(lambda: tr.step(st))
        net.cross_attention, net.layernorm, net.linear = cross, ln, lin
        hip.cross_attn_fewkeys, hip.cross_attn_fewkeys_backward = kf, kb
        agg = collections.defaultdict(lambda: [0, 0.0])
        for label, e0, e1 in recs:
            agg[label][0] += 1; agg[label][1] += e0.elapsed_time(e1)
        by_c = collections.defaultdict(lambda: [0, 0.0, 0.0])          # the backward kernels by width: calls, ms, minimum bytes
        for e0, e1, family, _, nbytes in hip.kernel_profile:
            if family == "attn_cross_bwd":
                r = by_c[int(nbytes)]
                r[0] += 1; r[1] += e0.elapsed_time(e1); r[2] += nbytes
        hip.kernel_profile = None
        listed = ("LayerNorm norm2", "to_q GEMM", "forward kernel", "backward kernels")
        total = sum(agg[k][1] for k in listed)
        rec["cross_attention"] = {
            "pieces": {k: {"calls": n, "ms": round(ms, 3), "share_of_step": round(ms / step_ms, 4)}
                       for k, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1])},
            "listed_pieces": list(listed), "total_ms": round(total, 3), "share_of_step": round(total / step_ms, 4),
            "total_with_closures_ms": round(sum(ms for _, ms in agg.values()), 3),
            "backward_kernels_by_minimum_bytes": [{"min_MB_per_call": round(b / 1e6, 2), "calls": n, "ms": round(ms, 3),
                                                   "GBps_of_minimum": round(tot / ms / 1e6, 1)}
                                                  for b, (n, ms, tot) in sorted(by_c.items(), reverse=True)],
            "step_ms_with_events": round(ms_prof, 1)}
    print(json.dumps(rec))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       f"r26a_train_step_ctx_P{P}_{8 * h}x{8 * w}x{Tn}_{'fp16' if dtype == torch.float16 else 'bf16'}.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--max_grad_norm", type=float, default=None, help="measure the cost of global-norm gradient clipping at this "
                    "threshold (the reference's DeepSpeed config uses 0.5) instead of the operator / sweep probes")
    ap.add_argument("--manip448", action="store_true", help="time the fine-tuning step on a 448 x 448 manipulation clip (14 frames "
                    "unless --frames says otherwise)")
    ap.add_argument("--frames", type=int, default=None, help="time the fine-tuning step at this many frames (1 .. 32; above 16 the "
                    "32-slot tape): a PH x PW navigation clip, or the --manip448 one")
    ap.add_argument("--gradient_checkpointing", action="store_true", help="with --frames / --manip448: the step without and with "
                    "activation checkpointing (off, on, off, on): forward / backward / step ms and peak GiB per mode, written to "
                    "profiles/r25a_train_step_ckpt_<size>x<frames>_<dtype>.json")
    ap.add_argument("--num_past_obs", type=int, default=None, help="time the fine-tuning step (PH x PW x 14 navigation) with this many "
                    "conditioning tokens per sample (1 .. 8) and, above 1, the 32 cross-attentions by piece; written to "
                    "profiles/r26a_train_step_ctx_P<P>_<size>x14_<dtype>.json")
    ap.add_argument("--batch", type=int, default=None, help="with --manip448 / --frames: the step on batches of 1, 2, 4, ... and "
                    "this many clips on one tape (ms per step, ms per clip, peak GiB, ratio to the B = 1 row; with "
                    "--gradient_checkpointing: under activation checkpointing); written to profiles/r27a_train_step_batch_*.json")
    ap.add_argument("--steps", type=int, default=5, help="--max_grad_norm / --manip448 / --frames / --num_past_obs: timed steps per block")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    args = ap.parse_args()
    if args.num_past_obs is not None:
        past_obs_probe(args.num_past_obs, torch.float16 if args.dtype == "fp16" else torch.bfloat16, args.steps)
        sys.exit(0)
    if args.batch is not None:
        if not 1 <= args.batch <= 64:
            ap.error("--batch: 1 .. 64 clips per step")
        batch_probe(args.batch, 14 if args.frames is None else args.frames, args.manip448,
                    torch.float16 if args.dtype == "fp16" else torch.bfloat16, args.steps, args.gradient_checkpointing)
        sys.exit(0)
    if args.gradient_checkpointing:
        if not (args.manip448 or args.frames is not None):
            ap.error("--gradient_checkpointing needs --frames N and / or --manip448")
        checkpoint_cost(14 if args.frames is None else args.frames, args.manip448,
                        torch.float16 if args.dtype == "fp16" else torch.bfloat16, args.steps)
        sys.exit(0)
    if args.manip448 or args.frames is not None:
        train_step_probe(14 if args.frames is None else args.frames, args.manip448,
                         torch.float16 if args.dtype == "fp16" else torch.bfloat16, args.steps)
        sys.exit(0)
    if args.max_grad_norm is not None:
        clip_cost(args.max_grad_norm, args.steps, torch.float16 if args.dtype == "fp16" else torch.bfloat16)
        sys.exit(0)
    if os.environ.get("ONLY", "") != "sweep":
        step_by_operator()
    if os.environ.get("ONLY", "") != "ops":
        wgrad_sweep()
