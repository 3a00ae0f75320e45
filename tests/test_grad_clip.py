"""Global-norm gradient clipping (the `gradient_clipping` of the reference's DeepSpeed configs), CPU side: the exported
symbols, `parallel.ShardedAdamW(max_grad_norm=)` and `train_unet.Trainer(max_grad_norm=)` at world size 2 under gloo around
torch restatements / a stub network, argument checking, the unchanged default path and the reference anchors of the GPU
tests (tests/test_hip_grad_clip.py)."""
import ctypes
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wiw_grad_sumsq_chunk", "wiw_grad_sumsq_partials", "wiw_grad_norm_finalize", "wiw_adamw_step_scaled")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _adamw_torch(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale=None):
    """`Hip.adamw_step` restated in torch, with the device-side gradient scale: the product is rounded to fp32 first."""
    if grad_scale is not None:
        g = g * grad_scale
    p.mul_(1 - lr * wd)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.addcdiv_(m / (1 - b1 ** step), (v / (1 - b2 ** step)).sqrt() + eps, value=-lr)


def _adamw_torch_10(p, g, m, v, step, lr, b1, b2, eps, wd):
    """The ten-argument signature existing callers pass: it must keep working while clipping is off."""
    _adamw_torch(p, g, m, v, step, lr, b1, b2, eps, wd)


def _spawn(target, *args, world=2, timeout=180):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time

    res, deadline = [], time.time() + timeout
    try:
        while len(res) < world:
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:                 # a worker that died will never answer: fail now, not at the timeout
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.time() < deadline, "workers did not answer in time"
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:                         # a failed run leaves no worker waiting in a collective
            if p.is_alive():
                p.terminate()
    return sorted(res, key=lambda r: r[0])


# ----------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import LIB_F16, build
    from wiw_amd.hip import EXPORTS

    txt = open(os.path.join(ROOT, "include", "wiw_svd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in txt.split("#define WIW_ABI_VERSION")[1].split("int wiw_abi_version")[0], f"{name}: not in the header's comment block"
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(wiw_[a-z0-9_]+)\s*\(", code))
    lib = build(verbose=False)
    for path in (lib, LIB_F16):
        so = ctypes.CDLL(path)
        so.wiw_abi_version.restype = ctypes.c_int
        assert so.wiw_abi_version() == 17                      # additive: the version does not move
        for name in NEW_SYMBOLS:
            assert name in declared and name in EXPORTS and hasattr(so, name), (name, os.path.basename(path))
        so.wiw_grad_sumsq_chunk.restype = ctypes.c_int
        L = so.wiw_grad_sumsq_chunk()
        assert L >= 1024 and L & (L - 1) == 0 and L % 4 == 0   # a power of two: the chunk sum is a complete pairwise tree


def test_entry_points_validate_before_launching():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import build
    from wiw_amd.hip import load_library

    lib = load_library(build(verbose=False))
    assert lib.wiw_grad_sumsq_partials(None, None, 1, 1, None, 0) == -1 and b"grad_sumsq" in lib.wiw_last_error()
    assert lib.wiw_grad_norm_finalize(None, None, 0, 0.5, None) == -1 and b"grad_norm_finalize" in lib.wiw_last_error()
    assert lib.wiw_adamw_step_scaled(None, 16, 16, 16, 16, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == -1
    assert b"gscale" in lib.wiw_last_error()


# ----------------------------------------------------------------------------------------------------------------
# ShardedAdamW(max_grad_norm=) against clip_grad_norm_ + torch.optim.AdamW on the mean gradient
# ----------------------------------------------------------------------------------------------------------------
def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import wiw_amd  # noqa: F401
    from wiw_amd.parallel import ShardedAdamW

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c, lr = 0.5, 1e-2
        g0 = torch.Generator().manual_seed(11)
        shapes = {"a.weight": (40, 7), "b.bias": (33,), "c.weight": (64, 9), "d.blend": (1,)}
        init = {k: torch.randn(*s, generator=g0) for k, s in shapes.items()}
        opt = ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, bucket_elems=256, lr=lr, weight_decay=0.05, max_grad_norm=c)
        opt.load(init)
        ref = {k: v.clone().requires_grad_(True) for k, v in init.items()}
        ropt = torch.optim.AdamW(list(ref.values()), lr=lr, weight_decay=0.05)
        # per-rank gradients: unit-variance noise times a step scale.  890 elements: the mean gradient's norm is about
        # scale * sqrt(890 / 2) = 21.1 * scale, so 1.0 and 0.1 clip at c = 0.5 (norms ~ 21 and ~ 2.1) and 0.005 does not (~ 0.11)
        coefs, ref_norms = [], []
        for step, scale in enumerate((1.0, 0.1, 0.005)):
            per_rank = [{k: scale * torch.randn(*s, generator=torch.Generator().manual_seed(100 * step + 10 * r + i))
                         for i, (k, s) in enumerate(shapes.items())} for r in range(world)]
            for k in shapes:
                opt.view(opt.grads, k).copy_(per_rank[rank][k])
                ref[k].grad = sum(pr[k] for pr in per_rank) / world
            opt.step()
            ref_norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), c)))
            ropt.step()
            rec = opt.clip_record.tolist()
            coefs.append(rec[2])
            assert rec[3] == 1.0 and abs(rec[1] - ref_norms[-1]) <= 1e-5 * ref_norms[-1], (rec, ref_norms)
            assert abs(rec[2] - min(1.0, c / (ref_norms[-1] + 1e-6))) <= 1e-6
        err = max(float((opt.view(opt.params, k) - ref[k].detach()).abs().max()) for k in shapes)
        mine = {k: opt.view(opt.params, k).clone() for k in shapes}
        both = [None] * world
        dist.all_gather_object(both, mine)
        same = all(torch.equal(both[0][k], both[1][k]) for k in shapes)
        q.put((rank, err, coefs, same))
    finally:
        dist.destroy_process_group()


def test_sharded_adamw_clips_like_clip_grad_norm_then_adamw():
    for rank, err, coefs, same in _spawn(_sharded_worker):
        assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0, coefs      # clipped, clipped, not clipped
        assert err <= 5e-6, err               # the gate of test_trainer_gloo.py: fp32 AdamW restated in another operation order
        assert same                           # every rank took the same coefficient: equal parameters after the all-gather


def test_update_fn_keeps_its_ten_arguments_while_clipping_is_off():
    sys.path.insert(0, ROOT)
    import wiw_amd  # noqa: F401
    from wiw_amd.parallel import ShardedAdamW

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        opt = ShardedAdamW({"w": (5, 3)}, torch.device("cpu"), _adamw_torch_10, bucket_elems=8, lr=1e-2)
        assert opt.max_grad_norm is None and opt.clip_record is None
        opt.load({"w": torch.ones(5, 3)})
        opt.view(opt.grads, "w").fill_(100.0)
        opt.step()                                                              # a TypeError here = the keyword leaked
        assert opt.clip_record is None
        for bad in (0, -1.0, float("inf"), float("nan"), "0.5", True):
            with pytest.raises(ValueError, match="max_grad_norm"):
                ShardedAdamW({"w": (5, 3)}, torch.device("cpu"), _adamw_torch, max_grad_norm=bad)
    finally:
        dist.destroy_process_group()


# ----------------------------------------------------------------------------------------------------------------
# Trainer at world size 2 around a stub network (the style of tests/test_trainer_gloo.py)
# ----------------------------------------------------------------------------------------------------------------
class _Tape:
    after_op = None


class _StubNet:
    """loss = 0.5 * sum_k c_k |w_k - t|^2: dL/dw_k = c_k (w_k - t), produced LAST parameter first with the tape hook after each."""
    dt, device = torch.bfloat16, torch.device("cpu")

    def __init__(self, poison_rank=None, gain=1.0):
        g = torch.Generator().manual_seed(3)
        self.master = {"a.weight": torch.randn(40, 7, generator=g), "b.bias": torch.randn(33, generator=g),
                       "c.weight": torch.randn(64, 9, generator=g), "frozen.weight": torch.randn(5, 5, generator=g)}
        self.coef = {"a.weight": 1.0 * gain, "b.bias": 0.5 * gain, "c.weight": 2.0 * gain}
        self.tape, self.grads, self.wants, self.hip, self._direct = _Tape(), {}, (lambda n: True), None, {}
        self.refreshed, self.poison = 0, poison_rank

    def forward(self, target, *_):
        self.grads, self._t = {}, float(target)
        return torch.zeros(1)

    def backward(self, dpred, loss_scale=1.0):
        for k in reversed(list(self.coef)):
            g = self.coef[k] * (self.master[k] - self._t)
            if self.poison is not None and dist.is_initialized() and dist.get_rank() == self.poison and k == "b.bias":
                g = g * float("inf")
            self.grads[k] = g
            if self.tape.after_op is not None:
                self.tape.after_op()
        return self.grads

    def refresh(self, names=None):
        self.refreshed += 1


class _St:
    def __init__(self, target):
        self.unet_input, self.timestep, self.ehs, self.added_time_ids, self.action_ids = target, None, None, None, None


def _stub_train_step():
    from wiw_amd import train as T

    class _TrainStep:                      # the EDM loss kernel is not part of these tests
        def __init__(self, hip):
            pass

        def loss_and_grad(self, pred, st):
            return torch.tensor(1.0), torch.zeros(1)
    T.TrainStep = _TrainStep


def _trainer_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import conftest  # noqa: F401  (registers the package alias)
    import wiw_amd  # noqa: F401
    from wiw_amd.parallel import ShardedAdamW
    from wiw_amd.train_unet import Trainer

    _stub_train_step()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lr, accum, c = 1e-2, 2, 0.5
        net = _StubNet()
        shapes = {k: tuple(v.shape) for k, v in net.master.items() if k in net.coef}
        opt = ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, bucket_elems=256, lr=lr, weight_decay=0.05, max_grad_norm=c)
        tr = Trainer(net, lr=lr, weight_decay=0.05, optimizer=opt, grad_accum=accum, loss_scale=1.0, max_grad_norm=c)
        assert tr.max_grad_norm == c and tr.grad_norm is None
        ref = {k: v.clone().requires_grad_(True) for k, v in net.master.items() if k in net.coef}
        ropt = torch.optim.AdamW(list(ref.values()), lr=lr, weight_decay=0.05)
        micro, norm_err, clipped = 0, 0.0, []
        for window in range(3):
            mean = {k: torch.zeros_like(v) for k, v in ref.items()}
            for mb in range(accum):
                for r in range(world):
                    t = 0.1 * (1 + r) + 0.01 * micro
                    for k in ref:
                        mean[k] += net.coef[k] * (ref[k].detach() - t) / (world * accum)
                tr.step(_St(0.1 * (1 + rank) + 0.01 * micro))
                micro += 1
            assert tr.steps == window + 1
            for k in ref:
                ref[k].grad = mean[k]
            n_ref = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), c))
            ropt.step()
            norm_err = max(norm_err, abs(tr.grad_norm - n_ref) / n_ref)          # the norm of the window's MEAN gradient, pre-clip
            clipped.append(n_ref > c)
        err = max(float((net.master[k] - ref[k].detach()).abs().max()) for k in ref)
        overlapped = opt.async_launched > 0                                       # the hand-over during the backward still happens
        # ---- overflow on ONE rank with clipping on: every rank skips, the scale halves, nothing moves, the norm is non-finite
        net2 = _StubNet(poison_rank=1)
        opt2 = ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, bucket_elems=256, lr=lr, max_grad_norm=c)
        tr2 = Trainer(net2, lr=lr, optimizer=opt2, loss_scale=4.0)                # the optimiser's own setting is enough
        assert tr2.max_grad_norm == c
        start = {k: v.clone() for k, v in net2.master.items()}
        tr2.step(_St(0.3))
        skipped = (tr2.steps == 0 and tr2.loss_scale == 2.0 and all(torch.equal(net2.master[k], start[k]) for k in start)
                   and not math.isfinite(tr2.grad_norm))
        net2.poison = None
        tr2.step(_St(0.3))
        moved = tr2.steps == 1 and not torch.equal(net2.master["a.weight"], start["a.weight"]) and math.isfinite(tr2.grad_norm)
        q.put((rank, err, norm_err, clipped, overlapped, skipped, moved))
    finally:
        dist.destroy_process_group()


def test_trainer_clips_the_window_mean_and_still_skips_globally():
    for rank, err, norm_err, clipped, overlapped, skipped, moved in _spawn(_trainer_worker):
        assert all(clipped), clipped          # the stub's gradients are far above 0.5: every window is clipped
        assert err <= 5e-6, err               # == clip_grad_norm_ + AdamW on the mean over ranks and micro-batches
        assert norm_err <= 1e-5, norm_err     # fp32 norm of 889 elements against torch's (another summation order)
        assert overlapped and skipped and moved, (rank, overlapped, skipped, moved)


def _one_rank_group():
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)


def test_bad_and_mismatched_thresholds_raise():
    sys.path.insert(0, ROOT)
    import wiw_amd  # noqa: F401
    from wiw_amd.parallel import ShardedAdamW
    from wiw_amd.train_unet import Trainer

    for bad in (0, 0.0, -0.5, float("inf"), float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Trainer(_StubNet(), max_grad_norm=bad)
    assert Trainer(_StubNet(), loss_scale=1.0).max_grad_norm is None
    _one_rank_group()
    try:
        net = _StubNet()
        shapes = {k: tuple(v.shape) for k, v in net.master.items() if k in net.coef}
        with pytest.raises(ValueError, match="disagree"):
            Trainer(net, optimizer=ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, max_grad_norm=1.0), max_grad_norm=0.5)
        with pytest.raises(ValueError, match="optimizer clips"):             # the Trainer never configures an external optimiser
            Trainer(net, optimizer=ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch), max_grad_norm=0.5)
        tr = Trainer(net, optimizer=ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, max_grad_norm=0.5), max_grad_norm=0.5)
        assert tr.max_grad_norm == 0.5
        with pytest.raises(RuntimeError, match="norm_ops"):                   # no torch stand-in for the HIP reduction on a GPU
            ShardedAdamW(shapes, torch.device("cuda", 0), _adamw_torch, max_grad_norm=0.5)
    finally:
        dist.destroy_process_group()


def test_default_is_off_and_bit_identical_to_the_plain_update():
    """max_grad_norm=None: the sharded stub run gives exactly the parameters of the parent's formula — the same torch
    restatement applied to the same mean gradients, outside Trainer / ShardedAdamW — and the step records keep their keys."""
    sys.path.insert(0, ROOT)
    import wiw_amd  # noqa: F401
    from wiw_amd.parallel import ShardedAdamW
    from wiw_amd.train_unet import Trainer

    _stub_train_step()
    _one_rank_group()
    try:
        lr = 1e-2
        net = _StubNet(gain=50.0)                                              # gradients far above any sensible threshold
        shapes = {k: tuple(v.shape) for k, v in net.master.items() if k in net.coef}
        opt = ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch_10, bucket_elems=256, lr=lr, weight_decay=0.05)
        tr = Trainer(net, lr=lr, weight_decay=0.05, optimizer=opt, loss_scale=1.0)
        p = {k: net.master[k].clone() for k in net.coef}
        m = {k: torch.zeros_like(v) for k, v in p.items()}
        v = {k: torch.zeros_like(x) for k, x in p.items()}
        log = tr.fit([_St(0.1 * i) for i in range(3)], max_train_steps=3)
        for i in range(3):
            for k in p:
                _adamw_torch_10(p[k], net.coef[k] * (p[k] - 0.1 * i), m[k], v[k], i + 1, lr, 0.9, 0.999, 1e-8, 0.05)
        assert all(torch.equal(net.master[k], p[k]) for k in p)
        assert tr.grad_norm is None and opt.clip_record is None
        assert [sorted(r) for r in log] == [["lr", "step", "train_loss"]] * 3
        # ... and with clipping on the record gains exactly one key
        net2 = _StubNet()
        opt2 = ShardedAdamW(shapes, torch.device("cpu"), _adamw_torch, bucket_elems=256, lr=lr, max_grad_norm=0.5)
        log2 = Trainer(net2, lr=lr, optimizer=opt2, loss_scale=1.0).fit([_St(0.1)], max_train_steps=1)
        assert sorted(log2[0]) == ["grad_norm", "lr", "step", "train_loss"] and log2[0]["grad_norm"] > 0.5
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fixture,anchor", [("train_step_tiny.npz", 1.3216), ("train_step_full_32x64.npz", 5.9572)])
def test_reference_global_norm_anchors(fixture, anchor):
    """sqrt(sum(grad_norms^2)) of the reference's own backward: the figure the GPU tests compare `Trainer.grad_norm` with.
    A regenerated fixture cannot move it silently.  The dead parameters add nothing visible to it."""
    import wiw_amd  # noqa: F401
    from wiw_amd.train_unet import Trainer

    g = np.load(os.path.join(ROOT, "tests", "golden", fixture), allow_pickle=True)
    norms = g["grad_norms"].astype(np.float64)
    total = float(np.sqrt((norms ** 2).sum()))
    assert round(total, 4) == anchor, total
    dead = np.array([Trainer.is_dead(str(n)) for n in g["grad_names"]])
    assert float(np.sqrt((norms[dead] ** 2).sum())) <= 1e-6 * total
