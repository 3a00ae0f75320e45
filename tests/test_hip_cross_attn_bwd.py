"""Backward of the few-keys cross-attention (csrc/cross_attn_bwd.hip, include/wiw_cross_attn_train.h) — GPU, both libraries.

dQ, dK, dV of `Hip.cross_attn_fewkeys_backward` against torch fp32 autograd through the same formula,
    O = softmax_p(q . k_p / 8) v_p     per row, head (64 channels) and item,
on the same 16-bit-rounded q, k, v, dO.  Gate: the project's kernel-level backward gate, relative max <= 2e-2 and rms <= 8e-3
(tests/test_hip_train_horizon.py, tests/test_hip_train.py `test_attention_backward`).  q, k ~ N(0, 1) with scale 1/8: the
logits are ~N(0, 1), the softmax neither uniform nor one-hot.  Shapes where the kernel can go wrong:

  heads 1 / 5 / 20   C = 64 / 320 / 1280: 32 row slots per block; 6 slots + 16 surplus threads; 1 slot + 96 surplus threads
  P 1 / 2 / 3 / 8    the closed form (dQ = dK = 0 exactly, dV = sum dO); the smallest softmax; an odd count; every register
  rows_per_item      1 (fewer rows than slots), 37 (a ragged tail), 600 (several blocks, the last one ragged)
  items 1 / 2        the partials of the second item start behind the first one's

Measured on MI355X, worst over the 24 shapes of a width: dQ bf16 max <= 3.4e-3, rms <= 1.9e-3 (fp16 3.9e-4 / 2.2e-4); dK and
dV (fp32 outputs of fp32 sums over exact 16-bit products) max <= 1.2e-6, rms <= 5.5e-7 in both builds.
"""
import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
GATE = (2e-2, 8e-3)
_HIPS = {}


def _hip(dtype):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    if dtype not in _HIPS:
        _HIPS[dtype] = Hip(torch.device(DEV), dtype)
    return _HIPS[dtype]


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)), float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _operands(dtype, heads, P, rpi, items, seed=0):
    r16 = lambda t: t.to(dtype).float()  # noqa: E731
    C, rows = heads * 64, items * rpi
    q, do = r16(_rnd(rows, C, seed=seed + 1)), r16(_rnd(rows, C, seed=seed + 2))
    k, v = r16(_rnd(items, P, C, seed=seed + 3)), r16(_rnd(items, P, C, seed=seed + 4))
    return q, k, v, do


def _autograd(q, k, v, do, heads, P, rpi, items):
    """fp32 autograd through the forward's formula -> (dQ [rows, C], dK, dV [items, P, C])."""
    C = heads * 64
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    qh = ql.reshape(items, rpi, heads, 64).permute(0, 2, 1, 3)
    kh, vh = (t.reshape(items, P, heads, 64).permute(0, 2, 1, 3) for t in (kl, vl))
    w = torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, dim=-1)
    o = (w @ vh).permute(0, 2, 1, 3).reshape(items * rpi, C)
    o.backward(do)
    return ql.grad, kl.grad, vl.grad


def _launch(hip, dtype, q, k, v, do, heads, P, rpi, items, ld=None):
    """ld: Q, dO and dQ are windows [:, :C] of wider [rows, ld] buffers (dQ's surroundings are checked by the caller)."""
    C, rows = heads * 64, items * rpi
    dev = lambda t: t.to(DEV, dtype).contiguous()  # noqa: E731
    K, V = dev(k), dev(v)
    if ld is None:
        return hip.cross_attn_fewkeys_backward(dev(q), C, K, V, dev(do), C, rows, rpi, heads, P, 0.125)
    Qb, dOb = (torch.full((rows, ld), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
    Qb[:, :C], dOb[:, :C] = dev(q), dev(do)
    dQb = torch.full((rows, ld), 7.0, dtype=dtype, device=DEV)
    _, dK, dV = hip.cross_attn_fewkeys_backward(Qb, ld, K, V, dOb, ld, rows, rpi, heads, P, 0.125, dQ=dQb, lddq=ld)
    return dQb, dK, dV


CASES = [(heads, P, rpi, items) for heads in (1, 5, 20) for P in (1, 2, 3, 8) for rpi in (1, 37, 600) for items in (1, 2)]


@DTYPES
@pytest.mark.parametrize("heads", [1, 5, 20])
def test_backward_matches_fp32_autograd(heads, dtype):
    """Every (P, rows_per_item, items) of the module docstring at one width; each launch is repeated and compared bit for bit."""
    hip = _hip(dtype)
    worst = {}
    for _, P, rpi, items in (c for c in CASES if c[0] == heads):
        q, k, v, do = _operands(dtype, heads, P, rpi, items, seed=10 * P + rpi)
        ref = _autograd(q, k, v, do, heads, P, rpi, items)
        got = _launch(hip, dtype, q, k, v, do, heads, P, rpi, items)
        again = _launch(hip, dtype, q, k, v, do, heads, P, rpi, items)
        torch.cuda.synchronize()
        tag = f"[cross_attn_bwd {dtype}] heads={heads} P={P} rows/item={rpi} items={items}"
        C = heads * 64
        assert tuple(got[0].shape) == (items * rpi, C) and got[0].dtype == dtype, tag
        assert tuple(got[1].shape) == tuple(got[2].shape) == (items, P, C) and got[1].dtype == got[2].dtype == torch.float32, tag
        for name, a, b in zip(("dQ", "dK", "dV"), got, again):
            assert bool(torch.isfinite(a.float()).all()), (tag, name)
            assert torch.equal(a, b), (tag, name, "two launches differ")
        if P == 1:        # softmax over one key == 1: dS = w (dP - delta) = 1 * (dP - dP)
            assert bool((got[0].float() == 0).all()) and bool((got[1] == 0).all()), tag
            assert float(ref[0].abs().max()) == 0.0 and float(ref[1].abs().max()) == 0.0
            names = ("dV",)
            exact = do.reshape(items, rpi, C).sum(1)
            mx, rms = _rel(got[2].reshape(items, C), exact)
            assert mx <= 1e-5, (tag, "dV = sum_m dO", mx)        # fp32 sums of <= 600 16-bit values: summation order only
        else:
            names = ("dQ", "dK", "dV")
        for name in names:
            i = ("dQ", "dK", "dV").index(name)
            mx, rms = _rel(got[i], ref[i])
            worst[name] = tuple(max(x, y) for x, y in zip(worst.get(name, (0.0, 0.0)), (mx, rms)))
            print(f"{tag} {name}: max_rel={mx:.2e} rms={rms:.2e}")
            assert mx <= GATE[0] and rms <= GATE[1], (tag, name, mx, rms)
    print(f"[cross_attn_bwd {dtype}] heads={heads} worst (max_rel, rms): {worst}")


@DTYPES
def test_strided_windows(dtype):
    """ldq, lddo, lddq > C: Q / dO / dQ are the first C columns of wider buffers whose other columns are NaN (inputs) or a
    sentinel (dQ) — same values as the dense launch bit for bit, sentinel untouched."""
    hip = _hip(dtype)
    heads, P, rpi, items = 5, 3, 37, 2
    C = heads * 64
    q, k, v, do = _operands(dtype, heads, P, rpi, items, seed=5)
    dense = _launch(hip, dtype, q, k, v, do, heads, P, rpi, items)
    wide = _launch(hip, dtype, q, k, v, do, heads, P, rpi, items, ld=C + 24)
    torch.cuda.synchronize()
    assert torch.equal(wide[0][:, :C], dense[0]) and bool((wide[0][:, C:] == 7.0).all())
    assert torch.equal(wide[1], dense[1]) and torch.equal(wide[2], dense[2])
    ref = _autograd(q, k, v, do, heads, P, rpi, items)
    for name, a, b in zip(("dQ", "dK", "dV"), (wide[0][:, :C], wide[1], wide[2]), ref):
        mx, rms = _rel(a, b)
        assert mx <= GATE[0] and rms <= GATE[1], (name, mx, rms)


@DTYPES
def test_argument_refusals(dtype):
    """Nothing is launched for arguments the header excludes: non-zero return and a `wiw_last_error` text."""
    hip = _hip(dtype)
    lib = hip.lib
    heads, rpi, items = 1, 8, 2
    C, rows = 64, 16
    Q = torch.zeros(rows, C + 8, dtype=dtype, device=DEV)
    dO, dQ = torch.zeros_like(Q), torch.zeros_like(Q)
    K = torch.zeros(items * 9 * C, dtype=dtype, device=DEV)
    V = torch.zeros_like(K)
    f = torch.zeros(items * 2 * 9 * C, dtype=torch.float32, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(ldq=C, lddo=C, lddq=C, rows=rows, rpi=rpi, P=2):
        return lib.wiw_cross_attn_fewkeys_bwd_bf16(hip._stream(), p(Q), ldq, p(K), p(V), p(dO), lddo, p(dQ), lddq, p(f), p(f), p(f),
                                                   rows, rpi, heads, P, 0.125)
    assert call() == 0
    assert call(P=9) != 0 and b"1 <= P <= 8" in lib.wiw_last_error()
    assert call(P=0) != 0 and b"1 <= P <= 8" in lib.wiw_last_error()
    assert call(rows=rows - 1) != 0 and b"whole items" in lib.wiw_last_error()
    assert call(lddq=C - 8) != 0 and b">= C" in lib.wiw_last_error()
    assert call(ldq=C + 4) != 0 and b"multiples of 8" in lib.wiw_last_error()
    assert int(lib.wiw_cross_attn_fewkeys_bwd_partials(rows, rpi, heads, 9)) == 0
    assert int(lib.wiw_cross_attn_fewkeys_bwd_partials(rows, rpi, heads, 2)) == items * 2 * 2 * C
    with pytest.raises(RuntimeError, match="1 <= P <= 8"):
        hip._ck(call(P=9), "wiw_cross_attn_fewkeys_bwd_bf16")
    torch.cuda.synchronize()
