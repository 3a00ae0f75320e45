"""The 32-frame-slot temporal attention kernels (csrc/temporal32.hip) against the fp32 restatement of
tests/test_hip_temporal_block.py (`reference()`), at that file's tolerances: max <= 2e-2 * max|ref|, rms <= 8e-3 (Q, K, V and
the probabilities are rounded to 16 bits between the MFMA stages).  Outputs are pre-filled with NaN and checked finite: a row
left unwritten, or a padding frame slot that reached O, shows.  GPU only."""
import math

import pytest
import torch

from test_hip_temporal_block import reference, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_HIPS = {}

# the whole product T x S (tails of the 8-site tile, and S = 1) x heads x B, both entries, both dtypes: one test per (T, dtype)
# walks S x heads x B (60 shapes) so that the operands and the fp32 restatement of a shape are made once for both entries
T_LIST, S_LIST, HEADS_LIST, B_LIST = (17, 24, 25, 31, 32), (9, 49, 196, 400, 1), (1, 5, 10, 20), (1, 2, 3)


def get_hip(name):
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip

    if name not in _HIPS:
        _HIPS[name] = Hip(torch.device(DEV), DTYPES[name])
    return _HIPS[name]


def operands(B, T, S, heads, dt):
    from wiw_amd.unet import pack_temporal_qkv

    C = heads * 64
    r16 = lambda t: t.to(dt).float()   # noqa: E731
    x = r16(rnd(B, T, S, C, seed=1) * 1.5 + 0.3)
    x[..., 5] += 4.0                                            # a channel with an offset: the fold must remove the mean
    x = r16(x)
    wq, wk, wv = (rnd(C, C, seed=s) / math.sqrt(C) for s in (2, 3, 4))
    gamma, beta = 1 + 0.2 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    wg, fold = pack_temporal_qkv(wq, wk, wv, gamma, beta, dtype=dt)
    return x, (wq, wk, wv, gamma, beta), wg, fold, r16


def run_fused(hip, x, wg, fold, B, T, S, heads, dt):
    C = heads * 64
    o = torch.full((B * T * S, C), float("nan"), dtype=dt, device=DEV)
    hip.temporal_attn_block32(x.reshape(-1, C).to(DEV, dt).contiguous(), wg.to(DEV), fold.to(DEV), o, C, B, T, S, heads, 1e-5, 0.125)
    torch.cuda.synchronize()
    return o


def errors(o, ref):
    out = o.float().cpu().reshape(ref.shape)
    assert torch.isfinite(out).all(), "rows left unwritten or non-finite"
    err = (out - ref).abs()
    return float(err.max() / ref.abs().max()), float(err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("T", T_LIST)
def test_kernels32_parity(T, name):
    """Fused block and unfused attention (its QKV made in fp32 from the same operands and rounded once) on every shape."""
    import torch.nn.functional as F

    hip, dt = get_hip(name), DTYPES[name]
    bad = []
    for S in S_LIST:
        for heads in HEADS_LIST:
            for B in B_LIST:
                C = heads * 64
                x, (wq, wk, wv, gamma, beta), wg, fold, r16 = operands(B, T, S, heads, dt)
                o = run_fused(hip, x, wg, fold, B, T, S, heads, dt)
                ref = reference(x, gamma, beta, r16(wq), r16(wk), r16(wv), heads)
                mx, rms = errors(o, ref)
                a = F.layer_norm(x, (C,), gamma, beta, 1e-5)
                qkv = r16(torch.cat([a @ r16(wq).t(), a @ r16(wk).t(), a @ r16(wv).t()], dim=-1))      # (B,T,S,3C)
                o2 = torch.full((B * T * S, C), float("nan"), dtype=dt, device=DEV)
                hip.attn_temporal32(qkv.reshape(-1, 3 * C).to(DEV, dt).contiguous(), 3 * C, o2, C, B, T, S, heads, 0.125)
                torch.cuda.synchronize()
                q, k, v = qkv.split(C, dim=-1)

                def perm(t):
                    return t.permute(0, 2, 1, 3).reshape(B * S, T, heads, 64).transpose(1, 2)

                ref2 = F.scaled_dot_product_attention(perm(q), perm(k), perm(v)).transpose(1, 2).reshape(B, S, T, C).permute(0, 2, 1, 3)
                mx2, rms2 = errors(o2, ref2)
                print(f"[parity] {name} B={B} T={T} S={S} heads={heads}: temporal_attn_block32 max_rel={mx:.3e} rms_rel={rms:.3e} | "
                      f"attn_temporal32 max_rel={mx2:.3e} rms_rel={rms2:.3e}")
                if not (mx <= 2e-2 and rms <= 8e-3 and mx2 <= 2e-2 and rms2 <= 8e-3):
                    bad.append((B, T, S, heads, mx, rms, mx2, rms2))
    assert not bad, bad


@pytest.mark.parametrize("T", [1, 4, 14, 16])
def test_both_entries_accept_short_horizons(T):
    """1 <= T <= 32 is the contract of both entries (the UNet routes T <= 16 to the 16-slot kernels; the ABI does not care)."""
    hip, dt = get_hip("bf16"), torch.bfloat16
    B, S, heads = 2, 20, 2
    x, (wq, wk, wv, gamma, beta), wg, fold, r16 = operands(B, T, S, heads, dt)
    ref = reference(x, gamma, beta, r16(wq), r16(wk), r16(wv), heads)
    mx, rms = errors(run_fused(hip, x, wg, fold, B, T, S, heads, dt), ref)
    assert mx <= 2e-2 and rms <= 8e-3


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_repeatable_and_batch_independent(name):
    """The same launch twice: the same bytes; item i of a B = 3 launch: the bytes of its own B = 1 launch (both entries)."""
    hip, dt = get_hip(name), DTYPES[name]
    B, T, S, heads = 3, 25, 49, 5
    C = heads * 64
    x, _, wg, fold, _ = operands(B, T, S, heads, dt)
    o1 = run_fused(hip, x, wg, fold, B, T, S, heads, dt)
    o2 = run_fused(hip, x, wg, fold, B, T, S, heads, dt)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    qkv = (rnd(B, T, S, 3 * C, seed=9)).to(dt)
    u = []
    for _ in range(2):
        o = torch.full((B * T * S, C), float("nan"), dtype=dt, device=DEV)
        hip.attn_temporal32(qkv.reshape(-1, 3 * C).to(DEV).contiguous(), 3 * C, o, C, B, T, S, heads, 0.125)
        u.append(o)
    torch.cuda.synchronize()
    assert torch.equal(u[0].view(torch.int16), u[1].view(torch.int16))
    for i in range(B):
        oi = run_fused(hip, x[i:i + 1], wg, fold, 1, T, S, heads, dt)
        assert torch.equal(oi.view(torch.int16), o1.reshape(B, T * S, C)[i].view(torch.int16)), f"fused: item {i}"
        ui = torch.full((T * S, C), float("nan"), dtype=dt, device=DEV)
        hip.attn_temporal32(qkv[i].reshape(-1, 3 * C).to(DEV).contiguous(), 3 * C, ui, C, 1, T, S, heads, 0.125)
        torch.cuda.synchronize()
        assert torch.equal(ui.view(torch.int16), u[0].reshape(B, T * S, C)[i].view(torch.int16)), f"unfused: item {i}"


def test_fused32_matches_unfused_chain_level0_shape():
    """2 x 25 x 9216 x 320, the first level of a 25-frame 576x1024 forward: the fused kernel against the unfused HIP chain
    (LayerNorm kernel -> QKV GEMM -> wiw_attn_temporal32_bf16) and against the fp32 restatement on a strided site sample."""
    from wiw_amd.unet import pack_temporal_qkv

    hip = get_hip("bf16")
    B, T, S, heads = 2, 25, 9216, 5
    C = heads * 64
    bf = lambda t: t.to(torch.bfloat16).float()   # noqa: E731
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (torch.randn(B * T * S, C, generator=g, device=DEV) * 1.5 + 0.3).to(torch.bfloat16)
    wq, wk, wv = (rnd(C, C, seed=s) / math.sqrt(C) for s in (2, 3, 4))
    gamma, beta = 1 + 0.2 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    wg, fold = pack_temporal_qkv(wq, wk, wv, gamma, beta)
    o = torch.full((B * T * S, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.temporal_attn_block32(x, wg.to(DEV), fold.to(DEV), o, C, B, T, S, heads, 1e-5, 0.125)
    a = hip.layernorm(x, B * T * S, C, gamma.to(DEV), beta.to(DEV))
    wqkv = torch.cat([wq, wk, wv]).to(DEV, torch.bfloat16).contiguous()
    qkv = torch.empty(B * T * S, 3 * C, dtype=torch.bfloat16, device=DEV)
    hip.gemm(a, wqkv, qkv, M=B * T * S, N=3 * C, K=C, C1=C)
    o2 = torch.full_like(o, float("nan"))
    hip.attn_temporal32(qkv, 3 * C, o2, C, B, T, S, heads, 0.125)
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and torch.isfinite(o2.float()).all()
    d = (o.float() - o2.float())
    rms_chain = float(d.pow(2).mean().sqrt() / o2.float().pow(2).mean().sqrt())
    sites = torch.arange(0, S, 37)
    xs = x.reshape(B, T, S, C)[:, :, sites.to(DEV)].float().cpu()
    ref = reference(xs, gamma, beta, bf(wq), bf(wk), bf(wv), heads)
    mx, rms = errors(o.reshape(B, T, S, C)[:, :, sites.to(DEV)], ref)
    print(f"[parity] temporal_attn_block32 2x25x9216x320: vs fp32 max_rel={mx:.3e} rms_rel={rms:.3e}; vs unfused HIP chain rms={rms_chain:.3e}")
    assert mx <= 2e-2 and rms <= 8e-3 and rms_chain <= 1.2e-2
