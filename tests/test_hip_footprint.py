"""WHERE every kernel entry point of include/wiw_svd.h reads and writes.  GPU only (the table itself imports without one).

Every operand sits in an arena of tests/footprint.py: strided (leading dimension = used width + the smallest step the entry
point's checks allow), aligned to the MINIMUM the header states and no better, between poisoned guards.  Each case runs three
launches — surroundings zero, finite garbage, NaN — and asserts

    P1 independence   the output windows of the garbage / NaN runs are bit-identical to the zero run
    P2 containment    every byte outside a declared output window is unchanged (padding the header says the kernel writes is
                      part of the window and is checked to hold the documented value)
    P3 inputs         bit-identical after the launch (documented aliasing has its own cases)
    P4 parity         the zero run is correct IN THIS LAYOUT: serving entries against the fp32 CPU reference and gate of the
                      entry's own test (tests/test_hip_kernels.py / _fp16 / _ffn / _clip / _vae / _horizon_kernels /
                      _temporal_block / _res32; fp16 gates that do not exist yet: the 8x rule of test_hip_fp16.py); training
                      entries against a dense-layout launch of the same kernel on the same values, bit for bit
    P5 library state  GroupNorm counters back at zero, scratch / counters arenas sized exactly by the library's size queries

Regions the header assigns to the caller stay as stated (the `zeros` operand, the zero columns S .. Sv-1 of the frame-padded
V^T, clip_preprocess's pre-zeroed A, zero GroupNorm counters).  Routing is decided by reading the dispatchers (csrc/gemm.hip
`launch<>`, `use_big_tile`, csrc/gemm_huge.hip `wiw_gemm_huge_ok`); no environment knob is set.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import footprint as FP

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
F32 = torch.float32
_HIPS = {}

# (max_rel, rms_rel) per build, copied from the entry's own test (see the module docstring); "x8": the 8x rule
GATES = {
    "k16":    {"bf16": (1.2e-2, 4e-3), "fp16": (1.5e-3, 5e-4)},       # test_hip_kernels.py / test_hip_fp16.py `check`
    "gemm2r": {"bf16": (1.2e-2, 4e-3), "fp16": (2e-3, 6e-4)},         # staged epilogue + residual: test_gemm_dense_with_epilogue
    "f32":    {"bf16": (2e-5, 2e-6), "fp16": (2e-5, 2e-6)},           # test_gemm_dense_plain, fp32 out
    "f32res": {"bf16": (2e-5, 3e-6), "fp16": (2e-5, 3e-6)},           # test_hip_res32.py test_gemm_fp32_residuals
    "splitk_f32": {"bf16": (1e-4, 1e-5), "fp16": (1e-4, 1e-5)},       # test_gemm_splitk_dense_all_epilogue_terms
    "lnfold": {"bf16": (1.5e-2, 5e-3), "fp16": (1.5e-2 / 8, 5e-3 / 8)},     # test_gemm_layernorm_fold_*; x8
    "attn":   {"bf16": (2e-2, 8e-3), "fp16": (3e-3, 1e-3)},           # test_attn_spatial*, both files
    "attn_x8": {"bf16": (2e-2, 8e-3), "fp16": (2e-2 / 8, 8e-3 / 8)},  # attn_temporal, attn_small: no fp16 twin; x8
    "cross":  {"bf16": (1.2e-2, 3e-3), "fp16": (1.2e-2 / 8, 3e-3 / 8)},     # test_cross_attention_over_a_few_keys; x8
    "tblock": {"bf16": (2e-2, 8e-3), "fp16": (4e-3, 1.2e-3)},         # test_hip_temporal_block.py / test_hip_fp16.py
    "t32":    {"bf16": (2e-2, 8e-3), "fp16": (2e-2, 8e-3)},           # test_hip_horizon_kernels.py, both builds
    "ffn":    {"bf16": (1.2e-2, 4e-3), "fp16": (1.5e-3, 6e-4)},       # test_hip_ffn.py `check`
    "sum_out": {"bf16": (1e-6, 1e-6), "fp16": (1e-6, 1e-6)},          # test_layernorm, sum_out
    "prep":   {"bf16": (8e-3, 4e-3), "fp16": (1e-3, 5e-4)},           # test_prep_and_euler; x8
    "euler":  {"bf16": (2e-6, 1e-6), "fp16": (2e-6, 1e-6)},
    "softmax": {"bf16": (4e-3, 4e-3), "fp16": (5e-4, 5e-4)},          # test_hip_vae.py test_softmax_rows; x8
    "tconv":  {"bf16": (1e-5, 1e-5), "fp16": (1e-5, 1e-5)},           # test_time_conv_out
    "gn_ab":  {"bf16": (1e-5, 1e-5), "fp16": (1e-5, 1e-5)},           # "fp32-output kernels: 1e-5 relative"
}

CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


class Env:
    def __init__(self, name):
        import wiw_amd  # noqa: F401
        from wiw_amd.hip import Hip

        if name not in _HIPS:
            _HIPS[name] = Hip(torch.device(DEV), DTYPES[name])
        self.name, self.dt, self.hip = name, DTYPES[name], _HIPS[name]
        self.lib = self.hip.lib

    def r(self, x):
        """round to the build's 16-bit type and back: what the kernels see"""
        return x.to(self.dt).float()

    def stream(self):
        return self.hip._stream()

    def ck(self, rc, what):
        self.hip._ck(rc, what)

    def gate(self, kind, what_prefix=""):
        mx_tol, rms_tol = GATES[kind][self.name]

        def check(got, ref, what):
            got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
            assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
            assert bool(torch.isfinite(got).all()), "non-finite output"
            err = (got - ref).abs()
            mx = float(err.max() / (ref.abs().max() + 1e-30))
            rms = float(err.pow(2).mean().sqrt() / (ref.pow(2).mean().sqrt() + 1e-30))
            near = "  [within 2x of its gate]" if (2 * mx > mx_tol or 2 * rms > rms_tol) else ""
            print(f"[footprint P4 {self.name}] {what}: max_rel={mx:.3e} rms_rel={rms:.3e} (gate {mx_tol:.1e} / {rms_tol:.1e}){near}")
            assert mx <= mx_tol and rms <= rms_tol, f"max_rel={mx:.3e} rms_rel={rms:.3e} over the gate {mx_tol:.1e} / {rms_tol:.1e}"
        return check

    def exact(self, got, ref, what):
        got, ref = got.detach().cpu(), ref.detach().cpu()
        assert got.shape == ref.shape and got.dtype == ref.dtype
        it = FP._INT[got.element_size()]
        same = torch.equal(got.contiguous().view(it), ref.contiguous().view(it))
        print(f"[footprint P4 {self.name}] {what}: bit-identical = {same}")
        assert same, "differs from the reference bit pattern"


@functools.lru_cache(maxsize=32)
def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rnd(*shape, seed=0, scale=1.0):
    """seeded N(0, scale); the draw is shared by the three runs of a case (and by its two builds), never modified in place"""
    return _randn(shape, seed) * scale


def ptr(a):
    return None if a is None else a.window().data_ptr()


def win(a):
    return None if a is None else a.window()


def weight(fp, name, w, dt, tiled=True, sw16=False):
    """A weight operand in an arena: plain [N][K] rows, or the TiledW layout — with N not a multiple of 8 the zero rows past N
    are part of the packed operand, the bytes after the last 1-KiB block are poison."""
    from wiw_amd.hip import TiledW, tile_weight

    if not tiled:
        return fp.inp(name, w, dt, gap=0).window()
    ar = fp.inp(name, tile_weight(w.to(dt), sw16=sw16), dt, gap=0)
    tw = TiledW.__new__(TiledW)
    tw.shape, tw.sw16, tw.data = tuple(w.shape), bool(sw16), ar.window().reshape(-1)
    return tw


def nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ======================================================================================================================
# wiw_gemm_bf16, dense mode
# ======================================================================================================================
def gemm_dense(M, N, K, *, tiled=True, bias=True, vec_align=16, rpv=0, res1=None, res2=None, alias=False, out="16", act=0,
               alpha=1.0, splitk=1, c2=0):
    """res1 / res2: None, "16" or "f32"; out: "16" or "f32"; alias: `out` aliases res1 (the documented in-place residual);
    vec_align = 4: bias / rowvec 4-byte and not 16-byte aligned (the dispatcher's scalar fallback)."""
    def body(fp, E):
        from wiw_amd import hip as H

        dt = E.dt
        a, w = E.r(rnd(M, K, seed=1)), E.r(rnd(N, K, seed=2) / math.sqrt(K))
        A = fp.inp("A", a[:, :K - c2], dt, gap=0)
        A2 = fp.inp("A2", a[:, K - c2:], dt, gap=0) if c2 else None
        W = weight(fp, "W", w, dt, tiled)
        b = rnd(N, seed=3) if bias else None
        Bv = fp.inp("bias", b, F32, gap=0, align=vec_align) if bias else None
        rv = rnd(-(-M // rpv), N, seed=4) if rpv else None
        RV = fp.inp("rowvec", rv, F32, gap=4, align=vec_align) if rpv else None
        b1, b2 = (1.0 if alias else 0.7), 0.3
        odt = F32 if out == "f32" else dt

        def residual(kind, seed, name):
            if kind is None:
                return None, None
            r = rnd(M, N, seed=seed) * 3.0 if kind == "f32" else E.r(rnd(M, N, seed=seed))
            return r, fp.inp(name, r, F32 if kind == "f32" else dt, gap=8 if splitk > 1 else None)      # split-K: ld % 8 == 0
        r1, R1 = (None, None)
        if alias:
            r1 = E.r(rnd(M, N, seed=5)) if out == "16" else rnd(M, N, seed=5) * 3.0
            O = R1 = fp.inout("out", r1, odt)
        else:
            r1, R1 = residual(res1, 5, "res1")
            O = fp.out("out", M, N, odt, gap=8 if splitk > 1 else None)
        r2, R2 = residual(res2, 6, "res2")
        epi = act | (H.EPI_OUT_F32 if out == "f32" else 0)
        saved = E.hip._splitk_ws
        if splitk > 1:      # the workspace is an arena too; its sentinel differs between the runs: the result must not depend on it
            ws = fp.out("workspace", 1, splitk * M * N, F32, gap=0)
            E.hip._splitk_ws = ws.window().reshape(-1)
        try:
            E.hip.gemm(A.window(), W, O.window(), M=M, N=N, K=K, C1=K - c2, A2=win(A2), C2=c2, bias=win(Bv), rowvec=win(RV),
                       rowvec_ld=RV.ld if RV else 0, rows_per_vec=rpv or 1, res1=win(R1), ldr1=R1.ld if R1 else 0, beta1=b1,
                       res2=win(R2), ldr2=R2.ld if R2 else 0, beta2=b2, alpha=alpha, ldo=O.ld, epilogue=epi, splitk=splitk)
        finally:
            E.hip._splitk_ws = saved

        def ref():
            y = a @ w.t()
            if bias:
                y = y + b
            if rpv:
                y = y + rv[torch.arange(M) // rpv]
            y = alpha * y
            if act == H.EPI_SILU:
                y = F.silu(y)
            elif act == H.EPI_GELU:
                y = F.gelu(y)
            elif act == H.EPI_QUICK_GELU:
                y = y * torch.sigmoid(1.702 * y)
            if r1 is not None:
                y = y + b1 * r1
            if r2 is not None:
                y = y + b2 * r2
            return y
        if out == "f32":
            kind = "splitk_f32" if splitk > 1 else ("f32res" if (r1 is not None or r2 is not None) else "f32")
        else:
            kind = "gemm2r" if (r1 is not None or r2 is not None or alpha != 1.0) else "k16"
        fp.expect(f"gemm {M}x{N}x{K}", O.window, ref, E.gate(kind))
    return body


def _gemm_cases():
    from_hip = dict(SILU=2, GELU=8, QUICK=16)
    G = "wiw_gemm_bf16"
    # 128x160 tile
    add("gemm-128x160-130x8x64", [G], gemm_dense(130, 8, 64, tiled=False))
    add("gemm-128x160-130x8x64-tiledW", [G], gemm_dense(130, 8, 64))
    add("gemm-128x160-300x200x128-Ntail", [G], gemm_dense(300, 200, 128, rpv=50, res1="16", res2="16", alpha=0.6))
    add("gemm-128x160-300x204x128-tiledW-N%8", [G], gemm_dense(300, 204, 128, bias=True))
    add("gemm-128x160-inplace-res1", [G], gemm_dense(300, 200, 128, alias=True))
    add("gemm-128x160-concatK", [G], gemm_dense(300, 200, 192, c2=64, tiled=False))
    for nm, bit in from_hip.items():
        add(f"gemm-128x160-{nm}", [G], gemm_dense(130, 160, 64, act=bit))
    add("gemm-128x160-out-f32", [G], gemm_dense(130, 8, 64, out="f32"))
    add("gemm-128x160-F32E", [G], gemm_dense(300, 200, 128, out="f32", res1="f32", res2="f32", rpv=50, alpha=0.7))
    add("gemm-128x160-F32E-16out", [G], gemm_dense(300, 200, 128, res1="f32", res2="16", rpv=50, alpha=0.7))
    add("gemm-128x160-F32E-inplace", [G], gemm_dense(300, 200, 128, out="f32", alias=True))
    add("gemm-128x160-vec4-fallback", [G], gemm_dense(300, 200, 128, rpv=50, res1="16", vec_align=4))
    add("gemm-128x160-F32E-vec4-fallback", [G], gemm_dense(300, 200, 128, out="f32", res1="f32", rpv=50, vec_align=4))
    for sk in (2, 3):
        add(f"gemm-splitk{sk}", [G], gemm_dense(300, 200, 384, rpv=50, res1="16", res2="16", alpha=0.75, splitk=sk))
    add("gemm-splitk2-f32", [G], gemm_dense(300, 200, 384, out="f32", res1="f32", splitk=2))
    # 256x160 tile: use_big_tile needs >= 256 tiles; wiw_gemm_huge_ok declines below 200 of its own
    Mb = 32 * 256 + 40
    add("gemm-256x160", [G], gemm_dense(Mb, 1280, 64, rpv=1000, res1="16"))
    add("gemm-256x160-F32E", [G], gemm_dense(Mb, 1280, 64, out="f32", res1="f32", rpv=1000))
    add("gemm-256x160-vec4-fallback", [G], gemm_dense(Mb, 1280, 64, rpv=1000, res1="16", vec_align=4))
    add("gemm-256x160-splitk2", [G], gemm_dense(Mb, 1280, 128, res1="16", splitk=2))
    # 256x320 tile: >= 200 tiles; 204 of 256 slots: fill 0.797 < 0.8 but the 160-wide count (408 of 512) fills no better
    Mh = 50 * 256 + 40
    add("gemm-256x320", [G], gemm_dense(Mh, 1280, 640, rpv=1000, res1="16", res2="16", alpha=0.6))
    add("gemm-256x320-F32E", [G], gemm_dense(Mh, 1280, 640, out="f32", res1="f32", res2="f32", rpv=1000, alpha=0.7))
    add("gemm-256x320-F32E-16out", [G], gemm_dense(Mh, 1280, 640, res1="f32", rpv=1000))
    add("gemm-256x320-N512-partial-tile", [G], gemm_dense(100 * 256 + 40, 512, 640, res1="16"))
    add("gemm-256x320-vec4-fallback", [G], gemm_dense(Mh, 1280, 640, rpv=1000, res1="16", vec_align=4))
    add("gemm-256x320-F32E-vec4-fallback", [G], gemm_dense(Mh, 1280, 640, out="f32", res1="f32", rpv=1000, vec_align=4))


_gemm_cases()


def gemm_geglu(M, Cn, lnfold=False):
    def body(fp, E):
        from wiw_amd import hip as H
        from wiw_amd.unet import pack_geglu

        dt = E.dt
        x = E.r(rnd(M, Cn, seed=1) * 1.2 - 0.3)
        if lnfold:
            x[:, 9] -= 5.0
            x = E.r(x)
        w0, b0 = rnd(8 * Cn, Cn, seed=2) / math.sqrt(Cn), rnd(8 * Cn, seed=3) * 0.2
        gamma, beta = 1 + 0.3 * rnd(Cn, seed=4), 0.2 * rnd(Cn, seed=5)
        if lnfold:
            wp, tp, n_half = pack_geglu(w0 * gamma[None, :], w0 @ beta + b0)
            wp = wp.to(dt)
            st = torch.stack([wp.float().sum(dim=1), tp.float()]).contiguous()
        else:
            wp, bp, n_half = pack_geglu(w0, b0)
            wp = wp.to(dt)
        A = fp.inp("A", x, dt, gap=0)               # rows after M are poison: they must not reach the in-kernel row statistics
        W = weight(fp, "W", wp.float(), dt)
        O = fp.out("out", M, n_half, dt)            # ldo = n_out + 8
        if lnfold:
            ST = fp.inp("lnfold", st, F32, gap=0)
            E.hip.gemm(A.window(), W, O.window(), M=M, N=wp.shape[0], K=Cn, C1=Cn, epilogue=H.EPI_GEGLU, n_out=n_half, ldo=O.ld,
                       lnfold=ST.window(), ln_eps=1e-5)
        else:
            Bv = fp.inp("bias", bp, F32, gap=0)
            E.hip.gemm(A.window(), W, O.window(), M=M, N=wp.shape[0], K=Cn, C1=Cn, bias=Bv.window(), epilogue=H.EPI_GEGLU,
                       n_out=n_half, ldo=O.ld)

        def ref():
            if lnfold:
                y = F.layer_norm(x, (Cn,), gamma, beta, 1e-5) @ w0.t() + b0
            else:
                y = x @ E.r(w0).t() + b0
            return y[:, :n_half] * F.gelu(y[:, n_half:])
        fp.expect(f"gemm GEGLU {M}x{Cn} lnfold={lnfold}", O.window, ref, E.gate("lnfold" if lnfold else "k16"))
    return body


def gemm_lnfold_plain(M, Cn, N):
    def body(fp, E):
        from wiw_amd.unet import fold_layernorm

        dt = E.dt
        x = E.r(rnd(M, Cn, seed=1) * 1.5 + 0.4)
        x[:, 5] += 6.0
        x = E.r(x)
        w, b = rnd(N, Cn, seed=2) / math.sqrt(Cn), rnd(N, seed=3) * 0.2
        gamma, beta = 1 + 0.3 * rnd(Cn, seed=4), 0.2 * rnd(Cn, seed=5)
        r1, rv = E.r(rnd(M, N, seed=6)), rnd(-(-M // 100), N, seed=7)
        wg, st = fold_layernorm(w, b, gamma, beta, dt)
        A = fp.inp("A", x, dt, gap=0)
        W = weight(fp, "W", wg.float(), dt)
        ST, R1, RV = fp.inp("lnfold", st, F32, gap=0), fp.inp("res1", r1, dt), fp.inp("rowvec", rv, F32, gap=4)
        O = fp.out("out", M, N, dt)
        E.hip.gemm(A.window(), W, O.window(), M=M, N=N, K=Cn, C1=Cn, lnfold=ST.window(), ln_eps=1e-5, res1=R1.window(), ldr1=R1.ld,
                   beta1=1.0, rowvec=RV.window(), rowvec_ld=RV.ld, rows_per_vec=100, ldo=O.ld)
        fp.expect(f"LN-fold GEMM {M}x{N}x{Cn}", O.window,
                  lambda: F.layer_norm(x, (Cn,), gamma, beta, 1e-5) @ w.t() + b + r1 + rv[torch.arange(M) // 100], E.gate("lnfold"))
    return body


add("gemm-geglu-128x160", ["wiw_gemm_bf16"], gemm_geglu(137, 64))
add("gemm-geglu-256x160", ["wiw_gemm_bf16"], gemm_geglu(128 * 256 + 40, 64))
add("gemm-lnfold-geglu-128x160", ["wiw_gemm_bf16"], gemm_geglu(137, 64, lnfold=True))
add("gemm-lnfold-geglu-256x160", ["wiw_gemm_bf16"], gemm_geglu(128 * 256 + 40, 64, lnfold=True))
add("gemm-lnfold-plain-128x160", ["wiw_gemm_bf16"], gemm_lnfold_plain(300, 128, 160))
add("gemm-lnfold-plain-256x160", ["wiw_gemm_bf16"], gemm_lnfold_plain(128 * 256 + 40, 64, 320))


# ======================================================================================================================
# wiw_gemm_bf16, convolution modes.  (h, w) = OUTPUT geometry; the frames before frame 0 and after the last are poison
# ======================================================================================================================
def gemm_conv(mode_name, n, c, cout, h, w, *, T=0, c2=0, c3=0, korder=None, tiled=True, extras=False, out="16", splitk=1):
    def body(fp, E):
        from wiw_amd import hip as H
        from wiw_amd.unet import conv_k_cmajor, conv_k_halo32

        dt = E.dt
        mode = getattr(H, "A_" + mode_name)
        hin, win_ = {"CONV3X3_S2": (2 * h, 2 * w), "CONV3X3_S2P": (2 * h, 2 * w), "CONV3X3_UP": (h // 2, w // 2)}.get(mode_name, (h, w))
        x = E.r(rnd(n, c, hin, win_, seed=1))
        b = rnd(cout, seed=6)
        if mode_name == "CONV_T3":
            wt = E.r(rnd(cout, c, 3, 1, 1, seed=4) / math.sqrt(3 * c))
            w_tap, taps = wt[:, :, :, 0, 0].permute(0, 2, 1).reshape(cout, -1), 3
            x5 = x.reshape(n // T, T, c, h, w).permute(0, 2, 1, 3, 4)
            ref0 = lambda: F.conv3d(x5, wt, b, padding=(1, 0, 0)).permute(0, 2, 1, 3, 4).reshape(n, cout, h, w)   # noqa: E731
        else:
            wt = E.r(rnd(cout, c, 3, 3, seed=4) / math.sqrt(9 * c))
            w_tap, taps = wt.permute(0, 2, 3, 1).reshape(cout, -1), 9
            ref0 = {"CONV3X3": lambda: F.conv2d(x, wt, b, padding=1),
                    "CONV3X3_S2": lambda: F.conv2d(x, wt, b, stride=2, padding=1),
                    "CONV3X3_S2P": lambda: F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2),
                    "CONV3X3_UP": lambda: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1)}[mode_name]
        wk = {None: w_tap, "cmajor": conv_k_cmajor(w_tap, taps), "halo": conv_k_halo32(w_tap) if taps == 9 else None}[korder]
        epi = {None: 0, "cmajor": H.K_CMAJOR, "halo": H.K_HALO32}[korder] | (H.EPI_OUT_F32 if out == "f32" else 0)
        M = n * h * w
        frame = hin * win_
        A = fp.inp("A", nhwc(x), dt, gap=0, guard_rows=max(256, 2 * frame))
        kw = {}
        s1 = s2 = wsc = None
        if c2:
            s1 = E.r(rnd(n, c2, h, w, seed=2))
            src = s1
            kw.update(A2=fp.inp("A2", nhwc(s1), dt, gap=0, guard_rows=max(256, 2 * frame)).window(), C2=c2)
            if c3:
                s2 = E.r(rnd(n, c3, h, w, seed=3))
                src = torch.cat([s1, s2], dim=1)
                kw.update(A3=fp.inp("A3", nhwc(s2), dt, gap=0, guard_rows=max(256, 2 * frame)).window(), C3=c3)
            wsc = E.r(rnd(cout, c2 + c3, 1, 1, seed=5) / math.sqrt(c2 + c3))[:, :, 0, 0]
            wk = torch.cat([wk, wsc], 1)
        W = weight(fp, "W", wk, dt, tiled)
        Bv = fp.inp("bias", b, F32, gap=0)
        vec = res = None
        if extras:
            vec = rnd(n, cout, seed=7)
            res = rnd(n, cout, h, w, seed=8) * 3.0 if out == "f32" else E.r(rnd(n, cout, h, w, seed=8))
            RV = fp.inp("rowvec", vec, F32, gap=4)
            R1 = fp.inp("res1", nhwc(res), F32 if out == "f32" else dt)
            kw.update(rowvec=RV.window(), rowvec_ld=RV.ld, rows_per_vec=h * w, res1=R1.window(), ldr1=R1.ld, beta1=1.0, alpha=0.75)
        O = fp.out("out", M, cout, F32 if out == "f32" else dt)
        saved = E.hip._splitk_ws
        if splitk > 1:
            E.hip._splitk_ws = fp.out("workspace", 1, splitk * M * cout, F32, gap=0).window().reshape(-1)
        try:
            E.hip.gemm(A.window(), W, O.window(), M=M, N=cout, K=wk.shape[1], C1=c, mode=mode, H=h, Wd=w, T=T, bias=Bv.window(),
                       ldo=O.ld, epilogue=epi, splitk=splitk, **kw)
        finally:
            E.hip._splitk_ws = saved

        def ref():
            y = ref0()
            if c2:
                y = y + F.conv2d(src, wsc[:, :, None, None])
            if extras:
                y = 0.75 * (y + vec[:, :, None, None]) + res
            return nhwc(y)
        kind = ("f32res" if extras else "f32") if out == "f32" else ("gemm2r" if extras else "k16")
        fp.expect(f"conv {mode_name} {n}x{c}->{cout}@{h}x{w} k={korder}", O.window, ref, E.gate(kind))
    return body


def _conv_cases():
    G = ["wiw_gemm_bf16"]
    add("conv-3x3", G, gemm_conv("CONV3X3", 3, 64, 96, 5, 8, tiled=False))
    add("conv-3x3-tiledW-extras", G, gemm_conv("CONV3X3", 3, 64, 96, 5, 8, extras=True))
    add("conv-3x3-shortcut-A2-A3", G, gemm_conv("CONV3X3", 3, 64, 96, 5, 8, c2=64, c3=128))
    add("conv-3x3-shortcut-F32E", G, gemm_conv("CONV3X3", 3, 64, 64, 5, 8, c2=128, out="f32", extras=True))
    add("conv-3x3-splitk3", G, gemm_conv("CONV3X3", 3, 64, 96, 5, 8, splitk=3, extras=True))
    add("conv-S2", G, gemm_conv("CONV3X3_S2", 3, 64, 64, 5, 8))
    add("conv-S2P", G, gemm_conv("CONV3X3_S2P", 3, 64, 64, 5, 8))
    add("conv-UP", G, gemm_conv("CONV3X3_UP", 3, 64, 64, 6, 8))
    add("conv-T3", G, gemm_conv("CONV_T3", 6, 64, 64, 5, 8, T=3))
    add("conv-T3-F32E", G, gemm_conv("CONV_T3", 6, 64, 64, 5, 8, T=3, out="f32", extras=True))
    add("conv-3x3-K_CMAJOR", G, gemm_conv("CONV3X3", 3, 128, 96, 5, 8, korder="cmajor", c2=64, c3=64))
    add("conv-S2-K_CMAJOR", G, gemm_conv("CONV3X3_S2", 3, 128, 64, 5, 8, korder="cmajor"))
    add("conv-UP-K_CMAJOR", G, gemm_conv("CONV3X3_UP", 3, 128, 64, 6, 8, korder="cmajor"))
    add("conv-T3-K_CMAJOR", G, gemm_conv("CONV_T3", 6, 128, 64, 5, 8, T=3, korder="cmajor"))
    # halo-staged: Wd = 32 (a frame edge inside a tile), 64, 128; rows of test_conv3x3_halo_staged_kernel
    add("conv-K_HALO32-Wd32", G, gemm_conv("CONV3X3", 4, 128, 320, 18, 32, korder="halo", extras=True))
    add("conv-K_HALO32-Wd64", G, gemm_conv("CONV3X3", 2, 64, 320, 4, 64, korder="halo"))
    add("conv-K_HALO32-Wd128", G, gemm_conv("CONV3X3", 3, 192, 320, 2, 128, korder="halo", extras=True))
    add("conv-K_HALO32-Wd32-shortcut-F32E", G, gemm_conv("CONV3X3", 4, 192, 320, 18, 32, korder="halo", c2=128, c3=64, extras=True, out="f32"))
    add("conv-K_HALO32-UP", G, gemm_conv("CONV3X3_UP", 2, 64, 320, 8, 64, korder="halo"))


_conv_cases()


# ======================================================================================================================
# attention
# ======================================================================================================================
PRESCALE = math.log2(math.e) / 8.0


def sdpa(q, k, v, heads, scale=None):
    Bn, S, C = q.shape
    d = C // heads
    q, k, v = (t.reshape(Bn, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax((q @ k.transpose(-1, -2)) * (scale if scale is not None else 1.0 / math.sqrt(d)), dim=-1)
    return (w @ v).transpose(1, 2).reshape(Bn, S, C)


def attn_spatial(entry, frames, S, heads, Sv=None):
    def body(fp, E):
        dt, C = E.dt, heads * 64
        q, k, v = (rnd(frames, S, C, seed=s, scale=sc) for s, sc in ((1, 1.5), (2, 1.5), (3, 1.0)))
        ps = entry != "attn_spatial"
        qs, k, v = E.r(q * PRESCALE if ps else q), E.r(k), E.r(v)
        QK = fp.inp("QK", torch.cat([qs, k], -1).reshape(frames * S, 2 * C), dt)          # rows after frames*S: poison
        if Sv is None:
            vt = v.reshape(frames * S, C).t()
        else:                       # columns S .. Sv-1 of every frame are the caller's zeros (header); after frames*Sv: poison
            vp = torch.zeros(frames, Sv, C)
            vp[:, :S] = v
            vt = vp.reshape(frames * Sv, C).t()
        VT = fp.inp("Vt", vt.contiguous(), dt)                                             # ldvt > frames * S
        O = fp.out("O", frames * S, C, dt, gap=4 if entry == "attn_spatial" else 8)
        if entry == "attn_spatial":
            E.hip.attn_spatial(QK.window(), QK.ld, C, VT.window(), VT.ld, O.window(), O.ld, frames, S, heads, 0.125)
        elif entry == "attn_spatial_ps":
            E.hip.attn_spatial_ps(QK.window(), QK.ld, C, VT.window(), VT.ld, O.window(), O.ld, frames, S, heads)
        else:
            E.hip.attn_spatial_ps_padded(QK.window(), QK.ld, C, VT.window(), VT.ld, O.window(), O.ld, frames, S, Sv, heads)
        fp.expect(f"{entry} frames={frames} S={S} heads={heads}", O.window,
                  lambda: sdpa(qs / PRESCALE if ps else qs, k, v, heads).reshape(frames * S, C), E.gate("attn"))
    return body


for _S in (8, 200):
    add(f"attn_spatial-S{_S}", ["wiw_attn_spatial_bf16"], attn_spatial("attn_spatial", 2, _S, 2))
for _S in (8, 200, 384):        # 8, 200: the fallback kernel; 384: the 32x32x16 kernel
    add(f"attn_spatial_ps-S{_S}", ["wiw_attn_spatial_ps_bf16"], attn_spatial("attn_spatial_ps", 2, _S, 2))
for _S, _Sv in ((49, 56), (196, 200)):
    add(f"attn_spatial_ps_padded-S{_S}", ["wiw_attn_spatial_ps_padded_bf16"], attn_spatial("attn_spatial_ps_padded", 3, _S, 2, Sv=_Sv))


def attn_temporal(entry, B, T, S, heads):
    def body(fp, E):
        dt, C = E.dt, heads * 64
        q, k, v = (E.r(rnd(B, T, S, C, seed=s, scale=1.5)) for s in (1, 2, 3))
        QKV = fp.inp("QKV", torch.cat([q, k, v], -1).reshape(B * T * S, 3 * C), dt)
        O = fp.out("O", B * T * S, C, dt, gap=4, align=8 if entry == "attn_temporal32" else 16)
        getattr(E.hip, entry)(QKV.window(), QKV.ld, O.window(), O.ld, B, T, S, heads, 0.125)

        def perm(t):
            return t.permute(0, 2, 1, 3).reshape(B * S, T, C)
        fp.expect(f"{entry} B={B} T={T} S={S} heads={heads}", O.window,
                  lambda: sdpa(perm(q), perm(k), perm(v), heads).reshape(B, S, T, C).permute(0, 2, 1, 3).reshape(B * T * S, C),
                  E.gate("attn_x8" if entry == "attn_temporal" else "t32"))
    return body


def temporal_block(entry, B, T, S, heads):
    def body(fp, E):
        from wiw_amd.unet import pack_temporal_qkv

        dt, C = E.dt, heads * 64
        x = E.r(rnd(B, T, S, C, seed=1) * 1.5 + 0.3)
        x[..., 5] += 4.0
        x = E.r(x)
        wq, wk, wv = (rnd(C, C, seed=s) / math.sqrt(C) for s in (2, 3, 4))
        gamma, beta = 1 + 0.2 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
        wg, fold = pack_temporal_qkv(wq, wk, wv, gamma, beta, dtype=dt)
        X = fp.inp("X", x.reshape(-1, C), dt, gap=0)
        WG = fp.inp("Wqkv", wg, dt, gap=0)
        FO = fp.inp("fold", fold, F32, gap=0)
        O = fp.out("O", B * T * S, C, dt)
        getattr(E.hip, entry)(X.window(), WG.window(), FO.window(), O.window(), O.ld, B, T, S, heads, 1e-5, 0.125)

        def ref():
            a = F.layer_norm(x, (C,), gamma, beta, 1e-5)
            qq, kk, vv = a @ E.r(wq).t(), a @ E.r(wk).t(), a @ E.r(wv).t()

            def perm(t):
                return t.permute(0, 2, 1, 3).reshape(B * S, T, heads, 64).transpose(1, 2)
            o = F.scaled_dot_product_attention(perm(qq), perm(kk), perm(vv))
            return o.transpose(1, 2).reshape(B, S, T, C).permute(0, 2, 1, 3).reshape(B * T * S, C)
        fp.expect(f"{entry} B={B} T={T} S={S} heads={heads}", O.window, ref, E.gate("tblock" if entry == "temporal_attn_block" else "t32"))
    return body


for _S, _h in ((8, 2), (72, 5)):
    for _T in (1, 3, 14):
        add(f"temporal_attn_block-T{_T}-S{_S}", ["wiw_temporal_attn_block_bf16"], temporal_block("temporal_attn_block", 2, _T, _S, _h))
    add(f"attn_temporal-T16-S{_S}", ["wiw_attn_temporal_bf16"], attn_temporal("attn_temporal", 2, 16, _S, _h))
    for _T in (17, 25, 32):
        add(f"attn_temporal32-T{_T}-S{_S}", ["wiw_attn_temporal32_bf16"], attn_temporal("attn_temporal32", 2, _T, _S, _h))
        add(f"temporal_attn_block32-T{_T}-S{_S}", ["wiw_temporal_attn_block32_bf16"], temporal_block("temporal_attn_block32", 2, _T, _S, _h))


def attn_small(seqs, S, heads, D):
    def body(fp, E):
        dt, C = E.dt, heads * D
        Sp = -(-S // 16) * 16
        q, k, v = (E.r(rnd(seqs, Sp, C, seed=s, scale=1.2)) for s in (1, 2, 3))
        qk = torch.cat([q, k], -1)
        if Sp > S:      # rows S .. Sp-1 of a sequence and the V^T columns S .. Sp-1 are padding the kernel masks: poison
            qk[:, S:] = fp.poison(seqs * (Sp - S) * 2 * C, dt).float().reshape(seqs, Sp - S, 2 * C)
            v[:, S:] = fp.poison(seqs * (Sp - S) * C, dt).float().reshape(seqs, Sp - S, C)
        QK = fp.inp("QK", qk.reshape(seqs * Sp, 2 * C), dt)
        VT = fp.inp("Vt", v.reshape(seqs * Sp, C).t().contiguous(), dt, gap=4)
        O = fp.out("O", seqs * Sp, C, dt, gap=4)
        E.hip.attn_small(QK.window(), QK.ld, C, VT.window(), VT.ld, O.window(), O.ld, seqs, S, Sp, heads, D, D ** -0.5)

        def padding_rows_are_zero():
            o = O.window().reshape(seqs, Sp, C)[:, S:]
            if not bool((o.view(torch.int16) == 0).all()):
                raise FP.FootprintViolation(FP.P2, "attn_small: query rows S .. Sp-1 must be written as zeros")
        fp.finally_check(padding_rows_are_zero)

        def sp(t):
            return t[:, :S].reshape(seqs, S, heads, D).transpose(1, 2)
        fp.expect(f"attn_small seqs={seqs} S={S} heads={heads} d={D}", lambda: O.window().reshape(seqs, Sp, C)[:, :S],
                  lambda: F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(seqs, S, C), E.gate("attn_x8"))
    return body


add("attn_small-S5", ["wiw_attn_small_bf16"], attn_small(2, 5, 2, 80))
add("attn_small-S257", ["wiw_attn_small_bf16"], attn_small(2, 257, 2, 80))


def cross_attn(heads, P, items, rpi):
    def body(fp, E):
        dt, C, rows = E.dt, heads * 64, items * rpi
        q = E.r(rnd(rows, C, seed=1, scale=1.5))
        k, v = E.r(rnd(items, P, C, seed=2, scale=1.2)), E.r(rnd(items, P, C, seed=3))
        Q = fp.inp("Q", q, dt)
        Kk, V = fp.inp("K", k.reshape(items * P, C), dt, gap=0), fp.inp("V", v.reshape(items * P, C), dt, gap=0)
        O = fp.out("O", rows, C, dt)
        E.hip.cross_attn_fewkeys(Q.window(), Q.ld, Kk.window().reshape(items, P, C), V.window().reshape(items, P, C), O.window(), O.ld,
                                 rows, rpi, heads, P, 0.125)

        def ref():
            qh = q.reshape(items, rpi, heads, 64).permute(0, 2, 1, 3)
            kh, vh = (t.reshape(items, P, heads, 64).permute(0, 2, 1, 3) for t in (k, v))
            w = torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, dim=-1)
            return (w @ vh).permute(0, 2, 1, 3).reshape(rows, C)
        fp.expect(f"cross_attn heads={heads} P={P} rows/item={rpi}", O.window, ref, E.gate("cross"))
    return body


for _P in (1, 3, 8):
    add(f"cross_attn_fewkeys-P{_P}", ["wiw_cross_attn_fewkeys_bf16"], cross_attn(5, _P, 2, 37))


# ======================================================================================================================
# fused FeedForward
# ======================================================================================================================
FC, FH = 320, 1280


def ffn(entry, M, rpv, *, ln=False):
    """entry: "bf16" (16-bit residuals / output), "f32stream" (fp32 residuals and output), "f32stream2" (fp32 X through the fused
    LayerNorm + out16), "ffn32" (the 32x32x16 kernel, 16-bit)."""
    def body(fp, E):
        from wiw_amd.hip import FFN_CHUNK
        from wiw_amd.unet import pack_geglu

        dt = E.dt
        ln_ = ln or entry == "f32stream2"
        w0 = rnd(2 * FH, FC, seed=43) / math.sqrt(FC)
        b0 = rnd(2 * FH, seed=44) * 0.3
        w2 = E.r(rnd(FC, FH, seed=45) / math.sqrt(FH))
        b2 = rnd(FC, seed=46) * 0.3
        if ln_:
            gamma, beta = 1.0 + 0.2 * rnd(FC, seed=40), 0.1 * rnd(FC, seed=41)
            w0, b0 = w0 * gamma[None, :], w0 @ beta + b0
        chunk = 32 if entry == "ffn32" else FFN_CHUNK
        w1p, b1p, _ = pack_geglu(w0, b0, chunk)
        if entry == "ffn32":
            b1p = b1p.clone().reshape(-1, 2, 32)
            b1p[:, 0] *= 0.5
            b1p = b1p.reshape(-1)
        W1 = weight(fp, "W1", E.r(w1p), dt, sw16=entry == "ffn32")
        W2 = weight(fp, "W2", w2, dt, sw16=entry == "ffn32")
        B1, B2 = fp.inp("b1", b1p.float(), F32, gap=0), fp.inp("b2", b2, F32, gap=0)
        if ln_:
            x = rnd(M, FC, seed=18) * 3.0 + 1.5 + rnd(M, 1, seed=19) * 4.0
        else:
            x = rnd(M, FC, seed=10)
        xdt = F32 if entry == "f32stream2" else dt
        x = x if xdt == F32 else E.r(x)
        f32res = entry in ("f32stream", "f32stream2")
        r1 = rnd(M, FC, seed=12) * 3.0 if f32res else E.r(rnd(M, FC, seed=12))
        r2 = rnd(M, FC, seed=14) if f32res else E.r(rnd(M, FC, seed=14))
        rv = rnd(-(-M // rpv), FC, seed=13)
        X = fp.inp("X", x, xdt, gap=8)              # ldx % 8 == 0 in elements, fp32 X included
        R1 = fp.inp("res1", r1, F32 if f32res else dt, gap=8)
        R2 = fp.inp("res2", r2, F32 if f32res else dt, gap=8)
        RV = fp.inp("rowvec", rv, F32, gap=4)
        O = fp.out("out", M, FC, F32 if f32res else dt, gap=8)
        O16 = fp.out("out16", M, FC, dt, gap=0) if entry == "f32stream2" else None          # the wrapper fixes ldo16 = 320
        a = 0.3
        kw = dict(ldx=X.ld, rowvec=RV.window(), rowvec_ld=RV.ld, rows_per_vec=rpv, res1=R1.window(), ldr1=R1.ld, beta1=1.0 - a,
                  res2=R2.window(), ldr2=R2.ld, beta2=a, alpha=1.0 - a, ldo=O.ld, ln=ln_)
        if entry == "ffn32":
            E.hip.ffn32_geglu(X.window(), W1, B1.window().reshape(-1), W2, B2.window().reshape(-1), O.window(), M, **kw)
        else:
            E.hip.ffn_geglu(X.window(), W1, B1.window().reshape(-1), W2, B2.window().reshape(-1), O.window(), M, out16=win(O16), **kw)

        def ref():          # tests/test_hip_ffn.py `oracle`
            xf = x.float()
            if ln_:
                xf = E.r(F.layer_norm(xf, (FC,), None, None, 1e-5))
            proj = xf @ E.r(w0).t() + b0
            hidden, gate = proj.chunk(2, dim=-1)
            y = E.r(hidden * F.gelu(gate)) @ w2.t() + b2 + rv[torch.arange(M) // rpv]
            return (1.0 - a) * y + (1.0 - a) * r1 + a * r2
        fp.expect(f"ffn {entry} M={M} rpv={rpv} ln={ln_}", O.window, ref, E.gate("ffn"))
        if O16 is not None:
            fp.expect("ffn out16 = the rounding of out", O16.window, lambda: O.window().to(dt), E.exact)
    return body


for _M, _rpv in ((137, 50), (7, 3)):
    add(f"ffn_geglu_bf16-M{_M}", ["wiw_ffn_geglu_bf16"], ffn("bf16", _M, _rpv))
    add(f"ffn_geglu_bf16-ln-M{_M}", ["wiw_ffn_geglu_bf16"], ffn("bf16", _M, _rpv, ln=True))
    add(f"ffn_geglu_f32stream-M{_M}", ["wiw_ffn_geglu_f32stream"], ffn("f32stream", _M, _rpv))
    add(f"ffn_geglu_f32stream2-M{_M}", ["wiw_ffn_geglu_f32stream2"], ffn("f32stream2", _M, _rpv))
    add(f"ffn32_geglu-M{_M}", ["wiw_ffn32_geglu"], ffn("ffn32", _M, _rpv))
    add(f"ffn32_geglu-ln-M{_M}", ["wiw_ffn32_geglu"], ffn("ffn32", _M, _rpv, ln=True))


# ======================================================================================================================
# GroupNorm family (P5: counters back at zero, scratch / counters sized exactly by the library)
# ======================================================================================================================
def _gn_ref(x, C, rpu, gamma, beta, silu):
    units = x.shape[0] // rpu
    xr = x.reshape(units, rpu, C).permute(0, 2, 1)
    y = F.group_norm(xr, 32, gamma, beta, 1e-5)
    y = F.silu(y) if silu else y
    return y.permute(0, 2, 1).reshape(-1, C)


def groupnorm_two_pass(units, rpu, c1, c2, rpb, f32in=False):
    def body(fp, E):
        dt, C, rows = E.dt, c1 + c2, units * rpu
        xdt = F32 if f32in else dt
        x = rnd(rows, C, seed=3) * 2.0 + rnd(1, C, seed=4) * 5.0
        x = x if f32in else E.r(x)
        gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
        X1 = fp.inp("X1", x[:, :c1], xdt, gap=0)
        X2 = fp.inp("X2", x[:, c1:], xdt, gap=0) if c2 else None
        Gm, Bt = fp.inp("gamma", gamma, F32, gap=0), fp.inp("beta", beta, F32, gap=0)
        ST = fp.out("stats", 1, units * 64, F32, gap=0)
        SC = fp.out("scratch", 1, int(E.lib.wiw_groupnorm_scratch_floats(rows, rpu, rpb)), F32, gap=0, compare=False)
        ncnt = int(E.lib.wiw_groupnorm_counters(rows, rpu, rpb))
        CN = fp.inout("counters", torch.zeros(1, ncnt, dtype=torch.int32), torch.int32, gap=0)     # the caller's zeros (header)
        s, L = E.stream(), E.lib
        fn = L.wiw_groupnorm_stats_f32in if f32in else L.wiw_groupnorm_stats
        E.ck(fn(s, ptr(X1), c1, ptr(X2), c2, rows, rpu, rpb, ptr(ST), ptr(SC), ptr(CN)), "groupnorm_stats")
        O = fp.out("out", rows, C, dt, gap=0)
        if f32in:
            RAW = fp.out("raw16", rows, C, dt, gap=0)
            E.ck(L.wiw_groupnorm_apply_stats_f32in(s, ptr(X1), c1, ptr(X2), c2, rows, rpu, ptr(ST), ptr(Gm), ptr(Bt), 1e-5, 1, ptr(O),
                                                   ptr(RAW)), "groupnorm_apply_stats_f32in")
            fp.expect("groupnorm raw16 = the rounded input", RAW.window, lambda: x.to(dt), E.exact)
        else:
            E.ck(L.wiw_groupnorm_apply_stats(s, ptr(X1), c1, ptr(X2), c2, rows, rpu, ptr(ST), ptr(Gm), ptr(Bt), 1e-5, 1, ptr(O)),
                 "groupnorm_apply_stats")
            AB = fp.out("ab", 1, units * 2 * C, F32, gap=0)
            O2 = fp.out("out_unfused", rows, C, dt, gap=0)
            E.ck(L.wiw_groupnorm_finalize(s, ptr(ST), ptr(Gm), ptr(Bt), units, C, rpu, 1e-5, ptr(AB)), "groupnorm_finalize")
            E.ck(L.wiw_groupnorm_apply(s, ptr(X1), c1, ptr(X2), c2, rows, rpu, ptr(AB), 0, ptr(O2)), "groupnorm_apply")
            fp.expect("groupnorm (finalize + apply)", O2.window, lambda: _gn_ref(x, C, rpu, gamma, beta, False), E.gate("k16"))

            def ab_ref():
                g = x.double().reshape(units, rpu, 32, C // 32).transpose(1, 2).reshape(units, 32, -1)
                m, var = g.mean(-1), g.var(-1, unbiased=False)
                sc = (gamma.double().reshape(1, 32, -1) / torch.sqrt(var + 1e-5)[..., None])
                sh = beta.double().reshape(1, 32, -1) - m[..., None] * sc
                return torch.stack([sc.reshape(units, C), sh.reshape(units, C)], 1).reshape(1, -1).float()
            fp.expect("groupnorm_finalize ab", AB.window, ab_ref, E.gate("gn_ab"))

        def state():
            if int(CN.window().abs().max()) != 0 or not E.hip.gn_counters_clean():
                raise FP.FootprintViolation("P5 library state", "GroupNorm counters are not back at zero")
        fp.finally_check(state)

        def stats_check(got, ref, what):        # test_groupnorm_statistics_in_one_launch: fp64 torch statistics
            st = got.reshape(units, 32, 2).cpu().double()
            g = x.double().reshape(units, rpu, 32, C // 32).transpose(1, 2).reshape(units, 32, -1)
            m, var = g.mean(-1), g.var(-1, unbiased=False)
            em, ev = float((st[..., 0] - m).abs().max() / m.abs().max()), float(((st[..., 1] - var).abs() / var).max())
            print(f"[footprint P4 {E.name}] {what}: mean rel {em:.2e} (gate 2e-6) var rel {ev:.2e} (gate 2e-5)")
            assert em <= 2e-6 and ev <= 2e-5, f"mean {em:.2e} var {ev:.2e}"
        fp.expect(f"groupnorm_stats units={units} rpu={rpu} C={c1}+{c2}", ST.window, lambda: None, stats_check)
        fp.expect(f"groupnorm apply_stats units={units} rpu={rpu} C={c1}+{c2} f32in={f32in}", O.window,
                  lambda: _gn_ref(x, C, rpu, gamma, beta, True), E.gate("k16"))
    return body


_GN = ["wiw_groupnorm_stats", "wiw_groupnorm_apply_stats", "wiw_groupnorm_finalize", "wiw_groupnorm_apply"]
_GNF = ["wiw_groupnorm_stats_f32in", "wiw_groupnorm_apply_stats_f32in"]
add("groupnorm-rpu37", _GN, groupnorm_two_pass(2, 37, 64, 0, 16))
add("groupnorm-rpu37-concat", _GN, groupnorm_two_pass(2, 37, 64, 32, 16))
add("groupnorm-rpu16432", _GN, groupnorm_two_pass(1, 16384 + 48, 64, 0, 16))
add("groupnorm-rpu16432-concat", _GN, groupnorm_two_pass(1, 16384 + 48, 32, 32, 16))
add("groupnorm_f32in-rpu37-raw16", _GNF, groupnorm_two_pass(2, 37, 64, 32, 16, f32in=True))
add("groupnorm_f32in-rpu16432-raw16", _GNF, groupnorm_two_pass(1, 16384 + 48, 64, 0, 16, f32in=True))


def groupnorm_onepass(units, rpu, c1, c2):
    def body(fp, E):
        dt, C, rows = E.dt, c1 + c2, units * rpu
        x = E.r(rnd(rows, C, seed=11) * 2 + rnd(1, C, seed=12) * 3)
        gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
        assert E.lib.wiw_groupnorm_onepass_ok(c1, c2, rows, rpu) == 1
        X1 = fp.inp("X1", x[:, :c1], dt, gap=0, guard_rows=rpu)
        X2 = fp.inp("X2", x[:, c1:], dt, gap=0, guard_rows=rpu) if c2 else None
        Gm, Bt = fp.inp("gamma", gamma, F32, gap=0), fp.inp("beta", beta, F32, gap=0)
        O = fp.out("out", rows, C, dt, gap=0, guard_rows=rpu)
        E.ck(E.lib.wiw_groupnorm_onepass(E.stream(), ptr(X1), c1, ptr(X2), c2, rows, rpu, ptr(Gm), ptr(Bt), 1e-5, 1, ptr(O)),
             "groupnorm_onepass")
        fp.expect(f"groupnorm_onepass rpu={rpu} C={c1}+{c2}", O.window, lambda: _gn_ref(x, C, rpu, gamma, beta, True), E.gate("k16"))
    return body


# (the kernel takes 40 or 80 channels per group only, wiw_groupnorm_onepass_ok: C = 1280 or 2560, C1 / C2 in slabs of 160)
for _rpu in (144, 576):
    add(f"groupnorm_onepass-rpu{_rpu}-1280", ["wiw_groupnorm_onepass"], groupnorm_onepass(2, _rpu, 1280, 0))
    add(f"groupnorm_onepass-rpu{_rpu}-1120+160", ["wiw_groupnorm_onepass"], groupnorm_onepass(2, _rpu, 1120, 160))
add("groupnorm_onepass-rpu144-1280+1280", ["wiw_groupnorm_onepass"], groupnorm_onepass(2, 144, 1280, 1280))


# ======================================================================================================================
# LayerNorm, cast, loop-side kernels, VAE / CLIP operators, transposes
# ======================================================================================================================
def layernorm16(rows, C, addvec):
    def body(fp, E):
        dt = E.dt
        x = E.r(rnd(rows, C, seed=1) * 1.7 + 0.3)
        gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
        X, Gm, Bt = fp.inp("X", x, dt, gap=0), fp.inp("gamma", gamma, F32, gap=0), fp.inp("beta", beta, F32, gap=0)
        O = fp.out("out", rows, C, dt, gap=0)
        if addvec:
            rpv = 10
            av = rnd(-(-rows // rpv), C, seed=4)
            AV, SO = fp.inp("addvec", av, F32, gap=4), fp.out("sum_out", rows, C, dt, gap=0)
            E.hip.layernorm(X.window(), rows, C, Gm.window(), Bt.window(), addvec=AV.window(), addvec_ld=AV.ld, rows_per_vec=rpv,
                            sum_out=SO.window(), out=O.window())
            xs = E.r(x + av.repeat_interleave(rpv, 0)[:rows])
            fp.expect("layernorm sum_out", SO.window, lambda: xs, E.gate("sum_out"))
            fp.expect(f"layernorm+add {rows}x{C}", O.window, lambda: F.layer_norm(xs, (C,), gamma, beta, 1e-5), E.gate("k16"))
        else:
            E.hip.layernorm(X.window(), rows, C, Gm.window(), Bt.window(), out=O.window())
            fp.expect(f"layernorm {rows}x{C}", O.window, lambda: F.layer_norm(x, (C,), gamma, beta, 1e-5), E.gate("k16"))
    return body


def layernorm_f32in(rows, C):
    def body(fp, E):
        x = rnd(rows, C, seed=1) * 1.7 + 0.3
        gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
        X, Gm, Bt = fp.inp("X", x, F32, gap=0), fp.inp("gamma", gamma, F32, gap=0), fp.inp("beta", beta, F32, gap=0)
        O = fp.out("out", rows, C, E.dt, gap=0)
        E.hip.layernorm(X.window(), rows, C, Gm.window(), Bt.window(), out=O.window())
        fp.expect(f"layernorm_f32in {rows}x{C}", O.window, lambda: F.layer_norm(x, (C,), gamma, beta, 1e-5), E.gate("k16"))
    return body


def cast16(fp, E):
    x = rnd(37, 8, seed=1) * 3.0
    X, O = fp.inp("X", x, F32, gap=0), fp.out("out", 37, 8, E.dt, gap=0)
    E.hip.cast16(X.window(), out=O.window())
    fp.expect("cast_f32_to_16", O.window, lambda: x.to(E.dt), E.exact)


for _r, _c in ((37, 64), (100, 320), (9, 2048)):
    add(f"layernorm-{_r}x{_c}", ["wiw_layernorm_bf16"], layernorm16(_r, _c, False))
    add(f"layernorm-addvec-{_r}x{_c}", ["wiw_layernorm_bf16"], layernorm16(_r, _c, True))
    add(f"layernorm_f32in-{_r}x{_c}", ["wiw_layernorm_f32in"], layernorm_f32in(_r, _c))
add("cast_f32_to_16", ["wiw_cast_f32_to_16"], cast16)


def emb_combine(fp, E):
    Bc, B, T, Em = 4, 2, 3, 264
    t, a, n = rnd(Bc, Em, seed=1), rnd(B * T, Em, seed=2), rnd(Bc, Em, seed=3)
    # element-wise accesses: the natural alignment of the element types is all the header asks
    Tm, A, N = (fp.inp(nm, v, F32, gap=0, align=4) for nm, v in (("time", t), ("act", a), ("noise", n)))
    O = fp.out("out", Bc * T, Em, E.dt, gap=0, align=2)
    E.hip.emb_combine(Tm.window(), A.window(), N.window(), Bc, B, T, Em, O.window())
    fp.expect("emb_combine", O.window, lambda: F.silu(t.repeat_interleave(T, 0) + a.reshape(B, T, Em).repeat(Bc // B, 1, 1).reshape(Bc * T, Em)
                                                      + n.repeat_interleave(T, 0)), E.gate("k16"))


def prep_unet_input(fp, E):
    B, T, h, w, Cpad = 2, 3, 3, 5, 64
    lat, img, sigma = rnd(B, T, 4, h, w, seed=1) * 30, rnd(B, 4, h, w, seed=2), 26.7572
    Lt, Im = fp.inp("latents", lat, F32, gap=0, align=4), fp.inp("image_latents", img, F32, gap=0, align=4)
    X = fp.out("X", 2 * B * T * h * w, Cpad, E.dt, gap=0)
    E.hip.prep_unet_input(Lt.window(), Im.window(), B, T, h * w, sigma, Cpad, X.window())

    def pad_is_zero():
        if not bool((X.window()[:, 8:].view(torch.int16) == 0).all()):
            raise FP.FootprintViolation(FP.P2, "prep_unet_input: the channel padding 8 .. Cpad-1 must be written as zeros")
    fp.finally_check(pad_is_zero)

    def ref():
        inp = torch.cat([lat, lat]) / (sigma ** 2 + 1) ** 0.5
        il = torch.cat([torch.zeros_like(img), img])[:, None].repeat(1, T, 1, 1, 1)
        return E.r(torch.cat([inp, il], 2).permute(0, 1, 3, 4, 2).reshape(-1, 8))
    fp.expect("prep_unet_input", lambda: X.window()[:, :8], ref, E.gate("prep"))


def cfg_euler_step(fp, E):
    import svd_oracle as O

    B, T, h, w = 2, 3, 3, 5
    lat = rnd(B, T, 4, h, w, seed=1) * 30
    vu, vc = rnd(B * T * h * w, 4, seed=5), rnd(B * T * h * w, 4, seed=6)
    V = fp.inp("V", torch.cat([vu, vc]), F32, gap=4, align=4)      # ldv = 8: channels 4 .. 7 are poison
    L = fp.inout("latents", lat, F32, gap=0, align=4)                        # updated in place (documented)
    E.hip.cfg_euler_step(V.window(), V.ld, L.window(), B, T, h * w, 2.5, 1.25, 1.0, 3.0)

    def ref():
        gs = torch.linspace(1.0, 3.0, T).reshape(1, T, 1, 1, 1)
        to5 = lambda t: t.reshape(B, T, h, w, 4).permute(0, 1, 4, 2, 3)  # noqa: E731
        return O.euler_step(to5(vu) + gs * (to5(vc) - to5(vu)), lat, 2.5, 1.25).reshape(1, -1)
    fp.expect("cfg + euler", L.window, ref, E.gate("euler"))


def softmax_rows(rows, cols):
    def body(fp, E):
        x = rnd(rows, cols, seed=1) * 4.0
        x[0, 3] = 30.0
        X, P = fp.inp("X", x, F32, gap=4), fp.out("P", rows, cols, E.dt, gap=4, align=8)
        E.hip.softmax_rows(X.window(), X.ld, rows, cols, P.window(), P.ld)
        fp.expect(f"softmax_rows {rows}x{cols}", P.window, lambda: torch.softmax(x, dim=-1), E.gate("softmax"))
    return body


def vae_time_conv_out(fp, E):
    B, T, h, w = 2, 3, 5, 7
    y = rnd(B * T, 3, h, w, seed=2)
    wt, b = rnd(3, 3, 3, 1, 1, seed=3) / 3.0, rnd(3, seed=4)
    Y = fp.inp("Y", y.permute(0, 2, 3, 1).reshape(-1, 3), F32, gap=1)               # ldy = 4: column 3 is poison
    Wt, Bv = fp.inp("weight", wt[:, :, :, 0, 0].reshape(1, -1), F32, gap=0), fp.inp("bias", b, F32, gap=0)
    O = fp.out("out", 1, B * T * 3 * h * w, F32, gap=0)
    E.hip.vae_time_conv_out(Y.window(), Y.ld, Wt.window(), Bv.window(), B * T, T, h * w, O.window())
    fp.expect("vae_time_conv_out", O.window, lambda: F.conv3d(y.reshape(B, T, 3, h, w).permute(0, 2, 1, 3, 4), wt, b, padding=(1, 0, 0))
              .permute(0, 2, 1, 3, 4).reshape(1, -1), E.gate("tconv"))


def nchw_to_nhwc(fp, E):
    x = rnd(3, 4, 6, 10, seed=5)
    X, O = fp.inp("X", x, F32, gap=0), fp.out("out", 3 * 60, 64, E.dt, gap=0)
    E.hip.nchw_to_nhwc(X.window(), 3, 4, 60, 0.5, 64, O.window())

    def ref():          # the channel padding 4 .. 63 is written as zeros (header)
        r = torch.zeros(3 * 60, 64)
        r[:, :4] = (0.5 * x).permute(0, 2, 3, 1).reshape(-1, 4)
        return r.to(E.dt)
    fp.expect("nchw_f32_to_nhwc", O.window, ref, E.exact)


def clip_preprocess(fp, E):
    from wiw_amd import frontend as FE
    from wiw_amd.clip import gaussian_taps

    B, H0, W0, P = 1, 96, 200, 32
    x = torch.rand(B, 3, H0, W0, generator=torch.Generator().manual_seed(1)) * 2 - 1
    grid = 224 // P
    Sp, Kp = -(-(1 + grid * grid) // 16) * 16, -(-(3 * P * P) // 64) * 64 + 64
    IM = fp.inp("img", x, F32, gap=0)
    TMP = fp.out("tmp", 1, B * 3 * H0 * 224, F32, gap=0, compare=False)
    A = fp.inout("A", torch.zeros(B * Sp, Kp), E.dt, gap=0)             # the caller zeroes the buffer once (header)
    E.hip.clip_preprocess(IM.window(), B, H0, W0, 224, P, gaussian_taps(W0, 224), gaussian_taps(H0, 224), FE.CLIP_MEAN,
                          [1.0 / s for s in FE.CLIP_STD], TMP.window(), A.window(), Sp, Kp)

    def untouched():        # class-token row 0, the padding rows and the padding columns are left untouched
        for b in range(B):
            A.untouched_in_window(rows=slice(b * Sp, b * Sp + 1))
            A.untouched_in_window(rows=slice(b * Sp + 1 + grid * grid, (b + 1) * Sp))
        A.untouched_in_window(cols=slice(3 * P * P, Kp))
    fp.finally_check(untouched)
    fp.expect("clip_preprocess", lambda: A.window().reshape(B, Sp, Kp)[:, 1:1 + grid * grid, :3 * P * P],
              lambda: F.unfold(FE.clip_preprocess(x), kernel_size=P, stride=P).transpose(1, 2), E.gate("k16"))


def transpose(rows, C, c0, extra):
    def body(fp, E):
        x = E.r(rnd(rows, c0 + C + extra, seed=rows + C))
        X, Y = fp.inp("X", x, E.dt), fp.out("Y", C, rows, E.dt)
        E.hip.transpose(X.window(), X.ld, c0, rows, C, Y.window(), Y.ld)
        fp.expect(f"transpose {rows}x{C}", Y.window, lambda: x[:, c0:c0 + C].t().to(E.dt), E.exact)
    return body


def transpose_framepad(frames, S, Sv, C, c0):
    def body(fp, E):
        x = E.r(rnd(frames * S, c0 + C, seed=S + C))
        X, Y = fp.inp("X", x, E.dt), fp.out("Y", C, frames * Sv, E.dt)

        E.hip.transpose_framepad(X.window(), X.ld, c0, frames, S, Sv, C, Y.window(), Y.ld)

        def ref():          # columns S .. Sv-1 of every frame are written as zeros (header)
            r = torch.zeros(frames, Sv, C)
            r[:, :S] = x[:, c0:].reshape(frames, S, C)
            return r.reshape(frames * Sv, C).t().to(E.dt)
        fp.expect(f"transpose_framepad S={S} Sv={Sv}", Y.window, ref, E.exact)
    return body


add("emb_combine", ["wiw_emb_combine"], emb_combine)
add("prep_unet_input", ["wiw_prep_unet_input"], prep_unet_input)
add("cfg_euler_step-inplace", ["wiw_cfg_euler_step"], cfg_euler_step)
add("softmax_rows-7x64", ["wiw_softmax_rows_f32_bf16"], softmax_rows(7, 64))
add("softmax_rows-4x1028", ["wiw_softmax_rows_f32_bf16"], softmax_rows(4, 1028))
add("vae_time_conv_out", ["wiw_vae_time_conv_out"], vae_time_conv_out)
add("nchw_f32_to_nhwc", ["wiw_nchw_f32_to_nhwc_bf16"], nchw_to_nhwc)
add("clip_preprocess", ["wiw_clip_preprocess"], clip_preprocess)
add("transpose-200x72", ["wiw_transpose_bf16"], transpose(200, 72, 8, 16))
add("transpose-8x8", ["wiw_transpose_bf16"], transpose(8, 8, 0, 0))
add("transpose_framepad-S49", ["wiw_transpose_framepad_bf16"], transpose_framepad(3, 49, 56, 72, 8))
add("transpose_framepad-S196", ["wiw_transpose_framepad_bf16"], transpose_framepad(2, 196, 200, 64, 0))


# ======================================================================================================================
# training entries (csrc/train.hip): P4 = a dense-layout launch of the same kernel on the same values, bit for bit
# ======================================================================================================================
class _Dense:
    def __init__(self, t):
        self.t, self.ld = t, t.shape[1]

    def window(self):
        return self.t


class DenseMem:
    """The plain layout: every operand dense at the start of its own allocation (the interface of footprint.Footprint)."""
    fill = "zero"

    def inp(self, name, data, dtype=None, **kw):
        data = data if data.dim() == 2 else data.reshape(1, -1)
        return _Dense(data.to(dtype or data.dtype).to(DEV).contiguous())

    inout = inp

    def out(self, name, rows, cols, dtype, **kw):
        return _Dense(torch.zeros(rows, cols, dtype=dtype, device=DEV))

    def poison(self, n, dtype):
        return torch.zeros(n, dtype=dtype)


def train(run, check=None):
    """run(mem, E) -> {name: operand} launches the entry with operands from `mem` (arenas, or the dense layout)."""
    def body(fp, E):
        outs = run(fp, E)
        cache = {}

        def dense(name):
            if not cache:
                cache.update(run(DenseMem(), E))
                torch.cuda.synchronize()
            return cache[name].window()
        for name, a in outs.items():
            fp.expect(f"{name} vs the dense-layout launch", a.window, lambda name=name: dense(name), check or E.exact)
    return body


def t_adamw(scaled):
    def run(m, E):
        n = 1001
        p, g, mm, v = (rnd(n, seed=s) for s in (1, 2, 3, 4))
        P, Mm, V = m.inout("p", p, F32, gap=0), m.inout("m", mm * 0.1, F32, gap=0), m.inout("v", v.abs() * 0.01, F32, gap=0)
        G = m.inp("g", g, F32, gap=0)
        P16 = m.out("p16", 1, n, E.dt, gap=0, align=8)
        if scaled:
            GS = m.inp("gscale", torch.tensor([0.37]), F32, gap=0, align=4)
            E.ck(E.lib.wiw_adamw_step_scaled(E.stream(), ptr(P), ptr(G), ptr(Mm), ptr(V), ptr(P16), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3,
                                             ptr(GS)), "adamw_step_scaled")
        else:
            E.ck(E.lib.wiw_adamw_step(E.stream(), ptr(P), ptr(G), ptr(Mm), ptr(V), ptr(P16), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3), "adamw_step")
        return dict(p=P, m=Mm, v=V, p16=P16)
    return train(run)


def t_edm(m, E):
    n, nb = 1001, 4
    Pr, No, Tg = (m.inp(nm, rnd(n, seed=s), F32, gap=0) for nm, s in (("pred", 1), ("noisy", 2), ("target", 3)))
    G, Pa = m.out("grad", 1, n, F32, gap=0), m.out("partial", 1, nb, F32, gap=0)
    E.ck(E.lib.wiw_edm_loss_grad(E.stream(), ptr(Pr), ptr(No), ptr(Tg), n, 1.7, ptr(G), ptr(Pa), nb), "edm_loss_grad")
    return dict(grad=G, partial=Pa)


def t_ema(m, E):
    n = 1001
    Sh, Pa = m.inout("shadow", rnd(n, seed=1), F32, gap=0), m.inp("param", rnd(n, seed=2), F32, gap=0)
    E.ck(E.lib.wiw_ema_step_f32(E.stream(), ptr(Sh), ptr(Pa), n, 0.01), "ema_step")
    return dict(shadow=Sh)


def t_sumsq(m, E):
    L = int(E.lib.wiw_grad_sumsq_chunk())
    sizes = (1001, L + 5, 3)
    ts = [m.inp(f"t{i}", rnd(n, seed=i + 1), F32, gap=0, align=4) for i, n in enumerate(sizes)]      # 4-byte alignment only (header)
    rows, first = [], 0
    for t, n in zip(ts, sizes):
        rows.append([t.window().data_ptr(), n, first])
        first += -(-n // L)
    TB = m.inp("table", torch.tensor(rows, dtype=torch.int64), torch.int64, gap=0, align=8)
    Pa = m.out("partial", 1, first, F32, gap=0, align=4)
    E.ck(E.lib.wiw_grad_sumsq_partials(E.stream(), ptr(TB), len(sizes), first, ptr(Pa), 0), "grad_sumsq_partials")
    OUT = m.out("record", 1, 4, F32, gap=0, align=4)
    E.ck(E.lib.wiw_grad_norm_finalize(E.stream(), ptr(Pa), first, 1.0, ptr(OUT)), "grad_norm_finalize")
    return dict(partial=Pa, record=OUT)


def _sumsq_check(E):
    def check(got, ref, what):
        # which elements ride the 16-byte body depends on the address (header): the two layouts differ by summation order,
        # each within (log2 L + 2) 2^-24 of the exact sum
        L = int(E.lib.wiw_grad_sumsq_chunk())
        tol = 2 * (math.log2(L) + 2) * 2.0 ** -24
        got, ref = got.cpu().double(), ref.cpu().double()
        err = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
        print(f"[footprint P4 {E.name}] {what}: max rel {err:.2e} (bound {tol:.2e})")
        assert err <= tol
    return check


def t_colsum(is_f32):
    def run(m, E):
        rows, C, parts = 101, 72, 3
        x = rnd(rows, C, seed=5)
        X = m.inp("X", x if is_f32 else E.r(x), F32 if is_f32 else E.dt, gap=0)
        O = m.out("out", parts, C, F32, gap=0)
        E.ck(E.lib.wiw_colsum(E.stream(), ptr(X), int(is_f32), rows, C, parts, ptr(O)), "colsum")
        return dict(out=O)
    return train(run)


def t_layernorm_bwd(m, E):
    rows, C = 37, 320
    X, dY = m.inp("X", E.r(rnd(rows, C, seed=1) * 1.5 + 0.3), E.dt, gap=0), m.inp("dY", E.r(rnd(rows, C, seed=2)), E.dt, gap=0)
    dR = m.inp("dRes", E.r(rnd(rows, C, seed=3)), E.dt, gap=0)
    Gm = m.inp("gamma", 1 + 0.1 * rnd(C, seed=4), F32, gap=0)
    nw = int(E.lib.wiw_layernorm_bwd_partials(rows))
    dX, Pa = m.out("dX", rows, C, E.dt, gap=0), m.out("partial", nw, 2 * C, F32, gap=0)
    E.ck(E.lib.wiw_layernorm_bwd(E.stream(), ptr(X), ptr(dY), ptr(Gm), rows, C, 1e-5, ptr(dR), ptr(dX), ptr(Pa)), "layernorm_bwd")
    return dict(dX=dX, partial=Pa)


def t_groupnorm_bwd(m, E):
    units, rpu, C, rpb = 2, 74, 64, 64
    rows, splits = units * rpu, -(-rpu // rpb)
    x = E.r(rnd(rows, C, seed=1) * 2 + 0.5)
    g = x.double().reshape(units, rpu, 32, C // 32).transpose(1, 2).reshape(units, 32, -1)
    stats = torch.stack([g.mean(-1), g.var(-1, unbiased=False)], -1).float().reshape(1, -1)
    X, dY = m.inp("X", x, E.dt, gap=0), m.inp("dY", E.r(rnd(rows, C, seed=2)), E.dt, gap=0)
    ST, Gm, Bt = m.inp("stats", stats, F32, gap=0), m.inp("gamma", 1 + 0.1 * rnd(C, seed=3), F32, gap=0), m.inp("beta", 0.1 * rnd(C, seed=4), F32, gap=0)
    dX, UC = m.out("dX", rows, C, E.dt, gap=0), m.out("unit_cs", units, 2 * C, F32, gap=0)
    AB, Pa = m.out("AB", 1, units * 64, F32, gap=0), m.out("partial", 1, units * splits * 2 * C, F32, gap=0)
    E.ck(E.lib.wiw_groupnorm_bwd(E.stream(), ptr(X), ptr(dY), ptr(ST), ptr(Gm), ptr(Bt), rows, C, rpu, 1e-5, 1, ptr(dX), ptr(UC), ptr(AB),
                                 ptr(Pa), rpb), "groupnorm_bwd")
    return dict(dX=dX, unit_cs=UC, AB=AB, partial=Pa)


def t_geglu(bwd):
    def run(m, E):
        rows, Ch = 37, 72
        P = m.inp("P", E.r(rnd(rows, 2 * Ch, seed=1)), E.dt, gap=0)
        if bwd:
            dH, dP = m.inp("dH", E.r(rnd(rows, Ch, seed=2)), E.dt, gap=0), m.out("dP", rows, 2 * Ch, E.dt, gap=0)
            E.ck(E.lib.wiw_geglu_bwd(E.stream(), ptr(P), ptr(dH), rows, Ch, ptr(dP)), "geglu_bwd")
            return dict(dP=dP)
        Hh = m.out("H", rows, Ch, E.dt, gap=0)
        E.ck(E.lib.wiw_geglu_fwd(E.stream(), ptr(P), rows, Ch, ptr(Hh)), "geglu_fwd")
        return dict(H=Hh)
    return train(run)


def t_attn_bwd(seqs, S, Sp, heads, given_lse=False):
    def run(m, E):
        dt, C, M = E.dt, heads * 64, seqs * Sp
        qkv = E.r(rnd(M, 3 * C, seed=1))
        o, do = E.r(rnd(M, C, seed=2)), E.r(rnd(M, C, seed=3))
        QKV, O, dO = m.inp("QKV", qkv, dt), m.inp("O", o, dt), m.inp("dO", do, dt)
        dQ = m.out("dQKV", M, 3 * C, dt, gap=4)
        DS = m.out("dsum", 1, seqs * heads * Sp, F32, gap=0)
        s = E.stream()
        if given_lse:
            q, k = qkv[:, :C].reshape(seqs, S, heads, 64).transpose(1, 2), qkv[:, C:2 * C].reshape(seqs, S, heads, 64).transpose(1, 2)
            lse = torch.logsumexp(q @ k.transpose(-1, -2) * 0.125, dim=-1) / math.log(2.0)             # [seqs][heads][S], log2 domain
            LS = m.inp("lse", lse.reshape(1, -1), F32, gap=0)
            E.ck(E.lib.wiw_attn_bwd_given_lse_bf16(s, ptr(QKV), QKV.ld, C, 2 * C, ptr(O), ptr(dO), O.ld, ptr(dQ), dQ.ld, ptr(LS), ptr(DS),
                                                   seqs, S, heads, 64, 0.125), "attn_bwd_given_lse")
            return dict(dQKV=dQ, dsum=DS)
        LS = m.out("lse", 1, seqs * heads * Sp, F32, gap=0)
        tiled = S == Sp and S % 32 == 0 and S >= 128
        Qt = Kt = dOt = None
        ldt = M
        if not tiled:
            Qt, Kt, dOt = (m.inp(nm, t.t().contiguous(), dt, gap=4) for nm, t in (("Qt", qkv[:, :C]), ("Kt", qkv[:, C:2 * C]), ("dOt", do)))
            ldt = Qt.ld
        assert O.ld == dO.ld
        E.ck(E.lib.wiw_attn_bwd_bf16(s, ptr(QKV), QKV.ld, C, 2 * C, ptr(Qt), ptr(Kt), ptr(dOt), ldt, ptr(O), ptr(dO), O.ld, ptr(dQ), dQ.ld,
                                     ptr(LS), ptr(DS), seqs, S, Sp, heads, 64, 0.125), "attn_bwd")
        return dict(dQKV=dQ, lse=LS, dsum=DS)
    return train(run)


def t_attn_lse(m, E):
    frames, S, heads = 2, 160, 2
    dt, C = E.dt, heads * 64
    q, k, v = (E.r(rnd(frames * S, C, seed=s)) for s in (1, 2, 3))
    QK, VT = m.inp("QK", torch.cat([q, k], -1), dt), m.inp("Vt", v.t().contiguous(), dt)
    O, LS = m.out("O", frames * S, C, dt, gap=4), m.out("lse", 1, frames * heads * S, F32, gap=0)
    E.hip.attn_spatial(QK.window(), QK.ld, C, VT.window(), VT.ld, O.window(), O.ld, frames, S, heads, 0.125, lse=LS.window())
    return dict(O=O, lse=LS)


def t_gather(transposed, n, C, h, w, T, temporal, stride):
    def run(m, E):
        M = n * h * w
        rows_in, taps = M * (4 if stride == 2 else 1), (3 if temporal else 9)
        X = m.inp("X", E.r(rnd(rows_in, C, seed=M)), E.dt, gap=0, guard_rows=max(256, 2 * rows_in // n))
        if transposed:
            Mp = -(-M // 8) * 8 + 8         # zero columns M .. Mp-1 are part of the declared window (header)
            Y = m.out("XcolT", taps * C, Mp, E.dt, gap=0)
            E.ck(E.lib.wiw_gather_taps_t_bf16(E.stream(), ptr(X), M, Mp, C, h, w, T, int(temporal), stride, ptr(Y)), "gather_taps_t")
            if isinstance(m, FP.Footprint):
                def zero_columns():
                    if not bool((Y.window()[:, M:].view(torch.int16) == 0).all()):
                        raise FP.FootprintViolation(FP.P2, "gather_taps_t: columns M .. Mp-1 must be written as zeros")
                m.finally_check(zero_columns)
            return dict(XcolT=Y)
        Y = m.out("Xcol", M, taps * C, E.dt, gap=0)
        E.ck(E.lib.wiw_gather_taps_bf16(E.stream(), ptr(X), M, C, h, w, T, int(temporal), stride, ptr(Y)), "gather_taps")
        return dict(Xcol=Y)
    return train(run)


def t_wgrad(m, E):
    M, N, K, splits = 100, 40, 72, 2
    dY, X = m.inp("dY", E.r(rnd(M, N, seed=1)), E.dt), m.inp("X", E.r(rnd(M, K, seed=2)), E.dt)      # rows after M: poison
    SL = m.out("slabs", splits, N * K, F32, gap=0)
    E.ck(E.lib.wiw_wgrad_tn_bf16(E.stream(), ptr(dY), dY.ld, ptr(X), X.ld, M, N, K, splits, ptr(SL)), "wgrad_tn")
    return dict(slabs=SL)


def t_axpby(m, E):
    n = 8 * 131
    X, Y, O = m.inp("X", E.r(rnd(n, seed=1)), E.dt, gap=0), m.inp("Y", E.r(rnd(n, seed=2)), E.dt, gap=0), m.out("out", 1, n, E.dt, gap=0)
    E.ck(E.lib.wiw_axpby_bf16(E.stream(), ptr(X), ptr(Y), 0.7, -0.3, n, ptr(O)), "axpby")
    return dict(out=O)


def t_silu(bwd):
    def run(m, E):
        n = 8 * 131
        X, O = m.inp("X", E.r(rnd(n, seed=1)), E.dt, gap=0), m.out("out", 1, n, E.dt, gap=0)
        dY = m.inp("dY", E.r(rnd(n, seed=2)), E.dt, gap=0) if bwd else None
        E.ck(E.lib.wiw_silu_bf16(E.stream(), ptr(X), ptr(dY), int(bwd), n, ptr(O)), "silu")
        return dict(out=O)
    return train(run)


def t_dot(m, E):
    n, nb = 8 * 1001, 4
    X, Y, Z = (m.inp(nm, E.r(rnd(n, seed=s)), E.dt, gap=0) for nm, s in (("X", 1), ("Y", 2), ("Z", 3)))
    Pa = m.out("partial", 1, nb, F32, gap=0)
    E.ck(E.lib.wiw_dot_bf16(E.stream(), ptr(X), ptr(Y), ptr(Z), n, ptr(Pa), nb), "dot")
    return dict(partial=Pa)


def t_row_map(mode):
    def run(m, E):
        n, H, W, C, B, T, Tp, S = 2, 3, 5, 72, 2, 3, 4, 5
        if mode in (0, 1):
            rows_in, out_rows, kw = n * H * W, n * 4 * H * W, (H, W, 0, 0, 0)
        elif mode == 2:
            rows_in, out_rows, kw = n * 4 * H * W, n * H * W, (H, W, 0, 0, 0)
        elif mode == 3:
            rows_in, out_rows, kw = B * T * S, B * S * Tp, (0, 0, T, Tp, S)
        else:
            rows_in, out_rows, kw = B * S * Tp, B * T * S, (0, 0, T, Tp, S)
        X, O = m.inp("X", E.r(rnd(rows_in, C, seed=mode + 1)), E.dt, gap=0), m.out("out", out_rows, C, E.dt, gap=0)
        E.ck(E.lib.wiw_row_map_bf16(E.stream(), ptr(X), mode, out_rows, C, *kw, ptr(O)), "row_map")
        return dict(out=O)
    return train(run)


def fill_f32(fp, E):
    O = fp.out("p", 1, 1001, F32, gap=0, align=4)
    E.ck(E.lib.wiw_fill_f32(E.stream(), ptr(O), 1001, 1.25), "fill_f32")
    fp.expect("fill_f32", O.window, lambda: torch.full((1, 1001), 1.25), E.exact)


add("adamw_step", ["wiw_adamw_step"], t_adamw(False))
add("adamw_step_scaled", ["wiw_adamw_step_scaled"], t_adamw(True))
add("edm_loss_grad", ["wiw_edm_loss_grad"], train(t_edm))
add("ema_step", ["wiw_ema_step_f32"], train(t_ema))
add("colsum-16", ["wiw_colsum"], t_colsum(False))
add("colsum-f32", ["wiw_colsum"], t_colsum(True))
add("layernorm_bwd", ["wiw_layernorm_bwd"], train(t_layernorm_bwd))
add("groupnorm_bwd", ["wiw_groupnorm_bwd"], train(t_groupnorm_bwd))
add("geglu_bwd", ["wiw_geglu_bwd"], t_geglu(True))
add("geglu_fwd", ["wiw_geglu_fwd"], t_geglu(False))
add("attn_bwd-tiled-S160", ["wiw_attn_bwd_bf16"], t_attn_bwd(2, 160, 160, 2))
add("attn_bwd-temporal-S14", ["wiw_attn_bwd_bf16"], t_attn_bwd(5, 14, 16, 2))
add("attn_bwd_given_lse-S160", ["wiw_attn_bwd_given_lse_bf16"], t_attn_bwd(2, 160, 160, 2, given_lse=True))
add("attn_spatial_lse-S160", ["wiw_attn_spatial_lse_bf16"], train(t_attn_lse))
add("gather_taps-3x3", ["wiw_gather_taps_bf16"], t_gather(False, 3, 72, 5, 7, 1, False, 1))
add("gather_taps-stride2", ["wiw_gather_taps_bf16"], t_gather(False, 3, 72, 5, 7, 1, False, 2))
add("gather_taps-temporal", ["wiw_gather_taps_bf16"], t_gather(False, 6, 72, 4, 6, 3, True, 1))
add("gather_taps_t-3x3", ["wiw_gather_taps_t_bf16"], t_gather(True, 3, 72, 5, 7, 1, False, 1))
add("gather_taps_t-stride2", ["wiw_gather_taps_t_bf16"], t_gather(True, 3, 72, 5, 7, 1, False, 2))
add("gather_taps_t-temporal", ["wiw_gather_taps_t_bf16"], t_gather(True, 6, 72, 4, 6, 3, True, 1))
add("wgrad_tn", ["wiw_wgrad_tn_bf16"], train(t_wgrad))
add("axpby", ["wiw_axpby_bf16"], train(t_axpby))
add("silu-fwd", ["wiw_silu_bf16"], t_silu(False))
add("silu-bwd", ["wiw_silu_bf16"], t_silu(True))
add("dot", ["wiw_dot_bf16"], train(t_dot))
for _mode in range(5):
    add(f"row_map-mode{_mode}", ["wiw_row_map_bf16"], t_row_map(_mode))
add("fill_f32", ["wiw_fill_f32"], fill_f32)


def _sumsq_body(fp, E):
    train(t_sumsq, check=_sumsq_check(E))(fp, E)


add("grad_sumsq", ["wiw_grad_sumsq_partials", "wiw_grad_norm_finalize"], _sumsq_body)

# ----------------------------------------------------------------------------------------------------------------------
# Coverage: every `wiw_*(` declaration of include/wiw_svd.h that returns int is in the table above or excluded here
# (tests/test_footprint_harness.py checks it without a GPU).
# ----------------------------------------------------------------------------------------------------------------------
EXCLUDED = {
    "wiw_abi_version": "no launch: a constant",
    "wiw_dtype": "no launch: a constant",
    "wiw_device_check": "no launch: device properties",
    "wiw_conv_halo_ok": "no launch: a geometry query",
    "wiw_groupnorm_onepass_ok": "no launch: a geometry query",
    "wiw_grad_sumsq_chunk": "no launch: a size query",
    "wiw_calib_mfma": "measurement loop of bench.py: register operands, writes 4 floats",
    "wiw_calib_mfma_random": "measurement loop of bench.py",
}
COVERED = sorted({e for _, entries, _ in CASES for e in entries})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_footprint(case, name):
    cid, entries, body = case
    E = Env(name)
    try:
        FP.run_footprint(lambda fp: body(fp, E), device=DEV, sync=torch.cuda.synchronize)
    except RuntimeError as e:       # a device fault poisons the context: nothing more is launched on the GPU from this session
        if "illegal memory access" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault in footprint case {cid} [{name}]: {e}", returncode=3)
        raise
