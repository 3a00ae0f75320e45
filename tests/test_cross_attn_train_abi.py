"""Fine-tuning with 2 .. 8 conditioning tokens per sample — CPU side.

  * include/wiw_cross_attn_train.h (the backward of the few-keys cross-attention) against its binding table
    `hip.EXPORTS_CROSS_TRAIN` and both libraries; include/wiw_svd.h and `hip.EXPORTS` keep their symbols and their version;
  * the footprint-coverage rule of tests/test_footprint_harness.py for the companion header: every `int wiw_*(` it declares has
    a case in tests/test_hip_cross_attn_bwd_footprint.py;
  * argument refusals of the new entry point (validated before any launch: no GPU needed);
  * `Trainer.is_dead` / `optimizer_shapes` with num_past_obs 1 and 3, the `num_past_obs` keyword of the tapes, the token-count
    check of `UNetTrain.forward`, and the (1, P, D) conditioning of `train.batch_from_pixels`;
  * tests/golden/train_step_ctx.npz: size, re-drawn inputs, and the generator's "newly live gradients are signal" ratios.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wiw_cross_attn_train.h")


@pytest.fixture(scope="module")
def lib_path():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import build

    return build(verbose=False)


def declared_symbols(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(wiw_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree():
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import EXPORTS, EXPORTS_CROSS_TRAIN

    assert declared_symbols() == sorted(EXPORTS_CROSS_TRAIN) == ["wiw_cross_attn_fewkeys_bwd_bf16", "wiw_cross_attn_fewkeys_bwd_partials"]
    assert not set(EXPORTS) & set(EXPORTS_CROSS_TRAIN)
    # the first header and its table are as they were: the addition is a second header, not a new ABI version
    main = declared_symbols(os.path.join(ROOT, "include", "wiw_svd.h"))
    assert main == sorted(EXPORTS) and len(main) == 67 and not set(main) & set(EXPORTS_CROSS_TRAIN)
    assert re.search(r"#define WIW_ABI_VERSION 17\b", open(os.path.join(ROOT, "include", "wiw_svd.h")).read())
    res, args = EXPORTS_CROSS_TRAIN["wiw_cross_attn_fewkeys_bwd_bf16"]
    assert res is ctypes.c_int and len(args) == 17
    assert EXPORTS_CROSS_TRAIN["wiw_cross_attn_fewkeys_bwd_partials"][0] is ctypes.c_int64


@pytest.mark.parametrize("variant,code", [("bf16", 0), ("fp16", 1)])
def test_both_libraries_export_the_companion_header(lib_path, variant, code):
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS_CROSS_TRAIN, load_library

    path = lib_path if variant == "bf16" else LIB_F16
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in wiw_cross_attn_train.h but not exported by {os.path.basename(path)}"
    lib = load_library(path)                      # binds both tables
    assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code
    for name, (res, args) in EXPORTS_CROSS_TRAIN.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_every_launching_entry_point_of_the_companion_header_has_a_footprint_case():
    """The rule of test_footprint_harness.py `test_every_launching_entry_point_has_a_footprint_case`, for this header."""
    import test_hip_cross_attn_bwd_footprint as T

    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    assert declared == {"wiw_cross_attn_fewkeys_bwd_bf16"}
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    missing = declared - covered - excluded
    assert not missing, f"entry points without a footprint case: {sorted(missing)}"
    assert all(isinstance(r, str) and r for r in T.EXCLUDED.values())
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 3


def test_argument_validation_without_gpu(lib_path):
    """Bad arguments return WIW_EINVAL (-1) with a message before anything is launched; the size query answers 0."""
    from wiw_amd.hip import load_library

    lib = load_library(lib_path)

    def call(ldq=64, lddo=64, lddq=64, rows=16, rpi=8, heads=1, P=2, Q=16, part=16):
        return lib.wiw_cross_attn_fewkeys_bwd_bf16(None, Q, ldq, 16, 16, 16, lddo, 16, lddq, 16, 16, part, rows, rpi, heads, P, 0.125)
    assert call(Q=None) == -1 and b"null" in lib.wiw_last_error()
    assert call(P=9) == -1 and b"1 <= P <= 8" in lib.wiw_last_error()
    assert call(P=0) == -1 and b"1 <= P <= 8" in lib.wiw_last_error()
    assert call(rows=15) == -1 and b"whole items" in lib.wiw_last_error()
    assert call(lddq=56) == -1 and b">= C" in lib.wiw_last_error()
    assert call(lddo=68) == -1 and b"multiples of 8" in lib.wiw_last_error()
    assert call(heads=33) == -1 and b"at most 2048" in lib.wiw_last_error()
    assert call(Q=8) == -1 and b"16-byte aligned" in lib.wiw_last_error()
    assert call(part=20) == -1 and b"16-byte aligned" in lib.wiw_last_error()
    q = lib.wiw_cross_attn_fewkeys_bwd_partials
    assert q(16, 8, 1, 9) == 0 and q(15, 8, 1, 2) == 0 and q(16, 8, 33, 2) == 0
    assert q(16, 8, 1, 2) == 2 * 1 * 2 * 2 * 64                       # items x blocks x [2][P][C]
    # C = 64: 32 row slots -> 256 rows per block; C = 1280: one slot -> 64 rows per block (csrc/cross_attn_bwd.hip)
    assert q(600, 600, 1, 3) == 3 * 2 * 3 * 64 and q(1200, 600, 20, 8) == 2 * 10 * 2 * 8 * 1280
    assert q(1 << 33, 1 << 20, 5, 2) == (1 << 13) * ((1 << 20) // 192 + 1) * 2 * 2 * 320     # 64-bit arithmetic


class _Stub:
    """What `Trainer.optimizer_shapes` reads of a net: the masters and (optionally) num_past_obs."""

    def __init__(self, P=None):
        import wiw_amd  # noqa: F401
        from wiw_amd.config import UNetConfig
        from wiw_amd.weights import random_state_dict

        self.master = random_state_dict(UNetConfig.tiny(4), 0)
        if P is not None:
            self.num_past_obs = P


def _newly_live(n):
    return ("attn2.to_q." in n) or ("attn2.to_k." in n) or ("transformer_blocks." in n and ".norm2." in n)


def test_dead_set_and_optimizer_shapes_follow_num_past_obs():
    from wiw_amd.train_unet import Trainer

    legacy, one, three = _Stub(), _Stub(1), _Stub(3)
    names = list(legacy.master)
    live_new = [n for n in names if _newly_live(n)]
    emb = [n for n in names if n.startswith("add_embedding.")]
    assert len(live_new) == 128 and len(emb) == 4                  # 16 transformers x 2 blocks x (to_q, to_k, norm2 w + b)
    for n in names:
        assert Trainer.is_dead(n) == Trainer.is_dead(n, 1) == (n in live_new or n in emb), n
        for P in (2, 3, 8):
            assert Trainer.is_dead(n, P) == Trainer.is_dead(n, num_past_obs=P) == (n in emb), n
    full1 = Trainer.optimizer_shapes(one, "full")
    assert full1 == Trainer.optimizer_shapes(legacy, "full") and len(full1) == len(names) - 132
    full3 = Trainer.optimizer_shapes(three, "full")
    assert list(full3) == [n for n in names if n not in emb] and set(full3) - set(full1) == set(live_new)
    assert all(full3[n] == tuple(three.master[n].shape) for n in full3)
    # `--train_param_type new` / `new+temp_layer` select by name; the temporal blocks' cross-attention joins the latter
    assert Trainer.optimizer_shapes(three, "new") == Trainer.optimizer_shapes(one, "new")
    t1, t3 = Trainer.optimizer_shapes(one, "new+temp_layer"), Trainer.optimizer_shapes(three, "new+temp_layer")
    assert set(t3) - set(t1) == {n for n in live_new if "temporal_transformer_block" in n} and len(set(t3) - set(t1)) == 64


class _NoHip:                      # the constructors need a Hip only for its dtype: nothing is launched on the CPU
    dtype = torch.bfloat16


def test_num_past_obs_keyword_of_the_tapes():
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain, UNetTrain32, make_unet_train

    cfg = UNetConfig.tiny(4)
    assert UNetTrain(cfg, {}, "cpu", hip=_NoHip()).num_past_obs == 1
    assert make_unet_train(cfg, {}, "cpu", hip=_NoHip()).num_past_obs == 1
    for cls in (UNetTrain, UNetTrain32, make_unet_train):
        for P in (1, 2, 8):
            assert cls(cfg, {}, "cpu", hip=_NoHip(), num_past_obs=P).num_past_obs == P
        for bad in (0, 9, -1, 2.0, True):
            with pytest.raises(ValueError, match="num_past_obs"):
                cls(cfg, {}, "cpu", hip=_NoHip(), num_past_obs=bad)
    net = make_unet_train(UNetConfig.tiny(25), {}, "cpu", hip=_NoHip(), num_past_obs=3)
    assert type(net) is UNetTrain32 and net.num_past_obs == 3


@pytest.mark.parametrize("built,given", [(1, 3), (3, 1), (3, 2), (2, 3)])
def test_token_count_mismatch_is_refused(built, given):
    """`forward` checks the conditioning before it touches a weight or launches anything."""
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain

    cfg = UNetConfig.tiny(4)
    net = UNetTrain(cfg, {}, "cpu", hip=_NoHip(), num_past_obs=built)
    with pytest.raises(ValueError, match=f"num_past_obs = {built}"):
        net.forward(torch.zeros(1, 4, 8, 8, 16), 0.1, torch.zeros(1, given, 1024), torch.zeros(1, 3), torch.zeros(1, 4, 4))


@pytest.mark.parametrize("P", [1, 3, 8])
def test_batch_from_pixels_embeds_every_past_observation(P):
    """past_obs (1, P, 3, H, W) -> `front._embed` on (P, 3, H, W) -> ehs (1, P, D), token p = the embedding of observation p;
    one conditioning-dropout draw zeroes all P tokens (svd_utils.py:176-241)."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T

    from test_train_any_size import _draws, _front

    g = torch.Generator().manual_seed(3)
    Tn, H, W = 4, 32, 128
    px = torch.tanh(torch.randn(1, Tn, 3, H, W, generator=g))
    past = torch.tanh(torch.randn(1, P, 3, H, W, generator=g))
    front = _front(None)
    seen = []

    def embed(x, clip_images):
        assert tuple(x.shape) == (P, 3, H, W) and clip_images is None
        seen.append(x.clone())
        return (x.mean(dim=(1, 2, 3))[:, None, None] + torch.arange(1024.0)[None, None]).float()     # (P, 1, D)
    front._embed = embed
    d = _draws(g, Tn, H, W)
    st = T.batch_from_pixels(front, px, past, np.array([[4, 1, 2, 3]]), dropout_prob=0.1, draws=d)
    assert len(seen) == 1 and torch.equal(seen[0], past[0])
    assert tuple(st.ehs.shape) == (1, P, 1024)
    for p in range(P):
        assert torch.allclose(st.ehs[0, p], past[0, p].mean() + torch.arange(1024.0))
    dropped = T.batch_from_pixels(front, px, past, np.array([[4, 1, 2, 3]]), dropout_prob=0.1, draws=dict(d, random_p=torch.tensor([0.05])))
    assert tuple(dropped.ehs.shape) == (1, P, 1024) and float(dropped.ehs.abs().max()) == 0.0


def test_ctx_fixture(golden):
    """tests/golden/train_step_ctx.npz: below 1 MiB, inputs re-draw to the stored checksums, and — what the generator asserted —
    every newly live gradient is signal: per transformer block |to_q|, |to_k| >= 1e-2 |to_v| and |norm2.weight| >= 1e-3 |to_v|."""
    from conftest import GOLDEN
    from ctx_fixtures import CTX_FULL, NAME, PREFIXES, SCENARIOS, ctx_config, ctx_inputs

    assert os.path.getsize(os.path.join(GOLDEN, NAME)) < (1 << 20)
    g = golden(NAME)
    for pre in PREFIXES:
        h, w, T, P, _, _, _, _, with_bf16 = SCENARIOS[pre]
        x = ctx_inputs(g, pre)
        cfg = ctx_config(pre)
        assert tuple(x["encoder_hidden_states"].shape) == (1, P, cfg.cross_attention_dim) and int(g[f"{pre}num_past_obs"]) == P
        assert tuple(x["latents"].shape) == tuple(g[f"{pre}model_pred"].shape) == (1, T, 4, h, w) and cfg.num_frames == T
        assert (f"{pre}loss_ref_bf16" in g.files) == with_bf16
        norms = dict(zip((str(n) for n in g[f"{pre}grad_names"]), g[f"{pre}grad_norms"]))
        blocks = [k[: -len("attn2.to_v.weight")] for k in norms if k.endswith(".attn2.to_v.weight")]
        assert len(blocks) == 32
        for b in blocks:
            nv = norms[b + "attn2.to_v.weight"]
            assert norms[b + "attn2.to_q.weight"] >= 1e-2 * nv and norms[b + "attn2.to_k.weight"] >= 1e-2 * nv, b
            assert norms[b + "norm2.weight"] >= 1e-3 * nv, b
        for name in CTX_FULL:
            key = name.replace(".", "__")
            assert f"{pre}grad__{key}" in g.files or f"{pre}grad8__{key}" in g.files, name
