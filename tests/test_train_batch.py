"""Fine-tuning several clips per step (`--per_gpu_batch_size B`) — CPU side.

  * include/wiw_train_batch.h against its binding table `hip.EXPORTS_TRAIN_BATCH` and both libraries; include/wiw_svd.h (67
    symbols, version 17) and include/wiw_cross_attn_train.h (two symbols) with their tables are as they were;
  * the footprint-coverage rule of tests/test_footprint_harness.py for the new header: every `int wiw_*(` it declares has a case
    in tests/test_hip_train_batch_footprint.py;
  * argument refusals of `wiw_edm_loss_grad_batched` (validated before any launch: no GPU needed);
  * `train.prepare_step` on (B, ...) tensors == the stack of the B single calls, bit for bit; B = 1 returns today's object;
  * `train.batch_from_pixels` on a loader batch == `train.collate` of the single-sample calls on an equally seeded generator;
  * `train.collate` refuses mixed shapes and mixed token counts;
  * `UNetTrain.forward` refuses a mismatched B and rows above MAX_BATCH_ROWS before anything is launched;
  * tests/golden/train_step_batch.npz: size, re-drawn inputs, consistency.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import batch_fixtures as BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wiw_train_batch.h")
FIELDS = ("unet_input", "noisy", "target", "added_time_ids", "ehs", "action_ids")


@pytest.fixture(scope="module")
def lib_path():
    import wiw_amd  # noqa: F401
    from wiw_amd.build import build

    return build(verbose=False)


def declared_symbols(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(wiw_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import EXPORTS, EXPORTS_CROSS_TRAIN, EXPORTS_TRAIN_BATCH

    assert declared_symbols() == sorted(EXPORTS_TRAIN_BATCH) == ["wiw_edm_loss_grad_batched"]
    assert not set(EXPORTS_TRAIN_BATCH) & (set(EXPORTS) | set(EXPORTS_CROSS_TRAIN))
    res, args = EXPORTS_TRAIN_BATCH["wiw_edm_loss_grad_batched"]
    assert res is ctypes.c_int and len(args) == 10 and args[4] is ctypes.c_int64 and args[5] is ctypes.c_int
    # the two earlier headers and their tables are as they were: the addition is a third header, not a new ABI version
    main = declared_symbols(os.path.join(ROOT, "include", "wiw_svd.h"))
    assert main == sorted(EXPORTS) and len(main) == 67
    assert re.search(r"#define WIW_ABI_VERSION 17\b", open(os.path.join(ROOT, "include", "wiw_svd.h")).read())
    cross = declared_symbols(os.path.join(ROOT, "include", "wiw_cross_attn_train.h"))
    assert cross == sorted(EXPORTS_CROSS_TRAIN) == ["wiw_cross_attn_fewkeys_bwd_bf16", "wiw_cross_attn_fewkeys_bwd_partials"]


@pytest.mark.parametrize("variant,code", [("bf16", 0), ("fp16", 1)])
def test_both_libraries_export_the_batched_header(lib_path, variant, code):
    from wiw_amd.build import LIB_F16
    from wiw_amd.hip import EXPORTS_TRAIN_BATCH, load_library

    path = lib_path if variant == "bf16" else LIB_F16
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in wiw_train_batch.h but not exported by {os.path.basename(path)}"
    lib = load_library(path)                      # binds all three tables
    assert lib.wiw_abi_version() == 17 and lib.wiw_dtype() == code
    for name, (res, args) in EXPORTS_TRAIN_BATCH.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_every_launching_entry_point_of_the_batched_header_has_a_footprint_case():
    """The rule of test_footprint_harness.py `test_every_launching_entry_point_has_a_footprint_case`, for this header."""
    import test_hip_train_batch_footprint as T

    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(HEADER).read(), flags=re.M))
    assert declared == {"wiw_edm_loss_grad_batched"}
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    missing = declared - covered - excluded
    assert not missing, f"entry points without a footprint case: {sorted(missing)}"
    assert all(isinstance(r, str) and r for r in T.EXCLUDED.values())
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 3


def test_argument_validation_without_gpu(lib_path):
    """Bad arguments return WIW_EINVAL (-1) with a message before anything is launched."""
    from wiw_amd.hip import load_library

    lib = load_library(lib_path)

    def call(pred=16, noisy=16, target=16, n=64, B=2, sig=16, grad=16, part=16, nb=4):
        return lib.wiw_edm_loss_grad_batched(None, pred, noisy, target, n, B, sig, grad, part, nb)
    for kw in ("pred", "noisy", "target", "sig", "grad", "part"):
        assert call(**{kw: None}) == -1 and b"null" in lib.wiw_last_error(), kw
    for B in (0, -1, 65):
        assert call(B=B) == -1 and b"1 <= B <= 64" in lib.wiw_last_error()
    for n in (0, -5):
        assert call(n=n) == -1 and b"n_per_sample" in lib.wiw_last_error()
    for nb in (0, -1, 4097):
        assert call(nb=nb) == -1 and b"1 <= n_partial <= 4096" in lib.wiw_last_error()


# ---- step inputs -------------------------------------------------------------------------------------------------------
def _same(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and torch.equal(x, y), f
    for f in ("sigma", "timestep"):
        x, y = getattr(a, f), getattr(b, f)
        assert type(x) is type(y), f
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, f


def test_prepare_step_of_a_batch_is_the_stack_of_single_calls():
    """B = 3 (the nav3 scenario: three noise levels, three noise_aug strengths, the three dropout branches): every tensor of the
    batched call equals the concatenation of the three single calls bit for bit; sigma / timestep are fp32 tensors of 3."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T

    st, singles = BF.batch_step_inputs("nav3")
    assert st.batch == 3 and len(singles) == 3
    for f in FIELDS:
        assert torch.equal(getattr(st, f), torch.cat([getattr(s, f) for s in singles])), f
    assert tuple(st.added_time_ids.shape) == (3, 3) and tuple(st.unet_input.shape) == (3, 4, 8, 24, 40)
    for f in ("sigma", "timestep"):
        v = getattr(st, f)
        assert isinstance(v, torch.Tensor) and v.dtype == torch.float32 and tuple(v.shape) == (3,)
        assert torch.equal(v, torch.tensor([getattr(s, f) for s in singles], dtype=torch.float32)), f
    assert [float(x) for x in st.added_time_ids[:, 2]] == [float(np.float32(a)) for a in BF.SCENARIOS["nav3"][7]]
    # the dropout branches: sample 0 lost its tokens, sample 1 its conditioning latents, sample 2 nothing
    assert float(st.ehs[0].abs().max()) == 0.0 and float(st.ehs[1].abs().max()) > 0 and float(st.ehs[2].abs().max()) > 0
    cond = st.unet_input[:, :, 4:]
    assert float(cond[1].abs().max()) == 0.0 and float(cond[0].abs().max()) > 0 and float(cond[2].abs().max()) > 0
    _same(T.collate(singles), st)
    # floats are broadcast; a wrong count is refused
    x = [BF.sample_inputs("nav3", b) for b in range(3)]
    cat = lambda k: torch.cat([s[k] for s in x])  # noqa: E731
    shared = T.prepare_step(cat("latents"), cat("noise"), 1.3, cat("conditional_latents"), cat("encoder_hidden_states"), 0.043,
                            cat("action_ids"))
    assert torch.equal(shared.sigma, torch.tensor([1.3] * 3)) and torch.equal(shared.noisy[0], st.noisy[0])
    with pytest.raises(ValueError, match="sigma"):
        T.prepare_step(cat("latents"), cat("noise"), [1.3, 0.4], cat("conditional_latents"), cat("encoder_hidden_states"), 0.043,
                       cat("action_ids"))
    with pytest.raises(ValueError, match="ehs"):
        T.prepare_step(cat("latents"), cat("noise"), 1.3, cat("conditional_latents"), cat("encoder_hidden_states")[:2], 0.043,
                       cat("action_ids"))


def test_prepare_step_of_one_sample_is_unchanged():
    """B = 1: Python floats for sigma / timestep, (1, 3) time ids — the values and types of the single-sample step as it was; a
    one-element sequence means the same; `collate` of one sample returns it."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T

    x = BF.sample_inputs("tiny2", 0)
    args = (x["latents"], x["noise"])
    rest = (x["conditional_latents"], x["encoder_hidden_states"])
    st = T.prepare_step(*args, 1.7, *rest, 0.043, x["action_ids"], dropout_prob=0.1, random_p=torch.tensor([0.9]))
    assert type(st.sigma) is float and st.sigma == 1.7 and type(st.timestep) is float
    assert st.timestep == 0.25 * float(torch.log(torch.tensor(1.7)))
    assert st.batch == 1 and tuple(st.added_time_ids.shape) == (1, 3) and st.added_time_ids.tolist() == [[7.0, 127.0, float(np.float32(0.043))]]
    noisy = x["latents"] + x["noise"] * 1.7
    assert torch.equal(st.noisy, noisy) and st.target is x["latents"]
    assert torch.equal(st.unet_input[:, :, :4], noisy / (1.7 ** 2 + 1) ** 0.5)
    assert torch.equal(st.unet_input[:, :, 4:], x["conditional_latents"].unsqueeze(1).repeat(1, 4, 1, 1, 1))
    _same(T.prepare_step(*args, [1.7], *rest, torch.tensor([0.043]), x["action_ids"], dropout_prob=0.1, random_p=torch.tensor([0.9])), st)
    assert T.collate([st]) is st


def test_batch_from_pixels_of_a_loader_batch_is_collate_of_single_calls():
    """B = 2 on a seeded generator == `collate` of two single-sample calls, in order, on an equally seeded generator; every
    sample has its own cond_sigma (added_time_ids) and sigma; `draws` is a list of B dicts; per-sample dropout."""
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T

    from test_train_any_size import _draws, _front

    g = torch.Generator().manual_seed(11)
    Tn, H, W = 4, 16, 128
    px = torch.tanh(torch.randn(2, Tn, 3, H, W, generator=g))
    past = torch.tanh(torch.randn(2, 1, 3, H, W, generator=g))
    acts = np.array([[4, 2, 3, 3], [4, 1, 1, 2]])
    front = _front((1, 3, H, W))
    seen = []
    front._embed = lambda x, clip_images: (seen.append(x.clone()), (x.mean() + torch.arange(1024.0)).reshape(1, 1, 1024))[1]
    batched = T.batch_from_pixels(front, px, past, acts, dropout_prob=0.1, generator=torch.Generator().manual_seed(5))
    assert len(seen) == 2 and torch.equal(seen[0], past[0]) and torch.equal(seen[1], past[1])
    g2 = torch.Generator().manual_seed(5)
    singles = [T.batch_from_pixels(front, px[b:b + 1], past[b:b + 1], acts[b:b + 1], dropout_prob=0.1, generator=g2) for b in range(2)]
    _same(batched, T.collate(singles))
    assert batched.batch == 2 and tuple(batched.sigma.shape) == (2,) and float(batched.sigma[0]) != float(batched.sigma[1])
    assert float(batched.added_time_ids[0, 2]) != float(batched.added_time_ids[1, 2])          # its own cond_sigma per sample
    assert tuple(batched.ehs.shape) == (2, 1, 1024) and tuple(batched.action_ids.shape) == (2, Tn, Tn)
    # explicit draws, one dict per sample: random_p 0.05 zeroes sample 0's tokens, 0.25 sample 1's conditioning latents
    gd = torch.Generator().manual_seed(7)
    d = [dict(_draws(gd, Tn, H, W), random_p=torch.tensor([p]), sigma=s, cond_sigma=c) for p, s, c in ((0.05, 0.8, 0.05), (0.25, 1.9, 0.02))]
    st = T.batch_from_pixels(front, px, past, acts, dropout_prob=0.1, draws=d)
    _same(st, T.collate([T.batch_from_pixels(front, px[b:b + 1], past[b:b + 1], acts[b:b + 1], dropout_prob=0.1, draws=d[b])
                         for b in range(2)]))
    assert float(st.ehs[0].abs().max()) == 0.0 and float(st.ehs[1].abs().max()) > 0
    assert float(st.unet_input[1, :, 4:].abs().max()) == 0.0 and float(st.unet_input[0, :, 4:].abs().max()) > 0
    assert torch.equal(st.sigma, torch.tensor([0.8, 1.9])) and [float(v) for v in st.added_time_ids[:, 2]] == [float(np.float32(0.05)), float(np.float32(0.02))]
    with pytest.raises(ValueError, match="list of 2 dicts"):
        T.batch_from_pixels(front, px, past, acts, draws=d[0])
    with pytest.raises(ValueError, match="2 samples"):
        T.batch_from_pixels(front, px, past[:1], acts)
    # manipulation poses (B, T, 8)
    poses = np.random.RandomState(3).uniform(0.1, 0.9, size=(2, Tn, 8)).astype(np.float32)
    m = T.batch_from_pixels(front, px, past, poses, draws=d)
    assert tuple(m.action_ids.shape) == (2, Tn, 10) and torch.allclose(m.noisy[0], m.target[0] + 0.8 * d[0]["latent_noise"][0], atol=1e-6)


def test_collate_refuses_mixed_shapes_and_token_counts():
    import wiw_amd  # noqa: F401
    from wiw_amd import train as T

    def one(h, w, P):
        z = torch.zeros
        return T.prepare_step(z(1, 4, 4, h, w), z(1, 4, 4, h, w), 1.0, z(1, 4, h, w), z(1, P, 1024), 0.02, z(1, 4, 4))
    a = one(8, 16, 1)
    assert T.collate([a, one(8, 16, 1), one(8, 16, 1)]).batch == 3
    with pytest.raises(ValueError, match="unet_input"):
        T.collate([a, one(8, 8, 1)])
    with pytest.raises(ValueError, match="ehs"):
        T.collate([a, one(8, 16, 3)])
    with pytest.raises(ValueError, match="no samples"):
        T.collate([])
    two = T.collate([a, one(8, 16, 1)])
    assert T.collate([two, a]).batch == 3 and tuple(T.collate([two, a]).sigma.shape) == (3,)      # batches concatenate too


# ---- forward's refusals --------------------------------------------------------------------------------------------------
class _NoHip:                      # the constructors need a Hip only for its dtype: nothing is launched on the CPU
    dtype = torch.bfloat16


def _args(B, T=4, h=8, w=16, P=1):
    z = torch.zeros
    return [z(B, T, 8, h, w), z(B) + 0.1 if B > 1 else 0.1, z(B, P, 1024), z(B, 3), z(B, T, T)]


@pytest.mark.parametrize("which", ["timestep", "ehs", "added_time_ids", "action_ids"])
@pytest.mark.parametrize("cls32", [False, True], ids=["UNetTrain", "UNetTrain32"])
def test_forward_refuses_a_mismatched_batch(which, cls32):
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import UNetTrain, UNetTrain32

    net = (UNetTrain32 if cls32 else UNetTrain)(UNetConfig.tiny(4), {}, "cpu", hip=_NoHip())
    i = ["sample", "timestep", "ehs", "added_time_ids", "action_ids"].index(which)
    for other in (3, 1):
        a, o = _args(2), _args(other)
        a[i] = o[i]
        with pytest.raises(ValueError, match=which):
            net.forward(*a)
        assert getattr(net, "tape", None) is None                  # refused before a tape exists: nothing was launched
    with pytest.raises(ValueError, match="timestep"):
        net.forward(*[x if j != 1 else 0.1 for j, x in enumerate(_args(2))])      # one float for two samples
    net3 = UNetTrain(UNetConfig.tiny(4), {}, "cpu", hip=_NoHip(), num_past_obs=3)
    with pytest.raises(ValueError, match="num_past_obs = 3"):
        net3.forward(*_args(2, P=2))


def test_forward_refuses_rows_above_the_envelope():
    """B > 1 above 32 x 72 x 128 first-level rows: ValueError naming the bound; B = 1 is not touched by it."""
    import wiw_amd  # noqa: F401
    from wiw_amd.config import UNetConfig
    from wiw_amd.train_unet import MAX_BATCH_ROWS, UNetTrain

    assert MAX_BATCH_ROWS == 32 * 72 * 128 == 294912
    net = UNetTrain(UNetConfig.tiny(14), {}, "cpu", hip=_NoHip())
    big = lambda B: [torch.zeros(B, 14, 8, 72, 128), torch.zeros(B) + 0.1, torch.zeros(B, 1, 1024),  # noqa: E731
                     torch.zeros(B, 3), torch.zeros(B, 14, 14)]
    with pytest.raises(ValueError, match=r"294912.*MAX_BATCH_ROWS"):
        net.forward(*big(3))                                        # 3 x 14 x 72 x 128 = 387 072 rows
    assert getattr(net, "tape", None) is None
    assert net._check_batch(*big(2))[0] == 2                        # 258 048 rows: inside
    one = big(1)
    one[1] = 0.1
    assert net._check_batch(*one) == (1, [0.1])


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_batch_fixture(golden):
    """tests/golden/train_step_batch.npz: below 1 MiB, inputs re-draw to the stored checksums, the loss is the mean of the
    per-sample losses, every live tensor has a norm, the watch list is stored."""
    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, BF.NAME)) < (1 << 20)
    g, pre = golden(BF.NAME), "full2__"
    h, w, T, B, P, seed, sig, aug, rp, _ = BF.SCENARIOS["full2"]
    assert int(g[f"{pre}input_seed"]) == seed and tuple(g[f"{pre}latent_hw"]) == (h, w) and int(g["weight_seed"]) == BF.WEIGHT_SEED
    assert np.array_equal(BF.checksums("full2"), g[f"{pre}input_checksums"]), "the re-drawn inputs are not the generator's"
    assert np.array_equal(g[f"{pre}sigmas"], np.array(sig, np.float32)) and np.array_equal(g[f"{pre}random_p"], np.array(rp, np.float32))
    assert np.array_equal(g[f"{pre}noise_aug_strength"], np.array(aug)) and float(g["dropout_prob"]) == BF.DROPOUT
    assert tuple(g[f"{pre}model_pred"].shape) == (B, T, 4, h, w)
    ls = g[f"{pre}sample_losses"]
    assert ls.shape == (B,) and abs(float(g[f"{pre}loss"]) - float(ls.mean())) <= 1e-12 and ls[0] != ls[1]
    names, norms = [str(n) for n in g[f"{pre}grad_names"]], g[f"{pre}grad_norms"]
    assert len(names) == len(set(names)) and set(BF.WATCH) <= set(names) and sum(BF.is_dead(n) for n in names) == 132
    for n, v in zip(names, norms):
        assert (v == 0.0) if BF.is_dead(n) else (v > 0.0), n
    for name in BF.WATCH:
        key = name.replace(".", "__")
        assert f"{pre}grad__{key}" in g.files or f"{pre}grad8__{key}" in g.files, name
