"""The footprint harness (tests/footprint.py) against fake Python "kernels" on CPU tensors: it passes a correct one and names
the violated property for every seeded defect — the evidence that tests/test_hip_footprint.py would fail on a kernel that is
subtly wrong about WHERE it reads and writes.  Also: the layout the harness promises (alignment, guards, gaps, fills)."""
import re

import pytest
import torch

import footprint as FP

M, N = 5, 16


def _x():
    return torch.randn(M, N, generator=torch.Generator().manual_seed(1))


def _kernel(x, o, defect=None):
    """out[m][n] = 2 x[m][n] written the way a kernel addresses memory: a flat pointer, a base and a leading dimension."""
    xf, of = x.flat, o.flat
    for m in range(M):
        src = xf[x.base + m * x.ld: x.base + m * x.ld + N].float()
        if defect == "mask_times_neighbour":      # a masked lane MULTIPLIED by zero instead of selected away
            src = src + 0.0 * xf[x.base + M * x.ld: x.base + M * x.ld + N].float()
        of[o.base + m * o.ld: o.base + m * o.ld + N] = (2.0 * src).to(o.dtype)
    if defect == "past_last_row":
        of[o.base + M * o.ld] = 1.0
    if defect == "gap_column":
        of[o.base + 2 * o.ld + N] = 1.0
    if defect == "modifies_input":
        xf[x.base + 3 * x.ld + 2] = 7.0


def _body(dtype, defect):
    def body(fp):
        x = fp.inp("x", _x(), dtype)
        o = fp.out("out", M, N, dtype)
        _kernel(x, o, defect)

        def check(got, ref, what):
            assert torch.equal(got, ref), what
        fp.expect("2x", lambda: o.window().float(), lambda: 2.0 * _x().to(dtype).float(), check)
    return body


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_correct_kernel_passes(dtype):
    outs = FP.run_footprint(_body(dtype, None))
    assert set(outs) == {"out"} and outs["out"].shape == (M, N)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("defect,prop", [("past_last_row", FP.P2), ("gap_column", FP.P2), ("mask_times_neighbour", FP.P1),
                                         ("modifies_input", FP.P3)])
def test_seeded_defect_is_named(dtype, defect, prop):
    with pytest.raises(FP.FootprintViolation) as e:
        FP.run_footprint(_body(dtype, defect))
    assert e.value.prop == prop and str(e.value).startswith(prop), str(e.value)


def test_defect_location_is_reported():
    with pytest.raises(FP.FootprintViolation, match=re.escape(f"row 2, column {N}")):
        FP.run_footprint(_body(torch.bfloat16, "gap_column"))
    with pytest.raises(FP.FootprintViolation, match=re.escape(f"row {M}, column 0")):
        FP.run_footprint(_body(torch.bfloat16, "past_last_row"))


def test_mask_times_neighbour_passes_on_clean_memory():
    """The defect is invisible to a test whose surroundings are zeros or finite numbers: 0 * v == 0.  Only the NaN (or, for an
    overflowing product, the garbage) run shows it — which is why every case runs all three."""
    FP.run_footprint(_body(torch.bfloat16, "mask_times_neighbour"), fills=("zero", "garbage"))
    with pytest.raises(FP.FootprintViolation):
        FP.run_footprint(_body(torch.bfloat16, "mask_times_neighbour"), fills=("zero", "nan"))


def test_parity_failure_is_p4():
    def body(fp):
        x = fp.inp("x", _x(), torch.float32)
        o = fp.out("out", M, N, torch.float32)
        _kernel(x, o)
        fp.expect("3x", lambda: o.window(), lambda: 3.0 * _x(), lambda g, r, w: (_ for _ in ()).throw(AssertionError("off")) if not torch.equal(g, r) else None)
    with pytest.raises(FP.FootprintViolation) as e:
        FP.run_footprint(body)
    assert e.value.prop == FP.P4


def test_unwritten_output_element_is_p1():
    """A declared output element the kernel never writes keeps the sentinel, which differs between the runs."""
    def body(fp):
        x = fp.inp("x", _x(), torch.float32)
        o = fp.out("out", M + 1, N, torch.float32)
        _kernel(x, o)
    with pytest.raises(FP.FootprintViolation) as e:
        FP.run_footprint(body)
    assert e.value.prop == FP.P1


@pytest.mark.parametrize("dtype,align", [(torch.bfloat16, 16), (torch.float16, 8), (torch.float32, 4), (torch.float32, 16)])
@pytest.mark.parametrize("fill", FP.FILLS)
def test_layout(dtype, align, fill):
    a = FP.Arena("t", 7, 24, dtype, device="cpu", fill=fill, data=torch.ones(7, 24), align=align)
    size = a.itemsize
    assert a.ptr() % 256 == align and a.ptr() % align == 0 and a.ptr() % (2 * align) != 0
    assert a.window().data_ptr() == a.ptr() and a.window().shape == (7, 24) and a.window().stride() == (a.ld, 1)
    assert a.ld == 24 + (8 if size == 2 else 4)
    assert a.guard >= 256 * a.ld and a.guard * size >= 4096
    assert a.flat.numel() == 2 * a.guard + 6 * a.ld + 24
    assert torch.equal(a.window().float(), torch.ones(7, 24))
    outside = a.flat[~a.mask].float()
    assert outside.numel() == 2 * a.guard + 6 * (a.ld - 24)
    if fill == "zero":
        assert bool((outside == 0).all())
    elif fill == "nan":
        assert bool(torch.isnan(outside).all())
        word = a.flat.view(a.int_dtype)[0].item() & ((1 << (8 * size)) - 1)
        assert word == (0x7FFF if size == 2 else 0x7FC00000)
    else:
        assert bool(torch.isfinite(outside).all())
        assert bool((outside.abs() >= (990.0 if size == 2 else 1e30)).all()) and (size == 4 or bool((outside.abs() <= 3.01e4).all()))
        assert bool((outside > 0).any()) and bool((outside < 0).any())
    a.outside_untouched()
    a.inputs_unchanged()


def test_output_prefill_is_a_sentinel_that_differs_between_runs():
    seen = set()
    for fill in FP.FILLS:
        o = FP.Arena("o", 3, 8, torch.float16, device="cpu", fill=fill, role="out")
        b = set(o.buf.tolist())
        assert len(b) == 1
        seen |= b
    assert len(seen) == len(FP.FILLS) and 0 not in seen


def test_documented_untouched_region():
    o = FP.Arena("A", 4, 8, torch.float32, device="cpu", fill="nan", role="inout", data=torch.zeros(4, 8))
    o.window()[1:, :6] = 1.0
    o.untouched_in_window(rows=slice(0, 1))
    o.untouched_in_window(cols=slice(6, 8))
    o.window()[0, 0] = 2.0
    with pytest.raises(FP.FootprintViolation) as e:
        o.untouched_in_window(rows=slice(0, 1))
    assert e.value.prop == FP.P2


def test_every_launching_entry_point_has_a_footprint_case():
    """include/wiw_svd.h is parsed for `int wiw_*(` declarations: each is in the case table of tests/test_hip_footprint.py or
    in its short, commented exclusion list — a new entry point cannot arrive without a footprint case."""
    import os

    import test_hip_footprint as T

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wiw_svd.h")
    declared = set(re.findall(r"^int\s+(wiw_\w+)\s*\(", open(header).read(), flags=re.M))
    assert len(declared) > 60 and "wiw_gemm_bf16" in declared and "wiw_fill_f32" in declared
    covered, excluded = set(T.COVERED), set(T.EXCLUDED)
    assert not (covered & excluded)
    assert covered <= declared and excluded <= declared, sorted((covered | excluded) - declared)
    missing = declared - covered - excluded
    assert not missing, f"entry points without a footprint case: {sorted(missing)}"
    assert all(n.endswith("_ok") or n.startswith("wiw_calib_") or n in ("wiw_abi_version", "wiw_dtype", "wiw_device_check",
                                                                         "wiw_grad_sumsq_chunk") for n in excluded)
    assert all(isinstance(r, str) and r for r in T.EXCLUDED.values())
    ids = [c[0] for c in T.CASES]
    assert len(ids) == len(set(ids))
