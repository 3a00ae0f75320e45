"""WHERE the entry points of include/wiw_cross_attn_train.h read and write — the rules and the harness of
tests/test_hip_footprint.py (tests/footprint.py) for the companion header.  GPU only (the table itself imports without one).

Q, dO and dQ are strided windows (leading dimension = C + 8, the smallest step the entry point's checks allow) at the minimum
alignment the header states (16 bytes and not 32) between poisoned guards; K / V, the fp32 dK / dV and the partials are dense
at that alignment; the partials arena has exactly `wiw_cross_attn_fewkeys_bwd_partials(...)` floats and must be fully written.
Three launches per case (surroundings zero, finite garbage, NaN): P1 independence, P2 containment, P3 inputs unchanged, and P4
— a training entry — the zero run against a dense-layout launch of the same kernel on the same values, bit for bit
(tests/test_hip_cross_attn_bwd.py holds the parity with fp32 autograd).
"""
import pytest
import torch

import footprint as FP
from test_hip_footprint import DEV, F32, Env, ptr, rnd, train

CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


def cross_attn_bwd(heads, P, items, rpi):
    def run(m, E):
        dt, C, rows = E.dt, heads * 64, items * rpi
        q, do = E.r(rnd(rows, C, seed=1)), E.r(rnd(rows, C, seed=4))
        k, v = E.r(rnd(items, P, C, seed=2)), E.r(rnd(items, P, C, seed=3))
        Q, dO = m.inp("Q", q, dt), m.inp("dO", do, dt)
        Kk, V = m.inp("K", k.reshape(items * P, C), dt, gap=0), m.inp("V", v.reshape(items * P, C), dt, gap=0)
        n = int(E.lib.wiw_cross_attn_fewkeys_bwd_partials(rows, rpi, heads, P))
        assert n > 0 and n % (2 * P * C) == 0
        dQ = m.out("dQ", rows, C, dt)
        dK, dV = m.out("dK", items * P, C, F32, gap=0), m.out("dV", items * P, C, F32, gap=0)
        Pa = m.out("partial", 1, n, F32, gap=0)
        E.ck(E.lib.wiw_cross_attn_fewkeys_bwd_bf16(E.stream(), ptr(Q), Q.ld, ptr(Kk), ptr(V), ptr(dO), dO.ld, ptr(dQ), dQ.ld, ptr(dK),
                                                   ptr(dV), ptr(Pa), rows, rpi, heads, P, 0.125), "cross_attn_fewkeys_bwd")
        return dict(dQ=dQ, dK=dK, dV=dV, partial=Pa)
    return train(run)


ENTRY = "wiw_cross_attn_fewkeys_bwd_bf16"
for _P in (1, 3, 8):                                                       # 6 row slots + 16 surplus threads, a ragged tail
    add(f"cross_attn_fewkeys_bwd-P{_P}", [ENTRY], cross_attn_bwd(5, _P, 2, 37))
add("cross_attn_fewkeys_bwd-1row", [ENTRY], cross_attn_bwd(1, 2, 2, 1))       # 32 row slots, one row: 31 slots add zeros
add("cross_attn_fewkeys_bwd-blocks", [ENTRY], cross_attn_bwd(20, 2, 1, 600))  # 1 slot + 96 surplus threads, 10 blocks, ragged last

# Coverage: every `int wiw_*(` declaration of include/wiw_cross_attn_train.h is in the table above or excluded here
# (tests/test_cross_attn_train_abi.py checks it without a GPU).  The size query returns int64_t and launches nothing.
EXCLUDED = {}
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
