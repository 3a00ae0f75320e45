"""WHERE the entry point of include/wiw_train_batch.h reads and writes — the rules and the harness of
tests/test_hip_footprint.py (tests/footprint.py) for the batched companion header.  GPU only (the table itself imports without
one).

pred / noisy / target / grad are dense [B][n_per_sample] fp32 and the partials dense [B][n_partial], each at the minimum
alignment the header states (4 bytes and not 8) between poisoned guards; the B sigmas sit in their own arena.  Three launches
per case (surroundings zero, finite garbage, NaN): P1 independence, P2 containment, P3 inputs unchanged, and P4 — a training
entry — the zero run against a dense-layout launch of the same kernel on the same values, bit for bit
(tests/test_hip_train_batch.py holds the parity with wiw_edm_loss_grad).
"""
import pytest
import torch

import footprint as FP
from test_hip_footprint import DEV, F32, Env, ptr, rnd, train

CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


def edm_batched(B, n, nb):
    def run(m, E):
        Pr, No, Tg = (m.inp(nm, rnd(B, n, seed=s), F32, gap=0, align=4) for nm, s in (("pred", 1), ("noisy", 2), ("target", 3)))
        Sg = m.inp("sigmas", torch.tensor([0.4 + 0.7 * b for b in range(B)]), F32, gap=0, align=4)
        G, Pa = m.out("grad", B, n, F32, gap=0, align=4), m.out("partial", B, nb, F32, gap=0, align=4)
        E.ck(E.lib.wiw_edm_loss_grad_batched(E.stream(), ptr(Pr), ptr(No), ptr(Tg), n, B, ptr(Sg), ptr(G), ptr(Pa), nb),
             "edm_loss_grad_batched")
        return dict(grad=G, partial=Pa)
    return train(run)


ENTRY = "wiw_edm_loss_grad_batched"
add("edm_loss_grad_batched-B1", [ENTRY], edm_batched(1, 1001, 4))          # the single-sample shape of test_hip_footprint.py
add("edm_loss_grad_batched-B3", [ENTRY], edm_batched(3, 1001, 2))          # odd B, two grid-stride passes, a ragged tail
add("edm_loss_grad_batched-idle", [ENTRY], edm_batched(2, 240, 3))         # blocks 1 and 2 of every sample have no element
add("edm_loss_grad_batched-B64", [ENTRY], edm_batched(64, 8, 1))           # the largest batch, 8 elements per sample

# Coverage: every `int wiw_*(` declaration of include/wiw_train_batch.h is in the table above or excluded here
# (tests/test_train_batch.py checks it without a GPU).
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
