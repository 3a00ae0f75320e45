"""WHERE the entry points of include/wiw_range.h read and write — the rules and the harness of tests/test_hip_footprint.py
(tests/footprint.py) for the range-statistics header.  GPU only (the table itself imports without one).

X is a STRIDED window: rows with gap columns that hold poison (an odd leading dimension puts the row starts at every
element alignment), its first byte at the element's own alignment and no more (2 bytes for the 16-bit type, 4 for fp32);
`partials`, `out` and `hist` at 8 bytes and not 16; everything between poisoned guards.  Three launches per case (surroundings
zero, finite garbage, NaN): P1 independence — a NaN in the padding must not be counted —, P2 containment (`out` is written in
its segments x 48 bytes and `hist` in its segments x 64 words only; `partials` is scratch of exactly the size the query
answers: containment alone), P3 inputs unchanged, and P4 — the zero run equals `range.reference_stats`, number for number.
"""
import numpy as np
import pytest
import torch

import footprint as FP
from test_hip_footprint import DEV, F32, Env, ptr

U8, I64 = torch.uint8, torch.int64
CASES = []          # (id, entry points, body(fp, E))


def add(cid, entries, body):
    CASES.append((cid, tuple(entries), body))


def _data(rows, cols, seed):
    """fp32 values every one of which is exact in bf16 and in fp16, with the special values sprinkled in."""
    rs = np.random.RandomState(seed)
    x = (rs.randint(-128, 128, size=(rows, cols)) * 2.0 ** rs.randint(-12, 8, size=(rows, cols))).astype(np.float32)
    flat = x.reshape(-1)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -14, 32768.0, 2.0 ** -13]
    for k, i in enumerate(rs.choice(flat.size, size=min(flat.size, 3 * len(special)), replace=False)):
        flat[i] = special[k % len(special)]
    flat[0], flat[-1] = np.inf, np.nan          # the first and the last element of the window
    return x


def range_case(f32, rows, cols, gap, segments, hist):
    def body(fp, E):
        from wiw_amd.range import reference_stats, stats_records

        x = _data(rows, cols, rows * 1000 + cols)
        dt = F32 if f32 else E.dt
        X = fp.inp("X", torch.from_numpy(x), dt, gap=gap, align=4 if f32 else 2)
        rps = rows // segments
        n = E.lib.wiw_range_stats_partials(rows, cols, rps, int(hist))
        assert n > 0 and n % 8 == 0
        Pt = fp.out("partials", 1, n, U8, gap=0, align=8, compare=False)
        O = fp.out("out", segments, 48, U8, gap=0, align=8)
        Hs = fp.out("hist", segments, 64, I64, gap=0, align=8) if hist else None
        hot, tiny = 1024.0, 2.0 ** -10
        E.ck(E.lib.wiw_range_stats(E.stream(), ptr(X), int(f32), rows, cols, X.ld, rps, hot, tiny, ptr(Pt), ptr(O), ptr(Hs)),
             "wiw_range_stats")

        def got():
            return stats_records(O.window().contiguous(), Hs.window().contiguous() if hist else None)

        def check(got, ref, what):
            same = all(np.array_equal(g[k], r[k]) for g, r in zip(got, ref) for k in r) and len(got) == len(ref)
            print(f"[footprint P4 {E.name}] {what}: equal = {same}")
            assert same, (got, ref)
        fp.expect(f"range_stats f32={f32} {rows}x{cols} ld {X.ld} in {segments} segment(s)", got,
                  lambda: reference_stats(x, rows_per_segment=rps, hot=hot, tiny=tiny, hist=hist), check)
    return body


R = "wiw_range_stats"
add("range-16-odd-ld", [R], range_case(False, 37, 53, 4, 1, True))               # ld 57: row starts at every 2-byte alignment
add("range-16-odd-ld-7", [R], range_case(False, 12, 45, 2, 3, False))            # ld 47: odd; 3 segments; no histogram
add("range-f32-segments", [R], range_case(True, 24, 130, 1, 4, True))            # ld 131: row starts at 4, 8, 12 mod 16
add("range-f32-many-blocks", [R], range_case(True, 80, 300, 5, 2, False))        # 40 units = 5 blocks per segment
add("range-16-long-rows", [R], range_case(False, 2, 9001, 5, 2, True))           # a row is three chunks, the last one short
add("range-16-contiguous", [R], range_case(False, 16, 1000, 0, 4, True))         # ld == cols: a segment is read as one row

# Coverage: every `int wiw_*(` declaration of include/wiw_range.h is in the table above or excluded here
# (tests/test_range.py checks it without a GPU).
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
