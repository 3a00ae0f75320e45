#!/usr/bin/env python
"""Prove that a source-only change left the device code alone: emit gfx950 assembly for every csrc source x library
variant of the working tree and of REV (default HEAD~1) and compare them line by line.  Compiler only: no library is
loaded and no GPU is touched.  Exit status 1 on any difference.

    python tools/isa_identity.py [REV]
hipcc's device assembly is deterministic for these sources except for the `__hip_cuid_<hash>` symbol, which is
replaced by a fixed token before the comparison."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "world-in-world_amd"
_spec = importlib.util.spec_from_file_location("wiw_build", os.path.join(ROOT, PKG, "build.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)   # build.py alone: SOURCES / FLAGS / EXTRA / VARIANTS, nothing of the package is imported
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def emit(csrc: str, src: str, defs: list, out: str) -> list:
    cmd = [B.HIPCC, *B.FLAGS, *defs, *B.EXTRA.get(src, []), "--offload-device-only", "-S",
           os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {csrc}/{src} {defs}:\n{r.stdout}")
    with open(out) as f:
        return [CUID.sub("__hip_cuid_X", line.rstrip("\n")) for line in f]


def main() -> int:
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", rev], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        # csrc includes ../../include/wiw_svd.h: extracting both directories keeps that relative path working
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, f"{PKG}/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=ar.stdout)
        if ar.wait() != 0:
            raise RuntimeError(f"git archive {rev} failed")
        trees = {"old": os.path.join(tmp, PKG, "csrc"), "new": B.CSRC}
        jobs = {}
        with ThreadPoolExecutor(max_workers=8) as pool:   # threads only wait on compilers: at most 8 at a time
            for _, bdir, defs in B.VARIANTS:
                for src in B.SOURCES:
                    for side, csrc in trees.items():
                        out = os.path.join(tmp, f"{side}_{bdir}_{src}.s")
                        jobs[side, bdir, src] = pool.submit(emit, csrc, src, defs, out)
        print(f"device assembly (gfx950) of the working tree against {sha}")
        bad = 0
        for _, bdir, defs in B.VARIANTS:
            for src in B.SOURCES:
                old, new = jobs["old", bdir, src].result(), jobs["new", bdir, src].result()
                tag = f"{src:16s} {' '.join(defs) or '(bf16)':12s}"
                if old == new:
                    print(f"{tag} identical  {len(new)} lines")
                    continue
                bad += 1
                n = next((i for i, (a, b) in enumerate(zip(old, new)) if a != b), min(len(old), len(new)))
                print(f"{tag} DIFFERS at line {n + 1} ({len(old)} -> {len(new)} lines)")
                for side, lines in (("-", old), ("+", new)):
                    for line in lines[n:n + 3]:
                        print(f"    {side} {line}")
        total = len(B.VARIANTS) * len(B.SOURCES)
        print(f"{total - bad} of {total} identical")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
