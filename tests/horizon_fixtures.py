"""Loader of the fixtures that tools/make_golden_horizon.py writes in parts (`<stem>.part0.npz`, `.part1.npz`, ...: no file of
the repository is larger than 1 MiB): one mapping with the arrays of every part."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_parts(stem):
    paths = sorted(glob.glob(os.path.join(GOLDEN, stem + ".part*.npz")))
    if not paths:
        raise FileNotFoundError(f"no parts of {stem} under {GOLDEN}: run tools/make_golden_horizon.py in the build container")
    out = {}
    for p in paths:
        with np.load(p, allow_pickle=False) as g:
            for k in g.files:
                assert k not in out, f"{k} appears in two parts of {stem}"
                out[k] = g[k]
    return out
