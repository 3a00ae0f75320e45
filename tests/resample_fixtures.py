"""Shared inputs and references of the image-resampling tests (tests/test_resample.py, tests/test_hip_resample*.py): seeded
uint8 planes with saturated bands, and `PIL.Image.resize` of them — computed once per geometry and never modified."""
import functools

import numpy as np
from PIL import Image

PIL_FILTER = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}

# (filter, H, W, ow, oh): the geometries `resample_reference` was found bit-equal to Pillow on
GEOMETRIES = [
    ("bicubic", 576, 1024, 480, 480),        # the served output resize
    ("bicubic", 448, 448, 480, 480),         # manipulation: both sides up
    ("bicubic", 64, 64, 48, 80),
    ("bicubic", 37, 53, 64, 64),             # odd sizes, both sides up
    ("bicubic", 64, 128, 64, 48),            # both sides down
    ("lanczos", 600, 800, 1024, 576),        # the served input resize
    ("lanczos", 512, 512, 448, 448),
    ("lanczos", 100, 90, 64, 128),
]
# one side unchanged: that pass is SKIPPED, as Pillow skips it
ONE_SIDED = [
    ("bicubic", 64, 128, 64, 64),            # height kept
    ("bicubic", 48, 40, 40, 96),             # width kept
]


@functools.lru_cache(maxsize=None)
def planes(H, W, N=1, seed=0):
    """Seeded random uint8 (N, H, W) with 8-row bands of 0 and of 255 every 24 rows: the overshoot clamp of both filters is hit."""
    a = np.random.RandomState(1000 * seed + H * 31 + W).randint(0, 256, size=(N, H, W), dtype=np.uint8)
    for y in range(0, H, 24):
        a[:, y:y + 8] = 0
        a[:, y + 8:y + 16] = 255
    a.setflags(write=False)
    return a


def pil_resize(a, ow, oh, filter):
    """`Image.resize((ow, oh), filter)` of every plane of uint8 (N, H, W)."""
    return np.stack([np.asarray(Image.fromarray(p).resize((ow, oh), PIL_FILTER[filter])) for p in a])


@functools.lru_cache(maxsize=None)
def pil_reference(filter, H, W, ow, oh, N=1, seed=0):
    out = pil_resize(planes(H, W, N, seed), ow, oh, filter)
    out.setflags(write=False)
    return out


def case_id(c):
    return "{}-{}x{}-to-{}x{}".format(*c)
