#!/usr/bin/env python
"""Generate tests/golden/unet_tiny_tails_24x40.npz by RUNNING THE REFERENCE UNet at a latent whose inner token counts are
not multiples of 8 (build container only, like oracle/make_golden.py, whose helpers it imports).

Latent 24x40: the four UNet levels are 24x40, 12x20, 6x10 and 3x5, i.e. S = 960, 240, 60 and 15 tokens — tails of 4 and 7
at the two inner levels (the frame-padded V^T path of the spatial attention).  Tiny UNet (UNetConfig.tiny(4),
weights seed 0), B = 1 with CFG: inputs, the fp32 reference output and the reference's own bf16 run.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_tails.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _ref_import import import_reference  # noqa: E402
from make_golden import ref_unet, save, unet_inputs  # noqa: E402
from wiw_amd.config import UNetConfig  # noqa: E402

H, W = 24, 40
TIMESTEP = 1.0640485   # sigma_8 of the 10-step table, as in unet_tiny_b1.npz


def main():
    torch.manual_seed(0)
    ns = import_reference()
    cfg = UNetConfig.tiny(4)
    sample, ehs, tids, acts = unet_inputs(cfg, 1, H, W, seed=5)
    aid = ns.get_action_ids(1, torch.from_numpy(acts), "micro_cond", torch.float32)
    m = ref_unet(ns, cfg, seed=0)
    with torch.no_grad():
        out = m(torch.from_numpy(sample), torch.tensor(TIMESTEP), torch.from_numpy(ehs), torch.from_numpy(tids),
                return_dict=False, added_action_ids=aid)[0]
    mb = ref_unet(ns, cfg, seed=0).to(torch.bfloat16)
    with torch.no_grad():
        out_bf16 = mb(torch.from_numpy(sample).bfloat16(), torch.tensor(TIMESTEP), torch.from_numpy(ehs).bfloat16(),
                      torch.from_numpy(tids).bfloat16(), return_dict=False, added_action_ids=aid.bfloat16())[0]
    save(f"unet_tiny_tails_{H}x{W}.npz", weight_seed=np.array(0), timestep=np.array(TIMESTEP, dtype=np.float32), sample=sample,
         ehs=ehs, added_time_ids=tids, actions=acts, action_ids=aid.numpy(), out=out.numpy(),
         out_ref_bf16=out_bf16.float().numpy())


if __name__ == "__main__":
    main()
