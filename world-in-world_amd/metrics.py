"""Validation frame metrics on the device: per-frame SSIM and PSNR as the reference's training loop logs them
(`evaluate_video_metrics(gt, gen, only_final=True)`, evaluation/FVD/cal_4metrics.py, called from train_svd.py:1176-1187).

The per-plane numbers come from `Hip.frame_metrics` (csrc/metrics.hip: fp64 SSIM on the valid region and the summed squared
error, straight from the frames in HBM); what remains here is the reference's bookkeeping on a few numbers per frame:

  * SSIM of a frame = mean of its three channel planes (calculate_ssim.py:26-41);
  * PSNR of a frame = 20 log10(1 / sqrt(mse)), mse over all 3 H W samples, or 100 when mse < 1e-10 (calculate_psnr.py:6-15);
  * the aggregation of calculate_ssim.py:80-92 / calculate_psnr.py:54-66, which is NOT what the flag's name says:
    `only_final=True` -> ONE mean and ONE population standard deviation over all clips and all frames;
    `only_final=False` -> one (mean, std) pair per frame index, over the clips.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def frame_scores(hip, gt, gen):
    """gt, gen: (B, T, 3, H, W) tensors, each fp32 in [0, 1] or uint8 (a byte u is float32(u) / float32(255), the reference's
    `to_tensor`), moved to `hip.device` if they are not there -> (ssim, psnr), float64 numpy arrays (B, T)."""
    gt, gen = torch.as_tensor(gt), torch.as_tensor(gen)
    assert gt.dim() == 5 and gt.shape == gen.shape, f"shape mismatch: {tuple(gt.shape)} vs {tuple(gen.shape)}"
    B, T, Cc, H, W = gt.shape
    planes = []
    for x in (gt, gen):
        if x.dtype != torch.uint8:
            x = x.to(torch.float32)
        x = x.to(hip.device)
        planes.append(x.contiguous().reshape(B * T * Cc, H, W))
    m = hip.frame_metrics(planes[0], planes[1]).cpu().numpy().reshape(B, T, Cc, 2)          # 16 bytes per plane leave the device
    ssim = m[..., 0].mean(-1)
    mse = m[..., 1].sum(-1) / float(Cc * H * W)
    psnr = np.array([[100.0 if v < 1e-10 else 20 * math.log10(1 / math.sqrt(v)) for v in row] for row in mse], np.float64)
    return ssim, psnr.reshape(B, T)


def aggregate(scores, only_final: bool = False) -> dict:
    """{"value", "value_std"} (lists of floats) of per-frame scores (B, T), as calculate_ssim.py:80-97."""
    s = np.asarray(scores, np.float64)
    assert s.ndim == 2
    if only_final:
        return {"value": [float(np.mean(s))], "value_std": [float(np.std(s))]}
    return {"value": [float(np.mean(s[:, t])) for t in range(s.shape[1])],
            "value_std": [float(np.std(s[:, t])) for t in range(s.shape[1])]}


def _as_videos(frames):
    """cal_4metrics.py:34-43: a (B, T, C, H, W) tensor, or a list of (C, H, W) / (N, C, H, W) / (B, T, C, H, W) tensors."""
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        return torch.as_tensor(frames)
    fs = [torch.as_tensor(f) for f in frames]
    if fs[0].dim() == 3:
        fs = [f.reshape(1, 1, *f.shape) for f in fs]
    elif fs[0].dim() == 4:
        fs = [f.unsqueeze(0) for f in fs]
    return torch.cat(fs, dim=0)


def evaluate_video_metrics(ground_truth_frames, generated_frames, only_final: bool = False, *, hip) -> dict:
    """The reference's `evaluate_video_metrics` for the metrics that need no network:
    {"ssim": {"value", "value_std"}, "psnr": {"value", "value_std"}}, computed on `hip`'s device.

    There is no "lpips" and no "fvd" key: they need the AlexNet / I3D checkpoints, which this tree does not hold (the reference
    itself has its FVD line commented out); a caller that has them adds those entries itself.  The reference's `resize_hw`
    option is not offered (its validation call does not use it).  Values must lie in [0, 1] (uint8 frames do by construction)."""
    gt, gen = _as_videos(ground_truth_frames), _as_videos(generated_frames)
    assert gt.dim() == 5 and gt.shape == gen.shape, f"Shape mismatch: {tuple(gt.shape)} vs {tuple(gen.shape)}"
    for x in (gt, gen):
        assert x.dtype == torch.uint8 or (float(x.min()) >= 0 and float(x.max()) <= 1)
    ssim, psnr = frame_scores(hip, gt, gen)
    return {"ssim": aggregate(ssim, only_final), "psnr": aggregate(psnr, only_final)}
