"""Validation frame metrics of one 576x1024x14 clip pair: the device path (`metrics.frame_scores` on `Hip.frame_metrics`,
csrc/metrics.hip) against the same numbers on the host (the fp64 numpy restatement of tests/metrics_fixtures.py, the separable
form of the reference's five float64 filter2D passes per plane), in one process, with the bytes that cross PCIe in each case.

The decoded clip is fp32 (14, 3, 576, 1024) on the device, as `VAEHIP.decode` leaves it; the ground truth is uint8 on the host, as a
data loader holds it.  Device path: quantise the clip on the device, upload the ground-truth bytes, two launches, 16 bytes per
plane back.  Host path: the fp32 clip goes to the host first (what `Trainer.validate` does for its "psnr" key).

    python tools/metrics_probe.py [--frames 14] [--height 576] [--width 1024] [--iters 10] [--host-planes 6]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-planes", type=int, default=6, help="planes the host restatement is timed on (scaled to the clip); 0 = all")
    args = ap.parse_args()

    import metrics_fixtures as MF
    import wiw_amd  # noqa: F401
    from wiw_amd.hip import Hip
    from wiw_amd.metrics import frame_scores
    from wiw_amd.vae import frames_to_uint8_device

    dev = torch.device("cuda:0")
    hip = Hip(dev)
    T, H, W = args.frames, args.height, args.width
    N = T * 3
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:H, 0:W]
    base = 127.5 + 90.0 * np.sin(0.011 * y + 0.007 * x)
    gt_u8 = np.clip(base[None, None] + rs.randint(-20, 21, size=(T, 3, H, W)), 0, 255).astype(np.uint8)
    clip = torch.from_numpy((np.clip(base[None, None] + rs.randint(-30, 31, size=(T, 3, H, W)), -10, 265) / 127.5 - 1.0).astype(np.float32)).to(dev)

    def device_path():
        gen = frames_to_uint8_device(clip).permute(0, 3, 1, 2)[None]
        return frame_scores(hip, torch.from_numpy(gt_u8)[None], gen)

    def kernels_only(a, b):
        return hip.frame_metrics(a, b)

    ssim_d, psnr_d = device_path()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        device_path()                      # ends with the read of the (N, 2) result: synchronous
    t_dev = (time.perf_counter() - t0) / args.iters
    a = torch.from_numpy(gt_u8.reshape(N, H, W)).to(dev)
    b = frames_to_uint8_device(clip).permute(0, 3, 1, 2).contiguous().reshape(N, H, W)
    kernels_only(a, b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        kernels_only(a, b)
    e1.record()
    torch.cuda.synchronize()
    t_k = e0.elapsed_time(e1) / args.iters * 1e-3

    # host path: the fp32 clip crosses PCIe, is quantised there, and every plane goes through the fp64 restatement
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_clip = clip.cpu()
    t_copy = time.perf_counter() - t0
    q = frames_to_uint8_device(host_clip).permute(0, 3, 1, 2).contiguous().numpy()
    n_host = N if args.host_planes <= 0 else min(N, args.host_planes)
    t0 = time.perf_counter()
    ref = MF.planes_metrics(gt_u8.reshape(N, H, W)[:n_host], q.reshape(N, H, W)[:n_host])
    t_host = (time.perf_counter() - t0) * N / n_host
    got = kernels_only(a, b).cpu().numpy()
    d_ssim = np.abs(got[:n_host, 0] - ref[:, 0]).max()
    d_psnr = max(abs(MF.psnr_of(g, H * W) - MF.psnr_of(r, H * W)) for g, r in zip(got[:n_host, 1], ref[:, 1]))

    print(f"clip pair {T} x 3 x {H} x {W} = {N} planes; mean SSIM {ssim_d.mean():.6f}, mean PSNR {psnr_d.mean():.4f} dB")
    print(f"device path (quantise + upload of the uint8 ground truth + 2 launches + read-back): {t_dev * 1e3:9.3f} ms per clip pair")
    print(f"  of which the two launches of wiw_frame_metrics (uint8 / uint8):                   {t_k * 1e3:9.3f} ms "
          f"({2 * N * H * W / t_k / 1e9:.1f} GB/s of operand bytes, {N * H * W / t_k / 1e9:.2f} Gpixel/s)")
    print(f"host path   (fp32 clip to the host {t_copy * 1e3:.1f} ms + fp64 numpy restatement, {n_host} of {N} planes timed, scaled): "
          f"{(t_copy + t_host) * 1e3:9.1f} ms per clip pair")
    print(f"bytes over PCIe, device path: {gt_u8.nbytes} up (uint8 ground truth) + {N * 16} down (two doubles per plane)")
    print(f"bytes over PCIe, host path:   {clip.numel() * 4} down (the fp32 clip)")
    print(f"device vs host restatement on the {n_host} timed planes: max |ssim| diff {d_ssim:.3e}, max |psnr| diff {d_psnr:.3e} dB")


if __name__ == "__main__":
    main()
