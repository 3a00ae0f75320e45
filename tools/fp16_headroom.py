"""How close does every 16-bit activation tensor of a checkpoint sit to its storage type's largest finite value?

One seeded request through the worker `serve_worker.py` builds from the same model arguments, launched EAGERLY for --steps
Euler steps with a `range.RangeProbe` attached: every operator called by `UNetHIP.forward`, the VAE encoder / decoder and the
CLIP encoder records `wiw_range_stats` (csrc/range.hip) of the activation tensor it wrote — counts of NaN / inf / zero / hot /
tiny elements, absmax, absmin and the 64-bin histogram of floor(log2 |x|) — under the module path it runs in.  The records
are read once, at the end; the probed request computes what the unprobed one computes, bit for bit.

Printed: the tensors sorted by headroom = largest finite value of the storage type / absmax (0 for a tensor that holds an
inf), every tensor with a NaN or an inf in launch order (the first one is where it starts), and the share of tiny elements
(below the smallest normal: precision already lost).  --out: the whole record set as JSON (an infinite value is null).

    python tools/fp16_headroom.py --random_weights [--steps 2] [--candidates 1] [--top 30] [--out headroom.json]
    python tools/fp16_headroom.py --unet_path <checkpoint dir> --svd_path <stable-video-diffusion-img2vid-xt> --out headroom.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import serve_worker  # noqa: E402


def probe_request(worker, probe, candidates: int, seed: int = 0):
    """Attach `probe` to the worker's library for one seeded request; -> the records."""
    hip = worker.frontend.vae.hip
    rs = np.random.RandomState(seed)
    T = worker.num_frames
    req = {"b_action": np.array([[4] + [1] * (T - 1)] * candidates, dtype=np.int64) if worker.task_type == "navigation"
           else np.tile(np.array([0.1, 0.0, 0.2, 0.0, 0.0, 0.0, 1.0, 1.0]), (candidates, T, 1)),
           "save_dirs": [f"unused-{j}" for j in range(candidates)], "request_model_name": worker.world_model_name,
           "b_image": rs.randint(0, 256, size=(candidates, 3, worker.height, worker.width), dtype=np.uint8),
           "return_objects": [True] * candidates}
    hip.range_probe = probe
    try:
        worker(req)
        return probe.records()
    finally:
        hip.range_probe = None


def summarise(records, top: int = 30, file=sys.stdout):
    def line(r):
        n = int(np.prod(r["shape"]))
        return (f"{r['headroom']:12.4g}  {r['absmax']:11.4g}  {r['n_inf']:9d} {r['n_nan']:9d}  {100.0 * r['n_hot'] / n:7.3f}% "
                f"{100.0 * r['n_tiny'] / n:7.3f}%  {r['dtype']:8s} {r['family']:16s} {r['scope']}#{r['ordinal']} {list(r['shape'])}")
    head = f"{'headroom':>12s}  {'absmax':>11s}  {'inf':>9s} {'NaN':>9s}  {'hot':>8s} {'tiny':>8s}  dtype    family           scope#ordinal shape"
    order = sorted(range(len(records)), key=lambda i: (records[i]["headroom"], i))
    print(f"[headroom] {len(records)} tensors; lowest headroom first", file=file)
    print(head, file=file)
    for i in order[:top]:
        print(line(records[i]), file=file)
    bad = [r for r in records if r["n_inf"] + r["n_nan"]]
    print(f"[headroom] {len(bad)} tensor(s) with inf or NaN" + (", in launch order:" if bad else ""), file=file)
    for r in bad:
        print(line(r), file=file)
    total = sum(int(np.prod(r["shape"])) for r in records)
    print(f"[headroom] tiny elements (finite, below the smallest normal of the storage type): "
          f"{100.0 * sum(r['n_tiny'] for r in records) / max(total, 1):.4f}% of {total} recorded elements; worst tensors:", file=file)
    for r in sorted(records, key=lambda r: -r["n_tiny"] / max(int(np.prod(r["shape"])), 1))[:5]:
        print(line(r), file=file)


def to_json(records):
    """The records as strict JSON values: arrays and tuples as lists, an infinite `headroom` / `absmin` (a tensor without a
    non-zero finite element) as null."""
    def value(v):
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, tuple):
            return list(v)
        if isinstance(v, float) and not np.isfinite(v):
            return None
        return v
    return [{k: value(v) for k, v in r.items()} for r in records]


def main(argv=None):
    ap = serve_worker.arg_parser()
    ap.description = __doc__.split("\n")[0]
    ap.add_argument("--steps", type=int, default=2, help="Euler steps of the probed request")
    ap.add_argument("--candidates", type=int, default=1)
    ap.add_argument("--top", type=int, default=30, help="rows of the headroom table")
    ap.add_argument("--out", type=str, default="", help="write every record (statistics and histogram) as JSON")
    args = ap.parse_args(argv)
    args.num_inference_steps, args.hip_graph, args.finite_guard = args.steps, False, "off"          # eager: a capture refuses the probe
    from wiw_amd.range import RangeProbe

    worker = serve_worker.build_worker(args)
    records = probe_request(worker, RangeProbe(), args.candidates)
    torch.cuda.synchronize()
    summarise(records, args.top)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(to_json(records), f, allow_nan=False)
        print(f"[headroom] {len(records)} records -> {args.out}")


if __name__ == "__main__":
    main()
