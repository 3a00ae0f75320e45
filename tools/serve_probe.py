"""Phase timing of one full-size request through the launcher's worker (random-init weights).
usage: python tools/serve_probe.py [n_requests] [candidates] [--device_resize] [--finite_guard=off|error|fallback]

Rows per request: frontend.encode (CLIP + VAE encoder; with --device_resize also the upload of the bytes and the LANCZOS
resize), denoise, vae.decode (summed over the candidates), and post-decode = everything between the end of the loop and the
response that is not vae.decode: frame quantisation, device-to-host copy, the BICUBIC resize (PIL on the host, or
csrc/resample.hip with --device_resize) and the response."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import serve_worker  # noqa: E402


def main():
    guard = [a for a in sys.argv[1:] if a.startswith("--finite_guard=")]          # the worker's finite guard (off by default)
    argv = [a for a in sys.argv[1:] if a != "--device_resize" and a not in guard]
    device_resize = "--device_resize" in sys.argv[1:]
    nreq = int(argv[0]) if len(argv) > 0 else 2
    B = int(argv[1]) if len(argv) > 1 else 1
    t0 = time.time()
    args = serve_worker.arg_parser().parse_args(["--random_weights", "--num_inference_steps", "2", "--port", "1"] +
                                                (["--device_resize"] if device_resize else []) + guard)
    w = serve_worker.build_worker(args)
    torch.cuda.synchronize()
    print(f"[probe] build_worker {time.time() - t0:.1f}s  device_resize={getattr(w, 'device_resize', False)}", flush=True)
    fe, den = w.frontend, w.denoise_fn
    spent = {}

    def timed(name, fn, quiet=False):
        def g(*a, **k):
            torch.cuda.synchronize(); t = time.time()
            r = fn(*a, **k)
            torch.cuda.synchronize(); dt = time.time() - t
            spent[name] = spent.get(name, 0.0) + dt
            spent["_end_" + name] = time.time()
            if not quiet:
                print(f"[probe]   {name}: {dt:.2f}s", flush=True)
            return r
        return g
    fe.encode = timed("frontend.encode", fe.encode)
    if hasattr(fe, "encode_uint8"):
        fe.encode_uint8 = timed("frontend.encode", fe.encode_uint8)
    w.denoise_fn = timed("denoise(2 steps)", den)
    fe.vae.decode = timed("vae.decode", fe.vae.decode, quiet=True)
    rs = np.random.RandomState(0)
    for i in range(nreq):
        req = {"b_action": np.array([[4] + [1] * 13] * B, dtype=np.int64), "save_dirs": [f"/tmp/p{i}_{j}" for j in range(B)],
               "request_model_name": "igen", "b_image": rs.randint(0, 256, size=(B, 3, 576, 1024), dtype=np.uint8),
               "return_objects": [True] * B}
        spent.clear()
        t = time.time()
        out = w(req)
        end = time.time()
        dec = spent.get("vae.decode", 0.0)
        print(f"[probe]   vae.decode (x{B}): {dec:.2f}s", flush=True)
        print(f"[probe]   post-decode (quantise + D2H + resize + response): {end - spent['_end_denoise(2 steps)'] - dec:.3f}s", flush=True)
        print(f"[probe] request {i}: {end - t:.2f}s  pred_frames {out['pred_frames'].shape}", flush=True)


if __name__ == "__main__":
    main()
