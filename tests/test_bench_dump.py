"""`bench.py --dump-outputs`: what it writes (names, dtypes, the size budget and its fixed sample) without a GPU."""
import numpy as np

import bench


def test_dump_outputs_writes_float_arrays(tmp_path):
    lat = np.arange(24, dtype=np.float16).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "out"), {"latents": lat, "loss": np.array([0.25], dtype=np.float64)})
    got = np.load(tmp_path / "out" / "latents.npy")
    assert got.dtype == np.float32 and got.shape == lat.shape and (got == lat.astype(np.float32)).all()
    loss = np.load(tmp_path / "out" / "loss.npy")
    assert loss.dtype == np.float64 and loss[0] == 0.25


def test_dump_outputs_samples_what_exceeds_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 400)
    big = np.arange(1000, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"latents": big})
    a, b = np.load(tmp_path / "a" / "latents_sample.npy"), np.load(tmp_path / "b" / "latents_sample.npy")
    assert a.dtype == np.float32 and a.nbytes == 400 and (a == b).all()      # fixed sample: same elements every run
    assert (np.diff(a) > 0).all() and np.isin(a, big).all()
    assert not (tmp_path / "a" / "latents.npy").exists()
