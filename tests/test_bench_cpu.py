"""bench.py's --dump-outputs helpers on the CPU: the seeded sample that large outputs are cut to."""
import numpy as np


def test_dump_sample_keeps_small_arrays_whole():
    import torch

    import bench

    t = torch.arange(12, dtype=torch.uint8).reshape(3, 4)
    got = bench.dump_sample(t, 12, 7)
    assert got.dtype == np.float32 and np.array_equal(got, np.arange(12, dtype=np.float32))


def test_dump_sample_is_seeded_sorted_and_capped():
    import torch

    import bench

    n, cap = 1000, 64
    t = torch.arange(n, dtype=torch.float32) * 0.5  # value = index / 2: the sample shows its indices
    a = bench.dump_sample(t, cap, 1984)
    assert a.dtype == np.float32 and a.shape == (cap,)
    assert np.array_equal(a, bench.dump_sample(t.clone(), cap, 1984))  # same seed, same elements
    idx = a * 2
    assert np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < n and np.array_equal(idx, idx.astype(np.int64))
    assert len(np.unique(idx)) > cap // 2  # spread over the array, not one element repeated
    assert not np.array_equal(a, bench.dump_sample(t, cap, 1985))  # fb.npy and image.npy use different seeds


def test_dump_outputs_writes_the_three_arrays(tmp_path, monkeypatch):
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_FB_ELEMS", 100)
    monkeypatch.setattr(bench, "DUMP_IMAGE_ELEMS", 50)
    fb = torch.rand(1000, generator=torch.Generator().manual_seed(1))
    image = torch.arange(60, dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path / "d"), fb, image, 12345)
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("fb", "image", "segments")}
    assert got["fb"].shape == (100,) and got["image"].shape == (50,) and got["fb"].dtype == got["image"].dtype == np.float32
    assert set(got["fb"].tolist()) <= set(fb.numpy().tolist()) and set(got["image"].tolist()) <= set(range(60))
    assert got["segments"].dtype == np.float64 and got["segments"].tolist() == [12345.0]
