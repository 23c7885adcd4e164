"""bench.py --dump-outputs (CPU): the files hold the frame it is given, as float32, whole up to
the pixel cap and as the same fixed sample of the pixels from run to run above it."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _frame(h, w):
    rng = np.random.default_rng(7)
    return rng.random((h, w, 3), dtype=np.float32), rng.integers(1, 1025, (h, w)).astype(np.int32)


def test_small_frame_is_written_whole(tmp_path):
    rgb, cnt = _frame(37, 53)
    bench.dump_outputs(str(tmp_path / "out"), rgb, cnt)
    assert sorted(os.listdir(tmp_path / "out")) == ["count.npy", "rgb.npy"]
    got_rgb, got_cnt = np.load(tmp_path / "out" / "rgb.npy"), np.load(tmp_path / "out" / "count.npy")
    assert got_rgb.dtype == np.float32 and got_cnt.dtype == np.float32
    assert np.array_equal(got_rgb.view(np.uint32), rgb.view(np.uint32))
    assert np.array_equal(got_cnt, cnt)


def test_large_frame_is_the_same_sample_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 500)
    rgb, cnt = _frame(37, 53)
    bench.dump_outputs(str(tmp_path / "a"), rgb, cnt)
    bench.dump_outputs(str(tmp_path / "b"), rgb.copy(), cnt.copy())
    a_rgb, a_cnt = np.load(tmp_path / "a" / "rgb.npy"), np.load(tmp_path / "a" / "count.npy")
    assert a_rgb.shape == (500, 3) and a_cnt.shape == (500,)
    assert np.array_equal(a_rgb, np.load(tmp_path / "b" / "rgb.npy"))
    assert np.array_equal(a_cnt, np.load(tmp_path / "b" / "count.npy"))
    # every sampled pixel is a pixel of the frame, radiance and count taken from the same one
    flat = {tuple(p.view(np.uint32)): c for p, c in zip(rgb.reshape(-1, 3), cnt.reshape(-1))}
    assert all(flat[tuple(p.view(np.uint32))] == c for p, c in zip(a_rgb, a_cnt))


def test_the_pixel_cap_keeps_the_files_under_the_size_limit():
    assert bench.DUMP_MAX_PIXELS * 16 <= 64 * 10 ** 6 and 1920 * 1080 <= bench.DUMP_MAX_PIXELS
