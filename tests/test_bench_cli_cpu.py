"""bench.py's command line and its --dump-outputs format, without a GPU (the runs themselves: tests/test_gpu_bench.py)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch


@pytest.fixture
def bench(monkeypatch):
    # importing bench.py sets GPU_MAX_HW_QUEUES if it is unset: keep that out of this process's environment
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    return importlib.import_module("bench")


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    assert a.also == "" and a.min_seconds == 0.0 and a.no_single_frame and a.no_cpu_baseline


def test_full_run_keeps_every_leg(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3", "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert a.also == "f32+h16x2,f32,f16" and a.min_seconds == 2.0 and not a.no_single_frame and not a.no_cpu_baseline


def _row(lanes, frames, h, w, seed):
    rng = np.random.default_rng(seed)
    row = []
    for _ in range(lanes):
        t = lambda c: torch.from_numpy(rng.random((frames, h, w, c), dtype=np.float32))
        row.append(dict(rgb=t(3), opacity=t(1), depth=t(1), local_samples=123, total_samples=1000 + len(row)))
    return row


def test_dump_outputs_whole_frames(bench, tmp_path):
    row = _row(2, 3, 8, 5, 0)
    bench.dump_outputs(str(tmp_path), row, 8, 5)
    d = {n: np.load(tmp_path / f"{n}.npy") for n in ("rgb", "opacity", "depth", "pixel_index", "samples_per_call")}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["pixel_index"], np.arange(40.0))
    assert np.array_equal(d["rgb"], np.concatenate([o["rgb"].numpy().reshape(3, 40, 3) for o in row]))
    assert np.array_equal(d["opacity"], np.concatenate([o["opacity"].numpy().reshape(3, 40) for o in row]))
    assert np.array_equal(d["depth"], np.concatenate([o["depth"].numpy().reshape(3, 40) for o in row]))
    assert np.array_equal(d["samples_per_call"], [1000.0, 1001.0])


def test_dump_outputs_seeded_sample_within_budget(bench, monkeypatch, tmp_path):
    row = _row(3, 4, 32, 16, 1)
    monkeypatch.setattr(bench, "DUMP_BYTES", 12 * 5 * 4 * 100)          # room for 100 pixels of each of the 12 frames
    bench.dump_outputs(str(tmp_path / "a"), row, 32, 16)
    bench.dump_outputs(str(tmp_path / "b"), row, 32, 16)
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.shape == (100,) and np.all(np.diff(idx) > 0) and idx.max() < 512
    assert np.array_equal(idx, np.load(tmp_path / "b" / "pixel_index.npy"))          # the same sample every run
    rgb = np.load(tmp_path / "a" / "rgb.npy")
    want = np.concatenate([o["rgb"].numpy().reshape(4, 512, 3) for o in row])[:, idx.astype(np.int64)]
    assert rgb.shape == (12, 100, 3) and np.array_equal(rgb, want)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES + 100 * 8 + 4096


def test_dump_budget_holds_for_the_default_workload(bench):
    frames, pixels = 3 * 16, 800 * 800                                  # lanes x frames per call of an 800x800 step
    keep = bench.DUMP_BYTES // (frames * 5 * 4)
    assert keep < pixels and frames * keep * 5 * 4 + keep * 8 + 5 * 4096 <= 64e6
