"""bench.py's plain run and ``--dump-outputs``: the arrays written are what the last timed
``sampler()`` call returned, as float32 / float64, capped in size by a fixed seeded row sample; the
plain line carries the headline fields and none of the ``--full`` blocks."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _outputs(B=12, T=5):
    g = torch.Generator().manual_seed(0)
    return {"ids": torch.randint(0, 10123, (B, T), generator=g),
            "alpha": torch.rand(B, T, 49, generator=g), "beta": torch.rand(B, T, 1, generator=g)}


def test_dump_outputs_writes_every_array(tmp_path):
    o = _outputs()
    bench.dump_outputs(str(tmp_path / "d"), o)
    assert sorted(os.listdir(tmp_path / "d")) == ["alpha.npy", "beta.npy", "ids.npy"]
    ids = np.load(tmp_path / "d" / "ids.npy")
    assert ids.dtype == np.float64 and np.array_equal(ids, o["ids"].numpy())
    for k in ("alpha", "beta"):
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, o[k].numpy())


def test_dump_outputs_caps_the_size_with_a_fixed_row_sample(tmp_path, monkeypatch):
    o = _outputs(B=64)
    full = sum(t.numel() * (8 if t.dtype == torch.int64 else 4) for t in o.values())
    monkeypatch.setattr(bench, "DUMP_BYTES", full // 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), o)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 6
    written = 0
    for k in ("ids", "alpha", "beta"):
        a, rows = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "a" / f"{k}_rows.npy").astype(np.int64)
        written += a.nbytes + rows.nbytes
        assert 0 < len(rows) < 64 and np.all(np.diff(rows) > 0)
        assert np.array_equal(a, o[k].numpy()[rows])
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))  # the same rows in every run
    assert written <= full // 3


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys, gpu_device):
    from adaptive_amd import Config, Encoder2Decoder
    from adaptive_amd.adaptive_attention import synthetic_features
    B, T, K = 24, 6, 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", "1", "--batch", str(B),
                                      "--max-len", str(T), "--dump-outputs", str(tmp_path / "d")])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "captions/s" and d["higher_is_better"] is True
    assert d["dtype"] == "fp32" and d["steps"] == K and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(B / (d["ms_per_step"] * 1e-3))
    for k in ("eval_loop", "pipelined", "kernels", "roofline", "cpu_baseline"):
        assert k not in d
    # the last timed step (k = K - 1) decodes feature buffer (K - 1) % 3, generated from that seed
    model = Encoder2Decoder(Config()).to(gpu_device).load_synthetic(123)
    ids, alpha, beta = model.sampler(synthetic_features(B, gpu_device, seed=(K - 1) % 3), max_len=T)
    assert np.array_equal(np.load(tmp_path / "d" / "ids.npy"), ids.cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "alpha.npy"), alpha.cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "beta.npy"), beta.cpu().numpy())
