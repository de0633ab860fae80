"""bench.py's command line: a plain run carries the headline figure and what the timed steps recorded, --full adds what takes
runs of its own, --dump-outputs writes the last timed step's outputs (float32 / float64, seeded row sample, <= 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("stages_s", "encoder", "cpu_baseline", "auroc_check", "product_default_text_dedup", "value_f32_gemm_mode",
             "encoder_f32_gemm_mode", "gemm_by_tower", "mscoco", "knn_1m")
SMALL = ["--arch", "tiny", "--n_train", "1500", "--n_val", "200", "--n_test", "200", "--knn_k", "5", "--encoder_batch", "256"]


def test_full_and_dump_outputs_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "/x/y"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "/x/y"


def test_dump_outputs_dtypes_sampling_and_budget(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"score": torch.rand(100_000, dtype=torch.float64, generator=g), "d_1": torch.rand(300, generator=g),
              "emb": torch.randn(5000, 16, generator=g), "I_n": torch.randint(0, 5000, (5000, 4), generator=g),
              "half": torch.randn(7, 3, generator=g).half()}
    total = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert total <= bench.DUMP_MAX_BYTES
    ld = lambda d, n: np.load(tmp_path / d / f"{n}.npy")
    assert ld("a", "score").dtype == np.float64 and ld("a", "score").shape == (bench.DUMP_ROWS_1D,)
    rows = ld("a", "score_rows")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
    assert np.array_equal(ld("a", "score"), arrays["score"].numpy()[rows.astype(np.int64)])
    assert ld("a", "d_1").dtype == np.float32 and np.array_equal(ld("a", "d_1"), arrays["d_1"].numpy())      # small: every row
    assert not os.path.exists(tmp_path / "a" / "d_1_rows.npy")
    er = ld("a", "emb_rows").astype(np.int64)
    assert ld("a", "emb").shape == (bench.DUMP_ROWS_ND, 16) and np.array_equal(ld("a", "emb"), arrays["emb"].numpy()[er])
    assert ld("a", "I_n").dtype == np.float64 and np.array_equal(ld("a", "I_n"), arrays["I_n"].numpy()[er].astype(np.float64))
    assert ld("a", "half").dtype == np.float32
    # the same outputs give the same files: the sample is fixed, not drawn per run
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), {f"m{i}": torch.zeros(1024, 4096) for i in range(5)})


def _run(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(hip, tmp_path):
    line = _run(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)] + SMALL, 600)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in line, key
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in line]
    for split, n in (("train", 1500), ("val", 200), ("test", 200)):
        s = np.load(tmp_path / f"{split}_score.npy")
        assert s.dtype == np.float64 and s.shape == (n,) and np.isfinite(s).all()
        e = np.load(tmp_path / f"{split}_emb_img.npy")
        assert e.dtype == np.float32 and e.shape == (min(n, bench.DUMP_ROWS_ND), 32)
        assert np.allclose(np.linalg.norm(e, axis=1), 1.0, atol=1e-5)
        i_n = np.load(tmp_path / f"{split}_I_n.npy")
        assert i_n.shape[1] == 5 and (i_n >= 0).all() and (i_n < 1500).all() and np.array_equal(i_n, np.round(i_n))
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= bench.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_full_run_keeps_the_extras(hip):
    line = _run(["--steps", "1", "--warmup", "1", "--full", "--no_knn_1m", "--no_mscoco"] + SMALL, 900)
    for key in ("stages_s", "encoder", "cpu_baseline", "auroc_check", "product_default_text_dedup", "value_f32_gemm_mode"):
        assert key in line, key
    assert line["auroc_check"]["topk_sets_identical"] and line["auroc_check"]["per_sample_arrays_bit_exact"]
