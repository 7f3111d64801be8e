"""CPU: bench.py's command line and its --dump-outputs writer (no GPU: the writer is fed CPU tensors)."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_default_and_steps_must_be_positive(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path):
    """The S1M-1080p step's arrays: small ones whole and in shape, large ones as the same seeded sample in every run,
    float32 (float64 kept), None skipped, 64 MB in all."""
    bench = _bench()
    P, H, W = 1_000_000, 1080, 1920
    g = torch.Generator().manual_seed(0)
    arrays = dict(color=torch.rand(9, H, W, generator=g), alpha=torch.rand(1, H, W, generator=g),
                  radii=torch.randint(0, 60, (P,), dtype=torch.int32, generator=g),
                  grad_opacities=torch.rand(P, 1, generator=g), grad_shs=torch.rand(P, 16, 3, generator=g),
                  grad_f64=torch.rand(P, 3, generator=g, dtype=torch.float64), grad_means2D=None)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(glob.glob(str(tmp_path / "a" / "*.npy")))
    assert [os.path.basename(f)[:-4] for f in files] == sorted(k for k, v in arrays.items() if v is not None)
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(f), np.load(f.replace(os.sep + "a" + os.sep, os.sep + "b" + os.sep))
        assert a.dtype == (np.float64 if "f64" in f else np.float32)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "radii.npy"), arrays["radii"].numpy().astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "grad_opacities.npy"), arrays["grad_opacities"].numpy())
    col = np.load(tmp_path / "a" / "color.npy")
    assert col.ndim == 1 and 0 < col.size < arrays["color"].numel()
    assert np.isin(col, arrays["color"].numpy().reshape(-1)).all()          # elements of the output, not new values
