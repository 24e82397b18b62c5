"""bench.py's command line and --dump-outputs writer (CPU only: the writer is fed host tensors whose values are
their global row numbers, so what it wrote can be checked row by row)."""
import os
import sys

import numpy as np
import pytest


def _bench(monkeypatch, argv=()):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    import bench
    return bench


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    b = _bench(monkeypatch)
    a = b.parse()
    assert a.full is False and a.dump_outputs is None
    a = _bench(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "d"]).parse()
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 2


def _rows_as_outputs(lo, hi, n=7):
    import torch
    r = torch.arange(lo, hi, dtype=torch.float32)
    return r[:, None].repeat(1, n), r[:, None, None].repeat(1, n, 2 * n)


@pytest.mark.parametrize("B", [4096, 1 << 20])
def test_dump_outputs_writes_a_fixed_bounded_row_sample(monkeypatch, tmp_path, B):
    b = _bench(monkeypatch)
    got = []
    for k in range(2):
        d = str(tmp_path / f"d{k}")
        info = b.dump_outputs(d, _rows_as_outputs(0, B), B, 0, None, 0)
        assert info["arrays"]["c"][0] == info["arrays"]["dc_du"][0]
        c, dc = np.load(os.path.join(d, "c.npy")), np.load(os.path.join(d, "dc_du.npy"))
        assert c.dtype == np.float32 and dc.dtype == np.float32 and dc.shape[1:] == (7, 14)
        assert os.path.getsize(os.path.join(d, "c.npy")) + os.path.getsize(os.path.join(d, "dc_du.npy")) <= 64 * 10**6
        rows = c[:, 0].astype(np.int64)
        assert np.all(np.diff(rows) > 0) and np.all(dc == rows[:, None, None])
        got.append(rows)
    assert np.array_equal(got[0], got[1])                       # the same rows in every run
    assert len(got[0]) == (B if B == 4096 else b.DUMP_ROWS)     # all rows while they fit, else the sample
