#!/usr/bin/env python3
"""HIP-event timings of rbd_second_order_idsva C-ABI launches (pre-allocated output, warm clock: 50 ms of the same
launches first).

    python tools/time_so.py            # the rows of DESIGN.md §4.9, fp32 and fp64
Run it under a time limit (timeout -k 10 300 ...).  Prints one line per (robot, B, precision): time, bytes written
(the [B, 4, n, n, n] output; the inputs are 3n scalars per row on top), the rate they imply and its fraction of 8 TB/s.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import make_robot  # noqa: E402
from rbdreference_amd import RBDReference  # noqa: E402

ROWS = [("iiwa_like", 65536), ("quadruped_like", 16384), ("atlas_like", 1024)]
PEAK_TBS = 8.0


def timed(fn, iters=50):
    t0 = time.time()
    while time.time() - t0 < 0.05:
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


def main():
    for name, B in ROWS:
        rbd = RBDReference(make_robot(name), build=False)
        n = rbd.n
        for dt in (torch.float32, torch.float64):
            esz = 4 if dt == torch.float32 else 8
            q, qd, qdd = ((torch.rand((B, n), device="cuda", dtype=torch.float64) * 2 - 1).to(dt) for _ in range(3))
            out = torch.empty((B, 4, n, n, n), device="cuda", dtype=dt)
            fn = rbd._fn("rbd_second_order_idsva", dt)
            st = torch.cuda.current_stream().cuda_stream
            args = (q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), -9.81, B, out.data_ptr(), st)
            rc = fn(*args)
            assert rc == 0, rbd._lib.check(rc)
            us = timed(lambda: fn(*args))
            by = B * 4 * n ** 3 * esz
            tbs = by / us / 1e6
            print(f"{name:15s} B={B:6d} {'fp32' if esz == 4 else 'fp64'}: {us:9.2f} us  {by / 1e6:8.1f} MB written  "
                  f"{tbs:5.2f} TB/s  {tbs / PEAK_TBS:5.1%} of {PEAK_TBS:.0f} TB/s", flush=True)


if __name__ == "__main__":
    main()
