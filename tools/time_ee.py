#!/usr/bin/env python3
"""HIP-event timings of rbd_ee_pose C-ABI launches (pre-allocated outputs, warm clock: 50 ms of the same launches first).

    python tools/time_ee.py            # the rows of DESIGN.md §4.8, fp32 and fp64
Run it under a time limit (timeout -k 10 300 ...).  Prints one line per (robot, B, sites, outputs, precision): time,
algorithmic bytes (q in, outputs out) and the rate they imply.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ee_oracle import ee_robot  # noqa: E402
from rbdreference_amd import RBDReference  # noqa: E402

ROWS = [("iiwa_like", 1 << 20), ("atlas_like", 16384), ("quadruped_like", 65536)]


def timed(fn, iters=100):
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
        rbd = RBDReference(ee_robot(name), build=False)
        n = rbd.n
        chunks, off, ns = rbd._ee_plan(None, [np.matrix([[0, 0, 0, 1]])])
        body, T = chunks[0]
        for dt in (torch.float32, torch.float64):
            esz = 4 if dt == torch.float32 else 8
            q = (torch.rand((B, n), device="cuda", dtype=torch.float64) * 6.2 - 3.1).to(dt)
            P = torch.empty((B, ns, 6), device="cuda", dtype=dt)
            G = torch.empty((B, ns, 6, n), device="cuda", dtype=dt)
            fn = rbd._fn("rbd_ee_pose", dt)
            st = torch.cuda.current_stream().cuda_stream
            for what, pp, gp, outs in (("pose", P, None, 6), ("grad", None, G, 6 * n), ("pose+grad", P, G, 6 + 6 * n)):
                args = (q.data_ptr(), B, body.ctypes.data, T.ctypes.data, off.ctypes.data, ns,
                        None if pp is None else pp.data_ptr(), None if gp is None else gp.data_ptr(), st)
                rc = fn(*args)
                assert rc == 0, rbd._lib.check(rc)
                us = timed(lambda: fn(*args))
                by = B * (n + ns * outs) * esz
                print(f"{name:15s} B={B:8d} sites={ns:2d} {what:9s} {'fp32' if esz == 4 else 'fp64'}: {us:9.2f} us  "
                      f"{by / B:7.0f} B/row  {by / us / 1e3:7.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
