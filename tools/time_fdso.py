#!/usr/bin/env python3
"""HIP-event timings of rbd_fdsva_so C-ABI launches and of what a user had to run before it existed (pre-allocated
outputs and workspaces, warm clock: 50 ms of the same launches first; best of 3 x 50 back-to-back launches).

    python tools/time_fdso.py            # the rows of DESIGN.md §4.10, fp32 and fp64
Run it under a time limit (timeout -k 10 600 ...).  Per (robot, B, precision) it prints, all measured in this one
process:
    fdsva_so      the whole entry point (forward_dynamics_grad + minv + second_order_idsva + the contraction kernel)
    so / fdg / minv, and their sum "components": the three existing entry points through the C-ABI, as inside fdsva_so
    contraction   fdsva_so - components: the new kernel(s); bytes it moves (reads 4 n^3 + 3 n^2, writes 4 n^3 scalars per
                  row; where the outputs are split over several launches dM_dq is read once per launch with an inner
                  sum) and the rate they imply
    einsum        the torch.einsum composition of RBDReference.py:1625-1629 on the components' outputs (the "before")
    goal          fdsva_so <= components + one more second_order_idsva time
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


def einsum_composition(Minv, fd, so, n):
    fd_dq, fd_dqd = fd[..., :n], fd[..., n:]
    d2q, d2qd, d2vq, dM = so[:, 0], so[:, 1], so[:, 2], so[:, 3]
    e = torch.einsum
    a = -e("bil,bljk->bijk", Minv, d2q + e("bilk,blj->bijk", dM, fd_dq) + e("bilk,blj->bikj", dM, fd_dq))
    b = -e("bil,bljk->bijk", Minv, d2vq + e("bilk,blj->bijk", dM, fd_dqd))
    c = -e("bil,bljk->bijk", Minv, d2qd)
    d = -e("bil,bljk->bijk", Minv, e("bilk,blj->bijk", dM, Minv))
    return a, b, c, d


def main():
    for name, B in ROWS:
        rbd = RBDReference(make_robot(name), build=False)
        lib = rbd._lib.lib
        n = rbd.n
        for dt in (torch.float32, torch.float64):
            esz = 4 if dt == torch.float32 else 8
            sfx = "f32" if esz == 4 else "f64"
            q, qd, u = ((torch.rand((B, n), device="cuda", dtype=torch.float64) * 2 - 1).to(dt) for _ in range(3))
            out = torch.empty((B, 4, n, n, n), device="cuda", dtype=dt)
            so = torch.empty((B, 4, n, n, n), device="cuda", dtype=dt)
            qdd = torch.empty((B, n), device="cuda", dtype=dt)
            fd = torch.empty((B, n, 2 * n), device="cuda", dtype=dt)
            Mi = torch.empty((B, n, n), device="cuda", dtype=dt)
            wsb = int(lib.rbd_fdsva_so_workspace_bytes(B, esz))
            ws = torch.empty((wsb,), device="cuda", dtype=torch.uint8)
            fwsb = int(lib.rbd_fd_workspace_bytes(B, esz))
            fws = torch.empty((max(fwsb, 1),), device="cuda", dtype=torch.uint8)
            mwsb = int(lib.rbd_minv_workspace_bytes(B, esz))
            mws = torch.empty((max(mwsb, 1),), device="cuda", dtype=torch.uint8)
            st = torch.cuda.current_stream().cuda_stream
            f_all = getattr(lib, f"rbd_fdsva_so_{sfx}")
            f_so = getattr(lib, f"rbd_second_order_idsva_{sfx}")
            f_fdg = getattr(lib, f"rbd_forward_dynamics_grad_{sfx}")
            f_minv = getattr(lib, f"rbd_minv_{sfx}")
            calls = {
                "fdsva_so": lambda: f_all(q.data_ptr(), qd.data_ptr(), u.data_ptr(), -9.81, B, out.data_ptr(), ws.data_ptr(), wsb, st),
                "fdg": lambda: f_fdg(q.data_ptr(), qd.data_ptr(), u.data_ptr(), -9.81, B, qdd.data_ptr(), fd.data_ptr(), fws.data_ptr(), fwsb, st),
                "minv": lambda: f_minv(q.data_ptr(), B, 1, Mi.data_ptr(), mws.data_ptr(), mwsb, st),
                "so": lambda: f_so(q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), -9.81, B, so.data_ptr(), st),
            }
            us = {}
            for k in ("fdg", "minv", "so", "fdsva_so"):
                rc = calls[k]()
                assert rc == 0, (k, rc, lib.rbd_last_error())
                us[k] = timed(calls[k])
            comp = us["fdg"] + us["minv"] + us["so"]
            ctr = us["fdsva_so"] - comp
            by = B * (8 * n ** 3 + 3 * n ** 2) * esz
            # one sample of the einsum composition is enough for the README sentence (it allocates its intermediates)
            torch.cuda.synchronize()
            t_e = timed(lambda: einsum_composition(Mi, fd, so, n), iters=5)
            goal = comp + us["so"]
            print(f"{name:15s} B={B:6d} {sfx}: fdsva_so {us['fdsva_so']:9.1f} us | so {us['so']:9.1f}  fdg {us['fdg']:8.1f}  "
                  f"minv {us['minv']:8.1f}  components {comp:9.1f} | contraction {ctr:9.1f} us  {by / 1e6:7.1f} MB (single-launch "
                  f"count)  {by / ctr / 1e6:5.2f} TB/s | einsum {t_e:9.1f} us | goal <= {goal:9.1f} us: "
                  f"{'met' if us['fdsva_so'] <= goal else 'MISSED'}", flush=True)


if __name__ == "__main__":
    main()
