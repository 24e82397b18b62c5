#!/usr/bin/env python3
"""HIP-event timings of rbd_rollout_grad, of its stages and of what it replaces.

    python tools/time_rollout_grad.py [--out profiles/rollout_grad_time.txt] [--quick]
Run it under a time limit (timeout -k 10 600 ...).  Per case the alternatives ALTERNATE in one process: three rounds over
all of them; every round of every one is at least 0.2 s of back-to-back calls between two device events, after a warm-up
of the same calls; the median round is reported, the spread of the rounds beside it.  The trajectory is rolled out once,
outside the timed windows.
    (a) grad      one rbd_rollout_grad call through the C-ABI with the workspace RBDReference.rollout_grad gives it by
                  default (everything, capped at 1 GiB: the horizon is then walked in chunks)
    (b) stages    rbd_aba, rbd_rnea_grad, rbd_minv on the T B flat rows, and one rbd_rollout_adjoint launch over all T steps
    (c) bytes     what the scan has to move: T B (n 2n + n n + 2n + n) + 4 B n scalars, and the rate over the scan's time
    (d) loop      what a user writes today from existing entry points: forward_dynamics_grad + minv on the flat rows, then
                  per step the recursion in torch (two in-place adds, w, mu, two bmm, two adds)
    (e) fd-based  the same composite on forward_dynamics_grad instead of aba + rnea_grad: forward_dynamics_grad + minv on
                  the flat rows, then the scan launch on buffers of the same shapes (a scan written for -Minv dc_du would
                  skip nu and flip a sign; it would read the same bytes)
    goal          (a) < (d) and (a) <= (e), by more than the spread between rounds
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import make_robot  # noqa: E402
from rbdreference_amd import RBDReference  # noqa: E402

CASES = [("iiwa_like", torch.float32, 4096, 32), ("iiwa_like", torch.float32, 65536, 32), ("atlas_like", torch.float32, 16384, 32)]
QUICK = [("iiwa_like", torch.float32, 130, 3), ("atlas_like", torch.float32, 130, 3)]
DT = 0.01
MIN_SECONDS = 0.2
ROUNDS = 3
WS_CAP = 1 << 30


def window(fn, iters):
    """Milliseconds of `iters` back-to-back calls between two device events."""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def calibrate(fn, min_seconds):
    """Warm up, then the number of calls that fill `min_seconds`."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    iters = 1
    while True:
        ms = window(fn, iters)
        if ms >= 50.0 or iters >= 1 << 20:
            return max(1, int(iters * min_seconds * 1e3 / max(ms, 1e-3)) + 1)
        iters *= 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_grad_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rollout_grad.py measures on a GPU; there is nothing to fall back to"
    min_s = 0.01 if a.quick else MIN_SECONDS
    lines = []
    for name, dt, B, T in (QUICK if a.quick else CASES):
        rbd = RBDReference(make_robot(name), build=False)
        lib = rbd._lib.lib
        n = rbd.n
        esz = 4 if dt == torch.float32 else 8
        sfx = "f32" if esz == 4 else "f64"
        R = T * B
        g = torch.Generator(device="cuda").manual_seed(B + T)

        def rand(shape, scale):
            return ((torch.rand(shape, device="cuda", dtype=torch.float64, generator=g) * 2 - 1) * scale).to(dt)
        q0, qd0, u = rand((B, n), 3.14159), rand((B, n), 1.0), rand((T, B, n), 5.0)
        gq, gqd = rand((T, B, n), 1.0), rand((T, B, n), 1.0)
        q, qd = rbd.rollout(q0, qd0, u, DT)
        # the linearisation points as flat rows [T B, n]: (q0, qd0), then slices 0 .. T-2 of the trajectory
        qs = torch.cat([q0[None], q[:-1]]).reshape(R, n).contiguous()
        qds = torch.cat([qd0[None], qd[:-1]]).reshape(R, n).contiguous()
        us = u.reshape(R, n)
        st = torch.cuda.current_stream().cuda_stream
        new = lambda *shape: torch.empty(shape, device="cuda", dtype=dt)            # noqa: E731
        gu, gq0, gqd0, lam = new(T, B, n), new(B, n), new(B, n), new(B, 2 * n)
        qdd, dc, Mi, fd = new(R, n), new(R, n, 2 * n), new(R, n, n), new(R, n, 2 * n)
        wsb = max(min(int(lib.rbd_rollout_grad_workspace_bytes(B, T, esz)), WS_CAP), int(lib.rbd_rollout_grad_workspace_bytes(B, 1, esz)))
        ws = torch.empty((wsb,), device="cuda", dtype=torch.uint8)
        mwsb = int(lib.rbd_minv_workspace_bytes(R, esz))
        mws = torch.empty((max(mwsb, 16),), device="cuda", dtype=torch.uint8)
        fwsb = int(lib.rbd_fd_workspace_bytes(R, esz))
        fws = torch.empty((max(fwsb, 16),), device="cuda", dtype=torch.uint8)
        f = {k: getattr(lib, f"rbd_{k}_{sfx}") for k in ("rollout_grad", "rollout_adjoint", "aba", "rnea_grad", "minv", "forward_dynamics_grad")}
        p = lambda t: t.data_ptr()                                                  # noqa: E731

        def ok(rc):
            assert rc == 0, lib.rbd_last_error()

        def grad():
            ok(f["rollout_grad"](p(q0), p(qd0), p(u), p(q), p(qd), p(gq), p(gqd), 0, DT, -9.81, 0, B, T, p(gu), p(gq0), p(gqd0), p(ws), wsb, st))

        def aba():
            ok(f["aba"](p(qs), p(qds), p(us), -9.81, R, p(qdd), st))

        def rnea_grad():
            ok(f["rnea_grad"](p(qs), p(qds), p(qdd), -9.81, 0, R, None, p(dc), st))

        def minv():
            ok(f["minv"](p(qs), R, 1, p(Mi), p(mws), mwsb, st))

        def scan_on(mat):
            lam.zero_()
            ok(f["rollout_adjoint"](p(mat), p(Mi), p(gq), p(gqd), 0, DT, 0, B, T, p(lam), p(gu), st))

        def fdg():
            ok(f["forward_dynamics_grad"](p(qs), p(qds), p(us), -9.81, R, p(qdd), p(fd), p(fws), fwsb, st))

        gu_loop, lam_loop = new(T, B, n), new(B, 2 * n)

        def recursion():
            fdv, Miv = fd.view(T, B, n, 2 * n), Mi.view(T, B, n, n)
            lq, lqd = torch.zeros_like(q0), torch.zeros_like(q0)
            for t in range(T - 1, -1, -1):
                lq.add_(gq[t])
                lqd.add_(gqd[t])
                w = torch.add(lqd, lq, alpha=DT)
                mu = (w * DT).unsqueeze(-1)
                gu_loop[t] = torch.bmm(Miv[t], mu).squeeze(-1)
                back = torch.bmm(fdv[t].transpose(1, 2), mu).squeeze(-1)             # fd = -Minv dc_du
                lq = lq + back[:, :n]
                lqd = w + back[:, n:]
            lam_loop[:, :n] = lq
            lam_loop[:, n:] = lqd

        def loop():
            fdg(); minv(); recursion()

        def fd_based():
            fdg(); minv(); scan_on(fd)

        # one pass of everything: the loop and the kernel compute the same gradient
        grad(); aba(); rnea_grad(); minv(); scan_on(dc); loop()
        torch.cuda.synchronize()
        tol = 2e-3 if esz == 4 else 1e-9
        for got, ref in ((gu, gu_loop), (torch.cat([gq0, gqd0], 1), lam_loop)):
            err = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
            assert err <= tol, (name, B, T, err)
        things = {"grad": grad, "aba": aba, "rnea_grad": rnea_grad, "minv": minv, "scan": lambda: scan_on(dc), "loop": loop,
                  "fd_based": fd_based, "fdg": fdg}
        iters = {k: calibrate(fn, min_s) for k, fn in things.items()}
        us_ = {k: [] for k in things}
        for _ in range(ROUNDS):
            for k, fn in things.items():
                us_[k].append(window(fn, iters[k]) / iters[k] * 1e3)
        med = {k: statistics.median(v) for k, v in us_.items()}
        spr = {k: (max(v) - min(v)) / med[k] * 100 for k, v in us_.items()}
        by = (R * (n * 2 * n + n * n + 2 * n + n) + 4 * B * n) * esz
        margin = lambda x, y: (med[y] - med[x]) / med[y] * 100                       # noqa: E731
        met_d = med["grad"] < med["loop"] and margin("grad", "loop") > spr["grad"] + spr["loop"]
        met_e = med["grad"] <= med["fd_based"]
        line = (f"{name:12s} B={B:6d} T={T:3d} {sfx}: (a) rollout_grad {med['grad']:9.1f} us (+-{spr['grad']:4.1f}%) | "
                f"(b) aba {med['aba']:8.1f} rnea_grad {med['rnea_grad']:8.1f} minv {med['minv']:8.1f} scan {med['scan']:8.1f} us "
                f"(+-{spr['aba']:.1f} {spr['rnea_grad']:.1f} {spr['minv']:.1f} {spr['scan']:.1f}%) | "
                f"(c) {by / 1e6:7.1f} MB {by / med['scan'] / 1e6:5.2f} TB/s | "
                f"(d) loop {med['loop']:9.1f} us (+-{spr['loop']:4.1f}%) = {med['loop'] / med['grad']:5.2f}x (a): {'met' if met_d else 'MISSED'} | "
                f"(e) fd-based {med['fd_based']:9.1f} us (+-{spr['fd_based']:4.1f}%; forward_dynamics_grad {med['fdg']:8.1f}) = "
                f"{med['fd_based'] / med['grad']:5.2f}x (a): {'met' if met_e else 'MISSED'}")
        print(line, flush=True)
        lines.append(line)
        del ws, mws, fws, dc, Mi, fd, qdd, gu, gu_loop, qs, qds, q, qd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
