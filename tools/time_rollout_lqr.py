#!/usr/bin/env python3
"""HIP-event timings of rbd_rollout_riccati, of rbd_rollout_lqr with its stages and of the loop they replace.

    python tools/time_rollout_lqr.py [--out profiles/rollout_lqr_time.txt] [--quick]
Run it under a time limit (timeout -k 10 900 ...).  The method is §4.11's: per case the alternatives ALTERNATE in one
process, three rounds over all of them; every round of every one is at least 0.2 s of back-to-back calls between two device
events, after a warm-up of the same calls; the median round is reported, the spread of the rounds beside it.  The
trajectory is rolled out once, outside the timed windows.
    (a) scan      one rbd_rollout_riccati launch over all T steps on a stored linearisation; what it has to move --
                  T B (3 n^2 + 6 n) scalars read, T B (2 n^2 + n) written, B (4 n^2 + 2 n + 3) both ways -- and the rate
    (b) lqr       one rbd_rollout_lqr call through the C-ABI with the workspace RBDReference.rollout_lqr gives it by default,
                  and its stages rbd_aba, rbd_rnea_grad, rbd_minv on the T B flat rows
    (c) loop      the recursion a user writes today on the same linearisation: per step torch.bmm for the products,
                  torch.linalg.cholesky_ex (no host check) and torch.cholesky_solve for the gains (about twenty launches per step)
    goal          (a) < (c) by more than the spread between rounds
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

CASES = [("iiwa_like", torch.float32, 4096, 32), ("iiwa_like", torch.float32, 65536, 32), ("atlas_like", torch.float32, 4096, 32)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_lqr_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rollout_lqr.py measures on a GPU; there is nothing to fall back to"
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

        def rand(shape, lo, hi):
            return (torch.rand(shape, device="cuda", dtype=torch.float64, generator=g) * (hi - lo) + lo).to(dt)
        q0, qd0, u = rand((B, n), -3.14159, 3.14159), rand((B, n), -1, 1), rand((T, B, n), -5, 5)
        gq, gqd, gu = rand((T, B, n), -1, 1), rand((T, B, n), -1, 1), rand((T, B, n), -1, 1)
        # (state Hessians small beside hess_u: over 32 steps of real dynamics Bm^T P Bm then stays where float32 still factors
        # Quu in every row -- torch's cholesky raises for the whole batch otherwise; the times do not depend on the values)
        hq, hqd, hu = rand((T, B, n), 0.05, 0.15), rand((T, B, n), 0.05, 0.15), rand((T, B, n), 1, 2)
        q, qd = rbd.rollout(q0, qd0, u, DT)
        # the linearisation points as flat rows [T B, n]: (q0, qd0), then slices 0 .. T-2 of the trajectory
        qs = torch.cat([q0[None], q[:-1]]).reshape(R, n).contiguous()
        qds = torch.cat([qd0[None], qd[:-1]]).reshape(R, n).contiguous()
        us = u.reshape(R, n)
        st = torch.cuda.current_stream().cuda_stream
        new = lambda *shape: torch.empty(shape, device="cuda", dtype=dt)            # noqa: E731
        k, K, lam, P, dV = new(T, B, n), new(T, B, n, 2 * n), new(B, 2 * n), new(B, 2 * n, 2 * n), new(B, 2)
        status = torch.empty((B,), device="cuda", dtype=torch.int32)
        qdd, dc, Mi = new(R, n), new(R, n, 2 * n), new(R, n, n)
        wsb = max(min(int(lib.rbd_rollout_lqr_workspace_bytes(B, T, esz)), WS_CAP), int(lib.rbd_rollout_lqr_workspace_bytes(B, 1, esz)))
        ws = torch.empty((wsb,), device="cuda", dtype=torch.uint8)
        mwsb = int(lib.rbd_minv_workspace_bytes(R, esz))
        mws = torch.empty((max(mwsb, 16),), device="cuda", dtype=torch.uint8)
        f = {s: getattr(lib, f"rbd_{s}_{sfx}") for s in ("rollout_lqr", "rollout_riccati", "aba", "rnea_grad", "minv")}
        p = lambda t: t.data_ptr()                                                  # noqa: E731

        def ok(rc):
            assert rc == 0, lib.rbd_last_error()

        def lqr():
            ok(f["rollout_lqr"](p(q0), p(qd0), p(u), p(q), p(qd), p(gq), p(gqd), p(hq), p(hqd), 0, p(gu), p(hu), 0, 0.0, DT, -9.81, 0,
                                B, T, p(k), p(K), p(lam), p(P), p(dV), p(status), p(ws), wsb, st))

        def aba():
            ok(f["aba"](p(qs), p(qds), p(us), -9.81, R, p(qdd), st))

        def rnea_grad():
            ok(f["rnea_grad"](p(qs), p(qds), p(qdd), -9.81, 0, R, None, p(dc), st))

        def minv():
            ok(f["minv"](p(qs), R, 1, p(Mi), p(mws), mwsb, st))

        def scan():
            lam.zero_(); P.zero_(); dV.zero_(); status.zero_()
            ok(f["rollout_riccati"](p(dc), p(Mi), p(gq), p(gqd), p(hq), p(hqd), 0, p(gu), p(hu), 0, 0.0, DT, 0, B, T, p(lam), p(P),
                                    p(dV), p(status), p(k), p(K), st))

        k_loop, K_loop = new(T, B, n), new(T, B, n, 2 * n)
        out_loop = {}
        eye = torch.eye(n, device="cuda", dtype=dt)
        A0 = torch.cat([torch.cat([eye, DT * eye], 1), torch.cat([0 * eye, eye], 1)])

        LOOP_ROWS = 32768      # torch's batched Cholesky fails for most of 65 536 matrices on this stack (63 247 rows with info > 0
                               # where the kernel factors every one): the loop walks the batch in halves there, as a user must

        def recursion():
            D, M = dc.view(T, B, n, 2 * n), Mi.view(T, B, n, n)
            out_loop["bad"] = torch.zeros(B, device="cuda", dtype=torch.bool)
            out_loop["lam"], out_loop["P"] = new(B, 2 * n), new(B, 2 * n, 2 * n)
            for b0 in range(0, B, LOOP_ROWS):
                sl = slice(b0, min(B, b0 + LOOP_ROWS))
                nb = sl.stop - sl.start
                lm = torch.zeros(nb, 2 * n, 1, device="cuda", dtype=dt)
                Pm = torch.zeros(nb, 2 * n, 2 * n, device="cuda", dtype=dt)
                for t in range(T - 1, -1, -1):
                    Mt = M[t, sl]
                    Bm = torch.cat([DT * DT * Mt, DT * Mt], 1)
                    A = A0 - torch.bmm(Bm, D[t, sl])
                    lm = lm + torch.cat([gq[t, sl], gqd[t, sl]], 1).unsqueeze(-1)
                    Pm = Pm + torch.diag_embed(torch.cat([hq[t, sl], hqd[t, sl]], 1))
                    PA = torch.bmm(Pm, A)
                    Qx = torch.bmm(A.transpose(1, 2), lm)
                    Qu = gu[t, sl].unsqueeze(-1) + torch.bmm(Bm.transpose(1, 2), lm)
                    Qxx = torch.bmm(A.transpose(1, 2), PA)
                    Qux = torch.bmm(Bm.transpose(1, 2), PA)
                    Quu = torch.diag_embed(hu[t, sl]) + torch.bmm(Bm.transpose(1, 2), torch.bmm(Pm, Bm))
                    L, info = torch.linalg.cholesky_ex(Quu)         # (no host check per step: the loop's best case)
                    out_loop["bad"][sl] |= info > 0
                    sol = -torch.cholesky_solve(torch.cat([Qu, Qux], 2), L)
                    kt, Kt = sol[:, :, :1], sol[:, :, 1:]
                    k_loop[t, sl] = kt.squeeze(-1)
                    K_loop[t, sl] = Kt
                    lm = Qx + torch.bmm(Kt.transpose(1, 2), torch.bmm(Quu, kt) + Qu) + torch.bmm(Qux.transpose(1, 2), kt)
                    Pm = Qxx + torch.bmm(Kt.transpose(1, 2), torch.bmm(Quu, Kt) + Qux) + torch.bmm(Qux.transpose(1, 2), Kt)
                    Pm = 0.5 * (Pm + Pm.transpose(1, 2))
                out_loop["lam"][sl], out_loop["P"][sl] = lm.squeeze(-1), Pm

        # one pass of everything: the loop and the kernel compute the same gains and value function
        lqr(); aba(); rnea_grad(); minv()
        torch.cuda.synchronize()
        from_lqr = [x.clone() for x in (k, K, lam, P)]
        scan(); recursion()
        torch.cuda.synchronize()
        # Over 32 steps of real dynamics a few rows in 65 536 drift to where float32 no longer factors Quu (the kernel counts
        # them in status and stores zero gains, torch's factor is meaningless there), and rows near that edge agree less well.
        # The sanity check is therefore per row: of the rows both sides factored, at least 99 % agree within tol.
        tol = 5e-3 if esz == 4 else 1e-8
        both = (status == 0) & ~out_loop["bad"]
        assert int(both.sum()) >= 0.99 * B, (name, B, T, "rows factored by both / kernel failed / torch failed / finite inputs",
                                             int(both.sum()), int((status != 0).sum()), int(out_loop["bad"].sum()),
                                             bool(torch.isfinite(dc).all() and torch.isfinite(Mi).all()),
                                             float(q.abs().max()), float(qd.abs().max()), float(Mi.abs().max()))

        def rows_agree(got, ref, time_major):
            d, r = (got.double() - ref.double()).abs(), ref.double().abs()
            if time_major:
                d, r = d.transpose(0, 1), r.transpose(0, 1)
            e = d.reshape(B, -1).amax(1) / r.reshape(B, -1).amax(1)
            return float(((e <= tol) & both).sum()) / float(both.sum())
        for tag, got, ref, tm in (("k", k, k_loop, True), ("K", K, K_loop, True), ("lam", lam, out_loop["lam"], False),
                                  ("P", P, out_loop["P"], False)):
            assert rows_agree(got, ref, tm) >= 0.99, (name, B, T, tag, rows_agree(got, ref, tm))
        for tag, got, ref, tm in zip("k K lam P".split(), from_lqr, (k, K, lam, P), (True, True, False, False)):
            assert rows_agree(got, ref, tm) >= 0.99, (name, B, T, "lqr vs scan", tag)
        factored = int(both.sum())
        things = {"scan": scan, "lqr": lqr, "aba": aba, "rnea_grad": rnea_grad, "minv": minv, "loop": recursion}
        iters = {s: calibrate(fn, min_s) for s, fn in things.items()}
        us_ = {s: [] for s in things}
        for _ in range(ROUNDS):
            for s, fn in things.items():
                us_[s].append(window(fn, iters[s]) / iters[s] * 1e3)
        med = {s: statistics.median(v) for s, v in us_.items()}
        spr = {s: (max(v) - min(v)) / med[s] * 100 for s, v in us_.items()}
        by = (R * (3 * n * n + 6 * n + 2 * n * n + n) + 2 * B * (4 * n * n + 2 * n + 3)) * esz
        flops = R * 2 * n * 14 * n * n * 2                                         # ~14 n^2 FMAs per thread and step, 2n threads
        margin = (med["loop"] - med["scan"]) / med["loop"] * 100
        met = med["scan"] < med["loop"] and margin > spr["scan"] + spr["loop"]
        line = (f"{name:12s} B={B:6d} T={T:3d} {sfx}: (a) scan {med['scan']:9.1f} us (+-{spr['scan']:4.1f}%) "
                f"{by / 1e6:7.1f} MB {by / med['scan'] / 1e6:5.2f} TB/s {flops / med['scan'] / 1e6:5.2f} TFLOP/s | "
                f"(b) rollout_lqr {med['lqr']:9.1f} us (+-{spr['lqr']:4.1f}%): aba {med['aba']:8.1f} rnea_grad {med['rnea_grad']:8.1f} "
                f"minv {med['minv']:8.1f} us (+-{spr['aba']:.1f} {spr['rnea_grad']:.1f} {spr['minv']:.1f}%) | "
                f"(c) torch loop {med['loop']:10.1f} us (+-{spr['loop']:4.1f}%) = {med['loop'] / med['scan']:6.2f}x (a): {'met' if met else 'MISSED'} | "
                f"rows factored by both {factored} of {B}")
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                      # after every case: a later case that stops keeps the earlier lines
            fh.write("\n".join(lines) + "\n")
        del ws, mws, dc, Mi, qdd, k, K, k_loop, K_loop, qs, qds, q, qd, from_lqr
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
