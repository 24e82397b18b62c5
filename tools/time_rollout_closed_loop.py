#!/usr/bin/env python3
"""HIP-event timings of rbd_rollout_closed_loop, of rbd_rollout on the same rows and of the per-step loop it replaces
(DESIGN.md §4.14).

    python tools/time_rollout_closed_loop.py [--out profiles/rollout_closed_loop_time.txt] [--quick]
Run it under a time limit (timeout -k 10 900 ...).  The method is §4.11's: per case the alternatives ALTERNATE in one
process, three rounds over all of them; every round of every one is at least 0.2 s of back-to-back calls between two device
events, after a warm-up of the same calls; the median round is reported, the spread of the rounds beside it.
    (a) closed    one rbd_rollout_closed_loop launch over all T steps, trajectory and u_applied stored; what it has to move
                  per row and step -- 2 n^2 + 4n scalars read (2 n^2 / A of them from the K shared by A candidates), 3n
                  written -- and the rate
    (b) rollout   rbd_rollout on the same rows (the nominal's controls), from the same build
    (c) loop      what a user writes without the entry point: per step RBDReference.aba, torch.baddbmm for K dx (a
                  broadcast matmul in the line-search shape), the two integrator updates and the copies into the trajectory
    goal          (a) < (c) by more than the spread between rounds; (a) / (b) is reported beside the ratio of the bytes
Inputs that stay finite for T steps: q0 uniform(-0.5, 0.5) at rest, ubar = rnea(q0, 0, 0) (holds the robot), K a PD law
-(50 I | 5 I) with 1 % noise, k small, the start off the reference by 0.01.  The PD law is halved until every state of the
closed loop is finite (a light link can turn 5 dt / inertia > 2 into a diverging velocity loop); the scale is reported.
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

# (robot, dtype, B_nom, A, T): A step sizes share one nominal of B_nom rows
CASES = [("iiwa_like", torch.float32, 4096, 1, 32), ("iiwa_like", torch.float32, 65536, 1, 32), ("atlas_like", torch.float32, 4096, 1, 32),
         ("iiwa_like", torch.float32, 8192, 8, 32)]
QUICK = [("iiwa_like", torch.float32, 130, 1, 3), ("atlas_like", torch.float32, 130, 1, 3), ("iiwa_like", torch.float32, 41, 4, 3)]
DT = 0.01
MIN_SECONDS = 0.2
ROUNDS = 3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_closed_loop_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rollout_closed_loop.py measures on a GPU; there is nothing to fall back to"
    min_s = 0.01 if a.quick else MIN_SECONDS
    lines = []
    for name, dt, Bn, A, T in (QUICK if a.quick else CASES):
        rbd = RBDReference(make_robot(name), build=False)
        lib = rbd._lib.lib
        n = rbd.n
        esz = 4 if dt == torch.float32 else 8
        sfx = "f32" if esz == 4 else "f64"
        B = A * Bn
        g = torch.Generator(device="cuda").manual_seed(Bn + T + A)

        def rand(shape, lo, hi):
            return (torch.rand(shape, device="cuda", dtype=torch.float64, generator=g) * (hi - lo) + lo).to(dt)

        def randn(shape):
            return torch.randn(shape, device="cuda", dtype=torch.float64, generator=g).to(dt)
        q0r = rand((Bn, n), -0.5, 0.5)
        qd0r = torch.zeros_like(q0r)
        ub = rbd.rnea(q0r, qd0r, qd0r)[0].expand(T, Bn, n).contiguous()                 # holds the robot at q0
        qr, qdr = rbd.rollout(q0r, qd0r, ub, DT)
        kf = 0.01 * randn((T, Bn, n))
        q0 = (q0r.repeat(A, 1) + rand((B, n), -0.01, 0.01)).contiguous()
        qd0 = rand((B, n), -0.01, 0.01)
        al = torch.linspace(1.0, 1.0 / A, A, device="cuda", dtype=dt).repeat_interleave(Bn).contiguous()
        eye = torch.eye(n, device="cuda", dtype=dt)
        pd = -torch.cat([50.0 * eye, 5.0 * eye], 1)
        st = torch.cuda.current_stream().cuda_stream
        new = lambda *shape: torch.empty(shape, device="cuda", dtype=dt)            # noqa: E731
        q, qd, ua = new(T, B, n), new(T, B, n), new(T, B, n)
        q_ro, qd_ro = new(T, B, n), new(T, B, n)
        q_lp, qd_lp, ua_lp = new(T, B, n), new(T, B, n), new(T, B, n)
        u_rows = ub.repeat(1, A, 1).contiguous()                                        # rbd_rollout's controls, one row each
        f_cl, f_ro = getattr(lib, f"rbd_rollout_closed_loop_{sfx}"), getattr(lib, f"rbd_rollout_{sfx}")
        p = lambda t: t.data_ptr()                                                  # noqa: E731

        def ok(rc):
            assert rc == 0, lib.rbd_last_error()

        scale, K = 2.0, None
        while True:                             # the PD law, halved until the closed loop stays finite
            scale *= 0.5
            assert scale > 1e-3, (name, "no PD scale keeps the closed loop finite")
            K = (scale * pd * (1.0 + 0.01 * randn((T, Bn, n, 2 * n)))).contiguous()

            def closed():
                ok(f_cl(p(q0), p(qd0), p(ub), p(kf), p(K), p(q0r), p(qd0r), p(qr), p(qdr), p(al), None, None, DT, -9.81, 0, B, Bn, T,
                        p(q), p(qd), 1, p(ua), st))
            closed()
            torch.cuda.synchronize()
            if bool(torch.isfinite(q).all() and torch.isfinite(qd).all() and torch.isfinite(ua).all()) and float(q.abs().max()) < 10.0:
                break

        def rollout():
            ok(f_ro(p(q0), p(qd0), p(u_rows), 0, DT, -9.81, 0, B, T, p(q_ro), p(qd_ro), 1, st))

        alk = (al.view(A, Bn, 1) * kf[:, None]).reshape(T, B, n).contiguous() + ub.repeat(1, A, 1)      # ubar + alpha k, formed once

        def loop():
            qt, qdt = q0, qd0
            for t in range(T):
                xr = torch.cat([q0r, qd0r] if t == 0 else [qr[t - 1], qdr[t - 1]], 1)
                x = torch.cat([qt, qdt], 1)
                if A == 1:
                    ut = torch.baddbmm(alk[t].unsqueeze(-1), K[t], (x - xr).unsqueeze(-1)).squeeze(-1)
                else:
                    dx = x.view(A, Bn, 2 * n) - xr
                    ut = alk[t] + torch.matmul(K[t], dx.unsqueeze(-1)).reshape(B, n)
                qdd = rbd.aba(qt, qdt, ut)
                qdt = qdt + DT * qdd
                qt = qt + DT * qdt
                q_lp[t], qd_lp[t], ua_lp[t] = qt, qdt, ut

        rollout(); loop()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(q_ro).all() and torch.isfinite(q_lp).all()), (name, "rollout or the loop is not finite")
        # the loop and the kernel integrate the same closed loop: a wrong index convention would differ by O(1); what
        # rounding leaves is reported
        diff = 0.0
        for tag, got, ref in (("q", q, q_lp), ("qd", qd, qd_lp), ("u", ua, ua_lp)):
            err = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
            assert err <= 0.05, (name, Bn, A, tag, err)
            diff = max(diff, err)
        things = {"closed": closed, "rollout": rollout, "loop": loop}
        iters = {s: calibrate(fn, min_s) for s, fn in things.items()}
        us_ = {s: [] for s in things}
        for _ in range(ROUNDS):
            for s, fn in things.items():
                us_[s].append(window(fn, iters[s]) / iters[s] * 1e3)
        med = {s: statistics.median(v) for s, v in us_.items()}
        spr = {s: (max(v) - min(v)) / med[s] * 100 for s, v in us_.items()}
        by_cl = T * B * (2 * n * n / A + 4 * n + 3 * n) * esz
        by_ro = T * B * 3 * n * esz
        margin = (med["loop"] - med["closed"]) / med["loop"] * 100
        met = med["closed"] < med["loop"] and margin > spr["closed"] + spr["loop"]
        line = (f"{name:12s} B_nom={Bn:6d} A={A} T={T:3d} {sfx} PD x{scale:g}: (a) closed loop {med['closed']:9.1f} us (+-{spr['closed']:4.1f}%) "
                f"{by_cl / 1e6:7.1f} MB {by_cl / med['closed'] / 1e6:5.2f} TB/s | (b) rollout {med['rollout']:9.1f} us (+-{spr['rollout']:4.1f}%) "
                f"{by_ro / 1e6:6.1f} MB: (a) / (b) = {med['closed'] / med['rollout']:5.2f}x time, {by_cl / by_ro:5.2f}x bytes | "
                f"(c) per-step loop {med['loop']:10.1f} us (+-{spr['loop']:4.1f}%) = {med['loop'] / med['closed']:6.2f}x (a): {'met' if met else 'MISSED'} | "
                f"kernel vs loop {diff:.1e} relative")
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                      # after every case: a later case that stops keeps the earlier lines
            fh.write("\n".join(lines) + "\n")
        del K, q, qd, ua, q_ro, qd_ro, q_lp, qd_lp, ua_lp, u_rows, alk, kf, qr, qdr, ub
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
