#!/usr/bin/env python3
"""HIP-event timings of rbd_mppi_update against the same update written in torch, and of one mppi iteration split into its
parts.

    python tools/time_mppi.py [--out profiles/mppi_time.txt] [--quick]
Run it under a time limit (timeout -k 10 900 ...).  The method is §4.11's: per case the alternatives ALTERNATE in one
process, three rounds over all of them; every round of every one is at least 0.2 s of back-to-back calls between two device
events, after a warm-up of the same calls; the median round is reported, the spread of the rounds beside it.  All cases are
fp32, the 7-joint arm, T = 32, limits on, through the Python API on both sides; by (P, S): (1, 65 536), (64, 1 024), (8 192, 8).
    (a)   mppi_update(J, du, u, lam, u_min, u_max)
    (b)   the same result in torch, with what a user had before it: where / min / exp for the softmin, the clamp and subtract
          passes over du, einsum for the weighted sum.  It does not depend on this library, so (b) of any build is the same code
    goal  (a) < (b) by more than the spread between rounds in all three cases; (a) and (b) within the order-free bound of
          tests/mppi_oracle.bounds of the float64 restatement (so within twice the bound of each other)
    also  the bytes of du over (a)'s time, and one mppi iteration (sigma = 0.1, the noise drawn by torch.randn) split into
          randn + scale, rollout_cost, mppi_update and the glue = mppi(iters=1) minus those three and the final rollout_cost
Inputs of the update are the tests': J uniform(5, 25), du normal(0, 0.3), u normal(0, 0.5), lam = 1, limits -0.6 .. 0.6.  The
iteration starts at rest in q0 uniform(-0.5, 0.5) under u = rnea(q0, 0, 0), with a cost that tracks q0 and limits -100 .. 100.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from conftest import make_robot  # noqa: E402
from mppi_oracle import bounds, mppi_update  # noqa: E402
from rbdreference_amd import QuadraticCost, RBDReference  # noqa: E402
from time_rollout_cost import measure  # noqa: E402

CASES = [(1, 65536, 32), (64, 1024, 32), (8192, 8, 32)]      # (P, S, T)
QUICK = [(1, 130, 3), (4, 70, 3), (40, 8, 3)]
DT = 0.01
MIN_SECONDS = 0.2
LO, HI = -0.6, 0.6
dt = torch.float32


def torch_update(J, du, u, lam, lo, hi):
    """(b): the update with torch's own kernels."""
    Jc = torch.where(torch.isnan(J), torch.full_like(J, float("inf")), J)
    e = torch.exp(-(Jc - Jc.min(dim=0).values) / lam)
    d = torch.clamp(u[:, None] + du, lo, hi) - u[:, None]
    D = torch.einsum("sp,tspj->tpj", e, d) / e.sum(dim=0)[None, :, None]
    return torch.clamp(u + D, lo, hi)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppi_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_mppi.py measures on a GPU; there is nothing to fall back to"
    min_s = 0.01 if a.quick else MIN_SECONDS
    rbd = RBDReference(make_robot("iiwa_like"), build=False)
    n = rbd.n
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                      # after every line: a later case that stops keeps the earlier ones
            fh.write("\n".join(lines) + "\n")

    for P, S, T in (QUICK if a.quick else CASES):
        g = torch.Generator(device="cuda").manual_seed(P + S + T)
        rand = lambda *s: torch.rand(s, device="cuda", dtype=torch.float64, generator=g)      # noqa: E731
        randn = lambda *s: torch.randn(s, device="cuda", dtype=torch.float64, generator=g)      # noqa: E731
        J, du, u = (5 + 20 * rand(S, P)).to(dt), (0.3 * randn(T, S, P, n)).to(dt), (0.5 * randn(T, P, n)).to(dt)
        lam = torch.ones((P,), device="cuda", dtype=dt)
        lo, hi = torch.full((n,), LO, device="cuda", dtype=dt), torch.full((n,), HI, device="cuda", dtype=dt)
        new = lambda: rbd.mppi_update(J, du, u, lam, u_min=lo, u_max=hi).u      # noqa: E731
        old = lambda: torch_update(J, du, u, lam, lo, hi)                       # noqa: E731
        ua, ub = new(), old()
        torch.cuda.synchronize()
        np64 = lambda x: x.double().cpu().numpy()      # noqa: E731
        ref = mppi_update(np64(J), np64(du), np64(u), np64(lam), LO, HI)
        b_u = bounds("f32", S, ref, np64(u), np64(du), True)[0]
        ra, rb = float((np.abs(np64(ua) - ref[0]) / b_u).max()), float((np.abs(np64(ub) - ref[0]) / b_u).max())
        rab = float((np.abs(np64(ua) - np64(ub)) / (2 * b_u)).max())
        assert ra <= 1.0 and rab <= 1.0, ((P, S), "err / bound: (a) against the float64 restatement, (a) against (b)", ra, rab)
        del ref, b_u
        med, spr = measure({"new": new, "old": old}, min_s)
        margin = (med["old"] - med["new"]) / med["old"] * 100
        met = med["new"] < med["old"] and margin > spr["new"] + spr["old"]
        mb = du.numel() * 4 / 1e6
        emit(f"iiwa_like update P={P:5d} S={S:6d} T={T:3d} f32 limits: (a) mppi_update {med['new']:9.1f} us (+-{spr['new']:4.1f}%) | (b) torch "
             f"{med['old']:9.1f} us (+-{spr['old']:4.1f}%) = {med['old'] / med['new']:5.2f}x (a): {'met' if met else 'MISSED'} | du {mb:6.1f} MB over (a) "
             f"{mb / med['new']:6.3f} TB/s | err / bound vs float64: (a) {ra:.3f} (b) {rb:.3f}; (a) vs (b) / twice the bound {rab:.3f}")
        # one iteration of the driver
        q0 = (rand(P, n) - 0.5).to(dt)
        qd0 = torch.zeros_like(q0)
        u0 = rbd.rnea(q0, qd0, qd0)[0].expand(T, P, n).contiguous()
        cost = QuadraticCost(w_q=torch.full((n,), 10.0, device="cuda", dtype=dt), w_qd=torch.ones((n,), device="cuda", dtype=dt),
                             q_target=q0.expand(T, P, n).contiguous(), w_u=torch.full((n,), 1e-3, device="cuda", dtype=dt))
        # (limits and lam as device tensors, as the driver makes them once before its loop: a float is uploaded per call)
        lims = dict(u_min=torch.full((n,), -100.0, device="cuda", dtype=dt), u_max=torch.full((n,), 100.0, device="cuda", dtype=dt))
        q0s, qd0s = q0.repeat(S, 1), qd0.repeat(S, 1)

        def noise():
            d = 0.1 * torch.randn((T, S, P, n), device="cuda", dtype=dt)
            d[:, 0] = 0
            return d
        d1 = noise()
        J1 = rbd.rollout_cost(q0s, qd0s, u0, DT, cost, du=d1.view(T, S * P, n), **lims).view(S, P)
        lam_it = J1.std(dim=0) if S > 1 else lam        # a temperature of the costs' own scale (made once: no host read in the loop)
        r = rbd.mppi(q0, qd0, u0, DT, cost, iters=1, samples=S, sigma=0.1, lam=lam_it, **lims)
        assert bool(torch.isfinite(r.cost).all()) and not bool(r.status.any())
        things = {
            "noise": noise,
            "cost": lambda: rbd.rollout_cost(q0s, qd0s, u0, DT, cost, du=d1.view(T, S * P, n), **lims),
            "update": lambda: rbd.mppi_update(J1, d1, u0, lam_it, **lims),
            "final": lambda: rbd.rollout_cost(q0, qd0, u0, DT, cost, return_trajectory=True, **lims),
            "mppi": lambda: rbd.mppi(q0, qd0, u0, DT, cost, iters=1, samples=S, sigma=0.1, lam=lam_it, **lims),
        }
        med, spr = measure(things, min_s)
        glue = med["mppi"] - med["final"] - med["noise"] - med["cost"] - med["update"]
        emit(f"iiwa_like mppi   P={P:5d} S={S:6d} T={T:3d} f32 limits: one iteration {med['mppi'] - med['final']:9.1f} us = randn + scale "
             f"{med['noise']:9.1f} us (+-{spr['noise']:4.1f}%) + rollout_cost {med['cost']:9.1f} us (+-{spr['cost']:4.1f}%) + mppi_update "
             f"{med['update']:9.1f} us (+-{spr['update']:4.1f}%) + glue {glue:8.1f} us | the final rollout_cost {med['final']:9.1f} us "
             f"(+-{spr['final']:4.1f}%); mppi(iters=1) {med['mppi']:9.1f} us (+-{spr['mppi']:4.1f}%); mean ess {float(r.ess.mean()):.1f} of {S} "
             f"(the start is the cost's optimum: the iteration is timed, not judged)")
        del J, du, u, d1, J1, q0s, qd0s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
