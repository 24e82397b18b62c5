#!/usr/bin/env python3
"""HIP-event timings of rbd_rollout_cost against what a user writes without it, and of one ilqr iteration split into its
launches.

    python tools/time_rollout_cost.py [--out profiles/rollout_cost_time.txt] [--quick]
Run it under a time limit (timeout -k 10 900 ...).  The method is §4.11's: per case the alternatives ALTERNATE in one
process, three rounds over all of them; every round of every one is at least 0.2 s of back-to-back calls between two device
events, after a warm-up of the same calls; the median round is reported, the spread of the rounds beside it.  All cases are
fp32, T = 32, through the Python API on both sides.
    line search   iiwa, B_nom = 8192, A = 8:  (a) rollout_cost(alpha=[A])  (b) rollout_closed_loop(alpha=[A]), then
                  QuadraticCost.value on its [T, A, B, n] outputs
    MPPI          iiwa, B_nom = 1, B = 65536, du normal(0, 0.1), no K:  (a) rollout_cost(du=du)  (b) rollout(q0, qd0, u + du)
                  with the trajectory, then .value
    Atlas         B = 4096, closed loop, A = 1: as the first row
    goal          (a) < (b) by more than the spread between rounds in the two iiwa cases; Atlas is reported
    ilqr          one iteration (iiwa, B = 8192, A = 6): rollout_lqr, the rollout_cost line search, the rollout_closed_loop
                  forward pass, and the torch glue = ilqr(iters=1) minus those three and the start's rollout_cost
rollout_closed_loop and rollout are untouched by rollout_cost, so (b) is the code a user had before it.
Inputs are time_rollout_closed_loop.py's, which stay finite for T steps: q0 uniform(-0.5, 0.5) at rest, ubar = rnea(q0, 0, 0),
K a PD law -(50 I | 5 I) with 1 % noise, halved until the closed loop stays finite, k small, the start off the reference by
0.01.  The cost tracks the nominal's trajectory: weights 5 .. 15 (state) and 1 .. 2 (control), c_u in -1 .. 1.
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
from rbdreference_amd import QuadraticCost, RBDReference  # noqa: E402
from time_rollout_closed_loop import calibrate, window  # noqa: E402

# (what, robot, B_nom, A or samples, T)
CASES = [("line search", "iiwa_like", 8192, 8, 32), ("mppi", "iiwa_like", 1, 65536, 32), ("line search", "atlas_like", 4096, 1, 32),
         ("ilqr", "iiwa_like", 8192, 6, 32)]
QUICK = [("line search", "iiwa_like", 41, 4, 3), ("mppi", "iiwa_like", 1, 130, 3), ("line search", "atlas_like", 40, 1, 3),
         ("ilqr", "iiwa_like", 41, 6, 3)]
DT = 0.01
MIN_SECONDS = 0.2
ROUNDS = 3
dt = torch.float32


def measure(things, min_s):
    """things: name -> callable.  -> (median us, spread % of the rounds) per name, the alternatives alternating."""
    iters = {s: calibrate(fn, min_s) for s, fn in things.items()}
    us_ = {s: [] for s in things}
    for _ in range(ROUNDS):
        for s, fn in things.items():
            us_[s].append(window(fn, iters[s]) / iters[s] * 1e3)
    med = {s: statistics.median(v) for s, v in us_.items()}
    return med, {s: (max(v) - min(v)) / med[s] * 100 for s, v in us_.items()}


def problem(rbd, Bn, T, g):
    """The nominal, a PD law that keeps the closed loop finite, and a cost that tracks the nominal."""
    n = rbd.n

    def rand(shape, lo, hi):
        return (torch.rand(shape, device="cuda", dtype=torch.float64, generator=g) * (hi - lo) + lo).to(dt)

    def randn(shape):
        return torch.randn(shape, device="cuda", dtype=torch.float64, generator=g).to(dt)
    q0r = rand((Bn, n), -0.5, 0.5)
    qd0r = torch.zeros_like(q0r)
    ub = rbd.rnea(q0r, qd0r, qd0r)[0].expand(T, Bn, n).contiguous()                 # holds the robot at q0
    qr, qdr = rbd.rollout(q0r, qd0r, ub, DT)
    kf = 0.01 * randn((T, Bn, n))
    q0 = (q0r + rand((Bn, n), -0.01, 0.01)).contiguous()
    qd0 = rand((Bn, n), -0.01, 0.01)
    eye = torch.eye(n, device="cuda", dtype=dt)
    pd = -torch.cat([50.0 * eye, 5.0 * eye], 1)
    scale = 2.0
    while True:                             # the PD law, halved until the closed loop stays finite
        scale *= 0.5
        assert scale > 1e-3, "no PD scale keeps the closed loop finite"
        K = (scale * pd * (1.0 + 0.01 * randn((T, Bn, n, 2 * n)))).contiguous()
        q, qd, ua = rbd.rollout_closed_loop(q0, qd0, ub, qr, qdr, K, DT, k=kf, q0_ref=q0r, qd0_ref=qd0r)
        if bool(torch.isfinite(q).all() and torch.isfinite(qd).all() and torch.isfinite(ua).all()) and float(q.abs().max()) < 10.0:
            break
    cost = QuadraticCost(w_q=rand((T, Bn, n), 5, 15), w_qd=rand((T, Bn, n), 5, 15), q_target=qr, qd_target=qdr,
                         w_u=rand((T, Bn, n), 1, 2), c_u=rand((T, Bn, n), -1, 1))
    return dict(q0=q0, qd0=qd0, u=ub, q_ref=qr, qd_ref=qdr, K=K, k=kf, q0_ref=q0r, qd0_ref=qd0r), cost, scale, rand, randn


def agree(a, b, tag):
    err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    assert err <= 1e-3, (tag, err)
    return err


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_cost_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rollout_cost.py measures on a GPU; there is nothing to fall back to"
    min_s = 0.01 if a.quick else MIN_SECONDS
    lines = []
    for what, name, Bn, A, T in (QUICK if a.quick else CASES):
        rbd = RBDReference(make_robot(name), build=False)
        n = rbd.n
        g = torch.Generator(device="cuda").manual_seed(Bn + T + A)
        c, cost, scale, rand, randn = problem(rbd, Bn, T, g)
        head = f"{name:10s} {what:11s} B_nom={Bn:5d} {'B' if what == 'mppi' else 'A'}={A:5d} T={T:3d} f32"
        if what == "line search":
            al = torch.linspace(1.0, 1.0 / A, A, device="cuda", dtype=dt) if A > 1 else 1.0
            new = lambda: rbd.rollout_cost(c["q0"], c["qd0"], c["u"], DT, cost, K=c["K"], q_ref=c["q_ref"], qd_ref=c["qd_ref"], k=c["k"],   # noqa: E731
                                           alpha=al, q0_ref=c["q0_ref"], qd0_ref=c["qd0_ref"])
            old = lambda: cost.value(*rbd.rollout_closed_loop(c["q0"], c["qd0"], c["u"], c["q_ref"], c["qd_ref"], c["K"], DT, k=c["k"],   # noqa: E731
                                                              alpha=al, q0_ref=c["q0_ref"], qd0_ref=c["qd0_ref"]))
            stored = 3 * T * max(A, 1) * Bn * n * 4
        elif what == "mppi":
            B = A
            q0, qd0 = c["q0"].expand(B, n).contiguous(), c["qd0"].expand(B, n).contiguous()
            du = 0.1 * randn((T, B, n))
            u1 = c["u"]                                                        # [T, 1, n]
            flat = lambda x: x[:, 0].contiguous()                              # noqa: E731  [T, 1, n] -> [T, n]: shared by every row
            cost = QuadraticCost(w_q=flat(cost.w_q), w_qd=flat(cost.w_qd), q_target=flat(cost.q_target), qd_target=flat(cost.qd_target),
                                 w_u=flat(cost.w_u), c_u=flat(cost.c_u))
            new = lambda: rbd.rollout_cost(q0, qd0, u1, DT, cost, du=du)       # noqa: E731

            def old():
                u = u1 + du
                q, qd = rbd.rollout(q0, qd0, u, DT)
                return cost.value(q, qd, u)
            stored = 3 * T * B * n * 4
        else:
            al = torch.tensor([1, .5, .25, .125, .03125, .0078125][:A], device="cuda", dtype=dt)
            q0, qd0, u = c["q0"], c["qd0"], c["u"]
            J0, q, qd, u = rbd.rollout_cost(q0, qd0, u, DT, cost, return_trajectory=True)
            k, K = rbd.rollout_lqr(q0, qd0, u, DT, q=q, qd=qd, **cost.derivatives(q, qd, u))[:2]
            ra = torch.ones((Bn,), device="cuda", dtype=dt)
            alist = al.tolist()                 # once: reading a device tensor back inside a timed call would synchronise it
            things = {
                "start": lambda: rbd.rollout_cost(q0, qd0, c["u"], DT, cost, return_trajectory=True),
                "lqr": lambda: rbd.rollout_lqr(q0, qd0, u, DT, q=q, qd=qd, **cost.derivatives(q, qd, u)),
                "search": lambda: rbd.rollout_cost(q0, qd0, u, DT, cost, K=K, q_ref=q, qd_ref=qd, k=k, alpha=al),
                "forward": lambda: rbd.rollout_closed_loop(q0, qd0, u, q, qd, K, DT, k=k, row_alpha=ra),
                "ilqr": lambda: rbd.ilqr(q0, qd0, c["u"], DT, cost, iters=1, alphas=alist),
            }
            r = rbd.ilqr(q0, qd0, c["u"], DT, cost, iters=1, alphas=alist)
            assert bool(torch.isfinite(r.cost).all()) and bool((r.cost[1] <= r.cost[0]).all())
            med, spr = measure(things, min_s)
            glue = med["ilqr"] - med["start"] - med["lqr"] - med["search"] - med["forward"]
            line = (f"{head}: one iteration {med['ilqr'] - med['start']:9.1f} us = rollout_lqr (with cost.derivatives) {med['lqr']:9.1f} us "
                    f"(+-{spr['lqr']:4.1f}%) + line search {med['search']:9.1f} us (+-{spr['search']:4.1f}%) + forward pass "
                    f"{med['forward']:9.1f} us (+-{spr['forward']:4.1f}%) + torch glue {glue:8.1f} us | the start's rollout_cost "
                    f"{med['start']:9.1f} us (+-{spr['start']:4.1f}%); ilqr(iters=1) {med['ilqr']:9.1f} us (+-{spr['ilqr']:4.1f}%); rows accepted "
                    f"{int((r.alpha[0] > 0).sum())} of {Bn}, mean cost {float(r.cost[0].mean()):.3f} -> {float(r.cost[1].mean()):.3f}")
            print(line, flush=True)
            lines.append(line)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            continue
        Ja, Jb = new(), old()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(Ja).all()), (name, what, "the cost is not finite")
        diff = agree(Ja, Jb, (name, what))
        med, spr = measure({"new": new, "old": old}, min_s)
        margin = (med["old"] - med["new"]) / med["old"] * 100
        met = med["new"] < med["old"] and margin > spr["new"] + spr["old"]
        verdict = ("met" if met else "MISSED") if name == "iiwa_like" else "reported"
        line = (f"{head} PD x{scale:g}: (a) rollout_cost {med['new']:9.1f} us (+-{spr['new']:4.1f}%) | (b) rollout + QuadraticCost.value "
                f"{med['old']:9.1f} us (+-{spr['old']:4.1f}%), {stored / 1e6:6.1f} MB of trajectory stored = {med['old'] / med['new']:5.2f}x (a): "
                f"{verdict} | (a) vs (b) {diff:.1e} relative")
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                      # after every case: a later case that stops keeps the earlier lines
            fh.write("\n".join(lines) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
