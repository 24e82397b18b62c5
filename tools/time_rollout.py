#!/usr/bin/env python3
"""HIP-event timings of rbd_rollout against what it replaces.

    python tools/time_rollout.py [--out profiles/rollout_time.txt] [--quick]
Run it under a time limit (timeout -k 10 600 ...).  Per case it times three things, ALTERNATING in one process (three
rounds of rollout, aba, loop; every round of every thing is at least 0.2 s of back-to-back launches between two device
events, after a warm-up of the same launches; the median round is reported, the spread of the rounds beside it):
    rollout   one rbd_rollout launch through the C-ABI (semi-implicit Euler, trajectory written), total and per step
    aba       one rbd_aba launch through the C-ABI at the same B (pre-allocated output)
    loop      what a user wrote before rollout existed, on the Python API: per step RBDReference.aba, the two in-place
              torch updates, and two copies into a [T, B, n] buffer
    bytes     what the algorithm has to move: (2 n + 2 n + T 3 n) B s -- q0 and qd0 in, the final state out, and per
              step u in and q, qd out -- and the rate over the rollout time
    goal      rollout <= 1.10 T aba: a step moves fewer bytes than an aba call and adds 2 n FMAs to its arithmetic; the
              10 % is for box-to-box spread.  The ratio to the loop is reported, not gated.
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

CASES = [("iiwa_like", torch.float32, 4096, 32), ("iiwa_like", torch.float32, 65536, 32), ("iiwa_like", torch.float32, 1048576, 16),
         ("quadruped_like", torch.float64, 65536, 32), ("atlas_like", torch.float32, 16384, 32)]
QUICK = [("iiwa_like", torch.float32, 130, 3), ("atlas_like", torch.float32, 130, 3)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_time.txt"))
    ap.add_argument("--quick", action="store_true", help="tiny shapes, short windows: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rollout.py measures on a GPU; there is nothing to fall back to"
    min_s = 0.01 if a.quick else MIN_SECONDS
    lines = []
    for name, dt, B, T in (QUICK if a.quick else CASES):
        rbd = RBDReference(make_robot(name), build=False)
        lib = rbd._lib.lib
        n = rbd.n
        esz = 4 if dt == torch.float32 else 8
        sfx = "f32" if esz == 4 else "f64"
        g = torch.Generator(device="cuda").manual_seed(B + T)
        q0 = ((torch.rand((B, n), device="cuda", dtype=torch.float64, generator=g) * 2 - 1) * 3.14159).to(dt)
        qd0 = (torch.rand((B, n), device="cuda", dtype=torch.float64, generator=g) * 2 - 1).to(dt)
        u = ((torch.rand((T, B, n), device="cuda", dtype=torch.float64, generator=g) * 2 - 1) * 5).to(dt)
        q_out, qd_out = (torch.empty((T, B, n), device="cuda", dtype=dt) for _ in range(2))
        qdd = torch.empty((B, n), device="cuda", dtype=dt)
        q_loop, qd_loop = (torch.empty((T, B, n), device="cuda", dtype=dt) for _ in range(2))
        st = torch.cuda.current_stream().cuda_stream
        f_roll = getattr(lib, f"rbd_rollout_{sfx}")
        f_aba = getattr(lib, f"rbd_aba_{sfx}")

        def roll():
            return f_roll(q0.data_ptr(), qd0.data_ptr(), u.data_ptr(), 0, DT, -9.81, 0, B, T, q_out.data_ptr(), qd_out.data_ptr(), 1, st)

        def aba():
            return f_aba(q0.data_ptr(), qd0.data_ptr(), u.data_ptr(), -9.81, B, qdd.data_ptr(), st)

        def loop():
            q, qd = q0.clone(), qd0.clone()
            for t in range(T):
                acc = rbd.aba(q, qd, u[t])
                qd.add_(acc, alpha=DT)
                q.add_(qd, alpha=DT)
                q_loop[t].copy_(q)
                qd_loop[t].copy_(qd)

        assert roll() == 0 and aba() == 0, lib.rbd_last_error()
        loop()
        torch.cuda.synchronize()
        # the loop and the kernel integrate the same thing (fused vs separate multiply-add: last bits only, then the dynamics
        # amplify them over T steps)
        diff = float((q_loop[0].double() - q_out[0].double()).abs().max())
        assert diff <= (1e-5 if esz == 4 else 1e-13) * max(1.0, float(q_out[0].abs().max())), diff
        things = {"rollout": roll, "aba": aba, "loop": loop}
        iters = {k: calibrate(f, min_s) for k, f in things.items()}
        us = {k: [] for k in things}
        for _ in range(ROUNDS):
            for k, f in things.items():
                us[k].append(window(f, iters[k]) / iters[k] * 1e3)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: (max(v) - min(v)) / med[k] * 100 for k, v in us.items()}
        by = (2 * n + 2 * n + T * 3 * n) * B * esz
        goal = 1.10 * T * med["aba"]
        line = (f"{name:15s} B={B:8d} T={T:3d} {sfx}: rollout {med['rollout']:10.1f} us ({med['rollout'] / T:8.2f} us/step, +-{spread['rollout']:4.1f}%) | "
                f"aba {med['aba']:8.2f} us (+-{spread['aba']:4.1f}%) | python loop {med['loop']:10.1f} us (+-{spread['loop']:4.1f}%), "
                f"{med['loop'] / med['rollout']:5.2f}x rollout | {by / 1e6:8.1f} MB  {by / med['rollout'] / 1e6:5.2f} TB/s | "
                f"goal <= 1.10 T aba = {goal:10.1f} us: {'met' if med['rollout'] <= goal else 'MISSED'}")
        print(line, flush=True)
        lines.append(line)
        del q_out, qd_out, q_loop, qd_loop, u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
