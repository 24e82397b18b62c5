#!/usr/bin/env python3
"""Generate tests/golden/so_<robot>.npz from the REAL reference's second_order_idsva_parallel.

Like tools/gen_golden_ee.py: the reference (``RBDReference.py``, imported by path from ``RBD_REFERENCE_DIR``, default
``/root/reference``) is fed this package's ``Robot`` objects -- the nine fixed-base fixture robots of
tests/so_oracle.py, i.e. robots whose libraries build() makes -- and ``second_order_idsva_parallel`` (:1387-1604) runs
one configuration at a time, as a user of the reference would.

    python tools/gen_golden_so.py [robot ...]     # rewrites tests/golden/so_<robot>.npz (all by default)

Fixture contents (S = 8 samples for n <= 9, else 4; n = DoF):
    q, qd, qdd                                    [S, n]        inputs: q uniform(-pi, pi), qd, qdd uniform(-1, 1)
    gravity                                       []            GRAVITY passed to the reference
    d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq        [S, n, n, n]  the reference's outputs as returned
    unbranched                                    []            every non-root body i has parent i - 1: the
                                                                reference's :1448 index is then right and its
                                                                d2tau_dq is the true derivative
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GRAVITY = -9.81


def reference_class():
    sys.path.insert(0, os.environ.get("RBD_REFERENCE_DIR", "/root/reference"))
    from RBDReference import RBDReference
    return RBDReference


def generate(name, Ref=None):
    from conftest import make_robot
    from so_oracle import unbranched
    Ref = Ref or reference_class()
    robot = make_robot(name)
    n = robot.get_num_joints()
    ref = Ref(robot)
    S = 8 if n <= 9 else 4
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    q = rng.uniform(-np.pi, np.pi, (S, n))
    qd = rng.uniform(-1, 1, (S, n))
    qdd = rng.uniform(-1, 1, (S, n))
    outs = [ref.second_order_idsva_parallel(q[s], qd[s], qdd[s], GRAVITY) for s in range(S)]
    out = {"q": q, "qd": qd, "qdd": qdd, "gravity": np.float64(GRAVITY), "unbranched": np.bool_(unbranched(robot))}
    for t, key in enumerate(("d2tau_dq", "d2tau_dqd", "d2tau_dvdq", "dM_dq")):
        out[key] = np.stack([np.asarray(o[t], dtype=np.float64) for o in outs])
    return out


def main(argv):
    from so_oracle import SO_ROBOTS
    Ref = reference_class()
    for name in (argv or SO_ROBOTS):
        out = generate(name, Ref)
        path = os.path.join(GOLDEN, f"so_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
