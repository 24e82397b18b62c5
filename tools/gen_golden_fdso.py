#!/usr/bin/env python3
"""Generate tests/golden/fdso_<robot>.npz from the REAL reference's fdsva_so.

Like tools/gen_golden_so.py: the reference (``RBDReference.py``, imported by path from ``RBD_REFERENCE_DIR``, default
``/root/reference``) is fed this package's ``Robot`` objects -- the nine fixed-base fixture robots of
tests/so_oracle.py, i.e. robots whose libraries build() makes -- and ``fdsva_so`` (:1606-1631) runs one configuration
at a time, as a user of the reference would.

    python tools/gen_golden_fdso.py [robot ...]     # rewrites tests/golden/fdso_<robot>.npz (all by default)

Fixture contents (S = 8 samples for n <= 9, 4 for 12 <= n <= 18, 2 for the 30-body robot; n = DoF):
    q, qd, u                                      [S, n]        inputs: q uniform(-pi, pi), qd uniform(-1, 1), u uniform(-5, 5)
    gravity                                       []            GRAVITY passed to the reference (the default, where its
                                                                forward dynamics, fixed at -9.81, agrees with it)
    daba_dqdq, daba_dvdq, daba_dvdv, daba_dtdq    [S, n, n, n]  the reference's outputs as returned
    unbranched                                    []            every non-root body i has parent i - 1: the reference's
                                                                :1448 index is then right and daba_dqdq is comparable
    has_prismatic                                 []            the robot has a prismatic joint: daba_dqdq inherits
                                                                rnea_grad's dc_dq, which is then not the q-derivative
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
KEYS = ("daba_dqdq", "daba_dvdq", "daba_dvdv", "daba_dtdq")


def reference_class():
    sys.path.insert(0, os.environ.get("RBD_REFERENCE_DIR", "/root/reference"))
    from RBDReference import RBDReference
    return RBDReference


def generate(name, Ref=None):
    from conftest import make_robot
    from fdso_oracle import has_prismatic, n_samples
    from so_oracle import unbranched
    Ref = Ref or reference_class()
    robot = make_robot(name)
    n = robot.get_num_joints()
    ref = Ref(robot)
    S = n_samples(n)
    rng = np.random.default_rng(3000 + sum(map(ord, name)))
    q = rng.uniform(-np.pi, np.pi, (S, n))
    qd = rng.uniform(-1, 1, (S, n))
    u = rng.uniform(-5, 5, (S, n))
    outs = [ref.fdsva_so(q[s], qd[s], u[s], GRAVITY) for s in range(S)]
    out = {"q": q, "qd": qd, "u": u, "gravity": np.float64(GRAVITY), "unbranched": np.bool_(unbranched(robot)),
           "has_prismatic": np.bool_(has_prismatic(robot))}
    for t, key in enumerate(KEYS):
        out[key] = np.stack([np.asarray(o[t], dtype=np.float64) for o in outs])
    return out


def main(argv):
    from so_oracle import SO_ROBOTS
    Ref = reference_class()
    for name in (argv or SO_ROBOTS):
        out = generate(name, Ref)
        path = os.path.join(GOLDEN, f"fdso_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
