#!/usr/bin/env python3
"""Generate tests/golden/ee_<robot>.npz from the REAL reference's end-effector kinematics.

Like oracle/gen_golden.py: the reference (``RBDReference.py``, imported by path from ``RBD_REFERENCE_DIR``, default
``/root/reference``) is fed this package's ``Robot`` objects -- the fixture robots of tests/ee_oracle.py, i.e. the
robots whose libraries build() makes, with two fixed frames attached -- and ``end_effector_pose`` (:220-274) /
``end_effector_pose_gradient`` (:286-386) run one configuration at a time, as a user of the reference would.

    python tools/gen_golden_ee.py [robot ...]     # rewrites tests/golden/ee_<robot>.npz (all by default)

Fixture contents (S = 16 samples, n = DoF, L = leaves, 4 = sites of the named selection):
    q                              [S, n]        inputs, uniform(-pi, pi)
    pose_default, grad_default     [S, L, 6], [S, L, 6, n]   default leaf selection
    names                          [4]           named selection (fixed and movable joints mixed)
    pose_named, grad_named         [S, 4, 6], [S, 4, 6, n]
    offset                         [4]           ee_offsets[0] of the last pair
    pose_offset, grad_offset       [S, L, 6], [S, L, 6, n]   default selection with that offset
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_SAMPLES = 16


def reference_class():
    sys.path.insert(0, os.environ.get("RBD_REFERENCE_DIR", "/root/reference"))
    from RBDReference import RBDReference
    return RBDReference


def generate(name, Ref=None):
    from ee_oracle import OFFSET, ee_robot, named_selection
    Ref = Ref or reference_class()
    robot = ee_robot(name)
    n = robot.get_num_joints()
    ref = Ref(robot)
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    q = rng.uniform(-np.pi, np.pi, (N_SAMPLES, n))
    names = named_selection(robot)
    off = np.matrix([list(OFFSET)])
    out = {"q": q, "names": np.array(names), "offset": np.array(OFFSET, dtype=np.float64)}
    for tag, sel, offs in (("default", None, None), ("named", names, None), ("offset", None, [off])):
        kw = {} if offs is None else {"ee_offsets": offs}
        P = [np.stack([np.asarray(x, dtype=np.float64).reshape(6) for x in ref.end_effector_pose(q[s], sel, **kw)])
             for s in range(N_SAMPLES)]
        G = [np.stack([np.asarray(x, dtype=np.float64).reshape(6, n) for x in ref.end_effector_pose_gradient(q[s], sel, **kw)])
             for s in range(N_SAMPLES)]
        out[f"pose_{tag}"] = np.stack(P)
        out[f"grad_{tag}"] = np.stack(G)
    return out


def main(argv):
    from ee_oracle import EE_ROBOTS
    Ref = reference_class()
    for name in (argv or EE_ROBOTS):
        out = generate(name, Ref)
        path = os.path.join(GOLDEN, f"ee_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
