"""Second-order forward-dynamics derivatives without a GPU: the numpy restatement (tests/fdso_oracle.py) against the
fixtures of the real reference (tests/golden/fdso_*.npz, tools/gen_golden_fdso.py) and against central differences of the
first-order oracle (oracle/rbd_oracle.py); plus the host-side behaviour of RBDReference.fdsva_so and the build plumbing."""
import os

import numpy as np
import pytest

from conftest import make_robot
from fdso_oracle import FDSOOracle, contract, has_prismatic, ingredients, n_samples
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from so_oracle import SO_ROBOTS, unbranched

pytestmark = pytest.mark.filterwarnings("ignore::PendingDeprecationWarning")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("daba_dqdq", "daba_dvdq", "daba_dvdv", "daba_dtdq")
UNBRANCHED = ["iiwa_like", "quadruped_like", "random_chain_n7", "random_twochains_n18"]
BRANCHED = [r for r in SO_ROBOTS if r not in UNBRANCHED]
PRISMATIC = ["random_prismatic_n6"]


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"fdso_{name}.npz")))


def _rel(x, r):
    return float(np.max(np.abs(x - r)) / np.max(np.abs(r)))


def test_fixture_robots_shapes_and_flags():
    assert sorted(UNBRANCHED + BRANCHED) == sorted(SO_ROBOTS) and len(SO_ROBOTS) == 9
    for name in SO_ROBOTS:
        g = _load(name)
        robot = make_robot(name)
        n = robot.get_num_joints()
        assert bool(g["unbranched"]) == (name in UNBRANCHED) == unbranched(robot)
        assert bool(g["has_prismatic"]) == (name in PRISMATIC) == has_prismatic(robot)
        S = 8 if n <= 9 else 4 if 12 <= n <= 18 else 2
        assert S == n_samples(n) and (n <= 18 or name == "atlas_like")
        assert float(g["gravity"]) == -9.81
        for k in ("q", "qd", "u"):
            assert g[k].shape == (S, n) and g[k].dtype == np.float64
        for k in KEYS:
            assert g[k].shape == (S, n, n, n) and g[k].dtype == np.float64


@pytest.mark.parametrize("name", SO_ROBOTS)
def test_oracle_reproduces_the_reference_fixtures(name):
    """All four outputs on the unbranched robots; the three that never read the composite force everywhere."""
    g = _load(name)
    out = FDSOOracle(make_robot(name))(g["q"], g["qd"], g["u"], float(g["gravity"]))
    keys = KEYS if name in UNBRANCHED else KEYS[1:]
    for k, x in zip(KEYS, out):
        e = _rel(x, g[k])
        print(name, k, f"{e:.2e}")
        if k in keys:
            assert e <= 1e-10, (name, k, e)


@pytest.mark.parametrize("name", BRANCHED)
def test_branched_daba_dqdq_differs_from_the_reference_on_purpose(name):
    """Decision 1: fdsva_so composes this package's second_order_idsva, whose composite-force
    sweep adds the child's force.  The restatement with the reference's :1448 index reproduces the fixture."""
    g = _load(name)
    o = FDSOOracle(make_robot(name))
    ours = o(g["q"], g["qd"], g["u"], float(g["gravity"]))[0]
    as_ref = o(g["q"], g["qd"], g["u"], float(g["gravity"]), fix_f=False)[0]
    print(name, f"default {_rel(ours, g['daba_dqdq']):.2e}  fix_f=False {_rel(as_ref, g['daba_dqdq']):.2e}")
    assert _rel(ours, g["daba_dqdq"]) > 1e-4
    assert _rel(as_ref, g["daba_dqdq"]) <= 1e-10


def _fd_grad(om, Q, QD, U):
    """The oracle's forward_dynamics_grad at the default gravity, as one [m, n, 2n] array."""
    a, b = orc.forward_dynamics_grad(om, Q, QD, U)
    return np.concatenate([a, b], -1)


def test_oracle_is_the_derivative_of_forward_dynamics_grad_and_minv():
    """Central differences (h = 1e-6) on each fixture's first sample: daba_dqdq, daba_dvdq against differences in q of
    fd_dq, fd_dqd; daba_dvdv against differences in qd of fd_dqd; daba_dtdq against differences in q of minv.  Left out:
    daba_dqdq on robots with a prismatic joint (decision 2: forward_dynamics_grad's qdd_dq is not the q-derivative
    there) -- for that pair the contraction is fed the central-difference qdd_dq of forward_dynamics and checked against
    second differences (h = 1e-4) of forward_dynamics."""
    left_out = 0
    for name in SO_ROBOTS:
        g = _load(name)
        robot = make_robot(name)
        om = orc.model_from_robot(robot)
        n = robot.get_num_joints()
        q, qd, u = g["q"][0], g["qd"][0], g["u"][0]
        dqq, dvq, dvv, dtq = FDSOOracle(robot)(q, qd, u)
        E = np.eye(n)
        h = 1e-6
        bc = lambda x: np.broadcast_to(x, (2 * n, n))      # noqa: E731
        Qk = np.concatenate([q + h * E, q - h * E])
        d = _fd_grad(om, Qk, bc(qd), bc(u))
        fdq = ((d[:n] - d[n:]) / (2 * h)).transpose(1, 2, 0)            # [i, j | n + j, k]
        Mi = orc.minv(om, Qk)
        fd_M = ((Mi[:n] - Mi[n:]) / (2 * h)).transpose(1, 2, 0)
        Qd = np.concatenate([qd + h * E, qd - h * E])
        dv = _fd_grad(om, bc(q), Qd, bc(u))[:, :, n:]
        fd_vv = ((dv[:n] - dv[n:]) / (2 * h)).transpose(1, 2, 0)
        checks = [("daba_dqdq", dqq, fdq[:, :n]), ("daba_dvdq", dvq, fdq[:, n:]), ("daba_dvdv", dvv, fd_vv),
                  ("daba_dtdq", dtq, fd_M)]
        for key, x, r in checks:
            e = _rel(x, r)
            print(name, key, f"{e:.2e}")
            if key == "daba_dqdq" and has_prismatic(robot):
                left_out += 1
                continue
            assert e <= 1e-6, (name, key, e)
        if has_prismatic(robot):
            # the contraction is right, the inherited input is what it is
            h1 = 1e-6
            Qk = np.concatenate([q + h1 * E, q - h1 * E])
            a = orc.forward_dynamics(om, Qk, bc(qd), bc(u))
            qdd_dq = ((a[:n] - a[n:]) / (2 * h1)).T                                  # [i, j]
            Minv, _, _, fd_dqd, d2q, d2qd, d2vq, dM = ingredients(om, q[None], qd[None], u[None])
            fed = contract(Minv[0], qdd_dq, fd_dqd[0], d2q[0], d2qd[0], d2vq[0], dM[0])[0]
            h2 = 1e-4
            sj = np.array([1, 1, -1, -1])[:, None]
            sk = np.array([1, -1, 1, -1])[:, None]
            Q = (q[None, None, None] + h2 * (sj[None, None] * E[:, None, None] + sk[None, None] * E[None, :, None])).reshape(-1, n)
            m = Q.shape[0]
            a = orc.forward_dynamics(om, Q, np.broadcast_to(qd, (m, n)), np.broadcast_to(u, (m, n))).reshape(n, n, 4, n)
            sd = ((a[:, :, 0] - a[:, :, 1] - a[:, :, 2] + a[:, :, 3]) / (4 * h2 * h2)).transpose(2, 0, 1)
            e = _rel(fed, sd)
            print(name, "daba_dqdq fed central-difference qdd_dq vs second differences", f"{e:.2e}")
            assert e <= 1e-5, (name, e)
    assert left_out == 1                       # exactly one of the 36 robot x output pairs


def test_oracle_identities():
    """Symmetries and u-independence that hold exactly."""
    for name in ("atlas_like", "random_prismatic_n6", "random_forest_n8"):
        g = _load(name)
        o = FDSOOracle(make_robot(name))
        dqq, dvq, dvv, dtq = o(g["q"], g["qd"], g["u"])
        _, _, dvv2, dtq2 = o(g["q"], g["qd"], 3.0 * g["u"] + 1.0)
        assert np.allclose(dqq, dqq.transpose(0, 1, 3, 2), rtol=0, atol=1e-12 * np.abs(dqq).max())
        assert np.allclose(dvv, dvv.transpose(0, 1, 3, 2), rtol=0, atol=1e-12 * np.abs(dvv).max())
        assert np.allclose(dtq, dtq.transpose(0, 2, 1, 3), rtol=0, atol=1e-12 * np.abs(dtq).max())
        for a, b in ((dvv, dvv2), (dtq, dtq2)):
            assert np.allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())


def test_oracle_carries_gravity_through_every_stage():
    """Decision 3: at another gravity the derivative check still holds, with forward dynamics restated at that gravity."""
    robot = make_robot("random_tree_n9")
    om = orc.model_from_robot(robot)
    g = _load("random_tree_n9")
    n = 9
    q, qd, u = g["q"][1], g["qd"][1], g["u"][1]
    grav = -3.7
    dqq = FDSOOracle(robot)(q, qd, u, grav)[0]
    h = 1e-6
    E = np.eye(n)
    Qk = np.concatenate([q + h * E, q - h * E])
    bc = lambda x: np.broadcast_to(x, (2 * n, n))      # noqa: E731
    fd_dq = ingredients(om, Qk, bc(qd), bc(u), grav)[2]
    fd = ((fd_dq[:n] - fd_dq[n:]) / (2 * h)).transpose(1, 2, 0)
    assert _rel(dqq, fd) <= 1e-6
    assert _rel(FDSOOracle(robot)(q, qd, u)[0], fd) > 1e-3


def test_api_refuses_floating_base_before_any_launch():
    from rbdreference_amd.api import RBDReference
    from rbdreference_amd.robot import floating_quadruped_like
    api = RBDReference.__new__(RBDReference)
    api.robot = floating_quadruped_like()
    api.model = pack_robot(api.robot)
    api.n = api.model.n
    api.nv = api.model.nv
    q = np.zeros(api.nv)
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.fdsva_so(q, q, q)


def test_family_and_exports():
    import re
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, _declare  # noqa: F401
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_fdsva_so") == "fdso"
    assert FAMILIES["fdso"][0] == "FDSO" and set(FAMILIES["fdso"]) == {"FDSO", "SO", "FD", "RNEA", "MINV"}
    assert "FDSO" in _ALL_FAMILY_UNITS
    assert "FDSO_F32" in TRANSLATION_UNITS and "FDSO_F64" in TRANSLATION_UNITS
    assert FAMILIES["so"] == ["SO"] and FAMILIES["fd"] == ["FD", "RNEA", "MINV"]
    names = {"rbd_fdsva_so_workspace_bytes", "rbd_fdsva_so_f32", "rbd_fdsva_so_f64"}
    assert names <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "rbd_hip.h")).read()
    assert "size_t rbd_fdsva_so_workspace_bytes(int64_t B, int elem_size);" in hdr
    assert "int rbd_fdsva_so_f32(" in hdr and "int rbd_fdsva_so_f64(" in hdr
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert names <= found and found == set(EXPORTED_SYMBOLS)
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2
