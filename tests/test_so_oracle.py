"""Second-order inverse-dynamics derivatives without a GPU: the numpy restatement (tests/so_oracle.py) against the
fixtures of the real reference (tests/golden/so_*.npz, tools/gen_golden_so.py) and against central differences of the
first-order oracle (oracle/rbd_oracle.py), which pins the corrected composite-force index; plus the host-side
behaviour of RBDReference.second_order_idsva_parallel and the build plumbing."""
import os

import numpy as np
import pytest

from conftest import make_robot
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from so_oracle import SO_ROBOTS, SOOracle, unbranched

pytestmark = pytest.mark.filterwarnings("ignore::PendingDeprecationWarning")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("d2tau_dq", "d2tau_dqd", "d2tau_dvdq", "dM_dq")
UNBRANCHED = ["iiwa_like", "quadruped_like", "random_chain_n7", "random_twochains_n18"]
BRANCHED = [r for r in SO_ROBOTS if r not in UNBRANCHED]


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"so_{name}.npz")))


def _rel(x, r):
    return float(np.max(np.abs(x - r)) / np.max(np.abs(r)))


def test_fixture_robots_and_unbranched_flag():
    assert sorted(UNBRANCHED + BRANCHED) == sorted(SO_ROBOTS) and len(SO_ROBOTS) == 9
    for name in SO_ROBOTS:
        g = _load(name)
        assert bool(g["unbranched"]) == (name in UNBRANCHED) == unbranched(make_robot(name))
        n = make_robot(name).get_num_joints()
        assert g["q"].shape == (8 if n <= 9 else 4, n)
        for k in KEYS:
            assert g[k].shape == g["q"].shape[:1] + (n, n, n)


@pytest.mark.parametrize("name", SO_ROBOTS)
def test_oracle_reproduces_the_reference_fixtures(name):
    """All four outputs where the reference's :1448 index is right; the three that never read f everywhere."""
    g = _load(name)
    out = SOOracle(make_robot(name))(g["q"], g["qd"], g["qdd"], float(g["gravity"]))
    keys = KEYS if name in UNBRANCHED else KEYS[1:]
    for k, x in zip(KEYS, out):
        if k in keys:
            assert _rel(x, g[k]) <= 1e-12, (name, k, _rel(x, g[k]))


@pytest.mark.parametrize("name", BRANCHED)
def test_branched_d2tau_dq_differs_from_the_reference_on_purpose(name):
    """The decision of DESIGN.md §4.9: the reference's f[:, pi + 1] (:1448) makes its d2tau_dq wrong on branched robots;
    this package returns the derivative.  The restatement with the reference's index reproduces the fixture."""
    g = _load(name)
    o = SOOracle(make_robot(name))
    ours = o(g["q"], g["qd"], g["qdd"], float(g["gravity"]))[0]
    assert _rel(ours, g["d2tau_dq"]) > 1e-2
    as_ref = o(g["q"], g["qd"], g["qdd"], float(g["gravity"]), fix_f=False)[0]
    assert _rel(as_ref, g["d2tau_dq"]) <= 1e-12


@pytest.mark.parametrize("name", SO_ROBOTS)
def test_oracle_is_the_derivative_of_rnea_rnea_grad_and_crba(name):
    """Central differences, every perturbation of a robot in one oracle call: d2tau_dq against second differences of
    rnea's c (never of rnea_grad's dc_dq, which is not the q-derivative of c for prismatic joints), d2tau_dqd and
    d2tau_dvdq against first differences of rnea_grad's dc_dqd, dM_dq against first differences of crba."""
    g = _load(name)
    robot = make_robot(name)
    om = orc.model_from_robot(robot)
    n = robot.get_num_joints()
    q, qd, qdd = g["q"][0], g["qd"][0], g["qdd"][0]
    d2q, d2qd, d2vq, dM = SOOracle(robot)(q, qd, qdd, -9.81)
    E = np.eye(n)
    h2 = 1e-4                                        # second differences of c: 4 rows per (j, k)
    sj = np.array([1, 1, -1, -1])[:, None]
    sk = np.array([1, -1, 1, -1])[:, None]
    Q = (q[None, None, None] + h2 * (sj[None, None] * E[:, None, None] + sk[None, None] * E[None, :, None]))
    Q = Q.reshape(-1, n)
    m = Q.shape[0]
    c = orc.rnea(om, Q, np.broadcast_to(qd, (m, n)), np.broadcast_to(qdd, (m, n)), -9.81)[0].reshape(n, n, 4, n)
    fd_q = (c[:, :, 0] - c[:, :, 1] - c[:, :, 2] + c[:, :, 3]) / (4 * h2 * h2)     # [j, k, i]
    assert _rel(d2q, fd_q.transpose(2, 0, 1)) <= 1e-6
    h1 = 1e-6                                        # first differences: q_k +- h, qd_j +- h
    Qk = np.concatenate([q + h1 * E, q - h1 * E])
    dc = orc.rnea_grad(om, Qk, np.broadcast_to(qd, (2 * n, n)), np.broadcast_to(qdd, (2 * n, n)), -9.81)
    dc_dqd = dc[:, :, n:]
    fd_vq = (dc_dqd[:n] - dc_dqd[n:]) / (2 * h1)                                   # [k, i, j]
    assert _rel(d2vq, fd_vq.transpose(1, 2, 0)) <= 1e-6
    Qd = np.concatenate([qd + h1 * E, qd - h1 * E])
    dcv = orc.rnea_grad(om, np.broadcast_to(q, (2 * n, n)), Qd, np.broadcast_to(qdd, (2 * n, n)), -9.81)[:, :, n:]
    fd_qd = (dcv[:n] - dcv[n:]) / (2 * h1)                                        # [k, i, j]
    assert _rel(d2qd, fd_qd.transpose(1, 2, 0)) <= 1e-6
    H = orc.crba(om, Qk)
    fd_M = (H[:n] - H[n:]) / (2 * h1)                                             # [k, i, j]
    assert _rel(dM, fd_M.transpose(1, 2, 0)) <= 1e-6


def test_oracle_identities():
    """Symmetries and qdd-independence that hold exactly in the reference's output (ISSUE: exact identities)."""
    for name in ("atlas_like", "random_prismatic_n6"):
        g = _load(name)
        o = SOOracle(make_robot(name))
        d2q, d2qd, d2vq, dM = o(g["q"], g["qd"], g["qdd"])
        _, d2qd2, d2vq2, dM2 = o(g["q"], g["qd"], 3.0 * g["qdd"] + 1.0)
        assert np.allclose(d2q, d2q.transpose(0, 1, 3, 2), rtol=0, atol=1e-12 * np.abs(d2q).max())
        assert np.allclose(d2qd, d2qd.transpose(0, 1, 3, 2), rtol=0, atol=1e-12 * np.abs(d2qd).max())
        assert np.allclose(dM, dM.transpose(0, 2, 1, 3), rtol=0, atol=1e-12 * np.abs(dM).max())
        for a, b in ((d2qd, d2qd2), (d2vq, d2vq2), (dM, dM2)):
            assert np.allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())


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
        api.second_order_idsva_parallel(q, q, q)


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, _declare  # noqa: F401
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_second_order_idsva") == "so"
    assert FAMILIES["so"] == ["SO"] and "SO" in _ALL_FAMILY_UNITS
    assert "SO_F32" in TRANSLATION_UNITS and "SO_F64" in TRANSLATION_UNITS
    assert {"rbd_second_order_idsva_f32", "rbd_second_order_idsva_f64"} <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "rbd_hip.h")).read()
    assert "int rbd_second_order_idsva_f32(" in hdr and "int rbd_second_order_idsva_f64(" in hdr
