"""rollout without a GPU: build wiring, the C-ABI's refusals (every check comes before the launch, so fake pointers are
never dereferenced), the API's refusals, and the numpy restatement the GPU tests compare against."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from rollout_oracle import INTEGRATORS, rest_bounds, rollout, step

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_INTEGRATORS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_rollout") == "roll"
    assert FAMILIES["roll"] == ["ROLL"]
    assert "ROLL" in _ALL_FAMILY_UNITS
    assert "ROLL_F32" in TRANSLATION_UNITS and "ROLL_F64" in TRANSLATION_UNITS
    assert "ROLL_F32" in _TU_COST and "ROLL_F64" in _TU_COST
    assert family_of("rbd_aba") == "fd" and FAMILIES["fd"] == ["FD", "RNEA", "MINV"]      # untouched
    names = {"rbd_rollout_f32", "rbd_rollout_f64"}
    assert names <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert "int rbd_rollout_f32(" in hdr and "int rbd_rollout_f64(" in hdr
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert names <= found and found == set(EXPORTED_SYMBOLS)
    assert "#define RBD_INTEGRATOR_SEMI_IMPLICIT 0" in hdr and "#define RBD_INTEGRATOR_EULER 1" in hdr
    assert RBD_INTEGRATORS == {"semi_implicit": 0, "euler": 1} and tuple(RBD_INTEGRATORS) == INTEGRATORS
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # an addition: the ABI version stays


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_roll_family_library_refuses_bad_arguments_before_any_launch(sfx, ft):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "roll", sfx)
    assert p == family_lib_path(m, "roll", sfx) and os.path.exists(p)
    lib = ctypes.CDLL(p)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 6
    assert lib.rbd_abi_version() == 2
    fn = getattr(lib, f"rbd_rollout_{sfx}")
    other = getattr(lib, f"rbd_rollout_{'f64' if sfx == 'f32' else 'f32'}")
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first

    def call(q0=fake, qd0=fake, u=fake, shared=0, dt=0.01, g=-9.81, integ=0, B=4, T=3, q=fake, qd=fake, traj=1):
        return fn(q0, qd0, u, shared, dt, g, integ, B, T, q, qd, traj, None)

    def refused(msg, **kw):
        assert call(**kw) == RBD_ERR_ARG, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    for name in ("q0", "qd0", "u", "q", "qd"):
        refused(b"must be non-null", **{name: None})
    refused(b"B < 0", B=-1)
    refused(b"T < 0", T=-1)
    for bad in (float("inf"), float("-inf"), float("nan")):
        refused(b"dt must be finite", dt=bad)
    for bad in (-1, 2, 7):
        refused(b"unknown integrator", integ=bad)
    refused(b"B too large", B=2 ** 62)
    refused(b"B * T * n too large", B=2 ** 30, T=2 ** 40)
    refused(b"B * T * n too large", B=1, T=2 ** 62)
    refused(b"16-byte aligned", q=ctypes.c_void_p(4096 + 8))
    # nothing to do: success, nothing touched (not even the null pointers)
    assert call(B=0) == 0 and call(T=0) == 0 and call(B=0, T=0, traj=0) == 0
    assert fn(None, None, None, 0, 0.01, -9.81, 0, 0, 5, None, None, 1, None) == 0
    assert fn(None, None, None, 1, 0.01, -9.81, 1, 5, 0, None, None, 0, None) == 0
    # the other precision is another family library's
    assert other(fake, fake, fake, 0, 0.01, -9.81, 0, 4, 3, fake, fake, 1, None) == -4
    assert b"not part of this family library" in lib.rbd_last_error()


def _bare_api(robot):
    from rbdreference_amd.api import RBDReference
    api = RBDReference.__new__(RBDReference)
    api.robot = robot
    api.model = pack_robot(robot)
    api.n = api.model.n
    api.nv = api.model.nv
    return api


def test_api_refuses_floating_base_before_any_launch():
    from rbdreference_amd.robot import floating_quadruped_like
    api = _bare_api(floating_quadruped_like())
    q = np.zeros(api.nv)
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout(q, q, np.zeros((3, api.nv)), 0.01)


def test_api_refuses_bad_shapes_and_integrators_before_any_launch():
    api = _bare_api(make_robot("iiwa_like"))
    n, B, T = 7, 5, 3
    q, u = np.zeros((B, n)), np.zeros((T, B, n))
    bad = [
        (q, q, np.zeros((0, B, n))),            # T == 0
        (q, q, np.zeros((0, n))),               # T == 0, shared sequence
        (q, q, np.zeros((B, T, n))),            # batch-major u
        (q, q, np.zeros((T, B + 1, n))),
        (q, q, np.zeros((T, B, n + 1))),
        (q, q, np.zeros((T, n + 1))),
        (q, q, np.zeros(n)),
        (q, q, np.zeros((1, T, B, n))),
        (q, np.zeros((B + 1, n)), u),
        (q, np.zeros(n), u),
        (np.zeros((B, n + 1)), np.zeros((B, n + 1)), u),
        (np.zeros((2, B, n)), np.zeros((2, B, n)), u),
        (np.zeros(n), np.zeros(n), np.zeros((T, 1, n))),    # an unbatched state takes u [T, n]
        (np.zeros(n + 1), np.zeros(n + 1), np.zeros((T, n + 1))),
    ]
    for q0, qd0, uu in bad:
        with pytest.raises(ValueError, match="rollout"):
            api.rollout(q0, qd0, uu, 0.01)
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout(q, q, u, 0.01, integrator=integ)


def test_oracle_shapes_and_integrators():
    om = orc.model_from_robot(make_robot("random_prismatic_n6"))
    rng = np.random.default_rng(5)
    B, T, n, dt = 3, 4, 6, 0.01
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
    for integ in INTEGRATORS:
        q, qd = rollout(om, q0, qd0, u, dt, integrator=integ)
        assert q.shape == qd.shape == (T, B, n)
        qf, qdf = rollout(om, q0, qd0, u, dt, integrator=integ, trajectory=False)
        assert np.array_equal(qf, q[-1]) and np.array_equal(qdf, qd[-1])
        q1, qd1, qdd = step(om, q0, qd0, u[0], dt, integrator=integ)
        assert np.array_equal(q1, q[0]) and np.array_equal(qd1, qd[0])
        assert np.array_equal(qdd, orc.aba(om, q0, qd0, u[0]))
        assert np.array_equal(qd1, qd0 + dt * qdd)
        assert np.array_equal(q1, q0 + dt * (qd1 if integ == "semi_implicit" else qd0))
    qs, _ = rollout(om, q0, qd0, u[:, 0], dt)                                  # one sequence for every row
    qe, _ = rollout(om, q0, qd0, np.repeat(u[:, :1], B, 1), dt)
    assert np.array_equal(qs, qe)
    a, b = rollout(om, q0, qd0, u, dt)[0], rollout(om, q0, qd0, u, dt, integrator="euler")[0]
    assert np.abs(a - b).max() > 1e-5                                          # the two integrators are told apart


@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_oracle_stays_at_rest_under_gravity_compensation(name):
    """qd0 = 0 and u_t = rnea(q0, 0, 0)[0]: the oracle's own residual acceleration is at most 1e-12 of the
    uncompensated one, integrated once into qd and twice into q (the GPU bound with 1e-9 replaced by 1e-12)."""
    om = orc.model_from_robot(make_robot(name))
    rng = np.random.default_rng(11)
    B, T, n, dt = 4, 16, om.n, 0.01
    q0 = rng.uniform(-np.pi, np.pi, (B, n))
    z = np.zeros_like(q0)
    u = np.broadcast_to(orc.rnea(om, q0, z, z)[0], (T, B, n))
    for integ in INTEGRATORS:
        q, qd = rollout(om, q0, z, u, dt, integrator=integ)
        bqd, bq = rest_bounds(om, q0, T, dt, 1e-12)
        wqd = np.max(np.abs(qd).max(-1) / bqd)
        wq = np.max(np.abs(q - q0).max(-1) / bq)
        print(name, integ, f"|qd| / bound {wqd:.3f}   |q - q0| / bound {wq:.3f}")
        assert wqd <= 1.0 and wq <= 1.0, (name, integ, wqd, wq)
