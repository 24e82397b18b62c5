"""rollout_grad / rollout_adjoint without a GPU: build wiring, the C-ABI's refusals (every check comes before any launch, so
fake pointers are never dereferenced), the API's refusals, and the numpy restatement of the reverse pass against central
differences of the oracle rollout."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from rollout_grad_oracle import adjoint, linearise, magnitude, rollout_grad
from rollout_oracle import INTEGRATORS, rollout

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
NEW = ["rbd_rollout_adjoint_f32", "rbd_rollout_adjoint_f64", "rbd_rollout_grad_workspace_bytes", "rbd_rollout_grad_f32",
       "rbd_rollout_grad_f64"]


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    for sym in ("rbd_rollout_grad", "rbd_rollout_adjoint", "rbd_rollout_grad_workspace_bytes"):
        assert family_of(sym) == "rollg"
    assert FAMILIES["rollg"] == ["ROLLG", "GRAD", "FD", "RNEA", "MINV"]
    assert "ROLLG" in _ALL_FAMILY_UNITS
    assert "ROLLG_F32" in TRANSLATION_UNITS and "ROLLG_F64" in TRANSLATION_UNITS
    assert "ROLLG_F32" in _TU_COST and "ROLLG_F64" in _TU_COST
    assert family_of("rbd_rollout") == "roll" and FAMILIES["roll"] == ["ROLL"]                # untouched
    assert family_of("rbd_aba") == "fd" and FAMILIES["fd"] == ["FD", "RNEA", "MINV"]
    assert set(NEW) <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for sym in NEW:
        assert re.search(r"\b(int|size_t) " + sym + r"\(", hdr), sym
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert found == set(EXPORTED_SYMBOLS)
    assert "PRISMATIC" in hdr                           # the caveat is stated where the entry points are declared
    fb = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_fb_kernels.hip")).read()
    assert "rbd_rollout_adjoint_##SFX" in fb and "rbd_rollout_grad_##SFX" in fb
    from rbdreference_amd.generic import GENERIC_EXPORTED_SYMBOLS
    assert not any("rollout" in s for s in GENERIC_EXPORTED_SYMBOLS)     # the model-handle library does not serve them
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # additions: the ABI version stays


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_rollg_family_library_refuses_bad_arguments_before_any_launch(sfx, ft):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RBD_ERR_WORKSPACE, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "rollg", sfx)
    assert p == family_lib_path(m, "rollg", sfx) and os.path.exists(p)
    lib = ctypes.CDLL(p)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 6
    assert lib.rbd_abi_version() == 2
    n, esz = 6, ctypes.sizeof(ft)
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first
    odd = ctypes.c_void_p(4096 + 8)

    # ---- the workspace query: grows with Tc, holds at least one step's linearisation and the adjoint
    wsb = lib.rbd_rollout_grad_workspace_bytes
    one, two = wsb(5, 1, esz), wsb(5, 2, esz)
    assert one >= 5 * (n + 2 * n * n + n * n + 2 * n) * esz and two > one and one % 16 == 0 and two - one < one
    assert wsb(0, 1, esz) == 0 and wsb(5, 0, esz) == 0 and wsb(-1, 1, esz) == 0 and wsb(5, 1, 2) == 0

    # ---- rbd_rollout_adjoint
    scan = getattr(lib, f"rbd_rollout_adjoint_{sfx}")

    def call_scan(dc=fake, Mi=fake, gq=fake, gqd=fake, fin=0, dt=0.01, integ=0, B=4, T=3, lam=fake, gu=fake):
        return scan(dc, Mi, gq, gqd, fin, dt, integ, B, T, lam, gu, None)

    # ---- rbd_rollout_grad
    grad = getattr(lib, f"rbd_rollout_grad_{sfx}")

    def call_grad(q0=fake, qd0=fake, u=fake, q=fake, qd=fake, gq=fake, gqd=fake, fin=0, dt=0.01, g=-9.81, integ=0, B=4, T=3,
                  gu=fake, gq0=fake, gqd0=fake, ws=fake, wsb_=1 << 40):
        return grad(q0, qd0, u, q, qd, gq, gqd, fin, dt, g, integ, B, T, gu, gq0, gqd0, ws, wsb_, None)

    def refused(call, msg, code=RBD_ERR_ARG, **kw):
        assert call(**kw) == code, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    for call, who, required, outputs in (
            (call_scan, b"rbd_rollout_adjoint", ("dc", "Mi", "lam", "gu"), ("lam", "gu")),
            (call_grad, b"rbd_rollout_grad", ("q0", "qd0", "u", "q", "qd", "gu", "gq0", "gqd0"), ("gu", "gq0", "gqd0"))):
        for name in required:
            refused(call, b"must be non-null", **{name: None})
        refused(call, who + b": B < 0", B=-1)
        refused(call, who + b": T < 0", T=-1)
        for bad in (float("inf"), float("-inf"), float("nan")):
            refused(call, b"dt must be finite", dt=bad)
        for bad in (-1, 2, 7):
            refused(call, b"unknown integrator", integ=bad)
        refused(call, b"B too large", B=2 ** 62)
        refused(call, b"B * T * n * 2n too large", B=2 ** 30, T=2 ** 40)
        refused(call, b"B * T * n * 2n too large", B=1, T=2 ** 62)
        for name in outputs:
            refused(call, b"16-byte aligned", **{name: odd})
        # nothing to do: success, nothing touched (not even null pointers)
        assert call(B=0) == 0 and call(T=0) == 0
    assert scan(None, None, None, None, 0, 0.01, 0, 0, 5, None, None, None) == 0
    assert grad(None, None, None, None, None, None, None, 0, 0.01, -9.81, 1, 5, 0, None, None, None, None, 0, None) == 0
    # the workspace: missing, short of one step, misaligned
    refused(call_grad, b"workspace missing or smaller", RBD_ERR_WORKSPACE, ws=None)
    refused(call_grad, b"workspace missing or smaller", RBD_ERR_WORKSPACE, wsb_=wsb(4, 1, esz) - 1)
    refused(call_grad, b"workspace missing or smaller", RBD_ERR_WORKSPACE, wsb_=0)
    refused(call_grad, b"workspace must be 16-byte aligned", ws=odd)
    # the other precision is another family library's
    o = "f64" if sfx == "f32" else "f32"
    assert getattr(lib, f"rbd_rollout_adjoint_{o}")(fake, fake, fake, fake, 0, 0.01, 0, 4, 3, fake, fake, None) == -4
    assert b"not part of this family library" in lib.rbd_last_error()
    assert getattr(lib, f"rbd_rollout_grad_{o}")(fake, fake, fake, fake, fake, fake, fake, 0, 0.01, -9.81, 0, 4, 3, fake, fake,
                                                  fake, fake, 1 << 40, None) == -4
    assert getattr(lib, f"rbd_rollout_{sfx}")(fake, fake, fake, 0, 0.01, -9.81, 0, 4, 3, fake, fake, 1, None) == -4


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
    nv = api.nv
    q = np.zeros(nv)
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout_grad(q, q, np.zeros((3, nv)), 0.01, grad_q=np.zeros((3, nv)))
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout_adjoint(np.zeros((3, 2, nv, 2 * nv)), np.zeros((3, 2, nv, nv)), 0.01, grad_q=np.zeros((3, 2, nv)))


def test_api_refuses_bad_shapes_and_integrators_before_any_launch():
    api = _bare_api(make_robot("iiwa_like"))
    n, B, T = 7, 5, 3
    q, u, g = np.zeros((B, n)), np.zeros((T, B, n)), np.zeros((T, B, n))
    bad = [
        dict(q0=q, qd0=q, u=np.zeros((0, B, n)), grad_q=np.zeros((0, B, n))),        # T == 0
        dict(q0=q, qd0=q, u=np.zeros((B, T, n)), grad_q=g),                           # batch-major u
        dict(q0=q, qd0=q, u=np.zeros((T, B, n + 1)), grad_q=g),
        dict(q0=q, qd0=np.zeros((B + 1, n)), u=u, grad_q=g),
        dict(q0=np.zeros(n), qd0=np.zeros(n), u=np.zeros((T, 1, n)), grad_q=np.zeros((T, n))),
        dict(q0=q, qd0=q, u=u),                                                        # no cost gradient at all
        dict(q0=q, qd0=q, u=u, grad_q=np.zeros((T, B + 1, n))),
        dict(q0=q, qd0=q, u=u, grad_q=np.zeros((T + 1, B, n))),
        dict(q0=q, qd0=q, u=u, grad_qd=np.zeros((B, n + 1))),
        dict(q0=q, qd0=q, u=u, grad_q=g, grad_qd=np.zeros((B, n))),                   # one dense, one final
        dict(q0=q, qd0=q, u=u, grad_q=g, q=g),                                         # q without qd
        dict(q0=q, qd0=q, u=u, grad_q=g, q=np.zeros((T - 1, B, n)), qd=np.zeros((T - 1, B, n))),
        dict(q0=q, qd0=q, u=u, grad_q=g, q=g, qd=np.zeros((T, B, n + 1))),
        dict(q0=q, qd0=q, u=u, grad_q=g, workspace_bytes=-1),
    ]
    for kw in bad:
        q0, qd0, uu = kw.pop("q0"), kw.pop("qd0"), kw.pop("u")
        with pytest.raises(ValueError, match="rollout_grad"):
            api.rollout_grad(q0, qd0, uu, 0.01, **kw)
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_grad(q, q, u, 0.01, grad_q=g, integrator=integ)
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_adjoint(np.zeros((T, B, n, 2 * n)), np.zeros((T, B, n, n)), 0.01, grad_q=g, integrator=integ)
    dc, Mi = np.zeros((T, B, n, 2 * n)), np.zeros((T, B, n, n))
    for kw in (dict(dc_du=dc[0], Minv=Mi[0], grad_q=g), dict(dc_du=dc, Minv=np.zeros((T, B, n, n + 1)), grad_q=g),
               dict(dc_du=np.zeros((T, B, n, n)), Minv=Mi, grad_q=g), dict(dc_du=dc, Minv=Mi),
               dict(dc_du=dc, Minv=Mi, grad_q=np.zeros((T, n))), dict(dc_du=dc, Minv=Mi, grad_q=g, lam=np.zeros((B, n))),
               dict(dc_du=dc[:0], Minv=Mi[:0], grad_q=g[:0])):
        with pytest.raises(ValueError, match="rollout_adjoint"):
            api.rollout_adjoint(kw.pop("dc_du"), kw.pop("Minv"), 0.01, **kw)
    import torch
    with pytest.raises(TypeError, match="differentiable=True takes torch tensors"):
        api.rollout(q, q, u, 0.01, differentiable=True)
    with pytest.raises(ValueError, match="unknown integrator"):
        api.rollout(torch.zeros(B, n), torch.zeros(B, n), torch.zeros(T, B, n), 0.01, integrator="rk4", differentiable=True)


def _fd_inputs(name, B, T, seed=1):
    n = orc.model_from_robot(make_robot(name)).n
    rng = np.random.default_rng(1000 * seed + n)
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
    return q0, qd0, u, rng.standard_normal((T, B, n)), rng.standard_normal((T, B, n))


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_oracle_matches_central_differences_of_the_oracle_rollout(name, integ):
    """L = sum(q gq) + sum(qd gqd) over the trajectory; every component of dL/du, dL/dq0, dL/dqd0 by central differences
    of the fp64 oracle rollout (h = 1e-6) against the adjoint recursion.  Bound 1e-6 max|fd| per output: the truncation
    and rounding of the differences is ~1e-8 of it (worst seen 9.2e-9); a swapped integrator moves the result by more than
    1e-5 of it (asserted below), and the prismatic discrepancy of dc_dq is 4.5e-2 on random_prismatic_n6 with these inputs."""
    om = orc.model_from_robot(make_robot(name))
    B, T, dt, h = 2, 5, 0.01, 1e-6
    q0, qd0, u, gq, gqd = _fd_inputs(name, B, T)
    n = om.n
    got = rollout_grad(om, q0, qd0, u, dt, gq, gqd, integrator=integ)[:3]

    def cost_rows(q0_, qd0_, u_):
        q, qd = rollout(om, q0_, qd0_, u_, dt, integrator=integ)
        return (q * gq).sum((0, 2)) + (qd * gqd).sum((0, 2))                  # [B]: rows do not interact

    def fd(which, idx):
        args = [q0.copy(), qd0.copy(), u.copy()]
        args[which][idx] += h
        up = cost_rows(*args)
        args[which][idx] -= 2 * h
        return (up - cost_rows(*args)) / (2 * h)

    fd_u = np.stack([np.stack([fd(2, (t, slice(None), j)) for j in range(n)], -1) for t in range(T)])
    fd_q0 = np.stack([fd(0, (slice(None), j)) for j in range(n)], -1)
    fd_qd0 = np.stack([fd(1, (slice(None), j)) for j in range(n)], -1)
    for tag, a, f in (("grad_u", got[0], fd_u), ("grad_q0", got[1], fd_q0), ("grad_qd0", got[2], fd_qd0)):
        rel = float(np.abs(a - f).max() / np.abs(f).max())
        print(f"{name} {integ} {tag}: max|adj - fd| / max|fd| = {rel:.2e}")
        assert rel <= 1e-6, (name, integ, tag, rel)
    # the other integrator's recursion on the same trajectory is told apart by far more than the bound
    other = rollout_grad(om, q0, qd0, u, dt, gq, gqd, integrator=[i for i in INTEGRATORS if i != integ][0],
                         q_traj=rollout(om, q0, qd0, u, dt, integrator=integ)[0], qd_traj=rollout(om, q0, qd0, u, dt, integrator=integ)[1])
    assert np.abs(other[0] - got[0]).max() > 1e-5 * np.abs(got[0]).max()


def test_oracle_forms_agree_and_the_magnitude_bounds_the_result():
    om = orc.model_from_robot(make_robot("random_prismatic_n6"))
    B, T, dt = 3, 4, 0.01
    q0, qd0, u, gq, gqd = _fd_inputs("random_prismatic_n6", B, T, seed=2)
    q, qd = rollout(om, q0, qd0, u, dt)
    dc, Mi = linearise(om, q0, qd0, u, q, qd)
    assert dc.shape == (T, B, 6, 12) and Mi.shape == (T, B, 6, 6)
    assert np.array_equal(dc[0], orc.rnea_grad(om, q0, qd0, orc.aba(om, q0, qd0, u[0])))
    assert np.array_equal(dc[2], orc.rnea_grad(om, q[1], qd[1], orc.aba(om, q[1], qd[1], u[2])))
    gu, gq0, gqd0, S = rollout_grad(om, q0, qd0, u, dt, gq, gqd)
    gu2, lam, S2 = adjoint(dc, Mi, dt, gq, gqd)
    assert np.array_equal(gu, gu2) and np.array_equal(lam, np.concatenate([gq0, gqd0], 1)) and np.array_equal(S, S2)
    Sbar = magnitude(dc, Mi, dt, gq, gqd)
    assert (Sbar >= S).all() and (S >= np.abs(lam).max(1)).all() and (S >= np.abs(gu).max((0, 2))).all()
    # a split scan carries lam: steps [k, T) first, then [0, k)
    for k in range(1, T):
        gu_hi, lam_hi, _ = adjoint(dc[k:], Mi[k:], dt, gq[k:], gqd[k:])
        gu_lo, lam_lo, _ = adjoint(dc[:k], Mi[:k], dt, gq[:k], gqd[:k], lam=lam_hi)
        assert np.array_equal(np.concatenate([gu_lo, gu_hi]), gu) and np.array_equal(lam_lo, lam)
    # a final-state gradient is the dense one with zeros before the last slice
    z = np.zeros_like(gq)
    z[-1] = gq[-1]
    assert np.array_equal(adjoint(dc, Mi, dt, gq[-1], None)[0], adjoint(dc, Mi, dt, z, None)[0])
