"""rollout_lqr / rollout_riccati without a GPU: the numpy restatement of the Riccati recursion against a linear-quadratic
problem it must solve exactly, its reduction to the adjoint recursion, the fp32 yardstick of the GPU tests, build wiring,
the API's refusals and the C-ABI's refusals (every check comes before any launch, so fake pointers are never
dereferenced)."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from rbdreference_amd.packer import pack_robot
from rollout_grad_oracle import adjoint
from rollout_lqr_oracle import closed_loop_cost, riccati
from rollout_oracle import INTEGRATORS

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
NEW = ["rbd_rollout_riccati_f32", "rbd_rollout_riccati_f64", "rbd_rollout_lqr_workspace_bytes", "rbd_rollout_lqr_f32",
       "rbd_rollout_lqr_f64"]


def scan_inputs(n, B, T, seed=0):
    """The distributions of the GPU scan tests: dc_du, Minv uniform(-1, 1) / n with Minv symmetrised, g and grad_u standard
    normal, hess_q, hess_qd uniform(5, 15), hess_u uniform(1, 2)."""
    rng = np.random.default_rng(7000 + 100 * seed + n)
    dc = rng.uniform(-1, 1, (T, B, n, 2 * n)) / n
    Mi = rng.uniform(-1, 1, (T, B, n, n)) / n
    Mi = 0.5 * (Mi + Mi.transpose(0, 1, 3, 2))
    d = dict(gq=rng.standard_normal((T, B, n)), gqd=rng.standard_normal((T, B, n)), hq=rng.uniform(5, 15, (T, B, n)),
             hqd=rng.uniform(5, 15, (T, B, n)), gu=rng.standard_normal((T, B, n)), hu=rng.uniform(1, 2, (T, B, n)))
    return dc, Mi, d


def row_err(a, r):
    """Per row, max norm relative to the reference's max norm over the row -> the worst row."""
    B = r.shape[0]
    a, r = np.asarray(a, np.float64).reshape(B, -1), np.asarray(r, np.float64).reshape(B, -1)
    return float((np.abs(a - r).max(1) / np.abs(r).max(1)).max())


def by_row(x):
    """[T, B, ...] -> [B, T, ...] so that ``row_err`` sees one row's whole output."""
    return np.moveaxis(x, 0, 1)


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    for sym in ("rbd_rollout_lqr", "rbd_rollout_riccati", "rbd_rollout_lqr_workspace_bytes"):
        assert family_of(sym) == "lqr"
    assert FAMILIES["lqr"] == ["LQR", "GRAD", "FD", "RNEA", "MINV"]
    assert "LQR" in _ALL_FAMILY_UNITS
    assert "LQR_F32" in TRANSLATION_UNITS and "LQR_F64" in TRANSLATION_UNITS
    assert "LQR_F32" in _TU_COST and "LQR_F64" in _TU_COST
    assert family_of("rbd_rollout_grad") == "rollg" and FAMILIES["rollg"] == ["ROLLG", "GRAD", "FD", "RNEA", "MINV"]   # untouched
    assert family_of("rbd_rollout") == "roll" and FAMILIES["roll"] == ["ROLL"]
    assert set(NEW) <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for sym in NEW:
        assert re.search(r"\b(int|size_t) " + sym + r"\(", hdr), sym
    assert set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr)) == set(EXPORTED_SYMBOLS)
    assert hdr.count("PRISMATIC") >= 2                  # the caveat is repeated where the new entry points are declared
    fb = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_fb_kernels.hip")).read()
    assert "rbd_rollout_riccati_##SFX" in fb and "rbd_rollout_lqr_##SFX" in fb
    from rbdreference_amd.generic import GENERIC_EXPORTED_SYMBOLS
    assert not any("rollout" in s for s in GENERIC_EXPORTED_SYMBOLS)     # the model-handle library does not serve them
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # additions: the ABI version stays


@pytest.mark.parametrize("reg", [0.0, 0.5])
@pytest.mark.parametrize("integ", INTEGRATORS)
def test_oracle_solves_a_linear_quadratic_problem(integ, reg):
    """A problem whose dynamics are the linearisation itself (n = 4, T = 6, a full terminal Hessian through P).  The
    closed-loop pass with the returned k, K changes the cost by exactly dV.sum() (for any reg: the full-form update tracks
    the policy's own value); with reg = 0 it is stationary in u, and lam and P are the first and second derivatives of the
    optimal cost in x0.  Everything at 1e-6 of the quantity's max norm; a quadratic makes central differences exact, so
    what is seen is rounding (worst seen: dV 5e-16, stationarity 9e-12, lam 8e-14, P 3e-13)."""
    n, B, T, dt = 4, 3, 6, 0.1
    dc, Mi, c = scan_inputs(n, B, T, seed=1)
    rng = np.random.default_rng(5)
    J = rng.standard_normal((B, 3, 2 * n))
    Pf = np.einsum("bkr,bkc->brc", J, J)                 # Gauss-Newton J^T J of a 3-dimensional target
    k, K, lam, P, dV, status = riccati(dc, Mi, dt, reg=reg, integrator=integ, P=Pf, **c)
    assert (status == 0).all()
    x0 = np.zeros((B, 2 * n))
    cost = lambda x, du=None: closed_loop_cost(dc, Mi, dt, k, K, x, integ, Pf=Pf, du=du, **c)
    J1, us = cost(x0)
    J0 = closed_loop_cost(dc, Mi, dt, 0 * k, 0 * K, x0, integ, Pf=Pf, **c)[0]
    e_dv = float(np.abs((J1 - J0) - dV.sum(1)).max() / np.abs(dV.sum(1)).max())
    print(f"{integ} reg={reg}: cost change {J1 - J0} vs dV.sum {dV.sum(1)}: rel {e_dv:.2e}")
    assert e_dv <= 1e-6
    assert (dV[:, 0] < 0).all() and (dV[:, 1] > 0).all()
    if reg != 0.0:
        return
    h = 1e-4
    # stationary: central-difference gradient of the cost in every u[t, :, j] (rows do not interact)
    grad = np.zeros((T, B, n))
    for t in range(T):
        for j in range(n):
            du = np.zeros((T, B, n))
            du[t, :, j] = h
            grad[t, :, j] = (cost(x0, du)[0] - cost(x0, -du)[0]) / (2 * h)
    e_st = float(np.abs(grad).max() / max(np.abs(c["gu"]).max(), 1.0))
    # lam, P: derivatives of the optimal cost in x0 (the policy is optimal from every x0: the problem is LQ)
    h = 1e-2
    E = np.eye(2 * n)
    d1 = np.stack([(cost(x0 + h * E[i])[0] - cost(x0 - h * E[i])[0]) / (2 * h) for i in range(2 * n)], 1)
    d2 = np.zeros((B, 2 * n, 2 * n))
    for i in range(2 * n):
        for j in range(2 * n):
            d2[:, i, j] = (cost(x0 + h * (E[i] + E[j]))[0] - cost(x0 + h * (E[i] - E[j]))[0] - cost(x0 - h * (E[i] - E[j]))[0]
                           + cost(x0 - h * (E[i] + E[j]))[0]) / (4 * h * h)
    e_lam, e_P = row_err(d1, lam), row_err(d2, P)
    print(f"{integ}: stationarity {e_st:.2e}, lam vs dJ*/dx0 {e_lam:.2e}, P vs d2J*/dx0^2 {e_P:.2e}")
    assert e_st <= 1e-6 and e_lam <= 1e-6 and e_P <= 1e-6
    assert np.array_equal(P, P.transpose(0, 2, 1))


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_oracle_reduces_to_the_adjoint_with_zero_gains(integ):
    n, B, T, dt = 5, 3, 4, 0.05
    dc, Mi, c = scan_inputs(n, B, T, seed=2)
    k, K, lam, P, dV, status = riccati(dc, Mi, dt, integrator=integ, zero_gains=True, **c)
    _, lam_adj, _ = adjoint(dc, Mi, dt, c["gq"], c["gqd"], integrator=integ)
    assert not k.any() and not K.any() and not dV.any() and not status.any()
    assert row_err(lam, lam_adj) <= 1e-13


def test_oracle_split_failure_and_final_only_forms():
    n, B, T, dt = 3, 4, 5, 0.1
    dc, Mi, c = scan_inputs(n, B, T, seed=3)
    full = riccati(dc, Mi, dt, **c)
    for s in range(1, T):
        hi = riccati(dc[s:], Mi[s:], dt, **{a: v[s:] for a, v in c.items()})
        lo = riccati(dc[:s], Mi[:s], dt, lam=hi[2], P=hi[3], dV=hi[4], status=hi[5], **{a: v[:s] for a, v in c.items()})
        assert np.array_equal(np.concatenate([lo[0], hi[0]]), full[0]) and np.array_equal(np.concatenate([lo[1], hi[1]]), full[1])
        assert all(np.array_equal(a, b) for a, b in zip(lo[2:], full[2:]))
    # final-only state costs are the dense ones with zeros before the last slice
    z = {a: np.zeros_like(c[a]) for a in ("gq", "gqd", "hq", "hqd")}
    for a in z:
        z[a][-1] = c[a][-1]
    fin = riccati(dc, Mi, dt, gu=c["gu"], hu=c["hu"], **{a: c[a][-1] for a in z})
    den = riccati(dc, Mi, dt, gu=c["gu"], hu=c["hu"], **z)
    assert all(np.array_equal(a, b) for a, b in zip(fin, den))
    # Quu = 0 in one row: no gains, status counts the steps, everything finite, the other rows untouched
    hu = c["hu"].copy()
    hu[:, 1] = 0
    bad = riccati(dc, Mi, dt, gu=c["gu"], hu=hu, gq=c["gq"])
    assert bad[5].tolist() == [0, T, 0, 0] and not bad[0][:, 1].any() and not bad[1][:, 1].any()
    assert all(np.isfinite(x).all() for x in bad[:5]) and not bad[4][1].any()
    ok = riccati(dc, Mi, dt, gu=c["gu"], hu=c["hu"], gq=c["gq"])
    keep = [0, 2, 3]
    for i, (x, y) in enumerate(zip(bad, ok)):          # k and K are time-major
        assert np.array_equal(x[:, keep], y[:, keep]) if i < 2 else np.array_equal(x[keep], y[keep])
    assert (riccati(dc, Mi, dt, gu=c["gu"], hu=hu, gq=c["gq"], reg=1.0)[5] == 0).all()


def test_float32_oracle_is_the_yardstick():
    """The fp32 bound of the GPU tests is max(8 e32, T 2n 2^-24) with e32 the error of the oracle run in float32.
    e32 < 1e-5 for the worst case there (n = 30, T = 5; seen: at most 9.6e-7, on P), so the bound cannot widen silently;
    and the bound tells the integrators apart (K moves by 7.7e-2 of its max norm, asserted at 1e-2)."""
    n, B, T, dt = 30, 41, 5, 0.1
    dc, Mi, c = scan_inputs(n, B, T)
    f32 = lambda x: np.asarray(x, np.float32)
    c32 = {a: f32(v) for a, v in c.items()}
    c64 = {a: v.astype(np.float64) for a, v in c32.items()}
    for integ in INTEGRATORS:
        ref = riccati(f32(dc), f32(Mi), dt, integrator=integ, **c64)
        low = riccati(f32(dc), f32(Mi), dt, integrator=integ, dtype=np.float32, **c32)
        assert all(x.dtype == np.float32 for x in low[:5])
        e32 = {name: row_err(by_row(a) if name in "kK" else a, by_row(r) if name in "kK" else r)
               for name, a, r in zip(("k", "K", "lam", "P", "dV"), low, ref)}
        print(integ, {a: f"{e:.2e}" for a, e in e32.items()})
        assert max(e32.values()) < 1e-5
    Ka, Kb = (riccati(f32(dc), f32(Mi), dt, integrator=i, **c64)[1] for i in ("semi_implicit", "euler"))
    sep = float((np.abs(Ka - Kb).max((0, 2, 3)) / np.abs(Ka).max((0, 2, 3))).min())
    print(f"integrators apart on K by {sep:.2e}")
    assert sep >= 1e-2


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
        api.rollout_lqr(q, q, np.zeros((3, nv)), 0.01, hess_u=np.ones(nv))
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout_riccati(np.zeros((3, 2, nv, 2 * nv)), np.zeros((3, 2, nv, nv)), 0.01, hess_u=np.ones(nv))


def test_api_refuses_bad_shapes_and_values_before_any_launch():
    api = _bare_api(make_robot("iiwa_like"))
    n, B, T = 7, 5, 3
    q, u, g, hu = np.zeros((B, n)), np.zeros((T, B, n)), np.zeros((T, B, n)), np.ones(n)
    bad = [
        dict(q0=q, qd0=q, u=np.zeros((0, B, n)), hess_u=hu),                           # T == 0
        dict(q0=q, qd0=q, u=np.zeros((B, T, n)), hess_u=hu),                           # batch-major u
        dict(q0=q, qd0=np.zeros((B + 1, n)), u=u, hess_u=hu),
        dict(q0=np.zeros(n), qd0=np.zeros(n), u=np.zeros((T, 1, n)), hess_u=hu),
        dict(q0=q, qd0=q, u=u),                                                        # hess_u is required
        dict(q0=q, qd0=q, u=u, hess_u=np.ones(n + 1)),
        dict(q0=q, qd0=q, u=u, hess_u=np.ones((B, n))),
        dict(q0=q, qd0=q, u=u, hess_u=hu, grad_u=np.zeros((B, n))),
        dict(q0=q, qd0=q, u=u, hess_u=hu, grad_q=np.zeros((T, B + 1, n))),
        dict(q0=q, qd0=q, u=u, hess_u=hu, grad_q=g, hess_q=np.zeros((B, n))),        # one dense, one final
        dict(q0=q, qd0=q, u=u, hess_u=hu, hess_qd=np.zeros((B, n + 1))),
        dict(q0=q, qd0=q, u=u, hess_u=hu, reg=-1.0),
        dict(q0=q, qd0=q, u=u, hess_u=hu, reg=float("nan")),
        dict(q0=q, qd0=q, u=u, hess_u=hu, q=g),                                        # q without qd
        dict(q0=q, qd0=q, u=u, hess_u=hu, q=np.zeros((T - 1, B, n)), qd=np.zeros((T - 1, B, n))),
        dict(q0=q, qd0=q, u=u, hess_u=hu, workspace_bytes=-1),
    ]
    for kw in bad:
        q0, qd0, uu = kw.pop("q0"), kw.pop("qd0"), kw.pop("u")
        with pytest.raises(ValueError, match="rollout_lqr"):
            api.rollout_lqr(q0, qd0, uu, 0.01, **kw)
    dc, Mi = np.zeros((T, B, n, 2 * n)), np.zeros((T, B, n, n))
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_lqr(q, q, u, 0.01, hess_u=hu, integrator=integ)
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_riccati(dc, Mi, 0.01, hess_u=hu, integrator=integ)
    for kw in (dict(dc_du=dc[0], Minv=Mi[0], hess_u=hu), dict(dc_du=dc, Minv=np.zeros((T, B, n, n + 1)), hess_u=hu),
               dict(dc_du=np.zeros((T, B, n, n)), Minv=Mi, hess_u=hu), dict(dc_du=dc, Minv=Mi),
               dict(dc_du=dc, Minv=Mi, hess_u=hu, grad_q=np.zeros((T, n))), dict(dc_du=dc, Minv=Mi, hess_u=hu, lam=np.zeros((B, n))),
               dict(dc_du=dc, Minv=Mi, hess_u=hu, P=np.zeros((B, 2 * n, n))), dict(dc_du=dc, Minv=Mi, hess_u=hu, dV=np.zeros((B, 3))),
               dict(dc_du=dc, Minv=Mi, hess_u=hu, status=np.zeros((B, 1), np.int32)), dict(dc_du=dc, Minv=Mi, hess_u=hu, reg=-0.5),
               dict(dc_du=dc[:0], Minv=Mi[:0], hess_u=hu)):
        with pytest.raises(ValueError, match="rollout_riccati"):
            api.rollout_riccati(kw.pop("dc_du"), kw.pop("Minv"), 0.01, **kw)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_lqr_family_library_refuses_bad_arguments_before_any_launch(sfx, ft):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RBD_ERR_WORKSPACE, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "lqr", sfx)
    assert p == family_lib_path(m, "lqr", sfx) and os.path.exists(p)
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

    wsb = lib.rbd_rollout_lqr_workspace_bytes
    one, two = wsb(5, 1, esz), wsb(5, 2, esz)
    assert one >= 5 * (n + 2 * n * n + n * n) * esz and two > one and one % 16 == 0 and two - one <= one
    assert wsb(0, 1, esz) == 0 and wsb(5, 0, esz) == 0 and wsb(-1, 1, esz) == 0 and wsb(5, 1, 2) == 0

    scan = getattr(lib, f"rbd_rollout_riccati_{sfx}")

    def call_scan(dc=fake, Mi=fake, gq=fake, gqd=fake, hq=fake, hqd=fake, fin=0, gu=fake, hu=fake, shared=0, reg=0.0, dt=0.01,
                  integ=0, B=4, T=3, lam=fake, P=fake, dV=fake, status=fake, k=fake, K=fake):
        return scan(dc, Mi, gq, gqd, hq, hqd, fin, gu, hu, shared, reg, dt, integ, B, T, lam, P, dV, status, k, K, None)

    lqr = getattr(lib, f"rbd_rollout_lqr_{sfx}")

    def call_lqr(q0=fake, qd0=fake, u=fake, q=fake, qd=fake, gq=fake, gqd=fake, hq=fake, hqd=fake, fin=0, gu=fake, hu=fake,
                 shared=0, reg=0.0, dt=0.01, g=-9.81, integ=0, B=4, T=3, k=fake, K=fake, lam=fake, P=fake, dV=fake, status=fake,
                 ws=fake, wsb_=1 << 40):
        return lqr(q0, qd0, u, q, qd, gq, gqd, hq, hqd, fin, gu, hu, shared, reg, dt, g, integ, B, T, k, K, lam, P, dV, status,
                   ws, wsb_, None)

    def refused(call, msg, code=RBD_ERR_ARG, **kw):
        assert call(**kw) == code, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    outs = ("lam", "P", "dV", "status", "k", "K")
    for call, who, required in ((call_scan, b"rbd_rollout_riccati", ("dc", "Mi", "hu") + outs),
                                (call_lqr, b"rbd_rollout_lqr", ("q0", "qd0", "u", "q", "qd", "hu") + outs)):
        for name in required:
            refused(call, b"must be non-null", **{name: None})
        refused(call, who + b": B < 0", B=-1)
        refused(call, who + b": T < 0", T=-1)
        for bad in (float("inf"), float("-inf"), float("nan")):
            refused(call, b"dt must be finite", dt=bad)
        for bad in (float("inf"), float("nan"), -1e-3, float("-inf")):
            refused(call, b"reg must be finite and >= 0", reg=bad)
        for bad in (-1, 2, 7):
            refused(call, b"unknown integrator", integ=bad)
        refused(call, b"B too large", B=2 ** 62)
        refused(call, b"B * T * n * 2n too large", B=2 ** 30, T=2 ** 40)
        refused(call, b"B * T * n * 2n too large", B=1, T=2 ** 62)
        for name in outs:
            refused(call, b"16-byte aligned", **{name: odd})
        # optional costs may be null (checked up to the point of launching: the workspace / nothing else is wrong here)
        assert call(B=0) == 0 and call(T=0) == 0
    assert scan(*([None] * 6), 0, None, None, 0, 0.0, 0.01, 0, 0, 5, *([None] * 6), None) == 0
    assert lqr(*([None] * 9), 0, None, None, 0, 0.0, 0.01, -9.81, 1, 5, 0, *([None] * 7), 0, None) == 0
    refused(call_lqr, b"workspace missing or smaller", RBD_ERR_WORKSPACE, ws=None)
    refused(call_lqr, b"workspace missing or smaller", RBD_ERR_WORKSPACE, wsb_=wsb(4, 1, esz) - 1)
    refused(call_lqr, b"workspace missing or smaller", RBD_ERR_WORKSPACE, wsb_=0)
    refused(call_lqr, b"workspace must be 16-byte aligned", ws=odd)
    # the other precision is another family library's, and so is rbd_rollout_grad
    o = "f64" if sfx == "f32" else "f32"
    assert getattr(lib, f"rbd_rollout_riccati_{o}")(*([fake] * 6), 0, fake, fake, 0, 0.0, 0.01, 0, 4, 3, *([fake] * 6), None) == -4
    assert b"not part of this family library" in lib.rbd_last_error()
    assert getattr(lib, f"rbd_rollout_adjoint_{sfx}")(fake, fake, fake, fake, 0, 0.01, 0, 4, 3, fake, fake, None) == -4
