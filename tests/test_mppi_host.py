"""mppi_update and mppi without a GPU: build wiring, the C-ABI's refusals (every check comes before the first launch, so
fake pointers are never dereferenced), the API's refusals, and the numpy restatement checked against its closed forms."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from mppi_oracle import mppi, mppi_update
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from rollout_closed_loop_oracle import ilqr_problem
from rollout_cost_oracle import cost_arrays, rollout_cost
from rollout_oracle import INTEGRATORS

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_mppi_update") == "mppi" and family_of("rbd_mppi_update_workspace_bytes") == "mppi"
    assert FAMILIES["mppi"] == ["MPPI"]
    assert "MPPI" in _ALL_FAMILY_UNITS
    assert "MPPI_F32" in TRANSLATION_UNITS and "MPPI_F64" in TRANSLATION_UNITS
    assert "MPPI_F32" in _TU_COST and "MPPI_F64" in _TU_COST
    assert family_of("rbd_rollout_cost") == "rollcost" and FAMILIES["rollcost"] == ["ROLLCOST"]      # untouched
    names = {"rbd_mppi_update_workspace_bytes", "rbd_mppi_update_f32", "rbd_mppi_update_f64"}
    assert names <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert "int rbd_mppi_update_f32(" in hdr and "int rbd_mppi_update_f64(" in hdr and "size_t rbd_mppi_update_workspace_bytes(" in hdr
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert names <= found and found == set(EXPORTED_SYMBOLS)
    src = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_kernels.hip")).read()
    assert '#include "rbd_mppi.h"' in src and "RBD_TU_MPPI_F32" in src and "RBD_TU_MPPI_F64" in src
    capi = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_capi.h")).read()
    assert "RBD_DEFS_MPPI" in capi and "RBD_STUBS_MPPI" in capi
    fb = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_fb_kernels.hip")).read()
    assert "rbd_mppi_update_##SFX" in fb
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # an addition: the ABI version stays


def test_chunk_constant_of_the_header_is_the_one_of_the_binding():
    from rbdreference_amd._lib import RBD_MPPI_CHUNK
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    m = re.findall(r"^#define\s+RBD_MPPI_CHUNK\s+(\d+)\s*$", hdr, flags=re.M)
    assert len(m) == 1 and int(m[0]) == RBD_MPPI_CHUNK and RBD_MPPI_CHUNK >= 2
    kh = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_mppi.h")).read()
    assert "MPPI_CHUNK = RBD_MPPI_CHUNK" in kh and "SUMMATION ORDER" in kh


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_mppi_family_library_refuses_bad_arguments_before_any_launch(sfx):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RBD_ERR_WORKSPACE, RBD_MPPI_CHUNK, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "mppi", sfx)
    assert p == family_lib_path(m, "mppi", sfx) and os.path.exists(p)
    lib = ctypes.CDLL(p)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 6
    assert lib.rbd_abi_version() == 2
    esz = 4 if sfx == "f32" else 8
    fn = getattr(lib, f"rbd_mppi_update_{sfx}")
    other = getattr(lib, f"rbd_mppi_update_{'f64' if sfx == 'f32' else 'f32'}")
    query = lib.rbd_mppi_update_workspace_bytes
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first
    S, P, T, n = 3 * RBD_MPPI_CHUNK + 1, 5, 4, 6
    need = query(S, P, T, esz)
    a16 = lambda x: (x + 15) & ~15      # noqa: E731
    assert need == a16(S * P * esz) + a16(P * esz) + a16(4 * T * P * n * esz)          # e | eta | the partials of 4 chunks
    assert query(RBD_MPPI_CHUNK, P, T, esz) == a16(RBD_MPPI_CHUNK * P * esz) + a16(P * esz)      # one chunk: no partials
    for bad in ((0, P, T, esz), (S, 0, T, esz), (S, P, 0, esz), (-1, P, T, esz), (S, P, T, 2), (2 ** 40, 2 ** 40, 1, esz), (2 ** 30, 2 ** 20, 2 ** 20, esz)):
        assert query(*bad) == 0, bad

    def call(J=fake, du=fake, u=fake, lam=fake, lo=None, hi=None, S=S, P=P, T=T, u_out=fake, w=fake, ess=fake, status=fake, ws=fake,
             wsb=need):
        return fn(J, du, u, lam, lo, hi, S, P, T, u_out, w, ess, status, ws, wsb, None)

    def refused(msg, code=RBD_ERR_ARG, **kw):
        assert call(**kw) == code, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    for name in ("J", "du", "u", "lam", "u_out", "status"):
        refused(b"must be non-null", **{name: None})
    refused(b"u_lo and u_hi", lo=fake)
    refused(b"u_lo and u_hi", hi=fake)
    refused(b"S < 0", S=-1)
    refused(b"P < 0", P=-1)
    refused(b"T < 0", T=-1)
    refused(b"too large", S=2 ** 40, P=2 ** 40)
    refused(b"too large", S=2 ** 30, P=2 ** 20, T=2 ** 20)
    refused(b"too large", S=1, P=1, T=2 ** 62)
    for name in ("u_out", "w", "ess", "status"):
        refused(b"16-byte aligned", **{name: ctypes.c_void_p(4096 + 8)})
    refused(b"workspace must be 16-byte aligned", ws=ctypes.c_void_p(4096 + 8))
    refused(b"workspace missing or smaller", code=RBD_ERR_WORKSPACE, ws=None)
    refused(b"workspace missing or smaller", code=RBD_ERR_WORKSPACE, wsb=need - 1)
    refused(b"workspace missing or smaller", code=RBD_ERR_WORKSPACE, wsb=0)
    # nothing to do: success, nothing touched (not even the null pointers or the missing workspace)
    assert call(S=0) == 0 and call(P=0) == 0 and call(T=0) == 0
    assert fn(None, None, None, None, None, None, 0, 5, 5, None, None, None, None, None, 0, None) == 0
    assert fn(None, None, None, None, fake, None, 5, 0, 5, None, None, None, None, None, 0, None) == 0
    # the other precision is another family library's
    assert other(fake, fake, fake, fake, None, None, S, P, T, fake, fake, fake, fake, fake, need, None) == -4
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
    from rbdreference_amd import QuadraticCost
    from rbdreference_amd.robot import floating_quadruped_like
    api = _bare_api(floating_quadruped_like())
    nv = api.nv
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.mppi_update(np.zeros((4, 2)), np.zeros((3, 4, 2, nv)), np.zeros((3, 2, nv)), 1.0)
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.mppi(np.zeros((2, nv)), np.zeros((2, nv)), np.zeros((3, 2, nv)), 0.01, QuadraticCost())


def test_api_refuses_bad_shapes_and_types_before_any_launch():
    import torch
    from rbdreference_amd import MppiResult, MppiUpdate, QuadraticCost
    assert MppiUpdate._fields == ("u", "w", "ess", "status") and MppiResult._fields == ("u", "q", "qd", "cost", "ess", "status")
    api = _bare_api(make_robot("iiwa_like"))
    n, S, P, T = 7, 5, 3, 4
    z = np.zeros
    good = dict(J=z((S, P)), du=z((T, S, P, n)), u=z((T, P, n)), lam=1.0)
    bad = [
        dict(J=z(S)), dict(J=z((S, P, 1))), dict(J=z((0, P))), dict(J=z((S, 0)), du=z((T, S, 0, n)), u=z((T, 0, n))),
        dict(u=z((T, P + 1, n))), dict(u=z((P, n))), dict(u=z((T, P, n + 1))), dict(u=z((0, P, n)), du=z((0, S, P, n))),
        dict(du=z((T, P, S, n))), dict(du=z((T, S * P, n))), dict(du=z((T, S + 1, P, n))),
        dict(lam=z(P + 1)), dict(lam=z((P, 1))), dict(lam=z((1,))),
        dict(u_min=-1.0), dict(u_max=1.0), dict(u_min=-np.ones(n + 1), u_max=np.ones(n + 1)), dict(u_min=-np.ones((1, n)), u_max=1.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="mppi_update"):
            api.mppi_update(**{**good, **kw})
    with pytest.raises(TypeError, match="mixing numpy and torch"):
        api.mppi_update(**{**good, "du": torch.zeros((T, S, P, n))})
    with pytest.raises(TypeError, match="mixing numpy and torch"):
        api.mppi_update(**{**good, "J": torch.zeros((S, P))})
    # the driver
    cm = QuadraticCost(w_q=np.ones((T, P, n)), w_u=np.ones(n))
    dgood = dict(q0=z((P, n)), qd0=z((P, n)), u=z((T, P, n)), dt=0.01, cost=cm, iters=2)
    dbad = [
        dict(q0=z(n), qd0=z(n)), dict(qd0=z((P + 1, n))), dict(q0=z((0, n)), qd0=z((0, n)), u=z((T, 0, n))),
        dict(u=z((T, P + 1, n))), dict(u=z((0, P, n))), dict(u=z((P, T, n))),
        dict(iters=-1), dict(samples=0),
        dict(noise=z((2, T, S, P, n)), generator=torch.Generator()),
        dict(noise=z((1, T, S, P, n))), dict(noise=z((2, T, S * P, n))), dict(noise=z((2, T, 0, P, n))), dict(noise=z((2, T, S, P, n + 1))),
        dict(sigma=z(n + 1)), dict(sigma=z((T, 1))), dict(sigma=z((T, P, n))),
        dict(lam=z(P + 1)), dict(u_min=-1.0), dict(u_min=-np.ones(n - 1), u_max=np.ones(n - 1)),
    ]
    for kw in dbad:
        with pytest.raises(ValueError, match="mppi"):
            api.mppi(**{**dgood, **kw})
    with pytest.raises(TypeError, match="QuadraticCost"):
        api.mppi(**{**dgood, "cost": dict(w_q=1.0)})
    with pytest.raises(TypeError, match="mixing numpy and torch"):
        api.mppi(**{**dgood, "noise": torch.zeros((2, T, S, P, n))})
    with pytest.raises(TypeError, match="mixing numpy and torch"):
        api.mppi(**{**dgood, "cost": QuadraticCost(w_u=torch.ones(n))})
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.mppi(**dgood, integrator=integ)


# ---- the oracle against its closed forms ---------------------------------------------------------------------------------
def _draw(seed, S, P, T=3, n=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(5, 25, (S, P)), rng.normal(0, 0.3, (T, S, P, n)), rng.normal(0, 0.5, (T, P, n))


@pytest.mark.parametrize("limits", [None, (-0.6, 0.6)])
def test_oracle_limits_of_the_softmin(limits):
    lo, hi = limits if limits else (None, None)
    J, du, u = _draw(1, 9, 4)
    # S = 1: the one sample
    u1, w1, x1, d1, D1, ess1, st1 = mppi_update(J[:1], du[:, :1], u, 1.0, lo, hi)
    ref = u + d1[:, 0]
    assert np.array_equal(u1, ref if lo is None else np.clip(ref, lo, hi)) and np.array_equal(w1, np.ones((1, 4))) and np.array_equal(ess1, np.ones(4))
    assert not st1.any() and not x1.any()
    # lam -> 0 with a unique minimum: that sample; lam -> inf: the mean
    uo, w, x, d, D, ess, st = mppi_update(J, du, u, 1e-30, lo, hi)
    am = J.argmin(axis=0)
    pick = np.stack([d[:, am[p], p] for p in range(4)], axis=1)
    assert np.array_equal(uo, u + pick if lo is None else np.clip(u + pick, lo, hi)) and np.array_equal(ess, np.ones(4))
    assert np.array_equal(w, (np.arange(9)[:, None] == am[None]).astype(float)) and not st.any()
    uo, w, x, d, D, ess, st = mppi_update(J, du, u, 1e30, lo, hi)
    assert np.allclose(w, 1 / 9, rtol=1e-12) and np.allclose(D, d.mean(axis=1), rtol=1e-12, atol=1e-15) and np.allclose(ess, 9, rtol=1e-12)
    # in between: the weights sum to one, x >= 0 with a zero at the minimum, ess in [1, S], limits respected
    for lam in (0.05, 1.0, 30.0, np.array([0.05, 1.0, 30.0, 2.0])):
        uo, w, x, d, D, ess, st = mppi_update(J, du, u, lam, lo, hi)
        assert np.allclose(w.sum(axis=0), 1.0, rtol=1e-14) and (x >= 0).all() and (x.min(axis=0) == 0).all()
        assert (ess >= 1).all() and (ess <= 9).all() and not st.any()
        if lo is not None:
            assert (uo >= lo).all() and (uo <= hi).all() and (u[:, None] + d >= lo - 1e-15).all() and (u[:, None] + d <= hi + 1e-15).all()
        else:
            assert np.array_equal(d, du)
    # scaling J and lam together changes nothing
    a = mppi_update(J, du, u, 0.7, lo, hi)
    b = mppi_update(2 * J, du, u, 1.4, lo, hi)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_oracle_status_and_nan_rules():
    J, du, u = _draw(2, 7, 5)
    Jb = J.copy()
    Jb[:, 1] = np.nan                      # every sample NaN
    Jb[:, 2] = np.inf
    Jb[3, 3] = -np.inf                     # a -inf among them
    Jb[2, 0] = np.nan                      # one NaN: that sample drops out
    lam = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    uo, w, x, d, D, ess, st = mppi_update(Jb, du, u, lam, -0.6, 0.6)
    assert st.tolist() == [0, 1, 1, 1, 0]
    for p in (1, 2, 3):
        assert np.array_equal(uo[:, p], np.clip(u[:, p], -0.6, 0.6)) and not w[:, p].any() and ess[p] == 0
    Ji = Jb.copy(); Ji[2, 0] = np.inf
    assert all(np.array_equal(a, b) for a, b in zip(mppi_update(Ji, du, u, lam, -0.6, 0.6), (uo, w, x, d, D, ess, st)))
    assert w[2, 0] == 0 and np.isclose(w[:, 0].sum(), 1)
    ref = mppi_update(J[:, 4:], du[:, :, 4:], u[:, 4:], 1.0, -0.6, 0.6)
    assert np.array_equal(uo[:, 4:], ref[0]) and np.array_equal(w[:, 4:], ref[1])      # the neighbours do not notice
    for bad in (0.0, -1.0, np.nan, np.inf):
        l2 = lam.copy(); l2[4] = bad
        uo2, w2, _, _, _, ess2, st2 = mppi_update(J, du, u, l2)
        assert st2.tolist() == [0, 0, 0, 0, 2] and np.array_equal(uo2[:, 4], u[:, 4]) and not w2[:, 4].any() and ess2[4] == 0
        assert np.array_equal(uo2[:, :4], mppi_update(J[:, :4], du[:, :, :4], u[:, :4], 1.0)[0])
    # a NaN in du shows in its own (t, p, j) alone
    dn = du.copy(); dn[1, 3, 2, 4] = np.nan
    un = mppi_update(J, dn, u, 1.0)[0]
    base = mppi_update(J, du, u, 1.0)[0]
    mask = np.zeros(u.shape, dtype=bool); mask[1, 2, 4] = True
    assert np.isnan(un[mask]).all() and np.array_equal(un[~mask], base[~mask])


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_driver_oracle_records_the_open_loop_cost_of_each_nominal(integ):
    om = orc.model_from_robot(make_robot("iiwa_like"))
    p = ilqr_problem(om.n)
    T, P, n = p["u"].shape
    S, iters = 9, 2
    noise = np.random.default_rng(3).standard_normal((iters, T, S, P, n))
    c = cost_arrays(p)
    for lims in (dict(), dict(u_min=-4.0, u_max=4.0)):
        r = mppi(om, p["q0"], p["qd0"], p["u"], 0.01, c, noise, sigma=0.5, lam=500.0, integrator=integ, **lims)
        assert r.cost.shape == (iters + 1, P) and r.ess.shape == r.status.shape == (iters, P) and not r.status.any()
        assert r.u.shape == r.q.shape == r.qd.shape == (T, P, n) and (r.ess > 1).all() and (r.ess <= S).all()
        for i in range(iters):
            J = rollout_cost(om, p["q0"], p["qd0"], r.nominal[i], 0.01, c, integrator=integ, **lims)[0]
            assert np.array_equal(r.cost[i], J), i
            assert not r.du[i][:, 0].any()
        Jf, q, qd, _ = rollout_cost(om, p["q0"], p["qd0"], r.u, 0.01, c, integrator=integ, **lims)
        assert np.array_equal(r.cost[iters], Jf) and np.array_equal(r.q, q) and np.array_equal(r.qd, qd)
        assert np.array_equal(r.u, r.update[-1][0])
    r0 = mppi(om, p["q0"], p["qd0"], p["u"], 0.01, c, noise[:0], integrator=integ)
    assert np.array_equal(r0.u, p["u"]) and r0.cost.shape == (1, P) and r0.ess.shape == (0, P)
