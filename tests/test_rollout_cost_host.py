"""rollout_cost and ilqr without a GPU: build wiring, the C-ABI's refusals (every check comes before the launch, so fake
pointers are never dereferenced), the API's refusals, QuadraticCost against the cost helpers of the closed-loop oracle, and
the numpy restatement of the iLQR driver on the quadratic tracking problem the GPU tests use."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from ilqr_oracle import ALPHAS, choose, ilqr
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from rollout_closed_loop_oracle import cost, cost_model, ilqr_problem, rollout_closed_loop
from rollout_cost_oracle import cost_arrays, cost_of_trajectory, draw_cost, rollout_cost
from rollout_oracle import INTEGRATORS, rollout

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_rollout_cost") == "rollcost"
    assert FAMILIES["rollcost"] == ["ROLLCOST"]
    assert "ROLLCOST" in _ALL_FAMILY_UNITS
    assert "ROLLCOST_F32" in TRANSLATION_UNITS and "ROLLCOST_F64" in TRANSLATION_UNITS
    assert "ROLLCOST_F32" in _TU_COST and "ROLLCOST_F64" in _TU_COST
    assert family_of("rbd_rollout_closed_loop") == "rollcl" and FAMILIES["rollcl"] == ["ROLLCL"]      # untouched
    assert family_of("rbd_rollout") == "roll" and FAMILIES["roll"] == ["ROLL"]
    names = {"rbd_rollout_cost_f32", "rbd_rollout_cost_f64"}
    assert names <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert "int rbd_rollout_cost_f32(" in hdr and "int rbd_rollout_cost_f64(" in hdr
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert names <= found and found == set(EXPORTED_SYMBOLS)
    src = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_kernels.hip")).read()
    assert '#include "rbd_rollout_cost.h"' in src and "RBD_TU_ROLLCOST_F32" in src and "RBD_TU_ROLLCOST_F64" in src
    capi = open(os.path.join(ROOT, "rbdreference_amd", "csrc", "rbd_capi.h")).read()
    assert "RBD_DEFS_ROLLCOST" in capi and "RBD_STUBS_ROLLCOST" in capi
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # an addition: the ABI version stays


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_rollcost_family_library_refuses_bad_arguments_before_any_launch(sfx, ft):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "rollcost", sfx)
    assert p == family_lib_path(m, "rollcost", sfx) and os.path.exists(p)
    lib = ctypes.CDLL(p)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 6
    assert lib.rbd_abi_version() == 2
    fn = getattr(lib, f"rbd_rollout_cost_{sfx}")
    other = getattr(lib, f"rbd_rollout_cost_{'f64' if sfx == 'f32' else 'f32'}")
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first

    def call(q0=fake, qd0=fake, u=fake, k=fake, K=fake, q0_ref=fake, qd0_ref=fake, q_ref=fake, qd_ref=fake, alpha=fake, du=fake,
             u_lo=None, u_hi=None, q_tgt=fake, qd_tgt=fake, w_q=fake, w_qd=fake, final=0, w_u=fake, c_u=fake, dt=0.01, g=-9.81,
             integ=0, B=4, B_nom=2, T=3, cost=fake, q=fake, qd=fake, traj=1, u_out=fake):
        return fn(q0, qd0, u, k, K, q0_ref, qd0_ref, q_ref, qd_ref, alpha, du, u_lo, u_hi, q_tgt, qd_tgt, w_q, w_qd, final, w_u, c_u,
                  dt, g, integ, B, B_nom, T, cost, q, qd, traj, u_out, None)

    def refused(msg, **kw):
        assert call(**kw) == RBD_ERR_ARG, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    for name in ("q0", "qd0", "u", "cost"):
        refused(b"must be non-null", **{name: None})
    for name in ("q0_ref", "qd0_ref", "q_ref", "qd_ref"):
        refused(b"K needs", **{name: None})
    refused(b"k and alpha", k=None)
    refused(b"k and alpha", alpha=None)
    refused(b"u_lo and u_hi", u_lo=fake)
    refused(b"u_lo and u_hi", u_hi=fake)
    refused(b"q_out and qd_out", q=None)
    refused(b"q_out and qd_out", qd=None)
    refused(b"B < 0", B=-1)
    refused(b"T < 0", T=-1)
    for bad in (0, -1, 3, 8):
        refused(b"B_nom must be positive and divide B", B_nom=bad)
    for bad in (float("inf"), float("-inf"), float("nan")):
        refused(b"dt must be finite", dt=bad)
    for bad in (-1, 2, 7):
        refused(b"unknown integrator", integ=bad)
    refused(b"B too large", B=2 ** 62, B_nom=2 ** 61)
    refused(b"B * T * n too large", B=2 ** 30, B_nom=1, T=2 ** 40)
    refused(b"B * T * n too large", B=1, B_nom=1, T=2 ** 62)
    refused(b"B_nom * T * n * 2n too large", B=1, B_nom=1, T=2 ** 52)
    for name in ("cost", "q", "qd", "u_out"):
        refused(b"16-byte aligned", **{name: ctypes.c_void_p(4096 + 8)})
    # nothing to do: success, nothing touched (not even the null pointers, and B_nom is not looked at)
    assert call(B=0) == 0 and call(T=0) == 0 and call(B=0, T=0, traj=0) == 0 and call(B=0, B_nom=0) == 0
    nul = [None] * 17
    assert fn(*nul, 0, None, None, 0.01, -9.81, 0, 0, 0, 5, None, None, None, 1, None, None) == 0
    assert fn(*nul, 1, None, None, 0.01, -9.81, 1, 5, 5, 0, None, None, None, 0, None, None) == 0
    # the other precision is another family library's
    assert other(*[fake] * 11, None, None, *[fake] * 4, 0, fake, fake, 0.01, -9.81, 0, 4, 2, 3, fake, fake, fake, 1, fake, None) == -4
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
    q, tr = np.zeros((2, api.nv)), np.zeros((3, 2, api.nv))
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout_cost(q, q, tr, 0.01, QuadraticCost())
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.ilqr(q, q, tr, 0.01, QuadraticCost())


def test_api_refuses_bad_shapes_and_types_before_any_launch():
    from rbdreference_amd import QuadraticCost
    api = _bare_api(make_robot("iiwa_like"))
    n, B, T = 7, 6, 3
    z = np.zeros
    cm = QuadraticCost(w_q=np.ones((T, B, n)), w_u=np.ones(n))
    good = dict(q0=z((B, n)), qd0=z((B, n)), u=z((T, B, n)), dt=0.01, cost=cm)
    fb = dict(K=z((T, B, n, 2 * n)), q_ref=z((T, B, n)), qd_ref=z((T, B, n)))
    bad = [
        dict(u=z((0, B, n))),                                   # T == 0
        dict(u=z((B, T, n))),                                   # batch-major u
        dict(u=z((T, n))),
        dict(u=z((T, 4, n))),                                   # B_nom does not divide B
        dict(q0=z(n), qd0=z(n)),
        dict(qd0=z((B + 1, n))),
        dict(q_ref=z((T, B, n))),                               # a reference without K
        dict(K=fb["K"]),                                        # K without the reference
        dict(**fb, q0_ref=z((B, n))),                           # one without the other
        dict({**fb, "K": z((T, B, n, n))}),
        dict(**fb, k=z((T, B))),
        dict(u=z((T, 2, n)), K=z((T, 2, n, 2 * n)), q_ref=z((T, 2, n)), qd_ref=z((T, 2, n))),   # shared nominal: q0_ref needed
        dict(du=z((T, B + 1, n))),
        dict(du=z((T, B, n)), k=z((T, B, n)), alpha=[1.0, 0.5]),                                # 1-D alpha: du is [T, A, B, n]
        dict(u=z((T, 2, n)), k=z((T, 2, n)), alpha=[1.0, 0.5]),
        dict(u_min=-1.0),
        dict(u_min=-np.ones(n + 1), u_max=np.ones(n + 1)),
        dict(alpha=z((2, 2))),
        dict(alpha=[]),
        dict(k=z((T, B, n)), alpha=0.5, row_alpha=z(B)),        # row_alpha given with alpha
        dict(k=z((T, B, n)), alpha=[1.0, 0.5], row_alpha=z(B)),
        dict(row_alpha=z(B)),                                   # nothing to scale
        dict(k=z((T, B, n)), row_alpha=z(B + 1)),
        dict(cost=QuadraticCost(w_q=np.ones((T, B + 1, n)))),
        dict(cost=QuadraticCost(w_q=np.ones((B, n)), terminal_state_only=True, c_u=np.ones((B, n + 1)))),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="rollout_cost|QuadraticCost"):
            api.rollout_cost(**{**good, **kw})
    with pytest.raises(TypeError, match="QuadraticCost"):
        api.rollout_cost(**{**good, "cost": dict(w_q=1.0)})
    with pytest.raises(ValueError, match="return_final or return_trajectory"):
        api.rollout_cost(**good, return_final=True, return_trajectory=True)
    import torch
    with pytest.raises(TypeError, match="mixing numpy and torch"):
        api.ilqr(**{**good, "cost": QuadraticCost(w_u=torch.ones(n))})
    with pytest.raises(ValueError, match="QuadraticCost"):
        QuadraticCost(w_q=np.ones((T, B, n)), terminal_state_only=True)
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_cost(**good, integrator=integ)
    # rollout_closed_loop's new keyword is refused the same way
    cl = dict(q0=z((B, n)), qd0=z((B, n)), u=z((T, B, n)), dt=0.01, **fb)
    for kw in (dict(k=z((T, B, n)), alpha=0.5, row_alpha=z(B)), dict(row_alpha=z(B)), dict(k=z((T, B, n)), row_alpha=z((B, 1)))):
        with pytest.raises(ValueError, match="row_alpha"):
            api.rollout_closed_loop(**cl, **kw)
    for kw in (dict(iters=-1), dict(alphas=[]), dict(reg=[0.0, 0.0], iters=3), dict(u=z((T, B + 1, n)))):
        with pytest.raises(ValueError, match="ilqr"):
            api.ilqr(**{**good, **kw})


@pytest.mark.parametrize("n", [7, 9])
def test_quadratic_cost_value_and_derivatives_match_the_closed_loop_oracles_cost(n):
    from rbdreference_amd import QuadraticCost
    p = ilqr_problem(n)
    T, B = p["u"].shape[:2]
    rng = np.random.default_rng(5)
    q, qd, u = rng.standard_normal((3, T, B, n))
    cm = QuadraticCost(**cost_arrays(p))
    assert np.array_equal(cm.value(q, qd, u), cost(p, q, qd, u))
    J, mag = cost_of_trajectory(cost_arrays(p), q, qd, u)
    assert np.allclose(J, cost(p, q, qd, u), rtol=1e-14, atol=0) and (mag >= np.abs(J)).all()
    qa, qda, ua = rng.standard_normal((3, T, 4, B, n))                     # a line search's [T, A, B, n]
    assert np.array_equal(cm.value(qa, qda, ua), cost(p, qa, qda, ua))
    d, ref = cm.derivatives(q, qd, u), cost_model(p, q, qd, u)
    for mine, theirs in (("grad_q", "gq"), ("grad_qd", "gqd"), ("hess_q", "hq"), ("hess_qd", "hqd"), ("grad_u", "gu"), ("hess_u", "hu")):
        assert d[mine].shape == (T, B, n) and np.allclose(d[mine], ref[theirs], rtol=1e-15, atol=0), mine
    # central differences of value: J is quadratic, so they are exact up to rounding
    h = 1e-2
    for x, g, hh in ((0, "grad_q", "hess_q"), (1, "grad_qd", "hess_qd"), (2, "grad_u", "hess_u")):
        t, j = 2, n // 2
        args = [q, qd, u]
        e = np.zeros((T, B, n)); e[t, :, j] = h
        plus, minus = [[a + s * e if i == x else a for i, a in enumerate(args)] for s in (1, -1)]
        Jp, Jm, J0 = cm.value(*plus), cm.value(*minus), cm.value(q, qd, u)
        scale = np.abs(d[g][t, :, j]).max()
        assert np.abs((Jp - Jm) / (2 * h) - d[g][t, :, j]).max() <= 1e-6 * scale
        assert np.abs((Jp - 2 * J0 + Jm) / h ** 2 - d[hh][t, :, j]).max() <= 1e-6 * np.abs(d[hh][t, :, j]).max()
    # torch tensors give the same numbers
    import torch
    tt = lambda a: torch.tensor(a)      # noqa: E731
    ct = QuadraticCost(**{k_: tt(v) for k_, v in cost_arrays(p).items()})
    assert np.allclose(ct.value(tt(q), tt(qd), tt(u)).numpy(), cm.value(q, qd, u), rtol=1e-14, atol=0)
    for key, v in ct.derivatives(tt(q), tt(qd), tt(u)).items():
        assert np.array_equal(v.numpy(), d[key]), key


def test_quadratic_cost_broadcast_terminal_and_missing_forms_equal_their_expanded_forms():
    from rbdreference_amd import QuadraticCost
    T, B, n = 4, 3, 5
    rng = np.random.default_rng(11)
    q, qd, u = rng.standard_normal((3, T, B, n))
    wn, wtn, tn = rng.uniform(1, 2, n), rng.uniform(1, 2, (T, n)), rng.uniform(-1, 1, (T, n))
    small = QuadraticCost(w_q=wn, w_qd=wtn, q_target=tn, w_u=wn, c_u=tn)
    ex = lambda a: np.broadcast_to(a if a.ndim == 1 else a[:, None, :], (T, B, n)).copy()      # noqa: E731
    big = QuadraticCost(w_q=ex(wn), w_qd=ex(wtn), q_target=ex(tn), w_u=ex(wn), c_u=ex(tn))
    assert np.array_equal(small.value(q, qd, u), big.value(q, qd, u))
    ds, db = small.derivatives(q, qd, u), big.derivatives(q, qd, u)
    for key in db:
        assert np.array_equal(ds[key], db[key]), key
    for key, v in small.dense(T, B, n).items():
        w = big.dense(T, B, n)[key]
        assert (v is None and w is None) or (v.shape == (T, B, n) and np.array_equal(v, w)), key
    # terminal state cost: the state terms of the last slice alone, [B, n] or [n]
    wf, tf = rng.uniform(1, 2, (B, n)), rng.uniform(-1, 1, (B, n))
    fin = QuadraticCost(w_q=wf, q_target=tf, w_qd=wn, w_u=wtn, terminal_state_only=True)
    J, _ = cost_of_trajectory(dict(w_q=wf, q_target=tf, w_qd=np.broadcast_to(wn, (B, n)), w_u=ex(wtn)), q, qd, u, final=True)
    assert np.allclose(fin.value(q, qd, u), J, rtol=1e-14, atol=0)
    d = fin.derivatives(q, qd, u)
    assert d["grad_q"].shape == d["hess_q"].shape == d["grad_qd"].shape == (B, n) and d["grad_u"].shape == (T, B, n)
    assert np.array_equal(d["grad_q"], wf * (q[-1] - tf)) and np.array_equal(d["grad_qd"], wn * qd[-1])
    # missing pieces: a missing weight drops its term, a missing target or c_u is zero
    none = QuadraticCost()
    assert np.array_equal(none.value(q, qd, u), np.zeros(B))
    d = none.derivatives(q, qd, u)
    assert d["grad_q"] is None and d["hess_qd"] is None and not d["hess_u"].any() and not d["grad_u"].any()
    only = QuadraticCost(q_target=tn, c_u=tn)                        # a target without its weight counts for nothing
    assert np.allclose(only.value(q, qd, u), (tn[:, None, :] * u).sum(axis=(0, -1)), rtol=1e-14, atol=0)


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_cost_oracle_is_the_closed_loop_oracle_with_the_cost_of_its_trajectory(integ):
    om = orc.model_from_robot(make_robot("random_prismatic_n6"))
    n, B, T = om.n, 4, 5
    rng = np.random.default_rng(9)
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
    q, qd = rollout(om, q0, qd0, u, 0.01, integrator=integ)
    k, K = rng.standard_normal(u.shape), rng.uniform(-2, 2, u.shape + (2 * n,))
    c = draw_cost(rng, T, B, n)
    J, qa, qda, ua = rollout_cost(om, q0 + 0.05, qd0, u, 0.01, c, K=K, q_ref=q, qd_ref=qd, k=k, alpha=0.7, q0_ref=q0, qd0_ref=qd0,
                                  integrator=integ)
    ref = rollout_closed_loop(om, q0 + 0.05, qd0, u, q, qd, K, 0.01, k=k, alpha=0.7, q0_ref=q0, qd0_ref=qd0, integrator=integ)
    assert all(np.array_equal(a, b) for a, b in zip((qa, qda, ua), ref))
    p = dict(hq=c["w_q"], hqd=c["w_qd"], tq=c["q_target"], tqd=c["qd_target"], hu=c["w_u"], cu=c["c_u"])
    assert np.allclose(J, cost(p, *ref), rtol=1e-14, atol=0)
    # open loop: the plain rollout; du adds to the control; a nominal of one row serves every row
    J0, qo, qdo, uo = rollout_cost(om, q0, qd0, u, 0.01, c, integrator=integ)
    assert np.array_equal(qo, q) and np.array_equal(qdo, qd) and np.array_equal(uo, u)
    du = rng.normal(0, 0.1, (T, B, n))
    c1 = {key: v[:, :1] for key, v in c.items()}
    Js, _, _, us = rollout_cost(om, q0, qd0, u[:, :1], 0.01, c1, du=du, integrator=integ)
    Jt, _, _, ut = rollout_cost(om, q0, qd0, np.tile(u[:, :1], (1, B, 1)) + du, 0.01, {key: np.tile(v, (1, B, 1)) for key, v in c1.items()},
                                integrator=integ)
    assert np.array_equal(us, ut) and np.array_equal(Js, Jt)


def test_choose_takes_the_lowest_index_minimum_and_counts_nan_as_infinite():
    Jc = np.array([[3.0, np.nan, 5.0, np.nan], [2.0, 4.0, 5.0, np.nan], [2.0, 1.0, 7.0, np.nan]])
    J = np.array([2.5, 1.0, 5.0, 9.0])
    J_best, idx, accept, ra = choose(Jc, J, [1.0, 0.5, 0.25])
    assert idx.tolist()[:3] == [1, 2, 0] and accept.tolist() == [True, False, False, False]
    assert J_best[:3].tolist() == [2.0, 1.0, 5.0] and np.isinf(J_best[3]) and ra.tolist() == [0.5, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_ilqr_oracle_accepts_the_full_step_and_never_raises_the_cost(name, integ):
    """On ilqr_problem (B = 3, T = 5) both robots accept alpha = 1 in every row at iterations 0 and 1 with status == 0; the
    best candidate is separated from the second best by at least 0.079 (relative) at iteration 0, and on the arm by at least
    7.5e-4 at iteration 1, while the tree's is below 1e-5 there (so the tree is compared at iteration 0 only) -- the margins that make the GPU test's comparison of choices meaningful."""
    om = orc.model_from_robot(make_robot(name))
    r = ilqr(om, ilqr_problem(om.n), 3, integrator=integ)
    print(name, integ, "cost history:\n", r.cost)
    assert r.cost.shape == (4, 3) and r.alpha.shape == (3, 3) and r.dV.shape == (3, 3, 2) and r.candidates.shape == (3, len(ALPHAS), 3)
    assert (r.alpha[:2] == 1.0).all() and (r.status[:2] == 0).all()
    assert (np.diff(r.cost, axis=0) <= 0).all()
    srt = np.sort(r.candidates, axis=1)
    gap = (srt[:, 1] - srt[:, 0]) / np.abs(srt[:, 0])
    print(name, integ, "relative gap best / second best:", gap.min(axis=1))
    assert gap[0].min() >= 0.079
    if name == "iiwa_like":
        # (this oracle gives 7.591e-4 with the semi-implicit integrator and 8.33e-4 with Euler: 7.6e-4 to two digits, so the
        # threshold is the next round figure below what the reference itself gives)
        assert gap[1].min() >= 7.5e-4
        assert r.cost[0].min() > 1e4 and r.cost[2].max() < 1e3
        if integ == "semi_implicit":
            assert np.allclose(r.cost[2], [529, 596, 653], atol=1.0)
    else:
        assert gap[1].min() < 1e-5
    # a rejected row keeps everything: make every candidate worse than the nominal by starting at the optimum's cost
    J = r.cost[-1]
    _, _, accept, ra = choose(r.candidates[-1] + 1e9, J, ALPHAS)
    assert not accept.any() and not ra.any()
