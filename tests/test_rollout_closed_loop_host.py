"""rollout_closed_loop without a GPU: build wiring, the C-ABI's refusals (every check comes before the launch, so fake
pointers are never dereferenced), the API's refusals, and the numpy restatement the GPU tests compare against -- with the
end-to-end cost check that pins the time-index convention of the control law."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot
from oracle import rbd_oracle as orc
from rbdreference_amd.packer import pack_robot
from rollout_closed_loop_oracle import cost, cost_model, ilqr_problem, predicted_ratio, rollout_closed_loop
from rollout_lqr_oracle import rollout_lqr
from rollout_oracle import INTEGRATORS, rollout

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def test_family_and_exports():
    from rbdreference_amd._lib import EXPORTED_SYMBOLS
    from rbdreference_amd.build import _ALL_FAMILY_UNITS, _TU_COST, FAMILIES, TRANSLATION_UNITS, family_of
    assert family_of("rbd_rollout_closed_loop") == "rollcl"
    assert FAMILIES["rollcl"] == ["ROLLCL"]
    assert "ROLLCL" in _ALL_FAMILY_UNITS
    assert "ROLLCL_F32" in TRANSLATION_UNITS and "ROLLCL_F64" in TRANSLATION_UNITS
    assert "ROLLCL_F32" in _TU_COST and "ROLLCL_F64" in _TU_COST
    assert family_of("rbd_rollout") == "roll" and FAMILIES["roll"] == ["ROLL"]            # untouched
    names = {"rbd_rollout_closed_loop_f32", "rbd_rollout_closed_loop_f64"}
    assert names <= set(EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert "int rbd_rollout_closed_loop_f32(" in hdr and "int rbd_rollout_closed_loop_f64(" in hdr
    found = set(re.findall(r"(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert names <= found and found == set(EXPORTED_SYMBOLS)
    from rbdreference_amd.packer import ABI_VERSION
    assert ABI_VERSION == 2                             # an addition: the ABI version stays


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("sfx,ft", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_rollcl_family_library_refuses_bad_arguments_before_any_launch(sfx, ft):
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RBD_ERR_ARG, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path
    m = pack_robot(make_robot("random_prismatic_n6"))
    p = build_family(m, "rollcl", sfx)
    assert p == family_lib_path(m, "rollcl", sfx) and os.path.exists(p)
    lib = ctypes.CDLL(p)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 6
    assert lib.rbd_abi_version() == 2
    fn = getattr(lib, f"rbd_rollout_closed_loop_{sfx}")
    other = getattr(lib, f"rbd_rollout_closed_loop_{'f64' if sfx == 'f32' else 'f32'}")
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first

    def call(q0=fake, qd0=fake, u=fake, k=fake, K=fake, q0_ref=fake, qd0_ref=fake, q_ref=fake, qd_ref=fake, alpha=fake, u_lo=None,
             u_hi=None, dt=0.01, g=-9.81, integ=0, B=4, B_nom=2, T=3, q=fake, qd=fake, traj=1, u_out=fake):
        return fn(q0, qd0, u, k, K, q0_ref, qd0_ref, q_ref, qd_ref, alpha, u_lo, u_hi, dt, g, integ, B, B_nom, T, q, qd, traj, u_out, None)

    def refused(msg, **kw):
        assert call(**kw) == RBD_ERR_ARG, kw
        assert msg in lib.rbd_last_error(), (kw, lib.rbd_last_error())

    for name in ("q0", "qd0", "u", "K", "q0_ref", "qd0_ref", "q_ref", "qd_ref", "q", "qd"):
        refused(b"must be non-null", **{name: None})
    refused(b"k and alpha", k=None)
    refused(b"k and alpha", alpha=None)
    refused(b"u_lo and u_hi", u_lo=fake)
    refused(b"u_lo and u_hi", u_hi=fake)
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
    for name in ("q", "qd", "u_out"):
        refused(b"16-byte aligned", **{name: ctypes.c_void_p(4096 + 8)})
    # nothing to do: success, nothing touched (not even the null pointers, and B_nom is not looked at)
    assert call(B=0) == 0 and call(T=0) == 0 and call(B=0, T=0, traj=0) == 0 and call(B=0, B_nom=0) == 0
    nul = [None] * 12
    assert fn(*nul, 0.01, -9.81, 0, 0, 0, 5, None, None, 1, None, None) == 0
    assert fn(*nul, 0.01, -9.81, 1, 5, 5, 0, None, None, 0, None, None) == 0
    # the other precision is another family library's
    assert other(*[fake] * 10, None, None, 0.01, -9.81, 0, 4, 2, 3, fake, fake, 1, fake, None) == -4
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
    q, tr = np.zeros(api.nv), np.zeros((3, api.nv))
    with pytest.raises(NotImplementedError, match="fixed-base robots only"):
        api.rollout_closed_loop(q, q, tr, tr, tr, np.zeros((3, api.nv, 2 * api.nv)), 0.01)


def test_api_refuses_bad_shapes_and_types_before_any_launch():
    api = _bare_api(make_robot("iiwa_like"))
    n, B, T = 7, 5, 3
    good = dict(q0=np.zeros((B, n)), qd0=np.zeros((B, n)), u=np.zeros((T, B, n)), q_ref=np.zeros((T, B, n)),
                qd_ref=np.zeros((T, B, n)), K=np.zeros((T, B, n, 2 * n)), dt=0.01)
    bad = [
        dict(u=np.zeros((0, B, n)), q_ref=np.zeros((0, B, n)), qd_ref=np.zeros((0, B, n)), K=np.zeros((0, B, n, 2 * n))),   # T == 0
        dict(u=np.zeros((B, T, n))),                  # batch-major u
        dict(u=np.zeros((T, n))),                     # a shared control sequence is rollout's, not this entry point's
        dict(u=np.zeros((T, B + 1, n))),
        dict(q_ref=np.zeros((T - 1, B, n))),          # the reference has T slices (the last is never read)
        dict(qd_ref=np.zeros((T, B, n + 1))),
        dict(K=np.zeros((T, B, n, n))),
        dict(K=np.zeros((T, B, 2 * n, n))),
        dict(K=np.zeros((B, n, 2 * n))),
        dict(K=None),
        dict(q_ref=None),
        dict(k=np.zeros((T, B))),
        dict(k=np.zeros((B, n))),
        dict(qd0=np.zeros((B + 1, n))),
        dict(q0=np.zeros((B, n + 1)), qd0=np.zeros((B, n + 1))),
        dict(q0=np.zeros(n), qd0=np.zeros(n)),        # an unbatched state takes u [T, n]
        dict(q0_ref=np.zeros((B, n))),                # one without the other
        dict(q0_ref=np.zeros((B, n)), qd0_ref=np.zeros((B + 1, n))),
        dict(q0_ref=np.zeros((1, n)), qd0_ref=np.zeros((1, n))),
        dict(u_min=-1.0),
        dict(u_max=np.ones(n)),
        dict(u_min=-np.ones(n + 1), u_max=np.ones(n + 1)),
        dict(u_min=-np.ones((B, n)), u_max=np.ones((B, n))),
        dict(alpha=np.zeros((2, 2))),
        dict(alpha=[]),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="rollout_closed_loop"):
            api.rollout_closed_loop(**{**good, **kw})
    for integ in ("rk4", "Euler", 0, None):
        with pytest.raises(ValueError, match="unknown integrator"):
            api.rollout_closed_loop(**good, integrator=integ)


def _nominal(name, integ, B=3, T=5, seed=3):
    om = orc.model_from_robot(make_robot(name))
    rng = np.random.default_rng(seed)
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, om.n)), rng.uniform(-1, 1, (B, om.n)), rng.uniform(-5, 5, (T, B, om.n))
    q, qd = rollout(om, q0, qd0, u, 0.01, integrator=integ)
    return om, rng, q0, qd0, u, q, qd


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_oracle_without_feedback_is_the_open_loop_rollout_bit_for_bit(integ):
    om, rng, q0, qd0, u, q, qd = _nominal("random_prismatic_n6", integ)
    n = om.n
    k, K = rng.standard_normal(u.shape), rng.uniform(-2, 2, u.shape + (2 * n,))
    # alpha = 0 and dx_0 = 0: the feedback term stays exactly zero along the nominal
    a = rollout_closed_loop(om, q0, qd0, u, q, qd, K, 0.01, k=k, alpha=0.0, integrator=integ)
    assert np.array_equal(a[0], q) and np.array_equal(a[1], qd) and np.array_equal(a[2], u)
    # K = 0 and no feed-forward term: whatever the reference is
    b = rollout_closed_loop(om, q0, qd0, u, q + 1.0, qd - 1.0, np.zeros_like(K), 0.01, q0_ref=q0 + 0.5, qd0_ref=qd0, integrator=integ)
    assert np.array_equal(b[0], q) and np.array_equal(b[1], qd) and np.array_equal(b[2], u)
    f = rollout_closed_loop(om, q0, qd0, u, q, qd, K, 0.01, k=k, alpha=0.0, integrator=integ, trajectory=False)
    assert np.array_equal(f[0], q[-1]) and np.array_equal(f[1], qd[-1]) and f[2].shape == u.shape
    # with feedback and a start off the reference it is another trajectory, and the limits bite
    c = rollout_closed_loop(om, q0 + 0.05, qd0, u, q, qd, K, 0.01, k=k, alpha=0.7, q0_ref=q0, qd0_ref=qd0, integrator=integ)
    assert np.abs(c[0] - q).max() > 1e-3
    d = rollout_closed_loop(om, q0 + 0.05, qd0, u, q, qd, K, 0.01, k=k, alpha=0.7, q0_ref=q0, qd0_ref=qd0, u_min=-3.0, u_max=3.0,
                            integrator=integ)
    assert d[2].min() == -3.0 and d[2].max() == 3.0 and np.abs(c[2]).max() > 3.0
    assert np.array_equal(d[2][0], np.clip(c[2][0], -3.0, 3.0))         # the first step sees the same state


def test_oracle_with_a_shared_nominal_equals_separate_calls():
    om, rng, q0, qd0, u, q, qd = _nominal("iiwa_like", "semi_implicit")
    k, K = rng.standard_normal(u.shape), rng.uniform(-2, 2, u.shape + (2 * om.n,))
    alphas = [1.0, 0.5, 0.0]
    for traj in (True, False):
        many = rollout_closed_loop(om, q0, qd0, u, q, qd, K, 0.01, k=k, alpha=alphas, trajectory=traj)
        assert many[0].shape == ((5, 3, 3, om.n) if traj else (3, 3, om.n)) and many[2].shape == (5, 3, 3, om.n)
        for i, a in enumerate(alphas):
            one = rollout_closed_loop(om, q0, qd0, u, q, qd, K, 0.01, k=k, alpha=a, trajectory=traj)
            for x, y in zip(many, one):
                assert np.array_equal(x[..., i, :, :], y)


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9", "atlas_like"])
def test_one_ilqr_step_changes_the_cost_as_the_backward_pass_predicts(name, integ):
    """rollout -> linearise -> riccati -> closed loop at alpha = 0.1 and 0.01: the cost changes by alpha dV[0] +
    alpha^2 dV[1] to within 0.1 alpha relative (the nonlinear remainder; the oracle chain itself gives at most 0.034 alpha
    on these draws).  Reading reference slice t instead of t - 1 in the control law moves u by O(1) and fails this by
    orders of magnitude: the check pins the time-index convention."""
    om = orc.model_from_robot(make_robot(name))
    p = ilqr_problem(om.n)
    q, qd = rollout(om, p["q0"], p["qd0"], p["u"], 0.01, integrator=integ)
    k, K, _, _, dV, status = rollout_lqr(om, p["q0"], p["qd0"], p["u"], 0.01, q, qd, integrator=integ, **cost_model(p, q, qd, p["u"]))
    assert (status == 0).all()
    alphas = [0.1, 0.01]
    qa, qda, ua = rollout_closed_loop(om, p["q0"], p["qd0"], p["u"], q, qd, K, 0.01, k=k, alpha=alphas, integrator=integ)
    r = np.abs(predicted_ratio(cost(p, q, qd, p["u"]), cost(p, qa, qda, ua), alphas, dV))
    print(name, integ, "|dJ / predicted - 1| / alpha:", (r.max(axis=1) / np.array(alphas)).round(4))
    assert (r <= 0.1 * np.array(alphas)[:, None]).all(), r
