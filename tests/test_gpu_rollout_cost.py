"""RBDReference.rollout_cost and RBDReference.ilqr on the GPU (rbd_rollout_cost_f32 / _f64, csrc/rbd_rollout_cost.h).

The cost check runs on the DEVICE'S OWN trajectory: the call stores q, qd and u_applied, which are exactly the on-chip
values the kernel's chain read, and the oracle sums the same 4 n T terms from them in float64.  Per row

    |J - J_ref| <= 2 (4 n T + 8) eps sum |terms|

-- 4 n T terms of at most four roundings each (the difference to the target, two products, the fused add) plus the chain of
their sum, doubled like the bounds of test_gpu_rollout_closed_loop.py.  The stored trajectory itself meets
test_gpu_rollout.check_teacher_forced's bounds and test_gpu_rollout_closed_loop.check_controls'."""
import ctypes

import numpy as np
import pytest

from conftest import make_robot
from ilqr_oracle import ALPHAS, choose, ilqr
from oracle import rbd_oracle as orc
from rollout_closed_loop_oracle import ilqr_problem
from rollout_cost_oracle import KEYS, cost_arrays, cost_of_trajectory, draw_cost
from rollout_oracle import INTEGRATORS
from test_gpu_rollout import DT, EPS32, EPS64, ROBOTS, _dev, _dtype, _np, _om, _rbd, _torch, check_teacher_forced
from test_gpu_rollout_closed_loop import ALPHA, _case, check_controls

pytestmark = pytest.mark.gpu


def _cost_dev(name, B, T, sfx, seed=0, final=False):
    """The six cost arrays drawn like ilqr_problem's, as device tensors of the run's precision."""
    n = _om(name).n
    c = draw_cost(np.random.default_rng(5000 * seed + n), T, B, n, final)
    return dict(zip(c, _dev(_dtype(sfx), *c.values())))


def _qc(cd, final=False, drop=()):
    from rbdreference_amd import QuadraticCost
    return QuadraticCost(**{key: (None if key in drop else v) for key, v in cd.items()}, terminal_state_only=final)


def check_cost(tag, cd, J, q, qd, ua, sfx, final=False, drop=()):
    """cd: the device cost arrays; J, q, qd, ua: what the kernel returned.  Prints the worst error / bound, then asserts."""
    eps = EPS32 if sfx == "f32" else EPS64
    T, B, n = ua.shape
    ref, mag = cost_of_trajectory({key: (None if key in drop else _np(v)) for key, v in cd.items()}, _np(q), _np(qd), _np(ua), final)
    J = _np(J)
    assert J.shape == (B,) and np.isfinite(J).all(), tag
    bound = 2 * (4 * n * T + 8) * eps * mag
    if not mag.any():
        assert not J.any(), tag
        return 0.0
    worst = float(np.max(np.abs(J - ref) / bound))
    print(f"{tag}: cost err / bound {worst:.4f}")
    assert worst <= 1.0, f"{tag}: cost error / bound = {worst:.4f}"
    return worst


# ---- 1. the cost against the oracle on the device's own trajectory ---------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_cost_matches_the_oracle_on_the_devices_own_trajectory(name, sfx, integ):
    torch = _torch()
    B, T = 130, 5                           # two whole 64-lane tiles and a ragged one of two
    rbd, om = _rbd(name), _om(name)
    n = om.n
    c = _case(name, B, T, sfx, integ)
    cd = _cost_dev(name, B, T, sfx)
    args = {key: v for key, v in c.items() if key != "k"}
    kw = dict(dt=DT, integrator=integ, return_trajectory=True)
    tag = f"{name} {sfx} {integ}"
    worst = 0.0
    base = None
    variants = [("feedback", dict(k=c["k"], alpha=ALPHA), None), ("limits", dict(k=c["k"], alpha=ALPHA, u_min=-3.0, u_max=3.0), (-3.0, 3.0)),
                ("k=None", dict(k=None), None)]
    for what, v, lim in variants:
        J, q, qd, ua = rbd.rollout_cost(**args, cost=_qc(cd), **v, **kw)
        assert q.shape == qd.shape == ua.shape == (T, B, n) and J.dtype == q.dtype == c["u"].dtype and J.is_contiguous()
        worst = max(worst, check_cost(f"{tag} {what}", cd, J, q, qd, ua, sfx))
        check_controls(f"{tag} {what}", c, q, qd, ua, sfx, alpha=ALPHA, k=v["k"] is not None, lim=lim)
        check_teacher_forced(f"{tag} {what}", om, _np(c["q0"]), _np(c["qd0"]), _np(ua), _np(q), _np(qd), sfx, -9.81, integ)
        cl = rbd.rollout_closed_loop(**args, dt=DT, integrator=integ, **v)
        print(f"{tag} {what}: bit-identical to rollout_closed_loop: {all(torch.equal(a, b) for a, b in zip((q, qd, ua), cl))}")
        if what == "feedback":
            base = (J, q, qd, ua)
    fb = dict(k=c["k"], alpha=ALPHA)
    # a terminal state cost: the state terms of slice T - 1 alone; the trajectory is the same
    cf = _cost_dev(name, B, T, sfx, seed=1, final=True)
    J, q, qd, ua = rbd.rollout_cost(**args, cost=_qc(cf, final=True), **fb, **kw)
    assert all(torch.equal(a, b) for a, b in zip((q, qd, ua), base[1:]))
    worst = max(worst, check_cost(f"{tag} x_final_only", cf, J, q, qd, ua, sfx, final=True))
    # each cost array absent in turn (a missing weight drops its term, a missing target or c_u is zero), then all of them
    for drop in [(key,) for key in KEYS] + [KEYS]:
        J, q, qd, ua = rbd.rollout_cost(**args, cost=_qc(cd, drop=drop), **fb, **kw)
        assert all(torch.equal(a, b) for a, b in zip((q, qd, ua), base[1:])), drop
        worst = max(worst, check_cost(f"{tag} without {'+'.join(drop)}", cd, J, q, qd, ua, sfx, drop=drop))
        if len(drop) == 1 and drop[0] in ("w_q", "w_qd", "w_u", "c_u"):
            assert not torch.equal(J, base[0]), drop
    # a perturbation of the control per row
    du, = _dev(_dtype(sfx), np.random.default_rng(77 + n).normal(0, 0.1, (T, B, n)))
    J, q, qd, ua = rbd.rollout_cost(**args, cost=_qc(cd), du=du, **fb, **kw)
    worst = max(worst, check_cost(f"{tag} du", cd, J, q, qd, ua, sfx))
    cdu = {**c, "u": c["u"] + du}          # (the control check's bound covers the rounding of this sum)
    check_controls(f"{tag} du", cdu, q, qd, ua, sfx, alpha=ALPHA)
    check_teacher_forced(f"{tag} du", om, _np(c["q0"]), _np(c["qd0"]), _np(ua), _np(q), _np(qd), sfx, -9.81, integ)
    assert not torch.equal(ua, base[3])
    print(f"{tag}: WORST cost err / bound {worst:.4f}")


# ---- 2. the variants are bitwise consistent --------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_rows_steps_and_optional_outputs_do_not_change_the_cost(name, sfx, integ):
    torch = _torch()
    rbd = _rbd(name)
    T = 5
    c = _case(name, 65, T, sfx, integ, seed=2)
    cd = _cost_dev(name, 65, T, sfx, seed=2)
    full = rbd.rollout_cost(**c, dt=DT, cost=_qc(cd), alpha=ALPHA, integrator=integ, return_trajectory=True)
    for B in (1, 63, 64, 65):
        s = {key: (v[:, :B] if v.dim() >= 3 else v[:B]).contiguous() for key, v in c.items()}
        sc = _qc({key: v[:, :B].contiguous() for key, v in cd.items()})
        traj = rbd.rollout_cost(**s, dt=DT, cost=sc, alpha=ALPHA, integrator=integ, return_trajectory=True)
        last = rbd.rollout_cost(**s, dt=DT, cost=sc, alpha=ALPHA, integrator=integ, return_final=True)
        none = rbd.rollout_cost(**s, dt=DT, cost=sc, alpha=ALPHA, integrator=integ)
        assert torch.equal(traj[0], full[0][:B])                              # rows do not see each other
        for i in range(1, 4):
            assert traj[i].shape == (T, B, rbd.n) and torch.equal(traj[i], full[i][:, :B]), (B, i)
        assert isinstance(none, torch.Tensor) and none.shape == (B,)
        assert torch.equal(none, traj[0]) and torch.equal(last[0], traj[0])   # what is stored changes nothing
        assert len(last) == 3 and last[1].shape == (B, rbd.n) and torch.equal(last[1], traj[1][-1]) and torch.equal(last[2], traj[2][-1])
    # steps do not see the future: the first steps of the same problem (and with one step, its cost is the first step's)
    for Ts in (1, 3):
        st = {key: (v[:Ts].contiguous() if v.dim() >= 3 else v) for key, v in c.items()}
        cut = rbd.rollout_cost(**st, dt=DT, cost=_qc({key: v[:Ts].contiguous() for key, v in cd.items()}), alpha=ALPHA, integrator=integ,
                               return_trajectory=True)
        for i in range(1, 4):
            assert torch.equal(cut[i], full[i][:Ts]), (Ts, i)


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_a_shared_nominal_is_bit_identical_to_the_tiled_one(name, sfx, integ):
    """B_nom = 41 rows of nominal and cost, A = 4 step sizes: 164 rows whose tiles straddle the wrap of r % B_nom, against
    the unshared launch on everything written out four times; then B_nom = 1 with du against the tiled nominal."""
    torch = _torch()
    rbd = _rbd(name)
    Bn, A, T, n = 41, 4, 3, rbd.n
    c = _case(name, Bn, T, sfx, integ, seed=3)
    cd = _cost_dev(name, Bn, T, sfx, seed=3)
    alphas = [1.0, 0.5, 0.25, 0.0]
    args = {key: v for key, v in c.items() if key not in ("q0", "qd0")}
    kw = dict(dt=DT, integrator=integ, return_trajectory=True)
    shared = rbd.rollout_cost(c["q0_ref"], c["qd0_ref"], **args, cost=_qc(cd), alpha=alphas, **kw)       # the iLQR start
    assert shared[0].shape == (A, Bn) and shared[1].shape == (T, A, Bn, n)
    tile = lambda v: v.repeat(*([1, A] if v.dim() >= 3 else [A]), *[1] * (v.dim() - (2 if v.dim() >= 3 else 1)))   # noqa: E731
    tiled = {key: tile(v) for key, v in c.items()}
    tiled["q0"], tiled["qd0"] = tiled["q0_ref"], tiled["qd0_ref"]
    al = torch.tensor(alphas, device="cuda:0", dtype=_dtype(sfx)).repeat_interleave(Bn)
    flat = rbd.rollout_cost(**tiled, cost=_qc({key: tile(v) for key, v in cd.items()}), row_alpha=al, **kw)
    for s, f in zip(shared, flat):
        assert torch.equal(s.reshape(f.shape), f)
    only = rbd.rollout_cost(c["q0_ref"], c["qd0_ref"], **args, cost=_qc(cd), alpha=alphas, dt=DT, integrator=integ)
    assert torch.equal(only, shared[0])
    # one nominal, many samples (the MPPI case): open loop, B_nom = 1, du per row
    B = 130
    q0, qd0 = tile(c["q0"])[:B].contiguous(), tile(c["qd0"])[:B].contiguous()
    du, = _dev(_dtype(sfx), np.random.default_rng(5 + n).normal(0, 0.1, (T, B, n)))
    u1 = c["u"][:, :1].contiguous()
    c1 = {key: v[:, :1].contiguous() for key, v in cd.items()}
    one = rbd.rollout_cost(q0, qd0, u1, DT, _qc(c1), du=du, integrator=integ, return_trajectory=True)
    many = rbd.rollout_cost(q0, qd0, u1.repeat(1, B, 1), DT, _qc({key: v.repeat(1, B, 1) for key, v in c1.items()}), du=du, integrator=integ,
                            return_trajectory=True)
    for a, b in zip(one, many):
        assert torch.equal(a, b)
    assert torch.equal(one[3], u1 + du)                                      # no feed-forward term, no feedback: one addition


# ---- 3. open loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_open_loop_is_zero_feedback_and_no_cost_is_zero(name, sfx, integ):
    torch = _torch()
    rbd, om = _rbd(name), _om(name)
    B, T = 70, 5
    c = _case(name, B, T, sfx, integ, seed=4)
    cd = _cost_dev(name, B, T, sfx, seed=4)
    kw = dict(dt=DT, integrator=integ)
    opn = rbd.rollout_cost(c["q0"], c["qd0"], c["u"], cost=_qc(cd), k=c["k"], alpha=ALPHA, return_trajectory=True, **kw)
    zero = rbd.rollout_cost(c["q0"], c["qd0"], c["u"], cost=_qc(cd), k=c["k"], alpha=ALPHA, K=torch.zeros_like(c["K"]), q_ref=c["q_ref"],
                            qd_ref=c["qd_ref"], q0_ref=c["q0_ref"], qd0_ref=c["qd0_ref"], return_trajectory=True, **kw)
    for a, b in zip(opn, zero):
        assert torch.equal(a, b)
    from rbdreference_amd import QuadraticCost
    J, q, qd, ua = rbd.rollout_cost(c["q0"], c["qd0"], c["u"], cost=QuadraticCost(), return_trajectory=True, **kw)
    assert J.shape == (B,) and not bool(J.any()) and torch.equal(ua, c["u"])
    tag = f"{name} {sfx} {integ} open loop"
    check_teacher_forced(tag, om, _np(c["q0"]), _np(c["qd0"]), _np(c["u"]), _np(q), _np(qd), sfx, -9.81, integ)
    Jf, qT, qdT = rbd.rollout_cost(c["q0"], c["qd0"], c["u"], cost=QuadraticCost(), return_final=True, **kw)
    assert not bool(Jf.any()) and torch.equal(qT, q[-1]) and torch.equal(qdT, qd[-1])
    ro = rbd.rollout(c["q0"], c["qd0"], c["u"], DT, integrator=integ, trajectory=False)
    print(f"{tag}: final state bit-identical to rollout(trajectory=False): {torch.equal(qT, ro[0]) and torch.equal(qdT, ro[1])}")


# ---- 4. a NaN stays in its row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)                           # atlas: the lanes of a block share an LDS image
def test_a_nan_in_one_row_stays_in_that_rows_cost(name, sfx, integ):
    torch = _torch()
    rbd = _rbd(name)
    B, T, n = 40, 5, rbd.n
    c = _case(name, B, T, sfx, integ, seed=6)
    cd = _cost_dev(name, B, T, sfx, seed=6)
    keep = torch.tensor(np.setdiff1d(np.arange(B), [17]), device="cuda:0")
    kw = dict(dt=DT, alpha=ALPHA, u_min=-3.0, u_max=3.0, integrator=integ)
    bad_K, bad_q0, bad_w = c["K"].clone(), c["q0"].clone(), cd["w_q"].clone()
    bad_K[1, 17, n // 2, 3] = float("nan")
    bad_q0[17, n // 2] = float("nan")
    bad_w[T - 1, 17, n - 1] = float("nan")
    clean = rbd.rollout_cost(**c, cost=_qc(cd), **kw)
    assert not bool(torch.isnan(clean).any())
    for what, cc, ccd in (("K", {**c, "K": bad_K}, cd), ("q0", {**c, "q0": bad_q0}, cd), ("w_q", c, {**cd, "w_q": bad_w})):
        dirty = rbd.rollout_cost(**cc, cost=_qc(ccd), **kw)
        assert torch.equal(clean[keep], dirty[keep]), what
        assert bool(torch.isnan(dirty[17])), what


# ---- 5. memory contract through ctypes -------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_capi_writes_exactly_the_outputs_and_leaves_the_inputs_alone(name, sfx, integ):
    torch = _torch()
    rbd = _rbd(name)
    Bn, A, T, n, GUARD, MARK = 65, 2, 5, rbd.n, 4096, -777.25
    B = A * Bn
    dt = _dtype(sfx)
    ig = INTEGRATORS.index(integ)
    c = _case(name, Bn, T, sfx, integ, seed=5)
    cd = _cost_dev(name, Bn, T, sfx, seed=5)
    c["q0"], c["qd0"] = c["q0"].repeat(A, 1), c["qd0"].repeat(A, 1)
    al = torch.linspace(0.0, 1.0, B, device="cuda:0", dtype=dt)
    du = torch.randn((T, B, n), device="cuda:0", dtype=dt) * 0.1
    lo, hi = torch.full((n,), -3.0, device="cuda:0", dtype=dt), torch.full((n,), 3.0, device="cuda:0", dtype=dt)
    ins = list(c.values()) + list(cd.values()) + [al, du, lo, hi]
    keep = [x.clone() for x in ins]
    fn = rbd._lib.fn("rbd_rollout_cost", sfx)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    Js = []
    for traj, want_x, want_u in ((1, True, True), (0, True, False), (1, False, True), (0, False, False)):
        sizes = [B, (T if traj else 1) * B * n, (T if traj else 1) * B * n, T * B * n]
        bufs = [torch.full((GUARD + s + GUARD,), MARK, device="cuda:0", dtype=dt) for s in sizes]
        for b, s in zip(bufs, sizes):
            b[GUARD:GUARD + s] = float("nan")
        J, qo, qdo, uo = [b[GUARD:GUARD + s] for b, s in zip(bufs, sizes)]
        given = [True, want_x, want_x, want_u]
        rc = fn(p(c["q0"]), p(c["qd0"]), p(c["u"]), p(c["k"]), p(c["K"]), p(c["q0_ref"]), p(c["qd0_ref"]), p(c["q_ref"]), p(c["qd_ref"]),
                p(al), p(du), p(lo), p(hi), p(cd["q_target"]), p(cd["qd_target"]), p(cd["w_q"]), p(cd["w_qd"]), 0, p(cd["w_u"]), p(cd["c_u"]),
                DT, -9.81, ig, B, Bn, T, p(J), p(qo) if want_x else None, p(qdo) if want_x else None, traj, p(uo) if want_u else None, st)
        assert rc == 0, rbd._lib.lib.rbd_last_error()
        torch.cuda.synchronize()
        for b, s, g in zip(bufs, sizes, given):
            assert bool((b[:GUARD] == MARK).all()) and bool((b[GUARD + s:] == MARK).all()), "a guard band was overwritten"
            if g:
                assert not bool(torch.isnan(b[GUARD:GUARD + s]).any()), "an output element was not written"
            else:
                assert bool(torch.isnan(b[GUARD:GUARD + s]).all()), "an output that was not asked for was written"
        for x, k0 in zip(ins, keep):
            assert torch.equal(x, k0), "an input was modified"
        Js.append(J.clone())
    assert all(torch.equal(Js[0], x) for x in Js[1:])                         # what is stored does not change the cost
    # the API's line-search form is this call: rows a Bn + b carry alpha[a]
    al2 = torch.tensor([0.3, 0.9], device="cuda:0", dtype=dt)
    api = rbd.rollout_cost(c["q0"][:Bn], c["qd0"][:Bn], c["u"], DT, _qc(cd), K=c["K"], q_ref=c["q_ref"], qd_ref=c["qd_ref"], k=c["k"], alpha=al2,
                           du=du.view(T, A, Bn, n), q0_ref=c["q0_ref"], qd0_ref=c["qd0_ref"], u_min=lo, u_max=hi, integrator=integ)
    J = torch.empty((B,), device="cuda:0", dtype=dt)
    ar = al2.repeat_interleave(Bn).contiguous()
    rc = fn(p(c["q0"]), p(c["qd0"]), p(c["u"]), p(c["k"]), p(c["K"]), p(c["q0_ref"]), p(c["qd0_ref"]), p(c["q_ref"]), p(c["qd_ref"]),
            p(ar), p(du), p(lo), p(hi), p(cd["q_target"]), p(cd["qd_target"]), p(cd["w_q"]), p(cd["w_qd"]), 0, p(cd["w_u"]), p(cd["c_u"]),
            DT, -9.81, ig, B, Bn, T, p(J), None, None, 0, None, st)
    assert rc == 0 and api.shape == (A, Bn) and torch.equal(api.reshape(B), J)


# ---- 6. first use and stubs ------------------------------------------------------------------------------------------
def test_first_call_of_a_never_built_robot_goes_through_the_rollcost_family_library(monkeypatch):
    """The robot's full library is held back (its background build waits until the end of the test), as on a first use:
    the call is answered by the small `rollcost` family library (build.FAMILIES), built on demand."""
    import threading
    import torch
    from rbdreference_amd import QuadraticCost, RBDReference, _lib
    from rbdreference_amd.build import family_lib_path
    from rbdreference_amd.robot import random_tree
    release = threading.Event()

    def held_back_full_build(model):
        release.wait(300)
        raise RuntimeError("full library held back by the test")
    monkeypatch.setattr(_lib, "build_model", held_back_full_build)
    robot = random_tree([-1, 0, 1, 1], seed=4326, prismatic_every=3, name="rollcost_first_use_n4")
    try:
        rbd = RBDReference(robot, generic="never")
        B, T, n = 100, 4, 4
        mk = lambda *s: torch.rand(s, device="cuda:0", dtype=torch.float64)      # noqa: E731
        c = dict(q0=mk(B, n), qd0=mk(B, n), u=mk(T, B, n), q_ref=mk(T, B, n), qd_ref=mk(T, B, n), K=mk(T, B, n, 2 * n) - 0.5, k=mk(T, B, n),
                 q0_ref=mk(B, n), qd0_ref=mk(B, n))
        cd = dict(w_q=mk(T, B, n) + 1, w_qd=mk(T, B, n) + 1, q_target=mk(T, B, n), qd_target=mk(T, B, n), w_u=mk(T, B, n) + 1, c_u=mk(T, B, n))
        J, q, qd, ua = rbd.rollout_cost(**c, dt=DT, cost=QuadraticCost(**cd), alpha=ALPHA, return_trajectory=True)
        lib = rbd._lib._tls.lib
        assert rbd._lib._full is None and lib._name == family_lib_path(rbd.model, "rollcost", "f64")
        check_cost("first use", cd, J, q, qd, ua, "f64")
        check_controls("first use", c, q, qd, ua, "f64", alpha=ALPHA)
        check_teacher_forced("first use", orc.model_from_robot(robot), _np(c["q0"]), _np(c["qd0"]), _np(ua), _np(q), _np(qd), "f64", -9.81,
                             "semi_implicit")
    finally:
        release.set()


def test_floating_base_library_exports_an_unsupported_stub():
    from rbdreference_amd import QuadraticCost, RBDReference
    from rbdreference_amd._lib import RBD_ERR_UNSUPPORTED
    from rbdreference_amd.robot import floating_quadruped_like
    rbd = RBDReference(floating_quadruped_like(), build=False)
    fake = ctypes.c_void_p(4096)
    for sfx in ("f32", "f64"):
        fn = rbd._lib.fn("rbd_rollout_cost", sfx)
        rc = fn(*[fake] * 11, None, None, *[fake] * 4, 0, fake, fake, DT, -9.81, 0, 4, 2, 3, fake, fake, fake, 1, fake, None)
        assert rc == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in rbd._lib.lib.rbd_last_error()
    tr = np.zeros((3, 2, rbd.nv))
    with pytest.raises(NotImplementedError):
        rbd.rollout_cost(np.zeros((2, rbd.nv)), np.zeros((2, rbd.nv)), tr, DT, QuadraticCost())
    with pytest.raises(NotImplementedError):
        rbd.ilqr(np.zeros((2, rbd.nv)), np.zeros((2, rbd.nv)), tr, DT, QuadraticCost())


# ---- 7. ilqr ---------------------------------------------------------------------------------------------------------
def _problem(name, dtype):
    torch = _torch()
    from rbdreference_amd import QuadraticCost
    p = ilqr_problem(_om(name).n)
    d = {key: torch.tensor(v, device="cuda:0", dtype=dtype) for key, v in p.items()}
    cm = QuadraticCost(**{key: torch.tensor(v, device="cuda:0", dtype=dtype) for key, v in cost_arrays(p).items()})
    return p, d, cm


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_one_ilqr_iteration_is_its_three_launches_and_agrees_with_the_oracle(name, integ):
    torch = _torch()
    rbd, om = _rbd(name), _om(name)
    p, d, cm = _problem(name, torch.float64)
    T, B, n = p["u"].shape
    kw = dict(integrator=integ)
    r = rbd.ilqr(d["q0"], d["qd0"], d["u"], DT, cm, iters=1, **kw)
    assert r.u.shape == r.q.shape == r.qd.shape == (T, B, n) and r.cost.shape == (2, B) and r.alpha.shape == (1, B)
    assert r.dV.shape == (1, B, 2) and r.status.shape == (1, B) and r.status.dtype == torch.int32
    ref = ilqr(om, p, 1, integrator=integ)
    # by hand, from the same nominal
    J0, q, qd, u = rbd.rollout_cost(d["q0"], d["qd0"], d["u"], DT, cm, return_trajectory=True, **kw)
    assert torch.equal(J0, r.cost[0]) and torch.equal(u, d["u"])
    k, K, _, _, dV, status = rbd.rollout_lqr(d["q0"], d["qd0"], u, DT, q=q, qd=qd, **cm.derivatives(q, qd, u), **kw)
    assert torch.equal(dV, r.dV[0]) and torch.equal(status, r.status[0]) and int(status.abs().sum()) == 0
    al = torch.tensor(ALPHAS, device="cuda:0", dtype=torch.float64)
    Jc = rbd.rollout_cost(d["q0"], d["qd0"], u, DT, cm, K=K, q_ref=q, qd_ref=qd, k=k, alpha=al, **kw)
    assert Jc.shape == (len(ALPHAS), B)
    rel = np.abs(_np(Jc) - ref.candidates[0]) / np.abs(ref.candidates[0])
    print(f"{name} {integ}: candidates vs oracle, worst relative difference {rel.max():.2e}; J0 {np.abs(_np(J0) - ref.cost[0]).max():.2e}")
    assert rel.max() <= 1e-9
    J_best, idx, accept, ra = choose(_np(Jc), _np(J0), ALPHAS)                 # the device's own candidates decide
    assert np.array_equal(_np(r.alpha[0]), ra) and accept.all() and np.array_equal(ra, ref.alpha[0])
    qn, qdn, un = rbd.rollout_closed_loop(d["q0"], d["qd0"], u, q, qd, K, DT, k=k, row_alpha=r.alpha[0], **kw)
    assert torch.equal(r.u, un) and torch.equal(r.q, qn) and torch.equal(r.qd, qdn)
    chosen = Jc[torch.tensor(idx, device="cuda:0"), torch.arange(B, device="cuda:0")]
    assert torch.equal(r.cost[1], chosen)
    # the new nominal's cost, open loop: another chain of controls (u_applied read back), the same cost up to rounding
    J1, q1, qd1, u1 = rbd.rollout_cost(d["q0"], d["qd0"], r.u, DT, cm, return_trajectory=True, **kw)
    _, mag = cost_of_trajectory(cost_arrays(p), _np(q1), _np(qd1), _np(u1))
    err = np.abs(_np(J1) - _np(r.cost[1])) / (2 * (4 * n * T + 8) * EPS64 * mag)
    print(f"{name} {integ}: open-loop cost of the new nominal vs cost[1]: err / bound {err.max():.3f}; bit-identical: {torch.equal(J1, r.cost[1])}; "
          f"trajectory bit-identical: {torch.equal(q1, r.q) and torch.equal(qd1, r.qd)}")
    assert err.max() <= 1.0


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_ilqr_history_follows_the_oracle_on_the_arm(integ):
    torch = _torch()
    rbd, om = _rbd("iiwa_like"), _om("iiwa_like")
    p, d, cm = _problem("iiwa_like", torch.float64)
    r = rbd.ilqr(d["q0"], d["qd0"], d["u"], DT, cm, iters=2, integrator=integ)
    ref = ilqr(om, p, 2, integrator=integ)
    assert bool((r.alpha == 1.0).all()) and int(r.status.abs().sum()) == 0
    rel = np.abs(_np(r.cost) - ref.cost) / np.abs(ref.cost)
    print(f"iiwa_like {integ}: cost history vs oracle, worst relative difference {rel.max():.2e}\n{_np(r.cost)}")
    assert rel.max() <= 1e-8
    # numpy in -> numpy out, the same numbers
    from rbdreference_amd import QuadraticCost
    rn = rbd.ilqr(p["q0"], p["qd0"], p["u"], DT, QuadraticCost(**cost_arrays(p)), iters=2, integrator=integ)
    assert isinstance(rn.cost, np.ndarray) and np.array_equal(rn.cost, _np(r.cost)) and np.array_equal(rn.u, _np(r.u))


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_ilqr_never_raises_the_cost_and_a_rejected_row_keeps_its_nominal(name, integ):
    torch = _torch()
    rbd = _rbd(name)
    p, d, cm = _problem(name, torch.float64)
    r5 = rbd.ilqr(d["q0"], d["qd0"], d["u"], DT, cm, iters=5, integrator=integ)
    r6 = rbd.ilqr(d["q0"], d["qd0"], d["u"], DT, cm, iters=6, integrator=integ)
    assert torch.equal(r6.cost[:6], r5.cost) and torch.equal(r6.alpha[:5], r5.alpha)      # deterministic: r5 is r6's fifth nominal
    assert bool((r6.cost[1:] <= r6.cost[:-1]).all()) and int(r6.status.abs().sum()) == 0
    print(f"{name} {integ}: alpha history\n{_np(r6.alpha)}\ncost history\n{_np(r6.cost)}")
    al = set(float(a) for a in ALPHAS) | {0.0}
    assert set(_np(r6.alpha).ravel().tolist()) <= al
    rej = r6.alpha == 0
    assert torch.equal(r6.cost[1:][rej], r6.cost[:-1][rej])                                # a rejected row's cost stays
    assert bool((r6.cost[1:][~rej] < r6.cost[:-1][~rej]).all())                            # an accepted row's falls
    last = rej[5]
    for a, b in zip((r6.u, r6.q, r6.qd), (r5.u, r5.q, r5.qd)):
        assert torch.equal(a[:, last], b[:, last])                                         # ... and its nominal, bit for bit
    # a row that cannot be improved: no control cost and no state cost, so Quu = 0 and the backward pass fails in every step
    bad = {key: v.clone() for key, v in cost_arrays(d).items()}
    for key in ("w_u", "w_q", "w_qd"):
        bad[key][:, 1] = 0
    from rbdreference_amd import QuadraticCost
    rb = rbd.ilqr(d["q0"], d["qd0"], d["u"], DT, QuadraticCost(**bad), iters=6, integrator=integ)
    assert bool((rb.status[:, 1] > 0).all()) and bool((rb.alpha[:, 1] == 0).all())
    assert torch.equal(rb.u[:, 1], d["u"][:, 1]) and torch.equal(rb.cost[:, 1], rb.cost[:1, 1].expand(7))
    for i in (0, 2):
        assert torch.equal(rb.cost[:, i], r6.cost[:, i]) and torch.equal(rb.alpha[:, i], r6.alpha[:, i]) and torch.equal(rb.status[:, i], r6.status[:, i])
        assert torch.equal(rb.u[:, i], r6.u[:, i]) and torch.equal(rb.q[:, i], r6.q[:, i]) and torch.equal(rb.qd[:, i], r6.qd[:, i])


@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_ilqr_in_single_precision_is_finite_and_never_raises_the_cost(name):
    torch = _torch()
    rbd = _rbd(name)
    _, d32, cm32 = _problem(name, torch.float32)
    _, d64, cm64 = _problem(name, torch.float64)
    r32 = rbd.ilqr(d32["q0"], d32["qd0"], d32["u"], DT, cm32, iters=2)
    r64 = rbd.ilqr(d64["q0"], d64["qd0"], d64["u"], DT, cm64, iters=2)
    assert r32.cost.dtype == r32.u.dtype == torch.float32
    assert all(bool(torch.isfinite(x).all()) for x in (r32.u, r32.q, r32.qd, r32.cost, r32.alpha, r32.dV))
    assert bool((r32.cost[1:] <= r32.cost[:-1]).all())
    rel = (r32.cost.double() - r64.cost).abs() / r64.cost.abs()
    print(f"{name}: fp32 cost history vs fp64, relative difference per iteration {_np(rel.max(dim=1).values)}")
