"""mppi_update and mppi on the GPU: accuracy against the numpy restatement under a bound that holds for any
summation order, the cases that are exact bit for bit, the memory contract of the C-ABI, the driver against its launches
made by hand and against the driver oracle, and the first-use family library.

The kernels depend on the robot through ``n`` alone: 7 (the arm), 6 (a multiple of the 16-byte load width in fp64 only) and 30.
``P`` in {1, 3, 65} are the specified sizes; ``P = 4`` and ``P = 64`` are added because none of those makes ``P n`` a multiple
of four, the condition of the 16-byte loads in fp32."""
import ctypes

import numpy as np
import pytest

from mppi_oracle import bounds, mppi, mppi_du, mppi_update
from rbdreference_amd._lib import RBD_MPPI_CHUNK as C
from rollout_closed_loop_oracle import ilqr_problem
from rollout_cost_oracle import cost_arrays, rollout_cost
from rollout_oracle import INTEGRATORS
from test_gpu_rollout import DT, _np, _om, _rbd, _torch

pytestmark = pytest.mark.gpu

ROBOTS3 = ["iiwa_like", "random_prismatic_n6", "atlas_like"]
LAMS = (0.05, 1.0, 30.0)
LO, HI = -0.6, 0.6
S_LIST = [1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]
P_LIST = [1, 3, 4, 65]


def _npdt(sfx):
    return np.float32 if sfx == "f32" else np.float64


def _tdt(sfx):
    torch = _torch()
    return torch.float32 if sfx == "f32" else torch.float64


def _draw(n, S, P, T, sfx, seed=0, lam=None):
    """J uniform(5, 25), du normal(0, 0.3), u normal(0, 0.5), lam cycling through LAMS (or the one given), rounded to the run's
    precision; float64 images of those values."""
    rng = np.random.default_rng(1000 * seed + 17 * n + S + 7 * P)
    dt = _npdt(sfx)
    J, du, u = rng.uniform(5, 25, (S, P)), rng.normal(0, 0.3, (T, S, P, n)), rng.normal(0, 0.5, (T, P, n))
    lam = np.array([LAMS[(p + seed) % 3] for p in range(P)]) if lam is None else np.full(P, float(lam))
    return [a.astype(dt).astype(np.float64) for a in (J, du, u, lam)]


def _dev(sfx, *arrs):
    torch = _torch()
    return [torch.tensor(a, device="cuda:0", dtype=_tdt(sfx)) for a in arrs]


def _lims(limits):
    return dict(u_min=LO, u_max=HI) if limits else {}


# ---- 1. accuracy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS3)
def test_update_matches_the_oracle_within_the_order_free_bound(name, sfx, limits):
    """Measured worst err / bound on an MI355X over all robots, precisions and sizes: 0.232 for u, 0.070 for w, 0.030 for
    ess."""
    rbd = _rbd(name)
    n, T = rbd.n, 3
    worst = dict(u=0.0, w=0.0, ess=0.0)
    for S in S_LIST:
        for P in P_LIST:
            for lam in (LAMS if P == 1 else (None,)):
                J, du, u, lm = _draw(n, S, P, T, sfx, lam=lam)
                ref = mppi_update(J, du, u, lm, *((LO, HI) if limits else (None, None)))
                tJ, tdu, tu, tl = _dev(sfx, J, du, u, lm)
                r = rbd.mppi_update(tJ, tdu, tu, tl, return_weights=True, **_lims(limits))
                assert r.u.shape == (T, P, n) and r.w.shape == (S, P) and r.ess.shape == r.status.shape == (P,)
                assert r.u.dtype == r.w.dtype == r.ess.dtype == tJ.dtype and str(r.status.dtype) == "torch.int32"
                assert not _np(r.status).any() and not ref[6].any()
                b_u, b_w, b_ess = bounds(sfx, S, ref, u, du, limits)
                ratios = dict(u=(np.abs(_np(r.u) - ref[0]) / b_u).max(), w=(np.abs(_np(r.w) - ref[1]) / b_w).max(),
                              ess=(np.abs(_np(r.ess) - ref[5]) / b_ess).max())
                for key, v in ratios.items():
                    worst[key] = max(worst[key], float(v))
                    assert v <= 1.0, (name, sfx, limits, S, P, lam, key, float(v))
                if limits:
                    assert bool(((r.u >= LO) & (r.u <= HI)).all())
    print(f"{name} {sfx} limits={limits}: worst err / bound  u {worst['u']:.3f}  w {worst['w']:.3f}  ess {worst['ess']:.3f}")


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_deep_sample_axes_cross_the_group_and_trip_thresholds(sfx):
    """The chunks are added in groups of C, and the kernels walk the groups in trips: more than one group needs S > C^2,
    a second trip of the weights kernel S > 1024 C, a second trip of the combine kernel S > 16 C^2 (the same size here).
    On the arm, with limits: the bound of test 1, and a problem among three against itself alone, bit for bit."""
    rbd = _rbd("iiwa_like")
    n, T = rbd.n, 2
    for S, P in ((C * C + C + 3, 3), (1024 * C + C + 3, 1)):
        J, du, u, lm = _draw(n, S, P, T, sfx, seed=7)
        ref = mppi_update(J, du, u, lm, LO, HI)
        tJ, tdu, tu, tl = _dev(sfx, J, du, u, lm)
        r = rbd.mppi_update(tJ, tdu, tu, tl, return_weights=True, **_lims(True))
        b_u, b_w, b_ess = bounds(sfx, S, ref, u, du, True)
        ratios = ((np.abs(_np(r.u) - ref[0]) / b_u).max(), (np.abs(_np(r.w) - ref[1]) / b_w).max(), (np.abs(_np(r.ess) - ref[5]) / b_ess).max())
        print(f"iiwa_like {sfx} S={S} P={P}: err / bound  u {ratios[0]:.4f}  w {ratios[1]:.4f}  ess {ratios[2]:.4f}")
        assert max(ratios) <= 1.0 and not bool(r.status.any())
        if P > 1:
            a = rbd.mppi_update(tJ[:, 1:2].contiguous(), tdu[:, :, 1:2].contiguous(), tu[:, 1:2].contiguous(), tl[1:2], return_weights=True, **_lims(True))
            assert _same(a.u, r.u[:, 1:2]) and _same(a.w, r.w[:, 1:2]) and _same(a.ess, r.ess[1:2])


# ---- 2. exact cases --------------------------------------------------------------------------------------------------
def _clamp_t(torch, v, limits):
    if not limits:
        return v
    lo, hi = torch.full_like(v, LO), torch.full_like(v, HI)
    return torch.where(v < lo, lo, torch.where(v > hi, hi, v))


def _same(a, b):
    """Bit for bit, NaNs included."""
    torch = _torch()
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.numel() else True)


def _same_update(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS3)
def test_closed_forms_hold_bit_for_bit(name, sfx, limits):
    torch = _torch()
    rbd = _rbd(name)
    n, T = rbd.n, 3
    kw = _lims(limits)
    for S, P in ((1, 3), (5, 4), (2 * C + 3, 3), (2 * C + 3, 64)):
        J, du, u, lam = _dev(sfx, *_draw(n, S, P, T, sfx, seed=1))
        d = _clamp_t(torch, u[:, None] + du, limits) - u[:, None] if limits else du
        # lam -> 0 with a unique minimum: that sample's perturbation, as rollout_cost applied it (S = 1: the one there is)
        assert int((J == J.min(dim=0).values[None]).sum()) == P
        r = rbd.mppi_update(J, du, u, lam if S == 1 else 1e-30, return_weights=True, **kw)
        am = J.argmin(dim=0)
        pick = torch.stack([d[:, am[p], p] for p in range(P)], dim=1)
        assert _same(r.u, _clamp_t(torch, u + pick, limits))
        assert _same(r.w, (torch.arange(S, device="cuda:0")[:, None] == am[None]).to(J.dtype)) and _same(r.ess, torch.ones_like(r.ess))
        assert not bool(r.status.any())
        # du = 0: the nominal stays.  (With limits a component OUTSIDE them is pulled to its limit by S equal perturbations
        # lo - u or hi - u, whose weighted mean is not that number bit for bit: there the result lies in the limits and
        # within the accuracy bound of the clamped nominal; every component inside the limits is exact.)
        base = rbd.mppi_update(J, du, u, lam, return_weights=True, **kw)
        z = rbd.mppi_update(J, torch.zeros_like(du), u, lam, **kw)
        uc = _clamp_t(torch, u, limits)
        inside = uc == u
        assert _same(z.u[inside], u[inside]) and _same(z.ess, base.ess) and _same(z.status, base.status)
        if limits:
            assert bool(((z.u >= LO) & (z.u <= HI)).all()) and bool(((base.u >= LO) & (base.u <= HI)).all())
            zero = np.zeros(tuple(du.shape))
            ref = mppi_update(_np(J), zero, _np(u), _np(lam), LO, HI)
            assert np.array_equal(ref[0][_np(inside) > 0], _np(u)[_np(inside) > 0])
            assert (np.abs(_np(z.u) - ref[0]) <= bounds(sfx, S, ref, _np(u), zero, True)[0]).all()
            zi = rbd.mppi_update(J, torch.zeros_like(du), uc, lam, **kw)        # a nominal inside the limits, as every update returns it
            assert _same(zi.u, uc)
        else:
            assert bool(inside.all())
        # scaling J and lam by two changes nothing; neither does asking for the weights, or asking twice
        assert _same_update(rbd.mppi_update(2 * J, du, u, 2 * lam, return_weights=True, **kw), base)
        now = rbd.mppi_update(J, du, u, lam, **kw)
        assert now.w is None and _same(now.u, base.u) and _same(now.ess, base.ess) and _same(now.status, base.status)
        assert _same_update(rbd.mppi_update(J, du, u, lam, return_weights=True, **kw), base)
        # the first step alone
        one = rbd.mppi_update(J, du[:1].contiguous(), u[:1].contiguous(), lam, return_weights=True, **kw)
        assert _same(one.u, base.u[:1]) and _same(one.w, base.w) and _same(one.ess, base.ess)


@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS3)
def test_problems_do_not_see_each_other(name, sfx, limits):
    rbd = _rbd(name)
    n, T = rbd.n, 3
    kw = _lims(limits)
    for S in (5, 2 * C + 3):
        for P, alone in ((65, (0, 63, 64)), (64, (0, 63))):
            J, du, u, lam = _dev(sfx, *_draw(n, S, P, T, sfx, seed=2))
            full = rbd.mppi_update(J, du, u, lam, return_weights=True, **kw)
            for p in alone:
                r = rbd.mppi_update(J[:, p:p + 1].contiguous(), du[:, :, p:p + 1].contiguous(), u[:, p:p + 1].contiguous(), lam[p:p + 1],
                                    return_weights=True, **kw)
                assert _same(r.u, full.u[:, p:p + 1]) and _same(r.w, full.w[:, p:p + 1]) and _same(r.ess, full.ess[p:p + 1]), (S, P, p)


@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS3)
def test_nan_infinite_and_degenerate_inputs_follow_the_rules(name, sfx, limits):
    torch = _torch()
    rbd = _rbd(name)
    n, T, P = rbd.n, 3, 5
    kw = _lims(limits)
    nan, inf = float("nan"), float("inf")
    for S in (5, 2 * C + 3):
        J, du, u, lam = _dev(sfx, *_draw(n, S, P, T, sfx, seed=3))
        base = rbd.mppi_update(J, du, u, lam, return_weights=True, **kw)
        keep = [0, 1, 3, 4]
        less = rbd.mppi_update(J[:, keep].contiguous(), du[:, :, keep].contiguous(), u[:, keep].contiguous(), lam[keep].contiguous(),
                               return_weights=True, **kw)
        assert _same(less.u, base.u[:, keep]) and _same(less.w, base.w[:, keep])
        # a NaN cost is an infinite cost: the sample drops out
        Jn, Ji = J.clone(), J.clone()
        Jn[S // 2, 1], Ji[S // 2, 1] = nan, inf
        rn, ri = rbd.mppi_update(Jn, du, u, lam, return_weights=True, **kw), rbd.mppi_update(Ji, du, u, lam, return_weights=True, **kw)
        assert _same_update(rn, ri) and float(rn.w[S // 2, 1]) == 0.0 and not bool(rn.status.any())
        if S > 1:
            assert not bool(torch.isnan(rn.u).any()) and abs(float(rn.w[:, 1].sum()) - 1) < 1e-3

        def degenerate(r, want):
            st = [0, 0, want, 0, 0]
            assert r.status.tolist() == st
            assert _same(r.u[:, 2], _clamp_t(torch, u[:, 2], limits)) and not bool(r.w[:, 2].any()) and float(r.ess[2]) == 0.0
            assert _same(r.u[:, keep], less.u) and _same(r.w[:, keep], less.w) and _same(r.ess[keep], less.ess)

        # a column without a finite minimum: all NaN, all +inf, a -inf among finite costs
        for col in (torch.full((S,), nan), torch.full((S,), inf), None):
            Jb = J.clone()
            if col is None:
                Jb[S - 1, 2] = -inf
            else:
                Jb[:, 2] = col.to(J)
            degenerate(rbd.mppi_update(Jb, du, u, lam, return_weights=True, **kw), 1)
        # a temperature that is not finite and positive
        for bad in (0.0, -1.0, nan, inf):
            lb = lam.clone()
            lb[2] = bad
            degenerate(rbd.mppi_update(J, du, u, lb, return_weights=True, **kw), 2)
        # a NaN in du shows in its own (t, p, j) and nowhere else
        t, s, p, j = 1, S - 1, 3, n - 1
        dn = du.clone()
        dn[t, s, p, j] = nan
        rn = rbd.mppi_update(J, dn, u, lam, return_weights=True, **kw)
        mask = torch.zeros_like(u, dtype=torch.bool)
        mask[t, p, j] = True
        assert bool(torch.isnan(rn.u[mask]).all()) and _same(rn.u[~mask], base.u[~mask]) and _same(rn.w, base.w) and _same(rn.ess, base.ess)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS3)
def test_capi_writes_exactly_the_outputs_and_leaves_the_inputs_alone(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    n, T, GUARD, MARK = rbd.n, 3, 4096, -777.25
    dt = _tdt(sfx)
    esz = 4 if sfx == "f32" else 8
    lib = rbd._lib.lib
    fn = getattr(lib, f"rbd_mppi_update_{sfx}")
    st = torch.cuda.current_stream().cuda_stream
    lo, hi = torch.full((n,), LO, device="cuda:0", dtype=dt), torch.full((n,), HI, device="cuda:0", dtype=dt)
    for S, P in ((5, 65), (2 * C + 3, 3), (2 * C + 3, 64)):
        J, du, u, lam = _dev(sfx, *_draw(n, S, P, T, sfx, seed=4))
        ins = [J, du, u, lam, lo, hi]
        keep = [x.clone() for x in ins]
        api = rbd.mppi_update(J, du, u, lam, u_min=lo, u_max=hi, return_weights=True)
        wsb = int(lib.rbd_mppi_update_workspace_bytes(S, P, T, esz))
        assert wsb > 0 and wsb % 16 == 0
        for want_w, want_ess in ((True, True), (False, True), (True, False), (False, False)):
            sizes = [T * P * n, S * P, P]
            bufs = [torch.full((GUARD + s + GUARD,), MARK, device="cuda:0", dtype=dt) for s in sizes]
            for b, s in zip(bufs, sizes):
                b[GUARD:GUARD + s] = float("nan")
            sbuf = torch.full((GUARD + P + GUARD,), -777, device="cuda:0", dtype=torch.int32)
            sbuf[GUARD:GUARD + P] = 12345
            ws = torch.full((GUARD + wsb + GUARD,), 0x5A, device="cuda:0", dtype=torch.uint8)
            uo, w, ess = [b[GUARD:GUARD + s] for b, s in zip(bufs, sizes)]
            rc = fn(J.data_ptr(), du.data_ptr(), u.data_ptr(), lam.data_ptr(), lo.data_ptr(), hi.data_ptr(), S, P, T, uo.data_ptr(),
                    w.data_ptr() if want_w else None, ess.data_ptr() if want_ess else None, sbuf[GUARD:].data_ptr(),
                    ws[GUARD:].data_ptr(), wsb, st)
            assert rc == 0, lib.rbd_last_error()
            torch.cuda.synchronize()
            for b, s, g in zip(bufs, sizes, (True, want_w, want_ess)):
                assert bool((b[:GUARD] == MARK).all()) and bool((b[GUARD + s:] == MARK).all()), "a guard band was overwritten"
                if g:
                    assert not bool(torch.isnan(b[GUARD:GUARD + s]).any()), "an output element was not written"
                else:
                    assert bool(torch.isnan(b[GUARD:GUARD + s]).all()), "an output that was not asked for was written"
            assert bool((sbuf[:GUARD] == -777).all()) and bool((sbuf[GUARD + P:] == -777).all()) and not bool(sbuf[GUARD:GUARD + P].any())
            assert bool((ws[:GUARD] == 0x5A).all()) and bool((ws[GUARD + wsb:] == 0x5A).all()), "the workspace's guard band was overwritten"
            for x, k0 in zip(ins, keep):
                assert torch.equal(x, k0), "an input was modified"
            assert _same(uo.view(T, P, n), api.u) and (not want_w or _same(w.view(S, P), api.w)) and (not want_ess or _same(ess, api.ess))
        # a workspace one byte short is refused before anything is launched
        from rbdreference_amd._lib import RBD_ERR_WORKSPACE
        out = torch.full((T * P * n,), float("nan"), device="cuda:0", dtype=dt)
        sb = torch.zeros((P,), device="cuda:0", dtype=torch.int32)
        ws = torch.empty((wsb,), device="cuda:0", dtype=torch.uint8)
        assert fn(J.data_ptr(), du.data_ptr(), u.data_ptr(), lam.data_ptr(), None, None, S, P, T, out.data_ptr(), None, None, sb.data_ptr(),
                  ws.data_ptr(), wsb - 1, st) == RBD_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())


def test_numpy_inputs_return_float64_numpy():
    rbd = _rbd("iiwa_like")
    J, du, u, lam = _draw(7, 9, 3, 2, "f64", seed=5)
    r = rbd.mppi_update(J, du, u, lam, u_min=LO, u_max=HI, return_weights=True)
    t = rbd.mppi_update(*_dev("f64", J, du, u, lam), u_min=LO, u_max=HI, return_weights=True)
    for a, b in zip(r, t):
        assert isinstance(a, np.ndarray) and np.array_equal(a, b.cpu().numpy())
    assert r.u.dtype == r.w.dtype == r.ess.dtype == np.float64 and r.status.dtype == np.int32
    assert rbd.mppi_update(J, du, u, 2.0).w is None


# ---- 3. the driver ---------------------------------------------------------------------------------------------------
_DRIVER = {}


def _driver_case(name, integ):
    """The problem, its noise, lam = the oracle's per-problem standard deviation of the first iteration's costs, and the
    driver oracle's two iterations -- computed once per (robot, integrator)."""
    if (name, integ) not in _DRIVER:
        om = _om(name)
        p = ilqr_problem(om.n)
        T, P, n = p["u"].shape
        S, iters = 65, 2
        noise = np.random.default_rng(100 + n).standard_normal((iters, T, S, P, n))
        c = cost_arrays(p)
        du0 = mppi_du(noise[0], 0.5)
        J0 = rollout_cost(om, np.tile(p["q0"], (S, 1)), np.tile(p["qd0"], (S, 1)), p["u"], DT, c, du=du0.reshape(T, S * P, n),
                          integrator=integ)[0].reshape(S, P)
        lam = J0.std(axis=0)
        ref = mppi(om, p["q0"], p["qd0"], p["u"], DT, c, noise, sigma=0.5, lam=lam, integrator=integ)
        assert np.array_equal(ref.J[0], J0)
        _DRIVER[(name, integ)] = (p, c, noise, lam, ref)
    return _DRIVER[(name, integ)]


def _driver_dev(p, c, noise, lam, dtype):
    torch = _torch()
    from rbdreference_amd import QuadraticCost
    t = lambda a: torch.tensor(a, device="cuda:0", dtype=dtype)      # noqa: E731
    return t(p["q0"]), t(p["qd0"]), t(p["u"]), QuadraticCost(**{k: t(v) for k, v in c.items()}), t(noise), t(lam)


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_the_driver_is_its_launches_and_agrees_with_the_oracle(name, integ):
    torch = _torch()
    rbd = _rbd(name)
    p, c, noise, lam, ref = _driver_case(name, integ)
    T, P, n = p["u"].shape
    S = noise.shape[2]
    q0, qd0, u, cm, tn, tl = _driver_dev(p, c, noise, lam, torch.float64)
    kw = dict(integrator=integ)
    r = rbd.mppi(q0, qd0, u, DT, cm, iters=2, sigma=0.5, lam=tl, noise=tn, **kw)
    assert r.u.shape == r.q.shape == r.qd.shape == (T, P, n) and r.cost.shape == (3, P) and r.ess.shape == r.status.shape == (2, P)
    assert r.status.dtype == torch.int32 and not bool(r.status.any())
    print(f"{name} {integ}: ess per iteration {_np(r.ess).round(2).tolist()} of S = {S}; oracle {ref.ess.round(2).tolist()}")
    assert float(r.ess.min()) > 2.0 and (ref.ess > 2.0).all()
    # by hand, from the same nominal
    assert _same(r.cost[0], rbd.rollout_cost(q0, qd0, u, DT, cm, **kw))
    du = 0.5 * tn[0]
    du[:, 0] = 0
    J = rbd.rollout_cost(q0.repeat(S, 1), qd0.repeat(S, 1), u, DT, cm, du=du.view(T, S * P, n), **kw).view(S, P)
    hand = rbd.mppi_update(J, du, u, tl)
    r1 = rbd.mppi(q0, qd0, u, DT, cm, iters=1, sigma=0.5, lam=tl, noise=tn[:1], **kw)
    assert _same(r1.u, hand.u) and _same(r1.ess[0], hand.ess) and _same(r1.status[0], hand.status)
    assert _same(r.ess[0], hand.ess) and _same(r.status[0], hand.status) and _same(r.cost[0], J[0]) and _same(r.cost[0], r1.cost[0])
    assert _same(r.cost[1], r1.cost[1])                                       # the nominal entering iteration 2 is iteration 1's result
    Jf, q, qd, _ = rbd.rollout_cost(q0, qd0, r.u, DT, cm, return_trajectory=True, **kw)
    assert _same(r.q, q) and _same(r.qd, qd) and _same(r.cost[2], Jf)
    r0 = rbd.mppi(q0, qd0, u, DT, cm, iters=0, **kw)
    J0, qs, qds, _ = rbd.rollout_cost(q0, qd0, u, DT, cm, return_trajectory=True, **kw)
    assert _same(r0.u, u) and _same(r0.q, qs) and _same(r0.qd, qds) and _same(r0.cost, J0[None]) and r0.ess.shape == r0.status.shape == (0, P)
    # against the driver oracle at the first iteration
    relJ = np.abs(_np(J) - ref.J[0]) / np.abs(ref.J[0])
    b_u, _, _ = bounds("f64", S, ref.update[0], p["u"], ref.du[0], False)
    _, w, _, d, D, _, _ = ref.update[0]
    shift = 2 * (np.abs(_np(J) - ref.J[0]).max(axis=0) / lam)[None, :, None] * (np.einsum("sp,tspj->tpj", w, np.abs(d)) + np.abs(D))
    ratio = np.abs(_np(r1.u) - ref.update[0][0]) / (b_u + shift)
    print(f"{name} {integ}: J vs oracle, worst relative difference {relJ.max():.2e}; new nominal err / bound {ratio.max():.3f}")
    assert relJ.max() <= 1e-9 and ratio.max() <= 1.0


@pytest.mark.parametrize("name", ["iiwa_like", "random_tree_n9"])
def test_the_driver_in_single_precision_is_finite_and_seeded_runs_repeat(name):
    torch = _torch()
    rbd = _rbd(name)
    p, c, noise, lam, ref = _driver_case(name, "semi_implicit")
    T, P, n = p["u"].shape
    q0, qd0, u, cm, tn, tl = _driver_dev(p, c, noise, lam, torch.float32)
    r = rbd.mppi(q0, qd0, u, DT, cm, iters=2, sigma=0.5, lam=tl, noise=tn)
    assert r.u.dtype == r.cost.dtype == torch.float32 and bool(torch.isfinite(r.u).all()) and bool(torch.isfinite(r.cost).all())
    print(f"{name}: fp32 vs the fp64 oracle, cost {np.abs(_np(r.cost) - ref.cost).max() / np.abs(ref.cost).max():.2e} (relative), "
          f"u {np.abs(_np(r.u) - ref.u).max():.2e} (absolute)")
    runs = []
    for _ in range(2):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(1234)
        runs.append(rbd.mppi(q0, qd0, u, DT, cm, iters=2, samples=33, sigma=np.full(n, 0.3), lam=float(lam.mean()), generator=g, u_min=-4.0, u_max=4.0))
    assert all(_same(a, b) for a, b in zip(*runs)) and bool(torch.isfinite(runs[0].u).all())
    assert bool(((runs[0].u >= -4.0) & (runs[0].u <= 4.0)).all()) and runs[0].ess.shape == (2, P)
    # numpy in, float64 numpy out
    from rbdreference_amd import QuadraticCost
    rn = rbd.mppi(p["q0"], p["qd0"], p["u"], DT, QuadraticCost(**c), iters=1, sigma=0.5, lam=lam, noise=noise[:1])
    assert all(isinstance(x, np.ndarray) for x in rn) and rn.u.dtype == np.float64 and rn.status.dtype == np.int32


# ---- 4. first use and stubs ------------------------------------------------------------------------------------------
def test_first_call_of_a_never_built_robot_goes_through_the_mppi_family_library(monkeypatch):
    """The robot's full library is held back (its background build waits until the end of the test), as on a first use:
    the call is answered by the small `mppi` family library (build.FAMILIES), built on demand."""
    import threading
    import torch
    from rbdreference_amd import RBDReference, _lib
    from rbdreference_amd.build import family_lib_path
    from rbdreference_amd.robot import random_tree
    release = threading.Event()

    def held_back_full_build(model):
        release.wait(300)
        raise RuntimeError("full library held back by the test")
    monkeypatch.setattr(_lib, "build_model", held_back_full_build)
    robot = random_tree([-1, 0, 1, 1], seed=4327, prismatic_every=3, name="mppi_first_use_n4")
    try:
        rbd = RBDReference(robot, generic="never")
        S, P, T, n = C + 5, 3, 2, 4
        J, du, u, lam = _draw(n, S, P, T, "f64", seed=6)
        r = rbd.mppi_update(*_dev("f64", J, du, u, lam), u_min=LO, u_max=HI, return_weights=True)
        lib = rbd._lib._tls.lib
        assert rbd._lib._full is None and lib._name == family_lib_path(rbd.model, "mppi", "f64")
        ref = mppi_update(J, du, u, lam, LO, HI)
        b_u, b_w, b_ess = bounds("f64", S, ref, u, du, True)
        assert (np.abs(_np(r.u) - ref[0]) <= b_u).all() and (np.abs(_np(r.w) - ref[1]) <= b_w).all() and (np.abs(_np(r.ess) - ref[5]) <= b_ess).all()
    finally:
        release.set()


def test_floating_base_library_exports_an_unsupported_stub():
    from rbdreference_amd import RBDReference
    from rbdreference_amd._lib import RBD_ERR_UNSUPPORTED
    from rbdreference_amd.robot import floating_quadruped_like
    rbd = RBDReference(floating_quadruped_like(), build=False)
    fake = ctypes.c_void_p(4096)
    assert rbd._lib.lib.rbd_mppi_update_workspace_bytes(8, 2, 3, 4) == 0
    for sfx in ("f32", "f64"):
        fn = rbd._lib.fn("rbd_mppi_update", sfx)
        assert fn(fake, fake, fake, fake, None, None, 8, 2, 3, fake, fake, fake, fake, fake, 1 << 20, None) == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in rbd._lib.lib.rbd_last_error()
    with pytest.raises(NotImplementedError):
        rbd.mppi_update(np.zeros((8, 2)), np.zeros((3, 8, 2, rbd.nv)), np.zeros((3, 2, rbd.nv)), 1.0)
