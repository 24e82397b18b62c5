"""RBDReference.rollout_lqr / rollout_riccati on the GPU (rbd_rollout_riccati, rbd_rollout_lqr; csrc/rbd_rollout_lqr.h).

Everything is compared with tests/rollout_lqr_oracle.py in fp64 on the exact device values, per row and per output
(k, K, lam, P, dV), in the max norm relative to that output's max norm over the row.

  scan alone    random dc_du, Minv (entries uniform(-1, 1) / n, Minv symmetrised), g and grad_u standard normal,
                hess_q, hess_qd uniform(5, 15), hess_u uniform(1, 2), dt = 0.1, reg = 0.  fp64: 1e-9 (TOL64).  fp32:
                max(8 e32, T 2n 2^-24), e32 the error of the oracle itself run in float32 on the same inputs (for the case and
                output): summation order, FMA contraction and another elimination order each obey the same dot-product
                bound.  test_rollout_lqr_host.py asserts e32 < 1e-5 and that the integrators differ on K by > 1e-2.
  composite     teacher-forced: rollout on the device, rollout_lqr on the stored trajectory; fp64 against the evaluating
                oracle at the device's stored states within T 1e-9; both precisions against rollout_riccati fed with aba,
                rnea_grad and minv called by hand on the same flat rows.  dt = 0.01 here, the step of the rollout tests:
                at dt = 0.1 these random torques drive the fixture robots far off within five steps (Minv reaches 2e3,
                P 1e81 on the 30-body robot in the fp64 oracle), and no precision factors that Quu."""
import ctypes

import numpy as np
import pytest

from conftest import all_golden_names, make_robot
from oracle import rbd_oracle as orc
from rollout_lqr_oracle import riccati, rollout_lqr as oracle_lqr
from rollout_oracle import INTEGRATORS, rollout as oracle_rollout

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
TOL64 = 1e-9                # as test_gpu_parity's fp64 aba / minv checks
DT = 0.1
DTC = 0.01                  # the composites: the rollout tests' step (see the module docstring)
B0 = 41                     # prime: the last block is ragged for every block of 2..40 rows (blocks hold 1, 1, 3, 4 rows here)
ROBOTS = all_golden_names()                 # the nine fixed-base fixture robots
SCAN_ROBOTS = ["iiwa_like", "random_tree_n9", "random_twochains_n18", "atlas_like"]     # n = 7, 9, 18, 30
NAMES = ("k", "K", "lam", "P", "dV")

_RBD, _OM = {}, {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


def _rbd(name):
    if name not in _RBD:
        from rbdreference_amd import RBDReference
        _RBD[name] = RBDReference(make_robot(name), build=False)   # prebuilt by __graft_entry__.build()
    return _RBD[name]


def _om(name):
    if name not in _OM:
        _OM[name] = orc.model_from_robot(make_robot(name))
    return _OM[name]


def _dtype(sfx):
    torch = _torch()
    return torch.float32 if sfx == "f32" else torch.float64


def _dt(sfx):
    return float(np.float32(DT)) if sfx == "f32" else DT


def _dev(dtype, *arrs):
    torch = _torch()
    return [None if a is None else torch.tensor(a, device="cuda:0", dtype=dtype) for a in arrs]


def _np(t):
    return None if t is None else t.double().cpu().numpy()


def _scan_data(n, B, T, seed):
    """test_gpu_rollout_grad._scan_data, then the cost model from the same generator."""
    rng = np.random.default_rng(seed)
    dc = rng.uniform(-1, 1, (T, B, n, 2 * n)) / n
    M = rng.uniform(-1, 1, (T, B, n, n)) / n
    M = 0.5 * (M + np.swapaxes(M, -1, -2))
    c = dict(gq=rng.standard_normal((T, B, n)), gqd=rng.standard_normal((T, B, n)), hq=rng.uniform(5, 15, (T, B, n)),
             hqd=rng.uniform(5, 15, (T, B, n)), gu=rng.standard_normal((T, B, n)), hu=rng.uniform(1, 2, (T, B, n)))
    return dc, M, c


def _rows(name, x):
    """An output as [B, everything of the row] (k and K are time-major)."""
    x = np.asarray(x, np.float64)
    if name in ("k", "K"):
        x = np.moveaxis(x, 0, 1)
    return x.reshape(x.shape[0], -1)


def _errs(got, ref):
    """{output: worst row's max|got - ref| / max|ref|}."""
    out = {}
    for name, a, r in zip(NAMES, got, ref):
        a, r = _rows(name, a), _rows(name, r)
        out[name] = float((np.abs(a - r).max(1) / np.abs(r).max(1)).max())
    return out


def _api_costs(t, final):
    """The dict of device tensors as rollout_riccati / rollout_lqr keywords; final: the state costs' last slice only."""
    f = (lambda x: x[-1].contiguous()) if final else (lambda x: x)
    return dict(grad_q=f(t["gq"]), grad_qd=f(t["gqd"]), hess_q=f(t["hq"]), hess_qd=f(t["hqd"]), grad_u=t["gu"], hess_u=t["hu"])


def _oracle_costs(c, final):
    f = (lambda x: x[-1]) if final else (lambda x: x)
    return dict(gq=f(c["gq"]), gqd=f(c["gqd"]), hq=f(c["hq"]), hqd=f(c["hqd"]), gu=c["gu"], hu=c["hu"])


# ---- 1. the scan alone, random data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("name", SCAN_ROBOTS)
def test_scan_matches_the_oracle(name, T, sfx, integ, final):
    rbd = _rbd(name)
    n, B = rbd.n, B0
    dc, M, c = _scan_data(n, B, T, seed=100 * n + T)
    dtype = _dtype(sfx)
    dc_t, M_t = _dev(dtype, dc, M)
    t = dict(zip(c, _dev(dtype, *c.values())))
    got = rbd.rollout_riccati(dc_t, M_t, DT, reg=0.0, integrator=integ, **_api_costs(t, final))
    assert [tuple(x.shape) for x in got] == [(T, B, n), (T, B, n, 2 * n), (B, 2 * n), (B, 2 * n, 2 * n), (B, 2), (B,)]
    assert got[5].dtype == _torch().int32 and not bool(got[5].any())
    dev = {a: _np(v) for a, v in t.items()}                    # the exact device values
    ref = riccati(_np(dc_t), _np(M_t), _dt(sfx), integrator=integ, **_oracle_costs(dev, final))
    err = _errs([_np(x) for x in got[:5]], ref)
    if sfx == "f64":
        bound = {a: TOL64 for a in NAMES}
    else:
        f32 = lambda x: np.asarray(x, np.float32)
        low = riccati(f32(_np(dc_t)), f32(_np(M_t)), np.float32(DT), integrator=integ, dtype=np.float32,
                      **{a: f32(v) for a, v in _oracle_costs(dev, final).items()})
        e32 = _errs(low[:5], ref)
        bound = {a: max(8 * e32[a], T * 2 * n * EPS32) for a in NAMES}
    worst = {a: err[a] / bound[a] for a in NAMES}
    print(f"{name} T={T} {sfx} {integ} final={final}: err / bound " + " ".join(f"{a} {w:.2e}" for a, w in worst.items()))
    assert max(worst.values()) <= 1.0, (err, bound)
    P = got[3]
    assert _torch().equal(P, P.transpose(1, 2))              # symmetrised bit for bit


def test_the_bound_tells_the_integrators_apart():
    rbd = _rbd("iiwa_like")
    n, B, T = rbd.n, B0, 5
    dc, M, c = _scan_data(n, B, T, seed=3)
    torch = _torch()
    dc_t, M_t = _dev(torch.float64, dc, M)
    t = dict(zip(c, _dev(torch.float64, *c.values())))
    Ka, Kb = (_np(rbd.rollout_riccati(dc_t, M_t, DT, integrator=i, **_api_costs(t, False))[1]) for i in INTEGRATORS)
    sep = float((np.abs(Ka - Kb).max((0, 2, 3)) / np.abs(Ka).max((0, 2, 3))).min())
    print(f"integrators apart on K by {sep:.2e}")
    assert sep >= 1e-2


# ---- 2. a split scan is bit-identical -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_split_scan_is_bit_identical(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    n, B, T = rbd.n, B0, 5
    dc, M, c = _scan_data(n, B, T, seed=7 * n)
    dtype = _dtype(sfx)
    dc_t, M_t = _dev(dtype, dc, M)
    t = dict(zip(c, _dev(dtype, *c.values())))
    for final in (False, True):
        full = rbd.rollout_riccati(dc_t, M_t, DT, **_api_costs(t, final))
        for s in range(1, T):
            hi_c = _api_costs({a: v[s:].contiguous() for a, v in t.items()}, final)
            lo_c = {a: v[:s].contiguous() for a, v in _api_costs(t, False).items()}
            if final:                                           # the state costs belong to the call that holds the last step
                for a in ("grad_q", "grad_qd", "hess_q", "hess_qd"):
                    lo_c[a] = None
            hi = rbd.rollout_riccati(dc_t[s:].contiguous(), M_t[s:].contiguous(), DT, **hi_c)
            lam, P, dV, st = (x.clone() for x in hi[2:])
            lo = rbd.rollout_riccati(dc_t[:s].contiguous(), M_t[:s].contiguous(), DT, lam=lam, P=P, dV=dV, status=st, **lo_c)
            assert lo[2].data_ptr() == lam.data_ptr() and lo[3].data_ptr() == P.data_ptr()        # updated in place
            assert torch.equal(torch.cat([lo[0], hi[0]]), full[0]) and torch.equal(torch.cat([lo[1], hi[1]]), full[1]), s
            for a, x, y in zip(NAMES[2:] + ("status",), lo[2:], full[2:]):
                assert torch.equal(x, y), (a, s, final)


# ---- 3. a factorisation that fails -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_failed_factorisation_is_contained_in_its_row(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    n, B, T, bad = rbd.n, B0, 5, 17
    dc, M, c = _scan_data(n, B, T, seed=11 * n)
    for a in ("hq", "hqd", "hu"):
        c[a][:, bad] = 0.0                                      # Quu = 0 in that row: no control cost, P stays zero
    # (the row keeps its grad_q, grad_qd and grad_u on purpose: Quu does not see them, and lam = Qx is still exercised)
    dtype = _dtype(sfx)
    dc_t, M_t = _dev(dtype, dc, M)
    t = dict(zip(c, _dev(dtype, *c.values())))
    got = rbd.rollout_riccati(dc_t, M_t, DT, reg=0.0, **_api_costs(t, False))
    st = got[5].cpu().numpy()
    assert st[bad] == T and not np.delete(st, bad).any()
    assert not bool(got[0][:, bad].any()) and not bool(got[1][:, bad].any())
    assert all(bool(torch.isfinite(x).all()) for x in got[:5])
    assert not bool(got[4][bad].any()) and not bool(got[3][bad].any())
    keep = [i for i in range(B) if i != bad]
    sub = rbd.rollout_riccati(dc_t[:, keep].contiguous(), M_t[:, keep].contiguous(), DT, reg=0.0,
                              **{a: v[:, keep].contiguous() for a, v in _api_costs(t, False).items()})
    for i, (x, y) in enumerate(zip(got, sub)):
        assert torch.equal(x[:, keep] if i < 2 else x[keep], y), i
    reg = rbd.rollout_riccati(dc_t, M_t, DT, reg=1.0, **_api_costs(t, False))
    assert not bool(reg[5].any()) and bool(reg[0][:, bad].any())      # (K stays zero there: P is zero)


# ---- 4. the composite, teacher-forced -------------------------------------------------------------------------------------
def _inputs(name, B, T, seed=1):
    n = _om(name).n
    rng = np.random.default_rng(1000 * seed + n)
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
    c = dict(gq=rng.standard_normal((T, B, n)), gqd=rng.standard_normal((T, B, n)), hq=rng.uniform(5, 15, (T, B, n)),
             hqd=rng.uniform(5, 15, (T, B, n)), gu=rng.standard_normal((T, B, n)), hu=rng.uniform(1, 2, (T, B, n)))
    return q0, qd0, u, c


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_composite_matches_the_oracle_and_the_hand_made_linearisation(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    n, B, T = rbd.n, B0, 5
    q0, qd0, u, c = _inputs(name, B, T)
    dtype = _dtype(sfx)
    q0_t, qd0_t, u_t = _dev(dtype, q0, qd0, u)
    t = dict(zip(c, _dev(dtype, *c.values())))
    q_t, qd_t = rbd.rollout(q0_t, qd0_t, u_t, DTC)
    got = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q_t, qd=qd_t, **_api_costs(t, False))
    assert not bool(got[5].any())
    # the same flat rows by hand: steps 1 .. T-1 in one call, step 0 in another
    flat = lambda x: x.reshape(-1, n)
    qdd = rbd.aba(flat(q_t[:T - 1]), flat(qd_t[:T - 1]), flat(u_t[1:]))
    dc_hi = rbd.rnea_grad(flat(q_t[:T - 1]), flat(qd_t[:T - 1]), qdd).reshape(T - 1, B, n, 2 * n)
    Mi_hi = rbd.minv(flat(q_t[:T - 1])).reshape(T - 1, B, n, n)
    dc_0 = rbd.rnea_grad(q0_t, qd0_t, rbd.aba(q0_t, qd0_t, u_t[0]))[None]
    Mi_0 = rbd.minv(q0_t)[None]
    hand = rbd.rollout_riccati(torch.cat([dc_0, dc_hi]), torch.cat([Mi_0, Mi_hi]), DTC, **_api_costs(t, False))
    same = all(torch.equal(x, y) for x, y in zip(got, hand))
    err = _errs([_np(x) for x in got[:5]], [_np(x) for x in hand[:5]])
    tol = TOL64 if sfx == "f64" else T * 2 * n * EPS32
    print(f"{name} {sfx}: composite vs hand-made linearisation bit-identical: {same}; worst {max(err.values()):.2e}")
    assert max(err.values()) <= tol, err
    if sfx == "f64":
        ref = oracle_lqr(_om(name), _np(q0_t), _np(qd0_t), _np(u_t), DTC, _np(q_t), _np(qd_t),
                         **_oracle_costs({a: _np(v) for a, v in t.items()}, False))
        err = _errs([_np(x) for x in got[:5]], ref)
        print(f"{name} f64: err / (T 1e-9) " + " ".join(f"{a} {e / (T * TOL64):.2e}" for a, e in err.items()))
        assert max(err.values()) <= T * TOL64, err


@pytest.mark.parametrize("name", ["iiwa_like", "random_prismatic_n6"])
def test_chunked_workspaces_agree_with_the_default(name):
    torch = _torch()
    rbd = _rbd(name)
    n, B, T = rbd.n, B0, 5
    q0, qd0, u, c = _inputs(name, B, T, seed=2)
    q0_t, qd0_t, u_t = _dev(torch.float64, q0, qd0, u)
    t = dict(zip(c, _dev(torch.float64, *c.values())))
    q_t, qd_t = rbd.rollout(q0_t, qd0_t, u_t, DTC)
    kw = dict(q=q_t, qd=qd_t, **_api_costs(t, False))
    full = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, **kw)
    wsb = rbd._lib.lib.rbd_rollout_lqr_workspace_bytes
    for steps in (1, 2):
        got = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, workspace_bytes=int(wsb(B, steps, 8)), **kw)
        err = _errs([_np(x) for x in got[:5]], [_np(x) for x in full[:5]])
        assert max(err.values()) <= TOL64 and torch.equal(got[5], full[5]), (steps, err)
    from rbdreference_amd._lib import RbdError
    with pytest.raises(RbdError, match="workspace missing or smaller"):
        rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, workspace_bytes=int(wsb(B, 1, 8)) - 16, **kw)


def test_convenience_paths():
    torch = _torch()
    name = "iiwa_like"
    rbd = _rbd(name)
    n, B, T = rbd.n, B0, 4
    q0, qd0, u, c = _inputs(name, B, T, seed=3)
    q0_t, qd0_t, u_t = _dev(torch.float64, q0, qd0, u)
    t = dict(zip(c, _dev(torch.float64, *c.values())))
    q_t, qd_t = rbd.rollout(q0_t, qd0_t, u_t, DTC)
    costs = _api_costs(t, False)
    want = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q_t, qd=qd_t, **costs)
    eq = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    # the trajectory is computed when omitted
    assert eq(rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, **costs), want)
    # a second stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q_t, qd=qd_t, **costs)
    s.synchronize()
    assert eq(other, want)
    # a shared control sequence is expanded, the gains stay per row
    us = u_t[:, 0].contiguous()
    sh = rbd.rollout_lqr(q0_t, qd0_t, us, DTC, **costs)
    assert sh[0].shape == (T, B, n) and eq(sh, rbd.rollout_lqr(q0_t, qd0_t, us[:, None].expand(T, B, n).contiguous(), DTC, **costs))
    # final-only state costs are the dense ones with zeros before the last slice; a shared hess_u is the expanded one
    z = {a: torch.zeros_like(costs[a]) for a in ("grad_q", "grad_qd", "hess_q", "hess_qd")}
    for a in z:
        z[a][-1] = costs[a][-1]
    hu = t["hu"][0, 0].contiguous()
    fin = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q_t, qd=qd_t, grad_u=t["gu"], hess_u=hu, **{a: costs[a][-1].contiguous() for a in z})
    den = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q_t, qd=qd_t, grad_u=t["gu"], hess_u=hu.expand(T, B, n).contiguous(), **z)
    assert eq(fin, den)
    # numpy in -> float64 numpy out; one row
    out = rbd.rollout_lqr(q0, qd0, u, DTC, **_api_costs(c, False))
    assert all(isinstance(x, np.ndarray) for x in out) and all(x.dtype == np.float64 for x in out[:5]) and out[5].dtype == np.int32
    assert max(_errs(out[:5], [_np(x) for x in want[:5]]).values()) <= TOL64
    one = rbd.rollout_lqr(q0[0], qd0[0], u[:, 0], DTC, hess_u=c["hu"][:, 0], grad_q=c["gq"][:, 0], hess_q=c["hq"][:, 0])
    assert [x.shape for x in one] == [(T, n), (T, n, 2 * n), (2 * n,), (2 * n, 2 * n), (2,), ()]
    # a full terminal Hessian goes in through P
    J = torch.randn(B, 3, 2 * n, device="cuda:0", dtype=torch.float64, generator=torch.Generator("cuda:0").manual_seed(1))
    Pf = torch.einsum("bkr,bkc->brc", J, J)
    dc = rbd.rnea_grad(q0_t, qd0_t, rbd.aba(q0_t, qd0_t, u_t[0]))[None]
    Mi = rbd.minv(q0_t)[None]
    got = rbd.rollout_riccati(dc, Mi, DTC, grad_u=t["gu"][:1].contiguous(), hess_u=hu, P=Pf.clone())
    ref = riccati(_np(dc), _np(Mi), DTC, gu=_np(t["gu"][:1]), hu=_np(hu), P=_np(Pf))
    assert max(_errs([_np(x) for x in got[:5]], ref).values()) <= TOL64


# ---- 5. memory contract through ctypes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_capi_overwrites_poisoned_outputs_and_nothing_else(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    B, T, n, GUARD = B0, 3, rbd.n, 1024
    dt = _dtype(sfx)
    esz = 4 if sfx == "f32" else 8
    q0, qd0, u, c = _inputs(name, B, T, seed=6)
    q0_t, qd0_t, u_t = _dev(dt, q0, qd0, u)
    t = dict(zip(c, _dev(dt, *c.values())))
    q, qd = rbd.rollout(q0_t, qd0_t, u_t, DTC)
    ins = (q0_t, qd0_t, u_t, q, qd, t["gq"], t["gqd"], t["hq"], t["hqd"], t["gu"], t["hu"])
    keep = [x.clone() for x in ins]
    lib = rbd._lib.lib
    fn = getattr(lib, f"rbd_rollout_lqr_{sfx}")
    st = torch.cuda.current_stream().cuda_stream
    want = rbd.rollout_lqr(q0_t, qd0_t, u_t, DTC, q=q, qd=qd, **_api_costs(t, False))
    for steps_in_ws in (T, 1):
        wsb = int(lib.rbd_rollout_lqr_workspace_bytes(B, steps_in_ws, esz))
        ws = torch.full((wsb + GUARD,), 0x5A, device="cuda:0", dtype=torch.uint8)
        sizes = (T * B * n, T * B * n * 2 * n, B * 2 * n, B * 4 * n * n, B * 2)           # k K lam P dV
        bufs = [torch.full((GUARD + s + GUARD,), float("nan"), device="cuda:0", dtype=dt) for s in sizes]
        sbuf = torch.full((GUARD + B + GUARD,), -7, device="cuda:0", dtype=torch.int32)
        for b_ in bufs:
            b_[:GUARD] = -777.25
            b_[-GUARD:] = -777.25
        outs = [b_[GUARD:GUARD + s] for b_, s in zip(bufs, sizes)]
        status = sbuf[GUARD:GUARD + B]
        rc = fn(*(x.data_ptr() for x in ins[:9]), 0, ins[9].data_ptr(), ins[10].data_ptr(), 0, 0.0, DTC, -9.81, 0, B, T,
                *(o.data_ptr() for o in outs), status.data_ptr(), ws.data_ptr(), wsb, st)
        assert rc == 0, lib.rbd_last_error()
        torch.cuda.synchronize()
        for b_, o in zip(bufs, outs):
            assert bool((b_[:GUARD] == -777.25).all()) and bool((b_[-GUARD:] == -777.25).all()), "guard band overwritten"
            assert not bool(torch.isnan(o).any()), "an output element was not written"
        assert bool((sbuf[:GUARD] == -7).all()) and bool((sbuf[-GUARD:] == -7).all()) and not bool(status.any())
        assert bool((ws[wsb:] == 0x5A).all()), "the workspace's guard tail was overwritten"
        for x, k in zip(ins, keep):
            assert torch.equal(x, k), "an input was modified"
        if steps_in_ws == T:
            for o, w in zip(outs, want):
                assert torch.equal(o.view(w.shape), w)


# ---- 6. first use --------------------------------------------------------------------------------------------------------
def test_first_call_of_a_never_built_robot_goes_through_the_lqr_family_library(monkeypatch):
    """The robot's full library is held back (its background build waits until the end of the test), as on a first use:
    the call is answered by the `lqr` family library (build.FAMILIES), built on demand."""
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
    # (the robot of the rollg first-use test: the units the two families share are compiled once)
    robot = random_tree([-1, 0, 1, 1], seed=4325, name="rollg_first_use_n4")
    om = orc.model_from_robot(robot)
    try:
        rbd = RBDReference(robot, generic="never")
        B, T, n = 100, 4, 4
        rng = np.random.default_rng(17)
        q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
        gq, hq, hu = rng.standard_normal((T, B, n)), rng.uniform(5, 15, (T, B, n)), rng.uniform(1, 2, n)
        q, qd = oracle_rollout(om, q0, qd0, u, DTC)            # (the trajectory from the oracle: no second family is built)
        t = _dev(torch.float64, q0, qd0, u, gq, hq, hu, q, qd)
        got = rbd.rollout_lqr(t[0], t[1], t[2], DTC, grad_q=t[3], hess_q=t[4], hess_u=t[5], q=t[6], qd=t[7])
        lib = rbd._lib._tls.lib
        assert rbd._lib._full is None and lib._name == family_lib_path(rbd.model, "lqr", "f64")
        ref = oracle_lqr(om, q0, qd0, u, DTC, q, qd, gq=gq, hq=hq, hu=hu)
        err = _errs([_np(x) for x in got[:5]], ref)
        print(f"first use: err / (T 1e-9) {max(err.values()) / (T * TOL64):.2e}")
        assert max(err.values()) <= T * TOL64
    finally:
        release.set()


# ---- 7. floating base ------------------------------------------------------------------------------------------------------
def test_floating_base_library_exports_unsupported_stubs():
    from rbdreference_amd import RBDReference
    from rbdreference_amd._lib import RBD_ERR_UNSUPPORTED
    from rbdreference_amd.robot import floating_quadruped_like
    rbd = RBDReference(floating_quadruped_like(), build=False)
    fake = ctypes.c_void_p(4096)
    lib = rbd._lib.lib
    assert lib.rbd_rollout_lqr_workspace_bytes(4, 3, 8) == 0
    for sfx in ("f32", "f64"):
        assert getattr(lib, f"rbd_rollout_riccati_{sfx}")(*([fake] * 6), 0, fake, fake, 0, 0.0, DTC, 0, 4, 3, *([fake] * 6),
                                                          None) == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in lib.rbd_last_error()
        assert getattr(lib, f"rbd_rollout_lqr_{sfx}")(*([fake] * 9), 0, fake, fake, 0, 0.0, DTC, -9.81, 0, 4, 3, *([fake] * 7),
                                                      1 << 30, None) == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in lib.rbd_last_error()
    with pytest.raises(NotImplementedError):
        rbd.rollout_lqr(np.zeros(rbd.nv), np.zeros(rbd.nv), np.zeros((3, rbd.nv)), DTC, hess_u=np.ones(rbd.nv))
