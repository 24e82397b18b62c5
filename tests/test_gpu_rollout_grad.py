"""RBDReference.rollout_grad / rollout_adjoint / rollout(differentiable=True) on the GPU (rbd_rollout_adjoint, rbd_rollout_grad;
csrc/rbd_rollout_adj.h).

Two kinds of parity check, both against tests/rollout_grad_oracle.py in fp64 on the exact device values:

  scan alone    random dc_du, Minv (entries uniform(-1, 1) / n, Minv symmetrised) and standard-normal g.  Bound per
                element and row: T (2n + 8) eps S-bar, eps the unit round-off of the run's precision -- the dot-product
                forward-error bound gamma_k |x|^T |y| (k <= 2n + 8: a dot product of n terms for nu, one of n for the
                back-substitution, the few operations of g, w and mu), carried through the same recursion with absolute
                values and no cancellation (S-bar, rollout_grad_oracle.magnitude), once per step.  This is the SHARP check
                of the new kernel, in both precisions.
  composite     teacher-forced: rollout on the device, rollout_grad on the stored trajectory, the evaluating oracle at
                the device's stored states.  fp64: T 1e-9 S per row, this suite's fp64 aba / minv tolerance once per
                step, S the running magnitude of the recursion; swapping the integrators moves every row by >= 1e-3 S, so
                this tells the integrators, a dropped w or an off-by-one linearisation point apart (asserted: the two
                integrators differ by more than 1e-6 S).  fp32: COND_SLACK EPS32 max_t cond(H_t) T S, the suite's
                conditioned bound -- it only guards the plumbing; the sharp fp32 check is the scan test.

|.| is the max norm over a row.  dt is the value the kernels received: 0.01 rounded to the run's precision."""
import ctypes

import numpy as np
import pytest

from conftest import all_golden_names, make_robot
from oracle import rbd_oracle as orc
from rollout_grad_oracle import adjoint, linearise, magnitude
from rollout_oracle import INTEGRATORS, rollout as oracle_rollout

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24          # unit round-off of float32
EPS64 = 2.0 ** -53
COND_SLACK = 8.0            # as test_gpu_parity.check_conditioned
TOL64 = 1e-9                # as test_gpu_parity's fp64 aba / minv checks
DT = 0.01
ROBOTS = all_golden_names()                 # the nine fixed-base fixture robots
SCAN_ROBOTS = ["iiwa_like", "random_tree_n9", "random_twochains_n18", "atlas_like"]     # n = 7, 9, 18, 30

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


def _inputs(name, B, T, seed=1):
    """test_gpu_rollout._inputs, then grad_q, grad_qd standard normal from the same generator."""
    n = _om(name).n
    rng = np.random.default_rng(1000 * seed + n)
    q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(-1, 1, (B, n)), rng.uniform(-5, 5, (T, B, n))
    return q0, qd0, u, rng.standard_normal((T, B, n)), rng.standard_normal((T, B, n))


def _scan_data(n, B, T, seed):
    rng = np.random.default_rng(seed)
    dc = rng.uniform(-1, 1, (T, B, n, 2 * n)) / n
    M = rng.uniform(-1, 1, (T, B, n, n)) / n
    M = 0.5 * (M + np.swapaxes(M, -1, -2))
    return dc, M, rng.standard_normal((T, B, n)), rng.standard_normal((T, B, n))


def _worst(got, ref, bound_rows, row_axis):
    """max over elements of |got - ref| / bound of the element's row."""
    shape = [1] * got.ndim
    shape[row_axis] = -1
    return float(np.max(np.abs(got - ref) / bound_rows.reshape(shape)))


# ---- 1. the scan alone, random data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("name", SCAN_ROBOTS)
def test_scan_matches_the_oracle_within_the_dot_product_bound(name, T, sfx, integ, final):
    rbd = _rbd(name)
    n = rbd.n
    C = 256 // (2 * n)
    B = 2 * C + 1                               # two full blocks and a ragged one
    dc, M, gq, gqd = _scan_data(n, B, T, seed=7 * n + T)
    if final:
        gq, gqd = gq[-1], gqd[-1]
    tdc, tM, tgq, tgqd = _dev(_dtype(sfx), dc, M, gq, gqd)
    gu, lam = rbd.rollout_adjoint(tdc, tM, DT, tgq, tgqd, integrator=integ)
    assert gu.shape == (T, B, n) and lam.shape == (B, 2 * n) and gu.dtype == lam.dtype == tdc.dtype
    dt = _dt(sfx)
    args = (_np(tdc), _np(tM), dt, _np(tgq), _np(tgqd), integ)
    ref_u, ref_lam, _ = adjoint(*args)
    bound = T * (2 * n + 8) * (EPS32 if sfx == "f32" else EPS64) * magnitude(*args)       # [B]
    w_u, w_l = _worst(_np(gu), ref_u, bound, 1), _worst(_np(lam), ref_lam, bound, 0)
    print(f"{name} n={n} B={B} T={T} {sfx} {integ} final={final}: grad_u err / bound {w_u:.3f}   lam err / bound {w_l:.3f}")
    assert np.isfinite(_np(gu)).all() and np.isfinite(_np(lam)).all()
    assert w_u <= 1.0 and w_l <= 1.0, (w_u, w_l)
    assert np.abs(ref_u).max() > 1e-4 and np.abs(ref_lam).max() > 0.1                      # the data exercise the recursion


# ---- 2. a scan split at any step is bit-identical ---------------------------------------------------------------------
@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_split_scan_is_bit_identical(name, sfx, final):
    torch = _torch()
    rbd = _rbd(name)
    n, T = rbd.n, 5
    B = 2 * (256 // (2 * n)) + 1
    dc, M, gq, gqd = _dev(_dtype(sfx), *_scan_data(n, B, T, seed=11 * n))
    for integ in INTEGRATORS:
        whole = rbd.rollout_adjoint(dc, M, DT, gq[-1] if final else gq, gqd[-1] if final else gqd, integrator=integ)
        for k in range(1, T):
            if final:       # the terminal gradient belongs to the call that holds the last step; the other one gets zeros
                hi_g, lo_g = (gq[-1], gqd[-1]), (torch.zeros_like(gq[:k]), None)
            else:
                hi_g, lo_g = (gq[k:].contiguous(), gqd[k:].contiguous()), (gq[:k].contiguous(), gqd[:k].contiguous())
            gu_hi, lam = rbd.rollout_adjoint(dc[k:].contiguous(), M[k:].contiguous(), DT, *hi_g, integrator=integ)
            gu_lo, lam2 = rbd.rollout_adjoint(dc[:k].contiguous(), M[:k].contiguous(), DT, *lo_g, integrator=integ, lam=lam)
            assert lam2.data_ptr() == lam.data_ptr()                                   # carried in place
            assert torch.equal(torch.cat([gu_lo, gu_hi]), whole[0]), (integ, k)
            assert torch.equal(lam2, whole[1]), (integ, k)


# ---- 3. the composite, teacher-forced ---------------------------------------------------------------------------------
def _composite_reference(name, sfx, integ, q0, qd0, u, q, qd, gq, gqd, grav=-9.81):
    """Oracle results at the device's stored states -> (grad_u, grad_q0, grad_qd0, bound [B], S [B], dc, Minv)."""
    om = _om(name)
    T = u.shape[0]
    dc, Mi = linearise(om, q0, qd0, u, q, qd, grav)
    gu, lam, S = adjoint(dc, Mi, _dt(sfx), gq, gqd, integ)
    n = om.n
    if sfx == "f64":
        bound = T * TOL64 * S
    else:
        qs = np.concatenate([q0[None], q[:T - 1]])
        cond = np.max(np.stack([np.linalg.cond(orc.crba(om, qs[t])) for t in range(T)]), axis=0)
        bound = COND_SLACK * EPS32 * cond * T * S
    return gu, lam[:, :n], lam[:, n:], bound, S, dc, Mi


def _check_composite(tag, got, ref):
    gu, gq0, gqd0, bound = ref[:4]
    w = (_worst(_np(got[0]), gu, bound, 1), _worst(_np(got[1]), gq0, bound, 0), _worst(_np(got[2]), gqd0, bound, 0))
    print(f"{tag}: err / bound  grad_u {w[0]:.3f}  grad_q0 {w[1]:.3f}  grad_qd0 {w[2]:.3f}")
    assert all(np.isfinite(_np(x)).all() for x in got), tag
    assert max(w) <= 1.0, (tag, w)


@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ROBOTS)
def test_rollout_grad_matches_the_oracle_at_the_stored_trajectory(name, sfx, integ):
    """fp64 bound T 1e-9 S; fp32 bound COND_SLACK EPS32 max_t cond(H_t) T S, which only guards the plumbing: the sharp
    fp32 check of the new kernel is test_scan_matches_the_oracle_within_the_dot_product_bound.  random_prismatic_n6 passes
    because the oracle uses the same rnea_grad (the prismatic caveat of rollout_grad is not a parity matter)."""
    rbd = _rbd(name)
    B, T, n = 130, 5, rbd.n
    x = _dev(_dtype(sfx), *_inputs(name, B, T, seed=1))
    q0, qd0, u, gq, gqd = x
    q, qd = rbd.rollout(q0, qd0, u, DT, integrator=integ)
    got = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, integrator=integ, q=q, qd=qd)
    assert got[0].shape == (T, B, n) and got[1].shape == got[2].shape == (B, n)
    assert all(g.dtype == q0.dtype and g.is_contiguous() for g in got)
    ref = _composite_reference(name, sfx, integ, *(_np(t) for t in (q0, qd0, u, q, qd, gq, gqd)))
    _check_composite(f"{name} {sfx} {integ}", got, ref)
    if sfx == "f64":
        # the other integrator's recursion along the same stored trajectory is told apart, row by row
        other = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, integrator=[i for i in INTEGRATORS if i != integ][0], q=q, qd=qd)
        diff = np.maximum.reduce([np.abs(_np(got[0]) - _np(other[0])).max((0, 2)), np.abs(_np(got[1]) - _np(other[1])).max(1),
                                  np.abs(_np(got[2]) - _np(other[2])).max(1)])
        sep = float(np.min(diff / ref[4]))
        print(f"{name} {integ}: the integrators differ by >= {sep:.2e} S in every row")
        assert sep > 1e-6


# ---- 4. chunking -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_chunked_workspaces_agree_and_a_short_one_is_refused(name):
    from rbdreference_amd._lib import RBD_ERR_WORKSPACE, RbdError
    torch = _torch()
    rbd = _rbd(name)
    B, T = 130, 5
    q0, qd0, u, gq, gqd = _dev(torch.float64, *_inputs(name, B, T, seed=1))
    q, qd = rbd.rollout(q0, qd0, u, DT)
    full = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd)
    ref = _composite_reference(name, "f64", "semi_implicit", *(_np(t) for t in (q0, qd0, u, q, qd, gq, gqd)))
    wsb = rbd._lib.lib.rbd_rollout_grad_workspace_bytes
    one, two = int(wsb(B, 1, 8)), int(wsb(B, 2, 8))
    assert 0 < one < two < int(wsb(B, T, 8))
    for tag, ws in (("one step", one), ("two steps", two), ("between", two + 16)):
        got = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd, workspace_bytes=ws)
        _check_composite(f"{name} workspace for {tag}", got, ref)
        w = max(_worst(_np(a), _np(b), ref[3], ax) for a, b, ax in zip(got, full, (1, 0, 0)))
        print(f"{name} workspace for {tag} vs default: diff / bound {w:.3f}")
        assert w <= 1.0
    with pytest.raises(RbdError) as e:
        rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd, workspace_bytes=one - 16)
    assert e.value.code == RBD_ERR_WORKSPACE and "workspace" in str(e.value)


# ---- 5. convenience paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_convenience_paths(sfx):
    torch = _torch()
    name = "random_limbs_n14"
    rbd = _rbd(name)
    B, T, n = 67, 4, rbd.n
    q0, qd0, u, gq, gqd = _dev(_dtype(sfx), *_inputs(name, B, T, seed=3))
    q, qd = rbd.rollout(q0, qd0, u, DT)
    want = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd)
    # the trajectory omitted: rolled out here, the same kernel on the same inputs
    got = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # only one of the two gradients; a final-state gradient is the dense one with zeros before the last slice
    zq = torch.zeros_like(gq)
    zq[-1] = gq[-1]
    fin = rbd.rollout_grad(q0, qd0, u, DT, grad_q=gq[-1].contiguous(), q=q, qd=qd)
    dense = rbd.rollout_grad(q0, qd0, u, DT, grad_q=zq, grad_qd=torch.zeros_like(zq), q=q, qd=qd)
    assert all(torch.equal(a, b) for a, b in zip(fin, dense))
    only_qd = rbd.rollout_grad(q0, qd0, u, DT, grad_qd=gqd, q=q, qd=qd)
    assert all(torch.equal(a, b) for a, b in zip(only_qd, rbd.rollout_grad(q0, qd0, u, DT, torch.zeros_like(gq), gqd, q=q, qd=qd)))
    # one control sequence for every row: the expanded call, summed over the batch
    us = u[:, 0].contiguous()
    shared = rbd.rollout_grad(q0, qd0, us, DT, gq, gqd)
    expanded = rbd.rollout_grad(q0, qd0, us[:, None, :].expand(T, B, n).contiguous(), DT, gq, gqd)
    assert shared[0].shape == (T, n) and shared[1].shape == (B, n)
    scale = expanded[0].abs().sum(1)
    assert bool(((shared[0] - expanded[0].sum(1)).abs() <= 4 * B * (EPS32 if sfx == "f32" else EPS64) * scale).all())
    assert torch.equal(shared[1], expanded[1]) and torch.equal(shared[2], expanded[2])
    # a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_s = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(on_s, want))
    with pytest.raises(TypeError):
        rbd.rollout_grad(q0, qd0, u, DT, _np(gq), gqd)                              # torch state, numpy gradient


def test_unbatched_numpy_call_returns_float64_arrays():
    torch = _torch()
    name = "iiwa_like"
    rbd = _rbd(name)
    T, n = 4, rbd.n
    q0, qd0, u, gq, gqd = _inputs(name, 3, T, seed=4)
    tq0, tqd0, tu, tgq, tgqd = _dev(torch.float64, q0, qd0, u, gq, gqd)
    want = [_np(x) for x in rbd.rollout_grad(tq0, tqd0, tu, DT, tgq, tgqd)]
    got = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd)                                  # numpy, batched
    one = rbd.rollout_grad(q0[1], qd0[1], u[:, 1], DT, gq[:, 1], gqd[:, 1])          # numpy, one configuration
    fin = rbd.rollout_grad(q0[1], qd0[1], u[:, 1], DT, grad_q=gq[-1, 1])             # ... with a terminal gradient [n]
    for k in range(3):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == np.float64 and np.array_equal(got[k], want[k])
        assert isinstance(one[k], np.ndarray) and one[k].dtype == np.float64
    assert one[0].shape == fin[0].shape == (T, n) and one[1].shape == one[2].shape == fin[1].shape == (n,)
    # (a batch of one row runs the small-batch kernels of rnea_grad / minv: equal to rounding, not bit for bit)
    scale = max(np.abs(want[0][:, 1]).max(), np.abs(want[1][1]).max(), np.abs(want[2][1]).max())      # <= the row's S
    for k, w in enumerate(want):
        ref = w[:, 1] if k == 0 else w[1]
        assert np.abs(one[k] - ref).max() <= T * TOL64 * scale
    gu, lam = rbd.rollout_adjoint(np.zeros((2, 3, n, 2 * n)), np.zeros((2, 3, n, n)), DT, grad_q=gq[:2, :3])
    assert isinstance(gu, np.ndarray) and gu.shape == (2, 3, n) and lam.shape == (3, 2 * n)
    assert np.array_equal(gu, np.zeros_like(gu)) and np.array_equal(lam[:, :n], gq[0, :3] + gq[1, :3])


# ---- 6. autograd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_autograd_backward_is_rollout_grad_bit_for_bit(sfx, integ):
    torch = _torch()
    name = "iiwa_like"
    rbd = _rbd(name)
    B, T = 70, 4
    q0, qd0, u, a, b = _dev(_dtype(sfx), *_inputs(name, B, T, seed=5))
    plain = rbd.rollout(q0, qd0, u, DT, integrator=integ, differentiable=False)
    assert all(x.grad_fn is None and not x.requires_grad for x in plain)
    for x in (q0, qd0, u):
        x.requires_grad_(True)
    q, qd = rbd.rollout(q0, qd0, u, DT, integrator=integ, differentiable=True)
    assert q.grad_fn is not None and torch.equal(q, plain[0]) and torch.equal(qd, plain[1])
    ((q * a).sum() + (qd * b).sum()).backward()
    want = rbd.rollout_grad(q0.detach(), qd0.detach(), u.detach(), DT, a, b, integrator=integ, q=plain[0], qd=plain[1])
    assert torch.equal(u.grad, want[0]) and torch.equal(q0.grad, want[1]) and torch.equal(qd0.grad, want[2])
    # the final state only: the trajectory is still kept for the backward pass, the gradient is a terminal one
    for x in (q0, qd0, u):
        x.grad = None
    qf, qdf = rbd.rollout(q0, qd0, u, DT, integrator=integ, trajectory=False, differentiable=True)
    assert qf.shape == (B, rbd.n) and torch.equal(qf, plain[0][-1]) and torch.equal(qdf, plain[1][-1])
    ((qf * a[-1]).sum() + (qdf * b[-1]).sum()).backward()
    want = rbd.rollout_grad(q0.detach(), qd0.detach(), u.detach(), DT, a[-1].contiguous(), b[-1].contiguous(), integrator=integ,
                            q=plain[0], qd=plain[1])
    assert torch.equal(u.grad, want[0]) and torch.equal(q0.grad, want[1]) and torch.equal(qd0.grad, want[2])
    # a shared control sequence: u.grad is summed over the batch
    us = u.detach()[:, 0].clone().requires_grad_(True)
    qs, _ = rbd.rollout(q0.detach(), qd0.detach(), us, DT, integrator=integ, differentiable=True)
    (qs * a).sum().backward()
    assert us.grad.shape == us.shape and bool(torch.isfinite(us.grad).all()) and float(us.grad.abs().max()) > 0


# ---- 7. memory contract through ctypes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_capi_overwrites_poisoned_outputs_and_nothing_else(name, sfx):
    torch = _torch()
    rbd = _rbd(name)
    B, T, n, GUARD = 257, 3, rbd.n, 1024
    dt = _dtype(sfx)
    esz = 4 if sfx == "f32" else 8
    q0, qd0, u, gq, gqd = _dev(dt, *_inputs(name, B, T, seed=6))
    q, qd = rbd.rollout(q0, qd0, u, DT)
    ins = (q0, qd0, u, q, qd, gq, gqd)
    keep = [x.clone() for x in ins]
    lib = rbd._lib.lib
    fn = getattr(lib, f"rbd_rollout_grad_{sfx}")
    st = torch.cuda.current_stream().cuda_stream
    want = rbd.rollout_grad(q0, qd0, u, DT, gq, gqd, q=q, qd=qd)
    for steps_in_ws in (T, 1):
        wsb = int(lib.rbd_rollout_grad_workspace_bytes(B, steps_in_ws, esz))
        ws = torch.full((wsb + GUARD,), 0x5A, device="cuda:0", dtype=torch.uint8)
        sizes = (T * B * n, B * n, B * n)
        bufs = [torch.full((GUARD + s + GUARD,), float("nan"), device="cuda:0", dtype=dt) for s in sizes]
        for b_ in bufs:
            b_[:GUARD] = -777.25
            b_[-GUARD:] = -777.25
        outs = [b_[GUARD:GUARD + s] for b_, s in zip(bufs, sizes)]
        rc = fn(*(x.data_ptr() for x in ins), 0, DT, -9.81, 0, B, T, *(o.data_ptr() for o in outs), ws.data_ptr(), wsb, st)
        assert rc == 0, lib.rbd_last_error()
        torch.cuda.synchronize()
        for b_, o in zip(bufs, outs):
            assert bool((b_[:GUARD] == -777.25).all()) and bool((b_[-GUARD:] == -777.25).all()), "guard band overwritten"
            assert not bool(torch.isnan(o).any()), "an output element was not written"
        assert bool((ws[wsb:] == 0x5A).all()), "the workspace's guard tail was overwritten"
        for x, k in zip(ins, keep):
            assert torch.equal(x, k), "an input was modified"
        if steps_in_ws == T:
            assert torch.equal(outs[0].view(T, B, n), want[0]) and torch.equal(outs[1].view(B, n), want[1])
            assert torch.equal(outs[2].view(B, n), want[2])


# ---- 8. first use --------------------------------------------------------------------------------------------------------
def test_first_call_of_a_never_built_robot_goes_through_the_rollg_family_library(monkeypatch):
    """The robot's full library is held back (its background build waits until the end of the test), as on a first use:
    the call is answered by the `rollg` family library (build.FAMILIES), built on demand."""
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
    robot = random_tree([-1, 0, 1, 1], seed=4325, name="rollg_first_use_n4")
    om = orc.model_from_robot(robot)
    try:
        rbd = RBDReference(robot, generic="never")
        B, T = 100, 4
        rng = np.random.default_rng(17)
        q0, qd0, u = rng.uniform(-np.pi, np.pi, (B, 4)), rng.uniform(-1, 1, (B, 4)), rng.uniform(-5, 5, (T, B, 4))
        gq, gqd = rng.standard_normal((T, B, 4)), rng.standard_normal((T, B, 4))
        q, qd = oracle_rollout(om, q0, qd0, u, DT)            # (the trajectory from the oracle: no second family is built)
        t = _dev(torch.float64, q0, qd0, u, gq, gqd, q, qd)
        got = rbd.rollout_grad(t[0], t[1], t[2], DT, t[3], t[4], q=t[5], qd=t[6])
        lib = rbd._lib._tls.lib
        assert rbd._lib._full is None and lib._name == family_lib_path(rbd.model, "rollg", "f64")
        dc, Mi = linearise(om, q0, qd0, u, q, qd)
        gu, lam, S = adjoint(dc, Mi, DT, gq, gqd)
        bound = T * TOL64 * S
        w = (_worst(_np(got[0]), gu, bound, 1), _worst(_np(got[1]), lam[:, :4], bound, 0), _worst(_np(got[2]), lam[:, 4:], bound, 0))
        print(f"first use: err / bound {w}")
        assert max(w) <= 1.0
    finally:
        release.set()


# ---- 9. floating base ------------------------------------------------------------------------------------------------------
def test_floating_base_library_exports_unsupported_stubs():
    from rbdreference_amd import RBDReference
    from rbdreference_amd._lib import RBD_ERR_UNSUPPORTED
    from rbdreference_amd.robot import floating_quadruped_like
    rbd = RBDReference(floating_quadruped_like(), build=False)
    fake = ctypes.c_void_p(4096)
    lib = rbd._lib.lib
    assert lib.rbd_rollout_grad_workspace_bytes(4, 3, 8) == 0
    for sfx in ("f32", "f64"):
        assert getattr(lib, f"rbd_rollout_adjoint_{sfx}")(fake, fake, fake, fake, 0, DT, 0, 4, 3, fake, fake, None) == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in lib.rbd_last_error()
        assert getattr(lib, f"rbd_rollout_grad_{sfx}")(fake, fake, fake, fake, fake, fake, fake, 0, DT, -9.81, 0, 4, 3, fake, fake, fake,
                                                       fake, 1 << 30, None) == RBD_ERR_UNSUPPORTED
        assert b"fixed-base robots only" in lib.rbd_last_error()
    with pytest.raises(NotImplementedError):
        rbd.rollout_grad(np.zeros(rbd.nv), np.zeros(rbd.nv), np.zeros((3, rbd.nv)), DT, grad_q=np.zeros((3, rbd.nv)))
