"""The argument layer of the rollout and control family (``rbdreference_amd/_rollout_args.py``) on the host: the call
context with CPU tensors, the pure checks, and -- through a bare ``RBDReference`` -- the full text of every refusal
the eleven methods make before anything touches the GPU."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from conftest import make_robot
from rbdreference_amd import QuadraticCost
from rbdreference_amd import _rollout_args as ra
from rbdreference_amd.packer import pack_robot

CPU = torch.device("cpu")
MIXING = "mixing numpy and torch"


def torch_ctx(dtp=torch.float32):
    return ra.Ctx(False, CPU, dtp)


def numpy_ctx():
    return ra.Ctx(True, CPU, torch.float64)


def test_ctx_derives_element_size_and_suffix():
    assert (torch_ctx().esz, torch_ctx().sfx) == (4, "f32")
    assert (numpy_ctx().esz, numpy_ctx().sfx) == (8, "f64")
    t = [torch.zeros(2, 3)]
    tensors, cx = ra.Ctx.from_prep((t, False, False, CPU, torch.float32))
    assert tensors is t and (cx.is_np, cx.dev, cx.dtp) == (False, CPU, torch.float32)


def test_tensor_of_a_torch_caller():
    cx = torch_ctx()
    assert cx.tensor(None) is None
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert cx.tensor(x) is x                                    # contiguous: no copy, so in-place arguments stay in place
    y = cx.tensor(x.t())
    assert y.is_contiguous() and torch.equal(y, x.t())
    for bad in (x.double(), x.to("meta")):
        with pytest.raises(TypeError) as e:
            cx.tensor(bad)
        assert str(e.value) == "all inputs must share device and dtype"
    for bad in (np.zeros(3), [1.0, 2.0]):
        with pytest.raises(TypeError, match=MIXING):
            cx.tensor(bad)
    s = torch.zeros(3, dtype=torch.int32)
    assert cx.tensor(s, torch.int32) is s
    with pytest.raises(TypeError) as e:
        cx.tensor(x, torch.int32)
    assert str(e.value) == "all inputs must share device and dtype (status: int32)"


def test_tensor_of_a_numpy_caller():
    cx = numpy_ctx()
    assert cx.tensor(None) is None
    with pytest.raises(TypeError, match=MIXING):
        cx.tensor(torch.zeros(3, dtype=torch.float64))
    t = cx.tensor([1, 2, 3])
    assert t.dtype == torch.float64 and t.tolist() == [1.0, 2.0, 3.0]
    a = np.arange(6, dtype=np.float32).reshape(2, 3).T
    t = cx.tensor(a)
    assert t.dtype == torch.float64 and t.is_contiguous() and np.array_equal(t.numpy(), a)
    b = cx.tensor(np.broadcast_to(np.arange(3.0), (2, 3)))      # a read-only broadcast view, as QuadraticCost.dense gives
    assert b.is_contiguous() and b.tolist() == [[0.0, 1.0, 2.0]] * 2
    s = cx.tensor([0, 2], torch.int32)
    assert s.dtype == torch.int32 and s.tolist() == [0, 2]


@pytest.mark.parametrize("dtp", [torch.float32, torch.float64])
def test_small_and_limits(dtp):
    cx, n = torch_ctx(dtp), 4
    other = torch.float64 if dtp == torch.float32 else torch.float32
    want = torch.tensor([0.5, 0.5, 0.5, 0.5], dtype=dtp)
    for x in (0.5, [0.5] * n, np.full(n, 0.5), torch.full((n,), 0.5, dtype=other)):
        s = cx.small(x)
        assert s.dtype == dtp and s.device == CPU and s.shape == np.shape(x)
        lo, hi = cx.limits(-np.asarray(x) if not isinstance(x, torch.Tensor) else -x, x, n)
        for t, w in ((lo, -want), (hi, want)):
            assert t.shape == (n,) and t.dtype == dtp and t.is_contiguous() and torch.equal(t, w)
    assert cx.limits(None, None, n) == (None, None)
    ready = torch.full((n,), 0.5, dtype=dtp)
    assert [t.data_ptr() for t in cx.limits(ready, ready, n)] == [ready.data_ptr()] * 2      # no copy inside the drivers' loops
    ra.check_limits("f", None, None, n)
    ra.check_limits("f", -1.0, np.ones(n), n)


def test_alpha_rows():
    cx, B, A, n = torch_ctx(), 3, 2, 4
    q0 = torch.arange(B * n, dtype=torch.float32).reshape(B, n)
    qd0 = -q0
    k = object()                                                # only its presence is looked at
    assert ra.check_alpha("f", 0.5) is None and ra.check_alpha("f", [1.0, 0.5]) == A and ra.check_alpha("f", torch.ones(A)) == A
    q, qd, al, rows = cx.alpha_rows(q0, qd0, 0.25, None, None, k, B)
    assert q is q0 and qd is qd0 and rows == B and al.dtype == torch.float32 and al.tolist() == [0.25] * B
    assert cx.alpha_rows(q0, qd0, 0.25, None, None, None, B)[2:] == (None, B)
    for alpha in ([1.0, 0.5], np.array([1.0, 0.5]), torch.tensor([1.0, 0.5], dtype=torch.float64)):
        q, qd, al, rows = cx.alpha_rows(q0, qd0, alpha, A, None, k, B)
        assert rows == A * B and al.shape == (A * B,) and al.dtype == torch.float32 and al.is_contiguous()
        for a in range(A):
            for b in range(B):
                assert al[a * B + b] == [1.0, 0.5][a] and torch.equal(q[a * B + b], q0[b]) and torch.equal(qd[a * B + b], qd0[b])
    assert cx.alpha_rows(q0, qd0, [1.0, 0.5], A, None, None, B)[2] is None
    ra_ = torch.tensor([0.0, 0.5, 1.0])
    q, qd, al, rows = cx.alpha_rows(q0, qd0, 1.0, None, ra_, k, B)
    assert q is q0 and rows == B and al.data_ptr() == ra_.data_ptr() and al.shape == (B,)
    assert cx.alpha_rows(q0[:1], qd0[:1], 1.0, None, torch.tensor(0.5), k, 1)[2].shape == (1,)      # one unbatched row
    with pytest.raises(TypeError, match=MIXING):
        cx.alpha_rows(q0, qd0, 1.0, None, np.ones(B), k, B)


def test_workspace_bytes():
    calls = []

    def query(per_step):
        def q(B, T, esz):
            calls.append((B, T, esz))
            return per_step * B * T * esz
        return q
    cap = 1000
    assert ra.workspace_bytes(query(10), 3, 4, 4, cap=cap) == 480              # below the cap: every step
    assert calls == [(3, 4, 4), (3, 1, 4)]
    assert ra.workspace_bytes(query(10), 3, 40, 4, cap=cap) == cap             # capped
    assert ra.workspace_bytes(query(100), 3, 40, 4, cap=cap) == 1200           # never below one step's need
    assert ra.workspace_bytes(query(10), 3, 40, 4, requested=77, cap=cap) == 77
    assert ra.workspace_bytes(query(10), 3, 40, 4, requested=0, cap=cap) == 0
    assert ra.workspace_bytes(query(1), 1 << 20, 1 << 8, 8) == ra.WS_CAP == 1 << 30
    ra.check_workspace_request("f", None)
    ra.check_workspace_request("f", 0)
    with pytest.raises(ValueError) as e:
        ra.check_workspace_request("f", -1)
    assert str(e.value) == "f: workspace_bytes < 0"


def test_to_caller():
    Res = namedtuple("Res", ["u", "w", "status"])
    res = Res(torch.ones(2, 3), None, torch.tensor([0, 1], dtype=torch.int32))
    assert torch_ctx().to_caller(res) is res
    out = numpy_ctx().to_caller(res)
    assert type(out) is Res and out.w is None
    assert isinstance(out.u, np.ndarray) and np.array_equal(out.u, np.ones((2, 3))) and out.status.dtype == np.int32
    pair = numpy_ctx().to_caller((res.u, res.status))
    assert type(pair) is tuple and all(isinstance(x, np.ndarray) for x in pair)
    assert isinstance(numpy_ctx().to_caller(res.u), np.ndarray) and numpy_ctx().to_caller(None) is None


def test_from_first_and_upload_refuse_before_the_gpu():
    x = torch.zeros(2, 3)
    with pytest.raises(TypeError, match=MIXING):
        ra.Ctx.from_first(np.zeros(3), x)
    with pytest.raises(TypeError, match=MIXING):
        ra.Ctx.from_first(x, x, np.zeros(3))
    with pytest.raises(RuntimeError, match="must live on a ROCm GPU"):
        ra.Ctx.from_first(x, x)
    with pytest.raises(TypeError, match=MIXING):
        ra.Ctx.upload(np.zeros(3), np.zeros(3), x, None, QuadraticCost(), strict=False)
    with pytest.raises(TypeError, match=MIXING):
        ra.Ctx.upload(x, x, np.zeros(3), None, QuadraticCost(), strict=True)
    c = QuadraticCost()
    cx, *same = ra.Ctx.upload(x, x, np.zeros(3), None, c, strict=False)      # a torch caller's inputs are left to the inner calls
    assert (cx.is_np, cx.dev, cx.dtp) == (False, CPU, torch.float32) and same[0] is x and same[4] is c


# ---- the refusals of the eleven methods, word for word ------------------------------------------------------------------
# Recorded by making the same calls with the argument handling each method had inline before this module existed; the
# existing tables (tests/test_*_host.py) only match the method's name.  (method, overriding kwargs, exception, message)
n, B, T, S = 7, 3, 2, 4
z = np.zeros


def good(n=n):
    base = dict(q0=z((B, n)), qd0=z((B, n)), u=z((T, B, n)), dt=0.01)
    lin = dict(dc_du=z((T, B, n, 2 * n)), Minv=z((T, B, n, n)), dt=0.01)
    return {
        "rollout": base,
        "rollout_closed_loop": dict(base, q_ref=z((T, B, n)), qd_ref=z((T, B, n)), K=z((T, B, n, 2 * n))),
        "rollout_cost": dict(base, cost=QuadraticCost()),
        "ilqr": dict(base, cost=QuadraticCost()),
        "mppi": dict(base, cost=QuadraticCost()),
        "mppi_update": dict(J=z((S, B)), du=z((T, S, B, n)), u=z((T, B, n)), lam=1.0),
        "rollout_grad": dict(base, grad_q=z((T, B, n))),
        "rollout_adjoint": dict(lin, grad_q=z((T, B, n))),
        "rollout_lqr": dict(base, hess_u=np.ones(n)),
        "rollout_riccati": dict(lin, hess_u=np.ones(n)),
    }


def bare_api(robot):
    from rbdreference_amd.api import RBDReference
    api = RBDReference.__new__(RBDReference)                    # no library, no GPU: a refusal must come before either
    api.robot, api.model = robot, pack_robot(robot)
    api.n, api.nv = api.model.n, api.model.nv
    return api


def refused(api, kwargs, rows):
    for method, override, etype, message in rows:
        with pytest.raises(etype) as e:
            getattr(api, method)(**{**kwargs[method], **override})
        assert type(e.value) is etype and str(e.value) == message, (method, override, str(e.value))


ROWS = [
    ('rollout', dict(integrator='rk4'), ValueError,
     "rollout: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout', dict(integrator=None), ValueError,
     "rollout: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_closed_loop', dict(integrator='rk4'), ValueError,
     "rollout_closed_loop: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_closed_loop', dict(integrator=None), ValueError,
     "rollout_closed_loop: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_cost', dict(integrator='rk4'), ValueError,
     "rollout_cost: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_cost', dict(integrator=None), ValueError,
     "rollout_cost: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('mppi', dict(integrator='rk4'), ValueError,
     "mppi: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('mppi', dict(integrator=None), ValueError,
     "mppi: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_grad', dict(integrator='rk4'), ValueError,
     "rollout_grad: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_grad', dict(integrator=None), ValueError,
     "rollout_grad: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_adjoint', dict(integrator='rk4'), ValueError,
     "rollout_adjoint: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_adjoint', dict(integrator=None), ValueError,
     "rollout_adjoint: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_lqr', dict(integrator='rk4'), ValueError,
     "rollout_lqr: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_lqr', dict(integrator=None), ValueError,
     "rollout_lqr: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout_riccati', dict(integrator='rk4'), ValueError,
     "rollout_riccati: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_riccati', dict(integrator=None), ValueError,
     "rollout_riccati: unknown integrator None; use one of ['euler', 'semi_implicit']"),
    ('rollout', dict(qd0=z((B + 1, n))), ValueError,
     'rollout: q0 and qd0 must both be [7] or [B, 7], got (3, 7) and (4, 7)'),
    ('rollout', dict(q0=z((B, n + 1))), ValueError,
     'rollout: q0 and qd0 must both be [7] or [B, 7], got (3, 8) and (3, 7)'),
    ('rollout', dict(q0=z(n), qd0=z(n)), ValueError,
     'rollout: q0 [7] takes u [T, 7], got (2, 3, 7)'),
    ('rollout', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'rollout: q0 and qd0 must both be [7] or [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('rollout_closed_loop', dict(qd0=z((B + 1, n))), ValueError,
     'rollout_closed_loop: q0 and qd0 must both be [7] or [B, 7], got (3, 7) and (4, 7)'),
    ('rollout_closed_loop', dict(q0=z((B, n + 1))), ValueError,
     'rollout_closed_loop: q0 and qd0 must both be [7] or [B, 7], got (3, 8) and (3, 7)'),
    ('rollout_closed_loop', dict(q0=z(n), qd0=z(n)), ValueError,
     "rollout_closed_loop: u must be ['T', 7] (time-major), got (2, 3, 7)"),
    ('rollout_closed_loop', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'rollout_closed_loop: q0 and qd0 must both be [7] or [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('rollout_cost', dict(qd0=z((B + 1, n))), ValueError,
     'rollout_cost: q0 and qd0 must both be [B, 7], got (3, 7) and (4, 7)'),
    ('rollout_cost', dict(q0=z((B, n + 1))), ValueError,
     'rollout_cost: q0 and qd0 must both be [B, 7], got (3, 8) and (3, 7)'),
    ('rollout_cost', dict(q0=z(n), qd0=z(n)), ValueError,
     'rollout_cost: q0 and qd0 must both be [B, 7], got (7,) and (7,)'),
    ('rollout_cost', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'rollout_cost: q0 and qd0 must both be [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('ilqr', dict(qd0=z((B + 1, n))), ValueError,
     'ilqr: q0 and qd0 must both be [B, 7], got (3, 7) and (4, 7)'),
    ('ilqr', dict(q0=z((B, n + 1))), ValueError,
     'ilqr: q0 and qd0 must both be [B, 7], got (3, 8) and (3, 7)'),
    ('ilqr', dict(q0=z(n), qd0=z(n)), ValueError,
     'ilqr: q0 and qd0 must both be [B, 7], got (7,) and (7,)'),
    ('ilqr', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'ilqr: q0 and qd0 must both be [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('mppi', dict(qd0=z((B + 1, n))), ValueError,
     'mppi: q0 and qd0 must both be [P, 7] with P > 0, got (3, 7) and (4, 7)'),
    ('mppi', dict(q0=z((B, n + 1))), ValueError,
     'mppi: q0 and qd0 must both be [P, 7] with P > 0, got (3, 8) and (3, 7)'),
    ('mppi', dict(q0=z(n), qd0=z(n)), ValueError,
     'mppi: q0 and qd0 must both be [P, 7] with P > 0, got (7,) and (7,)'),
    ('mppi', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'mppi: q0 and qd0 must both be [P, 7] with P > 0, got (1, 3, 7) and (1, 3, 7)'),
    ('rollout_grad', dict(qd0=z((B + 1, n))), ValueError,
     'rollout_grad: q0 and qd0 must both be [7] or [B, 7], got (3, 7) and (4, 7)'),
    ('rollout_grad', dict(q0=z((B, n + 1))), ValueError,
     'rollout_grad: q0 and qd0 must both be [7] or [B, 7], got (3, 8) and (3, 7)'),
    ('rollout_grad', dict(q0=z(n), qd0=z(n)), ValueError,
     'rollout_grad: q0 [7] takes u [T, 7], got (2, 3, 7)'),
    ('rollout_grad', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'rollout_grad: q0 and qd0 must both be [7] or [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('rollout_lqr', dict(qd0=z((B + 1, n))), ValueError,
     'rollout_lqr: q0 and qd0 must both be [7] or [B, 7], got (3, 7) and (4, 7)'),
    ('rollout_lqr', dict(q0=z((B, n + 1))), ValueError,
     'rollout_lqr: q0 and qd0 must both be [7] or [B, 7], got (3, 8) and (3, 7)'),
    ('rollout_lqr', dict(q0=z(n), qd0=z(n)), ValueError,
     'rollout_lqr: q0 [7] takes u [T, 7], got (2, 3, 7)'),
    ('rollout_lqr', dict(q0=z((1, B, n)), qd0=z((1, B, n))), ValueError,
     'rollout_lqr: q0 and qd0 must both be [7] or [B, 7], got (1, 3, 7) and (1, 3, 7)'),
    ('rollout', dict(u=z((B, T, n + 1))), ValueError,
     'rollout: u must be [T, 3, 7] or [T, 7] (time-major), got (3, 2, 8)'),
    ('rollout', dict(u=z((T, B + 1, n))), ValueError,
     'rollout: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 4, 7)'),
    ('rollout', dict(u=z((0, B, n))), ValueError,
     'rollout: u holds no step (T == 0)'),
    ('rollout', dict(u=z((T, 1, B, n))), ValueError,
     'rollout: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 1, 3, 7)'),
    ('rollout_closed_loop', dict(u=z((B, T, n + 1))), ValueError,
     "rollout_closed_loop: u must be ['T', 3, 7] (time-major), got (3, 2, 8)"),
    ('rollout_closed_loop', dict(u=z((T, B + 1, n))), ValueError,
     "rollout_closed_loop: u must be ['T', 3, 7] (time-major), got (2, 4, 7)"),
    ('rollout_closed_loop', dict(u=z((0, B, n))), ValueError,
     'rollout_closed_loop: u holds no step (T == 0)'),
    ('rollout_closed_loop', dict(u=z((T, 1, B, n))), ValueError,
     "rollout_closed_loop: u must be ['T', 3, 7] (time-major), got (2, 1, 3, 7)"),
    ('rollout_closed_loop', dict(u=z((T, n))), ValueError,
     "rollout_closed_loop: u must be ['T', 3, 7] (time-major), got (2, 7)"),
    ('rollout_cost', dict(u=z((B, T, n + 1))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (3, 2, 8)'),
    ('rollout_cost', dict(u=z((T, B + 1, n))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (2, 4, 7)'),
    ('rollout_cost', dict(u=z((0, B, n))), ValueError,
     'rollout_cost: u holds no step (T == 0)'),
    ('rollout_cost', dict(u=z((T, 1, B, n))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (2, 1, 3, 7)'),
    ('rollout_cost', dict(u=z((T, n))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (2, 7)'),
    ('ilqr', dict(u=z((B, T, n + 1))), ValueError,
     'ilqr: u must be [T, 3, 7] (time-major, T > 0), got (3, 2, 8)'),
    ('ilqr', dict(u=z((T, B + 1, n))), ValueError,
     'ilqr: u must be [T, 3, 7] (time-major, T > 0), got (2, 4, 7)'),
    ('ilqr', dict(u=z((0, B, n))), ValueError,
     'ilqr: u must be [T, 3, 7] (time-major, T > 0), got (0, 3, 7)'),
    ('ilqr', dict(u=z((T, 1, B, n))), ValueError,
     'ilqr: u must be [T, 3, 7] (time-major, T > 0), got (2, 1, 3, 7)'),
    ('ilqr', dict(u=z((T, n))), ValueError,
     'ilqr: u must be [T, 3, 7] (time-major, T > 0), got (2, 7)'),
    ('mppi', dict(u=z((B, T, n + 1))), ValueError,
     'mppi: u must be [T, 3, 7] (time-major, T > 0), got (3, 2, 8)'),
    ('mppi', dict(u=z((T, B + 1, n))), ValueError,
     'mppi: u must be [T, 3, 7] (time-major, T > 0), got (2, 4, 7)'),
    ('mppi', dict(u=z((0, B, n))), ValueError,
     'mppi: u must be [T, 3, 7] (time-major, T > 0), got (0, 3, 7)'),
    ('mppi', dict(u=z((T, 1, B, n))), ValueError,
     'mppi: u must be [T, 3, 7] (time-major, T > 0), got (2, 1, 3, 7)'),
    ('mppi', dict(u=z((T, n))), ValueError,
     'mppi: u must be [T, 3, 7] (time-major, T > 0), got (2, 7)'),
    ('rollout_grad', dict(u=z((B, T, n + 1))), ValueError,
     'rollout_grad: u must be [T, 3, 7] or [T, 7] (time-major), got (3, 2, 8)'),
    ('rollout_grad', dict(u=z((T, B + 1, n))), ValueError,
     'rollout_grad: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 4, 7)'),
    ('rollout_grad', dict(u=z((0, B, n))), ValueError,
     'rollout_grad: u holds no step (T == 0)'),
    ('rollout_grad', dict(u=z((T, 1, B, n))), ValueError,
     'rollout_grad: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 1, 3, 7)'),
    ('rollout_lqr', dict(u=z((B, T, n + 1))), ValueError,
     'rollout_lqr: u must be [T, 3, 7] or [T, 7] (time-major), got (3, 2, 8)'),
    ('rollout_lqr', dict(u=z((T, B + 1, n))), ValueError,
     'rollout_lqr: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 4, 7)'),
    ('rollout_lqr', dict(u=z((0, B, n))), ValueError,
     'rollout_lqr: u holds no step (T == 0)'),
    ('rollout_lqr', dict(u=z((T, 1, B, n))), ValueError,
     'rollout_lqr: u must be [T, 3, 7] or [T, 7] (time-major), got (2, 1, 3, 7)'),
    ('mppi_update', dict(u=z((B, T, n + 1))), ValueError,
     'mppi_update: u must be [T, 3, 7] (time-major, T > 0), got (3, 2, 8)'),
    ('mppi_update', dict(u=z((T, B + 1, n))), ValueError,
     'mppi_update: u must be [T, 3, 7] (time-major, T > 0), got (2, 4, 7)'),
    ('mppi_update', dict(u=z((0, B, n))), ValueError,
     'mppi_update: u must be [T, 3, 7] (time-major, T > 0), got (0, 3, 7)'),
    ('mppi_update', dict(u=z((T, 1, B, n))), ValueError,
     'mppi_update: u must be [T, 3, 7] (time-major, T > 0), got (2, 1, 3, 7)'),
    ('mppi_update', dict(u=z((T, n))), ValueError,
     'mppi_update: u must be [T, 3, 7] (time-major, T > 0), got (2, 7)'),
    ('rollout', dict(q0=z(n), qd0=z(n), u=z((T, 1, n))), ValueError,
     'rollout: q0 [7] takes u [T, 7], got (2, 1, 7)'),
    ('rollout', dict(q0=z(n), qd0=z(n), u=z((0, n))), ValueError,
     'rollout: u holds no step (T == 0)'),
    ('rollout_closed_loop', dict(q0=z(n), qd0=z(n), u=z((T, 1, n))), ValueError,
     "rollout_closed_loop: u must be ['T', 7] (time-major), got (2, 1, 7)"),
    ('rollout_closed_loop', dict(q0=z(n), qd0=z(n), u=z((0, n))), ValueError,
     'rollout_closed_loop: u holds no step (T == 0)'),
    ('rollout_grad', dict(q0=z(n), qd0=z(n), u=z((T, 1, n))), ValueError,
     'rollout_grad: q0 [7] takes u [T, 7], got (2, 1, 7)'),
    ('rollout_grad', dict(q0=z(n), qd0=z(n), u=z((0, n))), ValueError,
     'rollout_grad: u holds no step (T == 0)'),
    ('rollout_lqr', dict(q0=z(n), qd0=z(n), u=z((T, 1, n))), ValueError,
     'rollout_lqr: q0 [7] takes u [T, 7], got (2, 1, 7)'),
    ('rollout_lqr', dict(q0=z(n), qd0=z(n), u=z((0, n))), ValueError,
     'rollout_lqr: u holds no step (T == 0)'),
    ('rollout', dict(u=z((0, n))), ValueError,
     'rollout: u holds no step (T == 0)'),
    ('rollout_cost', dict(u=z((T, 2, n))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (2, 2, 7)'),
    ('rollout_cost', dict(u=z((T, 0, n))), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (2, 0, 7)'),
    ('rollout_closed_loop', dict(u_min=-1.0), ValueError,
     'rollout_closed_loop: give u_min and u_max together, or neither'),
    ('rollout_closed_loop', dict(u_max=np.ones(n)), ValueError,
     'rollout_closed_loop: give u_min and u_max together, or neither'),
    ('rollout_closed_loop', dict(u_min=-np.ones(n + 1), u_max=1.0), ValueError,
     'rollout_closed_loop: u_min must be a scalar or [7], got (8,)'),
    ('rollout_closed_loop', dict(u_min=-1.0, u_max=np.ones((1, n))), ValueError,
     'rollout_closed_loop: u_max must be a scalar or [7], got (1, 7)'),
    ('rollout_cost', dict(u_min=-1.0), ValueError,
     'rollout_cost: give u_min and u_max together, or neither'),
    ('rollout_cost', dict(u_max=np.ones(n)), ValueError,
     'rollout_cost: give u_min and u_max together, or neither'),
    ('rollout_cost', dict(u_min=-np.ones(n + 1), u_max=1.0), ValueError,
     'rollout_cost: u_min must be a scalar or [7], got (8,)'),
    ('rollout_cost', dict(u_min=-1.0, u_max=np.ones((1, n))), ValueError,
     'rollout_cost: u_max must be a scalar or [7], got (1, 7)'),
    ('mppi_update', dict(u_min=-1.0), ValueError,
     'mppi_update: give u_min and u_max together, or neither'),
    ('mppi_update', dict(u_max=np.ones(n)), ValueError,
     'mppi_update: give u_min and u_max together, or neither'),
    ('mppi_update', dict(u_min=-np.ones(n + 1), u_max=1.0), ValueError,
     'mppi_update: u_min must be a scalar or [7], got (8,)'),
    ('mppi_update', dict(u_min=-1.0, u_max=np.ones((1, n))), ValueError,
     'mppi_update: u_max must be a scalar or [7], got (1, 7)'),
    ('mppi', dict(u_min=-1.0), ValueError,
     'mppi: give u_min and u_max together, or neither'),
    ('mppi', dict(u_max=np.ones(n)), ValueError,
     'mppi: give u_min and u_max together, or neither'),
    ('mppi', dict(u_min=-np.ones(n + 1), u_max=1.0), ValueError,
     'mppi: u_min must be a scalar or [7], got (8,)'),
    ('mppi', dict(u_min=-1.0, u_max=np.ones((1, n))), ValueError,
     'mppi: u_max must be a scalar or [7], got (1, 7)'),
    ('rollout_closed_loop', dict(alpha=z((2, 2))), ValueError,
     'rollout_closed_loop: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape (2, 2)'),
    ('rollout_closed_loop', dict(alpha=[]), ValueError,
     'rollout_closed_loop: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape (0,)'),
    ('rollout_closed_loop', dict(k=z((T, B, n)), alpha=0.5, row_alpha=z(B)), ValueError,
     'rollout_closed_loop: give alpha or row_alpha, not both'),
    ('rollout_closed_loop', dict(k=z((T, B, n)), alpha=[1.0, 0.5], row_alpha=z(B)), ValueError,
     'rollout_closed_loop: give alpha or row_alpha, not both'),
    ('rollout_closed_loop', dict(k=z((T, B, n)), alpha=torch.ones(()), row_alpha=z(B)), ValueError,
     'rollout_closed_loop: give alpha or row_alpha, not both'),
    ('rollout_closed_loop', dict(row_alpha=z(B)), ValueError,
     'rollout_closed_loop: row_alpha scales k, which is missing'),
    ('rollout_closed_loop', dict(k=z((T, B, n)), row_alpha=z(B + 1)), ValueError,
     'rollout_closed_loop: row_alpha must be [3] (one step size per row), got (4,)'),
    ('rollout_closed_loop', dict(k=z((T, B, n)), row_alpha=z((B, 1))), ValueError,
     'rollout_closed_loop: row_alpha must be [3] (one step size per row), got (3, 1)'),
    ('rollout_closed_loop', dict(k=z((T, B))), ValueError,
     'rollout_closed_loop: k must be [2, 3, 7], got (2, 3)'),
    ('rollout_closed_loop', dict(q0_ref=z((B, n))), ValueError,
     'rollout_closed_loop: give q0_ref and qd0_ref together, or neither (they default to q0, qd0)'),
    ('rollout_cost', dict(alpha=z((2, 2))), ValueError,
     'rollout_cost: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape (2, 2)'),
    ('rollout_cost', dict(alpha=[]), ValueError,
     'rollout_cost: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape (0,)'),
    ('rollout_cost', dict(k=z((T, B, n)), alpha=0.5, row_alpha=z(B)), ValueError,
     'rollout_cost: give alpha or row_alpha, not both'),
    ('rollout_cost', dict(k=z((T, B, n)), alpha=[1.0, 0.5], row_alpha=z(B)), ValueError,
     'rollout_cost: give alpha or row_alpha, not both'),
    ('rollout_cost', dict(k=z((T, B, n)), alpha=torch.ones(()), row_alpha=z(B)), ValueError,
     'rollout_cost: give alpha or row_alpha, not both'),
    ('rollout_cost', dict(row_alpha=z(B)), ValueError,
     'rollout_cost: row_alpha scales k, which is missing'),
    ('rollout_cost', dict(k=z((T, B, n)), row_alpha=z(B + 1)), ValueError,
     'rollout_cost: row_alpha must be [3] (one step size per row), got (4,)'),
    ('rollout_cost', dict(k=z((T, B, n)), row_alpha=z((B, 1))), ValueError,
     'rollout_cost: row_alpha must be [3] (one step size per row), got (3, 1)'),
    ('rollout_cost', dict(k=z((T, B))), ValueError,
     'rollout_cost: k must be [2, 3, 7], got (2, 3)'),
    ('rollout_cost', dict(q0_ref=z((B, n))), ValueError,
     'rollout_cost: q_ref, qd_ref, q0_ref and qd0_ref belong to the feedback term; K is missing'),
    ('rollout_closed_loop', dict(K=None), ValueError,
     'rollout_closed_loop: K is required'),
    ('rollout_closed_loop', dict(q_ref=z((T, B)), K=None), ValueError,
     'rollout_closed_loop: q_ref must be [2, 3, 7], got (2, 3)'),
    ('rollout_closed_loop', dict(K=z((T, B, n, n))), ValueError,
     'rollout_closed_loop: K must be [2, 3, 7, 14], got (2, 3, 7, 7)'),
    ('rollout_closed_loop', dict(qd0_ref=z(n), q0_ref=z((B, n))), ValueError,
     'rollout_closed_loop: qd0_ref must be [3, 7], got (7,)'),
    ('rollout_cost', dict(du=z((T, B + 1, n))), ValueError,
     'rollout_cost: du must be [2, 3, 7], got (2, 4, 7)'),
    ('rollout_cost', dict(K=z((T, B, n, n)), q_ref=z((T, B, n)), qd_ref=z((T, B, n))), ValueError,
     'rollout_cost: K must be [2, 3, 7, 14], got (2, 3, 7, 7)'),
    ('rollout_grad', dict(q=z((T, B, n))), ValueError,
     'rollout_grad: give both q and qd (the trajectory of rollout) or neither'),
    ('rollout_grad', dict(qd=z((T, B, n))), ValueError,
     'rollout_grad: give both q and qd (the trajectory of rollout) or neither'),
    ('rollout_grad', dict(q=z((T, B, n)), qd=z((T, B + 1, n))), ValueError,
     'rollout_grad: q and qd must be the trajectory [2, 3, 7], got (2, 3, 7) and (2, 4, 7)'),
    ('rollout_grad', dict(q=z((B, T, n + 1)), qd=z((B, T, n + 1))), ValueError,
     'rollout_grad: q and qd must be the trajectory [2, 3, 7], got (3, 2, 8) and (3, 2, 8)'),
    ('rollout_grad', dict(workspace_bytes=-1), ValueError,
     'rollout_grad: workspace_bytes < 0'),
    ('rollout_grad', dict(q0=z(n), qd0=z(n), u=z((T, n)), q=z((T, 1, n)), qd=z((T, 1, n))), ValueError,
     'rollout_grad: grad_q and grad_qd must both be [2, 7] or both [7] (final state), got [(2, 3, 7)]'),
    ('rollout_lqr', dict(q=z((T, B, n))), ValueError,
     'rollout_lqr: give both q and qd (the trajectory of rollout) or neither'),
    ('rollout_lqr', dict(qd=z((T, B, n))), ValueError,
     'rollout_lqr: give both q and qd (the trajectory of rollout) or neither'),
    ('rollout_lqr', dict(q=z((T, B, n)), qd=z((T, B + 1, n))), ValueError,
     'rollout_lqr: q and qd must be the trajectory [2, 3, 7], got (2, 3, 7) and (2, 4, 7)'),
    ('rollout_lqr', dict(q=z((B, T, n + 1)), qd=z((B, T, n + 1))), ValueError,
     'rollout_lqr: q and qd must be the trajectory [2, 3, 7], got (3, 2, 8) and (3, 2, 8)'),
    ('rollout_lqr', dict(workspace_bytes=-1), ValueError,
     'rollout_lqr: workspace_bytes < 0'),
    ('rollout_lqr', dict(q0=z(n), qd0=z(n), u=z((T, n)), q=z((T, 1, n)), qd=z((T, 1, n))), ValueError,
     'rollout_lqr: q and qd must be the trajectory [2, 7], got (2, 1, 7) and (2, 1, 7)'),
    ('rollout_grad', dict(grad_q=None), ValueError,
     'rollout_grad: give grad_q, grad_qd or both (the gradient of the cost with respect to the trajectory)'),
    ('rollout_grad', dict(grad_q=z((T, B, n)), grad_qd=z((B, n))), ValueError,
     'rollout_grad: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(2, 3, 7), (3, 7)]'),
    ('rollout_grad', dict(grad_q=z((T, B))), ValueError,
     'rollout_grad: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(2, 3)]'),
    ('rollout_grad', dict(grad_q=None, grad_qd=z((B, n + 1))), ValueError,
     'rollout_grad: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(3, 8)]'),
    ('rollout_adjoint', dict(grad_q=None), ValueError,
     'rollout_adjoint: give grad_q, grad_qd or both (the gradient of the cost with respect to the trajectory)'),
    ('rollout_adjoint', dict(grad_q=z((T, B, n)), grad_qd=z((B, n))), ValueError,
     'rollout_adjoint: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(2, 3, 7), (3, 7)]'),
    ('rollout_adjoint', dict(grad_q=z((T, B))), ValueError,
     'rollout_adjoint: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(2, 3)]'),
    ('rollout_adjoint', dict(grad_q=None, grad_qd=z((B, n + 1))), ValueError,
     'rollout_adjoint: grad_q and grad_qd must both be [2, 3, 7] or both [3, 7] (final state), got [(3, 8)]'),
    ('rollout_lqr', dict(hess_u=None), ValueError,
     "rollout_lqr: hess_u is required (the diagonal of the control cost's Hessian, [T, B, n] or [n])"),
    ('rollout_lqr', dict(grad_q=z((T, B, n)), hess_q=z((B, n))), ValueError,
     'rollout_lqr: grad_q, grad_qd, hess_q and hess_qd must all be [2, 3, 7] or all [3, 7] (last step only), got [(2, 3, 7), (3, 7)]'),
    ('rollout_lqr', dict(grad_qd=z((T, B))), ValueError,
     'rollout_lqr: grad_q, grad_qd, hess_q and hess_qd must all be [2, 3, 7] or all [3, 7] (last step only), got [(2, 3)]'),
    ('rollout_lqr', dict(grad_u=z((B, n))), ValueError,
     'rollout_lqr: grad_u must be [2, 3, 7], got (3, 7)'),
    ('rollout_lqr', dict(hess_u=z((B, n))), ValueError,
     'rollout_lqr: hess_u must be [2, 3, 7] or [7] (shared by every row and step), got (3, 7)'),
    ('rollout_lqr', dict(reg=-1.0), ValueError,
     'rollout_lqr: reg must be finite and >= 0, got -1.0'),
    ('rollout_lqr', dict(reg=float('nan')), ValueError,
     'rollout_lqr: reg must be finite and >= 0, got nan'),
    ('rollout_lqr', dict(reg=float('inf')), ValueError,
     'rollout_lqr: reg must be finite and >= 0, got inf'),
    ('rollout_riccati', dict(hess_u=None), ValueError,
     "rollout_riccati: hess_u is required (the diagonal of the control cost's Hessian, [T, B, n] or [n])"),
    ('rollout_riccati', dict(grad_q=z((T, B, n)), hess_q=z((B, n))), ValueError,
     'rollout_riccati: grad_q, grad_qd, hess_q and hess_qd must all be [2, 3, 7] or all [3, 7] (last step only), got [(2, 3, 7), (3, 7)]'),
    ('rollout_riccati', dict(grad_qd=z((T, B))), ValueError,
     'rollout_riccati: grad_q, grad_qd, hess_q and hess_qd must all be [2, 3, 7] or all [3, 7] (last step only), got [(2, 3)]'),
    ('rollout_riccati', dict(grad_u=z((B, n))), ValueError,
     'rollout_riccati: grad_u must be [2, 3, 7], got (3, 7)'),
    ('rollout_riccati', dict(hess_u=z((B, n))), ValueError,
     'rollout_riccati: hess_u must be [2, 3, 7] or [7] (shared by every row and step), got (3, 7)'),
    ('rollout_riccati', dict(reg=-1.0), ValueError,
     'rollout_riccati: reg must be finite and >= 0, got -1.0'),
    ('rollout_riccati', dict(reg=float('nan')), ValueError,
     'rollout_riccati: reg must be finite and >= 0, got nan'),
    ('rollout_riccati', dict(reg=float('inf')), ValueError,
     'rollout_riccati: reg must be finite and >= 0, got inf'),
    ('rollout_adjoint', dict(dc_du=z((T, B, n, n))), ValueError,
     'rollout_adjoint: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7, 7) and (2, 3, 7, 7)'),
    ('rollout_adjoint', dict(Minv=z((T, B, n, 2 * n))), ValueError,
     'rollout_adjoint: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7, 14) and (2, 3, 7, 14)'),
    ('rollout_adjoint', dict(dc_du=z((T, B, n))), ValueError,
     'rollout_adjoint: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7) and (2, 3, 7, 7)'),
    ('rollout_adjoint', dict(dc_du=z((0, B, n, 2 * n)), Minv=z((0, B, n, n))), ValueError,
     'rollout_adjoint: no step (T == 0)'),
    ('rollout_adjoint', dict(lam=z((B, n))), ValueError,
     'rollout_adjoint: lam must be [3, 14], got (3, 7)'),
    ('rollout_adjoint', dict(lam=z((B + 1, 2 * n))), ValueError,
     'rollout_adjoint: lam must be [3, 14], got (4, 14)'),
    ('rollout_riccati', dict(dc_du=z((T, B, n, n))), ValueError,
     'rollout_riccati: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7, 7) and (2, 3, 7, 7)'),
    ('rollout_riccati', dict(Minv=z((T, B, n, 2 * n))), ValueError,
     'rollout_riccati: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7, 14) and (2, 3, 7, 14)'),
    ('rollout_riccati', dict(dc_du=z((T, B, n))), ValueError,
     'rollout_riccati: dc_du must be [T, B, 7, 14] and Minv [T, B, 7, 7], got (2, 3, 7) and (2, 3, 7, 7)'),
    ('rollout_riccati', dict(dc_du=z((0, B, n, 2 * n)), Minv=z((0, B, n, n))), ValueError,
     'rollout_riccati: no step (T == 0)'),
    ('rollout_riccati', dict(lam=z((B, n))), ValueError,
     'rollout_riccati: lam must be [3, 14], got (3, 7)'),
    ('rollout_riccati', dict(lam=z((B + 1, 2 * n))), ValueError,
     'rollout_riccati: lam must be [3, 14], got (4, 14)'),
    ('rollout_riccati', dict(P=z((B, 2 * n))), ValueError,
     'rollout_riccati: P must be [3, 14, 14], got (3, 14)'),
    ('rollout_riccati', dict(dV=z((B,))), ValueError,
     'rollout_riccati: dV must be [3, 2], got (3,)'),
    ('rollout_riccati', dict(status=z((B, 1))), ValueError,
     'rollout_riccati: status must be [3], got (3, 1)'),
    ('rollout_riccati', dict(lam=z((B, 2 * n)), status=z(B + 1)), ValueError,
     'rollout_riccati: status must be [3], got (4,)'),
    ('rollout', dict(integrator='rk4', q0=z(n)), ValueError,
     "rollout: unknown integrator 'rk4'; use one of ['euler', 'semi_implicit']"),
    ('rollout_closed_loop', dict(u_min=1.0, alpha=[]), ValueError,
     'rollout_closed_loop: give u_min and u_max together, or neither'),
    ('rollout_cost', dict(u=z((0, 2, n)), alpha=[]), ValueError,
     'rollout_cost: u must be [T, B_nom, 7] (time-major) with B_nom dividing B = 3, got (0, 2, 7)'),
    ('rollout_cost', dict(alpha=[], row_alpha=z(B)), ValueError,
     'rollout_cost: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape (0,)'),
    ('rollout_cost', dict(k=z((T, B)), u_min=0.0), ValueError,
     'rollout_cost: k must be [2, 3, 7], got (2, 3)'),
    ('rollout_grad', dict(grad_q=None, q=z((T, B, n)), workspace_bytes=-1), ValueError,
     'rollout_grad: give grad_q, grad_qd or both (the gradient of the cost with respect to the trajectory)'),
    ('rollout_lqr', dict(hess_u=None, workspace_bytes=-1, qd=z((T, B, n))), ValueError,
     "rollout_lqr: hess_u is required (the diagonal of the control cost's Hessian, [T, B, n] or [n])"),
    ('rollout_riccati', dict(reg=-1.0, lam=z(B)), ValueError,
     'rollout_riccati: reg must be finite and >= 0, got -1.0'),
    ('mppi_update', dict(lam=z(B + 1), u_min=0.0), ValueError,
     'mppi_update: lam must be a float or [3], got shape (4,)'),
    ('mppi', dict(sigma=z((T, n + 1)), u_max=0.0), ValueError,
     'mppi: sigma must be a float, [7] or [2, 7], got shape (2, 8)'),
    ('ilqr', dict(iters=-1), ValueError,
     'ilqr: iters < 0'),
    ('ilqr', dict(alphas=[]), ValueError,
     'ilqr: alphas must be a non-empty 1-D sequence of step sizes'),
    ('ilqr', dict(reg=[0.0, 0.0], iters=3), ValueError,
     'ilqr: reg must be a float or a sequence of iters = 3 floats, got 2'),
    ('ilqr', dict(cost=None), TypeError,
     'ilqr: cost must be a QuadraticCost'),
    ('mppi', dict(iters=-1), ValueError,
     'mppi: iters < 0'),
    ('mppi', dict(samples=0), ValueError,
     'mppi: samples < 1'),
    ('mppi', dict(noise=z((1, T, S, B, n)), generator=torch.Generator()), ValueError,
     'mppi: give noise or generator, not both'),
    ('mppi', dict(noise=z((2, T, S, B, n))), ValueError,
     'mppi: noise must be [iters = 1, 2, S, 3, 7] with S > 0, got (2, 2, 4, 3, 7)'),
    ('mppi', dict(lam=z(B + 1)), ValueError,
     'mppi: lam must be a float or [3], got shape (4,)'),
    ('mppi', dict(q0=z((0, n)), qd0=z((0, n))), ValueError,
     'mppi: q0 and qd0 must both be [P, 7] with P > 0, got (0, 7) and (0, 7)'),
    ('mppi_update', dict(J=z((S, 0))), ValueError,
     'mppi_update: J must be [S, P] with S, P > 0, got (4, 0)'),
    ('mppi_update', dict(du=z((T, S, B + 1, n))), ValueError,
     'mppi_update: du must be [2, 4, 3, 7], got (2, 4, 4, 7)'),
    ('mppi_update', dict(lam=z((B, 1))), ValueError,
     'mppi_update: lam must be a float or [3], got shape (3, 1)'),
    ('rollout_cost', dict(cost=dict(w_q=1.0)), TypeError,
     'rollout_cost: cost must be a QuadraticCost'),
    ('rollout_cost', dict(return_final=True, return_trajectory=True), ValueError,
     "rollout_cost: give return_final or return_trajectory, not both (the final state is the trajectory's last slice)"),
    ('rollout', dict(differentiable=True), TypeError,
     'rollout: differentiable=True takes torch tensors (autograd does not see numpy arrays)'),
    ('mppi_update', dict(du=torch.zeros((T, S, B, n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi_update', dict(J=torch.zeros((S, B))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi_update', dict(J=torch.zeros((S, B)), du=torch.zeros((T, S, B, n)), u=torch.zeros((T, B, n))), RuntimeError,
     'inputs must live on a ROCm GPU (cuda device); no CPU fallback'),
    ('rollout_adjoint', dict(dc_du=torch.zeros((T, B, n, 2 * n))), RuntimeError,
     'inputs must live on a ROCm GPU (cuda device); no CPU fallback'),
    ('rollout_riccati', dict(dc_du=torch.zeros((T, B, n, 2 * n), dtype=torch.float16)), RuntimeError,
     'inputs must live on a ROCm GPU (cuda device); no CPU fallback'),
    ('ilqr', dict(cost=QuadraticCost(w_u=torch.ones(n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('ilqr', dict(u=torch.zeros((T, B, n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi', dict(cost=QuadraticCost(c_u=torch.ones(n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi', dict(noise=torch.zeros((1, T, S, B, n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi', dict(q0=torch.zeros((B, n)), qd0=torch.zeros((B, n)), u=torch.zeros((T, B, n)), noise=z((1, T, S, B, n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('mppi', dict(q0=torch.zeros((B, n))), TypeError,
     'mixing numpy and torch inputs is not supported'),
    ('rollout', dict(q0=torch.zeros((B, n)), qd0=torch.zeros((B, n))), RuntimeError,
     'inputs must live on a ROCm GPU (cuda device); no CPU fallback'),
]
NO_GPU_ROWS = [
    ('mppi_update', dict(), RuntimeError,
     'rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)'),
    ('rollout_adjoint', dict(), RuntimeError,
     'rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)'),
    ('rollout_riccati', dict(), RuntimeError,
     'rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)'),
    ('ilqr', dict(), RuntimeError,
     'rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)'),
    ('mppi', dict(), RuntimeError,
     'rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)'),
]
FLOATING_ROWS = [
    ('rollout', dict(), NotImplementedError,
     'rollout: fixed-base robots only (a floating base needs an integrator on SE(3))'),
    ('rollout_closed_loop', dict(), NotImplementedError,
     'rollout_closed_loop: fixed-base robots only (rollout has no floating base)'),
    ('rollout_cost', dict(), NotImplementedError,
     'rollout_cost: fixed-base robots only (rollout has no floating base)'),
    ('ilqr', dict(), NotImplementedError,
     'ilqr: fixed-base robots only (rollout has no floating base)'),
    ('mppi', dict(), NotImplementedError,
     'mppi: fixed-base robots only (rollout has no floating base)'),
    ('mppi_update', dict(), NotImplementedError,
     'mppi_update: fixed-base robots only (rollout has no floating base)'),
    ('rollout_grad', dict(), NotImplementedError,
     'rollout_grad: fixed-base robots only (rollout has no floating base)'),
    ('rollout_adjoint', dict(), NotImplementedError,
     'rollout_adjoint: fixed-base robots only (rollout has no floating base)'),
    ('rollout_lqr', dict(), NotImplementedError,
     'rollout_lqr: fixed-base robots only (rollout has no floating base)'),
    ('rollout_riccati', dict(), NotImplementedError,
     'rollout_riccati: fixed-base robots only (rollout has no floating base)'),
]


def test_every_refusal_keeps_its_exception_and_its_words():
    refused(bare_api(make_robot("iiwa_like")), good(), ROWS)


def test_a_floating_base_is_refused_by_every_method():
    api = bare_api(make_robot("fb_quadruped_like"))
    refused(api, good(api.nv), FLOATING_ROWS)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of numpy input on a machine without a GPU")
def test_numpy_input_without_a_gpu_is_refused():
    refused(bare_api(make_robot("iiwa_like")), good(), NO_GPU_ROWS)
