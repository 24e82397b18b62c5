"""GPU tests of the store policy of the one-lane chain gradient kernels (run with ``-m gpu``).

`RBD_OPT_STORE_POLICY` (include/rbd_hip.h) only changes HOW the finished rows leave -- plain 16-byte stores, or
write-through ones (with or without the non-temporal hint) issued through a buffer descriptor that bounds each
half-tile (rbd_spatial.h, store16) -- never what is written.  So for every kernel that takes the policy (rnea_grad_idsva_pipe_kernel<float>, its
forward_dynamics_grad variant, rnea_grad_idsva_kernel<double>):

  * the forced policies give bit-identical `c` and `dc_du` (torch.equal),
  * a sample of at most 256 rows equals the oracle at the suite's bounds (1e-5 fp32, 1e-11 fp64, normwise per tensor;
    forward_dynamics_grad in fp32: the suite's per-row bound 8 eps32 cond(H)),
  * outputs carved out of a larger buffer leave the canary words before and after them untouched.

Batches: the edges of a 64-row tile (1, 63, 64, 65, 129), and one batch whose blocks walk three tiles and end on a
ragged one (393 253 rows = 6 145 tiles over the 2 048 resident waves), which is the only place the pipelined flush,
the last-tile flush and the ragged tail all run in one launch.
"""
import numpy as np
import pytest

from conftest import make_robot, rel_err

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 1e-5, 1e-11
CANARY = -1.2345e33
PAD = 64                      # canary scalars on either side (a multiple of 16 bytes in both precisions)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


_STATE = {}


def iiwa():
    if "rbd" not in _STATE:
        from oracle import rbd_oracle as orc
        from rbdreference_amd import RBDReference
        robot = make_robot("iiwa_like")
        _STATE["rbd"] = RBDReference(robot, build=False, generic="never")
        _STATE["om"] = orc.model_from_robot(robot)
    from oracle import rbd_oracle as orc
    return _STATE["rbd"], orc, _STATE["om"]


def inputs(B, dt, seed=0):
    """(numpy fp64 inputs as the kernel sees them, device tensors)"""
    torch = _torch()
    rng = np.random.default_rng(seed)
    npdt = np.float32 if dt == torch.float32 else np.float64
    xs = [rng.uniform(-np.pi, np.pi, (B, 7)).astype(npdt), rng.uniform(-1, 1, (B, 7)).astype(npdt), rng.uniform(-1, 1, (B, 7)).astype(npdt)]
    return [x.astype(np.float64) for x in xs], [torch.tensor(x, device="cuda:0") for x in xs]


def sample_rows(B):
    """At most 256 rows: the first and last 64 and the rows around tile boundaries in between."""
    if B <= 256:
        return np.arange(B)
    mid = np.linspace(64, B - 65, 128).astype(np.int64)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(B - 64, B)]))


def POLICIES():
    from rbdreference_amd import _lib as L
    return (L.RBD_STORE_POLICY_PLAIN, L.RBD_STORE_POLICY_WRITE_THROUGH, L.RBD_STORE_POLICY_WRITE_THROUGH_NT)


class forced:
    """the chain kernel at every batch size (AUTO serves small batches with the column kernel), one store policy"""

    def __init__(self, rbd, policy):
        self.rbd, self.policy = rbd, policy

    def __enter__(self):
        from rbdreference_amd import _lib as L
        self.rbd._lib.set_option(L.RBD_OPT_GRAD_KERNEL, L.RBD_GRAD_KERNEL_BATCH)
        self.rbd._lib.set_option(L.RBD_OPT_STORE_POLICY, self.policy)

    def __exit__(self, *exc):
        from rbdreference_amd import _lib as L
        self.rbd._lib.set_option(L.RBD_OPT_GRAD_KERNEL, L.RBD_GRAD_KERNEL_AUTO)
        self.rbd._lib.set_option(L.RBD_OPT_STORE_POLICY, L.RBD_STORE_POLICY_AUTO)
        return False


def carved(B, dt):
    """c [B, 7] and dc_du [B, 7, 14] inside larger canary-filled buffers; returns (c, dc, check)"""
    torch = _torch()
    bc = torch.full((PAD + B * 7 + PAD,), CANARY, device="cuda:0", dtype=dt)
    bd = torch.full((PAD + B * 98 + PAD,), CANARY, device="cuda:0", dtype=dt)
    c = bc[PAD:PAD + B * 7].view(B, 7)
    dc = bd[PAD:PAD + B * 98].view(B, 7, 14)
    want = torch.full((PAD,), CANARY, device="cuda:0", dtype=dt)

    def check(what):
        for nm, buf in (("c", bc), ("dc_du", bd)):
            assert torch.equal(buf[:PAD], want), f"{what}: words BEFORE {nm} were overwritten"
            assert torch.equal(buf[-PAD:], want), f"{what}: words AFTER {nm} were overwritten"
    return c, dc, check


def both_policies(B, dt, kernel_part, qdd=True, damping=False):
    """rnea_grad under every forced policy into carved buffers; asserts what the module docstring lists"""
    torch = _torch()
    from rbdreference_amd import _lib as L
    rbd, orc, om = iiwa()
    (q, qd, qdd_np), (tq, tqd, tqdd) = inputs(B, dt, seed=B % 1000)
    res = []
    for pol in POLICIES():
        c, dc, check = carved(B, dt)
        with forced(rbd, pol):
            assert kernel_part in rbd._lib.kernel_name(L.RBD_OP_RNEA_GRAD, 4 if dt == torch.float32 else 8, B)
            rbd.rnea_grad(tq, tqd, tqdd if qdd else None, USE_VELOCITY_DAMPING=damping, return_c=True, out=(c, dc))
            torch.cuda.synchronize()
        check(f"policy {pol}, B = {B}")
        res.append((c, dc))
    (c0, dc0), (c1, dc1) = res[0], res[-1]
    for k, (cw, dcw) in enumerate(res[1:]):
        assert torch.equal(c0, cw), f"c differs between PLAIN and store policy {POLICIES()[k + 1]}, B = {B}"
        assert torch.equal(dc0, dcw), f"dc_du differs between PLAIN and store policy {POLICIES()[k + 1]}, B = {B}"
    rows = sample_rows(B)
    c_ref, dc_ref = orc.rnea_grad(om, q[rows], qd[rows], qdd_np[rows] if qdd else None, USE_VELOCITY_DAMPING=damping, return_c=True)
    tol = TOL32 if dt == torch.float32 else TOL64
    tr = torch.as_tensor(rows, device="cuda:0")
    e_c, e_dc = rel_err(c1[tr].double().cpu().numpy(), c_ref), rel_err(dc1[tr].double().cpu().numpy(), dc_ref)
    print(f"B = {B}: c {e_c:.2e}  dc_du {e_dc:.2e}  (bound {tol:g})")
    assert e_c <= tol and e_dc <= tol, (B, e_c, e_dc)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 129, 393253])
def test_rnea_grad_f32_policies_agree_bit_for_bit(B):
    torch = _torch()
    both_policies(B, torch.float32, "rnea_grad_idsva_pipe_kernel<float")


@pytest.mark.parametrize("variant", ["qdd_none", "damped"])
def test_rnea_grad_f32_variants_policies_agree_bit_for_bit(variant):
    torch = _torch()
    both_policies(65, torch.float32, "rnea_grad_idsva_pipe_kernel<float", qdd=variant != "qdd_none", damping=variant == "damped")


def test_rnea_grad_f64_chain_kernel_policies_agree_bit_for_bit():
    torch = _torch()
    both_policies(65, torch.float64, "rnea_grad_idsva_kernel<double")


@pytest.mark.parametrize("B", [65, 129])
def test_forward_dynamics_grad_f32_policies_agree_bit_for_bit(B):
    torch = _torch()
    from rbdreference_amd import _lib as L
    rbd, orc, om = iiwa()
    (q, qd, u), (tq, tqd, tu) = inputs(B, torch.float32, seed=7 + B)
    res = []
    # through the C-ABI, as RBDReference.forward_dynamics_grad calls it, but with the [B, 7, 14] result carved out of a
    # canary-filled buffer (the Python API allocates its own).  Which gradient kernel runs is fixed when the library is
    # compiled (one chain, fp32: fd_pre_kernel<float> + rnea_grad_idsva_pipe_kernel<float,true,true>, rbd_kernels.hip);
    # rbd_kernel_name has no op for this entry point, so there is nothing to query or to force.
    lib = rbd._lib.resolve("rbd_forward_dynamics_grad", "f32")
    assert not getattr(lib, "is_generic", False)
    wsb = int(lib.rbd_fd_workspace_bytes(B, 4))
    ws = torch.empty((max(wsb, 1),), device="cuda:0", dtype=torch.uint8)
    qdd = torch.empty((B, 7), device="cuda:0", dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    want = torch.full((PAD,), CANARY, device="cuda:0", dtype=torch.float32)
    for pol in POLICIES():
        buf = torch.full((PAD + B * 98 + PAD,), CANARY, device="cuda:0", dtype=torch.float32)
        d = buf[PAD:PAD + B * 98].view(B, 7, 14)
        with forced(rbd, pol):
            rbd._lib.check(lib.rbd_forward_dynamics_grad_f32(tq.data_ptr(), tqd.data_ptr(), tu.data_ptr(), -9.81, B, qdd.data_ptr(),
                                                             d.data_ptr(), ws.data_ptr(), wsb, st))
            torch.cuda.synchronize()
        assert torch.equal(buf[:PAD], want) and torch.equal(buf[-PAD:], want), f"policy {pol}, B = {B}: words around the result were overwritten"
        res.append((d[:, :, :7].contiguous(), d[:, :, 7:].contiguous()))
    a_api, b_api = rbd.forward_dynamics_grad(tq, tqd, tu)
    assert torch.equal(a_api.contiguous(), res[0][0]) and torch.equal(b_api.contiguous(), res[0][1])
    for k, (aw, bw) in enumerate(res[1:]):
        assert torch.equal(res[0][0], aw) and torch.equal(res[0][1], bw), f"forward_dynamics_grad differs between PLAIN and store policy {POLICIES()[k + 1]}, B = {B}"
    # the suite's fp32 bound for this entry point (tests/test_gpu_parity.py, check_conditioned): the result is multiplied by
    # Minv, so a row's forward error is bounded by slack * eps32 * cond(H) of that row, slack = 8; the flat 1e-5 of
    # rnea_grad does not apply (measured here: 1.97e-5 / 1.52e-5 normwise at B = 65, the same bits under either policy)
    r1, r2 = orc.forward_dynamics_grad(om, q, qd, u)
    bound = 8.0 * np.finfo(np.float32).eps * np.array([np.linalg.cond(h) for h in orc.crba(om, q)])
    for nm, got, want in (("dq", res[-1][0], r1), ("dqd", res[-1][1], r2)):
        got = got.double().cpu().numpy().reshape(B, -1); want = np.asarray(want).reshape(B, -1)
        err = np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)
        worst = float(np.max(err / bound))
        print(f"forward_dynamics_grad B = {B} {nm}: worst error / (8 eps32 cond(H)) = {worst:.3f}  (max error {err.max():.2e})")
        assert worst <= 1.0, (B, nm, worst)
