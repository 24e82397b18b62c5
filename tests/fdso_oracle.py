"""Batched numpy restatement of the reference's second-order forward-dynamics derivatives (test helper, not product code).

Restates ``RBDReference.fdsva_so`` (``RBDReference.py:1606-1631``) over a batch of configurations, composed from the
first-order oracle (oracle/rbd_oracle.py) and the second-order inverse-dynamics restatement (tests/so_oracle.py):

    Minv = minv(q);  qdd = Minv (u - c(q, qd));  [fd_dq | fd_dqd] = -Minv rnea_grad(q, qd, qdd)
    d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq = second_order_idsva(q, qd, qdd)
    daba_dqdq[i,j,k] = -sum_l Minv[i,l] (d2tau_dq[l,j,k] + sum_m dM_dq[l,m,k] fd_dq[m,j] + sum_m dM_dq[l,m,j] fd_dq[m,k])
    daba_dvdq[i,j,k] = -sum_l Minv[i,l] (d2tau_dvdq[l,j,k] + sum_m dM_dq[l,m,k] fd_dqd[m,j])
    daba_dvdv[i,j,k] = -sum_l Minv[i,l] d2tau_dqd[l,j,k]
    daba_dtdq[i,j,k] = -sum_l Minv[i,l] sum_m dM_dq[l,m,k] Minv[m,j]

Two things differ from the reference as written.  ``GRAVITY`` is carried through every stage (the reference passes it to
``second_order_idsva_parallel`` only and evaluates forward dynamics at -9.81, :1621-1623; at the default the two agree).
And the second-order inverse-dynamics tensors are tests/so_oracle.py's, whose composite-force sweep adds the child's
force (``fix_f=True``); ``fix_f=False`` restates the reference's :1448 and reproduces its ``daba_dqdq`` on branched robots.
"""
import numpy as np

from oracle import rbd_oracle as orc
from so_oracle import second_order_idsva


def contract(Minv, fd_dq, fd_dqd, d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq):
    """The pure contraction (:1625-1629), batched over leading axes: -> (daba_dqdq, daba_dvdq, daba_dvdv, daba_dtdq)."""
    Eq = np.einsum("...lmk,...mj->...ljk", dM_dq, fd_dq)
    Ev = np.einsum("...lmk,...mj->...ljk", dM_dq, fd_dqd)
    Em = np.einsum("...lmk,...mj->...ljk", dM_dq, Minv)
    neg = lambda X: -np.einsum("...il,...ljk->...ijk", Minv, X)      # noqa: E731
    return neg(d2tau_dq + Eq + np.swapaxes(Eq, -1, -2)), neg(d2tau_dvdq + Ev), neg(d2tau_dqd), neg(Em)


def ingredients(m, q, qd, u, GRAVITY=-9.81, fix_f=True):
    """-> (Minv, qdd, fd_dq, fd_dqd, d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq) of a batch ``[B, n]``, one gravity throughout."""
    n = q.shape[-1]
    c = orc.rnea(m, q, qd, None, GRAVITY)[0]
    Minv = orc.minv(m, q)
    qdd = np.einsum("...ij,...j->...i", Minv, u - c)
    dc_du = orc.rnea_grad(m, q, qd, qdd, GRAVITY)
    fd = -np.einsum("...ij,...jk->...ik", Minv, dc_du)
    so = second_order_idsva(m, q, qd, qdd, GRAVITY, fix_f)
    return (Minv, qdd, fd[..., :n], fd[..., n:]) + tuple(so)


def fdsva_so(m, q, qd, u, GRAVITY=-9.81, fix_f=True):
    """-> (daba_dqdq, daba_dvdq, daba_dvdv, daba_dtdq), each ``[B, n, n, n]`` (``(n, n, n)`` for one configuration)."""
    q = np.asarray(q, dtype=np.float64); qd = np.asarray(qd, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    un = q.ndim == 1
    if un:
        q, qd, u = q[None], qd[None], u[None]
    Minv, _, fd_dq, fd_dqd, d2q, d2qd, d2vq, dM = ingredients(m, q, qd, u, GRAVITY, fix_f)
    out = contract(Minv, fd_dq, fd_dqd, d2q, d2qd, d2vq, dM)
    return tuple(x[0] for x in out) if un else out


class FDSOOracle:
    def __init__(self, robot):
        self.robot = robot
        self.m = orc.model_from_robot(robot)

    def __call__(self, q, qd, u, GRAVITY=-9.81, fix_f=True):
        return fdsva_so(self.m, q, qd, u, GRAVITY, fix_f)


def has_prismatic(robot):
    return bool(np.any(orc.model_from_robot(robot).prismatic))


def n_samples(n):
    """Samples per fixture: 8 for n <= 9, 4 for 12 <= n <= 18, 2 beyond (the 30-body robot)."""
    return 8 if n <= 9 else 4 if n <= 18 else 2
