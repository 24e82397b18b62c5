"""fp64 numpy restatement of the reverse pass of ``RBDReference.rollout`` (``rollout_grad`` / ``rollout_adjoint``), on top
of ``oracle.rbd_oracle``'s ``aba``, ``rnea_grad`` and ``minv`` (checker only).

With ``lam = (lq | lqd) = 0``, for ``t = T-1 ... 0`` at the linearisation point ``(q_t, qd_t, u_t)``::

    lq += gq[t];  lqd += gqd[t];  w = lqd + dt lq
    mu = dt w (semi_implicit) | dt lqd (euler);   nu = Minv(q_t) mu;   grad_u[t] = nu
    lq = lq - dc_dq^T nu;  lqd = w - dc_dqd^T nu        [dc_dq | dc_dqd] = rnea_grad(q_t, qd_t, aba(q_t, qd_t, u_t))

Both forms also return, per row, the running magnitude ``S = max_t max(|lq|, |lqd|, |nu|)`` (max norm); called with the
absolute values of every input, the recursion with ``+`` for every ``-`` bounds what rounding can reach (``magnitude``)."""
import numpy as np

from oracle import rbd_oracle as orc
from rollout_oracle import INTEGRATORS


def _g(g, t, T, shape):
    """Slice ``t`` of a cost gradient given as ``[T, B, n]``, ``[B, n]`` (final slice only) or None."""
    if g is None:
        return np.zeros(shape)
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 3:
        return g[t]
    return g if t == T - 1 else np.zeros(shape)


def adjoint(dc_du, Minv, dt, gq=None, gqd=None, integrator="semi_implicit", lam=None, absolute=False):
    """The scan fed with a given linearisation: ``dc_du [T, B, n, 2n]``, ``Minv [T, B, n, n]`` ->
    ``(grad_u [T, B, n], lam [B, 2n], S [B])``.  ``absolute=True``: every subtraction becomes an addition (the
    non-negative recursion of the error bound; the caller passes absolute values)."""
    if integrator not in INTEGRATORS:
        raise ValueError(integrator)
    dc_du = np.asarray(dc_du, dtype=np.float64)
    Minv = np.asarray(Minv, dtype=np.float64)
    T, B, n = dc_du.shape[:3]
    lam = np.zeros((B, 2 * n)) if lam is None else np.array(lam, dtype=np.float64)
    lq, lqd = lam[:, :n].copy(), lam[:, n:].copy()
    grad_u = np.zeros((T, B, n))
    S = np.zeros(B)
    sgn = 1.0 if absolute else -1.0
    for t in range(T - 1, -1, -1):
        lq = lq + _g(gq, t, T, (B, n))
        lqd = lqd + _g(gqd, t, T, (B, n))
        w = lqd + dt * lq
        mu = dt * (w if integrator == "semi_implicit" else lqd)
        nu = np.einsum("blj,bl->bj", Minv[t], mu)
        grad_u[t] = nu
        S = np.maximum(S, np.max(np.abs(np.concatenate([lq, lqd, w, nu], axis=1)), axis=1))
        back = np.einsum("bic,bi->bc", dc_du[t], nu)
        lq = lq + sgn * back[:, :n]
        lqd = w + sgn * back[:, n:]
        S = np.maximum(S, np.max(np.abs(np.concatenate([lq, lqd], axis=1)), axis=1))
    return grad_u, np.concatenate([lq, lqd], axis=1), S


def magnitude(dc_du, Minv, dt, gq=None, gqd=None, integrator="semi_implicit", lam=None):
    """``S-bar [B]``: ``S`` of the recursion with every input replaced by its absolute value and no cancellation."""
    a = lambda x: None if x is None else np.abs(np.asarray(x, dtype=np.float64))
    return adjoint(a(dc_du), a(Minv), abs(dt), a(gq), a(gqd), integrator, a(lam), absolute=True)[2]


def linearise(om, q0, qd0, u, q_traj, qd_traj, GRAVITY=-9.81):
    """``dc_du [T, B, n, 2n]`` and ``Minv [T, B, n, n]`` at the linearisation points of a stored trajectory: step 0 at
    ``(q0, qd0, u[0])``, step ``t >= 1`` at ``(q_traj[t-1], qd_traj[t-1], u[t])``."""
    u = np.asarray(u, dtype=np.float64)
    T = u.shape[0]
    qs = np.concatenate([np.asarray(q0, dtype=np.float64)[None], np.asarray(q_traj, dtype=np.float64)[:T - 1]])
    qds = np.concatenate([np.asarray(qd0, dtype=np.float64)[None], np.asarray(qd_traj, dtype=np.float64)[:T - 1]])
    dc, Mi = [], []
    for t in range(T):
        ut = np.broadcast_to(u[t], qs[t].shape)
        qdd = orc.aba(om, qs[t], qds[t], ut, GRAVITY=GRAVITY)
        dc.append(orc.rnea_grad(om, qs[t], qds[t], qdd, GRAVITY=GRAVITY))
        Mi.append(orc.minv(om, qs[t]))
    return np.stack(dc), np.stack(Mi)


def rollout_grad(om, q0, qd0, u, dt, gq=None, gqd=None, GRAVITY=-9.81, integrator="semi_implicit", q_traj=None, qd_traj=None):
    """The evaluating form -> ``(grad_u [T, B, n], grad_q0 [B, n], grad_qd0 [B, n], S [B])``.  ``q_traj, qd_traj``: the
    stored trajectory to linearise along (teacher forcing); the oracle's own rollout when omitted."""
    if q_traj is None:
        from rollout_oracle import rollout
        q_traj, qd_traj = rollout(om, q0, qd0, u, dt, GRAVITY, integrator)
    dc, Mi = linearise(om, q0, qd0, u, q_traj, qd_traj, GRAVITY)
    n = dc.shape[2]
    grad_u, lam, S = adjoint(dc, Mi, dt, gq, gqd, integrator)
    return grad_u, lam[:, :n], lam[:, n:], S
