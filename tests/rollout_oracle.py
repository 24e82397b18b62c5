"""fp64 numpy restatement of ``RBDReference.rollout``: a time loop over ``oracle.rbd_oracle.aba`` with the two
integrators of include/rbd_hip.h, and the one-step form the teacher-forced GPU checks use (checker only)."""
import numpy as np

from oracle import rbd_oracle as orc

INTEGRATORS = ("semi_implicit", "euler")


def step(om, q, qd, u, dt, GRAVITY=-9.81, integrator="semi_implicit"):
    """One step from ``(q, qd) [B, n]`` under ``u [B, n]`` -> ``(q', qd', qdd)``."""
    if integrator not in INTEGRATORS:
        raise ValueError(integrator)
    q = np.asarray(q, dtype=np.float64)
    qd = np.asarray(qd, dtype=np.float64)
    qdd = orc.aba(om, q, qd, np.broadcast_to(np.asarray(u, dtype=np.float64), q.shape), GRAVITY=GRAVITY)
    qd_new = qd + dt * qdd
    q_new = q + dt * (qd_new if integrator == "semi_implicit" else qd)
    return q_new, qd_new, qdd


def rollout(om, q0, qd0, u, dt, GRAVITY=-9.81, integrator="semi_implicit", trajectory=True):
    """``q0, qd0 [B, n]``, ``u [T, B, n]`` or ``[T, n]`` (time-major) -> ``(q, qd)``, ``[T, B, n]`` with slice ``t`` the
    state after step ``t + 1``, or the final state ``[B, n]``."""
    q = np.array(q0, dtype=np.float64)
    qd = np.array(qd0, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    qs, qds = [], []
    for t in range(u.shape[0]):
        q, qd, _ = step(om, q, qd, u[t], dt, GRAVITY, integrator)
        qs.append(q)
        qds.append(qd)
    if not trajectory:
        return q, qd
    return np.stack(qs), np.stack(qds)


def rest_bounds(om, q0, T, dt, tol, GRAVITY=-9.81):
    """Bounds on ``|qd_t|`` and ``|q_t - q0|`` (``t = 1..T``, ``[T, B]``) for a rollout that starts at rest under the
    gravity-compensating ``u = rnea(q0, 0, 0)[0]``: the compensation leaves an acceleration of at most aba's own
    tolerance ``tol`` times the uncompensated acceleration ``aba(q0, 0, 0)``, which a step integrates once into qd and
    twice into q."""
    z = np.zeros_like(q0)
    a_free = np.max(np.abs(orc.aba(om, q0, z, z, GRAVITY=GRAVITY)), axis=-1)           # [B]
    t = np.arange(1, T + 1, dtype=np.float64)[:, None]
    return t * dt * tol * a_free[None], t * t * dt * dt * tol * a_free[None]
