"""fp64 numpy restatement of ``RBDReference.rollout_closed_loop``: the time loop of ``rollout_oracle`` with the control law
``u_t = ubar[t] + alpha k[t] + K[t] (x_t - xref_t)`` in front of every step (checker only), and the one-step control the
teacher-forced GPU checks use."""
import numpy as np

from rollout_oracle import step


def control(x, xref, ubar, K, k=None, alpha=None, u_min=None, u_max=None):
    """``x, xref [R, 2n]``, ``ubar [R, n]``, ``K [R, n, 2n]``, ``k [R, n]`` or None, ``alpha [R]`` -> ``(u [R, n],
    mag [R, n])``: the control of one step and the sum of the absolute values of its terms (for rounding bounds).  The
    clip is the kernel's: ordered comparisons, so a NaN stays a NaN."""
    dx = x - xref
    u = np.array(ubar, dtype=np.float64)
    mag = np.abs(u)
    if k is not None:
        ff = np.asarray(alpha, dtype=np.float64)[:, None] * k
        u = u + ff
        mag = mag + np.abs(ff)
    u = u + np.einsum("rjc,rc->rj", K, dx)
    mag = mag + np.einsum("rjc,rc->rj", np.abs(K), np.abs(dx))
    if u_min is not None:
        lo, hi = np.broadcast_to(u_min, u.shape), np.broadcast_to(u_max, u.shape)
        u = np.where(u < lo, lo, np.where(u > hi, hi, u))
    return u, mag


def rollout_closed_loop(om, q0, qd0, u, q_ref, qd_ref, K, dt, k=None, alpha=1.0, q0_ref=None, qd0_ref=None, u_min=None,
                        u_max=None, GRAVITY=-9.81, integrator="semi_implicit", trajectory=True):
    """Batched form of the API: ``q0, qd0 [B, n]``, ``u, q_ref, qd_ref, k [T, B, n]``, ``K [T, B, n, 2n]`` ->
    ``(q, qd, u_applied)``.  A float ``alpha`` gives ``[T, B, n]``; a 1-D ``alpha`` of length ``A`` runs every step size
    against the shared nominal and gives ``[T, A, B, n]`` (final state ``[B, n]`` / ``[A, B, n]`` with
    ``trajectory=False``; ``u_applied`` always has the time axis)."""
    if np.ndim(alpha) == 1:
        outs = [rollout_closed_loop(om, q0, qd0, u, q_ref, qd_ref, K, dt, k, float(a), q0_ref, qd0_ref, u_min, u_max, GRAVITY,
                                    integrator, trajectory) for a in alpha]
        return tuple(np.stack([o[i] for o in outs], axis=-3) for i in range(3))
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    B = q.shape[0]
    u, q_ref, qd_ref, K = (np.asarray(x, dtype=np.float64) for x in (u, q_ref, qd_ref, K))
    xref = np.concatenate([q if q0_ref is None else np.asarray(q0_ref, dtype=np.float64),
                           qd if qd0_ref is None else np.asarray(qd0_ref, dtype=np.float64)], axis=-1)
    al = np.full(B, float(alpha))
    qs, qds, us = [], [], []
    for t in range(u.shape[0]):
        if t > 0:
            xref = np.concatenate([q_ref[t - 1], qd_ref[t - 1]], axis=-1)
        ut, _ = control(np.concatenate([q, qd], axis=-1), xref, u[t], K[t], None if k is None else np.asarray(k[t], dtype=np.float64),
                        al, u_min, u_max)
        q, qd, _ = step(om, q, qd, ut, dt, GRAVITY, integrator)
        qs.append(q)
        qds.append(qd)
        us.append(ut)
    if not trajectory:
        return q, qd, np.stack(us)
    return np.stack(qs), np.stack(qds), np.stack(us)


# ---- the quadratic tracking problem of the end-to-end cost checks (host and GPU) ---------------------------------------
def ilqr_problem(n, B=3, T=5):
    """Inputs and cost model drawn from ``default_rng(7 + n)`` in a fixed order: ``q0, qd0, u``, the diagonal Hessians
    ``hq, hqd`` (5 .. 15) and ``hu`` (1 .. 2), the targets ``tq, tqd`` and a linear control term ``cu``."""
    rng = np.random.default_rng(7 + n)
    p = dict(q0=rng.uniform(-np.pi, np.pi, (B, n)), qd0=rng.uniform(-1, 1, (B, n)), u=rng.uniform(-5, 5, (T, B, n)),
             hq=rng.uniform(5, 15, (T, B, n)), hqd=rng.uniform(5, 15, (T, B, n)), hu=rng.uniform(1, 2, (T, B, n)),
             tq=rng.uniform(-1, 1, (T, B, n)), tqd=rng.uniform(-1, 1, (T, B, n)), cu=rng.uniform(-1, 1, (T, B, n)))
    return p


def cost(p, q, qd, u):
    """``J`` per row of a trajectory ``q, qd, u [T, ..., B, n]`` (extra axes between T and B broadcast)."""
    ex = (slice(None),) + (None,) * (q.ndim - 3)
    w = lambda a: a[ex]
    J = 0.5 * w(p["hq"]) * (q - w(p["tq"])) ** 2 + 0.5 * w(p["hqd"]) * (qd - w(p["tqd"])) ** 2 + 0.5 * w(p["hu"]) * u ** 2 + w(p["cu"]) * u
    return J.sum(axis=(0, -1))


def cost_model(p, q, qd, u):
    """The cost's gradients and Hessians at a nominal trajectory ``q, qd, u [T, B, n]``, named as ``rollout_lqr`` names them."""
    return dict(gq=p["hq"] * (q - p["tq"]), gqd=p["hqd"] * (qd - p["tqd"]), hq=p["hq"], hqd=p["hqd"],
                gu=p["hu"] * u + p["cu"], hu=p["hu"])


def predicted_ratio(J0, J, alphas, dV):
    """``dJ / (alpha dV[0] + alpha^2 dV[1]) - 1`` for ``J [A, B]`` against the nominal's ``J0 [B]``, ``dV [B, 2]``."""
    a = np.asarray(alphas, dtype=np.float64)[:, None]
    return (J - J0[None]) / (a * dV[None, :, 0] + a * a * dV[None, :, 1]) - 1.0
