"""fp64 numpy restatement of ``RBDReference.rollout_cost`` (checker only): ``rollout_closed_loop_oracle``'s time loop, open
or closed loop, with the per-row perturbation ``du``, and the quadratic cost of ``rbdreference_amd.cost`` summed from a
trajectory -- together with the sum of the absolute values of its terms, which the GPU tests' rounding bound needs."""
import numpy as np

from rollout_closed_loop_oracle import control
from rollout_oracle import step

KEYS = ("w_q", "w_qd", "q_target", "qd_target", "w_u", "c_u")


def cost_arrays(p):
    """``ilqr_problem``'s dict in the names of ``QuadraticCost``."""
    return dict(w_q=p["hq"], w_qd=p["hqd"], q_target=p["tq"], qd_target=p["tqd"], w_u=p["hu"], c_u=p["cu"])


def draw_cost(rng, T, B, n, final=False):
    """Cost arrays drawn like ``ilqr_problem``'s: Hessians 5 .. 15 (state) and 1 .. 2 (control), targets and ``c_u`` in
    -1 .. 1; the four state arrays ``[B, n]`` with ``final``."""
    xs = (B, n) if final else (T, B, n)
    return dict(w_q=rng.uniform(5, 15, xs), w_qd=rng.uniform(5, 15, xs), q_target=rng.uniform(-1, 1, xs),
                qd_target=rng.uniform(-1, 1, xs), w_u=rng.uniform(1, 2, (T, B, n)), c_u=rng.uniform(-1, 1, (T, B, n)))


def cost_of_trajectory(c, q, qd, u, final=False):
    """``c``: the six arrays (``None`` = absent) with ``B_nom`` rows; ``q, qd, u [T, B, n]`` with ``B`` a multiple of
    ``B_nom`` (row r reads row r % B_nom) -> ``(J [B], mag [B])``: the cost and the sum of the absolute values of its
    ``4 n T`` terms."""
    T, B, n = u.shape
    tile = lambda a: None if a is None else np.tile(np.asarray(a, dtype=np.float64), (1,) * (np.ndim(a) - 2) + (B // np.shape(a)[-2], 1))   # noqa: E731
    c = {key: tile(c.get(key)) for key in KEYS}
    J, mag = np.zeros(B), np.zeros(B)

    def add(term):
        nonlocal J, mag
        ax = tuple(range(term.ndim - 2)) + (term.ndim - 1,)
        J = J + term.sum(axis=ax)
        mag = mag + np.abs(term).sum(axis=ax)

    if c["w_u"] is not None:
        add(0.5 * c["w_u"] * u * u)
    if c["c_u"] is not None:
        add(c["c_u"] * u)
    for w, tg, x in (("w_q", "q_target", q), ("w_qd", "qd_target", qd)):
        if c[w] is None:
            continue
        xs = x[-1] if final else x
        e = xs if c[tg] is None else xs - c[tg]
        add(0.5 * c[w] * e * e)
    return J, mag


def rollout_cost(om, q0, qd0, u, dt, c, K=None, q_ref=None, qd_ref=None, k=None, alpha=1.0, du=None, q0_ref=None, qd0_ref=None,
                 u_min=None, u_max=None, GRAVITY=-9.81, integrator="semi_implicit", final=False):
    """``q0, qd0 [B, n]``; the nominal (``u, k, K``, the reference, the cost) has ``B_nom`` rows, ``B_nom`` dividing ``B``;
    ``du [T, B, n]``; ``alpha``: a float or ``[B]`` -> ``(J [B], q, qd, u_applied [T, B, n])``."""
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    B, n = q.shape
    u = np.asarray(u, dtype=np.float64)
    T, Bn = u.shape[:2]
    rep = B // Bn
    nom = lambda a: None if a is None else np.tile(np.asarray(a, dtype=np.float64), (rep,) + (1,) * (np.ndim(a) - 1))   # noqa: E731  [Bn, ..] -> [B, ..]
    al = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (B,))
    zK = np.zeros((B, n, 2 * n))
    xref = None
    if K is not None:
        xref = np.concatenate([q if q0_ref is None else nom(q0_ref), qd if qd0_ref is None else nom(qd0_ref)], axis=-1)
    qs, qds, us = [], [], []
    for t in range(T):
        x = np.concatenate([q, qd], axis=-1)
        if K is not None and t > 0:
            xref = np.concatenate([nom(q_ref[t - 1]), nom(qd_ref[t - 1])], axis=-1)
        ub = nom(u[t]) + (0.0 if du is None else np.asarray(du[t], dtype=np.float64))
        ut, _ = control(x, x if K is None else xref, ub, zK if K is None else nom(K[t]), None if k is None else nom(k[t]), al, u_min, u_max)
        q, qd, _ = step(om, q, qd, ut, dt, GRAVITY, integrator)
        qs.append(q)
        qds.append(qd)
        us.append(ut)
    q, qd, ua = np.stack(qs), np.stack(qds), np.stack(us)
    return cost_of_trajectory(c, q, qd, ua, final)[0], q, qd, ua
