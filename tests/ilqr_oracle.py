"""fp64 numpy restatement of ``RBDReference.ilqr`` (checker only), built from the existing oracles: per iteration the cost
model at the nominal, ``rollout_lqr_oracle``'s backward pass, one closed-loop rollout per step size, the per-row choice and
the explicit accept / reject selection."""
from collections import namedtuple

import numpy as np

from rollout_closed_loop_oracle import cost, cost_model, rollout_closed_loop
from rollout_lqr_oracle import rollout_lqr
from rollout_oracle import rollout

ALPHAS = (1, .5, .25, .125, .03125, .0078125)
IlqrOracle = namedtuple("IlqrOracle", ["u", "q", "qd", "cost", "alpha", "dV", "status", "candidates"])


def choose(Jc, J, alphas):
    """``Jc [A, B]``, ``J [B]`` -> ``(J_best, index, accept, row_alpha)``: the lowest-index minimum with a NaN counted as
    +inf; a row accepts when that minimum is below its cost, and a rejected row's step size is 0."""
    Jc = np.where(np.isnan(Jc), np.inf, Jc)
    idx = np.argmin(Jc, axis=0)                       # numpy: the first occurrence
    J_best = np.take_along_axis(Jc, idx[None], axis=0)[0]
    accept = J_best < J
    return J_best, idx, accept, np.where(accept, np.asarray(alphas, dtype=np.float64)[idx], 0.0)


def ilqr(om, p, iters, alphas=ALPHAS, reg=0.0, dt=0.01, integrator="semi_implicit"):
    """``p``: ``ilqr_problem``'s dict -> the history of ``RBDReference.ilqr`` plus the candidates ``Jc [iters, A, B]``."""
    q0, qd0, u = p["q0"], p["qd0"], p["u"]
    q, qd = rollout(om, q0, qd0, u, dt, integrator=integrator)
    J = cost(p, q, qd, u)
    hist, h_al, h_dV, h_st, h_c = [J], [], [], [], []
    for _ in range(iters):
        k, K, _, _, dV, status = rollout_lqr(om, q0, qd0, u, dt, q, qd, integrator=integrator, reg=reg, **cost_model(p, q, qd, u))
        qa, qda, ua = rollout_closed_loop(om, q0, qd0, u, q, qd, K, dt, k=k, alpha=[float(a) for a in alphas], integrator=integrator)
        Jc = cost(p, qa, qda, ua)
        J_best, idx, accept, ra = choose(Jc, J, alphas)
        sel = accept[None, :, None]
        pick = lambda x: np.take_along_axis(x, idx[None, None, :, None], axis=1)[:, 0]      # noqa: E731  [T, A, B, n] -> [T, B, n]
        u, q, qd = np.where(sel, pick(ua), u), np.where(sel, pick(qa), q), np.where(sel, pick(qda), qd)
        J = np.where(accept, J_best, J)
        hist.append(J)
        h_al.append(ra)
        h_dV.append(dV)
        h_st.append(status)
        h_c.append(Jc)
    return IlqrOracle(u, q, qd, np.stack(hist), np.stack(h_al), np.stack(h_dV), np.stack(h_st), np.stack(h_c))
