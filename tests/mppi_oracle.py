"""fp64 numpy restatement of ``RBDReference.mppi_update`` and of the ``mppi`` driver (checker only).

``P`` independent problems with ``S`` samples each, in ``rollout_cost``'s row layout (row ``s P + p`` is sample ``s`` of problem
``p``): ``J [S, P]``, ``du [T, S, P, n]``, ``u [T, P, n]``, ``lam`` a float or ``[P]``, limits ``[n]`` or scalars.  Per problem:

    Jm = min_s J (a NaN counts as +inf);  x_s = (J_s - Jm) / lam;  e_s = exp(-x_s);  eta = sum e;  w = e / eta;
    ess = eta^2 / sum e^2;  d_s = du_s, or clamp(u + du_s) - u with limits (the clamp of ``rollout_closed_loop``: ordered
    comparisons, a NaN passes);  D = sum_s w_s d_s;  u_out = u + D, clamped once more with limits.
    status 2: lam not finite and positive; else 1: Jm not finite; else 0.  status != 0: u_out = u (clamped), w = 0, ess = 0.
"""
from types import SimpleNamespace

import numpy as np

from rollout_cost_oracle import rollout_cost


def clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def mppi_update(J, du, u, lam, u_lo=None, u_hi=None):
    """-> ``(u_out [T, P, n], w [S, P], x [S, P], d [T, S, P, n], D [T, P, n], ess [P], status [P])``; ``x`` is 0 where the
    problem's status is not 0."""
    J, du, u = (np.asarray(a, dtype=np.float64) for a in (J, du, u))
    S, P = J.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (P,))
    Jc = np.where(np.isnan(J), np.inf, J)
    Jm = Jc.min(axis=0)
    status = np.where(~((lam > 0) & np.isfinite(lam)), 2, np.where(np.isfinite(Jm), 0, 1)).astype(np.int32)
    ok = status == 0
    with np.errstate(all="ignore"):
        x = np.where(ok[None], (Jc - np.where(ok, Jm, 0.0)[None]) / np.where(ok, lam, 1.0)[None], 0.0)
        e = np.where(ok[None], np.exp(-x), 0.0)
        eta = e.sum(axis=0)
        w = np.where(ok[None], e / np.where(ok, eta, 1.0)[None], 0.0)
        ess = np.where(ok, eta * eta / np.where(ok, (e * e).sum(axis=0), 1.0), 0.0)
        limits = u_lo is not None
        if limits:
            lo, hi = np.broadcast_to(np.asarray(u_lo, dtype=np.float64), u.shape[-1:]), np.broadcast_to(np.asarray(u_hi, dtype=np.float64), u.shape[-1:])
            d = clamp(u[:, None] + du, lo, hi) - u[:, None]
        else:
            d = du
        D = np.einsum("sp,tspj->tpj", w, d)
        D = np.where(ok[None, :, None], D, 0.0)
        u_out = u + D
        if limits:
            u_out = clamp(u_out, lo, hi)
    return u_out, w, x, d, D, ess, status


def bounds(sfx, S, ref, u, du, limits):
    """The three bounds of DESIGN.md §4.16 from the oracle's ``(u_out, w, x, d, D, ess, status)``: they hold for any order
    of the sums.  c_s = 3 x_s + 2 (three roundings on the exponent's argument, exp within one ulp); v_s = w_s^2 / sum w^2."""
    fi = np.finfo(np.float32 if sfx == "f32" else np.float64)
    eps, tiny = float(fi.eps), float(fi.tiny)
    _, w, x, d, D, ess, _ = ref
    c = 3 * x + 2
    cw = c * w
    v = w * w / (w * w).sum(axis=0)
    A = np.einsum("sp,tspj->tpj", w, np.abs(d))
    Bc = np.einsum("sp,tspj->tpj", cw, np.abs(d)) + cw.sum(axis=0)[None, :, None] * np.abs(D)
    L = 2 * (np.abs(u) + np.einsum("sp,tspj->tpj", w, np.abs(du))) if limits else 0.0
    dmax = np.abs(d).max(axis=(0, 1, 3))[None, :, None]
    b_u = 2 * eps * ((S + 8) * A + Bc + np.abs(u) + np.abs(D) + L) + S * tiny * dmax
    b_w = 2 * eps * w * (c + S + 2 + cw.sum(axis=0)[None]) + 2 * tiny
    b_ess = 2 * eps * ess * (3 * S + 8 + 2 * cw.sum(axis=0) + 2 * (v * c).sum(axis=0))
    return b_u, b_w, b_ess


def mppi_du(noise_i, sigma):
    """``sigma`` (a float, ``[n]`` or ``[T, n]``) times the noise ``[T, S, P, n]``, sample 0 zeroed: the nominal itself."""
    sg = np.asarray(sigma, dtype=np.float64)
    du = (sg[:, None, None, :] if sg.ndim == 2 else sg) * np.asarray(noise_i, dtype=np.float64)
    du[:, 0] = 0.0
    return du


def mppi(om, q0, qd0, u, dt, c, noise, sigma=0.1, lam=1.0, u_min=None, u_max=None, GRAVITY=-9.81, integrator="semi_implicit"):
    """The driver on ``rollout_cost_oracle.rollout_cost``: ``q0, qd0 [P, n]``, ``u [T, P, n]``, ``c`` the cost's six arrays,
    ``noise [iters, T, S, P, n]`` -> a namespace with ``u, q, qd [T, P, n]``, ``cost [iters + 1, P]``, ``ess, status [iters, P]``
    and, per iteration, the lists ``J`` (``[S, P]``), ``du`` and ``update`` (``mppi_update``'s tuple) and ``nominal`` (the ``u``
    entering it)."""
    noise = np.asarray(noise, dtype=np.float64)
    iters, T, S, P, n = noise.shape
    u = np.array(u, dtype=np.float64)
    kw = dict(u_min=u_min, u_max=u_max, GRAVITY=GRAVITY, integrator=integrator)
    r = SimpleNamespace(J=[], du=[], update=[], nominal=[])
    cost, ess, status = [], [], []
    for i in range(iters):
        du = mppi_du(noise[i], sigma)
        J = rollout_cost(om, np.tile(q0, (S, 1)), np.tile(qd0, (S, 1)), u, dt, c, du=du.reshape(T, S * P, n), **kw)[0].reshape(S, P)
        up = mppi_update(J, du, u, lam, u_min, u_max)
        r.J.append(J); r.du.append(du); r.update.append(up); r.nominal.append(u)
        cost.append(J[0]); ess.append(up[5]); status.append(up[6])
        u = up[0]
    Jf, q, qd, _ = rollout_cost(om, q0, qd0, u, dt, c, **kw)
    cost.append(Jf)
    r.u, r.q, r.qd = u, q, qd
    r.cost = np.stack(cost)
    r.ess = np.stack(ess) if iters else np.zeros((0, P))
    r.status = np.stack(status) if iters else np.zeros((0, P), dtype=np.int32)
    return r
