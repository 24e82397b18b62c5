"""numpy restatement of the backward pass of iLQR / DDP over a rollout (``rollout_lqr`` / ``rollout_riccati``), on top of
``rollout_grad_oracle.linearise`` (checker only).  fp64 by default; ``dtype=np.float32`` runs the same code in float32
(the yardstick of the fp32 kernel's error).

With ``x = (q | qd)``, ``D = dc_du[t]`` and ``M = Minv[t]``::

    A0 = [[I, dt I], [0, I]];  b = [dt^2 I ; dt I] (semi_implicit) | [0 ; dt I] (euler);  Bm = b M;  A = A0 - Bm D

and, per row, ``lam [2n]``, ``P [2n, 2n]``, ``dV [2]``, ``status``, for ``t = T-1 ... 0``::

    lam += (gq[t] | gqd[t]);  P += diag(hq[t] | hqd[t])
    Qx = A^T lam;  Qu = gu[t] + Bm^T lam;  Qxx = A^T P A;  Qux = Bm^T P A;  Quu = diag(hu[t]) + Bm^T P Bm
    Cholesky of Quu + reg I;  k = -(Quu + reg I)^-1 Qu;  K = -(Quu + reg I)^-1 Qux
    dV[0] += k^T Qu;  dV[1] += 1/2 k^T Quu k
    lam = Qx + K^T Quu k + K^T Qu + Qux^T k;  P = Qxx + K^T Quu K + K^T Qux + Qux^T K;  P = 1/2 (P + P^T)

A pivot ``<= 0`` or not finite: ``k = K = 0`` for that row and step and ``status += 1``.  The matrices ``A`` and ``Bm`` are
formed and multiplied as written: nothing of the kernel's factored evaluation order is shared."""
import numpy as np

from rollout_grad_oracle import linearise
from rollout_oracle import INTEGRATORS


def _slice(a, t, T, shape, dtype):
    """Slice ``t`` of a state cost given as ``[T, B, n]``, ``[B, n]`` (last step only) or None."""
    if a is None:
        return np.zeros(shape, dtype)
    a = np.asarray(a, dtype=dtype)
    if a.ndim == 3:
        return a[t]
    return a if t == T - 1 else np.zeros(shape, dtype)


def cholesky(A):
    """Batched Cholesky ``[B, n, n] -> (L, ok [B])``; a row whose pivot is ``<= 0`` or not finite is flagged, its factor
    is meaningless but the other rows are untouched."""
    B, n, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[:, j, j] - np.einsum("bk,bk->b", L[:, j, :j], L[:, j, :j])
            good = (s > 0) & np.isfinite(s)
            ok &= good
            d = np.sqrt(np.where(good, s, 1)).astype(A.dtype)
            L[:, j, j] = d
            if j + 1 < n:
                L[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum("bik,bk->bi", L[:, j + 1:, :j], L[:, j, :j])) / d[:, None]
    return L, ok


def cho_solve(L, R):
    """``(L L^T)^-1 R`` for ``L [B, n, n]``, ``R [B, n, m]``."""
    n = L.shape[1]
    X = np.array(R)
    with np.errstate(all="ignore"):
        for i in range(n):
            X[:, i] = (X[:, i] - np.einsum("bk,bkm->bm", L[:, i, :i], X[:, :i])) / L[:, i, i, None]
        for i in range(n - 1, -1, -1):
            X[:, i] = (X[:, i] - np.einsum("bk,bkm->bm", L[:, i + 1:, i], X[:, i + 1:])) / L[:, i, i, None]
    return X


def dynamics(dc_du_t, Minv_t, dt, integrator, dtype=np.float64):
    """``(A [B, 2n, 2n], Bm [B, 2n, n])`` of one step."""
    D = np.asarray(dc_du_t, dtype=dtype)
    M = np.asarray(Minv_t, dtype=dtype)
    n = M.shape[-1]
    dt = dtype(dt)
    I, Z = np.eye(n, dtype=dtype), np.zeros((n, n), dtype)
    A0 = np.block([[I, dt * I], [Z, I]])
    b = np.concatenate([dt * dt * I if integrator == "semi_implicit" else Z, dt * I])
    Bm = np.einsum("ri,bij->brj", b, M)
    return A0[None] - np.einsum("bri,bic->brc", Bm, D), Bm


def riccati(dc_du, Minv, dt, gq=None, gqd=None, hq=None, hqd=None, gu=None, hu=None, reg=0.0, integrator="semi_implicit",
            lam=None, P=None, dV=None, status=None, dtype=np.float64, zero_gains=False):
    """The scan fed with a given linearisation: ``dc_du [T, B, n, 2n]``, ``Minv [T, B, n, n]`` ->
    ``(k [T, B, n], K [T, B, n, 2n], lam [B, 2n], P [B, 2n, 2n], dV [B, 2], status [B])``.  ``hu``: ``[T, B, n]`` or
    ``[n]``.  ``zero_gains=True`` forces every ``k`` and ``K`` to zero (the recursion of ``rollout_adjoint``)."""
    if integrator not in INTEGRATORS:
        raise ValueError(integrator)
    dc_du = np.asarray(dc_du, dtype=dtype)
    Minv = np.asarray(Minv, dtype=dtype)
    T, B, n = dc_du.shape[:3]
    hu = np.asarray(hu, dtype=dtype)
    reg = dtype(reg)
    half = dtype(0.5)
    lam = np.zeros((B, 2 * n), dtype) if lam is None else np.array(lam, dtype=dtype)
    P = np.zeros((B, 2 * n, 2 * n), dtype) if P is None else np.array(P, dtype=dtype)
    dV = np.zeros((B, 2), dtype) if dV is None else np.array(dV, dtype=dtype)
    status = np.zeros(B, np.int32) if status is None else np.array(status, dtype=np.int32)
    ks, Ks = np.zeros((T, B, n), dtype), np.zeros((T, B, n, 2 * n), dtype)
    idx = np.arange(2 * n)
    for t in range(T - 1, -1, -1):
        A, Bm = dynamics(dc_du[t], Minv[t], dt, integrator, dtype)
        lam = lam + np.concatenate([_slice(gq, t, T, (B, n), dtype), _slice(gqd, t, T, (B, n), dtype)], 1)
        P = P.copy()
        P[:, idx, idx] += np.concatenate([_slice(hq, t, T, (B, n), dtype), _slice(hqd, t, T, (B, n), dtype)], 1)
        Qx = np.einsum("brc,br->bc", A, lam)
        Qu = np.einsum("bri,br->bi", Bm, lam)
        if gu is not None:
            Qu = Qu + np.asarray(gu, dtype=dtype)[t]
        PA = np.einsum("brs,bsc->brc", P, A)
        Qxx = np.einsum("brc,brd->bcd", A, PA)
        Qux = np.einsum("bri,brc->bic", Bm, PA)
        Quu = np.einsum("bri,brj->bij", Bm, np.einsum("brs,bsj->brj", P, Bm))
        hut = hu if hu.ndim == 1 else hu[t]
        Quu[:, np.arange(n), np.arange(n)] += hut
        F = Quu.copy()
        F[:, np.arange(n), np.arange(n)] += reg
        L, ok = cholesky(F)
        if zero_gains:
            ok = np.zeros(B, bool)
        sol = cho_solve(L, np.concatenate([Qu[:, :, None], Qux], 2))
        with np.errstate(all="ignore"):
            k = np.where(ok[:, None], -sol[:, :, 0], 0).astype(dtype)
            K = np.where(ok[:, None, None], -sol[:, :, 1:], 0).astype(dtype)
        if not zero_gains:
            status = status + (~ok).astype(np.int32)
        ks[t], Ks[t] = k, K
        Quuk = np.einsum("bij,bj->bi", Quu, k)
        dV = dV + np.stack([np.einsum("bi,bi->b", k, Qu), half * np.einsum("bi,bi->b", k, Quuk)], 1)
        lam = Qx + np.einsum("bic,bi->bc", K, Quuk) + np.einsum("bic,bi->bc", K, Qu) + np.einsum("bic,bi->bc", Qux, k)
        P = (Qxx + np.einsum("bic,bid->bcd", K, np.einsum("bij,bjd->bid", Quu, K)) + np.einsum("bic,bid->bcd", K, Qux)
             + np.einsum("bic,bid->bcd", Qux, K))
        P = half * (P + P.transpose(0, 2, 1))
    return ks, Ks, lam, P, dV, status


def rollout_lqr(om, q0, qd0, u, dt, q_traj, qd_traj, GRAVITY=-9.81, **kw):
    """The evaluating form: linearise along the stored trajectory (teacher forcing), then ``riccati``."""
    dc, Mi = linearise(om, q0, qd0, u, q_traj, qd_traj, GRAVITY)
    return riccati(dc, Mi, dt, **kw)


def closed_loop_cost(dc_du, Minv, dt, k, K, x0, integrator, gq, gqd, hq, hqd, gu, hu, Pf=None, alpha=1.0, du=None):
    """For the linear-quadratic problem whose dynamics ARE the linearisation (``x_{t+1} = A_t x_t + Bm_t u_t`` about
    zero): the cost ``[B]`` of the pass ``u_t = alpha k_t + K_t x_t (+ du_t)`` from ``x0`` and the controls it applied.
    State costs attach to slices ``x_{t+1}``, control costs to ``u_t``, ``Pf`` to the last slice."""
    T, B, n = k.shape
    x = np.array(x0, dtype=np.float64)
    J = np.zeros(B)
    us = np.zeros((T, B, n))
    for t in range(T):
        A, Bm = dynamics(dc_du[t], Minv[t], dt, integrator)
        ut = alpha * k[t] + np.einsum("bic,bc->bi", K[t], x)
        if du is not None:
            ut = ut + du[t]
        us[t] = ut
        hut = hu if np.ndim(hu) == 1 else hu[t]
        J += (gu[t] * ut).sum(1) + 0.5 * (hut * ut * ut).sum(1)
        x = np.einsum("brc,bc->br", A, x) + np.einsum("bri,bi->br", Bm, ut)
        g = np.concatenate([gq[t], gqd[t]], 1)
        h = np.concatenate([hq[t], hqd[t]], 1)
        J += (g * x).sum(1) + 0.5 * (h * x * x).sum(1)
    if Pf is not None:
        J += 0.5 * np.einsum("br,brc,bc->b", x, Pf, x)
    return J, us
