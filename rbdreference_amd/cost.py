"""The quadratic tracking cost of ``RBDReference.rollout_cost`` and ``RBDReference.ilqr``.

Per row, with slice ``t`` the state after step ``t`` (``rollout``'s convention) and ``u_t`` the control applied::

    J = sum_t sum_j  1/2 w_u[t,j] u_t,j^2 + c_u[t,j] u_t,j
                   + 1/2 w_q[t,j] (q[t,j] - q_target[t,j])^2 + 1/2 w_qd[t,j] (qd[t,j] - qd_target[t,j])^2

``QuadraticCost`` holds the six arrays, gives the plain array expression of ``J`` (``value``: the checker and the timing
baseline of the kernel that accumulates ``J`` on chip) and the cost model ``rollout_lqr`` takes (``derivatives``)."""
from __future__ import annotations

import numpy as np
import torch

_STATE = ("w_q", "w_qd", "q_target", "qd_target")
_CONTROL = ("w_u", "c_u")


def _is_t(x):
    return isinstance(x, torch.Tensor)


def _broadcast(x, shape):
    return x.expand(shape) if _is_t(x) else np.broadcast_to(x, shape)


class QuadraticCost:
    """``w_q, w_qd, q_target, qd_target, w_u, c_u``: each ``None`` or an array (numpy or torch) of shape ``[T, B, n]``,
    ``[T, n]`` (shared by the rows) or ``[n]`` (shared by rows and steps).  A missing weight drops its term; a missing
    target or ``c_u`` is zero.  ``terminal_state_only=True``: the state terms belong to the LAST slice alone and the four
    state arrays are ``[B, n]`` or ``[n]``."""

    def __init__(self, w_q=None, w_qd=None, q_target=None, qd_target=None, w_u=None, c_u=None, terminal_state_only=False):
        self.w_q, self.w_qd, self.q_target, self.qd_target, self.w_u, self.c_u = w_q, w_qd, q_target, qd_target, w_u, c_u
        self.terminal_state_only = bool(terminal_state_only)
        for name in _STATE + _CONTROL:
            x = getattr(self, name)
            nd = len(np.shape(x)) if x is not None else 1
            top = 2 if (self.terminal_state_only and name in _STATE) else 3
            if not 1 <= nd <= top:
                raise ValueError(f"QuadraticCost: {name} must have 1 to {top} axes, got shape {tuple(np.shape(x))}")

    def _dense_one(self, name, T, B, n):
        """The array ``name`` in the dense form of the C-ABI (a broadcast view where the given form is smaller)."""
        x = getattr(self, name)
        if x is None:
            return None
        if not _is_t(x):
            x = np.asarray(x, dtype=np.float64)
        sh = tuple(x.shape)
        if self.terminal_state_only and name in _STATE:
            want = (B, n)
            ok = sh in ((n,), (B, n))
        else:
            want = (T, B, n)
            ok = sh in ((n,), (T, n), (T, B, n))
            if sh == (T, n):
                x = x[:, None, :]
        if not ok:
            forms = f"[{B}, {n}] or [{n}]" if len(want) == 2 else f"[{T}, {B}, {n}], [{T}, {n}] or [{n}]"
            raise ValueError(f"QuadraticCost: {name} must be {forms}, got {list(sh)}")
        return _broadcast(x, want)

    def dense(self, T, B, n):
        """-> dict of the six arrays as ``[T, B, n]`` (state arrays ``[B, n]`` with ``terminal_state_only``), ``None`` kept."""
        return {name: self._dense_one(name, T, B, n) for name in _STATE + _CONTROL}

    def value(self, q, qd, u):
        """``J`` per row of a trajectory ``q, qd, u [T, ..., B, n]`` (extra axes between ``T`` and ``B`` broadcast, as the
        ``[T, A, B, n]`` outputs of a line search) -> ``[..., B]``: a plain array expression."""
        T, B, n = u.shape[0], u.shape[-2], u.shape[-1]
        d = self.dense(T, B, n)
        if _is_t(u):
            d = {k_: (None if v is None else torch.as_tensor(v, dtype=u.dtype, device=u.device)) for k_, v in d.items()}
        extra = u.ndim - 3
        wt = lambda a: a[(slice(None),) + (None,) * extra]      # noqa: E731  [T, B, n] -> [T, 1.., B, n]
        if self.terminal_state_only:
            xs, xd, ws = q[-1], qd[-1], (lambda a: a)
        else:
            xs, xd, ws = q, qd, wt
        state, control = [], []
        if d["w_q"] is not None:
            e = xs if d["q_target"] is None else xs - ws(d["q_target"])
            state.append(0.5 * ws(d["w_q"]) * e ** 2)
        if d["w_qd"] is not None:
            e = xd if d["qd_target"] is None else xd - ws(d["qd_target"])
            state.append(0.5 * ws(d["w_qd"]) * e ** 2)
        if d["w_u"] is not None:
            control.append(0.5 * wt(d["w_u"]) * u ** 2)
        if d["c_u"] is not None:
            control.append(wt(d["c_u"]) * u)

        def total(terms, axes):
            s = terms[0]
            for x in terms[1:]:
                s = s + x
            return s.sum(axis=axes)

        if self.terminal_state_only:
            parts = [total(t, ax) for t, ax in ((control, (0, -1)), (state, -1)) if t]
        else:
            parts = [total(state + control, (0, -1))] if state + control else []
        if not parts:
            return 0.0 * u.sum(axis=(0, -1))
        return parts[0] if len(parts) == 1 else parts[0] + parts[1]

    def derivatives(self, q, qd, u):
        """The cost model at a nominal ``q, qd, u [T, B, n]`` as the keyword arguments of ``rollout_lqr``: ``grad_q, grad_qd,
        hess_q, hess_qd`` (``[T, B, n]``, or ``[B, n]`` with ``terminal_state_only``; ``None`` where the weight is missing),
        ``grad_u`` and ``hess_u [T, B, n]`` (zeros without ``w_u``: ``rollout_lqr`` requires the Hessian)."""
        T, B, n = u.shape
        d = self.dense(T, B, n)
        if _is_t(u):
            d = {k_: (None if v is None else torch.as_tensor(v, dtype=u.dtype, device=u.device)) for k_, v in d.items()}
        xs, xd = (q[-1], qd[-1]) if self.terminal_state_only else (q, qd)
        out = dict(grad_q=None, grad_qd=None, hess_q=None, hess_qd=None)
        if d["w_q"] is not None:
            out["grad_q"] = d["w_q"] * (xs if d["q_target"] is None else xs - d["q_target"])
            out["hess_q"] = d["w_q"]
        if d["w_qd"] is not None:
            out["grad_qd"] = d["w_qd"] * (xd if d["qd_target"] is None else xd - d["qd_target"])
            out["hess_qd"] = d["w_qd"]
        zero = torch.zeros_like(u) if _is_t(u) else np.zeros_like(u)
        gu = zero if d["w_u"] is None else d["w_u"] * u
        out["grad_u"] = gu if d["c_u"] is None else gu + d["c_u"]
        out["hess_u"] = zero if d["w_u"] is None else d["w_u"]
        return out
