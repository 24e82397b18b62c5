"""Argument handling of the rollout and control family of ``RBDReference`` (``rollout`` ... ``rollout_riccati``, ``ilqr``,
``mppi``): ONE definition of every rule the eleven methods share.

`Ctx` is what a call knows about its caller -- numpy or torch, device, dtype -- and turns inputs into contiguous
device tensors and results back into what the caller gave.  The module-level functions are pure shape and value
checks: they take ``who`` (the method's name, the prefix of every message), touch no GPU and no library, and so refuse
a call before anything is uploaded or launched.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import RBD_INTEGRATORS

WS_CAP = 1 << 30          # default cap of the linearisation scratch of rollout_grad / rollout_lqr (`workspace_bytes`)
_SKIP = object()
_MIXING = "mixing numpy and torch inputs is not supported"
_NO_GPU = "rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to cuda:0 (no CPU fallback)"


class Ctx:
    """Caller kind (``is_np``), device and dtype of one call, and what follows from them: ``esz``, ``sfx``, ``stream()``."""
    __slots__ = ("is_np", "dev", "dtp", "esz", "sfx")

    def __init__(self, is_np, dev, dtp):
        self.is_np, self.dev, self.dtp = is_np, dev, dtp
        self.esz = 4 if dtp == torch.float32 else 8
        self.sfx = "f32" if self.esz == 4 else "f64"

    @classmethod
    def from_prep(cls, prep):
        """From ``RBDReference._prep(q0, qd0)`` -> ``(its [B, n] tensors, context)``."""
        tensors, _, is_np, dev, dtp = prep
        return tensors, cls(is_np, dev, dtp)

    @classmethod
    def from_first(cls, first, *others):
        """From a first input that is no ``[B, n]`` state (``J``, ``dc_du``): numpy -> float64 on cuda:0, a tensor -> its
        GPU and float dtype.  ``others`` are refused first when their kind differs from ``first``'s."""
        is_np = not isinstance(first, torch.Tensor)
        if any(isinstance(x, torch.Tensor) == is_np for x in others):
            raise TypeError(_MIXING)
        if is_np:
            if not torch.cuda.is_available():
                raise RuntimeError(_NO_GPU)
            return cls(True, torch.device("cuda", 0), torch.float64)
        dev, dtp = first.device, first.dtype
        if dev.type != "cuda":
            raise RuntimeError("inputs must live on a ROCm GPU (cuda device); no CPU fallback")
        if dtp not in (torch.float32, torch.float64):
            raise TypeError(f"unsupported dtype {dtp}; use float32 or float64")
        return cls(False, dev, dtp)

    @classmethod
    def upload(cls, q0, qd0, u, noise, cost, strict):
        """For the drivers (``ilqr``, ``mppi``), whose loops work on tensors: a numpy caller's arrays and the arrays of its
        ``QuadraticCost`` go to cuda:0 in float64 -> ``(context, q0, qd0, u, noise, cost)``.  A torch caller's inputs are
        left to the inner calls, except that ``strict`` refuses a ``qd0``, ``u`` or ``noise`` that is no tensor here."""
        from .cost import QuadraticCost
        from .api import _COST_ARRAYS
        if not isinstance(q0, torch.Tensor):
            if any(isinstance(x, torch.Tensor) for x in (qd0, u, *(getattr(cost, a) for a in _COST_ARRAYS), noise)):
                raise TypeError(_MIXING)
            if not torch.cuda.is_available():
                raise RuntimeError(_NO_GPU)
            cx = cls(True, torch.device("cuda", 0), torch.float64)
            q0, qd0, u, noise = (cx.tensor(x) for x in (q0, qd0, u, noise))
            cost = QuadraticCost(*(cx.tensor(getattr(cost, a)) for a in _COST_ARRAYS), terminal_state_only=cost.terminal_state_only)
            return cx, q0, qd0, u, noise, cost
        if strict and not all(isinstance(x, torch.Tensor) for x in (qd0, u) + (() if noise is None else (noise,))):
            raise TypeError(_MIXING)
        return cls(False, q0.device, q0.dtype), q0, qd0, u, noise, cost

    def stream(self):
        """torch's current stream on the call's device, as the ``hipStream_t`` the C ABI takes."""
        return torch.cuda.current_stream(self.dev).cuda_stream

    def tensor(self, x, dtype=None):
        """An input as a contiguous device tensor of the call's dtype (``dtype=torch.int32``: of int32, for ``status``);
        ``None`` stays ``None``; numpy and torch inputs do not mix; a contiguous tensor is returned as it is."""
        if x is None:
            return None
        int32 = dtype is torch.int32
        if isinstance(x, torch.Tensor):
            if self.is_np:
                raise TypeError(_MIXING)
            if x.device != self.dev or x.dtype != (dtype or self.dtp):
                raise TypeError("all inputs must share device and dtype" + (" (status: int32)" if int32 else ""))
            return x.contiguous()
        if not self.is_np:
            raise TypeError(_MIXING)
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32 if int32 else np.float64), device=self.dev)

    def small(self, x):
        """A float, sequence, array or tensor as a tensor of the call's device and dtype (lam, sigma, alpha, the limits)."""
        if isinstance(x, torch.Tensor):
            return x.to(device=self.dev, dtype=self.dtp)
        return torch.as_tensor(np.asarray(x, dtype=np.float64), device=self.dev).to(self.dtp)

    def limits(self, u_min, u_max, n):
        """``u_min, u_max`` (scalars or ``[n]``, checked by `check_limits`) -> two contiguous ``[n]`` tensors, or two ``None``.
        Ready-made ``[n]`` tensors of the call's device and dtype come back as they are."""
        if u_min is None:
            return None, None
        return self.small(u_min).expand(n).contiguous(), self.small(u_max).expand(n).contiguous()

    def alpha_rows(self, q0, qd0, alpha, A, row_alpha, k, B):
        """The step size of every row of a closed-loop launch -> ``(q0, qd0, alpha per row or None, rows)``.  A line search
        (``alpha`` 1-D of length ``A``) runs ``rows = A B`` rows: row ``a B + b`` starts where row ``b`` does and takes
        ``alpha[a]``.  Without ``k`` there is nothing to scale and no tensor."""
        rows = B * (A or 1)
        if A is not None:
            q0, qd0 = q0.repeat(A, 1), qd0.repeat(A, 1)
        al = None
        if row_alpha is not None:
            al = self.tensor(row_alpha).reshape(rows)
        elif k is not None:
            if A is None:
                al = torch.full((rows,), float(alpha), device=self.dev, dtype=self.dtp)
            else:
                al = self.small(alpha).repeat_interleave(B).contiguous()
        return q0, qd0, al, rows

    def to_caller(self, x):
        """Results as the caller's kind: numpy arrays for a numpy caller, the tensors themselves otherwise; ``None`` stays,
        tuples and namedtuples keep their type."""
        if x is None or not self.is_np:
            return x
        if isinstance(x, tuple):
            parts = [self.to_caller(e) for e in x]
            return type(x)(*parts) if hasattr(x, "_fields") else tuple(parts)
        return x.cpu().numpy()


# ---- pure checks: shapes and values, before anything touches the GPU ----------------------------------------------------
def check_base_integrator(who, floating, integrator=_SKIP, why="rollout has no floating base"):
    """The family is for fixed-base robots and the integrators of ``RBD_INTEGRATORS`` (not looked at when omitted)."""
    if floating:
        raise NotImplementedError(f"{who}: fixed-base robots only ({why})")
    if integrator is not _SKIP and integrator not in RBD_INTEGRATORS:
        raise ValueError(f"{who}: unknown integrator {integrator!r}; use one of {sorted(RBD_INTEGRATORS)}")


def check_state(who, n, q0, qd0, unbatched=True):
    """``q0`` and ``qd0``: both ``[B, n]`` or, where ``unbatched``, both ``[n]`` -> their shape."""
    sq, sqd = tuple(np.shape(q0)), tuple(np.shape(qd0))
    if unbatched:
        if sq not in ((n,), sq[:1] + (n,)) or sqd != sq:
            raise ValueError(f"{who}: q0 and qd0 must both be [{n}] or [B, {n}], got {sq} and {sqd}")
    elif len(sq) != 2 or sq[1] != n or sqd != sq:
        raise ValueError(f"{who}: q0 and qd0 must both be [B, {n}], got {sq} and {sqd}")
    return sq


def check_shapes(who, n, q0, qd0, u, unbatched=True, shared_u=True, b_nom=False):
    """``(q0, qd0, u)`` of a time-major rollout -> ``(unbatched?, B, T, u shared by every row?)``.  ``u`` is ``[T, B, n]``
    (``[T, n]`` for ``q0 [n]``); with ``shared_u`` also ``[T, n]`` for a batch; with ``b_nom`` ``[T, B_nom, n]`` where
    ``B_nom`` divides ``B``."""
    sq = check_state(who, n, q0, qd0, unbatched)
    unb = len(sq) == 1
    B = 1 if unb else sq[0]
    su = tuple(np.shape(u))
    shared = False
    if b_nom:
        if len(su) != 3 or su[2] != n or su[1] == 0 or B % su[1] != 0:
            raise ValueError(f"{who}: u must be [T, B_nom, {n}] (time-major) with B_nom dividing B = {B}, got {su}")
    elif shared_u:
        shared = len(su) == 2
        if unb and not shared:
            raise ValueError(f"{who}: q0 [{n}] takes u [T, {n}], got {su}")
        if len(su) not in (2, 3) or su[1:] != ((n,) if shared else (B, n)):
            raise ValueError(f"{who}: u must be [T, {B}, {n}] or [T, {n}] (time-major), got {su}")
    elif su[1:] != sq:
        raise ValueError(f"{who}: u must be {['T', *sq]} (time-major), got {su}")
    if su[0] == 0:
        raise ValueError(f"{who}: u holds no step (T == 0)")
    return unb, B, su[0], shared


def check_u_steps(who, n, u, B):
    """``u [T, B, n]`` with ``T > 0`` -- the drivers' and ``mppi_update``'s nominal -> ``T``."""
    su = tuple(np.shape(u))
    if len(su) != 3 or su[1:] != (B, n) or su[0] == 0:
        raise ValueError(f"{who}: u must be [T, {B}, {n}] (time-major, T > 0), got {su}")
    return su[0]


def check_named_shapes(who, entries, required=()):
    """``entries``: ``(name, x, shape)`` in the order of refusal; ``None`` passes unless the name is ``required``."""
    for name, x, want in entries:
        if x is None:
            if name in required:
                raise ValueError(f"{who}: {name} is required")
        elif tuple(np.shape(x)) != tuple(want):
            raise ValueError(f"{who}: {name} must be {list(want)}, got {tuple(np.shape(x))}")


def check_limits(who, u_min, u_max, n):
    """``u_min, u_max``: both or neither, each a scalar or ``[n]``."""
    if (u_min is None) != (u_max is None):
        raise ValueError(f"{who}: give u_min and u_max together, or neither")
    for name, x in (("u_min", u_min), ("u_max", u_max)):
        if x is not None and tuple(np.shape(x)) not in ((), (n,)):
            raise ValueError(f"{who}: {name} must be a scalar or [{n}], got {tuple(np.shape(x))}")


def check_alpha(who, alpha):
    """``alpha``: a float -> ``None``, or a line search's non-empty 1-D sequence -> its length ``A``."""
    sa = tuple(np.shape(alpha))
    if len(sa) > 1 or (len(sa) == 1 and sa[0] == 0):
        raise ValueError(f"{who}: alpha must be a float or a non-empty 1-D sequence of step sizes, got shape {sa}")
    return sa[0] if sa else None


def check_row_alpha(who, row_alpha, alpha, k, lead):
    """``row_alpha``: one step size per row, instead of ``alpha`` (which must keep its default) and with ``k``."""
    if row_alpha is None:
        return
    if np.shape(alpha) != () or isinstance(alpha, torch.Tensor) or float(alpha) != 1.0:
        raise ValueError(f"{who}: give alpha or row_alpha, not both")
    if k is None:
        raise ValueError(f"{who}: row_alpha scales k, which is missing")
    if tuple(np.shape(row_alpha)) != tuple(lead):
        raise ValueError(f"{who}: row_alpha must be {list(lead)} (one step size per row), got {tuple(np.shape(row_alpha))}")


def rollg_g_shape(gq, gqd, T, B, n, unb, who):
    """Shape check of the two cost gradients, before anything touches the GPU -> g_final_only."""
    if gq is None and gqd is None:
        raise ValueError(f"{who}: give grad_q, grad_qd or both (the gradient of the cost with respect to the trajectory)")
    full, fin = ((T, n), (n,)) if unb else ((T, B, n), (B, n))
    shapes = [tuple(np.shape(g)) for g in (gq, gqd) if g is not None]
    if any(sh not in (full, fin) for sh in shapes) or len(set(shapes)) != 1:
        raise ValueError(f"{who}: grad_q and grad_qd must both be {list(full)} or both {list(fin)} (final state), got {shapes}")
    return shapes[0] == fin


def lqr_cost_shapes(T, B, n, unb, who, grad_q, grad_qd, hess_q, hess_qd, grad_u, hess_u, reg):
    """Shape and value checks of the cost model, before anything touches the GPU -> (x_final_only, hu_shared)."""
    if hess_u is None:
        raise ValueError(f"{who}: hess_u is required (the diagonal of the control cost's Hessian, [T, B, n] or [n])")
    full, fin = ((T, n), (n,)) if unb else ((T, B, n), (B, n))
    shapes = [tuple(np.shape(a)) for a in (grad_q, grad_qd, hess_q, hess_qd) if a is not None]
    if any(sh not in (full, fin) for sh in shapes) or len(set(shapes)) > 1:
        raise ValueError(f"{who}: grad_q, grad_qd, hess_q and hess_qd must all be {list(full)} or all {list(fin)} "
                         f"(last step only), got {shapes}")
    if grad_u is not None and tuple(np.shape(grad_u)) != full:
        raise ValueError(f"{who}: grad_u must be {list(full)}, got {tuple(np.shape(grad_u))}")
    sh = tuple(np.shape(hess_u))
    if sh != (n,) and sh != full:          # (unbatched: [T, n] is per step, [n] is shared)
        raise ValueError(f"{who}: hess_u must be {list(full)} or [{n}] (shared by every row and step), got {sh}")
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError(f"{who}: reg must be finite and >= 0, got {reg}")
    return bool(shapes) and shapes[0] == fin, sh == (n,)


def check_linearisation(who, dc_du, Minv, n):
    """``dc_du [T, B, n, 2n]`` and ``Minv [T, B, n, n]`` of ``T > 0`` steps -> ``(T, B)``."""
    sd, sm = tuple(np.shape(dc_du)), tuple(np.shape(Minv))
    if len(sd) != 4 or sd[2:] != (n, 2 * n) or sm != sd[:2] + (n, n):
        raise ValueError(f"{who}: dc_du must be [T, B, {n}, {2 * n}] and Minv [T, B, {n}, {n}], got {sd} and {sm}")
    if sd[0] == 0:
        raise ValueError(f"{who}: no step (T == 0)")
    return sd[:2]


def check_trajectory(who, q, qd, T, B, n, unb):
    """``q, qd``: the trajectory ``rollout`` returned, both or neither."""
    if (q is None) != (qd is None):
        raise ValueError(f"{who}: give both q and qd (the trajectory of rollout) or neither")
    traj = (T, n) if unb else (T, B, n)
    if q is not None and (tuple(np.shape(q)) != traj or tuple(np.shape(qd)) != traj):
        raise ValueError(f"{who}: q and qd must be the trajectory {list(traj)}, got {tuple(np.shape(q))} and {tuple(np.shape(qd))}")


def check_workspace_request(who, requested):
    if requested is not None and int(requested) < 0:
        raise ValueError(f"{who}: workspace_bytes < 0")


def workspace_bytes(query, B, T, esz, requested=None, cap=WS_CAP):
    """Scratch of the linearisation, which decides how many steps one chunk holds: what the caller asked for, else all
    ``T`` steps' (``query(B, T, esz)``, the library's ``..._workspace_bytes``) capped at ``cap`` but never below one step's."""
    if requested is not None:
        return int(requested)
    return max(min(int(query(B, T, esz)), cap), int(query(B, 1, esz)))
