"""Drop-in ``RBDReference`` whose rnea / rnea_grad / minv run as HIP kernels on MI355X.

Mirrors the reference's class (``/root/reference/RBDReference.py:5-7``) and the three methods its
README lists (``README.md:15-17``): same names, keyword arguments, defaults and return arity.
Extension: ``q, qd, qdd`` may be ``[n]`` (one configuration, reference shapes come back) or
``[B, n]`` (a batch; every output gains a leading B).  PyTorch-ROCm tensors in -> tensors out on the
same device / dtype (float32 or float64); numpy arrays or lists in -> uploaded to ``cuda:0`` in
float64, numpy out.  There is no CPU implementation here: without a GPU and the per-robot HIP
library every call raises.
"""
from __future__ import annotations

import contextlib
import os
import threading
from sys import getrefcount as _refs
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _rollout_args as _ra
from ._lib import RBD_INTEGRATORS, RbdLibrary
from .packer import PackedModel, pack_robot

__all__ = ["RBDReference", "BoundLaunch"]

_T = torch.Tensor
_F32, _F64 = torch.float32, torch.float64
_storage_uses = getattr(torch._C, "_storage_Use_Count", None)          # holders of a StorageImpl (views, detached aliases)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # hipStream_t of torch's current stream, as an int
_cur_dev = torch.cuda.current_device
_tid = threading.get_ident

# ---- one-shot calls without per-call allocations --------------------------------------------
# A method call used to cost 7-14 us of Python around an 11-25 us kernel: shape checks, a device guard, a stream
# look-up and one torch.empty per output.  The second call with the same signature (op, B, dtype, device, stream)
# is now: validate three tensors by attribute, take a FREE output set from a small pool, ONE ctypes call.
# "Free" keeps the reference's contract that every call returns fresh outputs (RBDReference.py:623, :785, :1345):
# a set is handed out again only when the caller holds neither its tensors (Python reference counts) nor any view or
# alias of their storage (StorageImpl use count) any more; while anything is still held, another set is used (up to
# POOL_SETS per signature, then a new one replaces the oldest -- which stays valid for whoever holds it).  Big outputs
# (> POOL_MAX_BYTES per set) are never pooled: there the kernel dwarfs the Python.  RBD_OUTPUT_POOL=0 turns it off.
POOL_SETS = 3
POOL_MAX_BYTES = 160 << 20
POOL_SIGNATURES = 16


_COST_ARRAYS = ("w_q", "w_qd", "q_target", "qd_target", "w_u", "c_u")      # QuadraticCost's arrays, in its constructor's order
# what RBDReference.ilqr returns: the final nominal and the per-iteration record
IlqrResult = namedtuple("IlqrResult", ["u", "q", "qd", "cost", "alpha", "dV", "status"])
# what RBDReference.mppi_update and RBDReference.mppi return
MppiUpdate = namedtuple("MppiUpdate", ["u", "w", "ess", "status"])
MppiResult = namedtuple("MppiResult", ["u", "q", "qd", "cost", "ess", "status"])


class _OutSet:
    __slots__ = ("flat", "outs", "ptrs", "cdata", "base")

    def __init__(self, shapes, dt, dev):
        esz = 4 if dt is _F32 else 8
        sizes = [(int(np.prod(sh)) * esz + 15) & ~15 for sh in shapes]
        self.flat = torch.empty((sum(sizes),), device=dev, dtype=torch.uint8)
        outs, off = [], 0
        for sh, nb in zip(shapes, sizes):
            outs.append(self.flat[off:off + int(np.prod(sh)) * esz].view(dt).view(sh))
            off += nb
        self.outs = tuple(outs)
        del outs
        self.ptrs = tuple(t.data_ptr() for t in self.outs)
        self.cdata = self.flat.untyped_storage()._cdata
        self.base = None
        self.base = self._probe()

    def _probe(self):
        return (_storage_uses(self.cdata), _refs(self.outs), *[_refs(t) for t in self.outs])

    def free(self):
        return self._probe() == self.base


class _Plan:
    """Everything of a call signature that does not change between calls."""
    __slots__ = ("fn", "sets", "epoch", "ws", "wsp", "wsb", "shapes", "dt", "dev")

    def __init__(self, fn, shapes, dt, dev, epoch, ws=None, wsb=0):
        self.fn, self.shapes, self.dt, self.dev, self.epoch = fn, shapes, dt, dev, epoch
        self.ws, self.wsb, self.wsp = ws, wsb, (ws.data_ptr() if ws is not None else None)
        self.sets = []

    def take(self):
        for s in self.sets:
            if s.free():
                return s
        s = _OutSet(self.shapes, self.dt, self.dev)
        if len(self.sets) >= POOL_SETS:
            self.sets.pop(0)
        self.sets.append(s)
        return s


class BoundLaunch:
    """What `RBDReference.bind` returns: ``launch()`` enqueues the bound entry point on torch's current stream of the
    inputs' device and returns ``launch.outputs`` (the same tensors every time).  The library that answers is the one
    that was serving the robot when `bind` ran (bind again after `RbdLibrary.wait_specialized()` to move from the
    model-handle library to the robot's own)."""

    def __init__(self, rbd, fn, args, inputs, outputs, keep, dev):
        self._rbd, self._fn, self._args, self.inputs, self.outputs, self._keep, self._dev = rbd, fn, args, inputs, outputs, keep, dev
        self._idx = dev.index if dev.index is not None else torch.cuda.current_device()

    def __call__(self):
        if torch.cuda.current_device() != self._idx:
            with torch.cuda.device(self._dev):
                return self.__call__()
        rc = self._fn(*self._args(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            self._rbd._lib.check(rc)
        return self.outputs


def _rollout_function():
    """The ``torch.autograd.Function`` behind ``rollout(..., differentiable=True)`` (made on first use)."""
    global _RolloutFunction
    if _RolloutFunction is None:
        from torch.autograd.function import once_differentiable

        class RolloutFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q0, qd0, u, rbd, dt, gravity, integrator, trajectory):
                q, qd = rbd.rollout(q0.detach(), qd0.detach(), u.detach(), dt, gravity, integrator, True)
                ctx.save_for_backward(q0, qd0, u, q, qd)
                ctx.args = (rbd, dt, gravity, integrator, trajectory)
                return (q, qd) if trajectory else (q[-1].clone(), qd[-1].clone())

            @staticmethod
            @once_differentiable
            def backward(ctx, gq, gqd):
                q0, qd0, u, q, qd = ctx.saved_tensors
                rbd, dt, gravity, integrator, trajectory = ctx.args
                gu, gq0, gqd0 = rbd.rollout_grad(q0, qd0, u, dt, gq, gqd, gravity, integrator, q=q, qd=qd)
                return gq0, gqd0, gu, None, None, None, None, None

        _RolloutFunction = RolloutFunction
    return _RolloutFunction.apply


_RolloutFunction = None


class RBDReference:
    def __init__(self, robotObj, build: bool = True, generic=None):
        """``generic`` ('auto' | 'only' | 'never', default ``RBD_GENERIC`` or 'auto'): whether the model-handle library
        (include/rbd_generic.h) may answer rnea / rnea_grad / minv / forward_dynamics(_grad) while -- or instead of --
        the robot's own compiled library (``_lib.RbdLibrary``)."""
        self.robot = robotObj                     # RBDReference.py:7
        self.model: PackedModel = pack_robot(robotObj)
        self._lib = RbdLibrary(self.model, build=build, generic=generic)
        self.n = self.model.n            # bodies
        self.nv = self.model.nv          # columns of q, qd, qdd, c: n, or n + 5 with a floating base
        self._plans = {}
        self._pool_on = (os.environ.get("RBD_OUTPUT_POOL", "1") != "0" and _storage_uses is not None and _raw_stream is not None)

    # ---- cached launch plans (see the note at the top of the module) ---------------------------------------------
    def _sig(self, q, qd, qdd):
        """``(B, dtype, device index, raw stream)`` when q, qd (qdd unless None) are plain contiguous ``[B, nv]`` tensors of one
        dtype on one GPU and the robot's own library is loaded; None sends the call down the general path."""
        if not self._pool_on or type(q) is not _T or self._lib._full is None:
            return None
        dt = q.dtype
        if dt is not _F32 and dt is not _F64:
            return None
        idx = q.get_device()
        shp = q.shape
        if idx < 0 or len(shp) != 2 or shp[1] != self.nv or shp[0] == 0 or not q.is_contiguous():
            return None
        if qd is not None and (type(qd) is not _T or qd.dtype is not dt or qd.get_device() != idx or qd.shape != shp or not qd.is_contiguous()):
            return None
        if qdd is not None and (type(qdd) is not _T or qdd.dtype is not dt or qdd.get_device() != idx or qdd.shape != shp or not qdd.is_contiguous()):
            return None
        st = _raw_stream(idx)
        if st == 0 and _cur_dev() != idx:       # the null stream belongs to the CURRENT device (include/rbd_hip.h)
            return None
        return shp[0], dt, idx, st

    def _plan(self, key, make):
        key = (_tid(), key)                     # one pool per host thread: a set is "free" by reference counts, which another
        p = self._plans.get(key)                # thread could not tell from "handed out a moment ago, not yet bound"
        if p is None or p.epoch != self._lib.epoch:
            p = make()
            if p is None:
                return None
            if len(self._plans) >= POOL_SIGNATURES:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def _mk_plan(self, base, dt, idx, shapes, has_qdd=True, ws_query=None):
        """A `_Plan` for entry point ``base``: function object, output shapes, and -- resolved from the SAME library object
        -- the scratch the entry point needs (``ws_query(lib, esz) -> bytes``)."""
        esz = 4 if dt is _F32 else 8
        if sum(int(np.prod(sh)) for sh in shapes) * esz > POOL_MAX_BYTES:
            return None
        dev = torch.device("cuda", idx)
        sfx = "f32" if esz == 4 else "f64"
        lib = self._lib.resolve(base, sfx, has_qdd)
        ws, wsb = None, 0
        if ws_query is not None:
            wsb = int(ws_query(lib, esz))
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
        return _Plan(getattr(lib, f"{base}_{sfx}"), shapes, dt, dev, self._lib.epoch, ws, wsb)

    def release_pools(self):
        """Drop the cached launch plans and their pooled output sets (tensors the caller still holds stay valid)."""
        self._plans.clear()

    @contextlib.contextmanager
    def shard_of(self, global_rows: int):
        """Declare that the calls inside the block evaluate SHARDS of a global batch of ``global_rows`` rows: wherever
        the library picks a kernel from the batch size it then decides from the global size (``RBD_OPT_SELECT_BATCH``,
        include/rbd_hip.h), so a shard is computed by the same kernel -- and is bit-identical, row by row -- as the
        unsharded call.  Process-wide like every option; restored on exit."""
        from ._lib import RBD_OPT_SELECT_BATCH
        g = int(global_rows)
        if not (0 <= g < 2 ** 31):
            raise ValueError("global_rows must be in [0, 2^31)")
        old = self._lib.get_option(RBD_OPT_SELECT_BATCH)
        self._lib.set_option(RBD_OPT_SELECT_BATCH, g)
        try:
            yield self
        finally:
            self._lib.set_option(RBD_OPT_SELECT_BATCH, old)

    # ------------------------------------------------------------------------------------
    def _prep(self, *arrs):
        """Normalise inputs -> (list of contiguous [B, n] device tensors, unbatched?, numpy?)."""
        first = arrs[0]
        is_np = not isinstance(first, torch.Tensor)
        if is_np:
            if not torch.cuda.is_available():
                raise RuntimeError("rbdreference_amd needs a ROCm GPU: numpy inputs are uploaded to "
                                   "cuda:0 and run through the HIP kernels (no CPU fallback)")
            dev, dt = torch.device("cuda", 0), torch.float64
        else:
            dev, dt = first.device, first.dtype
            if dev.type != "cuda":
                raise RuntimeError("inputs must live on a ROCm GPU (cuda device); no CPU fallback")
            if dt not in (torch.float32, torch.float64):
                raise TypeError(f"unsupported dtype {dt}; use float32 or float64")
        out = []
        unb = None
        for x in arrs:
            if x is None:
                out.append(None)
                continue
            if isinstance(x, torch.Tensor):
                if is_np:
                    raise TypeError("mixing numpy and torch inputs is not supported")
                if x.device != dev or x.dtype != dt:
                    raise TypeError("all inputs must share device and dtype")
                t = x
            else:
                t = torch.as_tensor(np.asarray(x, dtype=np.float64), device=dev)
            u = t.dim() == 1
            if u:
                t = t[None, :]
            if t.dim() != 2 or t.shape[1] != self.nv:
                raise ValueError(f"expected shape [{self.nv}] or [B, {self.nv}], got {tuple(x.shape) if hasattr(x, 'shape') else len(x)}")
            if unb is None:
                unb, B = u, t.shape[0]
            elif u != unb or t.shape[0] != B:
                raise ValueError("q, qd, qdd must have identical shapes")
            out.append(t.contiguous())
        return out, unb, is_np, dev, dt

    def _minv_ws(self, B: int, esz: int) -> int:
        """rbd_minv_workspace_bytes from the library that serves rbd_minv of that precision right now (a QUERY for
        callers who bring their own scratch; the methods themselves resolve the library once per call)."""
        lib = self._lib.serving("rbd_minv", "f32" if esz == 4 else "f64")
        return int(lib.rbd_minv_workspace_bytes(B, esz))

    @staticmethod
    def _ptr(t: Optional[torch.Tensor]):
        return None if t is None else t.data_ptr()

    @staticmethod
    def _ret(t: torch.Tensor, unb: bool, is_np: bool):
        if unb:
            t = t[0]
        return t.cpu().numpy() if is_np else t

    @staticmethod
    def _check_out(t, shape, dev, dt, name):
        """A caller-provided output tensor (`out=`): right shape, dtype, device, contiguous."""
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out: `{name}` must be a contiguous {dt} tensor of shape {tuple(shape)} on {dev}")
        return t

    @staticmethod
    def _out_ok(t, shape, dt, idx):
        """`out=` tensor usable by the cached launch plan as it is (else the general path checks it and says what is wrong)."""
        return type(t) is _T and t.dtype is dt and t.get_device() == idx and tuple(t.shape) == shape and t.is_contiguous()

    def _fn(self, base: str, dt, has_qdd: bool = True):
        return self._lib.fn(base, "f32" if dt == torch.float32 else "f64", has_qdd)

    # ------------------------------------------------------------------------------------
    def rnea(self, q, qd, qdd=None, GRAVITY=-9.81, f_ext=None, outputs: str = "cvaf", out=None):
        """RBDReference.rnea (``RBDReference.py:623-628``) -> ``(c, v, a, f)``; ``f`` is the
        accumulated force, ``f_ext`` is accepted and ignored exactly as there.
        ``outputs="c"`` skips v, a, f (returns ``(c, None, None, None)``).  ``out=(c, v, a, f)``: write into these
        pre-allocated device tensors (batched tensor inputs only) -- a loop that owns its buffers then pays the
        launch alone, not four allocations per call."""
        if out is None and outputs == "cvaf":
            sg = self._sig(q, qd, qdd)
            if sg is not None:
                B, dt, idx, st = sg
                p = self._plan(("rnea", B, dt, idx, st), lambda: self._mk_plan("rbd_rnea", dt, idx, ((B, self.nv), (B, 6, self.n), (B, 6, self.n), (B, 6, self.n))))
                if p is not None:
                    o = p.take()
                    rc = p.fn(q.data_ptr(), qd.data_ptr(), None if qdd is None else qdd.data_ptr(), float(GRAVITY), B, *o.ptrs, st)
                    if rc != 0:
                        self._lib.check(rc)
                    return o.outs
        if out is not None and outputs == "cvaf" and len(out) == 4:
            # pre-allocated outputs through the cached plan too: the call is the same single ctypes launch, without the pool
            sg = self._sig(q, qd, qdd)
            if sg is not None:
                B, dt, idx, st = sg
                vs = (B, 6, self.n)
                if self._out_ok(out[0], (B, self.nv), dt, idx) and all(self._out_ok(t, vs, dt, idx) for t in out[1:]):
                    p = self._plan(("rnea", B, dt, idx, st), lambda: self._mk_plan("rbd_rnea", dt, idx, ((B, self.nv), vs, vs, vs)))
                    if p is not None:
                        rc = p.fn(q.data_ptr(), qd.data_ptr(), None if qdd is None else qdd.data_ptr(), float(GRAVITY), B,
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), st)
                        if rc != 0:
                            self._lib.check(rc)
                        return out[0], out[1], out[2], out[3]
        (q, qd, qdd), unb, is_np, dev, dt = self._prep(q, qd, qdd)
        B = q.shape[0]
        if out is not None:
            if is_np or unb or outputs != "cvaf" or len(out) != 4:
                raise ValueError("out= needs batched tensor inputs, outputs='cvaf' and four tensors (c, v, a, f)")
            c = self._check_out(out[0], (B, self.nv), dev, dt, "c")
            v, a, f = (self._check_out(t, (B, 6, self.n), dev, dt, nm) for t, nm in zip(out[1:], "vaf"))
            with torch.cuda.device(dev):
                self._lib.check(self._fn("rbd_rnea", dt)(
                    self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), B,
                    self._ptr(c), self._ptr(v), self._ptr(a), self._ptr(f), torch.cuda.current_stream(dev).cuda_stream))
            return c, v, a, f
        with torch.cuda.device(dev):
            c = torch.empty((B, self.nv), device=dev, dtype=dt)
            if outputs == "cvaf":
                v = torch.empty((B, 6, self.n), device=dev, dtype=dt)
                a = torch.empty_like(v)
                f = torch.empty_like(v)
            elif outputs == "c":
                v = a = f = None
            else:
                raise ValueError("outputs must be 'cvaf' or 'c'")
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), B,
                self._ptr(c), self._ptr(v), self._ptr(a), self._ptr(f), st))
        if v is None:
            return self._ret(c, unb, is_np), None, None, None
        return tuple(self._ret(t, unb, is_np) for t in (c, v, a, f))

    def rnea_fpass(self, q, qd, qdd=None, GRAVITY=-9.81):
        """RBDReference.rnea_fpass (``RBDReference.py:559-598``) -> ``(v, a, f)`` with the LOCAL body
        forces (no backward accumulation) -- the per-pass surface of ``README.md:19``."""
        (q, qd, qdd), unb, is_np, dev, dt = self._prep(q, qd, qdd)
        B = q.shape[0]
        with torch.cuda.device(dev):
            v = torch.empty((B, 6, self.n), device=dev, dtype=dt)
            a = torch.empty_like(v)
            f = torch.empty_like(v)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_fpass", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), B,
                self._ptr(v), self._ptr(a), self._ptr(f), st))
        return tuple(self._ret(t, unb, is_np) for t in (v, a, f))

    def rnea_bpass(self, q, f):
        """RBDReference.rnea_bpass (``RBDReference.py:600-621``) -> ``(c, f)``.  Like the reference it
        accumulates into ``f`` IN PLACE when ``f`` is a contiguous device tensor (``:619``) and
        returns that same tensor; numpy input gets a new array back."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B = q.shape[0]
        if isinstance(f, torch.Tensor):
            if is_np or f.device != dev or f.dtype != dt:
                raise TypeError("f must share device and dtype with q")
            ft = f[None] if unb else f
            if ft.shape != (B, 6, self.n):
                raise ValueError(f"f must have shape [B, 6, {self.n}]")
            fc = ft if ft.is_contiguous() else ft.contiguous()
        else:
            fa = np.asarray(f, dtype=np.float64)
            fa = fa[None] if unb else fa
            if fa.shape != (B, 6, self.n):
                raise ValueError(f"f must have shape [B, 6, {self.n}]")
            fc = torch.as_tensor(fa, device=dev).contiguous()
            ft = None
        with torch.cuda.device(dev):
            c = torch.empty((B, self.nv), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_bpass", dt)(self._ptr(q), self._ptr(fc), B, self._ptr(c), st))
        if ft is not None and fc is not ft:
            ft.copy_(fc)
        if ft is not None:
            return self._ret(c, unb, is_np), f
        return self._ret(c, unb, is_np), self._ret(fc, unb, is_np)

    # ---- auxiliary (non-[B,n]) operands of the per-pass methods ---------------------------------
    def _aux(self, x, shape, unb, is_np, dev, dt, name):
        """Device tensor [B, *shape] for a per-pass operand.  Returns ``(work, origin)``: ``work`` is
        the contiguous device tensor handed to the kernel, ``origin`` the caller's object (tensor or
        writable ndarray) that an in-place pass must see updated, or None."""
        B = shape[0]
        if isinstance(x, torch.Tensor):
            if is_np or x.device != dev or x.dtype != dt:
                raise TypeError(f"{name} must share device and dtype with q")
            t = x[None] if unb else x
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must have shape {list(shape[1:]) if unb else list(shape)}, got {list(x.shape)}")
            return (t if t.is_contiguous() else t.contiguous()), x
        if not is_np:
            raise TypeError("mixing numpy and torch inputs is not supported")
        xa = np.asarray(x, dtype=np.float64)
        xb = xa[None] if unb else xa
        if xb.shape != tuple(shape):
            raise ValueError(f"{name} must have shape {list(shape[1:]) if unb else list(shape)}, got {list(xa.shape)}")
        origin = x if isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.writeable else None
        return torch.as_tensor(np.ascontiguousarray(xb), device=dev), origin

    @staticmethod
    def _writeback(work, origin, unb):
        """Mirror the reference's in-place mutation of an argument (e.g. ``RBDReference.py:1291``)."""
        if origin is None:
            return
        src = work[0] if unb else work
        if isinstance(origin, torch.Tensor):
            if origin.data_ptr() != src.data_ptr():
                origin.copy_(src)
        else:
            np.copyto(origin, src.cpu().numpy())

    def rnea_grad_fpass_dq(self, q, qd, v, a, GRAVITY=-9.81):
        """RBDReference.rnea_grad_fpass_dq (``RBDReference.py:1127-1187``) -> ``(dv_dq, da_dq,
        df_dq)``, each ``(6, n, NB)`` per configuration; ``v, a`` are rnea's outputs."""
        (q, qd), unb, is_np, dev, dt = self._prep(q, qd)
        B, n = q.shape
        nb = self.n                        # bodies (== n unless the base floats: n = NB + 5)
        v, _ = self._aux(v, (B, 6, nb), unb, is_np, dev, dt, "v")
        a, _ = self._aux(a, (B, 6, nb), unb, is_np, dev, dt, "a")
        with torch.cuda.device(dev):
            dv = torch.empty((B, 6, n, nb), device=dev, dtype=dt)
            da = torch.empty_like(dv)
            df = torch.empty_like(dv)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_grad_fpass_dq", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(v), self._ptr(a), float(GRAVITY), B,
                self._ptr(dv), self._ptr(da), self._ptr(df), st))
        return tuple(self._ret(t, unb, is_np) for t in (dv, da, df))

    def rnea_grad_fpass_dqd(self, q, qd, v):
        """RBDReference.rnea_grad_fpass_dqd (``RBDReference.py:1189-1255``) -> ``(dv_dqd, da_dqd,
        df_dqd)``, each ``(6, n, NB)`` per configuration."""
        (q, qd), unb, is_np, dev, dt = self._prep(q, qd)
        B, n = q.shape
        nb = self.n
        v, _ = self._aux(v, (B, 6, nb), unb, is_np, dev, dt, "v")
        with torch.cuda.device(dev):
            dv = torch.empty((B, 6, n, nb), device=dev, dtype=dt)
            da = torch.empty_like(dv)
            df = torch.empty_like(dv)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_grad_fpass_dqd", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(v), B, self._ptr(dv), self._ptr(da), self._ptr(df), st))
        return tuple(self._ret(t, unb, is_np) for t in (dv, da, df))

    def rnea_grad_bpass_dq(self, q, f, df_dq):
        """RBDReference.rnea_grad_bpass_dq (``RBDReference.py:1257-1297``) -> ``dc_dq (n, n)``.  ``f`` is
        rnea's ACCUMULATED force; ``df_dq`` is accumulated child -> parent IN PLACE like the
        reference's argument (``:1291-1294``)."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B, n = q.shape
        f, _ = self._aux(f, (B, 6, self.n), unb, is_np, dev, dt, "f")
        df, origin = self._aux(df_dq, (B, 6, n, self.n), unb, is_np, dev, dt, "df_dq")
        with torch.cuda.device(dev):
            dc = torch.empty((B, n, n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_grad_bpass_dq", dt)(
                self._ptr(q), self._ptr(f), self._ptr(df), B, self._ptr(dc), st))
        self._writeback(df, origin, unb)
        return self._ret(dc, unb, is_np)

    def rnea_grad_bpass_dqd(self, q, df_dqd, USE_VELOCITY_DAMPING=False):
        """RBDReference.rnea_grad_bpass_dqd (``RBDReference.py:1299-1343``) -> ``dc_dqd (n, n)``;
        ``df_dqd`` accumulated in place (``:1331``)."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B, n = q.shape
        df, origin = self._aux(df_dqd, (B, 6, n, self.n), unb, is_np, dev, dt, "df_dqd")
        with torch.cuda.device(dev):
            dc = torch.empty((B, n, n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_grad_bpass_dqd", dt)(
                self._ptr(q), self._ptr(df), int(bool(USE_VELOCITY_DAMPING)), B, self._ptr(dc), st))
        self._writeback(df, origin, unb)
        return self._ret(dc, unb, is_np)

    def minv_bpass(self, q):
        """RBDReference.minv_bpass (``RBDReference.py:630-735``) -> ``(Minv, F, U, Dinv)`` with shapes
        ``(n, n), (n, 6, n), (n, 6), (n,)`` per configuration; ``Dinv`` holds ``D`` as there (``:698``)."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B, n = q.shape
        with torch.cuda.device(dev):
            Minv = torch.empty((B, n, n), device=dev, dtype=dt)
            F = torch.empty((B, n, 6, n), device=dev, dtype=dt)
            U = torch.empty((B, n, 6), device=dev, dtype=dt)
            D = torch.empty((B, n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_minv_bpass", dt)(
                self._ptr(q), B, self._ptr(Minv), self._ptr(F), self._ptr(U), self._ptr(D), st))
        return tuple(self._ret(t, unb, is_np) for t in (Minv, F, U, D))

    def minv_fpass(self, q, Minv, F, U, Dinv):
        """RBDReference.minv_fpass (``RBDReference.py:737-783``) -> ``Minv`` (updated in place, whole
        rows as at ``:771``: valid upper triangle, by-products below it).  ``F`` is rebuilt in place
        (``:774-781``); its incoming values are not read."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B, n = q.shape
        Mw, Mo = self._aux(Minv, (B, n, n), unb, is_np, dev, dt, "Minv")
        Fw, Fo = self._aux(F, (B, n, 6, n), unb, is_np, dev, dt, "F")
        Uw, _ = self._aux(U, (B, n, 6), unb, is_np, dev, dt, "U")
        Dw, _ = self._aux(Dinv, (B, n), unb, is_np, dev, dt, "Dinv")
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_minv_fpass", dt)(
                self._ptr(q), B, self._ptr(Mw), self._ptr(Fw), self._ptr(Uw), self._ptr(Dw), st))
        self._writeback(Mw, Mo, unb)
        self._writeback(Fw, Fo, unb)
        if isinstance(Mo, torch.Tensor):
            return Minv
        return self._ret(Mw, unb, is_np)

    def rnea_grad(self, q, qd, qdd=None, GRAVITY=-9.81, USE_VELOCITY_DAMPING=False,
                  return_c: bool = False, out=None):
        """RBDReference.rnea_grad (``RBDReference.py:1345-1368``) -> ``dc_du = [dc_dq | dc_dqd]``,
        ``(n, 2n)`` per configuration.  ``return_c=True`` also returns the bias force ``c`` the
        reference computes internally (``:1353``) -> ``(c, dc_du)``.  Floating base: ``n = NB + 5`` and the
        base's six position columns are derivatives along a base-frame twist, as in the reference; robots
        with fewer than six bodies are refused (the reference raises IndexError for them, ``:1168``)."""
        if out is None:
            sg = self._sig(q, qd, qdd)
            if sg is not None:
                B, dt, idx, st = sg
                hq = qdd is not None
                p = self._plan(("rnea_grad", B, dt, idx, st, hq, return_c),
                               lambda: self._mk_plan("rbd_rnea_grad", dt, idx, ((B, self.nv), (B, self.nv, 2 * self.nv)) if return_c else ((B, self.nv, 2 * self.nv),), hq))
                if p is not None:
                    o = p.take()
                    rc = p.fn(q.data_ptr(), qd.data_ptr(), qdd.data_ptr() if hq else None, float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0, B,
                              o.ptrs[0] if return_c else None, o.ptrs[-1], st)
                    if rc != 0:
                        self._lib.check(rc)
                    return o.outs if return_c else o.outs[0]
        if out is not None:
            sg = self._sig(q, qd, qdd)
            if sg is not None:
                B, dt, idx, st = sg
                hq = qdd is not None
                oc, odc = (out if (return_c and type(out) in (tuple, list) and len(out) == 2) else (None, out))
                if self._out_ok(odc, (B, self.nv, 2 * self.nv), dt, idx) and (not return_c or self._out_ok(oc, (B, self.nv), dt, idx)):
                    p = self._plan(("rnea_grad", B, dt, idx, st, hq, return_c),
                                   lambda: self._mk_plan("rbd_rnea_grad", dt, idx, ((B, self.nv), (B, self.nv, 2 * self.nv)) if return_c else ((B, self.nv, 2 * self.nv),), hq))
                    if p is not None:
                        rc = p.fn(q.data_ptr(), qd.data_ptr(), qdd.data_ptr() if hq else None, float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0, B,
                                  oc.data_ptr() if return_c else None, odc.data_ptr(), st)
                        if rc != 0:
                            self._lib.check(rc)
                        return (oc, odc) if return_c else odc
        (q, qd, qdd), unb, is_np, dev, dt = self._prep(q, qd, qdd)
        B = q.shape[0]
        if out is not None:      # out=dc_du, or out=(c, dc_du) with return_c=True: pre-allocated device tensors
            if is_np or unb:
                raise ValueError("out= needs batched tensor inputs")
            oc, odc = (out if return_c else (None, out))
            dc = self._check_out(odc, (B, self.nv, 2 * self.nv), dev, dt, "dc_du")
            c = self._check_out(oc, (B, self.nv), dev, dt, "c") if return_c else None
            with torch.cuda.device(dev):
                self._lib.check(self._fn("rbd_rnea_grad", dt, qdd is not None)(
                    self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0, B,
                    self._ptr(c), self._ptr(dc), torch.cuda.current_stream(dev).cuda_stream))
            return (c, dc) if return_c else dc
        with torch.cuda.device(dev):
            dc = torch.empty((B, self.nv, 2 * self.nv), device=dev, dtype=dt)
            c = torch.empty((B, self.nv), device=dev, dtype=dt) if return_c else None
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_grad", dt, qdd is not None)(
                self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY),
                1 if USE_VELOCITY_DAMPING else 0, B, self._ptr(c), self._ptr(dc), st))
        if return_c:
            return self._ret(c, unb, is_np), self._ret(dc, unb, is_np)
        return self._ret(dc, unb, is_np)

    def rnea_and_grad(self, q, qd, qdd=None, GRAVITY=-9.81, USE_VELOCITY_DAMPING=False):
        """``rnea`` and ``rnea_grad`` of the same inputs in one call -> ``(c, v, a, f, dc_du)``: what the
        reference computes inside ``rnea_grad`` (``RBDReference.py:1353`` runs ``rnea`` and drops its
        outputs).  For small batches this is one launch of the column kernel."""
        sg = self._sig(q, qd, qdd)
        if sg is not None:
            B, dt, idx, st = sg
            p = self._plan(("rnea_and_grad", B, dt, idx, st), lambda: self._mk_plan(
                "rbd_rnea_with_grad", dt, idx, ((B, self.nv), (B, 6, self.n), (B, 6, self.n), (B, 6, self.n), (B, self.nv, 2 * self.nv))))
            if p is not None:
                o = p.take()
                rc = p.fn(q.data_ptr(), qd.data_ptr(), None if qdd is None else qdd.data_ptr(), float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0, B, *o.ptrs, st)
                if rc != 0:
                    self._lib.check(rc)
                return o.outs
        (q, qd, qdd), unb, is_np, dev, dt = self._prep(q, qd, qdd)
        B = q.shape[0]
        with torch.cuda.device(dev):
            c = torch.empty((B, self.nv), device=dev, dtype=dt)
            v = torch.empty((B, 6, self.n), device=dev, dtype=dt)
            a = torch.empty_like(v)
            f = torch.empty_like(v)
            dc = torch.empty((B, self.nv, 2 * self.nv), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_rnea_with_grad", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0, B,
                self._ptr(c), self._ptr(v), self._ptr(a), self._ptr(f), self._ptr(dc), st))
        return tuple(self._ret(t, unb, is_np) for t in (c, v, a, f, dc))

    def minv(self, q, output_dense=True, out=None, workspace=None):
        """RBDReference.minv (``RBDReference.py:785-806``) -> ``(n, n)`` per configuration.
        ``output_dense=False`` returns the upper triangle with a ZERO strict lower triangle (the
        reference leaves forward-pass by-products there, ``:771``).  ``out=`` / ``workspace=``: a pre-allocated
        ``[B, n, n]`` result tensor and a uint8 scratch tensor of ``minv_workspace_bytes(B, dtype)`` bytes
        (batched tensor input only), for loops that own their buffers."""
        if out is None and workspace is None:
            sg = self._sig(q, None, None)
            if sg is not None:
                B, dt, idx, st = sg
                p = self._plan(("minv", B, dt, idx, st), lambda: self._mk_plan(
                    "rbd_minv", dt, idx, ((B, self.nv, self.nv),), ws_query=lambda lib, esz: lib.rbd_minv_workspace_bytes(B, esz)))
                if p is not None:
                    o = p.take()
                    rc = p.fn(q.data_ptr(), B, 1 if output_dense else 0, o.ptrs[0], p.wsp if p.wsb else None, p.wsb, st)
                    if rc != 0:
                        self._lib.check(rc)
                    return o.outs[0]
        if out is not None and workspace is None:
            sg = self._sig(q, None, None)
            if sg is not None:
                B, dt, idx, st = sg
                if self._out_ok(out, (B, self.nv, self.nv), dt, idx):
                    p = self._plan(("minv", B, dt, idx, st), lambda: self._mk_plan(
                        "rbd_minv", dt, idx, ((B, self.nv, self.nv),), ws_query=lambda lib, esz: lib.rbd_minv_workspace_bytes(B, esz)))
                    if p is not None:
                        rc = p.fn(q.data_ptr(), B, 1 if output_dense else 0, out.data_ptr(), p.wsp if p.wsb else None, p.wsb, st)
                        if rc != 0:
                            self._lib.check(rc)
                        return out
        (q,), unb, is_np, dev, dt = self._prep(q)
        B = q.shape[0]
        esz = 4 if dt == torch.float32 else 8
        if out is not None and (is_np or unb):
            raise ValueError("out= needs a batched tensor input")
        with torch.cuda.device(dev):
            M = torch.empty((B, self.nv, self.nv), device=dev, dtype=dt) if out is None else \
                self._check_out(out, (B, self.nv, self.nv), dev, dt, "Minv")
            sfx = "f32" if esz == 4 else "f64"
            lib = self._lib.resolve("rbd_minv", sfx)            # ONE resolution: size and entry point from the same library
            wsb = int(lib.rbd_minv_workspace_bytes(B, esz))
            if workspace is not None:
                if workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < wsb or not workspace.is_contiguous():
                    raise ValueError(f"workspace: a contiguous uint8 tensor of >= {wsb} bytes on {dev}")
                ws = workspace
            else:
                ws = torch.empty((wsb,), device=dev, dtype=torch.uint8) if wsb > 0 else None   # most robots: no scratch at all
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(getattr(lib, f"rbd_minv_{sfx}")(
                self._ptr(q), B, 1 if output_dense else 0, self._ptr(M), ws.data_ptr() if ws is not None else None, wsb, st))
        return self._ret(M, unb, is_np)

    # ---- pre-resolved launches for loops that own their buffers --------------------------------------------------
    def bind(self, op: str, q, qd=None, qdd=None, GRAVITY=-9.81, USE_VELOCITY_DAMPING=False, output_dense=True):
        """A control loop calls the same entry point on the same buffers thousands of times; a call through the
        methods above costs 15-25 us of Python (shape checks, allocations, device guard) next to a 7 us kernel at
        B = 4096.  ``bind`` validates once, allocates the outputs once, and returns a `BoundLaunch`: calling it is ONE
        ctypes call into the C-ABI on torch's current stream (the caller rewrites ``q, qd, qdd`` in place between calls;
        capturable in a ``torch.cuda.graph``).  ``op``: 'rnea' -> outputs (c, v, a, f); 'rnea_grad' -> (c, dc_du);
        'rnea_and_grad' -> (c, v, a, f, dc_du); 'minv' -> (Minv,).  Batched tensor inputs only."""
        ins = (q,) if op == "minv" else (q, qd, qdd)
        if op != "minv" and (qd is None):
            raise ValueError("bind: qd is required")
        tens, unb, is_np, dev, dt = self._prep(*ins)
        if is_np or unb:
            raise ValueError("bind needs batched torch tensors (the bound launch reads them in place)")
        for given, prepared in zip(ins, tens):
            if given is not None and prepared.data_ptr() != given.data_ptr():
                raise ValueError("bind: inputs must be contiguous (the bound launch reads the caller's own buffers)")
        B = tens[0].shape[0]
        esz = 4 if dt == torch.float32 else 8
        E = lambda *shape: torch.empty(shape, device=dev, dtype=dt)   # noqa: E731
        with torch.cuda.device(dev):
            g, damp = float(GRAVITY), 1 if USE_VELOCITY_DAMPING else 0
            p = [self._ptr(t) for t in tens]
            if op == "rnea":
                outs = (E(B, self.nv), E(B, 6, self.n), E(B, 6, self.n), E(B, 6, self.n))
                fn = self._fn("rbd_rnea", dt)
                args = lambda st: (p[0], p[1], p[2], g, B, *[o.data_ptr() for o in outs], st)   # noqa: E731
            elif op == "rnea_grad":
                outs = (E(B, self.nv), E(B, self.nv, 2 * self.nv))
                fn = self._fn("rbd_rnea_grad", dt, tens[2] is not None)
                args = lambda st: (p[0], p[1], p[2], g, damp, B, outs[0].data_ptr(), outs[1].data_ptr(), st)   # noqa: E731
            elif op == "rnea_and_grad":
                outs = (E(B, self.nv), E(B, 6, self.n), E(B, 6, self.n), E(B, 6, self.n), E(B, self.nv, 2 * self.nv))
                fn = self._fn("rbd_rnea_with_grad", dt)
                args = lambda st: (p[0], p[1], p[2], g, damp, B, *[o.data_ptr() for o in outs], st)   # noqa: E731
            elif op == "minv":
                outs = (E(B, self.nv, self.nv),)
                lib = self._lib.resolve("rbd_minv", "f32" if esz == 4 else "f64")
                wsb = int(lib.rbd_minv_workspace_bytes(B, esz))
                ws = torch.empty((wsb,), device=dev, dtype=torch.uint8) if wsb > 0 else None
                fn = getattr(lib, "rbd_minv_f32" if esz == 4 else "rbd_minv_f64")
                wp = ws.data_ptr() if ws is not None else None
                args = lambda st: (p[0], B, 1 if output_dense else 0, outs[0].data_ptr(), wp, wsb, st)   # noqa: E731
                outs = outs + ((ws,) if ws is not None else ())      # (kept alive with the launch; not a result)
            else:
                raise ValueError("bind: op must be 'rnea', 'rnea_grad', 'rnea_and_grad' or 'minv'")
        n_res = len(outs) - (1 if (op == "minv" and len(outs) == 2) else 0)
        return BoundLaunch(self, fn, args, tens, outs[:n_res], outs, dev)

    def minv_workspace_bytes(self, B: int, dtype=torch.float32) -> int:
        """Scratch bytes ``minv`` needs for B rows (0 for robots served by a kernel without workspace)."""
        return int(self._minv_ws(int(B), 4 if dtype == torch.float32 else 8))

    def crba(self, q):
        """RBDReference.crba (fixed-base branch, ``RBDReference.py:1091-1124``) -> joint-space inertia
        ``H``, ``(n, n)`` per configuration."""
        (q,), unb, is_np, dev, dt = self._prep(q)
        B = q.shape[0]
        with torch.cuda.device(dev):
            H = torch.empty((B, self.n, self.n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_crba", dt)(self._ptr(q), B, self._ptr(H), st))
        return self._ret(H, unb, is_np)

    # ---- next row of SURVEY.md §8f: forward dynamics on top of the three kernels --------------
    def aba(self, q, qd, tau, f_ext=[], GRAVITY=-9.81):
        """RBDReference.aba (fixed-base branch, ``RBDReference.py:940-1024``) -> ``qdd``; ``f_ext`` is
        accepted and ignored exactly as that branch does."""
        (q, qd, tau), unb, is_np, dev, dt = self._prep(q, qd, tau)
        B = q.shape[0]
        with torch.cuda.device(dev):
            qdd = torch.empty((B, self.n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_aba", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(tau), float(GRAVITY), B, self._ptr(qdd), st))
        return self._ret(qdd, unb, is_np)

    def _fd(self, q, qd, u, GRAVITY, want_grad):
        sg = self._sig(q, qd, u) if u is not None else None
        if sg is not None:
            B, dt, idx, st = sg
            base = "rbd_forward_dynamics_grad" if want_grad else "rbd_forward_dynamics"
            shapes = ((B, self.nv), (B, self.nv, 2 * self.nv)) if want_grad else ((B, self.nv),)
            p = self._plan((base, B, dt, idx, st), lambda: self._mk_plan(base, dt, idx, shapes, ws_query=lambda lib, esz: lib.rbd_fd_workspace_bytes(B, esz)))
            if p is not None:
                o = p.take()
                if want_grad:
                    rc = p.fn(q.data_ptr(), qd.data_ptr(), u.data_ptr(), float(GRAVITY), B, o.ptrs[0], o.ptrs[1], p.wsp, p.wsb, st)
                else:
                    rc = p.fn(q.data_ptr(), qd.data_ptr(), u.data_ptr(), float(GRAVITY), B, o.ptrs[0], p.wsp, p.wsb, st)
                if rc != 0:
                    self._lib.check(rc)
                return o.outs[0], (o.outs[1] if want_grad else None), False, False
        (q, qd, u), unb, is_np, dev, dt = self._prep(q, qd, u)
        B = q.shape[0]
        esz = 4 if dt == torch.float32 else 8
        sfx = "f32" if esz == 4 else "f64"
        with torch.cuda.device(dev):
            qdd = torch.empty((B, self.nv), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            base = "rbd_forward_dynamics_grad" if want_grad else "rbd_forward_dynamics"
            lib = self._lib.resolve(base, sfx)              # ONE resolution: workspace size, branch and entry point from the same library
            generic = getattr(lib, "is_generic", False)
            fn = getattr(lib, f"{base}_{sfx}")
            if not want_grad and (self.model.floating or generic):   # rnea (bias force) + minv + one product: scratch for c and Minv
                wsb = int(lib.rbd_fd_workspace_bytes(B, esz))
                ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
                self._lib.check(fn(self._ptr(q), self._ptr(qd), self._ptr(u), float(GRAVITY), B, self._ptr(qdd), ws.data_ptr(), wsb, st))
                return qdd, None, unb, is_np
            if not want_grad:        # one articulated-body launch, no scratch
                self._lib.check(fn(self._ptr(q), self._ptr(qd), self._ptr(u), float(GRAVITY), B, self._ptr(qdd), None, 0, st))
                return qdd, None, unb, is_np
            wsb = int(lib.rbd_fd_workspace_bytes(B, esz))
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
            d = torch.empty((B, self.nv, 2 * self.nv), device=dev, dtype=dt)
            self._lib.check(fn(self._ptr(q), self._ptr(qd), self._ptr(u), float(GRAVITY), B, self._ptr(qdd),
                               self._ptr(d), ws.data_ptr(), wsb, st))
            return qdd, d, unb, is_np

    def forward_dynamics(self, q, qd, u, GRAVITY=-9.81):
        """RBDReference.forward_dynamics (``RBDReference.py:1371-1374``): ``minv(q) @ (u - c(q, qd))``,
        evaluated by the articulated-body sweeps (same value to rounding, neither factor is formed)."""
        qdd, _, unb, is_np = self._fd(q, qd, u, GRAVITY, False)
        return self._ret(qdd, unb, is_np)

    def forward_dynamics_grad(self, q, qd, u, GRAVITY=-9.81):
        """RBDReference.forward_dynamics_grad (``RBDReference.py:1376-1384``) -> ``(qdd_dq, qdd_dqd)``,
        each ``(n, n)`` per configuration (views of one ``[B, n, 2n]`` buffer for tensor inputs)."""
        _, d, unb, is_np = self._fd(q, qd, u, GRAVITY, True)
        n = self.nv
        d = self._ret(d, unb, is_np)
        return d[..., :n], d[..., n:]

    # ---- second-order inverse-dynamics derivatives (RBDReference.py:1387-1604): rbd_second_order_idsva --------------
    def second_order_idsva_parallel(self, q, qd, qdd, GRAVITY=-9.81):
        """RBDReference.second_order_idsva_parallel (``RBDReference.py:1387-1604``) -> ``(d2tau_dq, d2tau_dqd, d2tau_dvdq,
        dM_dq)``, each ``(n, n, n)`` per configuration, with ``c = rnea(q, qd, qdd, GRAVITY)[0]`` and ``H = crba(q)``:
        ``d2tau_dq[i, j, k] = d2 c_i / dq_j dq_k``, ``d2tau_dqd[i, j, k] = d2 c_i / dqd_j dqd_k``,
        ``d2tau_dvdq[i, j, k] = d (dc_dqd[i, j]) / dq_k`` and ``dM_dq[i, j, k] = d H_ij / dq_k``, zeros included.

        These are the true derivatives.  The reference's composite-force sweep adds ``f[:, pi + 1]`` to the parent
        (:1448); this method adds the child's force.  On robots whose non-root bodies all have parent ``i - 1`` the two
        agree; on a branched robot the reference's ``d2tau_dq`` is not the derivative and this one differs from it (the
        other three outputs do not read ``f``).  Fixed-base robots only, as in the reference.

        ``q [n]`` -> four ``(n, n, n)`` arrays (float64 ndarrays for numpy inputs); ``q [B, n]`` -> four ``[B, n, n, n]``
        views of one ``[B, 4, n, n, n]`` buffer."""
        if self.model.floating:
            raise NotImplementedError("second_order_idsva_parallel: fixed-base robots only (the reference indexes q per "
                                      "body, RBDReference.py:1387-1604)")
        (q, qd, qdd), unb, is_np, dev, dt = self._prep(q, qd, qdd)
        B, n = q.shape[0], self.n
        with torch.cuda.device(dev):
            out = torch.empty((B, 4, n, n, n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            self._lib.check(self._fn("rbd_second_order_idsva", dt)(
                self._ptr(q), self._ptr(qd), self._ptr(qdd), float(GRAVITY), B, self._ptr(out), st))
        out = self._ret(out, unb, is_np)
        return out[..., 0, :, :, :], out[..., 1, :, :, :], out[..., 2, :, :, :], out[..., 3, :, :, :]

    # ---- second-order forward-dynamics derivatives (RBDReference.py:1606-1631): rbd_fdsva_so ---------------------------
    def fdsva_so(self, q, qd, u, GRAVITY=-9.81):
        """RBDReference.fdsva_so (``RBDReference.py:1606-1631``) -> ``(daba_dqdq, daba_dvdq, daba_dvdv, daba_dtdq)``, each
        ``(n, n, n)`` per configuration: the second derivatives of ``qdd = forward_dynamics(q, qd, u)``,
        ``d2 qdd_i / dq_j dq_k``, ``d (qdd_dqd[i, j]) / dq_k``, ``d2 qdd_i / dqd_j dqd_k`` and ``d Minv[i, j] / dq_k``.

        It is the reference's composition (:1625-1629) of this package's own ``minv``, ``forward_dynamics_grad`` and
        ``second_order_idsva_parallel`` at ``qdd``, contracted in one HIP kernel.  Three things follow.  On branched
        robots ``daba_dqdq`` differs from the reference's, because ``d2tau_dq`` does (the corrected composite-force
        index, see ``second_order_idsva_parallel``); the other three outputs match it.  On robots with prismatic joints
        ``daba_dqdq`` is not the second derivative: it inherits ``forward_dynamics_grad``'s ``qdd_dq``, which reproduces
        the reference's ``rnea_grad`` and is not the q-derivative for such joints.  And ``GRAVITY`` is used in every
        stage (the reference evaluates forward dynamics at -9.81 whatever it is given).  Fixed-base robots only.

        ``q [n]`` -> four ``(n, n, n)`` arrays (float64 ndarrays for numpy inputs); ``q [B, n]`` -> four ``[B, n, n, n]``
        views of one ``[B, 4, n, n, n]`` buffer."""
        if self.model.floating:
            raise NotImplementedError("fdsva_so: fixed-base robots only (the reference's fdsva_so calls "
                                      "second_order_idsva_parallel, RBDReference.py:1606-1631)")
        (q, qd, u), unb, is_np, dev, dt = self._prep(q, qd, u)
        B, n = q.shape[0], self.n
        esz = 4 if dt == torch.float32 else 8
        sfx = "f32" if esz == 4 else "f64"
        with torch.cuda.device(dev):
            out = torch.empty((B, 4, n, n, n), device=dev, dtype=dt)
            st = torch.cuda.current_stream(dev).cuda_stream
            lib = self._lib.resolve("rbd_fdsva_so", sfx)    # ONE resolution: workspace size and entry point from the same library
            wsb = int(lib.rbd_fdsva_so_workspace_bytes(B, esz))
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
            self._lib.check(getattr(lib, f"rbd_fdsva_so_{sfx}")(
                self._ptr(q), self._ptr(qd), self._ptr(u), float(GRAVITY), B, self._ptr(out), ws.data_ptr(), wsb, st))
        out = self._ret(out, unb, is_np)
        return out[..., 0, :, :, :], out[..., 1, :, :, :], out[..., 2, :, :, :], out[..., 3, :, :, :]

    # ---- forward-simulation rollouts: rbd_rollout, T steps of aba + integrator in one launch -------------------------
    def rollout(self, q0, qd0, u, dt, GRAVITY=-9.81, integrator="semi_implicit", trajectory=True, differentiable=False):
        """Integrate ``qdd_t = aba(q_t, qd_t, u_t, GRAVITY)`` over ``T`` steps of size ``dt`` in ONE kernel launch (the
        state stays on chip between steps) -> ``(q, qd)``.  Not part of the reference: a sampling controller's loop.

        ``integrator``: ``"semi_implicit"`` -- ``qd_{t+1} = qd_t + dt qdd_t``, then ``q_{t+1} = q_t + dt qd_{t+1}`` -- or
        ``"euler"`` -- ``q_{t+1} = q_t + dt qd_t``, ``qd_{t+1} = qd_t + dt qdd_t``.  No angle wrapping, joint limits,
        damping or external forces.  Fixed-base robots only.

        Everything with a time axis is TIME-MAJOR.  ``q0, qd0 [B, n]`` with ``u [T, B, n]`` -- or ``[T, n]``, one control
        sequence shared by every row -- give ``q, qd [T, B, n]``: slice ``t`` is the state after step ``t + 1`` (the
        initial state is not copied), a contiguous ``[B, n]`` tensor that ``rnea_grad``, ``forward_dynamics_grad`` or
        ``fdsva_so`` take as it is.  ``trajectory=False`` returns the final state ``[B, n]`` only and writes nothing
        else.  ``q0 [n]`` with ``u [T, n]`` gives ``[T, n]`` (``[n]``).  numpy in -> float64 numpy out; tensors stay on
        their device and dtype and run on torch's current stream.

        ``differentiable=True`` (tensors only): the result comes from a ``torch.autograd.Function`` whose backward is
        ``rollout_grad`` on the saved trajectory (once differentiable), so ``loss(q, qd).backward()`` fills ``q0.grad``,
        ``qd0.grad`` and ``u.grad``.  With ``trajectory=False`` the trajectory is still computed and kept for the
        backward pass; the last slice is returned."""
        who, n = "rollout", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator, why="a floating base needs an integrator on SE(3)")
        if differentiable:
            if not all(isinstance(x, torch.Tensor) for x in (q0, qd0, u)):
                raise TypeError("rollout: differentiable=True takes torch tensors (autograd does not see numpy arrays)")
            return _rollout_function()(q0, qd0, u, self, float(dt), float(GRAVITY), integrator, bool(trajectory))
        unb, B, T, shared = _ra.check_shapes(who, n, q0, qd0, u)
        (q0, qd0), cx = _ra.Ctx.from_prep(self._prep(q0, qd0))
        u = cx.tensor(u)
        dev, dtp = cx.dev, cx.dtp
        with torch.cuda.device(dev):
            shape = (T, B, n) if trajectory else (B, n)
            q = torch.empty(shape, device=dev, dtype=dtp)
            qd = torch.empty(shape, device=dev, dtype=dtp)
            self._lib.check(self._fn("rbd_rollout", dtp)(
                self._ptr(q0), self._ptr(qd0), self._ptr(u), int(shared), float(dt), float(GRAVITY), RBD_INTEGRATORS[integrator],
                B, T, self._ptr(q), self._ptr(qd), int(bool(trajectory)), cx.stream()))
        if unb:
            q, qd = q.squeeze(-2), qd.squeeze(-2)
        return cx.to_caller((q, qd))

    # ---- closed-loop rollouts: rbd_rollout_closed_loop, the control law u = u + alpha k + K dx inside the time loop ----
    def rollout_closed_loop(self, q0, qd0, u, q_ref, qd_ref, K, dt, k=None, alpha=1.0, q0_ref=None, qd0_ref=None,
                            u_min=None, u_max=None, GRAVITY=-9.81, integrator="semi_implicit", trajectory=True, row_alpha=None):
        """The forward pass that consumes ``rollout_lqr``'s gains, in ONE kernel launch -> ``(q, qd, u_applied)``: an
        iLQR / DDP line search, a time-varying LQR tracking controller, roll-outs around a feedback policy.  Not part of
        the reference.  With ``x = (q | qd)``, per row and step

            ``dx = x_t - xref_t``;  ``u_t = u[t] + alpha k[t] + K[t] dx``;  clipped to ``[u_min, u_max]`` per joint when
            limits are given (a NaN stays a NaN);  ``qdd = aba(q_t, qd_t, u_t, GRAVITY)``, then ``rollout``'s integrator

        where ``x_0 = (q0, qd0)`` and ``x_t`` is slice ``t - 1`` of the trajectory, and the reference state ``xref_t``
        follows the same rule: ``(q0_ref, qd0_ref)`` -- by default ``(q0, qd0)``, so ``dx_0 = 0``, the iLQR case -- then
        slice ``t - 1`` of ``(q_ref, qd_ref)``, which are exactly what ``rollout`` returned for the nominal (their last
        slice is never read).

        Time-major like ``rollout``: ``q0, qd0 [B, n]``, ``u, q_ref, qd_ref [T, B, n]``, ``K [T, B, n, 2n]`` (the layout
        ``rollout_lqr`` returns), ``k [T, B, n]`` or ``None`` (no feed-forward term), ``u_min, u_max``: scalars or ``[n]``,
        both or neither.  A float ``alpha`` gives ``q, qd, u_applied [T, B, n]`` (``q, qd [B, n]`` with
        ``trajectory=False``; ``u_applied``, the controls actually applied, is ``[T, B, n]`` either way).  A 1-D ``alpha``
        of length ``A`` (sequence, array or tensor) is a line search: ``A B`` rows run against the one nominal -- every
        candidate shares its ``K`` stream -- and the outputs are ``[T, A, B, n]`` (final state ``[A, B, n]``).  Unbatched
        inputs (``q0 [n]``, ``u [T, n]``, ``K [T, n, 2n]``) drop the ``B`` axis.  ``row_alpha [B]`` gives every row its own
        step size instead (it needs ``k`` and the default ``alpha``): the forward pass of an optimiser that accepts or
        rejects per row.  numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's
        current stream.  Fixed-base robots only."""
        who, n = "rollout_closed_loop", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        unb, B, T, _ = _ra.check_shapes(who, n, q0, qd0, u, shared_u=False)
        sq, su = tuple(np.shape(q0)), tuple(np.shape(u))
        _ra.check_named_shapes(who, (("q_ref", q_ref, su), ("qd_ref", qd_ref, su), ("K", K, su + (2 * n,)), ("k", k, su),
                                    ("q0_ref", q0_ref, sq), ("qd0_ref", qd0_ref, sq)), required=("q_ref", "qd_ref", "K"))
        if (q0_ref is None) != (qd0_ref is None):
            raise ValueError(f"{who}: give q0_ref and qd0_ref together, or neither (they default to q0, qd0)")
        _ra.check_limits(who, u_min, u_max, n)
        A = _ra.check_alpha(who, alpha)
        _ra.check_row_alpha(who, row_alpha, alpha, k, sq[:-1])
        (q0, qd0), cx = _ra.Ctx.from_prep(self._prep(q0, qd0))
        u, q_ref, qd_ref, K, k = (cx.tensor(x) for x in (u, q_ref, qd_ref, K, k))
        q0_ref, qd0_ref = (q0, qd0) if q0_ref is None else (cx.tensor(q0_ref), cx.tensor(qd0_ref))
        dev, dtp = cx.dev, cx.dtp
        with torch.cuda.device(dev):
            lo, hi = cx.limits(u_min, u_max, n)
            q0, qd0, al, rows = cx.alpha_rows(q0, qd0, alpha, A, row_alpha, k, B)
            q = torch.empty((T, rows, n) if trajectory else (rows, n), device=dev, dtype=dtp)
            qd = torch.empty_like(q)
            ua = torch.empty((T, rows, n), device=dev, dtype=dtp)
            self._lib.check(self._fn("rbd_rollout_closed_loop", dtp)(
                self._ptr(q0), self._ptr(qd0), self._ptr(u), self._ptr(k), self._ptr(K), self._ptr(q0_ref), self._ptr(qd0_ref),
                self._ptr(q_ref), self._ptr(qd_ref), self._ptr(al), self._ptr(lo), self._ptr(hi), float(dt), float(GRAVITY),
                RBD_INTEGRATORS[integrator], rows, B, T, self._ptr(q), self._ptr(qd), int(bool(trajectory)), self._ptr(ua), cx.stream()))
        outs = []
        for x in (q, qd, ua):
            if A is not None:
                x = x.view(*x.shape[:-2], A, B, n)
            outs.append(x.squeeze(-2) if unb else x)
        return cx.to_caller(tuple(outs))

    # ---- rollouts that return their cost: rbd_rollout_cost, the quadratic cost accumulated inside the time loop ----------
    def rollout_cost(self, q0, qd0, u, dt, cost, K=None, q_ref=None, qd_ref=None, k=None, alpha=1.0, du=None, q0_ref=None,
                     qd0_ref=None, u_min=None, u_max=None, GRAVITY=-9.81, integrator="semi_implicit", row_alpha=None,
                     return_final=False, return_trajectory=False):
        """A rollout, open or closed loop, that returns its cost ``J [B]`` and stores nothing else: the line search of
        iLQR / DDP and the sample costs of a sampling controller (MPPI) in ONE kernel launch.  Not part of the reference.
        ``cost`` is a ``QuadraticCost``; per row and step

            ``u_t = u[t] + alpha k[t] + du[t] + K[t] dx`` (``rollout_closed_loop``'s control law; ``k``, ``du`` and ``K`` are
            each optional), clipped to ``[u_min, u_max]`` when limits are given;  the state advances as in ``rollout``;
            ``J += 1/2 w_u u_t^2 + c_u u_t + 1/2 w_q (q_{t+1} - q_target)^2 + 1/2 w_qd (qd_{t+1} - qd_target)^2`` summed
            over the joints, with ``u_t`` the control applied and slice ``t`` the state after step ``t``

        accumulated in the kernel's precision as one chain per row in a fixed order (per step: the control terms joint
        by joint, then the ``q`` terms, then the ``qd`` terms), so a row's ``J`` depends on that row alone.

        Time-major like ``rollout``: ``q0, qd0 [B, n]``; ``u [T, B_nom, n]`` where ``B_nom`` divides ``B`` (``B_nom = 1``:
        one nominal shared by ``B`` samples); ``K [T, B_nom, n, 2n]`` or ``None`` -- an OPEN loop, in which ``q_ref, qd_ref,
        q0_ref, qd0_ref`` are not used; with ``K``, ``q_ref, qd_ref [T, B_nom, n]`` are required and ``q0_ref, qd0_ref
        [B_nom, n]`` default to ``q0, qd0`` (``B_nom = B`` only).  ``k [T, B_nom, n]``; ``du [T, B, n]``, a perturbation per
        ROW.  The cost's arrays belong to the nominal (``B_nom`` rows).  A float ``alpha`` gives ``J [B]``; a 1-D
        ``alpha`` of length ``A`` runs ``A B`` rows against the one nominal and gives ``J [A, B]`` (``du`` is then
        ``[T, A, B, n]``); ``row_alpha [B]`` gives every row its own step size instead.  ``return_final=True`` ->
        ``(J, q_T, qd_T)``; ``return_trajectory=True`` -> ``(J, q, qd, u_applied)`` with ``rollout_closed_loop``'s shapes (one
        of the two, not both).
        numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's current stream.

        Robots with PRISMATIC joints: nothing here differentiates, but gains that come from ``rollout_lqr`` inherit its
        caveat (``rnea_grad``'s ``dc_dq`` is not the q-derivative for such joints).  Fixed-base robots only."""
        from .cost import QuadraticCost
        who, n = "rollout_cost", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        if not isinstance(cost, QuadraticCost):
            raise TypeError(f"{who}: cost must be a QuadraticCost")
        if return_final and return_trajectory:
            raise ValueError(f"{who}: give return_final or return_trajectory, not both (the final state is the trajectory's last slice)")
        _, B, T, _ = _ra.check_shapes(who, n, q0, qd0, u, unbatched=False, b_nom=True)
        su = tuple(np.shape(u))
        Bn = su[1]
        if K is None:
            if any(x is not None for x in (q_ref, qd_ref, q0_ref, qd0_ref)):
                raise ValueError(f"{who}: q_ref, qd_ref, q0_ref and qd0_ref belong to the feedback term; K is missing")
        else:
            if q_ref is None or qd_ref is None:
                raise ValueError(f"{who}: K needs q_ref and qd_ref (the nominal trajectory)")
            if (q0_ref is None) != (qd0_ref is None):
                raise ValueError(f"{who}: give q0_ref and qd0_ref together, or neither (they default to q0, qd0)")
            if q0_ref is None and Bn != B:
                raise ValueError(f"{who}: a nominal of {Bn} rows against {B} rows needs q0_ref and qd0_ref [{Bn}, {n}]")
        A = _ra.check_alpha(who, alpha)
        _ra.check_row_alpha(who, row_alpha, alpha, k, (B,))
        if A is not None and Bn != B:
            raise ValueError(f"{who}: a 1-D alpha shares one nominal of B rows among its candidates; u has {Bn} rows, q0 {B}")
        lead_du = (T,) + (() if A is None else (A,)) + (B, n)
        _ra.check_named_shapes(who, (("q_ref", q_ref, su), ("qd_ref", qd_ref, su), ("K", K, su + (2 * n,)), ("k", k, su),
                                    ("q0_ref", q0_ref, (Bn, n)), ("qd0_ref", qd0_ref, (Bn, n)), ("du", du, lead_du)))
        _ra.check_limits(who, u_min, u_max, n)
        cd = cost.dense(T, Bn, n)                 # (raises on a shape that is none of the accepted forms)
        (q0, qd0), cx = _ra.Ctx.from_prep(self._prep(q0, qd0))
        u, q_ref, qd_ref, K, k, du = (cx.tensor(x) for x in (u, q_ref, qd_ref, K, k, du))
        cd = {name: cx.tensor(x) for name, x in cd.items()}
        if K is not None:
            q0_ref, qd0_ref = (q0, qd0) if q0_ref is None else (cx.tensor(q0_ref), cx.tensor(qd0_ref))
        store = "trajectory" if return_trajectory else "final" if return_final else None
        dev, dtp = cx.dev, cx.dtp
        with torch.cuda.device(dev):
            lo, hi = cx.limits(u_min, u_max, n)
            q0, qd0, al, rows = cx.alpha_rows(q0, qd0, alpha, A, row_alpha, k, B)
            J = torch.empty((rows,), device=dev, dtype=dtp)
            q = qd = ua = None
            if store is not None:
                q = torch.empty((T, rows, n) if store == "trajectory" else (rows, n), device=dev, dtype=dtp)
                qd = torch.empty_like(q)
            if store == "trajectory":
                ua = torch.empty((T, rows, n), device=dev, dtype=dtp)
            self._lib.check(self._fn("rbd_rollout_cost", dtp)(
                self._ptr(q0), self._ptr(qd0), self._ptr(u), self._ptr(k), self._ptr(K), self._ptr(q0_ref), self._ptr(qd0_ref),
                self._ptr(q_ref), self._ptr(qd_ref), self._ptr(al), self._ptr(du), self._ptr(lo), self._ptr(hi),
                self._ptr(cd["q_target"]), self._ptr(cd["qd_target"]), self._ptr(cd["w_q"]), self._ptr(cd["w_qd"]),
                int(cost.terminal_state_only), self._ptr(cd["w_u"]), self._ptr(cd["c_u"]), float(dt), float(GRAVITY),
                RBD_INTEGRATORS[integrator], rows, Bn, T, self._ptr(J), self._ptr(q), self._ptr(qd),
                int(store == "trajectory"), self._ptr(ua), cx.stream()))
        outs = [J if A is None else J.view(A, B)]
        for x in (q, qd, ua):
            if x is not None:
                outs.append(x if A is None else x.view(*x.shape[:-2], A, B, n))
        return cx.to_caller(outs[0] if store is None else tuple(outs))

    # ---- iLQR: rollout_lqr -> rollout_cost (line search) -> rollout_closed_loop (forward pass), per-row accept / reject ----
    def ilqr(self, q0, qd0, u, dt, cost, iters=10, alphas=(1, .5, .25, .125, .03125, .0078125), reg=0.0, u_min=None,
             u_max=None, GRAVITY=-9.81, integrator="semi_implicit"):
        """``iters`` iterations of iLQR on ``B`` independent problems -> ``IlqrResult(u, q, qd [T, B, n], cost [iters + 1, B],
        alpha [iters, B], dV [iters, B, 2], status [iters, B])``.  Not part of the reference.  Per iteration, three
        launches and some elementwise glue, with no host synchronisation:

          1. ``cost.derivatives`` at the nominal and ``rollout_lqr(..., q=q, qd=qd, reg=reg)`` -> ``k, K, dV, status``;
          2. ``rollout_cost`` over all ``alphas`` in one launch -> ``Jc [A, B]``; per row the lowest-index minimum, a NaN
             counting as +inf; the row ACCEPTS when that minimum is below its current cost;
          3. one ``rollout_closed_loop(row_alpha=...)`` with the accepted step sizes (0 for a rejected row); accepted rows
             take the new ``u, q, qd`` and cost, rejected rows keep theirs (selected explicitly).

        ``cost[i]`` is the cost entering iteration ``i`` (``cost[0]``: the start's, from an open-loop ``rollout_cost``), non-
        increasing per row by construction; ``alpha`` records 0 for a rejected row; ``dV, status`` are ``rollout_lqr``'s.
        ``q0, qd0 [B, n]``, ``u [T, B, n]``, ``cost``: a ``QuadraticCost``; ``reg``: a float or ``iters`` floats (one
        regularisation for every row); ``u_min, u_max`` clip the controls applied (the backward pass does not know about
        them).  numpy in -> float64 numpy out; tensors stay on their device and dtype.

        Robots with PRISMATIC joints: ``rnea_grad``'s ``dc_dq`` reproduces the reference and is not the q-derivative for
        such joints (see ``rollout_lqr``), so the gains are not those of the true linearisation there; the line search
        still never accepts a step that raises the cost.  Fixed-base robots only."""
        from .cost import QuadraticCost
        who, n = "ilqr", self.n
        _ra.check_base_integrator(who, self.model.floating)
        if not isinstance(cost, QuadraticCost):
            raise TypeError(f"{who}: cost must be a QuadraticCost")
        B = _ra.check_state(who, n, q0, qd0, unbatched=False)[0]
        _ra.check_u_steps(who, n, u, B)
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"{who}: iters < 0")
        if np.ndim(alphas) != 1 or len(alphas) == 0:
            raise ValueError(f"{who}: alphas must be a non-empty 1-D sequence of step sizes")
        regs = [float(reg)] * iters if np.ndim(reg) == 0 else [float(r) for r in reg]
        if len(regs) != iters:
            raise ValueError(f"{who}: reg must be a float or a sequence of iters = {iters} floats, got {len(regs)}")
        cx, q0, qd0, u, _, cost = _ra.Ctx.upload(q0, qd0, u, None, cost, strict=False)
        dev, dtp = cx.dev, cx.dtp
        kw = dict(GRAVITY=GRAVITY, integrator=integrator)
        lim = dict(u_min=u_min, u_max=u_max)
        with torch.cuda.device(dev):
            al = torch.as_tensor(np.asarray(alphas, dtype=np.float64), device=dev).to(dtp)      # made once, before the loop
            A = al.shape[0]
            first = torch.arange(A, 0, -1, device=dev)[:, None]       # weights that make the LOWEST index win a tie
            inf = torch.full((), float("inf"), device=dev, dtype=dtp)
            zero = torch.zeros((), device=dev, dtype=dtp)
            J, q, qd, u = self.rollout_cost(q0, qd0, u, dt, cost, return_trajectory=True, **lim, **kw)
            hist, h_al, h_dV, h_st = [J], [], [], []
            for it in range(iters):
                d = cost.derivatives(q, qd, u)
                k, K, _, _, dV, status = self.rollout_lqr(q0, qd0, u, dt, reg=regs[it], q=q, qd=qd, **d, **kw)
                Jc = self.rollout_cost(q0, qd0, u, dt, cost, K=K, q_ref=q, qd_ref=qd, k=k, alpha=al, **lim, **kw)
                Jc = torch.where(torch.isnan(Jc), inf, Jc)
                J_best = Jc.min(dim=0).values
                idx = ((Jc == J_best[None]) * first).argmax(dim=0)
                accept = J_best < J
                ra = torch.where(accept, al[idx], zero)
                qn, qdn, un = self.rollout_closed_loop(q0, qd0, u, q, qd, K, dt, k=k, row_alpha=ra, **lim, **kw)
                sel = accept[None, :, None]
                u, q, qd = torch.where(sel, un, u), torch.where(sel, qn, q), torch.where(sel, qdn, qd)
                J = torch.where(accept, J_best, J)
                hist.append(J)
                h_al.append(ra)
                h_dV.append(dV)
                h_st.append(status)
            res = IlqrResult(u, q, qd, torch.stack(hist),
                             torch.stack(h_al) if iters else torch.empty((0, B), device=dev, dtype=dtp),
                             torch.stack(h_dV) if iters else torch.empty((0, B, 2), device=dev, dtype=dtp),
                             torch.stack(h_st) if iters else torch.empty((0, B), device=dev, dtype=torch.int32))
        return cx.to_caller(res)

    # ---- MPPI: rollout_cost (the sample costs) -> mppi_update (softmin weights, weighted sum of the perturbations) ----
    def mppi_update(self, J, du, u, lam, u_min=None, u_max=None, return_weights=False):
        """The update of a sampling controller from the sample costs ``rollout_cost`` wrote -> ``MppiUpdate(u, w, ess,
        status)``.  Not part of the reference.  ``P`` independent problems with ``S`` samples each, in ``rollout_cost``'s
        row layout (row ``s P + p`` is sample ``s`` of problem ``p``): ``J [S, P]``, ``du [T, S, P, n]``, ``u [T, P, n]``,
        ``lam`` a float or ``[P]``.  Per problem, in the inputs' precision:

            ``Jm = min_s J`` (a NaN counts as +inf);  ``e_s = exp(-(J_s - Jm) / lam)``;  ``eta = sum e``;  ``w = e / eta``;
            ``ess = eta^2 / sum e^2``;  ``d_s = du_s``, or with limits ``clamp(u + du_s) - u`` -- the perturbation
            ``rollout_cost`` applied;  ``u_new = u + (sum_s e_s d_s) / eta``, clamped once more when limits are given

        ``status [P]`` (int32): 0; 1 when ``Jm`` is not finite (every sample NaN or +inf, or a -inf among them); 2 when
        ``lam`` is not finite and positive.  Where it is not 0 the problem keeps its ``u`` (clamped), ``w = 0``, ``ess = 0``.
        A NaN in ``du`` poisons the ``(t, j)`` outputs of its own problem and no other.  The sums run in a fixed order that
        depends on ``S`` alone (chunks of ``RBD_MPPI_CHUNK`` samples), so a problem's result does not depend
        on ``P``, ``T`` or ``return_weights``.  ``w [S, P]`` is ``None`` unless ``return_weights``.
        numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's current stream.
        Fixed-base robots only."""
        who, n = "mppi_update", self.n
        _ra.check_base_integrator(who, self.model.floating)
        sJ = tuple(np.shape(J))
        if len(sJ) != 2 or 0 in sJ:
            raise ValueError(f"{who}: J must be [S, P] with S, P > 0, got {sJ}")
        S, P = sJ
        T = _ra.check_u_steps(who, n, u, P)
        _ra.check_named_shapes(who, (("du", du, (T, S, P, n)),))
        if tuple(np.shape(lam)) not in ((), (P,)):
            raise ValueError(f"{who}: lam must be a float or [{P}], got shape {tuple(np.shape(lam))}")
        _ra.check_limits(who, u_min, u_max, n)
        cx = _ra.Ctx.from_first(J, du, u)
        J, du, u = (cx.tensor(x) for x in (J, du, u))
        dev, dtp, esz, sfx = cx.dev, cx.dtp, cx.esz, cx.sfx
        with torch.cuda.device(dev):
            lam_t = cx.small(lam).expand(P).contiguous()
            lo, hi = cx.limits(u_min, u_max, n)
            u_new = torch.empty((T, P, n), device=dev, dtype=dtp)
            w = torch.empty((S, P), device=dev, dtype=dtp) if return_weights else None
            ess = torch.empty((P,), device=dev, dtype=dtp)
            status = torch.empty((P,), device=dev, dtype=torch.int32)
            lib = self._lib.resolve("rbd_mppi_update", sfx)     # ONE resolution: workspace size and entry point from the same library
            wsb = int(lib.rbd_mppi_update_workspace_bytes(S, P, T, esz))
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
            self._lib.check(getattr(lib, f"rbd_mppi_update_{sfx}")(
                self._ptr(J), self._ptr(du), self._ptr(u), self._ptr(lam_t), self._ptr(lo), self._ptr(hi), S, P, T, self._ptr(u_new),
                self._ptr(w), self._ptr(ess), self._ptr(status), ws.data_ptr(), wsb, cx.stream()))
        return cx.to_caller(MppiUpdate(u_new, w, ess, status))

    def mppi(self, q0, qd0, u, dt, cost, iters=1, samples=1024, sigma=0.1, lam=1.0, noise=None, generator=None, u_min=None,
             u_max=None, GRAVITY=-9.81, integrator="semi_implicit"):
        """``iters`` iterations of MPPI on ``P`` independent problems -> ``MppiResult(u, q, qd [T, P, n], cost [iters + 1, P],
        ess [iters, P], status [iters, P])``.  Not part of the reference.  Per iteration, with ``S = samples``:

          1. the noise ``eps [T, S, P, n]``: ``torch.randn(..., generator=generator)``, or ``noise[i]`` when ``noise [iters, T,
             S, P, n]`` is given (``S`` is then its third extent);  ``du = sigma eps`` with ``du[:, 0] = 0`` -- sample 0 is
             always the nominal, so its cost is the nominal's and needs no launch of its own;
          2. one ``rollout_cost`` of the ``S P`` rows against the ``P`` nominals -> ``J [S, P]``;
          3. one ``mppi_update`` -> the new ``u``, ``ess``, ``status``

        with no host synchronisation.  ``cost[i] = J[0]`` of iteration ``i``, the cost of the nominal entering it; after
        the loop one open-loop ``rollout_cost(return_trajectory=True)`` gives ``q, qd`` and ``cost[iters]``.
        ``q0, qd0 [P, n]``, ``u [T, P, n]``, ``cost``: a ``QuadraticCost``; ``sigma``: a float, ``[n]`` or ``[T, n]``; ``lam``:
        a float or ``[P]``; ``u_min, u_max`` clip the controls applied, and the update averages the clipped perturbations.
        MPPI's control-cost coupling ``lam ubar^T Sigma^-1 du`` is expressed through ``QuadraticCost``'s ``c_u`` (``c_u =
        lam ubar / sigma^2`` per step and joint): ``c_u (ubar + du)`` differs from it by ``c_u ubar``, a constant per
        problem, which the softmin does not see.  Not included: shifting the nominal between the steps of a receding
        horizon, and feedback gains around the samples.
        numpy in -> float64 numpy out; tensors stay on their device and dtype.  Fixed-base robots only."""
        from .cost import QuadraticCost
        who, n = "mppi", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        if not isinstance(cost, QuadraticCost):
            raise TypeError(f"{who}: cost must be a QuadraticCost")
        sq = tuple(np.shape(q0))                  # (inline: P > 0 is part of this method's rule and message)
        if len(sq) != 2 or sq[1] != n or sq[0] == 0 or tuple(np.shape(qd0)) != sq:
            raise ValueError(f"{who}: q0 and qd0 must both be [P, {n}] with P > 0, got {sq} and {tuple(np.shape(qd0))}")
        P = sq[0]
        T = _ra.check_u_steps(who, n, u, P)
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"{who}: iters < 0")
        if noise is not None:
            if generator is not None:
                raise ValueError(f"{who}: give noise or generator, not both")
            sn = tuple(np.shape(noise))
            if len(sn) != 5 or sn[:2] != (iters, T) or sn[3:] != (P, n) or sn[2] == 0:
                raise ValueError(f"{who}: noise must be [iters = {iters}, {T}, S, {P}, {n}] with S > 0, got {sn}")
            S = sn[2]
        else:
            S = int(samples)
            if S < 1:
                raise ValueError(f"{who}: samples < 1")
        if tuple(np.shape(sigma)) not in ((), (n,), (T, n)):
            raise ValueError(f"{who}: sigma must be a float, [{n}] or [{T}, {n}], got shape {tuple(np.shape(sigma))}")
        if tuple(np.shape(lam)) not in ((), (P,)):
            raise ValueError(f"{who}: lam must be a float or [{P}], got shape {tuple(np.shape(lam))}")
        _ra.check_limits(who, u_min, u_max, n)
        cx, q0, qd0, u, noise, cost = _ra.Ctx.upload(q0, qd0, u, noise, cost, strict=True)
        dev, dtp = cx.dev, cx.dtp
        kw = dict(GRAVITY=GRAVITY, integrator=integrator)
        with torch.cuda.device(dev):
            lo, hi = cx.limits(u_min, u_max, n)                        # the small tensors are made once, before the loop
            lim = dict(u_min=lo, u_max=hi)
            sg = cx.small(sigma)
            if sg.dim() == 2:
                sg = sg[:, None, None, :]
            lam_t = cx.small(lam).expand(P).contiguous()
            q0s, qd0s = q0.repeat(S, 1), qd0.repeat(S, 1)              # row s P + p starts where problem p does
            hist, h_ess, h_st = [], [], []
            for it in range(iters):
                eps = noise[it] if noise is not None else torch.randn((T, S, P, n), generator=generator, device=dev, dtype=dtp)
                du = sg * eps
                du[:, 0] = 0
                J = self.rollout_cost(q0s, qd0s, u, dt, cost, du=du.view(T, S * P, n), **lim, **kw).view(S, P)
                upd = self.mppi_update(J, du, u, lam_t, **lim)
                u = upd.u
                hist.append(J[0])
                h_ess.append(upd.ess)
                h_st.append(upd.status)
            Jf, q, qd, _ = self.rollout_cost(q0, qd0, u, dt, cost, return_trajectory=True, **lim, **kw)
            hist.append(Jf)
            res = MppiResult(u, q, qd, torch.stack(hist),
                             torch.stack(h_ess) if iters else torch.empty((0, P), device=dev, dtype=dtp),
                             torch.stack(h_st) if iters else torch.empty((0, P), device=dev, dtype=torch.int32))
        return cx.to_caller(res)

    # ---- reverse-mode gradient of a rollout: rbd_rollout_grad (aba, rnea_grad, minv per chunk + one scan launch) ------
    def rollout_grad(self, q0, qd0, u, dt, grad_q=None, grad_qd=None, GRAVITY=-9.81, integrator="semi_implicit",
                     q=None, qd=None, workspace_bytes=None):
        """Reverse-mode gradient of ``rollout``: for a scalar cost ``L`` of the returned slices, with
        ``grad_q[t] = dL/dq[t]`` and ``grad_qd[t] = dL/dqd[t]`` (the direct partials), ->
        ``(grad_u, grad_q0, grad_qd0) = (dL/du, dL/dq0, dL/dqd0)``.  Not part of the reference.

        The backward recursion over time runs as one HIP launch per chunk of the horizon with the adjoint on chip
        (``rbd_rollout_adj.h``), after ``aba``, ``rnea_grad`` and ``minv`` on the chunk's flat rows; it forms
        vector-Jacobian products only, never ``forward_dynamics_grad``'s ``-Minv dc_du``.

        Conventions are ``rollout``'s: time-major, ``q0, qd0 [B, n]``, ``u [T, B, n]`` -> ``grad_u [T, B, n]``; a shared
        ``u [T, n]`` is expanded and ``grad_u`` summed over ``B`` to ``[T, n]``; ``q0 [n]`` with ``u [T, n]`` is one row.
        ``grad_q, grad_qd``: ``[T, B, n]``, or ``[B, n]`` = the gradient with respect to the final state alone (a
        terminal cost); at least one must be given, both in the same form.  ``q, qd``: the trajectory ``rollout``
        returned for these inputs (``[T, B, n]``); computed here when omitted.  ``workspace_bytes``: device scratch for
        the linearisation, which decides how many steps one chunk holds (default: all of them, capped at 1 GiB).
        numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's current stream.

        Robots with PRISMATIC joints: ``rnea_grad``'s ``dc_dq`` reproduces the reference and is not the q-derivative for
        such joints (see ``fdsva_so``), and this gradient inherits that: it is the true gradient on robots with
        revolute joints only.  Fixed-base robots only."""
        who, n = "rollout_grad", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        unb, B, T, shared = _ra.check_shapes(who, n, q0, qd0, u)
        final = _ra.rollg_g_shape(grad_q, grad_qd, T, B, n, unb, who)
        _ra.check_trajectory(who, q, qd, T, B, n, unb)
        _ra.check_workspace_request(who, workspace_bytes)
        (q0, qd0), cx = _ra.Ctx.from_prep(self._prep(q0, qd0))
        u, gq, gqd, q, qd = (cx.tensor(x) for x in (u, grad_q, grad_qd, q, qd))
        dev, dtp, esz, sfx = cx.dev, cx.dtp, cx.esz, cx.sfx
        with torch.cuda.device(dev):
            if shared:
                u = u[:, None, :].expand(T, B, n).contiguous()
            if q is None:
                q, qd = self.rollout(q0, qd0, u, dt, GRAVITY, integrator)
            gu = torch.empty((T, B, n), device=dev, dtype=dtp)
            gq0 = torch.empty((B, n), device=dev, dtype=dtp)
            gqd0 = torch.empty((B, n), device=dev, dtype=dtp)
            lib = self._lib.resolve("rbd_rollout_grad", sfx)    # ONE resolution: workspace size and entry point from the same library
            wsb = _ra.workspace_bytes(lib.rbd_rollout_grad_workspace_bytes, B, T, esz, workspace_bytes)
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
            self._lib.check(getattr(lib, f"rbd_rollout_grad_{sfx}")(
                self._ptr(q0), self._ptr(qd0), self._ptr(u), self._ptr(q), self._ptr(qd), self._ptr(gq), self._ptr(gqd), int(final),
                float(dt), float(GRAVITY), RBD_INTEGRATORS[integrator], B, T, self._ptr(gu), self._ptr(gq0), self._ptr(gqd0),
                ws.data_ptr(), wsb, cx.stream()))
            if shared:
                gu = gu.sum(1)
        if unb:
            gq0, gqd0 = gq0[0], gqd0[0]
        return cx.to_caller((gu, gq0, gqd0))

    def rollout_adjoint(self, dc_du, Minv, dt, grad_q=None, grad_qd=None, integrator="semi_implicit", lam=None):
        """The scan of ``rollout_grad`` alone (``rbd_rollout_adjoint``), for a caller who holds the linearisation:
        ``dc_du [T, B, n, 2n]`` (``rnea_grad``) and ``Minv [T, B, n, n]`` (dense) of the ``T`` steps, time-major ->
        ``(grad_u [T, B, n], lam [B, 2n])``.  ``lam = (lq | lqd)`` is the adjoint entering at the END of these steps
        (default zeros) and is returned as it leaves at their beginning -- ``(dL/dq0 | dL/dqd0)`` when they start the
        horizon; a contiguous tensor is updated in place.  A horizon may be split: the later steps first, ``lam`` carried
        over, bit-identical to one call.  ``grad_q, grad_qd``: ``[T, B, n]``, or ``[B, n]`` for the last of these steps
        alone.  numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's current stream.
        The prismatic-joint caveat of ``rollout_grad`` applies.  Fixed-base robots only."""
        who, n = "rollout_adjoint", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        T, B = _ra.check_linearisation(who, dc_du, Minv, n)
        final = _ra.rollg_g_shape(grad_q, grad_qd, T, B, n, False, who)
        _ra.check_named_shapes(who, (("lam", lam, (B, 2 * n)),))
        cx = _ra.Ctx.from_first(dc_du)
        dc_du, Minv, gq, gqd = (cx.tensor(x) for x in (dc_du, Minv, grad_q, grad_qd))
        dev, dtp = cx.dev, cx.dtp
        with torch.cuda.device(dev):
            lam_t = torch.zeros((B, 2 * n), device=dev, dtype=dtp) if lam is None else cx.tensor(lam)
            gu = torch.empty((T, B, n), device=dev, dtype=dtp)
            self._lib.check(self._fn("rbd_rollout_adjoint", dtp)(
                self._ptr(dc_du), self._ptr(Minv), self._ptr(gq), self._ptr(gqd), int(final), float(dt),
                RBD_INTEGRATORS[integrator], B, T, self._ptr(lam_t), self._ptr(gu), cx.stream()))
        return cx.to_caller((gu, lam_t))

    # ---- backward pass of iLQR / DDP over a rollout: rbd_rollout_lqr (aba, rnea_grad, minv per chunk + the Riccati scan) ----
    def rollout_lqr(self, q0, qd0, u, dt, grad_q=None, grad_qd=None, hess_q=None, hess_qd=None, grad_u=None, hess_u=None,
                    reg=0.0, GRAVITY=-9.81, integrator="semi_implicit", q=None, qd=None, workspace_bytes=None):
        """Backward pass of iLQR / DDP / time-varying LQR along a rollout: from the linearisation of every step and a
        quadratic cost model -> ``(k [T, B, n], K [T, B, n, 2n], lam [B, 2n], P [B, 2n, 2n], dV [B, 2], status [B])``: the
        feed-forward terms and feedback gains of ``u = u + alpha k + K dx``, the value function's gradient and Hessian
        at the initial state, the expected cost change ``alpha dV[0] + alpha^2 dV[1]`` and, per row, the number of steps
        whose ``Quu + reg I`` could not be factored (their ``k`` and ``K`` are zero).  Not part of the reference.

        ``aba``, ``rnea_grad`` and ``minv`` run on the trajectory's flat rows per chunk of the horizon; the Riccati
        recursion over time is then one HIP launch per chunk with ``lam`` and ``P`` on chip (``rbd_rollout_lqr.h``; the
        recursion is written out in ``include/rbd_hip.h``).

        Conventions are ``rollout_grad``'s: time-major, slice ``t`` is the state after step ``t + 1``; state costs attach
        to slices, control costs to ``u[t]``.  ``grad_q, grad_qd, hess_q, hess_qd``: gradient and DIAGONAL Hessian of the
        state cost, all ``[T, B, n]`` or all ``[B, n]`` (last slice only); any may be omitted.  ``grad_u [T, B, n]``
        (optional), ``hess_u [T, B, n]`` or ``[n]`` (shared; required).  ``reg >= 0`` is added to ``Quu``'s diagonal in the
        factorisation.  A shared ``u [T, n]`` is expanded; the gains stay per row.  ``q0 [n]`` with ``u [T, n]`` is one
        row.  ``q, qd``: the trajectory ``rollout`` returned for these inputs; computed here when omitted.
        ``workspace_bytes``: device scratch for the linearisation, which decides how many steps one chunk holds
        (default: all of them, capped at 1 GiB).  A full terminal Hessian goes through ``rollout_riccati``'s ``P``.
        numpy in -> float64 numpy out; tensors stay on their device and dtype and run on torch's current stream.

        Robots with PRISMATIC joints: ``rnea_grad``'s ``dc_dq`` reproduces the reference and is not the q-derivative for
        such joints (see ``rollout_grad``), and the gains inherit that: they belong to the true linearisation on robots
        with revolute joints only.  Fixed-base robots only."""
        who, n = "rollout_lqr", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        unb, B, T, shared = _ra.check_shapes(who, n, q0, qd0, u)
        final, hu_shared = _ra.lqr_cost_shapes(T, B, n, unb, who, grad_q, grad_qd, hess_q, hess_qd, grad_u, hess_u, reg)
        _ra.check_trajectory(who, q, qd, T, B, n, unb)
        _ra.check_workspace_request(who, workspace_bytes)
        (q0, qd0), cx = _ra.Ctx.from_prep(self._prep(q0, qd0))
        u, gq, gqd, hq, hqd, gu, hu, q, qd = (cx.tensor(x) for x in (u, grad_q, grad_qd, hess_q, hess_qd, grad_u, hess_u, q, qd))
        dev, dtp, esz, sfx = cx.dev, cx.dtp, cx.esz, cx.sfx
        with torch.cuda.device(dev):
            if shared:
                u = u[:, None, :].expand(T, B, n).contiguous()
            if q is None:
                q, qd = self.rollout(q0, qd0, u, dt, GRAVITY, integrator)
            k = torch.empty((T, B, n), device=dev, dtype=dtp)
            K = torch.empty((T, B, n, 2 * n), device=dev, dtype=dtp)
            lam = torch.empty((B, 2 * n), device=dev, dtype=dtp)
            P = torch.empty((B, 2 * n, 2 * n), device=dev, dtype=dtp)
            dV = torch.empty((B, 2), device=dev, dtype=dtp)
            status = torch.empty((B,), device=dev, dtype=torch.int32)
            lib = self._lib.resolve("rbd_rollout_lqr", sfx)     # ONE resolution: workspace size and entry point from the same library
            wsb = _ra.workspace_bytes(lib.rbd_rollout_lqr_workspace_bytes, B, T, esz, workspace_bytes)
            ws = torch.empty((max(wsb, 1),), device=dev, dtype=torch.uint8)
            self._lib.check(getattr(lib, f"rbd_rollout_lqr_{sfx}")(
                self._ptr(q0), self._ptr(qd0), self._ptr(u), self._ptr(q), self._ptr(qd), self._ptr(gq), self._ptr(gqd),
                self._ptr(hq), self._ptr(hqd), int(final), self._ptr(gu), self._ptr(hu), int(hu_shared), float(reg), float(dt),
                float(GRAVITY), RBD_INTEGRATORS[integrator], B, T, self._ptr(k), self._ptr(K), self._ptr(lam), self._ptr(P),
                self._ptr(dV), self._ptr(status), ws.data_ptr(), wsb, cx.stream()))
        out = (k, K, lam, P, dV, status)
        if unb:
            out = (k[:, 0], K[:, 0], lam[0], P[0], dV[0], status[0])
        return cx.to_caller(out)

    def rollout_riccati(self, dc_du, Minv, dt, grad_q=None, grad_qd=None, hess_q=None, hess_qd=None, grad_u=None, hess_u=None,
                        reg=0.0, integrator="semi_implicit", lam=None, P=None, dV=None, status=None):
        """The scan of ``rollout_lqr`` alone (``rbd_rollout_riccati``), for a caller who holds the linearisation:
        ``dc_du [T, B, n, 2n]`` (``rnea_grad``) and ``Minv [T, B, n, n]`` (dense, symmetric) of the ``T`` steps, time-major
        -> ``(k [T, B, n], K [T, B, n, 2n], lam [B, 2n], P [B, 2n, 2n], dV [B, 2], status [B] int32)``.

        ``lam, P, dV, status`` are the value function entering at the END of these steps (default zeros; a full terminal
        Hessian, e.g. a Gauss-Newton ``J^T J``, goes in through ``P``, which must be symmetric) and are returned as they
        leave at their beginning; contiguous tensors are updated in place.  A horizon may be split: the later steps first,
        the four carried over, bit-identical to one call.  Costs as in ``rollout_lqr``; the ``[B, n]`` form of the state
        costs belongs to the last of THESE steps.  numpy in -> float64 numpy out; tensors stay on their device and dtype
        and run on torch's current stream.  The prismatic-joint caveat of ``rollout_grad`` applies to a linearisation
        that comes from ``rnea_grad``.  Fixed-base robots only."""
        who, n = "rollout_riccati", self.n
        _ra.check_base_integrator(who, self.model.floating, integrator)
        T, B = _ra.check_linearisation(who, dc_du, Minv, n)
        final, hu_shared = _ra.lqr_cost_shapes(T, B, n, False, who, grad_q, grad_qd, hess_q, hess_qd, grad_u, hess_u, reg)
        _ra.check_named_shapes(who, (("lam", lam, (B, 2 * n)), ("P", P, (B, 2 * n, 2 * n)), ("dV", dV, (B, 2)), ("status", status, (B,))))
        cx = _ra.Ctx.from_first(dc_du)
        dc_du, Minv, gq, gqd, hq, hqd, gu, hu = (cx.tensor(x) for x in (dc_du, Minv, grad_q, grad_qd, hess_q, hess_qd, grad_u, hess_u))
        dev, dtp = cx.dev, cx.dtp
        with torch.cuda.device(dev):
            lam_t = torch.zeros((B, 2 * n), device=dev, dtype=dtp) if lam is None else cx.tensor(lam)
            P_t = torch.zeros((B, 2 * n, 2 * n), device=dev, dtype=dtp) if P is None else cx.tensor(P)
            dV_t = torch.zeros((B, 2), device=dev, dtype=dtp) if dV is None else cx.tensor(dV)
            st_t = torch.zeros((B,), device=dev, dtype=torch.int32) if status is None else cx.tensor(status, torch.int32)
            k = torch.empty((T, B, n), device=dev, dtype=dtp)
            K = torch.empty((T, B, n, 2 * n), device=dev, dtype=dtp)
            self._lib.check(self._fn("rbd_rollout_riccati", dtp)(
                self._ptr(dc_du), self._ptr(Minv), self._ptr(gq), self._ptr(gqd), self._ptr(hq), self._ptr(hqd), int(final),
                self._ptr(gu), self._ptr(hu), int(hu_shared), float(reg), float(dt), RBD_INTEGRATORS[integrator], B, T,
                self._ptr(lam_t), self._ptr(P_t), self._ptr(dV_t), self._ptr(st_t), self._ptr(k), self._ptr(K), cx.stream()))
        return cx.to_caller((k, K, lam_t, P_t, dV_t, st_t))

    # ---- end-effector kinematics (RBDReference.py:190-386): rbd_ee_pose, one launch per <= 16 sites -----------------
    def _ee_plan(self, ee_joint_names, ee_offsets):
        """Site table of a selection, resolved once and cached: ``(chunks of (site_body int32 [k], site_T float64 [k, 12]),
        offset float64 [4], n_sites)`` in the reference's order -- every movable joint as given, then every fixed joint
        (``select_end_effector_joints``, :190-210; :263-273)."""
        if self.model.floating:
            raise NotImplementedError("end-effector kinematics: fixed-base robots only (the reference's end_effector_pose "
                                      "has no floating-base support, RBDReference.py:217)")
        o = np.asarray(ee_offsets[0], dtype=np.float64).reshape(-1)
        if o.size != 4:
            raise ValueError(f"ee_offsets[0] must hold 4 numbers (x, y, z, 1), got {o.size}")
        names = None if ee_joint_names is None else (ee_joint_names,) if isinstance(ee_joint_names, str) else tuple(ee_joint_names)
        key = (names, o.tobytes())
        cache = self.__dict__.setdefault("_ee_plans", {})
        plan = cache.get(key)
        if plan is not None:
            return plan
        r = self.robot
        frame = getattr(r, "link_frame_in_body", None)

        def link_in_body(i):
            T = np.eye(4)
            if frame is not None:
                T[:3, :3] = frame(i)
            return T
        if names is None:
            sites = [(int(j), link_in_body(int(j))) for j in r.get_leaf_nodes()]
        else:
            mov, fix = [], []
            for nm in names:
                j = r.get_joint_by_name(nm)
                if j is not None:
                    mov.append((int(j.get_id()), link_in_body(int(j.get_id()))))
                    continue
                fj = r.get_fixed_joint_by_name(nm)
                if fj is None:
                    raise ValueError("Could not find joint or fixed joint named: " + str(nm))
                body = int(r.get_joint_by_name(fj.parent_name).get_id())
                fix.append((body, link_in_body(body) @ np.asarray(fj.get_transformation_matrix_hom(), dtype=np.float64)))
            sites = mov + fix
        from ._lib import RBD_EE_MAX_SITES
        chunks = []
        for k in range(0, len(sites), RBD_EE_MAX_SITES):
            part = sites[k:k + RBD_EE_MAX_SITES]
            chunks.append((np.ascontiguousarray([b for b, _ in part], dtype=np.int32),
                           np.ascontiguousarray([T[:3, :].reshape(12) for _, T in part], dtype=np.float64)))
        plan = (chunks, np.ascontiguousarray(o), len(sites))
        if len(cache) >= 64:
            cache.pop(next(iter(cache)))
        cache[key] = plan
        return plan

    def _ee(self, q, ee_joint_names, ee_offsets, want_pose, want_grad):
        chunks, off, ns = self._ee_plan(ee_joint_names, ee_offsets)
        (q,), unb, is_np, dev, dt = self._prep(q)
        B, n = q.shape[0], self.n
        sfx = "f32" if dt == torch.float32 else "f64"
        with torch.cuda.device(dev):
            pose = torch.empty((B, ns, 6), device=dev, dtype=dt) if want_pose else None
            dpose = torch.empty((B, ns, 6, n), device=dev, dtype=dt) if want_grad else None
            st = torch.cuda.current_stream(dev).cuda_stream
            fn = self._lib.fn("rbd_ee_pose", sfx)
            if len(chunks) == 1:
                body, T = chunks[0]
                self._lib.check(fn(self._ptr(q), B, body.ctypes.data, T.ctypes.data, off.ctypes.data, len(body),
                                   self._ptr(pose), self._ptr(dpose), st))
            else:                                 # > RBD_EE_MAX_SITES sites: one launch per chunk into its own buffers
                ps, ds = [], []
                for body, T in chunks:
                    k = len(body)
                    p = torch.empty((B, k, 6), device=dev, dtype=dt) if want_pose else None
                    d = torch.empty((B, k, 6, n), device=dev, dtype=dt) if want_grad else None
                    self._lib.check(fn(self._ptr(q), B, body.ctypes.data, T.ctypes.data, off.ctypes.data, k,
                                       self._ptr(p), self._ptr(d), st))
                    ps.append(p); ds.append(d)
                if want_pose:
                    torch.cat(ps, dim=1, out=pose)
                if want_grad:
                    torch.cat(ds, dim=1, out=dpose)
        return pose, dpose, unb, is_np

    @staticmethod
    def _ee_ret(x, unb, is_np, col):
        """Batched: the [B, n_ee, ...] array / tensor.  One configuration: the reference's list of (6, 1) / (6, n)
        per end effector (np.matrix for numpy inputs, as the reference's np.vstack / np.hstack of matrices gives)."""
        if not unb:
            return x.cpu().numpy() if is_np else x
        x = x[0]
        if is_np:
            x = x.cpu().numpy()
            return [np.matrix(e.reshape(6, 1) if col else e) for e in x]
        return [e.reshape(6, 1) if col else e for e in x]

    def end_effector_pose(self, q, ee_joint_names=None, ee_offsets=[np.matrix([[0, 0, 0, 1]])]):  # noqa: B006 (reference signature)
        """RBDReference.end_effector_pose (``RBDReference.py:220-274``): per end effector ``[x, y, z, roll, pitch, yaw]``.
        ``ee_joint_names=None``: every leaf joint; else movable joints in the given order, then fixed joints.  Only
        ``ee_offsets[0]`` is used, for every end effector, as in the reference (:245).  ``q [n]`` -> list of (6, 1);
        ``q [B, n]`` -> ``[B, n_ee, 6]``."""
        pose, _, unb, is_np = self._ee(q, ee_joint_names, ee_offsets, True, False)
        return self._ee_ret(pose, unb, is_np, True)

    def end_effector_pose_gradient(self, q, ee_joint_names=None, ee_offsets=[np.matrix([[0, 0, 0, 1]])]):  # noqa: B006
        """RBDReference.end_effector_pose_gradient (``RBDReference.py:286-386``): d pose / d q per end effector, zero
        columns for joints off its chain.  ``q [n]`` -> list of (6, n); ``q [B, n]`` -> ``[B, n_ee, 6, n]``."""
        _, dpose, unb, is_np = self._ee(q, ee_joint_names, ee_offsets, False, True)
        return self._ee_ret(dpose, unb, is_np, False)

    def end_effector_pose_and_gradient(self, q, ee_joint_names=None, ee_offsets=[np.matrix([[0, 0, 0, 1]])]):  # noqa: B006
        """``(end_effector_pose(...), end_effector_pose_gradient(...))`` from ONE launch (like ``rnea_and_grad``)."""
        pose, dpose, unb, is_np = self._ee(q, ee_joint_names, ee_offsets, True, True)
        return self._ee_ret(pose, unb, is_np, True), self._ee_ret(dpose, unb, is_np, False)
