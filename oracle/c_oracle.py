"""ctypes front-end of oracle/rbd_oracle.c -- TEST INFRASTRUCTURE (see that file's header).

    from oracle import c_oracle
    co = c_oracle.COracle(robot)            # builds oracle/_build/librbd_oracle.so with gcc if needed
    c, dc_du = co.rnea_grad(q, qd, qdd)     # [B, n] float64 in -> numpy out, OpenMP over rows

    cf = c_oracle.COracle(robot, real="float")   # the same recursion in plain IEEE float32 (librbd_oracle_f32.so);
                                                 # inputs and model arrays are cast to float32, outputs are float32
    co = c_oracle.COracle(model)                 # an oracle.rbd_oracle.OracleModel instead of a robot (perturbed models)
"""
import ctypes
import os
import subprocess

import numpy as np

from . import rbd_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librbd_oracle.so")
LIB_F32 = os.path.join(HERE, "_build", "librbd_oracle_f32.so")
_REALS = {"double": (LIB, [], np.float64, ctypes.c_double),
          # plain IEEE float32: no FMA contraction, no fast-math; nothing cleverer than the recursion as written
          "float": (LIB_F32, ["-DRBDO_REAL=float", "-ffp-contract=off"], np.float32, ctypes.c_float)}


def build(force: bool = False, real: str = "double") -> str:
    lib, flags = _REALS[real][:2]
    src = os.path.join(HERE, "rbd_oracle.c")
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        tmp = f"{lib}.{os.getpid()}.tmp"          # (tests in several processes may build at once: rename is atomic)
        cmd = ["gcc", "-O2", "-fPIC", "-fopenmp", "-std=c11", *flags, "-shared", "-o", tmp, src, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("gcc failed for oracle/rbd_oracle.c:\n" + r.stderr)
        os.replace(tmp, lib)
    return lib


class _Model(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("parent", ctypes.c_void_p), ("prismatic", ctypes.c_void_p),
                ("S", ctypes.c_void_p), ("I", ctypes.c_void_p), ("X0", ctypes.c_void_p),
                ("Xs", ctypes.c_void_p), ("Xc", ctypes.c_void_p), ("damping", ctypes.c_void_p)]


class COracle:
    def __init__(self, robot, real: str = "double"):
        _, _, self.dtype, creal = _REALS[real]
        self.real = real
        self.lib = ctypes.CDLL(build(real=real))
        m = robot if isinstance(robot, orc.OracleModel) else orc.model_from_robot(robot)
        self.n = m.n
        dt = self.dtype
        self._keep = dict(parent=np.ascontiguousarray(m.parent, dtype=np.int32),
                          prismatic=np.ascontiguousarray(m.prismatic, dtype=np.int32),
                          S=np.ascontiguousarray(m.S, dtype=dt), I=np.ascontiguousarray(m.I, dtype=dt),
                          X0=np.ascontiguousarray(m.X0, dtype=dt), Xs=np.ascontiguousarray(m.Xs, dtype=dt),
                          Xc=np.ascontiguousarray(m.Xc, dtype=dt), damping=np.ascontiguousarray(m.damping, dtype=dt))
        self.model = _Model(m.n, *[self._keep[k].ctypes.data for k in
                                   ("parent", "prismatic", "S", "I", "X0", "Xs", "Xc", "damping")])
        self.lib.rbdo_num_threads.restype = ctypes.c_int
        dp = ctypes.c_void_p
        self.lib.rbdo_rnea_grad.argtypes = [ctypes.POINTER(_Model), dp, dp, dp, creal, ctypes.c_int,
                                            ctypes.c_int64, dp, dp, ctypes.c_int]
        self.lib.rbdo_rnea.argtypes = [ctypes.POINTER(_Model), dp, dp, dp, creal, ctypes.c_int64,
                                       dp, dp, dp, dp, ctypes.c_int]
        self.lib.rbdo_minv.argtypes = [ctypes.POINTER(_Model), dp, ctypes.c_int, ctypes.c_int64, dp, ctypes.c_int]
        self.lib.rbdo_crba.argtypes = [ctypes.POINTER(_Model), dp, ctypes.c_int64, dp, ctypes.c_int]
        self.lib.rbdo_aba.argtypes = [ctypes.POINTER(_Model), dp, dp, dp, creal, ctypes.c_int64, dp, ctypes.c_int]
        self.lib.rbdo_forward_dynamics.argtypes = [ctypes.POINTER(_Model), dp, dp, dp, creal, ctypes.c_int64, dp, ctypes.c_int]
        self.lib.rbdo_forward_dynamics_grad.argtypes = [ctypes.POINTER(_Model), dp, dp, dp, creal, ctypes.c_int64, dp, dp,
                                                        ctypes.c_int]
        for fn in ("rbdo_rnea_grad", "rbdo_rnea", "rbdo_minv", "rbdo_crba", "rbdo_aba", "rbdo_forward_dynamics",
                   "rbdo_forward_dynamics_grad"):
            getattr(self.lib, fn).restype = None

    @property
    def max_threads(self) -> int:
        return int(self.lib.rbdo_num_threads())

    def _a(self, x):
        return np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=self.dtype)))

    def rnea_grad(self, q, qd, qdd=None, GRAVITY=-9.81, USE_VELOCITY_DAMPING=False, threads=0, out=None):
        q, qd = self._a(q), self._a(qd)
        qdd = None if qdd is None else self._a(qdd)
        B, n = q.shape
        if out is None:
            c = np.empty((B, n), dtype=self.dtype); dc = np.empty((B, n, 2 * n), dtype=self.dtype)
        else:                       # reuse caller's buffers (timing loops: no page faults per call)
            c, dc = out
            assert c.shape == (B, n) and dc.shape == (B, n, 2 * n) and c.flags.c_contiguous and dc.flags.c_contiguous
            assert c.dtype == self.dtype and dc.dtype == self.dtype
        self.lib.rbdo_rnea_grad(ctypes.byref(self.model), q.ctypes.data, qd.ctypes.data,
                                None if qdd is None else qdd.ctypes.data, float(GRAVITY),
                                int(USE_VELOCITY_DAMPING), B, c.ctypes.data, dc.ctypes.data, int(threads))
        return c, dc

    def rnea(self, q, qd, qdd=None, GRAVITY=-9.81, threads=0):
        q, qd = self._a(q), self._a(qd)
        qdd = None if qdd is None else self._a(qdd)
        B, n = q.shape
        c = np.empty((B, n), dtype=self.dtype)
        v, a, f = (np.empty((B, 6, n), dtype=self.dtype) for _ in range(3))
        self.lib.rbdo_rnea(ctypes.byref(self.model), q.ctypes.data, qd.ctypes.data,
                           None if qdd is None else qdd.ctypes.data, float(GRAVITY), B,
                           c.ctypes.data, v.ctypes.data, a.ctypes.data, f.ctypes.data, int(threads))
        return c, v, a, f

    def minv(self, q, output_dense=True, threads=0):
        q = self._a(q)
        B, n = q.shape
        M = np.empty((B, n, n), dtype=self.dtype)
        self.lib.rbdo_minv(ctypes.byref(self.model), q.ctypes.data, int(bool(output_dense)), B, M.ctypes.data,
                           int(threads))
        return M

    def crba(self, q, threads=0):
        q = self._a(q)
        B, n = q.shape
        H = np.empty((B, n, n), dtype=self.dtype)
        self.lib.rbdo_crba(ctypes.byref(self.model), q.ctypes.data, B, H.ctypes.data, int(threads))
        return H

    def aba(self, q, qd, tau, GRAVITY=-9.81, threads=0):
        q, qd, tau = self._a(q), self._a(qd), self._a(tau)
        B, n = q.shape
        qdd = np.empty((B, n), dtype=self.dtype)
        self.lib.rbdo_aba(ctypes.byref(self.model), q.ctypes.data, qd.ctypes.data, tau.ctypes.data, float(GRAVITY), B,
                          qdd.ctypes.data, int(threads))
        return qdd

    def forward_dynamics(self, q, qd, u, GRAVITY=-9.81, threads=0):
        """``minv(q) @ (u - rnea(q, qd).c)`` -> qdd ``[B, n]``."""
        q, qd, u = self._a(q), self._a(qd), self._a(u)
        B, n = q.shape
        qdd = np.empty((B, n), dtype=self.dtype)
        self.lib.rbdo_forward_dynamics(ctypes.byref(self.model), q.ctypes.data, qd.ctypes.data, u.ctypes.data, float(GRAVITY), B,
                                       qdd.ctypes.data, int(threads))
        return qdd

    def forward_dynamics_grad(self, q, qd, u, GRAVITY=-9.81, threads=0):
        """-> (qdd ``[B, n]``, ``[fd_dq | fd_dqd]`` ``[B, n, 2n]``): ``-minv(q) @ rnea_grad(q, qd, qdd)`` at the composition's qdd."""
        q, qd, u = self._a(q), self._a(qd), self._a(u)
        B, n = q.shape
        qdd = np.empty((B, n), dtype=self.dtype); d = np.empty((B, n, 2 * n), dtype=self.dtype)
        self.lib.rbdo_forward_dynamics_grad(ctypes.byref(self.model), q.ctypes.data, qd.ctypes.data, u.ctypes.data, float(GRAVITY),
                                            B, qdd.ctypes.data, d.ctypes.data, int(threads))
        return qdd, d
