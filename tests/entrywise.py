"""Entry-wise fp32 accuracy yardstick for rnea / rnea_grad / minv and the forward-dynamics family (crba, aba, forward_dynamics,
forward_dynamics_grad) (checker only; everything here runs on the CPU).

The normwise checks of the fp32 path (``max|x - ref| / max|ref| <= 1e-5`` per configuration and tensor) let the largest
entry of a tensor set the scale for all the others, and the entries of ``dc_du``, ``Minv`` and ``f`` span five or more orders
of magnitude.  This module measures every entry against what the entry itself can be known to:

    ref    the double C oracle (oracle/rbd_oracle.c; tests/test_c_oracle.py pins it to the goldens) at float32-valued inputs
    S_e    max over DRAWS draws of |out_e - ref_e|, where a draw multiplies every entry of the model's I, X0, Xs, Xc and of
           q, qd, qdd independently by 1 + 2^-24 U(-1, 1) and runs the double oracle: what ONE float32 rounding of the data,
           which every fp32 kernel makes, does to the entry
    Y_e    S_e + 2^-24 blockmax_e, blockmax = max|ref| over the entry's block: the entry itself (c), the angular or the linear
           triple of one body (v, a, f), the dq or the dqd half of one joint row (dc_du, fd_du), one row (Minv, H).  The floor
           stands for cancellations that the perturbations leave intact and float32 arithmetic does not (axis-aligned robots).
           For the tensors that are a product with Minv -- qdd = Minv (u - c), fd_du = -Minv dc_du; the third input array is u --
           blockmax_e is replaced by the larger of it and (|Minv| |u - c|)_e or (|Minv| |dc_du|)_e of the double reference
           (product_floor)
    ratio  max_e |got_e - ref_e| / Y_e over entries with Y_e > 0; where Y_e = 0 the whole block is structurally zero and
           got_e must be exactly 0 (otherwise the ratio is inf)
    R_ref  ratio(the plain-float32 build of the same C oracle), computed for each (robot, regime, variant, tensor); for qdd the
           larger of the reference's two float32 routes, the composition Minv (u - c) and the ABA sweeps

A kernel passes when ratio(kernel) <= MARGIN * R_ref.  MARGIN = 4 is two bits: another equally stable algorithm (world-frame
IDSVA, factorised Minv), FMA contraction, another summation order, a hardware reciprocal with one Newton step.  Nothing in the
yardstick comes from the code under test.
"""
import functools
from types import SimpleNamespace

import numpy as np

from conftest import make_robot
from oracle import rbd_oracle as orc

B = 130                     # two 64-lane tiles and a ragged one of two
SEED = 20240607
DRAWS = 16
EPS32 = 2.0 ** -24
MARGIN = 4.0
REGIMES = {"std": dict(qd_scale=1.0, GRAVITY=-9.81),
           "fast0g": dict(qd_scale=10.0, GRAVITY=0.0)}     # no gravity terms: the velocity products set the scale
TENSORS = {"rnea": ("c", "v", "a", "f"), "rnea_grad": ("c", "dc_du"), "minv": ("Minv",),
           "crba": ("H",), "aba": ("qdd",), "forward_dynamics": ("qdd",), "forward_dynamics_grad": ("qdd", "fd_du")}
SOLVED = ("qdd", "fd_du")   # tensors that are a product with Minv: their floor also holds the product's componentwise bound


def inputs(n, regime):
    """-> (q, qd, qdd), float32 ``[B, n]``; the same rows for every robot of n bodies."""
    rng = np.random.default_rng([SEED, n])
    s = REGIMES[regime]["qd_scale"]
    q = rng.uniform(-np.pi, np.pi, (B, n)); qd = s * rng.uniform(-1, 1, (B, n)); qdd = rng.uniform(-1, 1, (B, n))
    return tuple(x.astype(np.float32) for x in (q, qd, qdd))


def blockmax(tensor, ref):
    """max|ref| over every entry's block, broadcast back to ref's shape."""
    a = np.abs(ref)
    if tensor in ("c", "qdd"):
        return a
    if tensor in ("v", "a", "f"):                       # [B, 6, n]: angular / linear triple of one body
        b = a.reshape(a.shape[0], 2, 3, a.shape[2])
        return np.broadcast_to(b.max(axis=2, keepdims=True), b.shape).reshape(a.shape)
    if tensor in ("dc_du", "fd_du"):                    # [B, n, 2n]: dq / dqd half of one joint row
        n = a.shape[1]
        b = a.reshape(a.shape[0], n, 2, n)
        return np.broadcast_to(b.max(axis=3, keepdims=True), b.shape).reshape(a.shape)
    if tensor in ("Minv", "H"):                         # [B, n, n]: one row
        return np.broadcast_to(a.max(axis=2, keepdims=True), a.shape)
    raise KeyError(tensor)


def ratio(got, ref, Y):
    """max_e |got_e - ref_e| / Y_e over Y_e > 0; inf if got is not finite or not exactly 0 where Y_e = 0."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.all(np.isfinite(got)):
        return float("inf")
    live = Y > 0
    if np.any(got[~live] != 0.0):
        return float("inf")
    return float(np.max(np.abs(got - ref)[live] / Y[live], initial=0.0))


def worst_entries(got, ref, Y, k=5):
    """The k entries with the largest |got - ref| / Y: ``[(index, got, ref, Y, ratio)]`` (for failure messages)."""
    got = np.asarray(got, dtype=np.float64)
    r = np.where(Y > 0, np.abs(got - ref) / np.where(Y > 0, Y, 1.0), np.where(got != 0.0, np.inf, 0.0))
    idx = np.argsort(r, axis=None)[::-1][:k]
    return [(tuple(int(i) for i in np.unravel_index(j, r.shape)), float(got.flat[j]), float(ref.flat[j]), float(Y.flat[j]),
             float(r.flat[j])) for j in idx]


def blind_share(ref, Y, T, rel):
    """Share of the nonzero ref entries that may carry a relative error ``rel`` and still pass ``|err| <= T Y``."""
    nz = ref != 0.0
    return float(np.mean((rel * np.abs(ref) < T * Y)[nz])) if np.any(nz) else 0.0


def blind_share_normwise(ref, tol, rel):
    """The same share under the normwise check ``max|x - ref| / max|ref| <= tol`` per configuration (conftest.rel_err_rows)."""
    nz = ref != 0.0
    rowmax = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return float(np.mean((rel * np.abs(ref) <= tol * rowmax)[nz])) if np.any(nz) else 0.0


def _run(co, entry, q, qd, qdd, GRAVITY, damped, dense):
    """One oracle call -> {tensor: array} for the entry point's tensors."""
    if entry == "rnea":
        return dict(zip("cvaf", co.rnea(q, qd, qdd, GRAVITY=GRAVITY)))
    if entry == "rnea_grad":
        return dict(zip(("c", "dc_du"), co.rnea_grad(q, qd, qdd, GRAVITY=GRAVITY, USE_VELOCITY_DAMPING=damped)))
    if entry == "minv":
        M = co.minv(q, output_dense=dense)
        return {"Minv": M if dense else np.triu(M)}   # (the reference leaves by-products below the diagonal)
    if entry == "crba":
        return {"H": co.crba(q)}
    if entry == "aba":                                # (the third array is u from here on, as in the goldens)
        return {"qdd": co.aba(q, qd, qdd, GRAVITY=GRAVITY)}
    if entry == "forward_dynamics":
        return {"qdd": co.forward_dynamics(q, qd, qdd, GRAVITY=GRAVITY)}
    if entry == "forward_dynamics_grad":
        return dict(zip(("qdd", "fd_du"), co.forward_dynamics_grad(q, qd, qdd, GRAVITY=GRAVITY)))
    raise KeyError(entry)


def product_floor(co, q, qd, u, GRAVITY):
    """-> {tensor: |Minv| |factor|} from the double oracle ``co``: what a float32 product of the exactly known factors
    ``Minv`` and ``u - c`` (qdd) or ``dc_du`` (fd_du) errs by per entry, in units of 2^-24 (Higham's componentwise bound for
    an inner product, to first order and without its length factor).  The data perturbations of S do not reproduce it: they
    move the factors, and a product of moved factors is still formed exactly in double."""
    Mi = np.abs(co.minv(q))
    c = co.rnea(q, qd, None, GRAVITY=GRAVITY)[0]
    qdd = co.forward_dynamics(q, qd, u, GRAVITY=GRAVITY)
    dc = co.rnea_grad(q, qd, qdd, GRAVITY=GRAVITY)[1]
    return {"qdd": np.einsum("bij,bj->bi", Mi, np.abs(u - c)), "fd_du": np.einsum("bij,bjk->bik", Mi, np.abs(dc))}


def _perturbed(m, rng):
    def p(x):
        return x * (1.0 + EPS32 * rng.uniform(-1, 1, x.shape))
    return orc.OracleModel(m.n, m.parent, m.subtree, m.S, p(m.I), m.damping, m.prismatic, p(m.X0), p(m.Xs), p(m.Xc))


@functools.lru_cache(maxsize=None)
def _model(name):
    return orc.model_from_robot(make_robot(name))


@functools.lru_cache(maxsize=None)
def yardstick(name, regime, entry, has_qdd=True, damped=False, dense=True):
    """-> {tensor: namespace(ref, S, Y, f32, R_ref)} for one robot, regime and variant of one entry point.  Computed once per
    process and shared (callers must not write into the arrays)."""
    from oracle.c_oracle import COracle
    m = _model(name)
    g = REGIMES[regime]["GRAVITY"]
    q, qd, qdd = (x.astype(np.float64) for x in inputs(m.n, regime))
    co = COracle(m)
    ref = _run(co, entry, q, qd, qdd if has_qdd else None, g, damped, dense)
    S = {t: np.zeros_like(r) for t, r in ref.items()}
    for d in range(DRAWS):
        rng = np.random.default_rng([SEED, m.n, d])           # the same perturbed model and inputs for every entry point
        pm = _perturbed(m, rng)
        pq, pqd, pqdd = (x * (1.0 + EPS32 * rng.uniform(-1, 1, x.shape)) for x in (q, qd, qdd))
        out = _run(COracle(pm), entry, pq, pqd, pqdd if has_qdd else None, g, damped, dense)
        for t in S:
            np.maximum(S[t], np.abs(out[t] - ref[t]), out=S[t])
    cf = COracle(m, real="float")
    f32 = _run(cf, entry, q, qd, qdd if has_qdd else None, g, damped, dense)
    floor = product_floor(co, q, qd, qdd, g) if any(t in SOLVED for t in ref) else {}
    res = {}
    for t in ref:
        Y = S[t] + EPS32 * (np.maximum(blockmax(t, ref[t]), floor[t]) if t in SOLVED else blockmax(t, ref[t]))
        for a in (ref[t], S[t], Y, f32[t]):
            a.setflags(write=False)
        R_ref = ratio(f32[t], ref[t], Y)
        if t == "qdd":        # the reference defines qdd two ways, and the GPU serves forward_dynamics with the ABA sweeps:
            R_ref = max(ratio(cf.forward_dynamics(q, qd, qdd, GRAVITY=g), ref[t], Y), ratio(cf.aba(q, qd, qdd, GRAVITY=g), ref[t], Y))
        res[t] = SimpleNamespace(ref=ref[t], S=S[t], Y=Y, f32=f32[t], R_ref=R_ref)
    return res
