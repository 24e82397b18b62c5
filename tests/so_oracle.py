"""Batched numpy restatement of the reference's second-order inverse-dynamics derivatives (test helper, not product code).

Restates ``RBDReference.second_order_idsva_parallel`` (``RBDReference.py:1387-1604``) over a batch of configurations,
with one index corrected: the composite-force sweep adds the child's force, ``f[:, pi] += f[:, i]``, where the
reference adds ``f[:, pi + 1]`` (``:1448``).  With that change all four outputs are the true derivatives (see
tests/test_so_oracle.py); on robots where every non-root body ``i`` has parent ``i - 1`` it is the reference itself.

Outputs, each ``[B, n, n, n]`` (or ``(n, n, n)`` for one configuration), ``c = rnea(q, qd, qdd)[0]``, ``H = crba(q)``:
    d2tau_dq   [i, j, k] = d2 c_i / dq_j dq_k
    d2tau_dqd  [i, j, k] = d2 c_i / dqd_j dqd_k
    d2tau_dvdq [i, j, k] = d (dc_dqd[i, j]) / dq_k
    dM_dq      [i, j, k] = d H_ij / dq_k

The scatter loops over (j, ancestor-or-self k) are kept as the reference writes them, vectorised over the batch and
over the subtree index lists.  Bilinear forms replace the reference's flattened dot products: for
``t = outer(u, w).flatten('F')``, ``t . M.flatten('F') = u^T M w`` and ``t . M.flatten() = w^T M u``.
"""
import numpy as np

from oracle.rbd_oracle import Xmats, model_from_robot


def crm(v):
    """[..., 6] -> [..., 6, 6], the motion cross operator (``cross_operator``, :9-21)."""
    o = np.zeros(v.shape[:-1] + (6, 6))
    w, u = v[..., :3], v[..., 3:]
    for blk, x in (((0, 0), w), ((3, 3), w), ((3, 0), u)):
        r, c = blk
        o[..., r + 0, c + 1] = -x[..., 2]; o[..., r + 0, c + 2] = x[..., 1]
        o[..., r + 1, c + 0] = x[..., 2]; o[..., r + 1, c + 2] = -x[..., 0]
        o[..., r + 2, c + 0] = -x[..., 1]; o[..., r + 2, c + 1] = x[..., 0]
    return o


def crf(v):
    """``dual_cross_operator`` (:23-25)."""
    return -np.swapaxes(crm(v), -1, -2)


def icrf(f):
    """``icrf`` (:33-43): icrf(f) v = crf(v) f."""
    o = np.zeros(f.shape[:-1] + (6, 6))
    n_, g = f[..., :3], f[..., 3:]
    for (r, c), x in (((0, 0), n_), ((0, 3), g), ((3, 0), g)):
        o[..., r + 0, c + 1] = x[..., 2]; o[..., r + 0, c + 2] = -x[..., 1]
        o[..., r + 1, c + 0] = -x[..., 2]; o[..., r + 1, c + 2] = x[..., 0]
        o[..., r + 2, c + 0] = x[..., 1]; o[..., r + 2, c + 1] = -x[..., 0]
    return o


def _mv(M, x):
    return np.einsum("...rc,...c->...r", M, x)


def _form(u, M, w):
    """u^T M w: u, w [B, 6], M [B, k, 6, 6] -> [B, k]."""
    return np.einsum("br,bkrc,bc->bk", u, M, w)


def _dot(p, T):
    """p . T: p [B, 6], T [B, k, 6] -> [B, k]."""
    return np.einsum("br,bkr->bk", p, T)


def world_state(m, q, qd, qdd, GRAVITY=-9.81, fix_f=True):
    """Forward and backward sweeps of :1413-1448 -> dict of S, psid, psidd, IC, BC, f ([B, n, ...])."""
    B, n = q.shape
    X = Xmats(m, q)
    Xup = np.zeros((B, n, 6, 6))
    S = np.zeros((B, n, 6)); psid = np.zeros((B, n, 6)); psidd = np.zeros((B, n, 6))
    v = np.zeros((B, n, 6)); a = np.zeros((B, n, 6)); f = np.zeros((B, n, 6))
    IC = np.zeros((B, n, 6, 6)); BC = np.zeros((B, n, 6, 6))
    g = np.zeros(6); g[5] = -GRAVITY
    for i in range(n):
        p = m.parent[i]
        if p == -1:
            Xup[:, i] = X[:, i]
            vp, ap = np.zeros((B, 6)), np.broadcast_to(g, (B, 6))
        else:
            Xup[:, i] = X[:, i] @ Xup[:, p]
            vp, ap = v[:, p], a[:, p]
        S[:, i] = np.linalg.solve(Xup[:, i], np.broadcast_to(m.S[i], (B, 6))[..., None])[..., 0]
        Si = S[:, i]
        vJ = Si * qd[:, i:i + 1]
        aJ = _mv(crm(vp), vJ) + Si * qdd[:, i:i + 1]
        psid[:, i] = _mv(crm(vp), Si)
        psidd[:, i] = _mv(crm(ap), Si) + _mv(crm(vp), psid[:, i])
        v[:, i] = vp + vJ
        a[:, i] = ap + aJ
        IC[:, i] = np.swapaxes(Xup[:, i], -1, -2) @ m.I[i] @ Xup[:, i]
        vi = v[:, i]
        BC[:, i] = crf(vi) @ IC[:, i] + icrf(_mv(IC[:, i], vi)) - IC[:, i] @ crm(vi)
        f[:, i] = _mv(IC[:, i], a[:, i]) + _mv(crf(vi) @ IC[:, i], vi)
    for i in range(n - 1, -1, -1):
        p = m.parent[i]
        if p >= 0:
            IC[:, p] += IC[:, i]
            BC[:, p] += BC[:, i]
            f[:, p] += f[:, i] if fix_f else f[:, p + 1]      # the corrected index (the reference: f[:, pi + 1], :1448)
    return dict(S=S, psid=psid, psidd=psidd, Sd=psid.copy(), IC=IC, BC=BC, f=f)


def body_terms(st):
    """Per body j (:1456-1484): A1 (D1, C order), A2 (D2), Bic_phii (D3), A3 (D4) and T1..T4."""
    S, psid, psidd, Sd, IC, BC, f = (st[k] for k in ("S", "psid", "psidd", "Sd", "IC", "BC", "f"))
    A1 = crf(S) @ IC - IC @ crm(S)
    ICS = _mv(IC, S)
    Bphi = A1 + icrf(ICS)
    A2 = crf(psid) @ IC + icrf(_mv(IC, psid)) - IC @ crm(psid) + crf(S) @ BC - BC @ crm(S)
    A3 = icrf(_mv(np.swapaxes(IC, -1, -2), S))
    T1 = ICS
    T2 = -_mv(np.swapaxes(BC, -1, -2), S)
    T3 = _mv(BC, psid) + _mv(IC, psidd) + _mv(icrf(f), S)
    T4 = _mv(BC, S) + _mv(IC, psid + Sd)
    return dict(A1=A1, A2=A2, Bphi=Bphi, A3=A3, T1=T1, T2=T2, T3=T3, T4=T4)


def second_order_idsva(m, q, qd, qdd, GRAVITY=-9.81, fix_f=True):
    """-> (d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq).  ``fix_f=False`` restates the reference's :1448 as written."""
    q = np.asarray(q, dtype=np.float64); qd = np.asarray(qd, dtype=np.float64); qdd = np.asarray(qdd, dtype=np.float64)
    un = q.ndim == 1
    if un:
        q, qd, qdd = q[None], qd[None], qdd[None]
    B, n = q.shape
    st = world_state(m, q, qd, qdd, GRAVITY, fix_f)
    bt = body_terms(st)
    S, psid, psidd, Sd = st["S"], st["psid"], st["psidd"], st["Sd"]
    A1, A2, Bphi, A3 = bt["A1"], bt["A2"], bt["Bphi"], bt["A3"]
    A1t = np.swapaxes(A1, -1, -2)          # D1 is A1 in C order: t . D1 = u^T A1^T w
    T1, T2, T3, T4 = bt["T1"], bt["T2"], bt["T3"], bt["T4"]
    d2q = np.zeros((B, n, n, n)); d2qd = np.zeros((B, n, n, n)); d2vq = np.zeros((B, n, n, n)); dM = np.zeros((B, n, n, n))
    for j in range(n - 1, -1, -1):
        st_j = list(m.subtree[j])
        succ = [i for i in st_j if i != j]
        anc = []
        p = m.parent[j]
        while p != -1:
            anc.append(p)
            p = m.parent[p]
        Sd_, psd_, psdd_, Sdd_ = S[:, j], psid[:, j], psidd[:, j], Sd[:, j]
        for k in anc + [j]:                                        # parent .. root, then j (:1504-1506)
            Sc, psc, Sdc, psddc = S[:, k], psid[:, k], Sd[:, k], psidd[:, k]
            p1 = _mv(crm(psc), Sd_)
            p2 = _mv(crm(psddc), Sd_)
            v_a = -_form(psd_, Bphi[:, st_j], psc) - _dot(p1, T2[:, st_j]) + _dot(p2, T1[:, st_j])
            d2q[:, st_j, j, k] = v_a
            d2vq[:, st_j, j, k] = -_form(Sd_, Bphi[:, st_j], psc)                  # t1 = outer(S_d, psid_c)
            if k < j:
                p3 = _mv(crm(Sc), Sd_)
                p4 = _mv(crm(Sdc + psc), Sd_) - 2 * _mv(crm(psd_), Sc)
                p5 = _mv(crm(Sd_), Sc)
                d2q[:, st_j, k, j] = v_a
                x = -_form(Sd_, Bphi[:, st_j], Sc)                                 # -t2 . D3
                d2qd[:, st_j, k, j] = x
                d2qd[:, st_j, j, k] = x
                d2vq[:, st_j, k, j] = -_form(Sc, Bphi[:, st_j], psd_) - _dot(p3, T2[:, st_j]) + _dot(p4, T1[:, st_j])
                d2q[:, k, st_j, j] = _form(Sc, A2[:, st_j], psd_) + _form(Sc, A1t[:, st_j], psdd_) - _dot(p5, T3[:, st_j])
                d2vq[:, k, st_j, j] = _form(Sc, Bphi[:, st_j], psd_) - _dot(p5, T4[:, st_j])
                ICj = st["IC"][:, j]
                d2qd[:, k, j, j] = (np.einsum("br,brc,bcd,bd->b", Sd_, ICj, crm(Sc), Sd_)
                                    + np.einsum("br,brc,bcd,bd->b", Sc, crf(Sd_), ICj, Sd_))
                x = _form(Sc, A3[:, st_j], Sd_)                                    # t8 . D4
                dM[:, k, st_j, j] = x
                dM[:, st_j, k, j] = x
                if succ:
                    x = _form(Sc, Bphi[:, succ], Sd_)
                    d2qd[:, k, succ, j] = x
                    d2qd[:, k, j, succ] = x
                    d2vq[:, k, j, succ] = _form(Sc, A2[:, succ], Sd_) + _form(Sc, A1t[:, succ], Sdd_ + psd_)
                    d2q[:, k, j, succ] = d2q[:, k, succ, j]
            if succ:
                x = _form(Sd_, A2[:, succ], psc) + _form(Sd_, A1t[:, succ], psddc)
                d2q[:, j, k, succ] = x
                d2q[:, j, succ, k] = x
                x = _form(Sd_, Bphi[:, succ], Sc)
                d2qd[:, j, k, succ] = x
                d2qd[:, j, succ, k] = x
                d2vq[:, j, succ, k] = _form(Sd_, Bphi[:, succ], psc)
                d2vq[:, j, k, succ] = _form(Sd_, A2[:, succ], Sc) + _form(Sd_, A1t[:, succ], Sdc + psc)
                x = _form(Sc, A1t[:, succ], Sd_)                                   # t8 . D1
                dM[:, k, j, succ] = x
                dM[:, j, k, succ] = x
            if k == j:
                d2qd[:, st_j, j, k] = -_form(Sd_, A1t[:, st_j], Sc)
    out = (d2q, d2qd, d2vq, dM)
    return tuple(x[0] for x in out) if un else out


class SOOracle:
    def __init__(self, robot):
        self.robot = robot
        self.m = model_from_robot(robot)

    def __call__(self, q, qd, qdd, GRAVITY=-9.81, fix_f=True):
        return second_order_idsva(self.m, q, qd, qdd, GRAVITY, fix_f)


# ---- the fixture robots: the nine fixed-base robots whose libraries build() makes ---------------------------------
SO_ROBOTS = ["iiwa_like", "quadruped_like", "atlas_like", "random_tree_n9", "random_chain_n7", "random_prismatic_n6",
             "random_forest_n8", "random_limbs_n14", "random_twochains_n18"]


def unbranched(robot):
    """Every non-root body i has parent i - 1: the reference's f[:, pi + 1] is then f[:, i] (:1448)."""
    n = robot.get_num_bodies()
    return all(robot.get_parent_id(i) in (-1, i - 1) for i in range(n))
