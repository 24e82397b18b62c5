"""The entry-wise fp32 yardstick (tests/entrywise.py) has teeth: CPU only, gcc.

* blind share: for every fixed-base fixture robot, both regimes and the six tensors of rnea / rnea_grad / minv, at most 15 % of
  the nonzero entries may carry a 1 % error and still pass ``MARGIN * R_ref`` (a cap derived from nothing the kernels compute;
  printed beside the share that passes the normwise 1e-5 check of tests/test_gpu_parity.py on the same rows); for the tensors
  of the forward-dynamics family (``H``, ``qdd`` of aba / forward_dynamics / forward_dynamics_grad, ``fd_du``) at most 20 %;
* mutants of the plain-float32 oracle's ``dc_du``, ``Minv``, ``fd_du`` and ``H`` on the arm and the humanoid: one entry off by
  1 %, one entry zeroed, the dq / dqd halves of a row swapped (dc_du, fd_du), two configurations exchanged; printed beside the
  rate at which the suite's earlier fp32 bound flags the same mutants (normwise 1e-5; for ``fd_du`` check_conditioned's
  ``8 * 2^-24 * cond(H)`` per row);
* the float32 oracle is deterministic across thread counts, and ``COracle(model)`` is ``COracle(robot)`` bit for bit.
"""
import shutil

import numpy as np
import pytest

import entrywise as ew
from conftest import all_golden_names, make_robot, rel_err_rows

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")

TOL32 = 1e-5                # the normwise fp32 tolerance of tests/test_gpu_parity.py (importing that module would mark this one gpu)
BLIND_CAP = 0.15
BLIND_CAP_FD = 0.20         # the forward-dynamics family: fd_du inherits the float32 oracle's dc_du and Minv (R_ref 15 .. 36 on the
#                             arm and the humanoid, worst share 0.149), and R_ref moves by tens of per cent with the summation order
COND_SLACK = 8.0            # as test_gpu_parity.check_conditioned
FD_ENTRIES = ("crba", "aba", "forward_dynamics", "forward_dynamics_grad")
N_MUTANTS = 200
NOISE64 = 2.0 ** -53 * 4096   # what the double oracle itself leaves of an entry that is exactly zero, relative to its block


def _tensors(name, regime):
    for entry in ("rnea", "rnea_grad", "minv"):
        for t, y in ew.yardstick(name, regime, entry).items():
            if not (entry == "rnea_grad" and t == "c"):          # (c is rnea's; rnea_grad's c is the same recursion)
                yield t, y


@pytest.mark.parametrize("regime", sorted(ew.REGIMES))
@pytest.mark.parametrize("name", all_golden_names())
def test_blind_share_is_capped(name, regime):
    seen = []
    for t, y in _tensors(name, regime):
        assert np.isfinite(y.R_ref), (name, regime, t, "the plain-float32 oracle is not exactly 0 where the reference's block is")
        new = ew.blind_share(y.ref, y.Y, ew.MARGIN * y.R_ref, 0.01)
        old = ew.blind_share_normwise(y.ref, TOL32, 0.01)
        print(f"{name:20s} {regime:7s} {t:6s} R_ref {y.R_ref:6.2f}  entries that may be 1% wrong: entry-wise {new:.3f}, normwise 1e-5 {old:.3f}")
        seen.append(t)
        assert new <= BLIND_CAP, (name, regime, t, new)
    assert seen == ["c", "v", "a", "f", "dc_du", "Minv"]
    seen = []
    for entry in FD_ENTRIES:
        for t, y in ew.yardstick(name, regime, entry).items():
            assert np.isfinite(y.R_ref), (name, regime, entry, t)
            new = ew.blind_share(y.ref, y.Y, ew.MARGIN * y.R_ref, 0.01)
            old = ew.blind_share_normwise(y.ref, TOL32, 0.01)
            print(f"{name:20s} {regime:7s} {entry:21s} {t:6s} R_ref {y.R_ref:6.2f}  entries that may be 1% wrong: entry-wise {new:.3f}, normwise 1e-5 {old:.3f}")
            seen.append(t)
            assert new <= BLIND_CAP_FD, (name, regime, entry, t, new)
    assert seen == ["H", "qdd", "qdd", "qdd", "fd_du"]


def _flags_new(y, x):
    return ew.ratio(x, y.ref, y.Y) > ew.MARGIN * y.R_ref


def _flags_old(y, x, cond=None):
    if cond is None:
        return rel_err_rows(x, y.ref) > TOL32
    d = np.abs(x - y.ref).reshape(len(x), -1).max(axis=1) / np.abs(y.ref).reshape(len(x), -1).max(axis=1)
    return bool(np.any(d > COND_SLACK * ew.EPS32 * cond))        # test_gpu_parity.check_conditioned


ENTRY_OF = {"dc_du": "rnea_grad", "Minv": "minv", "fd_du": "forward_dynamics_grad", "H": "crba"}


@pytest.mark.parametrize("tensor", ["dc_du", "Minv", "fd_du", "H"])
@pytest.mark.parametrize("name", ["iiwa_like", "atlas_like"])
def test_mutants_of_the_float32_oracle_are_flagged(name, tensor):
    y = ew.yardstick(name, "std", ENTRY_OF[tensor])[tensor]
    cond = np.linalg.cond(ew.yardstick(name, "std", "crba")["H"].ref) if tensor == "fd_du" else None
    old_name = "normwise 1e-5" if cond is None else "check_conditioned"
    base = np.array(y.f32, dtype=np.float64)
    assert not _flags_new(y, base)
    rng = np.random.default_rng([ew.SEED, 99])
    # "nonzero" = above the double reference's own rounding noise.  On the axis-aligned arm 5 % of dc_du's entries are
    # structural zeros that the double recursion leaves at 1e-21 .. 1e-13 of their block (a few thousand roundings of
    # 2^-53 each; the next entries up are at 1e-7): 0 is the right value there, and flagging it would be the error.
    known = np.abs(y.ref) > NOISE64 * ew.blockmax(tensor, y.ref)
    nz = np.flatnonzero(known)
    print(f"{name} {tensor}: {np.count_nonzero(y.ref)} entries of the reference are not 0.0, {nz.size} are above its own rounding noise")
    kills = {}
    for what, mutate in (("scaled by 1.01", lambda v: v * 1.01), ("zeroed", lambda v: 0.0)):
        new = old = 0
        for j in rng.choice(nz, N_MUTANTS, replace=False):
            x = base.copy()
            x.flat[j] = mutate(x.flat[j])
            new += _flags_new(y, x); old += _flags_old(y, x, cond)
        kills[what] = (new, old)
        print(f"{name} {tensor}: one nonzero entry {what}: entry-wise flags {new}/{N_MUTANTS}, {old_name} flags {old}/{N_MUTANTS}")
    n = y.ref.shape[1]
    new = old = total = 0
    if tensor in ("dc_du", "fd_du"):
        for b in (0, 63, 64, 129):
            for i in range(n):                                  # (c) the dq and dqd halves of one joint row swapped
                x = base.copy()
                x[b, i] = np.concatenate((base[b, i, n:], base[b, i, :n]))
                total += 1; new += _flags_new(y, x); old += _flags_old(y, x, cond)
        print(f"{name} {tensor}: halves of one row swapped: entry-wise flags {new}/{total}, {old_name} flags {old}/{total}")
        assert new == total
    new = old = total = 0
    for b0, b1 in ((0, 1), (63, 64), (5, 129), (128, 129)):     # (d) two configurations exchanged
        x = base.copy()
        x[[b0, b1]] = x[[b1, b0]]
        total += 1; new += _flags_new(y, x); old += _flags_old(y, x, cond)
    print(f"{name} {tensor}: two configurations exchanged: entry-wise flags {new}/{total}, {old_name} flags {old}/{total}")
    assert new == total
    # 1 - cap - 0.05 sampling slack over 200 mutants (cap 0.15; 0.20 for the forward-dynamics family)
    assert kills["scaled by 1.01"][0] >= (0.75 if tensor in ("fd_du", "H") else 0.85) * N_MUTANTS, kills
    assert kills["zeroed"][0] >= 0.95 * N_MUTANTS, kills


def test_float32_oracle_is_deterministic_across_thread_counts():
    from oracle.c_oracle import COracle
    co = COracle(make_robot("atlas_like"), real="float")
    q, qd, qdd = ew.inputs(co.n, "std")
    c1, d1 = co.rnea_grad(q, qd, qdd, threads=1)
    c4, d4 = co.rnea_grad(q, qd, qdd, threads=4)
    assert d1.dtype == np.float32 and np.array_equal(d1, d4) and np.array_equal(c1, c4)
    assert all(np.array_equal(x, z) for x, z in zip(co.rnea(q, qd, qdd, threads=1), co.rnea(q, qd, qdd, threads=4)))
    assert np.array_equal(co.minv(q, threads=1), co.minv(q, threads=4))
    assert np.array_equal(co.crba(q, threads=1), co.crba(q, threads=4))
    assert np.array_equal(co.aba(q, qd, qdd, threads=1), co.aba(q, qd, qdd, threads=4))
    assert np.array_equal(co.forward_dynamics(q, qd, qdd, threads=1), co.forward_dynamics(q, qd, qdd, threads=4))
    assert all(x.dtype == np.float32 and np.array_equal(x, z) for x, z in zip(co.forward_dynamics_grad(q, qd, qdd, threads=1),
                                                                              co.forward_dynamics_grad(q, qd, qdd, threads=4)))


@pytest.mark.parametrize("name", ["iiwa_like", "random_prismatic_n6"])
def test_c_oracle_from_a_model_equals_the_one_from_the_robot(name):
    from oracle import rbd_oracle as orc
    from oracle.c_oracle import COracle
    robot = make_robot(name)
    a, b = COracle(robot), COracle(orc.model_from_robot(robot))
    q, qd, qdd = ew.inputs(a.n, "std")
    for x, z in zip(a.rnea_grad(q, qd, qdd, USE_VELOCITY_DAMPING=True) + a.rnea(q, qd) + (a.minv(q), a.minv(q, output_dense=False)),
                    b.rnea_grad(q, qd, qdd, USE_VELOCITY_DAMPING=True) + b.rnea(q, qd) + (b.minv(q), b.minv(q, output_dense=False))):
        assert x.dtype == np.float64 and np.array_equal(x, z)
