"""Entry-wise accuracy of the fp32 forward-dynamics family: crba, aba, forward_dynamics, forward_dynamics_grad (run with
``-m gpu`` on a real MI355X).

The yardstick is tests/entrywise.py, as in tests/test_gpu_entrywise.py: a kernel passes when its worst entry is within
``MARGIN = 4`` of what the plain-float32 build of the C oracle loses on the same rows.  For the tensors that are a product with
``Minv`` (``qdd``, ``fd_du = [fd_dq | fd_dqd]``) the yardstick's floor also holds the product's componentwise bound
``2^-24 (|Minv| |factor|)_e``, and ``R_ref`` of ``qdd`` is the larger of the reference's two float32 routes (the composition
``Minv (u - c)`` and the ABA sweeps).  130 rows (two 64-row tiles and a ragged one: the whole-tile ``Minv`` workspace of
``fd_pre_kernel``), both regimes, the nine fixed-base fixture robots, the third input array as ``u``.

``forward_dynamics_grad`` has three launch paths (``fd_launch``, csrc/rbd_capi.h) and the robot decides at compile time which
one it takes; BRANCH below is that decision, read from the four constants it depends on.  Both outputs of the call are
measured: the ``qdd`` it writes -- the fused ``qdd = Minv (u - c)`` of ``fd_pre_kernel`` or of the ``minv`` kernels, which
nothing else in the suite holds to more than cond(H) -- and ``fd_du``.  Every case prints ``label  ratio  R_ref  ratio / R_ref``
with the branch and the two kernel names in the label; the measured table is in DESIGN.md §2.1.  Prebuilt libraries only.
"""
import functools

import numpy as np
import pytest

import entrywise as ew
from conftest import all_golden_names, make_robot
from test_gpu_entrywise import XFAIL as XFAIL_GRAD, XFAIL_GENERIC as XFAIL_GRAD_GENERIC, _Records, _dev
from test_gpu_parity import rbd_for

pytestmark = pytest.mark.gpu

# The branch of fd_launch<float> each robot takes (want_grad):
#   chain    fd_chain_ok && grad_chain_kernel: one chain of revolute joints, at most 8 bodies (GRAD_IDSVA_OK, n_groups() == 1,
#            grad_max_rows() == N).  fd_pre_kernel (bias force, Minv, qdd in one lane), then the world-frame chain gradient
#            kernel with the -Minv product on its finished entries (FDG epilogue).  No option changes either launch.
#   lane     otherwise, minv_use_lane (every root subtree, or the whole robot where they interleave, has at most 8 bodies) and
#            GRAD_ACC_IN_REGS (at most 72 related pairs): minv_lane_kernel computes the bias force and the fused qdd itself,
#            then rnea_grad_kernel (two lanes) with the -Minv epilogue.  No option changes either launch.
#   neg_mm   otherwise (more than 72 related pairs; none of these robots has minv_use_lane): rbd_rnea for c, rbd_minv with the
#            fused qdd in its last phase (RBD_OPT_MINV_PHASE_A: minv_fused_kernel, or minv_ia8_kernel / minv_ia_kernel and
#            minv_cols_kernel), rbd_rnea_grad into the workspace (RBD_OPT_GRAD_KERNEL), neg_mm_kernel.
# robot: (branch, bodies of the largest group -- random_forest_n8's root subtrees of 3 and 5 bodies interleave in the numbering
# and form one group --, related pairs)
BRANCH = {
    "atlas_like": ("neg_mm", 18, 270),
    "iiwa_like": ("chain", 7, 49),
    "quadruped_like": ("lane", 3, 36),
    "random_chain_n7": ("chain", 7, 49),
    "random_forest_n8": ("lane", 8, 26),
    "random_limbs_n14": ("neg_mm", 14, 100),
    "random_prismatic_n6": ("lane", 6, 32),
    "random_tree_n9": ("lane", 5, 33),
    "random_twochains_n18": ("neg_mm", 9, 162),
}

# (RBD_OPT_MINV_PHASE_A, RBD_OPT_GRAD_KERNEL, RBD_OPT_SELECT_BATCH) per option, in the order they run
OPTIONS = {"AUTO": (0, 0, 0), "LANE": (1, 0, 0), "IA8": (2, 0, 0), "FUSED": (3, 0, 0),
           "TREE": (0, 1, 0), "COLS": (0, 2, 0), "BATCH": (0, 3, 0), "AUTO@2^20": (0, 0, 1 << 20)}


def _options(name):
    """The options that can change a launch of this robot's branch: all of them where the path calls rbd_minv's phases and
    rbd_rnea_grad, none but AUTO where it does not (test_branch_table_matches_the_library: the one-lane minv kernel under
    every option)."""
    return tuple(OPTIONS) if BRANCH[name][0] == "neg_mm" else ("AUTO",)


# Margin over R_ref per first word of the label; not listed: ew.MARGIN = 4.  Empty: every kernel only this family runs measured
# within 1.93 R_ref, so none has a larger margin.
FAMILY_MARGIN = {}

# Open defects of fd_du: (robot, option) -> (gradient kernel family, measured worst ratio / R_ref over both regimes).  The known
# world-frame defect of the gradient kernels passing through the -Minv product: a distal joint's row of dc_du is
# 1e-7 absolute off where the joint's own inertia is small, and Minv's diagonal entry of that joint is large, so the entry of
# fd_du is wrong in its third or fourth digit (atlas_like fd_du[83, 17, 45] = -0.019556 comes out -0.019500).  Strict, so a kernel
# that gets better has to take its line out; the qdd of the same call is a case of its own and passes.
# test_open_defects_are_the_known_world_frame_defect shows where the error enters.
XFAIL = {
    ("atlas_like", "AUTO"): ("rnea_grad_tree_kernel", 22.2),
    ("atlas_like", "LANE"): ("rnea_grad_tree_kernel", 22.2),
    ("atlas_like", "IA8"): ("rnea_grad_tree_kernel", 22.2),
    ("iiwa_like", "AUTO"): ("rnea_grad_idsva_pipe_kernel", 34.0),
    ("random_limbs_n14", "AUTO"): ("rnea_grad_tree_kernel", 5.75),
    ("random_limbs_n14", "LANE"): ("rnea_grad_tree_kernel", 5.75),
    ("random_limbs_n14", "IA8"): ("rnea_grad_tree_kernel", 5.75),
}
XFAIL_GENERIC = {"iiwa_like": ("g_rnea_grad_world_kernel", 36.6), "random_limbs_n14": ("g_rnea_grad_world_kernel", 7.44)}


class _FdRecords(_Records):
    @staticmethod
    def margin(kernel):
        return FAMILY_MARGIN.get(kernel.split(" ")[0], ew.MARGIN)


def _set(rbd, option):
    from rbdreference_amd import _lib as L
    pa, gk, sb = OPTIONS[option]
    rbd._lib.set_option(L.RBD_OPT_MINV_PHASE_A, pa); rbd._lib.set_option(L.RBD_OPT_GRAD_KERNEL, gk); rbd._lib.set_option(L.RBD_OPT_SELECT_BATCH, sb)


def _names(rbd, name, option):
    """Set the option (the caller restores it) -> (minv kernel, gradient kernel) that forward_dynamics_grad runs for 130 rows."""
    from rbdreference_amd import _lib as L
    _set(rbd, option)
    branch = BRANCH[name][0]
    if branch == "chain":                    # neither launch asks the options
        return "fd_pre_kernel<float>", "rnea_grad_idsva_pipe_kernel<float,true,true>"
    minv = rbd._lib.kernel_name(L.RBD_OP_MINV, 4, ew.B)
    if branch == "lane":
        assert minv.startswith("minv_lane_kernel<"), (name, minv)
        return minv, "rnea_grad_kernel<float,true,true>"
    if minv.startswith("minv_cols_kernel"):  # one name, two phase A kernels in front of it (minv_select)
        pa, _, sb = OPTIONS[option]
        minv += " A=lane" if pa == L.RBD_MINV_PHASE_A_LANE or (pa != L.RBD_MINV_PHASE_A_IA8 and sb >= 64 * 1024 * 4) else " A=ia8"
    return minv, rbd._lib.kernel_name(L.RBD_OP_RNEA_GRAD, 4, ew.B)


def _restore(rbd):
    _set(rbd, "AUTO")


@functools.lru_cache(maxsize=None)
def run_grad_option(name, option):
    """forward_dynamics_grad under one option on one robot (fp32, 130 rows, both regimes) -> (label, _Records); records is
    None when an earlier option already ran this pair of kernels."""
    rbd = rbd_for(name)
    order = list(OPTIONS)
    try:
        earlier = {_names(rbd, name, o) for o in order[:order.index(option)]}
        pair = _names(rbd, name, option)
        label = f"{BRANCH[name][0]}: {pair[0]} + {pair[1]}"
        if pair in earlier:
            return label, None
        rec = _FdRecords()
        for regime in sorted(ew.REGIMES):
            g = ew.REGIMES[regime]["GRAVITY"]
            q, qd, u = _dev(*ew.inputs(rbd.n, regime))
            Y = ew.yardstick(name, regime, "forward_dynamics_grad")
            qdd, d = rbd._fd(q, qd, u, g, True)[:2]
            rec.add(name, regime, label, "fd_grad", "qdd", qdd, Y["qdd"]); rec.add(name, regime, label, "fd_grad", "fd_du", d, Y["fd_du"])
        return label, rec
    finally:
        _restore(rbd)


def _xfail(known):
    return [pytest.mark.xfail(strict=True, reason=f"fd_du through {known[0]}: ratio / R_ref = {known[1]} (open defect, DESIGN.md 2.1)")] if known else []


def _grad_cases():
    for name in all_golden_names():
        for option in _options(name):
            for tensor in ("qdd", "fd_du"):
                yield pytest.param(name, option, tensor, marks=_xfail(XFAIL.get((name, option)) if tensor == "fd_du" else None),
                                   id=f"{name}-{option}-{tensor}")


def _failures(rec, tensor):
    return [f for f in rec.failures() if f[2] == tensor]


@pytest.mark.parametrize("name,option,tensor", list(_grad_cases()))
def test_forward_dynamics_grad_entrywise(name, option, tensor):
    label, rec = run_grad_option(name, option)
    if rec is None:
        pytest.skip(f"{label}: an earlier option already ran this pair of kernels")
    assert sum(t == tensor for _, _, t, *_ in rec) == 2 and not _failures(rec, tensor), _failures(rec, tensor)


@functools.lru_cache(maxsize=None)
def run_entry(name, entry):
    """crba / aba / forward_dynamics of one robot (fp32, 130 rows, both regimes; no option reaches their one launch)."""
    rbd = rbd_for(name)
    rec = _FdRecords()
    kernel = {"crba": "crba_kernel<float>", "aba": "aba_kernel<float>", "forward_dynamics": "aba_kernel<float> (forward_dynamics)"}[entry]
    for regime in sorted(ew.REGIMES):
        g = ew.REGIMES[regime]["GRAVITY"]
        q, qd, u = _dev(*ew.inputs(rbd.n, regime))
        Y = ew.yardstick(name, regime, entry)
        if entry == "crba":
            rec.add(name, regime, kernel, entry, "H", rbd.crba(q), Y["H"])
        elif entry == "aba":
            rec.add(name, regime, kernel, entry, "qdd", rbd.aba(q, qd, u, GRAVITY=g), Y["qdd"])
        else:
            rec.add(name, regime, kernel, entry, "qdd", rbd.forward_dynamics(q, qd, u, GRAVITY=g), Y["qdd"])
    return rec


@pytest.mark.parametrize("name", all_golden_names())
@pytest.mark.parametrize("entry", ["crba", "aba", "forward_dynamics"])
def test_crba_aba_forward_dynamics_entrywise(entry, name):
    rec = run_entry(name, entry)
    assert len(rec) == 2 and not rec.failures(), rec.failures()


def test_branch_table_matches_the_library():
    """BRANCH against what the prebuilt libraries say of themselves: the one-lane minv kernel serves exactly the robots of
    the chain and lane branches; only the neg_mm branch has the dc_du workspace (FdWorkspace: GRAD_ACC_IN_REGS ? 0 : B 2 N N);
    only the chain robots have the pipelined chain kernel as their batch-parallel gradient kernel.  The group sizes and pair
    counts of the table are recomputed from the robots' parent arrays."""
    from rbdreference_amd import _lib as L
    assert sorted(BRANCH) == all_golden_names()
    for name, (branch, rows, pairs) in BRANCH.items():
        rbd = rbd_for(name)
        n = rbd.n
        parent = [make_robot(name).get_parent_id(i) for i in range(n)]
        anc = [set() for _ in range(n)]
        for i, p in enumerate(parent):
            anc[i] = ({p} | anc[p]) if p >= 0 else set()
        assert n + 2 * sum(len(a) for a in anc) == pairs, (name, n + 2 * sum(len(a) for a in anc))
        assert (pairs <= 72) == (branch != "neg_mm"), name
        try:
            minv = set()
            for option in OPTIONS:
                _set(rbd, option)
                minv.add(rbd._lib.kernel_name(L.RBD_OP_MINV, 4, ew.B).split("<")[0])
            _set(rbd, "BATCH")
            grad = rbd._lib.kernel_name(L.RBD_OP_RNEA_GRAD, 4, ew.B)
        finally:
            _restore(rbd)
        assert (minv == {"minv_lane_kernel"}) == (branch != "neg_mm") == (rows <= 8), (name, minv)
        assert "minv_lane_kernel" not in minv or len(minv) == 1, (name, minv)
        assert grad.startswith("rnea_grad_idsva_pipe_kernel<") == (branch == "chain"), (name, grad)
        ws = int(rbd._lib.resolve("rbd_forward_dynamics_grad", "f32").rbd_fd_workspace_bytes(ew.B, 4))
        assert (ws >= ew.B * 2 * n * n * 4) == (branch == "neg_mm"), (name, ws)


def test_every_branch_and_every_fused_qdd_was_measured():
    """The nine robots cover the three branches of fd_launch and the four minv kernels that carry the fused qdd: the one-lane
    kernel, the fused kernel, the eight-lane phase A (it finishes the groups of at most 8 bodies: Atlas's legs) and the
    column kernel (behind either phase A)."""
    ran = set()
    for name in all_golden_names():
        for option in _options(name):
            label, rec = run_grad_option(name, option)
            if rec:
                ran.add(label.replace("<float>", ""))
    assert {l.split(":")[0] for l in ran} == {"chain", "lane", "neg_mm"}, ran
    minv = {l.split(": ")[1].split(" + ")[0] for l in ran}
    assert minv == {"fd_pre_kernel", "minv_lane_kernel", "minv_fused_kernel", "minv_cols_kernel A=ia8", "minv_cols_kernel A=lane"}, minv
    assert run_grad_option("atlas_like", "IA8")[1] is not None      # (Atlas has two groups of 6 bodies and one of 18)


@functools.lru_cache(maxsize=None)
def attribution(name, generic):
    """Where the error of fd_du enters, per regime -> [(regime, R_ref, ratio of the call's fd_du, of -Minv dc_world, of
    -Minv dc_plain, of -Minv dc_mixed)].  Minv is the library's own (rbd.minv, fp32, under AUTO); dc_world is rnea_grad of the
    same world-frame kernel at the call's qdd; dc_plain is the plain-float32 C oracle's at the same qdd; dc_mixed is dc_world
    with the rows of the joints in the outer half of their chain (depth >= height) taken from dc_plain; the products are
    formed on the host in float64."""
    from oracle.c_oracle import COracle
    from rbdreference_amd import _lib as L
    if generic:
        from rbdreference_amd import RBDReference
        rbd = RBDReference(make_robot(name), build=False, generic="only")
        family = XFAIL_GENERIC[name][0]
    else:
        rbd = rbd_for(name)
        family = {f for (r, _), (f, _) in XFAIL.items() if r == name}
        assert len(family) == 1, (name, family)
        (family,) = family
        option = next(o for (r, o), (f, _) in XFAIL_GRAD.items() if r == name and f == family)      # (StopIteration: dc_du of this robot and family is no known defect)
    cf = COracle(ew._model(name), real="float")
    robot = make_robot(name)
    n = len(robot.links)
    parent = [robot.get_parent_id(i) for i in range(n)]
    depth, height = [0] * n, [0] * n
    for i in range(n):
        depth[i] = depth[parent[i]] + 1 if parent[i] >= 0 else 0
    for i in range(n - 1, -1, -1):
        if parent[i] >= 0:
            height[parent[i]] = max(height[parent[i]], height[i] + 1)
    outer = [i for i in range(n) if depth[i] >= height[i]]
    out = []
    try:
        for regime in sorted(ew.REGIMES):
            g = ew.REGIMES[regime]["GRAVITY"]
            q, qd, u = _dev(*ew.inputs(rbd.n, regime))
            y = ew.yardstick(name, regime, "forward_dynamics_grad")["fd_du"]
            qdd, d = rbd._fd(q, qd, u, g, True)[:2]
            qdd, d = qdd.clone(), d.double().cpu().numpy()
            Mi = rbd.minv(q).double().cpu().numpy()
            if not generic:
                rbd._lib.set_option(L.RBD_OPT_GRAD_KERNEL, ("AUTO", "TREE", "COLS", "BATCH").index(option))
            kernel = rbd._lib.kernel_name(L.RBD_OP_RNEA_GRAD, 4, ew.B)
            assert kernel.startswith(family + "<"), (name, kernel)
            dc_world = rbd.rnea_grad(q, qd, qdd, GRAVITY=g).double().cpu().numpy()
            if not generic:
                rbd._lib.set_option(L.RBD_OPT_GRAD_KERNEL, 0)
            dc_plain = cf.rnea_grad(*(x.cpu().numpy() for x in (q, qd, qdd)), GRAVITY=g)[1].astype(np.float64)
            dc_mixed = dc_world.copy()
            dc_mixed[:, outer] = dc_plain[:, outer]
            r = [ew.ratio(x, y.ref, y.Y) for x in (d, -Mi @ dc_world, -Mi @ dc_plain, -Mi @ dc_mixed)]
            print(f"\nATTRIBUTION {name:20s} {regime:7s} {family:28s} R_ref {y.R_ref:7.3f}  ratio / R_ref: fd_du of the call {r[0] / y.R_ref:7.3f}  "
                  f"-Minv dc_world {r[1] / y.R_ref:7.3f}  -Minv dc_plain {r[2] / y.R_ref:7.3f}  -Minv dc_mixed {r[3] / y.R_ref:7.3f} (rows {outer} from dc_plain)")
            out.append((regime, y.R_ref, *r))
    finally:
        if not generic:
            _restore(rbd)
    return out


def _defect_cases():
    return [(name, False) for name in sorted({r for r, _ in XFAIL})] + [(name, True) for name in sorted(XFAIL_GENERIC)]


@pytest.mark.parametrize("name,generic", _defect_cases())
def test_open_defects_are_the_known_world_frame_defect(name, generic):
    """Every xfail of this file is the open defect of the world-frame gradient kernels (tests/test_gpu_entrywise.py XFAIL, same
    robot, same family) passing through the -Minv product, and nothing this family adds: with the library's own fp32 Minv and
    the product formed in float64 on the host, the world-frame kernel's dc_du gives the worst ratio of the call's fd_du (within
    a factor of 2; measured: to four digits), and the plain-float32 oracle's dc_du at the same qdd is within the margin
    (measured: 0.5 .. 1.1 R_ref).  Taking only the rows of the joints in the outer half of their chain -- the rows DESIGN.md
    2.1 names -- from the oracle removes the larger part of the excess (printed; measured 22.2 -> 4.6 R_ref on atlas_like,
    34.0 -> 11.2 on iiwa_like): the rest is the inner rows' share of the same defect, the structural zeros dc_dqd[i, i] of
    every row among it."""
    if generic:
        assert XFAIL_GRAD_GENERIC[name][0] == XFAIL_GENERIC[name][0]
    else:
        known = {(r, f) for (r, _), (f, _) in XFAIL_GRAD.items()}
        for (r, option), (family, _) in XFAIL.items():
            if r == name:
                assert (name, family) in known, (name, family)
                label, _ = run_grad_option(name, option)
                assert f"+ {family}<" in label, (name, option, label)
    worst = 0.0
    for regime, R_ref, r_call, r_world, r_plain, r_mixed in attribution(name, generic):
        assert r_plain <= ew.MARGIN * R_ref, (name, regime, r_plain / R_ref)
        if r_call > ew.MARGIN * R_ref:
            assert r_world > ew.MARGIN * R_ref and 0.5 <= r_world / r_call <= 2.0, (name, regime, r_call / R_ref, r_world / R_ref)
            assert r_mixed < r_call, (name, regime, r_mixed / R_ref)
        worst = max(worst, r_call / R_ref)
    assert worst > ew.MARGIN


@functools.lru_cache(maxsize=None)
def run_generic(name, which):
    """The model-handle library, direct and staged output: 'columns' = crba, forward_dynamics and forward_dynamics_grad with
    the column-recursion gradient kernel; 'world' = forward_dynamics_grad with AUTO's world-frame gradient kernel."""
    from rbdreference_amd import RBDReference
    from rbdreference_amd._lib import RBD_OP_MINV, RBD_OP_RNEA_GRAD
    from rbdreference_amd.generic import RBD_G_GRAD_KERNEL_AUTO, RBD_G_GRAD_KERNEL_COLUMNS, load_generic_library
    rbd = RBDReference(make_robot(name), build=False, generic="only")
    lib = load_generic_library()
    rec = _FdRecords()
    q, qd, _ = _dev(*ew.inputs(rbd.n, "std"))
    rbd.rnea(q, qd)                              # (a handle exists from here on: kernel_name asks the library)
    try:
        assert lib.rbd_g_set_grad_kernel(RBD_G_GRAD_KERNEL_AUTO if which == "world" else RBD_G_GRAD_KERNEL_COLUMNS) == 0
        for staging, tag in ((1, "direct"), (2, "staged")):
            assert lib.rbd_g_set_output_staging(staging) == 0
            for regime in sorted(ew.REGIMES):
                g = ew.REGIMES[regime]["GRAVITY"]
                q, qd, u = _dev(*ew.inputs(rbd.n, regime))
                label = f"generic: {rbd._lib.kernel_name(RBD_OP_MINV, 4, ew.B)} + {rbd._lib.kernel_name(RBD_OP_RNEA_GRAD, 4, ew.B)} {tag}"
                if which == "columns":
                    rec.add(name, regime, f"generic: g_crba_kernel {tag}", "crba", "H", rbd.crba(q), ew.yardstick(name, regime, "crba")["H"])
                    rec.add(name, regime, label, "forward_dynamics", "qdd", rbd.forward_dynamics(q, qd, u, GRAVITY=g),
                            ew.yardstick(name, regime, "forward_dynamics")["qdd"])
                Y = ew.yardstick(name, regime, "forward_dynamics_grad")
                qdd, d = rbd._fd(q, qd, u, g, True)[:2]
                rec.add(name, regime, label, "fd_grad", "qdd", qdd, Y["qdd"]); rec.add(name, regime, label, "fd_grad", "fd_du", d, Y["fd_du"])
                assert rbd._lib.served_by_generic()
    finally:
        lib.rbd_g_set_grad_kernel(RBD_G_GRAD_KERNEL_AUTO)
        lib.rbd_g_set_output_staging(0)
    return rec


def _generic_cases():
    for name in ("iiwa_like", "random_limbs_n14"):
        for which, tensors in (("columns", ("H", "qdd", "fd_du")), ("world", ("qdd", "fd_du"))):
            for tensor in tensors:
                yield pytest.param(name, which, tensor, marks=_xfail(XFAIL_GENERIC.get(name) if (which, tensor) == ("world", "fd_du") else None),
                                   id=f"{name}-{which}-{tensor}")


@pytest.mark.parametrize("name,which,tensor", list(_generic_cases()))
def test_model_handle_library_entrywise(name, which, tensor):
    rec = run_generic(name, which)
    grads = {k.split(" + ")[1].split("<")[0] for k, *_ in rec if " + " in k}
    assert grads == ({"g_rnea_grad_world_kernel"} if which == "world" else {"g_rnea_grad_kernel"}), grads
    assert len(rec) == (8 if which == "world" else 16)       # two ways out of the kernels, two regimes: 2 and 4 tensors each
    assert any(t == tensor for _, _, t, *_ in rec) and not _failures(rec, tensor), _failures(rec, tensor)
