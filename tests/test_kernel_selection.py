"""Kernel selection, pinned (CPU only: rbd_kernel_name and rbd_minv_workspace_bytes are host code).

For five robots that between them reach every selection path -- one chain (pipelined / plain chain kernel, column kernel
below the batch threshold), a forest (two-lane kernel), a robot with limbs (segment waves, tree / workspace tree kernel,
fused and two-phase minv with its workspace) and a floating base -- in both precisions, under every value of
RBD_OPT_RNEA_KERNEL, RBD_OPT_GRAD_KERNEL and RBD_OPT_MINV_PHASE_A, with RBD_OPT_SELECT_BATCH at 0 and at 2^20 and B on both
sides of the column kernel's threshold (8192 rows), the library must name the kernels in the tables below.

The tables were recorded from libraries built at the commit BEFORE the host layer got one selection function per family
(every combination of the options was queried; each answer depended on its own option, the select batch and B only, which
is the form the tables have).  They are literals, never recomputed from the code under test.
"""
import ctypes
import itertools

import pytest

from conftest import make_robot

from rbdreference_amd import pack_robot

BATCHES = (8, 4096, 8192, 8193, 1 << 20)
SELECT_BATCHES = (0, 1 << 20)
OPT_GRAD, OPT_MINV, OPT_RNEA, OPT_SELECT = 0, 1, 2, 3
OP_RNEA, OP_GRAD, OP_MINV = 0, 1, 2

# RBD_OP_RNEA by RBD_OPT_RNEA_KERNEL (AUTO, BATCH, GROUPS); "%s" is float / double
RNEA = {
    "iiwa_like": ("rnea_kernel<%s>",) * 3,
    "random_chain_n7": ("rnea_kernel<%s>",) * 3,
    "random_forest_n8": ("rnea_kernel<%s>",) * 3,
    "random_limbs_n14": ("rnea_segments_kernel<%s>", "rnea_kernel<%s>", "rnea_kernel<%s>"),
    "fb_random_tree_n6": ("rnea_fbw_kernel<%s,true>",) * 3,
}
# RBD_OP_RNEA_GRAD by RBD_OPT_GRAD_KERNEL (AUTO, TREE, COLS, BATCH).  A string: for every B and select batch; a pair: (with
# select batch 0, one name per entry of BATCHES; with select batch 2^20)
_COLS32, _PIPE32, _TWO32 = "rnea_grad_cols_kernel<float,true>", "rnea_grad_idsva_pipe_kernel<float,true,false>", "rnea_grad_kernel<float,true,false>"
_CHAIN64, _TWO64 = "rnea_grad_idsva_kernel<double,true,false>", "rnea_grad_kernel<double,true,false>"
_TREE32, _TREE64, _TWS64 = "rnea_grad_tree_kernel<float,true>", "rnea_grad_tree_kernel<double,true>", "rnea_grad_tree_ws_kernel<double,true>"
_CHAIN_ROBOT = {4: (((_COLS32, _COLS32, _COLS32, _PIPE32, _PIPE32), _PIPE32), _TREE32, _COLS32, _PIPE32),
                8: (_CHAIN64, _TWS64, _CHAIN64, _CHAIN64)}
GRAD = {
    "iiwa_like": _CHAIN_ROBOT,
    "random_chain_n7": _CHAIN_ROBOT,
    "random_forest_n8": {4: (((_COLS32, _COLS32, _COLS32, _TWO32, _TWO32), _TWO32), _TREE32, _COLS32, _TWO32),
                         8: (_TWO64, _TREE64, _TWO64, _TWO64)},
    "random_limbs_n14": {4: (_TREE32,) * 4, 8: (_TWS64,) * 4},
    "fb_random_tree_n6": {4: ("rnea_grad_fbw_kernel<float,true>", "rnea_grad_fbw_kernel<float,true>", "rnea_grad_fb_kernel<float,true>",
                              "rnea_grad_fbw_kernel<float,true>"),
                          8: ("rnea_grad_fbw_kernel<double,true>", "rnea_grad_fbw_kernel<double,true>", "rnea_grad_fb_kernel<double,true>",
                              "rnea_grad_fbw_kernel<double,true>")},
}
# RBD_OP_MINV by RBD_OPT_MINV_PHASE_A (AUTO, LANE, IA8, FUSED), for every B and select batch
MINV = {
    "iiwa_like": ("minv_lane_kernel<%s>",) * 4,
    "random_chain_n7": ("minv_lane_kernel<%s>",) * 4,
    "random_forest_n8": ("minv_lane_kernel<%s>",) * 4,
    "random_limbs_n14": ("minv_fused_kernel<%s>", "minv_cols_kernel<%s>", "minv_cols_kernel<%s>", "minv_fused_kernel<%s>"),
    "fb_random_tree_n6": ("minv_fbm_kernel<%s>", "minv_fb_kernel<%s>", "minv_fbm_kernel<%s>", "minv_fbm_kernel<%s>"),
}
# rbd_minv_workspace_bytes(B, elem_size) / B by RBD_OPT_MINV_PHASE_A: {elem_size: bytes per row}
MINV_WS_PER_ROW = {
    "iiwa_like": ({4: 0, 8: 0},) * 4,
    "random_chain_n7": ({4: 0, 8: 0},) * 4,
    "random_forest_n8": ({4: 0, 8: 0},) * 4,
    "random_limbs_n14": ({4: 0, 8: 0}, {4: 672, 8: 1344}, {4: 672, 8: 1344}, {4: 0, 8: 0}),
    "fb_random_tree_n6": ({4: 0, 8: 0},) * 4,
}
NO_WORKSPACE_KERNELS = ("minv_lane_kernel", "minv_fused_kernel", "minv_fbm_kernel", "minv_fb_kernel")


def _name(L, op, esz, B):
    buf = ctypes.create_string_buffer(128)
    assert L.rbd_kernel_name(op, esz, B, buf, len(buf)) == 0, L.rbd_last_error()
    return buf.value.decode()


@pytest.mark.parametrize("robot", sorted(RNEA))
def test_kernel_names_and_minv_workspace_follow_the_recorded_selection(robot):
    from rbdreference_amd._lib import RbdLibrary
    L = RbdLibrary(pack_robot(make_robot(robot)), build=True, lazy=False).lib
    try:
        for rnea_opt, grad_opt, minv_opt, sel in itertools.product(range(3), range(4), range(4), SELECT_BATCHES):
            for opt, val in ((OPT_RNEA, rnea_opt), (OPT_GRAD, grad_opt), (OPT_MINV, minv_opt), (OPT_SELECT, sel)):
                assert L.rbd_set_option(opt, val) == 0
            for esz, t in ((4, "float"), (8, "double")):
                for ib, B in enumerate(BATCHES):
                    where = (robot, t, rnea_opt, grad_opt, minv_opt, sel, B)
                    assert _name(L, OP_RNEA, esz, B) == RNEA[robot][rnea_opt] % t, where
                    want = GRAD[robot][esz][grad_opt]
                    if not isinstance(want, str):
                        want = want[1] if sel else want[0][ib]
                    assert _name(L, OP_GRAD, esz, B) == want, where
                    minv = _name(L, OP_MINV, esz, B)
                    assert minv == MINV[robot][minv_opt] % t, where
                    ws = L.rbd_minv_workspace_bytes(B, esz)
                    assert ws == MINV_WS_PER_ROW[robot][minv_opt][esz] * B, where
                    assert (ws == 0) == minv.startswith(NO_WORKSPACE_KERNELS), where
    finally:
        for opt in (OPT_RNEA, OPT_GRAD, OPT_MINV, OPT_SELECT):
            L.rbd_set_option(opt, 0)
