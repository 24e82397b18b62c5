/* rbd_hip.h -- C-ABI of the MI355X batched rigid-body-dynamics back-end.
 *
 * One shared library is built PER ROBOT (librbd_<name>_<hash>.so): topology, joint axes, tree
 * transforms and inertias are compile-time constants of its kernels, so the entry points take no
 * model handle.  The reference offers no FFI of its own; the boundary it does offer is the Python
 * class  RBDReference(robot).rnea / .rnea_grad / .minv  (/root/reference/RBDReference.py:623,
 * :1345, :785; README.md:15-17).  Each entry point below replaces one of those methods for a whole
 * batch of configurations; rbdreference_amd/api.py binds them with ctypes (INTEGRATION.md shows the
 * stub a maintainer of the reference would add).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer to a dense row-major array, batch index outermost;
 *     the caller owns all buffers; nothing is allocated per call -- with ONE exception: rbd_rnea_grad_f64 /
 *     rbd_rnea_with_grad_f64 of a tree too big for registers and LDS (the 30-body humanoid; rbd_kernel_name says
 *     rnea_grad_tree_ws_kernel) keeps a LIBRARY-OWNED scratch buffer per (device, stream), sized by what is resident
 *     at once, not by B (126 MB for that robot): allocated (hipMalloc) by the first such call on a stream and reused by
 *     every later one.  A buffer that was handed out is never freed or moved by a later call (launches in flight,
 *     bound launches and captured graphs may hold its address); rbd_release_workspaces() frees them all.  GRAPH
 *     CAPTURE: make one such call on a stream before capturing calls on it into a hipGraph (hipMalloc is not
 *     capturable), and do not call rbd_release_workspaces() while such a graph may still be launched.  Calls on
 *     different streams use different buffers, calls on one stream are ordered and share one;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream of the calling thread's current device);
 *     launches are asynchronous; every entry point runs on the STREAM's device (it switches the calling thread's
 *     current device for the duration of the call if that is another one), and per-kernel launch attributes, grid
 *     sizes and the library-owned workspace are cached per that device;
 *   - return 0 on success, <0 for argument errors (RBD_ERR_*), >0 = hipError_t of a failed launch;
 *     rbd_last_error() returns a thread-local message for the last non-zero return;
 *   - no C++ exceptions cross this boundary; the model is immutable, so concurrent calls from
 *     several host threads / streams are safe.
 *
 * Output buffers (c, v, a, f, dc_du, Minv, qdd, ...) and workspaces must be 16-byte aligned -- any device
 * allocation is; a view into the middle of one may not be -- the kernels store 16-byte pieces.  A misaligned
 * output is refused with RBD_ERR_ARG.  Inputs may have any alignment of their element type.
 *
 * Floating-base robots (RBDReference.py:585-593, :652-691, :761-779; robot.floating_base): body 0
 * owns indices 0..5 of q, qd, qdd, c (q[0:6] = px, py, pz, rx, ry, rz of the world -> base transform,
 * qd[0:6] = the base twist in base coordinates), body i >= 1 owns index i + 5; "n" in the shapes
 * below then reads nv = n + 5 for q, qd, qdd, c, u, Minv and stays the body count for v, a, f.  Such a
 * library serves rbd_rnea, rbd_rnea_grad and rbd_rnea_with_grad -- dc_du [B, nv, 2 nv]; the base's six position
 * columns are derivatives along a base-frame twist, as in the reference, :1168-1175; robots with fewer
 * than six bodies are refused: the reference raises IndexError for them, :1168 -- rbd_minv and
 * rbd_forward_dynamics; every other entry point returns RBD_ERR_UNSUPPORTED (the reference's own
 * crba / aba raise for floating bases).
 */
#ifndef RBD_HIP_H
#define RBD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBD_MAX_BODIES 64

#define RBD_ERR_ARG (-1)          /* null / inconsistent arguments                         */
#define RBD_ERR_UNSUPPORTED (-2)  /* robot too large for this kernel's on-chip working set  */
#define RBD_ERR_WORKSPACE (-3)    /* workspace missing or too small                        */
#define RBD_ERR_NOT_BUILT (-4)    /* a FAMILY library (first-use build, rbdreference_amd/build.py) was asked for an entry
                                     point of another family: the caller picked the wrong library, nothing ran      */

typedef struct rbd_model_info {
  int32_t abi_version;
  int32_t n;                          /* bodies == joints == velocities (fixed base, 1-DoF)  */
  int32_t max_depth;                  /* longest root path, in bodies                        */
  uint64_t hash;                      /* first 64 bits of sha256 over the packed model       */
  char name[64];
  int32_t parent[RBD_MAX_BODIES];     /* -1 = child of the fixed base                        */
  int32_t joint_type[RBD_MAX_BODIES]; /* 0 revolute, 1 prismatic, 2 = the 6-DoF floating base */
  int32_t joint_axis[RBD_MAX_BODIES]; /* 0/1/2 = x/y/z of the body frame                     */
  int32_t floating_base;              /* 1: body 0 is attached by a 6-DoF joint (S = eye(6)), */
  int32_t nv;                         /*    and q, qd, qdd, c have nv = n + 5 columns (else n) */
} rbd_model_info_t;

int rbd_abi_version(void);
const char* rbd_last_error(void);
/* Frees every library-owned workspace (see "Conventions").  Synchronises each device that holds one first.  The caller
 * guarantees that no call into this library is in flight on another thread and that no captured graph containing one
 * of its launches will be replayed.  Returns 0, or the hipError_t of a failed synchronisation. */
int rbd_release_workspaces(void);
/* The robot this library was compiled for (host-side, no GPU needed). */
int rbd_model_info(rbd_model_info_t* out);

/* Kernel selection.  Several kernels may serve one entry point; which one runs is
 * decided per robot at compile time and per launch from B.  rbd_set_option overrides the choice
 * where the override is built into the library (tests run every kernel of every robot this way;
 * a value the library cannot honour is ignored).  Options only ever select between kernels that
 * compute the same result.  Process-wide, thread-safe, no environment variables are read.
 *   RBD_OPT_GRAD_KERNEL    rbd_rnea_grad: AUTO | TREE (chain-by-chain world-frame kernel) | COLS (one
 *                          lane per derivative column: AUTO picks it for small batches) | BATCH (the
 *                          robot's batch-parallel kernel at every batch size)
 *   RBD_OPT_MINV_PHASE_A   rbd_minv, robots too big for the one-lane kernel: AUTO | LANE (phase A with one lane
 *                          per configuration, then the column kernel) | IA8 (eight lanes per configuration,
 *                          then the column kernel) | FUSED (one launch from q to Minv; robots whose big
 *                          root subtrees have limbs; what AUTO picks for them)
 *   RBD_OPT_RNEA_KERNEL    rbd_rnea with v, a, f: AUTO | BATCH (one lane per configuration) | GROUPS (one
 *                          wave per independent root subtree).  AUTO: robots whose root subtrees carry
 *                          several big branches (Atlas' arms) get one wave per branch / stem / root
 *                          subtree, other multi-root robots GROUPS, single chains BATCH
 *   RBD_OPT_SELECT_BATCH   rows of the GLOBAL batch a call is a shard of (0 = the call's own B, the default).
 *                          Wherever AUTO decides from the batch size (the small-batch column kernel of
 *                          rbd_rnea_grad, phase A of rbd_minv), it decides from this number instead: a shard of
 *                          a sharded batch then runs the kernel the unsharded call would run, so sharded and
 *                          unsharded results are bit-identical row by row (rbdreference_amd.dist.ShardedRBD sets it)
 *   RBD_OPT_STORE_POLICY   how the one-lane chain gradient kernels (rbd_rnea_grad, rbd_forward_dynamics_grad of a
 *                          one-chain robot) store their finished rows: AUTO | PLAIN | WRITE_THROUGH (16-byte
 *                          write-through stores: nothing dirty is left in L2 for the end of the launch to write
 *                          back) | WRITE_THROUGH_NT (the same, non-temporal).  AUTO goes by the bytes the launch
 *                          writes: plain up to 4 MiB (a small result stays in L2 for its consumer), write-through
 *                          up to 64 MiB, non-temporal above.  The same bytes are written either way.
 * rbd_kernel_name writes the name of the kernel (the dominant one of a multi-launch entry point) that
 * `op` would launch for a batch of B rows of elem_size-byte scalars under the current options. */
#define RBD_OPT_GRAD_KERNEL 0
#define RBD_OPT_MINV_PHASE_A 1
#define RBD_OPT_RNEA_KERNEL 2
#define RBD_OPT_SELECT_BATCH 3
#define RBD_OPT_STORE_POLICY 4
#define RBD_OPT_COUNT_ 5
#define RBD_GRAD_KERNEL_AUTO 0
#define RBD_GRAD_KERNEL_TREE 1
#define RBD_GRAD_KERNEL_COLS 2
#define RBD_GRAD_KERNEL_BATCH 3
#define RBD_RNEA_KERNEL_AUTO 0
#define RBD_RNEA_KERNEL_BATCH 1
#define RBD_RNEA_KERNEL_GROUPS 2
#define RBD_MINV_PHASE_A_AUTO 0
#define RBD_MINV_PHASE_A_LANE 1
#define RBD_MINV_PHASE_A_IA8 2
#define RBD_MINV_PHASE_A_FUSED 3
#define RBD_STORE_POLICY_AUTO 0
#define RBD_STORE_POLICY_PLAIN 1
#define RBD_STORE_POLICY_WRITE_THROUGH 2
#define RBD_STORE_POLICY_WRITE_THROUGH_NT 3
#define RBD_OP_RNEA 0
#define RBD_OP_RNEA_GRAD 1
#define RBD_OP_MINV 2
int rbd_set_option(int option, int value);
int rbd_get_option(int option);
int rbd_kernel_name(int op, int elem_size, int64_t B, char* buf, size_t len);

/* RBDReference.rnea(q, qd, qdd=None, GRAVITY)            (RBDReference.py:623-628)
 *   q, qd, qdd : [B, n]   (qdd may be NULL == the reference's qdd=None, :589)
 *   c          : [B, n]
 *   v, a, f    : [B, 6, n] or all three NULL; f is the ACCUMULATED force the reference returns
 *                (its backward pass adds child forces in place, :619).                        */
int rbd_rnea_f32(const float* q, const float* qd, const float* qdd, float gravity, int64_t B,
                 float* c, float* v, float* a, float* f, void* stream);
int rbd_rnea_f64(const double* q, const double* qd, const double* qdd, double gravity, int64_t B,
                 double* c, double* v, double* a, double* f, void* stream);

/* Per-pass surface the reference designates for accelerator testing (README.md:19):
 * RBDReference.rnea_fpass(q, qd, qdd=None, GRAVITY) -> (v, a, f) with f LOCAL  (RBDReference.py:559-598)
 * RBDReference.rnea_bpass(q, f) -> (c, f): accumulates child forces into f IN PLACE (RBDReference.py:600-621) */
int rbd_rnea_fpass_f32(const float* q, const float* qd, const float* qdd, float gravity, int64_t B,
                       float* v, float* a, float* f, void* stream);
int rbd_rnea_fpass_f64(const double* q, const double* qd, const double* qdd, double gravity, int64_t B,
                       double* v, double* a, double* f, void* stream);
int rbd_rnea_bpass_f32(const float* q, float* f, int64_t B, float* c, void* stream);
int rbd_rnea_bpass_f64(const double* q, double* f, int64_t B, double* c, void* stream);

/* Gradient passes (README.md:19).  Layouts as the reference returns them, batch outermost:
 *   dv, da, df : [B, 6, n, NB]  -- element [b, r, c, i] = d(component r of body i) / d u_c
 * RBDReference.rnea_grad_fpass_dq(q, qd, v, a, GRAVITY) -> (dv_dq, da_dq, df_dq)     (RBDReference.py:1127-1187)
 *   v, a [B,6,NB] are the outputs of rnea (a includes the S qdd term, :1353-1358).
 * RBDReference.rnea_grad_fpass_dqd(q, qd, v) -> (dv_dqd, da_dqd, df_dqd)             (RBDReference.py:1189-1255)
 * RBDReference.rnea_grad_bpass_dq(q, f, df_dq) -> dc_dq [B,n,n]                      (RBDReference.py:1257-1297)
 *   f [B,6,NB] is the ACCUMULATED rnea force (:1353,:1362); df_dq is accumulated child -> parent
 *   IN PLACE as the reference does (:1291-1294).
 * RBDReference.rnea_grad_bpass_dqd(q, df_dqd, USE_VELOCITY_DAMPING) -> dc_dqd [B,n,n] (RBDReference.py:1299-1343)
 *   df_dqd accumulated in place (:1331). */
int rbd_rnea_grad_fpass_dq_f32(const float* q, const float* qd, const float* v, const float* a, float gravity, int64_t B,
                               float* dv_dq, float* da_dq, float* df_dq, void* stream);
int rbd_rnea_grad_fpass_dqd_f32(const float* q, const float* qd, const float* v, int64_t B, float* dv_dqd, float* da_dqd,
                                float* df_dqd, void* stream);
int rbd_rnea_grad_bpass_dq_f32(const float* q, const float* f, float* df_dq, int64_t B, float* dc_dq, void* stream);
int rbd_rnea_grad_bpass_dqd_f32(const float* q, float* df_dqd, int use_damping, int64_t B, float* dc_dqd, void* stream);
int rbd_rnea_grad_fpass_dq_f64(const double* q, const double* qd, const double* v, const double* a, double gravity, int64_t B,
                               double* dv_dq, double* da_dq, double* df_dq, void* stream);
int rbd_rnea_grad_fpass_dqd_f64(const double* q, const double* qd, const double* v, int64_t B, double* dv_dqd, double* da_dqd,
                                double* df_dqd, void* stream);
int rbd_rnea_grad_bpass_dq_f64(const double* q, const double* f, double* df_dq, int64_t B, double* dc_dq, void* stream);
int rbd_rnea_grad_bpass_dqd_f64(const double* q, double* df_dqd, int use_damping, int64_t B, double* dc_dqd, void* stream);

/* RBDReference.rnea_grad(q, qd, qdd=None, GRAVITY, USE_VELOCITY_DAMPING)   (RBDReference.py:1345-1368)
 *   dc_du : [B, n, 2n] = [dc_dq | dc_dqd]  (np.hstack, :1367)
 *   c     : [B, n] or NULL -- the bias force the reference computes on the way (:1353) and drops. */
int rbd_rnea_grad_f32(const float* q, const float* qd, const float* qdd, float gravity,
                      int use_damping, int64_t B, float* c, float* dc_du, void* stream);
int rbd_rnea_grad_f64(const double* q, const double* qd, const double* qdd, double gravity,
                      int use_damping, int64_t B, double* c, double* dc_du, void* stream);

/* rnea + rnea_grad in one call: everything RBDReference.rnea (:623-628) and RBDReference.rnea_grad
 * (:1345-1368) return for the same (q, qd, qdd) -- the reference's rnea_grad runs rnea internally
 * (:1353) and drops its outputs.  c [B,n]; v, a, f [B,6,n] (f accumulated); dc_du [B,n,2n]; all
 * non-null.  For small batches this is ONE launch (one lane per derivative column), otherwise the rnea
 * kernel followed by the gradient kernel on `stream`. */
int rbd_rnea_with_grad_f32(const float* q, const float* qd, const float* qdd, float gravity, int use_damping,
                           int64_t B, float* c, float* v, float* a, float* f, float* dc_du, void* stream);
int rbd_rnea_with_grad_f64(const double* q, const double* qd, const double* qdd, double gravity, int use_damping,
                           int64_t B, double* c, double* v, double* a, double* f, double* dc_du, void* stream);

/* RBDReference.minv(q, output_dense)                      (RBDReference.py:785-806)
 *   Minv : [B, n, n].  output_dense != 0: symmetric matrix (:799-804).  output_dense == 0: upper
 *   triangle as the reference defines it, strict lower triangle ZERO (the reference leaves
 *   by-products of its forward pass there, :771; documented deviation).
 *   workspace: device scratch of at least rbd_minv_workspace_bytes(B, sizeof(T)) bytes, 16-byte
 *   aligned.  0 bytes -- and then ignored, NULL is fine -- whenever the kernel selected by the current
 *   RBD_OPT_MINV_PHASE_A option does not go through HBM (the one-lane kernel of small robots, the
 *   one-launch kernel that AUTO picks for robots whose big groups have limbs): query it again after
 *   changing that option.                                                                          */
size_t rbd_minv_workspace_bytes(int64_t B, int elem_size);
int rbd_minv_f32(const float* q, int64_t B, int output_dense, float* Minv, void* workspace,
                 size_t workspace_bytes, void* stream);
int rbd_minv_f64(const double* q, int64_t B, int output_dense, double* Minv, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Minv passes (README.md:19).
 * RBDReference.minv_bpass(q) -> (Minv, F, U, Dinv)                                   (RBDReference.py:630-735)
 *   Minv [B,n,n]: row i filled on the columns of subtree(i) only (:700-708), zero elsewhere;
 *   F [B,n,6,n]; U [B,n,6]; Dinv [B,n] holds D = S^T U, NOT its inverse, exactly as the reference's
 *   array of that name does (:698).
 * RBDReference.minv_fpass(q, Minv, F, U, Dinv) -> Minv                               (RBDReference.py:737-783)
 *   Minv is updated IN PLACE over whole rows (:771), so its strict lower triangle receives the
 *   same by-products as in the reference; F is rebuilt (:774-781), its incoming contents are not read. */
int rbd_minv_bpass_f32(const float* q, int64_t B, float* Minv, float* F, float* U, float* Dinv, void* stream);
int rbd_minv_fpass_f32(const float* q, int64_t B, float* Minv, float* F, const float* U, const float* Dinv, void* stream);
int rbd_minv_bpass_f64(const double* q, int64_t B, double* Minv, double* F, double* U, double* Dinv, void* stream);
int rbd_minv_fpass_f64(const double* q, int64_t B, double* Minv, double* F, const double* U, const double* Dinv, void* stream);

/* RBDReference.crba(q)  (fixed-base branch, RBDReference.py:1091-1124): joint-space inertia H [B, n, n]. */
int rbd_crba_f32(const float* q, int64_t B, float* H, void* stream);
int rbd_crba_f64(const double* q, int64_t B, double* H, void* stream);

/* RBDReference.aba(q, qd, tau, f_ext=[], GRAVITY)  (fixed-base branch, RBDReference.py:940-1024) -> qdd [B, n].
 * Articulated-body algorithm; f_ext is not part of the C-ABI (the fixed-base branch never reads it).
 * Same result as the forward-dynamics entry points below, i.e. Minv (tau - c), to rounding; no workspace. */
int rbd_aba_f32(const float* q, const float* qd, const float* tau, float gravity, int64_t B, float* qdd, void* stream);
int rbd_aba_f64(const double* q, const double* qd, const double* tau, double gravity, int64_t B, double* qdd, void* stream);

/* RBDReference.forward_dynamics(q, qd, u)                 (RBDReference.py:1371-1374)
 *   qdd = minv(q) @ (u - rnea(q, qd)[0])        u, qdd : [B, n]
 * RBDReference.forward_dynamics_grad(q, qd, u)            (RBDReference.py:1376-1384)
 *   dqdd_du : [B, n, 2n] = [qdd_dq | qdd_dqd] = -minv(q) @ rnea_grad(q, qd, qdd)  (the reference
 *   returns the two halves as a tuple); qdd (nullable) also receives the forward dynamics itself.
 *   forward_dynamics is one launch (the articulated-body sweeps of rbd_aba give Minv (u - c) without
 *   forming either factor; its workspace arguments are accepted and unused).  forward_dynamics_grad
 *   is three / four launches on `stream`: rnea (bias force), minv with the Minv (u - c) product
 *   fused in, rnea_grad with the -Minv product fused into its epilogue; it needs a device scratch of
 *   at least rbd_fd_workspace_bytes(B, sizeof(T)) bytes, 16-byte aligned. */
size_t rbd_fd_workspace_bytes(int64_t B, int elem_size);
int rbd_forward_dynamics_f32(const float* q, const float* qd, const float* u, float gravity, int64_t B,
                             float* qdd, void* workspace, size_t workspace_bytes, void* stream);
int rbd_forward_dynamics_f64(const double* q, const double* qd, const double* u, double gravity, int64_t B,
                             double* qdd, void* workspace, size_t workspace_bytes, void* stream);
int rbd_forward_dynamics_grad_f32(const float* q, const float* qd, const float* u, float gravity, int64_t B,
                                  float* qdd, float* dqdd_du, void* workspace, size_t workspace_bytes,
                                  void* stream);
int rbd_forward_dynamics_grad_f64(const double* q, const double* qd, const double* u, double gravity,
                                  int64_t B, double* qdd, double* dqdd_du, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* RBDReference.end_effector_pose / end_effector_pose_gradient        (RBDReference.py:220-274, :286-386)
 * Fixed-base robots; a floating-base library returns RBD_ERR_UNSUPPORTED.  ONE launch computes pose, gradient or both.
 *   q         : [B, n] device
 *   site_body : int32 [n_sites], HOST -- body whose frame carries site s (0 <= id < n)
 *   site_T    : double [n_sites][12], HOST -- constant body -> site transform [R | t], row-major 3 x 4 (identity for the
 *               joint's link frame, the fixed frame's pose for a fixed joint)
 *   offset    : double [4], HOST -- ee_offsets[0] = (x, y, z, w) of the reference, shared by every site
 *   n_sites   : 1 .. RBD_EE_MAX_SITES, passed to the kernel by value
 *   pose      : [B, n_sites, 6]    xyz of R_s o + w t_s, then roll / pitch / yaw as the reference extracts them (:245-258)
 *   dpose     : [B, n_sites, 6, n] d pose / d q; zero columns for joints off the site's chain (:357-359, :378-380)
 *   Either output may be NULL (not both).  Arguments are checked before anything touches the GPU; B == 0 is a no-op. */
#define RBD_EE_MAX_SITES 16
int rbd_ee_pose_f32(const float* q, int64_t B, const int32_t* site_body, const double* site_T, const double* offset,
                    int n_sites, float* pose, float* dpose, void* stream);
int rbd_ee_pose_f64(const double* q, int64_t B, const int32_t* site_body, const double* site_T, const double* offset,
                    int n_sites, double* pose, double* dpose, void* stream);

/* RBDReference.second_order_idsva_parallel                                                        (RBDReference.py:1387-1604)
 * Fixed-base robots; a floating-base library returns RBD_ERR_UNSUPPORTED.
 *   q, qd, qdd : [B, n] device
 *   out        : [B, 4, n, n, n] = d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq, every entry written (zeros included)
 *                d2tau_dq[i][j][k] = d2 c_i / dq_j dq_k,  d2tau_dqd[i][j][k] = d2 c_i / dqd_j dqd_k,
 *                d2tau_dvdq[i][j][k] = d (dc_dqd[i][j]) / dq_k,  dM_dq[i][j][k] = d H_ij / dq_k
 *                (c = rnea(q, qd, qdd, gravity), H = crba(q)).  The composite-force sweep adds the child's force (the
 *                reference's :1448 adds f[:, pi + 1]): on a branched robot d2tau_dq is the true derivative where the
 *                reference's is not; elsewhere the two agree.
 * Arguments are checked before anything touches the GPU; B == 0 is a no-op. */
int rbd_second_order_idsva_f32(const float* q, const float* qd, const float* qdd, float gravity, int64_t B, float* out,
                               void* stream);
int rbd_second_order_idsva_f64(const double* q, const double* qd, const double* qdd, double gravity, int64_t B,
                               double* out, void* stream);

/* RBDReference.fdsva_so: second derivatives of forward dynamics                                  (RBDReference.py:1606-1631)
 * Fixed-base robots; a floating-base library returns RBD_ERR_UNSUPPORTED.
 *   q, qd, u : [B, n] device
 *   out      : [B, 4, n, n, n] = daba_dqdq, daba_dvdq, daba_dvdv, daba_dtdq, every entry written (zeros included).  With
 *              qdd = forward_dynamics(q, qd, u), [fd_dq | fd_dqd] = forward_dynamics_grad(q, qd, u), Minv = minv(q) and
 *              (d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq) = second_order_idsva(q, qd, qdd), all at the given gravity:
 *                daba_dqdq[i][j][k] = -sum_l Minv[i][l] (d2tau_dq[l][j][k] + sum_m dM_dq[l][m][k] fd_dq[m][j]
 *                                                                            + sum_m dM_dq[l][m][j] fd_dq[m][k])
 *                daba_dvdq[i][j][k] = -sum_l Minv[i][l] (d2tau_dvdq[l][j][k] + sum_m dM_dq[l][m][k] fd_dqd[m][j])
 *                daba_dvdv[i][j][k] = -sum_l Minv[i][l] d2tau_dqd[l][j][k]
 *                daba_dtdq[i][j][k] = -sum_l Minv[i][l] sum_m dM_dq[l][m][k] Minv[m][j]  (= d Minv[i][j] / dq_k)
 *              The second-order inverse-dynamics tensors are this library's (true derivatives on branched robots, see
 *              above), so daba_dqdq differs from the reference's on branched robots.  fd_dq is forward_dynamics_grad's:
 *              on a robot with prismatic joints it is not the q-derivative of qdd (the reference's rnea_grad, reproduced
 *              for parity), and daba_dqdq then is not the second derivative.  One gravity in every stage (the reference
 *              evaluates forward dynamics at -9.81 whatever GRAVITY is).
 *   ws       : device scratch of at least the bytes the workspace query below reports for (B, elem_size), 16-byte
 *              aligned; every intermediate lives there.  Everything runs on `stream`.
 * Arguments are checked before anything touches the GPU (null pointer, B < 0, B too large, workspace too small:
 * RBD_ERR_ARG); B == 0 is a no-op. */
size_t rbd_fdsva_so_workspace_bytes(int64_t B, int elem_size);
int rbd_fdsva_so_f32(const float* q, const float* qd, const float* u, float gravity, int64_t B, float* out, void* ws,
                     size_t ws_bytes, void* stream);
int rbd_fdsva_so_f64(const double* q, const double* qd, const double* u, double gravity, int64_t B, double* out, void* ws,
                     size_t ws_bytes, void* stream);

/* Forward-simulation rollout: T integration steps of forward dynamics in ONE launch (no counterpart in the reference; a
 * sampling controller's inner loop).  Fixed-base robots; a floating-base library returns RBD_ERR_UNSUPPORTED.
 * With qdd_t = aba(q_t, qd_t, u_t, gravity), the articulated-body sweeps of the aba entry point above, one step is
 *   integrator 0 (semi-implicit Euler): qd_{t+1} = qd_t + dt qdd_t, then q_{t+1} = q_t + dt qd_{t+1}
 *   integrator 1 (explicit Euler):      q_{t+1} = q_t + dt qd_t,         qd_{t+1} = qd_t + dt qdd_t
 * (each update one fused multiply-add).  No angle wrapping, joint limits, damping or external forces.
 *   q0, qd0       : [B, n] device, the state before step 0; never written
 *   u             : [T, B, n] device (u_shared == 0), or [T, n] (u_shared != 0): one sequence for every row
 *   q_out, qd_out : trajectory != 0: [T, B, n], slice t = the state AFTER step t + 1 (the initial state is not copied);
 *                   trajectory == 0: [B, n], the final state only -- nothing but that is written
 * Everything with a time axis is TIME-MAJOR: a step reads and writes one flat [B, n] tile, coalesced like every other
 * entry point's, and slice t of a trajectory is a dense [B, n] array that any entry point above takes as it is.
 * The state stays on chip for all T steps; a step reads n scalars and writes 2 n per row (0 without a trajectory).
 * Arguments are checked before anything touches the GPU: null pointer, B < 0, T < 0, dt not finite, unknown integrator,
 * B or B T n too large: RBD_ERR_ARG; a robot whose per-body state exceeds the LDS: RBD_ERR_UNSUPPORTED.  B == 0 or
 * T == 0 is a no-op (nothing is written, q_out does NOT receive q0). */
#define RBD_INTEGRATOR_SEMI_IMPLICIT 0
#define RBD_INTEGRATOR_EULER 1
int rbd_rollout_f32(const float* q0, const float* qd0, const float* u, int u_shared, float dt, float gravity, int integrator,
                    int64_t B, int64_t T, float* q_out, float* qd_out, int trajectory, void* stream);
int rbd_rollout_f64(const double* q0, const double* qd0, const double* u, int u_shared, double dt, double gravity,
                    int integrator, int64_t B, int64_t T, double* q_out, double* qd_out, int trajectory, void* stream);

/* Reverse-mode gradient of a rollout: for a scalar L of the returned slices, dL/du [T, B, n], dL/dq0 and dL/dqd0 [B, n]
 * from gq[t] = dL/dq[t] and gqd[t] = dL/dqd[t] (the direct partials; slice t is the state after step t + 1).  Fixed base
 * only; a floating-base library returns RBD_ERR_UNSUPPORTED.  With lam = (lq | lqd) = 0, for t = T-1 ... 0, at the
 * linearisation point (q_t, qd_t, u_t) -- (q0, qd0, u[0]) for t = 0, (q[t-1], qd[t-1], u[t]) after it:
 *   lq += gq[t];  lqd += gqd[t];  w = lqd + dt lq
 *   mu = dt w (integrator 0)  |  dt lqd (integrator 1);   nu = Minv(q_t) mu;   grad_u[t] = nu
 *   lq = lq - dc_dq^T nu;  lqd = w - dc_dqd^T nu     [dc_dq | dc_dqd] = rnea_grad at (q_t, qd_t, qdd_t), qdd_t = aba at (q_t, qd_t, u_t)
 * and grad_q0 = lq, grad_qd0 = lqd after t = 0.  Only vector-Jacobian products are formed: no -Minv dc_du.
 * PRISMATIC JOINTS: rbd_rnea_grad's dc_dq reproduces the reference and is not the q-derivative for prismatic joints,
 * and these gradients inherit that: they are the true gradient on robots with revolute joints only.
 *
 * rbd_rollout_adjoint: the scan alone, ONE launch that walks the time axis with lam on chip, for a caller that holds the
 * linearisation.  Per row and step it reads n 2n + n n + 2n scalars and writes n.
 *   dc_du [T, B, n, 2n], Minv [T, B, n, n] (dense, symmetric): step t's linearisation; T here is the number of steps
 *                 of THIS call
 *   gq, gqd     : g_final_only == 0: [T, B, n]; g_final_only != 0: [B, n], added at step T - 1 only (a terminal cost;
 *                 a caller that splits the time axis passes them to the call that holds the last step).  Either may be
 *                 NULL = zero
 *   lam         : [B, 2n], IN and OUT: the adjoint after step T (zeros at the end of the horizon) -> the adjoint after
 *                 step 0.  It is loaded and stored as it is, so a scan split at any step -- the later steps first, lam
 *                 carried through this buffer -- is bit-identical to the unsplit one
 *   grad_u      : [T, B, n]
 * rbd_rollout_grad: the composite.  q_traj, qd_traj [T, B, n] are rbd_rollout's trajectory (slice T - 1 is not read);
 * it zeroes lam and walks chunks of Tc steps from the end: rbd_aba, rbd_rnea_grad without damping and rbd_minv on the
 * chunk's Tc B flat rows (time-major: rows of steps 1 .. T-1 are contiguous in q_traj and u), then the scan; step 0 is
 * its own last chunk.  Tc is the largest chunk (at most T - 1, at least 1) whose rbd_rollout_grad_workspace_bytes(B, Tc,
 * elem_size) fits ws_bytes; rbd_rollout_grad_workspace_bytes(B, T, .) therefore always suffices.  The result does not
 * depend on Tc beyond the kernels rbd_rnea_grad / rbd_minv pick for a batch of Tc B rows.
 * Arguments are checked before anything touches the GPU: null required pointer, B < 0, T < 0, dt not finite, unknown
 * integrator, B T n 2n too large, misaligned lam / grad_u / grad_q0 / grad_qd0 / workspace: RBD_ERR_ARG; a workspace
 * that does not hold one step: RBD_ERR_WORKSPACE.  B == 0 or T == 0 is a no-op: nothing is written. */
int rbd_rollout_adjoint_f32(const float* dc_du, const float* Minv, const float* gq, const float* gqd, int g_final_only,
                            float dt, int integrator, int64_t B, int64_t T, float* lam, float* grad_u, void* stream);
int rbd_rollout_adjoint_f64(const double* dc_du, const double* Minv, const double* gq, const double* gqd, int g_final_only,
                            double dt, int integrator, int64_t B, int64_t T, double* lam, double* grad_u, void* stream);
size_t rbd_rollout_grad_workspace_bytes(int64_t B, int64_t Tc, int elem_size);
int rbd_rollout_grad_f32(const float* q0, const float* qd0, const float* u, const float* q_traj, const float* qd_traj,
                         const float* gq, const float* gqd, int g_final_only, float dt, float gravity, int integrator,
                         int64_t B, int64_t T, float* grad_u, float* grad_q0, float* grad_qd0, void* ws, size_t ws_bytes,
                         void* stream);
int rbd_rollout_grad_f64(const double* q0, const double* qd0, const double* u, const double* q_traj, const double* qd_traj,
                         const double* gq, const double* gqd, int g_final_only, double dt, double gravity, int integrator,
                         int64_t B, int64_t T, double* grad_u, double* grad_q0, double* grad_qd0, void* ws, size_t ws_bytes,
                         void* stream);

/* The backward pass of iLQR / DDP / time-varying LQR over a rollout: the Riccati recursion that turns the linearisation
 * dc_du, Minv of rbd_rollout's steps and a quadratic cost model (diagonal state and control Hessians, a full terminal
 * Hessian through P) into a feed-forward term k[t] [n] and feedback gains K[t] [n, 2n].  Fixed base only; a floating-base
 * library returns RBD_ERR_UNSUPPORTED.  Conventions are rbd_rollout_adjoint's: time-major, slice t is x_{t+1} = (q | qd),
 * state costs attach to slices and control costs to u[t].  With D = dc_du[t] and M = Minv[t] (symmetric):
 *   A0 = [[I, dt I], [0, I]];  b = [dt^2 I ; dt I] (integrator 0) | [0 ; dt I] (integrator 1);  Bm = b M;  A = A0 - Bm D
 * and, per row, carried lam [2n], P [2n, 2n], dV [2], status (int32), for t = T-1 ... 0:
 *   lam += (gq[t] | gqd[t]);  P += diag(hq[t] | hqd[t])
 *   Qx = A^T lam;  Qu = gu[t] + Bm^T lam;  Qxx = A^T P A;  Qux = Bm^T P A;  Quu = diag(hu[t]) + Bm^T P Bm
 *   Cholesky of Quu + reg I;  k[t] = -(Quu + reg I)^-1 Qu;  K[t] = -(Quu + reg I)^-1 Qux
 *   dV[0] += k^T Qu;  dV[1] += 1/2 k^T Quu k            (Quu without reg)
 *   lam = Qx + K^T Quu k + K^T Qu + Qux^T k;  P = Qxx + K^T Quu K + K^T Qux + Qux^T K;  P = 1/2 (P + P^T)
 * A pivot of the factorisation that is <= 0 or not finite: k[t] = 0 and K[t] = 0 are stored for that row and step,
 * status += 1, lam = Qx, P = Qxx, dV unchanged; no other row is affected.  dV[0] + dV[1] is the expected change of cost of
 * the closed-loop pass u = u + k + K dx.
 * PRISMATIC JOINTS: rbd_rnea_grad's dc_dq reproduces the reference and is not the q-derivative for prismatic joints, and
 * the gains of rbd_rollout_lqr inherit that: they belong to the true linearisation on robots with revolute joints only.
 *
 * rbd_rollout_riccati: the scan alone, ONE launch that walks the time axis with lam and P on chip and factors Quu on
 * chip, for a caller that holds the linearisation.  Per row and step it reads 3 n^2 + 6n scalars and writes 2 n^2 + n.
 *   dc_du [T, B, n, 2n], Minv [T, B, n, n] (dense, symmetric): step t's linearisation; T = the steps of THIS call
 *   gq, gqd, hq, hqd : x_final_only == 0: [T, B, n]; != 0: [B, n], added at step T - 1 only (a caller that splits the
 *                 time axis passes them to the call that holds the last step).  Any may be NULL = zero
 *   gu          : [T, B, n] or NULL = zero
 *   hu          : hu_shared == 0: [T, B, n]; != 0: [n], shared by every row and step.  Required
 *   reg         : finite, >= 0
 *   lam [B, 2n], P [B, 2n, 2n] (symmetric), dV [B, 2], status [B] (int32): IN and OUT, the value function after step T
 *                 (zeros, or a terminal Hessian in P) -> after step 0.  They are loaded and stored as they are and every
 *                 step runs the same instructions, so a scan split at any step -- the later steps first -- is
 *                 bit-identical to the unsplit one
 *   k [T, B, n], K [T, B, n, 2n]: OUT
 * rbd_rollout_lqr: the composite.  q_traj, qd_traj [T, B, n] are rbd_rollout's trajectory (slice T - 1 is not read); it
 * zeroes lam, P, dV and status (caller buffers) and walks chunks of Tc steps from the end exactly as rbd_rollout_grad
 * does: rbd_aba, rbd_rnea_grad without damping and rbd_minv on the chunk's Tc B flat rows, then the scan; step 0 at
 * (q0, qd0, u[0]) is its own last chunk.  Tc is the largest chunk (at most T - 1, at least 1) whose
 * rbd_rollout_lqr_workspace_bytes(B, Tc, elem_size) fits ws_bytes.
 * Arguments are checked before anything touches the GPU: null required pointer, B < 0, T < 0, dt or reg not finite,
 * reg < 0, unknown integrator, B T n 2n too large, misaligned lam / P / dV / status / k / K / workspace: RBD_ERR_ARG; a
 * workspace that does not hold one step: RBD_ERR_WORKSPACE; a robot whose step (8 n^2 scalars per row) does not fit 64 KiB
 * of LDS in this precision: RBD_ERR_UNSUPPORTED.  B == 0 or T == 0 is a no-op: nothing is written. */
int rbd_rollout_riccati_f32(const float* dc_du, const float* Minv, const float* gq, const float* gqd, const float* hq,
                            const float* hqd, int x_final_only, const float* gu, const float* hu, int hu_shared, float reg,
                            float dt, int integrator, int64_t B, int64_t T, float* lam, float* P, float* dV, int32_t* status,
                            float* k, float* K, void* stream);
int rbd_rollout_riccati_f64(const double* dc_du, const double* Minv, const double* gq, const double* gqd, const double* hq,
                            const double* hqd, int x_final_only, const double* gu, const double* hu, int hu_shared, double reg,
                            double dt, int integrator, int64_t B, int64_t T, double* lam, double* P, double* dV,
                            int32_t* status, double* k, double* K, void* stream);
size_t rbd_rollout_lqr_workspace_bytes(int64_t B, int64_t Tc, int elem_size);
int rbd_rollout_lqr_f32(const float* q0, const float* qd0, const float* u, const float* q_traj, const float* qd_traj,
                        const float* gq, const float* gqd, const float* hq, const float* hqd, int x_final_only,
                        const float* gu, const float* hu, int hu_shared, float reg, float dt, float gravity, int integrator,
                        int64_t B, int64_t T, float* k, float* K, float* lam, float* P, float* dV, int32_t* status, void* ws,
                        size_t ws_bytes, void* stream);
int rbd_rollout_lqr_f64(const double* q0, const double* qd0, const double* u, const double* q_traj, const double* qd_traj,
                        const double* gq, const double* gqd, const double* hq, const double* hqd, int x_final_only,
                        const double* gu, const double* hu, int hu_shared, double reg, double dt, double gravity,
                        int integrator, int64_t B, int64_t T, double* k, double* K, double* lam, double* P, double* dV,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* Closed-loop rollout: the forward pass that consumes the k, K of rbd_rollout_lqr -- an iLQR / DDP line search, a
 * time-varying LQR tracking controller, roll-outs from perturbed initial states around one feedback policy -- T steps in ONE
 * launch with the control law inside the time loop.  Fixed base only; a floating-base library returns RBD_ERR_UNSUPPORTED.
 * Integrators and conventions are rbd_rollout's.  Write x = (q | qd).  The state at which u[t] acts is x_t: x_0 = (q0, qd0),
 * x_t = slice t - 1 of the trajectory for t >= 1; the reference state xref_t follows the same rule with (q0_ref, qd0_ref) and
 * (q_ref, qd_ref).  Per row and step:
 *   dx  = x_t - xref_t
 *   u_t = u[t] + alpha k[t] + K[t] dx          (K[t] is n x 2n; one chain of fused multiply-adds per joint, in that order)
 *   u_t = u_t < u_lo ? u_lo : (u_t > u_hi ? u_hi : u_t)      per joint, when limits are given; a NaN stays a NaN
 *   qdd = aba(q_t, qd_t, u_t, gravity), then the integrator's two fused multiply-adds
 * SHARED NOMINAL: the rollout has B rows, the nominal B_nom rows, B a multiple of B_nom; row r reads row r % B_nom of u, k, K,
 * q0_ref, qd0_ref, q_ref, qd_ref and its own q0[r], qd0[r], alpha[r].  B_nom == B is the plain case; a line search over A
 * step sizes is B = A B_nom; many starts around one policy is B_nom = 1.  A row's arithmetic does not depend on B_nom: a
 * shared launch is bit-identical to the unshared one on the tiled nominal.
 *   q0, qd0            : [B, n] device, the state before step 0; never written
 *   u, k, K            : [T, B_nom, n], [T, B_nom, n] or NULL (no feed-forward term), [T, B_nom, n, 2n]
 *   q0_ref, qd0_ref    : [B_nom, n]
 *   q_ref, qd_ref      : [T, B_nom, n], what rbd_rollout returned for the nominal; slice T - 1 is never read
 *   alpha              : [B] device; NULL exactly when k is NULL
 *   u_lo, u_hi         : [n] device, or both NULL (no limits)
 *   q_out, qd_out      : trajectory != 0: [T, B, n], slice t = the state after step t + 1; trajectory == 0: [B, n], the final
 *                        state only
 *   u_out              : [T, B, n], the controls actually applied, or NULL
 * Per row and step it reads 2 n^2 + 4n scalars (the 2 n^2 of K shared by the rows of one nominal row) and writes up to 3n.
 * Arguments are checked before anything touches the GPU: null required pointer, k xor alpha null, u_lo xor u_hi null, B < 0,
 * T < 0, B > 0 with B_nom <= 0 or B not a multiple of B_nom, dt not finite, unknown integrator, misaligned output, B or
 * B T n or B_nom T n 2n too large: RBD_ERR_ARG; a robot whose state (17 scalars per body and row) exceeds the LDS:
 * RBD_ERR_UNSUPPORTED.  B == 0 or T == 0 is a no-op: nothing is written. */
int rbd_rollout_closed_loop_f32(const float* q0, const float* qd0, const float* u, const float* k, const float* K,
                                const float* q0_ref, const float* qd0_ref, const float* q_ref, const float* qd_ref,
                                const float* alpha, const float* u_lo, const float* u_hi, float dt, float gravity,
                                int integrator, int64_t B, int64_t B_nom, int64_t T, float* q_out, float* qd_out,
                                int trajectory, float* u_out, void* stream);
int rbd_rollout_closed_loop_f64(const double* q0, const double* qd0, const double* u, const double* k, const double* K,
                                const double* q0_ref, const double* qd0_ref, const double* q_ref, const double* qd_ref,
                                const double* alpha, const double* u_lo, const double* u_hi, double dt, double gravity,
                                int integrator, int64_t B, int64_t B_nom, int64_t T, double* q_out, double* qd_out,
                                int trajectory, double* u_out, void* stream);

/* Rollout with its cost: rbd_rollout_closed_loop's time loop, open or closed loop, with a quadratic tracking cost accumulated
 * inside it -- the line search of iLQR / DDP, the sample costs of a sampling controller -- in ONE launch that writes cost [B]
 * and nothing else unless asked.  Fixed base only; a floating-base library returns RBD_ERR_UNSUPPORTED.  Conventions, the
 * shared nominal (row r reads row r % B_nom) and the integrators are rbd_rollout_closed_loop's.  Per row and step:
 *   u_t = u[t] + alpha k[t], then + du[t], then + K[t] dx (the 2n products in order), then the limits
 *         (one chain per joint; k, du, K and the limits are each optional; K == NULL is an OPEN loop and the four reference
 *         pointers are not read)
 *   qdd = aba(q_t, qd_t, u_t, gravity), then the integrator's two fused multiply-adds
 *   J  += sum_j 1/2 w_u[t,j] u_t,j^2 + c_u[t,j] u_t,j                                    (u_t: the control applied, after limits)
 *       + sum_j 1/2 w_q[t,j] (q_{t+1,j} - q_tgt[t,j])^2 + sum_j 1/2 w_qd[t,j] (qd_{t+1,j} - qd_tgt[t,j])^2
 * J is ONE chain per row in a fixed order, in the kernel's precision: for t = 0 .. T - 1 the control terms j = 0 .. n - 1 (per
 * joint fma((w_u / 2 * u), u, J), then fma(c_u, u, J)), then the q terms j = 0 .. n - 1 (d = q - q_tgt; fma((w_q / 2 * d), d, J)),
 * then the qd terms.  A row's J depends on that row's values alone: not on B, B_nom, its lane or block, nor on which optional
 * outputs are stored.
 *   q0, qd0            : [B, n] device; never written
 *   u                  : [T, B_nom, n]
 *   k, alpha           : [T, B_nom, n] and [B], or both NULL
 *   K                  : [T, B_nom, n, 2n], or NULL (open loop)
 *   q0_ref, qd0_ref, q_ref, qd_ref : as rbd_rollout_closed_loop; required when K is given, ignored otherwise
 *   du                 : [T, B, n], a perturbation of the control per ROW, or NULL
 *   u_lo, u_hi         : [n] device, or both NULL
 *   q_tgt, qd_tgt, w_q, w_qd : x_final_only == 0: [T, B_nom, n]; x_final_only != 0: [B_nom, n], a cost on slice T - 1 alone.
 *                        Any may be NULL: a NULL weight drops its term, a NULL target is zero
 *   w_u, c_u           : [T, B_nom, n]; a NULL w_u drops the quadratic term, a NULL c_u the linear one
 *   cost               : [B], always written
 *   q_out, qd_out      : both or neither; trajectory != 0: [T, B, n]; trajectory == 0: [B, n], the final state.  NULL: not stored
 *   u_out              : [T, B, n], the controls applied, or NULL
 * Arguments are checked before anything touches the GPU: NULL q0, qd0, u or cost, K with a NULL reference pointer, k xor alpha
 * NULL, u_lo xor u_hi NULL, q_out xor qd_out NULL, B < 0, T < 0, B > 0 with B_nom <= 0 or B not a multiple of B_nom, dt not
 * finite, unknown integrator, misaligned output, B or B T n or B_nom T n 2n too large: RBD_ERR_ARG; a robot whose state exceeds
 * the LDS: RBD_ERR_UNSUPPORTED.  B == 0 or T == 0 is a no-op: nothing is written. */
int rbd_rollout_cost_f32(const float* q0, const float* qd0, const float* u, const float* k, const float* K,
                         const float* q0_ref, const float* qd0_ref, const float* q_ref, const float* qd_ref,
                         const float* alpha, const float* du, const float* u_lo, const float* u_hi, const float* q_tgt,
                         const float* qd_tgt, const float* w_q, const float* w_qd, int x_final_only, const float* w_u,
                         const float* c_u, float dt, float gravity, int integrator, int64_t B, int64_t B_nom, int64_t T,
                         float* cost, float* q_out, float* qd_out, int trajectory, float* u_out, void* stream);
int rbd_rollout_cost_f64(const double* q0, const double* qd0, const double* u, const double* k, const double* K,
                         const double* q0_ref, const double* qd0_ref, const double* q_ref, const double* qd_ref,
                         const double* alpha, const double* du, const double* u_lo, const double* u_hi, const double* q_tgt,
                         const double* qd_tgt, const double* w_q, const double* w_qd, int x_final_only, const double* w_u,
                         const double* c_u, double dt, double gravity, int integrator, int64_t B, int64_t B_nom, int64_t T,
                         double* cost, double* q_out, double* qd_out, int trajectory, double* u_out, void* stream);

/* The update of a sampling controller (MPPI) from the sample costs rbd_rollout_cost wrote: softmin weights and the weighted sum
 * of the perturbations, du read once.  P independent problems (rbd_rollout_cost's B_nom rows), S samples each, in its row
 * layout: row s P + p is sample s of problem p.  Fixed base only; a floating-base library returns RBD_ERR_UNSUPPORTED.  Per
 * problem p, in the entry point's precision:
 *   Jm  = min_s J[s,p]                                      (a NaN counts as +inf)
 *   x_s = (J[s,p] - Jm) / lam[p];  e_s = exp(-x_s)          (1 at a minimum, 0 for a NaN or +inf sample)
 *   eta = sum_s e_s;  w_s = e_s / eta;  ess = eta^2 / sum_s e_s^2
 *   d_s[t,j] = du[t,s,p,j], or with limits clamp(u[t,p,j] + du[t,s,p,j], u_lo[j], u_hi[j]) - u[t,p,j]  (what rbd_rollout_cost
 *              applied: u < lo ? lo : (u > hi ? hi : u))
 *   u_out[t,p,j] = u[t,p,j] + (sum_s e_s d_s[t,j]) / eta, clamped once more when limits are given
 *   status[p] = 2: lam[p] is not finite and positive; else 1: Jm is not finite (every sample NaN or +inf, or a -inf among
 *               them); else 0.  Where it is not 0: u_out[:,p] = u[:,p] (clamped when limits are given), w = 0, ess = 0.
 * Nothing else is special: a NaN in du poisons the (t, j) outputs of its own problem and no other.
 * Summation order -- a function of S and RBD_MPPI_CHUNK alone, not of P, T or the optional outputs; no floating-point atomics.
 * Each of eta, sum e^2 and sum e d[t,j]: per chunk of RBD_MPPI_CHUNK consecutive samples one chain from zero in ascending s
 * (a += e; a = fma(e, e, a); a = fma(e, d, a)); then per group of RBD_MPPI_CHUNK consecutive chunks the chunks added in
 * ascending order; then the groups added in ascending order.
 *   J                  : [S, P] device; never written (as every input)
 *   du                 : [T, S, P, n]
 *   u                  : [T, P, n]
 *   lam                : [P]
 *   u_lo, u_hi         : [n] device, or both NULL
 *   u_out              : [T, P, n]
 *   w_out              : [S, P], or NULL
 *   ess_out            : [P], or NULL
 *   status_out         : [P] int32
 *   ws, ws_bytes       : device scratch of at least rbd_mppi_update_workspace_bytes bytes (S, P, T, 4 or 8): e [S, P], eta [P]
 *                        and, when S > RBD_MPPI_CHUNK, the chunk partials [ceil(S / RBD_MPPI_CHUNK), T, P, n].  The query
 *                        returns 0 for a size that is not positive or too large, and on a floating-base library
 * Arguments are checked before anything touches the GPU: NULL J, du, u, lam, u_out or status_out, u_lo xor u_hi NULL, S, P or
 * T < 0, S P or T S P n too large, misaligned output or workspace: RBD_ERR_ARG; a workspace that is missing or too small:
 * RBD_ERR_WORKSPACE.  S == 0, P == 0 or T == 0 is a no-op: nothing is written. */
#define RBD_MPPI_CHUNK 64
size_t rbd_mppi_update_workspace_bytes(int64_t S, int64_t P, int64_t T, int elem_size);
int rbd_mppi_update_f32(const float* J, const float* du, const float* u, const float* lam, const float* u_lo, const float* u_hi,
                        int64_t S, int64_t P, int64_t T, float* u_out, float* w_out, float* ess_out, int32_t* status_out,
                        void* ws, size_t ws_bytes, void* stream);
int rbd_mppi_update_f64(const double* J, const double* du, const double* u, const double* lam, const double* u_lo,
                        const double* u_hi, int64_t S, int64_t P, int64_t T, double* u_out, double* w_out, double* ess_out,
                        int32_t* status_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RBD_HIP_H */
