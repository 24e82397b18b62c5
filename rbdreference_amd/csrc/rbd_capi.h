// rbd_capi.h -- the host half of a fixed-base robot's library: the C-ABI of include/rbd_hip.h over the kernels of
// rbd_kernels.hip, which includes this file last.  Per family of entry points: ONE selection function (the only place that
// reads the options and the compile-time *_ok / *_built predicates; the launcher switches on what it returns, and
// rbd_kernel_name / rbd_minv_workspace_bytes ask the same function), the launchers (argument checks, then rbd_host.h's
// launch path) and one RBD_DEFS_<FAMILY>(SFX, T) macro with the extern "C" wrappers of a precision.  Every section sits
// under the RBD_NEED_* / RBD_TU_* guard of its unit, so a unit's preprocessed text holds its own family's host code only.
#pragma once
#include "rbd_host.h"
#include <cstdlib>
#include <cstring>

// ---- owned by the COMMON unit ---------------------------------------------------------------------------------------------
#ifdef RBD_TU_COMMON
extern "C" char* rbd_err_buf(void) {
  static thread_local char buf[RBD_ERR_LEN] = "";
  return buf;
}
extern "C" std::atomic<int>* rbd_option_slot(int option) {
  static std::atomic<int> slots[RBD_OPT_COUNT_];
  return option >= 0 && option < RBD_OPT_COUNT_ ? &slots[option] : nullptr;
}
#include "rbd_ws_pool.h"
#endif

// ---- calls across translation units ---------------------------------------------------------------------------------------
// The forward-dynamics units reuse the kernels of the RNEA / MINV / GRAD units through their entry points instead of
// instantiating the same templates a second time (Atlas: the fp64 gradient kernel alone costs 200 s of compile time), and
// the qdd = None gradient kernels live in the GRADN units.  rbd_minv_fd_* = rbd_minv_* plus the fused qdd = Minv (u - c).
// Callers are templates over T: they use the overloads, which pick the precision's symbol.
#define RBD_CROSS_UNIT(SFX, T)                                                                                                   \
  extern "C" {                                                                                                                   \
  __attribute__((visibility("hidden"))) int rbd_grad_noqdd_##SFX(const T* q, const T* qd, T gravity, int use_damping, int64_t B, \
                                                                 T* c, T* dc_du, void* stream);                                  \
  __attribute__((visibility("hidden"))) int rbd_grad_cols_noqdd_##SFX(const T* q, const T* qd, T gravity, int use_damping,       \
                                                                      int64_t B, T* c, T* v, T* a, T* f, T* dc_du, void* stream); \
  __attribute__((visibility("hidden"))) int rbd_minv_fd_##SFX(const T* q, int64_t B, T* Minv, void* workspace, size_t wsb,       \
                                                              void* stream, const T* u, const T* c, T* qdd, const T* qd, T gravity); \
  }                                                                                                                              \
  namespace {                                                                                                                    \
  inline int rbd_rnea(const T* q, const T* qd, const T* qdd, T g, int64_t B, T* c, T* v, T* a, T* f, void* s) {                  \
    return rbd_rnea_##SFX(q, qd, qdd, g, B, c, v, a, f, s);                                                                      \
  }                                                                                                                              \
  inline int rbd_rnea_grad(const T* q, const T* qd, const T* qdd, T g, int damping, int64_t B, T* c, T* dc_du, void* s) {        \
    return rbd_rnea_grad_##SFX(q, qd, qdd, g, damping, B, c, dc_du, s);                                                          \
  }                                                                                                                              \
  inline int rbd_grad_noqdd(const T* q, const T* qd, T g, int damping, int64_t B, T* c, T* dc_du, void* s) {                     \
    return rbd_grad_noqdd_##SFX(q, qd, g, damping, B, c, dc_du, s);                                                              \
  }                                                                                                                              \
  inline int rbd_grad_cols_noqdd(const T* q, const T* qd, T g, int damping, int64_t B, T* c, T* v, T* a, T* f, T* dc_du, void* s) { \
    return rbd_grad_cols_noqdd_##SFX(q, qd, g, damping, B, c, v, a, f, dc_du, s);                                                \
  }                                                                                                                              \
  inline int rbd_minv(const T* q, int64_t B, int dense, T* Minv, void* ws, size_t wsb, void* s) {                                \
    return rbd_minv_##SFX(q, B, dense, Minv, ws, wsb, s);                                                                        \
  }                                                                                                                              \
  inline int rbd_minv_fd(const T* q, int64_t B, T* Minv, void* ws, size_t wsb, void* s, const T* u, const T* c, T* qdd,          \
                         const T* qd, T g) {                                                                                     \
    return rbd_minv_fd_##SFX(q, B, Minv, ws, wsb, s, u, c, qdd, qd, g);                                                          \
  }                                                                                                                              \
  inline int rbd_forward_dynamics_grad(const T* q, const T* qd, const T* u, T g, int64_t B, T* qdd, T* dqdd_du, void* ws,        \
                                       size_t wsb, void* s) {                                                                    \
    return rbd_forward_dynamics_grad_##SFX(q, qd, u, g, B, qdd, dqdd_du, ws, wsb, s);                                            \
  }                                                                                                                              \
  inline int rbd_second_order_idsva(const T* q, const T* qd, const T* qdd, T g, int64_t B, T* out, void* s) {                    \
    return rbd_second_order_idsva_##SFX(q, qd, qdd, g, B, out, s);                                                               \
  }                                                                                                                              \
  }
RBD_CROSS_UNIT(f32, float)
RBD_CROSS_UNIT(f64, double)
#undef RBD_CROSS_UNIT

namespace {
// =============================================================================================
// rnea
// =============================================================================================
#ifdef RBD_NEED_RNEA
// one wave per segment (stem / limb / limb-less group: Atlas fp32 B = 16 384), one wave per independent root group (faster
// than one lane per configuration at every batch size measured -- Atlas fp32: 17.4 -> 13.5 us at B = 16 384, 235 -> 167 us
// at B = 262 144; quadruped fp32 B = 1M: 199 -> 174 us = 6.4 TB/s), or one lane per configuration
enum class RneaKind { LANE, GROUPS, SEGMENTS };
template <class T>
constexpr bool rnea_groups_built() {   // (first-use build: not next to the segment kernel AUTO picks)
  return rbdk::rnea_groups_ok<T>() && !(RBD_FAST_STAGE && rbdk::rnea_segs_ok<T>());
}
// the wave kernels serve rbd_rnea with v, a, f only: c alone and rnea_fpass are always the one-lane kernel
template <class T>
RneaKind rnea_select(bool vaf, bool fpass_only) {
  if (!vaf || fpass_only) return RneaKind::LANE;
  const int opt = rbd_option(RBD_OPT_RNEA_KERNEL);
  if constexpr (rbdk::rnea_segs_ok<T>()) {
    if (opt != RBD_RNEA_KERNEL_BATCH && opt != RBD_RNEA_KERNEL_GROUPS) return RneaKind::SEGMENTS;
  }
  if constexpr (rnea_groups_built<T>()) {
    if (opt != RBD_RNEA_KERNEL_BATCH) return RneaKind::GROUPS;
  }
  return RneaKind::LANE;
}

template <class T>
int rnea_launch(const T* q, const T* qd, const T* qdd, T gravity, int64_t B, T* c, T* v, T* a, T* f,
                void* stream, int fpass_only = 0) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_rnea: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || (!c && !fpass_only)) return fail(RBD_ERR_ARG, "rbd_rnea: q, qd and c must be non-null");
  if (fpass_only && !(v && a && f)) return fail(RBD_ERR_ARG, "rbd_rnea_fpass: v, a, f must be non-null");
  const bool vaf = v || a || f;
  if (vaf && !(v && a && f)) return fail(RBD_ERR_ARG, "rbd_rnea: v, a, f must be all null or all non-null");
  if (misaligned(c, v, a, f)) return fail(RBD_ERR_ARG, "rbd_rnea: output buffers must be 16-byte aligned");
  unsigned grid;
  if (int rc = grid_for(B, 64, "rbd_rnea", &grid)) return rc;
  const bool has_qdd = qdd != nullptr;
  switch (rnea_select<T>(vaf, fpass_only != 0)) {
    case RneaKind::SEGMENTS:
      if constexpr (rnea_segs_ok<T>())
        return with_bool(has_qdd, [&](auto HQ) {
          return launch("rbd_rnea (segment waves) launch", rnea_segments_kernel<T, decltype(HQ)::value>, grid, 64 * RS_WAVES, rnea_segs_lds<T>(),
                        stream, q, qd, qdd, gravity, B, c, v, a, f);
        });
      break;
    case RneaKind::GROUPS:
      if constexpr (rnea_groups_built<T>())
        return with_bool(has_qdd, [&](auto HQ) {
          return launch("rbd_rnea (group waves) launch", rnea_groups_kernel<T, decltype(HQ)::value>, grid, 64 * RG_WAVES,
                        2 * sizeof(T) * 64 * (size_t)odd_pad<6 * N>(), stream, q, qd, qdd, gravity, B, c, v, a, f);
        });
      break;
    case RneaKind::LANE:
      break;
  }
  return with_bool(has_qdd, [&](auto HQ) {
    return with_bool(vaf, [&](auto VAF) {
      constexpr bool with_vaf = decltype(VAF)::value;
      return launch("rbd_rnea launch", rnea_kernel<T, decltype(HQ)::value, with_vaf>, grid, 64, rnea_lds_bytes<T>(with_vaf), stream,
                    q, qd, qdd, gravity, B, c, v, a, f, fpass_only);
    });
  });
}

template <class T>
int rnea_bpass_launch(const T* q, T* f, int64_t B, T* c, void* stream) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_rnea_bpass: B < 0");
  if (B == 0) return 0;
  if (!q || !f || !c) return fail(RBD_ERR_ARG, "rbd_rnea_bpass: q, f and c must be non-null");
  unsigned grid;
  if (int rc = grid_for(B, 64, "rbd_rnea_bpass", &grid)) return rc;
  return launch("rbd_rnea_bpass launch", rnea_bpass_kernel<T>, grid, 64, sizeof(T) * 64 * (size_t)odd_pad<6 * N>(), stream, q, f, B, c);
}

// RBD_OP_RNEA names the kernel rbd_rnea launches when v, a, f are requested
template <class T>
int rnea_kernel_name(int64_t, char* buf, size_t len) {
  const RneaKind k = rnea_select<T>(true, false);
  std::snprintf(buf, len, "%s<%s>", k == RneaKind::SEGMENTS ? "rnea_segments_kernel" : k == RneaKind::GROUPS ? "rnea_groups_kernel" : "rnea_kernel",
                type_name<T>());
  return 0;
}
#endif  // RBD_NEED_RNEA

// =============================================================================================
// rnea_grad
// =============================================================================================
#ifdef RBD_NEED_GRAD
// What is built for (robot, T):
//   cols      one lane per (configuration, derivative column) (rbd_grad_cols.h), for small batches
//   tree_ws   fp64 trees on the workspace kernel (rbd_idsva_tree_ws.h).  Default where the fp32 default is the tree kernel
//             (Atlas: the two-lane kernel spilled 388 registers there and is no longer built in fp64); with
//             RBD_OPT_GRAD_KERNEL = TREE for every other fp64 robot whose root path does not fit the register plan
//   tree      rbd_idsva_tree.h; in fp64 the root path's S / psid / psidd (36 registers per body) must fit 512 VGPRs without
//             scratch.  fp32 robots whose default it is build nothing else (Atlas: 404 VGPRs of code nobody runs)
//   chain     one lane per configuration, tile-walking blocks (rbd_idsva.h); one chain in fp32: the software-pipelined
//             tile loop (rbd_idsva_pipe.h)
//   two-lane  rnea_grad_kernel, where neither the chain kernel nor a tree kernel is the default
enum class GradKind { COLS, TREE_WS, TREE, CHAIN_PIPE, CHAIN, TWO_LANE };
template <class T>
constexpr bool grad_cols_built() { return !RBD_FAST_STAGE && rbdk::grad_cols_ok<T>(); }
template <class T>
constexpr bool tws_built() {
#ifndef RBD_HAVE_TWS
  return false;
#elif defined(RBD_TWS_FORCE)                                  // experiments: the workspace kernel for every eligible robot
  return rbdk::tws_ok<T>();
#else
  constexpr bool reg_plan = rbdk::N <= 12 && rbdm::MAXDEPTH <= 5;   // served by rnea_grad_tree_kernel<double>
  if constexpr (!rbdk::tws_ok<T>() || reg_plan) return false;
  else return rbdk::GRAD_TREE_DEFAULT || !RBD_FAST_STAGE;
#endif
}
template <class T>
constexpr bool tws_only() {
#ifdef RBD_TWS_FORCE
  return tws_built<T>();
#else
  return tws_built<T>() && rbdk::GRAD_TREE_DEFAULT;
#endif
}
template <class T>
constexpr bool grad_tree_only() { return rbdk::GRAD_TREE_DEFAULT && sizeof(T) == 4; }
template <class T>
constexpr bool grad_tree_built() {
  return RBD_FAST_STAGE ? grad_tree_only<T>() : rbdk::GRAD_TREE_OK && (sizeof(T) == 4 || (rbdk::N <= 12 && rbdm::MAXDEPTH <= 5));
}
template <class T>
constexpr bool grad_chain_built() { return !grad_tree_only<T>() && !tws_only<T>() && rbdk::grad_chain_kernel<T>(); }
template <class T>
constexpr bool grad_chain_pipe() { return rbdk::IDS_PIPE_OK && sizeof(T) == 4; }
template <class T>
constexpr bool grad_two_lane_built() { return !grad_tree_only<T>() && !tws_only<T>() && !rbdk::grad_chain_kernel<T>(); }

// the column kernel while the batch-parallel kernels would leave most of the chip idle: at most two of its waves per SIMD
constexpr int64_t GRAD_COLS_MAX_WAVES = 2048;
template <class T>
GradKind grad_select(int64_t B) {
  using namespace rbdk;
  const int opt = rbd_option(RBD_OPT_GRAD_KERNEL);
  if constexpr (grad_cols_built<T>()) {
    if (opt == RBD_GRAD_KERNEL_COLS) return GradKind::COLS;
    if (opt == RBD_GRAD_KERNEL_AUTO && (rbd_select_batch(B) + GC_CPW - 1) / GC_CPW <= GRAD_COLS_MAX_WAVES) return GradKind::COLS;
  }
  if constexpr (tws_built<T>()) {
    if (tws_only<T>() || opt == RBD_GRAD_KERNEL_TREE) return GradKind::TREE_WS;
  }
  if constexpr (grad_tree_built<T>()) {
    static_assert(!grad_tree_only<T>() || tree_lds_bytes<T>() <= LDS_MAX, "tree kernel is the only gradient kernel of this robot but does not fit LDS");
    if (grad_tree_only<T>() || (opt == RBD_GRAD_KERNEL_TREE && tree_lds_bytes<T>() <= LDS_MAX)) return GradKind::TREE;
  }
  if constexpr (grad_chain_built<T>()) return grad_chain_pipe<T>() ? GradKind::CHAIN_PIPE : GradKind::CHAIN;
  return GradKind::TWO_LANE;      // (never reached where a tree kernel is the only one: returned above)
}

template <class T, bool HAS_QDD, bool FDG>
int two_lane_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                    T* c, T* dc_du, void* stream, const T* minv_in) {
  using namespace rbdk;
  constexpr int CFGS = grad_cfgs<T>();
  unsigned blocks, grid;
  if (int rc = grid_for(B, CFGS, "rbd_rnea_grad", &blocks)) return rc;
  if (misaligned(dc_du)) return fail(RBD_ERR_ARG, "rbd_rnea_grad: dc_du must be 16-byte aligned");
  // independent root subtrees get their own blocks -- also with the fused -Minv epilogue (round 4): Minv and dc_du are
  // block-diagonal over the groups, so a group's block stages that group's Minv rows only (the quadruped's fp64
  // forward_dynamics_grad gradient leg: 151 us with every leg in one block, serial; 55 -> 28 KB of Minv tile, i.e. five
  // 64-thread blocks per CU instead of two)
  constexpr int split = (GRAD_PER_ROOT && n_groups() > 1) ? n_groups() : 1;
  const size_t lds = sizeof(T) * ((size_t)CFGS * GRAD_TS + (FDG ? (size_t)CFGS * (split > 1 ? (size_t)((grad_max_rows() * N) | 1) : (size_t)(N * N)) : 0));
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "rbd_rnea_grad: output tile does not fit LDS for this robot size");
  // whole XCD rounds (the kernel's block -> (configurations, group) map)
  if (int rc = checked_grid(split > 1 ? ((int64_t)blocks + 7) / 8 * 8 * split : blocks, "rbd_rnea_grad", &grid)) return rc;
  return launch("rbd_rnea_grad launch", rnea_grad_kernel<T, HAS_QDD, FDG>, grid, 2 * CFGS, lds, stream, q, qd, qdd, gravity,
                use_damping, B, c, dc_du, minv_in, split);
}

// The chain kernels, for rnea_grad (FDG = false) and for forward_dynamics_grad's -Minv epilogue (FDG = true, minv_in).
// Their flag word: damping, and the store policy of this launch (rbd_host.h: decided from the bytes the launch writes --
// dc_du, and c where it is asked for).
template <class T, bool HAS_QDD, bool FDG>
int chain_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                 T* c, T* dc_du, void* stream, const T* minv_in) {
  using namespace rbdk;
  unsigned tiles;
  if (int rc = grid_for(B, 64, "rbd_rnea_grad", &tiles)) return rc;
  if (misaligned(dc_du)) return fail(RBD_ERR_ARG, "rbd_rnea_grad: dc_du must be 16-byte aligned");
  const size_t lds = sizeof(T) * (size_t)64 * IDS_TS;
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "rbd_rnea_grad: output tile does not fit LDS for this robot size");
  const size_t out_bytes = (size_t)B * (size_t)(GRAD_TILE + (c ? N : 0)) * sizeof(T);
  const int flags = (use_damping ? RBD_KF_DAMPING : 0) | (rbd_store_flavour(rbd_option(RBD_OPT_STORE_POLICY), out_bytes) << RBD_KF_STORE_SHIFT);
  auto walk_tiles = [&](auto kernel) {      // the blocks that are resident at once walk the tiles
    int rc, resident = 0;
    if ((rc = ensure_lds(kernel, lds)) != 0) return rc;
    if ((rc = resident_blocks(kernel, 64, lds, &resident)) != 0) return rc;
    return launch("rbd_rnea_grad launch", kernel, tiles < (unsigned)resident ? tiles : (unsigned)resident, 64, lds, stream,
                  q, qd, qdd, gravity, flags, B, c, dc_du, minv_in);
  };
  // (the plain kernel is not even instantiated where the pipelined one serves the robot)
  if constexpr (grad_chain_pipe<T>()) return walk_tiles(rnea_grad_idsva_pipe_kernel<T, HAS_QDD, FDG>);
  else return walk_tiles(rnea_grad_idsva_kernel<T, HAS_QDD, FDG>);
}

template <class T, bool HAS_QDD>
int grad_cols_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                     T* c, T* v, T* a, T* f, T* dc_du, void* stream) {
  using namespace rbdk;
  if constexpr (!grad_cols_built<T>()) {
    return fail(RBD_ERR_UNSUPPORTED, "rbd_rnea_grad: the column kernel is not built for this robot size");
  } else {
    unsigned grid;
    if (int rc = grid_for(B, GC_CPW, "rbd_rnea_grad", &grid)) return rc;
    return launch("rbd_rnea_grad (column kernel) launch", rnea_grad_cols_kernel<T, HAS_QDD>, grid, 64, 0, stream, q, qd, qdd,
                  gravity, use_damping, B, c, v, a, f, dc_du);
  }
}

template <class T, bool HAS_QDD>
int tree_ws_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B, T* c, T* dc_du, void* stream) {
  using namespace rbdk;
#ifdef RBD_HAVE_TWS      // (fp64 units: the others never see rbd_idsva_tree_ws.h)
  if constexpr (tws_built<T>()) {
    constexpr size_t lds = tws_lds_bytes<T>();
    auto k = rnea_grad_tree_ws_kernel<T, HAS_QDD>;
    int rc, resident = 0;
    if ((rc = ensure_lds(k, lds)) != 0) return rc;
    if ((rc = resident_blocks(k, 64 * TWS_W, lds, &resident)) != 0) return rc;
    const int yroots = TWS_MULTI ? 1 : tree_n_roots();
    // one launch covers what is resident at once; larger batches walk the same workspace chunk by chunk.  The workspace
    // is sized by what is resident at once (never by B), one region per (x, root) block of the single-wave layout: a
    // (device, stream) sees ONE allocation for this kernel, whatever batch sizes follow (rbd_stream_workspace)
    const int64_t xres = resident / yroots > 0 ? resident / yroots : 1, need = (B + 63) / 64;
    const int64_t rows = (xres < need ? xres : need) * 64;
    void* ws = nullptr;
    if ((rc = rbd_stream_workspace(stream, (size_t)xres * 64 * yroots * TWS_SLOTS * sizeof(T), &ws)) != 0) return rc;
    T* pws = reinterpret_cast<T*>(ws);
    T* ews = pws + (size_t)64 * TWS_PATH_SLOTS;   // [block][slot][lane]: a block's entry slots follow its path slots
    for (int64_t r0 = 0; r0 < B; r0 += rows) {
      const int64_t nb = B - r0 < rows ? B - r0 : rows;
      rc = launch("rbd_rnea_grad (workspace tree kernel) launch", k, dim3((unsigned)((nb + 63) / 64), yroots), 64 * TWS_W, lds, stream,
                  q + r0 * N, qd + r0 * N, qdd ? qdd + r0 * N : nullptr, gravity, use_damping, nb, c ? c + r0 * N : nullptr,
                  dc_du + r0 * (2 * N * N), pws, ews);
      if (rc != 0) return rc;
    }
    return 0;
  }
#endif
  return fail(RBD_ERR_UNSUPPORTED, "rbd_rnea_grad: the workspace tree kernel is not built for this robot");
}

// One instantiation per (T, HAS_QDD): the forward-dynamics units only ever need HAS_QDD = true.  A kind's branch is
// compiled where that kind is built, so no kernel is instantiated that grad_select never returns.
template <class T, bool HAS_QDD>
int rnea_grad_launch_q(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                       T* c, T* dc_du, void* stream) {
  using namespace rbdk;
  switch (grad_select<T>(B)) {
    case GradKind::COLS:
      return grad_cols_launch<T, HAS_QDD>(q, qd, qdd, gravity, use_damping, B, c, nullptr, nullptr, nullptr, dc_du, stream);
    case GradKind::TREE_WS:
      return tree_ws_launch<T, HAS_QDD>(q, qd, qdd, gravity, use_damping, B, c, dc_du, stream);
    case GradKind::TREE:
      if constexpr (grad_tree_built<T>()) {
        unsigned grid;
        if (int rc = grid_for(B, 64, "rbd_rnea_grad", &grid)) return rc;
        return launch("rbd_rnea_grad (tree kernel) launch", rnea_grad_tree_kernel<T, HAS_QDD>, dim3(grid, TREE_MULTI ? 1 : tree_n_roots()),
                      64 * TREE_W, tree_lds_bytes<T>(), stream, q, qd, qdd, gravity, use_damping, B, c, dc_du);
      }
      break;
    case GradKind::CHAIN_PIPE:
    case GradKind::CHAIN:
      if constexpr (grad_chain_built<T>()) return chain_launch<T, HAS_QDD, false>(q, qd, qdd, gravity, use_damping, B, c, dc_du, stream, nullptr);
      break;
    case GradKind::TWO_LANE:
      if constexpr (grad_two_lane_built<T>()) return two_lane_launch<T, HAS_QDD, false>(q, qd, qdd, gravity, use_damping, B, c, dc_du, stream, nullptr);
      break;
  }
  return fail(RBD_ERR_UNSUPPORTED, "rbd_rnea_grad: no kernel");   // unreachable: grad_select returns built kinds only
}

template <class T>
int rnea_grad_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                     T* c, T* dc_du, void* stream) {
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_rnea_grad: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !dc_du) return fail(RBD_ERR_ARG, "rbd_rnea_grad: q, qd and dc_du must be non-null");
  if (misaligned(dc_du, c)) return fail(RBD_ERR_ARG, "rbd_rnea_grad: output buffers must be 16-byte aligned");
  if (qdd) return rnea_grad_launch_q<T, true>(q, qd, qdd, gravity, use_damping, B, c, dc_du, stream);
  return rbd_grad_noqdd(q, qd, gravity, use_damping, B, c, dc_du, stream);   // qdd = None (:589): the GRADN unit
}

// rnea + rnea_grad: (c, v, a, f, dc_du).  One launch when the column kernel serves the batch, otherwise the
// rnea kernel of the RNEA unit followed by the gradient kernel on the same stream.
template <class T>
int rnea_with_grad_launch(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B,
                          T* c, T* v, T* a, T* f, T* dc_du, void* stream) {
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_rnea_with_grad: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !c || !v || !a || !f || !dc_du) return fail(RBD_ERR_ARG, "rbd_rnea_with_grad: q, qd, c, v, a, f, dc_du must be non-null");
  if (misaligned(dc_du, c, v, a, f)) return fail(RBD_ERR_ARG, "rbd_rnea_with_grad: output buffers must be 16-byte aligned");
  if (grad_select<T>(B) == GradKind::COLS) {
    if (qdd) return grad_cols_launch<T, true>(q, qd, qdd, gravity, use_damping, B, c, v, a, f, dc_du, stream);
    return rbd_grad_cols_noqdd(q, qd, gravity, use_damping, B, c, v, a, f, dc_du, stream);
  }
  if (int rc = rbd_rnea(q, qd, qdd, gravity, B, c, v, a, f, stream)) return rc;
  return rnea_grad_launch<T>(q, qd, qdd, gravity, use_damping, B, nullptr, dc_du, stream);
}

// name of the kernel rnea_grad_launch<T> would run (HAS_QDD = true) under the current options
template <class T>
int grad_kernel_name(int64_t B, char* buf, size_t len) {
  const char* fmt = "";
  switch (grad_select<T>(B)) {
    case GradKind::COLS:       fmt = "rnea_grad_cols_kernel<%s,true>"; break;
    case GradKind::TREE_WS:    fmt = "rnea_grad_tree_ws_kernel<%s,true>"; break;
    case GradKind::TREE:       fmt = "rnea_grad_tree_kernel<%s,true>"; break;
    case GradKind::CHAIN_PIPE: fmt = "rnea_grad_idsva_pipe_kernel<%s,true,false>"; break;
    case GradKind::CHAIN:      fmt = "rnea_grad_idsva_kernel<%s,true,false>"; break;
    case GradKind::TWO_LANE:   fmt = "rnea_grad_kernel<%s,true,false>"; break;
  }
  std::snprintf(buf, len, fmt, type_name<T>());
  return 0;
}
#endif  // RBD_NEED_GRAD

// =============================================================================================
// minv, crba
// =============================================================================================
#ifdef RBD_NEED_MINV
// lane       fused one-lane-per-configuration kernel (rbd_minv_lane.h), where it serves the robot: no workspace
// fused      a robot whose big groups have limbs: everything in one launch (rbd_minv_fused.h), no workspace; measured on
//            Atlas against the two launches: 11.5 vs 17.3 us at B = 4 096, 27.0 vs 33.8 at 16 384, 174 vs 233 at 131 072,
//            785 vs 928 at 524 288
// two-phase  phase A through the HBM workspace, then minv_cols_kernel.  Phase A is one lane per configuration when that alone
//            fills the chip (>= 4 waves per SIMD), otherwise eight lanes per configuration (rbd_minv_ia8.h), which also
//            finishes the groups of <= 8 bodies
enum class MinvKind { LANE, FUSED, TWO_PHASE_LANE, TWO_PHASE_IA8 };
template <class T>
MinvKind minv_select(int64_t B) {
  using namespace rbdk;
  if constexpr (minv_use_lane<T>()) {
    return MinvKind::LANE;
  } else {
    const int pa = rbd_option(RBD_OPT_MINV_PHASE_A);
    if constexpr (MINV_FUSED_OK && mf_lds_bytes<T>() <= LDS_MAX) {
      if (pa == RBD_MINV_PHASE_A_FUSED || pa == RBD_MINV_PHASE_A_AUTO) return MinvKind::FUSED;
    }
    const bool lane_a = pa == RBD_MINV_PHASE_A_LANE || (pa != RBD_MINV_PHASE_A_IA8 && rbd_select_batch(B) >= 64 * 1024 * 4);
    return lane_a ? MinvKind::TWO_PHASE_LANE : MinvKind::TWO_PHASE_IA8;
  }
}
// does minv_launch<T> go through the HBM workspace under the current options?
template <class T>
int minv_needs_workspace(int64_t B) {
  const MinvKind k = minv_select<T>(B);
  return k == MinvKind::TWO_PHASE_LANE || k == MinvKind::TWO_PHASE_IA8;
}

template <class T>
int minv_launch(const T* q, int64_t B, int output_dense, T* Minv, void* workspace, size_t wsb, void* stream,
                const T* u = nullptr, const T* cbias = nullptr, T* qdd = nullptr, const T* qd = nullptr, T gravity = T(0)) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_minv: B < 0");
  if (B == 0) return 0;
  if (!q || (!Minv && !qdd)) return fail(RBD_ERR_ARG, "rbd_minv: q and Minv must be non-null");
  if (misaligned(Minv)) return fail(RBD_ERR_ARG, "rbd_minv: Minv must be 16-byte aligned");
  const MinvKind kind = minv_select<T>(B);
  unsigned grid;
  if constexpr (minv_use_lane<T>()) {
    if (int rc = grid_for(B, 64, "rbd_minv", &grid)) return rc;
    // (qd given instead of c: the kernel computes the bias force itself, rbd_minv_lane.h)
    if (qdd && !cbias && !qd) return fail(RBD_ERR_ARG, "rbd_minv (forward dynamics): c or qd must be given");
    return launch("rbd_minv launch", minv_lane_kernel<T>, grid, 64, sizeof(T) * (size_t)64 * MINV_LANE_TS, stream, q, B, output_dense,
                  Minv, u, cbias, qdd, cbias ? nullptr : qd, gravity);
  } else {
    if (qdd && !cbias) return fail(RBD_ERR_ARG, "rbd_minv (forward dynamics): this robot's kernels need the bias force c");
    if constexpr (MINV_FUSED_OK && mf_lds_bytes<T>() <= LDS_MAX) {
      if (kind == MinvKind::FUSED) {
        if (int rc = checked_grid(mf_blocks(B), "rbd_minv", &grid)) return rc;
        return launch("rbd_minv (fused) launch", minv_fused_kernel<T>, grid, 64 * MF_W, mf_lds_bytes<T>(), stream, q, B, output_dense,
                      Minv, u, cbias, qdd);
      }
    }
    const size_t need = (size_t)B * MINV_WS_PER_CFG * sizeof(T);
    if (!workspace || wsb < need) return fail(RBD_ERR_WORKSPACE, "rbd_minv: workspace missing or smaller than rbd_minv_workspace_bytes()");
    if (misaligned(workspace)) return fail(RBD_ERR_WORKSPACE, "rbd_minv: workspace must be 16-byte aligned");
    T* ws = reinterpret_cast<T*>(workspace);
    const bool lane_a = kind == MinvKind::TWO_PHASE_LANE;
    unsigned grid_b;
    if (int rc = checked_grid(minv_cols_blocks(B, !lane_a), "rbd_minv", &grid_b)) return rc;
    int rc;
    if (lane_a) {
      rc = launch("rbd_minv phase A launch", minv_ia_kernel<T>, (unsigned)((B + 63) / 64), 64, 0, stream, q, B, ws);
    } else {
      rc = launch("rbd_minv phase A launch", minv_ia8_kernel<T>, dim3((unsigned)((B + 7) / 8), n_groups()), 64, 0, stream, q, B, ws, 1,
                  output_dense, Minv, u, cbias, qdd);
    }
    if (rc != 0 || grid_b == 0) return rc;
    return launch("rbd_minv phase B launch", minv_cols_kernel<T>, grid_b, 64 * MINV_COLS_W, minv_cols_lds_bytes<T>(), stream, ws, B,
                  output_dense, Minv, u, cbias, qdd, lane_a ? 0 : 1);
  }
}

// name of the dominant kernel minv_launch<T> would run for B rows under the current options
template <class T>
int minv_kernel_name(int64_t B, char* buf, size_t len) {
  const MinvKind k = minv_select<T>(B);
  std::snprintf(buf, len, "%s<%s>", k == MinvKind::LANE ? "minv_lane_kernel" : k == MinvKind::FUSED ? "minv_fused_kernel" : "minv_cols_kernel",
                type_name<T>());
  return 0;
}

template <class T>
int crba_launch(const T* q, int64_t B, T* H, void* stream) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_crba: B < 0");
  if (B == 0) return 0;
  if (!q || !H) return fail(RBD_ERR_ARG, "rbd_crba: q and H must be non-null");
  unsigned grid;
  if (int rc = grid_for(B, 64, "rbd_crba", &grid)) return rc;
  return launch("rbd_crba launch", crba_kernel<T>, grid, 64, crba_tile_fits<T>() ? sizeof(T) * (size_t)64 * CRBA_TS : 0, stream, q, B, H);
}
#endif  // RBD_NEED_MINV

// =============================================================================================
// forward dynamics: compositions of the three kernels with fused epilogues
// =============================================================================================
template <class T>
struct FdWorkspace {
  size_t off_minv_ws, off_c, off_minv, off_qdd, off_dcdu, total;
  explicit FdWorkspace(int64_t B) {
    using namespace rbdk;
    size_t o = 0;
    off_minv_ws = o; o += align16((size_t)B * MINV_WS_PER_CFG * sizeof(T));
    off_c = o;       o += align16((size_t)B * N * sizeof(T));
    // (one-chain fp32 robots keep the packed upper triangle of Minv here, in whole tiles: rbd_fd_chain.h)
    const size_t dense = (size_t)B * N * N, packed = (size_t)((B + 63) / 64) * 64 * (N * (N + 1) / 2);
    off_minv = o;    o += align16((dense > packed ? dense : packed) * sizeof(T));
    off_qdd = o;     o += align16((size_t)B * N * sizeof(T));
    off_dcdu = o;    o += GRAD_ACC_IN_REGS ? 0 : align16((size_t)B * 2 * N * N * sizeof(T));
    total = o;
  }
};

// rbd_fdsva_so: the caller's workspace holds the forward_dynamics_grad workspace (minv's scratch is its first part and is
// reused by the dense minv that follows), then qdd [B, N], [fd_dq | fd_dqd] [B, N, 2N], Minv [B, N, N] and the
// second_order_idsva tensors [B, 4, N, N, N]
template <class T>
struct FdsoWorkspace {
  size_t fd_bytes, off_qdd, off_fd, off_minv, off_so, total;
  explicit FdsoWorkspace(int64_t B) {
    using namespace rbdk;
    const size_t nn = (size_t)N * N;
    size_t o = FdWorkspace<T>(B).total;
    fd_bytes = o;
    off_qdd = o;  o += align16((size_t)B * N * sizeof(T));
    off_fd = o;   o += align16((size_t)B * 2 * nn * sizeof(T));
    off_minv = o; o += align16((size_t)B * nn * sizeof(T));
    off_so = o;   o += align16((size_t)B * 4 * nn * N * sizeof(T));
    total = o;
  }
};
// largest B whose workspace and output sizes stay far inside size_t / int64 index arithmetic
inline int64_t fdso_max_batch() { return (int64_t)(INT64_MAX / (int64_t)(4 * (FdsoWorkspace<double>(1).total + 64))); }

#ifdef RBD_NEED_FD
template <class T>
int aba_launch(const T* q, const T* qd, const T* tau, T gravity, int64_t B, T* qdd, void* stream) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_aba: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !tau || !qdd) return fail(RBD_ERR_ARG, "rbd_aba: q, qd, tau and qdd must be non-null");
  unsigned grid;
  if (int rc = grid_for(B, ABA_PARK ? aba_lanes<T>() : 64, "rbd_aba", &grid)) return rc;
  constexpr size_t lds = aba_lds_bytes<T>();
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "rbd_aba: per-body state does not fit LDS for this robot size");
  return launch("rbd_aba launch", aba_kernel<T>, dim3(grid, ABA_PARK ? n_groups() : 1), 64, lds, stream, q, qd, tau, gravity, B, qdd);
}

template <class T>
int fd_launch(const T* q, const T* qd, const T* u, T gravity, int64_t B, T* qdd, T* dqdd_du, bool want_grad,
              void* workspace, size_t wsb, void* stream) {
  using namespace rbdk;
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_forward_dynamics: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !u) return fail(RBD_ERR_ARG, "rbd_forward_dynamics: q, qd, u must be non-null");
  if (want_grad ? !dqdd_du : !qdd) return fail(RBD_ERR_ARG, "rbd_forward_dynamics: output pointer is null");
  // refused HERE, before the first of the three launches (the gradient launcher's own check would come after two of them)
  if (misaligned(qdd, dqdd_du)) return fail(RBD_ERR_ARG, "rbd_forward_dynamics: output buffers must be 16-byte aligned");
  // qdd alone: the articulated-body sweep gives Minv (u - c) (:1372-1374) without forming Minv or c
  // (one launch, no workspace; 47 vs 76 us for the 7-DoF arm at B = 1M)
  if (!want_grad) return aba_launch<T>(q, qd, u, gravity, B, qdd, stream);
  const FdWorkspace<T> L(B);
  if (!workspace || wsb < L.total) return fail(RBD_ERR_WORKSPACE, "rbd_forward_dynamics: workspace missing or smaller than rbd_fd_workspace_bytes()");
  if (misaligned(workspace)) return fail(RBD_ERR_WORKSPACE, "rbd_forward_dynamics: workspace must be 16-byte aligned");
  char* w = reinterpret_cast<char*>(workspace);
  T* c = reinterpret_cast<T*>(w + L.off_c);
  T* Mi = reinterpret_cast<T*>(w + L.off_minv);
  T* qdd_buf = qdd ? qdd : reinterpret_cast<T*>(w + L.off_qdd);
  int rc;
  if constexpr (fd_chain_ok<T>() && grad_chain_kernel<T>()) {
    // one chain (rbd_fd_chain.h): fd_pre_kernel (bias force, Minv, qdd in one lane; Minv's upper triangle to a lane-major
    // workspace), then the world-frame chain gradient kernel with the -Minv product on its finished entries -- the
    // software-pipelined kernel in fp32 where it applies
    unsigned tiles;
    if ((rc = grid_for(B, 64, "rbd_forward_dynamics_grad", &tiles)) != 0) return rc;
    if ((rc = launch("rbd_forward_dynamics_grad (fd_pre_kernel) launch", fd_pre_kernel<T>, tiles, 64, 0, stream, q, qd, u, gravity, B, qdd_buf, Mi)) != 0) return rc;
    return chain_launch<T, true, true>(q, qd, qdd_buf, gravity, 0, B, nullptr, dqdd_du, stream, Mi);
  } else {
    // c = rnea(q, qd) with qdd = None (:1372): the c-only kernel of the RNEA unit -- or, where the one-lane minv kernel serves the
    // robot, no launch at all: that kernel computes the bias force of its groups from qd itself (rbd_minv_lane.h)
    constexpr bool bias_in_minv = minv_use_lane<T>();
    if constexpr (!bias_in_minv) {
      if ((rc = rbd_rnea(q, qd, nullptr, gravity, B, c, nullptr, nullptr, nullptr, stream)) != 0) return rc;
    }
    // qdd = Minv (u - c) (:1373-1374), fused into the last phase of minv (MINV unit)
    if ((rc = rbd_minv_fd(q, B, Mi, w + L.off_minv_ws, (size_t)B * MINV_WS_PER_CFG * sizeof(T), stream, u, bias_in_minv ? nullptr : c,
                          qdd_buf, qd, gravity)) != 0) return rc;
    // [qdd_dq | qdd_dqd] = -Minv rnea_grad(q, qd, qdd) (:1378-1383)
    if constexpr (GRAD_ACC_IN_REGS) {
      return two_lane_launch<T, true, true>(q, qd, qdd_buf, gravity, 0, B, nullptr, dqdd_du, stream, Mi);
    } else {
      // plain rnea_grad of the GRAD unit, then the -Minv product
      T* dc = reinterpret_cast<T*>(w + L.off_dcdu);
      if ((rc = rbd_rnea_grad(q, qd, qdd_buf, gravity, 0, B, nullptr, dc, stream)) != 0) return rc;
      unsigned grid;
      if ((rc = grid_for(B, negmm_cfgs<T, N>(), "rbd_forward_dynamics_grad", &grid)) != 0) return rc;
      return launch("rbd_forward_dynamics_grad apply launch", neg_mm_kernel<T, N>, grid, negmm_threads<T, N>(), 0, stream, Mi, dc, B, dqdd_du);
    }
  }
}
#endif  // RBD_NEED_FD

#ifdef RBD_NEED_FDSO
// rbd_fdsva_so: forward_dynamics_grad (qdd, fd_dq | fd_dqd), dense minv, second_order_idsva at that qdd -- the existing
// entry points, on the caller's stream -- then the contraction of rbd_fdsva_so.h.  Arguments are checked before any launch.
template <class T>
int fdso_launch(const T* q, const T* qd, const T* u, T gravity, int64_t B, T* out, void* workspace, size_t wsb, void* stream) {
  using namespace rbdk;
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "rbd_fdsva_so: fixed-base robots only");
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_fdsva_so: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !u || !out) return fail(RBD_ERR_ARG, "rbd_fdsva_so: q, qd, u and out must be non-null");
  if (B > fdso_max_batch()) return fail(RBD_ERR_ARG, "rbd_fdsva_so: B too large");
  unsigned grid;
  if (int rc = grid_for(B, fdso_cfgs(), "rbd_fdsva_so", &grid)) return rc;
  const FdsoWorkspace<T> L(B);
  if (!workspace || wsb < L.total) return fail(RBD_ERR_ARG, "rbd_fdsva_so: workspace missing or smaller than rbd_fdsva_so_workspace_bytes()");
  if (misaligned(workspace)) return fail(RBD_ERR_ARG, "rbd_fdsva_so: workspace must be 16-byte aligned");
  if constexpr (N > FDSO_MAX_N) {
    return fail(RBD_ERR_UNSUPPORTED, "rbd_fdsva_so: robots of more than 32 bodies are not supported (one thread per (j, k) column)");
  } else {
    char* w = reinterpret_cast<char*>(workspace);
    T* qdd = reinterpret_cast<T*>(w + L.off_qdd);
    T* fd = reinterpret_cast<T*>(w + L.off_fd);
    T* Mi = reinterpret_cast<T*>(w + L.off_minv);
    T* so = reinterpret_cast<T*>(w + L.off_so);
    int rc;
    if ((rc = rbd_forward_dynamics_grad(q, qd, u, gravity, B, qdd, fd, w, L.fd_bytes, stream)) != 0) return rc;
    if ((rc = rbd_minv(q, B, 1, Mi, w, L.fd_bytes, stream)) != 0) return rc;
    if ((rc = rbd_second_order_idsva(q, qd, qdd, gravity, B, so, stream)) != 0) return rc;
    // one launch per mask of the four outputs (rbd_fdsva_so.h, fdso_group)
    auto contract = [&](auto MASK) {
      return launch("rbd_fdsva_so contraction launch", fdso_contract_kernel<T, decltype(MASK)::value>, grid, fdso_threads(), 0, stream,
                    Mi, fd, so, B, out);
    };
    constexpr int G = fdso_group<T>();
    if constexpr (G == 4) {
      return contract(std::integral_constant<int, 15>{});
    } else if constexpr (G == 2) {
      if ((rc = contract(std::integral_constant<int, 3>{})) != 0) return rc;
      return contract(std::integral_constant<int, 12>{});
    } else {
      if ((rc = contract(std::integral_constant<int, 1>{})) != 0) return rc;
      if ((rc = contract(std::integral_constant<int, 2>{})) != 0) return rc;
      if ((rc = contract(std::integral_constant<int, 4>{})) != 0) return rc;
      return contract(std::integral_constant<int, 8>{});
    }
  }
}
#endif  // RBD_NEED_FDSO

#ifdef RBD_NEED_ROLL
// rbd_rollout: one launch for all T steps (rbd_rollout.h).  Arguments are checked before the launch.
template <class T>
int rollout_launch(const T* q0, const T* qd0, const T* u, int u_shared, T dt, T gravity, int integrator, int64_t B, int64_t steps,
                   T* q_out, T* qd_out, int trajectory, void* stream) {
  using namespace rbdk;
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "rbd_rollout: fixed-base robots only");
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_rollout: B < 0");
  if (steps < 0) return fail(RBD_ERR_ARG, "rbd_rollout: T < 0");
  if (!(dt - dt == T(0))) return fail(RBD_ERR_ARG, "rbd_rollout: dt must be finite");
  if (integrator != RBD_INTEGRATOR_SEMI_IMPLICIT && integrator != RBD_INTEGRATOR_EULER)
    return fail(RBD_ERR_ARG, "rbd_rollout: unknown integrator (0 = semi-implicit Euler, 1 = explicit Euler)");
  if (B == 0 || steps == 0) return 0;
  if (!q0 || !qd0 || !u || !q_out || !qd_out) return fail(RBD_ERR_ARG, "rbd_rollout: q0, qd0, u, q_out and qd_out must be non-null");
  if (misaligned(q_out, qd_out)) return fail(RBD_ERR_ARG, "rbd_rollout: output buffers must be 16-byte aligned");
  unsigned grid;
  if (int rc = grid_for(B, ABA_PARK ? roll_lanes<T>() : 64, "rbd_rollout", &grid)) return rc;
  // B T n elements of u and of each trajectory: byte offsets stay far inside int64
  if (steps > (INT64_MAX / 64) / (B * N)) return fail(RBD_ERR_ARG, "rbd_rollout: B * T * n too large");
  constexpr size_t lds = roll_lds_bytes<T>();
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "rbd_rollout: per-body state does not fit LDS for this robot size");
  const long long row = (long long)B * N;
  const int aligned = (row * (long long)sizeof(T)) % 16 == 0;      // every trajectory slice starts on a 16-byte boundary
  return launch("rbd_rollout launch", rollout_kernel<T>, dim3(grid, ABA_PARK ? n_groups() : 1), 64, lds, stream, q0, qd0,
                u, u_shared ? (long long)N : row, u_shared ? 1 : 0, dt, gravity, integrator, B, steps,
                q_out, qd_out, trajectory ? row : 0LL, aligned);
}
#endif  // RBD_NEED_ROLL

#ifdef RBD_NEED_ROLLCL
// rbd_rollout_closed_loop: one launch for all T steps, the control law inside the time loop (rbd_rollout_cl.h).  Arguments
// are checked before the launch.
template <class T>
int rollout_cl_launch(const T* q0, const T* qd0, const T* u, const T* k, const T* K, const T* q0_ref, const T* qd0_ref,
                      const T* q_ref, const T* qd_ref, const T* alpha, const T* u_lo, const T* u_hi, T dt, T gravity,
                      int integrator, int64_t B, int64_t B_nom, int64_t steps, T* q_out, T* qd_out, int trajectory, T* u_out,
                      void* stream) {
  using namespace rbdk;
  const char* who = "rbd_rollout_closed_loop";
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "%s: fixed-base robots only", who);
  if (B < 0) return fail(RBD_ERR_ARG, "%s: B < 0", who);
  if (steps < 0) return fail(RBD_ERR_ARG, "%s: T < 0", who);
  if (!(dt - dt == T(0))) return fail(RBD_ERR_ARG, "%s: dt must be finite", who);
  if (integrator != RBD_INTEGRATOR_SEMI_IMPLICIT && integrator != RBD_INTEGRATOR_EULER)
    return fail(RBD_ERR_ARG, "%s: unknown integrator (0 = semi-implicit Euler, 1 = explicit Euler)", who);
  if (B == 0 || steps == 0) return 0;
  if (B_nom <= 0 || B % B_nom != 0) return fail(RBD_ERR_ARG, "%s: B_nom must be positive and divide B", who);
  if (!q0 || !qd0 || !u || !K || !q0_ref || !qd0_ref || !q_ref || !qd_ref || !q_out || !qd_out)
    return fail(RBD_ERR_ARG, "%s: q0, qd0, u, K, q0_ref, qd0_ref, q_ref, qd_ref, q_out and qd_out must be non-null", who);
  if ((k == nullptr) != (alpha == nullptr)) return fail(RBD_ERR_ARG, "%s: k and alpha must be both null or both non-null", who);
  if ((u_lo == nullptr) != (u_hi == nullptr)) return fail(RBD_ERR_ARG, "%s: u_lo and u_hi must be both null or both non-null", who);
  if (misaligned(q_out, qd_out, u_out)) return fail(RBD_ERR_ARG, "%s: output buffers must be 16-byte aligned", who);
  unsigned grid;
  if (int rc = grid_for(B, ABA_PARK ? rollcl_lanes<T>() : 64, who, &grid)) return rc;
  // B T n elements of each trajectory, B_nom T n 2n of K: byte offsets stay far inside int64
  if (steps > (INT64_MAX / 64) / (B * N)) return fail(RBD_ERR_ARG, "%s: B * T * n too large", who);
  if (steps > (INT64_MAX / 64) / (B_nom * N * 2 * N)) return fail(RBD_ERR_ARG, "%s: B_nom * T * n * 2n too large", who);
  constexpr size_t lds = rollcl_lds_bytes<T>();
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "%s: per-body state does not fit LDS for this robot size", who);
  const long long row = (long long)B * N;
  const int aligned = (row * (long long)sizeof(T)) % 16 == 0;      // every trajectory slice starts on a 16-byte boundary
  return launch("rbd_rollout_closed_loop launch", rollout_closed_loop_kernel<T>, grid, ROLLCL_THREADS, lds, stream, q0, qd0, u, k, K, q0_ref,
                qd0_ref, q_ref, qd_ref, alpha, u_lo, u_hi, dt, gravity, integrator, B, B_nom, steps, q_out, qd_out,
                trajectory ? 1 : 0, u_out, row, aligned);
}
#endif  // RBD_NEED_ROLLCL

#ifdef RBD_NEED_ROLLCOST
// rbd_rollout_cost: one launch for all T steps, the control law and the cost's accumulation inside the time loop
// (rbd_rollout_cost.h).  Arguments are checked before the launch.
template <class T>
int rollout_cost_launch(const T* q0, const T* qd0, const T* u, const T* k, const T* K, const T* q0_ref, const T* qd0_ref,
                        const T* q_ref, const T* qd_ref, const T* alpha, const T* du, const T* u_lo, const T* u_hi,
                        const T* q_tgt, const T* qd_tgt, const T* w_q, const T* w_qd, int x_final_only, const T* w_u,
                        const T* c_u, T dt, T gravity, int integrator, int64_t B, int64_t B_nom, int64_t steps, T* cost,
                        T* q_out, T* qd_out, int trajectory, T* u_out, void* stream) {
  using namespace rbdk;
  const char* who = "rbd_rollout_cost";
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "%s: fixed-base robots only", who);
  if (B < 0) return fail(RBD_ERR_ARG, "%s: B < 0", who);
  if (steps < 0) return fail(RBD_ERR_ARG, "%s: T < 0", who);
  if (!(dt - dt == T(0))) return fail(RBD_ERR_ARG, "%s: dt must be finite", who);
  if (integrator != RBD_INTEGRATOR_SEMI_IMPLICIT && integrator != RBD_INTEGRATOR_EULER)
    return fail(RBD_ERR_ARG, "%s: unknown integrator (0 = semi-implicit Euler, 1 = explicit Euler)", who);
  if (B == 0 || steps == 0) return 0;
  if (B_nom <= 0 || B % B_nom != 0) return fail(RBD_ERR_ARG, "%s: B_nom must be positive and divide B", who);
  if (!q0 || !qd0 || !u || !cost) return fail(RBD_ERR_ARG, "%s: q0, qd0, u and cost must be non-null", who);
  if (K && (!q0_ref || !qd0_ref || !q_ref || !qd_ref))
    return fail(RBD_ERR_ARG, "%s: K needs q0_ref, qd0_ref, q_ref and qd_ref", who);
  if ((k == nullptr) != (alpha == nullptr)) return fail(RBD_ERR_ARG, "%s: k and alpha must be both null or both non-null", who);
  if ((u_lo == nullptr) != (u_hi == nullptr)) return fail(RBD_ERR_ARG, "%s: u_lo and u_hi must be both null or both non-null", who);
  if ((q_out == nullptr) != (qd_out == nullptr)) return fail(RBD_ERR_ARG, "%s: q_out and qd_out must be both null or both non-null", who);
  if (misaligned(cost, q_out, qd_out, u_out)) return fail(RBD_ERR_ARG, "%s: output buffers must be 16-byte aligned", who);
  unsigned grid;
  if (int rc = grid_for(B, ABA_PARK ? rollcl_lanes<T>() : 64, who, &grid)) return rc;
  // B T n elements of du and of each trajectory, B_nom T n 2n of K: byte offsets stay far inside int64
  if (steps > (INT64_MAX / 64) / (B * N)) return fail(RBD_ERR_ARG, "%s: B * T * n too large", who);
  if (steps > (INT64_MAX / 64) / (B_nom * N * 2 * N)) return fail(RBD_ERR_ARG, "%s: B_nom * T * n * 2n too large", who);
  constexpr size_t lds = rollcl_lds_bytes<T>();
  if (lds > LDS_MAX) return fail(RBD_ERR_UNSUPPORTED, "%s: per-body state does not fit LDS for this robot size", who);
  const long long row = (long long)B * N;
  const int aligned = (row * (long long)sizeof(T)) % 16 == 0;      // every trajectory slice starts on a 16-byte boundary
  const RollCostModel<T> cm{q_tgt, qd_tgt, w_q, w_qd, w_u, c_u, x_final_only ? 1 : 0};
  return launch("rbd_rollout_cost launch", rollout_cost_kernel<T>, grid, ROLLCL_THREADS, lds, stream, q0, qd0, u, k, K, q0_ref,
                qd0_ref, q_ref, qd_ref, alpha, du, u_lo, u_hi, cm, dt, gravity, integrator, B, B_nom, steps, cost, q_out,
                qd_out, trajectory ? 1 : 0, u_out, row, aligned);
}
#endif  // RBD_NEED_ROLLCOST

// rbd_mppi_update's workspace: e [S, P] | eta [P] | the chunk partials [ceil(S / C), T, P, N] when there is more than one chunk
#if defined(RBD_TU_COMMON) || defined(RBD_NEED_MPPI)
// S P and T S P n elements whose byte offsets stay far inside int64 (sizes are positive)
inline bool mppi_sizes_ok(int64_t S, int64_t P, int64_t steps) {
  const int64_t lim = INT64_MAX / 64;
  return S <= lim / P && steps <= lim / (S * P) && steps * S * P <= lim / rbdm::N;
}
struct MppiWorkspace {
  int64_t nchunks;
  size_t off_eta, off_part, total;
  MppiWorkspace(int64_t S, int64_t P, int64_t steps, size_t esz) {
    nchunks = (S + RBD_MPPI_CHUNK - 1) / RBD_MPPI_CHUNK;
    size_t o = align16((size_t)S * (size_t)P * esz);
    off_eta = o;  o += align16((size_t)P * esz);
    off_part = o; o += nchunks > 1 ? align16((size_t)nchunks * (size_t)steps * (size_t)P * rbdm::N * esz) : 0;
    total = o;
  }
};
#endif

#ifdef RBD_NEED_MPPI
// rbd_mppi_update: weights, the pass over du, the combine (rbd_mppi.h).  Arguments are checked before the first launch.
template <class T>
int mppi_launch(const T* J, const T* du, const T* u, const T* lam, const T* u_lo, const T* u_hi, int64_t S, int64_t P,
                int64_t steps, T* u_out, T* w_out, T* ess_out, int32_t* status_out, void* workspace, size_t wsb, void* stream) {
  using namespace rbdk;
  const char* who = "rbd_mppi_update";
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "%s: fixed-base robots only", who);
  if (S < 0) return fail(RBD_ERR_ARG, "%s: S < 0", who);
  if (P < 0) return fail(RBD_ERR_ARG, "%s: P < 0", who);
  if (steps < 0) return fail(RBD_ERR_ARG, "%s: T < 0", who);
  if (S == 0 || P == 0 || steps == 0) return 0;
  if (!J || !du || !u || !lam || !u_out || !status_out)
    return fail(RBD_ERR_ARG, "%s: J, du, u, lam, u_out and status_out must be non-null", who);
  if ((u_lo == nullptr) != (u_hi == nullptr)) return fail(RBD_ERR_ARG, "%s: u_lo and u_hi must be both null or both non-null", who);
  if (!mppi_sizes_ok(S, P, steps)) return fail(RBD_ERR_ARG, "%s: S * P or T * S * P * n too large", who);
  if (misaligned(u_out, w_out, ess_out, status_out)) return fail(RBD_ERR_ARG, "%s: output buffers must be 16-byte aligned", who);
  const MppiWorkspace L(S, P, steps, sizeof(T));
  if (!workspace || wsb < L.total)
    return fail(RBD_ERR_WORKSPACE, "%s: workspace missing or smaller than rbd_mppi_update_workspace_bytes(S, P, T, .)", who);
  if (misaligned(workspace)) return fail(RBD_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
  constexpr int VE = mppi_vec<T>();
  const int64_t R = P * N;
  const bool vec = R % VE == 0 && !misaligned(du);
  const int64_t groups = vec ? R / VE : R;
  unsigned grid_w, grid_p, grid_c = 0;
  const bool small = L.nchunks == 1;
  if (int rc = small ? grid_for(P, MPPI_THREADS, who, &grid_w) : checked_grid(P, who, &grid_w)) return rc;
  if (int rc = grid_for(steps * L.nchunks * groups, MPPI_THREADS, who, &grid_p)) return rc;
  if (!small)
    if (int rc = grid_for(steps * R, MPPI_COMB_O, who, &grid_c)) return rc;
  char* w = reinterpret_cast<char*>(workspace);
  T* e_ws = reinterpret_cast<T*>(w);
  T* eta_ws = reinterpret_cast<T*>(w + L.off_eta);
  T* part = reinterpret_cast<T*>(w + L.off_part);
  int rc = small ? launch("rbd_mppi_update (weights) launch", mppi_weights_small_kernel<T>, grid_w, MPPI_THREADS, 0, stream, J, lam,
                          S, P, e_ws, eta_ws, w_out, ess_out, status_out)
                 : launch("rbd_mppi_update (weights) launch", mppi_weights_kernel<T>, grid_w, MPPI_W_THREADS, 0, stream, J, lam, S, P,
                          e_ws, eta_ws, w_out, ess_out, status_out);
  if (rc != 0) return rc;
  T* out = small ? u_out : part;
  rc = vec ? launch("rbd_mppi_update (partials) launch", mppi_partials_kernel<T, VE>, grid_p, MPPI_THREADS, 0, stream, du, u, e_ws,
                    eta_ws, u_lo, u_hi, S, P, steps, L.nchunks, groups, out)
           : launch("rbd_mppi_update (partials) launch", mppi_partials_kernel<T, 1>, grid_p, MPPI_THREADS, 0, stream, du, u, e_ws,
                    eta_ws, u_lo, u_hi, S, P, steps, L.nchunks, groups, out);
  if (rc != 0 || small) return rc;
  return launch("rbd_mppi_update (combine) launch", mppi_combine_kernel<T>, grid_c, MPPI_THREADS, 0, stream, part, u, eta_ws, u_lo,
                u_hi, P, steps * R, L.nchunks, u_out);
}
#endif  // RBD_NEED_MPPI

// rbd_rollout_grad's workspace for chunks of Tc steps, R = Tc B flat rows: minv's scratch | qdd [R, N] | dc_du [R, N, 2N] |
// Minv [R, N, N] | lam [B, 2N]
#if defined(RBD_TU_COMMON) || defined(RBD_NEED_ROLLG)
constexpr int64_t ROLLG_MAX_ROWS = (int64_t)1 << 30;      // rows of one chunk, and B: every launcher's grid holds them
template <class T>
struct RollgWorkspace {
  size_t minv_ws_bytes, off_qdd, off_dcdu, off_minv, off_lam, total;
  RollgWorkspace(int64_t B, int64_t Tc) {
    using namespace rbdk;
    const size_t R = (size_t)B * (size_t)Tc;
    size_t o = 0;
    minv_ws_bytes = R * MINV_WS_PER_CFG * sizeof(T);
    o += align16(minv_ws_bytes);
    off_qdd = o;  o += align16(R * N * sizeof(T));
    off_dcdu = o; o += align16(R * 2 * N * N * sizeof(T));
    off_minv = o; o += align16(R * N * N * sizeof(T));
    off_lam = o;  o += align16((size_t)B * 2 * N * sizeof(T));
    total = o;
  }
};
#endif

#if defined(RBD_NEED_ROLLG) || defined(RBD_NEED_LQR)
// (rbd_aba of the FD unit, as the overloads of RBD_CROSS_UNIT)
inline int rbd_aba(const float* q, const float* qd, const float* tau, float g, int64_t B, float* qdd, void* s) {
  return rbd_aba_f32(q, qd, tau, g, B, qdd, s);
}
inline int rbd_aba(const double* q, const double* qd, const double* tau, double g, int64_t B, double* qdd, void* s) {
  return rbd_aba_f64(q, qd, tau, g, B, qdd, s);
}
#endif
#ifdef RBD_NEED_ROLLG
// what rbd_rollout_adjoint and rbd_rollout_grad refuse alike, before any launch
template <class T>
int rollg_check(const char* who, T dt, int integrator, int64_t B, int64_t steps) {
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "%s: fixed-base robots only", who);
  if (B < 0) return fail(RBD_ERR_ARG, "%s: B < 0", who);
  if (steps < 0) return fail(RBD_ERR_ARG, "%s: T < 0", who);
  if (!(dt - dt == T(0))) return fail(RBD_ERR_ARG, "%s: dt must be finite", who);
  if (integrator != RBD_INTEGRATOR_SEMI_IMPLICIT && integrator != RBD_INTEGRATOR_EULER)
    return fail(RBD_ERR_ARG, "%s: unknown integrator (0 = semi-implicit Euler, 1 = explicit Euler)", who);
  return 0;
}
// B T n 2n elements of dc_du: byte offsets stay far inside int64
int rollg_check_size(const char* who, int64_t B, int64_t steps) {
  if (B > ROLLG_MAX_ROWS) return fail(RBD_ERR_ARG, "%s: B too large", who);
  if (steps > (INT64_MAX / 64) / (B * rbdk::N * 2 * rbdk::N)) return fail(RBD_ERR_ARG, "%s: B * T * n * 2n too large", who);
  return 0;
}

// the scan (rbd_rollout_adj.h): one launch for `steps` steps; out_q0 / out_qd0 (the composite's last chunk) may be null
template <class T>
int rollg_scan(const char* who, const T* dc_du, const T* Minv, const T* gq, const T* gqd, int g_final_only, T dt, int integrator,
               int64_t B, int64_t steps, T* lam, T* grad_u, T* out_q0, T* out_qd0, void* stream) {
  using namespace rbdk;
  unsigned grid;
  if (int rc = grid_for(B, rollg_cfgs(), who, &grid)) return rc;
  return launch(who, rollout_adjoint_kernel<T>, grid, rollg_threads(), 0, stream, dc_du, Minv, gq, gqd, g_final_only ? 1 : 0, dt,
                integrator, B, steps, lam, grad_u, out_q0, out_qd0);
}

template <class T>
int rollout_adjoint_launch(const T* dc_du, const T* Minv, const T* gq, const T* gqd, int g_final_only, T dt, int integrator,
                           int64_t B, int64_t steps, T* lam, T* grad_u, void* stream) {
  if (int rc = rollg_check<T>("rbd_rollout_adjoint", dt, integrator, B, steps)) return rc;
  if (B == 0 || steps == 0) return 0;
  if (!dc_du || !Minv || !lam || !grad_u) return fail(RBD_ERR_ARG, "rbd_rollout_adjoint: dc_du, Minv, lam and grad_u must be non-null");
  if (misaligned(lam, grad_u)) return fail(RBD_ERR_ARG, "rbd_rollout_adjoint: output buffers must be 16-byte aligned");
  if (int rc = rollg_check_size("rbd_rollout_adjoint", B, steps)) return rc;
  return rollg_scan<T>("rbd_rollout_adjoint launch", dc_du, Minv, gq, gqd, g_final_only, dt, integrator, B, steps, lam, grad_u,
                       nullptr, nullptr, stream);
}

// rbd_rollout_grad: lam = 0, then chunks of the time axis from the end -- aba, rnea_grad, minv on the chunk's flat rows (the
// existing entry points, on the caller's stream), then the scan.  Step 0 is linearised at (q0, qd0, u[0]): its own chunk.
template <class T>
int rollout_grad_launch(const T* q0, const T* qd0, const T* u, const T* q_traj, const T* qd_traj, const T* gq, const T* gqd,
                        int g_final_only, T dt, T gravity, int integrator, int64_t B, int64_t steps, T* grad_u, T* grad_q0,
                        T* grad_qd0, void* workspace, size_t wsb, void* stream) {
  using namespace rbdk;
  if (int rc = rollg_check<T>("rbd_rollout_grad", dt, integrator, B, steps)) return rc;
  if (B == 0 || steps == 0) return 0;
  if (!q0 || !qd0 || !u || !q_traj || !qd_traj || !grad_u || !grad_q0 || !grad_qd0)
    return fail(RBD_ERR_ARG, "rbd_rollout_grad: q0, qd0, u, q_traj, qd_traj, grad_u, grad_q0 and grad_qd0 must be non-null");
  if (misaligned(grad_u, grad_q0, grad_qd0)) return fail(RBD_ERR_ARG, "rbd_rollout_grad: output buffers must be 16-byte aligned");
  if (int rc = rollg_check_size("rbd_rollout_grad", B, steps)) return rc;
  if (!workspace || wsb < RollgWorkspace<T>(B, 1).total)
    return fail(RBD_ERR_WORKSPACE, "rbd_rollout_grad: workspace missing or smaller than rbd_rollout_grad_workspace_bytes(B, 1, .)");
  if (misaligned(workspace)) return fail(RBD_ERR_ARG, "rbd_rollout_grad: workspace must be 16-byte aligned");
  // the largest chunk that fits (the size grows with Tc)
  int64_t Tc = 1, hi_tc = steps - 1 < ROLLG_MAX_ROWS / B ? steps - 1 : ROLLG_MAX_ROWS / B;
  while (Tc < hi_tc) {
    const int64_t mid = Tc + (hi_tc - Tc + 1) / 2;
    if (RollgWorkspace<T>(B, mid).total <= wsb) Tc = mid; else hi_tc = mid - 1;
  }
  const RollgWorkspace<T> L(B, Tc);
  char* w = reinterpret_cast<char*>(workspace);
  T* qdd = reinterpret_cast<T*>(w + L.off_qdd);
  T* dc = reinterpret_cast<T*>(w + L.off_dcdu);
  T* Mi = reinterpret_cast<T*>(w + L.off_minv);
  T* lam = reinterpret_cast<T*>(w + L.off_lam);
  const hipError_t e = hipMemsetAsync(lam, 0, (size_t)B * 2 * N * sizeof(T), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "rbd_rollout_grad (zeroing the adjoint)");
  const int64_t row = B * N;
  // steps [lo, hi) at rows q, qd, uu; g is dense [T, B, N] or belongs to step T - 1 alone
  auto chunk = [&](const T* q, const T* qd, int64_t lo, int64_t hi) {
    const int64_t R = (hi - lo) * B;
    const bool last = hi == steps;
    const T* cgq = g_final_only ? (last ? gq : nullptr) : (gq ? gq + lo * row : nullptr);
    const T* cgqd = g_final_only ? (last ? gqd : nullptr) : (gqd ? gqd + lo * row : nullptr);
    int rc;
    if ((rc = rbd_aba(q, qd, u + lo * row, gravity, R, qdd, stream)) != 0) return rc;
    if ((rc = rbd_rnea_grad(q, qd, qdd, gravity, 0, R, nullptr, dc, stream)) != 0) return rc;
    if ((rc = rbd_minv(q, R, 1, Mi, w, L.minv_ws_bytes, stream)) != 0) return rc;
    return rollg_scan<T>("rbd_rollout_grad (scan) launch", dc, Mi, cgq, cgqd, g_final_only, dt, integrator, B, hi - lo, lam,
                         grad_u + lo * row, lo == 0 ? grad_q0 : nullptr, lo == 0 ? grad_qd0 : nullptr, stream);
  };
  for (int64_t hi = steps; hi > 1;) {
    const int64_t lo = hi - Tc > 1 ? hi - Tc : 1;
    if (int rc = chunk(q_traj + (lo - 1) * row, qd_traj + (lo - 1) * row, lo, hi)) return rc;
    hi = lo;
  }
  return chunk(q0, qd0, 0, 1);
}
#endif  // RBD_NEED_ROLLG

// rbd_rollout_lqr's workspace for chunks of Tc steps, R = Tc B flat rows: minv's scratch | qdd [R, N] | dc_du [R, N, 2N] |
// Minv [R, N, N] (lam, P, dV and status are the caller's)
#if defined(RBD_TU_COMMON) || defined(RBD_NEED_LQR)
constexpr int64_t LQR_MAX_ROWS = (int64_t)1 << 30;        // rows of one chunk, and B: every launcher's grid holds them
template <class T>
struct LqrWorkspace {
  size_t minv_ws_bytes, off_qdd, off_dcdu, off_minv, total;
  LqrWorkspace(int64_t B, int64_t Tc) {
    using namespace rbdk;
    const size_t R = (size_t)B * (size_t)Tc;
    size_t o = 0;
    minv_ws_bytes = R * MINV_WS_PER_CFG * sizeof(T);
    o += align16(minv_ws_bytes);
    off_qdd = o;  o += align16(R * N * sizeof(T));
    off_dcdu = o; o += align16(R * 2 * N * N * sizeof(T));
    off_minv = o; o += align16(R * N * N * sizeof(T));
    total = o;
  }
};
#endif

#ifdef RBD_NEED_LQR
// what rbd_rollout_riccati and rbd_rollout_lqr refuse alike, before any launch
template <class T>
int lqr_check(const char* who, T reg, T dt, int integrator, int64_t B, int64_t steps) {
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "%s: fixed-base robots only", who);
  if (B < 0) return fail(RBD_ERR_ARG, "%s: B < 0", who);
  if (steps < 0) return fail(RBD_ERR_ARG, "%s: T < 0", who);
  if (!(dt - dt == T(0))) return fail(RBD_ERR_ARG, "%s: dt must be finite", who);
  if (!(reg - reg == T(0)) || reg < T(0)) return fail(RBD_ERR_ARG, "%s: reg must be finite and >= 0", who);
  if (integrator != RBD_INTEGRATOR_SEMI_IMPLICIT && integrator != RBD_INTEGRATOR_EULER)
    return fail(RBD_ERR_ARG, "%s: unknown integrator (0 = semi-implicit Euler, 1 = explicit Euler)", who);
  return 0;
}
// B T n 2n elements of dc_du and of K, B 2n 2n of P: byte offsets stay far inside int64; then what the kernel itself needs
template <class T>
int lqr_check_size(const char* who, int64_t B, int64_t steps) {
  if (B > LQR_MAX_ROWS) return fail(RBD_ERR_ARG, "%s: B too large", who);
  if (steps > (INT64_MAX / 64) / (B * rbdk::N * 2 * rbdk::N)) return fail(RBD_ERR_ARG, "%s: B * T * n * 2n too large", who);
  if (!rbdk::lqr_fits<T>())
    return fail(RBD_ERR_UNSUPPORTED, "%s: the step's matrices (8 n^2 scalars per row) do not fit LDS for this robot size and precision", who);
  return 0;
}

// the scan (rbd_rollout_lqr.h): one launch for `steps` steps
template <class T>
int lqr_scan(const char* who, const T* dc_du, const T* Minv, const T* gq, const T* gqd, const T* hq, const T* hqd, int x_final_only,
             const T* gu, const T* hu, int hu_shared, T reg, T dt, int integrator, int64_t B, int64_t steps, T* lam, T* P, T* dV,
             int32_t* status, T* k, T* K, void* stream) {
  using namespace rbdk;
  unsigned grid;
  if (int rc = grid_for(B, lqr_cfgs(), who, &grid)) return rc;
  return launch(who, rollout_riccati_kernel<T>, grid, lqr_threads(), 0, stream, dc_du, Minv, gq, gqd, hq, hqd, x_final_only ? 1 : 0,
                gu, hu, hu_shared ? 1 : 0, reg, dt, integrator, B, steps, lam, P, dV, reinterpret_cast<int*>(status), k, K);
}

template <class T>
int rollout_riccati_launch(const T* dc_du, const T* Minv, const T* gq, const T* gqd, const T* hq, const T* hqd, int x_final_only,
                           const T* gu, const T* hu, int hu_shared, T reg, T dt, int integrator, int64_t B, int64_t steps, T* lam,
                           T* P, T* dV, int32_t* status, T* k, T* K, void* stream) {
  if (int rc = lqr_check<T>("rbd_rollout_riccati", reg, dt, integrator, B, steps)) return rc;
  if (B == 0 || steps == 0) return 0;
  if (!dc_du || !Minv || !hu || !lam || !P || !dV || !status || !k || !K)
    return fail(RBD_ERR_ARG, "rbd_rollout_riccati: dc_du, Minv, hu, lam, P, dV, status, k and K must be non-null");
  if (misaligned(lam, P, dV, status, k, K)) return fail(RBD_ERR_ARG, "rbd_rollout_riccati: output buffers must be 16-byte aligned");
  if (int rc = lqr_check_size<T>("rbd_rollout_riccati", B, steps)) return rc;
  return lqr_scan<T>("rbd_rollout_riccati launch", dc_du, Minv, gq, gqd, hq, hqd, x_final_only, gu, hu, hu_shared, reg, dt,
                     integrator, B, steps, lam, P, dV, status, k, K, stream);
}

// rbd_rollout_lqr: lam = P = dV = status = 0, then chunks of the time axis from the end as rbd_rollout_grad walks them -- aba,
// rnea_grad, minv on the chunk's flat rows (the existing entry points, on the caller's stream), then the scan.  Step 0 is
// linearised at (q0, qd0, u[0]): its own chunk.
template <class T>
int rollout_lqr_launch(const T* q0, const T* qd0, const T* u, const T* q_traj, const T* qd_traj, const T* gq, const T* gqd,
                       const T* hq, const T* hqd, int x_final_only, const T* gu, const T* hu, int hu_shared, T reg, T dt, T gravity,
                       int integrator, int64_t B, int64_t steps, T* k, T* K, T* lam, T* P, T* dV, int32_t* status, void* workspace,
                       size_t wsb, void* stream) {
  using namespace rbdk;
  if (int rc = lqr_check<T>("rbd_rollout_lqr", reg, dt, integrator, B, steps)) return rc;
  if (B == 0 || steps == 0) return 0;
  if (!q0 || !qd0 || !u || !q_traj || !qd_traj || !hu || !k || !K || !lam || !P || !dV || !status)
    return fail(RBD_ERR_ARG, "rbd_rollout_lqr: q0, qd0, u, q_traj, qd_traj, hu, k, K, lam, P, dV and status must be non-null");
  if (misaligned(k, K, lam, P, dV, status)) return fail(RBD_ERR_ARG, "rbd_rollout_lqr: output buffers must be 16-byte aligned");
  if (int rc = lqr_check_size<T>("rbd_rollout_lqr", B, steps)) return rc;
  if (!workspace || wsb < LqrWorkspace<T>(B, 1).total)
    return fail(RBD_ERR_WORKSPACE, "rbd_rollout_lqr: workspace missing or smaller than rbd_rollout_lqr_workspace_bytes(B, 1, .)");
  if (misaligned(workspace)) return fail(RBD_ERR_ARG, "rbd_rollout_lqr: workspace must be 16-byte aligned");
  // the largest chunk that fits (the size grows with Tc)
  int64_t Tc = 1, hi_tc = steps - 1 < LQR_MAX_ROWS / B ? steps - 1 : LQR_MAX_ROWS / B;
  while (Tc < hi_tc) {
    const int64_t mid = Tc + (hi_tc - Tc + 1) / 2;
    if (LqrWorkspace<T>(B, mid).total <= wsb) Tc = mid; else hi_tc = mid - 1;
  }
  const LqrWorkspace<T> L(B, Tc);
  char* w = reinterpret_cast<char*>(workspace);
  T* qdd = reinterpret_cast<T*>(w + L.off_qdd);
  T* dc = reinterpret_cast<T*>(w + L.off_dcdu);
  T* Mi = reinterpret_cast<T*>(w + L.off_minv);
  hipError_t e = hipMemsetAsync(lam, 0, (size_t)B * 2 * N * sizeof(T), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(P, 0, (size_t)B * 4 * N * N * sizeof(T), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(dV, 0, (size_t)B * 2 * sizeof(T), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "rbd_rollout_lqr (zeroing the value function)");
  const int64_t row = B * N;
  // steps [lo, hi) at rows q, qd; the state costs are dense [T, B, N] or belong to step T - 1 alone
  auto chunk = [&](const T* q, const T* qd, int64_t lo, int64_t hi) {
    const int64_t R = (hi - lo) * B;
    const bool last = hi == steps;
    auto at = [&](const T* a) { return x_final_only ? (last ? a : nullptr) : (a ? a + lo * row : nullptr); };
    int rc;
    if ((rc = rbd_aba(q, qd, u + lo * row, gravity, R, qdd, stream)) != 0) return rc;
    if ((rc = rbd_rnea_grad(q, qd, qdd, gravity, 0, R, nullptr, dc, stream)) != 0) return rc;
    if ((rc = rbd_minv(q, R, 1, Mi, w, L.minv_ws_bytes, stream)) != 0) return rc;
    return lqr_scan<T>("rbd_rollout_lqr (scan) launch", dc, Mi, at(gq), at(gqd), at(hq), at(hqd), x_final_only,
                       gu ? gu + lo * row : nullptr, hu_shared ? hu : hu + lo * row, hu_shared, reg, dt, integrator, B, hi - lo, lam,
                       P, dV, status, k + lo * row, K + lo * row * 2 * N, stream);
  };
  for (int64_t hi = steps; hi > 1;) {
    const int64_t lo = hi - Tc > 1 ? hi - Tc : 1;
    if (int rc = chunk(q_traj + (lo - 1) * row, qd_traj + (lo - 1) * row, lo, hi)) return rc;
    hi = lo;
  }
  return chunk(q0, qd0, 0, 1);
}
#endif  // RBD_NEED_LQR

#ifdef RBD_NEED_EE
// rbd_ee_pose: site table (host arrays) -> EeSites kernel argument; one launch for pose, gradient or both
template <class T>
int ee_launch(const T* q, int64_t B, const int32_t* site_body, const double* site_T, const double* offset, int n_sites,
              T* pose, T* dpose, void* stream) {
  using namespace rbdk;
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "rbd_ee_pose: fixed-base robots only");
  if (n_sites < 1 || n_sites > RBD_EE_MAX_SITES) return fail(RBD_ERR_ARG, "rbd_ee_pose: n_sites must be in [1, RBD_EE_MAX_SITES]");
  if (!site_body || !site_T || !offset) return fail(RBD_ERR_ARG, "rbd_ee_pose: site_body, site_T and offset must be non-null");
  EeSites<T> st;
  std::memset(&st, 0, sizeof(st));
  st.n_sites = n_sites;
  const double w = offset[3];
  st.w = (T)w;
  for (int s = 0; s < n_sites; ++s) {
    if (site_body[s] < 0 || site_body[s] >= rbdm::N) return fail(RBD_ERR_ARG, "rbd_ee_pose: site body id out of range");
    st.body[s] = site_body[s];
    const double* M = site_T + 12 * s;              // [R | t] row-major 3 x 4
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) st.M[s][3 * r + c] = (T)M[4 * r + c];
      st.pl[s][r] = (T)(M[4 * r] * offset[0] + M[4 * r + 1] * offset[1] + M[4 * r + 2] * offset[2] + w * M[4 * r + 3]);
    }
  }
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_ee_pose: B < 0");
  if (B == 0) return 0;                             // (empty outputs may come as null pointers)
  if (!q) return fail(RBD_ERR_ARG, "rbd_ee_pose: q must be non-null");
  if (!pose && !dpose) return fail(RBD_ERR_ARG, "rbd_ee_pose: pose and dpose are both null");
  if (misaligned(pose, dpose)) return fail(RBD_ERR_ARG, "rbd_ee_pose: output buffers must be 16-byte aligned");
  unsigned grid;
  if (int rc = grid_for(B, 64, "rbd_ee_pose", &grid)) return rc;
  const size_t lds = ee_lds_bytes<T>(n_sites, pose != nullptr, dpose != nullptr);
  if (lds > LDS_MAX)                // (a robot near RBD_MAX_BODIES in fp64: its [64][6n] gradient tile alone)
    return fail(RBD_ERR_UNSUPPORTED, "rbd_ee_pose: the q / pose / gradient tiles exceed the 160 KB of LDS of a CU for this "
                                     "robot and precision; pass fewer sites per call");
  auto go = [&](auto kernel) { return launch("rbd_ee_pose launch", kernel, grid, 64, lds, stream, q, B, st, pose, dpose); };
  return pose && dpose ? go(ee_pose_kernel<T, true, true>) : pose ? go(ee_pose_kernel<T, true, false>) : go(ee_pose_kernel<T, false, true>);
}
#endif  // RBD_NEED_EE

#ifdef RBD_NEED_SO
// rbd_second_order_idsva: out [B, 4, N, N, N]; arguments checked before anything touches the GPU
template <class T>
int so_launch(const T* q, const T* qd, const T* qdd, T gravity, int64_t B, T* out, void* stream) {
  using namespace rbdk;
  if (rbdm::FLOATING_BASE) return fail(RBD_ERR_UNSUPPORTED, "rbd_second_order_idsva: fixed-base robots only");
  if (B < 0) return fail(RBD_ERR_ARG, "rbd_second_order_idsva: B < 0");
  if (B == 0) return 0;
  if (!q || !qd || !qdd || !out) return fail(RBD_ERR_ARG, "rbd_second_order_idsva: q, qd, qdd and out must be non-null");
  unsigned grid;
  if (int rc = grid_for(B, so_configs_per_block<T>(), "rbd_second_order_idsva", &grid)) return rc;
  if (B > (int64_t)(INT64_MAX / SO_PER_CFG)) return fail(RBD_ERR_ARG, "rbd_second_order_idsva: B too large");
  return launch("rbd_second_order_idsva launch", so_idsva_kernel<T>, grid, SO_THREADS, 0, stream, q, qd, qdd, gravity, B, out);
}
#endif  // RBD_NEED_SO

#ifdef RBD_NEED_PASS
// ---- per-pass entry points (rbd_passes.h): one lane per configuration, no LDS ---------------------------------------------
template <class... P>
int pass_launch(const char* who, bool args_ok, void (*kernel)(P...), int64_t B, void* stream, typename rbd_as_declared<P>::type... args) {
  if (B < 0) return fail(RBD_ERR_ARG, "%s: B < 0", who);
  unsigned grid;
  if (int rc = grid_for(B, 64, who, &grid)) return rc;
  if (B == 0) return 0;
  if (!args_ok) return fail(RBD_ERR_ARG, "%s: null pointer argument", who);
  return launch(who, kernel, grid, 64, 0, stream, args...);
}
template <class T, bool DQ>
int grad_fpass_launch(const T* q, const T* qd, const T* v, const T* a, T gravity, int64_t B, T* dv, T* da, T* df, void* stream) {
  return pass_launch(DQ ? "rbd_rnea_grad_fpass_dq" : "rbd_rnea_grad_fpass_dqd", q && qd && v && (!DQ || a) && dv && da && df,
                     rbdk::grad_fpass_kernel<T, DQ>, B, stream, q, qd, v, a, gravity, B, dv, da, df);
}
template <class T, bool DQ>
int grad_bpass_launch(const T* q, const T* f, T* df, int use_damping, int64_t B, T* dc, void* stream) {
  return pass_launch(DQ ? "rbd_rnea_grad_bpass_dq" : "rbd_rnea_grad_bpass_dqd", q && (!DQ || f) && df && dc,
                     rbdk::grad_bpass_kernel<T, DQ>, B, stream, q, f, df, use_damping, B, dc);
}
template <class T>
int minv_bpass_launch(const T* q, int64_t B, T* Minv, T* F, T* U, T* D, void* stream) {
  return pass_launch("rbd_minv_bpass", q && Minv && F && U && D, rbdk::minv_bpass_kernel<T>, B, stream, q, B, Minv, F, U, D);
}
template <class T>
int minv_fpass_launch(const T* q, int64_t B, T* Minv, T* F, const T* U, const T* D, void* stream) {
  return pass_launch("rbd_minv_fpass", q && Minv && F && U && D, rbdk::minv_fpass_kernel<T>, B, stream, q, B, Minv, F, U, D);
}
#endif  // RBD_NEED_PASS
}  // namespace

// =============================================================================================
// extern "C": the wrappers of a family and a precision (RBD_DEFS_*), and what stands in for them in a first-use family
// library (RBD_STUBS_*: -DRBD_TU_STUBS with -DRBD_STUB_<unit> per missing unit -- such a library holds COMMON, the units of
// one family and the stubs, so that it links and loads like a full library; an entry point of another family says so)
// =============================================================================================
extern "C" {
// every family unit answers for its own kernels (the selection lives there); rbd_kernel_name and
// rbd_minv_workspace_bytes of the COMMON unit ask it
#define RBD_DECLS_SELECTION(SFX)                                                                           \
  __attribute__((visibility("hidden"))) int rbd_rnea_kernel_name_##SFX(int64_t B, char* buf, size_t len);  \
  __attribute__((visibility("hidden"))) int rbd_grad_kernel_name_##SFX(int64_t B, char* buf, size_t len);  \
  __attribute__((visibility("hidden"))) int rbd_minv_kernel_name_##SFX(int64_t B, char* buf, size_t len);  \
  __attribute__((visibility("hidden"))) int rbd_minv_needs_ws_##SFX(int64_t B);
RBD_DECLS_SELECTION(f32)
RBD_DECLS_SELECTION(f64)
#undef RBD_DECLS_SELECTION

// an entry point that launches: on the stream's device for the duration of the call (rbd_host.h)
#define RBD_ENTER RbdStreamDevice sd_(stream); return
#define RBD_STUB_BODY(name) { return fail(RBD_ERR_NOT_BUILT, name ": not part of this family library (rbdreference_amd.build: first-use build)"); }

#define RBD_DEFS_RNEA(SFX, T)                                                                                                    \
  int rbd_rnea_kernel_name_##SFX(int64_t B, char* buf, size_t len) { return rnea_kernel_name<T>(B, buf, len); }                  \
  int rbd_rnea_##SFX(const T* q, const T* qd, const T* qdd, T gravity, int64_t B, T* c, T* v, T* a, T* f, void* stream) {        \
    RBD_ENTER rnea_launch<T>(q, qd, qdd, gravity, B, c, v, a, f, stream);                                                        \
  }                                                                                                                              \
  int rbd_rnea_fpass_##SFX(const T* q, const T* qd, const T* qdd, T gravity, int64_t B, T* v, T* a, T* f, void* stream) {        \
    RBD_ENTER rnea_launch<T>(q, qd, qdd, gravity, B, nullptr, v, a, f, stream, 1);                                               \
  }                                                                                                                              \
  int rbd_rnea_bpass_##SFX(const T* q, T* f, int64_t B, T* c, void* stream) { RBD_ENTER rnea_bpass_launch<T>(q, f, B, c, stream); }
#define RBD_STUBS_RNEA(SFX, T)                                                                                                   \
  int rbd_rnea_kernel_name_##SFX(int64_t, char*, size_t) RBD_STUB_BODY("rbd_kernel_name(RBD_OP_RNEA)")                           \
  int rbd_rnea_##SFX(const T*, const T*, const T*, T, int64_t, T*, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea")                  \
  int rbd_rnea_fpass_##SFX(const T*, const T*, const T*, T, int64_t, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_fpass")          \
  int rbd_rnea_bpass_##SFX(const T*, T*, int64_t, T*, void*) RBD_STUB_BODY("rbd_rnea_bpass")

#define RBD_DEFS_GRAD(SFX, T)                                                                                                    \
  int rbd_grad_kernel_name_##SFX(int64_t B, char* buf, size_t len) { return grad_kernel_name<T>(B, buf, len); }                  \
  int rbd_rnea_grad_##SFX(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B, T* c, T* dc_du,          \
                          void* stream) {                                                                                        \
    RBD_ENTER rnea_grad_launch<T>(q, qd, qdd, gravity, use_damping, B, c, dc_du, stream);                                        \
  }                                                                                                                              \
  int rbd_rnea_with_grad_##SFX(const T* q, const T* qd, const T* qdd, T gravity, int use_damping, int64_t B, T* c, T* v, T* a,   \
                               T* f, T* dc_du, void* stream) {                                                                   \
    RBD_ENTER rnea_with_grad_launch<T>(q, qd, qdd, gravity, use_damping, B, c, v, a, f, dc_du, stream);                          \
  }
#define RBD_STUBS_GRAD(SFX, T)                                                                                                   \
  int rbd_grad_kernel_name_##SFX(int64_t, char*, size_t) RBD_STUB_BODY("rbd_kernel_name(RBD_OP_RNEA_GRAD)")                      \
  int rbd_rnea_grad_##SFX(const T*, const T*, const T*, T, int, int64_t, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_grad")           \
  int rbd_rnea_with_grad_##SFX(const T*, const T*, const T*, T, int, int64_t, T*, T*, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_with_grad")

#define RBD_DEFS_GRADN(SFX, T)                                                                                                   \
  int rbd_grad_noqdd_##SFX(const T* q, const T* qd, T gravity, int use_damping, int64_t B, T* c, T* dc_du, void* stream) {       \
    RBD_ENTER rnea_grad_launch_q<T, false>(q, qd, nullptr, gravity, use_damping, B, c, dc_du, stream);                           \
  }                                                                                                                              \
  int rbd_grad_cols_noqdd_##SFX(const T* q, const T* qd, T gravity, int use_damping, int64_t B, T* c, T* v, T* a, T* f,          \
                                T* dc_du, void* stream) {                                                                        \
    RBD_ENTER grad_cols_launch<T, false>(q, qd, nullptr, gravity, use_damping, B, c, v, a, f, dc_du, stream);                    \
  }
#define RBD_STUBS_GRADN(SFX, T)                                                                                                  \
  int rbd_grad_noqdd_##SFX(const T*, const T*, T, int, int64_t, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_grad (qdd = NULL)")      \
  int rbd_grad_cols_noqdd_##SFX(const T*, const T*, T, int, int64_t, T*, T*, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_with_grad (qdd = NULL)")

#define RBD_DEFS_MINV(SFX, T)                                                                                                    \
  int rbd_minv_kernel_name_##SFX(int64_t B, char* buf, size_t len) { return minv_kernel_name<T>(B, buf, len); }                  \
  int rbd_minv_needs_ws_##SFX(int64_t B) { return minv_needs_workspace<T>(B); }                                                  \
  int rbd_crba_##SFX(const T* q, int64_t B, T* H, void* stream) { RBD_ENTER crba_launch<T>(q, B, H, stream); }                   \
  int rbd_minv_##SFX(const T* q, int64_t B, int output_dense, T* Minv, void* workspace, size_t workspace_bytes, void* stream) {  \
    RBD_ENTER minv_launch<T>(q, B, output_dense, Minv, workspace, workspace_bytes, stream);                                      \
  }                                                                                                                              \
  int rbd_minv_fd_##SFX(const T* q, int64_t B, T* Minv, void* workspace, size_t wsb, void* stream, const T* u, const T* c,       \
                        T* qdd, const T* qd, T gravity) {                                                                        \
    RBD_ENTER minv_launch<T>(q, B, 1, Minv, workspace, wsb, stream, u, c, qdd, qd, gravity);                                     \
  }
#define RBD_STUBS_MINV(SFX, T)                                                                                                   \
  int rbd_minv_kernel_name_##SFX(int64_t, char*, size_t) RBD_STUB_BODY("rbd_kernel_name(RBD_OP_MINV)")                           \
  int rbd_minv_needs_ws_##SFX(int64_t) { return 1; }                                                                             \
  int rbd_crba_##SFX(const T*, int64_t, T*, void*) RBD_STUB_BODY("rbd_crba")                                                     \
  int rbd_minv_##SFX(const T*, int64_t, int, T*, void*, size_t, void*) RBD_STUB_BODY("rbd_minv")                                 \
  int rbd_minv_fd_##SFX(const T*, int64_t, T*, void*, size_t, void*, const T*, const T*, T*, const T*, T) RBD_STUB_BODY("rbd_minv")

#define RBD_DEFS_FD(SFX, T)                                                                                                      \
  int rbd_aba_##SFX(const T* q, const T* qd, const T* tau, T gravity, int64_t B, T* qdd, void* stream) {                         \
    RBD_ENTER aba_launch<T>(q, qd, tau, gravity, B, qdd, stream);                                                                \
  }                                                                                                                              \
  int rbd_forward_dynamics_##SFX(const T* q, const T* qd, const T* u, T gravity, int64_t B, T* qdd, void* workspace,             \
                                 size_t workspace_bytes, void* stream) {                                                         \
    RBD_ENTER fd_launch<T>(q, qd, u, gravity, B, qdd, nullptr, false, workspace, workspace_bytes, stream);                       \
  }                                                                                                                              \
  int rbd_forward_dynamics_grad_##SFX(const T* q, const T* qd, const T* u, T gravity, int64_t B, T* qdd, T* dqdd_du,             \
                                      void* workspace, size_t workspace_bytes, void* stream) {                                   \
    RBD_ENTER fd_launch<T>(q, qd, u, gravity, B, qdd, dqdd_du, true, workspace, workspace_bytes, stream);                        \
  }
#define RBD_STUBS_FD(SFX, T)                                                                                                     \
  int rbd_aba_##SFX(const T*, const T*, const T*, T, int64_t, T*, void*) RBD_STUB_BODY("rbd_aba")                                \
  int rbd_forward_dynamics_##SFX(const T*, const T*, const T*, T, int64_t, T*, void*, size_t, void*) RBD_STUB_BODY("rbd_forward_dynamics") \
  int rbd_forward_dynamics_grad_##SFX(const T*, const T*, const T*, T, int64_t, T*, T*, void*, size_t, void*) RBD_STUB_BODY("rbd_forward_dynamics_grad")

#define RBD_DEFS_PASS(SFX, T)                                                                                                    \
  int rbd_rnea_grad_fpass_dq_##SFX(const T* q, const T* qd, const T* v, const T* a, T gravity, int64_t B, T* dv_dq, T* da_dq,    \
                                   T* df_dq, void* stream) {                                                                     \
    RBD_ENTER grad_fpass_launch<T, true>(q, qd, v, a, gravity, B, dv_dq, da_dq, df_dq, stream);                                  \
  }                                                                                                                              \
  int rbd_rnea_grad_fpass_dqd_##SFX(const T* q, const T* qd, const T* v, int64_t B, T* dv_dqd, T* da_dqd, T* df_dqd,             \
                                    void* stream) {                                                                              \
    RBD_ENTER grad_fpass_launch<T, false>(q, qd, v, nullptr, T(0), B, dv_dqd, da_dqd, df_dqd, stream);                           \
  }                                                                                                                              \
  int rbd_rnea_grad_bpass_dq_##SFX(const T* q, const T* f, T* df_dq, int64_t B, T* dc_dq, void* stream) {                        \
    RBD_ENTER grad_bpass_launch<T, true>(q, f, df_dq, 0, B, dc_dq, stream);                                                      \
  }                                                                                                                              \
  int rbd_rnea_grad_bpass_dqd_##SFX(const T* q, T* df_dqd, int use_damping, int64_t B, T* dc_dqd, void* stream) {                \
    RBD_ENTER grad_bpass_launch<T, false>(q, nullptr, df_dqd, use_damping, B, dc_dqd, stream);                                   \
  }                                                                                                                              \
  int rbd_minv_bpass_##SFX(const T* q, int64_t B, T* Minv, T* F, T* U, T* Dinv, void* stream) {                                  \
    RBD_ENTER minv_bpass_launch<T>(q, B, Minv, F, U, Dinv, stream);                                                              \
  }                                                                                                                              \
  int rbd_minv_fpass_##SFX(const T* q, int64_t B, T* Minv, T* F, const T* U, const T* Dinv, void* stream) {                      \
    RBD_ENTER minv_fpass_launch<T>(q, B, Minv, F, U, Dinv, stream);                                                              \
  }
#define RBD_STUBS_PASS(SFX, T)                                                                                                   \
  int rbd_rnea_grad_fpass_dq_##SFX(const T*, const T*, const T*, const T*, T, int64_t, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_grad_fpass_dq") \
  int rbd_rnea_grad_fpass_dqd_##SFX(const T*, const T*, const T*, int64_t, T*, T*, T*, void*) RBD_STUB_BODY("rbd_rnea_grad_fpass_dqd") \
  int rbd_rnea_grad_bpass_dq_##SFX(const T*, const T*, T*, int64_t, T*, void*) RBD_STUB_BODY("rbd_rnea_grad_bpass_dq")           \
  int rbd_rnea_grad_bpass_dqd_##SFX(const T*, T*, int, int64_t, T*, void*) RBD_STUB_BODY("rbd_rnea_grad_bpass_dqd")              \
  int rbd_minv_bpass_##SFX(const T*, int64_t, T*, T*, T*, T*, void*) RBD_STUB_BODY("rbd_minv_bpass")                             \
  int rbd_minv_fpass_##SFX(const T*, int64_t, T*, T*, const T*, const T*, void*) RBD_STUB_BODY("rbd_minv_fpass")

#define RBD_DEFS_EE(SFX, T)                                                                                                      \
  int rbd_ee_pose_##SFX(const T* q, int64_t B, const int32_t* site_body, const double* site_T, const double* offset,             \
                        int n_sites, T* pose, T* dpose, void* stream) {                                                          \
    RBD_ENTER ee_launch<T>(q, B, site_body, site_T, offset, n_sites, pose, dpose, stream);                                       \
  }
#define RBD_STUBS_EE(SFX, T)                                                                                                     \
  int rbd_ee_pose_##SFX(const T*, int64_t, const int32_t*, const double*, const double*, int, T*, T*, void*) RBD_STUB_BODY("rbd_ee_pose")

#define RBD_DEFS_SO(SFX, T)                                                                                                      \
  int rbd_second_order_idsva_##SFX(const T* q, const T* qd, const T* qdd, T gravity, int64_t B, T* out, void* stream) {          \
    RBD_ENTER so_launch<T>(q, qd, qdd, gravity, B, out, stream);                                                                 \
  }
#define RBD_STUBS_SO(SFX, T)                                                                                                     \
  int rbd_second_order_idsva_##SFX(const T*, const T*, const T*, T, int64_t, T*, void*) RBD_STUB_BODY("rbd_second_order_idsva")

#define RBD_DEFS_FDSO(SFX, T)                                                                                                    \
  int rbd_fdsva_so_##SFX(const T* q, const T* qd, const T* u, T gravity, int64_t B, T* out, void* ws, size_t ws_bytes,           \
                         void* stream) {                                                                                         \
    RBD_ENTER fdso_launch<T>(q, qd, u, gravity, B, out, ws, ws_bytes, stream);                                                   \
  }
#define RBD_STUBS_FDSO(SFX, T)                                                                                                   \
  int rbd_fdsva_so_##SFX(const T*, const T*, const T*, T, int64_t, T*, void*, size_t, void*) RBD_STUB_BODY("rbd_fdsva_so")

#define RBD_DEFS_ROLL(SFX, T)                                                                                                    \
  int rbd_rollout_##SFX(const T* q0, const T* qd0, const T* u, int u_shared, T dt, T gravity, int integrator, int64_t B,         \
                        int64_t steps, T* q_out, T* qd_out, int trajectory, void* stream) {                                      \
    RBD_ENTER rollout_launch<T>(q0, qd0, u, u_shared, dt, gravity, integrator, B, steps, q_out, qd_out, trajectory, stream);     \
  }
#define RBD_STUBS_ROLL(SFX, T)                                                                                                   \
  int rbd_rollout_##SFX(const T*, const T*, const T*, int, T, T, int, int64_t, int64_t, T*, T*, int, void*) RBD_STUB_BODY("rbd_rollout")

#define RBD_DEFS_ROLLCL(SFX, T)                                                                                                  \
  int rbd_rollout_closed_loop_##SFX(const T* q0, const T* qd0, const T* u, const T* k, const T* K, const T* q0_ref,              \
                                    const T* qd0_ref, const T* q_ref, const T* qd_ref, const T* alpha, const T* u_lo,            \
                                    const T* u_hi, T dt, T gravity, int integrator, int64_t B, int64_t B_nom, int64_t steps,     \
                                    T* q_out, T* qd_out, int trajectory, T* u_out, void* stream) {                               \
    RBD_ENTER rollout_cl_launch<T>(q0, qd0, u, k, K, q0_ref, qd0_ref, q_ref, qd_ref, alpha, u_lo, u_hi, dt, gravity, integrator, \
                                   B, B_nom, steps, q_out, qd_out, trajectory, u_out, stream);                                   \
  }
#define RBD_STUBS_ROLLCL(SFX, T)                                                                                                 \
  int rbd_rollout_closed_loop_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*,    \
                                    const T*, const T*, const T*, T, T, int, int64_t, int64_t, int64_t, T*, T*, int, T*, void*)  \
      RBD_STUB_BODY("rbd_rollout_closed_loop")

#define RBD_DEFS_ROLLCOST(SFX, T)                                                                                                \
  int rbd_rollout_cost_##SFX(const T* q0, const T* qd0, const T* u, const T* k, const T* K, const T* q0_ref, const T* qd0_ref,   \
                             const T* q_ref, const T* qd_ref, const T* alpha, const T* du, const T* u_lo, const T* u_hi,         \
                             const T* q_tgt, const T* qd_tgt, const T* w_q, const T* w_qd, int x_final_only, const T* w_u,       \
                             const T* c_u, T dt, T gravity, int integrator, int64_t B, int64_t B_nom, int64_t steps, T* cost,    \
                             T* q_out, T* qd_out, int trajectory, T* u_out, void* stream) {                                      \
    RBD_ENTER rollout_cost_launch<T>(q0, qd0, u, k, K, q0_ref, qd0_ref, q_ref, qd_ref, alpha, du, u_lo, u_hi, q_tgt, qd_tgt,     \
                                     w_q, w_qd, x_final_only, w_u, c_u, dt, gravity, integrator, B, B_nom, steps, cost, q_out,   \
                                     qd_out, trajectory, u_out, stream);                                                         \
  }
#define RBD_STUBS_ROLLCOST(SFX, T)                                                                                               \
  int rbd_rollout_cost_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, \
                             const T*, const T*, const T*, const T*, const T*, const T*, const T*, int, const T*, const T*, T,   \
                             T, int, int64_t, int64_t, int64_t, T*, T*, T*, int, T*, void*) RBD_STUB_BODY("rbd_rollout_cost")

#define RBD_DEFS_MPPI(SFX, T)                                                                                                    \
  int rbd_mppi_update_##SFX(const T* J, const T* du, const T* u, const T* lam, const T* u_lo, const T* u_hi, int64_t S,          \
                            int64_t P, int64_t steps, T* u_out, T* w_out, T* ess_out, int32_t* status_out, void* ws,             \
                            size_t ws_bytes, void* stream) {                                                                     \
    RBD_ENTER mppi_launch<T>(J, du, u, lam, u_lo, u_hi, S, P, steps, u_out, w_out, ess_out, status_out, ws, ws_bytes, stream);   \
  }
#define RBD_STUBS_MPPI(SFX, T)                                                                                                   \
  int rbd_mppi_update_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, int64_t, int64_t, int64_t, T*, T*, T*,   \
                            int32_t*, void*, size_t, void*) RBD_STUB_BODY("rbd_mppi_update")

#define RBD_DEFS_ROLLG(SFX, T)                                                                                           \
  int rbd_rollout_adjoint_##SFX(const T* dc_du, const T* Minv, const T* gq, const T* gqd, int g_final_only, T dt, int integrator, \
                                int64_t B, int64_t steps, T* lam, T* grad_u, void* stream) {                                     \
    RBD_ENTER rollout_adjoint_launch<T>(dc_du, Minv, gq, gqd, g_final_only, dt, integrator, B, steps, lam, grad_u, stream);      \
  }                                                                                                                              \
  int rbd_rollout_grad_##SFX(const T* q0, const T* qd0, const T* u, const T* q_traj, const T* qd_traj, const T* gq,              \
                             const T* gqd, int g_final_only, T dt, T gravity, int integrator, int64_t B, int64_t steps,          \
                             T* grad_u, T* grad_q0, T* grad_qd0, void* ws, size_t ws_bytes, void* stream) {                      \
    RBD_ENTER rollout_grad_launch<T>(q0, qd0, u, q_traj, qd_traj, gq, gqd, g_final_only, dt, gravity, integrator, B, steps,      \
                                     grad_u, grad_q0, grad_qd0, ws, ws_bytes, stream);                                           \
  }
#define RBD_STUBS_ROLLG(SFX, T)                                                                                                  \
  int rbd_rollout_adjoint_##SFX(const T*, const T*, const T*, const T*, int, T, int, int64_t, int64_t, T*, T*, void*)            \
      RBD_STUB_BODY("rbd_rollout_adjoint")                                                                                       \
  int rbd_rollout_grad_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, const T*, int, T, T, int, int64_t,      \
                             int64_t, T*, T*, T*, void*, size_t, void*) RBD_STUB_BODY("rbd_rollout_grad")

#define RBD_DEFS_LQR(SFX, T)                                                                                                     \
  int rbd_rollout_riccati_##SFX(const T* dc_du, const T* Minv, const T* gq, const T* gqd, const T* hq, const T* hqd,             \
                                int x_final_only, const T* gu, const T* hu, int hu_shared, T reg, T dt, int integrator,          \
                                int64_t B, int64_t steps, T* lam, T* P, T* dV, int32_t* status, T* k, T* K, void* stream) {      \
    RBD_ENTER rollout_riccati_launch<T>(dc_du, Minv, gq, gqd, hq, hqd, x_final_only, gu, hu, hu_shared, reg, dt, integrator, B,  \
                                        steps, lam, P, dV, status, k, K, stream);                                                \
  }                                                                                                                              \
  int rbd_rollout_lqr_##SFX(const T* q0, const T* qd0, const T* u, const T* q_traj, const T* qd_traj, const T* gq, const T* gqd, \
                            const T* hq, const T* hqd, int x_final_only, const T* gu, const T* hu, int hu_shared, T reg, T dt,   \
                            T gravity, int integrator, int64_t B, int64_t steps, T* k, T* K, T* lam, T* P, T* dV,                \
                            int32_t* status, void* ws, size_t ws_bytes, void* stream) {                                          \
    RBD_ENTER rollout_lqr_launch<T>(q0, qd0, u, q_traj, qd_traj, gq, gqd, hq, hqd, x_final_only, gu, hu, hu_shared, reg, dt,     \
                                    gravity, integrator, B, steps, k, K, lam, P, dV, status, ws, ws_bytes, stream);              \
  }
#define RBD_STUBS_LQR(SFX, T)                                                                                                    \
  int rbd_rollout_riccati_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, int, const T*, const T*, int, T, T,  \
                                int, int64_t, int64_t, T*, T*, T*, int32_t*, T*, T*, void*) RBD_STUB_BODY("rbd_rollout_riccati") \
  int rbd_rollout_lqr_##SFX(const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, const T*, int,       \
                            const T*, const T*, int, T, T, T, int, int64_t, int64_t, T*, T*, T*, T*, T*, int32_t*, void*, size_t, \
                            void*) RBD_STUB_BODY("rbd_rollout_lqr")

#if defined(RBD_TU_RNEA_F32)
RBD_DEFS_RNEA(f32, float)
#elif defined(RBD_STUB_RNEA_F32)
RBD_STUBS_RNEA(f32, float)
#endif
#if defined(RBD_TU_RNEA_F64)
RBD_DEFS_RNEA(f64, double)
#elif defined(RBD_STUB_RNEA_F64)
RBD_STUBS_RNEA(f64, double)
#endif
#if defined(RBD_TU_GRAD_F32)
RBD_DEFS_GRAD(f32, float)
#elif defined(RBD_STUB_GRAD_F32)
RBD_STUBS_GRAD(f32, float)
#endif
#if defined(RBD_TU_GRAD_F64)
RBD_DEFS_GRAD(f64, double)
#elif defined(RBD_STUB_GRAD_F64)
RBD_STUBS_GRAD(f64, double)
#endif
#if defined(RBD_TU_GRADN_F32)
RBD_DEFS_GRADN(f32, float)
#elif defined(RBD_STUB_GRADN_F32)
RBD_STUBS_GRADN(f32, float)
#endif
#if defined(RBD_TU_GRADN_F64)
RBD_DEFS_GRADN(f64, double)
#elif defined(RBD_STUB_GRADN_F64)
RBD_STUBS_GRADN(f64, double)
#endif
#if defined(RBD_TU_MINV_F32)
RBD_DEFS_MINV(f32, float)
#elif defined(RBD_STUB_MINV_F32)
RBD_STUBS_MINV(f32, float)
#endif
#if defined(RBD_TU_MINV_F64)
RBD_DEFS_MINV(f64, double)
#elif defined(RBD_STUB_MINV_F64)
RBD_STUBS_MINV(f64, double)
#endif
#if defined(RBD_TU_FD_F32)
RBD_DEFS_FD(f32, float)
#elif defined(RBD_STUB_FD_F32)
RBD_STUBS_FD(f32, float)
#endif
#if defined(RBD_TU_FD_F64)
RBD_DEFS_FD(f64, double)
#elif defined(RBD_STUB_FD_F64)
RBD_STUBS_FD(f64, double)
#endif
#if defined(RBD_TU_PASS_F32)
RBD_DEFS_PASS(f32, float)
#elif defined(RBD_STUB_PASS_F32)
RBD_STUBS_PASS(f32, float)
#endif
#if defined(RBD_TU_PASS_F64)
RBD_DEFS_PASS(f64, double)
#elif defined(RBD_STUB_PASS_F64)
RBD_STUBS_PASS(f64, double)
#endif
#if defined(RBD_TU_EE_F32)
RBD_DEFS_EE(f32, float)
#elif defined(RBD_STUB_EE_F32)
RBD_STUBS_EE(f32, float)
#endif
#if defined(RBD_TU_EE_F64)
RBD_DEFS_EE(f64, double)
#elif defined(RBD_STUB_EE_F64)
RBD_STUBS_EE(f64, double)
#endif
#if defined(RBD_TU_SO_F32)
RBD_DEFS_SO(f32, float)
#elif defined(RBD_STUB_SO_F32)
RBD_STUBS_SO(f32, float)
#endif
#if defined(RBD_TU_SO_F64)
RBD_DEFS_SO(f64, double)
#elif defined(RBD_STUB_SO_F64)
RBD_STUBS_SO(f64, double)
#endif
#if defined(RBD_TU_FDSO_F32)
RBD_DEFS_FDSO(f32, float)
#elif defined(RBD_STUB_FDSO_F32)
RBD_STUBS_FDSO(f32, float)
#endif
#if defined(RBD_TU_FDSO_F64)
RBD_DEFS_FDSO(f64, double)
#elif defined(RBD_STUB_FDSO_F64)
RBD_STUBS_FDSO(f64, double)
#endif
#if defined(RBD_TU_ROLL_F32)
RBD_DEFS_ROLL(f32, float)
#elif defined(RBD_STUB_ROLL_F32)
RBD_STUBS_ROLL(f32, float)
#endif
#if defined(RBD_TU_ROLL_F64)
RBD_DEFS_ROLL(f64, double)
#elif defined(RBD_STUB_ROLL_F64)
RBD_STUBS_ROLL(f64, double)
#endif

#if defined(RBD_TU_ROLLCL_F32)
RBD_DEFS_ROLLCL(f32, float)
#elif defined(RBD_STUB_ROLLCL_F32)
RBD_STUBS_ROLLCL(f32, float)
#endif
#if defined(RBD_TU_ROLLCL_F64)
RBD_DEFS_ROLLCL(f64, double)
#elif defined(RBD_STUB_ROLLCL_F64)
RBD_STUBS_ROLLCL(f64, double)
#endif

#if defined(RBD_TU_ROLLCOST_F32)
RBD_DEFS_ROLLCOST(f32, float)
#elif defined(RBD_STUB_ROLLCOST_F32)
RBD_STUBS_ROLLCOST(f32, float)
#endif
#if defined(RBD_TU_ROLLCOST_F64)
RBD_DEFS_ROLLCOST(f64, double)
#elif defined(RBD_STUB_ROLLCOST_F64)
RBD_STUBS_ROLLCOST(f64, double)
#endif

#if defined(RBD_TU_MPPI_F32)
RBD_DEFS_MPPI(f32, float)
#elif defined(RBD_STUB_MPPI_F32)
RBD_STUBS_MPPI(f32, float)
#endif
#if defined(RBD_TU_MPPI_F64)
RBD_DEFS_MPPI(f64, double)
#elif defined(RBD_STUB_MPPI_F64)
RBD_STUBS_MPPI(f64, double)
#endif

#if defined(RBD_TU_ROLLG_F32)
RBD_DEFS_ROLLG(f32, float)
#elif defined(RBD_STUB_ROLLG_F32)
RBD_STUBS_ROLLG(f32, float)
#endif
#if defined(RBD_TU_ROLLG_F64)
RBD_DEFS_ROLLG(f64, double)
#elif defined(RBD_STUB_ROLLG_F64)
RBD_STUBS_ROLLG(f64, double)
#endif

#if defined(RBD_TU_LQR_F32)
RBD_DEFS_LQR(f32, float)
#elif defined(RBD_STUB_LQR_F32)
RBD_STUBS_LQR(f32, float)
#endif
#if defined(RBD_TU_LQR_F64)
RBD_DEFS_LQR(f64, double)
#elif defined(RBD_STUB_LQR_F64)
RBD_STUBS_LQR(f64, double)
#endif

#ifdef RBD_TU_COMMON
int rbd_abi_version(void) { return RBD_ABI_VERSION; }
const char* rbd_last_error(void) { return rbd_err_buf(); }

int rbd_set_option(int option, int value) {
  std::atomic<int>* s = rbd_option_slot(option);
  if (!s) return fail(RBD_ERR_ARG, "rbd_set_option: unknown option");
  if (value < 0 || (option != RBD_OPT_SELECT_BATCH && value > (option == RBD_OPT_RNEA_KERNEL ? 2 : 3)))
    return fail(RBD_ERR_ARG, "rbd_set_option: value out of range");
  s->store(value, std::memory_order_relaxed);
  return 0;
}
int rbd_get_option(int option) {
  std::atomic<int>* s = rbd_option_slot(option);
  return s ? s->load(std::memory_order_relaxed) : RBD_ERR_ARG;
}
int rbd_kernel_name(int op, int elem_size, int64_t B, char* buf, size_t len) {
  if (!buf || len == 0 || (elem_size != 4 && elem_size != 8)) return fail(RBD_ERR_ARG, "rbd_kernel_name: bad arguments");
  switch (op) {
    case RBD_OP_RNEA:
      return elem_size == 4 ? rbd_rnea_kernel_name_f32(B, buf, len) : rbd_rnea_kernel_name_f64(B, buf, len);
    case RBD_OP_RNEA_GRAD:
      return elem_size == 4 ? rbd_grad_kernel_name_f32(B, buf, len) : rbd_grad_kernel_name_f64(B, buf, len);
    case RBD_OP_MINV:
      return elem_size == 4 ? rbd_minv_kernel_name_f32(B, buf, len) : rbd_minv_kernel_name_f64(B, buf, len);
    default:
      return fail(RBD_ERR_ARG, "rbd_kernel_name: unknown op");
  }
}

int rbd_model_info(rbd_model_info_t* out) {
  if (!out) return fail(RBD_ERR_ARG, "rbd_model_info: out is null");
  std::memset(out, 0, sizeof(*out));
  out->abi_version = RBD_ABI_VERSION;
  out->n = rbdm::N;
  out->max_depth = rbdm::MAXDEPTH;
  out->hash = RBD_MODEL_HASH;
  out->floating_base = rbdm::FLOATING_BASE ? 1 : 0;
  out->nv = rbdm::NV;
  std::snprintf(out->name, sizeof(out->name), "%s", RBD_MODEL_NAME);
  for (int i = 0; i < rbdm::N && i < RBD_MAX_BODIES; ++i) {
    out->parent[i] = rbdm::PARENT[i];
    out->joint_type[i] = rbdm::JTYPE[i];
    out->joint_axis[i] = rbdm::AXIS[i];
  }
  return 0;
}
size_t rbd_minv_workspace_bytes(int64_t B, int elem_size) {
  if (B <= 0 || (elem_size != 4 && elem_size != 8)) return 0;
  if (rbdm::FLOATING_BASE) return 0;
  // none when the kernel selected by the current RBD_OPT_MINV_PHASE_A runs without it (the one-lane kernel, the
  // one-launch kernel): query again after changing that option
  if (!(elem_size == 4 ? rbd_minv_needs_ws_f32(B) : rbd_minv_needs_ws_f64(B))) return 0;
  return (size_t)B * rbdk::MINV_WS_PER_CFG * (size_t)elem_size;
}
size_t rbd_fd_workspace_bytes(int64_t B, int elem_size) {
  if (B <= 0) return 0;
  if (rbdm::FLOATING_BASE) {      // c [B, NV] | Minv [B, NV, NV] | qdd [B, NV] | dc_du [B, NV, 2 NV]  (rbd_fb_kernels.hip; the
    if (elem_size != 4 && elem_size != 8) return 0;   // last two serve forward_dynamics_grad only)
    return align16((size_t)B * rbdm::NV * elem_size) + align16((size_t)B * rbdm::NV * rbdm::NV * elem_size) +
           align16((size_t)B * rbdm::NV * elem_size) + align16((size_t)B * rbdm::NV * 2 * rbdm::NV * elem_size);
  }
  if (elem_size == 4) return FdWorkspace<float>(B).total;
  if (elem_size == 8) return FdWorkspace<double>(B).total;
  return 0;
}
size_t rbd_fdsva_so_workspace_bytes(int64_t B, int elem_size) {
  if (B <= 0 || rbdm::FLOATING_BASE || B > fdso_max_batch()) return 0;
  if (elem_size == 4) return FdsoWorkspace<float>(B).total;
  if (elem_size == 8) return FdsoWorkspace<double>(B).total;
  return 0;
}
size_t rbd_rollout_grad_workspace_bytes(int64_t B, int64_t Tc, int elem_size) {
  if (B <= 0 || Tc <= 0 || rbdm::FLOATING_BASE || B > ROLLG_MAX_ROWS || Tc > ROLLG_MAX_ROWS / B) return 0;
  if (elem_size == 4) return RollgWorkspace<float>(B, Tc).total;
  if (elem_size == 8) return RollgWorkspace<double>(B, Tc).total;
  return 0;
}
size_t rbd_rollout_lqr_workspace_bytes(int64_t B, int64_t Tc, int elem_size) {
  if (B <= 0 || Tc <= 0 || rbdm::FLOATING_BASE || B > LQR_MAX_ROWS || Tc > LQR_MAX_ROWS / B) return 0;
  if (elem_size == 4) return LqrWorkspace<float>(B, Tc).total;
  if (elem_size == 8) return LqrWorkspace<double>(B, Tc).total;
  return 0;
}
size_t rbd_mppi_update_workspace_bytes(int64_t S, int64_t P, int64_t T, int elem_size) {
  if (S <= 0 || P <= 0 || T <= 0 || rbdm::FLOATING_BASE || (elem_size != 4 && elem_size != 8) || !mppi_sizes_ok(S, P, T)) return 0;
  return MppiWorkspace(S, P, T, (size_t)elem_size).total;
}
#endif  // RBD_TU_COMMON
}  // extern "C"
