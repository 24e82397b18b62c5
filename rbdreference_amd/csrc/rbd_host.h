// rbd_host.h -- host-side helpers shared by the translation units of a per-robot library (rbd_kernels.hip,
// rbd_fb_kernels.hip): error reporting, options, argument checks and the one launch path.  No device code, header-only,
// no allocation on the launch path.  Everything here has internal linkage: a library exports its C-ABI and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rbd_hip.h"
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <unordered_map>

constexpr int RBD_MAX_DEVICES = 16;
constexpr size_t RBD_ERR_LEN = 512;
// one instance each, owned by the COMMON unit: the thread-local message buffer behind rbd_last_error(), the tuning
// options of rbd_set_option (rbd_capi.h) and the workspace pool (rbd_ws_pool.h)
extern "C" __attribute__((visibility("hidden"))) char* rbd_err_buf(void);
extern "C" __attribute__((visibility("hidden"))) std::atomic<int>* rbd_option_slot(int option);
extern "C" __attribute__((visibility("hidden"))) int rbd_stream_workspace(void* stream, size_t bytes, void** out);

// Every C-ABI entry point that launches runs on the STREAM's device: if the calling thread's current device is another
// one, it is switched for the duration of the call and restored afterwards.  Everything the launchers cache per device
// (dynamic-LDS attributes, resident-block counts, the library-owned workspace of rbd_stream_workspace) is therefore
// keyed by the device the kernels actually run on, not by whatever device the thread happened to have selected
// (VERDICT r3 item 9).  The null stream IS the current device's stream: no HIP call at all is made for it, so the
// argument checks of the entry points still run on a machine without a GPU.
struct RbdStreamDevice {
  int prev = -1;
  explicit RbdStreamDevice(void* stream) {
    if (!stream) return;
    int cur = 0, dev = 0;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (dev != cur && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~RbdStreamDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  RbdStreamDevice(const RbdStreamDevice&) = delete;
  RbdStreamDevice& operator=(const RbdStreamDevice&) = delete;
};

// Store policy of the chain gradient kernels (rbd_spatial.h, store16; RBD_OPT_STORE_POLICY).  Their rows are written once
// and never read back by the launch.  Left as plain stores they wait, dirty, in L2 -- up to all of it -- for the release at
// the end of the launch; written through they leave as they are produced.  AUTO goes by the bytes the launch writes
// (measured on the 7-DoF arm, profiles/store_policy.txt):
//   <= 4 MiB      plain: the launch gains 0.15 us of 10.8 from writing through, and the result stays in L2 for its consumer
//   <= 64 MiB     write-through (`sc1`): 1.1 us of 12.6 at 13 MiB, 1.1 us of 20.0 at 52 MiB
//   above         write-through, non-temporal (`sc1 nt`): 3.4 us of 36.2 at 105 MiB, 3.7 us of 129.8 at 420 MiB, where
//                 `sc1` alone gains 1.2 and 2.9 (and is the better one at 52 MiB: 18.9 against 19.8 us)
// Returns the flavour (RBD_STORE_PLAIN / _WT / _WT_NT); `policy` is the option's value.
constexpr size_t RBD_STORE_WT_MIN_BYTES = (size_t)4 << 20, RBD_STORE_NT_MIN_BYTES = (size_t)64 << 20;
inline int rbd_store_flavour(int policy, size_t out_bytes) {
  if (policy != 0) return policy - 1;        // RBD_STORE_POLICY_PLAIN, _WRITE_THROUGH, _WRITE_THROUGH_NT
  return out_bytes > RBD_STORE_NT_MIN_BYTES ? 2 : out_bytes > RBD_STORE_WT_MIN_BYTES ? 1 : 0;
}

namespace {
constexpr size_t LDS_MAX = 160 * 1024;      // LDS of a CU: what a block may ask for
template <class T>
constexpr const char* type_name() { return sizeof(T) == 4 ? "float" : "double"; }   // as rbd_kernel_name spells T

// ---- errors: the message goes to rbd_last_error(), the code to the caller ---------------------------------------------
__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(rbd_err_buf(), RBD_ERR_LEN, fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t e, const char* where) {
  fail(0, "%s: %s", where, hipGetErrorString(e));
  return (int)e > 0 ? (int)e : 1;
}

// ---- options (relaxed atomics: an option only ever selects between kernels that compute the same result) -------------
int rbd_option(int option) { return rbd_option_slot(option)->load(std::memory_order_relaxed); }
// the batch size kernel selection looks at: the call's own, unless the caller has declared the global batch it is a shard of
int64_t rbd_select_batch(int64_t B) {
  const int g = rbd_option(RBD_OPT_SELECT_BATCH);
  return g > 0 ? (int64_t)g : B;
}

// ---- argument checks --------------------------------------------------------------------------------------------------
constexpr size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// is any of these pointers not 16-byte aligned?  (null counts as aligned: optional outputs)
template <class... P>
bool misaligned(const P*... p) { return ((... | reinterpret_cast<uintptr_t>(p)) & 15u) != 0; }
// a block count as a grid dimension
int checked_grid(int64_t blocks, const char* who, unsigned* grid) {
  if (blocks > 0x7fffffffLL) return fail(RBD_ERR_ARG, "%s: B too large", who);
  *grid = (unsigned)blocks;
  return 0;
}
// the grid that covers B rows with `rows` of them per block
int grid_for(int64_t B, int64_t rows, const char* who, unsigned* grid) { return checked_grid((B + rows - 1) / rows, who, grid); }

// ---- per-kernel, per-device facts ---------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is needed once per kernel (and device), not per
// launch: the granted sizes are remembered.
template <class K>
int ensure_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return 0;
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> granted[RBD_MAX_DEVICES];
  int dev = 0;
  (void)hipGetDevice(&dev);
  const void* key = reinterpret_cast<const void*>(kernel);
  const int slot = dev >= 0 && dev < RBD_MAX_DEVICES ? dev : 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = granted[slot].find(key);
    if (it != granted[slot].end() && it->second >= bytes) return 0;
  }
  hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
  std::lock_guard<std::mutex> g(mu);
  granted[slot][key] = bytes;
  return 0;
}

// Blocks of `threads` threads and `lds` bytes that are resident at once on the current device
// (occupancy per CU x CUs), remembered per kernel and device: the grid of the tile-walking kernels.
template <class K>
int resident_blocks(K kernel, int threads, size_t lds, int* out) {
  static std::mutex mu;
  static std::unordered_map<const void*, int> known[RBD_MAX_DEVICES];
  int dev = 0;
  (void)hipGetDevice(&dev);
  const void* key = reinterpret_cast<const void*>(kernel);
  const int slot = dev >= 0 && dev < RBD_MAX_DEVICES ? dev : 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = known[slot].find(key);
    if (it != known[slot].end()) { *out = it->second; return 0; }
  }
  int per_cu = 0, cus = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
  if (e != hipSuccess) return hip_fail(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute(MultiprocessorCount)");
  const int n = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
  std::lock_guard<std::mutex> g(mu);
  known[slot][key] = n;
  *out = n;
  return 0;
}

// ---- the launch path ----------------------------------------------------------------------------------------------------
// LDS attribute, launch, error check; `who` names the launch in the message.  The argument types come from the kernel's
// own signature, not from the arguments: call sites pass nullptr and int64_t as they are, and a wrong argument does not compile.
template <class X>
struct rbd_as_declared { using type = X; };
template <class... P>
int launch(const char* who, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, void* stream,
           typename rbd_as_declared<P>::type... args) {
  if (int rc = ensure_lds(kernel, lds)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, who);
}

// a run-time flag as a compile-time one: with_bool(qdd != nullptr, [&](auto HQ) { ... kernel<T, decltype(HQ)::value> ... })
template <class F>
auto with_bool(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
}  // namespace
