// rbd_ws_pool.h -- the library-owned workspace pool behind rbd_stream_workspace / rbd_release_workspaces.  One pool per
// library, owned by (and only included in) the COMMON unit.
//
// Library-owned scratch of the workspace gradient kernel (rbd_idsva_tree_ws.h): one buffer per (device, stream), keyed
// by the STREAM's device (hipStreamGetDevice; the null stream belongs to the calling thread's current device).
// Launches on one stream are ordered and share it; launches on different streams get different buffers.
// Lifetime rule: a buffer that was ever handed out is NEVER freed or moved by a later call -- launches in flight, bound
// launches and captured hipGraphs may hold its address.  The callers ask for a size that depends on the kernel's
// occupancy, not on B, so a (device, stream) normally sees one allocation; should a later call need more (another
// kernel of the library), a larger buffer is allocated NEXT TO the old one, which is retired, not released.  Only
// rbd_release_workspaces() frees (after hipDeviceSynchronize, by contract with no call of this library in flight and
// no graph that contains one still alive).  The first call on a stream allocates (hipMalloc is not capturable: run a
// call once before capturing it into a graph, as for every kernel that needs the dynamic-LDS attribute set); no call ever
// synchronises the device.
#pragma once
#include "rbd_host.h"
#include <vector>

namespace {
struct RbdWsBuf { void* p = nullptr; size_t n = 0; };
struct RbdWsEntry { RbdWsBuf cur; std::vector<RbdWsBuf> retired; };
std::mutex& rbd_ws_mutex() { static std::mutex mu; return mu; }
std::unordered_map<const void*, RbdWsEntry>* rbd_ws_pool() {
  static std::unordered_map<const void*, RbdWsEntry> pool[RBD_MAX_DEVICES];
  return pool;
}
int rbd_ws_device_of(void* stream, int* dev) {
  int d = 0;
  hipError_t e = stream ? hipStreamGetDevice((hipStream_t)stream, &d) : hipGetDevice(&d);
  if (e != hipSuccess) { (void)hipGetLastError(); e = hipGetDevice(&d); }
  if (e != hipSuccess) return (int)e;
  *dev = d;
  return 0;
}
}  // namespace
extern "C" int rbd_stream_workspace(void* stream, size_t bytes, void** out) {
  int dev = 0;
  if (rbd_ws_device_of(stream, &dev) != 0) return hip_fail(hipErrorInvalidDevice, "rbd workspace: device of the stream");
  if (dev < 0 || dev >= RBD_MAX_DEVICES) return fail(RBD_ERR_UNSUPPORTED, "rbd workspace: device index beyond RBD_MAX_DEVICES");
  std::lock_guard<std::mutex> g(rbd_ws_mutex());
  RbdWsEntry& en = rbd_ws_pool()[dev][stream];
  if (en.cur.n < bytes) {
    int cur_dev = dev;
    (void)hipGetDevice(&cur_dev);
    if (cur_dev != dev) (void)hipSetDevice(dev);            // allocate on the stream's device
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (cur_dev != dev) (void)hipSetDevice(cur_dev);
    if (e != hipSuccess) return hip_fail(e, "rbd workspace hipMalloc");
    if (en.cur.p) en.retired.push_back(en.cur);               // may still be referenced: kept, not freed
    en.cur.p = p;
    en.cur.n = bytes;
  }
  *out = en.cur.p;
  return 0;
}
extern "C" int rbd_release_workspaces(void) {
  std::lock_guard<std::mutex> g(rbd_ws_mutex());
  int cur_dev = 0;
  const bool have_dev = hipGetDevice(&cur_dev) == hipSuccess;
  if (!have_dev) (void)hipGetLastError();
  int rc = 0;
  for (int dev = 0; dev < RBD_MAX_DEVICES; ++dev) {
    auto& m = rbd_ws_pool()[dev];
    if (m.empty()) continue;
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess && rc == 0) rc = hip_fail(e, "rbd_release_workspaces: hipDeviceSynchronize");
    for (auto& kv : m) {
      if (kv.second.cur.p) (void)hipFree(kv.second.cur.p);
      for (auto& b : kv.second.retired) (void)hipFree(b.p);
    }
    m.clear();
  }
  if (have_dev) (void)hipSetDevice(cur_dev);
  return rc;
}
