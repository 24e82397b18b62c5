// rbd_fdsva_so.h -- the contraction that closes RBDReference.fdsva_so (RBDReference.py:1625-1629): second derivatives of
// forward dynamics from Minv [B, N, N], fd = [fd_dq | fd_dqd] [B, N, 2N] (forward_dynamics_grad) and the four tensors of
// second_order_idsva so = [d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq] [B, 4, N, N, N]:
//
//   out0[i,j,k] = -sum_l Minv[i,l] (so0[l,j,k] + sum_m so3[l,m,k] fd_dq[m,j] + sum_m so3[l,m,j] fd_dq[m,k])     daba_dqdq
//   out1[i,j,k] = -sum_l Minv[i,l] (so2[l,j,k] + sum_m so3[l,m,k] fd_dqd[m,j])                                  daba_dvdq
//   out2[i,j,k] = -sum_l Minv[i,l]  so1[l,j,k]                                                                  daba_dvdv
//   out3[i,j,k] = -sum_l Minv[i,l]  sum_m so3[l,m,k] Minv[m,j]                                                  daba_dtdq
//
// Work mapping.  A thread owns ONE column (j, k) of ONE configuration, in every output of the launch's MASK: N
// accumulators per output in registers, like neg_mm_kernel's (rbd_negmm.h).  The block walks the slabs l = 0 .. N-1.  Of
// slab l a thread loads exactly its own entry of each so tensor -- consecutive threads, consecutive addresses; every
// input scalar is read from HBM once per launch, one slab ahead of its use -- and parks its dM_dq entry in LDS,
// TRANSPOSED ([k][m], double-buffered: one barrier per slab).  The inner sums over m are then 16-byte LDS reads of two
// rows of that slab (k and j) against the rows j and k of the transposed fd_dq / fd_dqd and row j of Minv (symmetric,
// :799-804, so row j is column j), all staged once per block; robots small enough keep those four rows in registers for
// the whole launch.  The outer product reads row l of Minv (= column l) from LDS, 16 bytes per read, the same address for
// every thread of a configuration.  Row strides are padded so that the transposed 4-byte writes spread over 8 banks.
//
// Registers decide how many outputs one launch carries: N accumulators per output and column.  fdso_group() picks 4, 2
// or 1 from the block's wave count; the host launches the masks {all}, {0,1},{2,3} or {0},{1},{2},{3} accordingly (dM_dq is
// re-read by every launch that has an inner sum).  Every entry of out is written, structural zeros included.
#pragma once
#include <hip/hip_runtime.h>

namespace rbdk {

constexpr int FDSO_MAX_N = 32;                                   // N * N threads of one configuration must fit a block
template <class T>
constexpr int fdso_ve() { return 16 / (int)sizeof(T); }
template <class T>
constexpr int fdso_np() {                                         // padded row length (scalars) of the LDS matrices
  constexpr int ve = fdso_ve<T>();
  int np = (N + ve - 1) / ve * ve;
  if ((np * (int)sizeof(T) / 4) % 8 == 0) np += ve;
  return np;
}
constexpr int fdso_cfgs() { return 256 / (N * N) > 0 ? 256 / (N * N) : 1; }            // configurations per block
constexpr int fdso_threads() { return (fdso_cfgs() * N * N + 63) / 64 * 64; }
// VGPRs a thread may count on: the block's waves share a SIMD's 512; capped at 176 (beyond that the unrolled inner sums of
// an 18-body robot in fp64 spilled)
constexpr int fdso_reg_budget() { return 512 / ((fdso_threads() + 255) / 256) < 176 ? 512 / ((fdso_threads() + 255) / 256) : 176; }
template <class T>
constexpr int fdso_group() {                                      // outputs per launch: accumulators + 48 within the budget
  constexpr int per = N * (int)sizeof(T) / 4;
  return 4 * per + 48 <= fdso_reg_budget() ? 4 : 2 * per + 48 <= fdso_reg_budget() ? 2 : 1;
}
template <class T>
constexpr bool fdso_hoist() {                                     // rows j, k of fd_dq, j of fd_dqd and Minv in registers
  return fdso_group<T>() == 4 && (4 * N + 4 * fdso_np<T>()) * (int)sizeof(T) / 4 + 48 <= fdso_reg_budget();
}

template <class T, int MASK>
__global__ __launch_bounds__(fdso_threads()) void fdso_contract_kernel(const T* __restrict__ Minv, const T* __restrict__ fd,
                                                                       const T* __restrict__ so, long long B, T* __restrict__ out) {
  constexpr bool O0 = (MASK & 1) != 0, O1 = (MASK & 2) != 0, O2 = (MASK & 4) != 0, O3 = (MASK & 8) != 0;
  constexpr bool NEED_D = O0 || O1 || O3;
  constexpr bool HOIST = MASK == 15 && fdso_hoist<T>();
  constexpr int NN = N * N, NP = fdso_np<T>(), VE = fdso_ve<T>(), NV = NP / VE, CS = N * NP;
  constexpr int C = fdso_cfgs(), TPB = fdso_threads();
  constexpr long long N3 = (long long)N * NN;
  typedef T V __attribute__((ext_vector_type(VE)));
  __shared__ __attribute__((aligned(16))) T Ms[C * CS];                  // Minv, rows padded to NP
  __shared__ __attribute__((aligned(16))) T Qs[O0 ? C * CS : VE];        // fd_dq transposed:  Qs[j][m] = fd_dq[m][j]
  __shared__ __attribute__((aligned(16))) T Vs[O1 ? C * CS : VE];        // fd_dqd transposed
  __shared__ __attribute__((aligned(16))) T Dt[NEED_D ? 2 * C * CS : VE]; // slab l of dM_dq transposed: Dt[k][m] = dM_dq[l][m][k]
  const int tid = threadIdx.x;
  const long long cfg0 = (long long)blockIdx.x * C;
  const int cl = tid / NN, c = tid - cl * NN, j = c / N, k = c - j * N;
  const bool active = cl < C && cfg0 + cl < B;
  const long long cfg = cfg0 + cl;
  // the padding is read by the 16-byte loops: zero everything once
  for (int g = tid; g < C * CS; g += TPB) {
    Ms[g] = T(0);
    if constexpr (O0) Qs[g] = T(0);
    if constexpr (O1) Vs[g] = T(0);
    if constexpr (NEED_D) { Dt[g] = T(0); Dt[C * CS + g] = T(0); }
  }
  __syncthreads();
  const T* sp = so + cfg * 4 * N3 + c;                                   // so[t][l][j][k] = sp[t * N3 + l * NN]
  T pa = T(0), pb = T(0), pc = T(0), pd = T(0);
  if (active) {
    Ms[cl * CS + j * NP + k] = Minv[cfg * NN + c];
    if constexpr (O0) Qs[cl * CS + k * NP + j] = fd[cfg * 2 * NN + j * 2 * N + k];
    if constexpr (O1) Vs[cl * CS + k * NP + j] = fd[cfg * 2 * NN + j * 2 * N + N + k];
    if constexpr (O0) pa = sp[0];
    if constexpr (O2) pb = sp[N3];
    if constexpr (O1) pc = sp[2 * N3];
    if constexpr (NEED_D) pd = sp[3 * N3];
  }
  __syncthreads();
  const int base = active ? cl * CS : 0;
  V hqj[HOIST ? NV : 1], hqk[HOIST ? NV : 1], hvj[HOIST ? NV : 1], hmj[HOIST ? NV : 1];
  if constexpr (HOIST) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      hqj[v] = reinterpret_cast<const V*>(Qs + base + j * NP)[v];
      hqk[v] = reinterpret_cast<const V*>(Qs + base + k * NP)[v];
      hvj[v] = reinterpret_cast<const V*>(Vs + base + j * NP)[v];
      hmj[v] = reinterpret_cast<const V*>(Ms + base + j * NP)[v];
    }
  }
  T acc0[O0 ? N : 1], acc1[O1 ? N : 1], acc2[O2 ? N : 1], acc3[O3 ? N : 1];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if constexpr (O0) acc0[i] = T(0);
    if constexpr (O1) acc1[i] = T(0);
    if constexpr (O2) acc2[i] = T(0);
    if constexpr (O3) acc3[i] = T(0);
  }
#pragma unroll 1
  for (int l = 0; l < N; ++l) {
    const T a = pa, b = pb, cc = pc;
    T* Dl = Dt + (NEED_D ? (l & 1) * C * CS : 0);
    if constexpr (NEED_D) {
      if (active) Dl[base + k * NP + j] = pd;                            // dM_dq[l][m = j][k] -> Dl[k][m]
      __syncthreads();
    }
    if (active && l + 1 < N) {                                           // slab l + 1, in flight during slab l's arithmetic
      const T* sn = sp + (long long)(l + 1) * NN;
      if constexpr (O0) pa = sn[0];
      if constexpr (O2) pb = sn[N3];
      if constexpr (O1) pc = sn[2 * N3];
      if constexpr (NEED_D) pd = sn[3 * N3];
    }
    if (active) {
      T eq = T(0), eqt = T(0), ev = T(0), em = T(0);
      if constexpr (NEED_D) {
        const V* dk = reinterpret_cast<const V*>(Dl + base + k * NP);
        const V* dj = reinterpret_cast<const V*>(Dl + base + j * NP);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const V x = dk[v];
          if constexpr (O0) {
            const V y = dj[v];
            const V qj = HOIST ? hqj[v] : reinterpret_cast<const V*>(Qs + base + j * NP)[v];
            const V qk = HOIST ? hqk[v] : reinterpret_cast<const V*>(Qs + base + k * NP)[v];
#pragma unroll
            for (int e = 0; e < VE; ++e) { eq += qj[e] * x[e]; eqt += qk[e] * y[e]; }
          }
          if constexpr (O1) {
            const V vj = HOIST ? hvj[v] : reinterpret_cast<const V*>(Vs + base + j * NP)[v];
#pragma unroll
            for (int e = 0; e < VE; ++e) ev += vj[e] * x[e];
          }
          if constexpr (O3) {
            const V mj = HOIST ? hmj[v] : reinterpret_cast<const V*>(Ms + base + j * NP)[v];
#pragma unroll
            for (int e = 0; e < VE; ++e) em += mj[e] * x[e];
          }
        }
      }
      const T t0 = a + eq + eqt, t1 = cc + ev, t2 = b, t3 = em;
      const V* ml = reinterpret_cast<const V*>(Ms + base + l * NP);      // Minv[l][i] == Minv[i][l]
#pragma unroll
      for (int v = 0; v < (N + VE - 1) / VE; ++v) {
        const V m = ml[v];
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const int i = v * VE + e;
          if (i < N) {
            if constexpr (O0) acc0[i] -= m[e] * t0;
            if constexpr (O1) acc1[i] -= m[e] * t1;
            if constexpr (O2) acc2[i] -= m[e] * t2;
            if constexpr (O3) acc3[i] -= m[e] * t3;
          }
        }
      }
    }
  }
  if (!active) return;
  T* op = out + cfg * 4 * N3 + c;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if constexpr (O0) op[i * NN] = acc0[i];
    if constexpr (O1) op[N3 + i * NN] = acc1[i];
    if constexpr (O2) op[2 * N3 + i * NN] = acc2[i];
    if constexpr (O3) op[3 * N3 + i * NN] = acc3[i];
  }
}

}  // namespace rbdk
