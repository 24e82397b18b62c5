// rbd_rollout_adj.h -- reverse-mode gradient of a rollout (rbd_rollout.h): the backward recursion over time as ONE launch
// that walks the time axis with the adjoint on chip (gfx950).
//
// With lam = (lq | lqd) the adjoint of the state after step t, g the direct partials of the cost with respect to the
// returned slices and [dc_dq | dc_dqd] = rnea_grad, Minv = minv at step t's linearisation point (q_t, qd_t, u_t):
//   lq += gq[t];  lqd += gqd[t];  w = lqd + dt lq
//   mu = dt w (semi-implicit Euler)  |  dt lqd (explicit Euler);   nu = Minv mu   -> grad_u[t] = nu
//   lq = lq - dc_dq^T nu;  lqd = w - dc_dqd^T nu
// Only vector-Jacobian products: the n x n x 2n product -Minv dc_du of forward_dynamics_grad (rbd_negmm.h) is never formed.
// PRISMATIC JOINTS: rnea_grad's dc_dq reproduces the reference and is not the q-derivative there (rbd_fdsva_so.h, api.py);
// what this kernel returns inherits that and is the true gradient on robots with revolute joints only.
//
// Work mapping, in the style of rbd_negmm.h.  2 N threads per configuration, C = 256 / (2 N) consecutive configurations
// per block; thread c owns component c of (lq | lqd) for the whole launch, in a register.  Per step:
//   1. every thread adds its g and parks its component in LDS                                               (barrier)
//   2. nu_j = sum_l Minv[l][j] mu_l is split over the two threads j and N + j of a configuration, rows l < ceil(N / 2) and
//      the rest: both halves of the block load, and a thread holds half a column.  Minv is symmetric, so column j is
//      row j, and for each l consecutive threads read consecutive addresses.  mu_l is formed from the parked lam on
//      the fly (two LDS reads of an address the whole configuration shares); the partial sums go to LDS     (barrier)
//   3. thread j < N adds the two partial sums, stores nu_j to grad_u and parks it                           (barrier)
//   4. thread c accumulates sum_i dc_du[i][c] nu_i -- row i of dc_du is the 2 N consecutive scalars of the
//      configuration's threads -- and takes it from lq (c < N) or w (c >= N).
// The block's reads at step t are one contiguous span of each input.  Nothing a step loads depends on lam, so step
// t - 1's column of dc_du, half column of Minv and g are loaded before step t computes and wait in registers (where they
// fit, rollg_prefetch): the only dependent chain is lam -> mu -> nu -> lam.  Per configuration and step N 2N + N N + 2N scalars are read, N written.
//
// lam enters and leaves through a global [B, 2N] buffer, loaded and stored as it is: the host may run the time axis in
// chunks, and a scan split at any step is bit-identical to the unsplit one (every step runs the same instructions).
// g is ALWAYS added, as zero where there is none, for the same reason.  All element offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

namespace rbdk {

constexpr int rollg_cfgs() { return 256 / (2 * N) > 0 ? 256 / (2 * N) : 1; }          // configurations per block
constexpr int rollg_threads() { return (rollg_cfgs() * 2 * N + 63) / 64 * 64; }
constexpr int ROLLG_HALF = (N + 1) / 2;                                                // rows of Minv of a thread c < N
// the next step's operands wait in registers where two steps' worth of them is at most 120 VGPRs (the 30-body robot in
// fp32: 146 VGPRs in all, three waves per SIMD); otherwise (that robot in fp64) a step loads its own at its start and the
// other waves of the SIMD hide the latency
template <class T>
constexpr bool rollg_prefetch() { return 2 * (N + ROLLG_HALF) * (int)sizeof(T) / 4 <= 120; }

// g_final: gq / gqd are [B, N] and belong to step `steps - 1`; otherwise [steps, B, N].  Either may be null (zero).
// out_q0 / out_qd0: when non-null, the final lq / lqd are stored there as [B, N] each, as well as to lam.
template <class T>
__global__ __launch_bounds__(rollg_threads()) void rollout_adjoint_kernel(
    const T* __restrict__ dc, const T* __restrict__ Minv, const T* __restrict__ gq, const T* __restrict__ gqd, int g_final, T dt,
    int integrator, long long B, long long steps, T* __restrict__ lam, T* __restrict__ grad_u, T* __restrict__ out_q0,
    T* __restrict__ out_qd0) {
  constexpr int N2 = 2 * N, C = rollg_cfgs(), H = ROLLG_HALF;
  __shared__ T lam_s[C * N2];        // (lq | lqd) after g was added
  __shared__ T part_s[C * N2];       // the two partial sums of nu_j: [j] and [N + j]
  __shared__ T nu_s[C * N];
  const int tid = threadIdx.x;
  const int cl = tid / N2, c = tid - cl * N2;
  const long long cfg = (long long)blockIdx.x * C + cl;
  const bool live = cl < C && cfg < B;                     // the others only keep the barriers company
  const bool upper = c >= N;                               // owns a component of lqd
  const int j = upper ? c - N : c;
  const int l0 = upper ? H : 0;                            // first row of this thread's half column of Minv
  const T* gp = upper ? gqd : gq;
  const long long row_n = (long long)N, rows_dc = (long long)N * N2, rows_m = (long long)N * N;

  T d[N], dn[N], m[H], mn[H];
  T g = T(0), gn = T(0);
  auto load = [&](long long t, T (&dd)[N], T (&mm)[H], T& gg) {
    const long long r = t * B + cfg;                       // flat row of step t
    const T* dp = dc + r * rows_dc + c;
    const T* mp = Minv + r * rows_m + (long long)l0 * N + j;
#pragma unroll
    for (int i = 0; i < N; ++i) dd[i] = dp[i * N2];
#pragma unroll
    for (int k = 0; k < H; ++k) mm[k] = (k < N - H || !upper) ? mp[k * N] : T(0);      // (N odd: the upper half is one row shorter)
    gg = T(0);
    if (gp != nullptr) {
      if (!g_final) gg = gp[r * row_n + j];
      else if (t == steps - 1) gg = gp[cfg * row_n + j];
    }
  };
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = dn[i] = T(0);
#pragma unroll
  for (int k = 0; k < H; ++k) m[k] = mn[k] = T(0);

  T lv = T(0);
  if (live) {
    lv = lam[cfg * N2 + c];
    load(steps - 1, d, m, g);
  }
#pragma nounroll
  for (long long t = steps - 1; t >= 0; --t) {
    if constexpr (rollg_prefetch<T>()) {
      if (live && t > 0) load(t - 1, dn, mn, gn);          // in flight while this step computes
    } else {
      if (live && t < steps - 1) load(t, d, m, g);
    }
    if (live) {
      lv += g;
      lam_s[cl * N2 + c] = lv;
    }
    __syncthreads();
    T w = lv;
    if (live) {
      const T* ls = lam_s + cl * N2;
      if (upper) w = fma_(dt, ls[j], lv);
      T acc = T(0);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        if (k < N - H || !upper) {
          const int l = l0 + k;
          const T mu = dt * (integrator == 0 ? fma_(dt, ls[l], ls[N + l]) : ls[N + l]);
          acc = fma_(m[k], mu, acc);
        }
      }
      part_s[cl * N2 + c] = acc;
    }
    __syncthreads();
    if (live && !upper) {
      const T nu = part_s[cl * N2 + c] + part_s[cl * N2 + N + c];
      nu_s[cl * N + c] = nu;
      grad_u[(t * B + cfg) * row_n + c] = nu;
    }
    __syncthreads();
    if (live) {
      const T* ns = nu_s + cl * N;
      T acc = T(0);
#pragma unroll
      for (int i = 0; i < N; ++i) acc = fma_(d[i], ns[i], acc);
      lv = w - acc;
    }
    if constexpr (rollg_prefetch<T>()) {
#pragma unroll
      for (int i = 0; i < N; ++i) d[i] = dn[i];
#pragma unroll
      for (int k = 0; k < H; ++k) m[k] = mn[k];
      g = gn;
    }
  }
  if (live) {
    lam[cfg * N2 + c] = lv;
    T* o = upper ? out_qd0 : out_q0;
    if (o != nullptr) o[cfg * row_n + j] = lv;
  }
}

}  // namespace rbdk
