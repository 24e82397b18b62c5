// rbd_mppi.h -- the update of a sampling controller (MPPI): softmin weights of the sample costs rbd_rollout_cost wrote, and
// the weighted sum of the perturbations it applied, read ONCE (gfx950).  P independent problems (the B_nom rows of
// rbd_rollout_cost), S samples each, in its row layout: row s P + p is sample s of problem p.
//
//   Jm  = min_s J[s,p]                       (a NaN counts as +inf)
//   x_s = (J[s,p] - Jm) / lam[p];   e_s = exp(-x_s)   (the accurate exp: 1 at a minimum, 0 for a NaN or +inf sample)
//   eta = sum_s e_s;   w_s = e_s / eta;   ess = eta^2 / sum_s e_s^2
//   d_s[t,j] = du[t,s,p,j], or with limits rollcl_clamp(u[t,p,j] + du[t,s,p,j], lo_j, hi_j) - u[t,p,j]: what rbd_rollout_cost
//              applied (rbd_rollout_cl.h)
//   u_out[t,p,j] = u[t,p,j] + (sum_s e_s d_s[t,j]) / eta, clamped once more when limits are given
//   status[p] = 2: lam[p] is not finite and positive; else 1: Jm is not finite (every sample NaN or +inf, or a -inf among
//               them); else 0.  status != 0: u_out[:,p] = u[:,p] (clamped), w = 0, ess = 0.
// Nothing else is special: a NaN in du poisons the (t, j) outputs of its own problem (0 * NaN is NaN).
//
// SUMMATION ORDER (no floating-point atomics; a function of S and C = RBD_MPPI_CHUNK alone -- not of P, T, the grid, the
// load width or the optional outputs).  Each of eta, sum e^2 and sum e d[t,j]:
//   chunk k = samples k C .. min(S, (k + 1) C) - 1:  ONE chain from zero in ascending s
//            (eta: a += e_s;  sum e^2: a = fma(e_s, e_s, a);  sum e d: a = fma(e_s, d_s, a)),
//   group g = chunks g C .. (g + 1) C - 1 (C^2 samples):  the chunks added in ascending k  (grp = chunk_gC; grp += chunk_gC+1; ...),
//   then the groups in ascending g:  total = group_0; total += group_1; ...
// (the groups exist for depth: S = 65 536 is 1 024 chunks, and one chain over them was 20 us of LDS latency per launch)
//
// Three launches on one stream:
//   mppi_weights_kernel / mppi_weights_small_kernel   J -> e [S, P] and eta [P] in the workspace, w, ess, status.  J is S P
//            scalars: one block per problem, or one thread per problem when S <= C (one chunk, many problems)
//   mppi_partials_kernel   reads du once.  A thread owns (t, chunk, VE consecutive scalars of the P n of a sample's row) and
//            runs the chunk's chain; the scalars of a row are contiguous, so a wave's load is one contiguous run when P n is
//            large (16-byte loads when P n is a multiple of VE and du is aligned) and a few short runs, one per chunk, when
//            it is small (P = 1: 224 outputs, 1024 chunks of S = 65 536 in flight).  S <= C: it finishes u_out itself
//   mppi_combine_kernel    chunk partials [ceil(S / C), T, P, n] -> u_out: 16 outputs per block; thread (g, o) chains the C
//            chunks of group g for output o (independent loads), then threads 0 .. 15 add their output's groups from LDS
#pragma once
#include "../../include/rbd_hip.h"
#include "rbd_rollout_cl.h"

namespace rbdk {

constexpr int MPPI_CHUNK = RBD_MPPI_CHUNK;
constexpr int MPPI_THREADS = 256;            // partials, combine, weights_small
constexpr int MPPI_W_THREADS = 1024;         // weights: one block per problem
constexpr int MPPI_W_GROUPS = MPPI_W_THREADS / MPPI_CHUNK;      // weights: whole groups of C chunks per trip of 1024 chunks
static_assert(MPPI_W_THREADS % MPPI_CHUNK == 0 && MPPI_W_GROUPS <= 64, "a trip of the weights kernel is whole groups");
constexpr int MPPI_COMB_O = 16;              // combine: outputs per block
constexpr int MPPI_COMB_G = MPPI_THREADS / MPPI_COMB_O;         // combine: groups per trip, one thread each per output
template <class T>
constexpr int mppi_vec() { return 16 / (int)sizeof(T); }

RBD_DEV float mppi_exp(float x) { return expf(x); }
RBD_DEV double mppi_exp(double x) { return exp(x); }
template <class T>
RBD_DEV T mppi_inf() { return T(__builtin_huge_valf()); }
template <class T>
RBD_DEV bool mppi_finite(T x) { return x - x == T(0); }

// e_s of one sample (Jm finite, lam finite and positive)
template <class T>
RBD_DEV T mppi_e(T J, T Jm, T lam) {
  const T Jc = J == J ? J : mppi_inf<T>();
  return mppi_exp(-((Jc - Jm) / lam));
}
// what a problem's status is, from its minimum and temperature
template <class T>
RBD_DEV int mppi_status(T Jm, T lam) {
  if (!(lam > T(0) && lam < mppi_inf<T>())) return 2;
  return mppi_finite(Jm) ? 0 : 1;
}
// the last step of an output: eta == 0 marks a problem whose status is not 0 (eta >= 1 otherwise)
template <class T>
RBD_DEV T mppi_finish(T u, T acc, T eta, bool limits, T lo, T hi) {
  const T v = eta > T(0) ? u + acc / eta : u;
  return limits ? rollcl_clamp(v, lo, hi) : v;
}

// ---- weights, S > C: one block per problem ---------------------------------------------------------------------------------
// phase 1: the minimum (exact in any order);  phase 2: e_s, stored (and w's numerator);  phase 3: thread i runs the chains
// of chunks i, i + 1024, ... on the stored e;  phase 4: the chunks of a group, then the groups, in ascending order (eta in
// wave 0, sum e^2 in wave 1)
template <class T>
__global__ __launch_bounds__(MPPI_W_THREADS) void mppi_weights_kernel(const T* __restrict__ J, const T* __restrict__ lam,
                                                                     long long S, long long P, T* __restrict__ e_ws,
                                                                     T* __restrict__ eta_ws, T* __restrict__ w_out,
                                                                     T* __restrict__ ess_out, int* __restrict__ status_out) {
  __shared__ T red[MPPI_W_THREADS];
  __shared__ T red2[MPPI_W_THREADS];
  __shared__ T grp[2][MPPI_W_GROUPS];
  const long long p = blockIdx.x;
  const int tid = threadIdx.x;
  T m = mppi_inf<T>();
  for (long long s = tid; s < S; s += MPPI_W_THREADS) {
    const T v = J[s * P + p];
    if (v < m) m = v;                        // (a NaN compares false: it counts as +inf)
  }
  red[tid] = m;
  __syncthreads();
  for (int h = MPPI_W_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h && red[tid + h] < red[tid]) red[tid] = red[tid + h];
    __syncthreads();
  }
  const T Jm = red[0];
  const T l = lam[p];
  const int status = mppi_status(Jm, l);
  __syncthreads();
  for (long long s = tid; s < S; s += MPPI_W_THREADS) e_ws[s * P + p] = status == 0 ? mppi_e(J[s * P + p], Jm, l) : T(0);
  __threadfence_block();
  __syncthreads();
  const long long nchunks = (S + MPPI_CHUNK - 1) / MPPI_CHUNK;
  T tot = T(0);                              // running total across the trips of 1024 chunks: eta in thread 0, sum e^2 in thread 64
  for (long long k0 = 0; k0 < nchunks; k0 += MPPI_W_THREADS) {
    const long long k = k0 + tid;
    T a = T(0), b = T(0);
    if (k < nchunks) {
      const long long s0 = k * MPPI_CHUNK;
      const long long s1 = s0 + MPPI_CHUNK < S ? s0 + MPPI_CHUNK : S;
      constexpr int VE = mppi_vec<T>();
      if (P == 1 && s1 - s0 == MPPI_CHUNK) {            // one problem: a chunk is contiguous, 16-byte loads (same order)
        typedef T V __attribute__((ext_vector_type(VE)));
        const V* src = reinterpret_cast<const V*>(e_ws + s0);
#pragma unroll 4
        for (int i = 0; i < MPPI_CHUNK / VE; ++i) {
          const V v = src[i];
#pragma unroll
          for (int j = 0; j < VE; ++j) {
            a += v[j];
            b = fma_(v[j], v[j], b);
          }
        }
      } else {
#pragma unroll 8
        for (long long s = s0; s < s1; ++s) {
          const T e = e_ws[s * P + p];
          a += e;
          b = fma_(e, e, b);
        }
      }
    }
    red[tid] = a;
    red2[tid] = b;
    __syncthreads();
    // the trip's chunks are MPPI_W_GROUPS whole groups (the last may be short): lanes 0 .. 15 of wave 0 chain eta's groups,
    // lanes 0 .. 15 of wave 1 those of sum e^2; then lane 0 of each adds the groups in ascending order
    const int cnt = nchunks - k0 < MPPI_W_THREADS ? (int)(nchunks - k0) : MPPI_W_THREADS;
    const int half = tid >> 6, gl = tid & 63;
    if (half < 2 && gl < MPPI_W_GROUPS && gl * MPPI_CHUNK < cnt) {
      const T* part = (half == 0 ? red : red2) + gl * MPPI_CHUNK;
      const int m = cnt - gl * MPPI_CHUNK < MPPI_CHUNK ? cnt - gl * MPPI_CHUNK : MPPI_CHUNK;
      T gs = part[0];
#pragma unroll 8
      for (int i = 1; i < m; ++i) gs += part[i];
      grp[half][gl] = gs;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
      const int ng = (cnt + MPPI_CHUNK - 1) / MPPI_CHUNK;
      int i = 0;
      if (k0 == 0) { tot = grp[half][0]; i = 1; }
      for (; i < ng; ++i) tot += grp[half][i];
    }
    __syncthreads();
  }
  if (tid == 64) red2[0] = tot;
  __syncthreads();
  if (tid == 0) {
    red[0] = tot;
    eta_ws[p] = status == 0 ? tot : T(0);
    if (ess_out) ess_out[p] = status == 0 ? (tot * tot) / red2[0] : T(0);
    status_out[p] = status;
  }
  __syncthreads();
  if (w_out) {
    const T et = red[0];
    for (long long s = tid; s < S; s += MPPI_W_THREADS) w_out[s * P + p] = status == 0 ? e_ws[s * P + p] / et : T(0);
  }
}

// ---- weights, S <= C (one chunk): one thread per problem, every access coalesced over p ------------------------------------
template <class T>
__global__ __launch_bounds__(MPPI_THREADS) void mppi_weights_small_kernel(const T* __restrict__ J, const T* __restrict__ lam,
                                                                         long long S, long long P, T* __restrict__ e_ws,
                                                                         T* __restrict__ eta_ws, T* __restrict__ w_out,
                                                                         T* __restrict__ ess_out, int* __restrict__ status_out) {
  const long long p = (long long)blockIdx.x * MPPI_THREADS + threadIdx.x;
  if (p >= P) return;
  T Jm = mppi_inf<T>();
  for (long long s = 0; s < S; ++s) {
    const T v = J[s * P + p];
    if (v < Jm) Jm = v;
  }
  const T l = lam[p];
  const int status = mppi_status(Jm, l);
  T eta = T(0), sq = T(0);
  for (long long s = 0; s < S; ++s) {
    const T e = status == 0 ? mppi_e(J[s * P + p], Jm, l) : T(0);
    e_ws[s * P + p] = e;
    eta += e;
    sq = fma_(e, e, sq);
  }
  eta_ws[p] = status == 0 ? eta : T(0);
  if (ess_out) ess_out[p] = status == 0 ? (eta * eta) / sq : T(0);
  status_out[p] = status;
  if (w_out)
    for (long long s = 0; s < S; ++s) w_out[s * P + p] = status == 0 ? e_ws[s * P + p] / eta : T(0);
}

// ---- the pass over du --------------------------------------------------------------------------------------------------------
// unit = (t, chunk k, group g of VE consecutive scalars of the R = P n of a row), g fastest.  out: nchunks > 1: the partials
// [nchunks, T, R]; nchunks == 1: u_out [T, R], finished here.  VE > 1 needs R % VE == 0 and du 16-byte aligned (the host
// decides); groups = R / VE.
template <class T, int VE>
__global__ __launch_bounds__(MPPI_THREADS) void mppi_partials_kernel(const T* __restrict__ du, const T* __restrict__ u,
                                                                    const T* __restrict__ e_ws, const T* __restrict__ eta_ws,
                                                                    const T* __restrict__ u_lo, const T* __restrict__ u_hi,
                                                                    long long S, long long P, long long steps,
                                                                    long long nchunks, long long groups, T* __restrict__ out) {
  typedef T V __attribute__((ext_vector_type(VE)));
  const long long R = P * N;
  const long long unit = (long long)blockIdx.x * MPPI_THREADS + threadIdx.x;
  if (unit >= steps * nchunks * groups) return;
  const long long g = unit % groups;
  const long long k = (unit / groups) % nchunks;
  const long long t = unit / (groups * nchunks);
  const long long c0 = g * VE;
  const bool limits = u_lo != nullptr;
  long long pp[VE];
  T uu[VE], lo[VE], hi[VE], acc[VE];
#pragma unroll
  for (int i = 0; i < VE; ++i) {
    const long long c = c0 + i;
    pp[i] = c / N;
    const int j = (int)(c - pp[i] * N);
    uu[i] = u[t * R + c];
    lo[i] = limits ? u_lo[j] : T(0);
    hi[i] = limits ? u_hi[j] : T(0);
    acc[i] = T(0);
  }
  const long long s0 = k * MPPI_CHUNK;
  const long long s1 = s0 + MPPI_CHUNK < S ? s0 + MPPI_CHUNK : S;
  const T* src = du + (t * S + s0) * R + c0;
  const T* es = e_ws + s0 * P;
#pragma unroll 8
  for (long long s = s0; s < s1; ++s, src += R, es += P) {
    T d[VE];
    if constexpr (VE > 1) {
      const V v = *reinterpret_cast<const V*>(src);
#pragma unroll
      for (int i = 0; i < VE; ++i) d[i] = v[i];
    } else {
      d[0] = src[0];
    }
#pragma unroll
    for (int i = 0; i < VE; ++i) {
      const T x = limits ? rollcl_clamp(uu[i] + d[i], lo[i], hi[i]) - uu[i] : d[i];
      acc[i] = fma_(es[pp[i]], x, acc[i]);
    }
  }
  T* dst = out + (k * steps + t) * R + c0;
#pragma unroll
  for (int i = 0; i < VE; ++i) dst[i] = nchunks > 1 ? acc[i] : mppi_finish(uu[i], acc[i], eta_ws[pp[i]], limits, lo[i], hi[i]);
}

// ---- chunk partials -> u_out ---------------------------------------------------------------------------------------------------
// O = T R outputs, MPPI_COMB_O per block; thread (gl, ol) = (tid / 16, tid % 16) chains the chunks of group g0 + gl for
// output o0 + ol; then threads 0 .. 15 continue their output's chain over the trip's MPPI_COMB_G groups
template <class T>
__global__ __launch_bounds__(MPPI_THREADS) void mppi_combine_kernel(const T* __restrict__ part, const T* __restrict__ u,
                                                                   const T* __restrict__ eta_ws, const T* __restrict__ u_lo,
                                                                   const T* __restrict__ u_hi, long long P, long long O,
                                                                   long long nchunks, T* __restrict__ u_out) {
  __shared__ T tile[MPPI_COMB_G][MPPI_COMB_O];
  const int tid = threadIdx.x;
  const int gl = tid / MPPI_COMB_O, ol = tid % MPPI_COMB_O;
  const long long o0 = (long long)blockIdx.x * MPPI_COMB_O;
  const long long o = o0 + ol < O ? o0 + ol : O - 1;       // (a ragged block's spare lanes load a valid output, store nothing)
  const long long ngroups = (nchunks + MPPI_CHUNK - 1) / MPPI_CHUNK;
  T acc = T(0);
  for (long long g0 = 0; g0 < ngroups; g0 += MPPI_COMB_G) {
    const long long kb = (g0 + gl) * MPPI_CHUNK;           // this thread's group: chunks kb .. kb + m - 1, loads independent
    if (kb < nchunks) {
      const int m = nchunks - kb < MPPI_CHUNK ? (int)(nchunks - kb) : MPPI_CHUNK;
      const T* src = part + kb * O + o;
      T gs = src[0];
#pragma unroll 8
      for (int i = 1; i < m; ++i) gs += src[i * O];
      tile[gl][ol] = gs;
    }
    __syncthreads();
    if (tid < MPPI_COMB_O) {
      const int ng = ngroups - g0 < MPPI_COMB_G ? (int)(ngroups - g0) : MPPI_COMB_G;
      int i = 0;
      if (g0 == 0) { acc = tile[0][ol]; i = 1; }
      for (; i < ng; ++i) acc += tile[i][ol];
    }
    __syncthreads();
  }
  if (tid < MPPI_COMB_O && o0 + ol < O) {
    const long long R = P * N;
    const long long c = o % R;
    const long long p = c / N;
    const int j = (int)(c - p * N);
    const bool limits = u_lo != nullptr;
    u_out[o] = mppi_finish(u[o], acc, eta_ws[p], limits, limits ? u_lo[j] : T(0), limits ? u_hi[j] : T(0));
  }
}

}  // namespace rbdk
