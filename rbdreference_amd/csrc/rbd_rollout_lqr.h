// rbd_rollout_lqr.h -- the backward pass of iLQR / DDP / time-varying LQR over a rollout (rbd_rollout.h): the Riccati
// recursion over time as ONE launch that walks the time axis with the value function's gradient lam and Hessian P on chip
// and factors Quu on chip (gfx950).
//
// With x = (q | qd), D = dc_du[t] = rnea_grad (N x 2N) and M = Minv[t] (N x N, symmetric) at step t's linearisation point:
//   A0 = [[I, dt I], [0, I]];  b = [dt^2 I ; dt I] (semi-implicit Euler) | [0 ; dt I] (explicit Euler);  Bm = b M;  A = A0 - Bm D
//   lam += (gq[t] | gqd[t]);  P += diag(hq[t] | hqd[t])
//   Qx = A^T lam;  Qu = gu[t] + Bm^T lam;  Qxx = A^T P A;  Qux = Bm^T P A;  Quu = diag(hu[t]) + Bm^T P Bm
//   L L^T = Quu + reg I;  k = -(Quu + reg I)^-1 Qu;  K = -(Quu + reg I)^-1 Qux          -> k[t] [N], K[t] [N, 2N]
//   dV[0] += k^T Qu;  dV[1] += 1/2 k^T Quu k
//   lam = Qx + K^T (Quu k + Qu) + Qux^T k;  P = Qxx + K^T (Quu K + Qux) + Qux^T K;  P = 1/2 (P + P^T)
// A pivot of the factorisation that is <= 0 or not finite: k = K = 0 for that row and step, status += 1, and the updates
// degenerate to lam = Qx, P = Qxx (symmetrised), dV unchanged.
// PRISMATIC JOINTS: rnea_grad's dc_dq reproduces the reference and is not the q-derivative there (rbd_fdsva_so.h, api.py);
// the gains inherit that and belong to the true linearisation on robots with revolute joints only.
//
// The products are never formed with A or Bm.  With S = P Bm = (beta P[:, :N] + dt P[:, N:]) M (beta = dt^2 | 0),
// G = Bm^T S = M (beta S[:N] + dt S[N:]) and Y = S^T A0:
//   Qux = Y - G D;  Qxx = A0^T P A0 - Y^T D - D^T Qux;  Quu = G + diag(hu);  Qx = A0^T lam - D^T nu,  nu = M mu(lam) as in
// rbd_rollout_adj.h.  About 14 N^2 FMAs per thread and step; 3 N^2 scalars read and 2 N^2 written per row and step.
//
// Work mapping.  2N threads per configuration as in rbd_rollout_adj.h: thread c owns component c of lam and column c of P
// (= row c: P is symmetric), in registers for the whole launch, and column c of every N x 2N matrix of a step.  A
// configuration's threads NEVER straddle a wave: a block is one wave of 64 / 2N configurations (N <= 32), so each of the
// 2N + 11 synchronisation points of a step (N Cholesky columns take two each) orders LDS traffic inside one wave; the
// __syncthreads() that marks them needs no other wave to arrive.  (2N > 64: one configuration per block of several waves,
// same code, real barriers.)
// Registers hold p[2N] and one N-vector at a time (unrolled index); every other operand is read from LDS inside loops whose
// OUTER index is a run-time value and whose inner, unrolled index addresses registers and immediate LDS offsets: the code
// stays a few thousand instructions for N = 30, not the ~40 000 of a fully unrolled step.  LDS per configuration, in
// scalars: M | D | X | Y | G = N^2 + 3 * 2N^2 + N^2 = 8 N^2 (X: left half of P, then S, then K; Y: Y, then Qux; M: M, then
// the Cholesky factor; D's place takes nothing else, and the transpose buffer of the symmetrisation, 2N (2N + 1), lies over
// M, D and X when they are dead) + 10 N + 2 for the vectors.
// Step t - 1's operands (column of D, N / 2 scalars of M, the costs) are loaded while step t computes and wait in
// registers where that is at most LQR_PREFETCH_REGS of them.  All element offsets are 64-bit.
//
// lam, P, dV and status enter and leave through global buffers, loaded and stored as they are, and absent costs are added
// as zero: every step runs the same instructions, so a scan split at any step is bit-identical to the unsplit one.
#pragma once
#include <hip/hip_runtime.h>

namespace rbdk {

constexpr int LQR_N2 = 2 * N;
constexpr int LQR_HALF = (N + 1) / 2;
constexpr int lqr_threads() { return (LQR_N2 + 63) / 64 * 64; }
constexpr int lqr_cfgs() { return LQR_N2 <= 64 ? 64 / LQR_N2 : 1; }                    // configurations per block
constexpr int LQR_PER_CFG = 8 * N * N + 10 * N + 2;                                    // LDS scalars per configuration
constexpr int LQR_PREFETCH_REGS = 72;
template <class T>
constexpr size_t lqr_lds_bytes() { return (size_t)lqr_cfgs() * LQR_PER_CFG * sizeof(T); }
template <class T>
constexpr bool lqr_fits() { return lqr_lds_bytes<T>() <= 65536; }                      // else the entry point refuses
template <class T>
constexpr bool lqr_prefetch() { return (N + LQR_HALF + 4) * (int)sizeof(T) / 4 <= LQR_PREFETCH_REGS; }

// The rank-one updates of p read whole rows of 2N scalars from LDS.  Where such a row is more than 64 registers (fp64,
// N > 16) the scheduler may not gather it at once: beside p[2N] it would not fit the register file (scratch).
template <class T>
__device__ __forceinline__ void lqr_row_fence(int r) {
  if constexpr (LQR_N2 * (int)sizeof(T) / 4 > 64) {
    if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  }
}

// x_final: gq / gqd / hq / hqd are [B, N] and belong to step `steps - 1`; otherwise [steps, B, N].  Any may be null (zero).
// gu: [steps, B, N] or null.  hu: [steps, B, N], or [N] (hu_shared).
template <class T>
__global__ __launch_bounds__(lqr_threads()) void rollout_riccati_kernel(
    const T* __restrict__ dc, const T* __restrict__ Minv, const T* __restrict__ gq, const T* __restrict__ gqd,
    const T* __restrict__ hq, const T* __restrict__ hqd, int x_final, const T* __restrict__ gu, const T* __restrict__ hu,
    int hu_shared, T reg, T dt, int integrator, long long B, long long steps, T* __restrict__ lam, T* __restrict__ P,
    T* __restrict__ dV, int* __restrict__ status, T* __restrict__ kout, T* __restrict__ Kout) {
  if constexpr (!lqr_fits<T>()) {
    return;
  } else {
    constexpr int N2 = LQR_N2, C = lqr_cfgs(), H = LQR_HALF, NN = N * N, ZS = N2 + 1;
    __shared__ T smem[C * LQR_PER_CFG];
    const int tid = threadIdx.x;
    const int cl = tid / N2, c = tid - cl * N2;
    const long long cfg = (long long)blockIdx.x * C + cl;
    const bool live = cl < C && cfg < B;                   // the others only keep the barriers company
    const bool upper = c >= N;                             // owns a component of lqd
    const int j = upper ? c - N : c;
    T* const sm = smem + (live ? cl : 0) * LQR_PER_CFG;
    T* const Ms = sm;                                      // M [N][N]; later the Cholesky factor (lower triangle)
    T* const Ds = Ms + NN;                                 // D [N][2N]
    T* const Xs = Ds + 2 * NN;                             // left half of P [2N][N]; S [2N][N]; K [N][2N]
    T* const Ys = Xs + 2 * NN;                             // Y [N][2N]; Qux [N][2N]
    T* const Gs = Ys + 2 * NN;                             // G = Bm^T P Bm [N][N]
    T* const lam_s = Gs + NN;                              // [2N]
    T* const nu_s = lam_s + N2;
    T* const qu_s = nu_s + N;
    T* const hu_s = qu_s + N;
    T* const k_s = hu_s + N;
    T* const e_s = k_s + N;
    T* const dva_s = e_s + N;
    T* const dvb_s = dva_s + N;
    T* const dinv_s = dvb_s + N;
    T* const piv_s = dinv_s + N;
    T* const Zs = sm;                                      // [2N][2N + 1], over M, D, X: the transpose of the symmetrisation
    const T beta = integrator == 0 ? dt * dt : T(0);
    const T* gp = upper ? gqd : gq;
    const T* hp = upper ? hqd : hq;
    const long long row_n = (long long)N, rows_dc = (long long)N * N2, rows_m = (long long)NN;

    T p[N2], x[N];                                         // column c of P; the N-vector of the stage at hand
    T d[N], dn[N], m[H], mn[H];
    T g = T(0), h = T(0), guv = T(0), huv = T(0), gn = T(0), hn = T(0), gun = T(0), hun = T(0);
    auto load = [&](long long t, T (&dd)[N], T (&mm)[H], T& gg, T& hh, T& gguu, T& hhuu) {
      const long long r = t * B + cfg;                     // flat row of step t
      const T* dp = dc + r * rows_dc + c;
      const T* mp = Minv + r * rows_m + c;
#pragma unroll
      for (int i = 0; i < N; ++i) dd[i] = dp[i * N2];
#pragma unroll
      for (int k = 0; k < H; ++k) mm[k] = (c + k * N2 < NN) ? mp[k * N2] : T(0);
      gg = hh = T(0);
      if (!x_final) {
        if (gp != nullptr) gg = gp[r * row_n + j];
        if (hp != nullptr) hh = hp[r * row_n + j];
      } else if (t == steps - 1) {
        if (gp != nullptr) gg = gp[cfg * row_n + j];
        if (hp != nullptr) hh = hp[cfg * row_n + j];
      }
      gguu = hhuu = T(0);
      if (!upper) {
        if (gu != nullptr) gguu = gu[r * row_n + j];
        hhuu = hu_shared ? hu[j] : hu[r * row_n + j];
      }
    };
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = dn[i] = x[i] = T(0);
#pragma unroll
    for (int k = 0; k < H; ++k) m[k] = mn[k] = T(0);
#pragma unroll
    for (int r = 0; r < N2; ++r) p[r] = T(0);

    T lv = T(0), dv = T(0);                                // dv: dV[0] in thread 0, dV[1] in thread 1
    int st = 0;
    if (live) {
      lv = lam[cfg * N2 + c];
      const T* pp = P + cfg * (long long)(N2 * N2) + c;
#pragma unroll
      for (int r = 0; r < N2; ++r) p[r] = pp[r * N2];
      if (c < 2) dv = dV[cfg * 2 + c];
      if (c == 0) st = status[cfg];
      if constexpr (lqr_prefetch<T>()) load(steps - 1, d, m, g, h, guv, huv);
    }
#pragma nounroll
    for (long long t = steps - 1; t >= 0; --t) {
      // (what a step defines under `live` is defined here for every lane, or it would live round the loop in registers)
#pragma unroll
      for (int i = 0; i < N; ++i) x[i] = T(0);
      if constexpr (lqr_prefetch<T>()) {
        if (live && t > 0) load(t - 1, dn, mn, gn, hn, gun, hun);          // in flight while this step computes
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = T(0);
#pragma unroll
        for (int k = 0; k < H; ++k) m[k] = T(0);
        if (live) load(t, d, m, g, h, guv, huv);           // dead again once stage A has parked them
      }
      // (the unrolled comparisons with c and j below must not leave the loop: hoisted, their ~5N lane masks spill the SGPRs)
      int cv = c, jv = j;
      asm volatile("" : "+v"(cv), "+v"(jv));
      // ---- A: costs; park lam, D, M and the left half of P; row c of W = beta P[:, :N] + dt P[:, N:] ----------------
      if (live) {
        lv += g;
        lam_s[c] = lv;
#pragma unroll
        for (int r = 0; r < N2; ++r) p[r] += (r == cv) ? h : T(0);
#pragma unroll
        for (int i = 0; i < N; ++i) Ds[i * N2 + c] = d[i];
#pragma unroll
        for (int k = 0; k < H; ++k)
          if (c + k * N2 < NN) Ms[c + k * N2] = m[k];
        if (!upper) {
#pragma unroll
          for (int r = 0; r < N2; ++r) Xs[r * N + c] = p[r];
          hu_s[c] = huv;
        }
#pragma unroll
        for (int l = 0; l < N; ++l) x[l] = fma_(beta, p[l], dt * p[N + l]);
      }
      __syncthreads();
      // ---- B: p = column c of A0^T P A0; nu = M mu(lam), Qu = gu + nu ------------------------------------------------
      if (live) {
        if (upper) {
#pragma unroll
          for (int r = 0; r < N2; ++r) p[r] = fma_(dt, Xs[r * N + j], p[r]);
        }
#pragma unroll
        for (int r = 0; r < N; ++r) p[N + r] = fma_(dt, p[r], p[N + r]);
        if (!upper) {
          T acc = T(0);
#pragma unroll
          for (int l = 0; l < N; ++l) {
            const T mu = dt * (integrator == 0 ? fma_(dt, lam_s[l], lam_s[N + l]) : lam_s[N + l]);
            acc = fma_(Ms[c * N + l], mu, acc);
          }
          nu_s[c] = acc;
          qu_s[c] = guv + acc;
        }
      }
      __syncthreads();
      // ---- row c of S = W M (M symmetric: column jj is row jj) -------------------------------------------------------
      if (live) {
#pragma nounroll
        for (int jj = 0; jj < N; ++jj) {
          const T* mr = Ms + jj * N;
          T a0 = T(0), a1 = T(0);
#pragma unroll
          for (int l = 0; l + 1 < N; l += 2) {
            a0 = fma_(x[l], mr[l], a0);
            a1 = fma_(x[l + 1], mr[l + 1], a1);
          }
          if (N & 1) a0 = fma_(x[N - 1], mr[N - 1], a0);
          Xs[c * N + jj] = a0 + a1;
        }
      }
      __syncthreads();
      // ---- C: column c of Y = S^T A0; half of column j of G = M (beta S[:N] + dt S[N:]); Qx --------------------------
      T qx = T(0);
      if (live) {
#pragma nounroll
        for (int i = 0; i < N; ++i) Ys[i * N2 + c] = upper ? fma_(dt, Xs[j * N + i], Xs[c * N + i]) : Xs[c * N + i];
#pragma unroll
        for (int l = 0; l < N; ++l) x[l] = fma_(beta, Xs[l * N + j], dt * Xs[(N + l) * N + j]);
        const int i0 = upper ? H : 0, i1 = upper ? N : H;
#pragma nounroll
        for (int i = i0; i < i1; ++i) {
          const T* mr = Ms + i * N;
          T a0 = T(0), a1 = T(0);
#pragma unroll
          for (int l = 0; l + 1 < N; l += 2) {
            a0 = fma_(mr[l], x[l], a0);
            a1 = fma_(mr[l + 1], x[l + 1], a1);
          }
          if (N & 1) a0 = fma_(mr[N - 1], x[N - 1], a0);
          Gs[i * N + j] = a0 + a1;
        }
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < N; ++i) acc = fma_(Ds[i * N2 + c], nu_s[i], acc);
        qx = (upper ? fma_(dt, lam_s[j], lv) : lv) - acc;
      }
      __syncthreads();
      // ---- D: p -= Y^T D[:, c];  Qux[:, c] = Y[:, c] - G D[:, c] (over Y);  p -= D^T Qux[:, c]  -> p = Qxx[:, c] -------
      if (live) {
#pragma nounroll
        for (int i = 0; i < N; ++i) {
          const T* yr = Ys + i * N2;
          const T di = -Ds[i * N2 + c];
#pragma unroll
          for (int r = 0; r < N2; ++r) {
            p[r] = fma_(yr[r], di, p[r]);
            lqr_row_fence<T>(r);
          }
        }
      }
      __syncthreads();
      if (live) {
#pragma unroll
        for (int l = 0; l < N; ++l) x[l] = Ds[l * N2 + c];
#pragma nounroll
        for (int i = 0; i < N; ++i) {
          const T* gr = Gs + i * N;
          T a0 = T(0), a1 = T(0);
#pragma unroll
          for (int l = 0; l + 1 < N; l += 2) {
            a0 = fma_(gr[l], x[l], a0);
            a1 = fma_(gr[l + 1], x[l + 1], a1);
          }
          if (N & 1) a0 = fma_(gr[N - 1], x[N - 1], a0);
          Ys[i * N2 + c] -= a0 + a1;
        }
      }
      __syncthreads();
      if (live) {
#pragma nounroll
        for (int i = 0; i < N; ++i) {
          const T* dr = Ds + i * N2;
          const T qi = -Ys[i * N2 + c];
#pragma unroll
          for (int r = 0; r < N2; ++r) {
            p[r] = fma_(dr[r], qi, p[r]);
            lqr_row_fence<T>(r);
          }
        }
        // row j of Quu + reg I (its lower triangle is what the factorisation reads)
#pragma unroll
        for (int l = 0; l < N; ++l) x[l] = Gs[j * N + l] + (l == jv ? hu_s[j] + reg : T(0));
      }
      // ---- E: Cholesky, left-looking; threads j and N + j both hold row j, the factor goes to M's place ---------------
      bool ok = true;
#pragma unroll
      for (int jj = 0; jj < N; ++jj) {
        T s = x[jj];
        if (live) {
          const T* lr = Ms + jj * N;
#pragma unroll
          for (int k = 0; k < jj; ++k) s = fma_(-x[k], lr[k], s);
          __builtin_amdgcn_sched_barrier(0);               // a row's LDS reads stay with the row (registers)
          if (cv == jj) piv_s[0] = s;
        }
        __syncthreads();
        if (live) {
          const T dd = piv_s[0];
          const bool good = dd > T(0) && dd - dd == T(0);
          ok = ok && good;
          const T ljj = good ? sqrt(dd) : T(1);
          const T inv = T(1) / ljj;
          x[jj] = (jv == jj) ? ljj : s * inv;
          if (cv >= jj && cv < N) Ms[j * N + jj] = x[jj];
          if (cv == jj) dinv_s[jj] = inv;
        }
        __syncthreads();
      }
      // ---- F: k = -(L L^T)^-1 Qu (every thread, the same numbers), then column c of K = -(L L^T)^-1 Qux ---------------
#pragma nounroll
      for (int pass = 0; pass < 2; ++pass) {
        if (live) {
#pragma unroll
          for (int i = 0; i < N; ++i) x[i] = pass == 0 ? qu_s[i] : Ys[i * N2 + c];
#pragma unroll
          for (int i = 0; i < N; ++i) {
            T s = x[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s = fma_(-Ms[i * N + k], x[k], s);
            x[i] = s * dinv_s[i];
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = N - 1; i >= 0; --i) {
            T s = x[i];
#pragma unroll
            for (int k = i + 1; k < N; ++k) s = fma_(-Ms[k * N + i], x[k], s);
            x[i] = s * dinv_s[i];
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < N; ++i) x[i] = ok ? -x[i] : T(0);
          if (pass == 0) {
            if (c == 0) {
#pragma unroll
              for (int i = 0; i < N; ++i) k_s[i] = x[i];
            }
          } else {
            T* Kp = Kout + (t * B + cfg) * rows_dc + c;
#pragma unroll
            for (int i = 0; i < N; ++i) {
              Xs[i * N2 + c] = x[i];
              Kp[i * N2] = x[i];
            }
          }
        }
      }
      __syncthreads();
      // ---- G: e = Quu k + Qu, the terms of dV; then lam ---------------------------------------------------------------
      if (live && !upper) {
        const T kc = k_s[c];
        T zk = hu_s[c] * kc;
#pragma unroll
        for (int l = 0; l < N; ++l) zk = fma_(Gs[c * N + l], k_s[l], zk);
        e_s[c] = zk + qu_s[c];
        dva_s[c] = kc * qu_s[c];
        dvb_s[c] = kc * zk;
        kout[(t * B + cfg) * row_n + c] = kc;
      }
      __syncthreads();
      if (live) {
        T a0 = T(0), a1 = T(0);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          a0 = fma_(x[i], e_s[i], a0);
          a1 = fma_(Ys[i * N2 + c], k_s[i], a1);
        }
        lv = qx + a0 + a1;
        if (c < 2) {
          const T* dp = c == 0 ? dva_s : dvb_s;
          T s = T(0);
#pragma unroll
          for (int i = 0; i < N; ++i) s += dp[i];
          dv += c == 0 ? s : T(0.5) * s;
        }
        if (c == 0) st += ok ? 0 : 1;
        // ---- H: p += K^T (Quu K[:, c] + Qux[:, c]) + Qux^T K[:, c] ----------------------------------------------------
#pragma nounroll
        for (int i = 0; i < N; ++i) {
          const T* gr = Gs + i * N;
          const T* kr = Xs + i * N2;
          const T* yr = Ys + i * N2;
          T b0 = T(0), b1 = T(0);
#pragma unroll
          for (int l = 0; l + 1 < N; l += 2) {
            b0 = fma_(gr[l], x[l], b0);
            b1 = fma_(gr[l + 1], x[l + 1], b1);
          }
          if (N & 1) b0 = fma_(gr[N - 1], x[N - 1], b0);
          const T ki = kr[c];
          const T ei = fma_(hu_s[i], ki, b0 + b1) + yr[c];
#pragma unroll
          for (int r = 0; r < N2; ++r) {
            p[r] = fma_(yr[r], ki, fma_(kr[r], ei, p[r]));
            lqr_row_fence<T>(r);
          }
        }
      }
      __syncthreads();
      // ---- I: P = 1/2 (P + P^T) through LDS ---------------------------------------------------------------------------
      if (live) {
#pragma unroll
        for (int r = 0; r < N2; ++r) Zs[r * ZS + c] = p[r];
      }
      __syncthreads();
      if (live) {
#pragma unroll
        for (int r = 0; r < N2; ++r) p[r] = T(0.5) * (p[r] + Zs[c * ZS + r]);
      }
      __syncthreads();
      if constexpr (lqr_prefetch<T>()) {
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = dn[i];
#pragma unroll
        for (int k = 0; k < H; ++k) m[k] = mn[k];
        g = gn; h = hn; guv = gun; huv = hun;
      }
    }
    if (live) {
      lam[cfg * N2 + c] = lv;
      T* pp = P + cfg * (long long)(N2 * N2) + c;
#pragma unroll
      for (int r = 0; r < N2; ++r) pp[r * N2] = p[r];
      if (c < 2) dV[cfg * 2 + c] = dv;
      if (c == 0) status[cfg] = st;
    }
  }
}

}  // namespace rbdk
