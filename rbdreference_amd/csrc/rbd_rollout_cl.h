// rbd_rollout_cl.h -- closed-loop rollout: the forward pass of iLQR / DDP / a time-varying LQR tracking controller, T
// integration steps in one launch with the control law INSIDE the time loop, one configuration per lane (gfx950).
//
//   x_t = (q_t | qd_t);   dx = x_t - xref_t          (xref_0 = (q0_ref | qd0_ref), xref_t = slice t - 1 of (q_ref | qd_ref))
//   u_t = ubar[t] + alpha k[t] + K[t] dx             (K[t]: n x 2n, the layout rbd_rollout_lqr writes; alpha per row)
//   u_t = u_t < u_lo ? u_lo : (u_t > u_hi ? u_hi : u_t)     per joint, when limits are given; a NaN stays a NaN
//   qdd = aba(q_t, qd_t, u_t, GRAVITY), then roll_step of rbd_rollout.h
//
// Row r of the rollout reads row r % B_nom of everything that belongs to the nominal (ubar, k, K, the reference); its own
// q0, qd0, alpha.  The control of joint j is ONE chain of fused multiply-adds in a fixed order -- fma(alpha, k_j, ubar_j),
// then c = 0 .. 2n - 1 -- on values the lane loads itself, so a row's arithmetic does not depend on B, B_nom or the lane
// it runs in.  The row of K[t] (2 n^2 contiguous scalars) is read by its lane with plain loads: consecutive loads of a
// lane walk the same cache lines, and lanes that share a nominal row hit the lines another lane has brought in.
// The state has the two homes of rbd_rollout.h:
//   registers  RollRegs as it is (tauv holds the applied control); step t + 1's ubar, k and reference rows are loaded
//              right after step t's control is formed, so the sweeps hide them; q, qd and u_applied leave through
//              roll_store
//   parked     the feedback couples the root subtrees (every joint's u depends on every joint's dx), so ONE block takes a
//              tile through all of its subtrees, group after group, each step: all N bodies x (aba's slots, q, qd, u) in
//              lane-private LDS columns.  The block has ROLLCL_WAVES waves: every wave forms the controls of its share
//              of the joints (a run-time loop over the joints; a column is read by any wave without conflicts), then
//              wave 0 runs the sweeps while the others stream u_applied out; two block barriers per step, whole
//              [cfg][N] rows stored cooperatively
#pragma once
#include "rbd_rollout.h"

namespace rbdk {

constexpr int ROLLCL_SLOTS = ABA_SLOTS + 3;          // parked: aba's slots, then q, qd, u
template <class T>
constexpr int rollcl_lanes() {                       // configurations per block when parked (the rule of roll_lanes, all N rows)
  int l = 64;
  while (l > 8 && (size_t)N * ROLLCL_SLOTS * l * sizeof(T) > 160u * 1024u) l /= 2;
  return l;
}
// parked: the waves of a block share the joints of the control law; wave 0 runs the sweeps
constexpr int ROLLCL_WAVES = ABA_PARK ? 4 : 1;
constexpr int ROLLCL_THREADS = 64 * ROLLCL_WAVES;
template <class T>
constexpr size_t rollcl_lds_bytes() {
  const size_t park = ABA_PARK ? (size_t)N * ROLLCL_SLOTS * rollcl_lanes<T>() * sizeof(T) : 0;
  const size_t stage = (size_t)64 * odd_pad<N>() * sizeof(T);
  return park > stage ? park : stage;
}

template <class T, int LANES>
struct RollClParked {
  T* base;              // lds + lane; aba's slot K = I * ABA_SLOTS + s sits at (I * ROLLCL_SLOTS + s) * LANES
  static constexpr int at(int k) { return ((k / ABA_SLOTS) * ROLLCL_SLOTS + k % ABA_SLOTS) * LANES; }
  static constexpr int own(int i, int s) { return (i * ROLLCL_SLOTS + s) * LANES; }
  template <int K> RBD_DEV void put(T x) { base[at(K)] = x; }
  template <int K> RBD_DEV T get() const { return base[at(K)]; }
  template <int I> RBD_DEV JTrig<T> trig() const { return JTrig<T>{base[own(I, 12)], base[own(I, 13)]}; }
  template <int I> RBD_DEV T qd() const { return base[own(I, ABA_SLOTS + 1)]; }
  template <int I> RBD_DEV T tau() const { return base[own(I, ABA_SLOTS + 2)]; }
  template <int I> RBD_DEV void set_qdd(T x) { base[own(I, 0)] = x; }
};

// the joint limits: ordered comparisons, so a NaN passes through unchanged
template <class T>
RBD_DEV T rollcl_clamp(T u, T lo, T hi) { return u < lo ? lo : (u > hi ? hi : u); }

// Pointers of the nominal (ubar, k, K, q0_ref, qd0_ref, q_ref, qd_ref) have B_nom rows per step; alpha has B.  k and alpha
// are null together (no feed-forward term), u_lo and u_hi are null together (no limits), u_out may be null.  row = B n:
// elements between consecutive slices of an output; trajectory == 0 keeps the final state only (q_out, qd_out [B, n],
// stored once after the loop) -- u_out is [T, B, n] either way.
template <class T>
__global__ __launch_bounds__(ROLLCL_THREADS) void rollout_closed_loop_kernel(
    const T* __restrict__ q0, const T* __restrict__ qd0, const T* __restrict__ ubar, const T* __restrict__ kff,
    const T* __restrict__ Kfb, const T* __restrict__ q0_ref, const T* __restrict__ qd0_ref, const T* __restrict__ q_ref,
    const T* __restrict__ qd_ref, const T* __restrict__ alpha, const T* __restrict__ u_lo, const T* __restrict__ u_hi, T dt,
    T grav, int integrator, long long B, long long B_nom, long long steps, T* __restrict__ q_out, T* __restrict__ qd_out,
    int trajectory, T* __restrict__ u_out, long long row, int aligned) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int LANES = ABA_PARK ? rollcl_lanes<T>() : 64;
  constexpr int N2 = 2 * N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cfg0 = (long long)blockIdx.x * LANES;
  const long long rem = B - cfg0;
  const int nvalid = rem < LANES ? (int)rem : LANES;
  const long long b = cfg0 + (lane < nvalid ? lane : nvalid - 1);
  const long long bn = b % B_nom;                 // this row's row of the nominal
  const long long nom_step = B_nom * N;           // elements between the nominal's rows of consecutive steps
  const T* ub_mine = ubar + bn * N;
  const T* kf_mine = kff ? kff + bn * N : nullptr;
  const T* K_mine = Kfb + bn * N * N2;
  const T al = alpha ? alpha[b] : T(0);
  const bool limits = u_lo != nullptr;
  // the reference state the control of step t is measured against
  auto qref_at = [&](long long t) { return t == 0 ? q0_ref + bn * N : q_ref + (t - 1) * nom_step + bn * N; };
  auto qdref_at = [&](long long t) { return t == 0 ? qd0_ref + bn * N : qd_ref + (t - 1) * nom_step + bn * N; };

  if constexpr (ABA_PARK) {
    using St = RollClParked<T, LANES>;
    T* mine = lds + (lane < LANES ? lane : 0);
    if (wave == 0 && lane < LANES) {
      sfor<0, N>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const T qj = q0[b * N + j];
        const JTrig<T> g = make_trig<j>(qj);
        mine[St::own(j, 12)] = g.s;
        mine[St::own(j, 13)] = g.c;
        mine[St::own(j, ABA_SLOTS)] = qj;
        mine[St::own(j, ABA_SLOTS + 1)] = qd0[b * N + j];
      });
    }
    __syncthreads();
#pragma nounroll
    for (long long t = 0; t < steps; ++t) {
      if (lane < LANES) {
        // ---- the control law: wave w forms the controls of joints w, w + ROLLCL_WAVES, ... of the tile's configurations
        // (the K stream of a step is the long pole: four waves keep four times the loads in flight); dx in registers, one
        // joint per trip of a run-time loop (its 2n products unrolled, the same chain whichever wave runs it) ----
        T dx[N2];
        {
          const T* qr = qref_at(t);
          const T* qdr = qdref_at(t);
          sfor<0, N>([&](auto C) {
            constexpr int c = decltype(C)::value;
            dx[c] = mine[St::own(c, ABA_SLOTS)] - qr[c];
            dx[N + c] = mine[St::own(c, ABA_SLOTS + 1)] - qdr[c];
          });
        }
        const T* ub_t = ub_mine + t * nom_step;
        const T* kf_t = kf_mine ? kf_mine + t * nom_step : nullptr;
        const T* K_t = K_mine + t * nom_step * N2;
#pragma nounroll
        for (int j = wave; j < N; j += ROLLCL_WAVES) {
          T acc = ub_t[j];
          if (kf_t) acc = fma_(al, kf_t[j], acc);
          const T* Kj = K_t + j * N2;
          sfor<0, N2>([&](auto C) { constexpr int c = decltype(C)::value; acc = fma_(Kj[c], dx[c], acc); });
          if (limits) acc = rollcl_clamp(acc, u_lo[j], u_hi[j]);
          mine[(j * ROLLCL_SLOTS + ABA_SLOTS + 2) * LANES] = acc;
        }
      }
      __syncthreads();     // the step's controls are parked
      if (wave == 0) {
        if (lane < LANES) {
          // ---- the sweeps, root subtree after root subtree, then the integrator: wave 0, lane-private columns ----
          St st{mine};
          sfor<0, N>([&](auto Rt) {
            constexpr int rt = decltype(Rt)::value;
            if constexpr (grp_head(rt)) aba_group<T, grp_row0(rt), grp_rows(rt)>(grav, st);
          });
          sfor<0, N>([&](auto J) {
            constexpr int j = decltype(J)::value;
            T qj = mine[St::own(j, ABA_SLOTS)], qdj = mine[St::own(j, ABA_SLOTS + 1)];
            roll_step(dt, integrator, mine[St::own(j, 0)], qj, qdj);
            mine[St::own(j, ABA_SLOTS)] = qj;
            mine[St::own(j, ABA_SLOTS + 1)] = qdj;
            const JTrig<T> g = make_trig<j>(qj);
            mine[St::own(j, 12)] = g.s;
            mine[St::own(j, 13)] = g.c;
          });
        }
      } else if (u_out != nullptr) {
        // meanwhile the other waves stream the applied controls out (read-only during the sweeps): whole rows
        // u_out[t][cfg0 + cfg][i]
        T* uo = u_out + t * row + cfg0 * N;
        for (int g = (int)threadIdx.x - 64; g < nvalid * N; g += ROLLCL_THREADS - 64) {
          const int cfg = g / N;
          const int i = g - cfg * N;
          uo[g] = lds[(i * ROLLCL_SLOTS + ABA_SLOTS + 2) * LANES + cfg];
        }
      }
      __syncthreads();     // the new state is parked, the controls are out
      if (trajectory != 0 || t == steps - 1) {
        // q, qd sit in two slots of every body -> whole rows out[t][cfg0 + cfg][i]; the next step's control law only reads
        // them, and its sweeps start behind the next barrier
        T* qo = q_out + (trajectory != 0 ? t * row : 0) + cfg0 * N;
        T* qdo = qd_out + (trajectory != 0 ? t * row : 0) + cfg0 * N;
        for (int g = threadIdx.x; g < nvalid * N; g += ROLLCL_THREADS) {
          const int cfg = g / N;
          const int i = g - cfg * N;
          const T* src = lds + (i * ROLLCL_SLOTS + ABA_SLOTS) * LANES + cfg;
          qo[g] = src[0];
          qdo[g] = src[LANES];
        }
      }
    }
  } else {
    RollRegs<T> st;
    T ub[N], kf[N], qr[N], qdr[N];     // the nominal's rows of the step whose control is formed next
    sfor<0, N>([&](auto J) {
      constexpr int j = decltype(J)::value;
      st.qv[j] = q0[b * N + j];
      st.qdv[j] = qd0[b * N + j];
      ub[j] = ub_mine[j];
      kf[j] = kf_mine ? kf_mine[j] : T(0);
      qr[j] = q0_ref[bn * N + j];
      qdr[j] = qd0_ref[bn * N + j];
    });
#pragma nounroll
    for (long long t = 0; t < steps; ++t) {
      // ---- the control law ----
      T dx[N2];
      sfor<0, N>([&](auto C) {
        constexpr int c = decltype(C)::value;
        dx[c] = st.qv[c] - qr[c];
        dx[N + c] = st.qdv[c] - qdr[c];
      });
      const T* K_t = K_mine + t * nom_step * N2;
      sfor<0, N>([&](auto J) {
        constexpr int j = decltype(J)::value;
        T acc = ub[j];
        if (kf_mine) acc = fma_(al, kf[j], acc);
        sfor<0, N2>([&](auto C) { constexpr int c = decltype(C)::value; acc = fma_(K_t[j * N2 + c], dx[c], acc); });
        if (limits) acc = rollcl_clamp(acc, u_lo[j], u_hi[j]);
        st.tauv[j] = acc;
      });
      // the next step's rows of the nominal (the last step reloads its own): in flight while the sweeps run
      {
        const long long tn = t + 1 < steps ? t + 1 : t;
        const T* ub_n = ub_mine + tn * nom_step;
        const T* kf_n = kf_mine ? kf_mine + tn * nom_step : nullptr;
        const T* qr_n = qref_at(tn);
        const T* qdr_n = qdref_at(tn);
        sfor<0, N>([&](auto J) {
          constexpr int j = decltype(J)::value;
          ub[j] = ub_n[j];
          if (kf_n) kf[j] = kf_n[j];
          qr[j] = qr_n[j];
          qdr[j] = qdr_n[j];
        });
      }
      sfor<0, N>([&](auto J) { constexpr int j = decltype(J)::value; st.tr[j] = make_trig<j>(st.qv[j]); });
      sfor<0, N>([&](auto Rt) {
        constexpr int rt = decltype(Rt)::value;
        if constexpr (grp_head(rt)) aba_group<T, grp_row0(rt), grp_rows(rt)>(grav, st);
      });
      sfor<0, N>([&](auto J) {
        constexpr int j = decltype(J)::value;
        roll_step(dt, integrator, st.qddv[j], st.qv[j], st.qdv[j]);
      });
      if (trajectory != 0) {
        roll_store<N>(lds, st.qv, q_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
        roll_store<N>(lds, st.qdv, qd_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
      }
      if (u_out != nullptr) roll_store<N>(lds, st.tauv, u_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
    }
    if (trajectory == 0) {
      staged_store<N>(lds, st.qv, q_out + cfg0 * N, lane, nvalid);
      staged_store<N>(lds, st.qdv, qd_out + cfg0 * N, lane, nvalid);
    }
  }
}

}  // namespace rbdk
