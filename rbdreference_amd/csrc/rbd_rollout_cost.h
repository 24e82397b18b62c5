// rbd_rollout_cost.h -- a rollout, open or closed loop, whose quadratic tracking cost is accumulated INSIDE the time loop:
// the line search of iLQR / DDP and the sample costs of a sampling controller (MPPI) in one launch that writes J [B] and,
// unless asked, nothing else (gfx950).  The time loop is rollout_closed_loop_kernel's (rbd_rollout_cl.h) around the
// unchanged aba_group; what differs:
//
//   u_t,j = fma(alpha, k_j, ubar_j), then + du_j, then the 2n products of K[t] dx (c = 0 .. 2n - 1), then the limits
//           k, du, K, the limits: each optional.  K == null is an OPEN loop: the reference state is not read.
//           du [T, B, n] belongs to the ROW (a sampler's perturbation of a nominal it shares through B_nom)
//   J = sum_t sum_j  1/2 w_u[t,j] u_t,j^2 + c_u[t,j] u_t,j  +  1/2 w_q[t,j] (q_{t+1,j} - q_tgt[t,j])^2
//                                                            +  1/2 w_qd[t,j] (qd_{t+1,j} - qd_tgt[t,j])^2
//           (u_t the control applied, after the limits; slice t = the state after step t).  The six arrays belong to the
//           nominal (row r reads row r % B_nom); w_u, c_u [T, B_nom, n]; the four state arrays [T, B_nom, n], or
//           [B_nom, n] with x_final_only (slice T - 1 alone).  A null weight drops its term, a null target or c_u is zero.
//
// The accumulation is ONE chain per row in a fixed order -- for t = 0 .. T - 1: the control terms j = 0 .. n - 1 (for each
// j: J = fma((w_u/2 u) , u, J), then J = fma(c_u, u, J)), then the q terms j = 0 .. n - 1 (d = q - q_tgt,
// J = fma((w_q/2 d), d, J)), then the qd terms j = 0 .. n - 1 -- on values the lane loads itself, so a row's J does not depend
// on B, B_nom, the lane or block it runs in, or on which optional outputs are stored.
//
// Why the controls come first: in the parked home the u slots of step t are overwritten by the control law of step t + 1,
// and no barrier sits between the q / qd store phase and that control law.  So the u terms are read between the two
// barriers of step t (where waves 1-3 stream u_applied out), and the state terms behind the second barrier, where q and qd
// are read-only until the next sweeps.  The chain belongs to wave 1, lanes < LANES: wave 0's sweeps are where the register
// file is full.  In the register home the lane that owns the row owns its chain.
#pragma once
#include "rbd_rollout_cl.h"

namespace rbdk {

// the cost's arrays (any may be null) and the two optional inputs the closed-loop kernel does not have
template <class T>
struct RollCostModel {
  const T* q_tgt;
  const T* qd_tgt;
  const T* w_q;
  const T* w_qd;
  const T* w_u;
  const T* c_u;
  int x_final_only;
};

// one control term and one state term of the chain (the only two places that round the cost)
template <class T>
RBD_DEV T rollcost_u(T J, const T* w, const T* c, int j, T u) {
  if (w) J = fma_((T(0.5) * w[j]) * u, u, J);
  if (c) J = fma_(c[j], u, J);
  return J;
}
template <class T>
RBD_DEV T rollcost_x(T J, const T* w, const T* tgt, int j, T x) {
  const T d = tgt ? x - tgt[j] : x;
  return fma_((T(0.5) * w[j]) * d, d, J);
}

// Pointers of the nominal (ubar, k, K, the reference, the cost) have B_nom rows per step; q0, qd0, alpha, du and the outputs
// have B.  k and alpha are null together, u_lo and u_hi are null together, q_out and qd_out are null together; K == null:
// open loop.  row = B n: elements between consecutive slices of du and of an output; trajectory == 0 keeps the final state
// only (q_out, qd_out [B, n]) -- u_out is [T, B, n] either way.
template <class T>
__global__ __launch_bounds__(ROLLCL_THREADS) void rollout_cost_kernel(
    const T* __restrict__ q0, const T* __restrict__ qd0, const T* __restrict__ ubar, const T* __restrict__ kff,
    const T* __restrict__ Kfb, const T* __restrict__ q0_ref, const T* __restrict__ qd0_ref, const T* __restrict__ q_ref,
    const T* __restrict__ qd_ref, const T* __restrict__ alpha, const T* __restrict__ du, const T* __restrict__ u_lo,
    const T* __restrict__ u_hi, RollCostModel<T> cm, T dt, T grav, int integrator, long long B, long long B_nom,
    long long steps, T* __restrict__ cost, T* __restrict__ q_out, T* __restrict__ qd_out, int trajectory,
    T* __restrict__ u_out, long long row, int aligned) {
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
  const T* du_mine = du ? du + b * N : nullptr;
  const T* K_mine = Kfb ? Kfb + bn * N * N2 : nullptr;
  const T al = alpha ? alpha[b] : T(0);
  const bool limits = u_lo != nullptr;
  const bool closed = Kfb != nullptr;
  const bool store_x = q_out != nullptr;
  // the reference state the control of step t is measured against (closed loop only)
  auto qref_at = [&](long long t) { return t == 0 ? q0_ref + bn * N : q_ref + (t - 1) * nom_step + bn * N; };
  auto qdref_at = [&](long long t) { return t == 0 ? qd0_ref + bn * N : qd_ref + (t - 1) * nom_step + bn * N; };
  // the cost's rows of step t for this row of the nominal
  const bool state_cost = cm.w_q != nullptr || cm.w_qd != nullptr;
  auto state_off = [&](long long t) { return (cm.x_final_only ? 0 : t * nom_step) + bn * N; };
  auto has_state = [&](long long t) { return state_cost && (!cm.x_final_only || t == steps - 1); };
  T J = T(0);

  if constexpr (ABA_PARK) {
    using St = RollClParked<T, LANES>;
    T* mine = lds + (lane < LANES ? lane : 0);
    if (wave == 0 && lane < LANES) {
      sfor<0, N>([&](auto Jt) {
        constexpr int j = decltype(Jt)::value;
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
        // ---- the control law: wave w forms the controls of joints w, w + ROLLCL_WAVES, ... (rbd_rollout_cl.h) ----
        T dx[N2];
        if (closed) {
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
        const T* du_t = du_mine ? du_mine + t * row : nullptr;
#pragma nounroll
        for (int j = wave; j < N; j += ROLLCL_WAVES) {
          T acc = ub_t[j];
          if (kf_t) acc = fma_(al, kf_t[j], acc);
          if (du_t) acc += du_t[j];
          if (closed) {
            const T* Kj = K_mine + t * nom_step * N2 + j * N2;
            sfor<0, N2>([&](auto C) { constexpr int c = decltype(C)::value; acc = fma_(Kj[c], dx[c], acc); });
          }
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
          sfor<0, N>([&](auto Jt) {
            constexpr int j = decltype(Jt)::value;
            T qj = mine[St::own(j, ABA_SLOTS)], qdj = mine[St::own(j, ABA_SLOTS + 1)];
            roll_step(dt, integrator, mine[St::own(j, 0)], qj, qdj);
            mine[St::own(j, ABA_SLOTS)] = qj;
            mine[St::own(j, ABA_SLOTS + 1)] = qdj;
            const JTrig<T> g = make_trig<j>(qj);
            mine[St::own(j, 12)] = g.s;
            mine[St::own(j, 13)] = g.c;
          });
        }
      } else {
        // meanwhile wave 1 adds the step's control terms to its rows' chains (the u slots are read-only until the next
        // control law; eight joints per trip, so that the loads of the weights -- which do not wait for the chain -- are
        // in flight together) ...
        if (wave == 1 && lane < LANES && (cm.w_u != nullptr || cm.c_u != nullptr)) {
          const T* wu = cm.w_u ? cm.w_u + t * nom_step + bn * N : nullptr;
          const T* cu = cm.c_u ? cm.c_u + t * nom_step + bn * N : nullptr;
#pragma unroll 8
          for (int j = 0; j < N; ++j) J = rollcost_u(J, wu, cu, j, mine[(j * ROLLCL_SLOTS + ABA_SLOTS + 2) * LANES]);
        }
        // ... and waves 1-3 stream the applied controls out: whole rows u_out[t][cfg0 + cfg][i]
        if (u_out != nullptr) {
          T* uo = u_out + t * row + cfg0 * N;
          for (int g = (int)threadIdx.x - 64; g < nvalid * N; g += ROLLCL_THREADS - 64) {
            const int cfg = g / N;
            const int i = g - cfg * N;
            uo[g] = lds[(i * ROLLCL_SLOTS + ABA_SLOTS + 2) * LANES + cfg];
          }
        }
      }
      __syncthreads();     // the new state is parked, the controls are out
      // the state terms: q, qd are read-only until the sweeps behind the next step's first barrier
      if (wave == 1 && lane < LANES && has_state(t)) {
        const long long off = state_off(t);
        if (cm.w_q) {
          const T* w = cm.w_q + off;
          const T* tg = cm.q_tgt ? cm.q_tgt + off : nullptr;
#pragma unroll 8
          for (int j = 0; j < N; ++j) J = rollcost_x(J, w, tg, j, mine[(j * ROLLCL_SLOTS + ABA_SLOTS) * LANES]);
        }
        if (cm.w_qd) {
          const T* w = cm.w_qd + off;
          const T* tg = cm.qd_tgt ? cm.qd_tgt + off : nullptr;
#pragma unroll 8
          for (int j = 0; j < N; ++j) J = rollcost_x(J, w, tg, j, mine[(j * ROLLCL_SLOTS + ABA_SLOTS + 1) * LANES]);
        }
      }
      if (store_x && (trajectory != 0 || t == steps - 1)) {
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
    if (wave == 1 && lane < nvalid) cost[cfg0 + lane] = J;
  } else {
    RollRegs<T> st;
    T ub[N], kf[N], qr[N], qdr[N];     // the nominal's rows of the step whose control is formed next
    // (open loop: the reference registers are loaded all the same, from the row's own start -- a load that is always valid
    // keeps the loop free of branches around register arrays -- and never used)
    const T* qr0 = closed ? q0_ref + bn * N : q0 + b * N;
    const T* qdr0 = closed ? qd0_ref + bn * N : qd0 + b * N;
    sfor<0, N>([&](auto Jt) {
      constexpr int j = decltype(Jt)::value;
      st.qv[j] = q0[b * N + j];
      st.qdv[j] = qd0[b * N + j];
      ub[j] = ub_mine[j];
      kf[j] = (kf_mine ? kf_mine : ub_mine)[j];
      qr[j] = qr0[j];
      qdr[j] = qdr0[j];
    });
#pragma nounroll
    for (long long t = 0; t < steps; ++t) {
      // ---- the control law ----
      const T* du_t = du_mine ? du_mine + t * row : nullptr;
      sfor<0, N>([&](auto Jt) {
        constexpr int j = decltype(Jt)::value;
        T acc = ub[j];
        if (kf_mine) acc = fma_(al, kf[j], acc);
        if (du_t) acc += du_t[j];
        st.tauv[j] = acc;
      });
      if (closed) {
        T dx[N2];
        sfor<0, N>([&](auto C) {
          constexpr int c = decltype(C)::value;
          dx[c] = st.qv[c] - qr[c];
          dx[N + c] = st.qdv[c] - qdr[c];
        });
        const T* K_t = K_mine + t * nom_step * N2;
        sfor<0, N>([&](auto Jt) {
          constexpr int j = decltype(Jt)::value;
          T acc = st.tauv[j];
          sfor<0, N2>([&](auto C) { constexpr int c = decltype(C)::value; acc = fma_(K_t[j * N2 + c], dx[c], acc); });
          st.tauv[j] = acc;
        });
      }
      if (limits) sfor<0, N>([&](auto Jt) { constexpr int j = decltype(Jt)::value; st.tauv[j] = rollcl_clamp(st.tauv[j], u_lo[j], u_hi[j]); });
      // the step's control terms of the chain
      if (cm.w_u != nullptr || cm.c_u != nullptr) {
        const T* wu = cm.w_u ? cm.w_u + t * nom_step + bn * N : nullptr;
        const T* cu = cm.c_u ? cm.c_u + t * nom_step + bn * N : nullptr;
        sfor<0, N>([&](auto Jt) { constexpr int j = decltype(Jt)::value; J = rollcost_u(J, wu, cu, j, st.tauv[j]); });
      }
      // the next step's rows of the nominal (the last step reloads its own): in flight while the sweeps run
      {
        const long long tn = t + 1 < steps ? t + 1 : t;
        const T* ub_n = ub_mine + tn * nom_step;
        const T* kf_n = kf_mine ? kf_mine + tn * nom_step : ub_n;      // (no k: loaded from a valid row, never used)
        sfor<0, N>([&](auto Jt) {
          constexpr int j = decltype(Jt)::value;
          ub[j] = ub_n[j];
          kf[j] = kf_n[j];
        });
        const T* qr_n = closed ? qref_at(tn) : qr0;
        const T* qdr_n = closed ? qdref_at(tn) : qdr0;
        sfor<0, N>([&](auto Jt) {
          constexpr int j = decltype(Jt)::value;
          qr[j] = qr_n[j];
          qdr[j] = qdr_n[j];
        });
      }
      sfor<0, N>([&](auto Jt) { constexpr int j = decltype(Jt)::value; st.tr[j] = make_trig<j>(st.qv[j]); });
      sfor<0, N>([&](auto Rt) {
        constexpr int rt = decltype(Rt)::value;
        if constexpr (grp_head(rt)) aba_group<T, grp_row0(rt), grp_rows(rt)>(grav, st);
      });
      sfor<0, N>([&](auto Jt) {
        constexpr int j = decltype(Jt)::value;
        roll_step(dt, integrator, st.qddv[j], st.qv[j], st.qdv[j]);
      });
      // the state terms of the chain
      if (has_state(t)) {
        const long long off = state_off(t);
        if (cm.w_q) {
          const T* w = cm.w_q + off;
          const T* tg = cm.q_tgt ? cm.q_tgt + off : nullptr;
          sfor<0, N>([&](auto Jt) { constexpr int j = decltype(Jt)::value; J = rollcost_x(J, w, tg, j, st.qv[j]); });
        }
        if (cm.w_qd) {
          const T* w = cm.w_qd + off;
          const T* tg = cm.qd_tgt ? cm.qd_tgt + off : nullptr;
          sfor<0, N>([&](auto Jt) { constexpr int j = decltype(Jt)::value; J = rollcost_x(J, w, tg, j, st.qdv[j]); });
        }
      }
      if (store_x && trajectory != 0) {
        roll_store<N>(lds, st.qv, q_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
        roll_store<N>(lds, st.qdv, qd_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
      }
      if (u_out != nullptr) roll_store<N>(lds, st.tauv, u_out + t * row + cfg0 * N, lane, nvalid, aligned != 0);
    }
    if (store_x && trajectory == 0) {
      staged_store<N>(lds, st.qv, q_out + cfg0 * N, lane, nvalid);
      staged_store<N>(lds, st.qdv, qd_out + cfg0 * N, lane, nvalid);
    }
    if (lane < nvalid) cost[cfg0 + lane] = J;
  }
}

}  // namespace rbdk
