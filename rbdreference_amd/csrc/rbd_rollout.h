// rbd_rollout.h -- forward-simulation rollout: T integration steps of the articulated-body algorithm in one launch,
// one configuration per lane (gfx950).
//
//   qdd_t = aba(q_t, qd_t, u_t, GRAVITY)                               (aba_group of rbd_aba.h, unchanged)
//   semi-implicit Euler (integrator 0): qd_{t+1} = qd_t + dt qdd_t, then q_{t+1} = q_t + dt qd_{t+1}
//   explicit Euler      (integrator 1): q_{t+1} = q_t + dt qd_t,         qd_{t+1} = qd_t + dt qdd_t
//
// A RUN-TIME loop over t around aba_group (not unrolled: the code stays the size of aba_kernel's).  q and qd never leave
// the chip between steps: per step and configuration the kernel reads u_t (n scalars) and, when the trajectory is
// wanted, writes the new state (2 n scalars).  Everything with a time axis is time-major -- u [T, B, n] (or [T, n], one
// sequence for every row), trajectories [T, B, n] -- so a step's read and write are the flat [B, n] tile of every other
// entry point.  The state has the two homes of rbd_aba.h:
//   registers  RollRegs = AbaRegs + q[N]; step t + 1's u row is loaded before step t's sweeps, so the dependent chain of
//              the sweeps hides the load; one staged_store each for q and qd per step
//   parked     RollParked = AbaParked with two more lane-private LDS slots per body (q, qd); tau() reads the step's u
//              row; one block per (tile, root subtree) runs its group through all T steps (the subtrees of a fixed-base
//              robot never interact); per step a block barrier and the cooperative row store of aba_kernel
#pragma once
#include "rbd_aba.h"

namespace rbdk {

constexpr int ROLL_SLOTS = ABA_SLOTS + 2;            // parked: aba's slots, then q (ABA_SLOTS) and qd (ABA_SLOTS + 1)
template <class T>
constexpr int roll_lanes() {                         // configurations per block when parked (the rule of aba_lanes)
  int l = 64;
  while (l > 8 && (size_t)ABA_PARK_ROWS * ROLL_SLOTS * l * sizeof(T) > 160u * 1024u) l /= 2;
  return l;
}
template <class T>
constexpr size_t roll_lds_bytes() {
  const size_t park = ABA_PARK ? (size_t)ABA_PARK_ROWS * ROLL_SLOTS * roll_lanes<T>() * sizeof(T) : 0;
  const size_t stage = (size_t)64 * odd_pad<N>() * sizeof(T);
  return park > stage ? park : stage;
}

template <class T>
struct RollRegs {
  JTrig<T> tr[N];
  T qv[N], qdv[N], tauv[N], qddv[N];
  T r[N * ABA_SLOTS];
  template <int K> RBD_DEV void put(T x) { r[K] = x; }
  template <int K> RBD_DEV T get() const { return r[K]; }
  template <int I> RBD_DEV JTrig<T> trig() const { return tr[I]; }
  template <int I> RBD_DEV T qd() const { return qdv[I]; }
  template <int I> RBD_DEV T tau() const { return tauv[I]; }
  template <int I> RBD_DEV void set_qdd(T x) { qddv[I] = x; }
};
template <class T, int LANES, int ROW0>
struct RollParked {
  T* base;              // lds + lane; aba's slot K = I * ABA_SLOTS + s sits at ((I - ROW0) * ROLL_SLOTS + s) * LANES
  const T* tau_row;     // this step's u row
  static constexpr int at(int k) { return ((k / ABA_SLOTS - ROW0) * ROLL_SLOTS + k % ABA_SLOTS) * LANES; }
  static constexpr int own(int i, int s) { return ((i - ROW0) * ROLL_SLOTS + s) * LANES; }
  template <int K> RBD_DEV void put(T x) { base[at(K)] = x; }
  template <int K> RBD_DEV T get() const { return base[at(K)]; }
  template <int I> RBD_DEV JTrig<T> trig() const { return JTrig<T>{base[own(I, 12)], base[own(I, 13)]}; }
  template <int I> RBD_DEV T qd() const { return base[own(I, ABA_SLOTS + 1)]; }
  template <int I> RBD_DEV T tau() const { return tau_row[I]; }
  template <int I> RBD_DEV void set_qdd(T x) { base[own(I, 0)] = x; }
};

// one integration step of one joint: (q, qd, qdd) -> (q', qd'), each update one fused multiply-add
template <class T>
RBD_DEV void roll_step(T dt, int integrator, T qdd, T& q, T& qd) {
  const T qd_new = fma_(dt, qdd, qd);
  q = fma_(dt, integrator == 0 ? qd_new : qd, q);
  qd = qd_new;
}

// staged_store for a destination that may sit at any element offset (slice t of a trajectory starts t B n elements
// into the buffer: 16-byte aligned only when B n is a multiple of 16 bytes); same coalesced rows, element-wise
template <int K, class T>
RBD_DEV void roll_store(T* lds, const T (&vals)[K], T* gdst, int lane, int nvalid, bool aligned) {
  if (aligned) {
    staged_store<K>(lds, vals, gdst, lane, nvalid);
    return;
  }
  constexpr int KP = odd_pad<K>();
  __syncthreads();
  sfor<0, K>([&](auto I) { lds[lane * KP + decltype(I)::value] = vals[decltype(I)::value]; });
  __syncthreads();
  const int total = nvalid * K;
#pragma unroll 4
  for (int g = lane; g < total; g += 64) {
    const int cfg = g / K;
    gdst[g] = lds[cfg * KP + (g - cfg * K)];
  }
}

// u_step: elements between the u rows of consecutive steps (B n, or n for a shared sequence); u_shared: every
// configuration reads row 0 of a step.  slice: elements between consecutive trajectory slices (B n; 0 = keep the
// final state only, which is then stored once after the loop).
template <class T>
__global__ __launch_bounds__(64) void rollout_kernel(const T* __restrict__ q0, const T* __restrict__ qd0,
                                                     const T* __restrict__ u, long long u_step, int u_shared, T dt, T grav,
                                                     int integrator, long long B, long long steps, T* __restrict__ q_out,
                                                     T* __restrict__ qd_out, long long slice, int aligned) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int LANES = ABA_PARK ? roll_lanes<T>() : 64;
  const int lane = threadIdx.x;
  const long long cfg0 = (long long)blockIdx.x * LANES;
  const long long rem = B - cfg0;
  const int nvalid = rem < LANES ? (int)rem : LANES;
  const long long b = cfg0 + (lane < nvalid ? lane : nvalid - 1);
  const T* u_mine = u + (u_shared ? 0 : b * N);

  if constexpr (ABA_PARK) {
    const int gsel = blockIdx.y;
    sfor<0, N>([&](auto Rt) {
      constexpr int rt = decltype(Rt)::value;
      if constexpr (grp_head(rt)) {
        constexpr int gi = grp_index(rt);
        constexpr int row0 = grp_row0(rt), rows = grp_rows(rt);
        if (gi == gsel) {
          using St = RollParked<T, LANES, row0>;
          T* mine = lds + (lane < LANES ? lane : 0);
          if (lane < LANES) {
            sfor<row0, row0 + rows>([&](auto J) {
              constexpr int j = decltype(J)::value;
              const T qj = q0[b * N + j];
              const JTrig<T> g = make_trig<j>(qj);
              mine[St::own(j, 12)] = g.s;
              mine[St::own(j, 13)] = g.c;
              mine[St::own(j, ABA_SLOTS)] = qj;
              mine[St::own(j, ABA_SLOTS + 1)] = qd0[b * N + j];
            });
          }
#pragma nounroll
          for (long long t = 0; t < steps; ++t) {
            if (lane < LANES) {
              St st{mine, u_mine + t * u_step};
              aba_group<T, row0, rows>(grav, st);
              sfor<row0, row0 + rows>([&](auto J) {
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
            if (slice != 0 || t == steps - 1) {
              __syncthreads();
              // q, qd sit in two slots of every body of the group -> out[t][cfg0 + cfg][row0 + i]
              T* qo = q_out + t * slice + cfg0 * N + row0;
              T* qdo = qd_out + t * slice + cfg0 * N + row0;
              for (int g = lane; g < nvalid * rows; g += 64) {
                const int cfg = g / rows;
                const int i = g - cfg * rows;
                qo[(long long)cfg * N + i] = lds[(i * ROLL_SLOTS + ABA_SLOTS) * LANES + cfg];
                qdo[(long long)cfg * N + i] = lds[(i * ROLL_SLOTS + ABA_SLOTS + 1) * LANES + cfg];
              }
              __syncthreads();   // the rows are out before their owners write the next step's state
            }
          }
        }
      }
    });
  } else {
    RollRegs<T> st;
    sfor<0, N>([&](auto J) {
      constexpr int j = decltype(J)::value;
      st.qv[j] = q0[b * N + j];
      st.qdv[j] = qd0[b * N + j];
      st.tauv[j] = u_mine[j];
    });
#pragma nounroll
    for (long long t = 0; t < steps; ++t) {
      // the next step's u row (the last step reloads its own): in flight while the sweeps run
      const T* u_next = u_mine + (t + 1 < steps ? t + 1 : t) * u_step;
      T un[N];
      sfor<0, N>([&](auto J) { constexpr int j = decltype(J)::value; un[j] = u_next[j]; });
      sfor<0, N>([&](auto J) { constexpr int j = decltype(J)::value; st.tr[j] = make_trig<j>(st.qv[j]); });
      sfor<0, N>([&](auto Rt) {
        constexpr int rt = decltype(Rt)::value;
        if constexpr (grp_head(rt)) aba_group<T, grp_row0(rt), grp_rows(rt)>(grav, st);
      });
      sfor<0, N>([&](auto J) {
        constexpr int j = decltype(J)::value;
        roll_step(dt, integrator, st.qddv[j], st.qv[j], st.qdv[j]);
        st.tauv[j] = un[j];
      });
      if (slice != 0) {
        roll_store<N>(lds, st.qv, q_out + t * slice + cfg0 * N, lane, nvalid, aligned != 0);
        roll_store<N>(lds, st.qdv, qd_out + t * slice + cfg0 * N, lane, nvalid, aligned != 0);
      }
    }
    if (slice == 0) {
      staged_store<N>(lds, st.qv, q_out + cfg0 * N, lane, nvalid);
      staged_store<N>(lds, st.qdv, qd_out + cfg0 * N, lane, nvalid);
    }
  }
}

}  // namespace rbdk
