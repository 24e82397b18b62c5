// rbd_ee.h -- end-effector pose and pose gradient (RBDReference.end_effector_pose / end_effector_pose_gradient,
// RBDReference.py:220-274, :286-386) for a batch of configurations.  Included by rbd_kernels.hip in the EE units only.
//
// One lane per configuration.  For each site of the call's site table (wave-uniform: the same for every lane) the
// kernel branches on the site's body into a compile-time path that chains the body frames root -> body once
// (W = prod T_tree_j T_J(q_j); T_tree constants and their structural zeros resolved by the compiler) and records
// each chain joint's world axis w_j and origin p_j.  The site frame is W M (M = the constant 3x4 body -> site
// transform of the site table), its point P = R_s o + w t_s (o = ee_offsets[0] = (o, w)).  The gradient is closed
// form -- no per-column chain product as in the reference (:300-318):
//   revolute j:  dP = w_j x (P - w p_j),  dR_s = [w_j]x R_s;      prismatic j:  dP = w w_j,  dR_s = 0;
// and roll / pitch / yaw follow the reference's darctan2 / sqrt-term rule (:322-340) on the five entries of R_s
// and dR_s it reads.  Columns of joints off the site's chain are zero (:357-359, :378-380).
// q stays in LDS as a [64][N] tile; sin / cos of a chain joint are evaluated on the chain (rbd_sincos.h), which keeps
// the live set to one chain -- what an all-bodies selection of a 30-body robot needs to stay out of scratch.
// Outputs leave through LDS: pose [B, n_sites, 6] as one contiguous tile per block, dpose [B, n_sites, 6, N] one
// [64][6N] tile per site whose rows are streamed out as contiguous 6N-element runs.
#pragma once

namespace rbdk {

constexpr int EE_MAX_SITES = 16;

// per-call site table, passed by value in the kernel arguments (kernarg segment: uniform scalar loads)
template <class T>
struct EeSites {
  int body[EE_MAX_SITES];
  T M[EE_MAX_SITES][9];       // body -> site rotation, row-major (R_s = R_body M)
  T pl[EE_MAX_SITES][3];      // M_R o + w M_t: the offset point in body coordinates, per site
  T w;                        // ee_offsets[0][3]
  int n_sites;
};

struct EeChain {
  int id[64];
  int len;
};
constexpr EeChain ee_chain(int b) {
  EeChain c{};
  int tmp[64] = {};
  int k = 0;
  for (int i = b; i != -1; i = PARENT[i]) tmp[k++] = i;
  c.len = k;
  for (int d = 0; d < k; ++d) c.id[d] = tmp[k - 1 - d];   // root first
  return c;
}
// T_tree_j = [[E^T, r], [0, 1]] of X_tree = plux(E, r): E^T[m][c] = XT[c][m], r from the lower-left block -E r^x
constexpr double ee_ET(int j, int m, int c) { return XT[j][c * 6 + m]; }
constexpr double ee_rx(int j, int a, int b) {             // (r^x)[a][b] = -(E^T L)[a][b], L = XT[3:, :3]
  double s = 0.0;
  for (int m = 0; m < 3; ++m) s -= XT[j][m * 6 + a] * XT[j][(3 + m) * 6 + b];
  return s;
}
constexpr double ee_r(int j, int k) { return k == 0 ? ee_rx(j, 2, 1) : k == 1 ? ee_rx(j, 0, 2) : ee_rx(j, 1, 0); }

// x * c + acc for a compile-time constant c (0 and +-1 cost nothing)
template <class T, class CV>
RBD_DEV T ee_madd(T x, CV, T acc) {
  constexpr double c = CV::value;
  if constexpr (c == 0.0) return acc;
  else if constexpr (c == 1.0) return acc + x;
  else if constexpr (c == -1.0) return acc - x;
  else return fma(x, T(c), acc);
}
template <int J, int M, int C>
struct ee_ETc { static constexpr double value = ee_ET(J, M, C); };
template <int J, int M>
struct ee_rc { static constexpr double value = ee_r(J, M); };
template <int B>
struct ee_chain_of { static constexpr EeChain value = ee_chain(B); };

template <class T>
RBD_DEV T ee_atan2(T y, T x) { return atan2(y, x); }
template <>
RBD_DEV float ee_atan2<float>(float y, float x) { return atan2f(y, x); }
template <class T>
RBD_DEV T ee_sqrt(T x) { return sqrt(x); }
template <>
RBD_DEV float ee_sqrt<float>(float x) { return sqrtf(x); }

template <int I, class F>
RBD_DEV void ee_body_switch(int b, F&& f) {
  if constexpr (I < N) {
    if (b == I) f(std::integral_constant<int, I>{});
    else ee_body_switch<I + 1>(b, static_cast<F&&>(f));
  }
}

// stream a [64][KP]-strided LDS tile out as nvalid rows of K elements, row r to dst + r * stride
template <int K, class T>
RBD_DEV void ee_flush_rows(const T* lds, T* dst, long long stride, int lane, int nvalid) {
  constexpr int KP = odd_pad<K>();
  const int total = nvalid * K;
#pragma unroll 4
  for (int g = lane; g < total; g += 64) {
    const int cfg = g / K;
    const int r = g - cfg * K;
    dst[(long long)cfg * stride + r] = lds[cfg * KP + r];
  }
}

template <class T>
constexpr size_t ee_lds_bytes(int n_sites, bool pose, bool grad) {
  return sizeof(T) * (64 * (size_t)N + (pose ? 64 * 6 * (size_t)n_sites : 0) + (grad ? 64 * (size_t)odd_pad<6 * N>() : 0));
}

template <class T, bool POSE, bool GRAD>
__global__ __launch_bounds__(64) void ee_pose_kernel(const T* __restrict__ q, long long B, const EeSites<T> st,
                                                     T* __restrict__ pose, T* __restrict__ dpose) {
  extern __shared__ __align__(16) unsigned char ee_smem[];
  T* lds = reinterpret_cast<T*>(ee_smem);
  constexpr int K = 6 * N;
  constexpr int KP = odd_pad<K>();
  const int lane = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * 64;
  const int nvalid = (int)((B - b0) < 64 ? (B - b0) : 64);
  const int ns = st.n_sites;

  // q tile: coalesced load; it stays in LDS, each site's chain reads its joints' rows from it
  T* qt = lds;
  for (int g = lane; g < nvalid * N; g += 64) qt[g] = q[b0 * N + g];
  __syncthreads();
  const T* qrow = qt + (lane < nvalid ? lane : 0) * N;
  T* ptile = lds + 64 * N;
  T* gtile = ptile + (POSE ? 64 * 6 * ns : 0);
  const T w = st.w;

  for (int s = 0; s < ns; ++s) {
    // this site's row of the table (uniform), read here so that the body paths below capture registers only
    const int sb = st.body[s];
    T M[9], pl[3];
    sfor<0, 9>([&](auto I) { M[decltype(I)::value] = st.M[s][decltype(I)::value]; });
    sfor<0, 3>([&](auto I) { pl[decltype(I)::value] = st.pl[s][decltype(I)::value]; });
    ee_body_switch<0>(sb, [&](auto BODY) {
      constexpr int bd = decltype(BODY)::value;
      using CH_ = ee_chain_of<bd>;
      constexpr int D = CH_::value.len;
      T R[3][3], t[3];
      T ax[D][3], org[D][3];
      sfor<0, D>([&](auto DI) {
        constexpr int d = decltype(DI)::value;
        constexpr int j = CH_::value.id[d];
        if constexpr (d == 0) {                     // W = T_tree_j (constants)
          sfor<0, 3>([&](auto RI) {
            constexpr int r = decltype(RI)::value;
            sfor<0, 3>([&](auto CI) { R[r][decltype(CI)::value] = T(ee_ET(j, r, decltype(CI)::value)); });
            t[r] = T(ee_r(j, r));
          });
        } else {                                    // W = W T_tree_j
          T Rn[3][3], tn[3];
          sfor<0, 3>([&](auto RI) {
            constexpr int r = decltype(RI)::value;
            T acc = t[r];
            sfor<0, 3>([&](auto MI) { acc = ee_madd(R[r][decltype(MI)::value], ee_rc<j, decltype(MI)::value>{}, acc); });
            tn[r] = acc;
            sfor<0, 3>([&](auto CI) {
              constexpr int c = decltype(CI)::value;
              T a = T(0);
              sfor<0, 3>([&](auto MI) { a = ee_madd(R[r][decltype(MI)::value], ee_ETc<j, decltype(MI)::value, c>{}, a); });
              Rn[r][c] = a;
            });
          });
          sfor<0, 3>([&](auto RI) {
            constexpr int r = decltype(RI)::value;
            t[r] = tn[r];
            sfor<0, 3>([&](auto CI) { R[r][decltype(CI)::value] = Rn[r][decltype(CI)::value]; });
          });
        }
        constexpr int k = AXIS[j];
        const T qj = qrow[j];
        if constexpr (JTYPE[j] == 0) {              // W = W Rot_k(q): columns a, b turn
          constexpr int a = (k + 1) % 3, b = (k + 2) % 3;
          T sj, cj;
          sincos_(qj, &sj, &cj);
          sfor<0, 3>([&](auto RI) {
            constexpr int r = decltype(RI)::value;
            const T Ra = R[r][a], Rb = R[r][b];
            R[r][a] = fma(cj, Ra, sj * Rb);
            R[r][b] = fma(cj, Rb, -sj * Ra);
          });
        } else {                                    // t += q R e_k
          sfor<0, 3>([&](auto RI) { t[decltype(RI)::value] = fma(qj, R[decltype(RI)::value][k], t[decltype(RI)::value]); });
        }
        sfor<0, 3>([&](auto RI) {
          ax[d][decltype(RI)::value] = R[decltype(RI)::value][k];
          org[d][decltype(RI)::value] = t[decltype(RI)::value];
        });
      });
      // site frame: R_s = R M, P = R pl + w t
      T Rs[3][3], P[3];
      sfor<0, 3>([&](auto RI) {
        constexpr int r = decltype(RI)::value;
        P[r] = fma(R[r][0], pl[0], fma(R[r][1], pl[1], fma(R[r][2], pl[2], w * t[r])));
        sfor<0, 3>([&](auto CI) {
          constexpr int c = decltype(CI)::value;
          Rs[r][c] = fma(R[r][0], M[c], fma(R[r][1], M[3 + c], R[r][2] * M[6 + c]));
        });
      });
      const T rr = Rs[2][2] * Rs[2][2] + Rs[2][1] * Rs[2][1];
      const T sp = ee_sqrt(rr);
      if constexpr (POSE) {
        T* o = ptile + lane * 6 * ns + 6 * s;
        o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
        o[3] = ee_atan2(Rs[2][1], Rs[2][2]);        // (:248-257)
        o[4] = ee_atan2(-Rs[2][0], sp);
        o[5] = ee_atan2(Rs[1][0], Rs[0][0]);
      }
      if constexpr (GRAD) {
        const T i_rr = T(1) / rr;
        const T i_sp = T(1) / sp;
        const T i_pp = T(1) / (sp * sp + Rs[2][0] * Rs[2][0]);
        const T i_yy = T(1) / (Rs[0][0] * Rs[0][0] + Rs[1][0] * Rs[1][0]);
        __syncthreads();                            // the previous site's tile has left
        T* g = gtile + lane * KP;
        sfor<0, N>([&](auto CI) {
          constexpr int c = decltype(CI)::value;
          constexpr int d = DEPTH[c];
          if constexpr (d < D && CH_::value.id[d < D ? d : 0] == c) {
            const T* wj = ax[d];
            if constexpr (JTYPE[c] == 0) {
              const T u0 = P[0] - w * org[d][0], u1 = P[1] - w * org[d][1], u2 = P[2] - w * org[d][2];
              g[0 * N + c] = wj[1] * u2 - wj[2] * u1;
              g[1 * N + c] = wj[2] * u0 - wj[0] * u2;
              g[2 * N + c] = wj[0] * u1 - wj[1] * u0;
              const T d00 = wj[1] * Rs[2][0] - wj[2] * Rs[1][0];
              const T d10 = wj[2] * Rs[0][0] - wj[0] * Rs[2][0];
              const T d20 = wj[0] * Rs[1][0] - wj[1] * Rs[0][0];
              const T d21 = wj[0] * Rs[1][1] - wj[1] * Rs[0][1];
              const T d22 = wj[0] * Rs[1][2] - wj[1] * Rs[0][2];
              // darctan2(y, x, y', x') = (-x' y + x y') / (x x + y y)   (:326-327)
              g[3 * N + c] = (-d22 * Rs[2][1] + Rs[2][2] * d21) * i_rr;
              const T dsp = (Rs[2][2] * d22 + Rs[2][1] * d21) * i_sp;
              g[4 * N + c] = (-dsp * -Rs[2][0] + sp * -d20) * i_pp;
              g[5 * N + c] = (-d00 * Rs[1][0] + Rs[0][0] * d10) * i_yy;
            } else {
              g[0 * N + c] = w * wj[0];
              g[1 * N + c] = w * wj[1];
              g[2 * N + c] = w * wj[2];
              g[3 * N + c] = T(0) * i_rr;
              g[4 * N + c] = T(0) * i_pp;
              g[5 * N + c] = T(0) * i_yy;
            }
          } else {
            sfor<0, 6>([&](auto RI) { g[decltype(RI)::value * N + c] = T(0); });
          }
        });
        __syncthreads();
        ee_flush_rows<K>(gtile, dpose + (b0 * ns + s) * K, (long long)ns * K, lane, nvalid);
      }
    });
  }
  if constexpr (POSE) {
    __syncthreads();
    const int total = nvalid * 6 * ns;
    T* dst = pose + b0 * 6 * ns;
#pragma unroll 4
    for (int g = lane; g < total; g += 64) dst[g] = ptile[g];
  }
}

}  // namespace rbdk
