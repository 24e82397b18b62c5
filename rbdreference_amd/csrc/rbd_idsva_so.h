// rbd_idsva_so.h -- second-order inverse-dynamics derivatives (RBDReference.second_order_idsva_parallel,
// RBDReference.py:1387-1604) for a batch of configurations.  Included by rbd_kernels.hip in the SO units only.
//
// Output per configuration: [4][N][N][N] = d2tau_dq, d2tau_dqd, d2tau_dvdq, dM_dq, every entry written (structural zeros
// included), the rows of a block contiguous in memory.  The composite-force sweep adds the CHILD's force to its parent
// (the reference adds f[:, pi + 1], :1448; identical on robots whose non-root bodies have parent i - 1): the outputs are
// the true derivatives.
//
// One block of SO_THREADS lanes serves SO_G configurations, whose state lives in LDS ([SO_G][N][SO_BS] scalars):
//   phase 1  one lane per configuration: world-frame sweep root -> leaf (ws_down / comp_local of rbd_world.h, revolute and
//            prismatic) writing S, psid, psidd and the body's own composite terms, then the composite sweep leaf -> root;
//   phase 2  one lane per (configuration, body): T1..T4 (:1481-1484) and the 6x6 matrices A1 (D1, :1467) and A2 (D2,
//            :1469); Bic_phii (D3) = A1 + icrf(IC S) and A3 (D4) = icrf(IC S) are applied from T1 = IC S when needed;
//   phase 3  one lane per output ENTRY: the reference scatters each (j, ancestor-or-self k) term into subtree(j)
//            (:1494-1603); every entry is written at most once there, so each entry is evaluated directly from the
//            ancestry of its three indices (a gather) -- one or two bilinear forms u^T M_i w plus a 6-term dot -- and
//            the lanes of a wave write consecutive elements of the block's contiguous output.
// No lane-per-configuration register state survives a phase: the 30-body robot's D1..D4 would not fit in registers.
#pragma once
#include "rbd_world.h"

namespace rbdk {

constexpr int SO_THREADS = 256;
// per-body LDS record: S psid psidd | T1 T2 T3 T4 | A1 (row-major) | A2 (row-major)
constexpr int SO_S = 0, SO_PD = 6, SO_PDD = 12, SO_T1 = 18, SO_T2 = 24, SO_T3 = 30, SO_T4 = 36, SO_A1 = 42, SO_A2 = 78;
constexpr int SO_BS = 114;
// phase 1 scratch inside the A1 / A2 slots of the body (dead before phase 2 writes them): world state, own composite
constexpr int SO_WS = 42, SO_CP = 66;
static_assert(SO_WS + 24 <= SO_CP && SO_CP + TREE_COMP_SCALARS <= SO_BS, "so: phase 1 scratch overlaps");
constexpr int SO_N3 = N * N * N;
constexpr int SO_PER_CFG = 4 * SO_N3;           // output scalars per configuration
template <class T>
constexpr int so_configs_per_block() {          // ~40 KB of LDS per block: several blocks per CU
  const int per = N * SO_BS * (int)sizeof(T);
  const int g = 40960 / per;
  return g < 1 ? 1 : g > 64 ? 64 : g;
}

constexpr unsigned long long so_anc_mask(int b) {   // bit a: a is an ancestor-or-self of b
  unsigned long long m = 0;
  for (int i = b; i != -1; i = PARENT[i]) m |= 1ull << i;
  return m;
}
static_assert(N <= 64, "so: ancestor masks hold 64 bodies");

template <class T>
RBD_DEV void so_ld6(const T* p, T (&v)[6]) {
#pragma unroll
  for (int r = 0; r < 6; ++r) v[r] = p[r];
}
template <class T>
RBD_DEV void so_st6(T* p, const T (&v)[6]) {
#pragma unroll
  for (int r = 0; r < 6; ++r) p[r] = v[r];
}
// u^T M w, M row-major 6x6 in LDS
template <class T>
RBD_DEV T so_form(const T (&u)[6], const T* M, const T (&w)[6]) {
  T acc = T(0);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    T mw = T(0);
#pragma unroll
    for (int c = 0; c < 6; ++c) mw = fma_(M[6 * r + c], w[c], mw);
    acc = fma_(u[r], mw, acc);
  }
  return acc;
}
// u^T icrf(h) w = u . (crf(w) h)
template <class T>
RBD_DEV T so_iform(const T (&u)[6], const T (&h)[6], const T (&w)[6]) {
  T t[6];
  fxv<false>(w, h, t);
  return dot6(u, t);
}
// (crm(a) b) . t
template <class T>
RBD_DEV T so_cdot(const T (&a)[6], const T (&b)[6], const T (&t)[6]) {
  T x[6];
  crm6(a, b, x);
  return dot6(x, t);
}

// ---- phase 2: one body of one configuration ---------------------------------------------------------------------
// IC = [[Ibar, h^x], [-h^x, m 1]];  BC = [[TL, G^x], [-G^x, 0]] + icrf(pm)  (the Sym part and momentum of rbd_world.h)
template <class T>
RBD_DEV void so_skew_add(T (&M)[6][6], int r0, int c0, const T (&x)[3], T s) {
  M[r0 + 0][c0 + 1] -= s * x[2]; M[r0 + 0][c0 + 2] += s * x[1];
  M[r0 + 1][c0 + 0] += s * x[2]; M[r0 + 1][c0 + 2] -= s * x[0];
  M[r0 + 2][c0 + 0] -= s * x[1]; M[r0 + 2][c0 + 1] += s * x[0];
}
// o += crf(a) X - X crm(a)   (dot_matrix, :27-31)
template <class T>
RBD_DEV void so_dotmat_acc(const T (&X)[6][6], const T (&a)[6], T (&o)[6][6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    T col[6], fc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) col[r] = X[r][c];
    fxv<false>(a, col, fc);                       // crf(a) X[:, c]
#pragma unroll
    for (int r = 0; r < 6; ++r) o[r][c] += fc[r];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {                   // -(X crm(a))[r, :] = (crf(a) X[r, :]^T)^T, as crm(a)^T = -crf(a)
    T row[6], y[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) row[c] = X[r][c];
    fxv<false>(a, row, y);
#pragma unroll
    for (int c = 0; c < 6; ++c) o[r][c] += y[c];
  }
}
template <class T>
RBD_DEV void so_body_terms(T* st) {
  T S[6], P[6], Q[6];
  so_ld6(st + SO_S, S); so_ld6(st + SO_PD, P); so_ld6(st + SO_PDD, Q);
  const T* cp = st + SO_CP;                       // m, h[3], Ibar[6], TL[6], G[3], pm[6], f[6]
  T IC[6][6], BC[6][6], f[6];
  {
    const T m = cp[0];
    const T h[3] = {cp[1], cp[2], cp[3]};
    const T G[3] = {cp[16], cp[17], cp[18]};
    const T pn[3] = {cp[19], cp[20], cp[21]}, pg[3] = {cp[22], cp[23], cp[24]};
    constexpr int IX[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) { IC[r][c] = T(0); BC[r][c] = T(0); }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { IC[r][c] = cp[4 + IX[r][c]]; BC[r][c] = cp[10 + IX[r][c]]; }
      IC[3 + r][3 + r] = m;
    }
    so_skew_add(IC, 0, 3, h, T(1)); so_skew_add(IC, 3, 0, h, T(-1));
    so_skew_add(BC, 0, 3, G, T(1)); so_skew_add(BC, 3, 0, G, T(-1));
    so_skew_add(BC, 0, 0, pn, T(-1)); so_skew_add(BC, 0, 3, pg, T(-1)); so_skew_add(BC, 3, 0, pg, T(-1));   // icrf(pm)
#pragma unroll
    for (int r = 0; r < 6; ++r) f[r] = cp[25 + r];
  }
  T ICS[6], ICP[6], ICQ[6], BCS[6], BCP[6], BtS[6], fS[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    T a = T(0), b = T(0), c = T(0), d = T(0), e = T(0), t = T(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      a = fma_(IC[r][k], S[k], a); b = fma_(IC[r][k], P[k], b); c = fma_(IC[r][k], Q[k], c);
      d = fma_(BC[r][k], S[k], d); e = fma_(BC[r][k], P[k], e); t = fma_(BC[k][r], S[k], t);
    }
    ICS[r] = a; ICP[r] = b; ICQ[r] = c; BCS[r] = d; BCP[r] = e; BtS[r] = t;
  }
  fxv<false>(S, f, fS);                           // icrf(f) S = crf(S) f
  T T1[6], T2[6], T3[6], T4[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    T1[r] = ICS[r];
    T2[r] = -BtS[r];
    T3[r] = BCP[r] + ICQ[r] + fS[r];
    T4[r] = fma_(T(2), ICP[r], BCS[r]);           // IC (psid + Sd), Sd = crm(v) S = psid (:1432-1433)
  }
  T A[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) A[r][c] = T(0);
  so_dotmat_acc(IC, S, A);                        // A1 = crf(S) IC - IC crm(S)
  so_st6(st + SO_T1, T1); so_st6(st + SO_T2, T2); so_st6(st + SO_T3, T3); so_st6(st + SO_T4, T4);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) { st[SO_A1 + 6 * r + c] = A[r][c]; A[r][c] = T(0); }
  // A2 = dot_matrix(IC, psid) + icrf(IC psid) + dot_matrix(BC, S)  (:1462-1469)
  so_dotmat_acc(IC, P, A);
  so_dotmat_acc(BC, S, A);
  {
    T Ai[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) Ai[r][c] = T(0);
    const T pn[3] = {ICP[0], ICP[1], ICP[2]}, pg[3] = {ICP[3], ICP[4], ICP[5]};
    so_skew_add(Ai, 0, 0, pn, T(-1)); so_skew_add(Ai, 0, 3, pg, T(-1)); so_skew_add(Ai, 3, 0, pg, T(-1));
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) st[SO_A2 + 6 * r + c] = A[r][c] + Ai[r][c];
  }
}

// ---- phase 3: one output entry [o][x][y][z] of one configuration (st: its [N][SO_BS] record) ------------------------
// anc(a, b): a is an ancestor-or-self of b.  The cases are those of :1494-1603 (DESIGN.md §4.9 lists them).
template <class T>
RBD_DEV T so_entry(const T* st, const unsigned long long* am, int o, int x, int y, int z) {
  auto anc = [&](int a, int b) { return ((am[b] >> a) & 1ull) != 0; };
  auto V = [&](int b, int off, T (&v)[6]) { so_ld6(st + b * SO_BS + off, v); };
  auto A1 = [&](int b) { return st + b * SO_BS + SO_A1; };
  auto A2 = [&](int b) { return st + b * SO_BS + SO_A2; };
  const bool yx = anc(y, x), zx = anc(z, x);                 // y, z ancestors-or-self of x
  const bool xy = anc(x, y) && x != y, xz = anc(x, z) && x != z;   // y, z strictly below x
  T u[6], w[6], h[6], t[6];
  if (o == 0) {                                              // d2tau_dq
    if (yx && zx) {                                          // (:1524, :1534) J the deeper of y, z
      const bool zd = anc(y, z);
      const int J = zd ? z : y, K = zd ? y : z;
      T SJ[6], pK[6], qK[6];
      V(J, SO_PD, u); V(K, SO_PD, w); V(x, SO_T1, h); V(J, SO_S, SJ); V(K, SO_PD, pK); V(K, SO_PDD, qK);
      T r = -(so_form(u, A1(x), w) + so_iform(u, h, w));
      V(x, SO_T2, t);
      r -= so_cdot(pK, SJ, t);
      r += so_cdot(qK, SJ, h);
      return r;
    }
    int I, J;
    bool third = false;
    if (xy && xz) {                                          // (:1546, :1563) x above both: J the shallower
      if (anc(y, z)) { J = y; I = z; } else if (anc(z, y)) { J = z; I = y; } else return T(0);
      third = true;
    } else if (yx && xz) { J = y; I = z; }                   // (:1577-1583) y <= x < z
    else if (zx && xy) { J = z; I = y; }                     //              z <= x < y
    else return T(0);
    T Sx[6], q2[6];
    V(x, SO_S, Sx); V(J, SO_PD, w); V(J, SO_PDD, q2);
    T r = so_form(Sx, A2(I), w) + so_form(q2, A1(I), Sx);
    if (third) {
      T SJ[6];
      V(J, SO_S, SJ); V(I, SO_T3, t);
      r -= so_cdot(SJ, Sx, t);
    }
    return r;
  }
  if (o == 1) {                                              // d2tau_dqd
    if (yx && zx) {
      if (y == z) {                                          // (:1601)
        V(y, SO_S, u);
        return -so_form(u, A1(x), u);
      }
      const bool zd = anc(y, z);                             // (:1538-1539)
      const int J = zd ? z : y, K = zd ? y : z;
      V(J, SO_S, u); V(K, SO_S, w); V(x, SO_T1, h);
      return -(so_form(u, A1(x), w) + so_iform(u, h, w));
    }
    int I, K;
    if (xy && xz) {                                          // (:1556, :1566-1567) J the shallower
      if (anc(y, z)) { K = y; I = z; } else if (anc(z, y)) { K = z; I = y; } else return T(0);
    } else if (yx && xz) { K = y; I = z; }                   // (:1586-1587)
    else if (zx && xy) { K = z; I = y; }
    else return T(0);
    V(x, SO_S, u); V(K, SO_S, w); V(I, SO_T1, h);
    return so_form(u, A1(I), w) + so_iform(u, h, w);
  }
  if (o == 2) {                                              // d2tau_dvdq
    T Sx[6];
    if (yx && zx) {
      V(y, SO_S, u); V(z, SO_PD, w); V(x, SO_T1, h);
      T r = -(so_form(u, A1(x), w) + so_iform(u, h, w));    // (:1525)
      if (!anc(z, y)) {                                      // y above z (:1542)
        T Sz[6], py2[6], pz[6];
        V(z, SO_S, Sz); V(y, SO_PD, py2); V(z, SO_PD, pz);
        V(x, SO_T2, t);
        r -= so_cdot(u, Sz, t);
#pragma unroll
        for (int k = 0; k < 6; ++k) py2[k] = T(2) * py2[k];
        r += so_cdot(py2, Sz, h) - T(2) * so_cdot(pz, u, h);
      }
      return r;
    }
    V(x, SO_S, Sx);
    if (xy && anc(z, y) && (zx || xz)) {                     // z <= x < y (:1590) or x < z <= y (:1550)
      V(z, SO_PD, w); V(y, SO_T1, h);
      T r = so_form(Sx, A1(y), w) + so_iform(Sx, h, w);
      if (xz) {
        T Sz[6];
        V(z, SO_S, Sz); V(y, SO_T4, t);
        r -= so_cdot(Sz, Sx, t);
      }
      return r;
    }
    if (xz && anc(y, z) && y != z && (yx || xy)) {           // y <= x < z (:1593) or x < y < z (:1570)
      T Sy[6], p2[6];
      V(y, SO_S, Sy); V(y, SO_PD, p2);
#pragma unroll
      for (int k = 0; k < 6; ++k) p2[k] = T(2) * p2[k];
      return so_form(Sx, A2(z), Sy) + so_form(p2, A1(z), Sx);
    }
    return T(0);
  }
  // dM_dq
  const bool xbz = anc(x, z) && x != z, ybz = anc(y, z) && y != z;
  if (xbz && ybz) {                                          // (:1596-1597) both above z: J the deeper
    const bool yd = anc(x, y);
    const int J = yd ? y : x, K = yd ? x : y;
    V(J, SO_S, u); V(K, SO_S, w);
    return so_form(u, A1(z), w);
  }
  int K, I;
  if (xbz && anc(z, y)) { K = x; I = y; }                    // (:1559-1560)
  else if (ybz && anc(z, x)) { K = y; I = x; }
  else return T(0);
  V(K, SO_S, u); V(z, SO_S, w); V(I, SO_T1, h);
  return so_iform(u, h, w);
}

template <class T>
__global__ __launch_bounds__(SO_THREADS) void so_idsva_kernel(const T* __restrict__ q, const T* __restrict__ qd,
                                                              const T* __restrict__ qdd, T grav, long long B,
                                                              T* __restrict__ out) {
  constexpr int G = so_configs_per_block<T>();
  __shared__ T sm[G * N * SO_BS];
  __shared__ unsigned long long am[N];
  const int tid = threadIdx.x;
  const long long g0 = (long long)blockIdx.x * G;
  const int nvalid = (int)((B - g0) < G ? (B - g0) : G);
  if (tid == SO_THREADS - 1)                                 // (literals: no table in memory)
    sfor<0, N>([&](auto B_) { constexpr int b = decltype(B_)::value; am[b] = so_anc_mask(b); });
  if (tid < G) {                                             // phase 1: one lane per configuration
    const long long g = g0 + (tid < nvalid ? tid : nvalid - 1);   // (a tail block repeats its last row; not written)
    T* st = sm + tid * N * SO_BS;
    const T* qg = q + g * N;
    const T* qdg = qd + g * N;
    const T* qddg = qdd + g * N;
    sfor<0, N>([&](auto J_) {
      constexpr int J = decltype(J_)::value;
      WState<T> s;
      if constexpr (PARENT[J] >= 0) {
        const T* ps = st + PARENT[J] * SO_BS + SO_WS;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) s.R[r][c] = ps[3 * r + c];
          s.p[r] = ps[9 + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) { s.v[r] = ps[12 + r]; s.a[r] = ps[18 + r]; }
      }
      const JTrig<T> tr = make_trig<J>(qg[J]);
      T Sv[6], Pd[6], Pdd[6];
      ws_down<J>(s, tr, qdg[J], qddg[J], grav, Sv, Pd, Pdd);
      T* bs = st + J * SO_BS;
      so_st6(bs + SO_S, Sv); so_st6(bs + SO_PD, Pd); so_st6(bs + SO_PDD, Pdd);
      T* ws = bs + SO_WS;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ws[3 * r + c] = s.R[r][c];
        ws[9 + r] = s.p[r];
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) { ws[12 + r] = s.v[r]; ws[18 + r] = s.a[r]; }
      Comp<T> L;
      comp_local<J>(s, L);
      T* cp = bs + SO_CP;
      comp_each(L, [&](int k, T& x) { cp[k] = x; });
    });
    sfor_down<0, N>([&](auto J_) {                           // composites leaf -> root, the child's f included (:1448)
      constexpr int J = decltype(J_)::value;
      if constexpr (PARENT[J] >= 0) {
        const T* c = st + J * SO_BS + SO_CP;
        T* p = st + PARENT[J] * SO_BS + SO_CP;
#pragma unroll
        for (int k = 0; k < TREE_COMP_SCALARS; ++k) p[k] += c[k];
      }
    });
  }
  __syncthreads();
  for (int it = tid; it < G * N; it += SO_THREADS) so_body_terms(sm + it * SO_BS);   // phase 2 ([G][N] records)
  __syncthreads();
  const int total = nvalid * SO_PER_CFG;                     // phase 3: the block's rows are one contiguous run
  T* dst = out + g0 * SO_PER_CFG;
  for (int e = tid; e < total; e += SO_THREADS) {
    const int c = e / SO_PER_CFG;
    int r = e - c * SO_PER_CFG;
    const int o = r / SO_N3;
    r -= o * SO_N3;
    const int x = r / (N * N);
    r -= x * (N * N);
    const int y = r / N;
    const int z = r - y * N;
    dst[e] = so_entry(sm + c * N * SO_BS, am, o, x, y, z);
  }
}

}  // namespace rbdk
