// Invariant-Transformer edge message + aggregation: the ET message (et_message.hip) with the vector
// channels removed -- the scalar form of tmdnet_et_message_fwd / _bwd / _bwd2 (TMDNET_ET_SCALAR).
//
// Reference: MultiHeadAttention.forward/message (models/torchmd_t.py:246-283).  For every edge
// e = (t <- s), head h, channel c of the head (d = H / heads):
//     sc[e,h]    = sum_c q[t,h,c] k[s,h,c] A(pk[e,h,c])
//     a[e,h]     = B(sc[e,h]) * C[e]
//     out[t,h,c] = sum_{e in row t} v[s,h,c] A(pv[e,h,c]) a[e,h]
// The layout mirrors et_message.hip:
//   * one wave64 owns one destination row t; its node rows sit in registers and the wave streams t's
//     CSR row: a lane owns V contiguous channels (H = 32 V: two edges per wave instruction; H < 32:
//     64 / H edges), the pre-activation dk / dv rows are read coalesced (2H values per edge) and the
//     k / v rows of the sources gathered (2H): 4H values per edge against the vector form's 8H;
//   * heads are aligned lane groups: the q.k.dk product is a group_sum over d / V lanes;
//   * the per-edge scalars (source, cutoff, reversed edge) are fetched 64 edges at a time by one
//     coalesced load and handed to the edge slots by cross-lane permutes;
//   * every output is written once, by the wave that owns its row: no atomics, deterministic;
//   * the first backward serves both roles of a node in ONE walk of its row: as destination of edge
//     e (gq, gpk, gpv, gcut) and as source of the reversed edge (gk, gv), which on the symmetric lists
//     the model builds has the same pk, pv and C (tmdnet_et_message_bwd's precondition);
//   * the second order walks the row twice, once per role, so that one role's ~20 row segments are
//     live at a time; its per-edge cotangents are not pair-symmetric, so the source role reads those
//     of the reversed edge through the transpose map.
#include "common.h"
#include "tmdnet.h"

namespace tmd {
namespace tmsg {

template <typename T> struct V4;
template <> struct V4<float> { using t2 = float2; using t4 = float4; };
template <> struct V4<double> { using t2 = double2; using t4 = double4; };

// V contiguous channels of a row: 16-byte loads where V allows (V = 8: two of them)
template <typename T, int V> __device__ __forceinline__ void ldv(T (&o)[V], const T* p) {
  if constexpr (V == 1) {
    o[0] = *p;
  } else if constexpr (V == 2) {
    const typename V4<T>::t2 x = *reinterpret_cast<const typename V4<T>::t2*>(p);
    o[0] = x.x; o[1] = x.y;
  } else {
#pragma unroll
    for (int j = 0; j < V; j += 4) {
      const typename V4<T>::t4 x = *reinterpret_cast<const typename V4<T>::t4*>(p + j);
      o[j] = x.x; o[j + 1] = x.y; o[j + 2] = x.z; o[j + 3] = x.w;
    }
  }
}
template <typename T, int V> __device__ __forceinline__ void stv(T* p, const T (&o)[V]) {
  if constexpr (V == 1) {
    *p = o[0];
  } else if constexpr (V == 2) {
    typename V4<T>::t2 x;
    x.x = o[0]; x.y = o[1];
    *reinterpret_cast<typename V4<T>::t2*>(p) = x;
  } else {
#pragma unroll
    for (int j = 0; j < V; j += 4) {
      typename V4<T>::t4 x;
      x.x = o[j]; x.y = o[j + 1]; x.z = o[j + 2]; x.w = o[j + 3];
      *reinterpret_cast<typename V4<T>::t4*>(p + j) = x;
    }
  }
}
template <typename T, int V> __device__ __forceinline__ void zero(T (&o)[V]) {
#pragma unroll
  for (int i = 0; i < V; ++i) o[i] = T(0);
}
// an optional row: absent (NULL) reads as zeros
template <typename T, int V> __device__ __forceinline__ void ldv_opt(T (&o)[V], const T* p, size_t off) {
  if (p) ldv<T, V>(o, p + off); else zero(o);
}
// sum over the edge slots of a wave (lanes L apart hold the same channels)
template <typename T, int V> __device__ __forceinline__ void xor_slots(T (&a)[V], int L) {
  for (int o = L; o < TMD_WAVE; o <<= 1)
#pragma unroll
    for (int i = 0; i < V; ++i) a[i] += __shfl_xor(a[i], o);
}

template <typename T> struct Args {
  int n, H, L, lph, cap;
  const int32_t* row_ptr;
  const int32_t* src;
  const int32_t* order;
  const int32_t* tr;
  const T* q; int ldq;
  const T* k; int ldk;
  const T* v; int ldv;
  const T* pk; int ldpk;
  const T* pv; int ldpv;
  const T* C;
  int act_kv, act_at;
  T* xo;          // forward output
  const T* gx;    // upstream gradient of x_out [N][H]
  T* gq; T* gk; T* gv; T* gpk; T* gpv; T* gC;  // first backward outputs
  // second order: cotangents of (gq, gk, gv, gpk, gpv, gC), NULL = zero ...
  const T* ggq; int ldggq;
  const T* ggk; int ldggk;
  const T* ggv; int ldggv;
  const T* ggpk; int ldggpk;
  const T* ggpv; int ldggpv;
  const T* ggC;
  // ... and its outputs (NULL = not wanted)
  T* o_gx;
  T* o_q; int ldoq;
  T* o_k; int ldok;
  T* o_v; int ldov;
  T* o_pk; int ldopk;
  T* o_pv; int ldopv;
  T* o_C;
};

// activation of a pre-activation row segment with DER derivatives (absent projection: 1, 0, 0)
template <typename T, int V, int DER>
__device__ __forceinline__ void act(const T (&x)[V], bool has, int code, T (&s)[V], T (&d1)[DER >= 1 ? V : 1],
                                    T (&d2)[DER >= 2 ? V : 1]) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    if (has) {
      const ActF<T> f(x[i], code);
      s[i] = f.s;
      if constexpr (DER >= 1) d1[i] = f.d(x[i]);
      if constexpr (DER >= 2) d2[i] = f.dd(x[i]);
    } else {
      s[i] = T(1);
      if constexpr (DER >= 1) d1[i] = T(0);
      if constexpr (DER >= 2) d2[i] = T(0);
    }
  }
}

// The node of this wave (wave-uniform) and its lane's place: edge slot `es` (lanes [es L, (es + 1) L)
// stream one edge) and first channel c0.  XCD-contiguous block remap as the ET kernels.
struct Geo { int node, es, c0; };
template <typename T> __device__ __forceinline__ Geo geo(const Args<T>& A) {
  Geo g;
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int w = __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
  g.node = w < A.n ? (A.order ? __builtin_amdgcn_readfirstlane(A.order[w]) : w) : -1;
  const int lane = lane_id();
  g.es = lane / A.L;
  g.c0 = (lane % A.L) * (A.H / A.L);
  return g;
}

// Row traversal: chunks of 64 edges; pre(k) loads the per-edge scalars of edge k into this lane (one
// coalesced load per scalar), body(k, jj) runs once per edge on the lanes of its slot, jj being the lane
// that holds the edge's scalars.  The chunk and slot loops are wave-uniform.
template <typename T, typename P, typename F>
__device__ __forceinline__ void edge_chunks(const Args<T>& A, int b, int e, const Geo& G, P&& pre, F&& body) {
  const int lane = lane_id();
  const int EPW = TMD_WAVE / A.L;
  for (int c = b; c < e; c += TMD_WAVE) {
    const int n = min(TMD_WAVE, e - c);
    pre(c + min(lane, n - 1));
    for (int j0 = 0; j0 < n; j0 += EPW) {
      const int j = j0 + G.es;
      body(c + min(j, n - 1), min(j, n - 1), j < n);
    }
  }
}

// ------------------------------------------------------------------ forward
// GA: the activation codes are read at run time (else SiLU / SiLU as compile-time constants)
template <typename T, int V, bool GA>
__global__ __launch_bounds__(256) void k_t_fwd(Args<T> A) {
  const int AKV = GA ? A.act_kv : kActSilu, AAT = GA ? A.act_at : kActSilu;
  const Geo G = geo(A);
  const int t = G.node, c0 = G.c0;
  if (t < 0) return;
  const bool hk = A.pk != nullptr, hv = A.pv != nullptr;
  T q[V], ax[V];
  ldv<T, V>(q, A.q + (size_t)t * A.ldq + c0);
  zero(ax);
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  int s_r = 0;
  T C_r = T(0);
  edge_chunks(A, b, e, G,
      [&](int k) {
        s_r = A.src[k];
        TMD_DCHECK(s_r >= 0 && s_r < A.n);
        C_r = A.C[k];
      },
      [&](int k, int jj, bool live) {
        const int s = __shfl(s_r, jj);
        const T Ce = __shfl(C_r, jj);
        if (!live) return;
        T kk[V], vv[V], pk[V], pv[V];
        ldv<T, V>(kk, A.k + (size_t)s * A.ldk + c0);
        ldv<T, V>(vv, A.v + (size_t)s * A.ldv + c0);
        ldv_opt<T, V>(pk, A.pk, (size_t)k * A.ldpk + c0);
        ldv_opt<T, V>(pv, A.pv, (size_t)k * A.ldpv + c0);
        T ak[V], av[V], u1[1], u2[1];
        act<T, V, 0>(pk, hk, AKV, ak, u1, u2);
        act<T, V, 0>(pv, hv, AKV, av, u1, u2);
        T part = T(0);
#pragma unroll
        for (int i = 0; i < V; ++i) part += q[i] * kk[i] * ak[i];
        part = group_sum(part, A.lph);
        const ActF<T> sa(part, AAT);
        const T a = sa.s * Ce;
#pragma unroll
        for (int i = 0; i < V; ++i) ax[i] += vv[i] * av[i] * a;
      });
  xor_slots(ax, A.L);
  if (G.es == 0) stv<T, V>(A.xo + (size_t)t * A.H + c0, ax);
}

// Static-capacity lists: rows [row_ptr[n], cap) of the per-edge outputs belong to no CSR row and are
// written as zeros, spread over the grid.
template <typename T>
__device__ __forceinline__ void zero_pad_rows(const Args<T>& A, T* pk, int ldpk, T* pv, int ldpv, T* C) {
  const int e0 = min(A.row_ptr[A.n], A.cap);
  if (e0 >= A.cap) return;
  const long long rows = A.cap - e0;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  if (pk)
    for (long long i = tid; i < rows * A.H; i += nth) pk[(size_t)(e0 + i / A.H) * ldpk + i % A.H] = T(0);
  if (pv)
    for (long long i = tid; i < rows * A.H; i += nth) pv[(size_t)(e0 + i / A.H) * ldpv + i % A.H] = T(0);
  if (C)
    for (long long i = tid; i < rows; i += nth) C[e0 + i] = T(0);
}

// ------------------------------------------------------------------ first backward
// Node t in both roles, one walk of its row.  Edge e = (t <- s):
//   destination role (q_t, gx_t | k_s, v_s):  sc, ga = sum_c gx v A(pv), gsc = ga C B'(sc), a = B(sc) C
//     gq[t] += gsc k_s A(pk),  gpk[e] = gsc q_t k_s A'(pk),  gpv[e] = gx_t v_s a A'(pv),  gC[e] = sum_h ga B(sc)
//   source role, the reversed edge (s <- t) with the same pk, pv, C (q_s, gx_s | k_t, v_t):
//     gk[t] += gsc' q_s A(pk),  gv[t] += gx_s A(pv) a'
template <typename T, int V, bool GA>
__global__ __launch_bounds__(256) void k_t_bwd(Args<T> A) {
  const int AKV = GA ? A.act_kv : kActSilu, AAT = GA ? A.act_at : kActSilu;
  zero_pad_rows(A, A.gpk, A.ldpk, A.gpv, A.ldpv, A.gC);
  const Geo G = geo(A);
  const int t = G.node, c0 = G.c0;
  if (t < 0) return;
  const bool hk = A.pk != nullptr, hv = A.pv != nullptr;
  const bool lead = c0 == 0;
  T q[V], gx[V], kt[V], vt[V], gq[V], gk[V], gv[V];
  ldv<T, V>(q, A.q + (size_t)t * A.ldq + c0);
  ldv<T, V>(gx, A.gx + (size_t)t * A.H + c0);
  ldv<T, V>(kt, A.k + (size_t)t * A.ldk + c0);
  ldv<T, V>(vt, A.v + (size_t)t * A.ldv + c0);
  zero(gq); zero(gk); zero(gv);
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  int s_r = 0;
  T C_r = T(0);
  edge_chunks(A, b, e, G,
      [&](int k) {
        s_r = A.src[k];
        TMD_DCHECK(s_r >= 0 && s_r < A.n);
        C_r = A.C[k];
      },
      [&](int k, int jj, bool live) {
        const int s = __shfl(s_r, jj);
        const T Ce = __shfl(C_r, jj);
        if (!live) return;
        T ks[V], vs[V], qs[V], gxs[V], pk[V], pv[V];
        ldv<T, V>(ks, A.k + (size_t)s * A.ldk + c0);
        ldv<T, V>(vs, A.v + (size_t)s * A.ldv + c0);
        ldv<T, V>(qs, A.q + (size_t)s * A.ldq + c0);
        ldv<T, V>(gxs, A.gx + (size_t)s * A.H + c0);
        ldv_opt<T, V>(pk, A.pk, (size_t)k * A.ldpk + c0);
        ldv_opt<T, V>(pv, A.pv, (size_t)k * A.ldpv + c0);
        T ak[V], ak1[V], av[V], av1[V], u2[1];
        act<T, V, 1>(pk, hk, AKV, ak, ak1, u2);
        act<T, V, 1>(pv, hv, AKV, av, av1, u2);
        T sc = T(0), pa = T(0), sc2 = T(0), ga2 = T(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          sc += q[i] * ks[i] * ak[i];
          pa += gx[i] * vs[i] * av[i];
          sc2 += qs[i] * kt[i] * ak[i];
          ga2 += gxs[i] * vt[i] * av[i];
        }
        sc = group_sum(sc, A.lph);
        const T ga = group_sum(pa, A.lph);
        sc2 = group_sum(sc2, A.lph);
        ga2 = group_sum(ga2, A.lph);
        const ActF<T> f(sc, AAT), f2(sc2, AAT);
        const T gsc = ga * Ce * f.d(sc), a = f.s * Ce;
        const T gsc2 = ga2 * Ce * f2.d(sc2), a2 = f2.s * Ce;
        T opk[V], opv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
          gq[i] += gsc * ks[i] * ak[i];
          opk[i] = gsc * q[i] * ks[i] * ak1[i];
          opv[i] = gx[i] * vs[i] * a * av1[i];
          gk[i] += gsc2 * qs[i] * ak[i];
          gv[i] += gxs[i] * av[i] * a2;
        }
        if (A.gpk) stv<T, V>(A.gpk + (size_t)k * A.ldpk + c0, opk);
        if (A.gpv) stv<T, V>(A.gpv + (size_t)k * A.ldpv + c0, opv);
        const T gc = group_sum(pa * f.s, A.L);  // B(sc) is uniform over a head's lanes
        if (A.gC && lead) A.gC[k] = gc;
      });
  xor_slots(gq, A.L); xor_slots(gk, A.L); xor_slots(gv, A.L);
  if (G.es == 0) {
    if (A.gq) stv<T, V>(A.gq + (size_t)t * A.ldq + c0, gq);
    if (A.gk) stv<T, V>(A.gk + (size_t)t * A.ldk + c0, gk);
    if (A.gv) stv<T, V>(A.gv + (size_t)t * A.ldv + c0, gv);
  }
}

// ------------------------------------------------------------------ second order
// VJP of the first backward for the cotangents (G_q, G_k, G_v, G_pk, G_pv, G_C) of (gq, gk, gv, gpk,
// gpv, gC).  Per edge e = (t <- s) and head, with A = A(pk), A' and A'' its derivatives (Av.. for pv):
//   P = sum_c A (G_q[t] k_s + G_k[s] q_t) + G_pk[e] q_t k_s A'      (the coefficient of gsc)
//   R = sum_c gx_t Av G_v[s] + G_pv[e] gx_t v_s Av'                 (the coefficient of a)
//   Dga = C B' P + G_C B,    Dsc = ga C B'' P + B' C R + G_C ga B'
//   d_gx[t] += Dga v_s Av + a (Av G_v[s] + G_pv v_s Av')
//   d_q[t]  += Dsc k_s A + gsc (A G_k[s] + G_pk k_s A')
//   d_k[s]  += Dsc q_t A + gsc (A G_q[t] + G_pk q_t A')
//   d_v[s]  += Dga gx_t Av + a G_pv gx_t Av'
//   d_pk[e]  = Dsc q k A' + gsc (A' (G_q k + G_k q) + G_pk q k A'')
//   d_pv[e]  = Dga gx v Av' + a (gx Av' G_v + G_pv gx v Av'')
//   d_C[e]   = sum_h ga B' P + B R
// Rows on the destination side (X = q, GX = gx, YQ = G_q) and on the source side (K, VV, YK = G_k,
// YV = G_v) of one edge; DST: this wave owns the destination (else the source).
template <typename T, int V> struct Edge2 {
  T sc, pa, ga, P, Rp, R, gsc, a, Dga, Dsc, Bs, B1;
};

template <typename T, int V>
__device__ __forceinline__ Edge2<T, V> edge2(const T (&X)[V], const T (&GX)[V], const T (&YQ)[V], const T (&K)[V],
                                             const T (&VV)[V], const T (&YK)[V], const T (&YV)[V],
                                             const T (&ak)[V], const T (&ak1)[V], const T (&av)[V],
                                             const T (&av1)[V], const T (&ypk)[V], const T (&ypv)[V], T Ce, T yC,
                                             int lph, int AAT) {
  Edge2<T, V> r;
  T sc = T(0), pa = T(0), P = T(0), Rp = T(0);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    sc += X[i] * K[i] * ak[i];
    pa += GX[i] * VV[i] * av[i];
    P += ak[i] * (YQ[i] * K[i] + YK[i] * X[i]) + ypk[i] * X[i] * K[i] * ak1[i];
    Rp += GX[i] * (av[i] * YV[i] + ypv[i] * VV[i] * av1[i]);
  }
  r.sc = group_sum(sc, lph);
  r.pa = pa;
  r.ga = group_sum(pa, lph);
  r.P = group_sum(P, lph);
  r.Rp = Rp;
  r.R = group_sum(Rp, lph);
  const ActF<T> f(r.sc, AAT);
  r.Bs = f.s;
  r.B1 = f.d(r.sc);
  const T B2 = f.dd(r.sc);
  r.gsc = r.ga * Ce * r.B1;
  r.a = r.Bs * Ce;
  r.Dga = Ce * r.B1 * r.P + yC * r.Bs;
  r.Dsc = r.ga * Ce * B2 * r.P + r.B1 * Ce * r.R + yC * r.ga * r.B1;
  return r;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_t_bwd2(Args<T> A) {
  const int AKV = A.act_kv, AAT = A.act_at;
  zero_pad_rows(A, A.o_pk, A.ldopk, A.o_pv, A.ldopv, A.o_C);
  const Geo G = geo(A);
  const int t = G.node, c0 = G.c0;
  if (t < 0) return;
  const bool hk = A.pk != nullptr, hv = A.pv != nullptr;
  const bool lead = c0 == 0;
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  int s_r = 0;
  T C_r = T(0), yC_r = T(0);
  {  // ---- destination role: d_gx[t], d_q[t] and the per-edge outputs of row t
    T q[V], gx[V], yq[V], dgx[V], dq[V];
    ldv<T, V>(q, A.q + (size_t)t * A.ldq + c0);
    ldv<T, V>(gx, A.gx + (size_t)t * A.H + c0);
    ldv_opt<T, V>(yq, A.ggq, (size_t)t * A.ldggq + c0);
    zero(dgx); zero(dq);
    edge_chunks(A, b, e, G,
        [&](int k) {
          s_r = A.src[k];
          TMD_DCHECK(s_r >= 0 && s_r < A.n);
          C_r = A.C[k];
          yC_r = A.ggC ? A.ggC[k] : T(0);
        },
        [&](int k, int jj, bool live) {
          const int s = __shfl(s_r, jj);
          const T Ce = __shfl(C_r, jj), yC = __shfl(yC_r, jj);
          if (!live) return;
          T ks[V], vs[V], yk[V], yv[V], pk[V], pv[V], ypk[V], ypv[V];
          ldv<T, V>(ks, A.k + (size_t)s * A.ldk + c0);
          ldv<T, V>(vs, A.v + (size_t)s * A.ldv + c0);
          ldv_opt<T, V>(yk, A.ggk, (size_t)s * A.ldggk + c0);
          ldv_opt<T, V>(yv, A.ggv, (size_t)s * A.ldggv + c0);
          ldv_opt<T, V>(pk, A.pk, (size_t)k * A.ldpk + c0);
          ldv_opt<T, V>(pv, A.pv, (size_t)k * A.ldpv + c0);
          ldv_opt<T, V>(ypk, A.ggpk, (size_t)k * A.ldggpk + c0);
          ldv_opt<T, V>(ypv, A.ggpv, (size_t)k * A.ldggpv + c0);
          T ak[V], ak1[V], ak2[V], av[V], av1[V], av2[V];
          act<T, V, 2>(pk, hk, AKV, ak, ak1, ak2);
          act<T, V, 2>(pv, hv, AKV, av, av1, av2);
          const Edge2<T, V> E = edge2<T, V>(q, gx, yq, ks, vs, yk, yv, ak, ak1, av, av1, ypk, ypv, Ce, yC, A.lph, AAT);
          T opk[V], opv[V];
#pragma unroll
          for (int i = 0; i < V; ++i) {
            dgx[i] += E.Dga * vs[i] * av[i] + E.a * (av[i] * yv[i] + ypv[i] * vs[i] * av1[i]);
            dq[i] += E.Dsc * ks[i] * ak[i] + E.gsc * (ak[i] * yk[i] + ypk[i] * ks[i] * ak1[i]);
            opk[i] = E.Dsc * q[i] * ks[i] * ak1[i] +
                     E.gsc * (ak1[i] * (yq[i] * ks[i] + yk[i] * q[i]) + ypk[i] * q[i] * ks[i] * ak2[i]);
            opv[i] = E.Dga * gx[i] * vs[i] * av1[i] +
                     E.a * gx[i] * (av1[i] * yv[i] + ypv[i] * vs[i] * av2[i]);
          }
          if (A.o_pk) stv<T, V>(A.o_pk + (size_t)k * A.ldopk + c0, opk);
          if (A.o_pv) stv<T, V>(A.o_pv + (size_t)k * A.ldopv + c0, opv);
          const T dc = group_sum(E.pa * E.B1 * E.P + E.Bs * E.Rp, A.L);
          if (A.o_C && lead) A.o_C[k] = dc;
        });
    xor_slots(dgx, A.L); xor_slots(dq, A.L);
    if (G.es == 0) {
      if (A.o_gx) stv<T, V>(A.o_gx + (size_t)t * A.H + c0, dgx);
      if (A.o_q) stv<T, V>(A.o_q + (size_t)t * A.ldoq + c0, dq);
    }
  }
  if (!A.o_k && !A.o_v) return;
  {  // ---- source role: d_k[t], d_v[t] over the reversed edges r = (s <- t) of row t's edges (t <- s)
    T kt[V], vt[V], yk[V], yv[V], dk[V], dv[V];
    ldv<T, V>(kt, A.k + (size_t)t * A.ldk + c0);
    ldv<T, V>(vt, A.v + (size_t)t * A.ldv + c0);
    ldv_opt<T, V>(yk, A.ggk, (size_t)t * A.ldggk + c0);
    ldv_opt<T, V>(yv, A.ggv, (size_t)t * A.ldggv + c0);
    zero(dk); zero(dv);
    int r_r = -1;
    edge_chunks(A, b, e, G,
        [&](int k) {
          s_r = A.src[k];
          C_r = A.C[k];
          r_r = A.tr[k];
          if (r_r < 0 || r_r >= A.cap) r_r = -1;  // no reversed edge in the list: its cotangents read as zero
          yC_r = (A.ggC && r_r >= 0) ? A.ggC[r_r] : T(0);
        },
        [&](int k, int jj, bool live) {
          const int s = __shfl(s_r, jj), r = __shfl(r_r, jj);
          const T Ce = __shfl(C_r, jj), yC = __shfl(yC_r, jj);
          if (!live) return;
          T qs[V], gxs[V], yq[V], pk[V], pv[V], ypk[V], ypv[V];
          ldv<T, V>(qs, A.q + (size_t)s * A.ldq + c0);
          ldv<T, V>(gxs, A.gx + (size_t)s * A.H + c0);
          ldv_opt<T, V>(yq, A.ggq, (size_t)s * A.ldggq + c0);
          ldv_opt<T, V>(pk, A.pk, (size_t)k * A.ldpk + c0);
          ldv_opt<T, V>(pv, A.pv, (size_t)k * A.ldpv + c0);
          ldv_opt<T, V>(ypk, r >= 0 ? A.ggpk : nullptr, (size_t)(r >= 0 ? r : 0) * A.ldggpk + c0);
          ldv_opt<T, V>(ypv, r >= 0 ? A.ggpv : nullptr, (size_t)(r >= 0 ? r : 0) * A.ldggpv + c0);
          T ak[V], ak1[V], av[V], av1[V], u2[1];
          act<T, V, 1>(pk, hk, AKV, ak, ak1, u2);
          act<T, V, 1>(pv, hv, AKV, av, av1, u2);
          const Edge2<T, V> E = edge2<T, V>(qs, gxs, yq, kt, vt, yk, yv, ak, ak1, av, av1, ypk, ypv, Ce, yC, A.lph, AAT);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            dk[i] += E.Dsc * qs[i] * ak[i] + E.gsc * (ak[i] * yq[i] + ypk[i] * qs[i] * ak1[i]);
            dv[i] += E.Dga * gxs[i] * av[i] + E.a * ypv[i] * gxs[i] * av1[i];
          }
        });
    xor_slots(dk, A.L); xor_slots(dv, A.L);
    if (G.es == 0) {
      if (A.o_k) stv<T, V>(A.o_k + (size_t)t * A.ldok + c0, dk);
      if (A.o_v) stv<T, V>(A.o_v + (size_t)t * A.ldov + c0, dv);
    }
  }
}

// ------------------------------------------------------------------ host side
template <typename T> static bool aligned(const void* p, int ld, int V) {
  if (!p) return true;
  const int VA = V > 4 ? 4 : V;
  return ((uintptr_t)p % (sizeof(T) * VA)) == 0 && (ld % VA) == 0;
}

// The width envelope (the ET message's): H = 32 V with V in {1, 2, 4, 8} and d / V a power of two, or
// H < 32 with H and d powers of two (V = 1, one edge per H lanes).
static int envelope(int H, int heads, int& V) {
  if (H <= 0 || heads <= 0 || H % heads) return kBadArgument;
  const int d = H / heads;
  if (H % 32 == 0) V = H / 32;
  else if (H < 32 && !(H & (H - 1))) V = 1;
  else return kUnsupported;
  if (V != 1 && V != 2 && V != 4 && V != 8) return kUnsupported;
  if (d % V) return kUnsupported;
  const int lph = d / V;
  if (lph & (lph - 1)) return kUnsupported;
  return kOk;
}

template <typename T>
static int setup(Args<T>& A, int n, int H, int heads, int V, const int32_t* row_ptr, const int32_t* src, int cap,
                 const void* q, int ldq, const void* k, int ldk, const void* v, int ldv_, const void* pk, int ldpk,
                 const void* pv, int ldpv, const void* C, int flags) {
  if (n < 0 || cap < 0 || !row_ptr || !src || !q || !k || !v || !C) return kBadArgument;
  if (ldq < H || ldk < H || ldv_ < H || (pk && ldpk < H) || (pv && ldpv < H)) return kBadArgument;
  if (!aligned<T>(q, ldq, V) || !aligned<T>(k, ldk, V) || !aligned<T>(v, ldv_, V) || !aligned<T>(pk, ldpk, V) ||
      !aligned<T>(pv, ldpv, V))
    return kBadArgument;
  A = Args<T>{};
  A.n = n; A.H = H; A.L = H / V; A.lph = H / heads / V; A.cap = cap;
  A.row_ptr = row_ptr; A.src = src;
  A.q = (const T*)q; A.ldq = ldq; A.k = (const T*)k; A.ldk = ldk; A.v = (const T*)v; A.ldv = ldv_;
  A.pk = (const T*)pk; A.ldpk = ldpk; A.pv = (const T*)pv; A.ldpv = ldpv; A.C = (const T*)C;
  A.act_kv = (flags >> 8) & 15;
  A.act_at = (flags >> 12) & 15;
  if (A.act_kv > kActSigmoid || A.act_at > kActSigmoid) return kBadArgument;
  return kOk;
}

template <typename T, int KIND, int V>
static void launch_k(const Args<T>& A, hipStream_t st) {
  const dim3 g((A.n + 3) / 4), b(256);
  const bool silu = A.act_kv == kActSilu && A.act_at == kActSilu;
  if constexpr (KIND == 0) {
    if (silu) hipLaunchKernelGGL((k_t_fwd<T, V, false>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_t_fwd<T, V, true>), g, b, 0, st, A);
  } else if constexpr (KIND == 1) {
    if (silu) hipLaunchKernelGGL((k_t_bwd<T, V, false>), g, b, 0, st, A);
    else hipLaunchKernelGGL((k_t_bwd<T, V, true>), g, b, 0, st, A);
  } else {
    hipLaunchKernelGGL((k_t_bwd2<T, V>), g, b, 0, st, A);
  }
}

template <typename T, int KIND>
static int launch(int V, const Args<T>& A, hipStream_t st) {
  if (A.n <= 0) return kOk;
  switch (V) {
    case 1: launch_k<T, KIND, 1>(A, st); break;
    case 2: launch_k<T, KIND, 2>(A, st); break;
    case 4: launch_k<T, KIND, 4>(A, st); break;
    case 8:
      if constexpr (KIND != 2) { launch_k<T, KIND, 8>(A, st); break; }
      return kUnsupported;
    default: return kUnsupported;
  }
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

static constexpr int kKnownBits = TMDNET_ET_SCALAR | 0xff00;  // every other bit belongs to the vector form

template <typename T>
static int fwd(int n, int H, int heads, const int32_t* row_ptr, const int32_t* src, int cap, const void* q, int ldq,
               const void* k, int ldk, const void* v, int ldv_, const void* pk, int ldpk, const void* pv, int ldpv,
               const void* C, void* xo, int flags, const int32_t* order, hipStream_t st) {
  int V;
  int rc = envelope(H, heads, V);
  if (rc) return rc;
  Args<T> A;
  if ((rc = setup<T>(A, n, H, heads, V, row_ptr, src, cap, q, ldq, k, ldk, v, ldv_, pk, ldpk, pv, ldpv, C, flags)))
    return rc;
  if (!xo || !aligned<T>(xo, H, V)) return kBadArgument;
  A.xo = (T*)xo;
  A.order = order;
  return launch<T, 0>(V, A, st);
}

template <typename T>
static int bwd(int n, int H, int heads, const int32_t* row_ptr, const int32_t* src, int cap, const void* q, int ldq,
               const void* k, int ldk, const void* v, int ldv_, const void* pk, int ldpk, const void* pv, int ldpv,
               const void* C, const void* gx, void* gq, void* gk, void* gv, void* gpk, void* gpv, void* gC, int flags,
               const int32_t* order, hipStream_t st) {
  int V;
  int rc = envelope(H, heads, V);
  if (rc) return rc;
  Args<T> A;
  if ((rc = setup<T>(A, n, H, heads, V, row_ptr, src, cap, q, ldq, k, ldk, v, ldv_, pk, ldpk, pv, ldpv, C, flags)))
    return rc;
  if (!gx || !aligned<T>(gx, H, V) || (gpk && !pk) || (gpv && !pv)) return kBadArgument;
  if (!aligned<T>(gq, ldq, V) || !aligned<T>(gk, ldk, V) || !aligned<T>(gv, ldv_, V) || !aligned<T>(gpk, ldpk, V) ||
      !aligned<T>(gpv, ldpv, V))
    return kBadArgument;
  A.gx = (const T*)gx;
  A.gq = (T*)gq; A.gk = (T*)gk; A.gv = (T*)gv; A.gpk = (T*)gpk; A.gpv = (T*)gpv; A.gC = (T*)gC;
  A.order = order;
  return launch<T, 1>(V, A, st);
}

struct Bwd2 {  // the second order's cotangents, outputs and their row strides (0 = H)
  const int32_t* tr;
  const void *ggq, *ggk, *ggv, *ggpk, *ggpv, *ggC;
  int ldggq, ldggk, ldggv, ldggpk, ldggpv;
  void *o_gx, *o_q, *o_k, *o_v, *o_pk, *o_pv, *o_C;
  int ldoq, ldok, ldov, ldopk, ldopv;
};

template <typename T>
static int bwd2(int n, int H, int heads, const int32_t* row_ptr, const int32_t* src, int cap, const void* q, int ldq,
                const void* k, int ldk, const void* v, int ldv_, const void* pk, int ldpk, const void* pv, int ldpv,
                const void* C, const void* gx, const Bwd2& X, int flags, hipStream_t st) {
  int V;
  int rc = envelope(H, heads, V);
  if (rc) return rc;
  if (!X.tr) return kUnsupported;  // the source role reads the reversed edges' cotangents through it
  // narrower lanes than the first order (one edge per wave instruction from H = 64): a role keeps ~20 row
  // segments of an edge live
  if (H % 64 == 0) V = H / 64;
  Args<T> A;
  if ((rc = setup<T>(A, n, H, heads, V, row_ptr, src, cap, q, ldq, k, ldk, v, ldv_, pk, ldpk, pv, ldpv, C, flags)))
    return rc;
  auto pick = [H](int x) { return x ? x : H; };
  A.tr = X.tr;
  A.gx = (const T*)gx;
  A.ggq = (const T*)X.ggq; A.ldggq = pick(X.ldggq);
  A.ggk = (const T*)X.ggk; A.ldggk = pick(X.ldggk);
  A.ggv = (const T*)X.ggv; A.ldggv = pick(X.ldggv);
  A.ggpk = (const T*)X.ggpk; A.ldggpk = pick(X.ldggpk);
  A.ggpv = (const T*)X.ggpv; A.ldggpv = pick(X.ldggpv);
  A.ggC = (const T*)X.ggC;
  A.o_gx = (T*)X.o_gx;
  A.o_q = (T*)X.o_q; A.ldoq = pick(X.ldoq);
  A.o_k = (T*)X.o_k; A.ldok = pick(X.ldok);
  A.o_v = (T*)X.o_v; A.ldov = pick(X.ldov);
  A.o_pk = (T*)X.o_pk; A.ldopk = pick(X.ldopk);
  A.o_pv = (T*)X.o_pv; A.ldopv = pick(X.ldopv);
  A.o_C = (T*)X.o_C;
  if (!gx || (!pk && (X.ggpk || X.o_pk)) || (!pv && (X.ggpv || X.o_pv))) return kBadArgument;
  if (A.ldggq < H || A.ldggk < H || A.ldggv < H || A.ldggpk < H || A.ldggpv < H || A.ldoq < H || A.ldok < H ||
      A.ldov < H || A.ldopk < H || A.ldopv < H)
    return kBadArgument;
  if (!aligned<T>(gx, H, V) || !aligned<T>(A.ggq, A.ldggq, V) || !aligned<T>(A.ggk, A.ldggk, V) ||
      !aligned<T>(A.ggv, A.ldggv, V) || !aligned<T>(A.ggpk, A.ldggpk, V) || !aligned<T>(A.ggpv, A.ldggpv, V) ||
      !aligned<T>(A.o_gx, H, V) || !aligned<T>(A.o_q, A.ldoq, V) || !aligned<T>(A.o_k, A.ldok, V) ||
      !aligned<T>(A.o_v, A.ldov, V) || !aligned<T>(A.o_pk, A.ldopk, V) || !aligned<T>(A.o_pv, A.ldopv, V))
    return kBadArgument;
  return launch<T, 2>(V, A, st);
}

}  // namespace tmsg

// The scalar form of the three ET message entry points (et_message.hip dispatches here when the call
// carries TMDNET_ET_SCALAR).  Operands of the vector form must be absent: checked by the callers below
// before anything is launched.
int t_message_fwd(int dtype, int n, int H, int heads, const int32_t* row_ptr, const int32_t* src, int cap,
                  const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* vec_in,
                  const void* pk, int ldpk, const void* pv, int ldpv, const void* C, const void* unit, void* xo,
                  void* vec_out, int flags, const int32_t* pk_rows, const int32_t* order, hipStream_t st) {
  if (vec_in || unit || vec_out || pk_rows || (flags & ~tmsg::kKnownBits)) return kBadArgument;
  if (dtype == TMDNET_F32)
    return tmsg::fwd<float>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, xo, flags,
                            order, st);
  if (dtype == TMDNET_F64)
    return tmsg::fwd<double>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, xo, flags,
                             order, st);
  return kUnsupported;
}

int t_message_bwd(int dtype, int n, int H, int heads, const int32_t* row_ptr, const int32_t* src, int cap,
                  const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* vec_in,
                  const void* pk, int ldpk, const void* pv, int ldpv, const void* C, const void* unit, const void* gx,
                  const void* grad_vec, void* gq, void* gk, void* gv, void* gvec_in, void* gpk, void* gpv, void* gC,
                  void* gunit, const void* dpk, const void* dpv, void* gdist, int flags, const int32_t* pk_rows,
                  const int32_t* order, hipStream_t st) {
  if (vec_in || unit || grad_vec || gvec_in || gunit || dpk || dpv || gdist || pk_rows ||
      (flags & ~tmsg::kKnownBits))
    return kBadArgument;
  if (dtype == TMDNET_F32)
    return tmsg::bwd<float>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, gx, gq, gk,
                            gv, gpk, gpv, gC, flags, order, st);
  if (dtype == TMDNET_F64)
    return tmsg::bwd<double>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, gx, gq,
                             gk, gv, gpk, gpv, gC, flags, order, st);
  return kUnsupported;
}

int t_message_bwd2(int dtype, int n, int H, int heads, const int32_t* row_ptr, const int32_t* src,
                   const int32_t* transpose, int cap, const void* q, int ldq, const void* k, int ldk, const void* v,
                   int ldv, const void* vec_in, const void* pk, int ldpk, const void* pv, int ldpv, const void* C,
                   const void* unit, const void* gx, const void* grad_vec, const void* gg_q, int ld_ggq,
                   const void* gg_k, int ld_ggk, const void* gg_v, int ld_ggv, const void* gg_vec, const void* gg_pk,
                   int ld_ggpk, const void* gg_pv, int ld_ggpv, const void* gg_cut, const void* gg_unit,
                   void* d_grad_x, void* d_grad_vec, void* d_q, int ld_dq, void* d_k, int ld_dk, void* d_v, int ld_dv,
                   void* d_vec, void* d_pk, int ld_dpk, void* d_pv, int ld_dpv, void* d_cut, void* d_unit,
                   const int32_t* pk_rows, const void* gg_pkv_scale, int flags, hipStream_t st) {
  if (vec_in || unit || grad_vec || gg_vec || gg_unit || d_grad_vec || d_vec || d_unit || pk_rows || gg_pkv_scale ||
      (flags & ~tmsg::kKnownBits))
    return kBadArgument;
  const tmsg::Bwd2 X{transpose, gg_q, gg_k, gg_v, gg_pk, gg_pv, gg_cut, ld_ggq, ld_ggk, ld_ggv, ld_ggpk, ld_ggpv,
                     d_grad_x, d_q, d_k, d_v, d_pk, d_pv, d_cut, ld_dq, ld_dk, ld_dv, ld_dpk, ld_dpv};
  if (dtype == TMDNET_F32)
    return tmsg::bwd2<float>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, gx, X,
                             flags, st);
  if (dtype == TMDNET_F64)
    return tmsg::bwd2<double>(n, H, heads, row_ptr, src, cap, q, ldq, k, ldk, v, ldv, pk, ldpk, pv, ldpv, C, gx, X,
                              flags, st);
  return kUnsupported;
}

}  // namespace tmd
