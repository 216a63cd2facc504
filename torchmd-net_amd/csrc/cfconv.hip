// Continuous-filter convolution of the graph-network model (reference models/torchmd_gn.py:236-272,
// CFConv.message / propagate) over the destination-grouped CSR edge list:
//   m[e][f]   = h[src_e][f] * w[e][f] * C[e]
//   out[t][f] = aggr_{e in row t} m[e][f],   aggr = add | mean | max
// with the first backward (gh, gw, gC) and its VJP (force-matching training).  Nothing here assumes
// that w or C agree on an edge and its reverse: every reverse-edge quantity is read through the
// transpose map.  Self loops are ordinary edges.  A wave owns one row (or a share of one); lanes own
// V-wide channel groups and loop over them when F > 64 V.  Plain vector loads and stores only, no
// atomics: every output element has one writer and a fixed summation order (bitwise reproducible).
//
// max: ties go to the LOWEST edge index of the row (the scan is in ascending edge order and replaces
// only on a strictly greater message); an empty row gives out = 0, arg = -1.
#include <initializer_list>
#include <utility>

#include "common.h"
#include "tmdnet.h"

namespace tmd {
namespace cf {

template <typename T, int V> struct alignas(sizeof(T) * V) Pack { T v[V]; };

template <typename T, int V> __device__ __forceinline__ void ldv(T (&o)[V], const T* p) {
  const Pack<T, V> q = *reinterpret_cast<const Pack<T, V>*>(p);
#pragma unroll
  for (int i = 0; i < V; ++i) o[i] = q.v[i];
}
template <typename T, int V> __device__ __forceinline__ void stv(T* p, const T (&o)[V]) {
  Pack<T, V> q;
#pragma unroll
  for (int i = 0; i < V; ++i) q.v[i] = o[i];
  *reinterpret_cast<Pack<T, V>*>(p) = q;
}
template <typename T, int V> __device__ __forceinline__ void zero(T (&o)[V]) {
#pragma unroll
  for (int i = 0; i < V; ++i) o[i] = T(0);
}

template <typename T> struct CfArgs {
  int n, F, cap, aggr;
  const int32_t* row_ptr;
  const int32_t* src;
  const int32_t* tr;  // tr[e] = index of the reversed edge (source passes)
  const T* h; int ldh;
  const T* w; int ldw;
  const T* C;
  T* out;
  int32_t* arg;            // [n][F] winning edge of the max (written by the forward, read by the rest)
  const T* g; int ldg;     // incoming gradient rows
  T* gh; T* gw; T* gC;
  // second order: cotangents of gh / gw / gC (NULL = 0) and their VJP outputs (NULL = not wanted)
  const T* ggh; const T* ggw; const T* ggC;
  T* dg; T* dh; T* dw; T* dC;
};

constexpr int CF_U = 4;  // edges per step: their row loads are in flight together

__device__ __forceinline__ int row_len(const int32_t* row_ptr, int row, int cap) {
  return min(row_ptr[row + 1], cap) - min(row_ptr[row], cap);
}

// Edge loop of a row [b, e): src, C (and the transpose map) of up to 64 edges arrive in one coalesced
// load each and are broadcast by shuffle.  body(sq, kq, cq, xq) per CF_U edges:
//   sq  the other node of the edge (-1: past the row end or out of range -- contributes nothing)
//   kq  the edge whose w / C / arg apply: the row's own edge, or with REV its reverse tr[e] (the edge
//       LEAVING this row's node)
//   cq  C[kq]; with REV and mean also times 1 / max(deg(sq), 1), the scale of the row kq lives in
//   xq  extra[kq] (same scaling; 0 without `extra`)
// (sub, nsub): this wave takes every nsub-th group of CF_U edges (waves sharing a node).
template <typename T, bool REV, typename F>
__device__ __forceinline__ void cf_edges(const CfArgs<T>& A, int b, int e, const T* extra, F&& body, int sub = 0,
                                         int nsub = 1) {
  const int lane = lane_id();
  for (int base = b; base < e; base += TMD_WAVE) {
    const int cnt = min(TMD_WAVE, e - base);
    int s_l = lane < cnt ? A.src[base + lane] : -1;
    int k_l = base + lane;
    if (REV) k_l = lane < cnt ? A.tr[base + lane] : -1;
    if ((unsigned)s_l >= (unsigned)A.n || (unsigned)k_l >= (unsigned)A.cap) s_l = -1;
    T c_l = T(0), x_l = T(0);
    if (s_l >= 0) {
      c_l = A.C[k_l];
      if (extra) x_l = extra[k_l];
      if (REV && A.aggr == TMDNET_AGGR_MEAN) {
        const T sc = T(1) / T(max(row_len(A.row_ptr, s_l, A.cap), 1));
        c_l *= sc;
        x_l *= sc;
      }
    }
    for (int q = sub * CF_U; q < cnt; q += CF_U * nsub) {
      int sq[CF_U], kq[CF_U];
      T cq[CF_U], xq[CF_U];
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const int l = (q + u) & (TMD_WAVE - 1);
        sq[u] = __shfl(s_l, l);
        kq[u] = REV ? __shfl(k_l, l) : base + q + u;
        cq[u] = __shfl(c_l, l);
        xq[u] = __shfl(x_l, l);
        if (q + u >= cnt) sq[u] = -1;
      }
      body(sq, kq, cq, xq);
    }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_cf_fwd(CfArgs<T> A) {
  const int t = blockIdx.x * (blockDim.x / TMD_WAVE) + threadIdx.x / TMD_WAVE;
  if (t >= A.n) return;
  const int lane = lane_id();
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  const bool mx = A.aggr == TMDNET_AGGR_MAX;
  const T scale = A.aggr == TMDNET_AGGR_MEAN ? T(1) / T(max(e - b, 1)) : T(1);
  for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {
    const bool on = cb + lane * V < A.F;
    const int c0 = on ? cb + lane * V : 0;
    T acc[V];
    int32_t best[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc[i] = mx ? -T(INFINITY) : T(0);
      best[i] = -1;
    }
    cf_edges<T, false>(A, b, e, nullptr, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                             const T (&)[CF_U]) {
      T hs[CF_U][V], wk[CF_U][V];
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const int s = live ? sq[u] : t, k = live ? kq[u] : b;
        ldv<T, V>(hs[u], A.h + (size_t)s * A.ldh + c0);
        ldv<T, V>(wk[u], A.w + (size_t)k * A.ldw + c0);
      }
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const T ce = live ? cq[u] : T(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const T m = hs[u][i] * (wk[u][i] * ce);
          if (mx) {
            if (live && m > acc[i]) {
              acc[i] = m;
              best[i] = kq[u];
            }
          } else {
            acc[i] += m;
          }
        }
      }
    });
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (mx && best[i] < 0) acc[i] = T(0);
      acc[i] *= scale;
    }
    if (on) {
      stv<T, V>(A.out + (size_t)t * A.F + c0, acc);
      if (mx) stv<int32_t, V>(A.arg + (size_t)t * A.F + c0, best);
    }
  }
}

// destination pass: gw[e] = sel g[t] h[s] C[e] scale_t, gC[e] = sum_f sel g[t] h[s] w[e] scale_t; the
// padding slots [row_ptr[n], cap) of gw / gC are zeroed here too (no memset before the launch)
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cf_bwd_dst(CfArgs<T> A) {
  {
    const int e0 = min(A.row_ptr[A.n], A.cap);
    const long long rows = A.cap - e0;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    for (long long i = tid; i < rows * A.F; i += nth) A.gw[(size_t)e0 * A.F + i] = T(0);
    for (long long i = tid; i < rows; i += nth) A.gC[e0 + i] = T(0);
  }
  // four waves per node, each a quarter of the row's edges (the outputs are per edge: no reduction)
  const int t = blockIdx.x, sub = threadIdx.x / TMD_WAVE, nsub = blockDim.x / TMD_WAVE;
  if (t >= A.n) return;
  const int lane = lane_id();
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  const bool mx = A.aggr == TMDNET_AGGR_MAX;
  const T scale = A.aggr == TMDNET_AGGR_MEAN ? T(1) / T(max(e - b, 1)) : T(1);
  cf_edges<T, false>(A, b, e, nullptr, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                           const T (&)[CF_U]) {
    T gc[CF_U];
    zero(gc);
    for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {  // gC's channel sum spans the whole loop
      const bool on = cb + lane * V < A.F;
      const int c0 = on ? cb + lane * V : 0;
      T go[V], hs[CF_U][V], wk[CF_U][V];
      int32_t ar[V];
      ldv<T, V>(go, A.g + (size_t)t * A.ldg + c0);
      if (mx) ldv<int32_t, V>(ar, A.arg + (size_t)t * A.F + c0);
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const int s = live ? sq[u] : t, k = live ? kq[u] : b;
        ldv<T, V>(hs[u], A.h + (size_t)s * A.ldh + c0);
        ldv<T, V>(wk[u], A.w + (size_t)k * A.ldw + c0);
      }
#pragma unroll
      for (int i = 0; i < V; ++i) go[i] = on ? go[i] * scale : T(0);
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const T ce = live ? cq[u] : T(0);
        T gw[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const T gs = (mx && ar[i] != kq[u]) ? T(0) : go[i];
          gw[i] = gs * hs[u][i] * ce;
          gc[u] += gs * hs[u][i] * wk[u][i];
        }
        if (on && kq[u] < e) stv<T, V>(A.gw + (size_t)kq[u] * A.F + c0, gw);  // (an out-of-range source: zeros)
      }
    }
#pragma unroll
    for (int u = 0; u < CF_U; ++u) gc[u] = wave_sum(gc[u]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < CF_U; ++u)
        if (kq[u] < e) A.gC[kq[u]] = sq[u] >= 0 ? gc[u] : T(0);
    }
  }, sub, nsub);
}

// source pass: gh[j] = sum over the edges e = tr[e'] leaving j (e' in row j, e' = (m -> j)) of
//   sel(m, f, e) g[m] w[e] C[e] scale_m
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cf_bwd_src(CfArgs<T> A) {
  const int j = blockIdx.x * (blockDim.x / TMD_WAVE) + threadIdx.x / TMD_WAVE;
  if (j >= A.n) return;
  const int lane = lane_id();
  const int b = min(A.row_ptr[j], A.cap), e = min(A.row_ptr[j + 1], A.cap);
  const bool mx = A.aggr == TMDNET_AGGR_MAX;
  for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {
    const bool on = cb + lane * V < A.F;
    const int c0 = on ? cb + lane * V : 0;
    T acc[V];
    zero(acc);
    cf_edges<T, true>(A, b, e, nullptr, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                            const T (&)[CF_U]) {
      T gm[CF_U][V], wk[CF_U][V];
      int32_t ar[CF_U][V];
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const int m = live ? sq[u] : j, k = live ? kq[u] : 0;
        ldv<T, V>(gm[u], A.g + (size_t)m * A.ldg + c0);
        ldv<T, V>(wk[u], A.w + (size_t)k * A.ldw + c0);
        if (mx) ldv<int32_t, V>(ar[u], A.arg + (size_t)m * A.F + c0);
      }
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const T ce = sq[u] >= 0 ? cq[u] : T(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const T gs = (mx && ar[u][i] != kq[u]) ? T(0) : gm[u][i];
          acc[i] += gs * (wk[u][i] * ce);
        }
      }
    });
    if (on) stv<T, V>(A.gh + (size_t)j * A.F + c0, acc);
  }
}

// Second order.  The backward is trilinear in (g, h, w, C) given arg and deg (piecewise constant), so
// with S = sel(t, f, e) scale_t its VJP for cotangents (ggh, ggw, ggC) of (gh, gw, gC) is
//   d_g[t] = sum_{e in row t} S (ggh[s] w_e C_e + h[s] (ggw_e C_e + ggC_e w_e))
//   d_w[e] = S g[t] (C_e ggh[s] + ggC_e h[s])
//   d_C[e] = sum_f S g[t] (ggh[s] w_e + ggw_e h[s])                              (destination pass)
//   d_h[j] = sum_{e = tr[e'], e' in row j} S g[dst_e] (ggw_e C_e + ggC_e w_e)      (source pass)
// d_g accumulates over a row's edges per channel group, d_C over the channel groups per edge: with one
// group (F <= 64 V) both come out of one sweep, otherwise d_C takes a second sweep of the row.
template <typename T, int V, typename St>
__device__ __forceinline__ void cf_bwd2_group(const CfArgs<T>& A, int t, int b, int e, int c0, bool on, T scale,
                                              const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                              const T (&xq)[CF_U], T (&acc)[V], T (&dc)[CF_U], St&& store_dw) {
  const bool mx = A.aggr == TMDNET_AGGR_MAX;
  T go[V], hs[CF_U][V], wk[CF_U][V], gxs[CF_U][V], gwk[CF_U][V];
  int32_t ar[V];
  ldv<T, V>(go, A.g + (size_t)t * A.ldg + c0);
  if (mx) ldv<int32_t, V>(ar, A.arg + (size_t)t * A.F + c0);
#pragma unroll
  for (int u = 0; u < CF_U; ++u) {
    const bool live = sq[u] >= 0;
    const int s = live ? sq[u] : t, k = live ? kq[u] : b;
    ldv<T, V>(hs[u], A.h + (size_t)s * A.ldh + c0);
    ldv<T, V>(wk[u], A.w + (size_t)k * A.ldw + c0);
    if (A.ggh) ldv<T, V>(gxs[u], A.ggh + (size_t)s * A.F + c0); else zero(gxs[u]);
    if (A.ggw) ldv<T, V>(gwk[u], A.ggw + (size_t)k * A.F + c0); else zero(gwk[u]);
  }
#pragma unroll
  for (int i = 0; i < V; ++i) go[i] = on ? go[i] * scale : T(0);
#pragma unroll
  for (int u = 0; u < CF_U; ++u) {
    const bool live = sq[u] >= 0;
    const T ce = live ? cq[u] : T(0), gc = live ? xq[u] : T(0);
    T dw[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool sel = live && !(mx && ar[i] != kq[u]);
      const T gs = sel ? go[i] : T(0);
      const T a = ce * (gxs[u][i] * wk[u][i] + hs[u][i] * gwk[u][i]) + gc * hs[u][i] * wk[u][i];
      acc[i] += sel ? a : T(0);
      dw[i] = gs * (ce * gxs[u][i] + gc * hs[u][i]);
      dc[u] += gs * (gxs[u][i] * wk[u][i] + gwk[u][i] * hs[u][i]);
    }
    if (on && kq[u] < e) store_dw(kq[u], dw);  // (an out-of-range source: zeros, as k_cf_bwd_dst)
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_cf_bwd2_dst(CfArgs<T> A) {
  const int t = blockIdx.x * (blockDim.x / TMD_WAVE) + threadIdx.x / TMD_WAVE;
  if (t >= A.n) return;
  const int lane = lane_id();
  const int b = min(A.row_ptr[t], A.cap), e = min(A.row_ptr[t + 1], A.cap);
  const T scale = A.aggr == TMDNET_AGGR_MEAN ? T(1) / T(max(e - b, 1)) : T(1);
  const bool one = A.F <= TMD_WAVE * V;
  auto put_dc = [&](const int (&sq)[CF_U], const int (&kq)[CF_U], T (&dc)[CF_U]) {
#pragma unroll
    for (int u = 0; u < CF_U; ++u) dc[u] = wave_sum(dc[u]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < CF_U; ++u)
        if (kq[u] < e) A.dC[kq[u]] = dc[u];  // (dc is 0 for an out-of-range source)
    }
  };
  if (A.dg || A.dw || (A.dC && one)) {
    for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {
      const bool on = cb + lane * V < A.F;
      const int c0 = on ? cb + lane * V : 0;
      T acc[V];
      zero(acc);
      cf_edges<T, false>(A, b, e, A.ggC, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                             const T (&xq)[CF_U]) {
        T dc[CF_U];
        zero(dc);
        cf_bwd2_group<T, V>(A, t, b, e, c0, on, scale, sq, kq, cq, xq, acc, dc, [&](int k, const T (&dw)[V]) {
          if (A.dw) stv<T, V>(A.dw + (size_t)k * A.F + c0, dw);
        });
        if (A.dC && one) put_dc(sq, kq, dc);
      });
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] *= scale;
      if (on && A.dg) stv<T, V>(A.dg + (size_t)t * A.F + c0, acc);
    }
  }
  if (A.dC && !one) {
    cf_edges<T, false>(A, b, e, A.ggC, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                           const T (&xq)[CF_U]) {
      T dc[CF_U], acc[V];
      zero(dc);
      zero(acc);
      for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {
        const bool on = cb + lane * V < A.F;
        const int c0 = on ? cb + lane * V : 0;
        cf_bwd2_group<T, V>(A, t, b, e, c0, on, scale, sq, kq, cq, xq, acc, dc, [](int, const T (&)[V]) {});
      }
      put_dc(sq, kq, dc);
    });
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_cf_bwd2_src(CfArgs<T> A) {
  const int j = blockIdx.x * (blockDim.x / TMD_WAVE) + threadIdx.x / TMD_WAVE;
  if (j >= A.n) return;
  const int lane = lane_id();
  const int b = min(A.row_ptr[j], A.cap), e = min(A.row_ptr[j + 1], A.cap);
  const bool mx = A.aggr == TMDNET_AGGR_MAX;
  for (int cb = 0; cb < A.F; cb += TMD_WAVE * V) {
    const bool on = cb + lane * V < A.F;
    const int c0 = on ? cb + lane * V : 0;
    T acc[V];
    zero(acc);
    cf_edges<T, true>(A, b, e, A.ggC, [&](const int (&sq)[CF_U], const int (&kq)[CF_U], const T (&cq)[CF_U],
                                          const T (&xq)[CF_U]) {
      T gm[CF_U][V], wk[CF_U][V], gwk[CF_U][V];
      int32_t ar[CF_U][V];
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const int m = live ? sq[u] : j, k = live ? kq[u] : 0;
        ldv<T, V>(gm[u], A.g + (size_t)m * A.ldg + c0);
        ldv<T, V>(wk[u], A.w + (size_t)k * A.ldw + c0);
        if (A.ggw) ldv<T, V>(gwk[u], A.ggw + (size_t)k * A.F + c0); else zero(gwk[u]);
        if (mx) ldv<int32_t, V>(ar[u], A.arg + (size_t)m * A.F + c0);
      }
#pragma unroll
      for (int u = 0; u < CF_U; ++u) {
        const bool live = sq[u] >= 0;
        const T ce = live ? cq[u] : T(0), gc = live ? xq[u] : T(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const T gs = (mx && ar[u][i] != kq[u]) ? T(0) : gm[u][i];
          acc[i] += gs * (gwk[u][i] * ce + gc * wk[u][i]);
        }
      }
    });
    if (on) stv<T, V>(A.dh + (size_t)j * A.F + c0, acc);
  }
}

// ------------------------------------------------------------------ host side
template <typename T>
static bool aligned(const void* p, int ld, int V) {
  if (!p) return true;
  return ((uintptr_t)p % (sizeof(T) * V)) == 0 && (ld % V) == 0;
}

// widest V in {4, 2, 1} that divides F, fills a wave's 64 lanes (F >= 64 V) and that every row base
// and stride is aligned for
template <typename T>
static int pick_vec(int F, std::initializer_list<std::pair<const void*, int>> rows) {
  for (int V = 4; V > 1; V >>= 1) {
    if (F % V || F < TMD_WAVE * V) continue;
    bool ok = true;
    for (const auto& r : rows) ok = ok && aligned<T>(r.first, r.second, V);
    if (ok) return V;
  }
  return 1;
}

template <typename T>
static int setup(CfArgs<T>& A, int aggr, int n, int F, const int32_t* row_ptr, const int32_t* src,
                 const int32_t* tr, int cap, const void* h, int ldh, const void* w, int ldw, const void* C,
                 const int32_t* arg) {
  if (aggr != TMDNET_AGGR_ADD && aggr != TMDNET_AGGR_MEAN && aggr != TMDNET_AGGR_MAX) return kUnsupported;
  if (n < 0 || F < 1 || cap < 0 || !row_ptr || (cap > 0 && (!src || !w || !C)) || (n > 0 && !h)) return kBadArgument;
  A = CfArgs<T>{};
  A.n = n; A.F = F; A.cap = cap; A.aggr = aggr; A.row_ptr = row_ptr; A.src = src; A.tr = tr;
  A.h = (const T*)h; A.ldh = ldh ? ldh : F; A.w = (const T*)w; A.ldw = ldw ? ldw : F; A.C = (const T*)C;
  A.arg = const_cast<int32_t*>(arg);
  if (A.ldh < F || A.ldw < F) return kBadArgument;
  if (aggr == TMDNET_AGGR_MAX && !arg && n > 0) return kBadArgument;
  return kOk;
}

template <typename T, int V> struct KFwd { static constexpr auto fn = k_cf_fwd<T, V>; };
template <typename T, int V> struct KDst { static constexpr auto fn = k_cf_bwd_dst<T, V>; };
template <typename T, int V> struct KSrc { static constexpr auto fn = k_cf_bwd_src<T, V>; };
template <typename T, int V> struct K2Dst { static constexpr auto fn = k_cf_bwd2_dst<T, V>; };
template <typename T, int V> struct K2Src { static constexpr auto fn = k_cf_bwd2_src<T, V>; };

// wpn waves of a 256-thread block share a node (4: one block per node), else one wave per node
template <typename T, template <typename, int> class K>
static int launch(int V, int n, bool block_per_node, const CfArgs<T>& A, hipStream_t st) {
  if (n <= 0) return kOk;
  const int tb = 256, wpb = tb / TMD_WAVE;
  dim3 g(block_per_node ? n : (n + wpb - 1) / wpb);
  if (V == 1) hipLaunchKernelGGL((K<T, 1>::fn), g, dim3(tb), 0, st, A);
  else if (V == 2) hipLaunchKernelGGL((K<T, 2>::fn), g, dim3(tb), 0, st, A);
  else hipLaunchKernelGGL((K<T, 4>::fn), g, dim3(tb), 0, st, A);
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

template <typename T>
static int fwd(int aggr, int n, int F, const int32_t* row_ptr, const int32_t* src, int cap, const void* h, int ldh,
               const void* w, int ldw, const void* C, void* out, int32_t* arg, hipStream_t st) {
  CfArgs<T> A;
  int rc = setup<T>(A, aggr, n, F, row_ptr, src, nullptr, cap, h, ldh, w, ldw, C, arg);
  if (rc) return rc;
  if (!out && n > 0) return kBadArgument;
  A.out = (T*)out;
  int V = pick_vec<T>(F, {{h, A.ldh}, {w, A.ldw}, {out, F}});
  if (!aligned<int32_t>(arg, F, V)) V = 1;
  return launch<T, KFwd>(V, n, false, A, st);
}

template <typename T>
static int bwd(int aggr, int n, int F, const int32_t* row_ptr, const int32_t* src, const int32_t* tr, int cap,
               const void* h, int ldh, const void* w, int ldw, const void* C, const int32_t* arg, const void* g,
               int ldg, void* gh, void* gw, void* gC, hipStream_t st) {
  CfArgs<T> A;
  int rc = setup<T>(A, aggr, n, F, row_ptr, src, tr, cap, h, ldh, w, ldw, C, arg);
  if (rc) return rc;
  if ((n > 0 && !g) || (cap > 0 && (!gw || !gC))) return kBadArgument;
  if (gh && !tr && cap > 0) return kUnsupported;  // the source pass needs the reverse of every edge
  A.g = (const T*)g; A.ldg = ldg ? ldg : F;
  if (A.ldg < F) return kBadArgument;
  A.gh = (T*)gh; A.gw = (T*)gw; A.gC = (T*)gC;
  int V = pick_vec<T>(F, {{h, A.ldh}, {w, A.ldw}, {g, A.ldg}, {gh, F}, {gw, F}});
  if (!aligned<int32_t>(arg, F, V)) V = 1;
  if (n == 0 && cap > 0) {  // no row, so no destination pass: every slot is padding
    if (hipMemsetAsync(gw, 0, (size_t)cap * F * sizeof(T), st) != hipSuccess ||
        hipMemsetAsync(gC, 0, (size_t)cap * sizeof(T), st) != hipSuccess)
      return kLaunchFailed;
  }
  rc = launch<T, KDst>(V, n, true, A, st);
  if (rc || !gh) return rc;
  return launch<T, KSrc>(V, n, false, A, st);
}

template <typename T>
static int bwd2(int aggr, int n, int F, const int32_t* row_ptr, const int32_t* src, const int32_t* tr, int cap,
                const void* h, int ldh, const void* w, int ldw, const void* C, const int32_t* arg, const void* g,
                int ldg, const void* ggh, const void* ggw, const void* ggC, void* dg, void* dh, void* dw, void* dC,
                hipStream_t st) {
  CfArgs<T> A;
  int rc = setup<T>(A, aggr, n, F, row_ptr, src, tr, cap, h, ldh, w, ldw, C, arg);
  if (rc) return rc;
  if (n > 0 && !g) return kBadArgument;
  if (dh && !tr && cap > 0) return kUnsupported;
  A.g = (const T*)g; A.ldg = ldg ? ldg : F;
  if (A.ldg < F) return kBadArgument;
  A.ggh = (const T*)ggh; A.ggw = (const T*)ggw; A.ggC = (const T*)ggC;
  A.dg = (T*)dg; A.dh = (T*)dh; A.dw = (T*)dw; A.dC = (T*)dC;
  int V = pick_vec<T>(F, {{h, A.ldh}, {w, A.ldw}, {g, A.ldg}, {ggh, F}, {ggw, F}, {dg, F}, {dh, F}, {dw, F}});
  if (!aligned<int32_t>(arg, F, V)) V = 1;
  if (dg || dw || dC) {
    rc = launch<T, K2Dst>(V, n, false, A, st);
    if (rc) return rc;
  }
  return dh ? launch<T, K2Src>(V, n, false, A, st) : kOk;
}

}  // namespace cf
}  // namespace tmd

using namespace tmd;

extern "C" int tmdnet_cfconv_fwd(int dtype, int aggr, int n_nodes, int filters, const int32_t* row_ptr,
                                 const int32_t* src, int max_pairs, const void* h, int ld_h, const void* w,
                                 int ld_w, const void* cutoff, void* out, int32_t* arg, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDNET_F32) return cf::fwd<float>(aggr, n_nodes, filters, row_ptr, src, max_pairs, h, ld_h, w, ld_w, cutoff, out, arg, st);
  if (dtype == TMDNET_F64) return cf::fwd<double>(aggr, n_nodes, filters, row_ptr, src, max_pairs, h, ld_h, w, ld_w, cutoff, out, arg, st);
  return kUnsupported;
}

extern "C" int tmdnet_cfconv_bwd(int dtype, int aggr, int n_nodes, int filters, const int32_t* row_ptr,
                                 const int32_t* src, const int32_t* transpose, int max_pairs, const void* h,
                                 int ld_h, const void* w, int ld_w, const void* cutoff, const int32_t* arg,
                                 const void* grad_out, int ld_grad_out, void* gh, void* gw, void* gcut,
                                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
#define TMD_CF(T)                                                                                              \
  return cf::bwd<T>(aggr, n_nodes, filters, row_ptr, src, transpose, max_pairs, h, ld_h, w, ld_w, cutoff, arg, \
                    grad_out, ld_grad_out, gh, gw, gcut, st)
  if (dtype == TMDNET_F32) TMD_CF(float);
  if (dtype == TMDNET_F64) TMD_CF(double);
#undef TMD_CF
  return kUnsupported;
}

extern "C" int tmdnet_cfconv_bwd2(int dtype, int aggr, int n_nodes, int filters, const int32_t* row_ptr,
                                  const int32_t* src, const int32_t* transpose, int max_pairs, const void* h,
                                  int ld_h, const void* w, int ld_w, const void* cutoff, const int32_t* arg,
                                  const void* grad_out, int ld_grad_out, const void* gg_h, const void* gg_w,
                                  const void* gg_cut, void* d_grad_out, void* d_h, void* d_w, void* d_cut,
                                  void* stream) {
  hipStream_t st = (hipStream_t)stream;
#define TMD_CF(T)                                                                                               \
  return cf::bwd2<T>(aggr, n_nodes, filters, row_ptr, src, transpose, max_pairs, h, ld_h, w, ld_w, cutoff, arg, \
                     grad_out, ld_grad_out, gg_h, gg_w, gg_cut, d_grad_out, d_h, d_w, d_cut, st)
  if (dtype == TMDNET_F32) TMD_CF(float);
  if (dtype == TMDNET_F64) TMD_CF(double);
#undef TMD_CF
  return kUnsupported;
}
