// Pair-potential priors (reference priors/zbl.py:46-63, d2.py:163-193, coulomb.py:38-50) over the
// symmetric destination-grouped CSR list of tmdnet_nl_build:
//   E_mol = 1/2 sum_{edges e of mol} phi_kind(r_e; a_src, b_src, a_dst, b_dst)
// (every pair appears in both directions, hence the 1/2).  The per-atom parameters a, b are gathered by
// the caller once per call; the unit constants c0..c3 are formed in double on the host, so no raw SI
// constant (1e-28 ...) ever meets float arithmetic here.
//
//   fwd:  e_atom[i] = 1/2 sum_row phi,  dphi[e] = 1/2 phi'(r_e)        (the backward reuses dphi)
//   bwd:  g_r[e] = gy[batch[dst(e)]] * dphi[e]; slots no row references (static-capacity padding) = 0
//   bwd2: d_r[e] = gg[e] * gy[mol] * 1/2 phi''(r_e),  t[i] = sum_row gg * dphi  (-> d_gy by the atom sum)
//
// Layout: 16 lanes per CSR row, four rows per wave64.  QM9 / SPICE rows are 20-60 edges: with 16 lanes a
// row of 40 takes 3 steps at 83 % lane use (a whole wave per row would idle 38 % of its lanes in one step,
// 8 lanes would serialise 5 transcendental-heavy steps and leave a 640-atom batch with 80 waves for 256
// CUs).  A row of any length loops in steps of 16.  The row sum is a 4-step xor shuffle inside the group:
// no atomics, a fixed summation order.  Every index read from the list is range-checked (a
// capacity-truncated list has row_ptr entries past n_slots), so an overflowing build cannot fault here.
#include "common.h"
#include "tmdnet.h"

namespace tmd {
namespace pp {

constexpr int kGroup = 16;
constexpr int kBlock = 256;

template <typename T> struct Consts { T c0, c1, c2, c3; };
template <typename T> struct Phi { T p, d1, d2; };  // phi, phi', phi'' (with respect to r)

template <typename T> __device__ __forceinline__ T sum16(T v) {
#pragma unroll
  for (int o = kGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kGroup);
  return v;
}

// ZBL: c0 = k_e, c1 = k_a, c2 = cutoff, c3 = pi / cutoff; a = Z, b = Z^0.23.
//   phi = k_e Z_i Z_j f(x) C(r) / r,  x = r k_a (b_i + b_j),  C = (cos(pi r / cutoff) + 1) / 2 for r < cutoff
template <typename T, int ORDER>
__device__ __forceinline__ Phi<T> phi_zbl(T r, T ai, T aj, T bi, T bj, const Consts<T>& c) {
  const T K = c.c0 * ai * aj, s = c.c1 * (bi + bj), x = s * r;
  const T e1 = T(0.1818) * exp(T(-3.2) * x), e2 = T(0.5099) * exp(T(-0.9423) * x),
          e3 = T(0.2802) * exp(T(-0.4029) * x), e4 = T(0.02817) * exp(T(-0.2016) * x);
  const bool in = r < c.c2;
  const T cs = cos(c.c3 * r), sn = sin(c.c3 * r);
  const T f = e1 + e2 + e3 + e4;
  const T C = in ? T(0.5) * (cs + T(1)) : T(0);
  const T ir = T(1) / r;
  const T u = f * C;
  Phi<T> o{K * u * ir, T(0), T(0)};
  if (ORDER >= 1) {
    const T f1 = -s * (T(3.2) * e1 + T(0.9423) * e2 + T(0.4029) * e3 + T(0.2016) * e4);
    const T C1 = in ? T(-0.5) * c.c3 * sn : T(0);
    const T u1 = f1 * C + f * C1;
    o.d1 = K * (u1 - u * ir) * ir;
    if (ORDER >= 2) {
      const T f2 = s * s * (T(3.2 * 3.2) * e1 + T(0.9423 * 0.9423) * e2 + T(0.4029 * 0.4029) * e3 +
                            T(0.2016 * 0.2016) * e4);
      const T C2 = in ? T(-0.5) * c.c3 * c.c3 * cs : T(0);
      const T u2 = f2 * C + T(2) * f1 * C1 + f * C2;
      o.d2 = K * (u2 - T(2) * u1 * ir + T(2) * u * ir * ir) * ir;
    }
  }
  return o;
}

// D2: c0 = k_e, c1 = r -> nm, c2 = damping steepness d (20); a = sqrt(C6), b = R_r.
//   phi = -k_e a_i a_j R^-6 / (1 + exp(-d (R / (b_i + b_j) - 1))),  R = c1 r
template <typename T, int ORDER>
__device__ __forceinline__ Phi<T> phi_d2(T r, T ai, T aj, T bi, T bj, const Consts<T>& c) {
  const T K = -c.c0 * ai * aj, R = c.c1 * r, Rr = bi + bj;
  const T sg = T(1) / (T(1) + exp(-c.c2 * (R / Rr - T(1))));
  const T iR = T(1) / R, iR2 = iR * iR, P = iR2 * iR2 * iR2;
  Phi<T> o{K * P * sg, T(0), T(0)};
  if (ORDER >= 1) {
    const T k = c.c2 / Rr, w = sg * (T(1) - sg);
    const T P1 = T(-6) * P * iR, S1 = w * k;
    o.d1 = K * c.c1 * (P1 * sg + P * S1);
    if (ORDER >= 2) {
      const T P2 = T(42) * P * iR2, S2 = w * (T(1) - T(2) * sg) * k * k;
      o.d2 = K * c.c1 * c.c1 * (P2 * sg + T(2) * P1 * S1 + P * S2);
    }
  }
  return o;
}

// Coulomb: c0 = k_e, c1 = r -> nm, c2 = alpha' (per nm); a = partial charge, b unused.
//   phi = k_e erf(alpha' R) q_i q_j / R,  R = c1 r
template <typename T, int ORDER>
__device__ __forceinline__ Phi<T> phi_coulomb(T r, T ai, T aj, const Consts<T>& c) {
  const T K = c.c0 * ai * aj, R = c.c1 * r, t = c.c2 * R;
  const T E = erf(t), iR = T(1) / R;
  Phi<T> o{K * E * iR, T(0), T(0)};
  if (ORDER >= 1) {
    const T E1 = c.c2 * T(1.1283791670955125739) * exp(-t * t);  // 2 / sqrt(pi)
    o.d1 = K * c.c1 * (E1 - E * iR) * iR;
    if (ORDER >= 2) {
      const T E2 = T(-2) * c.c2 * c.c2 * R * E1;
      o.d2 = K * c.c1 * c.c1 * (E2 - T(2) * E1 * iR + T(2) * E * iR * iR) * iR;
    }
  }
  return o;
}

template <typename T, int KIND, int ORDER>
__device__ __forceinline__ Phi<T> phi(T r, T ai, T aj, T bi, T bj, const Consts<T>& c) {
  if (KIND == TMDNET_PRIOR_ZBL) return phi_zbl<T, ORDER>(r, ai, aj, bi, bj, c);
  if (KIND == TMDNET_PRIOR_D2) return phi_d2<T, ORDER>(r, ai, aj, bi, bj, c);
  return phi_coulomb<T, ORDER>(r, ai, aj, c);
}

// The 16-lane group's row and its slot range, clamped to the slots that exist.
struct Row {
  long long gid;
  int row, g, e0, e1;
  bool on;
};

__device__ __forceinline__ Row my_row(int n, int n_slots, const int32_t* __restrict__ row_ptr) {
  Row w;
  w.gid = (long long)blockIdx.x * kBlock + threadIdx.x;
  w.g = threadIdx.x & (kGroup - 1);
  const long long row = w.gid / kGroup;
  w.on = row < n;
  w.row = w.on ? (int)row : 0;
  w.e0 = w.on ? min(max(row_ptr[w.row], 0), n_slots) : 0;
  w.e1 = w.on ? min(max(row_ptr[w.row + 1], 0), n_slots) : 0;
  return w;
}

// zero the slots past the last row (grid-stride; the grid is sized by the rows, not by the slots)
template <typename T>
__device__ __forceinline__ void zero_tail(int n, int n_slots, const int32_t* __restrict__ row_ptr, long long gid,
                                          T* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long e = min(max(row_ptr[n], 0), n_slots) + gid; e < n_slots; e += stride) out[e] = T(0);
}

template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void k_fwd(int n, int n_slots, const int32_t* __restrict__ row_ptr,
                                                const int32_t* __restrict__ src, const T* __restrict__ r,
                                                const T* __restrict__ a, const T* __restrict__ b, Consts<T> c,
                                                T* __restrict__ e_atom, T* __restrict__ dphi) {
  const Row w = my_row(n, n_slots, row_ptr);
  const T ai = w.on ? a[w.row] : T(0), bi = (w.on && b) ? b[w.row] : T(0);
  T acc = T(0);
  for (int e = w.e0 + w.g; e < w.e1; e += kGroup) {
    const int j = src[e];
    T d = T(0);
    if ((unsigned)j < (unsigned)n) {
      const Phi<T> o = phi<T, KIND, 1>(r[e], ai, a[j], bi, b ? b[j] : T(0), c);
      acc += o.p;
      d = T(0.5) * o.d1;
    }
    dphi[e] = d;
  }
  acc = sum16(acc);
  if (w.on && w.g == 0) e_atom[w.row] = T(0.5) * acc;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_bwd(int n, int n_slots, int n_mol, const int32_t* __restrict__ row_ptr,
                                                const int64_t* __restrict__ batch, const T* __restrict__ gy,
                                                const T* __restrict__ dphi, T* __restrict__ g_r) {
  const Row w = my_row(n, n_slots, row_ptr);
  const int64_t m = w.on ? batch[w.row] : -1;
  const T g = (m >= 0 && m < n_mol) ? gy[m] : T(0);
  for (int e = w.e0 + w.g; e < w.e1; e += kGroup) g_r[e] = g * dphi[e];
  zero_tail(n, n_slots, row_ptr, w.gid, g_r);
}

template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void k_bwd2(int n, int n_slots, int n_mol, const int32_t* __restrict__ row_ptr,
                                                 const int32_t* __restrict__ src, const int64_t* __restrict__ batch,
                                                 const T* __restrict__ r, const T* __restrict__ a,
                                                 const T* __restrict__ b, Consts<T> c, const T* __restrict__ gy,
                                                 const T* __restrict__ gg, const T* __restrict__ dphi,
                                                 T* __restrict__ d_r, T* __restrict__ t) {
  const Row w = my_row(n, n_slots, row_ptr);
  const int64_t m = w.on ? batch[w.row] : -1;
  const T g = (m >= 0 && m < n_mol) ? gy[m] : T(0);
  const T ai = w.on ? a[w.row] : T(0), bi = (w.on && b) ? b[w.row] : T(0);
  T acc = T(0);
  for (int e = w.e0 + w.g; e < w.e1; e += kGroup) {
    const int j = src[e];
    T d = T(0);
    if ((unsigned)j < (unsigned)n) {
      const Phi<T> o = phi<T, KIND, 2>(r[e], ai, a[j], bi, b ? b[j] : T(0), c);
      const T q = gg[e];
      d = q * g * T(0.5) * o.d2;
      acc += q * dphi[e];
    }
    d_r[e] = d;
  }
  acc = sum16(acc);
  if (w.on && w.g == 0) t[w.row] = acc;
  zero_tail(n, n_slots, row_ptr, w.gid, d_r);
}

static bool kind_ok(int kind) {
  return kind == TMDNET_PRIOR_ZBL || kind == TMDNET_PRIOR_D2 || kind == TMDNET_PRIOR_COULOMB;
}

// one group of 16 lanes per row; at least one block so the tail of an atom-less call is still zeroed
static dim3 row_grid(int n) { return dim3((unsigned)(((long long)max(n, 1) * kGroup + kBlock - 1) / kBlock)); }

template <typename T>
static Consts<T> consts(double c0, double c1, double c2, double c3) {
  return Consts<T>{(T)c0, (T)c1, (T)c2, (T)c3};
}

template <typename T>
static void launch_fwd(int kind, int n, int n_slots, const int32_t* row_ptr, const int32_t* src, const void* r,
                       const void* a, const void* b, Consts<T> c, void* e_atom, void* dphi, hipStream_t st) {
#define TMD_PP_FWD(K)                                                                                         \
  hipLaunchKernelGGL((k_fwd<T, K>), row_grid(n), dim3(kBlock), 0, st, n, n_slots, row_ptr, src, (const T*)r,  \
                     (const T*)a, (const T*)b, c, (T*)e_atom, (T*)dphi)
  if (kind == TMDNET_PRIOR_ZBL) TMD_PP_FWD(TMDNET_PRIOR_ZBL);
  else if (kind == TMDNET_PRIOR_D2) TMD_PP_FWD(TMDNET_PRIOR_D2);
  else TMD_PP_FWD(TMDNET_PRIOR_COULOMB);
#undef TMD_PP_FWD
}

template <typename T>
static void launch_bwd2(int kind, int n, int n_slots, int n_mol, const int32_t* row_ptr, const int32_t* src,
                        const int64_t* batch, const void* r, const void* a, const void* b, Consts<T> c,
                        const void* gy, const void* gg, const void* dphi, void* d_r, void* t, hipStream_t st) {
#define TMD_PP_BWD2(K)                                                                                         \
  hipLaunchKernelGGL((k_bwd2<T, K>), row_grid(n), dim3(kBlock), 0, st, n, n_slots, n_mol, row_ptr, src, batch, \
                     (const T*)r, (const T*)a, (const T*)b, c, (const T*)gy, (const T*)gg, (const T*)dphi,     \
                     (T*)d_r, (T*)t)
  if (kind == TMDNET_PRIOR_ZBL) TMD_PP_BWD2(TMDNET_PRIOR_ZBL);
  else if (kind == TMDNET_PRIOR_D2) TMD_PP_BWD2(TMDNET_PRIOR_D2);
  else TMD_PP_BWD2(TMDNET_PRIOR_COULOMB);
#undef TMD_PP_BWD2
}

}  // namespace pp
}  // namespace tmd

using namespace tmd;

extern "C" int tmdnet_pair_prior_fwd(int dtype, int kind, int n_atoms, int n_slots, const int32_t* row_ptr,
                                     const int32_t* src, const void* r, const void* a, const void* b, double c0,
                                     double c1, double c2, double c3, void* e_atom, void* dphi, void* stream) {
  if (!pp::kind_ok(kind) || n_atoms <= 0 || n_slots < 0 || !row_ptr || !a || !e_atom) return kBadArgument;
  if (kind != TMDNET_PRIOR_COULOMB && !b) return kBadArgument;
  if (n_slots > 0 && (!src || !r || !dphi)) return kBadArgument;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDNET_F32)
    pp::launch_fwd<float>(kind, n_atoms, n_slots, row_ptr, src, r, a, b, pp::consts<float>(c0, c1, c2, c3), e_atom,
                          dphi, st);
  else if (dtype == TMDNET_F64)
    pp::launch_fwd<double>(kind, n_atoms, n_slots, row_ptr, src, r, a, b, pp::consts<double>(c0, c1, c2, c3),
                           e_atom, dphi, st);
  else
    return kUnsupported;
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

extern "C" int tmdnet_pair_prior_bwd(int dtype, int n_atoms, int n_slots, int n_mol, const int32_t* row_ptr,
                                     const int64_t* batch, const void* gy, const void* dphi, void* g_r,
                                     void* stream) {
  if (n_atoms <= 0 || n_slots < 0 || n_mol <= 0 || !row_ptr || !batch || !gy) return kBadArgument;
  if (dtype != TMDNET_F32 && dtype != TMDNET_F64) return kUnsupported;
  if (n_slots == 0) return kOk;
  if (!dphi || !g_r) return kBadArgument;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDNET_F32)
    hipLaunchKernelGGL(pp::k_bwd<float>, pp::row_grid(n_atoms), dim3(pp::kBlock), 0, st, n_atoms, n_slots, n_mol,
                       row_ptr, batch, (const float*)gy, (const float*)dphi, (float*)g_r);
  else
    hipLaunchKernelGGL(pp::k_bwd<double>, pp::row_grid(n_atoms), dim3(pp::kBlock), 0, st, n_atoms, n_slots, n_mol,
                       row_ptr, batch, (const double*)gy, (const double*)dphi, (double*)g_r);
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

extern "C" int tmdnet_pair_prior_bwd2(int dtype, int kind, int n_atoms, int n_slots, int n_mol,
                                      const int32_t* row_ptr, const int32_t* src, const int64_t* batch,
                                      const void* r, const void* a, const void* b, double c0, double c1, double c2,
                                      double c3, const void* gy, const void* gg, const void* dphi, void* d_r,
                                      void* t, void* stream) {
  if (!pp::kind_ok(kind) || n_atoms <= 0 || n_slots < 0 || n_mol <= 0 || !row_ptr || !batch || !a || !gy || !t)
    return kBadArgument;
  if (kind != TMDNET_PRIOR_COULOMB && !b) return kBadArgument;
  if (n_slots > 0 && (!src || !r || !gg || !dphi || !d_r)) return kBadArgument;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDNET_F32)
    pp::launch_bwd2<float>(kind, n_atoms, n_slots, n_mol, row_ptr, src, batch, r, a, b,
                           pp::consts<float>(c0, c1, c2, c3), gy, gg, dphi, d_r, t, st);
  else if (dtype == TMDNET_F64)
    pp::launch_bwd2<double>(kind, n_atoms, n_slots, n_mol, row_ptr, src, batch, r, a, b,
                            pp::consts<double>(c0, c1, c2, c3), gy, gg, dphi, d_r, t, st);
  else
    return kUnsupported;
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}
