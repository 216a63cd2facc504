// Continuous-filter convolution with the filter network inside the edge kernel (the graph network's
// optimize() path; reference optimize.py / NNPOps CFConv).  For edge e of CSR row t (source s, distance r,
// cutoff C):
//   a_e = act(W1 f(r) + b1),  w_e = W2 a_e + b2          (registers only: no E x F rows in memory)
//   out[t] = scale_t sum_{e in row t} h[s] * w_e * C_e
// and the backward for g = grad_out, which needs d w_e / d r: the kernel carries the TANGENT of the filter
// network beside its value (u = W1 f'(r), da = act'(z) u, dw = W2 da), so both layers use the weights in
// the forward orientation and one image serves forward and backward:
//   gcut[e]  = scale_t sum_f g[t][f] h[s][f] w_e[f]
//   gdist[e] = scale_t C_e sum_f g[t][f] h[s][f] dw_e[f]
//   gh[t]    = sum_{e in row t} scale_s g[s] * w_e * C_e
// PRECONDITION of gh: the list is pair symmetric (every edge has its reverse, with the same r and C), so
// the edge leaving t towards s carries the w_e and C_e of the row's own edge (s -> t) and the source pass
// runs over t's own row, sharing the filter evaluation with the destination pass.  For mean the reverse
// edge's scale is the source atom's, 1 / max(deg_s, 1).
//
// Arithmetic: the bf16 MFMA (v_mfma_f32_16x16x32_bf16) on the exact three-piece split of xsplit.h, six
// piece products per operand pair, fp32 accumulation (~2^-24 relative: the project's fp32 bar).  The
// three-piece bf16 split is chosen over the two-piece fp16 split of et_fused.hip because layer 2's operand
// is an activation: ssp and silu are unbounded above, so fp16 pieces would need an exact per-edge
// power-of-two scale carried through the tangent as well; bf16 pieces have fp32's exponent range and need
// none.  The price is 6 instead of 3 MFMAs per product.
//
// Orientation: weights are the A operand (rows = output channels), a tile of 16 edges the B operand
// (columns = edges).  A lane's accumulator holds 4 consecutive output rows of one edge; its B fragment
// holds 8 consecutive k of one edge.  The image stores W1's rows PERMUTED so that two layer-1 accumulator
// blocks of a lane are, in order, the 8 k values of its layer-2 B fragment: image row
// p = 32 s + 16 b + 4 g + i holds the true row 32 s + 8 g + 4 b + i (s the layer-2 k step, g the lane
// group, b the block of the pair, i the register).  The layer-1 result never moves between lanes.
//
// Image of one layer (tmdnet_cfconv_fused_image), bytes, Fp = F rounded up to 32, Rp = R rounded up to 32:
//   [3 pieces][Fp/16 row blocks][Rp/32 k steps][64 lanes][8 bf16]   W1 (permuted rows; zero padding)
//   [3 pieces][F /16 row blocks][Fp/32 k steps][64 lanes][8 bf16]   W2
//   [Fp] fp32 b1 (permuted), [F] fp32 b2
// i.e. every MFMA A fragment is one conflict-free 16-byte LDS read per lane.  At F = 128, R <= 64 the image
// is 145 KB of the 160 KiB LDS: one workgroup per CU, the image read once per launch; waves take nodes from
// an LDS counter over the workgroup's contiguous node range.  Padded layer-1 rows give act(0) = 0 (ssp and
// silu both), padded k columns are zero in the image.
//
// Deterministic: one writer per output element, fixed summation order, no atomics on outputs.
#include "common.h"
#include "tmdnet.h"
#include "xsplit.h"

namespace tmd {
namespace cff {

using xs::bf8;
using xs::f4v;

constexpr int kMaxLayers = 16;  // layers per image-build launch
constexpr int kNW = 4;          // waves per workgroup
constexpr int kCopyU = 12;      // image copy: loads in flight per thread

__host__ __device__ constexpr int up32(int x) { return (x + 31) & ~31; }
__host__ __device__ constexpr size_t a1_bytes(int F, int R) { return (size_t)6 * up32(F) * up32(R); }
__host__ __device__ constexpr size_t a2_bytes(int F) { return (size_t)6 * F * up32(F); }
__host__ __device__ constexpr size_t image_bytes(int F, int R) {
  return a1_bytes(F, R) + a2_bytes(F) + 4 * (size_t)up32(F) + 4 * (size_t)F;
}

static bool in_envelope(int F, int R) { return F >= 16 && F <= 128 && F % 16 == 0 && R >= 1 && R <= 64; }

// ------------------------------------------------------------------ image build
struct ImgArgs {
  int F, R;
  const float* w1[kMaxLayers];
  const float* b1[kMaxLayers];
  const float* w2[kMaxLayers];
  const float* b2[kMaxLayers];
  unsigned char* img;
};

__device__ __forceinline__ int perm_row(int p) {  // image row of layer 1 -> true row
  return (p & ~31) + 8 * ((p >> 2) & 3) + 4 * ((p >> 4) & 1) + (p & 3);
}

// one thread per A-fragment slot (8 k values of one row): blockIdx.y = layer
__global__ __launch_bounds__(256) void k_image(ImgArgs P) {
  const int L = blockIdx.y, F = P.F, R = P.R, Fp = up32(F), Rp = up32(R);
  const float* W1 = P.w1[L];
  const float* W2 = P.w2[L];
  unsigned char* img = P.img + (size_t)L * image_bytes(F, R);
  const int n1 = Fp * Rp / 8, n2 = F * Fp / 8;
  const int nth = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = tid; i < n1 + n2; i += nth) {
    const bool first = i < n1;
    const int q = first ? i : i - n1;
    const int nks = (first ? Rp : Fp) / 32, nmb = (first ? Fp : F) / 16;
    const int lane = q & 63, ks = (q >> 6) % nks, mb = (q >> 6) / nks;
    const int p = 16 * mb + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
    const int row = first ? perm_row(p) : p;
    const int K = first ? R : F;
    const float* W = first ? W1 : W2;
    unsigned pc[3][4] = {};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (row < F && k0 + j < K) ? W[(size_t)row * K + k0 + j] : 0.0f;
      unsigned h, m, l;
      xs::split3(x, h, m, l);
      const int sh = (j & 1) ? 0 : 16;  // element 2p in the low half of register p
      pc[0][j >> 1] |= h >> sh;
      pc[1][j >> 1] |= m >> sh;
      pc[2][j >> 1] |= l >> sh;
    }
    unsigned char* base = img + (first ? 0 : a1_bytes(F, R));
    const size_t piece = (size_t)nmb * nks * 64 * 16;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<uint4*>(base + c * piece + (size_t)q * 16) = make_uint4(pc[c][0], pc[c][1], pc[c][2], pc[c][3]);
  }
  float* bb = reinterpret_cast<float*>(img + a1_bytes(F, R) + a2_bytes(F));
  for (int i = tid; i < Fp + F; i += nth) {
    float v = 0.0f;
    if (i < Fp) {
      const int row = perm_row(i);
      if (row < F && P.b1[L]) v = P.b1[L][row];
    } else if (P.b2[L]) {
      v = P.b2[L][i - Fp];
    }
    bb[i] = v;
  }
}

// ------------------------------------------------------------------ edge kernels
struct Args {
  int n, F, R, cap, aggr, act, rbf;
  const int32_t* row_ptr;
  const int32_t* src;
  const float* h; int ldh;
  const float* r;
  const float* C;
  const float* mu;
  const float* beta;
  float cl, cu, alpha;
  const unsigned char* img;
  float* out;
  const float* g; int ldg;
  float* gh; float* gcut; float* gdist;
};

__device__ __forceinline__ float pi_f() { return 3.14159265358979323846f; }

// CosineCutoff(0, cu) and its derivative: the factor of the expnorm basis (edge_geom.hip cosine_cutoff)
__device__ __forceinline__ void cos_cut0(float r, float cu, float& c, float& dc) {
  const bool in = r < cu;
  const float arg = r * pi_f() / cu;
  c = in ? 0.5f * (cosf(arg) + 1.0f) : 0.0f;
  dc = in ? -0.5f * sinf(arg) * pi_f() / cu : 0.0f;
}

__device__ __forceinline__ int next_item(int* counter) {
  int it = 0;
  if (lane_id() == 0) it = atomicAdd(counter, 1);
  return __builtin_amdgcn_readfirstlane(__shfl(it, 0));
}

// act(x) and act'(x) for the two supported codes on the hardware exp2 / log2 / rcp (<= 1 ulp each; the
// argument scaling of __expf costs |x| 2^-24 relative, the sum 1 + e one rounding: ~1e-7 absolute on values of
// order one).  One exponential serves the sigmoid and the softplus.
__device__ __forceinline__ void act_fast(float x, int code, float& s, float& d) {
  const float e = __expf(-fabsf(x));
  const float q = __builtin_amdgcn_rcpf(1.0f + e);
  const float sg = x >= 0.0f ? q : e * q;  // sigmoid(x)
  if (code == TMDNET_ACT_SILU) {
    s = x * sg;
    d = sg * (1.0f + x * (1.0f - sg));
  } else {  // ShiftedSoftplus: softplus(x) - log 2 (the fp32-rounded shift of common.h ActF)
    s = fmaxf(x, 0.0f) + __logf(1.0f + e) - 0.693147182464599609375f;
    d = sg;
  }
}

// two independent accumulator chains interleaved (a dependent MFMA waits out the previous one's passes)
__device__ __forceinline__ void mfma_x3_dual(const bf8 (&wa)[3], const bf8 (&ba)[3], f4v& ca, const bf8 (&wb)[3],
                                             const bf8 (&bb)[3], f4v& cb) {
#define TMD_CFF_STEP(i, j)                                                           \
  ca = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i], ba[j], ca, 0, 0, 0);         \
  cb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[i], bb[j], cb, 0, 0, 0)
  TMD_CFF_STEP(2, 0); TMD_CFF_STEP(1, 1); TMD_CFF_STEP(0, 2); TMD_CFF_STEP(1, 0); TMD_CFF_STEP(0, 1); TMD_CFF_STEP(0, 0);
#undef TMD_CFF_STEP
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ void split_pair(const f4v& a, const f4v& b, bf8 (&f)[3]) {
  xs::split8(make_float4(a[0], a[1], a[2], a[3]), make_float4(b[0], b[1], b[2], b[3]), f);
}

// sum over the 16 edge columns of a tile (the lanes that share lane >> 4)
__device__ __forceinline__ float col_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// NK1 = Rp / 32 layer-1 k steps, NK2 = Fp / 32 layer-2 k steps; BWD: the tangent stream and the gradients
template <int NK1, int NK2, bool BWD>
__global__ __launch_bounds__(kNW * 64, 1) void k_edge(Args P) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[image_bytes(32 * NK2, 32 * NK1) + 16];
  constexpr int MB1 = 2 * NK2;
  const int F = P.F, MB2 = F / 16;
  const size_t nimg = image_bytes(F, P.R);
  int* s_next = reinterpret_cast<int*>(lds + nimg);
  {  // the image: kCopyU 16-byte loads in flight per thread before their LDS stores (a load-store loop of
     // one is 36 serial round trips to L2 at F = 128), then a tail of less than one batch
    const uint4* gi = reinterpret_cast<const uint4*>(P.img);
    uint4* li = reinterpret_cast<uint4*>(lds);
    constexpr int nt = kNW * 64;
    const int n16 = (int)(nimg / 16);
    int i0 = threadIdx.x;
    for (; i0 + (kCopyU - 1) * nt < n16; i0 += kCopyU * nt) {
      uint4 v[kCopyU];
#pragma unroll
      for (int u = 0; u < kCopyU; ++u) v[u] = gi[i0 + u * nt];
#pragma unroll
      for (int u = 0; u < kCopyU; ++u) li[i0 + u * nt] = v[u];
    }
    for (; i0 < n16; i0 += nt) li[i0] = gi[i0];
  }
  if (threadIdx.x == 0) *s_next = 0;
  if constexpr (BWD) {  // the padding slots beyond the last row read as zero
    const int e0 = min(P.row_ptr[P.n], P.cap);
    for (long long i = e0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < P.cap;
         i += (long long)gridDim.x * blockDim.x) {
      P.gcut[i] = 0.0f;
      P.gdist[i] = 0.0f;
    }
  }
  __syncthreads();

  const uint4* A1 = reinterpret_cast<const uint4*>(lds);
  const uint4* A2 = reinterpret_cast<const uint4*>(lds + a1_bytes(F, P.R));
  const float* s_b1 = reinterpret_cast<const float*>(lds + a1_bytes(F, P.R) + a2_bytes(F));
  const float* s_b2 = s_b1 + 32 * NK2;
  const int piece1 = MB1 * NK1 * 64, piece2 = MB2 * NK2 * 64;  // in 16-byte fragments

  const int lane = lane_id(), c = lane & 15, grp = lane >> 4;
  // this lane's basis centres: k = 32 ks + 8 grp + j, the same for every tile
  float mu[NK1][8], be[NK1][8];
#pragma unroll
  for (int ks = 0; ks < NK1; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * ks + 8 * grp + j;
      mu[ks][j] = k < P.R ? P.mu[k] : 0.0f;
      be[ks][j] = k < P.R ? P.beta[k] : 0.0f;
    }

  const int x0 = (int)((long long)P.n * blockIdx.x / gridDim.x), x1 = (int)((long long)P.n * (blockIdx.x + 1) / gridDim.x);
  const bool mean = P.aggr == TMDNET_AGGR_MEAN;

  for (;;) {
    const int t = x0 + next_item(s_next);
    if (t >= x1) break;
    const int b = min(P.row_ptr[t], P.cap), e = min(P.row_ptr[t + 1], P.cap);
    const float scale_t = mean ? 1.0f / (float)max(e - b, 1) : 1.0f;
    f4v o[MB1];  // forward: out[t]; backward: gh[t]
#pragma unroll
    for (int mb = 0; mb < MB1; ++mb) o[mb] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

    for (int base = b; base < e; base += 16) {
      const int ei = base + c;
      int s = ei < e ? P.src[ei] : -1;
      if ((unsigned)s >= (unsigned)P.n) s = -1;
      const bool live = s >= 0;
      const float r = live ? P.r[ei] : 1.0f;
      float Ce = live ? P.C[ei] : 0.0f;
      float sc_s = 1.0f;
      if (BWD && mean && live) sc_s = 1.0f / (float)max(min(P.row_ptr[s + 1], P.cap) - min(P.row_ptr[s], P.cap), 1);
      const size_t so = (size_t)(live ? s : t);

      // ---- basis fragments (and their r derivative)
      bf8 fb[NK1][3], fd[BWD ? NK1 : 1][3];
      {
        float c0 = 1.0f, dc0 = 0.0f, u = 0.0f, du = 0.0f;
        const bool en = P.rbf == TMDNET_RBF_EXPNORM;
        if (en) {
          cos_cut0(r, P.cu, c0, dc0);
          u = __expf(P.alpha * (P.cl - r));
          du = -P.alpha * u;
        }
#pragma unroll
        for (int ks = 0; ks < NK1; ++ks) {
          float f[8], d[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool on = 32 * ks + 8 * grp + j < P.R;
            float v, dv;
            if (en) {
              const float z = u - mu[ks][j];
              const float gk = __expf(-be[ks][j] * z * z);
              v = c0 * gk;
              dv = dc0 * gk + c0 * (gk * (-2.0f * be[ks][j] * z * du));
            } else {
              const float z = r - mu[ks][j];
              v = __expf(be[ks][j] * z * z);
              dv = v * 2.0f * be[ks][j] * z;
            }
            f[j] = on ? v : 0.0f;
            d[j] = on ? dv : 0.0f;
          }
          xs::split8(make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]), fb[ks]);
          if constexpr (BWD) xs::split8(make_float4(d[0], d[1], d[2], d[3]), make_float4(d[4], d[5], d[6], d[7]), fd[ks]);
        }
      }

      // ---- layer 1: z = W1 f + b1 (u1 = W1 f'), rows in the permuted order
      f4v z[MB1], u1[BWD ? MB1 : 1];
      auto frag1 = [&](int mb, int ks, bf8 (&w)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p) w[p] = __builtin_bit_cast(bf8, A1[p * piece1 + (mb * NK1 + ks) * 64 + lane]);
      };
      auto bias4 = [&](const float* b) {
        const float4 bi = ld4(b);
        return f4v{bi.x, bi.y, bi.z, bi.w};
      };
      if constexpr (BWD) {
#pragma unroll
        for (int mb = 0; mb < MB1; ++mb) {
          f4v acc = bias4(s_b1 + 16 * mb + 4 * grp), dac = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < NK1; ++ks) {
            bf8 w[3];
            frag1(mb, ks, w);
            mfma_x3_dual(w, fb[ks], acc, w, fd[ks], dac);
          }
          z[mb] = acc;
          u1[mb] = dac;
        }
      } else {
#pragma unroll
        for (int mb = 0; mb < MB1; mb += 2) {
          f4v a0 = bias4(s_b1 + 16 * mb + 4 * grp), a1 = bias4(s_b1 + 16 * (mb + 1) + 4 * grp);
#pragma unroll
          for (int ks = 0; ks < NK1; ++ks) {
            bf8 w0[3], w1[3];
            frag1(mb, ks, w0);
            frag1(mb + 1, ks, w1);
            mfma_x3_dual(w0, fb[ks], a0, w1, fb[ks], a1);
          }
          z[mb] = a0;
          z[mb + 1] = a1;
        }
      }
      // ---- activation (and its tangent), then the layer-2 B fragments: no lane movement
      bf8 fa[NK2][3], fda[BWD ? NK2 : 1][3];
#pragma unroll
      for (int mb = 0; mb < MB1; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float av, ad;
          act_fast(z[mb][i], P.act, av, ad);
          if constexpr (BWD) u1[mb][i] *= ad;
          z[mb][i] = av;
        }
#pragma unroll
      for (int ks = 0; ks < NK2; ++ks) {
        split_pair(z[2 * ks], z[2 * ks + 1], fa[ks]);
        if constexpr (BWD) split_pair(u1[2 * ks], u1[2 * ks + 1], fda[ks]);
      }

      // ---- layer 2 per 16-row block, consumed at once
      float pc = 0.0f, pd = 0.0f;
      auto frag2 = [&](int mb, int ks, bf8 (&a)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p) a[p] = __builtin_bit_cast(bf8, A2[p * piece2 + (mb * NK2 + ks) * 64 + lane]);
      };
      // w (and dw) of one row block, times the gathered rows
      auto consume = [&](int mb, const f4v& w, const f4v& dw) {
        const int f0 = 16 * mb + 4 * grp;
        const float4 hs = ld4(P.h + so * P.ldh + f0);
        const float hv[4] = {hs.x, hs.y, hs.z, hs.w};
        if constexpr (!BWD) {
#pragma unroll
          for (int i = 0; i < 4; ++i) o[mb][i] += hv[i] * (w[i] * Ce);
        } else {
          const float4 gs4 = ld4(P.g + so * P.ldg + f0);
          const float4 gt4 = ld4(P.g + (size_t)t * P.ldg + f0);
          const float gs[4] = {gs4.x, gs4.y, gs4.z, gs4.w}, gt[4] = {gt4.x, gt4.y, gt4.z, gt4.w};
          const float cs = Ce * sc_s;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            o[mb][i] += gs[i] * (w[i] * cs);
            const float q = gt[i] * hv[i];
            pc += q * w[i];
            pd += q * dw[i];
          }
        }
      };
      const f4v zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (BWD) {
#pragma unroll
        for (int mb = 0; mb < MB1; ++mb) {
          if (mb < MB2) {
            f4v w = bias4(s_b2 + 16 * mb + 4 * grp), dw = zero4;
#pragma unroll
            for (int ks = 0; ks < NK2; ++ks) {
              bf8 a[3];
              frag2(mb, ks, a);
              mfma_x3_dual(a, fa[ks], w, a, fda[ks], dw);
            }
            consume(mb, w, dw);
          }
        }
      } else {
#pragma unroll
        for (int mb = 0; mb < MB1; mb += 2) {
          if (mb + 1 < MB2) {
            f4v w0 = bias4(s_b2 + 16 * mb + 4 * grp), w1 = bias4(s_b2 + 16 * (mb + 1) + 4 * grp);
#pragma unroll
            for (int ks = 0; ks < NK2; ++ks) {
              bf8 a0[3], a1[3];
              frag2(mb, ks, a0);
              frag2(mb + 1, ks, a1);
              mfma_x3_dual(a0, fa[ks], w0, a1, fa[ks], w1);
            }
            consume(mb, w0, zero4);
            consume(mb + 1, w1, zero4);
          } else if (mb < MB2) {  // F / 16 odd: the last block alone
            f4v w = bias4(s_b2 + 16 * mb + 4 * grp);
#pragma unroll
            for (int ks = 0; ks < NK2; ++ks) {
              bf8 a[3];
              frag2(mb, ks, a);
              w = xs::mfma_x3(a, fa[ks], w);
            }
            consume(mb, w, zero4);
          }
        }
      }
      if constexpr (BWD) {  // per edge: the sum over the four lane groups' rows
        pc += __shfl_xor(pc, 16);
        pc += __shfl_xor(pc, 32);
        pd += __shfl_xor(pd, 16);
        pd += __shfl_xor(pd, 32);
        if (grp == 0 && ei < e) {
          P.gcut[ei] = live ? scale_t * pc : 0.0f;
          P.gdist[ei] = live ? scale_t * Ce * pd : 0.0f;
        }
      }
    }

    // ---- the row's sum over its edges: columns of the tiles
    float* dst = BWD ? P.gh : P.out;
    const float sc = BWD ? 1.0f : scale_t;
#pragma unroll
    for (int mb = 0; mb < MB1; ++mb) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = col_sum(o[mb][i]) * sc;
      if (c == 0 && dst && mb < MB2)
        *reinterpret_cast<float4*>(dst + (size_t)t * F + 16 * mb + 4 * grp) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ------------------------------------------------------------------ host side
static int num_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 256;
    return v > 0 ? v : 256;
  }();
  return n;
}

template <int NK1, int NK2, bool BWD>
static int launch_k(const Args& A, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((k_edge<NK1, NK2, BWD>), dim3(nwg), dim3(kNW * 64), 0, st, A);
  return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

template <bool BWD>
static int launch(const Args& A, hipStream_t st) {
  const int nk1 = up32(A.R) / 32, nk2 = up32(A.F) / 32;
  const size_t lds_bytes = image_bytes(32 * nk2, 32 * nk1) + 16;  // the kernel's static LDS
  // small images leave room for several workgroups per CU; the big ones take one CU each
  const int per_cu = (int)((160 * 1024) / lds_bytes);
  const int want = (A.n + kNW - 1) / kNW;
  const int nwg = max(1, min(want, num_cus() * max(1, min(per_cu, 4))));
#define TMD_CFF(K1, K2) \
  if (nk1 == K1 && nk2 == K2) return launch_k<K1, K2, BWD>(A, nwg, st)
  TMD_CFF(1, 1); TMD_CFF(1, 2); TMD_CFF(1, 3); TMD_CFF(1, 4);
  TMD_CFF(2, 1); TMD_CFF(2, 2); TMD_CFF(2, 3); TMD_CFF(2, 4);
#undef TMD_CFF
  return kUnsupported;
}

static int setup(Args& A, int dtype, int aggr, int act, int rbf, int n, int F, int R, const int32_t* row_ptr,
                 const int32_t* src, int cap, const void* h, int ldh, const void* dist, const void* C,
                 const void* mu, const void* beta, double cl, double cu, const void* img) {
  if (dtype != TMDNET_F32 || !in_envelope(F, R)) return kUnsupported;
  if (aggr != TMDNET_AGGR_ADD && aggr != TMDNET_AGGR_MEAN) return kUnsupported;
  if (act != TMDNET_ACT_SILU && act != TMDNET_ACT_SSP) return kUnsupported;
  if (rbf != TMDNET_RBF_EXPNORM && rbf != TMDNET_RBF_GAUSS) return kUnsupported;
  if (n < 0 || cap < 0 || !row_ptr || !mu || !beta || !img || (n > 0 && !h) || (cap > 0 && (!src || !dist || !C)))
    return kBadArgument;
  if (!(cu > cl)) return kBadArgument;
  A = Args{};
  A.n = n; A.F = F; A.R = R; A.cap = cap; A.aggr = aggr; A.act = act; A.rbf = rbf;
  A.row_ptr = row_ptr; A.src = src; A.h = (const float*)h; A.ldh = ldh ? ldh : F;
  A.r = (const float*)dist; A.C = (const float*)C; A.mu = (const float*)mu; A.beta = (const float*)beta;
  A.cl = (float)cl; A.cu = (float)cu; A.alpha = (float)(5.0 / (cu - cl));
  A.img = (const unsigned char*)img;
  if (A.ldh < F) return kBadArgument;
  if (A.ldh % 4 || ((uintptr_t)h | (uintptr_t)img) & 15) return kUnsupported;  // float4 rows, 16-byte image
  return kOk;
}

}  // namespace cff
}  // namespace tmd

using namespace tmd;

extern "C" size_t tmdnet_cfconv_fused_image_bytes(int filters, int num_rbf) {
  return cff::in_envelope(filters, num_rbf) ? cff::image_bytes(filters, num_rbf) : 0;
}

extern "C" int tmdnet_cfconv_fused_image(int n_layers, int filters, int num_rbf, const void* const* w1,
                                         const void* const* b1, const void* const* w2, const void* const* b2,
                                         void* img, void* stream) {
  if (!cff::in_envelope(filters, num_rbf)) return kUnsupported;
  if (n_layers < 0 || !w1 || !w2 || !img) return kBadArgument;
  if ((uintptr_t)img & 15) return kUnsupported;
  for (int l = 0; l < n_layers; ++l)
    if (!w1[l] || !w2[l]) return kBadArgument;
  const size_t per = cff::image_bytes(filters, num_rbf);
  const int Fp = cff::up32(filters), Rp = cff::up32(num_rbf);
  const int slots = (Fp * Rp + filters * Fp) / 8;
  for (int l0 = 0; l0 < n_layers; l0 += cff::kMaxLayers) {  // one launch per 16 layers
    const int nl = n_layers - l0 < cff::kMaxLayers ? n_layers - l0 : cff::kMaxLayers;
    cff::ImgArgs P{};
    P.F = filters; P.R = num_rbf;
    for (int l = 0; l < nl; ++l) {
      P.w1[l] = (const float*)w1[l0 + l];
      P.b1[l] = b1 ? (const float*)b1[l0 + l] : nullptr;
      P.w2[l] = (const float*)w2[l0 + l];
      P.b2[l] = b2 ? (const float*)b2[l0 + l] : nullptr;
    }
    P.img = (unsigned char*)img + (size_t)l0 * per;
    hipLaunchKernelGGL(cff::k_image, dim3((slots + 255) / 256, nl), dim3(256), 0, (hipStream_t)stream, P);
    if (hipGetLastError() != hipSuccess) return kLaunchFailed;
  }
  return kOk;
}

extern "C" int tmdnet_cfconv_fused_fwd(int dtype, int aggr, int act, int rbf_type, int n_nodes, int filters,
                                       int num_rbf, const int32_t* row_ptr, const int32_t* src, int max_pairs,
                                       const void* h, int ld_h, const void* dist, const void* cutoff,
                                       const void* mu, const void* beta, double cutoff_lower,
                                       double cutoff_upper, const void* img, void* out, void* stream) {
  cff::Args A;
  const int rc = cff::setup(A, dtype, aggr, act, rbf_type, n_nodes, filters, num_rbf, row_ptr, src, max_pairs, h,
                            ld_h, dist, cutoff, mu, beta, cutoff_lower, cutoff_upper, img);
  if (rc) return rc;
  if (n_nodes > 0 && !out) return kBadArgument;
  if ((uintptr_t)out & 15) return kUnsupported;
  if (n_nodes == 0) return kOk;
  A.out = (float*)out;
  return cff::launch<false>(A, (hipStream_t)stream);
}

extern "C" int tmdnet_cfconv_fused_bwd(int dtype, int aggr, int act, int rbf_type, int n_nodes, int filters,
                                       int num_rbf, const int32_t* row_ptr, const int32_t* src, int max_pairs,
                                       const void* h, int ld_h, const void* dist, const void* cutoff,
                                       const void* mu, const void* beta, double cutoff_lower,
                                       double cutoff_upper, const void* img, const void* grad_out,
                                       int ld_grad_out, void* gh, void* gcut, void* gdist, void* stream) {
  cff::Args A;
  const int rc = cff::setup(A, dtype, aggr, act, rbf_type, n_nodes, filters, num_rbf, row_ptr, src, max_pairs, h,
                            ld_h, dist, cutoff, mu, beta, cutoff_lower, cutoff_upper, img);
  if (rc) return rc;
  if ((n_nodes > 0 && !grad_out) || (max_pairs > 0 && (!gcut || !gdist))) return kBadArgument;
  A.g = (const float*)grad_out; A.ldg = ld_grad_out ? ld_grad_out : filters;
  if (A.ldg < filters) return kBadArgument;
  if (A.ldg % 4 || ((uintptr_t)grad_out | (uintptr_t)gh) & 15) return kUnsupported;
  A.gh = (float*)gh; A.gcut = (float*)gcut; A.gdist = (float*)gdist;
  hipStream_t st = (hipStream_t)stream;
  if (n_nodes == 0) {  // no row: every slot is padding
    if (max_pairs > 0 && (hipMemsetAsync(gcut, 0, (size_t)max_pairs * 4, st) != hipSuccess ||
                          hipMemsetAsync(gdist, 0, (size_t)max_pairs * 4, st) != hipSuccess))
      return kLaunchFailed;
    return kOk;
  }
  return cff::launch<true>(A, st);
}
