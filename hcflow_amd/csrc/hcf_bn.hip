// BatchNorm2d(C, affine) + LeakyReLU(0.2) / ReLU on the auxiliary nets' NHWC fp32 layout, with an output WINDOW: the layers of
// Discriminator_VGG_128 and PatchGANDiscriminator (codes/models/modules/discriminator_vgg_arch.py:6-65,159-189) in
// hcflow_amd/gan.py. A padding-0 conv is the interior of the same-padded conv the aux kernels compute (hcf_aux.hip), so the
// caller runs hcf_aux_conv2d and hands the window (y0, x0, Ho, Wo) = (1, 1, H-2, W-2) of its H x W output to these kernels,
// which read the window and write a compact Ho x Wo result; the backward pass writes dx into the full H x W buffer with a zero
// border, i.e. exactly the gradient of the same-padded conv's output.
//   x, dx:  NHWC [B][H][W][cs_x]  (cs % 4 == 0, 16-byte aligned)       y, dy:  NHWC [B][Ho][Wo][cs_y]
// Per-channel statistics: per-block fp64 partials over a shape-determined grid, reduced in a fixed order by one finalize block
// per channel (no atomics: bit-reproducible). Every data kernel walks rows of the window with a [rows][float4 column] thread
// layout, so a thread loads its channels' parameters once and then streams float4s.
#include <algorithm>
#include <cmath>

#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace {

constexpr int BN_T = 256;          // threads per block (4 waves)
constexpr int BN_MAX_PART = 1024;  // partial blocks of a statistics reduction (fixed by the shape, never by the device)
constexpr int BN_MAX_APPLY = 2048; // blocks of an elementwise pass (>= 8 per CU on 256 CUs)
constexpr int BN_FIN_T = 256;

enum { BN_MODE_NONE = 0, BN_MODE_TRAIN = 1, BN_MODE_EVAL = 2 };

struct BnShape {
  int C, B, H, W, y0, x0, Ho, Wo;
};

static inline int bn_nblk(int B, int Ho) { return std::min(B * Ho, BN_MAX_PART); }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: [0) partial sums [nblk][C] f64 | [1) partial second sums [nblk][C] f64 | k1 [Cp] f32 | k2 [Cp] f32
struct BnPlan {
  int nblk, Cp;
  size_t o_q, o_k1, o_k2, total;
};
static BnPlan bn_plan(int C, int B, int Ho) {
  BnPlan p;
  p.nblk = bn_nblk(B, Ho);
  p.Cp = (C + 3) & ~3;
  const size_t part = al256((size_t)p.nblk * C * sizeof(double));
  p.o_q = part;
  p.o_k1 = p.o_q + part;
  p.o_k2 = p.o_k1 + al256((size_t)p.Cp * sizeof(float));
  p.total = p.o_k2 + al256((size_t)p.Cp * sizeof(float));
  return p;
}

__device__ inline float4 ld4_masked(const float* p, int c0, int C) {
  float4 v;
  v.x = c0 + 0 < C ? p[c0 + 0] : 0.f;
  v.y = c0 + 1 < C ? p[c0 + 1] : 0.f;
  v.z = c0 + 2 < C ? p[c0 + 2] : 0.f;
  v.w = c0 + 3 < C ? p[c0 + 3] : 0.f;
  return v;
}
__device__ inline float f4(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ inline void f4set(float4& v, int k, float s) {
  if (k == 0) v.x = s; else if (k == 1) v.y = s; else if (k == 2) v.z = s; else v.w = s;
}
__device__ inline float act_slope(int act) { return act == 2 ? 0.2f : 0.f; }

// Per-channel affine in ONE form shared by the forward pass and the backward pass (the backward recomputes the LeakyReLU mask
// from it, so both must round identically): z = (x - mean) * (gamma * invstd) + beta
struct ChanAffine {
  float4 m, inv, sc, be;
};
__device__ inline ChanAffine chan_affine(const float* mean, const float* invstd, const float* gamma, const float* beta, int c0,
                                         int C) {
  ChanAffine a;
  a.m = ld4_masked(mean, c0, C);
  a.inv = ld4_masked(invstd, c0, C);
  const float4 g = ld4_masked(gamma, c0, C);
  a.be = ld4_masked(beta, c0, C);
  a.sc = make_float4(g.x * a.inv.x, g.y * a.inv.y, g.z * a.inv.z, g.w * a.inv.w);
  return a;
}
__device__ inline float affine_k(const ChanAffine& a, float x, int k) {
  return fmaf(x - f4(a.m, k), f4(a.sc, k), f4(a.be, k));
}

// Thread layout of the data kernels: gq float4 columns per block (<= 64), rows = 256 / gq pixel lanes.
struct Lanes {
  int gq, rows, tr, q;
  bool live;
};
__device__ inline Lanes lanes(int ncol) {
  Lanes l;
  l.gq = min(ncol, 64);
  l.rows = BN_T / l.gq;
  l.tr = threadIdx.x / l.gq;
  l.q = blockIdx.y * l.gq + (threadIdx.x - l.tr * l.gq);
  l.live = l.tr < l.rows && l.q < ncol;
  return l;
}

// Block-level fixed-order reduction of 2 x 4 fp64 per thread into per-block partials [blk][C]
__device__ inline void block_partials(const Lanes& l, const double (&s)[4], const double (&s2)[4], int C, double* __restrict__ ps,
                                      double* __restrict__ pq) {
  __shared__ double ls[2][BN_T * 4];
  const int w = l.gq * 4;
  if (l.tr < l.rows) {
    const int tq = threadIdx.x - l.tr * l.gq;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ls[0][l.tr * w + tq * 4 + k] = s[k];
      ls[1][l.tr * w + tq * 4 + k] = s2[k];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < w) {
    double a = 0.0, b = 0.0;
    for (int r = 0; r < l.rows; ++r) {
      a += ls[0][r * w + threadIdx.x];
      b += ls[1][r * w + threadIdx.x];
    }
    const int c = blockIdx.y * w + threadIdx.x;
    if (c < C) {
      ps[(size_t)blockIdx.x * C + c] = a;
      pq[(size_t)blockIdx.x * C + c] = b;
    }
  }
}

// ---- forward, train(): per-block partial sum / sum of squares over the window
__global__ __launch_bounds__(BN_T) void bn_stats_kernel(const float* __restrict__ x, int cs_x, BnShape sh, double* __restrict__ ps,
                                                        double* __restrict__ pq) {
  const Lanes l = lanes((sh.C + 3) / 4);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (l.live) {
    const int R = sh.B * sh.Ho;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
      const int b = r / sh.Ho, i = r - b * sh.Ho;
      const float* row = x + ((size_t)(b * sh.H + sh.y0 + i) * sh.W + sh.x0) * cs_x + 4 * l.q;
      for (int j = l.tr; j < sh.Wo; j += l.rows) {
        const float4 v = *reinterpret_cast<const float4*>(row + (size_t)j * cs_x);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double d = (double)f4(v, k);
          s[k] += d;
          s2[k] = fma(d, d, s2[k]);
        }
      }
    }
  }
  block_partials(l, s, s2, sh.C, ps, pq);
}

// Fixed-order sum of partials [nblk][C] for channel blockIdx.x: strided per-thread sums, then an LDS tree of fixed shape.
__device__ inline void sum_partials(const double* __restrict__ ps, const double* __restrict__ pq, int nblk, int C, double& a,
                                    double& b) {
  __shared__ double t0[BN_FIN_T], t1[BN_FIN_T];
  const int c = blockIdx.x;
  double u = 0.0, v = 0.0;
  for (int k = threadIdx.x; k < nblk; k += BN_FIN_T) {
    u += ps[(size_t)k * C + c];
    v += pq[(size_t)k * C + c];
  }
  t0[threadIdx.x] = u;
  t1[threadIdx.x] = v;
  __syncthreads();
  for (int h = BN_FIN_T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      t0[threadIdx.x] += t0[threadIdx.x + h];
      t1[threadIdx.x] += t1[threadIdx.x + h];
    }
    __syncthreads();
  }
  a = t0[0];
  b = t1[0];
}

// ---- forward finalize (one block per channel): batch statistics (train) or running statistics (eval) -> save_mean / save_invstd;
// train() also moves running_mean / running_var (unbiased variance) in place
__global__ __launch_bounds__(BN_FIN_T) void bn_finalize_fwd_kernel(const double* __restrict__ ps, const double* __restrict__ pq,
                                                                   int nblk, int C, double N, int mode, double momentum, double eps,
                                                                   float* __restrict__ rmean, float* __restrict__ rvar,
                                                                   float* __restrict__ smean, float* __restrict__ sinv) {
  const int c = blockIdx.x;
  if (mode == BN_MODE_TRAIN) {
    double s, q;
    sum_partials(ps, pq, nblk, C, s, q);
    if (threadIdx.x == 0) {
      const double mean = s / N;
      const double var = fmax(q / N - mean * mean, 0.0);
      smean[c] = (float)mean;
      sinv[c] = (float)(1.0 / sqrt(var + eps));
      if (rmean) rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
      if (rvar) rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * var * (N / (N - 1.0)));
    }
  } else if (threadIdx.x == 0) {
    smean[c] = rmean[c];
    sinv[c] = (float)(1.0 / sqrt((double)rvar[c] + eps));
  }
}

// ---- forward apply: y[b, i, j] = act(affine(x[b, y0 + i, x0 + j])) (affine skipped in mode none); channels >= C written 0
__global__ __launch_bounds__(BN_T) void bn_apply_fwd_kernel(const float* __restrict__ x, int cs_x, BnShape sh, const float* mean,
                                                            const float* invstd, const float* gamma, const float* beta, int norm,
                                                            int act, float* __restrict__ y, int cs_y) {
  const Lanes l = lanes(cs_y / 4);
  if (!l.live) return;
  const int c0 = 4 * l.q;
  const bool has = c0 < sh.C;
  ChanAffine a;
  if (norm && has) a = chan_affine(mean, invstd, gamma, beta, c0, sh.C);
  const float slope = act_slope(act);
  const int R = sh.B * sh.Ho;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = r / sh.Ho, i = r - b * sh.Ho;
    const float* row = x + ((size_t)(b * sh.H + sh.y0 + i) * sh.W + sh.x0) * cs_x + c0;
    float* orow = y + (size_t)r * sh.Wo * cs_y + c0;
#pragma unroll 2
    for (int j = l.tr; j < sh.Wo; j += l.rows) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has) {
        const float4 v = *reinterpret_cast<const float4*>(row + (size_t)j * cs_x);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float z = norm ? affine_k(a, f4(v, k), k) : f4(v, k);
          if (act) z = z > 0.f ? z : z * slope;
          f4set(o, k, c0 + k < sh.C ? z : 0.f);
        }
      }
      *reinterpret_cast<float4*>(orow + (size_t)j * cs_y) = o;
    }
  }
}

// ---- backward reduction: per-block partials of sum dy' and sum dy' * xhat, dy' = dy * act'(z)
__global__ __launch_bounds__(BN_T) void bn_bwd_reduce_kernel(const float* __restrict__ x, int cs_x, BnShape sh,
                                                             const float* __restrict__ dy, int cs_dy, const float* mean,
                                                             const float* invstd, const float* gamma, const float* beta, int act,
                                                             double* __restrict__ ps, double* __restrict__ pq) {
  const Lanes l = lanes((sh.C + 3) / 4);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (l.live) {
    const int c0 = 4 * l.q;
    const ChanAffine a = chan_affine(mean, invstd, gamma, beta, c0, sh.C);
    const float slope = act_slope(act);
    const int R = sh.B * sh.Ho;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
      const int b = r / sh.Ho, i = r - b * sh.Ho;
      const float* row = x + ((size_t)(b * sh.H + sh.y0 + i) * sh.W + sh.x0) * cs_x + c0;
      const float* grow = dy + (size_t)r * sh.Wo * cs_dy + c0;
      for (int j = l.tr; j < sh.Wo; j += l.rows) {
        const float4 v = *reinterpret_cast<const float4*>(row + (size_t)j * cs_x);
        const float4 g = *reinterpret_cast<const float4*>(grow + (size_t)j * cs_dy);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float gk = f4(g, k);
          if (act && !(affine_k(a, f4(v, k), k) > 0.f)) gk *= slope;
          const float xh = (f4(v, k) - f4(a.m, k)) * f4(a.inv, k);
          s[k] += (double)gk;
          s2[k] = fma((double)gk, (double)xh, s2[k]);
        }
      }
    }
  }
  block_partials(l, s, s2, sh.C, ps, pq);
}

// ---- backward finalize (one block per channel): dbeta = sum dy', dgamma = sum dy' xhat (each nullable); k1 = sum dy' / N,
// k2 = sum dy' xhat / N for the train() data gradient
__global__ __launch_bounds__(BN_FIN_T) void bn_finalize_bwd_kernel(const double* __restrict__ ps, const double* __restrict__ pq,
                                                                   int nblk, int C, double N, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, float* __restrict__ k1,
                                                                   float* __restrict__ k2) {
  double s, q;
  sum_partials(ps, pq, nblk, C, s, q);
  if (threadIdx.x == 0) {
    const int c = blockIdx.x;
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
    k1[c] = (float)(s / N);
    k2[c] = (float)(q / N);
  }
}

// ---- backward apply over the FULL H x W input: inside the window
//   train: dx = gamma invstd (dy' - k1 - xhat k2);  eval: dx = gamma invstd dy';  none: dx = dy'
// and exactly 0 on the border and in channels >= C
__global__ __launch_bounds__(BN_T) void bn_apply_bwd_kernel(const float* __restrict__ x, int cs_x, BnShape sh,
                                                            const float* __restrict__ dy, int cs_dy, const float* mean,
                                                            const float* invstd, const float* gamma, const float* beta,
                                                            const float* k1, const float* k2, int mode, int act,
                                                            float* __restrict__ dx, int cs_dx) {
  const Lanes l = lanes(cs_dx / 4);
  if (!l.live) return;
  const int c0 = 4 * l.q;
  const bool has = c0 < sh.C;
  const bool norm = mode != BN_MODE_NONE;
  ChanAffine a;
  float4 m1 = make_float4(0.f, 0.f, 0.f, 0.f), m2 = m1;
  if (norm && has) {
    a = chan_affine(mean, invstd, gamma, beta, c0, sh.C);
    if (mode == BN_MODE_TRAIN) {
      m1 = ld4_masked(k1, c0, sh.C);
      m2 = ld4_masked(k2, c0, sh.C);
    }
  }
  const float slope = act_slope(act);
  const int R = sh.B * sh.H;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = r / sh.H, h = r - b * sh.H;
    const int i = h - sh.y0;
    const bool row_in = i >= 0 && i < sh.Ho;
    const float* xrow = x + (size_t)r * sh.W * cs_x + c0;
    const float* grow = dy + (size_t)(b * sh.Ho + (row_in ? i : 0)) * sh.Wo * cs_dy + c0;
    float* orow = dx + (size_t)r * sh.W * cs_dx + c0;
#pragma unroll 2
    for (int w = l.tr; w < sh.W; w += l.rows) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has && row_in && w >= sh.x0 && w < sh.x0 + sh.Wo) {
        const float4 g = *reinterpret_cast<const float4*>(grow + (size_t)(w - sh.x0) * cs_dy);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (norm || act) v = *reinterpret_cast<const float4*>(xrow + (size_t)w * cs_x);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float gk = f4(g, k);
          const float z = norm ? affine_k(a, f4(v, k), k) : f4(v, k);
          if (act && !(z > 0.f)) gk *= slope;
          float d = gk;
          if (norm) {
            if (mode == BN_MODE_TRAIN) {
              const float xh = (f4(v, k) - f4(a.m, k)) * f4(a.inv, k);
              d = f4(a.sc, k) * (gk - f4(m1, k) - xh * f4(m2, k));
            } else {
              d = f4(a.sc, k) * gk;
            }
          }
          f4set(o, k, c0 + k < sh.C ? d : 0.f);
        }
      }
      *reinterpret_cast<float4*>(orow + (size_t)w * cs_dx) = o;
    }
  }
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int bn_check_shape(const float* x, int cs_x, const BnShape& s) {
  if (!x || !al16(x) || s.C < 1 || s.B < 1 || s.H < 1 || s.W < 1 || (cs_x & 3) || cs_x < s.C || s.y0 < 0 || s.x0 < 0 ||
      s.Ho < 1 || s.Wo < 1 || s.y0 + s.Ho > s.H || s.x0 + s.Wo > s.W)
    return HCF_ERR_ARG;
  // 32-bit row indices; 64-bit element offsets
  if ((int64_t)s.B * s.H > (1 << 30)) return HCF_ERR_SHAPE;
  return HCF_OK;
}

static dim3 bn_grid(int rows_total, int ncol, int cap) {
  const int gq = std::min(ncol, 64);
  return dim3((unsigned)std::min(rows_total, cap), (unsigned)((ncol + gq - 1) / gq));
}

}  // namespace
}  // namespace hcf

using namespace hcf;

extern "C" {

size_t hcf_aux_bn_act_workspace(int32_t C, int32_t B, int32_t Ho, int32_t Wo) {
  if (C < 1 || B < 1 || Ho < 1 || Wo < 1) return 0;
  return bn_plan(C, B, Ho).total;
}

int hcf_aux_bn_act(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t Ho,
                   int32_t Wo, const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t mode,
                   double momentum, double eps, int32_t act, float* y, int32_t cs_y, float* save_mean, float* save_invstd,
                   void* work, size_t work_bytes, hcf_stream_t stream) {
  const BnShape sh = {C, B, H, W, y0, x0, Ho, Wo};
  int rc = bn_check_shape(x, cs_x, sh);
  if (rc != HCF_OK) return rc;
  if (!y || !al16(y) || (cs_y & 3) || cs_y < C || act < 0 || act > 2 || mode < BN_MODE_NONE || mode > BN_MODE_EVAL)
    return HCF_ERR_ARG;
  const double N = (double)B * Ho * Wo;
  hipStream_t st = (hipStream_t)stream;
  if (mode != BN_MODE_NONE) {
    if (!gamma || !beta || !save_mean || !save_invstd || !(eps > 0.0)) return HCF_ERR_ARG;
    if (mode == BN_MODE_EVAL && (!running_mean || !running_var)) return HCF_ERR_ARG;
    if (mode == BN_MODE_TRAIN && (N < 2.0 || !work || !(momentum >= 0.0 && momentum <= 1.0) || (!running_mean != !running_var)))
      return HCF_ERR_ARG;                                  // torch: "Expected more than 1 value per channel when training"
    const BnPlan p = bn_plan(C, B, Ho);
    if (mode == BN_MODE_TRAIN && work_bytes < p.total) return HCF_ERR_NOMEM;
    double* ps = (double*)work;
    double* pq = (double*)((char*)work + p.o_q);
    if (mode == BN_MODE_TRAIN) {
      hipLaunchKernelGGL(bn_stats_kernel, bn_grid(B * Ho, (C + 3) / 4, BN_MAX_PART), dim3(BN_T), 0, st, x, cs_x, sh, ps, pq);
      if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
    }
    hipLaunchKernelGGL(bn_finalize_fwd_kernel, dim3((unsigned)C), dim3(BN_FIN_T), 0, st, ps, pq, p.nblk, C, N, mode, momentum, eps,
                       running_mean, running_var, save_mean, save_invstd);
    if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  }
  hipLaunchKernelGGL(bn_apply_fwd_kernel, bn_grid(B * Ho, cs_y / 4, BN_MAX_APPLY), dim3(BN_T), 0, st, x, cs_x, sh, save_mean,
                     save_invstd, gamma, beta, mode != BN_MODE_NONE ? 1 : 0, act, y, cs_y);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_aux_bn_act_backward(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, int32_t y0, int32_t x0,
                            int32_t Ho, int32_t Wo, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, int32_t mode, int32_t act, const float* dy, int32_t cs_dy, float* dx,
                            int32_t cs_dx, float* dgamma, float* dbeta, void* work, size_t work_bytes, hcf_stream_t stream) {
  const BnShape sh = {C, B, H, W, y0, x0, Ho, Wo};
  int rc = bn_check_shape(x, cs_x, sh);
  if (rc != HCF_OK) return rc;
  if (!dy || !al16(dy) || (cs_dy & 3) || cs_dy < C || !dx || !al16(dx) || (cs_dx & 3) || cs_dx < C || act < 0 || act > 2 ||
      mode < BN_MODE_NONE || mode > BN_MODE_EVAL)
    return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const double N = (double)B * Ho * Wo;
  const float* k1 = nullptr;
  const float* k2 = nullptr;
  if (mode != BN_MODE_NONE) {
    if (!gamma || !beta || !save_mean || !save_invstd) return HCF_ERR_ARG;
    // the reduction feeds the train() data gradient and the parameter gradients; eval() without parameter gradients skips it
    if (mode == BN_MODE_TRAIN || dgamma || dbeta) {
      if (!work) return HCF_ERR_ARG;
      const BnPlan p = bn_plan(C, B, Ho);
      if (work_bytes < p.total) return HCF_ERR_NOMEM;
      double* ps = (double*)work;
      double* pq = (double*)((char*)work + p.o_q);
      float* w1 = (float*)((char*)work + p.o_k1);
      float* w2 = (float*)((char*)work + p.o_k2);
      hipLaunchKernelGGL(bn_bwd_reduce_kernel, bn_grid(B * Ho, (C + 3) / 4, BN_MAX_PART), dim3(BN_T), 0, st, x, cs_x, sh, dy, cs_dy,
                         save_mean, save_invstd, gamma, beta, act, ps, pq);
      if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
      hipLaunchKernelGGL(bn_finalize_bwd_kernel, dim3((unsigned)C), dim3(BN_FIN_T), 0, st, ps, pq, p.nblk, C, N, dgamma, dbeta, w1,
                         w2);
      if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
      k1 = w1;
      k2 = w2;
    }
  }
  hipLaunchKernelGGL(bn_apply_bwd_kernel, bn_grid(B * H, cs_dx / 4, BN_MAX_APPLY), dim3(BN_T), 0, st, x, cs_x, sh, dy, cs_dy,
                     save_mean, save_invstd, gamma, beta, k1, k2, mode, act, dx, cs_dx);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
