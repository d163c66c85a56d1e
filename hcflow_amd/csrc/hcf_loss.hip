// The training criteria of the reference's callers (models/modules/loss.py and the expressions around it in
// HCFlow_SR_model.py:207-287, HCFlow_Rescaling_model.py:214-232) on the device, each with its backward:
//   pair criterion   |d|, d^2, sqrt(d^2 + eps) of two [B][n] tensors, as one scalar and / or one value per sample
//   sum of squares   the mean square of up to 8 tensors of any lengths (the rescaling net's latent term)
//   GAN criteria     BCE-with-logits / least squares / Wasserstein on one or two logit tensors, plain or relativistic
// include/hcflow.h states the contract. Every term is fp64 from fp32 inputs; a reduction is per-block fp64 partials of a grid that
// the shape alone decides plus ONE fixed-order final block (as vgg_loss_partial_kernel / vgg_loss_final_kernel, hcf_vgg.hip): no
// atomics, no tickets, no block waits for another. The work of a block is defined on LOGICAL quads (elements 4q .. 4q + 3 of a row),
// so which element meets which accumulator in which order never depends on an address: a 16-byte aligned call loads a quad as one
// float4, any other call as four floats (which the compiler may still fetch with one wide load: a global load needs 4-byte
// alignment only), and both give the same bits.
#include <algorithm>
#include <cmath>

#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace {

constexpr int LS_T = 256;                 // threads per block (4 waves)
constexpr int LS_PER_BLK = LS_T * 4 * 4;  // floats one partial block covers before the sample's grid wraps (4 quads per thread)
constexpr int LS_MAX_PART = 1024;         // partial blocks per sample (fixed by n, never by the device)
constexpr int LS_MAX_BLK = 2048;          // blocks of an elementwise (backward) pass
constexpr int LS_MAX_TENS = 8;            // tensors of one sum-of-squares call
constexpr int LS_BWD_TENS_BLK = 256;      // blocks per tensor of the sum-of-squares backward
constexpr int LG_T = 1024;                // threads of the single block of a GAN criterion
constexpr int64_t LG_MAX_N = (int64_t)1 << 20;
constexpr int64_t LS_MAX_ELEMS = (int64_t)1 << 40;
constexpr int64_t LS_MAX_GRID = (int64_t)1 << 23;   // blocks of one launch (2^31 threads)

static inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int pair_nblk(int64_t n) { return (int)std::min<int64_t>((n + LS_PER_BLK - 1) / LS_PER_BLK, LS_MAX_PART); }

template <bool VEC>
__device__ inline float4 load_quad(const float* p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ inline void store_quad(float* p, const float4& v) {
  if (VEC) { *reinterpret_cast<float4*>(p) = v; return; }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

template <int KIND>
__device__ inline double pair_term(float a, float b, double eps) {
  const double d = (double)a - (double)b;
  if (KIND == 0) return fabs(d);
  if (KIND == 1) return d * d;
  return sqrt(d * d + eps);
}

// fp32(g * scale * f'(d)); exact zero for g == 0 whatever d is (a dropped term), NaN / inf of d propagate otherwise
template <int KIND>
__device__ inline float pair_grad(float a, float b, float g, double scale, double eps) {
  if (g == 0.f) return 0.f;
  const double d = (double)a - (double)b;
  double fp;
  if (KIND == 0) fp = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;        // 0 at 0, NaN stays NaN
  else if (KIND == 1) fp = 2.0 * d;
  else fp = d / sqrt(d * d + eps);
  return (float)((double)g * scale * fp);
}

// sum of a block's LS_T values through an LDS tree of fixed shape; every thread returns the total
template <int T>
__device__ inline double block_sum(double s, double* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();                                               // red is free for the next call
  return r;
}

// The sum block p of P takes of one row of n floats: quads p * LS_T + t, + P * LS_T, ...; block 0 adds the <= 3 floats behind
// the last quad. y == nullptr: zeros.
template <int KIND, bool VEC>
__device__ inline double pair_block_sum(const float* __restrict__ x, const float* __restrict__ y, int64_t n, int p, int P, double eps,
                                        double* red) {
  const int64_t nq = n >> 2;
  double s = 0.0;
#pragma unroll 2
  for (int64_t q = (int64_t)p * LS_T + threadIdx.x; q < nq; q += (int64_t)P * LS_T) {
    const float4 u = load_quad<VEC>(x + 4 * q);
    const float4 v = y ? load_quad<VEC>(y + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += pair_term<KIND>(u.x, v.x, eps);
    s += pair_term<KIND>(u.y, v.y, eps);
    s += pair_term<KIND>(u.z, v.z, eps);
    s += pair_term<KIND>(u.w, v.w, eps);
  }
  if (p == 0 && (int64_t)threadIdx.x < n - 4 * nq) {
    const int64_t i = 4 * nq + threadIdx.x;
    s += pair_term<KIND>(x[i], y ? y[i] : 0.f, eps);
  }
  return block_sum<LS_T>(s, red);
}

// grid = B * P blocks, block b * P + p: partial p of sample b
template <int KIND, bool VEC>
__global__ __launch_bounds__(LS_T) void loss_pair_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                                 int P, double eps, double* __restrict__ part) {
  __shared__ double red[LS_T];
  const int64_t b = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x - b * P);
  const double s = pair_block_sum<KIND, VEC>(x + b * n, y ? y + b * n : nullptr, n, p, P, eps, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One block. Wave w joins the P partials of samples w, w + 4, ...: lane l adds partials l, l + 64, ... in order, then a shuffle tree
// of fixed shape -- S_b depends on P and the partials alone, not on B. Thread 0 then adds S_0, S_1, ... in index order.
__global__ __launch_bounds__(LS_T) void loss_pair_final_kernel(const double* __restrict__ part, int64_t B, int P, double scale,
                                                               double row_scale, double* __restrict__ sums, float* __restrict__ out,
                                                               float* __restrict__ out_rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = wave; b < B; b += LS_T / 64) {
    const double* pp = part + b * P;
    double s = 0.0;
    for (int k = lane; k < P; k += 64) s += pp[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
      sums[b] = s;
      if (out_rows) out_rows[b] = (float)(row_scale * s);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && out) {
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) s += sums[b];
    out[0] = (float)(scale * s);
  }
}

// Elementwise over the N = B * n floats of the flat tensors; g[b * g_stride] with b = the element's row.
template <int KIND, bool VEC>
__global__ __launch_bounds__(LS_T) void loss_pair_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t N,
                                                             int64_t n, double eps, double scale, const float* __restrict__ g,
                                                             int g_stride, float* __restrict__ gx, float* __restrict__ gy) {
  const int64_t nq = N >> 2;
  const float g0 = g[0];
  for (int64_t q = (int64_t)blockIdx.x * LS_T + threadIdx.x; q < nq; q += (int64_t)gridDim.x * LS_T) {
    const int64_t e = 4 * q;
    const float4 u = load_quad<VEC>(x + e);
    const float4 v = y ? load_quad<VEC>(y + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    float gq[4] = {g0, g0, g0, g0};
    if (g_stride) {
      int64_t b = e / n, r = e - b * n;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        while (r >= n) { r -= n; ++b; }
        gq[k] = g[b];
        ++r;
      }
    }
    float4 o;
    o.x = pair_grad<KIND>(u.x, v.x, gq[0], scale, eps);
    o.y = pair_grad<KIND>(u.y, v.y, gq[1], scale, eps);
    o.z = pair_grad<KIND>(u.z, v.z, gq[2], scale, eps);
    o.w = pair_grad<KIND>(u.w, v.w, gq[3], scale, eps);
    if (gx) store_quad<VEC>(gx + e, o);
    if (gy) store_quad<VEC>(gy + e, make_float4(-o.x, -o.y, -o.z, -o.w));
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < N - 4 * nq) {
    const int64_t i = 4 * nq + threadIdx.x;
    const float o = pair_grad<KIND>(x[i], y ? y[i] : 0.f, g_stride ? g[i / n] : g0, scale, eps);
    if (gx) gx[i] = o;
    if (gy) gy[i] = -o;
  }
}

// ---- sum of squares over a table of tensors. Blocks [blk0[k], blk0[k + 1]) belong to tensor k.
struct SumsqTab {
  const float* z[LS_MAX_TENS];
  float* gz[LS_MAX_TENS];
  long long len[LS_MAX_TENS];
  int blk0[LS_MAX_TENS + 1];
  int count;
};

__device__ inline int sumsq_tensor_of(const SumsqTab& t, int blk) {
  int k = 0;
  while (k + 1 < t.count && blk >= t.blk0[k + 1]) ++k;
  return k;
}

__global__ __launch_bounds__(LS_T) void loss_sumsq_partial_kernel(SumsqTab t, double* __restrict__ part) {
  __shared__ double red[LS_T];
  const int k = sumsq_tensor_of(t, (int)blockIdx.x);
  const int p = (int)blockIdx.x - t.blk0[k], P = t.blk0[k + 1] - t.blk0[k];
  const float* z = t.z[k];
  const double s = (((uintptr_t)z & 15) == 0) ? pair_block_sum<1, true>(z, nullptr, t.len[k], p, P, 0.0, red)
                                              : pair_block_sum<1, false>(z, nullptr, t.len[k], p, P, 0.0, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(LS_T) void loss_sumsq_bwd_kernel(SumsqTab t, double scale, const float* __restrict__ g) {
  const int k = sumsq_tensor_of(t, (int)blockIdx.x);
  float* gz = t.gz[k];
  if (!gz) return;
  const int p = (int)blockIdx.x - t.blk0[k], P = t.blk0[k + 1] - t.blk0[k];
  const float* z = t.z[k];
  const int64_t n = t.len[k], nq = n >> 2;
  const float g0 = g[0];
  const bool vec = (((uintptr_t)z | (uintptr_t)gz) & 15) == 0;
  for (int64_t q = (int64_t)p * LS_T + threadIdx.x; q < nq; q += (int64_t)P * LS_T) {
    const float4 u = vec ? load_quad<true>(z + 4 * q) : load_quad<false>(z + 4 * q);
    float4 o;
    o.x = pair_grad<1>(u.x, 0.f, g0, scale, 0.0);
    o.y = pair_grad<1>(u.y, 0.f, g0, scale, 0.0);
    o.z = pair_grad<1>(u.z, 0.f, g0, scale, 0.0);
    o.w = pair_grad<1>(u.w, 0.f, g0, scale, 0.0);
    if (vec) store_quad<true>(gz + 4 * q, o); else store_quad<false>(gz + 4 * q, o);
  }
  if (p == 0 && (int64_t)threadIdx.x < n - 4 * nq) {
    const int64_t i = 4 * nq + threadIdx.x;
    gz[i] = pair_grad<1>(z[i], 0.f, g0, scale, 0.0);
  }
}

// ---- GAN criteria: one block of LG_T threads, thread t takes elements t, t + LG_T, ... of a tensor
__device__ inline double gan_term(double v, double t, int type) {
  if (type == 0) return fmax(v, 0.0) - v * t + log1p(exp(-fabs(v)));
  if (type == 1) return (v - t) * (v - t);
  return t > 0.5 ? -v : v;
}
__device__ inline double gan_dterm(double v, double t, int type) {
  if (type == 0) {
    // sigmoid(v) - t without overflow and without cancellation: for v >= 0, sigmoid(v) = 1 - e / (1 + e), and 1 - t is exact for
    // the labels 1 and 0 -- a saturated logit on the right side of its label keeps its tiny gradient to full precision
    const double e = exp(-fabs(v)), r = e / (1.0 + e);
    return v >= 0.0 ? (1.0 - t) - r : r - t;
  }
  if (type == 1) return 2.0 * (v - t);
  return t > 0.5 ? -1.0 : 1.0;
}

struct GanArgs {
  const float* a; long long na; double ta;
  const float* b; long long nb; double tb;
  int type, rel, halve;
};

__device__ inline double gan_sum(const float* __restrict__ p, long long n, double* red) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += LG_T) s += (double)p[i];
  return block_sum<LG_T>(s, red);
}
__device__ inline double gan_term_sum(const float* __restrict__ p, long long n, double shift, double t, int type, bool deriv,
                                      double* red) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += LG_T) {
    const double v = (double)p[i] - shift;
    s += deriv ? gan_dterm(v, t, type) : gan_term(v, t, type);
  }
  return block_sum<LG_T>(s, red);
}

__global__ __launch_bounds__(LG_T) void loss_gan_kernel(GanArgs q, float* __restrict__ out) {
  __shared__ double red[LG_T];
  const double ma = gan_sum(q.a, q.na, red) / (double)q.na;
  const double mb = q.nb ? gan_sum(q.b, q.nb, red) / (double)q.nb : 0.0;
  const double ta_ = gan_term_sum(q.a, q.na, q.rel ? mb : 0.0, q.ta, q.type, false, red) / (double)q.na;
  const double tb_ = q.nb ? gan_term_sum(q.b, q.nb, q.rel ? ma : 0.0, q.tb, q.type, false, red) / (double)q.nb : 0.0;
  if (threadIdx.x == 0) {
    out[0] = (float)ta_;
    out[1] = (float)tb_;
    out[2] = (float)((ta_ + tb_) * (q.halve ? 0.5 : 1.0));
    out[3] = (float)ma;
    out[4] = (float)mb;
  }
}

// total = w (A + Bt), A = mean_i f(a_i - mb), Bt = mean_j f(b_j - ma):
//   d total / d a_i = w (f'(va_i) / na - Db / (na nb)),  d total / d b_j = w (f'(vb_j) / nb - Da / (na nb)),
// Da = sum_i f'(va_i), Db = sum_j f'(vb_j): the second terms are the paths through the means (relativistic form only).
__global__ __launch_bounds__(LG_T) void loss_gan_bwd_kernel(GanArgs q, const float* __restrict__ g, float* __restrict__ ga,
                                                            float* __restrict__ gb) {
  __shared__ double red[LG_T];
  const float g0 = g[0];
  double sa = 0.0, sb = 0.0, ca = 0.0, cb = 0.0;
  if (q.rel && g0 != 0.f) {
    sb = gan_sum(q.a, q.na, red) / (double)q.na;                 // the shift of b is mean(a)
    sa = gan_sum(q.b, q.nb, red) / (double)q.nb;
    const double Da = gan_term_sum(q.a, q.na, sa, q.ta, q.type, true, red);
    const double Db = gan_term_sum(q.b, q.nb, sb, q.tb, q.type, true, red);
    ca = Db / ((double)q.na * (double)q.nb);
    cb = Da / ((double)q.na * (double)q.nb);
  }
  const double w = (double)g0 * (q.halve ? 0.5 : 1.0);
  if (ga) {
    for (long long i = threadIdx.x; i < q.na; i += LG_T)
      ga[i] = g0 == 0.f ? 0.f : (float)(w * (gan_dterm((double)q.a[i] - sa, q.ta, q.type) / (double)q.na - ca));
  }
  if (gb) {
    for (long long i = threadIdx.x; i < q.nb; i += LG_T)
      gb[i] = g0 == 0.f ? 0.f : (float)(w * (gan_dterm((double)q.b[i] - sb, q.tb, q.type) / (double)q.nb - cb));
  }
}

static int pair_check(const float* x, const float* y, int64_t B, int64_t n, int32_t kind, double eps) {
  if (!x || !al4(x) || !al4(y) || B < 1 || n < 1 || kind < 0 || kind > 2 || !(eps >= 0.0) || !std::isfinite(eps)) return HCF_ERR_ARG;
  if (B > LS_MAX_ELEMS / n) return HCF_ERR_SHAPE;                                   // B * n <= 2^40, without the overflow
  if (B * (int64_t)pair_nblk(n) > LS_MAX_GRID) return HCF_ERR_SHAPE;
  return HCF_OK;
}

template <bool VEC>
static void launch_pair_partial(int kind, unsigned grid, hipStream_t st, const float* x, const float* y, int64_t n, int P, double eps,
                                double* part) {
  if (kind == 0) hipLaunchKernelGGL((loss_pair_partial_kernel<0, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, n, P, eps, part);
  else if (kind == 1) hipLaunchKernelGGL((loss_pair_partial_kernel<1, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, n, P, eps, part);
  else hipLaunchKernelGGL((loss_pair_partial_kernel<2, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, n, P, eps, part);
}

template <bool VEC>
static void launch_pair_bwd(int kind, unsigned grid, hipStream_t st, const float* x, const float* y, int64_t N, int64_t n, double eps,
                            double scale, const float* g, int g_stride, float* gx, float* gy) {
  if (kind == 0)
    hipLaunchKernelGGL((loss_pair_bwd_kernel<0, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, N, n, eps, scale, g, g_stride, gx, gy);
  else if (kind == 1)
    hipLaunchKernelGGL((loss_pair_bwd_kernel<1, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, N, n, eps, scale, g, g_stride, gx, gy);
  else
    hipLaunchKernelGGL((loss_pair_bwd_kernel<2, VEC>), dim3(grid), dim3(LS_T), 0, st, x, y, N, n, eps, scale, g, g_stride, gx, gy);
}

// the table of a sum-of-squares call: HCF_OK and the total length in *N, blocks per tensor from `blocks_of`
template <typename F>
static int sumsq_table(const float* const* z, const int64_t* len, int32_t count, float* const* gz, F blocks_of, SumsqTab* t,
                       int64_t* N) {
  if (!z || !len || count < 1 || count > LS_MAX_TENS) return HCF_ERR_ARG;
  int64_t total = 0;
  t->count = count;
  t->blk0[0] = 0;
  for (int k = 0; k < LS_MAX_TENS; ++k) {
    const bool live = k < count;
    if (live && (!z[k] || !al4(z[k]) || len[k] < 1 || (gz && !al4(gz[k])))) return HCF_ERR_ARG;
    if (live && (len[k] > LS_MAX_ELEMS || (total += len[k]) > LS_MAX_ELEMS)) return HCF_ERR_SHAPE;
    t->z[k] = live ? z[k] : nullptr;
    t->gz[k] = live && gz ? gz[k] : nullptr;
    t->len[k] = live ? len[k] : 0;
    t->blk0[k + 1] = t->blk0[k] + (live ? blocks_of(len[k]) : 0);
  }
  *N = total;
  return HCF_OK;
}

static int gan_check(const float* a, int64_t na, double ta, const float* b, int64_t nb, double tb, int32_t type, int32_t rel,
                     int32_t halve) {
  if (!a || !al4(a) || !al4(b) || na < 1 || nb < 0 || (!b != (nb == 0)) || type < 0 || type > 2 || rel < 0 || rel > 1 || halve < 0 ||
      halve > 1 || (rel && !b) || !std::isfinite(ta) || !std::isfinite(tb))
    return HCF_ERR_ARG;
  if (na > LG_MAX_N || nb > LG_MAX_N) return HCF_ERR_SHAPE;
  return HCF_OK;
}

}  // namespace
}  // namespace hcf

using namespace hcf;

extern "C" {

size_t hcf_loss_pair_workspace(int64_t B, int64_t n) {
  if (pair_check((const float*)16, nullptr, B, n, 0, 0.0) != HCF_OK) return 0;
  return (((size_t)B * (size_t)pair_nblk(n) + (size_t)B) * sizeof(double) + 255) & ~(size_t)255;
}

int hcf_loss_pair(const float* x, const float* y, int64_t B, int64_t n, int32_t kind, double eps, double scale, double row_scale,
                  float* out, float* out_rows, void* work, size_t work_bytes, hcf_stream_t stream) {
  const int rc = pair_check(x, y, B, n, kind, eps);
  if (rc != HCF_OK) return rc;
  if ((!out && !out_rows) || !al4(out) || !al4(out_rows) || !work || ((uintptr_t)work & 7)) return HCF_ERR_ARG;
  if (work_bytes < hcf_loss_pair_workspace(B, n)) return HCF_ERR_NOMEM;
  const int P = pair_nblk(n);
  const unsigned grid = (unsigned)(B * P);
  double* part = (double*)work;
  double* sums = part + (size_t)B * P;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = al16(x) && (!y || al16(y)) && (B == 1 || (n & 3) == 0);      // every row starts 16-byte aligned
  if (vec) launch_pair_partial<true>(kind, grid, st, x, y, n, P, eps, part);
  else launch_pair_partial<false>(kind, grid, st, x, y, n, P, eps, part);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  hipLaunchKernelGGL(loss_pair_final_kernel, dim3(1), dim3(LS_T), 0, st, (const double*)part, B, P, scale, row_scale, sums, out,
                     out_rows);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_loss_pair_backward(const float* x, const float* y, int64_t B, int64_t n, int32_t kind, double eps, double scale,
                           const float* g, int32_t g_stride, float* gx, float* gy, hcf_stream_t stream) {
  const int rc = pair_check(x, y, B, n, kind, eps);
  if (rc != HCF_OK) return rc;
  if (!g || !al4(g) || g_stride < 0 || g_stride > 1 || (!gx && !gy) || !al4(gx) || !al4(gy)) return HCF_ERR_ARG;
  const int64_t N = B * n;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((N >> 2) + LS_T - 1) / LS_T, LS_MAX_BLK));
  hipStream_t st = (hipStream_t)stream;
  const bool vec = al16(x) && (!y || al16(y)) && (!gx || al16(gx)) && (!gy || al16(gy));   // flat pass: the bases alone matter
  if (vec) launch_pair_bwd<true>(kind, grid, st, x, y, N, n, eps, scale, g, g_stride, gx, gy);
  else launch_pair_bwd<false>(kind, grid, st, x, y, N, n, eps, scale, g, g_stride, gx, gy);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

size_t hcf_loss_sumsq_workspace(const int64_t* len, int32_t count) {
  if (!len || count < 1 || count > LS_MAX_TENS) return 0;
  size_t blocks = 0;
  for (int k = 0; k < count; ++k) {
    if (len[k] < 1 || len[k] > LS_MAX_ELEMS) return 0;
    blocks += (size_t)pair_nblk(len[k]);
  }
  return ((blocks + 1) * sizeof(double) + 255) & ~(size_t)255;
}

int hcf_loss_sumsq(const float* const* z, const int64_t* len, int32_t count, float* out, void* work, size_t work_bytes,
                   hcf_stream_t stream) {
  SumsqTab t;
  int64_t N = 0;
  const int rc = sumsq_table(z, len, count, nullptr, pair_nblk, &t, &N);
  if (rc != HCF_OK) return rc;
  if (!out || !al4(out) || !work || ((uintptr_t)work & 7)) return HCF_ERR_ARG;
  if (work_bytes < hcf_loss_sumsq_workspace(len, count)) return HCF_ERR_NOMEM;
  const int nblk = t.blk0[LS_MAX_TENS];
  double* part = (double*)work;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_sumsq_partial_kernel, dim3((unsigned)nblk), dim3(LS_T), 0, st, t, part);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  hipLaunchKernelGGL(loss_pair_final_kernel, dim3(1), dim3(LS_T), 0, st, (const double*)part, (int64_t)1, nblk, 1.0 / (double)N, 0.0,
                     part + nblk, out, (float*)nullptr);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_loss_sumsq_backward(const float* const* z, const int64_t* len, int32_t count, const float* g, float* const* gz,
                            hcf_stream_t stream) {
  if (!gz) return HCF_ERR_ARG;
  SumsqTab t;
  int64_t N = 0;
  const int rc = sumsq_table(z, len, count, gz, [](int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(((n >> 2) + LS_T - 1) / LS_T, LS_BWD_TENS_BLK)); }, &t, &N);
  if (rc != HCF_OK) return rc;
  bool any = false;
  for (int k = 0; k < count; ++k) any = any || gz[k];
  if (!g || !al4(g) || !any) return HCF_ERR_ARG;
  hipLaunchKernelGGL(loss_sumsq_bwd_kernel, dim3((unsigned)t.blk0[LS_MAX_TENS]), dim3(LS_T), 0, (hipStream_t)stream, t,
                     1.0 / (double)N, g);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_loss_gan(const float* a, int64_t na, double ta, const float* b, int64_t nb, double tb, int32_t type, int32_t relativistic,
                 int32_t halve, float* out, hcf_stream_t stream) {
  const int rc = gan_check(a, na, ta, b, nb, tb, type, relativistic, halve);
  if (rc != HCF_OK) return rc;
  if (!out || !al4(out)) return HCF_ERR_ARG;
  const GanArgs q = {a, na, ta, b, nb, tb, type, relativistic, halve};
  hipLaunchKernelGGL(loss_gan_kernel, dim3(1), dim3(LG_T), 0, (hipStream_t)stream, q, out);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_loss_gan_backward(const float* a, int64_t na, double ta, const float* b, int64_t nb, double tb, int32_t type,
                          int32_t relativistic, int32_t halve, const float* g, float* ga, float* gb, hcf_stream_t stream) {
  const int rc = gan_check(a, na, ta, b, nb, tb, type, relativistic, halve);
  if (rc != HCF_OK) return rc;
  if (!g || !al4(g) || (!ga && !gb) || (gb && !b) || !al4(ga) || !al4(gb)) return HCF_ERR_ARG;
  const GanArgs q = {a, na, ta, b, nb, tb, type, relativistic, halve};
  hipLaunchKernelGGL(loss_gan_bwd_kernel, dim3(1), dim3(LG_T), 0, (hipStream_t)stream, q, g, ga, gb);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
