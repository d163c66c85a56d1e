// The reference's SSIM (utils/util.py:914-955 ssim / calculate_ssim) as a differentiable criterion on the device, beside the
// criteria of hcf_loss.hip and by their rules: every term is fp64 from the fp32 inputs, every sum has a fixed order (per-block
// partials of a grid the shape alone decides plus ONE final block; no atomics, no tickets), a result is rounded to fp32 once.
// include/hcflow.h states the contract. Pixels are read one float per lane (rows are walked by consecutive lanes), so an address
// never decides which element meets which accumulator: any 4-byte aligned view gives the bits of an aligned copy.
//
//   forward   ssim_fwd_kernel: one block (256 threads) per 16 x 32 tile of window positions (top-left corners) of one plane. The
//             26 x 42 pixels under the tile's 11 x 11 windows are staged as fp64 in LDS; pass 1 filters the five moments
//             (x, y, x^2, y^2, xy) along the rows, pass 2 down the columns and evaluates S; the block's sum goes to its slot.
//             ssim_final_kernel: one block joins the slots of every plane, the planes of every sample and the samples.
//   backward  ssim_bwd_kernel: one block (512 threads) per 16 x 32 tile of PIXELS of one plane, recomputing from the inputs:
//             dS/dx_q = sum_p w(p - q) [A_p + 2 B_p x_q + C_p y_q],  A, B, C = dS_p / d(mu_x, E[x^2], E[xy]).
//             The tile needs the coefficient maps at 26 x 42 positions (+-5 pixels) and those the inputs at 36 x 52 pixels
//             (+-10): stage, filter the moments along rows then columns, evaluate the coefficients, filter them back by the
//             transposed window (columns of a row, then rows), combine with the pixel's own values, scale, round once. With both
//             gradients asked for there are four maps (B and C are shared), with one there are three.
//
// Identical inputs give S = 1.0 exactly: numerator and denominator of S are then products of equal bits, which is why this file
// forbids the compiler to contract a * b + c on its own (every fma below is written out) and keeps the two sides of S symmetric.
#include <algorithm>
#include <cmath>

#include "../../include/hcflow.h"
#include "hcf_common.h"
#include "hcf_ssim_window.h"

#pragma clang fp contract(off)

namespace hcf {
namespace {

constexpr int SS_TH = 16, SS_TW = 32;                    // tile: positions (forward) / pixels (backward)
constexpr int SS_FT = 256;                               // forward threads
constexpr int SS_FH = SS_TH + 10, SS_FW = SS_TW + 10;    // forward: staged pixels 26 x 42
constexpr int SS_BT = 512;                               // backward threads
constexpr int SS_PH = SS_TH + 10, SS_PW = SS_TW + 10;    // backward: positions 26 x 42
constexpr int SS_XH = SS_TH + 20, SS_XW = SS_TW + 20;    // backward: staged pixels 36 x 52
constexpr int SS_MAX_SIDE = 1 << 20;                     // H, W
constexpr int SS_MAX_PLANES = 65535;                     // gridDim.z

static inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// pixel `off` of a plane; Y_CH: the luma of the three planes `hw` apart (data/util.py:209-230 bgr2ycbcr(only_y=True) in units
// of the data range: yoff = 16 * data_range)
template <bool Y_CH>
__device__ __forceinline__ double ss_pixel(const float* __restrict__ p, size_t hw, size_t off, double yoff) {
  if (!Y_CH) return (double)p[off];
  const double r = (double)p[off], g = (double)p[off + hw], b = (double)p[off + 2 * hw];
  return fma(65.481, r, fma(128.553, g, fma(24.966, b, yoff))) / 255.0;
}

// the five moments of 11 consecutive pixels of a staged row
__device__ __forceinline__ void ss_row_moments(const double* __restrict__ a, const double* __restrict__ b, const Gauss11& gk,
                                               double* m) {
  m[0] = m[1] = m[2] = m[3] = m[4] = 0.0;
#pragma unroll
  for (int j = 0; j < 11; ++j) {
    const double u = a[j], t = b[j], w = gk.g[j];
    m[0] = fma(w, u, m[0]);
    m[1] = fma(w, t, m[1]);
    m[2] = fma(w, u * u, m[2]);
    m[3] = fma(w, t * t, m[3]);
    m[4] = fma(w, u * t, m[4]);
  }
}

// v = {mu_x, mu_y, E[x^2], E[y^2], E[xy]} -> the two factors of S as numerator / denominator pairs
__device__ __forceinline__ void ss_factors(const double* v, double C1, double C2, double& A1, double& A2, double& B1, double& B2) {
  const double mxx = v[0] * v[0], myy = v[1] * v[1], mxy = v[0] * v[1];
  A1 = 2.0 * mxy + C1;
  A2 = 2.0 * (v[4] - mxy) + C2;
  B1 = (mxx + myy) + C1;
  B2 = ((v[2] - mxx) + (v[3] - myy)) + C2;
}

// sum over the block's T threads: lanes by a shuffle tree, the waves in index order; every thread returns the total
template <int T>
__device__ __forceinline__ double ss_block_sum(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < T / 64; ++w) r += red[w];
  return r;
}

// grid (tiles x, tiles y, planes); part[plane][tile y][tile x] = the sum of S over the tile's valid positions
template <bool Y_CH>
__global__ __launch_bounds__(SS_FT) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                         Gauss11 gk, double C1, double C2, double yoff, double* __restrict__ part) {
  __shared__ double ta[SS_FH][SS_FW], tb[SS_FH][SS_FW];
  __shared__ double hm[5][SS_FH][SS_TW];
  __shared__ double red[SS_FT / 64];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * SS_TH, x0 = blockIdx.x * SS_TW;
  const size_t hw = (size_t)H * W;
  const size_t base = (size_t)blockIdx.z * (Y_CH ? 3 : 1) * hw;
  for (int i = tid; i < SS_FH * SS_FW; i += SS_FT) {
    const int r = i / SS_FW, c = i % SS_FW;
    const int py = y0 + r, px = x0 + c;
    double u = 0.0, t = 0.0;
    if (py < H && px < W) {
      const size_t off = base + (size_t)py * W + px;
      u = ss_pixel<Y_CH>(x, hw, off, yoff);
      t = ss_pixel<Y_CH>(y, hw, off, yoff);
    }
    ta[r][c] = u;
    tb[r][c] = t;
  }
  __syncthreads();
  for (int i = tid; i < SS_FH * SS_TW; i += SS_FT) {
    const int r = i / SS_TW, c = i % SS_TW;
    double m[5];
    ss_row_moments(&ta[r][c], &tb[r][c], gk, m);
#pragma unroll
    for (int k = 0; k < 5; ++k) hm[k][r][c] = m[k];
  }
  __syncthreads();
  double s = 0.0;
  for (int i = tid; i < SS_TH * SS_TW; i += SS_FT) {
    const int r = i / SS_TW, c = i % SS_TW;
    if (y0 + r > H - 11 || x0 + c > W - 11) continue;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 11; ++j) {
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] = fma(gk.g[j], hm[k][r + j][c], v[k]);
    }
    double A1, A2, B1, B2;
    ss_factors(v, C1, C2, A1, A2, B1, B2);
    s += (A1 * A2) / (B1 * B2);
  }
  s = ss_block_sum<SS_FT>(s, red);
  if (tid == 0) part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// One block. Wave w joins the `tiles` slots of planes w, w + 4, ...: lane l adds slots l, l + 64, ... in order, then a shuffle
// tree of fixed shape; the plane's mean = sum / nv. Thread t then joins the cn plane means of samples t, t + 256, ... in index
// order (a row depends on its own planes alone), thread 0 the samples in index order.
__global__ __launch_bounds__(SS_FT) void ssim_final_kernel(const double* __restrict__ part, int64_t B, int cn, int tiles, double nv,
                                                           double* __restrict__ plane_mean, double* __restrict__ vals,
                                                           float* __restrict__ rows, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t planes = B * cn;
  for (int64_t p = wave; p < planes; p += SS_FT / 64) {
    const double* pp = part + p * tiles;
    double s = 0.0;
    for (int k = lane; k < tiles; k += 64) s += pp[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) plane_mean[p] = s / nv;
  }
  __syncthreads();
  for (int64_t b = threadIdx.x; b < B; b += SS_FT) {
    double s = 0.0;
    for (int c = 0; c < cn; ++c) s += plane_mean[b * cn + c];
    const double v = s / (double)cn;
    vals[b] = v;
    rows[b] = (float)v;
  }
  __syncthreads();
  if (threadIdx.x == 0 && loss) {
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) s += vals[b];
    loss[0] = (float)(1.0 - s / (double)B);
  }
}

// grid (tiles x, tiles y, planes) over PIXELS. BOTH: gx and gy (four coefficient maps); else gx alone (three; the host swaps x
// and y for a lone gy: S is symmetric and so is every expression below). norm = scale / (planes per sample * positions).
template <bool Y_CH, bool BOTH>
__global__ __launch_bounds__(SS_BT) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int cn, int H,
                                                         int W, Gauss11 gk, double C1, double C2, double yoff,
                                                         const float* __restrict__ g, int g_stride, double norm,
                                                         float* __restrict__ gx, float* __restrict__ gy) {
  constexpr int NM = BOTH ? 4 : 3;                       // maps: B (d E[x^2] = d E[y^2]), C (d E[xy]), A_x (d mu_x), A_y (d mu_y)
  __shared__ double pa[SS_XH][SS_XW], pb[SS_XH][SS_XW];
  __shared__ double hm[5 * SS_XH * SS_PW];               // row-filtered moments [5][36][42]; later th [NM][26][32]
  __shared__ double cf[NM][SS_PH][SS_PW];
  const int tid = threadIdx.x;
  const int oy0 = blockIdx.y * SS_TH, ox0 = blockIdx.x * SS_TW;
  const size_t hw = (size_t)H * W;
  const size_t base = (size_t)blockIdx.z * (Y_CH ? 3 : 1) * hw;
  const float gb = g[g_stride ? (size_t)(blockIdx.z / (unsigned)cn) : 0];
  if (gb == 0.f) {                                       // block-uniform: a dropped sample gets exact zeros whatever its pixels are
    const int r = tid / SS_TW, c = tid % SS_TW;
    if (oy0 + r < H && ox0 + c < W) {
      const size_t off = base + (size_t)(oy0 + r) * W + (ox0 + c);
#pragma unroll
      for (int k = 0; k < (Y_CH ? 3 : 1); ++k) {
        if (gx) gx[off + k * hw] = 0.f;
        if (BOTH && gy) gy[off + k * hw] = 0.f;
      }
    }
    return;
  }
  for (int i = tid; i < SS_XH * SS_XW; i += SS_BT) {
    const int r = i / SS_XW, c = i % SS_XW;
    const int py = oy0 - 10 + r, px = ox0 - 10 + c;
    double u = 0.0, t = 0.0;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const size_t off = base + (size_t)py * W + px;
      u = ss_pixel<Y_CH>(x, hw, off, yoff);
      t = ss_pixel<Y_CH>(y, hw, off, yoff);
    }
    pa[r][c] = u;
    pb[r][c] = t;
  }
  __syncthreads();
  for (int i = tid; i < SS_XH * SS_PW; i += SS_BT) {
    const int r = i / SS_PW, c = i % SS_PW;
    double m[5];
    ss_row_moments(&pa[r][c], &pb[r][c], gk, m);
#pragma unroll
    for (int k = 0; k < 5; ++k) hm[(k * SS_XH + r) * SS_PW + c] = m[k];
  }
  __syncthreads();
  for (int i = tid; i < SS_PH * SS_PW; i += SS_BT) {
    const int r = i / SS_PW, c = i % SS_PW;
    const int py = oy0 - 10 + r, px = ox0 - 10 + c;
    double cB = 0.0, cC = 0.0, cAx = 0.0, cAy = 0.0;
    if (py >= 0 && py <= H - 11 && px >= 0 && px <= W - 11) {      // a position outside the map contributes nothing
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < 11; ++j) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = fma(gk.g[j], hm[(k * SS_XH + r + j) * SS_PW + c], v[k]);
      }
      double A1, A2, B1, B2;
      ss_factors(v, C1, C2, A1, A2, B1, B2);
      const double r1 = A1 / B1, r2 = A2 / B2, i1 = 1.0 / B1, i2 = 1.0 / B2;
      cB = -(r1 * r2) * i2;
      cC = 2.0 * r1 * i2;
      cAx = 2.0 * (r2 * (v[1] - r1 * v[0]) * i1 + r1 * (r2 * v[0] - v[1]) * i2);
      cAy = 2.0 * (r2 * (v[0] - r1 * v[1]) * i1 + r1 * (r2 * v[1] - v[0]) * i2);
    }
    cf[0][r][c] = cB;
    cf[1][r][c] = cC;
    cf[2][r][c] = cAx;
    if (BOTH) cf[NM - 1][r][c] = cAy;
  }
  __syncthreads();                                       // hm is free: the transposed row pass writes th over it
  double* th = hm;                                       // [NM][SS_PH][SS_TW]
  for (int i = tid; i < NM * SS_PH * SS_TW; i += SS_BT) {
    const int k = i / (SS_PH * SS_TW), r = (i / SS_TW) % SS_PH, c = i % SS_TW;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) s = fma(gk.g[j], cf[k][r][c + 10 - j], s);   // pixel column ox0 + c lies j right of position c + 10 - j
    th[i] = s;
  }
  __syncthreads();
  {
    const int r = tid / SS_TW, c = tid % SS_TW;          // SS_BT threads = the tile's SS_TH x SS_TW pixels
    if (oy0 + r < H && ox0 + c < W) {
      double F[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 11; ++j) s = fma(gk.g[j], th[(k * SS_PH + r + 10 - j) * SS_TW + c], s);
        F[k] = s;
      }
      const double xq = pa[r + 10][c + 10], yq = pb[r + 10][c + 10];
      const double f = (double)gb * norm;
      const size_t off = base + (size_t)(oy0 + r) * W + (ox0 + c);
      // two rounded products, then the sums: for identical inputs C = -2 B bit for bit at every position, so the products
      // cancel exactly and, A being 0 there, the gradient is an exact zero
      const double dx = f * (((2.0 * xq) * F[0] + yq * F[1]) + F[2]);
      const double dy = BOTH ? f * (((2.0 * yq) * F[0] + xq * F[1]) + F[NM - 1]) : 0.0;
      if (Y_CH) {
        const double wc[3] = {65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (gx) gx[off + k * hw] = (float)(dx * wc[k]);
          if (BOTH && gy) gy[off + k * hw] = (float)(dy * wc[k]);
        }
      } else {
        if (gx) gx[off] = (float)dx;
        if (BOTH && gy) gy[off] = (float)dy;
      }
    }
  }
}

static_assert(SS_BT == SS_TH * SS_TW, "the backward's last pass gives one pixel to each thread");
static_assert(5 * SS_XH * SS_PW >= 4 * SS_PH * SS_TW, "th fits into hm");

struct SsimShape {
  int cn = 0;                 // planes per sample
  int64_t planes = 0;
  int ftx = 0, fty = 0;       // forward tiles (over positions)
  int btx = 0, bty = 0;       // backward tiles (over pixels)
  double nv = 0;              // positions per plane
};

static int ssim_shape(int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel, double data_range, SsimShape* s) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || y_channel < 0 || y_channel > 1 || !(data_range > 0.0) || !std::isfinite(data_range))
    return HCF_ERR_ARG;
  if (H < 11 || W < 11 || (y_channel && C != 3) || H > SS_MAX_SIDE || W > SS_MAX_SIDE) return HCF_ERR_SHAPE;
  s->cn = y_channel ? 1 : C;
  if (B > SS_MAX_PLANES / s->cn) return HCF_ERR_SHAPE;
  s->planes = B * s->cn;
  s->ftx = (W - 10 + SS_TW - 1) / SS_TW;
  s->fty = (H - 10 + SS_TH - 1) / SS_TH;
  s->btx = (W + SS_TW - 1) / SS_TW;
  s->bty = (H + SS_TH - 1) / SS_TH;
  if (s->bty > 65535 || (int64_t)s->ftx * s->fty > (int64_t)1 << 30) return HCF_ERR_SHAPE;
  s->nv = (double)(H - 10) * (double)(W - 10);
  return HCF_OK;
}

static size_t ssim_work_bytes(const SsimShape& s, int64_t B) {
  const size_t doubles = (size_t)s.planes * s.ftx * s.fty + (size_t)s.planes + (size_t)B;
  return (doubles * sizeof(double) + 255) & ~(size_t)255;
}

}  // namespace
}  // namespace hcf

using namespace hcf;

extern "C" {

size_t hcf_loss_ssim_workspace(int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel) {
  SsimShape s;
  if (ssim_shape(B, C, H, W, y_channel, 1.0, &s) != HCF_OK) return 0;
  return ssim_work_bytes(s, B);
}

int hcf_loss_ssim(const float* x, const float* y, int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel, double data_range,
                  float* out_rows, float* out_loss, void* work, size_t work_bytes, hcf_stream_t stream) {
  SsimShape s;
  if (!x || !y || !out_rows || !work || !al4(x) || !al4(y) || !al4(out_rows) || !al4(out_loss) || ((uintptr_t)work & 7))
    return HCF_ERR_ARG;
  const int rc = ssim_shape(B, C, H, W, y_channel, data_range, &s);
  if (rc != HCF_OK) return rc;
  if (work_bytes < ssim_work_bytes(s, B)) return HCF_ERR_NOMEM;
  const int tiles = s.ftx * s.fty;
  double* part = (double*)work;
  double* plane_mean = part + (size_t)s.planes * tiles;
  double* vals = plane_mean + s.planes;
  const Gauss11 gk = gauss11();
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const double yoff = 16.0 * data_range;
  const dim3 grid((unsigned)s.ftx, (unsigned)s.fty, (unsigned)s.planes);
  hipStream_t st = (hipStream_t)stream;
  if (y_channel) hipLaunchKernelGGL(ssim_fwd_kernel<true>, grid, dim3(SS_FT), 0, st, x, y, H, W, gk, C1, C2, yoff, part);
  else hipLaunchKernelGGL(ssim_fwd_kernel<false>, grid, dim3(SS_FT), 0, st, x, y, H, W, gk, C1, C2, yoff, part);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(SS_FT), 0, st, (const double*)part, B, s.cn, tiles, s.nv, plane_mean, vals,
                     out_rows, out_loss);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_loss_ssim_backward(const float* x, const float* y, int64_t B, int32_t C, int32_t H, int32_t W, int32_t y_channel,
                           double data_range, const float* g, int32_t g_stride, double scale, float* gx, float* gy,
                           hcf_stream_t stream) {
  SsimShape s;
  if (!x || !y || !g || (!gx && !gy) || !al4(x) || !al4(y) || !al4(g) || !al4(gx) || !al4(gy) || g_stride < 0 || g_stride > 1 ||
      !std::isfinite(scale))
    return HCF_ERR_ARG;
  const int rc = ssim_shape(B, C, H, W, y_channel, data_range, &s);
  if (rc != HCF_OK) return rc;
  const Gauss11 gk = gauss11();
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const double yoff = 16.0 * data_range;
  const double norm = scale / ((double)s.cn * s.nv);
  const dim3 grid((unsigned)s.btx, (unsigned)s.bty, (unsigned)s.planes);
  hipStream_t st = (hipStream_t)stream;
  if (gx && gy) {
    if (y_channel)
      hipLaunchKernelGGL((ssim_bwd_kernel<true, true>), grid, dim3(SS_BT), 0, st, x, y, s.cn, H, W, gk, C1, C2, yoff, g, g_stride, norm,
                         gx, gy);
    else
      hipLaunchKernelGGL((ssim_bwd_kernel<false, true>), grid, dim3(SS_BT), 0, st, x, y, s.cn, H, W, gk, C1, C2, yoff, g, g_stride, norm,
                         gx, gy);
  } else {
    const float* a = gx ? x : y;                         // a lone gy is the gx of the exchanged pair
    const float* b = gx ? y : x;
    float* ga = gx ? gx : gy;
    if (y_channel)
      hipLaunchKernelGGL((ssim_bwd_kernel<true, false>), grid, dim3(SS_BT), 0, st, a, b, s.cn, H, W, gk, C1, C2, yoff, g, g_stride, norm,
                         ga, (float*)nullptr);
    else
      hipLaunchKernelGGL((ssim_bwd_kernel<false, false>), grid, dim3(SS_BT), 0, st, a, b, s.cn, H, W, gk, C1, C2, yoff, g, g_stride,
                         norm, ga, (float*)nullptr);
  }
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
