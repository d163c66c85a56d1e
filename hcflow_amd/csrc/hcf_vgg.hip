// The memory-bound ops between the convolutions of the VGG19 perceptual loss of the HCFlow++ generator step
//   l_g_fea = l_fea_w * cri_fea(netF(fake_H), netF(real_H).detach())     (HCFlow_SR_model.py:229-232)
// with netF = VGGFeatureExtractor(feature_layer=34, use_bn=False) (discriminator_vgg_arch.py:130-157): input normalisation +
// NCHW -> NHWC, MaxPool2d(2, 2), the fused max-pool + ReLU backward, the ReLU backward of the layers no pool follows, and the
// L1 / MSE feature criterion with its gradient. hcflow_amd/gan.py: PerceptualLoss chains them with hcf_aux_conv2d /
// hcf_aux_conv2d_backward (hcf_aux.hip); nothing in this file launches a convolution.
//   activations: dense NHWC fp32 [B][H][W][cs], cs % 4 == 0, 16-byte aligned; a thread owns one float4 of channels, consecutive
//   threads walk the channel axis first (coalesced), every kernel is a grid-stride loop over a grid capped at VG_MAX_BLK blocks.
// All of them are selections or one or two roundings per element: no reduction except the criterion, which sums in fp64 through
// per-block partials of a shape-determined grid and one fixed-order final block (as hcf_bn.hip): bit-reproducible, no atomics.
#include <algorithm>
#include <cmath>

#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace {

constexpr int VG_T = 256;           // threads per block (4 waves)
constexpr int VG_MAX_BLK = 2048;    // blocks of an elementwise pass (8 per CU on 256 CUs)
constexpr int VG_MAX_PART = 1024;   // partial blocks of the criterion's reduction (fixed by n, never by the device)
constexpr int VG_PER_BLK = VG_T * 4 * 4;  // floats one partial block covers before the grid wraps (4 float4 per thread)

static inline bool vg_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int vg_grid(int64_t items) { return (int)std::min<int64_t>((items + VG_T - 1) / VG_T, VG_MAX_BLK); }

__device__ inline float vg_get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ inline void vg_set(float4& v, int k, float s) {
  if (k == 0) v.x = s; else if (k == 1) v.y = s; else if (k == 2) v.z = s; else v.w = s;
}

// ---- input normalisation: NCHW [B][3][HW] -> NHWC [B][HW][4]. One thread per pixel: three coalesced plane reads, one float4 store.
__global__ __launch_bounds__(VG_T) void vgg_input_norm_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ sd, int64_t HW, int64_t npix,
                                                              float* __restrict__ y) {
  float m[3] = {0.f, 0.f, 0.f}, s[3] = {1.f, 1.f, 1.f};
  const bool norm = mean != nullptr;
  if (norm) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { m[c] = mean[c]; s[c] = sd[c]; }
  }
  for (int64_t p = (int64_t)blockIdx.x * VG_T + threadIdx.x; p < npix; p += (int64_t)gridDim.x * VG_T) {
    const int64_t b = p / HW, r = p - b * HW;
    const float* src = x + b * 3 * HW + r;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = src[c * HW];
      if (norm) v[c] = (v[c] - m[c]) / s[c];             // the reference's two roundings (IEEE divide)
    }
    *reinterpret_cast<float4*>(y + p * 4) = make_float4(v[0], v[1], v[2], 0.f);
  }
}

__global__ __launch_bounds__(VG_T) void vgg_input_norm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ sd,
                                                                  int64_t HW, int64_t npix, float* __restrict__ dx) {
  float s[3] = {1.f, 1.f, 1.f};
  const bool norm = sd != nullptr;
  if (norm) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = sd[c];
  }
  for (int64_t p = (int64_t)blockIdx.x * VG_T + threadIdx.x; p < npix; p += (int64_t)gridDim.x * VG_T) {
    const int64_t b = p / HW, r = p - b * HW;
    const float4 v = *reinterpret_cast<const float4*>(g + p * 4);
    float* dst = dx + b * 3 * HW + r;
    dst[0] = norm ? v.x / s[0] : v.x;
    dst[HW] = norm ? v.y / s[1] : v.y;
    dst[2 * HW] = norm ? v.z / s[2] : v.z;
  }
}

struct PoolShape {
  int C, B, H, W, Hp, Wp;          // Hp = H / 2, Wp = W / 2 (floor)
};

// ---- MaxPool2d(2, 2) forward: one thread per (output pixel, float4 of channels)
__global__ __launch_bounds__(VG_T) void vgg_maxpool2_kernel(const float* __restrict__ x, int cs_x, PoolShape sh,
                                                            float* __restrict__ y, int cs_y) {
  const int ncol = cs_y >> 2;
  const int64_t items = (int64_t)sh.B * sh.Hp * sh.Wp * ncol;
  for (int64_t t = (int64_t)blockIdx.x * VG_T + threadIdx.x; t < items; t += (int64_t)gridDim.x * VG_T) {
    const int q = (int)(t % ncol);
    const int64_t pix = t / ncol;
    const int j = (int)(pix % sh.Wp);
    const int64_t bi = pix / sh.Wp;
    const int i = (int)(bi % sh.Hp);
    const int64_t b = bi / sh.Hp;
    const int c0 = 4 * q;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < sh.C) {
      const float* p00 = x + ((b * sh.H + 2 * i) * sh.W + 2 * j) * cs_x + c0;
      const float4 v0 = *reinterpret_cast<const float4*>(p00);
      const float4 v1 = *reinterpret_cast<const float4*>(p00 + cs_x);
      const float4 v2 = *reinterpret_cast<const float4*>(p00 + (int64_t)sh.W * cs_x);
      const float4 v3 = *reinterpret_cast<const float4*>(p00 + (int64_t)sh.W * cs_x + cs_x);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float m = vg_get(v0, k);
        const float a1 = vg_get(v1, k), a2 = vg_get(v2, k), a3 = vg_get(v3, k);
        if (a1 > m || a1 != a1) m = a1;                  // PyTorch: (val > maxval) || isnan(val)
        if (a2 > m || a2 != a2) m = a2;
        if (a3 > m || a3 != a3) m = a3;
        vg_set(o, k, c0 + k < sh.C ? m : 0.f);
      }
    }
    *reinterpret_cast<float4*>(y + pix * cs_y + c0) = o;
  }
}

// ---- fused MaxPool2d(2, 2) + activation backward: one thread per (2x2 window of the FULL H x W map, float4 of channels),
// windows counted over ceil(H/2) x ceil(W/2) so the odd last row / column gets its zeros from the same pass.
__global__ __launch_bounds__(VG_T) void vgg_maxpool2_act_bwd_kernel(const float* __restrict__ gp, int cs_gp,
                                                                    const float* __restrict__ y, int cs_y, PoolShape sh, int act,
                                                                    float* __restrict__ gpre, int cs_g) {
  const int ncol = cs_g >> 2;
  const int Hc = (sh.H + 1) >> 1, Wc = (sh.W + 1) >> 1;
  const int64_t items = (int64_t)sh.B * Hc * Wc * ncol;
  for (int64_t t = (int64_t)blockIdx.x * VG_T + threadIdx.x; t < items; t += (int64_t)gridDim.x * VG_T) {
    const int q = (int)(t % ncol);
    const int64_t win = t / ncol;
    const int j = (int)(win % Wc);
    const int64_t bi = win / Wc;
    const int i = (int)(bi % Hc);
    const int64_t b = bi / Hc;
    const int c0 = 4 * q;
    const bool row1 = 2 * i + 1 < sh.H, col1 = 2 * j + 1 < sh.W;   // the window's second row / column exists
    const int64_t o00 = (b * sh.H + 2 * i) * sh.W + 2 * j;           // pixel index of the window's corner
    float4 o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row1 && col1 && c0 < sh.C) {
      const float* p00 = y + o00 * cs_y + c0;
      float4 v[4];
      v[0] = *reinterpret_cast<const float4*>(p00);
      v[1] = *reinterpret_cast<const float4*>(p00 + cs_y);
      v[2] = *reinterpret_cast<const float4*>(p00 + (int64_t)sh.W * cs_y);
      v[3] = *reinterpret_cast<const float4*>(p00 + (int64_t)sh.W * cs_y + cs_y);
      const float4 g = *reinterpret_cast<const float4*>(gp + ((b * sh.Hp + i) * sh.Wp + j) * cs_gp + c0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float m = vg_get(v[0], k);
        int arg = 0;
#pragma unroll
        for (int e = 1; e < 4; ++e) {
          const float a = vg_get(v[e], k);
          if (a > m || a != a) { m = a; arg = e; }
        }
        const bool keep = c0 + k < sh.C && (act == 0 || m > 0.f);
        const float gk = keep ? vg_get(g, k) : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) vg_set(o[e], k, e == arg ? gk : 0.f);
      }
    }
    float* d00 = gpre + o00 * cs_g + c0;
    *reinterpret_cast<float4*>(d00) = o[0];
    if (col1) *reinterpret_cast<float4*>(d00 + cs_g) = o[1];
    if (row1) *reinterpret_cast<float4*>(d00 + (int64_t)sh.W * cs_g) = o[2];
    if (row1 && col1) *reinterpret_cast<float4*>(d00 + (int64_t)sh.W * cs_g + cs_g) = o[3];
  }
}

// ---- activation backward over a flat tensor: gpre = g * act'(y), in place allowed (each float4 is read before it is written)
__global__ __launch_bounds__(VG_T) void vgg_act_bwd_kernel(const float* g, const float* __restrict__ y, int act, int64_t n4,
                                                           float* gpre) {
  const float neg = act == 2 ? 0.2f : 0.f;
  for (int64_t t = (int64_t)blockIdx.x * VG_T + threadIdx.x; t < n4; t += (int64_t)gridDim.x * VG_T) {
    float4 v = *reinterpret_cast<const float4*>(g + 4 * t);
    if (act) {
      const float4 a = *reinterpret_cast<const float4*>(y + 4 * t);
      v.x *= a.x > 0.f ? 1.f : neg;
      v.y *= a.y > 0.f ? 1.f : neg;
      v.z *= a.z > 0.f ? 1.f : neg;
      v.w *= a.w > 0.f ? 1.f : neg;
    }
    *reinterpret_cast<float4*>(gpre + 4 * t) = v;
  }
}

// ---- feature criterion. One element: its fp64 term and its gradient (difference and scale in fp64, one rounding to fp32)
__device__ inline double loss_term(float a, float b, int kind, double inv_n, float* grad) {
  const double d = (double)a - (double)b;
  if (kind == 0) {
    if (grad) *grad = d > 0.0 ? (float)inv_n : d < 0.0 ? -(float)inv_n : (d == 0.0 ? 0.f : (float)d);   // NaN stays NaN
    return fabs(d);
  }
  if (grad) *grad = (float)(2.0 * d * inv_n);
  return d * d;
}

static inline int loss_nblk(int64_t n) { return (int)std::min<int64_t>((n + VG_PER_BLK - 1) / VG_PER_BLK, VG_MAX_PART); }

__global__ __launch_bounds__(VG_T) void vgg_loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                                int kind, double inv_n, float* __restrict__ grad,
                                                                double* __restrict__ part) {
  __shared__ double red[VG_T];
  const int64_t n4 = n >> 2;
  double s = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * VG_T + threadIdx.x; t < n4; t += (int64_t)gridDim.x * VG_T) {
    const float4 u = *reinterpret_cast<const float4*>(a + 4 * t);
    const float4 v = *reinterpret_cast<const float4*>(b + 4 * t);
    float4 gq;
    s += loss_term(u.x, v.x, kind, inv_n, grad ? &gq.x : nullptr);
    s += loss_term(u.y, v.y, kind, inv_n, grad ? &gq.y : nullptr);
    s += loss_term(u.z, v.z, kind, inv_n, grad ? &gq.z : nullptr);
    s += loss_term(u.w, v.w, kind, inv_n, grad ? &gq.w : nullptr);
    if (grad) *reinterpret_cast<float4*>(grad + 4 * t) = gq;
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * n4) {          // the <= 3 floats behind the last float4
    const int64_t i = 4 * n4 + threadIdx.x;
    s += loss_term(a[i], b[i], kind, inv_n, grad ? grad + i : nullptr);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = VG_T / 2; h > 0; h >>= 1) {                              // LDS tree of fixed shape
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(VG_T) void vgg_loss_final_kernel(const double* __restrict__ part, int nblk, double inv_n,
                                                              float* __restrict__ loss) {
  __shared__ double red[VG_T];
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += VG_T) s += part[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = VG_T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] * inv_n);
}

static int pool_check(const float* x, int cs_x, int C, int B, int H, int W) {
  if (!x || !vg_al16(x) || C < 1 || B < 1 || H < 1 || W < 1 || (cs_x & 3) || cs_x < C) return HCF_ERR_ARG;
  if ((int64_t)B * H * W > ((int64_t)1 << 40)) return HCF_ERR_SHAPE;   // 64-bit element offsets throughout
  return HCF_OK;
}

}  // namespace
}  // namespace hcf

using namespace hcf;

extern "C" {

int hcf_aux_input_norm(const float* x, const float* mean, const float* stdev, int32_t B, int32_t H, int32_t W, float* y,
                       hcf_stream_t stream) {
  if (!x || !y || !vg_al16(y) || B < 1 || H < 1 || W < 1 || (!mean != !stdev)) return HCF_ERR_ARG;
  const int64_t HW = (int64_t)H * W, npix = HW * B;
  hipLaunchKernelGGL(vgg_input_norm_kernel, dim3((unsigned)vg_grid(npix)), dim3(VG_T), 0, (hipStream_t)stream, x, mean, stdev, HW,
                     npix, y);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_aux_input_norm_backward(const float* g, const float* stdev, int32_t B, int32_t H, int32_t W, float* dx,
                                hcf_stream_t stream) {
  if (!g || !vg_al16(g) || !dx || B < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  const int64_t HW = (int64_t)H * W, npix = HW * B;
  hipLaunchKernelGGL(vgg_input_norm_bwd_kernel, dim3((unsigned)vg_grid(npix)), dim3(VG_T), 0, (hipStream_t)stream, g, stdev, HW,
                     npix, dx);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_aux_maxpool2(const float* x, int32_t cs_x, int32_t C, int32_t B, int32_t H, int32_t W, float* y, int32_t cs_y,
                     hcf_stream_t stream) {
  const int rc = pool_check(x, cs_x, C, B, H, W);
  if (rc != HCF_OK) return rc;
  if (!y || !vg_al16(y) || (cs_y & 3) || cs_y < C || H < 2 || W < 2) return HCF_ERR_ARG;
  const PoolShape sh = {C, B, H, W, H / 2, W / 2};
  const int64_t items = (int64_t)B * sh.Hp * sh.Wp * (cs_y / 4);
  hipLaunchKernelGGL(vgg_maxpool2_kernel, dim3((unsigned)vg_grid(items)), dim3(VG_T), 0, (hipStream_t)stream, x, cs_x, sh, y,
                     cs_y);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_aux_maxpool2_act_backward(const float* gp, int32_t cs_gp, const float* y, int32_t cs_y, int32_t C, int32_t B, int32_t H,
                                  int32_t W, int32_t act, float* gpre, int32_t cs_g, hcf_stream_t stream) {
  const int rc = pool_check(y, cs_y, C, B, H, W);
  if (rc != HCF_OK) return rc;
  if (!gp || !vg_al16(gp) || (cs_gp & 3) || cs_gp < C || !gpre || !vg_al16(gpre) || (cs_g & 3) || cs_g < C || H < 2 || W < 2 ||
      act < 0 || act > 1 || gpre == y || gpre == gp)
    return HCF_ERR_ARG;
  const PoolShape sh = {C, B, H, W, H / 2, W / 2};
  const int64_t items = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (cs_g / 4);
  hipLaunchKernelGGL(vgg_maxpool2_act_bwd_kernel, dim3((unsigned)vg_grid(items)), dim3(VG_T), 0, (hipStream_t)stream, gp, cs_gp, y,
                     cs_y, sh, act, gpre, cs_g);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_aux_act_backward(const float* g, const float* y, int32_t act, int64_t n, float* gpre, hcf_stream_t stream) {
  if (!g || !vg_al16(g) || !gpre || !vg_al16(gpre) || n < 4 || (n & 3) || act < 0 || act > 2 || (act && (!y || !vg_al16(y))))
    return HCF_ERR_ARG;
  hipLaunchKernelGGL(vgg_act_bwd_kernel, dim3((unsigned)vg_grid(n / 4)), dim3(VG_T), 0, (hipStream_t)stream, g, y, act, n / 4,
                     gpre);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

size_t hcf_aux_feature_loss_workspace(int64_t n) {
  if (n < 1) return 0;
  return ((size_t)loss_nblk(n) * sizeof(double) + 255) & ~(size_t)255;
}

int hcf_aux_feature_loss(const float* a, const float* b, int64_t n, int32_t kind, float* loss, float* grad, void* work,
                         size_t work_bytes, hcf_stream_t stream) {
  if (!a || !vg_al16(a) || !b || !vg_al16(b) || n < 1 || kind < 0 || kind > 1 || !loss || (grad && !vg_al16(grad)) || !work ||
      ((uintptr_t)work & 7))
    return HCF_ERR_ARG;
  if (work_bytes < hcf_aux_feature_loss_workspace(n)) return HCF_ERR_NOMEM;
  const int nblk = loss_nblk(n);
  const double inv_n = 1.0 / (double)n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vgg_loss_partial_kernel, dim3((unsigned)nblk), dim3(VG_T), 0, st, a, b, n, kind, inv_n, grad, (double*)work);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  hipLaunchKernelGGL(vgg_loss_final_kernel, dim3(1), dim3(VG_T), 0, st, (const double*)work, nblk, inv_n, loss);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
