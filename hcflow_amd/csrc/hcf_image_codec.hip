// The 8-bit image boundary of a rescaling net used as a codec (downscale, store the LR as an 8-bit image, upscale later):
//
//   hcf_metric_quantize    x fp32 [B,3,H,W] RGB -> q = rint(clamp(x, 0, 1) * 255.f) / 255.f  (Basic.Quant.forward, Basic.py:186-202:
//                          the forward value of the reference's Quantization) and / or the same integers as the uint8 [B,H,W,3] BGR
//                          image util.tensor2img (utils/util.py:790-816) makes of x -- what hcf_metric_pair_compare's image_out holds.
//   hcf_metric_from_image  uint8 [B,H,W,3] BGR -> fp32 [B,3,H,W] RGB = float(u) / 255.f: what the reference's datasets make of a stored
//                          image (astype(np.float32) / 255., BGR -> RGB, HWC -> CHW).
//
// Both are memory-bound element-wise kernels. A thread owns the SAME pixels of all three planes (the image interleaves them), so every
// plane is read / written with consecutive lanes on consecutive addresses. Vec form: four pixels per thread -- one 16-byte access per
// plane and one 12-byte access of the image -- taken only when H * W is a multiple of 4 (every plane and image row of four then starts
// aligned) and the base addresses allow it; otherwise (odd planes, a batch slice of an odd-sized tensor, an offset view) the scalar
// form runs one pixel per thread over the whole tensor. Plain vector stores, no atomics, nothing allocated or synchronised.
//
// The divisions are IEEE fp32 divisions (the Makefile passes no fast-math flag, and hipcc's default keeps fp32 division correctly
// rounded): k / 255.f is bit for bit numpy's and torch's value, and a stored image is a fixed point of quantize(from_image(.)).
#include <stdint.h>
#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace imgq {

struct Word3 { unsigned a, b, c; };    // 12 bytes, 4-byte aligned: four BGR pixels

// one value: q and the integer it stands for, as torch.clamp's min(max(x, 0), 1) on the host: NaN stays NaN in q (its image byte is
// 0, as tensor2img's clamp makes it in hcf_metric_pair_compare); -0.0 passes the clamp and gives q = -0.0 (== 0, byte 0); +-inf
// clamp to 1 / 0
__device__ __forceinline__ float quant_unit(float x, unsigned& u) {
  const float v = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  const float r = rintf(v * 255.0f);                     // round half to even
  u = r == r ? (unsigned)r : 0u;
  return r / 255.0f;
}

__device__ __forceinline__ Word3 pack_bgr(const unsigned (&u)[3][4]) {   // u[c (R,G,B)][pixel] -> B G R B G R ...
  Word3 w;
  w.a = u[2][0] | (u[1][0] << 8) | (u[0][0] << 16) | (u[2][1] << 24);
  w.b = u[1][1] | (u[0][1] << 8) | (u[2][2] << 16) | (u[1][2] << 24);
  w.c = u[0][2] | (u[2][3] << 8) | (u[1][3] << 16) | (u[0][3] << 24);
  return w;
}

// blockIdx.y = image; thread i owns pixels [4 i, 4 i + 4) (Vec) or pixel i of its image
template <bool Vec>
__global__ __launch_bounds__(256) void quantize_kernel(const float* x, float* q, uint8_t* img, long long hw) {
  const long long n = Vec ? hw >> 2 : hw;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t b = blockIdx.y;
  const size_t plane0 = b * 3 * (size_t)hw;
  if constexpr (Vec) {
    unsigned u[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = plane0 + (size_t)c * hw + 4 * (size_t)i;
      const float4 f = *reinterpret_cast<const float4*>(x + o);
      float4 r;
      r.x = quant_unit(f.x, u[c][0]); r.y = quant_unit(f.y, u[c][1]); r.z = quant_unit(f.z, u[c][2]); r.w = quant_unit(f.w, u[c][3]);
      if (q) *reinterpret_cast<float4*>(q + o) = r;
    }
    if (img) *reinterpret_cast<Word3*>(img + (b * (size_t)hw + 4 * (size_t)i) * 3) = pack_bgr(u);
  } else {
    unsigned u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = plane0 + (size_t)c * hw + (size_t)i;
      const float r = quant_unit(x[o], u[c]);
      if (q) q[o] = r;
    }
    if (img) {
      uint8_t* o = img + (b * (size_t)hw + (size_t)i) * 3;
      o[0] = (uint8_t)u[2]; o[1] = (uint8_t)u[1]; o[2] = (uint8_t)u[0];
    }
  }
}

template <bool Vec>
__global__ __launch_bounds__(256) void from_image_kernel(const uint8_t* img, float* out, long long hw) {
  const long long n = Vec ? hw >> 2 : hw;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t b = blockIdx.y;
  const size_t plane0 = b * 3 * (size_t)hw;
  if constexpr (Vec) {
    const Word3 w = *reinterpret_cast<const Word3*>(img + (b * (size_t)hw + 4 * (size_t)i) * 3);
    const unsigned by[12] = {w.a & 255u, (w.a >> 8) & 255u, (w.a >> 16) & 255u, w.a >> 24, w.b & 255u, (w.b >> 8) & 255u,
                             (w.b >> 16) & 255u, w.b >> 24, w.c & 255u, (w.c >> 8) & 255u, (w.c >> 16) & 255u, w.c >> 24};
#pragma unroll
    for (int c = 0; c < 3; ++c) {                       // plane c (R, G, B) is byte 2 - c of every pixel
      float4 r;
      r.x = (float)by[2 - c] / 255.0f; r.y = (float)by[5 - c] / 255.0f; r.z = (float)by[8 - c] / 255.0f; r.w = (float)by[11 - c] / 255.0f;
      *reinterpret_cast<float4*>(out + plane0 + (size_t)c * hw + 4 * (size_t)i) = r;
    }
  } else {
    const uint8_t* p = img + (b * (size_t)hw + (size_t)i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[plane0 + (size_t)c * hw + (size_t)i] = (float)p[2 - c] / 255.0f;
  }
}

// B, H, W a launch can address: blockIdx.y = image, blockIdx.x = a block of 256 pixels (or quads)
static bool shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && (long long)H * W <= (1LL << 36);
}

static bool aligned(const void* p, uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace imgq
}  // namespace hcf

using namespace hcf::imgq;

extern "C" {

int hcf_metric_quantize(const float* x, int32_t B, int32_t H, int32_t W, float* q, uint8_t* image_out, hcf_stream_t stream) {
  if (!x || (!q && !image_out) || !shape_ok(B, H, W)) return HCF_ERR_ARG;
  const long long hw = (long long)H * W;
  const bool vec = (hw & 3) == 0 && aligned(x, 16) && aligned(q, 16) && aligned(image_out, 4);
  const long long n = vec ? hw >> 2 : hw;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(quantize_kernel<true>, grid, dim3(256), 0, st, x, q, image_out, hw);
  else hipLaunchKernelGGL(quantize_kernel<false>, grid, dim3(256), 0, st, x, q, image_out, hw);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_metric_from_image(const uint8_t* image, int32_t B, int32_t H, int32_t W, float* out, hcf_stream_t stream) {
  if (!image || !out || !shape_ok(B, H, W)) return HCF_ERR_ARG;
  const long long hw = (long long)H * W;
  const bool vec = (hw & 3) == 0 && aligned(image, 4) && aligned(out, 16);
  const long long n = vec ? hw >> 2 : hw;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(from_image_kernel<true>, grid, dim3(256), 0, st, image, out, hw);
  else hipLaunchKernelGGL(from_image_kernel<false>, grid, dim3(256), 0, st, image, out, hw);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
