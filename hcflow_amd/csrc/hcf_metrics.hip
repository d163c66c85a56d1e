// Streaming per-pixel statistics of a sample set on the device (hcf_metric_stats_*): the sample diversity
// of test_HCFlow.py without holding the samples. float64 arithmetic like the reference. The PSNR / SSIM / imresize entries of
// the same log line live in hcf_pair_metrics.hip.
#include <math.h>
#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace metrics {

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return (threadIdx.x == 0) ? sh[0] + sh[1] + sh[2] + sh[3] : 0.0;
}

// What test_HCFlow.py:127-131,165-167 gets from torch.cat(sr_img_list).std([0]) with all M samples held: here the state is one
// (mean, M2) pair of doubles per element, updated by Welford's recurrence as each sample arrives:
//   d = x - mean;  mean += d / n;  M2 += d * (x - mean)          (n = samples seen, this one included; n = 1: mean = x, M2 = 0)
// so a set of identical samples keeps mean == x and M2 == 0 exactly (d = 0), and mean lies between the old mean and x (rounding
// is monotonic), so every M2 increment is >= 0. Elementwise: 4 B in, one 16 B record in and out per element; nothing depends
// on the image an element belongs to.
__global__ __launch_bounds__(256) void stats_add_kernel(double2* state, const float* x, long long total, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double v = (double)x[i];
  double2 s;
  if (n == 1) {                                                  // the first sample defines the state: no clearing pass
    s.x = v; s.y = 0.0;
  } else {
    s = state[i];
    const double d = v - s.x;
    s.x += d / (double)n;
    s.y += d * (v - s.x);
  }
  state[i] = s;
}

#define HCF_STATS_EPT 4      // elements per thread of the finishing pass: one partial sum per 1024 elements of an image
// mean / unbiased std in the samples' own units as fp32, and per block the sum of 255 * std (fp64) in a fixed order: each
// thread adds its elements in index order, block_sum_d's tree joins the threads; partial[b][blockIdx.x]
__global__ __launch_bounds__(256) void stats_finish_kernel(const double2* state, long long per_image, long long n, float* mean,
                                                          float* sd, double* partial) {
  __shared__ double sh[4];
  const long long base = (long long)blockIdx.y * per_image;
  const long long i0 = (long long)blockIdx.x * (256 * HCF_STATS_EPT) + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < HCF_STATS_EPT; ++k) {
    const long long i = i0 + (long long)k * 256;
    if (i < per_image) {
      const double2 s = state[base + i];
      const double dev = n > 1 ? sqrt(s.y / (double)(n - 1)) : 0.0;
      mean[base + i] = (float)s.x;
      sd[base + i] = (float)dev;
      acc += 255.0 * dev;
    }
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// diversity[b] = sum of the image's partials / elements: one block per image, thread t adds partials t, t + 256, ... in order
__global__ __launch_bounds__(256) void stats_diversity_kernel(const double* partial, int nblk, long long per_image, double* out) {
  __shared__ double sh[4];
  const double* p = partial + (size_t)blockIdx.x * nblk;
  double acc = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) acc += p[j];
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = t / (double)per_image;
}

static inline long long stats_blocks(long long per_image) { return (per_image + 256 * HCF_STATS_EPT - 1) / (256 * HCF_STATS_EPT); }
// state layout: [B * 3HW] (mean, M2) records, then [B][blocks per image] partial sums of the finishing pass
static bool stats_layout(int B, int H, int W, long long& per_image, long long& nblk, size_t& bytes) {
  if (B < 1 || H < 1 || W < 1) return false;
  per_image = 3LL * H * W;
  nblk = stats_blocks(per_image);
  const long long total = (long long)B * per_image;
  if ((total + 255) / 256 > 0x7fffffffLL || nblk > 0x7fffffffLL || B > 65535) return false;
  bytes = (size_t)total * sizeof(double2) + (size_t)B * (size_t)nblk * sizeof(double);
  return true;
}

}  // namespace metrics
}  // namespace hcf

using namespace hcf;
using namespace hcf::metrics;

extern "C" {

size_t hcf_metric_stats_bytes(int32_t B, int32_t H, int32_t W) {
  long long per_image = 0, nblk = 0;
  size_t bytes = 0;
  return stats_layout(B, H, W, per_image, nblk, bytes) ? bytes : 0;
}

int hcf_metric_stats_add(void* state, size_t state_bytes, const float* x, int32_t B, int32_t H, int32_t W, int64_t n,
                         hcf_stream_t stream) {
  long long per_image = 0, nblk = 0;
  size_t bytes = 0;
  if (!state || !x || n < 1 || !stats_layout(B, H, W, per_image, nblk, bytes)) return HCF_ERR_ARG;
  if (state_bytes < bytes) return HCF_ERR_SHAPE;
  const long long total = (long long)B * per_image;
  hipLaunchKernelGGL(stats_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (double2*)state, x,
                     total, (long long)n);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_metric_stats_finish(void* state, size_t state_bytes, int32_t B, int32_t H, int32_t W, int64_t n, float* mean, float* std,
                            double* diversity, hcf_stream_t stream) {
  long long per_image = 0, nblk = 0;
  size_t bytes = 0;
  if (!state || !mean || !std || !diversity || n < 1 || !stats_layout(B, H, W, per_image, nblk, bytes)) return HCF_ERR_ARG;
  if (state_bytes < bytes) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)((char*)state + (size_t)B * per_image * sizeof(double2));
  hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st, (const double2*)state, per_image,
                     (long long)n, mean, std, partial);
  hipLaunchKernelGGL(stats_diversity_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)partial, (int)nblk, per_image,
                     diversity);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
