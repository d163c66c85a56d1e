// Device-side training batches: the reference's GT_dataset.__getitem__ (codes/data/GT_dataset.py:79-118, train phase) on images
// that already live in HBM as packed HWC uint8 -- crop, augment (flip / flip / transpose), BGR -> RGB, HWC -> CHW, uint8 -> float
// and the MATLAB-style antialiased bicubic LR (data/util.py:407-474, imresize_np of the WHOLE image) of the crop, one launch per
// batch. Contract and index rules: include/hcflow.h (hcf_data_prepare_batch); layout and LDS banks: DESIGN.md section 7.
//
// One block owns an 8 x 32 tile of a sample's LR crop (coordinates BEFORE the augment, which is an index map of the stores):
//   H pass  global uint8 -> LDS fp32 [channel][tile row][window column]: consecutive lanes read consecutive bytes of a source row
//           (HWC: column-major over (column, channel)), each over the 4 S live taps of the source rows;
//   W pass  LDS -> LR output, the reflection in W being the window column's source column (the H result of the reflected column
//           IS the reflected H result);
//   GT      the (8 S) x (32 S) source pixels of the tile, uint8 / 255.f, stored through the same index map.
// Every output value is one fixed chain of fmaf over the taps in tap order, whatever tile or sample it lands in: a crop is
// bit-identical to the same window of the whole image.
//
// Paired banks (hcf_data_prepare_paired: LRHR_PKL_dataset.py:96-135, GTLQnpy_dataset.py:42-78, GTLQx_dataset.py:82-122) keep the LQ
// images as data beside the HR images: prepare_paired_kernel is the GT copy above for both halves, LQ at scale 1, no taps, no LDS.
// Both entries share the host side: check_geometry, check_table, check_crops and launch_chunks.
#include <math.h>
#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
namespace data {

constexpr int kTH = 8, kTW = 32;                 // LR tile
constexpr int kMaxTaps = 4 * 8 + 2;

struct Sample { long long off; int H, W, top, left, flags, pad; };      // flags: bit 0 hflip, 1 vflip, 2 rot90

struct Args {
  const uint8_t* bank;
  float* gt;               // first sample of this launch, or nullptr
  float* lq;
  int lr_h, lr_w, bgr, tiles_x;
  float w[kMaxTaps];       // tap k of every output pixel (taps 0 and P - 1, for odd scales also P - 2, are zero)
  Sample s[HCF_DATA_LAUNCH_BATCH];
};
static_assert(sizeof(Args) <= 4096, "the records travel in the kernel argument block");

template <int S> struct Geo {
  static constexpr int P = 4 * S + 2;
  static constexpr int C0 = S - 1 - (5 * S) / 2;           // S - 1 + floor(0.5 - 2.5 S)
  static constexpr int WC = (kTW - 1) * S + P;             // window columns of a full tile
  // row pitch = 1 mod 32: the W pass reads with R = gcd(S, 32) tile rows across the lanes (bank = row + S * column: 32 distinct)
  static constexpr int RP = (WC + 30) / 32 * 32 + 1;
  // channel pitch = 11 mod 32: the H pass writes 32 consecutive (column, channel) pairs = 11 columns of 3 planes, 11 banks apart
  static constexpr int CP = kTH * RP + 3;
  static constexpr int R = S & -S;
};

__device__ __forceinline__ int reflect_clamp(int i, int n) {
  i = i < 0 ? -i - 1 : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

template <int S>
__global__ __launch_bounds__(256) void prepare_batch_kernel(const Args a) {
  using G = Geo<S>;
  __shared__ float tile[3 * G::CP];
  const Sample sm = a.s[blockIdx.y];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * kTH, x0 = tx * kTW;                   // tile origin in the crop's LR grid
  const int th = min(kTH, a.lr_h - y0), tw = min(kTW, a.lr_w - x0);
  const uint8_t* img = a.bank + sm.off;
  const size_t pitch = (size_t)sm.W * 3;
  const int hf = sm.flags & 1, vf = (sm.flags >> 1) & 1, rot = (sm.flags >> 2) & 1;
  const int t = threadIdx.x;

  if (a.lq) {
    const int wc3 = ((tw - 1) * S + G::P) * 3;
    const int gx0 = (sm.left + x0) * S + G::C0, gy0 = (sm.top + y0) * S + G::C0;
    // two tile rows per step: their taps share 3 S of the 5 S source rows, and all 5 S loads are in flight before the first use
    // (one row per step left the block waiting out one memory latency per row with 4 taps' worth of bytes in flight)
    for (int r = 0; r < th; r += 2) {
      for (int j = t; j < wc3; j += 256) {
        const int col = j / 3, c = j - col * 3;
        const uint8_t* p = img + (size_t)reflect_clamp(gx0 + col, sm.W) * 3 + c;
        uint8_t b[5 * S];
#pragma unroll
        for (int m = 0; m < 5 * S; ++m) b[m] = p[(size_t)reflect_clamp(gy0 + r * S + 1 + m, sm.H) * pitch];
        float v[5 * S];
#pragma unroll
        for (int m = 0; m < 5 * S; ++m) v[m] = (float)b[m] / 255.f;
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int k = 1; k <= 4 * S; ++k) {
          acc0 = fmaf(a.w[k], v[k - 1], acc0);
          acc1 = fmaf(a.w[k], v[S + k - 1], acc1);
        }
        tile[c * G::CP + r * G::RP + col] = acc0;
        tile[c * G::CP + (r + 1) * G::RP + col] = acc1;      // r + 1 <= 7; a row past th is never read
      }
    }
    __syncthreads();
    float* out = a.lq + (size_t)blockIdx.y * 3 * a.lr_h * a.lr_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int rl = t % G::R, x = (t / G::R) % kTW, r = t / (G::R * kTW) * G::R + rl;
      if (r < th && x < tw) {
        const float* q = tile + c * G::CP + r * G::RP + x * S;
        float acc = 0.f;
#pragma unroll
        for (int k = 1; k <= 4 * S; ++k) acc = fmaf(a.w[k], q[k], acc);
        int y = y0 + r, xx = x0 + x;
        if (hf) xx = a.lr_w - 1 - xx;
        if (vf) y = a.lr_h - 1 - y;
        const size_t o = rot ? (size_t)xx * a.lr_h + y : (size_t)y * a.lr_w + xx;
        out[(size_t)(a.bgr ? 2 - c : c) * a.lr_h * a.lr_w + o] = acc;
      }
    }
  }

  if (a.gt) {
    const int gh = a.lr_h * S, gw = a.lr_w * S;
    const size_t plane = (size_t)gh * gw;
    float* out = a.gt + (size_t)blockIdx.y * 3 * plane;
    const int w3 = tw * S * 3;
    constexpr int U = 8;                                     // source rows per step: U loads in flight per lane, then U stores
    for (int r0 = 0; r0 < th * S; r0 += U) {
      for (int j = t; j < w3; j += 256) {
        const int col = j / 3, c = j - col * 3;
        const int cx = x0 * S + col;                           // column in the crop
        const uint8_t* p = img + (size_t)min(max(sm.left * S + cx, 0), sm.W - 1) * 3 + c;
        uint8_t b[U];
#pragma unroll
        for (int u = 0; u < U; ++u)                            // rows past the tile are clamped into the image and dropped below
          b[u] = p[(size_t)min(max((sm.top + y0) * S + r0 + u, 0), sm.H - 1) * pitch];
        const int x = hf ? gw - 1 - cx : cx;
        float* q = out + (size_t)(a.bgr ? 2 - c : c) * plane;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int cy = y0 * S + r0 + u;                      // row in the crop
          const int y = vf ? gh - 1 - cy : cy;
          if (r0 + u < th * S) q[rot ? (size_t)x * gh + y : (size_t)y * gw + x] = (float)b[u] / 255.f;
        }
      }
    }
  }
}

static double cubic(double x) {
  const double ax = fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
  if (ax <= 1.0) return 1.5 * ax3 - 2.5 * ax2 + 1.0;
  if (ax <= 2.0) return -0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0;
  return 0.0;
}

// calculate_weights_indices (data/util.py:283-335) for the factor 1 / S: u - left = 0.5 - 0.5 S - floor(0.5 - 2.5 S) for every
// output pixel, weight k = cubic((u - left - k) / S) / S, normalised to sum 1
static void tap_weights(int S, float* w) {
  const int P = 4 * S + 2;
  const double d0 = 0.5 - 0.5 * S + (double)((5 * S) / 2);
  double v[kMaxTaps], sum = 0.0;
  for (int k = 0; k < P; ++k) { v[k] = cubic((d0 - k) / S) / S; sum += v[k]; }
  for (int k = 0; k < kMaxTaps; ++k) w[k] = k < P ? (float)(v[k] / sum) : 0.f;
}

// ---- paired banks (LRHR_PKL, GTLQ / GTLQnpy / GTLQx): the LQ image is data of its own, not a function of the HR image ----
struct PairSample { long long gt_off, lq_off; int gt_h, gt_w, lq_h, lq_w, top, left, flags, pad; };

struct PairArgs {
  const uint8_t* gt_bank;
  const uint8_t* lq_bank;
  float* gt;               // first sample of this launch, or nullptr
  float* lq;
  int lr_h, lr_w, scale, bgr, tiles_x, pad;
  PairSample s[HCF_DATA_LAUNCH_BATCH];
};
static_assert(sizeof(PairArgs) <= 4096, "the records travel in the kernel argument block");

// The rows x cols window of an H x W HWC image at (top + cy0, left + cx0) -> the (cy0, cx0) corner of a crop of ch x cw pixels in
// `out` (3 planes of ch * cw), uint8 / 255.f, through the augment's index map. Consecutive lanes read consecutive bytes of a
// source row; U rows are in flight per lane before the first store. Every source index is clamped into the image.
template <int U>
__device__ __forceinline__ void copy_window(const uint8_t* img, int H, int W, int top, int left, int cy0, int cx0, int rows,
                                            int cols, int ch, int cw, int flags, int bgr, float* out) {
  const size_t pitch = (size_t)W * 3, plane = (size_t)ch * cw;
  const int hf = flags & 1, vf = (flags >> 1) & 1, rot = (flags >> 2) & 1;
  const int w3 = cols * 3;
  for (int r0 = 0; r0 < rows; r0 += U) {
    for (int j = threadIdx.x; j < w3; j += 256) {
      const int col = j / 3, c = j - col * 3;
      const int cx = cx0 + col;                                // column in the crop
      const uint8_t* p = img + (size_t)min(max(left + cx, 0), W - 1) * 3 + c;
      uint8_t b[U];
#pragma unroll
      for (int u = 0; u < U; ++u)                              // rows past the tile are clamped into the image and dropped below
        b[u] = p[(size_t)min(max(top + cy0 + r0 + u, 0), H - 1) * pitch];
      const int x = hf ? cw - 1 - cx : cx;
      float* q = out + (size_t)(bgr ? 2 - c : c) * plane;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int cy = cy0 + r0 + u;                           // row in the crop
        const int y = vf ? ch - 1 - cy : cy;
        if (r0 + u < rows) q[rot ? (size_t)x * ch + y : (size_t)y * cw + x] = (float)b[u] / 255.f;
      }
    }
  }
}

// One block owns an 8 x 32 tile of a sample's LQ crop and the (8 scale) x (32 scale) HR pixels above it. No taps: scale is a
// runtime argument. Rows in flight: the LQ tile has 8; for GT 16 measured 2 % under 8 and 32 no better.
__global__ __launch_bounds__(256) void prepare_paired_kernel(const PairArgs a) {
  const PairSample sm = a.s[blockIdx.y];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * kTH, x0 = tx * kTW;                     // tile origin in the crop's LQ grid
  const int th = min(kTH, a.lr_h - y0), tw = min(kTW, a.lr_w - x0);
  const int S = a.scale;
  if (a.lq)
    copy_window<8>(a.lq_bank + sm.lq_off, sm.lq_h, sm.lq_w, sm.top, sm.left, y0, x0, th, tw, a.lr_h, a.lr_w, sm.flags, a.bgr,
                a.lq + (size_t)blockIdx.y * 3 * a.lr_h * a.lr_w);
  if (a.gt)
    copy_window<16>(a.gt_bank + sm.gt_off, sm.gt_h, sm.gt_w, sm.top * S, sm.left * S, y0 * S, x0 * S, th * S, tw * S, a.lr_h * S,
                a.lr_w * S, sm.flags, a.bgr, a.gt + (size_t)blockIdx.y * 3 * a.lr_h * S * a.lr_w * S);
}

typedef void (*Kernel)(const Args);
static Kernel kernel_of(int S) {
  switch (S) {
    case 2: return prepare_batch_kernel<2>;
    case 3: return prepare_batch_kernel<3>;
    case 4: return prepare_batch_kernel<4>;
    case 5: return prepare_batch_kernel<5>;
    case 6: return prepare_batch_kernel<6>;
    case 7: return prepare_batch_kernel<7>;
    case 8: return prepare_batch_kernel<8>;
  }
  return nullptr;
}

// ---- the host side of both entries. Every record is checked before any HIP call: the kernels read what these tables say ----
static int check_geometry(int scale, int n_images, int B, int lr_h, int lr_w) {
  if (scale < 2 || scale > 8 || n_images < 1 || B < 0 || lr_h < 1 || lr_w < 1) return HCF_ERR_ARG;
  if (lr_h > (1 << 20) || lr_w > (1 << 20)) return HCF_ERR_ARG;
  return HCF_OK;
}

// {byte offset, H, W} rows of one bank's host table; an image with a side below min_side is HCF_ERR_SHAPE
static int check_table(const int64_t* images, int n_images, size_t bank_bytes, int min_side) {
  for (int i = 0; i < n_images; ++i) {
    const int64_t off = images[3 * i], H = images[3 * i + 1], W = images[3 * i + 2];
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || off < 0) return HCF_ERR_ARG;
    if (H < min_side || W < min_side) return HCF_ERR_SHAPE;
    if ((uint64_t)off > bank_bytes || (uint64_t)(3 * H * W) > bank_bytes - (uint64_t)off) return HCF_ERR_ARG;
  }
  return HCF_OK;
}

// {image, top, left, hflip, vflip, rot90} rows; a window of lr_h x lr_w crop pixels is (lr_h unit) x (lr_w unit) pixels of the
// table that bounds it: unit = scale on the HR table of the single bank, 1 on the LQ table of the paired banks
static int check_crops(const int32_t* crops, int B, const int64_t* images, int n_images, int lr_h, int lr_w, int unit) {
  for (int b = 0; b < B; ++b) {
    const int32_t* c = crops + 6 * b;
    if (c[0] < 0 || c[0] >= n_images || c[1] < 0 || c[2] < 0) return HCF_ERR_ARG;
    for (int f = 3; f < 6; ++f)
      if (c[f] != 0 && c[f] != 1) return HCF_ERR_ARG;
    if (c[5] && lr_h != lr_w) return HCF_ERR_ARG;
    const int64_t H = images[3 * c[0] + 1], W = images[3 * c[0] + 2];
    if (((int64_t)c[1] + lr_h) * unit > H || ((int64_t)c[2] + lr_w) * unit > W) return HCF_ERR_ARG;
  }
  return HCF_OK;
}

// The launches of one batch, at most HCF_DATA_LAUNCH_BATCH records each: `a` arrives with its banks (and taps) set, image(s, c)
// fills record s with the table rows of crop row c.
template <class A, class Image>
static int launch_chunks(void (*kernel)(const A), A& a, const int32_t* crops, int B, int lr_h, int lr_w, int scale, int bgr,
                         float* gt, float* lq, hcf_stream_t stream, Image image) {
  if (B == 0) return HCF_OK;
  a.lr_h = lr_h; a.lr_w = lr_w; a.bgr = bgr ? 1 : 0;
  a.tiles_x = (lr_w + kTW - 1) / kTW;
  const long long tiles = (long long)a.tiles_x * ((lr_h + kTH - 1) / kTH);
  if (tiles > 0x7fffffffLL) return HCF_ERR_ARG;
  const size_t lq_n = (size_t)3 * lr_h * lr_w, gt_n = lq_n * scale * scale;
  for (int b0 = 0; b0 < B; b0 += HCF_DATA_LAUNCH_BATCH) {
    const int nb = B - b0 < HCF_DATA_LAUNCH_BATCH ? B - b0 : HCF_DATA_LAUNCH_BATCH;
    for (int i = 0; i < HCF_DATA_LAUNCH_BATCH; ++i) {
      const int32_t* c = crops + 6 * (size_t)(b0 + (i < nb ? i : 0));      // unused slots repeat a valid record
      image(a.s[i], c);
      a.s[i].top = c[1]; a.s[i].left = c[2]; a.s[i].flags = c[3] | (c[4] << 1) | (c[5] << 2); a.s[i].pad = 0;
    }
    a.gt = gt ? gt + (size_t)b0 * gt_n : nullptr;
    a.lq = lq ? lq + (size_t)b0 * lq_n : nullptr;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  }
  return HCF_OK;
}

}  // namespace data
}  // namespace hcf

extern "C" {

int hcf_data_prepare_batch(const uint8_t* bank, size_t bank_bytes, const int64_t* images, int32_t n_images, const int32_t* crops,
                           int32_t B, int32_t lr_h, int32_t lr_w, int32_t scale, int32_t bgr, float* gt, float* lq,
                           hcf_stream_t stream) {
  using namespace hcf::data;
  if (!bank || !images || !crops || (!gt && !lq)) return HCF_ERR_ARG;
  int rc = check_geometry(scale, n_images, B, lr_h, lr_w);
  if (rc == HCF_OK) rc = check_table(images, n_images, bank_bytes, 4 * scale);      // below 4 * scale one reflection does not reach
  if (rc == HCF_OK) rc = check_crops(crops, B, images, n_images, lr_h, lr_w, scale);
  if (rc != HCF_OK) return rc;

  Args a;
  a.bank = bank;
  tap_weights(scale, a.w);
  return launch_chunks(kernel_of(scale), a, crops, B, lr_h, lr_w, scale, bgr, gt, lq, stream, [&](Sample& s, const int32_t* c) {
    s.off = images[3 * c[0]]; s.H = (int)images[3 * c[0] + 1]; s.W = (int)images[3 * c[0] + 2];
  });
}

int hcf_data_prepare_paired(const uint8_t* gt_bank, size_t gt_bytes, const int64_t* gt_images, const uint8_t* lq_bank,
                            size_t lq_bytes, const int64_t* lq_images, int32_t n_images, const int32_t* crops, int32_t B,
                            int32_t lr_h, int32_t lr_w, int32_t scale, int32_t bgr, float* gt, float* lq, hcf_stream_t stream) {
  using namespace hcf::data;
  if (!gt_bank || !gt_images || !lq_bank || !lq_images || !crops || (!gt && !lq)) return HCF_ERR_ARG;
  int rc = check_geometry(scale, n_images, B, lr_h, lr_w);
  if (rc == HCF_OK) rc = check_table(gt_images, n_images, gt_bytes, 1);
  if (rc == HCF_OK) rc = check_table(lq_images, n_images, lq_bytes, 1);
  if (rc != HCF_OK) return rc;
  for (int i = 0; i < n_images; ++i)       // a larger HR image is the mod-crop case: its extra rows and columns are never read
    if (gt_images[3 * i + 1] < scale * lq_images[3 * i + 1] || gt_images[3 * i + 2] < scale * lq_images[3 * i + 2])
      return HCF_ERR_SHAPE;
  rc = check_crops(crops, B, lq_images, n_images, lr_h, lr_w, 1);
  if (rc != HCF_OK) return rc;

  PairArgs a;
  a.gt_bank = gt_bank; a.lq_bank = lq_bank; a.scale = scale; a.pad = 0;
  return launch_chunks(prepare_paired_kernel, a, crops, B, lr_h, lr_w, scale, bgr, gt, lq, stream,
                       [&](PairSample& s, const int32_t* c) {
    const int64_t* g = gt_images + 3 * c[0];
    const int64_t* l = lq_images + 3 * c[0];
    s.gt_off = g[0]; s.gt_h = (int)g[1]; s.gt_w = (int)g[2];
    s.lq_off = l[0]; s.lq_h = (int)l[1]; s.lq_w = (int)l[2];
  });
}

}  // extern "C"
