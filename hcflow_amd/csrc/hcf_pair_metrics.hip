// Validation metrics on the device: what test_HCFlow.py computes per image on the CPU -- tensor2img
// (utils/util.py:790-816), calculate_psnr_ssim (:898-982) with the Y channel of data/util.py:209-230, and the same on MATLAB-style
// bicubic down-scaled copies (utils/imresize.py) -- in float64 like the reference, every sum joined in a fixed order (no atomics).
// The project's one PSNR / SSIM / imresize implementation. hcf_metric_pair_* compare sample batches against ONE prepared GT: the
// GT-side work is done once, nothing is allocated, copied from the host or synchronised per sample. hcf_metric_psnr_ssim and
// hcf_metric_imresize_down are one-shot host wrappers over them (allocate, embed, compare, read back, free).
//
//   embed    gt -> reference buffer: the tensor2img planes as uint8 [B][3 (B,G,R)][H][W]; for scale > 1 the bicubic down-scaled
//            planes as fp64 [B][3][Ho][Wo] (rows first, not re-quantised) and the weight / index tables of contributions().
//   compare  one [B,3,H,W] fp32 sample against the reference:
//              pair_tile_kernel<FullSrc>   full resolution: quantise in registers, squared differences, separable SSIM
//              pair_rows_kernel, pair_cols_kernel + pair_tile_kernel<LowSrc>   (scale > 1) the same on the down-scaled pair
//              pair_finish_kernel          adds the blocks' slots in index order, applies log10 / the means -> out [B][8]
//
// pair_tile_kernel: one block per 16 x 32 tile of top-left positions; the (16 + 10) x (32 + 10) pixels under its 11 x 11 windows
// are staged plane by plane (B, G, R, then the Y the staging threads accumulated from them) as fp64 in LDS; pass 1 forms the five
// horizontally filtered moments (a, b, a^2, b^2, ab) of every staged row, pass 2 filters them vertically and evaluates the SSIM
// map. Half a wave walks 32 consecutive doubles of one row in every LDS access of both passes (one bank row of 256 B: no
// conflicts, no padding needed). The block's six sums go to workspace slot [image][block][6].
#include <math.h>
#include <stdint.h>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include "../../include/hcflow.h"
#include "hcf_common.h"
#include "hcf_bicubic_tables.h"
#include "hcf_ssim_window.h"

namespace hcf {
namespace pairm {

#define PM_TH 16                       // tile: rows / columns of top-left positions (= owned pixels)
#define PM_TW 32
#define PM_SH (PM_TH + 10)             // staged rows
#define PM_SW 44                       // staged columns: 32 + 10, rounded up to whole quads
#define PM_QUADS (PM_SH * (PM_SW / 4)) // 286 quads of 4 pixels
#define PM_ITEMS 2                     // quads per thread (256 threads)
#define PM_NQ 6                        // per block: sq(B,G,R), sq(Y), ssim B, G, R, Y

// tensor2img of one value: clamp to [0, 1], * 255 in fp32, round half to even (numpy .round())
__device__ __forceinline__ double quant255(float x) {
  const float v = fminf(fmaxf(x, 0.f), 1.f);
  return rint((double)(v * 255.0f));
}

// sources of a tile: plane p (0..2 = B, G, R) of both images at four pixels (gy, gx .. gx + 3); 0 outside the image
struct FullSrc {                       // uint8 reference planes + the fp32 RGB sample, quantised here
  const uint8_t* ref;
  const float* sr;
  uint8_t* img;                        // [B][H][W][3] BGR or null
  int vec;                             // W % 4 == 0: every quad is whole and 16-byte aligned
  static constexpr bool kImage = true;
  __device__ __forceinline__ void load(int b, int p, int gy, int gx, int H, int W, double* va, double* vb) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) va[e] = vb[e] = 0.0;
    if (gy >= H || gx >= W) return;
    const size_t oa = (((size_t)b * 3 + p) * H + gy) * W + gx;
    const size_t ob = (((size_t)b * 3 + (2 - p)) * H + gy) * W + gx;
    if (vec) {
      const uchar4 u = *reinterpret_cast<const uchar4*>(ref + oa);
      const float4 f = *reinterpret_cast<const float4*>(sr + ob);
      va[0] = u.x; va[1] = u.y; va[2] = u.z; va[3] = u.w;
      vb[0] = quant255(f.x); vb[1] = quant255(f.y); vb[2] = quant255(f.z); vb[3] = quant255(f.w);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gx + e < W) { va[e] = ref[oa + e]; vb[e] = quant255(sr[ob + e]); }
    }
  }
};

struct LowSrc {                        // two fp64 images [3][H][W] per batch entry, sa / sb doubles apart
  const double* a;
  const double* b;
  size_t sa, sb;
  static constexpr bool kImage = false;
  __device__ __forceinline__ void load(int bi, int p, int gy, int gx, int H, int W, double* va, double* vb) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) va[e] = vb[e] = 0.0;
    if (gy >= H) return;
    const size_t o = ((size_t)p * H + gy) * W + gx;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (gx + e < W) { va[e] = a[(size_t)bi * sa + o + e]; vb[e] = b[(size_t)bi * sb + o + e]; }
  }
};

// a position (top-left y, x) of the SSIM map is valid when its window lies in the cropped image
__device__ __forceinline__ bool pos_ok(int v, int n, int crop) { return v >= crop && v + 10 < n - crop; }

template <class Src>
__global__ __launch_bounds__(256) void pair_tile_kernel(Src src, int H, int W, int crop, Gauss11 gk, double* work, size_t img_stride,
                                                        size_t slot0) {
  __shared__ double ta[PM_SH][PM_SW], tb[PM_SH][PM_SW];
  __shared__ double hm[5][PM_SH][PM_TW];
  __shared__ double red[4][PM_NQ];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int y0 = blockIdx.y * PM_TH, x0 = blockIdx.x * PM_TW;
  // block-uniform: does the tile hold a valid position at all (border tiles, windows under 11 pixels: none)
  const bool any_ssim = max(y0, crop) <= min(y0 + PM_TH - 1, H - crop - 11) && max(x0, crop) <= min(x0 + PM_TW - 1, W - crop - 11);
  double ya[PM_ITEMS][4], yb[PM_ITEMS][4];
  unsigned qp[PM_ITEMS][3];
  double sq3 = 0.0, sqy = 0.0, ss[4] = {0.0, 0.0, 0.0, 0.0};

#pragma unroll
  for (int p = 0; p < 4; ++p) {
#pragma unroll
    for (int it = 0; it < PM_ITEMS; ++it) {
      const int q = tid + it * 256;
      if (q < PM_QUADS) {
        const int r = q / (PM_SW / 4), c4 = (q % (PM_SW / 4)) * 4;
        const int gy = y0 + r, gx = x0 + c4;
        double va[4], vb[4];
        if (p < 3) {
          src.load(b, p, gy, gx, H, W, va, vb);
          if constexpr (Src::kImage) qp[it][p] = (unsigned)vb[0] | ((unsigned)vb[1] << 8) | ((unsigned)vb[2] << 16) | ((unsigned)vb[3] << 24);
          const double cy = p == 0 ? 24.966 : p == 1 ? 128.553 : 65.481;      // bgr2ycbcr(only_y), 255 units
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            ya[it][e] = p == 0 ? cy * va[e] : fma(cy, va[e], ya[it][e]);
            yb[it][e] = p == 0 ? cy * vb[e] : fma(cy, vb[e], yb[it][e]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { va[e] = ya[it][e] / 255.0 + 16.0; vb[e] = yb[it][e] / 255.0 + 16.0; }
        }
        const bool own_row = r < PM_TH && gy >= crop && gy < H - crop;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ta[r][c4 + e] = va[e];
          tb[r][c4 + e] = vb[e];
          if (own_row && c4 + e < PM_TW && gx + e >= crop && gx + e < W - crop) {
            const double d = va[e] - vb[e];
            if (p < 3) sq3 = fma(d, d, sq3); else sqy = fma(d, d, sqy);
          }
        }
        if constexpr (Src::kImage) if (p == 2 && src.img && r < PM_TH && c4 < PM_TW && gy < H && gx < W) {
          uint8_t* o = src.img + (((size_t)b * H + gy) * W + gx) * 3;
          const unsigned B_ = qp[it][0], G_ = qp[it][1], R_ = qp[it][2];
          if (src.vec) {                                                     // 12 bytes B G R B G R ... , 4-byte aligned
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
            o4[0] = (B_ & 255u) | ((G_ & 255u) << 8) | ((R_ & 255u) << 16) | (((B_ >> 8) & 255u) << 24);
            o4[1] = ((G_ >> 8) & 255u) | (((R_ >> 8) & 255u) << 8) | (((B_ >> 16) & 255u) << 16) | (((G_ >> 16) & 255u) << 24);
            o4[2] = ((R_ >> 16) & 255u) | ((B_ >> 24) << 8) | ((G_ >> 24) << 16) | ((R_ >> 24) << 24);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (gx + e < W) {
                o[3 * e + 0] = (uint8_t)(B_ >> (8 * e));
                o[3 * e + 1] = (uint8_t)(G_ >> (8 * e));
                o[3 * e + 2] = (uint8_t)(R_ >> (8 * e));
              }
          }
        }
      }
    }
    __syncthreads();
    if (any_ssim) {
      // pass 1: the five moments filtered along the row, for every staged row and the tile's 32 columns
#pragma unroll
      for (int k = 0; k < (PM_SH * PM_TW + 255) / 256; ++k) {
        const int i = tid + k * 256;
        if (i < PM_SH * PM_TW) {
          const int r = i / PM_TW, x = i % PM_TW;
          double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
          for (int j = 0; j < 11; ++j) {
            const double u = ta[r][x + j], t = tb[r][x + j], wu = gk.g[j] * u, wt = gk.g[j] * t;
            m1 += wu; m2 += wt;
            s11 = fma(wu, u, s11); s22 = fma(wt, t, s22); s12 = fma(wu, t, s12);
          }
          hm[0][r][x] = m1; hm[1][r][x] = m2; hm[2][r][x] = s11; hm[3][r][x] = s22; hm[4][r][x] = s12;
        }
      }
    }
    __syncthreads();
    if (any_ssim) {
      // pass 2: two vertically adjacent positions per thread share 10 of their 11 rows
      const int x = tid % PM_TW, ly = (tid / PM_TW) * 2;
      double v0[5] = {0, 0, 0, 0, 0}, v1[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 12; ++j) {
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          const double h = hm[m][ly + j][x];
          if (j < 11) v0[m] = fma(gk.g[j < 11 ? j : 0], h, v0[m]);
          if (j > 0) v1[m] = fma(gk.g[j > 0 ? j - 1 : 0], h, v1[m]);
        }
      }
      const double C1 = 6.5025, C2 = 58.5225;                       // (0.01 * 255)^2, (0.03 * 255)^2
      const bool xok = pos_ok(x0 + x, W, crop);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const double* v = o ? v1 : v0;
        if (xok && pos_ok(y0 + ly + o, H, crop)) {
          const double mu11 = v[0] * v[0], mu22 = v[1] * v[1], mu12 = v[0] * v[1];
          ss[p] += ((2 * mu12 + C1) * (2 * (v[4] - mu12) + C2)) / ((mu11 + mu22 + C1) * ((v[2] - mu11) + (v[3] - mu22) + C2));
        }
      }
    }
  }
  // the block's six sums: lanes by shuffle, the four waves in order
  double q6[PM_NQ] = {sq3, sqy, ss[0], ss[1], ss[2], ss[3]};
#pragma unroll
  for (int k = 0; k < PM_NQ; ++k) {
    double v = q6[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < PM_NQ) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    work[(size_t)b * img_stride + slot0 + blk * PM_NQ + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
}

// GT -> uint8 planes [B][3 (B,G,R)][H][W]
__global__ __launch_bounds__(256) void pair_quant_kernel(const float* x, uint8_t* q, long long hw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int b = blockIdx.y;
#pragma unroll
  for (int c = 0; c < 3; ++c) q[((size_t)b * 3 + (2 - c)) * hw + i] = (uint8_t)quant255(x[((size_t)b * 3 + c) * hw + i]);
}

// imresize of the uint8 planes, rows first: the row pass of each of the P columns a position needs is formed on the fly (run
// once per GT), by the same fma chain as pair_rows_kernel + pair_cols_kernel: a sample equal to the GT gives the same bits
__global__ __launch_bounds__(256) void pair_embed_down_kernel(const uint8_t* q, double* low, int H, int W, int Ho, int Wo, int P,
                                                             const double* w0, const int* i0, const double* w1, const int* i1) {
  const long long n = (long long)Ho * Wo;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int yo = (int)(i / Wo), xo = (int)(i % Wo);
  const uint8_t* p = q + (size_t)blockIdx.y * H * W;
  double s = 0.0;
  for (int kx = 0; kx < P; ++kx) {
    const int jx = i1[xo * P + kx];
    double t = 0.0;
    for (int ky = 0; ky < P; ++ky) t = fma(w0[yo * P + ky], (double)p[(size_t)i0[yo * P + ky] * W + jx], t);
    s = fma(w1[xo * P + kx], t, s);
  }
  low[(size_t)blockIdx.y * n + i] = s;
}

// sample, row pass: t[b][c][o][x] = sum_k w0[o][k] * tensor2img(sr)[c][i0[o][k]][x]     (blockIdx.y = o, blockIdx.z = b * 3 + c)
__global__ __launch_bounds__(256) void pair_rows_kernel(const float* sr, double* work, size_t img_stride, size_t t0, int H, int W,
                                                        int Ho, int P, const double* w0, const int* i0) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const int o = blockIdx.y, b = blockIdx.z / 3, c = blockIdx.z % 3;
  const float* p = sr + ((size_t)b * 3 + (2 - c)) * H * W;
  double s = 0.0;
  for (int k = 0; k < P; ++k) s = fma(w0[o * P + k], quant255(p[(size_t)i0[o * P + k] * W + x]), s);
  work[(size_t)b * img_stride + t0 + ((size_t)c * Ho + o) * W + x] = s;
}

// sample, column pass: low[b][c][y][xo] = sum_k w1[xo][k] * t[b][c][y][i1[xo][k]]
__global__ __launch_bounds__(256) void pair_cols_kernel(double* work, size_t img_stride, size_t t0, size_t l0, int W, int Ho, int Wo,
                                                        int P, const double* w1, const int* i1) {
  const long long n = 3LL * Ho * Wo;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int xo = (int)(i % Wo);
  const long long row = i / Wo;                                    // c * Ho + y
  double* base = work + (size_t)blockIdx.y * img_stride;
  const double* t = base + t0 + (size_t)row * W;
  double s = 0.0;
  for (int k = 0; k < P; ++k) s = fma(w1[xo * P + k], t[i1[xo * P + k]], s);
  base[l0 + i] = s;
}

struct FinishArgs {
  size_t img_stride, slotF, slotL;
  int nblkF, nblkL, H, W, crop, Ho, Wo, low;
};

__device__ __forceinline__ double psnr_of(double sum, double n) {
  const double mse = sum / n;
  return mse == 0 ? (double)INFINITY : 20 * log10(255.0 / sqrt(mse));
}

// one block per image: thread t adds slots t, t + 256, ... of each quantity in order, the block joins them in a fixed tree
__global__ __launch_bounds__(256) void pair_finish_kernel(const double* work, FinishArgs a, double* out) {
  __shared__ double red[4][2 * PM_NQ];
  const int tid = threadIdx.x;
  const double* base = work + (size_t)blockIdx.x * a.img_stride;
#pragma unroll
  for (int k = 0; k < 2 * PM_NQ; ++k) {
    const bool lo = k >= PM_NQ;
    const double* p = base + (lo ? a.slotL : a.slotF) + (lo ? k - PM_NQ : k);
    const int n = lo ? (a.low ? a.nblkL : 0) : a.nblkF;
    double v = 0.0;
    for (int j = tid; j < n; j += 256) v += p[(size_t)j * PM_NQ];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double s[2 * PM_NQ];
  for (int k = 0; k < 2 * PM_NQ; ++k) s[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  double* o = out + (size_t)blockIdx.x * 8;
  {
    const int Hc = a.H - 2 * a.crop, Wc = a.W - 2 * a.crop;
    const bool has = Hc >= 11 && Wc >= 11;                         // else the reference's valid region is empty: nan
    const double nv = has ? (double)(Hc - 10) * (double)(Wc - 10) : 0.0;
    o[0] = psnr_of(s[0], 3.0 * Hc * Wc);
    o[1] = has ? (s[2] + s[3] + s[4]) / (3.0 * nv) : (double)NAN;
    o[2] = psnr_of(s[1], (double)Hc * Wc);
    o[3] = has ? s[5] / nv : (double)NAN;
  }
  if (a.low) {
    const bool has = a.Ho >= 11 && a.Wo >= 11;
    const double nv = has ? (double)(a.Ho - 10) * (double)(a.Wo - 10) : 0.0;
    o[4] = psnr_of(s[6], 3.0 * a.Ho * a.Wo);
    o[5] = has ? (s[8] + s[9] + s[10]) / (3.0 * nv) : (double)NAN;
    o[6] = psnr_of(s[7], (double)a.Ho * a.Wo);
    o[7] = has ? s[11] / nv : (double)NAN;
  } else {
    o[4] = o[5] = o[6] = o[7] = 0.0;
  }
}

static inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// reference: [u8 planes][low fp64 planes][w0][w1][i0][i1]; workspace per image (doubles): [full slots][low slots][t][low sample]
struct Layout {
  int Ho = 0, Wo = 0, P = 0, low = 0;
  int tilesX = 0, tilesY = 0, ltX = 0, ltY = 0;
  size_t r_low = 0, r_w0 = 0, r_w1 = 0, r_i0 = 0, r_i1 = 0, ref_bytes = 0;
  size_t slotF = 0, slotL = 0, t0 = 0, l0 = 0, img_stride = 0, work_bytes = 0;
};

static bool layout(int B, int H, int W, int scale, Layout& L) {
  if (B < 1 || H < 1 || W < 1 || scale < 0) return false;
  if (B > 21845 || H > 1000000 || W > 1000000 || scale > 1024) return false;      // grid limits: blockIdx.z = b * 3 + c, blockIdx.y = row
  L.low = scale > 1;
  L.tilesX = (W + PM_TW - 1) / PM_TW;
  L.tilesY = (H + PM_TH - 1) / PM_TH;
  if (L.tilesY > 65535 || (long long)H * W > (1LL << 36)) return false;
  size_t off = up16((size_t)B * 3 * H * W);
  if (L.low) {
    L.Ho = (H + scale - 1) / scale;
    L.Wo = (W + scale - 1) / scale;
    L.P = (int)ceil(4.0 / (1.0 / scale)) + 2;                      // as contributions() forms it
    L.ltX = (L.Wo + PM_TW - 1) / PM_TW;
    L.ltY = (L.Ho + PM_TH - 1) / PM_TH;
    if (L.Ho > 65535) return false;
    L.r_low = off; off += (size_t)B * 3 * L.Ho * L.Wo * sizeof(double);
    L.r_w0 = off; off += (size_t)L.Ho * L.P * sizeof(double);
    L.r_w1 = off; off += (size_t)L.Wo * L.P * sizeof(double);
    L.r_i0 = off; off += up16((size_t)L.Ho * L.P * sizeof(int));
    L.r_i1 = off; off += up16((size_t)L.Wo * L.P * sizeof(int));
  }
  L.ref_bytes = off;
  size_t d = 0;
  L.slotF = d; d += (size_t)L.tilesX * L.tilesY * PM_NQ;
  if (L.low) {
    L.slotL = d; d += (size_t)L.ltX * L.ltY * PM_NQ;
    L.t0 = d; d += (size_t)3 * L.Ho * W;
    L.l0 = d; d += (size_t)3 * L.Ho * L.Wo;
  }
  L.img_stride = d;                                                // a function of (H, W, scale) alone
  L.work_bytes = (size_t)B * d * sizeof(double);
  return true;
}

// host tables of contributions() (hcf_bicubic_tables.h), built once per (length, scale) and kept for the life of the process: embed's stream-ordered
// uploads read them after the call has returned
struct Table { std::vector<double> w; std::vector<int> idx; int P = 0; };
static const Table* table_for(int len, int scale) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, Table*> cache;
  std::lock_guard<std::mutex> g(mu);
  Table*& t = cache[std::make_pair(len, scale)];
  if (!t) {
    t = new Table();
    contributions(len, (len + scale - 1) / scale, 1.0 / scale, t->w, t->idx, t->P);
  }
  return t;
}

// the device buffers of a one-shot call, freed when it returns. The work queued on them is stream-ordered: the caller
// synchronises the stream before returning, unless nothing was launched
struct DevBuf {
  std::vector<void*> ptrs;
  bool ok = true;
  template <class T> T* get(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(p);
    return (T*)p;
  }
  ~DevBuf() { for (void* p : ptrs) hipFree(p); }
};

}  // namespace pairm
}  // namespace hcf

using namespace hcf;
using namespace hcf::pairm;

extern "C" {

size_t hcf_metric_pair_ref_bytes(int32_t B, int32_t H, int32_t W, int32_t scale) {
  Layout L;
  return layout(B, H, W, scale, L) ? L.ref_bytes : 0;
}

size_t hcf_metric_pair_workspace(int32_t B, int32_t H, int32_t W, int32_t scale) {
  Layout L;
  return layout(B, H, W, scale, L) ? L.work_bytes : 0;
}

int hcf_metric_pair_embed(const float* gt, int32_t B, int32_t H, int32_t W, int32_t crop_border, int32_t scale, void* ref,
                          size_t ref_bytes, hcf_stream_t stream) {
  Layout L;
  if (!gt || !ref || crop_border < 0 || scale < 0 || !layout(B, H, W, scale, L)) return HCF_ERR_ARG;
  if (ref_bytes < L.ref_bytes || H - 2 * crop_border < 1 || W - 2 * crop_border < 1) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  char* r = (char*)ref;
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(pair_quant_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)B), dim3(256), 0, st, gt, (uint8_t*)r, hw);
  if (L.low) {
    const Table* t0 = table_for(H, scale);
    const Table* t1 = table_for(W, scale);
    if (t0->P != L.P || t1->P != L.P) return HCF_ERR_STATE;
    if (hipMemcpyAsync(r + L.r_w0, t0->w.data(), t0->w.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r + L.r_w1, t1->w.data(), t1->w.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r + L.r_i0, t0->idx.data(), t0->idx.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r + L.r_i1, t1->idx.data(), t1->idx.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
      return HCF_ERR_HIP;
    const long long n = (long long)L.Ho * L.Wo;
    hipLaunchKernelGGL(pair_embed_down_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(B * 3)), dim3(256), 0, st,
                       (const uint8_t*)r, (double*)(r + L.r_low), H, W, L.Ho, L.Wo, L.P, (const double*)(r + L.r_w0),
                       (const int*)(r + L.r_i0), (const double*)(r + L.r_w1), (const int*)(r + L.r_i1));
  }
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_metric_pair_compare(const void* ref, size_t ref_bytes, const float* sr, int32_t B, int32_t H, int32_t W, int32_t crop_border,
                            int32_t scale, double* out, uint8_t* image_out, void* work, size_t work_bytes, hcf_stream_t stream) {
  Layout L;
  if (!ref || !sr || !out || !work || crop_border < 0 || scale < 0 || !layout(B, H, W, scale, L)) return HCF_ERR_ARG;
  if (ref_bytes < L.ref_bytes || work_bytes < L.work_bytes || H - 2 * crop_border < 1 || W - 2 * crop_border < 1) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const char* r = (const char*)ref;
  double* wk = (double*)work;
  const Gauss11 gk = gauss11();
  FullSrc fs;
  fs.ref = (const uint8_t*)r; fs.sr = sr; fs.img = image_out; fs.vec = (W & 3) == 0;
  hipLaunchKernelGGL(pair_tile_kernel<FullSrc>, dim3((unsigned)L.tilesX, (unsigned)L.tilesY, (unsigned)B), dim3(256), 0, st, fs, H, W,
                     crop_border, gk, wk, L.img_stride, L.slotF);
  if (L.low) {
    hipLaunchKernelGGL(pair_rows_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)L.Ho, (unsigned)(B * 3)), dim3(256), 0, st, sr, wk,
                       L.img_stride, L.t0, H, W, L.Ho, L.P, (const double*)(r + L.r_w0), (const int*)(r + L.r_i0));
    const long long n = 3LL * L.Ho * L.Wo;
    hipLaunchKernelGGL(pair_cols_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, wk, L.img_stride, L.t0, L.l0,
                       W, L.Ho, L.Wo, L.P, (const double*)(r + L.r_w1), (const int*)(r + L.r_i1));
    LowSrc ls;                                                     // the sample's low-resolution planes sit in each image's part of the workspace
    ls.a = (const double*)(r + L.r_low); ls.sa = (size_t)3 * L.Ho * L.Wo;
    ls.b = wk + L.l0; ls.sb = L.img_stride;
    hipLaunchKernelGGL(pair_tile_kernel<LowSrc>, dim3((unsigned)L.ltX, (unsigned)L.ltY, (unsigned)B), dim3(256), 0, st, ls, L.Ho, L.Wo, 0,
                       gk, wk, L.img_stride, L.slotL);
  }
  FinishArgs fa;
  fa.img_stride = L.img_stride; fa.slotF = L.slotF; fa.slotL = L.slotL;
  fa.nblkF = L.tilesX * L.tilesY; fa.nblkL = L.ltX * L.ltY;
  fa.H = H; fa.W = W; fa.crop = crop_border; fa.Ho = L.Ho; fa.Wo = L.Wo; fa.low = L.low;
  hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)wk, fa, out);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

// one-shot: embed gt, compare sr, read the rows back. Everything is refused before the first device call; once work may have
// been launched the stream is synchronised before the buffers go, on the error paths too
int hcf_metric_psnr_ssim(const float* gt, const float* sr, int32_t B, int32_t H, int32_t W, int32_t crop_border,
                         int32_t scale, double* out, hcf_stream_t stream) {
  Layout L;
  if (!gt || !sr || !out || crop_border < 0 || scale < 0 || !layout(B, H, W, scale, L)) return HCF_ERR_ARG;
  if (H - 2 * crop_border < 1 || W - 2 * crop_border < 1) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  DevBuf d;
  char* ref = d.get<char>(L.ref_bytes);
  char* work = d.get<char>(L.work_bytes);
  double* rows = d.get<double>((size_t)B * 8);
  if (!d.ok) return HCF_ERR_NOMEM;
  int rc = hcf_metric_pair_embed(gt, B, H, W, crop_border, scale, ref, L.ref_bytes, stream);
  if (rc == HCF_OK)
    rc = hcf_metric_pair_compare(ref, L.ref_bytes, sr, B, H, W, crop_border, scale, rows, nullptr, work, L.work_bytes, stream);
  if (rc == HCF_OK && hipMemcpyAsync(out, rows, sizeof(double) * (size_t)B * 8, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = HCF_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && rc == HCF_OK) rc = HCF_ERR_HIP;
  return rc;
}

// one-shot: embed x and read back the reference's down-scaled planes [B][3][Ho][Wo] (rows first, not re-quantised)
int hcf_metric_imresize_down(const float* x, int32_t B, int32_t H, int32_t W, int32_t scale, double* out, hcf_stream_t stream) {
  Layout L;
  if (!x || !out || scale < 2 || !layout(B, H, W, scale, L)) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DevBuf d;
  char* ref = d.get<char>(L.ref_bytes);
  if (!d.ok) return HCF_ERR_NOMEM;
  int rc = hcf_metric_pair_embed(x, B, H, W, 0, scale, ref, L.ref_bytes, stream);
  if (rc == HCF_OK && hipMemcpyAsync(out, ref + L.r_low, sizeof(double) * (size_t)B * 3 * L.Ho * L.Wo, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = HCF_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess && rc == HCF_OK) rc = HCF_ERR_HIP;
  return rc;
}

}  // extern "C"
