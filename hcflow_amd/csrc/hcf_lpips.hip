// LPIPS v0.1 with AlexNet (the perceptual column of the reference's test log: codes/test_HCFlow.py:48,132-133,
// `lpips.LPIPS(net='alex')` applied to (2 gt - 1, 2 sr - 1)) as one call on device tensors, hcflow_amd/lpips.py.
//
//   prep      scaling layer (x - shift) / scale, NCHW -> NHWC, space-to-depth by 4 (channel c*16 + a*4 + b for input row 4Y+a,
//             col 4X+b; zeros beyond the image), in0 and in1 stacked into one batch of 2B images: every later launch covers both
//   conv1     11x11 stride 4 pad 2 == 5x5 stride 1 pad 2 on the s2d grid with the re-indexed weight [64,48,5,5] (lpips.py:
//             alex_conv1_as_s2d): the flow's fp32-MFMA conv kernel (hcf_conv.hip, TAPS = 25), bias + ReLU fused
//   pool1     MaxPool 3 / 2 (floor mode) over the valid conv1 rows / cols only (the s2d grid carries one or two spare ones)
//   conv2     5x5 pad 2, 64 -> 192, same kernel, three 64-channel blocks
//   pool2
//   conv3..5  3x3 pad 1 through hcf_aux_conv2d (exact fp32 MFMA), bias + ReLU fused
//   head      per layer and pixel: n_i = sum_c f_i^2, d = sum_c w_c (f0 / (sqrt n0 + 1e-10) - f1 / (sqrt n1 + 1e-10))^2; per-block
//             partial sums in a fixed order, then out[b] = sum_l (sum of layer l's partials) / (h_l w_l), in layer order.
// Every reduction has a fixed order that depends only on (H, W): results are bit-reproducible and per image independent of B.
// The call leaves the s2d input and every feature map in its workspace; hcf_lpips_alex_backward (below) walks back down from
// there to the image gradients (hcflow_amd/lpips.py: LPIPSLoss).
// hcf_lpips_alex_embed / hcf_lpips_alex_map (hcflow_amd/lpips.py: LPIPSMap) run the same walk over ONE input of B images, the head
// against a stored reference (the same per-pixel function: bit-equal values), and one fused kernel for the per-pixel map
// D = sum_l bilinear_up(d_l), the per-pixel best over a sample set and their means.
#include <algorithm>
#include <cstring>

#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLpipsLayers = 5;
constexpr int kHeadPix = 128;                       // pixels per head block: 16 groups of 16 lanes, 8 pixels each
static const int kAlexC[kLpipsLayers] = {64, 192, 384, 256, 256};

static inline size_t lp_al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct LpipsPlan {
  int Hs, Ws, H1, W1, H2, W2, H3, W3;
  int chunk0[kLpipsLayers], nchunk[kLpipsLayers], nchunk_total;
  size_t o_s2d, o_f1, o_p1, o_f2, o_p2, o_f3, o_f4, o_f5, o_pk, o_bias, o_scale, o_part, o_aux, aux_bytes, total;
};

// The slabs hold Nimg images: 2B for the metric (in0 and in1 stacked), B for one embedded input (hcf_lpips_alex_embed / _map).
static bool lpips_plan_n(int B, int Nimg, int H, int W, LpipsPlan& p) {
  memset(&p, 0, sizeof(p));
  if (B < 1 || Nimg < B || H < 31 || W < 31 || H >= 32768 || W >= 32768) return false;
  p.Hs = (H + 3) / 4; p.Ws = (W + 3) / 4;
  p.H1 = (H - 7) / 4 + 1; p.W1 = (W - 7) / 4 + 1;            // conv1: floor((H + 4 - 11) / 4) + 1
  p.H2 = (p.H1 - 3) / 2 + 1; p.W2 = (p.W1 - 3) / 2 + 1;
  p.H3 = (p.H2 - 3) / 2 + 1; p.W3 = (p.W2 - 3) / 2 + 1;
  const int hw[kLpipsLayers] = {p.H1 * p.W1, p.H2 * p.W2, p.H3 * p.W3, p.H3 * p.W3, p.H3 * p.W3};
  int c0 = 0;
  for (int l = 0; l < kLpipsLayers; ++l) {
    p.chunk0[l] = c0;
    p.nchunk[l] = (hw[l] + kHeadPix - 1) / kHeadPix;
    c0 += p.nchunk[l];
  }
  p.nchunk_total = c0;
  const size_t N = (size_t)Nimg, f = sizeof(float);
  const size_t gs = N * p.Hs * p.Ws, g2 = N * p.H2 * p.W2, g3 = N * p.H3 * p.W3;
  size_t o = 256;                                              // [0, 256): unused header
  auto take = [&](size_t bytes) { const size_t r = o; o += lp_al256(bytes); return r; };
  p.o_s2d = take(gs * 48 * f);
  p.o_f1 = take(gs * 64 * f);
  p.o_p1 = take(g2 * 64 * f);
  p.o_f2 = take(g2 * 192 * f);
  p.o_p2 = take(N * p.H3 * p.W3 * 192 * f);
  p.o_f3 = take(g3 * 384 * f);
  p.o_f4 = take(g3 * 256 * f);
  p.o_f5 = take(g3 * 256 * f);
  // fp32 conv pack [chunk][tap][2][64][8] + one zero K-step: conv1 3 chunks, conv2 4 chunks of 16 input channels
  p.o_pk = take(conv_pack_bytes(4, 25, 64));
  p.o_bias = take(64 * f);
  p.o_scale = take(64 * f);
  p.o_part = take((size_t)B * p.nchunk_total * f);
  size_t aux = 0;
  for (int l = 2; l < kLpipsLayers; ++l)
    aux = std::max(aux, hcf_aux_conv2d_workspace(kAlexC[l - 1], kAlexC[l], 3, (int)N, p.H3, p.W3));
  p.aux_bytes = aux;
  p.o_aux = take(aux);
  p.total = o;
  return aux > 0;
}

static bool lpips_plan(int B, int H, int W, LpipsPlan& p) { return lpips_plan_n(B, 2 * B, H, W, p); }

// ---- prep: one thread per (image n of N = 2B, or of N = B with in0 alone, s2d pixel, 4-channel unit q = c * 4 + a) -> 4 input columns 4X .. 4X+3 of row 4Y+a
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ in0, const float* __restrict__ in1, int B,
                                                         int N, int H, int W, int Hs, int Ws, int normalize,
                                                         const float* __restrict__ shift, const float* __restrict__ scale,
                                                         float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)N * Hs * Ws * 12;
  if (i >= total) return;
  const int q = (int)(i % 12);
  const long long pix = i / 12;
  const int X = (int)(pix % Ws);
  const int Y = (int)((pix / Ws) % Hs);
  const int n = (int)(pix / ((long long)Ws * Hs));
  const int c = q >> 2, a = q & 3;
  const float* src = (n < B) ? in0 + (size_t)n * 3 * H * W : in1 + (size_t)(n - B) * 3 * H * W;
  const int y = 4 * Y + a;
  const float sh = shift[c], sc = scale[c];
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = 4 * X + j;
    float t = 0.f;                                              // zero padding in the SCALED domain (conv1's padding)
    if (y < H && x < W) {
      float s = src[((size_t)c * H + y) * W + x];
      if (normalize) s = 2.f * s - 1.f;
      t = (s - sh) / sc;
    }
    v[j] = t;
  }
  f32x4 o4 = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(out + (size_t)pix * 48 + q * 4) = o4;
}

// ---- MaxPool 3 / 2, floor mode, NHWC: in [N][Hst][Wst][C] with the valid region Hin x Win, out dense [N][Ho][Wo][C]
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float* __restrict__ in, int N, int Hst, int Wst, int C,
                                                            int Ho, int Wo, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C4 = C >> 2;
  const long long total = (long long)N * Ho * Wo * C4;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  const long long pix = i / C4;
  const int ox = (int)(pix % Wo);
  const int oy = (int)((pix / Wo) % Ho);
  const int n = (int)(pix / ((long long)Wo * Ho));
  const float* base = in + (size_t)n * Hst * Wst * C + 4 * c4;
  f32x4 m = *reinterpret_cast<const f32x4*>(base + ((size_t)(2 * oy) * Wst + 2 * ox) * C);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((size_t)(2 * oy + dy) * Wst + 2 * ox + dx) * C);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  *reinterpret_cast<f32x4*>(out + (size_t)pix * C + 4 * c4) = m;
}

// ---- head
struct LpipsLayer {
  const float* f;     // [2B][Hst][Wst][C]: images 0..B-1 from in0, B..2B-1 from in1
  const float* lin;   // [C]
  int C, Hst, Wst, h, w, chunk0;
};
struct LpipsHeadArgs {
  LpipsLayer L[kLpipsLayers];
  int B, nchunk_total;
  float* part;        // [B][nchunk_total]
};

__device__ __forceinline__ float group16_sum(float v) {      // butterfly over the 16 lanes of a group; lane 0 of it is used
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// One pixel's layer value d = sum_c w_c (f0_c / (sqrt n0 + 1e-10) - f1_c / (sqrt n1 + 1e-10))^2 by the 16 lanes of a group (lane j
// over the float4 channel units j + 16 i, i < ni = C / 64); f0, f1: the pixel's C channels in the two feature maps. Every lane of
// the group returns the sum. The two head kernels share it: their values agree bit for bit.
__device__ __forceinline__ float lpips_pixel_term(const float* __restrict__ f0, const float* __restrict__ f1,
                                                  const float* __restrict__ lin, int ni, int j) {
  const float eps = 1e-10f;
  f32x4 v0[6], v1[6];
  float n0 = 0.f, n1 = 0.f;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i < ni) {
      v0[i] = *reinterpret_cast<const f32x4*>(f0 + 4 * (j + 16 * i));
      v1[i] = *reinterpret_cast<const f32x4*>(f1 + 4 * (j + 16 * i));
      n0 += v0[i].x * v0[i].x + v0[i].y * v0[i].y + v0[i].z * v0[i].z + v0[i].w * v0[i].w;
      n1 += v1[i].x * v1[i].x + v1[i].y * v1[i].y + v1[i].z * v1[i].z + v1[i].w * v1[i].w;
    }
  }
  n0 = __shfl(group16_sum(n0), 0, 16);
  n1 = __shfl(group16_sum(n1), 0, 16);
  const float d0 = sqrtf(n0) + eps, d1 = sqrtf(n1) + eps;
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i < ni) {
      const float* w = lin + 4 * (j + 16 * i);                  // (any alignment: four scalar loads)
      const float ex = v0[i].x / d0 - v1[i].x / d1, ey = v0[i].y / d0 - v1[i].y / d1;
      const float ez = v0[i].z / d0 - v1[i].z / d1, ew = v0[i].w / d0 - v1[i].w / d1;
      t += w[0] * ex * ex + w[1] * ey * ey + w[2] * ez * ez + w[3] * ew * ew;
    }
  }
  return group16_sum(t);
}

// the 16 group sums of a head block, added in group order by thread 0
__device__ __forceinline__ void lpips_head_block_sum(float s, int g, int j, float* gsum, float* dst) {
  if (j == 0) gsum[g] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += gsum[k];
    *dst = t;
  }
}

// grid (nchunk_total, B), 256 threads: 16 groups x 16 lanes, one pixel per group at a time, lanes over float4 channel units
__global__ __launch_bounds__(256) void lpips_head_kernel(const LpipsHeadArgs a) {
  __shared__ float gsum[16];
  const int b = blockIdx.y, blk = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < kLpipsLayers; ++k) l = (blk >= a.L[k].chunk0) ? k : l;
  const LpipsLayer L = a.L[l];
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int hw = L.h * L.w, C = L.C, ni = C >> 6;              // C / 4 float4 units over 16 lanes: 1 .. 6 each
  float s = 0.f;
  for (int k = 0; k < kHeadPix / 16; ++k) {
    const int p = (blk - L.chunk0) * kHeadPix + k * 16 + g;
    if (p >= hw) break;                                         // (uniform over the group)
    const int y = p / L.w, x = p - y * L.w;
    const float* f0 = L.f + (((size_t)b * L.Hst + y) * L.Wst + x) * C;
    const float* f1 = L.f + (((size_t)(a.B + b) * L.Hst + y) * L.Wst + x) * C;
    s += lpips_pixel_term(f0, f1, L.lin, ni, j);                // lane 0's value is the one kept
  }
  lpips_head_block_sum(s, g, j, gsum, a.part + (size_t)b * a.nchunk_total + blk);
}

// ---- head over two feature bases (hcf_lpips_alex_map): image b of the reference store against image b of the sample's maps, both
// slabs of B images. The grid, the lane layout and the partials of lpips_head_kernel; each pixel's d_l also goes to the layer-map
// buffer dl [B][dl_total] (layer l's h_l x w_l grid, row-major, from dl0[l] on), which the map kernel upsamples.
struct LpipsHead2Args {
  LpipsLayer L[kLpipsLayers];          // f: the sample's maps
  const float* fr[kLpipsLayers];       // the reference's maps, the same layout
  int dl0[kLpipsLayers], dl_total, nchunk_total;
  float* dl;
  float* part;                         // [B][nchunk_total]
};

__global__ __launch_bounds__(256) void lpips_head2_kernel(const LpipsHead2Args a) {
  __shared__ float gsum[16];
  const int b = blockIdx.y, blk = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < kLpipsLayers; ++k) l = (blk >= a.L[k].chunk0) ? k : l;
  const LpipsLayer L = a.L[l];
  const float* const fr = a.fr[l];
  float* const dl = a.dl + (size_t)b * a.dl_total + a.dl0[l];
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int hw = L.h * L.w, C = L.C, ni = C >> 6;
  float s = 0.f;
  for (int k = 0; k < kHeadPix / 16; ++k) {
    const int p = (blk - L.chunk0) * kHeadPix + k * 16 + g;
    if (p >= hw) break;                                         // (uniform over the group)
    const int y = p / L.w, x = p - y * L.w;
    const size_t o = (((size_t)b * L.Hst + y) * L.Wst + x) * C;
    const float d = lpips_pixel_term(fr + o, L.f + o, L.lin, ni, j);
    if (j == 0) dl[p] = d;
    s += d;
  }
  lpips_head_block_sum(s, g, j, gsum, a.part + (size_t)b * a.nchunk_total + blk);
}

// ---- the spatial map: D[b, y, x] = sum over l = 0..4, in that order, of the bilinear upsampling (align_corners = False) of d_l to
// H x W. Source row of output row y on an h-row grid: sy = max(0, (y + 0.5) h / H - 0.5) = max(0, ((2y + 1) h - H) / (2H)),
// i0 = floor(sy), i1 = min(i0 + 1, h - 1), weight sy - i0 -- taken from the integer quotient and remainder, so the weight carries
// one rounding. Columns alike. A thread owns 4 consecutive columns of one row: w_l <= W / 4, so they read at most 3 source columns.
// The divisors 2H, 2W and W4 are the launch's: quotients come from a float estimate with the host's reciprocal and one correction
// step (lpips_divmod), weights from a multiplication by that reciprocal.
struct LpipsMapArgs {
  const float* dl;                     // [B][dl_total]
  int dl0[kLpipsLayers], dl_total;
  int h[3], w[3];                      // the grids of layer 0, layer 1 and layers 2..4
  int H, W, W4, nblk, first, vec;      // W4 = ceil(W / 4) units per row; nblk blocks of 256 units per image; vec: 16-byte accesses
  float inv2H, inv2W, invW4;           // 1 / (2H), 1 / (2W), 1 / W4
  float* out_map;                      // [B][H][W] or null
  float* best_map;                     // [B][H][W] or null: best = first ? D : fminf(best, D)
  double* part;                        // [B][nblk][2]: the block's sums of D and of the updated best_map
};

struct LpipsAxis { int i0, i1, rem; float t; };

// q = floor(num / d) and *rem = num - q d for 0 <= num < 2^31, d >= 1 and q < 2^15, inv = 1.f / d: the float product is within
// q 2^-22 < 1 of the quotient, so its truncation is off by at most one, which the remainder shows
__device__ __forceinline__ int lpips_divmod(int num, int d, float inv, int* rem) {
  int q = (int)((float)num * inv);
  int r = num - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
  *rem = r;
  return q;
}

// output index y of an H-long axis on an h-long source axis; twoH = 2H, inv = 1.f / twoH. rem: the numerator's remainder (the
// numerator itself where it is <= 0 and the source coordinate clamps to 0)
__device__ __forceinline__ LpipsAxis lpips_axis(int y, int h, int twoH, float inv) {
  const int num = (2 * y + 1) * h - (twoH >> 1);
  LpipsAxis a;
  if (num <= 0) { a.i0 = 0; a.rem = num; a.t = 0.f; }
  else { a.i0 = lpips_divmod(num, twoH, inv, &a.rem); a.t = (float)a.rem * inv; }
  a.i1 = min(a.i0 + 1, h - 1);
  return a;
}

__device__ __forceinline__ double wave_sum_f64(double v) {     // butterfly: every lane gets the sum, in a fixed order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (nblk, B), 256 threads, one unit (row y, columns 4u .. 4u + 3) each
__global__ __launch_bounds__(256) void lpips_map_kernel(const LpipsMapArgs a) {
  __shared__ double wsum[4][2];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.H * a.W4;
  double sd = 0.0, sb = 0.0;
  if (live) {
    int u;
    const int y = lpips_divmod(i, a.W4, a.invW4, &u), x0 = u * 4;
    float D[4] = {0.f, 0.f, 0.f, 0.f};
    const float* const dimg = a.dl + (size_t)b * a.dl_total;
    // layers 2, 3, 4 share one grid: three sets of indices and weights serve the five layers
    LpipsAxis r[3];
    int ci[3][3], up[3][4];
    float tx[3][4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int h = a.h[q], w = a.w[q];
      r[q] = lpips_axis(y, h, 2 * a.H, a.inv2H);
      const LpipsAxis c = lpips_axis(x0, w, 2 * a.W, a.inv2W);
      ci[q][0] = c.i0; ci[q][1] = min(c.i0 + 1, w - 1); ci[q][2] = min(c.i0 + 2, w - 1);
      // column k: numerator (2 (x0 + k) + 1) w - W = that of column 0 + 2 k w; 6 w < 2 W, so the quotient grows by at most 1
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int rem = max(c.rem + 2 * k * w, 0);
        up[q][k] = rem >= 2 * a.W;
        rem = up[q][k] ? rem - 2 * a.W : rem;
        tx[q][k] = (float)rem * a.inv2W;
      }
    }
#pragma unroll
    for (int l = 0; l < kLpipsLayers; ++l) {
      const int q = l < 2 ? l : 2, w = a.w[q];
      const float* const r0 = dimg + a.dl0[l] + r[q].i0 * w;
      const float* const r1 = dimg + a.dl0[l] + r[q].i1 * w;
      // the three source columns, interpolated along y
      const float v0 = r0[ci[q][0]] + r[q].t * (r1[ci[q][0]] - r0[ci[q][0]]);
      const float v1 = r0[ci[q][1]] + r[q].t * (r1[ci[q][1]] - r0[ci[q][1]]);
      const float v2 = r0[ci[q][2]] + r[q].t * (r1[ci[q][2]] - r0[ci[q][2]]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float lo = up[q][k] ? v1 : v0, hi = up[q][k] ? v2 : v1;
        D[k] += lo + tx[q][k] * (hi - lo);
      }
    }
    const size_t o = ((size_t)b * a.H + y) * a.W + x0;
    const int nv = min(4, a.W - x0);
    float Bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec) {                                               // (W % 4 == 0 and 16-byte aligned bases: nv == 4)
      const f32x4 d4 = {D[0], D[1], D[2], D[3]};
      if (a.out_map) *reinterpret_cast<f32x4*>(a.out_map + o) = d4;
      if (a.best_map) {
        f32x4 b4 = d4;
        if (!a.first) {
          const f32x4 old = *reinterpret_cast<const f32x4*>(a.best_map + o);
          b4.x = fminf(old.x, d4.x); b4.y = fminf(old.y, d4.y); b4.z = fminf(old.z, d4.z); b4.w = fminf(old.w, d4.w);
        }
        *reinterpret_cast<f32x4*>(a.best_map + o) = b4;
        Bv[0] = b4.x; Bv[1] = b4.y; Bv[2] = b4.z; Bv[3] = b4.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          if (a.out_map) a.out_map[o + k] = D[k];
          if (a.best_map) {
            Bv[k] = a.first ? D[k] : fminf(a.best_map[o + k], D[k]);
            a.best_map[o + k] = Bv[k];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nv) { sd += (double)D[k]; sb += (double)Bv[k]; }
    }
  }
  sd = wave_sum_f64(sd);
  sb = wave_sum_f64(sb);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wsum[wv][0] = sd; wsum[wv][1] = sb; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double t = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
    a.part[((size_t)b * a.nblk + blockIdx.x) * 2 + threadIdx.x] = t;
  }
}

// one block of 64 threads per image: lane t adds the blocks t, t + 64, .. in order, a butterfly adds the lanes; / (H W)
__global__ __launch_bounds__(64) void lpips_map_final_kernel(const double* __restrict__ part, int nblk, double hw,
                                                             float* __restrict__ out_map_mean, float* __restrict__ out_best_mean) {
  const int b = blockIdx.x, t = threadIdx.x;
  const double* p = part + (size_t)b * nblk * 2;
  double sd = 0.0, sb = 0.0;
  for (int k = t; k < nblk; k += 64) { sd += p[2 * k]; sb += p[2 * k + 1]; }
  sd = wave_sum_f64(sd);
  sb = wave_sum_f64(sb);
  if (t == 0) {
    if (out_map_mean) out_map_mean[b] = (float)(sd / hw);
    if (out_best_mean) out_best_mean[b] = (float)(sb / hw);
  }
}

struct LpipsFinalArgs {
  int chunk0[kLpipsLayers], nchunk[kLpipsLayers], hw[kLpipsLayers];
  int nchunk_total;
  const float* part;
  float* out;         // [B]
  float* out_layers;  // [B][5] or null
};

// one block per image: thread l sums layer l's partials in order (double), then thread 0 adds the five layer means in order
__global__ void lpips_final_kernel(const LpipsFinalArgs a) {
  __shared__ float lay[kLpipsLayers];
  const int b = blockIdx.x, l = threadIdx.x;
  if (l < kLpipsLayers) {
    const float* p = a.part + (size_t)b * a.nchunk_total + a.chunk0[l];
    double s = 0.0;
    for (int k = 0; k < a.nchunk[l]; ++k) s += (double)p[k];
    const float v = (float)(s / (double)a.hw[l]);
    lay[l] = v;
    if (a.out_layers) a.out_layers[(size_t)b * kLpipsLayers + l] = v;
  }
  __syncthreads();
  if (l == 0) {
    float v = lay[0];
    for (int k = 1; k < kLpipsLayers; ++k) v += lay[k];
    a.out[b] = v;
  }
}

static int lpips_grid(long long total, unsigned* g) {
  const long long n = (total + 255) / 256;
  if (n < 1 || n > 0x7fffffffLL) return HCF_ERR_ARG;
  *g = (unsigned)n;
  return HCF_OK;
}

// conv 5x5 pad 2 (TAPS = 25) of x [N][H][W][cin] (cin % 16 == 0) into y[..., oc0 .. oc0+64) of a cs_out-channel slab, bias + ReLU
static int lpips_conv5(const float* x, int cin, int N, int H, int W, const float* w, const float* bias, float* y, int cs_out,
                       int oc0, char* wk, const LpipsPlan& p, hipStream_t st) {
  return launch_conv_block(w + (size_t)oc0 * cin * 25, cin, 25, 0, 0, bias + oc0, 64, 64, mkview(const_cast<float*>(x), cin, 0, cin),
                           cin / 16, mkview(y, cs_out, oc0, 64), ACT_RELU, N, H, W, (float*)(wk + p.o_bias), (float*)(wk + p.o_scale),
                           (float*)(wk + p.o_pk), st);
}

static int lpips_pool(const float* in, int N, int Hst, int Wst, int C, int Ho, int Wo, float* out, hipStream_t st) {
  unsigned g;
  if (lpips_grid((long long)N * Ho * Wo * (C / 4), &g) != HCF_OK) return HCF_ERR_ARG;
  hipLaunchKernelGGL(lpips_maxpool_kernel, dim3(g), dim3(256), 0, st, in, N, Hst, Wst, C, Ho, Wo, out);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

// ---- backward (hcf_lpips_alex_backward): dL/d in0, dL/d in1 from gout[b] = dL/d out[b], the forward's workspace as the tape.
// The gradient slabs hold only the halves of the stacked batch that want a gradient: Nb = B or 2B images, gradient image m
// belongs to forward image m + off. Every kernel below is a gather with a fixed summation order: no atomics.
//   head      per layer and pixel, a_c = 2 w_c (f0_c / d0 - f1_c / d1) gout[b] / (h w), d_i = sqrt(n_i) + 1e-10:
//             g_f0_c = a_c / d0 - f0_c (sum_k a_k f0_k) / (d0^2 sqrt n0), g_f1 likewise with -a; the term through the norm is
//             DEFINED as 0 where n_i = 0 (autograd of the stock formulation gives 0 * inf = NaN there). Stored under the
//             producer's ReLU mask (f > 0).
//   conv5..3  data gradients through hcf_aux_conv2d_backward (dw = NULL); g_l = f_l > 0 ? g_l + dx : 0 joins the layer below
//   pool      MaxPool 3 / 2 backward as a gather: an element takes the gradient of each window (at most 2 x 2) whose FIRST
//             maximum in row-major order it is (PyTorch's rule), plus its head gradient, under the ReLU mask; the spare rows /
//             cols of the conv1 slab are written 0
//   conv2, 1  the 5x5 kernel on the tap-flipped transposed pack (launch_conv_block, transposed = 1)
//   un-prep   s2d gradient [Nb][Hs][Ws][48] -> NCHW [B,3,H,W]: / scale[c], * 2 with normalize, cropped to H x W
struct LpipsBwdPlan {
  int Nb, off;
  size_t o_g[kLpipsLayers], o_t, o_gp2, o_gp1, o_gs2d, o_pk, o_bias, o_scale, o_aux, aux_bytes, total;
};

static bool lpips_bwd_plan(int B, int which, const LpipsPlan& p, LpipsBwdPlan& q) {
  memset(&q, 0, sizeof(q));
  if (which < 1 || which > 3) return false;
  q.Nb = (which == 3) ? 2 * B : B;
  q.off = (which == 2) ? B : 0;
  const size_t N = (size_t)q.Nb, f = sizeof(float);
  const size_t gs = N * p.Hs * p.Ws, g2 = N * p.H2 * p.W2, g3 = N * p.H3 * p.W3;
  const size_t pix[kLpipsLayers] = {gs, g2, g3, g3, g3};
  size_t o = 256;
  auto take = [&](size_t bytes) { const size_t r = o; o += lp_al256(bytes); return r; };
  for (int l = 0; l < kLpipsLayers; ++l) q.o_g[l] = take(pix[l] * kAlexC[l] * f);
  q.o_t = take(g3 * 384 * f);                                   // dx of conv5 / conv4 before it joins g4 / g3
  q.o_gp2 = take(g3 * 192 * f);
  q.o_gp1 = take(g2 * 64 * f);
  q.o_gs2d = take(gs * 48 * f);
  q.o_pk = take(conv_pack_bytes(12, 25, 64));                   // conv2's data gradient: K = 192 = 12 chunks
  q.o_bias = take(64 * f);
  q.o_scale = take(64 * f);
  size_t aux = 0;
  for (int l = 2; l < kLpipsLayers; ++l)
    aux = std::max(aux, hcf_aux_conv2d_workspace(kAlexC[l - 1], kAlexC[l], 3, q.Nb, p.H3, p.W3));
  q.aux_bytes = aux;
  q.o_aux = take(aux);
  q.total = o;
  return aux > 0;
}

struct LpipsHeadBwdArgs {
  LpipsLayer L[kLpipsLayers];
  float* g[kLpipsLayers];   // [Nb][Hst][Wst][C], the layout of L[l].f
  int B, which;
  const float* gout;        // [B]
};

// the grid and the lane layout of lpips_head_kernel; n_i is summed in the same order as there
__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(const LpipsHeadBwdArgs a) {
  const int b = blockIdx.y, blk = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < kLpipsLayers; ++k) l = (blk >= a.L[k].chunk0) ? k : l;
  const LpipsLayer L = a.L[l];
  float* const gl = a.g[l];
  const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int hw = L.h * L.w, C = L.C, ni = C >> 6;
  const float eps = 1e-10f;
  const float s = a.gout[b] / (float)hw;
  const int m1 = (a.which == 3) ? a.B + b : b;                  // gradient image of the in1 half
  for (int k = 0; k < kHeadPix / 16; ++k) {
    const int p = (blk - L.chunk0) * kHeadPix + k * 16 + g;
    if (p >= hw) break;                                         // (uniform over the group)
    const int y = p / L.w, x = p - y * L.w;
    const size_t po = ((size_t)y * L.Wst + x) * C, img = (size_t)L.Hst * L.Wst * C;
    const float* f0 = L.f + (size_t)b * img + po;
    const float* f1 = L.f + (size_t)(a.B + b) * img + po;
    f32x4 v0[6], v1[6], ac[6];
    float n0 = 0.f, n1 = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < ni) {
        v0[i] = *reinterpret_cast<const f32x4*>(f0 + 4 * (j + 16 * i));
        v1[i] = *reinterpret_cast<const f32x4*>(f1 + 4 * (j + 16 * i));
        n0 += v0[i].x * v0[i].x + v0[i].y * v0[i].y + v0[i].z * v0[i].z + v0[i].w * v0[i].w;
        n1 += v1[i].x * v1[i].x + v1[i].y * v1[i].y + v1[i].z * v1[i].z + v1[i].w * v1[i].w;
      }
    }
    n0 = __shfl(group16_sum(n0), 0, 16);
    n1 = __shfl(group16_sum(n1), 0, 16);
    const float r0 = sqrtf(n0), r1 = sqrtf(n1);
    const float d0 = r0 + eps, d1 = r1 + eps;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < ni) {
        const float* w = L.lin + 4 * (j + 16 * i);
        f32x4 t;
        t.x = 2.f * w[0] * (v0[i].x / d0 - v1[i].x / d1) * s; t.y = 2.f * w[1] * (v0[i].y / d0 - v1[i].y / d1) * s;
        t.z = 2.f * w[2] * (v0[i].z / d0 - v1[i].z / d1) * s; t.w = 2.f * w[3] * (v0[i].w / d0 - v1[i].w / d1) * s;
        ac[i] = t;
        s0 += t.x * v0[i].x + t.y * v0[i].y + t.z * v0[i].z + t.w * v0[i].w;
        s1 += t.x * v1[i].x + t.y * v1[i].y + t.z * v1[i].z + t.w * v1[i].w;
      }
    }
    s0 = __shfl(group16_sum(s0), 0, 16);
    s1 = __shfl(group16_sum(s1), 0, 16);
    const float k0 = (n0 > 0.f) ? s0 / (d0 * d0 * r0) : 0.f;   // n == 0: the term through the norm is defined as 0
    const float k1 = (n1 > 0.f) ? s1 / (d1 * d1 * r1) : 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < ni) {
        const f32x4 t = ac[i], u0 = v0[i], u1 = v1[i];
        if (a.which & 1) {
          f32x4 o;
          o.x = u0.x > 0.f ? t.x / d0 - u0.x * k0 : 0.f; o.y = u0.y > 0.f ? t.y / d0 - u0.y * k0 : 0.f;
          o.z = u0.z > 0.f ? t.z / d0 - u0.z * k0 : 0.f; o.w = u0.w > 0.f ? t.w / d0 - u0.w * k0 : 0.f;
          *reinterpret_cast<f32x4*>(gl + (size_t)b * img + po + 4 * (j + 16 * i)) = o;
        }
        if (a.which & 2) {
          f32x4 o;
          o.x = u1.x > 0.f ? u1.x * k1 - t.x / d1 : 0.f; o.y = u1.y > 0.f ? u1.y * k1 - t.y / d1 : 0.f;
          o.z = u1.z > 0.f ? u1.z * k1 - t.z / d1 : 0.f; o.w = u1.w > 0.f ? u1.w * k1 - t.w / d1 : 0.f;
          *reinterpret_cast<f32x4*>(gl + (size_t)m1 * img + po + 4 * (j + 16 * i)) = o;
        }
      }
    }
  }
}

// g = f > 0 ? g + t : 0 over n4 float4 units (f: the forward slab from its image `off` on)
__global__ __launch_bounds__(256) void lpips_relu_join_kernel(const float* __restrict__ f, const float* __restrict__ t,
                                                              float* __restrict__ g, long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 fv = reinterpret_cast<const f32x4*>(f)[i], tv = reinterpret_cast<const f32x4*>(t)[i];
  f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
  gv.x = fv.x > 0.f ? gv.x + tv.x : 0.f; gv.y = fv.y > 0.f ? gv.y + tv.y : 0.f;
  gv.z = fv.z > 0.f ? gv.z + tv.z : 0.f; gv.w = fv.w > 0.f ? gv.w + tv.w : 0.f;
  reinterpret_cast<f32x4*>(g)[i] = gv;
}

// MaxPool 3 / 2 backward + the producer's ReLU mask + the head gradient already in g. One thread per float4 of the pool's INPUT
// slab g [Nb][Hst][Wst][C] (valid Hin x Win; beyond: 0). f [.][Hst][Wst][C] and the pool output p [.][Ho][Wo][C] are the
// forward's, read from image `off` on; gp [Nb][Ho][Wo][C] is the gradient of the pool output. An element with f > 0 that equals a
// window's maximum takes that window's gradient unless an EARLIER element of the window (row-major) equals it too.
__global__ __launch_bounds__(256) void lpips_pool_bwd_kernel(const float* __restrict__ f, const float* __restrict__ p,
                                                             const float* __restrict__ gp, float* __restrict__ g, int Nb, int off,
                                                             int Hst, int Wst, int Hin, int Win, int C, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C4 = C >> 2;
  const long long total = (long long)Nb * Hst * Wst * C4;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  const long long pix = i / C4;
  const int x = (int)(pix % Wst);
  const int y = (int)((pix / Wst) % Hst);
  const int m = (int)(pix / ((long long)Wst * Hst));
  f32x4* gptr = reinterpret_cast<f32x4*>(g + (size_t)pix * C + 4 * c4);
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (y < Hin && x < Win) {
    const float* fb = f + (size_t)(m + off) * Hst * Wst * C + 4 * c4;
    const f32x4 me = *reinterpret_cast<const f32x4*>(fb + ((size_t)y * Wst + x) * C);
    if (me.x > 0.f || me.y > 0.f || me.z > 0.f || me.w > 0.f) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int oy0 = max((y - 1) >> 1, 0), oy1 = min(y >> 1, Ho - 1);
      const int ox0 = max((x - 1) >> 1, 0), ox1 = min(x >> 1, Wo - 1);
      for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
          const size_t wo = ((size_t)oy * Wo + ox) * C + 4 * c4;
          const f32x4 pv = *reinterpret_cast<const f32x4*>(p + (size_t)(m + off) * Ho * Wo * C + wo);
          bool cx = me.x > 0.f && me.x == pv.x, cy = me.y > 0.f && me.y == pv.y;
          bool cz = me.z > 0.f && me.z == pv.z, cw = me.w > 0.f && me.w == pv.w;
          if (!(cx || cy || cz || cw)) continue;
          for (int yy = 2 * oy; yy <= y; ++yy) {                 // the elements of the window before (y, x)
            const int xe = (yy < y) ? 2 * ox + 3 : x;
            for (int xx = 2 * ox; xx < xe; ++xx) {
              const f32x4 e = *reinterpret_cast<const f32x4*>(fb + ((size_t)yy * Wst + xx) * C);
              cx = cx && e.x != pv.x; cy = cy && e.y != pv.y; cz = cz && e.z != pv.z; cw = cw && e.w != pv.w;
            }
          }
          const f32x4 gv = *reinterpret_cast<const f32x4*>(gp + (size_t)m * Ho * Wo * C + wo);
          acc.x += cx ? gv.x : 0.f; acc.y += cy ? gv.y : 0.f; acc.z += cz ? gv.z : 0.f; acc.w += cw ? gv.w : 0.f;
        }
      const f32x4 hg = *gptr;
      o.x = me.x > 0.f ? hg.x + acc.x : 0.f; o.y = me.y > 0.f ? hg.y + acc.y : 0.f;
      o.z = me.z > 0.f ? hg.z + acc.z : 0.f; o.w = me.w > 0.f ? hg.w + acc.w : 0.f;
    }
  }
  *gptr = o;
}

// un-prep: one thread per (gradient image m, s2d row Y, unit q = c * 4 + a, s2d column X): the 4 image columns 4X .. 4X+3 of row
// 4Y + a, channel c. Image m < B goes to ga, the others to gb.
__global__ __launch_bounds__(256) void lpips_unprep_kernel(const float* __restrict__ gs, int Nb, int B, int H, int W, int Hs,
                                                           int Ws, int normalize, const float* __restrict__ scale,
                                                           float* __restrict__ ga, float* __restrict__ gb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)Nb * Hs * 12 * Ws;
  if (i >= total) return;
  const int X = (int)(i % Ws);
  const int q = (int)((i / Ws) % 12);
  const int Y = (int)((i / ((long long)Ws * 12)) % Hs);
  const int m = (int)(i / ((long long)Ws * 12 * Hs));
  const int c = q >> 2, y = 4 * Y + (q & 3);
  if (y >= H) return;
  const f32x4 v = *reinterpret_cast<const f32x4*>(gs + (((size_t)m * Hs + Y) * Ws + X) * 48 + q * 4);
  const float sc = scale[c], mul = normalize ? 2.f : 1.f;
  float* dst = ((m < B) ? ga + (size_t)m * 3 * H * W : gb + (size_t)(m - B) * 3 * H * W) + ((size_t)c * H + y) * W;
  const float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = 4 * X + k;
    if (xx < W) dst[xx] = r[k] / sc * mul;
  }
}

}  // namespace hcf

using namespace hcf;

extern "C" {

size_t hcf_lpips_workspace(int32_t B, int32_t H, int32_t W) {
  LpipsPlan p;
  return lpips_plan(B, H, W, p) ? p.total : 0;
}

// prep, conv1, pool1, conv2, pool2, conv3..5 over the N images of plan p (N = 2B: in0 and in1 stacked; N = B: in0 alone) into `wk`
static int lpips_features(const float* in0, const float* in1, int B, int N, int H, int W, int normalize, const float* const* params,
                          char* wk, const LpipsPlan& p, hcf_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  float *s2d = (float*)(wk + p.o_s2d), *f1 = (float*)(wk + p.o_f1), *p1 = (float*)(wk + p.o_p1), *f2 = (float*)(wk + p.o_f2);
  float *p2 = (float*)(wk + p.o_p2), *f3 = (float*)(wk + p.o_f3), *f4 = (float*)(wk + p.o_f4), *f5 = (float*)(wk + p.o_f5);
  const float *shift = params[0], *scale = params[1];
  const float* cw[kLpipsLayers] = {params[2], params[4], params[6], params[8], params[10]};
  const float* cb[kLpipsLayers] = {params[3], params[5], params[7], params[9], params[11]};

  unsigned g;
  if (lpips_grid((long long)N * p.Hs * p.Ws * 12, &g) != HCF_OK) return HCF_ERR_ARG;
  hipLaunchKernelGGL(lpips_prep_kernel, dim3(g), dim3(256), 0, st, in0, in1, B, N, H, W, p.Hs, p.Ws, normalize, shift, scale, s2d);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  int rc = lpips_conv5(s2d, 48, N, p.Hs, p.Ws, cw[0], cb[0], f1, 64, 0, wk, p, st);
  if (rc == HCF_OK) rc = lpips_pool(f1, N, p.Hs, p.Ws, 64, p.H2, p.W2, p1, st);
  for (int oc0 = 0; oc0 < 192 && rc == HCF_OK; oc0 += 64) rc = lpips_conv5(p1, 64, N, p.H2, p.W2, cw[1], cb[1], f2, 192, oc0, wk, p, st);
  if (rc == HCF_OK) rc = lpips_pool(f2, N, p.H2, p.W2, 192, p.H3, p.W3, p2, st);
  if (rc != HCF_OK) return rc;
  void* aux = wk + p.o_aux;
  if (hipMemsetAsync(aux, 0, 256, st) != hipSuccess) return HCF_ERR_HIP;          // hcf_aux_conv2d's flag + zero page
  const float* xin[3] = {p2, f3, f4};
  float* yout[3] = {f3, f4, f5};
  for (int l = 2; l < kLpipsLayers && rc == HCF_OK; ++l)
    rc = hcf_aux_conv2d(xin[l - 2], kAlexC[l - 1], kAlexC[l - 1], N, p.H3, p.W3, cw[l], cb[l], kAlexC[l], 3, ACT_RELU,
                        yout[l - 2], kAlexC[l], aux, p.aux_bytes, HCF_PRECISION_EXACT, stream);
  return rc;
}

// the head's view of the five feature maps in `wk` (plan p), and the final kernel's chunk table
static void lpips_head_layers(const char* wk, const LpipsPlan& p, const float* const* params, LpipsLayer* L, LpipsFinalArgs* fa) {
  const size_t feat[kLpipsLayers] = {p.o_f1, p.o_f2, p.o_f3, p.o_f4, p.o_f5};
  const int hst[kLpipsLayers] = {p.Hs, p.H2, p.H3, p.H3, p.H3}, wst[kLpipsLayers] = {p.Ws, p.W2, p.W3, p.W3, p.W3};
  const int hh[kLpipsLayers] = {p.H1, p.H2, p.H3, p.H3, p.H3}, ww[kLpipsLayers] = {p.W1, p.W2, p.W3, p.W3, p.W3};
  for (int l = 0; l < kLpipsLayers; ++l) {
    L[l].f = (const float*)(wk + feat[l]); L[l].C = kAlexC[l]; L[l].Hst = hst[l]; L[l].Wst = wst[l]; L[l].h = hh[l]; L[l].w = ww[l];
    L[l].chunk0 = p.chunk0[l];
    L[l].lin = params[12 + l];
    fa->chunk0[l] = p.chunk0[l]; fa->nchunk[l] = p.nchunk[l]; fa->hw[l] = hh[l] * ww[l];
  }
  fa->nchunk_total = p.nchunk_total;
}

int hcf_lpips_alex(const float* in0, const float* in1, int32_t B, int32_t H, int32_t W, int32_t normalize,
                   const float* const* params, float* out, float* out_layers, void* work, size_t work_bytes,
                   hcf_stream_t stream) {
  if (!in0 || !in1 || !params || !out || !work) return HCF_ERR_ARG;
  for (int i = 0; i < HCF_LPIPS_NPARAMS; ++i)
    if (!params[i]) return HCF_ERR_ARG;
  LpipsPlan p;
  if (!lpips_plan(B, H, W, p)) return HCF_ERR_SHAPE;
  if (work_bytes < p.total) return HCF_ERR_NOMEM;
  hipStream_t st = (hipStream_t)stream;
  char* wk = (char*)work;
  const int rc = lpips_features(in0, in1, B, 2 * B, H, W, normalize, params, wk, p, stream);
  if (rc != HCF_OK) return rc;

  LpipsHeadArgs h;
  memset(&h, 0, sizeof(h));
  LpipsFinalArgs fa;
  memset(&fa, 0, sizeof(fa));
  lpips_head_layers(wk, p, params, h.L, &fa);
  h.B = B; h.nchunk_total = p.nchunk_total; h.part = (float*)(wk + p.o_part);
  hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)p.nchunk_total, (unsigned)B), dim3(256), 0, st, h);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  fa.part = h.part; fa.out = out; fa.out_layers = out_layers;
  hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)B), dim3(64), 0, st, fa);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

// ---- one embedded input and the map against it (hcflow_amd/lpips.py: LPIPSMap). The store of hcf_lpips_alex_embed and the
// front of hcf_lpips_alex_map's work are one B-image plan; behind it the map call keeps the layer maps d_l, the map kernel's
// fp64 partials and a [B] vector for the final kernel when `out` is not asked for.
struct LpipsMapPlan {
  int dl0[kLpipsLayers], dl_total, W4, nblk;
  size_t o_dl, o_mpart, o_out, total;
};

static bool lpips_map_plan(int B, int H, int W, LpipsPlan& p, LpipsMapPlan& q) {
  memset(&q, 0, sizeof(q));
  if (!lpips_plan_n(B, B, H, W, p)) return false;
  const int hw[kLpipsLayers] = {p.H1 * p.W1, p.H2 * p.W2, p.H3 * p.W3, p.H3 * p.W3, p.H3 * p.W3};
  for (int l = 0; l < kLpipsLayers; ++l) { q.dl0[l] = q.dl_total; q.dl_total += hw[l]; }
  q.W4 = (W + 3) / 4;
  q.nblk = (int)(((long long)H * q.W4 + 255) / 256);
  size_t o = p.total;
  auto take = [&](size_t bytes) { const size_t r = o; o += lp_al256(bytes); return r; };
  q.o_dl = take((size_t)B * q.dl_total * sizeof(float));
  q.o_mpart = take((size_t)B * q.nblk * 2 * sizeof(double));
  q.o_out = take((size_t)B * sizeof(float));
  q.total = o;
  return true;
}

size_t hcf_lpips_embed_bytes(int32_t B, int32_t H, int32_t W) {
  LpipsPlan p;
  return lpips_plan_n(B, B, H, W, p) ? p.total : 0;
}

int hcf_lpips_alex_embed(const float* x, int32_t B, int32_t H, int32_t W, int32_t normalize, const float* const* params,
                         void* store, size_t store_bytes, hcf_stream_t stream) {
  if (!x || !params || !store) return HCF_ERR_ARG;
  for (int i = 0; i < HCF_LPIPS_NPARAMS; ++i)
    if (!params[i]) return HCF_ERR_ARG;
  LpipsPlan p;
  if (!lpips_plan_n(B, B, H, W, p)) return HCF_ERR_SHAPE;
  if (store_bytes < p.total) return HCF_ERR_NOMEM;
  return lpips_features(x, x, B, B, H, W, normalize, params, (char*)store, p, stream);
}

size_t hcf_lpips_map_workspace(int32_t B, int32_t H, int32_t W) {
  LpipsPlan p;
  LpipsMapPlan q;
  return lpips_map_plan(B, H, W, p, q) ? q.total : 0;
}

int hcf_lpips_alex_map(const void* ref_store, size_t ref_bytes, const float* x, int32_t B, int32_t H, int32_t W,
                       int32_t normalize, const float* const* params, float* out, float* out_layers, float* out_map,
                       float* out_map_mean, float* best_map, float* out_best_mean, int32_t first, void* work, size_t work_bytes,
                       hcf_stream_t stream) {
  if (!ref_store || !x || !params || !work || (out_best_mean && !best_map)) return HCF_ERR_ARG;
  for (int i = 0; i < HCF_LPIPS_NPARAMS; ++i)
    if (!params[i]) return HCF_ERR_ARG;
  LpipsPlan p;
  LpipsMapPlan q;
  if (!lpips_map_plan(B, H, W, p, q)) return HCF_ERR_SHAPE;
  if (ref_bytes < p.total || work_bytes < q.total) return HCF_ERR_NOMEM;
  hipStream_t st = (hipStream_t)stream;
  char* wk = (char*)work;
  const int rc = lpips_features(x, x, B, B, H, W, normalize, params, wk, p, stream);
  if (rc != HCF_OK) return rc;

  LpipsHead2Args h;
  memset(&h, 0, sizeof(h));
  LpipsLayer ref[kLpipsLayers];
  LpipsFinalArgs fa, fa_ref;
  memset(&fa, 0, sizeof(fa));
  lpips_head_layers(wk, p, params, h.L, &fa);
  lpips_head_layers((const char*)ref_store, p, params, ref, &fa_ref);
  for (int l = 0; l < kLpipsLayers; ++l) { h.fr[l] = ref[l].f; h.dl0[l] = q.dl0[l]; }
  h.dl_total = q.dl_total; h.nchunk_total = p.nchunk_total;
  h.dl = (float*)(wk + q.o_dl); h.part = (float*)(wk + p.o_part);
  hipLaunchKernelGGL(lpips_head2_kernel, dim3((unsigned)p.nchunk_total, (unsigned)B), dim3(256), 0, st, h);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  if (out || out_layers) {
    fa.part = h.part; fa.out = out ? out : (float*)(wk + q.o_out); fa.out_layers = out_layers;
    hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)B), dim3(64), 0, st, fa);
    if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  }
  if (!out_map && !out_map_mean && !best_map) return HCF_OK;

  LpipsMapArgs m;
  memset(&m, 0, sizeof(m));
  m.dl = h.dl; m.dl_total = q.dl_total;
  for (int l = 0; l < kLpipsLayers; ++l) m.dl0[l] = q.dl0[l];
  const int gh[3] = {p.H1, p.H2, p.H3}, gw[3] = {p.W1, p.W2, p.W3};
  for (int g = 0; g < 3; ++g) { m.h[g] = gh[g]; m.w[g] = gw[g]; }
  m.H = H; m.W = W; m.W4 = q.W4; m.nblk = q.nblk; m.first = first != 0;
  m.inv2H = 1.f / (float)(2 * H); m.inv2W = 1.f / (float)(2 * W); m.invW4 = 1.f / (float)q.W4;
  m.vec = (W % 4 == 0) && (((uintptr_t)out_map | (uintptr_t)best_map) & 15) == 0;
  m.out_map = out_map; m.best_map = best_map; m.part = (double*)(wk + q.o_mpart);
  hipLaunchKernelGGL(lpips_map_kernel, dim3((unsigned)q.nblk, (unsigned)B), dim3(256), 0, st, m);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  if (!out_map_mean && !out_best_mean) return HCF_OK;
  hipLaunchKernelGGL(lpips_map_final_kernel, dim3((unsigned)B), dim3(64), 0, st, m.part, q.nblk, (double)H * (double)W,
                     out_map_mean, out_best_mean);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

size_t hcf_lpips_backward_workspace(int32_t B, int32_t H, int32_t W, int32_t which) {
  LpipsPlan p;
  LpipsBwdPlan q;
  return (lpips_plan(B, H, W, p) && lpips_bwd_plan(B, which, p, q)) ? q.total : 0;
}

int hcf_lpips_alex_backward(int32_t B, int32_t H, int32_t W, int32_t normalize, const float* const* params, const float* gout,
                            int32_t which, float* gin0, float* gin1, const void* fwd_work, size_t fwd_work_bytes, void* work,
                            size_t work_bytes, hcf_stream_t stream) {
  if (!params || !gout || !fwd_work || !work || which < 1 || which > 3 || ((which & 1) && !gin0) || ((which & 2) && !gin1))
    return HCF_ERR_ARG;
  for (int i = 0; i < HCF_LPIPS_NPARAMS; ++i)
    if (!params[i]) return HCF_ERR_ARG;
  LpipsPlan p;
  LpipsBwdPlan q;
  if (!lpips_plan(B, H, W, p) || !lpips_bwd_plan(B, which, p, q)) return HCF_ERR_SHAPE;
  if (fwd_work_bytes < p.total || work_bytes < q.total) return HCF_ERR_NOMEM;
  hipStream_t st = (hipStream_t)stream;
  const char* fw = (const char*)fwd_work;
  char* wk = (char*)work;
  const int Nb = q.Nb, off = q.off;
  const float* feat[kLpipsLayers] = {(const float*)(fw + p.o_f1), (const float*)(fw + p.o_f2), (const float*)(fw + p.o_f3),
                                     (const float*)(fw + p.o_f4), (const float*)(fw + p.o_f5)};
  const float *p1 = (const float*)(fw + p.o_p1), *p2 = (const float*)(fw + p.o_p2);
  float* g[kLpipsLayers];
  for (int l = 0; l < kLpipsLayers; ++l) g[l] = (float*)(wk + q.o_g[l]);
  float *t = (float*)(wk + q.o_t), *gp2 = (float*)(wk + q.o_gp2), *gp1 = (float*)(wk + q.o_gp1), *gs2d = (float*)(wk + q.o_gs2d);
  float *bvec = (float*)(wk + q.o_bias), *svec = (float*)(wk + q.o_scale), *pk = (float*)(wk + q.o_pk);
  const float* cw[kLpipsLayers] = {params[2], params[4], params[6], params[8], params[10]};
  const int hst[kLpipsLayers] = {p.Hs, p.H2, p.H3, p.H3, p.H3}, wst[kLpipsLayers] = {p.Ws, p.W2, p.W3, p.W3, p.W3};
  const int hh[kLpipsLayers] = {p.H1, p.H2, p.H3, p.H3, p.H3}, ww[kLpipsLayers] = {p.W1, p.W2, p.W3, p.W3, p.W3};

  // ---- head: the ReLU-masked head gradient of all five layers, for the halves asked for
  LpipsHeadBwdArgs h;
  memset(&h, 0, sizeof(h));
  for (int l = 0; l < kLpipsLayers; ++l) {
    h.L[l].f = feat[l]; h.L[l].C = kAlexC[l]; h.L[l].Hst = hst[l]; h.L[l].Wst = wst[l]; h.L[l].h = hh[l]; h.L[l].w = ww[l];
    h.L[l].chunk0 = p.chunk0[l];
    h.L[l].lin = params[12 + l];
    h.g[l] = g[l];
  }
  h.B = B; h.which = which; h.gout = gout;
  hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3((unsigned)p.nchunk_total, (unsigned)B), dim3(256), 0, st, h);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;

  // ---- conv5, conv4, conv3: g5 -> t -> g4 -> t -> g3 -> gp2
  void* aux = wk + q.o_aux;
  if (hipMemsetAsync(aux, 0, 256, st) != hipSuccess) return HCF_ERR_HIP;
  const size_t img3 = (size_t)p.H3 * p.W3;
  unsigned grid;
  int rc = HCF_OK;
  for (int l = 4; l >= 2; --l) {
    const int cin = kAlexC[l - 1];
    const float* xin = ((l == 2) ? p2 : feat[l - 1]) + (size_t)off * img3 * cin;   // conv l's input, from the first wanted image on
    rc = hcf_aux_conv2d_backward(xin, cin, cin, Nb, p.H3, p.W3, cw[l], kAlexC[l], 3, g[l], kAlexC[l], (l == 2) ? gp2 : t, cin,
                                 nullptr, aux, q.aux_bytes, HCF_PRECISION_EXACT, stream);
    if (rc != HCF_OK) return rc;
    if (l == 2) break;                                          // conv3's input is pool2's output: no ReLU, no head term
    const long long n4 = (long long)Nb * (long long)img3 * (cin / 4);
    if (lpips_grid(n4, &grid) != HCF_OK) return HCF_ERR_ARG;
    hipLaunchKernelGGL(lpips_relu_join_kernel, dim3(grid), dim3(256), 0, st, xin, t, g[l - 1], n4);
    if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  }

  // ---- pool2, conv2, pool1 (which also clears the spare rows / cols of the conv1 slab), conv1
  if (lpips_grid((long long)Nb * p.H2 * p.W2 * (192 / 4), &grid) != HCF_OK) return HCF_ERR_ARG;
  hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3(grid), dim3(256), 0, st, feat[1], p2, gp2, g[1], Nb, off, p.H2, p.W2, p.H2, p.W2,
                     192, p.H3, p.W3);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  rc = launch_conv_block(cw[1], 64, 25, 1, 0, nullptr, 64, 64, mkview(g[1], 192, 0, 192), 12, mkview(gp1, 64, 0, 64), ACT_NONE, Nb,
                         p.H2, p.W2, bvec, svec, pk, st);
  if (rc != HCF_OK) return rc;
  if (lpips_grid((long long)Nb * p.Hs * p.Ws * (64 / 4), &grid) != HCF_OK) return HCF_ERR_ARG;
  hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3(grid), dim3(256), 0, st, feat[0], p1, gp1, g[0], Nb, off, p.Hs, p.Ws, p.H1, p.W1,
                     64, p.H2, p.W2);
  if (hipGetLastError() != hipSuccess) return HCF_ERR_HIP;
  rc = launch_conv_block(cw[0], 48, 25, 1, 0, nullptr, 48, 64, mkview(g[0], 64, 0, 64), 4, mkview(gs2d, 48, 0, 48), ACT_NONE, Nb,
                         p.Hs, p.Ws, bvec, svec, pk, st);
  if (rc != HCF_OK) return rc;

  // ---- un-prep
  if (lpips_grid((long long)Nb * p.Hs * 12 * p.Ws, &grid) != HCF_OK) return HCF_ERR_ARG;
  hipLaunchKernelGGL(lpips_unprep_kernel, dim3(grid), dim3(256), 0, st, gs2d, Nb, B, H, W, p.Hs, p.Ws, normalize, params[1],
                     (which & 1) ? gin0 : gin1, gin1);
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

}  // extern "C"
