// MATLAB-style bicubic resize of fp32 NCHW tensors on the device, down (antialiased) and up by an integer factor 2 .. 8, with
// its exact transpose as the backward (utils/imresize.py::imresize, float input, bicubic; no clipping).
//
// Per axis the op is the matrix A of contributions() (hcf_bicubic_tables.h): y = A_h x A_w^T, rows first. The weights are
// computed in float64 on the host and rounded once to fp32; every pass is one fp32 fma chain per output element in the table's
// entry order, so a result is a function of the image alone: bit-reproducible, independent of the batch, no atomics.
//
//   forward    resize_h_kernel (x -> t [Ho x W], table of A_h), resize_w_kernel (t -> y [Ho x Wo], table of A_w)
//   backward   gx = A_h^T gy A_w, columns first, in GATHER form over transposed tables (per input index the list of
//              (output index, weight) entries in ascending (output, tap) order, mirrored duplicates kept apart):
//              resize_w_kernel (gy -> u [Ho x W], table of A_w^T), resize_h_kernel (u -> gx [H x W], table of A_h^T)
//
// Both kernels are the same program on either kind of table: per output index a list of cnt (index, weight) entries. A block
// owns a tile of outputs; the host has recorded, per tile of output indices, the span [lo, hi] of source indices its lists
// touch (mirroring only folds the range, so the span stays about tile * s + taps), and the block stages exactly that span in
// LDS: each source element is read from memory once per block, with 16-byte loads where the row base and the row length allow
// and 4-byte loads with the same arithmetic otherwise.
//   resize_h_kernel: tile 16 output rows x 64 columns; LDS [span][64] floats; a thread owns 4 adjacent columns of one output
//     row, reads them as one float4 per entry (16 lanes = one 256-byte bank row: no conflicts) and stores 16 bytes.
//   resize_w_kernel: tile 16 rows x 64 outputs; LDS [16][stride], element j of a row at j + (j >> 5): neighbouring outputs read
//     s floats apart, and the one-in-32 padding spreads 32 lanes over 32 banks for every s in 2 .. 8. A lane owns one output
//     column and 4 rows, so a wave stores 256 contiguous bytes per row.
// Tables are tap-major on the device ([k][rows]): the lanes of resize_w_kernel read consecutive addresses.
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "../../include/hcflow.h"
#include "hcf_common.h"
#include "hcf_bicubic_tables.h"

namespace hcf {
namespace rsz {

#define RZ_ROWS 16
#define RZ_COLS 64
#define RZ_GRID_Y 65535
#define RZ_LDS_MAX 65536

// ---- host tables ---------------------------------------------------------------------------------------------------------
// rows lists of up to L entries; entry k of row r at [r * L + k] (idx -1 / weight 0 behind cnt[r]). Forward: row = output index,
// entries = its P taps in tap order. Transposed: row = input index, entries = (output, weight) in ascending (output, tap) order.
struct HostTable {
  int rows = 0, n_src = 0, L = 0;
  std::vector<double> w;
  std::vector<int> idx, cnt;
};

static int out_len_of(int in_len, int s, int up) { return up ? in_len * s : (in_len + s - 1) / s; }

static void build_table(int in_len, int s, int up, int transposed, HostTable& t) {
  const int out_len = out_len_of(in_len, s, up);
  std::vector<double> w;
  std::vector<int> idx;
  int P = 0;
  contributions(in_len, out_len, up ? (double)s : 1.0 / s, w, idx, P);
  if (!transposed) {
    t.rows = out_len; t.n_src = in_len; t.L = P;
    t.w = w; t.idx = idx;
    t.cnt.assign((size_t)out_len, P);
    return;
  }
  t.rows = in_len; t.n_src = out_len;
  t.cnt.assign((size_t)in_len, 0);
  for (size_t e = 0; e < idx.size(); ++e) ++t.cnt[idx[e]];
  t.L = 0;
  for (int i = 0; i < in_len; ++i) t.L = t.cnt[i] > t.L ? t.cnt[i] : t.L;
  t.w.assign((size_t)in_len * t.L, 0.0);
  t.idx.assign((size_t)in_len * t.L, -1);
  std::vector<int> fill((size_t)in_len, 0);
  for (int o = 0; o < out_len; ++o)
    for (int k = 0; k < P; ++k) {
      const int i = idx[(size_t)o * P + k];
      const size_t at = (size_t)i * t.L + fill[i]++;
      t.idx[at] = o;
      t.w[at] = w[(size_t)o * P + k];
    }
}

// ---- device tables -------------------------------------------------------------------------------------------------------
struct DevTable {
  int rows = 0, n_src = 0, L = 0;
  int span_h = 0, span_w = 0;          // longest source span of a tile of RZ_ROWS / RZ_COLS list rows
  const int* cnt = nullptr;            // [rows]
  const int* idx = nullptr;            // [L][rows]
  const float* w = nullptr;            // [L][rows]
  const int2* tile_h = nullptr;        // [ceil(rows / RZ_ROWS)] {lo, hi}
  const int2* tile_w = nullptr;        // [ceil(rows / RZ_COLS)]
};

static void spans(const HostTable& t, int tile, std::vector<int2>& out, int& longest) {
  const int nt = (t.rows + tile - 1) / tile;
  out.resize((size_t)nt);
  longest = 1;
  for (int b = 0; b < nt; ++b) {
    int lo = INT_MAX, hi = -1;
    for (int r = b * tile; r < t.rows && r < (b + 1) * tile; ++r)
      for (int k = 0; k < t.cnt[r]; ++k) {
        const int i = t.idx[(size_t)r * t.L + k];
        lo = i < lo ? i : lo; hi = i > hi ? i : hi;
      }
    if (hi < 0) lo = hi = 0;
    out[(size_t)b] = make_int2(lo, hi);
    longest = hi - lo + 1 > longest ? hi - lo + 1 : longest;
  }
}

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// One table per (device, length, factor, direction, transposed), uploaded at its first use (allocates, copies and waits once)
// and kept for the life of the process; every later call finds it here and touches neither the allocator nor the host.
static int table_for(int len, int s, int up, int transposed, DevTable& out) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int, int>, DevTable> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return HCF_ERR_HIP;
  std::lock_guard<std::mutex> g(mu);
  const auto key = std::make_tuple(dev, len, s, up, transposed);
  auto it = cache.find(key);
  if (it != cache.end()) { out = it->second; return HCF_OK; }
  HostTable h;
  build_table(len, s, up, transposed, h);
  std::vector<int2> th, tw;
  DevTable d;
  d.rows = h.rows; d.n_src = h.n_src; d.L = h.L;
  spans(h, RZ_ROWS, th, d.span_h);
  spans(h, RZ_COLS, tw, d.span_w);
  const size_t n = (size_t)h.rows * h.L;
  const size_t o_cnt = 0, o_idx = up16(o_cnt + sizeof(int) * h.rows), o_w = up16(o_idx + sizeof(int) * n),
               o_th = up16(o_w + sizeof(float) * n), o_tw = up16(o_th + sizeof(int2) * th.size()),
               bytes = up16(o_tw + sizeof(int2) * tw.size());
  std::vector<char> img(bytes, 0);
  int* pc = (int*)(img.data() + o_cnt);
  int* pi = (int*)(img.data() + o_idx);
  float* pw = (float*)(img.data() + o_w);
  for (int r = 0; r < h.rows; ++r) {
    pc[r] = h.cnt[r];
    for (int k = 0; k < h.L; ++k) {                                // tap-major; unused slots: index 0, weight 0, never read
      const int i = h.idx[(size_t)r * h.L + k];
      pi[(size_t)k * h.rows + r] = i < 0 ? 0 : i;
      pw[(size_t)k * h.rows + r] = (float)h.w[(size_t)r * h.L + k];
    }
  }
  memcpy(img.data() + o_th, th.data(), sizeof(int2) * th.size());
  memcpy(img.data() + o_tw, tw.data(), sizeof(int2) * tw.size());
  char* p = nullptr;
  if (hipMalloc((void**)&p, bytes) != hipSuccess) return HCF_ERR_NOMEM;
  if (hipMemcpy(p, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { hipFree(p); return HCF_ERR_HIP; }
  d.cnt = (const int*)(p + o_cnt); d.idx = (const int*)(p + o_idx); d.w = (const float*)(p + o_w);
  d.tile_h = (const int2*)(p + o_th); d.tile_w = (const int2*)(p + o_tw);
  cache[key] = d;
  out = d;
  return HCF_OK;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------
struct Pass {
  const float* src; float* dst;
  long long planes;
  size_t src_plane, dst_plane;         // floats per plane
  int n_src, n_dst;                    // lengths of the resampled axis
  int other;                           // length of the other axis (H pass: W, W pass: rows)
  int rows;                            // list rows of the table (= n_dst)
  const int* cnt; const int* idx; const float* w; const int2* tile;
  int tiles_x;                         // tiles along W (H pass) / along the outputs (W pass)
  int vec_src, vec_dst;                // 16-byte accesses allowed (base and row length)
  int stride;                          // W pass: floats between LDS rows
};

__device__ __forceinline__ int lds_pos(int j) { return j + (j >> 5); }

__global__ __launch_bounds__(256) void resize_h_kernel(Pass p) {
  extern __shared__ float4 rz_lds4[];                             // [span][RZ_COLS / 4]
  const long long plane = (long long)blockIdx.z * RZ_GRID_Y + blockIdx.y;
  if (plane >= p.planes) return;
  const int tid = threadIdx.x, W = p.other;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int x0 = tx * RZ_COLS, o0 = ty * RZ_ROWS;
  const int2 sp = p.tile[ty];
  const int nq = (sp.y - sp.x + 1) * (RZ_COLS / 4);
  const float* s = p.src + (size_t)plane * p.src_plane;
  for (int q = tid; q < nq; q += 256) {
    const int gx = x0 + (q & 15) * 4;
    const float* row = s + (size_t)(sp.x + (q >> 4)) * W;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.vec_src) {
      if (gx < W) v = *reinterpret_cast<const float4*>(row + gx);  // W % 4 == 0: the quad is whole
    } else {
      if (gx < W) v.x = row[gx];
      if (gx + 1 < W) v.y = row[gx + 1];
      if (gx + 2 < W) v.z = row[gx + 2];
      if (gx + 3 < W) v.w = row[gx + 3];
    }
    rz_lds4[q] = v;
  }
  __syncthreads();
  const int o = o0 + (tid >> 4), c4 = tid & 15, gx = x0 + c4 * 4;
  if (o >= p.n_dst || gx >= W) return;
  const int n = p.cnt[o];
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < n; ++k) {
    const size_t e = (size_t)k * p.rows + o;
    const float wk = p.w[e];
    const float4 v = rz_lds4[(p.idx[e] - sp.x) * (RZ_COLS / 4) + c4];
    a.x = fmaf(wk, v.x, a.x); a.y = fmaf(wk, v.y, a.y); a.z = fmaf(wk, v.z, a.z); a.w = fmaf(wk, v.w, a.w);
  }
  float* d = p.dst + (size_t)plane * p.dst_plane + (size_t)o * W + gx;
  if (p.vec_dst) {
    *reinterpret_cast<float4*>(d) = a;
  } else {
    d[0] = a.x;
    if (gx + 1 < W) d[1] = a.y;
    if (gx + 2 < W) d[2] = a.z;
    if (gx + 3 < W) d[3] = a.w;
  }
}

__global__ __launch_bounds__(256) void resize_w_kernel(Pass p) {
  extern __shared__ float4 rz_lds4[];                             // [RZ_ROWS][stride] floats
  float* lds = reinterpret_cast<float*>(rz_lds4);
  const long long plane = (long long)blockIdx.z * RZ_GRID_Y + blockIdx.y;
  if (plane >= p.planes) return;
  const int tid = threadIdx.x, R = p.other;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int o0 = tx * RZ_COLS, y0 = ty * RZ_ROWS;
  const int2 sp = p.tile[tx];
  const float* s = p.src + (size_t)plane * p.src_plane;
  const int base = p.vec_src ? (sp.x & ~3) : sp.x;                 // source index of LDS element 0
  if (p.vec_src) {
    const int n4 = ((sp.y - base) >> 2) + 1;                       // n_src % 4 == 0: every quad lies in the row
    for (int q = tid; q < RZ_ROWS * n4; q += 256) {
      const int r = q / n4, j = (q - r * n4) * 4, gy = y0 + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy < R) v = *reinterpret_cast<const float4*>(s + (size_t)gy * p.n_src + base + j);
      float* l = lds + r * p.stride;
      l[lds_pos(j)] = v.x; l[lds_pos(j + 1)] = v.y; l[lds_pos(j + 2)] = v.z; l[lds_pos(j + 3)] = v.w;
    }
  } else {
    const int n1 = sp.y - base + 1;
    for (int q = tid; q < RZ_ROWS * n1; q += 256) {
      const int r = q / n1, j = q - r * n1, gy = y0 + r;
      lds[r * p.stride + lds_pos(j)] = gy < R ? s[(size_t)gy * p.n_src + base + j] : 0.f;
    }
  }
  __syncthreads();
  const int o = o0 + (tid & 63), r0 = (tid >> 6) * 4;
  if (o >= p.n_dst) return;
  const int n = p.cnt[o];
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const float* l = lds + r0 * p.stride;
  for (int k = 0; k < n; ++k) {
    const size_t e = (size_t)k * p.rows + o;
    const float wk = p.w[e];
    const int j = lds_pos(p.idx[e] - base);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = fmaf(wk, l[i * p.stride + j], a[i]);
  }
  float* d = p.dst + (size_t)plane * p.dst_plane + o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (y0 + r0 + i < R) d[(size_t)(y0 + r0 + i) * p.n_dst] = a[i];
}

// ---- launch --------------------------------------------------------------------------------------------------------------
struct Dims {
  long long planes = 0;
  int Ho = 0, Wo = 0;
  size_t work_bytes = 0;               // the [B C][Ho][W] intermediate of either direction
};

// HCF_ERR_ARG: a value outside its domain; HCF_ERR_SHAPE: a legal shape this build cannot index or launch
static int dims_of(int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up, Dims& d) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || s < 2 || s > 8 || (up != 0 && up != 1)) return HCF_ERR_ARG;
  const long long Ho = up ? (long long)H * s : ((long long)H + s - 1) / s;
  const long long Wo = up ? (long long)W * s : ((long long)W + s - 1) / s;
  if (Ho > INT_MAX || Wo > INT_MAX) return HCF_ERR_SHAPE;
  const __int128 planes = (__int128)B * C, lim = (__int128)INT64_MAX / 4;   // byte counts stay in int64 as well
  if (planes * H * W > lim || planes * Ho * Wo > lim || planes * Ho * W > lim) return HCF_ERR_SHAPE;
  if (planes > (__int128)RZ_GRID_Y * RZ_GRID_Y) return HCF_ERR_SHAPE;
  const long long big = Ho > H ? Ho : H, wide = Wo > W ? Wo : W;  // tiles of one plane in blockIdx.x
  if (((big + RZ_ROWS - 1) / RZ_ROWS) * ((wide + RZ_COLS - 1) / RZ_COLS) > INT_MAX) return HCF_ERR_SHAPE;
  d.planes = (long long)planes; d.Ho = (int)Ho; d.Wo = (int)Wo;
  d.work_bytes = (size_t)(planes * Ho * W) * sizeof(float);
  return HCF_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static dim3 grid_of(long long tiles, long long planes) {
  const long long gy = planes < RZ_GRID_Y ? planes : RZ_GRID_Y;
  return dim3((unsigned)tiles, (unsigned)gy, (unsigned)((planes + RZ_GRID_Y - 1) / RZ_GRID_Y));
}

// dst [planes][t.rows][W] = table applied along the rows of src [planes][t.n_src][W]
static int pass_h(const float* src, float* dst, long long planes, int W, const DevTable& t, hipStream_t st) {
  const size_t lds = (size_t)t.span_h * RZ_COLS * sizeof(float);
  if (lds > RZ_LDS_MAX) return HCF_ERR_UNSUPPORTED;
  Pass p;
  p.src = src; p.dst = dst; p.planes = planes;
  p.src_plane = (size_t)t.n_src * W; p.dst_plane = (size_t)t.rows * W;
  p.n_src = t.n_src; p.n_dst = t.rows; p.other = W; p.rows = t.rows;
  p.cnt = t.cnt; p.idx = t.idx; p.w = t.w; p.tile = t.tile_h;
  p.tiles_x = (W + RZ_COLS - 1) / RZ_COLS;
  p.vec_src = aligned16(src) && (W & 3) == 0;
  p.vec_dst = aligned16(dst) && (W & 3) == 0;
  p.stride = 0;
  const long long tiles = (long long)p.tiles_x * ((t.rows + RZ_ROWS - 1) / RZ_ROWS);
  hipLaunchKernelGGL(resize_h_kernel, grid_of(tiles, planes), dim3(256), lds, st, p);
  return HCF_OK;
}

// dst [planes][R][t.rows] = table applied along the columns of src [planes][R][t.n_src]
static int pass_w(const float* src, float* dst, long long planes, int R, const DevTable& t, hipStream_t st) {
  Pass p;
  // a 16-byte staging starts up to 3 elements before the span and ends up to 3 behind it: span + 6 elements, at lds_pos()
  p.stride = t.span_w + 5 + ((t.span_w + 5) >> 5) + 1;
  const size_t lds = (size_t)RZ_ROWS * p.stride * sizeof(float);
  if (lds > RZ_LDS_MAX) return HCF_ERR_UNSUPPORTED;
  p.src = src; p.dst = dst; p.planes = planes;
  p.src_plane = (size_t)R * t.n_src; p.dst_plane = (size_t)R * t.rows;
  p.n_src = t.n_src; p.n_dst = t.rows; p.other = R; p.rows = t.rows;
  p.cnt = t.cnt; p.idx = t.idx; p.w = t.w; p.tile = t.tile_w;
  p.tiles_x = (t.rows + RZ_COLS - 1) / RZ_COLS;
  p.vec_src = aligned16(src) && (t.n_src & 3) == 0;
  p.vec_dst = 0;
  const long long tiles = (long long)p.tiles_x * ((R + RZ_ROWS - 1) / RZ_ROWS);
  hipLaunchKernelGGL(resize_w_kernel, grid_of(tiles, planes), dim3(256), lds, st, p);
  return HCF_OK;
}

}  // namespace rsz
}  // namespace hcf

using namespace hcf;
using namespace hcf::rsz;

extern "C" {

size_t hcf_resize_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up) {
  Dims d;
  return dims_of(B, C, H, W, s, up, d) == HCF_OK ? d.work_bytes : 0;
}

int hcf_resize_bicubic(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up, float* y, void* work,
                       size_t work_bytes, hcf_stream_t stream) {
  if (!x || !y || !work) return HCF_ERR_ARG;
  Dims d;
  int rc = dims_of(B, C, H, W, s, up, d);
  if (rc != HCF_OK) return rc;
  if (work_bytes < d.work_bytes) return HCF_ERR_SHAPE;
  DevTable th, tw;
  if ((rc = table_for(H, s, up, 0, th)) != HCF_OK || (rc = table_for(W, s, up, 0, tw)) != HCF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = pass_h(x, (float*)work, d.planes, W, th, st)) != HCF_OK) return rc;
  if ((rc = pass_w((const float*)work, y, d.planes, d.Ho, tw, st)) != HCF_OK) return rc;
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_resize_bicubic_backward(const float* gy, int32_t B, int32_t C, int32_t H, int32_t W, int32_t s, int32_t up, float* gx,
                                void* work, size_t work_bytes, hcf_stream_t stream) {
  if (!gy || !gx || !work) return HCF_ERR_ARG;
  Dims d;
  int rc = dims_of(B, C, H, W, s, up, d);
  if (rc != HCF_OK) return rc;
  if (work_bytes < d.work_bytes) return HCF_ERR_SHAPE;
  DevTable th, tw;
  if ((rc = table_for(H, s, up, 1, th)) != HCF_OK || (rc = table_for(W, s, up, 1, tw)) != HCF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = pass_w(gy, (float*)work, d.planes, d.Ho, tw, st)) != HCF_OK) return rc;
  if ((rc = pass_h((const float*)work, gx, d.planes, W, th, st)) != HCF_OK) return rc;
  return hipGetLastError() == hipSuccess ? HCF_OK : HCF_ERR_HIP;
}

int hcf_resize_tables(int32_t in_len, int32_t s, int32_t up, int32_t transposed, double* w, int32_t* idx, int32_t* cnt,
                      int64_t capacity) {
  if (in_len < 1 || s < 2 || s > 8 || (up != 0 && up != 1) || (transposed != 0 && transposed != 1)) return HCF_ERR_ARG;
  if ((long long)in_len * s > INT_MAX / 64) return HCF_ERR_SHAPE;  // rows * L stays far inside int
  if ((w || idx || cnt) && !(w && idx && cnt)) return HCF_ERR_ARG;
  HostTable t;
  build_table(in_len, s, up, transposed, t);
  if (!w) return t.L;
  if (capacity < (int64_t)t.rows * t.L) return HCF_ERR_SHAPE;
  for (size_t e = 0; e < (size_t)t.rows * t.L; ++e) { w[e] = t.w[e]; idx[e] = t.idx[e]; }
  for (int r = 0; r < t.rows; ++r) cnt[r] = t.cnt[r];
  return t.L;
}

}  // extern "C"
