// Per-op C-ABI entry points used by the unit parity tests (tests/test_gpu_ops.py). They wrap the
// same kernels the engine launches, on caller-provided NCHW device tensors; temporaries are
// hipMalloc'ed per call (test path, not the hot path). The conv entries build host packs and launch
// through route_conv (hcf_conv_route.hip), the engine's own router, so they take the kernel it takes.
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/hcflow.h"
#include "hcf_common.h"

namespace hcf {
void pack_conv_weights(const float* w, int cin, int cout, int taps, const int* srcs, int nsrc, std::vector<float>& pk,
                       int& nchunk, int& npad);
bool pack_conv_weights_f16x3(const float* w, int cin, int cout, int taps, const int* srcs, int nsrc,
                             std::vector<float>& pk_as_float, int& nchunk, int& npad);
static int g_op_precision = PREC_EXACT;
static double g_last_clock_mhz = 0;
extern int g_f16x3_ablation;   // hcf_conv_f16x3.hip

static inline int ru4(int c) { return (c + 3) & ~3; }

struct Tmp {
  std::vector<void*> ptrs;
  bool ok = true;
  float* dev(size_t nfloat) {
    void* p = nullptr;
    if (hipMalloc(&p, nfloat * sizeof(float) + 256) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(p);
    return (float*)p;
  }
  float* up(const std::vector<float>& v) {
    float* d = dev(v.size());
    if (d && hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  ~Tmp() {
    for (void* p : ptrs) hipFree(p);
  }
};

static View nhwc_from_nchw(Tmp& t, const float* x, int B, int C, int H, int W, hipStream_t st, int& rc) {
  float* p = t.dev((size_t)B * H * W * ru4(C));
  View v = mkview(p, ru4(C), 0, C);
  if (!p) { rc = HCF_ERR_NOMEM; return v; }
  if (hipMemsetAsync(p, 0, (size_t)B * H * W * ru4(C) * sizeof(float), st) != hipSuccess) rc = HCF_ERR_HIP;
  const int r = launch_nchw_to_nhwc(x, v, B, C, H, W, st);
  if (r != HCF_OK) rc = r;
  return v;
}

// ---- the shared pieces of the conv entries: arguments, host packs, the plan in info[], the range flag --------------------------
static inline int ru32(int c) { return (c + 31) / 32 * 32; }
static float* table(Tmp& t, const float* v, int n, int npad, float fill) {
  std::vector<float> h(npad, fill);
  for (int c = 0; c < n && v; ++c) h[c] = v[c];
  return t.up(h);
}

// the process-wide op precision takes the f16 forms for convs of <= 64 output channels
static bool op_f16(int cout) { return g_op_precision == PREC_F16X3 && cout <= 64; }

// NCHW source tensors of a conv on [B, H, W] staged as NHWC views (source i at H >> up, W >> up)
static void stage_sources(Tmp& t, const float* const* src, const int32_t* src_c, const int32_t* src_up, int n_src, int B, int H, int W,
                          View* dst, int* srcs, int& cin, hipStream_t st, int& rc) {
  cin = 0;
  for (int i = 0; i < n_src; ++i) {
    const int up = src_up ? src_up[i] : 0;
    dst[i] = nhwc_from_nchw(t, src[i], B, src_c[i], H >> up, W >> up, st, rc);
    dst[i].up = up;
    srcs[i] = src_c[i];
    cin += src_c[i];
  }
}

// The arguments of one conv on [B, H, W]: the sources (unused slots repeat source 0), bias / scale tables of cout entries padded to
// 32s (null: zeros / ones), the out view, no residuals, and -- f16: the call may take an f16 form -- the range flag with its zero
// page (a.ovf, a.zeros and pk.flag). pk starts empty: conv_packs fills it.
static int conv_call(Tmp& t, ConvArgs& a, ConvPacks& pk, const View* src, int n_src, int B, int H, int W, const float* bias,
                     const float* scale, int cout, int act, View out, bool f16, hipStream_t st) {
  memset(&a, 0, sizeof(a));
  memset(&pk, 0, sizeof(pk));
  for (int i = 0; i < kMaxSrc; ++i) a.src[i] = src[i < n_src ? i : 0];
  a.nsrc = n_src;
  a.B = B; a.H = H; a.W = W;
  a.bias = table(t, bias, cout, ru32(cout), 0.f);
  a.scale = table(t, scale, cout, ru32(cout), 1.f);
  a.act = act;
  a.out = out;
  a.res1 = mkview(nullptr, 0, 0, 0);
  a.res2 = mkview(nullptr, 0, 0, 0);
  if (f16) {
    a.ovf = pk.flag = (int*)t.dev(64);
    if (a.ovf && hipMemsetAsync(a.ovf, 0, 256, st) != hipSuccess) return HCF_ERR_HIP;
    a.zeros = reinterpret_cast<const float*>(a.ovf) + 16;
  }
  return t.ok ? HCF_OK : HCF_ERR_NOMEM;
}

// Host packs of w [cout][cin][k][k] in device memory, for the forms of `allow` (hcf_launch.h) -- f16: the f16x3 pack
// (HCF_ERR_UNSUPPORTED: a weight beyond its range), the Winograd pack where the layer has one (wino_min: from that many input
// channels on, -1 = the engine's rule) and the exact pack a 1x1 falls back to; else the exact pack alone. a.wpack = the first of them.
static int conv_packs(Tmp& t, ConvArgs& a, ConvPacks& pk, const float* w, int cin, int cout, int taps, const int* srcs, int n_src,
                      bool f16, unsigned allow, int wino_min = -1) {
  std::vector<float> h16, hw, h;
  int npad = 0;
  if (f16) {
    if (!pack_conv_weights_f16x3(w, cin, cout, taps, srcs, n_src, h16, a.nchunk, npad)) return HCF_ERR_UNSUPPORTED;
    a.wpack = pk.f16 = t.up(h16);
    if (taps == 9 && (allow & 1u << CONV_WINO) && pack_conv_weights_wino(w, cin, cout, srcs, n_src, hw, wino_min)) pk.wino = t.up(hw);
  }
  if ((allow & 1u << CONV_EXACT) && (!f16 || taps == 1)) {
    pack_conv_weights(w, cin, cout, taps, srcs, n_src, h, a.nchunk, npad);
    pk.exact = t.up(h);
    if (!f16) a.wpack = pk.exact;
  }
  return t.ok ? HCF_OK : HCF_ERR_NOMEM;
}

// the plan launch_conv_f16x3 dispatched from -> info[0] = 1, info[1 .. nf] (include/hcflow.h: 12 fields for hcf_op_fcn12 and
// hcf_op_conv2d_step_inverse, 14 for the view entries)
static F16x3Plan info_f16x3(const ConvArgs& a, int taps, int nf, int32_t* info) {
  const F16x3Plan p = plan_conv_f16x3(a, taps);
  const int32_t v[14] = {p.status, p.v.ntb, p.v.vec, p.v.up, p.v.fuse2, p.v.tailc, p.v.th, p.v.scaled, p.v.k1, p.v.n16,
                         (int32_t)p.grid, (int32_t)p.block, p.vec_epi, p.strip_w};
  info[0] = 1;
  for (int i = 0; i < nf; ++i) info[1 + i] = v[i];
  return p;
}

// stream done, then the range flag (null: an exact call): HCF_ERR_UNSUPPORTED when an input left the f16 range, the caller must use
// the exact kernel (info, where given: info[15] = the flag word)
static int conv_finish(const int* flag, int32_t* info, hipStream_t st) {
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  int h = 0;
  if (flag && hipMemcpy(&h, flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return HCF_ERR_HIP;
  if (flag && info) info[15] = h;
  return h ? HCF_ERR_UNSUPPORTED : HCF_OK;
}

// host packs + launch of a conv2d / hcf_bench_conv call: the f16 forms for 3x3 convs only
static int pack_and_launch(Tmp& t, ConvArgs& a, ConvPacks& pk, const float* w, int cin, int cout, int k, const int* srcs, int n_src,
                           hipStream_t st) {
  const int rc = conv_packs(t, a, pk, w, cin, cout, k * k, srcs, n_src, op_f16(cout) && k == 3, kAllowAll);
  return rc != HCF_OK ? rc : route_conv(a, pk, k * k, kAllowAll, st).status;
}

// *slot (zero-initialised by the caller) = max |x| over the source windows, as the running maximum of the engine's backward is
static int sources_absmax(const View* src, int n_src, int B, int H, int W, float* slot, hipStream_t st) {
  int rc = HCF_OK;
  for (int i = 0; i < n_src && rc == HCF_OK; ++i) rc = launch_absmax(src[i], B, H >> src[i].up, W >> src[i].up, slot, st);
  return rc;
}

// a.in_max (the scaled f16x3 forms) = a fresh slot with max |x| over the sources
static int conv_in_max(Tmp& t, ConvArgs& a, hipStream_t st) {
  float* m = t.dev(1);
  if (!m) return HCF_ERR_NOMEM;
  if (hipMemsetAsync(m, 0, sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;
  a.in_max = m;
  return sources_absmax(a.src, a.nsrc, a.B, a.H, a.W, m, st);
}

// The f16 weight gradient's ranges: g is scaled by a power of two from max |g| (wa.g_max), X is split without a scale -- an |x| beyond
// the f16 range (nothing range-checked this caller's tensor) would turn the hi part into inf, so wa.g_max stays null and the fp32
// kernel takes such inputs. Synchronises.
static int wgrad_f16_range(Tmp& t, WgradArgs& wa, hipStream_t st) {
  float* gm = t.dev(2);
  if (!gm) return HCF_ERR_NOMEM;
  if (hipMemsetAsync(gm, 0, 2 * sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;
  int rc = launch_absmax(wa.g, wa.B, wa.H, wa.W, gm, st);
  if (rc == HCF_OK) rc = sources_absmax(wa.src, wa.nsrc, wa.B, wa.H, wa.W, gm + 1, st);
  float xmax = 0.f;
  if (hipMemcpyAsync(&xmax, gm + 1, sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HCF_ERR_HIP;
  if (rc == HCF_OK && xmax < 65504.f) wa.g_max = gm;           // NaN / inf compare false -> fp32 kernel
  return rc;
}

static bool invert64(const float* Wm, int n, std::vector<float>& out_padded, int M) {
  std::vector<double> a((size_t)n * n), inv((size_t)n * n, 0.0);
  for (int i = 0; i < n * n; ++i) a[i] = Wm[i];
  for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
  for (int col = 0; col < n; ++col) {
    int piv = col;
    double best = fabs(a[(size_t)col * n + col]);
    for (int r = col + 1; r < n; ++r)
      if (fabs(a[(size_t)r * n + col]) > best) { best = fabs(a[(size_t)r * n + col]); piv = r; }
    if (best == 0.0) return false;
    if (piv != col)
      for (int c = 0; c < n; ++c) {
        std::swap(a[(size_t)piv * n + c], a[(size_t)col * n + c]);
        std::swap(inv[(size_t)piv * n + c], inv[(size_t)col * n + c]);
      }
    const double d = a[(size_t)col * n + col];
    for (int c = 0; c < n; ++c) { a[(size_t)col * n + c] /= d; inv[(size_t)col * n + c] /= d; }
    for (int r = 0; r < n; ++r) {
      if (r == col) continue;
      const double f = a[(size_t)r * n + col];
      if (f == 0.0) continue;
      for (int c = 0; c < n; ++c) {
        a[(size_t)r * n + c] -= f * a[(size_t)col * n + c];
        inv[(size_t)r * n + c] -= f * inv[(size_t)col * n + c];
      }
    }
  }
  out_padded.assign((size_t)M * M, 0.f);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) out_padded[(size_t)r * M + c] = (float)inv[(size_t)r * n + c];
  return true;
}

}  // namespace hcf

using namespace hcf;

extern "C" {

int hcf_op_conv2d(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src, int32_t B,
                  int32_t H, int32_t W, const float* w, const float* bias, const float* scale, int32_t cout, int32_t k,
                  int32_t act, const float* res1, float rs1, const float* res2, float rs2, float* out,
                  hcf_stream_t stream) {
  if (!src || !src_c || !w || !out || n_src < 1 || n_src > kMaxSrc || (k != 1 && k != 3) || cout < 1 || cout > 96)
    return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  ConvArgs a;
  ConvPacks pk;
  View sv[kMaxSrc];
  int cin = 0, srcs[kMaxSrc];
  stage_sources(t, src, src_c, src_up, n_src, B, H, W, sv, srcs, cin, st, rc);
  const View ov = mkview(t.dev((size_t)B * H * W * ru4(cout)), ru4(cout), 0, cout);
  const int rb = conv_call(t, a, pk, sv, n_src, B, H, W, bias, scale, cout, act, ov, op_f16(cout) && k == 3, st);
  if (res1) { a.res1 = nhwc_from_nchw(t, res1, B, cout, H, W, st, rc); a.rs1 = rs1; }
  if (res2) { a.res2 = nhwc_from_nchw(t, res2, B, cout, H, W, st, rc); a.rs2 = rs2; }
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = rb;
  if (rc != HCF_OK) return rc;
  rc = pack_and_launch(t, a, pk, w, cin, cout, k, srcs, n_src, st);
  if (rc != HCF_OK) return rc;
  rc = launch_nhwc_to_nchw(a.out, out, B, cout, H, W, 0, st);
  const int fin = conv_finish(pk.flag, nullptr, st);
  return fin != HCF_OK ? fin : rc;
}

// Transposed weights for the data gradient of source window [off, off + n) of a conv with weight w [cout][cin][k][k]:
// wt[ic][oc][t] = w[oc][off + ic][taps - 1 - t]  (a 3x3 "same" conv of the output gradient with the flipped kernel)
static void transpose_weights(const float* w, int cin, int cout, int taps, int off, int n, std::vector<float>& wt) {
  wt.assign((size_t)n * cout * taps, 0.f);
  for (int ic = 0; ic < n; ++ic)
    for (int oc = 0; oc < cout; ++oc)
      for (int t = 0; t < taps; ++t)
        wt[((size_t)ic * cout + oc) * taps + t] = w[((size_t)oc * cin + off + ic) * taps + (taps - 1 - t)];
}

// Gradients of y = conv2d(cat(up(src_i)), w) + bias w.r.t. the sources, the weight and the bias, given
// g = dL/dy (torch.autograd of F.conv2d; the training path of SURVEY.md 8f rank 1). dsrc[i] may be NULL.
int hcf_op_conv2d_backward(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src,
                           int32_t B, int32_t H, int32_t W, const float* w, int32_t cout, int32_t k, const float* g,
                           float* const* dsrc, float* dw, float* dbias, hcf_stream_t stream) {
  if (!src || !src_c || !w || !g || n_src < 1 || n_src > kMaxSrc || (k != 1 && k != 3) || cout < 1 || cout > 96)
    return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  const int taps = k * k;
  int cin = 0;
  for (int i = 0; i < n_src; ++i) cin += src_c[i];
  View gv = nhwc_from_nchw(t, g, B, cout, H, W, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  // ---- data gradients: one conv of g per <= 64-channel block of each source window
  int off = 0;
  for (int i = 0; i < n_src && rc == HCF_OK; ++i) {
    const int up = src_up ? src_up[i] : 0, n = src_c[i];
    if (dsrc && dsrc[i]) {
      float* full = t.dev((size_t)B * H * W * ru4(n));
      if (!t.ok) return HCF_ERR_NOMEM;
      for (int c0 = 0; c0 < n && rc == HCF_OK; c0 += 64) {
        const int nb = std::min(64, n - c0);
        std::vector<float> wt;
        transpose_weights(w, cin, cout, taps, off + c0, nb, wt);
        ConvArgs a;
        ConvPacks pk;
        int one = cout;
        rc = conv_call(t, a, pk, &gv, 1, B, H, W, nullptr, nullptr, nb, ACT_NONE, mkview(full, ru4(n), c0, nb), op_f16(nb) && k == 3, st);
        if (rc == HCF_OK) rc = pack_and_launch(t, a, pk, wt.data(), cout, nb, k, &one, 1, st);
      }
      if (rc != HCF_OK) break;
      View fv = mkview(full, ru4(n), 0, n);
      if (up > 0) {
        float* low = t.dev((size_t)B * (H >> up) * (W >> up) * ru4(n));
        if (!t.ok) return HCF_ERR_NOMEM;
        View lv = mkview(low, ru4(n), 0, n);
        rc = launch_sumpool(fv, lv, B, H >> up, W >> up, up, 0, st);
        if (rc == HCF_OK) rc = launch_nhwc_to_nchw(lv, dsrc[i], B, n, H >> up, W >> up, 0, st);
      } else {
        rc = launch_nhwc_to_nchw(fv, dsrc[i], B, n, H, W, 0, st);
      }
    }
    off += n;
  }
  // ---- weight gradient
  if (rc == HCF_OK && dw) {
    WgradArgs wa;
    memset(&wa, 0, sizeof(wa));
    int srcs[kMaxSrc];
    stage_sources(t, src, src_c, src_up, n_src, B, H, W, wa.src, srcs, cin, st, rc);
    wa.nsrc = n_src;
    wa.g = gv;
    wa.B = B; wa.H = H; wa.W = W; wa.taps = taps;
    const size_t nw = (size_t)cout * cin * taps;
    wa.dw = t.dev(nw);
    if (!t.ok) return HCF_ERR_NOMEM;
    if (hipMemsetAsync(wa.dw, 0, nw * sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;
    wa.part_cap = conv_wgrad_scratch_floats(wa);
    wa.part = t.dev(wa.part_cap);
    if (!t.ok) return HCF_ERR_NOMEM;
    if (rc == HCF_OK && g_op_precision == PREC_F16X3) rc = wgrad_f16_range(t, wa, st);      // f16 matrix cores
    if (rc == HCF_OK) rc = launch_conv_wgrad(wa, st);
    if (rc == HCF_OK && hipMemcpyAsync(dw, wa.dw, nw * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) rc = HCF_ERR_HIP;
  }
  // ---- bias gradient: per-channel sums of g
  std::vector<double> hs;
  if (rc == HCF_OK && dbias) {
    double* sd = (double*)t.dev(4 * (size_t)cout);
    if (!t.ok) return HCF_ERR_NOMEM;
    hs.resize(2 * (size_t)cout);
    rc = launch_channel_stats(gv, B, H, W, sd, st);
    if (rc == HCF_OK && hipMemcpyAsync(hs.data(), sd, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = HCF_ERR_HIP;
  }
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  if (rc == HCF_OK && dbias)
    for (int c = 0; c < cout; ++c) dbias[c] = (float)hs[c];
  return rc;
}

// shader clock (MHz) observed inside the last hcf_bench_conv kernels (s_memtime / s_memrealtime)
double hcf_debug_last_clock_mhz(void) {
  const double probe = hcf::wino_clock_probe_mhz();       // (hcf_debug_clock_probe: the 64-channel Winograd kernel's own clock since the enable)
  return probe > 0.0 ? probe : g_last_clock_mhz;
}
int hcf_debug_clock_probe(int32_t enable) { return hcf::wino_clock_probe(enable); }
// the kAbl* bits of hcf_switches.h (tools/conv_bench.py --ablate, the tests' kernel-variant comparisons); 0 = off
int hcf_debug_set_ablation(int32_t bits) { hcf::g_f16x3_ablation = bits; return HCF_OK; }

// launch selection without a GPU (layouts: include/hcflow.h). The views get made-up addresses: the plans test them, nothing reads them
static float* plan_case_ptr(int base, int aligned) { return reinterpret_cast<float*>((uintptr_t)(base * 0x1000 + (aligned ? 0 : 4))); }
static void plan_case_args(const int32_t* in, ConvArgs& c, WgradArgs& w) {
  memset(&c, 0, sizeof(c));
  memset(&w, 0, sizeof(w));
  c.B = w.B = in[2]; c.H = w.H = in[3]; c.W = w.W = in[4];
  c.nsrc = w.nsrc = in[5];
  for (int i = 0; i < kMaxSrc; ++i) {
    const int32_t* s = in + 6 + 5 * i;
    if (s[1]) c.src[i] = w.src[i] = mkview(plan_case_ptr(1 + i, s[4]), s[1], s[2], s[0], s[3]);
  }
  c.out = w.g = mkview(plan_case_ptr(4, in[24]), in[22], in[23], in[21]);
  if (in[39] & 1) c.out.p = nullptr;
  if (in[25]) c.res1 = mkview(plan_case_ptr(5, in[25] == 1), in[26], in[27], in[21]);
  if (in[28]) c.res2 = mkview(plan_case_ptr(6, in[28] == 1), in[29], in[30], in[21]);
  c.tC = in[31]; w.blocks_hint = in[31];
  if (in[32] & 1) c.w2 = plan_case_ptr(7, 1);
  if (in[32] & 2) c.bias2 = plan_case_ptr(8, 1);
  if (in[32] & 4) c.scale2 = plan_case_ptr(9, 1);
  if (in[33]) c.in_max = w.g_max = plan_case_ptr(10, 1);
  c.act = in[34];
  if (in[35]) c.fb_y = mkview(plan_case_ptr(11, in[35] == 1), in[36], in[37], in[21]);
  if (in[38] & 1) c.fb_part = plan_case_ptr(12, 1);
  if (in[38] & 2) c.fb_scale = plan_case_ptr(13, !(in[38] & 4));
  c.fb_max2 = (in[38] & 8) ? const_cast<float*>(c.in_max) : plan_case_ptr(14, 1);
  if (!(in[39] & 2)) c.ovf = reinterpret_cast<int*>(plan_case_ptr(15, 1));
  w.taps = in[1];
  w.dw = plan_case_ptr(16, 1); w.part = plan_case_ptr(17, 1); w.part_cap = (size_t)1 << 40;
}
int hcf_debug_conv_plan(const int32_t* in, int32_t n_in, int64_t* out, int32_t n_out) {
  if (!in || !out || n_in != HCF_PLAN_N_IN || n_out != HCF_PLAN_N_OUT || (in[0] != 0 && in[0] != 1)) return HCF_ERR_ARG;
  ConvArgs c;
  WgradArgs w;
  plan_case_args(in, c, w);
  int th = 8;
  const F16x3Plan p = in[0] == 0 ? plan_conv_f16x3(c, in[1]) : F16x3Plan{};
  const WgradPlan q = in[0] == 1 ? plan_conv_wgrad(w) : WgradPlan{};
  const int64_t conv[HCF_PLAN_N_OUT] = {p.status, p.v.ntb, p.v.vec, p.v.up, p.v.fuse2, p.v.tailc, p.v.th, p.v.scaled, p.v.k1, p.v.n16, p.grid, p.block, p.any_up,
                                        p.vec_epi, p.strip_w, p.strip_magic,      // then the partial-sum rows the engine plans for (conv_tile_blocks)
                                        conv_f16x3_scaled_blocks(c.B, c.H, c.W, nullptr, &th), conv_f16x3_scaled_blocks_max(c.B, c.H, c.W)};
  const int64_t wgrad[HCF_PLAN_N_OUT] = {q.status, q.f16, q.taps, q.vec, q.db, q.nblk_x, q.nicb, q.nocb, q.block, q.lds_bytes, q.tpb, q.cin_total, q.strip_w,
                                         q.strip_magic, (int64_t)q.scratch_floats, q.nbx};
  for (int i = 0; i < n_out; ++i) out[i] = in[0] == 0 ? conv[i] : wgrad[i];
  return HCF_OK;
}

// the forms route_conv would try, in order, without a launch (layout: include/hcflow.h)
int hcf_debug_conv_route(int32_t taps, int32_t packs, int32_t tail, int32_t allow, int32_t* forms, int32_t n_forms) {
  if (!forms || n_forms != 4 || (taps != 1 && taps != 9) || packs < 0 || packs > 31 || allow < 0 || allow > 15) return HCF_ERR_ARG;
  ConvArgs c;
  memset(&c, 0, sizeof(c));
  c.tC = tail ? 12 : 0;
  const ConvPacks p = {(packs & 1) ? plan_case_ptr(1, 1) : nullptr, (packs & 2) ? plan_case_ptr(2, 1) : nullptr,
                       (packs & 4) ? plan_case_ptr(3, 1) : nullptr, (packs & 8) ? plan_case_ptr(4, 1) : nullptr,
                       (packs & 16) ? plan_case_ptr(5, 1) : nullptr, nullptr};
  int f[4] = {CONV_NONE, CONV_NONE, CONV_NONE, CONV_NONE};
  const int n = conv_route_forms(c, p, taps, (unsigned)allow, f);
  for (int i = 0; i < 4; ++i) forms[i] = f[i];
  return n;
}

int hcf_op_set_precision(int32_t mode) {
  if (mode != PREC_EXACT && mode != PREC_F16X3) return HCF_ERR_ARG;
  g_op_precision = mode;
  return HCF_OK;
}

int hcf_op_squeeze2d(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t haar,
                     hcf_stream_t stream) {
  if (!x || !out || (H & 1) || (W & 1)) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  View in = nhwc_from_nchw(t, x, B, C, H, W, st, rc);
  float* o = t.dev((size_t)B * (H / 2) * (W / 2) * ru4(4 * C));
  if (!t.ok) return HCF_ERR_NOMEM;
  View ov = mkview(o, ru4(4 * C), 0, 4 * C);
  if (rc == HCF_OK) rc = haar ? launch_haar_fwd(in, ov, B, C, H, W, st) : launch_squeeze(in, ov, B, C, H, W, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(ov, out, B, 4 * C, H / 2, W / 2, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_unsqueeze2d(const float* x, float* out, int32_t B, int32_t C4, int32_t H, int32_t W, int32_t haar,
                       hcf_stream_t stream) {
  if (!x || !out || (C4 & 3)) return HCF_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  View in = nhwc_from_nchw(t, x, B, C4, H, W, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  // exercises the fused boundary form (unsqueeze -> NCHW) used for the final HR image
  if (rc == HCF_OK) rc = launch_unsqueeze_nchw(in, out, B, C4, H, W, haar, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_step_inverse(const float* z, const float* h, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                        int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_bias,
                        const float* an_logs, hcf_stream_t stream) {
  if (!z || !h || !out || !an_bias || !an_logs) return HCF_ERR_ARG;
  const int M = step_cmax(C);
  if (M < 0) return HCF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.W = W; a.C = C; a.ns = ns; a.mode = mode;
  a.z = nhwc_from_nchw(t, z, B, C, H, W, st, rc);
  a.h = nhwc_from_nchw(t, h, B, hC, H, W, st, rc);
  a.out = a.z;
  std::vector<float> hb(M, 0.f), hm(M, 0.f);
  for (int c = 0; c < C; ++c) { hb[c] = an_bias[c]; hm[c] = expf(-an_logs[c]); }
  a.an_bias = t.up(hb);
  a.an_mul = t.up(hm);
  if (mat) {
    std::vector<float> wi;
    if (!invert64(mat, C, wi, M)) return HCF_ERR_ARG;
    a.mat = t.up(wi);
  }
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_step_tail_inv(a, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.out, out, B, C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_step_forward_head(const float* z, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mat,
                             const float* an_bias, const float* an_logs, hcf_stream_t stream) {
  if (!z || !out || !an_bias || !an_logs) return HCF_ERR_ARG;
  const int M = step_cmax(C);
  if (M < 0) return HCF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.z = nhwc_from_nchw(t, z, B, C, H, W, st, rc);
  a.out = a.z;
  std::vector<float> hb(M, 0.f), hm(M, 0.f);
  for (int c = 0; c < C; ++c) { hb[c] = an_bias[c]; hm[c] = expf(an_logs[c]); }
  a.an_bias = t.up(hb);
  a.an_mul = t.up(hm);
  if (mat) {
    std::vector<float> wf((size_t)M * M, 0.f);
    for (int r = 0; r < C; ++r)
      for (int c = 0; c < C; ++c) wf[(size_t)r * M + c] = mat[(size_t)r * C + c];
    a.mat = t.up(wf);
  }
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_step_head_fwd(a, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.out, out, B, C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_step_forward_couple(const float* z, const float* h, float* out, float* logdet, int32_t B, int32_t C,
                               int32_t H, int32_t W, int32_t hC, int32_t mode, int32_t ns, hcf_stream_t stream) {
  if (!z || !h || !out) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.W = W; a.C = C; a.ns = ns; a.mode = mode;
  a.z = nhwc_from_nchw(t, z, B, C, H, W, st, rc);
  a.h = nhwc_from_nchw(t, h, B, hC, H, W, st, rc);
  a.out = a.z;
  const int nb = step_blocks_per_sample(H, W);
  float* part = nullptr;
  if (logdet) {
    part = t.dev((size_t)B * nb);
    a.partial = part;
    a.partial_stride = nb;
  }
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_step_couple_fwd(a, st);
  if (rc == HCF_OK && logdet) {
    // engine-style final reduction; nll output unused here
    rc = launch_reduce_partials(part, nb, (mode == CPL_AFFINE) ? nb : 0, B, 0.0, 1.0, logdet, nullptr, st);
  }
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.out, out, B, C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_gauss_logp(const float* h, const float* x, float* out_logp, int32_t B, int32_t C, int32_t H, int32_t W,
                      hcf_stream_t stream) {
  if (!h || !x || !out_logp) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  GaussArgs g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.H = H; g.W = W; g.C = C;
  g.h = nhwc_from_nchw(t, h, B, 2 * C, H, W, st, rc);
  g.out = nhwc_from_nchw(t, x, B, C, H, W, st, rc);
  const int nb = step_blocks_per_sample(H, W);
  g.partial = t.dev((size_t)B * nb);
  g.partial_stride = nb;
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_gauss_logp(g, st);
  if (rc == HCF_OK) rc = launch_reduce_partials(g.partial, nb, nb, B, 0.0, 1.0, out_logp, nullptr, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_gauss_sample(const float* h, const float* eps, float tau, uint64_t seed, float* out, int32_t B, int32_t C,
                        int32_t H, int32_t W, int32_t rescale, hcf_stream_t stream) {
  if (!h || !out) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  GaussArgs g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.H = H; g.W = W; g.C = C;
  g.h = nhwc_from_nchw(t, h, B, 2 * C, H, W, st, rc);
  g.rescale = rescale;
  g.eps = eps; g.tau = tau; g.seed = seed; g.offset = 0; g.tau_b = nullptr;
  float* o = t.dev((size_t)B * H * W * ru4(C));
  g.out = mkview(o, ru4(C), 0, C);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_gauss_sample(g, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(g.out, out, B, C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}


// ---- backward kernels of the training path (hcf_train.hip), one entry per launcher ------------------------------------
}  // extern "C"

namespace hcf {

// an NCHW tensor of n channels (nullptr: zeros) as channels [c0, c0 + n) of a dense, zero-filled NHWC buffer of cs floats per pixel
static View nhwc_window(Tmp& t, const float* x, int B, int n, int H, int W, int cs, int c0, hipStream_t st, int& rc) {
  const size_t nf = (size_t)B * H * W * cs;
  float* p = t.dev(nf);
  View v = mkview(p, cs, c0, n);
  if (!p) { rc = HCF_ERR_NOMEM; return v; }
  if (hipMemsetAsync(p, 0, nf * sizeof(float), st) != hipSuccess) rc = HCF_ERR_HIP;
  if (x) {
    const int r = launch_nchw_to_nhwc(x, v, B, n, H, W, st);
    if (r != HCF_OK) rc = r;
  }
  return v;
}

// per-block partial rows as the engine allocates them (hcf_engine_train.inc), every float a NaN until a block writes its row
static float* part_rows(Tmp& t, size_t nfloat, hipStream_t st, int& rc) {
  float* p = t.dev(nfloat);
  if (!p) { rc = HCF_ERR_NOMEM; return nullptr; }
  if (hipMemsetAsync(p, 0xff, nfloat * sizeof(float), st) != hipSuccess) rc = HCF_ERR_HIP;
  return p;
}

// the engine's fixed-order reduction of those rows: one job, one launch_sum_jobs
static int reduce_rows(Tmp& t, const float* part, int nblk, int n, int pstride, float* d0, float* d1, float mult1, hipStream_t st) {
  SumJob j;
  memset(&j, 0, sizeof(j));
  j.part = part; j.nblk = nblk; j.n = n; j.pstride = pstride; j.dst0 = d0; j.dst1 = d1; j.mult1 = mult1;
  SumJob* jd = reinterpret_cast<SumJob*>(t.dev((sizeof(SumJob) + 3) / 4));
  if (!jd) return HCF_ERR_NOMEM;
  if (hipMemcpyAsync(jd, &j, sizeof(j), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HCF_ERR_HIP;
  return launch_sum_jobs(jd, 1, st);
}

static bool step_shape_ok(int B, int C, int H, int W, int hC, int mode, int ns) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return false;
  if (mode == CPL_AFFINE) return ns >= 0 && ns <= C && hC == 2 * (C - ns) && hC >= 1;
  return mode == CPL_SHIFT3 && C >= 3 && hC == 3;
}

}  // namespace hcf

extern "C" {

int hcf_op_step_forward_backward(const float* gzout, const float* zout, const float* h, const float* za, float* gzin,
                                 float* gh, float* g_bias, float* g_logs, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_logs, float gobj,
                                 hcf_stream_t stream) {
  if (!gzout || !zout || !h || !za || !gzin || !gh || !g_bias || !g_logs || !an_logs) return HCF_ERR_ARG;
  if (!step_shape_ok(B, C, H, W, hC, mode, ns)) return HCF_ERR_ARG;
  const int M = step_cmax(C);
  if (M < 0) return HCF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  StepBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.W = W; a.C = C; a.ns = ns; a.mode = mode;
  a.gzout = nhwc_from_nchw(t, gzout, B, C, H, W, st, rc);
  a.zout = nhwc_from_nchw(t, zout, B, C, H, W, st, rc);
  a.h = nhwc_from_nchw(t, h, B, hC, H, W, st, rc);
  a.za = nhwc_from_nchw(t, za, B, C, H, W, st, rc);
  a.gzb = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  a.gh = nhwc_window(t, nullptr, B, hC, H, W, ru4(hC), 0, st, rc);
  a.gzin = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  a.gobj = gobj;
  std::vector<float> hm(M, 0.f);
  for (int c = 0; c < C; ++c) hm[c] = expf(an_logs[c]);
  a.an_mul = t.up(hm);
  if (mat) {                                            // row c of the table = column c of W
    std::vector<float> wt((size_t)M * M, 0.f);
    for (int r = 0; r < C; ++r)
      for (int c = 0; c < C; ++c) wt[(size_t)c * M + r] = mat[(size_t)r * C + c];
    a.matT = t.up(wt);
  }
  a.g_bias = g_bias; a.g_logs = g_logs;
  const int nblk = B * step_blocks_per_sample(H, W);
  a.part = part_rows(t, (size_t)nblk * 2 * M, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_step_couple_bwd(a, st);
  if (rc == HCF_OK) rc = launch_step_head_bwd(a, st);
  if (rc == HCF_OK) rc = reduce_rows(t, a.part, nblk, C, M, g_bias, g_logs, 1.f, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.gzin, gzin, B, C, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.gh, gh, B, hC, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_step_inverse_backward(const float* gx, const float* x, const float* zc, const float* h, float* gz, float* gh,
                                 float* gzc, float* y, float* g_bias, float* g_logs, int32_t B, int32_t C, int32_t H,
                                 int32_t W, int32_t hC, int32_t mode, int32_t ns, const float* mat, const float* an_bias,
                                 const float* an_logs, hcf_stream_t stream) {
  if (!gx || !x || !zc || !h || !gz || !gh || !gzc || !y || !g_bias || !g_logs || !an_bias || !an_logs) return HCF_ERR_ARG;
  if (!step_shape_ok(B, C, H, W, hC, mode, ns)) return HCF_ERR_ARG;
  const int M = step_cmax(C);
  if (M < 0) return HCF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  StepInvBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.H = H; a.W = W; a.C = C; a.ns = ns; a.mode = mode;
  a.gx = nhwc_from_nchw(t, gx, B, C, H, W, st, rc);
  a.x = nhwc_from_nchw(t, x, B, C, H, W, st, rc);
  a.zc = nhwc_from_nchw(t, zc, B, C, H, W, st, rc);
  a.h = nhwc_from_nchw(t, h, B, hC, H, W, st, rc);
  a.gz = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  a.gh = nhwc_window(t, nullptr, B, hC, H, W, ru4(hC), 0, st, rc);
  a.gzc = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  a.y = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  std::vector<float> hb(M, 0.f), hf(M, 0.f), hi(M, 0.f);
  for (int c = 0; c < C; ++c) { hb[c] = an_bias[c]; hf[c] = expf(an_logs[c]); hi[c] = expf(-an_logs[c]); }
  a.an_bias = t.up(hb);
  a.mul_fwd = t.up(hf);
  a.mul_inv = t.up(hi);
  if (mat) {                                            // row j of the table = column j of W^-1
    std::vector<float> wi;
    if (!invert64(mat, C, wi, M)) return HCF_ERR_ARG;
    std::vector<float> wit((size_t)M * M, 0.f);
    for (int r = 0; r < C; ++r)
      for (int c = 0; c < C; ++c) wit[(size_t)c * M + r] = wi[(size_t)r * M + c];
    a.matInvT = t.up(wit);
  }
  a.g_bias = g_bias; a.g_logs = g_logs;
  const int nblk = B * step_blocks_per_sample(H, W);
  a.part = part_rows(t, (size_t)nblk * 2 * M, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_step_inv_bwd(a, st);
  if (rc == HCF_OK) rc = reduce_rows(t, a.part, nblk, C, M, g_bias, g_logs, 1.f, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.gz, gz, B, C, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.gh, gh, B, hC, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.gzc, gzc, B, C, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(a.y, y, B, C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_prior_backward(int32_t kind, const float* a, const float* h, float* ga, float* gh, const float* gz_nchw,
                          int32_t B, int32_t C, int32_t H, int32_t W, int32_t rescale, float gobj, hcf_stream_t stream) {
  if (!a || !h || !ga || !gh || kind < 0 || kind > 2 || B < 1 || C < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  PriorBwdArgs p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.H = H; p.W = W; p.C = C;
  p.a = nhwc_from_nchw(t, a, B, C, H, W, st, rc);
  p.h = nhwc_from_nchw(t, h, B, 2 * C, H, W, st, rc);
  p.ga = nhwc_window(t, kind == 1 ? ga : nullptr, B, C, H, W, ru4(C), 0, st, rc);       // sample: ga is the input
  p.gh = nhwc_window(t, nullptr, B, 2 * C, H, W, ru4(2 * C), 0, st, rc);
  p.gobj = gobj; p.rescale = rescale; p.gz_nchw = gz_nchw;
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = kind == 0 ? launch_gauss_logp_bwd(p, st) : kind == 1 ? launch_gauss_sample_bwd(p, st) : launch_gauss_encode_bwd(p, st);
  if (rc == HCF_OK && kind != 1) rc = launch_nhwc_to_nchw(p.ga, ga, B, C, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(p.gh, gh, B, 2 * C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_prior_sample_backward(const float* a, const float* h, const float* ga, float* gh, float* geps_nchw, int32_t B,
                                 int32_t C, int32_t H, int32_t W, int32_t rescale, hcf_stream_t stream) {
  if (!a || !h || !ga || !gh || B < 1 || C < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  PriorBwdArgs p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.H = H; p.W = W; p.C = C;
  p.a = nhwc_from_nchw(t, a, B, C, H, W, st, rc);
  p.h = nhwc_from_nchw(t, h, B, 2 * C, H, W, st, rc);
  p.ga = nhwc_window(t, ga, B, C, H, W, ru4(C), 0, st, rc);
  p.gh = nhwc_window(t, nullptr, B, 2 * C, H, W, ru4(2 * C), 0, st, rc);
  p.rescale = rescale; p.geps_nchw = geps_nchw;         // straight into the caller's NCHW tensor, as the engine's pass does
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_gauss_sample_bwd(p, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(p.gh, gh, B, 2 * C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_quant_logp_backward(const float* z, const float* lr, float* gz, int32_t B, int32_t H, int32_t W, float gobj,
                               hcf_stream_t stream) {
  return hcf_op_quant_logp_backward_lr(z, lr, gz, nullptr, B, H, W, gobj, stream);
}

int hcf_op_quant_logp_backward_lr(const float* z, const float* lr, float* gz, float* glr, int32_t B, int32_t H, int32_t W,
                                  float gobj, hcf_stream_t stream) {
  if (!z || !lr || !gz || B < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  View zv = nhwc_from_nchw(t, z, B, 3, H, W, st, rc);
  View gv = nhwc_from_nchw(t, gz, B, 3, H, W, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_quant_logp_bwd(zv, lr, gv, B, H, W, gobj, glr, st);      // glr: straight into the caller's NCHW tensor
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(gv, gz, B, 3, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_prior_encode_logp_backward(const float* a, const float* h, float* ga, float* gh, const float* geps_nchw,
                                      const float* glogp, int32_t B, int32_t C, int32_t H, int32_t W, int32_t rescale, float gobj,
                                      hcf_stream_t stream) {
  if (!a || !h || !ga || !gh || B < 1 || C < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  PriorBwdArgs p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.H = H; p.W = W; p.C = C;
  p.a = nhwc_from_nchw(t, a, B, C, H, W, st, rc);
  p.h = nhwc_from_nchw(t, h, B, 2 * C, H, W, st, rc);
  p.ga = nhwc_window(t, nullptr, B, C, H, W, ru4(C), 0, st, rc);
  p.gh = nhwc_window(t, nullptr, B, 2 * C, H, W, ru4(2 * C), 0, st, rc);
  p.gobj = gobj; p.gobj_b = glogp; p.rescale = rescale; p.gz_nchw = geps_nchw;
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_gauss_encode_logp_bwd(p, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(p.ga, ga, B, C, H, W, 0, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(p.gh, gh, B, 2 * C, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_input_grad(const float* gz, float* ghr, int32_t B, int32_t C, int32_t H, int32_t W, int32_t haar,
                      hcf_stream_t stream) {
  if (!gz || !ghr || B < 1 || C < 1 || H < 1 || W < 1 || haar < 0 || haar > 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  View gv = nhwc_from_nchw(t, gz, B, 4 * C, H, W, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_input_grad_emit(gv, ghr, B, C, H, W, haar, st);           // straight into the caller's NCHW tensor
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_output_grad_backward(int32_t kind, const float* g, const float* z, float* gz, int32_t B, int32_t C, int32_t H,
                                int32_t W, hcf_stream_t stream) {
  if (!z || !gz || (!g && kind != 2) || kind < 0 || kind > 3 || B < 1 || C < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  if (kind == 3) {
    rc = launch_mask_flat(g, z, gz, (size_t)B * C * H * W, st);
  } else {
    View zv = nhwc_from_nchw(t, z, B, C, H, W, st, rc);
    View gv = nhwc_from_nchw(t, gz, B, C, H, W, st, rc);
    if (!t.ok) return HCF_ERR_NOMEM;
    if (rc == HCF_OK) rc = kind == 2 ? launch_mask_unit_range(zv, gv, B, H, W, st) : launch_add_nchw_grad(g, zv, gv, B, H, W, kind, st);
    if (rc == HCF_OK) rc = launch_nhwc_to_nchw(gv, gz, B, C, H, W, 0, st);
  }
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_conv_epilogue_backward(const float* gy, const float* y, const float* scale, int32_t act, int32_t has1, float rs1,
                                  float* g1, int32_t has2, float rs2, float* g2, float* gpre, float* sum_pre, float* sum_zy,
                                  float zy_mult, float* absmax, float* absmax2, const float* carry2, int32_t B, int32_t n,
                                  int32_t H, int32_t W, int32_t cs, int32_t c0, hcf_stream_t stream) {
  if (!gy || !gpre || B < 1 || n < 1 || n > 256 || H < 1 || W < 1 || c0 < 0 || cs < c0 + n) return HCF_ERR_ARG;
  if (act < ACT_NONE || act > ACT_LRELU || (!y && (act != ACT_NONE || sum_zy)) || (absmax2 && !absmax)) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  EpiBwdArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.H = H; e.W = W;
  e.gy = nhwc_window(t, gy, B, n, H, W, cs, c0, st, rc);
  e.y = y ? nhwc_window(t, y, B, n, H, W, cs, c0, st, rc) : mkview(nullptr, cs, c0, n);
  e.gpre = e.gy;                                        // in place, as the engine runs it (bwd_conv)
  if (scale) {
    std::vector<float> hs((size_t)((n + 31) / 32) * 32, 1.f);
    for (int c = 0; c < n; ++c) hs[c] = scale[c];
    e.scale = t.up(hs);
  }
  e.act = act;
  e.has1 = has1; e.rs1 = rs1; e.has2 = has2; e.rs2 = rs2;
  e.g1 = (has1 && g1) ? nhwc_window(t, g1, B, n, H, W, cs, c0, st, rc) : mkview(nullptr, cs, c0, n);
  e.g2 = (has2 && g2) ? nhwc_window(t, g2, B, n, H, W, cs, c0, st, rc) : mkview(nullptr, cs, c0, n);
  e.sum_pre = sum_pre; e.sum_zy = sum_zy; e.zy_mult = zy_mult;
  e.absmax = absmax; e.absmax2 = absmax2; e.carry2 = carry2;
  const int nblk = conv_epilogue_bwd_blocks(B, H, W);
  if (sum_pre || sum_zy) e.part = part_rows(t, (size_t)nblk * 2 * n, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = launch_conv_epilogue_bwd(e, st);
  if (rc == HCF_OK && e.part) rc = reduce_rows(t, e.part, nblk, n, n, sum_pre, sum_zy, zy_mult, st);
  if (rc == HCF_OK) rc = launch_nhwc_to_nchw(e.gpre, gpre, B, n, H, W, 0, st);
  if (rc == HCF_OK && e.g1.p) rc = launch_nhwc_to_nchw(e.g1, g1, B, n, H, W, 0, st);
  if (rc == HCF_OK && e.g2.p) rc = launch_nhwc_to_nchw(e.g2, g2, B, n, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_lu_chain(const float* dW, const float* P, const float* L, const float* U, float* dl, float* du, float* dlog_s,
                    int32_t C, hcf_stream_t stream) {
  if (!dW || !P || !L || !U || !dl || !du || !dlog_s || C < 1 || C > 48) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  LuChainArgs a;
  a.dW = dW; a.P = P; a.L = L; a.U = U; a.dl = dl; a.du = du; a.dlog_s = dlog_s; a.C = C;
  const int rc = launch_lu_chain(a, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_seed_sum(const float* g, int32_t B, float* out, hcf_stream_t stream) {
  if (!g || !out || B < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_seed_sum(g, B, out, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_axpy_job(const float* x, float* y, int32_t n, float alpha, const float* k_dev, hcf_stream_t stream) {
  if (!y || n < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  AxpyJob j;
  j.x = x; j.y = y; j.n = n; j.alpha = alpha; j.k_dev = k_dev;
  AxpyJob* jd = reinterpret_cast<AxpyJob*>(t.dev((sizeof(AxpyJob) + sizeof(float) - 1) / sizeof(float)));
  if (!t.ok) return HCF_ERR_NOMEM;
  if (hipMemcpy(jd, &j, sizeof(j), hipMemcpyHostToDevice) != hipSuccess) return HCF_ERR_HIP;
  const int rc = launch_axpy_jobs(jd, 1, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

// ---- the fused f16x3 conv launches of the inference path, one launch per call (tests/test_gpu_fused_convs.py) ----------

int hcf_op_fcn12(const float* const* src, const int32_t* src_c, const int32_t* src_up, int32_t n_src, int32_t B, int32_t H,
                 int32_t W, const float* w1, const float* bias1, const float* scale1, const float* w2, const float* bias2,
                 const float* scale2, const float* pre, float* out, int32_t form, int32_t* info, hcf_stream_t stream) {
  if (!src || !src_c || !w1 || !w2 || !out || !info || n_src < 1 || n_src > kMaxSrc || B < 1 || H < 1 || W < 1 || (form != 0 && form != 1))
    return HCF_ERR_ARG;
  for (int i = 0; i < n_src; ++i) {
    const int up = src_up ? src_up[i] : 0;
    if (!src[i] || src_c[i] < 1 || up < 0 || up > 8 || !up_divides(H, W, up)) return HCF_ERR_ARG;
  }
  for (int i = 0; i < 16; ++i) info[i] = 0;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  ConvArgs a;
  ConvPacks pk;
  View sv[kMaxSrc];
  int cin = 0, srcs[kMaxSrc];
  stage_sources(t, src, src_c, src_up, n_src, B, H, W, sv, srcs, cin, st, rc);
  const size_t nout = (size_t)B * H * W * 64;
  float* o = t.dev(nout);
  const int rb = conv_call(t, a, pk, sv, n_src, B, H, W, bias1, scale1, 64, ACT_RELU, mkview(o, 64, 0, 64), true, st);
  a.bias2 = table(t, bias2, 64, 64, 0.f);
  a.scale2 = table(t, scale2, 64, 64, 1.f);
  a.act2 = ACT_RELU;
  if (pre) a.res1 = nhwc_from_nchw(t, pre, B, 64, H, W, st, rc);        // the pre-activation term travels as res1
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = rb;
  if (rc != HCF_OK) return rc;
  if (hipMemsetAsync(o, 0xff, nout * sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;      // a pixel the launch skips reads NaN
  const unsigned allow = (form == 0 ? 1u << CONV_FCN12 : 0u) | 1u << CONV_F16X3;
  if ((rc = conv_packs(t, a, pk, w1, cin, 64, 9, srcs, n_src, true, allow)) != HCF_OK) return rc;
  std::vector<float> h2;
  int one = 64, nchunk2 = 0, npad2 = 0;
  if (!pack_conv_weights_f16x3(w2, 64, 64, 1, &one, 1, h2, nchunk2, npad2)) return HCF_ERR_UNSUPPORTED;
  a.w2 = pk.f16_2 = t.up(h2);
  if (!t.ok) return HCF_ERR_NOMEM;
  const ConvRoute rt = route_conv(a, pk, 9, allow, st);
  rc = rt.status;
  if (rt.form == CONV_FCN12) {
    info[0] = 0; info[1] = rc; info[11] = (int32_t)rt.fcn_grid; info[12] = 256; info[13] = rt.fcn_tiles; info[14] = pre ? 1 : 0;
  } else {
    info_f16x3(a, 9, 12, info);
  }
  if (rc != HCF_OK) { hipStreamSynchronize(st); return rc; }      // (the temporaries are freed behind the staging launches)
  if ((rc = conv_finish(pk.flag, info, st)) != HCF_OK) return rc;
  rc = launch_nhwc_to_nchw(a.out, out, B, 64, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_conv2d_step_inverse(const float* h2, int32_t hid, const float* w3, const float* bias3, const float* scale3,
                               int32_t f_out, const float* z, int32_t C, int32_t mode, int32_t ns, const float* mat,
                               const float* an_bias, const float* an_logs, float* out_z, float* out_zpad, int32_t zpad_n,
                               int32_t B, int32_t H, int32_t W, int32_t* info, hcf_stream_t stream) {
  if (!h2 || !w3 || !z || !an_bias || !an_logs || !out_z || !info || hid < 1 || f_out < 1 || f_out > 96) return HCF_ERR_ARG;
  if (!step_shape_ok(B, C, H, W, f_out, mode, ns) || (out_zpad && (zpad_n < 0 || zpad_n > 16 || zpad_n > C))) return HCF_ERR_ARG;
  for (int i = 0; i < 16; ++i) info[i] = 0;
  const int M = step_cmax(C);
  if (M < 0) return HCF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  ConvArgs a;
  ConvPacks pk;
  const View hv = nhwc_from_nchw(t, h2, B, hid, H, W, st, rc);
  // (out: sc.hout of the engine, the fused launch leaves it alone)
  const int rb = conv_call(t, a, pk, &hv, 1, B, H, W, bias3, scale3, f_out, ACT_NONE,
                           mkview(t.dev((size_t)B * H * W * ru4(f_out)), ru4(f_out), 0, f_out), true, st);
  // the tail fields of the step's StepArgs (in place on z)
  a.tz = nhwc_from_nchw(t, z, B, C, H, W, st, rc);
  a.tzo = a.tz;
  std::vector<float> hb(M, 0.f), hm(M, 0.f);
  for (int c = 0; c < C; ++c) { hb[c] = an_bias[c]; hm[c] = expf(-an_logs[c]); }
  a.tbias = t.up(hb);
  a.tmul = t.up(hm);
  if (mat) {
    std::vector<float> wi;
    if (!invert64(mat, C, wi, M)) return HCF_ERR_ARG;
    a.tmat = t.up(wi);
  }
  a.tC = C; a.tns = ns; a.tmode = mode;
  const size_t npadz = (size_t)B * H * W * 16;
  if (out_zpad) {
    a.tzpad = t.dev(npadz);
    a.tzpad_n = zpad_n;
  }
  if (!t.ok) return HCF_ERR_NOMEM;
  if (rc == HCF_OK) rc = rb;
  if (rc != HCF_OK) return rc;
  if (a.tzpad && hipMemsetAsync(a.tzpad, 0xff, npadz * sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;
  int one = hid;
  if ((rc = conv_packs(t, a, pk, w3, hid, f_out, 9, &one, 1, true, 1u << CONV_F16X3)) != HCF_OK) return rc;
  rc = route_conv(a, pk, 9, 1u << CONV_F16X3, st).status;
  info_f16x3(a, 9, 12, info);
  if (rc != HCF_OK) { hipStreamSynchronize(st); return rc; }
  if ((rc = conv_finish(pk.flag, info, st)) != HCF_OK) return rc;
  rc = launch_nhwc_to_nchw(a.tzo, out_z, B, C, H, W, 0, st);
  if (rc == HCF_OK && out_zpad) rc = launch_nhwc_to_nchw(mkview(a.tzpad, 16, 0, 16), out_zpad, B, 16, H, W, 0, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

}  // extern "C"

// ---- the conv kernels on the caller's channel windows, one launch per call (tests/test_gpu_view_convs.py) --------------
namespace hcf {

// a well-formed descriptor (include/hcflow.h: hcf_view); max_up = 0 for every view that is not a conv source
static bool view_ok(const hcf_view* v, int max_up) {
  return v && v->p && v->cs >= 1 && v->c0 >= 0 && v->n >= 1 && (long long)v->c0 + v->n <= v->cs && v->up >= 0 && v->up <= max_up;
}
static View as_view(const hcf_view* v) { return v ? mkview(v->p, v->cs, v->c0, v->n, v->up) : mkview(nullptr, 0, 0, 0); }

// 1 .. 3 source descriptors of a conv on [B, H, W] -> views (unused slots repeat source 0, as everywhere); false: HCF_ERR_ARG
static bool views_of_sources(const hcf_view* src, int n_src, int H, int W, View* dst, int* srcs, int& cin) {
  if (!src || n_src < 1 || n_src > kMaxSrc) return false;
  cin = 0;
  for (int i = 0; i < n_src; ++i) {
    if (!view_ok(&src[i], 8) || !up_divides(H, W, src[i].up)) return false;
    dst[i] = as_view(&src[i]);
    srcs[i] = src[i].n;
    cin += src[i].n;
  }
  for (int i = n_src; i < kMaxSrc; ++i) dst[i] = dst[0];
  return true;
}

}  // namespace hcf

extern "C" {

int hcf_op_conv2d_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const float* w, const float* bias,
                        const float* scale, int32_t k, int32_t act, const hcf_view* res1, float rs1, const hcf_view* res2,
                        float rs2, const hcf_view* out, int32_t scaled, int32_t* info, hcf_stream_t stream) {
  if (!w || !info || (k != 1 && k != 3) || B < 1 || H < 1 || W < 1 || act < ACT_NONE || act > ACT_LRELU) return HCF_ERR_ARG;
  if (!view_ok(out, 0) || out->n > 96) return HCF_ERR_ARG;
  if ((res1 && (!view_ok(res1, 0) || res1->n != out->n)) || (res2 && (!view_ok(res2, 0) || res2->n != out->n))) return HCF_ERR_ARG;
  ConvArgs a;
  ConvPacks pk;
  View sv[kMaxSrc];
  int cin = 0, srcs[kMaxSrc];
  if (!views_of_sources(src, n_src, H, W, sv, srcs, cin)) return HCF_ERR_ARG;
  for (int i = 0; i < 16; ++i) info[i] = 0;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  const int cout = out->n, taps = k * k;
  const bool f16 = op_f16(cout);      // (a stand-alone 1x1 too, where the f16x3 plan accepts it)
  int rc = conv_call(t, a, pk, sv, n_src, B, H, W, bias, scale, cout, act, as_view(out), f16, st);
  if (rc != HCF_OK) return rc;
  a.res1 = as_view(res1); a.rs1 = res1 ? rs1 : 0.f;
  a.res2 = as_view(res2); a.rs2 = res2 ? rs2 : 0.f;
  if (f16 && scaled && (rc = conv_in_max(t, a, st)) != HCF_OK) { hipStreamSynchronize(st); return rc; }
  if ((rc = conv_packs(t, a, pk, w, cin, cout, taps, srcs, n_src, f16, kAllowAll)) != HCF_OK) { hipStreamSynchronize(st); return rc; }
  // (a stand-alone 1x1 the f16x3 plan refuses reaches the exact kernel with ovf, zeros and in_max still set, as in the engine: that
  //  kernel reads none of them, and the flag nobody raised is read into info[15] as 0)
  const ConvRoute rt = route_conv(a, pk, taps, kAllowAll, st);
  rc = rt.status;
  if (rt.form == CONV_WINO) {
    info[0] = cout == 64 ? 3 : 2; info[1] = rc; info[11] = conv_wino_grid(B, H, W, cout / 32);
  } else if (rt.form == CONV_F16X3) {
    info_f16x3(a, taps, 14, info);
  } else {
    const ExactPlan p = plan_conv_exact(a, taps);
    info[0] = 0; info[1] = p.status; info[2] = p.vec; info[3] = p.vec_epi; info[4] = p.nt;
    info[11] = (int32_t)p.grid; info[12] = 256; info[13] = p.vec_epi;
  }
  // (a refusal synchronises too: the temporaries are freed behind the staging work)
  if (rc != HCF_OK) return hipStreamSynchronize(st) != hipSuccess ? HCF_ERR_HIP : rc;
  return conv_finish(pk.flag, info, st);
}

int hcf_op_conv2d_dgrad_fused_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const float* w, int32_t k,
                                    const hcf_view* y, int32_t fb_act, const float* fb_scale, int32_t want_zy, float zy_mult,
                                    const hcf_view* out, float* sum_pre, float* sum_zy, float* fb_max, float* fb_max2, int32_t* info,
                                    hcf_stream_t stream) {
  if (!w || !info || !sum_pre || !fb_max || (k != 1 && k != 3) || B < 1 || H < 1 || W < 1 || fb_act < ACT_NONE || fb_act > ACT_LRELU)
    return HCF_ERR_ARG;
  if (!view_ok(out, 0) || out->n > 64 || !view_ok(y, 0) || y->n != out->n || (want_zy && !sum_zy)) return HCF_ERR_ARG;
  ConvArgs a;
  ConvPacks pk;
  View sv[kMaxSrc];
  int cin = 0, srcs[kMaxSrc];
  if (!views_of_sources(src, n_src, H, W, sv, srcs, cin)) return HCF_ERR_ARG;
  for (int i = 0; i < n_src; ++i)
    if (src[i].up) return HCF_ERR_ARG;                   // a data gradient's sources are gradients at the output's size
  for (int i = 0; i < 18; ++i) info[i] = 0;
  if (g_op_precision != PREC_F16X3) return HCF_ERR_UNSUPPORTED;      // the fused form exists in f16x3 only
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  const int n = out->n, taps = k * k;
  // launch_dgrad's arguments (hcf_engine_train.inc): unit bias and scale, no activation, plain store, the fused epilogue backward
  int rc = conv_call(t, a, pk, sv, n_src, B, H, W, nullptr, nullptr, n, ACT_NONE, as_view(out), true, st);
  if (rc != HCF_OK) return rc;
  if ((rc = conv_in_max(t, a, st)) != HCF_OK) { hipStreamSynchronize(st); return rc; }
  const int rows_cap = std::max(conv_f16x3_scaled_blocks_max(B, H, W), conv_wino_grid(B, H, W, 1));
  a.fb_y = as_view(y); a.fb_act = fb_act; a.fb_max = fb_max; a.fb_max2 = fb_max2;
  a.fb_part = part_rows(t, (size_t)rows_cap * 2 * n, st, rc);
  if (rc != HCF_OK) { hipStreamSynchronize(st); return rc; }
  if (fb_scale) a.fb_scale = table(t, fb_scale, n, ru32(n), 1.f);
  a.fb_zy = want_zy ? 1 : 0;
  // (the Winograd pack from 16 input channels on, the narrowest the engine builds for this kernel: a unit count beyond one round of
  //  blocks stays affordable for a test only on a narrow source)
  if ((rc = conv_packs(t, a, pk, w, cin, n, taps, srcs, n_src, true, 1u << CONV_WINO | 1u << CONV_F16X3, 16)) != HCF_OK) {
    hipStreamSynchronize(st);
    return rc;
  }
  // fused Winograd first, then the fused scaled f16x3 kernel once its rows are known to fit fb_part; never an unfused launch
  int rows = conv_wino_grid(B, H, W, 1);
  const ConvRoute rt = route_conv(a, pk, taps, 1u << CONV_WINO, st);
  rc = rt.status;
  if (rc != HCF_ERR_UNSUPPORTED) {
    info[0] = 2; info[1] = rc; info[11] = rows; info[17] = (int32_t)wino_units(B, H, W, 1);
  } else {
    const F16x3Plan p = info_f16x3(a, taps, 14, info);
    int sw = 0, th = 8;
    rows = conv_f16x3_scaled_blocks(B, H, W, &sw, &th);      // (conv_tile_blocks of the engine: the rows it hands to its sum job)
    rc = (p.status == HCF_OK && ((long long)p.grid > rows_cap || rows > rows_cap)) ? HCF_ERR_ARG
                                                                                   : route_conv(a, pk, taps, 1u << CONV_F16X3, st).status;
  }
  if (rc == HCF_OK) {
    info[16] = rows;
    rc = reduce_rows(t, a.fb_part, rows, n, n, sum_pre, sum_zy, zy_mult, st);      // (want_zy off: the second row holds the kernel's zeros)
  }
  if (rc != HCF_OK) return hipStreamSynchronize(st) != hipSuccess ? HCF_ERR_HIP : rc;
  return conv_finish(pk.flag, info, st);
}

int hcf_op_conv2d_wgrad_views(const hcf_view* src, int32_t n_src, int32_t B, int32_t H, int32_t W, const hcf_view* g, int32_t taps,
                              float* dw, int32_t* info, hcf_stream_t stream) {
  if (!dw || !info || (taps != 1 && taps != 9) || B < 1 || H < 1 || W < 1 || !view_ok(g, 0) || g->n > 96) return HCF_ERR_ARG;
  WgradArgs wa;
  memset(&wa, 0, sizeof(wa));
  int cin = 0, srcs[kMaxSrc];
  if (!views_of_sources(src, n_src, H, W, wa.src, srcs, cin)) return HCF_ERR_ARG;
  for (int i = 0; i < 16; ++i) info[i] = 0;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  wa.nsrc = n_src;
  wa.g = as_view(g);
  wa.B = B; wa.H = H; wa.W = W; wa.taps = taps;
  const size_t nw = (size_t)g->n * cin * taps;
  wa.dw = t.dev(nw);
  if (!t.ok) return HCF_ERR_NOMEM;
  if (hipMemsetAsync(wa.dw, 0, nw * sizeof(float), st) != hipSuccess) return HCF_ERR_HIP;
  if (g_op_precision == PREC_F16X3 && (rc = wgrad_f16_range(t, wa, st)) != HCF_OK) return rc;
  wa.part_cap = conv_wgrad_scratch_floats(wa);
  wa.part = t.dev(wa.part_cap);
  if (!t.ok) return HCF_ERR_NOMEM;
  const WgradPlan p = plan_conv_wgrad(wa);
  const int32_t v[8] = {p.status, p.f16, p.taps, p.vec, p.db, p.strip_w, p.tpb, p.nblk_x};
  for (int i = 0; i < 8; ++i) info[i] = v[i];
  rc = launch_conv_wgrad(wa, st);
  if (rc == HCF_OK && hipMemcpyAsync(dw, wa.dw, nw * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) rc = HCF_ERR_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

int hcf_op_conv_epilogue_backward_views(const hcf_view* gy, const hcf_view* y, const float* scale, int32_t act, int32_t has1,
                                        float rs1, const hcf_view* g1, int32_t has2, float rs2, const hcf_view* g2,
                                        const hcf_view* gpre, float* sum_pre, float* sum_zy, float zy_mult, float* absmax,
                                        float* absmax2, const float* carry2, int32_t B, int32_t H, int32_t W, int32_t* info,
                                        hcf_stream_t stream) {
  if (!info || !view_ok(gy, 0) || !view_ok(gpre, 0) || gy->n > 256 || gpre->n != gy->n || B < 1 || H < 1 || W < 1) return HCF_ERR_ARG;
  const int n = gy->n;
  if ((y && (!view_ok(y, 0) || y->n != n)) || (g1 && (!view_ok(g1, 0) || g1->n != n)) || (g2 && (!view_ok(g2, 0) || g2->n != n)))
    return HCF_ERR_ARG;
  if (act < ACT_NONE || act > ACT_LRELU || (!y && (act != ACT_NONE || sum_zy)) || (absmax2 && !absmax)) return HCF_ERR_ARG;
  for (int i = 0; i < 4; ++i) info[i] = 0;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  int rc = HCF_OK;
  EpiBwdArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.H = H; e.W = W;
  e.gy = as_view(gy);
  e.gpre = as_view(gpre);
  e.y = y ? as_view(y) : mkview(nullptr, gy->cs, gy->c0, n);
  if (scale) e.scale = table(t, scale, n, ru32(n), 1.f);
  e.act = act;
  e.has1 = has1; e.rs1 = rs1; e.has2 = has2; e.rs2 = rs2;
  e.g1 = (has1 && g1) ? as_view(g1) : mkview(nullptr, gy->cs, gy->c0, n);
  e.g2 = (has2 && g2) ? as_view(g2) : mkview(nullptr, gy->cs, gy->c0, n);
  e.sum_pre = sum_pre; e.sum_zy = sum_zy; e.zy_mult = zy_mult;
  e.absmax = absmax; e.absmax2 = absmax2; e.carry2 = carry2;
  const int nblk = conv_epilogue_bwd_blocks(B, H, W);
  if (sum_pre || sum_zy) e.part = part_rows(t, (size_t)nblk * 2 * n, st, rc);
  if (!t.ok) return HCF_ERR_NOMEM;
  info[0] = conv_epilogue_bwd_vec(e); info[1] = nblk;
  if (rc == HCF_OK) rc = launch_conv_epilogue_bwd(e, st);
  if (rc == HCF_OK && e.part) rc = reduce_rows(t, e.part, nblk, n, n, sum_pre, sum_zy, zy_mult, st);
  if (hipStreamSynchronize(st) != hipSuccess) return HCF_ERR_HIP;
  return rc;
}

}  // extern "C"

// ---- micro-benchmark of the conv kernel (tools/conv_bench.py) ---------------------------------
// Allocates NHWC slabs once, launches the conv `iters` times back to back and times them with HIP
// events on the given stream. Inputs are uniform random in [-1, 1) (never zeros: DVFS, cdna guide
// rule 25); weights random. ms = average per launch.
extern "C" int hcf_bench_conv(int32_t B, int32_t H, int32_t W, const int32_t* src_c, int32_t n_src, int32_t cout,
                              int32_t k, int32_t iters, double* ms_per_launch, double* flops_per_launch,
                              hcf_stream_t stream) {
  if (!src_c || n_src < 1 || n_src > kMaxSrc || iters < 1) return HCF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Tmp t;
  ConvArgs a;
  ConvPacks pk;
  View sv[kMaxSrc];
  int cin = 0, srcs[kMaxSrc];
  uint32_t rng = 12345u;
  auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return ((rng >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
  for (int i = 0; i < n_src; ++i) {
    const int cs = ru4(src_c[i]);
    const size_t n = (size_t)B * H * W * cs;
    std::vector<float> h(n);
    for (size_t j = 0; j < n; ++j) h[j] = rnd();
    sv[i] = mkview(t.up(h), cs, 0, src_c[i]);
    srcs[i] = src_c[i];
    cin += src_c[i];
  }
  std::vector<float> w((size_t)cout * cin * k * k);
  for (auto& v : w) v = rnd() * 0.05f;
  const std::vector<float> hb(cout, 0.1f);
  std::vector<float> hpad(ru32(cout), 0.1f);      // (the padding entries of the bias table too)
  int rc = conv_call(t, a, pk, sv, n_src, B, H, W, hb.data(), nullptr, cout, ACT_LRELU,
                     mkview(t.dev((size_t)B * H * W * ru4(cout)), ru4(cout), 0, cout), op_f16(cout) && k == 3, st);
  if (rc != HCF_OK) return rc;
  if (hipMemcpy(const_cast<float*>(a.bias), hpad.data(), hpad.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return HCF_ERR_HIP;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  a.dbg = (unsigned long long*)t.dev(32);
  if (a.dbg) hipMemsetAsync(a.dbg, 0, 128, st);
  rc = pack_and_launch(t, a, pk, w.data(), cin, cout, k, srcs, n_src, st);     // pack + warm-up
  if (a.dbg) hipMemsetAsync(a.dbg, 0, 128, st);
  const bool f16 = a.ovf != nullptr;
  hipEventRecord(e0, st);
  for (int i = 0; i < iters && rc == HCF_OK; ++i) rc = f16 ? launch_conv_f16x3(a, k * k, st) : launch_conv(a, k * k, st);
  hipEventRecord(e1, st);
  if (hipEventSynchronize(e1) != hipSuccess) rc = HCF_ERR_HIP;
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (a.dbg) {
    unsigned long long hd[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    hipMemcpy(hd, a.dbg, 80, hipMemcpyDeviceToHost);
    if (hd[5] && hd[6])
      fprintf(stderr, "prologue parts: setup %.2f us, load issue %.2f us, wait + split %.2f us, LDS write + barrier %.2f us\n",
              hd[6] / 100.0 / hd[5], hd[7] / 100.0 / hd[5], hd[8] / 100.0 / hd[5], hd[9] / 100.0 / hd[5]);
    if (hd[1]) g_last_clock_mhz = 100.0 * (double)hd[0] / (double)hd[1];
    if (hd[5])
      fprintf(stderr, "block phases (avg of %llu blocks): prologue %.2f us, chunk loop %.2f us, epilogue %.2f us\n", hd[5],
              hd[2] / 100.0 / hd[5], hd[3] / 100.0 / hd[5], hd[4] / 100.0 / hd[5]);
  }
  if (ms_per_launch) *ms_per_launch = ms / iters;
  if (flops_per_launch) *flops_per_launch = 2.0 * k * k * cin * (double)cout * B * H * W;
  return rc;
}
