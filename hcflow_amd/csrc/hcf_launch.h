// Host-side predicates and launch plans shared by the conv launchers (included by hcf_common.h).
//
// A plan_* function is PURE (arguments, process-wide switches and environment in; no HIP call, no launch) and decides all a launcher
// decides: the launcher is "plan, look the variant up in its table, launch", and hcf_debug_conv_plan pins the selection without a GPU.
#pragma once

namespace hcf {

static inline bool ptr16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// a channel window every pixel of which can be read / written as 16-byte quads
static inline bool view_vec16(const View& v) { return ((v.cs | v.c0) & 3) == 0 && ptr16(v.p); }
static inline bool view_vec16_or_null(const View& v) { return !v.p || view_vec16(v); }      // optional views (residuals)
// ConvArgs / WgradArgs::strip_magic: 2^32 / strip_w + 1 (exact division of values < 2^16 by a multiply-high), 0 without strips
static inline unsigned strip_magic(int strip_w) { return strip_w ? (unsigned)(0x100000000ull / (unsigned)strip_w) + 1u : 0u; }
// an output of H x W can be read through a nearest upsample by 2^up
static inline bool up_divides(int H, int W, int up) { return (H >> up) << up == H && (W >> up) << up == W; }

// One-time opt-in of `kernel` to `bytes` (> 64 KB) of dynamic LDS on the current device; `done` = the kernel's per-device flags, kept
// beside it in its launcher's table (several GPUs in one process: nn.DataParallel replicas). false: a HIP call failed.
static inline bool lds_opt_in(const void* kernel, int bytes, bool (&done)[64]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  if (!done[dev] && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  return done[dev] = true;
}

// ---- exact fp32 conv (hcf_conv.hip) ----
struct ExactPlan {
  int status;              // HCF_OK, or why launch_conv refuses the call
  int nt; bool vec;        // conv_mfma_kernel<taps, nt, vec>
  int vec_epi;             // the ConvArgs field "set by the launcher" (the 1x1 kernel of 64 / 96 channels has the scalar epilogue only)
  unsigned grid;
};
ExactPlan plan_conv_exact(const ConvArgs& a, int taps);
bool conv_epilogue_bwd_vec(const EpiBwdArgs& a);      // launch_conv_epilogue_bwd runs conv_epilogue_bwd_vec_kernel (hcf_train.hip)

// ---- f16x3 conv (hcf_conv_f16x3.hip) ----
struct F16x3Variant { int ntb, vec, up, fuse2, tailc, th, scaled, k1, n16; };      // conv_f16x3_kernel's template arguments (no padding: rows compare bytewise)
struct F16x3Plan {
  int status;              // HCF_OK, or why launch_conv_f16x3 refuses the call (HCF_ERR_ARG / HCF_ERR_UNSUPPORTED); the rest is then zero
  F16x3Variant v;
  unsigned grid, block;
  int any_up, vec_epi, strip_w; unsigned strip_magic;      // the ConvArgs fields "set by the launcher"
};
F16x3Plan plan_conv_f16x3(const ConvArgs& a, int taps);
// rows of ConvArgs::fb_part no scaled launch on [B, H, W] exceeds, whatever tile height and walk conv_f16x3_scaled_blocks picks
int conv_f16x3_scaled_blocks_max(int B, int H, int W);

// ---- conv weight gradient (hcf_conv_wgrad.hip) ----
struct WgradPlan {
  int status;              // HCF_OK or HCF_ERR_ARG (the geometry is filled in all the same: workspaces are sized from half-filled arguments)
  bool f16; int taps; bool vec; int db;      // kernel: f16x3 (a.g_max) or fp32; conv_wgrad_f16x3_kernel<taps, vec, db> / conv_wgrad_kernel<taps, vec>
  int nblk_x, nicb, nocb;  // grid of the one-conv launch; the batched launch gives the job nblk_x * nicb * nocb blocks
  int block, lds_bytes;
  int tpb, cin_total, strip_w; unsigned strip_magic;      // the WgradArgs fields "set by the launcher"
  size_t scratch_floats;   // partial tiles the launch leaves in WgradArgs::part
  int nbx;                 // the reduce step runs on a grid of (nbx, nicb, nocb) over nblk_x partial tiles per element
};
WgradPlan plan_conv_wgrad(const WgradArgs& a);

long long wino_units(int B, int H, int W, int ntile_n);      // units a Winograd launch walks (hcf_conv_wino.hip)

// ---- which kernel family a conv call takes (hcf_conv_route.hip) ----
// The one place that knows the order: the engine's forward and data-gradient convs, the per-op entries of hcf_ops.hip and the auxiliary
// nets' hcf_aux_conv2d all launch through route_conv. What differs between callers arrives as a null pack or a cleared `allow` bit.
enum ConvForm { CONV_NONE = -1, CONV_WINO = 0, CONV_FCN12 = 1, CONV_F16X3 = 2, CONV_EXACT = 3 };
constexpr unsigned kAllowAll = 15u;                           // `allow`: bit (1 << form)
struct ConvPacks {           // the weight packs a caller has for one conv; null: none, the forms that need it are not tried
  const float* exact;        // fp32 pack (launch_conv)
  const float* f16;          // f16x3 pack (launch_fcn12, launch_conv_f16x3)
  const void* wino;          // Winograd pack (launch_conv_wino)
  const float* f16_2;        // a fused 1x1 second layer: its f16x3 pack ... (these two pointers, not ConvArgs::bias2 / scale2 / act2 which the
                             // caller fills as well, are what tells the router that a second layer is fused)
  const void* wino_frag2;    // ... and its fragment for the 64-channel Winograd kernel's epilogue
  int* flag;                 // the f16 forms' range flag, 64 bytes of zeros 64 bytes behind it (-> ConvArgs::ovf, zeros)
};
struct ConvRoute {
  int form, status;          // the last form tried (CONV_NONE: none was) and its answer; HCF_ERR_UNSUPPORTED: every form tried declined
  unsigned fcn_grid; int fcn_tiles;      // CONV_FCN12 only: what launch_fcn12 reports
};
// The forms route_conv would try for the call, in order, without a launch (PURE, as the plans above); returns how many
int conv_route_forms(const ConvArgs& a, const ConvPacks& p, int taps, unsigned allow, int forms[4]);
// Tries them until one answers something other than HCF_ERR_UNSUPPORTED. `a` is complete but for what depends on the form -- wpack,
// w2, wf1x1, ovf, zeros -- which each form patches into a copy that it hands on to the next
ConvRoute route_conv(const ConvArgs& a, const ConvPacks& p, int taps, unsigned allow, hipStream_t st);

}  // namespace hcf
