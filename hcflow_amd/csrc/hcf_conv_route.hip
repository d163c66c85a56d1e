// Which kernel family a conv call takes (declared in hcf_launch.h). Every caller of the conv kernels routes here: run_conv and
// launch_dgrad of the engine, the per-op entries of hcf_ops.hip, hcf_aux_conv2d. The order:
//   1. Winograd: a Winograd pack, no fused tail, no fused second layer unless its Winograd fragment came along, kAblNoWino off;
//   2. with an f16x3 pack and 3x3 taps, or a 1x1 that fuses nothing: fcn12 (a second layer, no tail), then f16x3, then -- the 1x1
//      only, for views its one-tap form does not take -- exact;
//   3. otherwise exact.
// A form whose pack is null is not tried, exact included. Whether a second layer is fused is read from the PACKS (f16_2 / wino_frag2), a
// fused tail from ConvArgs::tC: a caller without either pack of its second layer gets the conv alone.
// A form is tried when its `allow` bit is set; the first answer other than HCF_ERR_UNSUPPORTED ends the walk.
#include "hcf_common.h"

namespace hcf {
extern int g_f16x3_ablation;   // hcf_conv_f16x3.hip

int conv_route_forms(const ConvArgs& a, const ConvPacks& p, int taps, unsigned allow, int forms[4]) {
  const bool fuse2 = p.f16_2 || p.wino_frag2, tail = a.tC > 0;
  int n = 0;
  auto add = [&](int form) { if ((allow & (1u << form)) && (form != CONV_EXACT || p.exact)) forms[n++] = form; };      // (no exact pack: no exact launch)
  if (p.wino && !tail && (!fuse2 || p.wino_frag2) && !(g_f16x3_ablation & kAblNoWino)) add(CONV_WINO);
  if (p.f16 && (taps == 9 || (taps == 1 && !fuse2 && !tail))) {
    if (fuse2 && !tail) add(CONV_FCN12);      // one K chunk: the persistent small-K form (res1 = pre-activation term, if any)
    add(CONV_F16X3);
    if (taps == 1) add(CONV_EXACT);
  } else {
    add(CONV_EXACT);
  }
  return n;
}

ConvRoute route_conv(const ConvArgs& a, const ConvPacks& p, int taps, unsigned allow, hipStream_t st) {
  int forms[4];
  const int n = conv_route_forms(a, p, taps, allow, forms);
  ConvRoute r = {CONV_NONE, HCF_ERR_UNSUPPORTED, 0u, 0};
  ConvArgs c = a;
  for (int i = 0; i < n && r.status == HCF_ERR_UNSUPPORTED; ++i) {
    r.form = forms[i];
    if (r.form != CONV_EXACT) {
      c.ovf = p.flag;
      c.zeros = reinterpret_cast<const float*>(p.flag) + 16;
    }
    switch (r.form) {
      case CONV_WINO:
        c.wf1x1 = p.wino_frag2;
        r.status = launch_conv_wino(c, p.wino, st);
        break;
      case CONV_FCN12:
        c.wpack = p.f16; c.w2 = p.f16_2;
        r.status = launch_fcn12(c, st, &r.fcn_grid, &r.fcn_tiles);
        break;
      case CONV_F16X3:
        c.wpack = p.f16; c.w2 = p.f16_2;
        r.status = launch_conv_f16x3(c, taps, st);
        break;
      default:
        c.wpack = p.exact;
        r.status = launch_conv(c, taps, st);
    }
  }
  return r;
}

}  // namespace hcf
