// Which element of a PyTorch-layout weight lands where in a derived pack: the index mappings of the repack jobs, shared by the
// device kernels that run the jobs (hcf_repack.hip, hcf_conv_wino.hip) and the host execution of the same recipes at finalize
// (hcf_engine_packs.inc), so each mapping exists once in the source. Loads only: the arithmetic stays with the kernels / packers.
#pragma once
#include "hcf_common.h"

namespace hcf {

// logical weight L[n][ci][t] of a direct (exact / f16x3) pack:
//   forward packs     L = w[n][ci][t]                          (w: [cout][cin][taps])
//   transposed packs  L = w[ci][off + n][taps - 1 - t]         (data gradient of channel block [off, off + nb))
__host__ __device__ __forceinline__ float logical_weight(const RepackArgs& a, int n, int ci, int t) {
  if (!a.transposed) return a.w[((size_t)n * a.cin_w + ci) * a.taps + t];
  return a.w[((size_t)ci * a.cin_w + a.off + n) * a.taps + (a.taps - 1 - t)];
}

// the 3x3 taps g of element (oc, ic) of a Winograd pack (struct RepackWinoJob: two row sources, row strides, a zero-padded z1
// window; tr: input channels [k0, k0 + kn) from one forward conv's weight, transposed and flipped)
__host__ __device__ __forceinline__ void wino_taps(const RepackWinoJob& jb, int oc, int ic, float g[9]) {
  if (jb.tr) {
    const float* src = jb.w + (size_t)(ic - jb.k0) * jb.ld + (size_t)(jb.tr_off + oc) * 9;
    for (int t = 0; t < 9; ++t) g[t] = src[8 - t];
  } else {
    const int ld = jb.ld ? jb.ld : jb.cin * 9, ld2 = jb.ld2 ? jb.ld2 : jb.cin * 9;
    const float* row = (!jb.w2 || oc < jb.split) ? jb.w + (size_t)oc * ld : jb.w2 + (size_t)(oc - jb.split) * ld2;
    const int col = jb.z1_pad == 0 ? ic : (ic < jb.z1_n ? ic : ic < jb.z1_pad ? -1 : ic - jb.z1_pad + jb.z1_n);
    for (int t = 0; t < 9; ++t) g[t] = col >= 0 ? row[(size_t)col * 9 + t] : 0.f;
  }
}

}  // namespace hcf
