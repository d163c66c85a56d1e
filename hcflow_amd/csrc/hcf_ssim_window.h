// The 11-tap window of the reference's SSIM (utils/util.py:918-920: cv2.getGaussianKernel(11, 1.5), window = k k^T), shared by the
// validation metrics (hcf_pair_metrics.hip) and the SSIM criterion (hcf_ssim.hip): one table, built on the host per call and
// passed to the kernels by value.
#ifndef HCF_SSIM_WINDOW_H_
#define HCF_SSIM_WINDOW_H_
#include <math.h>

namespace hcf {

struct Gauss11 { double g[11]; };

static Gauss11 gauss11() {
  Gauss11 gk;
  double sum = 0;
  for (int i = 0; i < 11; ++i) { gk.g[i] = exp(-((i - 5.0) * (i - 5.0)) / (2.0 * 1.5 * 1.5)); sum += gk.g[i]; }
  for (int i = 0; i < 11; ++i) gk.g[i] /= sum;
  return gk;
}

}  // namespace hcf
#endif  // HCF_SSIM_WINDOW_H_
