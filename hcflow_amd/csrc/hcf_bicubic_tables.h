// The MATLAB-style bicubic resize rule of the reference (utils/imresize.py) as host tables: one copy, shared by the PairMetrics
// kernels (hcf_pair_metrics.hip: float64 on a quantised image) and the tensor-to-tensor resize (hcf_resize.hip: fp32, both
// directions, with a backward). Host code only.
#pragma once
#include <math.h>
#include <vector>

namespace hcf {

static double cubic(double x) {                                   // utils/imresize.py:50-57
  const double ax = fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
  if (ax <= 1) return 1.5 * ax3 - 2.5 * ax2 + 1;
  if (ax <= 2) return -0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2;
  return 0.0;
}

// utils/imresize.py:60-82 (all columns kept: the dropped ones have zero weight)
static void contributions(int in_len, int out_len, double scale, std::vector<double>& w, std::vector<int>& idx, int& P) {
  const double kw = (scale < 1) ? 4.0 / scale : 4.0;
  P = (int)ceil(kw) + 2;
  w.assign((size_t)out_len * P, 0.0);
  idx.assign((size_t)out_len * P, 0);
  for (int o = 0; o < out_len; ++o) {
    const double u = (o + 1) / scale + 0.5 * (1 - 1 / scale);
    const double left = floor(u - kw / 2);
    double sum = 0;
    for (int k = 0; k < P; ++k) {
      const int ind = (int)(left + k - 1);
      const double t = u - ind - 1;
      const double v = (scale < 1) ? scale * cubic(scale * t) : cubic(t);
      w[(size_t)o * P + k] = v;
      sum += v;
      const int m = 2 * in_len;
      int r = ((ind % m) + m) % m;                                // mirror padding through aux = [0..n-1, n-1..0]
      idx[(size_t)o * P + k] = r < in_len ? r : 2 * in_len - 1 - r;
    }
    for (int k = 0; k < P; ++k) w[(size_t)o * P + k] /= sum;
  }
}

}  // namespace hcf
