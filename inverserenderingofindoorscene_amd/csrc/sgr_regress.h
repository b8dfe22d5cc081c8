// Device arithmetic shared by the streaming operators (sgr_loss.hip, sgr_brdf_loss.hip, sgr_recon_fold.h, sgr_glue.hip, sgr_brdf_input.hip, sgr_gn_stage.hip): the LSregress /
// LSregressDiffSpec coefficients from their folded sums (models.py:7-21, 23-84) and torch's bilinear source index.  One definition each,
// so that the operators that restate the same lines of the reference cannot drift apart.  The source index also compiles for the host
// (tests/host_emul, test infrastructure only).  The reductions that produce the folded sums are sgr_reduce.h (device only).
#pragma once

#include "sgr_math.h"

namespace sgr {

#if defined(__HIPCC__)

// (c_d, c_s) of models.py:44-63 from the five masked sums
__device__ __forceinline__ void diffspec_coefs(const double (&s)[5], float n_elems, float& cd, float& cs) {
  const float a11 = (float)s[0], a22 = (float)s[1], a12 = (float)s[2], b1 = (float)s[3], b2 = (float)s[4];
  const float frac = a11 * a22 - a12 * a12;
  const float c1 = (b1 * a22 - b2 * a12) / fmaxf(frac, 1e-2f);
  const float c2 = (-b1 * a12 + a11 * b2) / fmaxf(frac, 1e-2f);
  const float c3 = fminf(fmaxf(b1 / fmaxf(a11, 1e-5f), 0.001f), 1000.0f);
  const bool two = (frac / n_elems) > 1e-2f;
  cd = fminf(fmaxf(two ? c1 : c3, 0.0f), 1000.0f);
  cs = fminf(fmaxf(two ? c2 : 0.0f, 0.0f), 1000.0f);
}
__device__ __forceinline__ float unit_coef(double num, double den) {   // models.py:13-14, 72-77
  return fminf(fmaxf((float)num / fmaxf((float)den, 1e-5f), 0.001f), 1000.0f);
}

#endif  // __HIPCC__

// torch's upsample_bilinear2d source index (align_corners = False): max(scale * (dst + 0.5) - 0.5, 0)
SGR_HD void src_index(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
  const float r = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
  i0 = (int)r < in_size - 1 ? (int)r : in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = r - (float)i0;
  l0 = 1.0f - l1;
}

}  // namespace sgr
