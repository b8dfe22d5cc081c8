// tanh of the decoder output heads (sgr_heads.hip: decoderLight's tail; sgr_brdf_heads.hip: decoder0's).  One definition, so that the
// two operators -- whose clamp kinks sit on the bits of 1.01 tanh(x) -- cannot drift apart.
#pragma once

#include "sgr_math.h"

namespace sgr {

// tanh to ~1 ulp: odd polynomial below 0.625 (no cancellation), 1 - 2/(e^{2|x|} + 1) above
__device__ __forceinline__ float tanh_f(float x) {
  const float ax = fabsf(x);
  const float z = x * x;
  float p = -5.70498872745e-3f;
  p = fmaf(p, z, 2.06390887954e-2f);
  p = fmaf(p, z, -5.37397155531e-2f);
  p = fmaf(p, z, 1.33314422036e-1f);
  p = fmaf(p, z, -3.33332819422e-1f);
  const float small = fmaf(p * z, x, x);
  const float e = fexp2(ax * 2.8853900817779268f);        // e^{2|x|}
  const float big = copysignf(1.0f - 2.0f / (e + 1.0f), x);
  return ax < 0.625f ? small : big;
}

}  // namespace sgr
