// The decisions of the real-image loaders' batch preparation (nyuDataLoader.py:75-131, 143-173; iiwDataLoader.py:136-137, 205-214), one
// definition each: the byte -> value maps of loadImage, the two normalisations of the normal, the crop rectangle and its clamp, the depth
// mask, the mirrored column and the colour scale.  The resize is OpenCV's INTER_LINEAR rule of sgr_export.h (src_of, lerp2), taken against
// the CROP.  `__host__ __device__`: the gfx950 kernels (sgr_real_loader.hip) call these functions and so does the host build the CPU tests
// run against the reference-made fixtures (tests/host_emul/real_loader_main.cpp), so this header compiles with g++.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sgr_export.h"

#if defined(__HIPCC__)
#define SGR_RL_HD __host__ __device__ __forceinline__
#else
#define SGR_RL_HD inline
#endif

namespace sgr {
namespace rl {

// ---- before the resize: one evaluation per byte value (the kernels keep the 256 results of each map in LDS) ------------------------------
// loadImage reverses cv2.imread's channels (:150): output channel k of im and normal is file channel 2 - k
SGR_RL_HD int file_channel(int k) { return 2 - k; }
// segNormal is channel 0 AFTER that reversal (:88): file channel 2
constexpr int kSegFileChannel = 2;
// :158: (im - 127.5) / 127.5 in fp32, a correctly rounded division
SGR_RL_HD float byte_unit(int u8) { return ((float)u8 - 127.5f) / 127.5f; }
// :88: 0.5 * (. + 1)
SGR_RL_HD float byte_seg(int u8) { return 0.5f * (byte_unit(u8) + 1.0f); }
// :155-156, 91: 0.5 * ((2 * (im / 255) ** 2.2 - 1) + 1); 2.2 used as fp32, as numpy does with a Python float
SGR_RL_HD float byte_im(int u8) { return 0.5f * ((2.0f * powf((float)u8 / 255.0f, 2.2f) - 1.0f) + 1.0f); }
// iiwDataLoader.py:137, 206: (im / 255) ** 2.2
SGR_RL_HD float byte_gamma(int u8) { return powf((float)u8 / 255.0f, 2.2f); }

// :95, per source pixel: n / sqrt(max(sum_c n^2, 1e-5)), the sum in channel order
SGR_RL_HD void unit_normal(float& n0, float& n1, float& n2) {
  const float d = sqrtf(fmaxf(n0 * n0 + n1 * n1 + n2 * n2, 1e-5f));
  n0 /= d;
  n1 /= d;
  n2 /= d;
}

// ---- the crop --------------------------------------------------------------------------------------------------------------------------
// (rs, cs, cropH, cropW) as the array OpenCV sees: rows rs .. rs + h - 1, columns cs .. cs + w - 1 of the source.
struct Rect { int rs, cs, h, w; };
SGR_RL_HD bool rect_inside(int rs, int cs, int h, int w, int Hs, int Ws) {
  return h >= 1 && w >= 1 && rs >= 0 && cs >= 0 && rs <= Hs - h && cs <= Ws - w;
}
// A rectangle that comes from device memory cannot be refused: it is moved and cut to lie inside the source, so nothing outside the source is
// read whatever it holds.  A rectangle that lies inside is returned as it is.
SGR_RL_HD Rect clamp_rect(int rs, int cs, int h, int w, int Hs, int Ws) {
  Rect r;
  r.rs = rs < 0 ? 0 : rs > Hs - 1 ? Hs - 1 : rs;
  r.cs = cs < 0 ? 0 : cs > Ws - 1 ? Ws - 1 : cs;
  r.h = h < 1 ? 1 : h > Hs - r.rs ? Hs - r.rs : h;
  r.w = w < 1 ? 1 : w > Ws - r.cs ? Ws - r.cs : w;
  return r;
}
// the two source elements of output index d along an axis of the crop, as offsets INSIDE the crop (0 .. n - 1), and the weight of the second
struct Tap { int a, b; float f; };
SGR_RL_HD Tap tap_of(int d, int n, int out) {
  const ex::Src s = ex::src_of(d, n, out);
  return Tap{s.s, s.s + 1 < n ? s.s + 1 : n - 1, s.f};
}
// columns first, then rows (v00 v01 / v10 v11)
SGR_RL_HD float bilerp(float v00, float v01, float v10, float v11, float fx, float fy) {
  return ex::lerp2(ex::lerp2(v00, v01, fx), ex::lerp2(v10, v11, fx), fy);
}

// ---- after the resize --------------------------------------------------------------------------------------------------------------------
// :103: (depth > 1) & (depth < 10) on the resized depth, exact 0 / 1 (a NaN gives 0)
SGR_RL_HD float seg_depth(float d) { return (d > 1.0f && d < 10.0f) ? 1.0f : 0.0f; }
// :109: n / max(sqrt(sum_c n^2), 1e-5)
SGR_RL_HD void renormalise(float& n0, float& n1, float& n2) {
  const float d = fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-5f);
  n0 /= d;
  n1 /= d;
  n2 /= d;
}
// :122-127: output column x takes column W - 1 - x where the image is mirrored
SGR_RL_HD int mirrored(int x, int W, bool flip) { return flip ? W - 1 - x : x; }
// :128-130, 137: numpy's fp32 array times a float64 array, cast back to fp32
SGR_RL_HD float colour_scale(float im, double c) { return (float)((double)im * c); }

}  // namespace rl
}  // namespace sgr
