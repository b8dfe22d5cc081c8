// The decisions of testReal's output stage and of the image writers (testReal.py:542-657, utils.py:65-76, 102-154), one definition each:
// OpenCV's INTER_LINEAR source index for float data, the point maps of every kind before and after the resize, the quantiser, and the
// geometry of the env mosaic.  `__host__ __device__`: the gfx950 kernels (sgr_export.hip) call these functions and so does the host build
// the CPU tests run against the reference-made fixtures (tests/host_emul/export_main.cpp), so this header compiles with g++.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SGR_EX_HD __host__ __device__ __forceinline__
#else
#define SGR_EX_HD inline
#endif

namespace sgr {
namespace ex {

// the `kind` argument of sgr_export_image (include/sgrender.h: SGR_EXPORT_*)
enum Kind { kAlbedo = 0, kNormal = 1, kRough = 2, kDepth = 3, kRendered = 4, kShading = 5, kImage = 6, kImageGamma = 7, kKinds = 8 };
enum Stat { kNoStat = 0, kMean = 1, kMax = 2 };

SGR_EX_HD int kind_stat(int kind) { return kind == kDepth || kind == kShading ? kMean : kind == kRendered ? kMax : kNoStat; }
// the kinds the reference resizes to the photograph's size; the others leave at the source's
SGR_EX_HD bool kind_resizes(int kind) { return kind <= kRendered; }
// source channels a kind takes: 3, 1, or (the image writers) either
SGR_EX_HD bool kind_takes(int kind, int C) { return (kind == kRough || kind == kDepth) ? C == 1 : (kind >= kImage) ? (C == 1 || C == 3) : C == 3; }
// channels written: utils.py:73-74 repeats a one-channel image three times; rough and depth stay single
SGR_EX_HD int kind_out_channels(int kind, int C) { return (kind >= kImage) ? 3 : C; }

// ---- cv2.resize(INTER_LINEAR), float data ------------------------------------------------------------------------------------------------
// Output index d of an axis of `out` elements reads source elements s and s + 1 with weights 1 - f and f.  The coordinate is formed in
// double and rounded to fp32 once, as OpenCV does (torch's src_index of sgr_regress.h forms the scale in fp32: another rule).  s is
// monotone in d.  f == 0 at both borders, so element s + 1 is never needed beyond the axis.
struct Src { int s; float f; };
SGR_EX_HD Src src_of(int d, int in, int out) {
  float f = (float)(((double)d + 0.5) * ((double)in / (double)out) - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.0f;
  }
  if (s >= in - 1) {
    s = in - 1;
    f = 0.0f;
  }
  return Src{s, f};
}
// S[s] (1 - f) + S[s + 1] f; f == 0 takes S[s] itself (the same bits for finite data, and a NaN next door stays next door)
SGR_EX_HD float lerp2(float a, float b, float f) { return f == 0.0f ? a : a * (1.0f - f) + b * f; }

// ---- the point maps ------------------------------------------------------------------------------------------------------------------------
// 1 / 2.2 formed in double, used as fp32: what numpy does with `fp32_array ** (1.0 / 2.2)`
SGR_EX_HD float gamma_exp() { return (float)(1.0 / 2.2); }

// the per-image parameter p of the maps below from the kind's statistic (the sum or the maximum over the image's n elements) or from `scale`
SGR_EX_HD float stat_param(int kind, double sum_or_max, double n) {
  if (kind == kDepth) return fmaxf((float)(sum_or_max / n), 1e-10f);      // testReal.py:582
  if (kind == kShading) return (float)(sum_or_max / n);                   // :640
  return (float)sum_or_max;                                               // :652
}

// before the resize: one evaluation per source element
SGR_EX_HD float pre_map(int kind, float x, float p) {
  switch (kind) {
    case kAlbedo: return powf(x * p, gamma_exp());           // :546, 551
    case kDepth: return x / p * 3.0f;                        // :582
    case kRendered: return powf(x / p, gamma_exp());         // :652
    default: return x;
  }
}
SGR_EX_HD float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
// after the resize: t, the value the cast truncates
SGR_EX_HD float post_map(int kind, float v, float p) {
  switch (kind) {
    case kAlbedo: return 255.0f * v;                                                  // :554
    case kNormal:
    case kRough: return 127.5f * (v + 1.0f);                                          // :566, 574: (255 * 0.5) * (n + 1)
    case kDepth: return 255.0f * (1.0f / fminf(fmaxf(v + 1.0f, 1e-6f), 10.0f));       // :585-586
    case kRendered: return clip01(v) * 255.0f;                                        // :656
    case kShading: return 255.0f * powf(clip01(v / p / 3.0f), gamma_exp());           // :640-642
    case kImage: return 255.0f * clip01(v);                                           // utils.py:69, 72
    default: return 255.0f * powf(clip01(v), gamma_exp());                            // utils.py:71; writeEnvToFile :126-127
  }
}
// (uint8) min(max(t, 0), 255) by truncation; fmaxf drops a NaN, so a NaN gives 0
SGR_EX_HD unsigned quantise(float t) { return (unsigned)(int)fminf(fmaxf(t, 0.0f), 255.0f); }

// ---- the env mosaic (utils.py:102-128) -----------------------------------------------------------------------------------------------------
// Every interY-th row and interX-th column of cells, tile (rId, cId) at (rId (eh + gap), cId (ew + gap)) on a background of 1.0.
struct Mosaic { int interY, interX, tilesY, tilesX, Hm, Wm; };
SGR_EX_HD Mosaic mosaic_of(int R, int C, int eh, int ew, int nrows, int ncols, int gap) {
  Mosaic m;
  m.interY = R / nrows;      // int(envRow / nrows); nrows > R is refused before this is called
  m.interX = C / ncols;
  m.tilesY = (R + m.interY - 1) / m.interY;      // len(np.arange(0, envRow, interY)): may exceed nrows
  m.tilesX = (C + m.interX - 1) / m.interX;
  m.Hm = m.tilesY * (eh + gap) + gap;
  m.Wm = m.tilesX * (ew + gap) + gap;
  return m;
}
// output coordinate y of an axis -> the sampled cell and the texel inside it; false: background (a gap, or the closing margin)
SGR_EX_HD bool mosaic_src(int y, int e, int gap, int tiles, int inter, int& cell, int& texel) {
  const int t = y / (e + gap);
  texel = y - t * (e + gap);
  cell = t * inter;
  return t < tiles && texel < e;
}

}  // namespace ex
}  // namespace sgr
