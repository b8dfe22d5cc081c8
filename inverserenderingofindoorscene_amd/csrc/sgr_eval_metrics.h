// The decisions of the three evaluation metrics (CompareWHDR.py:8-66, CompareNormal.py:18-42, CompareDepth.py:16-32), one definition each:
// the lightness of a judged pixel and the class the algorithm gives a pair, the six sums a judgement feeds, the unit ground-truth normal and
// the angle, the depth mask and the logarithm, and the walk of the two-rank radix select behind numpy's median.  The resize is OpenCV's
// INTER_LINEAR rule of sgr_export.h (src_of, lerp2), the keys and the bucket walk are those of sgr_loader_prep.h (key_of, pick_bucket): not
// restated.  `__host__ __device__`: the gfx950 kernels (sgr_eval_metrics.hip) call these functions and so does the host build the CPU tests
// run against numpy and the reference-made fixtures (tests/host_emul/eval_metrics_main.cpp), so this header compiles with g++.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sgr_export.h"
#include "sgr_loader_prep.h"

#if defined(__HIPCC__)
#define SGR_EM_HD __host__ __device__ __forceinline__
#else
#define SGR_EM_HD inline
#endif

namespace sgr {
namespace em {

// ---- WHDR (CompareWHDR.py:8-66) ------------------------------------------------------------------------------------------------------------
enum Label { kEqual = 0, kFirst = 1, kSecond = 2 };      // 'E', '1', '2'
// the six sums, in the order of `sums`
enum Sum { kErr = 0, kErrEq = 1, kErrIneq = 2, kWgt = 3, kWgtEq = 4, kWgtIneq = 5, kSums = 6 };

// :86: the saved PNG's byte / 255.0 in fp32, a correctly rounded division
SGR_EM_HD float byte_reflectance(int u8) { return (float)u8 / 255.0f; }
// :39: max(1e-10, np.mean(pixel)): the three channels added in order, divided by 3, all in fp32
SGR_EM_HD float lightness(float c0, float c1, float c2) { return fmaxf(1e-10f, ((c0 + c1) + c2) / 3.0f); }
// :43-48
SGR_EM_HD int whdr_class(float l1, float l2, float delta) {
  const float thr = 1.0f + delta;
  return l2 / l1 > thr ? kFirst : l1 / l2 > thr ? kSecond : kEqual;
}
// pixel (r, c) of an H x W image, or false: outside, never dereferenced
SGR_EM_HD bool inside(int r, int c, int H, int W) { return r >= 0 && r < H && c >= 0 && c < W; }
// does the judgement count at all (:25, 30; the stated deviations: a label outside 0..2 or a point outside the image counts as weight 0)
SGR_EM_HD bool judgement_counts(float weight, int label, bool both_inside) { return weight > 0.0f && label >= kEqual && label <= kSecond && both_inside; }
// :50-61: what a counted judgement adds to the six sums
SGR_EM_HD void whdr_add(double (&s)[kSums], int label, int alg, double w) {
  const bool wrong = label != alg;
  if (label == kEqual) {
    if (wrong) s[kErrEq] += w;
    s[kWgtEq] += w;
  } else {
    if (wrong) s[kErrIneq] += w;
    s[kWgtIneq] += w;
  }
  if (wrong) s[kErr] += w;
  s[kWgt] += w;
}
// :63-64; weight_sum == 0 gives 0 / 0 = NaN where the reference returns None
SGR_EM_HD void whdr_ratios(const double (&s)[kSums], float& whdr, float& equal, float& inequal) {
  whdr = (float)(s[kErr] / s[kWgt]);
  equal = (float)(s[kErrEq] / (s[kWgtEq] + 1e-10));
  inequal = (float)(s[kErrIneq] / (s[kWgtIneq] + 1e-10));
}

// ---- normal angle (CompareNormal.py:18-42) --------------------------------------------------------------------------------------------------
// :33: (byte - 127.5) / 127.5; :36: divided by its norm, the squares added in channel order (never zero for integer bytes)
SGR_EM_HD void gt_normal(int b0, int b1, int b2, float& g0, float& g1, float& g2) {
  g0 = ((float)b0 - 127.5f) / 127.5f;
  g1 = ((float)b1 - 127.5f) / 127.5f;
  g2 = ((float)b2 - 127.5f) / 127.5f;
  const float n = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
  g0 /= n;
  g1 /= n;
  g2 /= n;
}
// :38-39: arccos(clip(sum_c pred gt, -1, 1)) / pi * 180 in fp32; a NaN passes the clip, as it passes np.clip
SGR_EM_HD float angle_deg(float p0, float p1, float p2, float g0, float g1, float g2) {
  const float c = (p0 * g0 + p1 * g1) + p2 * g2;
  const float cc = c < -1.0f ? -1.0f : c > 1.0f ? 1.0f : c;
  return acosf(cc) / (float)M_PI * 180.0f;
}
// :27-28
SGR_EM_HD bool mask_counts(int m0, int m1, int m2) { return (m0 < m1 ? (m0 < m2 ? m0 : m2) : (m1 < m2 ? m1 : m2)) == 255; }

// ---- the median: two adjacent ranks in one radix select --------------------------------------------------------------------------------------
// Uncounted pixels carry kSentinel, the largest key, so no rank below the count reaches them (an angle's key is far below it).
constexpr uint32_t kSentinel = 0xffffffffu;
// numpy's median of n values: the elements of rank (n - 1) / 2 and n / 2 (the same element when n is odd)
SGR_EM_HD unsigned rank_lo(unsigned n) { return (n - 1) / 2; }
SGR_EM_HD unsigned rank_hi(unsigned n) { return n / 2; }
// The state of the two selects: the prefix found so far and the rank inside it.  Pass p histograms the p-th digit of the keys that carry
// prefix[0] into hist0 and of those that carry prefix[1] into hist1; while the two prefixes are equal only hist0 is filled and both ranks
// walk it.
struct Sel2 { uint32_t prefix[2]; unsigned rank[2]; };
SGR_EM_HD bool sel2_shared(const Sel2& s, int pass) { return pass == 0 || s.prefix[0] == s.prefix[1]; }
SGR_EM_HD void sel2_step(Sel2& s, const unsigned* hist0, const unsigned* hist1, int pass) {
  const bool shared = sel2_shared(s, pass);
  const int d0 = lp::pick_bucket(hist0, s.rank[0]);
  const int d1 = lp::pick_bucket(shared ? hist0 : hist1, s.rank[1]);
  s.prefix[0] = (pass ? s.prefix[0] << lp::kRadixBits : 0u) | (unsigned)d0;
  s.prefix[1] = (pass ? s.prefix[1] << lp::kRadixBits : 0u) | (unsigned)d1;
}
// (a + b) * 0.5f in fp32, numpy's mean of the two middle elements; count == 0 or a NaN among the counted angles: NaN
SGR_EM_HD float median_of(uint32_t key_lo, uint32_t key_hi, unsigned count, unsigned nans) {
  if (count == 0 || nans != 0) return NAN;
  return (lp::float_of(key_lo) + lp::float_of(key_hi)) * 0.5f;
}

// ---- log-depth RMSE (CompareDepth.py:16-32) --------------------------------------------------------------------------------------------------
// :20: strict on both sides (a NaN gives false)
SGR_EM_HD bool depth_counts(float gt) { return gt > 1.0f && gt < 10.0f; }
// :25-26
SGR_EM_HD float log_depth(float x) { return logf(x + 1e-20f); }
// the five sums of the one-pass form: log d and log g over ALL n pixels, and m, m (d - g), m (d - g)^2
enum DepthSum { kSd = 0, kSg = 1, kSm = 2, kSmx = 3, kSmxx = 4, kDepthSums = 5 };
SGR_EM_HD void depth_add(double (&s)[kDepthSums], float pred, float gt) {
  const double ld = (double)log_depth(pred), lg = (double)log_depth(gt), x = ld - lg;
  s[kSd] += ld;
  s[kSg] += lg;
  if (depth_counts(gt)) {
    s[kSm] += 1.0;
    s[kSmx] += x;
    s[kSmxx] += x * x;
  }
}
// :28-32: sum m ((d - md) - (g - mg))^2 / sum m with D = md - mg: (sum m x^2 - 2 D sum m x + D^2 sum m) / sum m; an empty mask: 0 / 0 = NaN
// No contraction here: with every product rounded, one counted pixel gives a - 2 a + a = 0 exactly, as the reference's 0 - 0; a fused
// multiply-add would leave the rounding error of x^2 behind.
SGR_EM_HD float depth_rmse(const double (&s)[kDepthSums], double n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double D = s[kSd] / n - s[kSg] / n;
  const double e = (s[kSmxx] - 2.0 * D * s[kSmx] + D * D * s[kSm]) / s[kSm];
  return (float)sqrt(e < 0.0 ? 0.0 : e);
}

}  // namespace em
}  // namespace sgr
