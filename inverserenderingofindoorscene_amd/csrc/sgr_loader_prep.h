// The decisions of the synthetic loader's batch preparation (dataLoader.py:118-154, 251-259), one definition each: the byte -> value maps of
// loadImage, the three mask bits, the order-preserving integer image of a float and the bucket walk of the radix select behind scaleHdr,
// and the 7-wide AND of the separable erosion.  `__host__ __device__`: the gfx950 kernels (sgr_loader_prep.hip) call these functions and so
// does the host build the CPU tests run against np.sort and scipy (tests/host_emul/loader_prep_main.cpp), so this header compiles with g++.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SGR_LP_HD __host__ __device__ __forceinline__
#else
#define SGR_LP_HD inline
#endif

namespace sgr {
namespace lp {

// loadImage (dataLoader.py:231): (im - 127.5) / 127.5 in fp32, a correctly rounded division
SGR_LP_HD float byte_unit(int u8) { return ((float)u8 - 127.5f) / 127.5f; }
// :120: seg = 0.5 * (. + 1)
SGR_LP_HD float byte_seg(int u8) { return 0.5f * (byte_unit(u8) + 1.0f); }

// :121-123 before the erosion.  kObj is bit 0: and7 below reads it
enum { kObj = 1, kArea = 2, kEnv = 4 };
SGR_LP_HD int seg_bits(int u8) {
  const float s = byte_seg(u8);
  return ((s > 0.49f && s < 0.51f) ? kArea : 0) | (s < 0.1f ? kEnv : 0) | (s > 0.9f ? kObj : 0);
}

// ---- radix select ---------------------------------------------------------------------------------------------------------------------
// key_of is monotone: a < b as floats  <=>  key_of(a) < key_of(b) as unsigned, with -0.0 one below +0.0 (they compare equal as floats, so
// either is "the" order statistic).  NaNs sort above +inf (sign clear) or below -inf (sign set): outside the domain, but only integers
// from here on, so nothing can fault.
SGR_LP_HD uint32_t key_of(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SGR_LP_HD float float_of(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  float x;
  memcpy(&x, &u, 4);
  return x;
}
constexpr int kRadixBits = 8, kBuckets = 1 << kRadixBits, kPasses = 32 / kRadixBits;
// pass p = 0 .. 3 looks at bits 31-8p .. 24-8p of the keys whose bits above them equal `prefix` (p = 0: every key)
SGR_LP_HD bool in_prefix(uint32_t key, uint32_t prefix, int pass) { return pass == 0 || (key >> (32 - kRadixBits * pass)) == prefix; }
SGR_LP_HD int digit_of(uint32_t key, int pass) { return (int)((key >> (32 - kRadixBits * (pass + 1))) & (kBuckets - 1)); }
// the bucket that holds the element of rank `rank` (0-based, ascending) among those counted in hist; rank becomes the rank inside it.
// rank < the histogram's total is the caller's invariant; the last bucket is returned if it is broken, so the walk cannot run off the end.
SGR_LP_HD int pick_bucket(const unsigned* hist, unsigned& rank) {
  int d = 0;
  for (; d < kBuckets - 1; ++d) {
    const unsigned c = hist[d];
    if (rank < c) break;
    rank -= c;
  }
  return d;
}

// ---- erosion --------------------------------------------------------------------------------------------------------------------------
// ndimage.binary_erosion(., ones((7, 7)), border_value=1): the AND over the 7 x 7 window, what lies outside the image counting as set.  A box
// is separable: the AND of 7 along x, then of 7 along y.  `p` points at the window's first element, `stride` apart.
constexpr int kErodeR = 3;
SGR_LP_HD int and7(const unsigned char* p, int stride) {
  int a = 1;
  for (int t = 0; t < 2 * kErodeR + 1; ++t) a &= p[t * stride];
  return a;
}

}  // namespace lp
}  // namespace sgr
