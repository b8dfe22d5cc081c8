// The index rule and the accumulation orders of the BRDF decoders' final pad + 3x3 convolution (sgr_final_conv.hip): ReplicationPad2d(1)
// followed by Conv2d(C -> 3, k = 3), models.py:155-156, 187.  `__host__ __device__`, so that the expressions the gfx950 kernels evaluate
// also compile with g++ (tests/host_emul/final_conv_emul.cpp, test infrastructure only -- the product has no CPU path).  DESIGN.md
// section 8g states the contract.
#pragma once

#include "sgr_math.h"

namespace sgr {

constexpr int kFcOut = 3;          // output channels: exactly three
constexpr int kFcMaxC = 256;       // input channels, at most: the weight tile [C][28] stays in LDS beside the map tiles (28 KiB of 64)
constexpr int kFcWPitch = 28;      // floats per input channel of the weight tile: [o][kh][kw] = 27, padded to a 16-byte multiple

// the pad: an index outside the map reads the nearest one inside
SGR_HD int fc_cl(int t, int n) { return t < 0 ? 0 : t > n - 1 ? n - 1 : t; }

// R_n(h) = {(i, k): 0 <= i < n, k in {0, 1, 2}, cl(i + k - 1, n) == h}: the outputs i that read input h, each with the tap k it reads it
// through.  Always three pairs, listed by k, then by i:
//   inside          (h+1, 0) (h, 1) (h-1, 2)
//   h = 0,   n >= 2 (0, 0) (1, 0) (0, 1)
//   h = n-1, n >= 2 (n-1, 1) (n-2, 2) (n-1, 2)
//   n = 1           (0, 0) (0, 1) (0, 2)
struct FcPairs { int i[3], k[3]; };
SGR_HD FcPairs fc_pairs(int h, int n) {
  // four cases written out: every array index is a constant, so the pairs stay in registers on the device
  const bool lo = h == 0, hi = h == n - 1;
  FcPairs p;
  p.i[0] = lo ? 0 : hi ? h : h + 1;
  p.i[1] = lo ? (hi ? 0 : 1) : hi ? h - 1 : h;
  p.i[2] = lo ? 0 : hi ? h : h - 1;
  p.k[0] = !lo && hi ? 1 : 0;
  p.k[1] = lo ? (hi ? 1 : 0) : hi ? 2 : 1;
  p.k[2] = lo && !hi ? 1 : 2;
  return p;
}

// FORWARD, one output out[b, o, i, j].  The order is fixed and does not depend on tile position or layout:
//   for every input channel c in turn:  t = 0;  for kh, for kw:  t = fmaf(Wt[o, c, kh, kw], y[b, c, cl(i+kh-1), cl(j+kw-1)], t);  acc += t
//   out = acc + bias[o]
// (one fmaf per tap; the nine taps of a channel are summed on their own and then added to the running sum: the chain of C * 9 fmaf into
// one accumulator loses about three times as much to rounding, and tests/test_final_conv.py holds the order to half the GPU bounds)
// w: the nine weights of (o, c) as [kh][kw]; v: the nine values as [kh][kw]
SGR_HD float fc_taps(const float* w, const float (&v)[9]) {
  float t = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; ++k) t = fmaf(w[k], v[k], t);
  return t;
}

// BACKWARD, DATA, one dy[b, c, h, w].  The cotangents of the outputs that read (h, w) are first gathered per tap:
//   G[o][kh][kw] = sum over the row pairs (i, kh') of R_H(h) with kh' == kh, in the order of fc_pairs, of
//                  sum over the column pairs (j, kw') of R_W(w) with kw' == kw, in that order, of g[b, o, i, j]
// (inside the map every sum has one term; on a border a tap holds up to two rows and two columns, and the tap on the far side holds none:
// G = 0), then, with weights that are the same for every pixel of the map,
//   dy = 0;  for o, for kh, for kw:  dy = fmaf(Wt[o, c, kh, kw], G[o][kh][kw], dy)
// gv: g[b, o, rows.i[r], cols.i[q]] as [r][q].  Terms that do not belong to a tap are added as +0, which changes no bit.
SGR_HD void fc_gather_taps(const float (&gv)[3][3], const FcPairs& rows, const FcPairs& cols, float (&G)[9]) {
  float r[3][3];      // [kh][q]: rows folded
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float s = 0.0f;
#pragma unroll
      for (int p = 0; p < 3; ++p) s += rows.k[p] == kh ? gv[p][q] : 0.0f;
      r[kh][q] = s;
    }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      float s = 0.0f;
#pragma unroll
      for (int q = 0; q < 3; ++q) s += cols.k[q] == kw ? r[kh][q] : 0.0f;
      G[3 * kh + kw] = s;
    }
}
// w: the 27 weights of channel c as [o][kh][kw]; G: [o][kh * 3 + kw]
SGR_HD float fc_dy(const float* w, const float (&G)[3][9]) {
  float d = 0.0f;
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int k = 0; k < 9; ++k) d = fmaf(w[9 * o + k], G[o][k], d);
  return d;
}

// BACKWARD, WEIGHTS: a thread adds, pixel by pixel of its strip in raster order, acc[o][kh][kw] = fmaf(g[b, o, i, j], y[b, c, cl(i+kh-1),
// cl(j+kw-1)], acc[o][kh][kw]) in fp32; the threads of a workgroup are added by sgr_reduce.h's block_sum, and the workgroups' partials in
// double in index order (b, then slice).  v: the nine values around the pixel as [kh][kw]; g3: the pixel's three cotangents.
SGR_HD void fc_dw_pixel(const float (&g3)[3], const float (&v)[9], float (&acc)[27]) {
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[9 * o + k] = fmaf(g3[o], v[k], acc[9 * o + k]);
}

}  // namespace sgr
