// Per-element arithmetic of the CNN stage glue (sgr_gn_stage.hip): GroupNorm + ReLU, the 2x bilinear upsample of models.py:163-183 /
// 310-330 and its adjoint, the resize to the skip's size of models.py:165-166 and its adjoint.  `__host__ __device__`, so that the
// expressions the gfx950 kernels evaluate also compile with g++ (tests/host_emul/gn_stage_emul.cpp and gn_resize_emul.cpp, test
// infrastructure only -- the product has no CPU path).  DESIGN.md section 8e states the contract.
#pragma once

#include "sgr_math.h"
#include "sgr_regress.h"

namespace sgr {

// ---- bf16 input / output: the kernels of the same-size stage are instantiated on the type of x, skip, the result,
// the cotangent, dx and dskip; everything between a load and a store is the fp32 arithmetic below.  A bf16 element travels as its 16 bits.
struct bf16 { unsigned short bits; };
// upcast: the 16 bits become the upper half of the fp32 pattern -- exact, NaN and infinities included
SGR_HD float bf16_up(unsigned short h) {
  const unsigned u = (unsigned)h << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// round to nearest, ties to even, on the bit pattern: the carry of the addition moves into the exponent where the mantissa overflows, up
// to infinity from the largest finite values.  A NaN stays a NaN (quiet, sign and upper payload kept); infinities have a zero lower half
// and pass through.
SGR_HD unsigned short bf16_round(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x0040u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
// what a kernel does with an element of its I/O type T (float or bf16) on load and on store
SGR_HD float gn_in(float v) { return v; }
SGR_HD float gn_in(bf16 v) { return bf16_up(v.bits); }
template <typename T> SGR_HD T gn_out(float v);
template <> SGR_HD float gn_out<float>(float v) { return v; }
template <> SGR_HD bf16 gn_out<bf16>(float v) { return bf16{bf16_round(v)}; }

// (mean, rstd) of a group from its two double-precision sums over n elements.  The mean is kept as an fp32 pair (mh + ml): at
// x = 100 + N(0,1) an fp32 mean alone is off by up to 4e-6 of the standard deviation, in every element of the group alike.
SGR_HD void gn_finish(double s, double ss, double n, float eps, float& mh, float& ml, float& rstd, float& var) {
  const double m = s / n;
  double v = ss / n - m * m;
  v = v > 0.0 ? v : 0.0;
  mh = (float)m;
  ml = (float)(m - (double)mh);
  var = (float)v;
  rstd = (float)(1.0 / sqrt(v + (double)eps));
}
// The forward and the backward evaluate these two lines, and nothing else, for the ReLU's argument: the mask is the forward's.
SGR_HD float gn_xhat(float x, float mh, float ml, float rstd) { return ((x - mh) - ml) * rstd; }
SGR_HD float gn_pre(float xhat, float w, float b) { return fmaf(xhat, w, b); }
// dx = rstd (dy w - c1 - xhat c2), c1 = sum_g(dy w) / n, c2 = sum_g(dy w xhat) / n
SGR_HD float gn_dx(float dy, float xhat, float w, float rstd, float c1, float c2) { return rstd * fmaf(-xhat, c2, fmaf(dy, w, -c1)); }

// weights (l0, l1) of the two taps of output index o at scale 2 (sgr_regress.h's rule; the taps are o / 2 - 1 + (o & 1) and its successor,
// clamped -- a clamped tap carries the weight the rule gives it, which is 0 at the low edge and adds up to 1 at the high edge)
struct UpTap { float l0, l1; };
SGR_HD UpTap up_tap(int o, int n) {
  int i0, i1;
  UpTap t;
  src_index(o, 0.5f, n, i0, i1, t.l0, t.l1);
  return t;
}
// what source index `src` receives from output index o: the rule's own weights, read backwards
SGR_HD float up_adj_w(int o, int src, int n) {
  if (o < 0 || o >= 2 * n) return 0.0f;
  int i0, i1;
  float l0, l1;
  src_index(o, 0.5f, n, i0, i1, l0, l1);
  return (i0 == src ? l0 : 0.0f) + (i1 == src ? l1 : 0.0f);
}
// For an output index inside the map the rule's weights depend on nothing but o == 0 and o's parity: the three pairs, read off src_index
// once per thread instead of once per output
struct UpTaps { UpTap first, even, odd; };
SGR_HD UpTaps up_taps() { return {up_tap(0, 2), up_tap(2, 2), up_tap(1, 2)}; }
SGR_HD UpTap up_pick(const UpTaps& t, int o) { return o == 0 ? t.first : (o & 1) ? t.odd : t.even; }
// The four adjoint weights of source index src (outputs 2 src - 1 .. 2 src + 2).  They are the same for every 1 <= src <= n - 2, so a
// thread evaluates the rule for src = 0, 1 and n - 1 once and picks (src = 0 first: with n = 1 it is both edges)
SGR_HD void up_adj_sets(int n, float (&low)[4], float (&mid)[4], float (&high)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    low[k] = up_adj_w(k - 1, 0, n);
    mid[k] = up_adj_w(1 + k, 1, n);
    high[k] = up_adj_w(2 * (n - 1) - 1 + k, n - 1, n);
  }
}
SGR_HD void up_adj_pick(const float (&low)[4], const float (&mid)[4], const float (&high)[4], int src, int n, float (&w)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = src == 0 ? low[k] : src == n - 1 ? high[k] : mid[k];
}
SGR_HD float up_lerp(UpTap t, float a, float b) { return fmaf(t.l1, b, t.l0 * a); }

// Output rows 2i, 2i+1 x columns 4jj .. 4jj+3 from the source rows (i-1, i, i+1) x columns (2jj-1 .. 2jj+2), all clamped by the caller.
// Columns first, then rows, as torch's kernel does.
SGR_HD void up_quad(const float (&v)[3][4], const UpTap (&tc)[4], UpTap ttop, UpTap tbot, float (&top)[4], float (&bot)[4]) {
  float h[3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    h[r][0] = up_lerp(tc[0], v[r][0], v[r][1]);
    h[r][1] = up_lerp(tc[1], v[r][1], v[r][2]);
    h[r][2] = up_lerp(tc[2], v[r][1], v[r][2]);
    h[r][3] = up_lerp(tc[3], v[r][2], v[r][3]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    top[k] = up_lerp(ttop, h[0][k], h[1][k]);
    bot[k] = up_lerp(tbot, h[1][k], h[2][k]);
  }
}
// The adjoint at the source pixels (i, 2jj) and (i, 2jj+1): g holds output rows 2i-1 .. 2i+2 x columns 4jj-1 .. 4jj+4 (0 outside the map),
// wr / wa / wb the up_adj_w weights of those rows, of columns 4jj-1 .. 4jj+2 for 2jj and of columns 4jj+1 .. 4jj+4 for 2jj+1.  A gather
// in a fixed order: columns, then rows.
SGR_HD void up_adjoint(const float (&g)[4][6], const float (&wr)[4], const float (&wa)[4], const float (&wb)[4], float& a, float& b) {
  a = 0.0f;
  b = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ha = fmaf(wa[3], g[r][3], fmaf(wa[2], g[r][2], fmaf(wa[1], g[r][1], wa[0] * g[r][0])));
    const float hb = fmaf(wb[3], g[r][5], fmaf(wb[2], g[r][4], fmaf(wb[1], g[r][3], wb[0] * g[r][2])));
    a = fmaf(wr[r], ha, a);
    b = fmaf(wr[r], hb, b);
  }
}

// ---- the resize to the skip's size (models.py:165-166 and its siblings, 185-186): F.interpolate(y, [ns_h, ns_w], mode='bilinear') with
// n <= ns <= 2 n on either axis.  The rule is src_index at scale = (float)n / (float)ns, formed in fp32 on the host and passed in.
// ORDER OF THE LERPS: a resized value is the lerp of its two COLUMN taps in either source row first, then the lerp of the two ROWS, as
// torch's kernel does, and is an fp32 number before the 2x stage reads it (the reference materialises the map).
struct RsTap { int i0, i1; float l0, l1; };
SGR_HD RsTap rs_tap(int o, float scale, int n) {
  RsTap t;
  src_index(o, scale, n, t.i0, t.i1, t.l0, t.l1);
  return t;
}
SGR_HD float rs_lerp(const RsTap& t, float a, float b) { return fmaf(t.l1, b, t.l0 * a); }
// y at (rows tr.i0, tr.i1) x (columns tc.i0, tc.i1) -> the resized value
SGR_HD float rs_value(float p00, float p01, float p10, float p11, const RsTap& tr, const RsTap& tc) {
  return rs_lerp(tr, rs_lerp(tc, p00, p01), rs_lerp(tc, p10, p11));
}
// The adjoint, gathered: source index src receives from the resized indices o whose taps name it.  With n <= ns <= 2 n those are at most
// four, and they lie in the window of kRsFan consecutive indices that starts at rs_adj_first (inv = (float)ns / (float)n; the window has
// one spare index on either side of the real-valued bound, so the rounding of the bound cannot lose one --
// tests/host_emul/gn_resize_emul.cpp checks that exhaustively).  An index of the window that does not name src, or lies outside the
// map, carries the weight 0.
constexpr int kRsFan = 6;
SGR_HD int rs_adj_first(int src, float inv) { return (int)floorf(((float)src - 0.5f) * inv - 0.5f); }
SGR_HD float rs_adj_w(int o, int src, float scale, int n, int ns) {
  if (o < 0 || o >= ns) return 0.0f;
  const RsTap t = rs_tap(o, scale, n);
  return (t.i0 == src ? t.l0 : 0.0f) + (t.i1 == src ? t.l1 : 0.0f);
}
SGR_HD void rs_adj_weights(int src, float scale, float inv, int n, int ns, int& first, float (&w)[kRsFan]) {
  first = rs_adj_first(src, inv);
#pragma unroll
  for (int k = 0; k < kRsFan; ++k) w[k] = rs_adj_w(first + k, src, scale, n, ns);
}
// a: the cotangent at the window's rows x columns (any finite number where the weight is 0).  A gather in a fixed order: columns, then rows.
SGR_HD float rs_adjoint(const float (&a)[kRsFan][kRsFan], const float (&wr)[kRsFan], const float (&wc)[kRsFan]) {
  float s = 0.0f;
#pragma unroll
  for (int r = 0; r < kRsFan; ++r) {
    float h = wc[0] * a[r][0];
#pragma unroll
    for (int k = 1; k < kRsFan; ++k) h = fmaf(wc[k], a[r][k], h);
    s = fmaf(wr[r], h, s);
  }
  return s;
}

}  // namespace sgr
