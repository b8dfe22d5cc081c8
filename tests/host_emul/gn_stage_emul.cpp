// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// Compiles the per-element arithmetic of the CNN stage glue (inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h, the expressions the
// gfx950 kernels of sgr_gn_stage.hip evaluate) for the host and drives it with serial loops that mirror the kernels' thread mapping: a
// position (i, jj) makes output rows 2i, 2i+1 x columns 4jj .. 4jj+3 forward and gathers the source pixels (i, 2jj), (i, 2jj+1) backward.
// The double-precision sums run in index order here and as a tree on the device.  tests/test_gn_stage.py holds this to the GPU tests'
// bounds on the fixtures, so the numerics are vetted where there is no GPU; strides, vector paths and launch plumbing are the GPU tests'.
#include <cstddef>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h"

using namespace sgr;

namespace {
inline int lo(int a) { return a > 0 ? a : 0; }
inline int hi(int a, int n) { return a < n ? a : n - 1; }
}  // namespace

extern "C" {

// contiguous tensors; skip == nullptr (Cs == 0): the plain form
void emul_gn_stage_fwd(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, int B, int C, int G, int Cs, int H,
                       int W, float eps) {
  const int cpg = C / G, HW = H * W, W2 = (W + 1) / 2, OW = 2 * W;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double s = 0.0, ss = 0.0;
      const float* xg = x + ((size_t)b * C + (size_t)g * cpg) * HW;
      for (size_t e = 0; e < (size_t)cpg * HW; ++e) { s += (double)xg[e]; ss += (double)xg[e] * (double)xg[e]; }
      float* st = stats + 4 * ((size_t)b * G + g);
      gn_finish(s, ss, (double)cpg * HW, eps, st[0], st[1], st[2], st[3]);
    }
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < C + Cs; ++ch) {
      const bool norm = ch < C;
      const float* st = stats + 4 * ((size_t)b * G + (norm ? ch / cpg : 0));
      const float mh = st[0], ml = st[1], rstd = st[2], wc = norm ? weight[ch] : 1.0f, bc = norm ? bias[ch] : 0.0f;
      const float* src = norm ? x + ((size_t)b * C + ch) * HW : skip + ((size_t)b * Cs + (ch - C)) * HW;
      auto val = [&](int r, int c) {
        const float t = src[(size_t)r * W + c];
        return norm ? fmaxf(gn_pre(gn_xhat(t, mh, ml, rstd), wc, bc), 0.0f) : t;
      };
      if (!skip) {
        float* y = out + ((size_t)b * C + ch) * HW;
        for (int p = 0; p < HW; ++p) y[p] = val(p / W, p % W);
        continue;
      }
      float* op = out + ((size_t)b * (C + Cs) + ch) * 4 * HW;
      for (int i = 0; i < H; ++i)
        for (int jj = 0; jj < W2; ++jj) {
          const int c0 = 2 * jj;
          const int rows[3] = {lo(i - 1), i, hi(i + 1, H)}, cols[4] = {lo(c0 - 1), c0, hi(c0 + 1, W), hi(c0 + 2, W)};
          float v[3][4], top[4], bot[4];
          for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 4; ++k) v[a][k] = val(rows[a], cols[k]);
          const UpTap tc[4] = {up_tap(4 * jj, W), up_tap(4 * jj + 1, W), up_tap(4 * jj + 2, W), up_tap(4 * jj + 3, W)};
          up_quad(v, tc, up_tap(2 * i, H), up_tap(2 * i + 1, H), top, bot);
          for (int k = 0; k < 4; ++k)
            if (4 * jj + k < OW) {
              op[(size_t)(2 * i) * OW + 4 * jj + k] = top[k];
              op[(size_t)(2 * i + 1) * OW + 4 * jj + k] = bot[k];
            }
        }
    }
}

// the weights the kernels pick per thread (up_pick, up_adj_pick) against the rule evaluated at every position of an axis of n: mismatches
int emul_up_picks_mismatch(int n) {
  int bad = 0;
  const UpTaps taps = up_taps();
  float low[4], mid[4], high[4];
  up_adj_sets(n, low, mid, high);
  for (int o = 0; o < 2 * n; ++o) {
    const UpTap a = up_tap(o, n), b = up_pick(taps, o);
    bad += !(a.l0 == b.l0 && a.l1 == b.l1);
  }
  for (int src = 0; src < n; ++src) {
    float w[4];
    up_adj_pick(low, mid, high, src, n, w);
    for (int k = 0; k < 4; ++k) bad += !(w[k] == up_adj_w(2 * src - 1 + k, src, n));
  }
  return bad;
}

// every gradient; dskip is ignored when Cs == 0
void emul_gn_stage_bwd(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight, float* dbias,
                       float* dskip, int B, int C, int G, int Cs, int H, int W) {
  const bool up = Cs > 0;
  const int cpg = C / G, HW = H * W, W2 = (W + 1) / 2, OW = up ? 2 * W : W, OH = up ? 2 * H : H;
  std::vector<float> dy((size_t)B * C * HW);
  std::vector<double> s1((size_t)B * C, 0.0), s2((size_t)B * C, 0.0);
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < C + Cs; ++ch) {
      const bool norm = ch < C;
      const float* st = stats + 4 * ((size_t)b * G + (norm ? ch / cpg : 0));
      const float mh = st[0], ml = st[1], rstd = st[2];
      const float* gp = g + ((size_t)b * (C + Cs) + ch) * OH * OW;
      float* dst = norm ? dy.data() + ((size_t)b * C + ch) * HW : dskip + ((size_t)b * Cs + (ch - C)) * HW;
      for (int i = 0; i < H; ++i)
        for (int jj = 0; jj < W2; ++jj) {
          const int c0 = 2 * jj;
          const bool two = c0 + 1 < W;
          float a0, a1;
          if (up) {
            float gv[4][6], wr[4], wa[4], wb[4];
            for (int k = 0; k < 4; ++k) {
              wr[k] = up_adj_w(2 * i - 1 + k, i, H);
              wa[k] = up_adj_w(4 * jj - 1 + k, c0, W);
              wb[k] = two ? up_adj_w(4 * jj + 1 + k, c0 + 1, W) : 0.0f;
              const int orow = 2 * i - 1 + k;
              for (int u = 0; u < 6; ++u) {
                const int oc = 4 * jj - 1 + u;
                gv[k][u] = orow >= 0 && orow < OH && oc >= 0 && oc < OW ? gp[(size_t)orow * OW + oc] : 0.0f;
              }
            }
            up_adjoint(gv, wr, wa, wb, a0, a1);
          } else {
            a0 = gp[(size_t)i * W + c0];
            a1 = two ? gp[(size_t)i * W + c0 + 1] : 0.0f;
          }
          if (norm) {
            const float* xp = x + ((size_t)b * C + ch) * HW;
            const float h0 = gn_xhat(xp[(size_t)i * W + c0], mh, ml, rstd), h1 = two ? gn_xhat(xp[(size_t)i * W + c0 + 1], mh, ml, rstd) : 0.0f;
            a0 = gn_pre(h0, weight[ch], bias[ch]) > 0.0f ? a0 : 0.0f;
            a1 = two && gn_pre(h1, weight[ch], bias[ch]) > 0.0f ? a1 : 0.0f;
            s1[(size_t)b * C + ch] += (double)a0 + (double)a1;
            s2[(size_t)b * C + ch] += (double)a0 * (double)h0 + (double)a1 * (double)h1;
          }
          dst[(size_t)i * W + c0] = a0;
          if (two) dst[(size_t)i * W + c0 + 1] = a1;
        }
    }
  for (int c = 0; c < C; ++c) {
    double a = 0.0, q = 0.0;
    for (int b = 0; b < B; ++b) { a += s1[(size_t)b * C + c]; q += s2[(size_t)b * C + c]; }
    dbias[c] = (float)a;
    dweight[c] = (float)q;
  }
  for (int b = 0; b < B; ++b)
    for (int gi = 0; gi < G; ++gi) {
      double a = 0.0, q = 0.0;
      for (int c = gi * cpg; c < (gi + 1) * cpg; ++c) { a += (double)weight[c] * s1[(size_t)b * C + c]; q += (double)weight[c] * s2[(size_t)b * C + c]; }
      const double n = (double)cpg * HW;
      const float c1 = (float)(a / n), c2 = (float)(q / n);
      const float* st = stats + 4 * ((size_t)b * G + gi);
      for (int c = gi * cpg; c < (gi + 1) * cpg; ++c)
        for (int p = 0; p < HW; ++p) {
          const size_t o = ((size_t)b * C + c) * HW + p;
          dx[o] = gn_dx(dy[o], gn_xhat(x[o], st[0], st[1], st[2]), weight[c], st[2], c1, c2);
        }
    }
}

}  // extern "C"
