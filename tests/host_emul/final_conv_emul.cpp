// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// Compiles the index rule and the accumulation orders of the final pad + 3x3 convolution (inverserenderingofindoorscene_amd/csrc/
// sgr_final_conv.h, the expressions the gfx950 kernels of sgr_final_conv.hip evaluate) for the host and runs them serially, output by output,
// in the stated order.  The GroupNorm prologue is sgr_gn_stage.h's.  The weight gradient's workgroup and double folds run in index order
// here (fp32 per strip of 32 pixels, as a thread's, then double) and as trees on the device.  tests/test_final_conv.py holds this to half
// the GPU tests' bounds on the fixtures, so the numerics are vetted where there is no GPU; strides, tiles, vector paths and launch plumbing
// are the GPU tests'.
#include <cstddef>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_final_conv.h"
#include "../../inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h"

using namespace sgr;

extern "C" {

// mismatches of fc_pairs against the definition of R_n(h), over every h of an axis of n: a wrong count, a pair outside the set, a pair twice
int emul_fc_pairs_mismatch(int n) {
  int bad = 0;
  for (int h = 0; h < n; ++h) {
    const FcPairs p = fc_pairs(h, n);
    int members = 0;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) members += fc_cl(i + k - 1, n) == h;
    bad += members != 3;
    for (int m = 0; m < 3; ++m) {
      bad += !(p.i[m] >= 0 && p.i[m] < n && p.k[m] >= 0 && p.k[m] < 3 && fc_cl(p.i[m] + p.k[m] - 1, n) == h);
      for (int q = 0; q < m; ++q) bad += p.i[m] == p.i[q] && p.k[m] == p.k[q];
    }
  }
  return bad;
}

// stats [B,G,4] from x (double sums in index order), as sgr_gn_moments
void emul_gn_moments(const float* x, float* stats, int B, int C, int G, int H, int W, float eps) {
  const int cpg = C / G, HW = H * W;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double s = 0.0, ss = 0.0;
      const float* xg = x + ((size_t)b * C + (size_t)g * cpg) * HW;
      for (size_t e = 0; e < (size_t)cpg * HW; ++e) { s += (double)xg[e]; ss += (double)xg[e] * (double)xg[e]; }
      float* st = stats + 4 * ((size_t)b * G + g);
      gn_finish(s, ss, (double)cpg * HW, eps, st[0], st[1], st[2], st[3]);
    }
}

// y [B,C,H,W]: x itself (stats == nullptr) or relu(gn(x)) by the prologue's two functions
static void prologue(const float* x, const float* gnw, const float* gnb, const float* stats, std::vector<float>& y, int B, int C, int G, int H, int W) {
  const int HW = H * W;
  y.assign(x, x + (size_t)B * C * HW);
  if (!stats) return;
  const int cpg = C / G;
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c) {
      const float* st = stats + 4 * ((size_t)b * G + c / cpg);
      float* p = y.data() + ((size_t)b * C + c) * HW;
      for (int e = 0; e < HW; ++e) p[e] = fmaxf(gn_pre(gn_xhat(p[e], st[0], st[1], st[2]), gnw[c], gnb[c]), 0.0f);
    }
}

static void window(const float* plane, int i, int j, int H, int W, float (&v)[9]) {
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw) v[3 * kh + kw] = plane[(size_t)fc_cl(i + kh - 1, H) * W + fc_cl(j + kw - 1, W)];
}

void emul_final_conv_fwd(const float* x, const float* Wt, const float* bias, const float* gnw, const float* gnb, const float* stats, float* out, int B, int C, int G,
                         int H, int W) {
  std::vector<float> y;
  prologue(x, gnw, gnb, stats, y, B, C, G, H, W);
  const int HW = H * W;
  for (int b = 0; b < B; ++b)
    for (int o = 0; o < 3; ++o)
      for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
          float acc = 0.0f;
          for (int c = 0; c < C; ++c) {
            float v[9];
            window(y.data() + ((size_t)b * C + c) * HW, i, j, H, W, v);
            acc += fc_taps(Wt + ((size_t)o * C + c) * 9, v);
          }
          out[(((size_t)b * 3 + o) * H + i) * W + j] = acc + bias[o];
        }
}

// dy [B,C,H,W] (the gradient at y: unmasked with a prologue), dWt [3,C,3,3], dbias [3]
void emul_final_conv_bwd(const float* g, const float* x, const float* Wt, const float* gnw, const float* gnb, const float* stats, float* dy, float* dWt, float* dbias,
                         int B, int C, int G, int H, int W) {
  std::vector<float> y;
  prologue(x, gnw, gnb, stats, y, B, C, G, H, W);
  const int HW = H * W;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const FcPairs rows = fc_pairs(h, H), cols = fc_pairs(w, W);
        float Gt[3][9];
        for (int o = 0; o < 3; ++o) {
          float gv[3][3];
          for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) gv[p][q] = g[(((size_t)b * 3 + o) * H + rows.i[p]) * W + cols.i[q]];
          fc_gather_taps(gv, rows, cols, Gt[o]);
        }
        for (int c = 0; c < C; ++c) {
          float wc[27];
          for (int o = 0; o < 3; ++o)
            for (int k = 0; k < 9; ++k) wc[9 * o + k] = Wt[((size_t)o * C + c) * 9 + k];
          dy[(((size_t)b * C + c) * H + h) * W + w] = fc_dy(wc, Gt);
        }
      }
  // weights: fp32 over strips of 32 pixels in raster order (a thread's share), the strips in double
  std::vector<double> dw((size_t)27 * C, 0.0);
  double db[3] = {0.0, 0.0, 0.0};
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c) {
      const float* plane = y.data() + ((size_t)b * C + c) * HW;
      for (int p0 = 0; p0 < HW; p0 += 32) {
        float acc[27] = {0.0f};
        float gb[3] = {0.0f, 0.0f, 0.0f};
        for (int p = p0; p < HW && p < p0 + 32; ++p) {
          const int i = p / W, j = p - i * W;
          float v[9];
          window(plane, i, j, H, W, v);
          const float g3[3] = {g[((size_t)b * 3 + 0) * HW + p], g[((size_t)b * 3 + 1) * HW + p], g[((size_t)b * 3 + 2) * HW + p]};
          fc_dw_pixel(g3, v, acc);
          for (int o = 0; o < 3; ++o) gb[o] += g3[o];
        }
        for (int k = 0; k < 27; ++k) dw[(size_t)c * 27 + k] += (double)acc[k];
        if (c == 0)
          for (int o = 0; o < 3; ++o) db[o] += (double)gb[o];
      }
    }
  for (int o = 0; o < 3; ++o) {
    dbias[o] = (float)db[o];
    for (int c = 0; c < C; ++c)
      for (int k = 0; k < 9; ++k) dWt[((size_t)o * C + c) * 9 + k] = (float)dw[(size_t)c * 27 + 9 * o + k];
  }
}

}  // extern "C"
