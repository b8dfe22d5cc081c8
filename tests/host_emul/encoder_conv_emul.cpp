// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// Compiles the index rule, the tile loops' addresses, the K orderings and the accumulation orders of the encoders' pad + 4x4 stride-2
// convolution (inverserenderingofindoorscene_amd/csrc/sgr_encoder_conv.h, the functions the gfx950 kernels of sgr_encoder_conv.hip call)
// for the host and runs the kernels' tile loops serially: workgroup by workgroup, wave by wave, with the LDS tiles as arrays and the
// software v_mfma_f32_16x16x4_f32 of light_final_conv_emul.cpp -- 64 lanes' a, b and four accumulator registers, placed by the header's
// maps, the fmaf chain in k order.  The weight gradient's strip partials are added in double in index order, as on the device; the bias
// gradient runs in fp32 per thread's share of a slice, then double in index order, where the device adds the threads of a workgroup as a
// tree.  tests/test_encoder_conv.py holds this to half the GPU tests' bounds on the fixtures, so the numerics are vetted where there is no
// GPU; strides, vector paths and launch plumbing are the GPU tests'.  With -DEC_EMUL_MAIN the file is a program that runs the fixtures'
// shapes (for a sanitizer build).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_encoder_conv.h"

using namespace sgr;

namespace {

// which lane holds A[i][k] and which B[k][j], found from the header's maps
struct LaneTables {
  int a[16][4], b[4][16];
  LaneTables() {
    for (int l = 0; l < 64; ++l) {
      a[lf_a_row(l)][lf_a_k(l)] = l;
      b[lf_b_k(l)][lf_b_col(l)] = l;
    }
  }
};
const LaneTables kLanes;

// d[l][r] = D[lf_d_row(l, r)][lf_d_col(l)]: the chain fmaf(A[i][k], B[k][j], .) for k = 0, 1, 2, 3 starting from C
void soft_mfma(const float (&a)[64], const float (&b)[64], float (&d)[64][4]) {
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) {
      const int i = lf_d_row(l, r), j = lf_d_col(l);
      float t = d[l][r];
      for (int k = 0; k < 4; ++k) t = fmaf(a[kLanes.a[i][k]], b[kLanes.b[k][j]], t);
      d[l][r] = t;
    }
}

float x_at(const float* x, int b, int c, int C, int H, int W, int t_r, int t_c, int mode) {
  const int sr = ec_src(t_r, H, mode), sc = ec_src(t_c, W, mode);
  return sr < 0 || sc < 0 ? 0.0f : x[(((size_t)b * C + c) * H + sr) * W + sc];
}

}  // namespace

extern "C" {

// the header's R_n(h) as (i, k, i, k); i = -1: a slot without a member
void emul_encoder_conv_pairs(int h, int n, int mode, int* out) {
  const EcPairs p = ec_pairs(h, n, mode);
  for (int s = 0; s < 2; ++s) {
    out[2 * s] = p.i[s];
    out[2 * s + 1] = p.k[s];
  }
}

void emul_encoder_conv_fwd(const float* x, const float* Wt, const float* bias, float* out, int B, int C, int O, int H, int W, int mode) {
  const int Ho = ec_out(H), Wo = ec_out(W);
  const int tilesX = (Wo + kEcTW - 1) / kEcTW, tilesY = (Ho + kEcTH - 1) / kEcTH, passes = (O + kEcPassO - 1) / kEcPassO;
  std::vector<float> at((size_t)kEcKC * kEcCHP), wl((size_t)16 * kEcKC * kEcWP);
  std::vector<float> run((size_t)4 * 4 * kEcPassNT * 64 * 4);      // [wave][m][n][lane][reg]
  auto R = [&](int wave, int m, int n, int l, int r) -> float& { return run[((((size_t)wave * 4 + m) * kEcPassNT + n) * 64 + l) * 4 + r]; };
  for (int b = 0; b < B; ++b)
    for (int ty = 0; ty < tilesY; ++ty)
      for (int tx = 0; tx < tilesX; ++tx)
        for (int pass = 0; pass < passes; ++pass) {
          const int j0 = tx * kEcTW, i0 = ty * kEcTH, o0 = pass * kEcPassO, nnt = std::min(kEcPassNT, (O - o0) / 16);
          std::fill(run.begin(), run.end(), 0.0f);
          for (int c0 = 0; c0 < C; c0 += kEcKC) {
            std::fill(at.begin(), at.end(), 0.0f);
            std::fill(wl.begin(), wl.end(), 0.0f);
            for (int cc = 0; cc < kEcKC && c0 + cc < C; ++cc)
              for (int r = 0; r < kEcRows; ++r)
                for (int tc = 0; tc < kEcCols; ++tc) at[ec_fwd_tile_idx(cc, r, tc)] = x_at(x, b, c0 + cc, C, H, W, 2 * i0 - 1 + r, 2 * j0 - 1 + tc, mode);
            for (int q = 0; q < 16 * kEcKC; ++q)
              for (int o = 0; o < 16 * nnt; ++o)
                if (c0 + (q >> 4) < C) wl[ec_fwd_w_idx(q, o)] = Wt[((size_t)(o0 + o) * C + c0) * 16 + q];
            for (int wave = 0; wave < 4; ++wave)
              for (int m = 0; m < 4; ++m)
                for (int n = 0; n < nnt; ++n) {
                  float acc[64][4] = {};
                  for (int s = 0; s < kEcSteps; ++s) {
                    float a[64], bv[64];
                    for (int l = 0; l < 64; ++l) {
                      a[l] = at[ec_fwd_a_addr(l, s, wave, m)];
                      bv[l] = wl[ec_fwd_b_addr(l, s, n)];
                    }
                    soft_mfma(a, bv, acc);
                  }
                  for (int l = 0; l < 64; ++l)
                    for (int r = 0; r < 4; ++r) R(wave, m, n, l, r) += acc[l][r];
                }
          }
          for (int wave = 0; wave < 4; ++wave)
            for (int m = 0; m < 4; ++m)
              for (int n = 0; n < nnt; ++n)
                for (int l = 0; l < 64; ++l)
                  for (int r = 0; r < 4; ++r) {
                    const int o = o0 + 16 * n + lf_d_col(l), gy = i0 + ec_fwd_tile_row(wave, m), gx = j0 + ec_fwd_tile_col(m) + lf_d_row(l, r);
                    if (gy < Ho && gx < Wo) out[(((size_t)b * O + o) * Ho + gy) * Wo + gx] = R(wave, m, n, l, r) + bias[o];
                  }
        }
}

// dx [B,C,H,W], dWt [O,C,4,4], dbias [O]
void emul_encoder_conv_bwd(const float* g, const float* x, const float* Wt, float* dx, float* dWt, float* dbias, int B, int C, int O, int H, int W, int mode) {
  const int Ho = ec_out(H), Wo = ec_out(W), HWo = Ho * Wo, groups = O / kEcDOC;
  {
    const int tilesX = ((W + 1) / 2 + kEcDW - 1) / kEcDW, tilesY = ((H + 1) / 2 + kEcDH - 1) / kEcDH, passes = (C + kEcDPassC - 1) / kEcDPassC;
    std::vector<float> gt((size_t)kEcDOC * kEcDGPlane), wl((size_t)kEcDOC * 16 * kEcDCP);
    std::vector<float> run((size_t)4 * 2 * 2 * kEcDPassNT * 64 * 4);      // [wave][m][pw][n][lane][reg]
    auto R = [&](int wave, int m, int pw, int n, int l, int r) -> float& { return run[(((((size_t)wave * 2 + m) * 2 + pw) * kEcDPassNT + n) * 64 + l) * 4 + r]; };
    for (int b = 0; b < B; ++b)
      for (int ty = 0; ty < tilesY; ++ty)
        for (int tx = 0; tx < tilesX; ++tx)
          for (int pass = 0; pass < passes; ++pass) {
            const int b0 = tx * kEcDW, a0 = ty * kEcDH, c0p = pass * kEcDPassC, ncp = std::min(kEcDPassC, C - c0p), nnt = (ncp + 15) / 16;
            std::fill(run.begin(), run.end(), 0.0f);
            for (int jg = 0; jg < groups; ++jg) {
              std::fill(gt.begin(), gt.end(), 0.0f);
              std::fill(wl.begin(), wl.end(), 0.0f);
              for (int oc = 0; oc < kEcDOC; ++oc) {
                const int o = kEcDOC * jg + oc;
                for (int r = 0; r < kEcDGRows; ++r)
                  for (int col = 0; col < kEcDGCols; ++col) {
                    const int i = a0 - 1 + r, j = b0 - 1 + col;
                    if (i >= 0 && i < Ho && j >= 0 && j < Wo) gt[ec_dx_g_idx(oc, r, col)] = g[((size_t)b * O + o) * HWo + (size_t)i * Wo + j];
                  }
                for (int c = 0; c < ncp; ++c)
                  for (int tap = 0; tap < 16; ++tap) wl[ec_dx_w_idx_of_tap(oc, tap >> 2, tap & 3, c)] = Wt[((size_t)o * C + c0p + c) * 16 + tap];
              }
              for (int wave = 0; wave < 4; ++wave)
                for (int m = 0; m < 2; ++m)
                  for (int pw = 0; pw < 2; ++pw)
                    for (int n = 0; n < nnt; ++n) {
                      const int ph = wave & 1, m0 = 2 * (wave >> 1);
                      float acc[64][4] = {};
                      for (int oc = 0; oc < kEcDOC; ++oc) {
                        float a[64], bv[64];
                        for (int l = 0; l < 64; ++l) {
                          a[l] = gt[ec_dx_a_addr(l, oc, ph, pw, m0 + m)];
                          bv[l] = wl[ec_dx_b_addr(l, oc, ph, pw, n)];
                        }
                        soft_mfma(a, bv, acc);
                      }
                      for (int l = 0; l < 64; ++l)
                        for (int r = 0; r < 4; ++r) R(wave, m, pw, n, l, r) += acc[l][r];
                    }
            }
            for (int wave = 0; wave < 4; ++wave)
              for (int m = 0; m < 2; ++m)
                for (int pw = 0; pw < 2; ++pw)
                  for (int n = 0; n < nnt; ++n)
                    for (int l = 0; l < 64; ++l)
                      for (int r = 0; r < 4; ++r) {
                        const int ph = wave & 1, m0 = 2 * (wave >> 1), cl = 16 * n + lf_d_col(l);
                        const int h = 2 * (a0 + m0 + m) + ph, w = 2 * (b0 + lf_d_row(l, r)) + pw;
                        if (cl < ncp && h < H && w < W) dx[(((size_t)b * C + c0p + cl) * H + h) * W + w] = R(wave, m, pw, n, l, r);
                      }
          }
    if (mode == kEcReplicate)
      for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
          for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w)
              if (h == 0 || h == H - 1 || w == 0 || w == W - 1)
                dx[(((size_t)b * C + c) * H + h) * W + w] = ec_dx_border(g + (size_t)b * O * HWo, Wt, c, h, w, C, O, H, W);
  }
  // weights: the strips' fp32 partials by the kernel's tile loop, then double in index order (b, then strip)
  const int wtilesX = (Wo + kEcWW - 1) / kEcWW, wtiles = wtilesX * ((Ho + kEcWH - 1) / kEcWH), strips = (wtiles + kEcWStrip - 1) / kEcWStrip;
  const int opasses = (O + kEcPassO - 1) / kEcPassO;
  std::vector<double> dw((size_t)O * C * 16, 0.0), db((size_t)O, 0.0);
  std::vector<float> xt((size_t)kEcWCB * kEcWCHP), gtl((size_t)kEcPassO * kEcWGP);
  for (int b = 0; b < B; ++b)
    for (int strip = 0; strip < strips; ++strip)
      for (int c0 = 0; c0 < C; c0 += kEcWCB)
        for (int opass = 0; opass < opasses; ++opass) {
          const int ncb = std::min(kEcWCB, C - c0), o0 = opass * kEcPassO, nnt = std::min(kEcPassNT, (O - o0) / 16);
          std::vector<float> run((size_t)kEcWCB * kEcPassNT * 64 * 4, 0.0f);      // [cc][n][lane][reg]
          for (int t = strip * kEcWStrip; t < std::min((strip + 1) * kEcWStrip, wtiles); ++t) {
            const int tyi = t / wtilesX, j0 = (t - tyi * wtilesX) * kEcWW, i0 = tyi * kEcWH;
            std::fill(xt.begin(), xt.end(), 0.0f);
            std::fill(gtl.begin(), gtl.end(), 0.0f);
            for (int cc = 0; cc < ncb; ++cc)
              for (int r = 0; r < kEcWRows; ++r)
                for (int tc = 0; tc < kEcWCols; ++tc) xt[ec_w_x_idx(cc, r, tc)] = x_at(x, b, c0 + cc, C, H, W, 2 * i0 - 1 + r, 2 * j0 - 1 + tc, mode);
            for (int o = 0; o < 16 * nnt; ++o)
              for (int p = 0; p < 64; ++p) {
                const int gy = i0 + (p >> 4), gx = j0 + (p & 15);
                if (gy < Ho && gx < Wo) gtl[ec_w_g_idx(o, p)] = g[((size_t)b * O + o0 + o) * HWo + (size_t)gy * Wo + gx];
              }
            for (int cc = 0; cc < ncb; ++cc)
              for (int n = 0; n < nnt; ++n) {
                float acc[64][4] = {};
                for (int s = 0; s < 16; ++s) {
                  float a[64], bv[64];
                  for (int l = 0; l < 64; ++l) {
                    a[l] = xt[ec_w_a_addr(l, s, cc)];
                    bv[l] = gtl[ec_w_b_addr(l, s, n)];
                  }
                  soft_mfma(a, bv, acc);
                }
                for (int l = 0; l < 64; ++l)
                  for (int r = 0; r < 4; ++r) run[(((size_t)cc * kEcPassNT + n) * 64 + l) * 4 + r] += acc[l][r];
              }
          }
          for (int cc = 0; cc < ncb; ++cc)
            for (int n = 0; n < nnt; ++n)
              for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r)
                  dw[((size_t)(o0 + 16 * n + lf_d_col(l)) * C + c0 + cc) * 16 + lf_d_row(l, r)] += (double)run[(((size_t)cc * kEcPassNT + n) * 64 + l) * 4 + r];
        }
  // bias: fp32 over a thread's share of a slice (8 runs of 4 pixels, 1024 pixels apart), the shares in double
  for (int b = 0; b < B; ++b)
    for (int o = 0; o < O; ++o)
      for (long long s0 = 0; s0 < HWo; s0 += kEcBSlice)
        for (int th = 0; th < 256; ++th) {
          float gb = 0.0f;
          for (int r = 0; r < kEcBRounds; ++r)
            for (int u = 0; u < 4; ++u) {
              const long long p = s0 + 4 * ((long long)r * 256 + th) + u;
              if (p < HWo) gb += g[((size_t)b * O + o) * HWo + p];
            }
          db[o] += (double)gb;
        }
  for (size_t e = 0; e < dw.size(); ++e) dWt[e] = (float)dw[e];
  for (int o = 0; o < O; ++o) dbias[o] = (float)db[o];
}

}  // extern "C"

#ifdef EC_EMUL_MAIN
#include <cstdio>
// the fixtures' shapes (and two that take several tiles, passes and strips) on pseudo-random data: a run for a sanitizer build
int main() {
  const int shapes[][6] = {{2, 3, 64, 6, 10, 0}, {3, 17, 64, 5, 7, 0}, {2, 11, 32, 9, 13, 0}, {1, 11, 32, 2, 2, 0}, {1, 11, 32, 3, 3, 0}, {1, 3, 64, 2, 9, 0},
                           {1, 3, 64, 7, 2, 0}, {2, 32, 64, 5, 8, 1}, {1, 32, 64, 3, 3, 1}, {1, 70, 128, 19, 70, 0}, {1, 5, 16, 17, 133, 1}};
  unsigned seed = 12345u;
  auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 32768.0f - 1.0f; };
  double sum = 0.0;
  for (const auto& s : shapes) {
    const int B = s[0], C = s[1], O = s[2], H = s[3], W = s[4], mode = s[5], Ho = H / 2, Wo = W / 2;
    std::vector<float> x((size_t)B * C * H * W), Wt((size_t)O * C * 16), bias(O), ct((size_t)B * O * Ho * Wo), out(ct.size()), dx(x.size()), dW(Wt.size()), db(O);
    for (auto* v : {&x, &Wt, &bias, &ct})
      for (float& f : *v) f = rnd();
    emul_encoder_conv_fwd(x.data(), Wt.data(), bias.data(), out.data(), B, C, O, H, W, mode);
    emul_encoder_conv_bwd(ct.data(), x.data(), Wt.data(), dx.data(), dW.data(), db.data(), B, C, O, H, W, mode);
    for (auto* v : {&out, &dx, &dW, &db})
      for (float f : *v) sum += f;
  }
  std::printf("encoder_conv_emul: %zu shapes, checksum %.6f\n", sizeof(shapes) / sizeof(shapes[0]), sum);
  return std::isfinite(sum) ? 0 : 1;
}
#endif
