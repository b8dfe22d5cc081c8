// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// The several-source form of the encoders' convolution (sgr.encoder_conv_cat) on the host: the tile loops of
// encoder_conv_emul.cpp -- which this file includes, so both run behind the same software v_mfma_f32_16x16x4_f32 -- with the channels read
// through the header's source table (ec_source_of / ec_source_plane / ec_source_at of csrc/sgr_encoder_conv.h, the text the gfx950 kernels
// compile) and the data gradient run once per source over that source's channel range (channel base, total channel count), as
// sgr_encoder_conv_cat_bwd launches it.  emul_encoder_conv_cat_selfcheck compares them with the single-source emulation on the concatenated
// data, bit for bit, for the value, dW, db and every dx, over the splits and planes of tests/test_gpu_encoder_conv_cat.py, with every
// source in a layout of its own (contiguous, channels-last, a channel slice of a larger tensor, a padded row pitch).  With
// -DEC_CAT_EMUL_MAIN the file is a program that runs the self-check (for a sanitizer build).
#include <cstdio>
#include <cstring>

#include "encoder_conv_emul.cpp"

namespace {

struct CatArgs {
  int S;
  const float* const* xs;
  const int* channels;
  const long long* strides;
};

EcSources table_of(const CatArgs& a, int* total) {
  EcSources tab{};
  int first = 0;
  for (int i = 0; i < kEcMaxSources; ++i) {
    if (i < a.S) {
      tab.s[i] = EcSource{a.xs ? a.xs[i] : nullptr, a.strides ? a.strides[4 * i] : 0, a.strides ? a.strides[4 * i + 1] : 0, a.strides ? a.strides[4 * i + 2] : 0,
                          a.strides ? a.strides[4 * i + 3] : 0, first};
      first += a.channels[i];
    } else {
      tab.s[i] = EcSource{nullptr, 0, 0, 0, 0, kEcNoSource};
    }
  }
  *total = first;
  return tab;
}

// x[b, c, src(t_r), src(t_c)] of the concatenation, through the table
float cat_at(const EcSources& tab, int b, int c, int H, int W, int t_r, int t_c, int mode) {
  const EcSource s = ec_source_of(tab, c);
  return ec_source_at(s, ec_source_plane(s, b, c), ec_src(t_r, H, mode), ec_src(t_c, W, mode));
}

}  // namespace

extern "C" {

void emul_encoder_conv_cat_fwd(int S, const float* const* xs, const int* channels, const long long* strides, const float* Wt, const float* bias, float* out, int B,
                               int O, int H, int W, int mode) {
  int C = 0;
  const EcSources tab = table_of(CatArgs{S, xs, channels, strides}, &C);
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
          for (int c0 = 0; c0 < C; c0 += kEcKC) {      // the concatenation's chunks: a chunk may hold channels of two sources
            std::fill(at.begin(), at.end(), 0.0f);
            std::fill(wl.begin(), wl.end(), 0.0f);
            for (int cc = 0; cc < kEcKC && c0 + cc < C; ++cc)
              for (int r = 0; r < kEcRows; ++r)
                for (int tc = 0; tc < kEcCols; ++tc) at[ec_fwd_tile_idx(cc, r, tc)] = cat_at(tab, b, c0 + cc, H, W, 2 * i0 - 1 + r, 2 * j0 - 1 + tc, mode);
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

// one source's data gradient: dx [B, C, H, W] holds the channels cbase .. cbase + C - 1 of the Ct channels of Wt [O, Ct, 4, 4]
static void cat_dx_range(const float* g, const float* Wt, float* dx, int B, int C, int O, int H, int W, int mode, int cbase, int Ct) {
  const int Ho = ec_out(H), Wo = ec_out(W), HWo = Ho * Wo, groups = O / kEcDOC;
  const int tilesX = ((W + 1) / 2 + kEcDW - 1) / kEcDW, tilesY = ((H + 1) / 2 + kEcDH - 1) / kEcDH, passes = (C + kEcDPassC - 1) / kEcDPassC;
  std::vector<float> gt((size_t)kEcDOC * kEcDGPlane), wl((size_t)kEcDOC * 16 * kEcDCP);
  std::vector<float> run((size_t)4 * 2 * 2 * kEcDPassNT * 64 * 4);      // [wave][m][pw][n][lane][reg]
  auto R = [&](int wave, int m, int pw, int n, int l, int r) -> float& { return run[(((((size_t)wave * 2 + m) * 2 + pw) * kEcDPassNT + n) * 64 + l) * 4 + r]; };
  for (int b = 0; b < B; ++b)
    for (int ty = 0; ty < tilesY; ++ty)
      for (int tx = 0; tx < tilesX; ++tx)
        for (int pass = 0; pass < passes; ++pass) {      // the source's own passes of 64 channels: the chain of one dx runs over k alone
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
                for (int tap = 0; tap < 16; ++tap) wl[ec_dx_w_idx_of_tap(oc, tap >> 2, tap & 3, c)] = Wt[((size_t)o * Ct + cbase + c0p + c) * 16 + tap];
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
              dx[(((size_t)b * C + c) * H + h) * W + w] = ec_dx_border(g + (size_t)b * O * HWo, Wt, cbase + c, h, w, Ct, O, H, W);
}

// dxs[i] [B, channels[i], H, W] or NULL (not wanted); dWt [O, C, 4, 4] or NULL; dbias [O] or NULL
void emul_encoder_conv_cat_bwd(int S, const float* g, const float* const* xs, const int* channels, const long long* strides, const float* Wt, float* const* dxs,
                               float* dWt, float* dbias, int B, int O, int H, int W, int mode) {
  int C = 0;
  const EcSources tab = table_of(CatArgs{S, dWt ? xs : nullptr, channels, dWt ? strides : nullptr}, &C);
  const int Ho = ec_out(H), Wo = ec_out(W), HWo = Ho * Wo;
  for (int i = 0, cbase = 0; i < S; cbase += channels[i], ++i)
    if (dxs && dxs[i]) cat_dx_range(g, Wt, dxs[i], B, channels[i], O, H, W, mode, cbase, C);
  if (dWt) {      // the concatenation's blocks of 16 channels: a block may hold channels of several sources
    const int wtilesX = (Wo + kEcWW - 1) / kEcWW, wtiles = wtilesX * ((Ho + kEcWH - 1) / kEcWH), strips = (wtiles + kEcWStrip - 1) / kEcWStrip;
    const int opasses = (O + kEcPassO - 1) / kEcPassO;
    std::vector<double> dw((size_t)O * C * 16, 0.0);
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
                  for (int tc = 0; tc < kEcWCols; ++tc) xt[ec_w_x_idx(cc, r, tc)] = cat_at(tab, b, c0 + cc, H, W, 2 * i0 - 1 + r, 2 * j0 - 1 + tc, mode);
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
    for (size_t e = 0; e < dw.size(); ++e) dWt[e] = (float)dw[e];
  }
  if (dbias) {      // as encoder_conv_emul.cpp: the sources do not enter
    for (int o = 0; o < O; ++o) {
      double db = 0.0;
      for (int b = 0; b < B; ++b)
        for (long long s0 = 0; s0 < HWo; s0 += kEcBSlice)
          for (int th = 0; th < 256; ++th) {
            float gb = 0.0f;
            for (int r = 0; r < kEcBRounds; ++r)
              for (int u = 0; u < 4; ++u) {
                const long long p = s0 + 4 * ((long long)r * 256 + th) + u;
                if (p < HWo) gb += g[((size_t)b * O + o) * HWo + p];
              }
            db += (double)gb;
          }
      dbias[o] = (float)db;
    }
  }
}

// Every split of tests/test_gpu_encoder_conv_cat.py on two of its planes (every plane three times), both pad modes, B = 2 or 3; the
// output channels shrink as the channels and the plane grow (128, 48, 16) and the widest plane meets the narrow splits, to keep a software
// MFMA quick.
// Returns the number of arrays that differ from the single-source emulation on the concatenated data in any bit (0 = all equal);
// cases = how many ran.
int emul_encoder_conv_cat_selfcheck(int* cases) {
  const int nsplit = 9, splits[nsplit][5] = {{2, 1, 1}, {3, 3, 5, 1}, {2, 15, 2}, {2, 63, 2}, {3, 17, 47, 3}, {2, 64, 7}, {2, 64, 84}, {4, 1, 1, 1, 1}, {4, 40, 40, 40, 40}};
  const int planes[6][2] = {{2, 2}, {3, 3}, {5, 7}, {6, 10}, {17, 4}, {18, 70}};
  const int plane_of[nsplit][2] = {{0, 5}, {1, 5}, {2, 3}, {4, 0}, {3, 1}, {2, 4}, {3, 2}, {5, 4}, {0, 1}};
  unsigned seed = 2401u;
  auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 32768.0f - 1.0f; };
  int bad = 0, ran = 0;
  for (int si = 0; si < nsplit; ++si)
    for (int k = 0; k < 2; ++k) {
      const int pi = plane_of[si][k], S = splits[si][0], *ch = splits[si] + 1, H = planes[pi][0], W = planes[pi][1], mode = (si + k) % 2;
      int Cs = 0;
      for (int i = 0; i < S; ++i) Cs += ch[i];
      const int O = (Cs <= 9 && pi <= 1) ? 128 : (Cs <= 67 && pi != 5) ? 48 : 16, B = Cs > 100 ? 2 : 2 + (si + k) % 2;
      const int Ho = H / 2, Wo = W / 2;
      int C = 0;
      for (int i = 0; i < S; ++i) C += ch[i];
      std::vector<float> cat((size_t)B * C * H * W), Wt((size_t)O * C * 16), bias(O), ct((size_t)B * O * Ho * Wo);
      for (auto* v : {&cat, &Wt, &bias, &ct})
        for (float& f : *v) f = rnd();
      // every source in a layout of its own: 0 contiguous, 1 channels-last, 2 channels 1 .. C_i of a tensor with C_i + 2, 3 a row pitch of W + 3
      std::vector<std::vector<float>> store(S);
      const float* xs[kEcMaxSources] = {};
      long long strides[4 * kEcMaxSources] = {};
      for (int i = 0, first = 0; i < S; first += ch[i], ++i) {
        const int Ci = ch[i], kind = (i + si) % 4;
        long long sb, sc, sh, sw, off = 0;
        if (kind == 0) { sb = (long long)Ci * H * W; sc = (long long)H * W; sh = W; sw = 1; }
        else if (kind == 1) { sb = (long long)Ci * H * W; sc = 1; sh = (long long)W * Ci; sw = Ci; }
        else if (kind == 2) { sb = (long long)(Ci + 2) * H * W; sc = (long long)H * W; sh = W; sw = 1; off = sc; }
        else { sb = (long long)Ci * H * (W + 3); sc = (long long)H * (W + 3); sh = W + 3; sw = 1; }
        store[i].assign((size_t)B * sb, 7.0f);      // what is not a source element is never read
        for (int b = 0; b < B; ++b)
          for (int c = 0; c < Ci; ++c)
            for (int h = 0; h < H; ++h)
              for (int w = 0; w < W; ++w) store[i][off + b * sb + c * sc + h * sh + w * sw] = cat[(((size_t)b * C + first + c) * H + h) * W + w];
        xs[i] = store[i].data() + off;
        const long long st[4] = {sb, sc, sh, sw};
        std::memcpy(strides + 4 * i, st, sizeof st);
      }
      std::vector<float> out0(ct.size()), out1(ct.size(), -3.0f), dx0(cat.size()), dW0(Wt.size()), dW1(Wt.size(), -3.0f), db0(O), db1(O, -3.0f);
      emul_encoder_conv_fwd(cat.data(), Wt.data(), bias.data(), out0.data(), B, C, O, H, W, mode);
      emul_encoder_conv_bwd(ct.data(), cat.data(), Wt.data(), dx0.data(), dW0.data(), db0.data(), B, C, O, H, W, mode);
      emul_encoder_conv_cat_fwd(S, xs, ch, strides, Wt.data(), bias.data(), out1.data(), B, O, H, W, mode);
      std::vector<std::vector<float>> dxs(S);
      float* dxp[kEcMaxSources] = {};
      for (int i = 0; i < S; ++i) {
        if (S > 1 && i == (si % S) && pi % 2) continue;      // a source that wants no gradient: the others' bits do not move
        dxs[i].assign((size_t)B * ch[i] * H * W, -3.0f);
        dxp[i] = dxs[i].data();
      }
      emul_encoder_conv_cat_bwd(S, ct.data(), xs, ch, strides, Wt.data(), dxp, dW1.data(), db1.data(), B, O, H, W, mode);
      bad += std::memcmp(out0.data(), out1.data(), out0.size() * sizeof(float)) != 0;
      bad += std::memcmp(dW0.data(), dW1.data(), dW0.size() * sizeof(float)) != 0;
      bad += std::memcmp(db0.data(), db1.data(), db0.size() * sizeof(float)) != 0;
      for (int i = 0, first = 0; i < S; first += ch[i], ++i) {
        if (!dxp[i]) continue;
        for (int b = 0; b < B; ++b)
          bad += std::memcmp(dx0.data() + ((size_t)b * C + first) * H * W, dxs[i].data() + (size_t)b * ch[i] * H * W, (size_t)ch[i] * H * W * sizeof(float)) != 0;
      }
      ++ran;
    }
  if (cases) *cases = ran;
  return bad;
}

}  // extern "C"

#ifdef EC_CAT_EMUL_MAIN
int main() {
  int cases = 0;
  const int bad = emul_encoder_conv_cat_selfcheck(&cases);
  std::printf("encoder_conv_cat_emul: %d cases, %d arrays differ\n", cases, bad);
  return bad == 0 && cases == 18 ? 0 : 1;
}
#endif
