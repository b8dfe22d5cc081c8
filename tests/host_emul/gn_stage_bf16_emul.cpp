// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// The bf16 side of the CNN stage glue on the host: the conversions of
// inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h (bf16_up, bf16_round -- the text the gfx950 kernels compile) over every pattern,
// and the stage's per-element arithmetic with the kernels' loads and stores in their places: x, skip, the cotangent, the result, dx and
// dskip are of the I/O type T (gn_in on every load, gn_out<T> on every store), the statistics, pass 1's masked adjoint `dy`, dweight and
// dbias are fp32.  The serial loops are those of gn_stage_emul.cpp (same thread mapping, sums in index order), so with T = float this
// file computes what that one does, and tests/test_gn_stage_bf16.py holds T = bf16 to it: its result on the upcast input, rounded once.
// Built as a shared object for the test, and with -DGN_BF16_EMUL_MAIN as a stand-alone program for a sanitizer run.
#include <cstddef>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h"

using namespace sgr;

namespace {
inline int lo(int a) { return a > 0 ? a : 0; }
inline int hi(int a, int n) { return a < n ? a : n - 1; }

template <typename T>
void stage_fwd(const T* x, const float* weight, const float* bias, const T* skip, T* out, float* stats, int B, int C, int G, int Cs, int H, int W, float eps) {
  const int cpg = C / G, HW = H * W, W2 = (W + 1) / 2, OW = 2 * W;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double s = 0.0, ss = 0.0;
      const T* xg = x + ((size_t)b * C + (size_t)g * cpg) * HW;
      for (size_t e = 0; e < (size_t)cpg * HW; ++e) {
        const double d = (double)gn_in(xg[e]);
        s += d;
        ss += d * d;
      }
      float* st = stats + 4 * ((size_t)b * G + g);
      gn_finish(s, ss, (double)cpg * HW, eps, st[0], st[1], st[2], st[3]);
    }
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < C + Cs; ++ch) {
      const bool norm = ch < C;
      const float* st = stats + 4 * ((size_t)b * G + (norm ? ch / cpg : 0));
      const float mh = st[0], ml = st[1], rstd = st[2], wc = norm ? weight[ch] : 1.0f, bc = norm ? bias[ch] : 0.0f;
      const T* src = norm ? x + ((size_t)b * C + ch) * HW : skip + ((size_t)b * Cs + (ch - C)) * HW;
      auto val = [&](int r, int c) {
        const float t = gn_in(src[(size_t)r * W + c]);
        return norm ? fmaxf(gn_pre(gn_xhat(t, mh, ml, rstd), wc, bc), 0.0f) : t;
      };
      if (!skip) {
        T* y = out + ((size_t)b * C + ch) * HW;
        for (int p = 0; p < HW; ++p) y[p] = gn_out<T>(val(p / W, p % W));
        continue;
      }
      T* op = out + ((size_t)b * (C + Cs) + ch) * 4 * HW;
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
              op[(size_t)(2 * i) * OW + 4 * jj + k] = gn_out<T>(top[k]);
              op[(size_t)(2 * i + 1) * OW + 4 * jj + k] = gn_out<T>(bot[k]);
            }
        }
    }
}

template <typename T>
void stage_bwd(const T* g, const T* x, const float* weight, const float* bias, const float* stats, T* dx, float* dweight, float* dbias, T* dskip, int B, int C,
               int G, int Cs, int H, int W) {
  const bool up = Cs > 0;
  const int cpg = C / G, HW = H * W, W2 = (W + 1) / 2, OW = up ? 2 * W : W, OH = up ? 2 * H : H;
  std::vector<float> dy((size_t)B * C * HW);      // fp32, as the kernels' workspace
  std::vector<double> s1((size_t)B * C, 0.0), s2((size_t)B * C, 0.0);
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < C + Cs; ++ch) {
      const bool norm = ch < C;
      const float* st = stats + 4 * ((size_t)b * G + (norm ? ch / cpg : 0));
      const float mh = st[0], ml = st[1], rstd = st[2];
      const T* gp = g + ((size_t)b * (C + Cs) + ch) * OH * OW;
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
                gv[k][u] = orow >= 0 && orow < OH && oc >= 0 && oc < OW ? gn_in(gp[(size_t)orow * OW + oc]) : 0.0f;
              }
            }
            up_adjoint(gv, wr, wa, wb, a0, a1);
          } else {
            a0 = gn_in(gp[(size_t)i * W + c0]);
            a1 = two ? gn_in(gp[(size_t)i * W + c0 + 1]) : 0.0f;
          }
          if (norm) {
            const T* xp = x + ((size_t)b * C + ch) * HW;
            const float h0 = gn_xhat(gn_in(xp[(size_t)i * W + c0]), mh, ml, rstd), h1 = two ? gn_xhat(gn_in(xp[(size_t)i * W + c0 + 1]), mh, ml, rstd) : 0.0f;
            a0 = gn_pre(h0, weight[ch], bias[ch]) > 0.0f ? a0 : 0.0f;
            a1 = two && gn_pre(h1, weight[ch], bias[ch]) > 0.0f ? a1 : 0.0f;
            s1[(size_t)b * C + ch] += (double)a0 + (double)a1;
            s2[(size_t)b * C + ch] += (double)a0 * (double)h0 + (double)a1 * (double)h1;
            float* dst = dy.data() + ((size_t)b * C + ch) * HW;
            dst[(size_t)i * W + c0] = a0;
            if (two) dst[(size_t)i * W + c0 + 1] = a1;
          } else {
            T* dst = dskip + ((size_t)b * Cs + (ch - C)) * HW;
            dst[(size_t)i * W + c0] = gn_out<T>(a0);
            if (two) dst[(size_t)i * W + c0 + 1] = gn_out<T>(a1);
          }
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
          dx[o] = gn_out<T>(gn_dx(dy[o], gn_xhat(gn_in(x[o]), st[0], st[1], st[2]), weight[c], st[2], c1, c2));
        }
    }
}
}  // namespace

extern "C" {

// out[h] = the fp32 value of the bf16 pattern h, h = 0 .. 65535
void emul_bf16_up_all(float* out) {
  for (unsigned h = 0; h < 65536u; ++h) out[h] = bf16_up((unsigned short)h);
}
void emul_bf16_round(const float* in, unsigned short* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = bf16_round(in[i]);
}

// contiguous tensors; the bf16 ones as their 16-bit patterns; skip == nullptr (Cs == 0): the plain form
void emul_gn_stage_fwd_bf16(const unsigned short* x, const float* weight, const float* bias, const unsigned short* skip, unsigned short* out, float* stats, int B,
                            int C, int G, int Cs, int H, int W, float eps) {
  stage_fwd(reinterpret_cast<const bf16*>(x), weight, bias, reinterpret_cast<const bf16*>(skip), reinterpret_cast<bf16*>(out), stats, B, C, G, Cs, H, W, eps);
}
void emul_gn_stage_bwd_bf16(const unsigned short* g, const unsigned short* x, const float* weight, const float* bias, const float* stats, unsigned short* dx,
                            float* dweight, float* dbias, unsigned short* dskip, int B, int C, int G, int Cs, int H, int W) {
  stage_bwd(reinterpret_cast<const bf16*>(g), reinterpret_cast<const bf16*>(x), weight, bias, stats, reinterpret_cast<bf16*>(dx), dweight, dbias,
            reinterpret_cast<bf16*>(dskip), B, C, G, Cs, H, W);
}
// the same loops on fp32 tensors: what gn_stage_emul.cpp computes (the test asserts that, bit for bit)
void emul_gn_stage_fwd_f32(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, int B, int C, int G, int Cs, int H,
                           int W, float eps) {
  stage_fwd(x, weight, bias, skip, out, stats, B, C, G, Cs, H, W, eps);
}
void emul_gn_stage_bwd_f32(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight, float* dbias,
                           float* dskip, int B, int C, int G, int Cs, int H, int W) {
  stage_bwd(g, x, weight, bias, stats, dx, dweight, dbias, dskip, B, C, G, Cs, H, W);
}

}  // extern "C"

#ifdef GN_BF16_EMUL_MAIN
// Stand-alone run for -fsanitize=address,undefined: every conversion pattern, then both forms forward and backward at the shapes whose
// index arithmetic differs (odd width, one pixel, one row), on values from a fixed generator.  Exit code 0 and no sanitizer report: clean.
#include <cstdio>

int main() {
  std::vector<float> up(65536);
  emul_bf16_up_all(up.data());
  std::vector<float> probe;
  const unsigned lows[6] = {0x0000u, 0x0001u, 0x7fffu, 0x8000u, 0x8001u, 0xffffu};
  for (unsigned h = 0; h < 65536u; ++h)
    for (unsigned l : lows) {
      const unsigned u = (h << 16) | l;
      float f;
      __builtin_memcpy(&f, &u, 4);
      probe.push_back(f);
    }
  std::vector<unsigned short> rounded(probe.size());
  emul_bf16_round(probe.data(), rounded.data(), (long long)probe.size());
  unsigned long long check = 0;
  for (unsigned short r : rounded) check += r;
  unsigned state = 12345u;
  auto next = [&] { state = state * 1664525u + 1013904223u; return (float)((state >> 8) & 0xffff) / 32768.0f - 1.0f; };
  const int shapes[4][6] = {{2, 8, 2, 4, 3, 5}, {1, 4, 2, 2, 1, 1}, {2, 8, 4, 0, 1, 7}, {1, 8, 2, 3, 4, 8}};      // B, C, G, Cs, H, W
  for (const auto& s : shapes) {
    const int B = s[0], C = s[1], G = s[2], Cs = s[3], H = s[4], W = s[5], HW = H * W;
    const size_t no = Cs ? (size_t)B * (C + Cs) * 4 * HW : (size_t)B * C * HW;
    std::vector<unsigned short> x((size_t)B * C * HW), skip((size_t)B * Cs * HW), ct(no), out(no), dx(x.size()), ds(skip.size());
    std::vector<float> w(C), b(C), stats((size_t)B * G * 4), dw(C), db(C);
    for (auto& v : x) v = bf16_round(next());
    for (auto& v : skip) v = bf16_round(next());
    for (auto& v : ct) v = bf16_round(next());
    for (auto& v : w) v = next();
    for (auto& v : b) v = 0.3f * next();
    emul_gn_stage_fwd_bf16(x.data(), w.data(), b.data(), Cs ? skip.data() : nullptr, out.data(), stats.data(), B, C, G, Cs, H, W, 1e-5f);
    emul_gn_stage_bwd_bf16(ct.data(), x.data(), w.data(), b.data(), stats.data(), dx.data(), dw.data(), db.data(), Cs ? ds.data() : nullptr, B, C, G, Cs, H, W);
    for (unsigned short v : out) check += v;
    for (unsigned short v : dx) check += v;
  }
  std::printf("gn_stage_bf16_emul: checksum %llu\n", check);
  return 0;
}
#endif
