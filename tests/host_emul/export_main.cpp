// Host build of the export kernels' decisions (csrc/sgr_export.h): a stand-alone program, so that it can run under
// -fsanitize=address,undefined (tests/test_export.py compiles and runs it; nothing here is loaded into python).
//
//   export_main <input> <output>
//   input:  int32 mode
//     mode 0 (image):  int32 kind, B, C, h, w, nh, nw, bgr, has_scale; float x[B*C*h*w]; float scale[B] when has_scale
//     mode 1 (mosaic): int32 B, R, C, eh, ew, nrows, ncols, gap, bgr; float env[B*3*R*C*eh*ew]
//     mode 2 (index):  int32 in, out                 -> int32 s[out], float f[out]
//   output: the bytes as the kernels form them -- the statistic folded in double, the before-resize map once per source element into a
//   staged copy, columns first then rows, the after-resize map, the quantiser; for the mosaic the geometry and cell walk of ex_mosaic.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_export.h"

using namespace sgr::ex;

static bool get(FILE* f, int* v, int n) { return fread(v, 4, n, f) == (size_t)n; }

static int image(FILE* f, FILE* o) {
  int a[9];
  if (!get(f, a, 9)) return 3;
  const int kind = a[0], B = a[1], C = a[2], h = a[3], w = a[4], nh = a[5], nw = a[6], bgr = a[7], has_scale = a[8];
  if (kind < 0 || kind >= kKinds || B <= 0 || h <= 0 || w <= 0 || nh <= 0 || nw <= 0 || !kind_takes(kind, C)) return 3;
  if (!kind_resizes(kind) && (nh != h || nw != w)) return 3;
  std::vector<float> x((size_t)B * C * h * w), scale(B, 1.0f);
  if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
  if (has_scale && fread(scale.data(), 4, B, f) != (size_t)B) return 3;
  const int cout = kind_out_channels(kind, C), n = C * h * w;
  std::vector<unsigned char> out((size_t)B * nh * nw * cout);
  std::vector<float> staged(n);
  for (int b = 0; b < B; ++b) {
    const float* xb = &x[(size_t)b * n];
    float p = scale[b];
    if (kind_stat(kind) == kMean) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += xb[i];
      p = stat_param(kind, s, (double)n);
    } else if (kind_stat(kind) == kMax) {
      float m = -INFINITY;
      for (int i = 0; i < n; ++i) m = fmaxf(m, xb[i]);
      p = stat_param(kind, (double)m, 1.0);
    }
    for (int i = 0; i < n; ++i) staged[i] = pre_map(kind, xb[i], p);
    for (int y = 0; y < nh; ++y) {
      const Src sy = src_of(y, h, nh);
      const int yB = sy.s + 1 < h ? sy.s + 1 : h - 1;
      for (int xx = 0; xx < nw; ++xx) {
        const Src sx = src_of(xx, w, nw);
        const int xB = sx.s + 1 < w ? sx.s + 1 : w - 1;
        for (int k = 0; k < cout; ++k) {
          const int c = C == 1 ? 0 : (bgr ? C - 1 - k : k);
          const float* s = &staged[(size_t)c * h * w];
          const float top = lerp2(s[sy.s * w + sx.s], s[sy.s * w + xB], sx.f), bot = lerp2(s[yB * w + sx.s], s[yB * w + xB], sx.f);
          out[(((size_t)b * nh + y) * nw + xx) * cout + k] = (unsigned char)quantise(post_map(kind, lerp2(top, bot, sy.f), p));
        }
      }
    }
  }
  return fwrite(out.data(), 1, out.size(), o) == out.size() ? 0 : 4;
}

static int mosaic(FILE* f, FILE* o) {
  int a[9];
  if (!get(f, a, 9)) return 3;
  const int B = a[0], R = a[1], C = a[2], eh = a[3], ew = a[4], nrows = a[5], ncols = a[6], gap = a[7], bgr = a[8];
  if (B <= 0 || R <= 0 || C <= 0 || eh <= 0 || ew <= 0 || nrows <= 0 || ncols <= 0 || gap < 0 || nrows > R || ncols > C) return 3;
  const size_t plane = (size_t)eh * ew, chan = (size_t)R * C * plane;
  std::vector<float> env((size_t)B * 3 * chan);
  if (fread(env.data(), 4, env.size(), f) != env.size()) return 3;
  const Mosaic m = mosaic_of(R, C, eh, ew, nrows, ncols, gap);
  std::vector<unsigned char> out((size_t)B * m.Hm * m.Wm * 3);
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < m.Hm; ++y) {
      int r, iy;
      const bool row_in = mosaic_src(y, eh, gap, m.tilesY, m.interY, r, iy);
      for (int xx = 0; xx < m.Wm; ++xx) {
        int c, ix;
        const bool in = mosaic_src(xx, ew, gap, m.tilesX, m.interX, c, ix) && row_in;
        for (int k = 0; k < 3; ++k) {
          const int ch = bgr ? 2 - k : k;
          const unsigned q = in ? quantise(post_map(kImageGamma, env[((size_t)b * 3 + ch) * chan + ((size_t)r * C + c) * plane + (size_t)iy * ew + ix], 1.0f)) : 255u;
          out[(((size_t)b * m.Hm + y) * m.Wm + xx) * 3 + k] = (unsigned char)q;
        }
      }
    }
  int dims[2] = {m.Hm, m.Wm};
  if (fwrite(dims, 4, 2, o) != 2) return 4;
  return fwrite(out.data(), 1, out.size(), o) == out.size() ? 0 : 4;
}

static int index_rule(FILE* f, FILE* o) {
  int a[2];
  if (!get(f, a, 2) || a[0] <= 0 || a[1] <= 0) return 3;
  std::vector<int> s(a[1]);
  std::vector<float> fr(a[1]);
  for (int d = 0; d < a[1]; ++d) {
    const Src v = src_of(d, a[0], a[1]);
    s[d] = v.s;
    fr[d] = v.f;
  }
  return fwrite(s.data(), 4, s.size(), o) == s.size() && fwrite(fr.data(), 4, fr.size(), o) == fr.size() ? 0 : 4;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int mode = -1;
  int rc = 3;
  if (get(f, &mode, 1)) rc = mode == 0 ? image(f, o) : mode == 1 ? mosaic(f, o) : mode == 2 ? index_rule(f, o) : 3;
  fclose(f);
  fclose(o);
  return rc;
}
