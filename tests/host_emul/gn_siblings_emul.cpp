// TEST INFRASTRUCTURE ONLY -- never shipped, never loaded by the product package.
//
// The sibling forms of the decoders' upcat stage on the host: D siblings through the per-element arithmetic of
// inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h, as tests/host_emul/gn_stage_emul.cpp and gn_resize_emul.cpp drive it for one
// operator (both are included here, each in a namespace of its own: they carry the same helper names).  What the sibling kernels add is
// the order of dskip: a skip channel's adjoint is formed per sibling exactly as the single operator forms it and the siblings are added
// in fp32 in sibling order, ((s_0 + s_1) + s_2) + ...; a sibling without a cotangent (NULL) is left out.  Everything else is the single
// operator per sibling.  tests/test_gn_siblings.py holds this to half the GPU tests' bound on the reference's fixtures.
//
// Built as a shared object for the test, and with -DGN_SIBLINGS_EMUL_MAIN as a stand-alone program for a sanitizer run.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_gn_stage.h"

namespace same_size {
#include "gn_stage_emul.cpp"
}
namespace resized {
#include "gn_resize_emul.cpp"
}

extern "C" {

// contiguous tensors; xs, weights, biases, outs: D pointers; stats [D,B,G,4]; (Hs, Ws) == (H, W): the same-size form
void emul_gn_siblings_fwd(int D, const float* const* xs, const float* const* weights, const float* const* biases, const float* skip, float* const* outs,
                          float* stats, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws, float eps) {
  for (int d = 0; d < D; ++d) {
    float* st = stats + (size_t)d * B * G * 4;
    if (Hs == H && Ws == W) same_size::emul_gn_stage_fwd(xs[d], weights[d], biases[d], skip, outs[d], st, B, C, G, Cs, H, W, eps);
    else resized::emul_gn_resize_fwd(xs[d], weights[d], biases[d], skip, outs[d], st, B, C, G, Cs, H, W, Hs, Ws, eps);
  }
}

// gs[d] == NULL: sibling d has no cotangent; dxs / dweights / dbiases: D pointers (the entries of such a sibling are not written)
void emul_gn_siblings_bwd(int D, const float* const* gs, const float* const* xs, const float* const* weights, const float* const* biases, const float* stats,
                          float* const* dxs, float* const* dweights, float* const* dbiases, float* dskip, int B, int C, int G, int Cs, int H, int W, int Hs,
                          int Ws) {
  const size_t ns = (size_t)B * Cs * Hs * Ws;
  std::vector<float> s(ns);
  bool first = true;
  for (int d = 0; d < D; ++d) {
    if (!gs[d]) continue;
    const float* st = stats + (size_t)d * B * G * 4;
    if (Hs == H && Ws == W) same_size::emul_gn_stage_bwd(gs[d], xs[d], weights[d], biases[d], st, dxs[d], dweights[d], dbiases[d], s.data(), B, C, G, Cs, H, W);
    else resized::emul_gn_resize_bwd(gs[d], xs[d], weights[d], biases[d], st, dxs[d], dweights[d], dbiases[d], s.data(), B, C, G, Cs, H, W, Hs, Ws);
    for (size_t e = 0; e < ns; ++e) dskip[e] = first ? s[e] : dskip[e] + s[e];
    first = false;
  }
}

}  // extern "C"

#ifdef GN_SIBLINGS_EMUL_MAIN
// Stand-alone run for -fsanitize=address,undefined: both forms forward and backward for D = 1, 3 and 8 with one sibling left out, at the
// shapes whose index arithmetic differs (odd width, one pixel, both axes resized), on values from a fixed generator.
#include <cstdio>

int main() {
  unsigned state = 12345u;
  auto next = [&]() {
    state = state * 1664525u + 1013904223u;
    return (float)((state >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  const int shapes[][6] = {{2, 8, 3, 5, 3, 5}, {1, 8, 1, 1, 1, 1}, {2, 8, 3, 5, 4, 6}, {1, 8, 1, 1, 2, 2}, {2, 8, 2, 3, 4, 6}};
  double checksum = 0.0;
  for (const auto& sh : shapes)
    for (int D : {1, 3, 8}) {
      const int B = sh[0], C = sh[1], G = 2, Cs = 3, H = sh[2], W = sh[3], Hs = sh[4], Ws = sh[5];
      const size_t nx = (size_t)B * C * H * W, no = (size_t)B * (C + Cs) * 4 * Hs * Ws, ns = (size_t)B * Cs * Hs * Ws;
      std::vector<std::vector<float>> x(D), w(D), b(D), o(D), g(D), dx(D), dw(D), db(D);
      std::vector<const float*> px(D), pw(D), pb(D), pg(D);
      std::vector<float*> po(D), pdx(D), pdw(D), pdb(D);
      for (int d = 0; d < D; ++d) {
        x[d].resize(nx); w[d].resize(C); b[d].resize(C); o[d].resize(no); g[d].resize(no); dx[d].resize(nx); dw[d].resize(C); db[d].resize(C);
        for (auto& v : x[d]) v = (d == 1 ? 100.0f : 0.0f) + next();
        for (auto& v : w[d]) v = next();
        for (auto& v : b[d]) v = 0.3f * next();
        for (auto& v : g[d]) v = next();
        px[d] = x[d].data(); pw[d] = w[d].data(); pb[d] = b[d].data(); po[d] = o[d].data();
        pg[d] = D > 1 && d == 1 ? nullptr : g[d].data();      // sibling 1 left out of the loss
        pdx[d] = dx[d].data(); pdw[d] = dw[d].data(); pdb[d] = db[d].data();
      }
      std::vector<float> skip(ns), stats((size_t)D * B * G * 4), ds(ns);
      for (auto& v : skip) v = next();
      emul_gn_siblings_fwd(D, px.data(), pw.data(), pb.data(), skip.data(), po.data(), stats.data(), B, C, G, Cs, H, W, Hs, Ws, 1e-5f);
      emul_gn_siblings_bwd(D, pg.data(), px.data(), pw.data(), pb.data(), stats.data(), pdx.data(), pdw.data(), pdb.data(), ds.data(), B, C, G, Cs, H, W, Hs, Ws);
      for (int d = 0; d < D; ++d) {
        for (float v : o[d]) checksum += v;
        if (pg[d])
          for (float v : dx[d]) checksum += v;
      }
      for (float v : ds) checksum += v;
    }
  if (!std::isfinite(checksum)) return 1;
  std::printf("checksum %.6f\n", checksum);
  return 0;
}
#endif
