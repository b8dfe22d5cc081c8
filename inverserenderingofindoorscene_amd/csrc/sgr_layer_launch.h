// Host side of the render layer: what stands between an extern "C" entry point and hipLaunchKernelGGL, defined once -- the dims
// block, the pooling and decoder-heads predicates, the half-wave grid and the compile-time choice of POOL / envWidth.  Included by
// sgr_forward.inl, sgr_backward.inl and sgr_bwd_brdf.hip after the kernels (it needs Args, kPx and fast_ok; check_pool, pool1, the
// direction table's layout and choose / with_flag, which need nothing of the layer, are in sgr_launch.h, which every file with an entry
// point shares).  No kernel and no device function lives here.
#pragma once
#include "sgr_fast.inl"

namespace sgr {

static inline void layer_dims(Args& a, int bn, int K, int R, int C, int eh, int ew, int imH, int imW) {
  const DirLayout t = dir_layout(eh, ew);
  a.bn = bn; a.K = K; a.R = R; a.C = C; a.J = eh * ew; a.Jpad = t.Jpad; a.imH = imH; a.imW = imW;
  a.eh = eh; a.ew = ew;
  a.rows = reinterpret_cast<const float*>(a.dirs) + t.rows;      // separable form of the table (include/sgrender.h)
  a.cols = reinterpret_cast<const float*>(a.dirs) + t.cols;
}

// after check_pool: the maps are at the env grid's size (POOL = 1), else at twice it (POOL = 2)
static inline bool pool1(const Args& a) { return pool1(a.R, a.C, a.imH, a.imW); }

// premap == 3 (the decoder heads as a prologue, their chain rule as the backward's epilogue) is implemented in the packed kernels'
// lobe loader (sgr_pk.inl) only: the shapes the default dispatch sends there
static inline bool heads_ok(const Args& a) { return fast_ok(a) && !sgr_generic_forced() && a.K > 6 && a.K <= 24; }

// the packed half-wave kernels: one workgroup (wave) per 32 pixels of one image
static inline int half_wave_tiles(int R, int C) { return (R * C + kPx - 1) / kPx; }
static inline dim3 half_wave_grid(int bn, int R, int C) { return dim3((unsigned)(bn * half_wave_tiles(R, C))); }

// the layer's two run-time choices of a template argument (choose, sgr_launch.h):
//   with_pool(pool1(a), [&](auto P) { hipLaunchKernelGGL((kernel<P()>), ...); });
template <class F> static inline auto with_pool(bool p1, F&& f) { return choose<Int<1>, Int<2>>(p1, f); }
template <class F> static inline auto with_ew(int ew, F&& f) { return choose<Int<16>, Int<32>>(ew == 16, f); }      // after fast_ok

}  // namespace sgr
