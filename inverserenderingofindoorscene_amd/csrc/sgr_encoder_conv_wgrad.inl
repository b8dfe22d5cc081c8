// The weight gradient's matrix kernel of the encoders' pad + 4x4 stride-2 convolution, and what every kernel of sgr_encoder_conv.hip shares
// with it.  It lives in a file of its own because it is compiled in two translation units: sgr_encoder_conv.hip instantiates the
// single-source form, sgr_encoder_conv_cat.hip the several-source form.  Instantiated side by side in one module, the several-source form
// moved the single-source form's instruction stream (the optimiser's module-wide passes; profiles/r23_encoder_conv_cat_asm_compare.txt),
// and the single-source kernels are not to move.
#pragma once

#include "sgr_encoder_conv.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"        // block_sum, wave_sum, Vec<4>, aligned16

namespace sgr {

constexpr int kEcThreads = 256;
constexpr unsigned kEcAbsent = 0xffffffffu;      // the offset of a zeros-mode pad element

struct EcStrides { long long b, c, h, w; };
using ec_f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ ec_f32x4 ec_mfma(float a, float b, ec_f32x4 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}

// The kernels carry a flag, CAT, in the form of a trailing argument pack.  An empty pack is the single-source kernel, which the flag leaves
// as it was: the same arguments at the same offsets, and every CAT branch an `if constexpr`.  A pack of one is the several-source kernel:
// an EcSources table (sgr_encoder_conv.h; x and xs are then unused) or, in the data gradient, an EcRange.
struct EcRange { int cbase, Ct; };      // dx's channels are cbase .. cbase + C - 1 of the Ct channels of Wt [O, Ct, 4, 4]
template <typename T> __device__ __forceinline__ const T& ec_only(const T& t) { return t; }

// grid (strips of 25 pixel tiles, channel blocks x output passes, B).  partial[(((b S + strip) C + c) 16 + tap) O + o].  NT: N tiles of the
// largest pass, CW: channels per wave of the largest block; a channel past C is a plane of zeros, an output past O a zero cotangent, and
// neither is stored
// CAT: the block's 16 channels are the concatenation's and may belong to several sources.  Wave w then carries the channels w, w + 4, ..
// of the block (those its own MFMAs read, 340 halo elements each, six a lane) so that the source of a load is uniform across the wave; the
// tile in LDS is the same tile
template <int NT, int CW, typename... Tab>
__global__ __launch_bounds__(kEcThreads) void ec_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ x, EcStrides xs, float* __restrict__ partial,
                                                              int C, int O, int H, int W, int tilesX, int tiles, int opasses, int mode, Tab... tab) {
  constexpr bool CAT = sizeof...(Tab) == 1;
  constexpr int kHalo = kEcWRows * kEcWCols, kXElems = kEcWCB * kHalo, kCatPer = (kHalo + 63) / 64;
  constexpr int kXLoads = CAT ? CW * kCatPer : (kXElems + kEcThreads - 1) / kEcThreads;
  constexpr int kGLoads = kEcPassO * 64 / kEcThreads;
  __shared__ float xt[kEcWCB * kEcWCHP];
  __shared__ float gtl[kEcPassO * kEcWGP];
  const int Ho = ec_out(H), Wo = ec_out(W);
  const int strip = blockIdx.x, cblk = blockIdx.y / opasses, opass = blockIdx.y - cblk * opasses, b = blockIdx.z;
  const int c0 = cblk * kEcWCB, ncb = min(kEcWCB, C - c0), o0 = opass * kEcPassO, nnt = min(kEcPassNT, (O - o0) / 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = strip * kEcWStrip, t1 = min(t0 + kEcWStrip, tiles);
  const float* xb = x + (long long)b * xs.b + (long long)c0 * xs.c;
  const float* gb = g + ((long long)b * O + o0) * Ho * Wo;
  float rx[kXLoads], rg[kGLoads];
  auto fetch = [&](int t) {
    const int tyi = t / tilesX, j0 = (t - tyi * tilesX) * kEcWW, i0 = tyi * kEcWH;
    if constexpr (CAT) {
      const int uwave = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
      for (int a = 0; a < CW; ++a) {
        const int cc = uwave + 4 * a;
        const bool live = cc < ncb;
        const EcSource src = ec_source_of(ec_only(tab...), live ? c0 + cc : 0);
        const float* xp = ec_source_plane(src, b, live ? c0 + cc : 0);
#pragma unroll
        for (int j = 0; j < kCatPer; ++j) {
          const int e = lane + 64 * j < kHalo ? lane + 64 * j : -1, r = e < 0 ? 0 : e / kEcWCols, tc = e < 0 ? 0 : e - r * kEcWCols;
          rx[a * kCatPer + j] = (live && e >= 0) ? ec_source_at(src, xp, ec_src(2 * i0 - 1 + r, H, mode), ec_src(2 * j0 - 1 + tc, W, mode)) : 0.0f;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kXLoads; ++k) {
        const int e = tid + k * kEcThreads, cc = e / kHalo, r2 = e - cc * kHalo, r = r2 / kEcWCols, tc = r2 - r * kEcWCols;
        const int sr = ec_src(2 * i0 - 1 + r, H, mode), sc = ec_src(2 * j0 - 1 + tc, W, mode);
        rx[k] = (e < kXElems && cc < ncb && sr >= 0 && sc >= 0) ? xb[(long long)cc * xs.c + (unsigned)sr * (unsigned)xs.h + (unsigned)sc * (unsigned)xs.w] : 0.0f;
      }
    }
    // pixel p = tid & 63 of the tile, outputs (tid >> 6) + 4 k; outside the map and past the pass's outputs: exact zeros
    const int p = tid & 63, gy = i0 + (p >> 4), gx = j0 + (p & 15);
    const bool in = gy < Ho && gx < Wo;
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) {
      const int o = (tid >> 6) + 4 * k;
      rg[k] = (in && o < 16 * nnt) ? gb[((long long)o * Ho + gy) * Wo + gx] : 0.0f;
    }
  };
  auto put = [&]() {
    if constexpr (CAT) {
#pragma unroll
      for (int a = 0; a < CW; ++a)
#pragma unroll
        for (int j = 0; j < kCatPer; ++j) {
          const int e = lane + 64 * j < kHalo ? lane + 64 * j : -1, r = e < 0 ? 0 : e / kEcWCols, tc = e < 0 ? 0 : e - r * kEcWCols;
          if (e >= 0) xt[ec_w_x_idx(wave + 4 * a, r, tc)] = rx[a * kCatPer + j];
        }
    } else {
#pragma unroll
      for (int k = 0; k < kXLoads; ++k) {
        const int e = tid + k * kEcThreads, cc = e / kHalo, r2 = e - cc * kHalo, r = r2 / kEcWCols, tc = r2 - r * kEcWCols;
        if (e < kXElems) xt[ec_w_x_idx(cc, r, tc)] = rx[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) gtl[ec_w_g_idx((tid >> 6) + 4 * k, tid & 63)] = rg[k];
  };
  ec_f32x4 run[CW][NT];
#pragma unroll
  for (int a = 0; a < CW; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n) run[a][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  fetch(t0);
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    __syncthreads();      // the previous tile's readers are done
    put();
    __syncthreads();
    if (t + 1 < t1) fetch(t + 1);      // in flight while tile t is consumed
    ec_f32x4 acc[CW][NT];
#pragma unroll
    for (int a = 0; a < CW; ++a)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[a][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      float bv[NT], av[CW];
#pragma unroll
      for (int n = 0; n < NT; ++n) bv[n] = gtl[ec_w_b_addr(lane, s, n)];
#pragma unroll
      for (int a = 0; a < CW; ++a) av[a] = xt[ec_w_a_addr(lane, s, wave + 4 * a)];
#pragma unroll
      for (int a = 0; a < CW; ++a)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = ec_mfma(av[a], bv[n], acc[a][n]);
    }
#pragma unroll
    for (int a = 0; a < CW; ++a)
#pragma unroll
      for (int n = 0; n < NT; ++n) run[a][n] += acc[a][n];
  }
  float* pw = partial + ((long long)b * gridDim.x + strip) * C * 16 * O;
#pragma unroll
  for (int a = 0; a < CW; ++a) {
    const int cc = wave + 4 * a;
    if (cc >= ncb) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if (n >= nnt) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[((long long)(c0 + cc) * 16 + lf_d_row(lane, r)) * O + o0 + 16 * n + lf_d_col(lane)] = run[a][n][r];
    }
  }
}

// the several-source launch (sgr_encoder_conv_cat.hip): grid (strips, channel blocks x output passes, B); NT, CW as sgr_encoder_conv_bwd picks them
void ec_launch_w_cat(dim3 grid, hipStream_t st, int NT, int CW, const float* g, const EcSources& tab, float* partial, int C, int O, int H, int W, int tilesX,
                     int tiles, int opasses, int mode);

}  // namespace sgr
