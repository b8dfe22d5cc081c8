// The light decoders' last step on gfx950: x_orig = dconvFinal(dpadFinal(dx6)), models.py:297-302, 334 -- ReplicationPad2d(1) followed by
// Conv2d(C -> O, k = 3, stride 1) with O = SGNum or 3 SGNum (12 / 36), as one operator without the padded copy.  DESIGN.md section 8h
// states the contract; the fragment maps, the K orderings, the LDS addresses and the accumulation orders are sgr_light_final_conv.h.
//
// Forward, one launch, an implicit GEMM on v_mfma_f32_16x16x4_f32: a workgroup makes a 32 x 8 tile of all O output planes.  Eight input
// channels at a time, the tile with its halo (34 x 10, through y's strides, clamped at the map's border, which is the pad) and the chunk's
// weights as [k][o] go from HBM to LDS while the previous chunk is consumed from the other buffer; a wave keeps 4 M tiles x NT N tiles of
// accumulators for the chunk and adds them to its running sums on the vector ALU.
// Backward, data, one launch, the same instruction: per group of four outputs the cotangent tile (34 x 6 with halo) and the weights as
// [k][c] are staged, a lane gathers the nine per-tap sums of its pixel (fc_gather_taps) as the A operands, and 2 M tiles x up to 8 N tiles
// (128 channels) of dy are accumulated; 128-bit stores where the plane allows.
// Backward, weights, two launches, the same instruction with the pixels as K: a workgroup takes one image, 16 (or 32) channels and a strip
// of ten 32 x 4 pixel tiles; the map tile with its halo and the cotangent tile (zeros outside the map) are staged through registers while
// the previous tile is consumed; a wave owns 4 or 5 (channel sub-block, tap) pairs with their N tiles, sums 64 pixels at a time and adds that to its
// running sums; the strip's fp32 partial goes to the workspace with ordinary vector stores and a second launch folds the partials in double
// in index order.  Backward, bias, two launches on the vector ALU: sgr_final_conv.hip's scheme.  No atomics anywhere: two runs give the
// same bits.
#include "sgr_light_final_conv.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"        // block_sum, wave_sum, Vec<4>, aligned16

namespace sgr {

constexpr int kLfThreads = 256;
constexpr int kLfRounds = 8;                  // runs of four pixels per thread in the bias pass

struct LfStrides { long long b, c, h, w; };
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f32x4 lf_mfma(float a, float b, f32x4 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kLfThreads) void lf_fwd_kernel(const float* __restrict__ y, LfStrides ys, const float* __restrict__ Wt,
                                                            const float* __restrict__ bias, float* __restrict__ out, int C, int O, int H, int W,
                                                            int tilesX) {
  constexpr int WP = lf_wpitch(NT), kHalo = kLfRows * kLfPitch, kWElems = 9 * kLfKC * 16 * NT;
  constexpr int kALoads = (kHalo + kLfThreads - 1) / kLfThreads, kWLoads = (kWElems + kLfThreads - 1) / kLfThreads;
  extern __shared__ float4 lf_smem4[];
  float* at = reinterpret_cast<float*>(lf_smem4);      // [2][kLfKC * kLfPlane]
  float* wl = at + 2 * kLfKC * kLfPlane;               // [2][72 * WP]
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int x0 = txi * kLfTW, y0 = tyi * kLfTH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // what this thread carries from HBM to LDS for every channel: element e = tid + 256 k of the 10 x 34 halo tile
  unsigned off[kALoads];
  int lidx[kALoads];
#pragma unroll
  for (int k = 0; k < kALoads; ++k) {
    const int e = tid + k * kLfThreads;
    const bool valid = e < kHalo;
    const int r = valid ? e / kLfPitch : 0, col = valid ? e - r * kLfPitch : 0;
    off[k] = (unsigned)fc_cl(y0 - 1 + r, H) * (unsigned)ys.h + (unsigned)fc_cl(x0 - 1 + col, W) * (unsigned)ys.w;      // fits 31 bits (host check)
    lidx[k] = valid ? lf_fwd_tile_idx(0, r, col) : -1;
  }
  const float* yb = y + (long long)b * ys.b;
  float ra[kLfKC][kALoads], rw[kWLoads];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int cc = 0; cc < kLfKC; ++cc) {
      const float* yp = yb + (long long)(c0 + cc) * ys.c;
#pragma unroll
      for (int k = 0; k < kALoads; ++k) ra[cc][k] = lidx[k] >= 0 ? yp[off[k]] : 0.0f;
    }
    // the chunk's weights of output o are 72 consecutive floats of Wt: [cc][tap]
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kLfThreads, o = e / (9 * kLfKC), r = e - o * (9 * kLfKC);
      rw[k] = (e < kWElems && o < O) ? Wt[((long long)o * C + c0) * 9 + r] : 0.0f;      // o >= O: the zero columns of the last N tile
    }
  };
  auto put = [&](int buf) {
    float* ad = at + buf * (kLfKC * kLfPlane);
    float* wd = wl + buf * (9 * kLfKC * WP);
#pragma unroll
    for (int cc = 0; cc < kLfKC; ++cc)
#pragma unroll
      for (int k = 0; k < kALoads; ++k)
        if (lidx[k] >= 0) ad[cc * kLfPlane + lidx[k]] = ra[cc][k];
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kLfThreads, o = e / (9 * kLfKC), r = e - o * (9 * kLfKC), cc = r / 9, tap = r - 9 * cc;
      if (e < kWElems) wd[lf_fwd_w_idx(tap * kLfKC + cc, o, WP)] = rw[k];
    }
  };
  f32x4 run[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) run[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  fetch(0);
  put(0);
  __syncthreads();
  const int chunks = C / kLfKC;
#pragma unroll 1
  for (int ci = 0; ci < chunks; ++ci) {
    if (ci + 1 < chunks) fetch((ci + 1) * kLfKC);      // in flight while chunk ci is consumed
    const float* ab = at + (ci & 1) * (kLfKC * kLfPlane);
    const float* wb = wl + (ci & 1) * (9 * kLfKC * WP);
    f32x4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < kLfSteps; ++s) {
      float a[4], bv[NT];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = ab[lf_fwd_a_addr(lane, s, wave, m)];
#pragma unroll
      for (int n = 0; n < NT; ++n) bv[n] = wb[lf_fwd_b_addr(lane, s, n, WP)];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = lf_mfma(a[m], bv[n], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) run[m][n] += acc[m][n];
    if (ci + 1 < chunks) put((ci + 1) & 1);      // the other buffer: chunk ci - 1's readers passed the barrier below
    __syncthreads();
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int o = 16 * n + lf_d_col(lane);
    if (o >= O) continue;
    const float bo = bias[o];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int gy = y0 + lf_fwd_tile_row(wave, m), gx = x0 + lf_fwd_tile_col(m) + lf_d_row(lane, 0);
      if (gy >= H || gx >= W) continue;
      float* op = out + (((long long)b * O + o) * H + gy) * W + gx;
      if (VEC) {      // W % 4 == 0: a run that starts inside the map ends inside it
        Vec<4> q;
#pragma unroll
        for (int r = 0; r < 4; ++r) q.v[r] = run[m][n][r] + bo;
        *reinterpret_cast<Vec<4>*>(op) = q;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gx + r < W) op[r] = run[m][n][r] + bo;
      }
    }
  }
}

// grid (tiles, B, passes of 128 channels)
template <bool VEC>
__global__ __launch_bounds__(kLfThreads) void lf_bwd_data_kernel(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dy, int C,
                                                                 int O, int H, int W, int tilesX) {
  constexpr int kHalo = kLfGRows * kLfPitch, kGLoads = (4 * kHalo + kLfThreads - 1) / kLfThreads;
  constexpr int kWLoads = (9 * kLfPassC + kLfThreads - 1) / kLfThreads, kNT = kLfPassC / 16;
  __shared__ float gt[2][4 * kLfGPlane];
  __shared__ float wl[2][36 * kLfCP];
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int x0 = txi * kLfTW, y0 = tyi * kLfTHb;
  const int c0p = blockIdx.z * kLfPassC, ncp = min(kLfPassC, C - c0p), nnt = ncp / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the cotangent tile of a group: element e = tid + 256 k of [u][6][34]
  unsigned goff[kGLoads];
  int gu[kGLoads], glidx[kGLoads];
#pragma unroll
  for (int k = 0; k < kGLoads; ++k) {
    const int e = tid + k * kLfThreads;
    const bool valid = e < 4 * kHalo;
    const int u = valid ? e / kHalo : 0, r2 = e - u * kHalo, r = valid ? r2 / kLfPitch : 0, col = valid ? r2 - r * kLfPitch : 0;
    goff[k] = (unsigned)fc_cl(y0 - 1 + r, H) * (unsigned)W + (unsigned)fc_cl(x0 - 1 + col, W);
    gu[k] = u;
    glidx[k] = valid ? lf_bwd_g_idx(u, r, col) : -1;
  }
  const float* gb = g + (long long)b * O * H * W;
  float rg[kGLoads], rw[4][kWLoads];
  auto fetch = [&](int jg) {
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) {
      const int o = 4 * jg + gu[k];
      rg[k] = (glidx[k] >= 0 && o < O) ? gb[(long long)o * H * W + goff[k]] : 0.0f;
    }
    // the weights of output o for the workgroup's channels are 9 ncp consecutive floats of Wt: [c][tap]
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = 4 * jg + u;
#pragma unroll
      for (int k = 0; k < kWLoads; ++k) {
        const int r = tid + k * kLfThreads;
        rw[u][k] = (r < 9 * ncp && o < O) ? Wt[((long long)o * C + c0p) * 9 + r] : 0.0f;
      }
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int k = 0; k < kGLoads; ++k)
      if (glidx[k] >= 0) gt[buf][glidx[k]] = rg[k];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < kWLoads; ++k) {
        const int r = tid + k * kLfThreads, c = r / 9, tap = r - 9 * c;
        if (r < 9 * ncp) wl[buf][lf_bwd_w_idx(tap, u, c)] = rw[u][k];
      }
  };
  // a lane outside the map works on the nearest pixel inside it and stores nothing: every LDS index stays inside the tile
  const int h = y0 + wave, hc = fc_cl(h, H);
  f32x4 run[2][kNT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < kNT; ++n) run[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int groups = (O + 3) / 4;
  fetch(0);
  put(0);
  __syncthreads();
#pragma unroll 1
  for (int jg = 0; jg < groups; ++jg) {
    if (jg + 1 < groups) fetch(jg + 1);
    const float* gtb = gt[jg & 1];
    const float* wb = wl[jg & 1];
    float G[2][9];
#pragma unroll
    for (int m = 0; m < 2; ++m) lf_bwd_a_operands(gtb, lane, hc, fc_cl(x0 + 16 * m + lf_a_row(lane), W), y0, x0, H, W, G[m]);
    f32x4 acc[2][kNT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < kNT; ++n) acc[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int n = 0; n < kNT; ++n)
        if (n < nnt) {      // uniform in the workgroup
          const float bv = wb[lf_bwd_b_addr(lane, tap, n)];
          acc[0][n] = lf_mfma(G[0][tap], bv, acc[0][n]);
          acc[1][n] = lf_mfma(G[1][tap], bv, acc[1][n]);
        }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < kNT; ++n) run[m][n] += acc[m][n];
    if (jg + 1 < groups) put((jg + 1) & 1);
    __syncthreads();
  }
  if (h >= H) return;      // no barrier below
#pragma unroll
  for (int n = 0; n < kNT; ++n) {
    if (n >= nnt) continue;
    const int c = c0p + 16 * n + lf_d_col(lane);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int gx = x0 + 16 * m + lf_d_row(lane, 0);
      if (gx >= W) continue;
      float* op = dy + (((long long)b * C + c) * H + h) * W + gx;
      if (VEC) {
        Vec<4> q;
#pragma unroll
        for (int r = 0; r < 4; ++r) q.v[r] = run[m][n][r];
        *reinterpret_cast<Vec<4>*>(op) = q;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gx + r < W) op[r] = run[m][n][r];
      }
    }
  }
}

// grid (strips of 10 pixel tiles, C / (16 CBT), B).  partial[((((b S + strip) 9 + tap) C + c) OP + o], OP = 16 NT: every o < OP is written
template <int NT, int CBT>
__global__ __launch_bounds__(kLfThreads) void lf_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ y, LfStrides ys, float* __restrict__ partial,
                                                              int C, int O, int H, int W, int tilesX, int tiles) {
  constexpr int OP = 16 * NT, CB = 16 * CBT, kPairsAll = 9 * CBT, kPairs = (kPairsAll + 3) / 4;
  constexpr int kHalo = kLfWRows * kLfPitch, kYElems = CB * kHalo, kYLoads = (kYElems + kLfThreads - 1) / kLfThreads, kGLoads = OP / 2;
  __shared__ float yt[CB * kLfWPlane];
  __shared__ float gtl[OP * kLfWGP];
  const int strip = blockIdx.x, c0 = blockIdx.y * CB, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = strip * kLfWStrip, t1 = min(t0 + kLfWStrip, tiles);
  const float* yb = y + (long long)b * ys.b + (long long)c0 * ys.c;
  const float* gb = g + (long long)b * O * H * W;
  float ry[kYLoads], rg[kGLoads];
  auto fetch = [&](int t) {
    const int tyi = t / tilesX, x0 = (t - tyi * tilesX) * kLfTW, y0 = tyi * kLfTHw;
#pragma unroll
    for (int k = 0; k < kYLoads; ++k) {
      const int e = tid + k * kLfThreads, cc = e / kHalo, r2 = e - cc * kHalo, r = r2 / kLfPitch, col = r2 - r * kLfPitch;
      ry[k] = e < kYElems ? yb[(long long)cc * ys.c + (unsigned)fc_cl(y0 - 1 + r, H) * (unsigned)ys.h + (unsigned)fc_cl(x0 - 1 + col, W) * (unsigned)ys.w] : 0.0f;
    }
    // pixel p = tid & 127 of the tile, outputs of the parity tid >> 7; outside the map and past the outputs: exact zeros
    const int p = tid & 127, gy = y0 + (p >> 5), gx = x0 + (p & 31);
    const bool in = gy < H && gx < W;
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) {
      const int o = 2 * k + (tid >> 7);
      rg[k] = (in && o < O) ? gb[((long long)o * H + gy) * W + gx] : 0.0f;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int k = 0; k < kYLoads; ++k) {
      const int e = tid + k * kLfThreads, cc = e / kHalo, r2 = e - cc * kHalo, r = r2 / kLfPitch, col = r2 - r * kLfPitch;
      if (e < kYElems) yt[lf_w_y_idx(cc, r, col)] = ry[k];
    }
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) gtl[lf_w_g_idx(2 * k + (tid >> 7), tid & 127)] = rg[k];
  };
  f32x4 run[kPairs][NT];
#pragma unroll
  for (int a = 0; a < kPairs; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n) run[a][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  fetch(t0);
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    __syncthreads();      // the previous tile's readers are done
    put();
    __syncthreads();
    if (t + 1 < t1) fetch(t + 1);      // in flight while tile t is consumed
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      f32x4 acc[kPairs][NT];
#pragma unroll
      for (int a = 0; a < kPairs; ++a)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        float bv[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[n] = gtl[lf_w_b_addr(lane, s, hf, n)];
#pragma unroll
        for (int a = 0; a < kPairs; ++a) {
          const int pr = wave + 4 * a;
          if (pr < kPairsAll) {      // uniform in the wave
            const float av = yt[lf_w_a_addr(lane, s, hf, lf_w_pair_cb(pr), lf_w_pair_tap(pr))];
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[a][n] = lf_mfma(av, bv[n], acc[a][n]);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < kPairs; ++a)
#pragma unroll
        for (int n = 0; n < NT; ++n) run[a][n] += acc[a][n];
    }
  }
  float* pw = partial + ((long long)b * gridDim.x + strip) * 9 * C * OP;
#pragma unroll
  for (int a = 0; a < kPairs; ++a) {
    const int pr = wave + 4 * a;
    if (pr >= kPairsAll) continue;
    const int cb = lf_w_pair_cb(pr), tap = lf_w_pair_tap(pr);
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[((long long)tap * C + c0 + 16 * cb + lf_d_row(lane, r)) * OP + 16 * n + lf_d_col(lane)] = run[a][n][r];
  }
}

// One thread per element e = (tap C + c) OP + o of a partial: dWt[o, c, tap] = the sum over the P = B S partials, in double, in index order
__global__ __launch_bounds__(kLfThreads) void lf_bwd_w_fold_kernel(const float* __restrict__ partial, float* __restrict__ dWt, int P, int C, int O, int OP) {
  const int e = blockIdx.x * kLfThreads + threadIdx.x, n = 9 * C * OP;
  if (e >= n) return;
  const int tap = e / (C * OP), rem = e - tap * C * OP, c = rem / OP, o = rem - c * OP;
  if (o >= O) return;
  double a = 0.0;
#pragma unroll 8
  for (int p = 0; p < P; ++p) a += (double)partial[(long long)p * n + e];
  dWt[((long long)o * C + c) * 9 + tap] = (float)a;
}

// dbias on the vector ALU.  grid (S strips of 8192 pixels, T output triplets, B): partial_b[((b T + t) S + s) 4 + oo]
__global__ __launch_bounds__(kLfThreads) void lf_bwd_b_kernel(const float* __restrict__ g, float* __restrict__ partial_b, int O, int H, int W) {
  __shared__ float lds[4 * 3];
  const int s = blockIdx.x, t = blockIdx.y, b = blockIdx.z, S = gridDim.x, T = gridDim.y;
  const float* gp = g + (long long)b * O * H * W;
  float gbs[3] = {0.0f, 0.0f, 0.0f};
  const int W4 = (W + 3) >> 2;
  const int q0 = s * kLfRounds * kLfThreads + threadIdx.x, di = kLfThreads / W4, dj = kLfThreads - di * W4;
  int i = q0 / W4, jq = q0 - i * W4;
#pragma unroll 1
  for (int r = 0; r < kLfRounds && i < H; ++r) {
    const int c0 = 4 * jq;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int oo = 0; oo < 3; ++oo) gbs[oo] += (c0 + u < W && 3 * t + oo < O) ? gp[((long long)(3 * t + oo) * H + i) * W + c0 + u] : 0.0f;
    i += di;
    jq += dj;
    if (jq >= W4) { jq -= W4; ++i; }
  }
  block_sum(gbs, lds);
  if (threadIdx.x == 0) {
    float* o = partial_b + (((long long)b * T + t) * S + s) * 4;
    o[0] = gbs[0]; o[1] = gbs[1]; o[2] = gbs[2];
  }
}

// One wave per output: lane l takes the entries l, l + 64, .. of the (b, s) list in order, in double; the lanes are added by wave_sum
__global__ __launch_bounds__(64) void lf_bwd_b_fold_kernel(const float* __restrict__ partial_b, float* __restrict__ dbias, int B, int O, int S) {
  const int o = blockIdx.x, lane = threadIdx.x, T = lf_triplets(O), t = o / 3, oo = o - 3 * t;
  double a = 0.0;
  for (int e = lane; e < B * S; e += 64) {
    const int b = e / S, s = e - b * S;
    a += (double)partial_b[(((long long)b * T + t) * S + s) * 4 + oo];
  }
  a = wave_sum(a);
  if (lane == 0) dbias[o] = (float)a;
}

static bool lf_plane_fits(const long long* s, int H, int W) {
  return s[2] >= 0 && s[3] >= 0 && (long long)(H - 1) * s[2] + (long long)(W - 1) * s[3] < (1ll << 31);
}
static int lf_w_slices(int H, int W) {
  const long long runs = (long long)H * ((W + 3) / 4), per = (long long)kLfThreads * kLfRounds;
  return (int)((runs + per - 1) / per);
}
static bool lf_sizes_ok(int B, int C, int O, int H, int W) {
  return B > 0 && C > 0 && O > 0 && H > 0 && W > 0 && O <= kLfMaxO && C >= kLfMinC && C <= kLfMaxC && C % 16 == 0 && B <= 65535 &&
         (long long)H * W < (1ll << 26);
}

#define LF_COMPOSE "; compose F.pad(., (1, 1, 1, 1), mode='replicate') and F.conv2d instead"
#define LF_CHECK_SIZES(who)                                                                                                          \
  SGR_REQUIRE(B > 0 && C > 0 && O > 0 && H > 0 && W > 0, who ": non-positive size");                                                 \
  SGR_SUPPORTED(O <= kLfMaxO, who ": more than 48 output channels" LF_COMPOSE);                                                      \
  SGR_SUPPORTED(C >= kLfMinC && C <= kLfMaxC && C % 16 == 0, who ": the input channels must be a multiple of 16 in 16..256" LF_COMPOSE); \
  SGR_SUPPORTED(B <= 65535, who ": B > 65535");                                                                                      \
  SGR_SUPPORTED((long long)H * W < (1ll << 26), who ": H * W out of range")

}  // namespace sgr

using namespace sgr;

// the two parts of the workspace: the weight partials [B][strips][9][C][OP], then the bias partials [B][T][S][4]
static long long lf_w_strips(int H, int W) {
  const long long tiles = (long long)((W + kLfTW - 1) / kLfTW) * ((H + kLfTHw - 1) / kLfTHw);
  return (tiles + kLfWStrip - 1) / kLfWStrip;
}
static long long lf_w_floats(int B, int C, int O, int H, int W) { return (long long)B * lf_w_strips(H, W) * 9 * C * ((O + 15) / 16 * 16); }

extern "C" long long sgr_light_final_conv_workspace_floats(int B, int C, int O, int H, int W) {
  if (!lf_sizes_ok(B, C, O, H, W)) return 0;
  return lf_w_floats(B, C, O, H, W) + (long long)B * lf_triplets(O) * lf_w_slices(H, W) * 4;
}

extern "C" int sgr_light_final_conv_fwd(const float* y, const float* weight, const float* bias, float* out, int B, int C, int O, int H, int W,
                                        const long long* y_strides, void* stream) {
  SGR_REQUIRE(y && weight && bias && out && y_strides, "sgr_light_final_conv_fwd: NULL tensor");
  LF_CHECK_SIZES("sgr_light_final_conv_fwd");
  SGR_SUPPORTED(lf_plane_fits(y_strides, H, W), "sgr_light_final_conv_fwd: negative or out-of-range plane strides");
  const LfStrides ys{y_strides[0], y_strides[1], y_strides[2], y_strides[3]};
  const int tilesX = (W + kLfTW - 1) / kLfTW, tilesY = (H + kLfTH - 1) / kLfTH, NT = (O + 15) / 16;
  const dim3 grid(tilesX * tilesY, B), block(kLfThreads);
  const size_t lds = sizeof(float) * 2 * ((size_t)kLfKC * kLfPlane + (size_t)9 * kLfKC * lf_wpitch(NT));
  hipStream_t st = (hipStream_t)stream;
  auto fwd = [&](auto N) {
    with_flag(W % 4 == 0 && aligned16({out}), [&](auto VEC) {
      hipLaunchKernelGGL((lf_fwd_kernel<N(), VEC()>), grid, block, lds, st, y, ys, weight, bias, out, C, O, H, W, tilesX);
    });
  };
  if (NT == 1) fwd(Int<1>{}); else if (NT == 2) fwd(Int<2>{}); else fwd(Int<3>{});
  return sgr_check((int)hipGetLastError(), "sgr_light_final_conv_fwd");
}

extern "C" int sgr_light_final_conv_bwd(const float* g, const float* y, const float* weight, float* dy, float* dweight, float* dbias, float* workspace,
                                        int B, int C, int O, int H, int W, const long long* y_strides, void* stream) {
  SGR_REQUIRE(g, "sgr_light_final_conv_bwd: NULL cotangent");
  SGR_REQUIRE(dy || dweight || dbias, "sgr_light_final_conv_bwd: no gradient requested");
  SGR_REQUIRE(!dy || weight, "sgr_light_final_conv_bwd: NULL tensor");
  SGR_REQUIRE(!dweight || (y && y_strides), "sgr_light_final_conv_bwd: NULL tensor");
  SGR_REQUIRE(!(dweight || dbias) || workspace, "sgr_light_final_conv_bwd: NULL tensor");
  LF_CHECK_SIZES("sgr_light_final_conv_bwd");
  SGR_SUPPORTED(!dweight || lf_plane_fits(y_strides, H, W), "sgr_light_final_conv_bwd: negative or out-of-range plane strides");
  hipStream_t st = (hipStream_t)stream;
  if (dy) {
    const int tilesX = (W + kLfTW - 1) / kLfTW, tilesY = (H + kLfTHb - 1) / kLfTHb;
    const dim3 grid(tilesX * tilesY, B, (C + kLfPassC - 1) / kLfPassC), block(kLfThreads);
    with_flag(W % 4 == 0 && aligned16({dy}), [&](auto VEC) {
      hipLaunchKernelGGL(lf_bwd_data_kernel<VEC()>, grid, block, 0, st, g, weight, dy, C, O, H, W, tilesX);
    });
  }
  SGR_SUPPORTED(!dweight || (long long)B * lf_w_strips(H, W) < (1ll << 31), "sgr_light_final_conv_bwd: B * H * W out of range for dweight");
  if (dweight) {
    const LfStrides ys{y_strides[0], y_strides[1], y_strides[2], y_strides[3]};
    const int tilesX = (W + kLfTW - 1) / kLfTW, tiles = tilesX * ((H + kLfTHw - 1) / kLfTHw), strips = (int)lf_w_strips(H, W), NT = (O + 15) / 16;
    // 32 channels at a time where C allows: 18 (channel sub-block, tap) pairs over the four waves
    const bool wide = C % 32 == 0;
    const dim3 grid(strips, C / (wide ? 32 : 16), B);
    auto bwd_w = [&](auto N) {
      choose<Int<2>, Int<1>>(wide, [&](auto CBT) {
        hipLaunchKernelGGL((lf_bwd_w_kernel<N(), CBT()>), grid, dim3(kLfThreads), 0, st, g, y, ys, workspace, C, O, H, W, tilesX, tiles);
      });
    };
    if (NT == 1) bwd_w(Int<1>{}); else if (NT == 2) bwd_w(Int<2>{}); else bwd_w(Int<3>{});
    const int n = 9 * C * 16 * NT;
    hipLaunchKernelGGL(lf_bwd_w_fold_kernel, dim3((n + kLfThreads - 1) / kLfThreads), dim3(kLfThreads), 0, st, workspace, dweight, B * strips, C, O, 16 * NT);
  }
  if (dbias) {
    const int S = lf_w_slices(H, W), T = lf_triplets(O);
    float* partial_b = workspace + lf_w_floats(B, C, O, H, W);
    hipLaunchKernelGGL(lf_bwd_b_kernel, dim3(S, T, B), dim3(kLfThreads), 0, st, g, partial_b, O, H, W);
    hipLaunchKernelGGL(lf_bwd_b_fold_kernel, dim3(O), dim3(64), 0, st, partial_b, dbias, B, O, S);
  }
  return sgr_check((int)hipGetLastError(), "sgr_light_final_conv_bwd");
}
