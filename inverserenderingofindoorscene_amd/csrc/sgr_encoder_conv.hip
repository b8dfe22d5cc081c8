// The encoders' down-sampling layers on gfx950: Conv2d(C -> O, k = 4, stride = 2) behind ReplicationPad2d(1) or ZeroPad2d(1), models.py:93-115,
// 122-126, 213-246, 254-266 (encoder0.conv1 / conv2, encoderLight.preProcess[1] / [5] / conv1), as one operator without the padded copy.
// DESIGN.md section 8i states the contract; the index rule, the tile loops, the LDS addresses, the K orderings and the accumulation
// orders are sgr_encoder_conv.h.
//
// Forward, one launch, an implicit GEMM on v_mfma_f32_16x16x4_f32: a workgroup makes a 32 x 8 tile of up to 64 output planes.  Four input
// channels at a time, the input tile with its halo (66 x 18, through x's strides, the border rule applied on load: a clamp or a zero) goes
// to LDS split into even and odd columns, and the chunk's weights as [k][o], through registers while the previous chunk is consumed; a
// wave keeps 4 M tiles x up to 4 N tiles of accumulators for the chunk and adds them to its running sums on the vector ALU.
// Backward, data, one launch (two in replicate mode), the same instruction: per parity class of the source pixel a GEMM with K = 4 O; a
// wave owns one row parity and both column parities, so a lane holds eight consecutive dx of a row: 128-bit stores where the plane
// allows.  In replicate mode a small vector-ALU launch then writes the first and last row and column again with their extra members: a
// gather as well.  Backward, weights, two launches, the same instruction with the output pixels as K: a workgroup takes one image, 16
// channels, up to 64 outputs and a strip of 25 16 x 4 pixel tiles; the strip's fp32 partial goes to the workspace with ordinary vector
// stores and a second launch folds the partials in double in index order.  Backward, bias, two launches on the vector ALU:
// sgr_final_conv.hip's scheme.  No atomics anywhere: two runs give the same bits.
#include "sgr_encoder_conv_wgrad.inl"      // the shared prelude (kEcThreads, EcStrides, ec_mfma, the CAT flag) and ec_bwd_w_kernel

namespace sgr {

// grid (tiles, B, passes of 64 outputs).  NT: N tiles of the largest pass; a tile past a pass's outputs holds zero weights and is not stored
template <int NT, bool VEC, typename... Tab>
__global__ __launch_bounds__(kEcThreads) void ec_fwd_kernel(const float* __restrict__ x, EcStrides xs, const float* __restrict__ Wt,
                                                            const float* __restrict__ bias, float* __restrict__ out, int C, int O, int H, int W,
                                                            int tilesX, int mode, Tab... tab) {
  constexpr bool CAT = sizeof...(Tab) == 1;
  constexpr int kHalo = kEcRows * kEcCols, kALoads = (kHalo + kEcThreads - 1) / kEcThreads;
  constexpr int kWElems = 16 * kEcKC * kEcPassO, kWLoads = kWElems / kEcThreads;
  __shared__ float at[kEcKC * kEcCHP];
  __shared__ float wl[16 * kEcKC * kEcWP];
  const int Ho = ec_out(H), Wo = ec_out(W);
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int j0 = txi * kEcTW, i0 = tyi * kEcTH;
  const int o0 = blockIdx.z * kEcPassO, nnt = min(kEcPassNT, (O - o0) / 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // what this thread carries from HBM to LDS for every channel: element e = tid + 256 k of the 18 x 66 halo tile
  unsigned off[kALoads];
  int lidx[kALoads], srow[kALoads], scol[kALoads];      // CAT: the source row and column; the offset waits for the channel's strides
#pragma unroll
  for (int k = 0; k < kALoads; ++k) {
    const int e = tid + k * kEcThreads;
    const bool valid = e < kHalo;
    const int r = valid ? e / kEcCols : 0, tc = valid ? e - r * kEcCols : 0;
    const int sr = ec_src(2 * i0 - 1 + r, H, mode), sc = ec_src(2 * j0 - 1 + tc, W, mode);
    if constexpr (CAT) {
      srow[k] = sr;
      scol[k] = sc;
    } else {
      off[k] = (sr < 0 || sc < 0) ? kEcAbsent : (unsigned)sr * (unsigned)xs.h + (unsigned)sc * (unsigned)xs.w;      // fits 31 bits (host check)
    }
    lidx[k] = valid ? ec_fwd_tile_idx(0, r, tc) : -1;
  }
  const float* xb = x + (long long)b * xs.b;
  float ra[kEcKC][kALoads], rw[kWLoads];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int cc = 0; cc < kEcKC; ++cc) {
      const bool live = c0 + cc < C;      // past the last channel: a plane of zeros
      if constexpr (CAT) {
        // the channel is the loop's, so the lookup is uniform across the wave; a chunk may hold channels of two sources
        const EcSource src = ec_source_of(ec_only(tab...), live ? c0 + cc : 0);
        const float* xp = ec_source_plane(src, b, live ? c0 + cc : 0);
#pragma unroll
        for (int k = 0; k < kALoads; ++k) ra[cc][k] = (live && lidx[k] >= 0) ? ec_source_at(src, xp, srow[k], scol[k]) : 0.0f;
      } else {
        const float* xp = xb + (long long)(live ? c0 + cc : 0) * xs.c;
#pragma unroll
        for (int k = 0; k < kALoads; ++k) ra[cc][k] = (live && lidx[k] >= 0 && off[k] != kEcAbsent) ? xp[off[k]] : 0.0f;
      }
    }
    // the chunk's weights of output o are 64 consecutive floats of Wt, [cc][kh][kw] = q; element e = tid + 256 k is (q = e >> 6, o = e & 63)
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kEcThreads, q = e >> 6, o = e & 63;
      rw[k] = (o < 16 * nnt && c0 + (q >> 4) < C) ? Wt[((long long)(o0 + o) * C + c0) * 16 + q] : 0.0f;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int cc = 0; cc < kEcKC; ++cc)
#pragma unroll
      for (int k = 0; k < kALoads; ++k)
        if (lidx[k] >= 0) at[cc * kEcCHP + lidx[k]] = ra[cc][k];
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kEcThreads;
      wl[ec_fwd_w_idx(e >> 6, e & 63)] = rw[k];
    }
  };
  ec_f32x4 run[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) run[m][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int chunks = (C + kEcKC - 1) / kEcKC;
  fetch(0);
#pragma unroll 1
  for (int ci = 0; ci < chunks; ++ci) {
    __syncthreads();      // the previous chunk's readers are done
    put();
    __syncthreads();
    if (ci + 1 < chunks) fetch((ci + 1) * kEcKC);      // in flight while chunk ci is consumed
    ec_f32x4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < kEcSteps; ++s) {
      float a[4], bv[NT];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = at[ec_fwd_a_addr(lane, s, wave, m)];
#pragma unroll
      for (int n = 0; n < NT; ++n) bv[n] = wl[ec_fwd_b_addr(lane, s, n)];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = ec_mfma(a[m], bv[n], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) run[m][n] += acc[m][n];
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    if (n >= nnt) continue;
    const int o = o0 + 16 * n + lf_d_col(lane);
    const float bo = bias[o];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int gy = i0 + ec_fwd_tile_row(wave, m), gx = j0 + ec_fwd_tile_col(m) + lf_d_row(lane, 0);
      if (gy >= Ho || gx >= Wo) continue;
      float* op = out + (((long long)b * O + o) * Ho + gy) * Wo + gx;
      if (VEC) {      // Wo % 4 == 0: a run that starts inside the map ends inside it
        Vec<4> q;
#pragma unroll
        for (int r = 0; r < 4; ++r) q.v[r] = run[m][n][r] + bo;
        *reinterpret_cast<Vec<4>*>(op) = q;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gx + r < Wo) op[r] = run[m][n][r] + bo;
      }
    }
  }
}

// grid (tiles of the (a, b) grid, B, passes of 64 channels).  NT: N tiles of the largest pass; a channel past C has zero weights and is not stored.
// CAT: dx [B, C, H, W] is one source's, and `range` places its channels in Wt
template <int NT, bool VEC, typename... Range>
__global__ __launch_bounds__(kEcThreads) void ec_bwd_data_kernel(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dx, int C,
                                                                 int O, int H, int W, int tilesX, Range... range) {
  int cbase = 0, Ct = C;
  if constexpr (sizeof...(Range) == 1) {
    cbase = ec_only(range...).cbase;
    Ct = ec_only(range...).Ct;
  }
  constexpr int kGElems = kEcDOC * kEcDGPlane, kGLoads = (kGElems + kEcThreads - 1) / kEcThreads;
  constexpr int kWElems = kEcDOC * 16 * kEcDPassC, kWLoads = kWElems / kEcThreads;
  __shared__ float gt[kEcDOC * kEcDGPlane];
  __shared__ float wl[kEcDOC * 16 * kEcDCP];
  const int Ho = ec_out(H), Wo = ec_out(W);
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int b0 = txi * kEcDW, a0 = tyi * kEcDH;
  const int c0p = blockIdx.z * kEcDPassC, ncp = min(kEcDPassC, C - c0p), nnt = (ncp + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ph = wave & 1, m0 = 2 * (wave >> 1);
  // the cotangent tile of a chunk: element e = tid + 256 k of [oc][6][18]; outside the map: zero
  unsigned goff[kGLoads];
  int goc[kGLoads], glidx[kGLoads];
#pragma unroll
  for (int k = 0; k < kGLoads; ++k) {
    const int e = tid + k * kEcThreads;
    const bool valid = e < kGElems;
    const int oc = valid ? e / kEcDGPlane : 0, r2 = e - oc * kEcDGPlane, r = valid ? r2 / kEcDGCols : 0, col = valid ? r2 - r * kEcDGCols : 0;
    const int i = a0 - 1 + r, j = b0 - 1 + col;
    const bool in = i >= 0 && i < Ho && j >= 0 && j < Wo;
    goff[k] = in ? (unsigned)i * (unsigned)Wo + (unsigned)j : kEcAbsent;
    goc[k] = oc;
    glidx[k] = valid ? ec_dx_g_idx(oc, r, col) : -1;
  }
  const float* gb = g + (long long)b * O * Ho * Wo;
  float rg[kGLoads], rw[kWLoads];
  auto fetch = [&](int og) {
#pragma unroll
    for (int k = 0; k < kGLoads; ++k) rg[k] = (glidx[k] >= 0 && goff[k] != kEcAbsent) ? gb[(long long)(og + goc[k]) * Ho * Wo + goff[k]] : 0.0f;
    // element e = tid + 256 k is (oc, tap, c) = (e >> 10, (e >> 6) & 15, e & 63): Wt[o, c0p + c, tap]; a channel >= C: zero
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kEcThreads, oc = e >> 10, tap = (e >> 6) & 15, c = e & 63;
      rw[k] = c < ncp ? Wt[((long long)(og + oc) * Ct + cbase + c0p + c) * 16 + tap] : 0.0f;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int k = 0; k < kGLoads; ++k)
      if (glidx[k] >= 0) gt[glidx[k]] = rg[k];
#pragma unroll
    for (int k = 0; k < kWLoads; ++k) {
      const int e = tid + k * kEcThreads, oc = e >> 10, tap = (e >> 6) & 15, c = e & 63;
      wl[ec_dx_w_idx_of_tap(oc, tap >> 2, tap & 3, c)] = rw[k];
    }
  };
  ec_f32x4 run[2][2][NT];      // [m][pw][n]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int pw = 0; pw < 2; ++pw)
#pragma unroll
      for (int n = 0; n < NT; ++n) run[m][pw][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int groups = O / kEcDOC;      // O is a multiple of 16
  fetch(0);
#pragma unroll 1
  for (int jg = 0; jg < groups; ++jg) {
    __syncthreads();
    put();
    __syncthreads();
    if (jg + 1 < groups) fetch((jg + 1) * kEcDOC);
    ec_f32x4 acc[2][2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int pw = 0; pw < 2; ++pw)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][pw][n] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int oc = 0; oc < kEcDOC; ++oc)
#pragma unroll
      for (int pw = 0; pw < 2; ++pw) {
        const float a0v = gt[ec_dx_a_addr(lane, oc, ph, pw, m0)], a1v = gt[ec_dx_a_addr(lane, oc, ph, pw, m0 + 1)];
        float bv[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[n] = wl[ec_dx_b_addr(lane, oc, ph, pw, n)];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          acc[0][pw][n] = ec_mfma(a0v, bv[n], acc[0][pw][n]);
          acc[1][pw][n] = ec_mfma(a1v, bv[n], acc[1][pw][n]);
        }
      }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int pw = 0; pw < 2; ++pw)
#pragma unroll
        for (int n = 0; n < NT; ++n) run[m][pw][n] += acc[m][pw][n];
  }
  // lane l holds, for channel c, the source columns 2 (b0 + 4 (l >> 4)) .. + 7 of row 2 (a0 + m) + ph: pw interleaves them
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int cl = 16 * n + lf_d_col(lane);
    if (n >= nnt || cl >= ncp) continue;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int h = 2 * (a0 + m0 + m) + ph, w0 = 2 * (b0 + lf_d_row(lane, 0));
      if (h >= H || w0 >= W) continue;
      float* op = dx + (((long long)b * C + c0p + cl) * H + h) * W + w0;
      if (VEC) {      // W % 4 == 0: a run of four that starts inside the map ends inside it
        Vec<4> q0, q1;
        q0.v[0] = run[m][0][n][0]; q0.v[1] = run[m][1][n][0]; q0.v[2] = run[m][0][n][1]; q0.v[3] = run[m][1][n][1];
        q1.v[0] = run[m][0][n][2]; q1.v[1] = run[m][1][n][2]; q1.v[2] = run[m][0][n][3]; q1.v[3] = run[m][1][n][3];
        *reinterpret_cast<Vec<4>*>(op) = q0;
        if (w0 + 4 < W) *reinterpret_cast<Vec<4>*>(op + 4) = q1;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int pw = 0; pw < 2; ++pw)
            if (w0 + 2 * r + pw < W) op[2 * r + pw] = run[m][pw][n][r];
      }
    }
  }
}

// replicate mode: the 2 W + 2 (H - 2) pixels of the first and last row and column of every channel, one thread each.  grid (.., B).
// dx [B, C, H, W]; its channels are cbase .. cbase + C - 1 of the Ct channels of Wt (the single-source kernel: 0 and C)
__device__ __forceinline__ void ec_bwd_data_border_body(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dx, int C, int O, int H,
                                                        int W, int cbase, int Ct) {
  const int ring = 2 * W + 2 * (H - 2);
  const long long e = (long long)blockIdx.x * kEcThreads + threadIdx.x;
  if (e >= (long long)ring * C) return;
  const int c = (int)(e / ring), t = (int)(e - (long long)c * ring), b = blockIdx.y;
  int h, w;
  if (t < W) { h = 0; w = t; }
  else if (t < 2 * W) { h = H - 1; w = t - W; }
  else { const int u = t - 2 * W; h = 1 + (u >> 1); w = (u & 1) ? W - 1 : 0; }
  const int Ho = ec_out(H), Wo = ec_out(W);
  dx[(((long long)b * C + c) * H + h) * W + w] = ec_dx_border(g + (long long)b * O * Ho * Wo, Wt, cbase + c, h, w, Ct, O, H, W);
}
__global__ __launch_bounds__(kEcThreads) void ec_bwd_data_border_kernel(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dx, int C,
                                                                        int O, int H, int W) {
  ec_bwd_data_border_body(g, Wt, dx, C, O, H, W, 0, C);
}
__global__ __launch_bounds__(kEcThreads) void ec_bwd_data_border_cat_kernel(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dx, int C,
                                                                            int O, int H, int W, int cbase, int Ct) {
  ec_bwd_data_border_body(g, Wt, dx, C, O, H, W, cbase, Ct);
}

// One thread per element e = (c 16 + tap) O + o of a partial: dWt[o, c, tap] = the sum over the P = B S partials, in double, in index order
__global__ __launch_bounds__(kEcThreads) void ec_bwd_w_fold_kernel(const float* __restrict__ partial, float* __restrict__ dWt, int P, int C, int O) {
  const int e = blockIdx.x * kEcThreads + threadIdx.x, n = C * 16 * O;
  if (e >= n) return;
  const int ct = e / O, o = e - ct * O;
  double a = 0.0;
#pragma unroll 8
  for (int p = 0; p < P; ++p) a += (double)partial[(long long)p * n + e];
  dWt[(long long)o * C * 16 + ct] = (float)a;
}

// dbias on the vector ALU.  grid (S slices of 8192 pixels, O, B): partial_b[(b O + o) S + s]
__global__ __launch_bounds__(kEcThreads) void ec_bwd_b_kernel(const float* __restrict__ g, float* __restrict__ partial_b, int O, long long HW) {
  __shared__ float lds[4];
  const int s = blockIdx.x, o = blockIdx.y, b = blockIdx.z, S = gridDim.x;
  const float* gp = g + ((long long)b * O + o) * HW;
  float acc[1] = {0.0f};
#pragma unroll 1
  for (int r = 0; r < kEcBRounds; ++r) {
    const long long p0 = 4 * (((long long)s * kEcBRounds + r) * kEcThreads + threadIdx.x);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[0] += p0 + u < HW ? gp[p0 + u] : 0.0f;
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) partial_b[((long long)b * O + o) * S + s] = acc[0];
}

// One wave per output: lane l takes the entries l, l + 64, .. of the (b, s) list in order, in double; the lanes are added by wave_sum
__global__ __launch_bounds__(64) void ec_bwd_b_fold_kernel(const float* __restrict__ partial_b, float* __restrict__ dbias, int B, int O, int S) {
  const int o = blockIdx.x, lane = threadIdx.x;
  double a = 0.0;
  for (int e = lane; e < B * S; e += 64) {
    const int b = e / S, s = e - b * S;
    a += (double)partial_b[((long long)b * O + o) * S + s];
  }
  a = wave_sum(a);
  if (lane == 0) dbias[o] = (float)a;
}

static bool ec_plane_fits(const long long* s, int H, int W) {
  return s[2] >= 0 && s[3] >= 0 && (long long)(H - 1) * s[2] + (long long)(W - 1) * s[3] < (1ll << 31);
}
static bool ec_sizes_ok(int B, int C, int O, int H, int W) {
  return B > 0 && C > 0 && O > 0 && H > 0 && W > 0 && C <= kEcMaxC && O >= kEcMinO && O <= kEcMaxO && O % 16 == 0 && H >= 2 && W >= 2 && B <= 65535 &&
         (long long)ec_out(H) * ec_out(W) < (1ll << 26);
}

#define EC_COMPOSE "; compose F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead"
// `compose`: the composition a refusal names
#define EC_CHECK_SIZES_C(who, compose)                                                                                                           \
  SGR_REQUIRE(B > 0 && C > 0 && O > 0 && H > 0 && W > 0, who ": non-positive size");                                                         \
  SGR_SUPPORTED(pad_mode == kEcReplicate || pad_mode == kEcZeros, who ": pad_mode must be 0 (replicate) or 1 (zeros)" compose);           \
  SGR_SUPPORTED(C <= kEcMaxC, who ": more than 160 input channels (the deeper encoder layers are plain GEMMs with small zero-padded copies)" compose); \
  SGR_SUPPORTED(O >= kEcMinO && O <= kEcMaxO && O % 16 == 0, who ": the output channels must be a multiple of 16 in 16..128" compose);    \
  SGR_SUPPORTED(H >= 2 && W >= 2, who ": H and W must be at least 2" compose);                                                            \
  SGR_SUPPORTED(B <= 65535, who ": B > 65535");                                                                                              \
  SGR_SUPPORTED((long long)ec_out(H) * ec_out(W) < (1ll << 26), who ": Ho * Wo out of range")
#define EC_CHECK_SIZES(who) EC_CHECK_SIZES_C(who, EC_COMPOSE)

}  // namespace sgr

using namespace sgr;

// the two parts of the workspace: the weight partials [B][strips][C][16][O], then the bias partials [B][O][S]
static long long ec_w_strips(int H, int W) {
  const long long tiles = (long long)((ec_out(W) + kEcWW - 1) / kEcWW) * ((ec_out(H) + kEcWH - 1) / kEcWH);
  return (tiles + kEcWStrip - 1) / kEcWStrip;
}
static long long ec_b_slices(int H, int W) { return ((long long)ec_out(H) * ec_out(W) + kEcBSlice - 1) / kEcBSlice; }
static long long ec_w_floats(int B, int C, int O, int H, int W) { return (long long)B * ec_w_strips(H, W) * C * 16 * O; }

extern "C" long long sgr_encoder_conv_workspace_floats(int B, int C, int O, int H, int W) {
  if (!ec_sizes_ok(B, C, O, H, W)) return 0;
  return ec_w_floats(B, C, O, H, W) + (long long)B * O * ec_b_slices(H, W);
}

extern "C" int sgr_encoder_conv_fwd(const float* x, const float* weight, const float* bias, float* out, int B, int C, int O, int H, int W,
                                    const long long* x_strides, int pad_mode, void* stream) {
  SGR_REQUIRE(x && weight && bias && out && x_strides, "sgr_encoder_conv_fwd: NULL tensor");
  EC_CHECK_SIZES("sgr_encoder_conv_fwd");
  SGR_SUPPORTED(ec_plane_fits(x_strides, H, W), "sgr_encoder_conv_fwd: negative or out-of-range plane strides");
  const EcStrides xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
  const int Ho = ec_out(H), Wo = ec_out(W), tilesX = (Wo + kEcTW - 1) / kEcTW, tilesY = (Ho + kEcTH - 1) / kEcTH;
  const dim3 grid(tilesX * tilesY, B, (O + kEcPassO - 1) / kEcPassO), block(kEcThreads);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Wo % 4 == 0 && aligned16({out});
  const int NT = O >= kEcPassO ? kEcPassNT : O / 16;
#define EC_FWD(N, V) hipLaunchKernelGGL((ec_fwd_kernel<N, V>), grid, block, 0, st, x, xs, weight, bias, out, C, O, H, W, tilesX, pad_mode)
#define EC_FWD_N(N) do { if (vec) EC_FWD(N, true); else EC_FWD(N, false); } while (0)
  if (NT == 1) EC_FWD_N(1); else if (NT == 2) EC_FWD_N(2); else if (NT == 3) EC_FWD_N(3); else EC_FWD_N(4);
#undef EC_FWD_N
#undef EC_FWD
  return sgr_check((int)hipGetLastError(), "sgr_encoder_conv_fwd");
}

extern "C" int sgr_encoder_conv_bwd(const float* g, const float* x, const float* weight, float* dx, float* dweight, float* dbias, float* workspace,
                                    int B, int C, int O, int H, int W, const long long* x_strides, int pad_mode, void* stream) {
  SGR_REQUIRE(g, "sgr_encoder_conv_bwd: NULL cotangent");
  SGR_REQUIRE(dx || dweight || dbias, "sgr_encoder_conv_bwd: no gradient requested");
  SGR_REQUIRE(!dx || weight, "sgr_encoder_conv_bwd: NULL tensor");
  SGR_REQUIRE(!dweight || (x && x_strides), "sgr_encoder_conv_bwd: NULL tensor");
  SGR_REQUIRE(!(dweight || dbias) || workspace, "sgr_encoder_conv_bwd: NULL tensor");
  EC_CHECK_SIZES("sgr_encoder_conv_bwd");
  SGR_SUPPORTED(!dweight || ec_plane_fits(x_strides, H, W), "sgr_encoder_conv_bwd: negative or out-of-range plane strides");
  SGR_SUPPORTED(!dx || (long long)H * W < (1ll << 30), "sgr_encoder_conv_bwd: H * W out of range for dx");
  SGR_SUPPORTED(!dweight || (long long)B * ec_w_strips(H, W) < (1ll << 31), "sgr_encoder_conv_bwd: B * Ho * Wo out of range for dweight");
  hipStream_t st = (hipStream_t)stream;
  const int Ho = ec_out(H), Wo = ec_out(W);
  if (dx) {
    // the (a, b) grid of a parity class: ceil(H / 2) x ceil(W / 2)
    const int tilesX = ((W + 1) / 2 + kEcDW - 1) / kEcDW, tilesY = ((H + 1) / 2 + kEcDH - 1) / kEcDH;
    const dim3 grid(tilesX * tilesY, B, (C + kEcDPassC - 1) / kEcDPassC), block(kEcThreads);
    const bool vec = W % 4 == 0 && aligned16({dx});
    const int NT = C >= kEcDPassC ? kEcDPassNT : (C + 15) / 16;
#define EC_DX(N, V) hipLaunchKernelGGL((ec_bwd_data_kernel<N, V>), grid, block, 0, st, g, weight, dx, C, O, H, W, tilesX)
#define EC_DX_N(N) do { if (vec) EC_DX(N, true); else EC_DX(N, false); } while (0)
    if (NT == 1) EC_DX_N(1); else if (NT == 2) EC_DX_N(2); else if (NT == 3) EC_DX_N(3); else EC_DX_N(4);
#undef EC_DX_N
#undef EC_DX
    if (pad_mode == kEcReplicate) {
      const long long n = (long long)(2 * W + 2 * (H - 2)) * C;
      hipLaunchKernelGGL(ec_bwd_data_border_kernel, dim3((unsigned)((n + kEcThreads - 1) / kEcThreads), B), block, 0, st, g, weight, dx, C, O, H, W);
    }
  }
  if (dweight) {
    const EcStrides xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
    const int tilesX = (Wo + kEcWW - 1) / kEcWW, tiles = tilesX * ((Ho + kEcWH - 1) / kEcWH), strips = (int)ec_w_strips(H, W);
    const int opasses = (O + kEcPassO - 1) / kEcPassO, cblocks = (C + kEcWCB - 1) / kEcWCB;
    const int NT = O >= kEcPassO ? kEcPassNT : O / 16, CW = C >= kEcWCB ? kEcWCB / 4 : (C + 3) / 4;
#define EC_W(N, K) hipLaunchKernelGGL((ec_bwd_w_kernel<N, K>), dim3(strips, cblocks * opasses, B), dim3(kEcThreads), 0, st, g, x, xs, workspace, C, O, H, W, tilesX, tiles, opasses, pad_mode)
#define EC_W_N(N) do { if (CW == 1) EC_W(N, 1); else if (CW == 2) EC_W(N, 2); else if (CW == 3) EC_W(N, 3); else EC_W(N, 4); } while (0)
    if (NT == 1) EC_W_N(1); else if (NT == 2) EC_W_N(2); else if (NT == 3) EC_W_N(3); else EC_W_N(4);
#undef EC_W_N
#undef EC_W
    const int n = C * 16 * O;
    hipLaunchKernelGGL(ec_bwd_w_fold_kernel, dim3((n + kEcThreads - 1) / kEcThreads), dim3(kEcThreads), 0, st, workspace, dweight, B * strips, C, O);
  }
  if (dbias) {
    const int S = (int)ec_b_slices(H, W);
    float* partial_b = workspace + ec_w_floats(B, C, O, H, W);
    hipLaunchKernelGGL(ec_bwd_b_kernel, dim3(S, O, B), dim3(kEcThreads), 0, st, g, partial_b, O, (long long)Ho * Wo);
    hipLaunchKernelGGL(ec_bwd_b_fold_kernel, dim3(O), dim3(64), 0, st, partial_b, dbias, B, O, S);
  }
  return sgr_check((int)hipGetLastError(), "sgr_encoder_conv_bwd");
}

// ---- several sources ("several sources") -----------------------------------------------------------------------------
#define EC_CAT_COMPOSE "; compose torch.cat(xs, 1), F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead"

// the checks both entry points share: the list, the channel counts and (where the sources are read) their strides.  C: the summed channels
#define EC_CAT_CHECK_LIST(who)                                                                                                               \
  SGR_SUPPORTED(S >= 1 && S <= kEcMaxSources, who ": the number of sources must be 1 .. 4" EC_CAT_COMPOSE);                                  \
  SGR_REQUIRE(channels, who ": NULL tensor");                                                                                                \
  int C = 0;                                                                                                                                 \
  for (int i = 0; i < S; ++i) {                                                                                                              \
    SGR_REQUIRE(channels[i] > 0, who ": non-positive size");                                                                                 \
    SGR_SUPPORTED(channels[i] <= kEcMaxC, who ": more than 160 input channels (the deeper encoder layers are plain GEMMs with small zero-padded copies)" EC_CAT_COMPOSE); \
    C += channels[i];                                                                                                                        \
  }

static EcSources ec_table(int S, const float* const* xs, const int* channels, const long long* strides) {
  EcSources tab{};
  int first = 0;
  for (int i = 0; i < kEcMaxSources; ++i) {
    if (i < S) {
      tab.s[i] = EcSource{xs[i], strides[4 * i], strides[4 * i + 1], strides[4 * i + 2], strides[4 * i + 3], first};
      first += channels[i];
    } else {
      tab.s[i] = EcSource{nullptr, 0, 0, 0, 0, kEcNoSource};
    }
  }
  return tab;
}

extern "C" int sgr_encoder_conv_cat_fwd(int S, const float* const* xs, const int* channels, const long long* strides, const float* weight, const float* bias,
                                        float* out, int B, int O, int H, int W, int pad_mode, void* stream) {
  EC_CAT_CHECK_LIST("sgr_encoder_conv_cat_fwd");
  SGR_REQUIRE(xs && strides && weight && bias && out, "sgr_encoder_conv_cat_fwd: NULL tensor");
  for (int i = 0; i < S; ++i) SGR_REQUIRE(xs[i], "sgr_encoder_conv_cat_fwd: NULL tensor");
  if (S == 1) return sgr_encoder_conv_fwd(xs[0], weight, bias, out, B, C, O, H, W, strides, pad_mode, stream);      // launch for launch
  EC_CHECK_SIZES_C("sgr_encoder_conv_cat_fwd", EC_CAT_COMPOSE);
  for (int i = 0; i < S; ++i) SGR_SUPPORTED(ec_plane_fits(strides + 4 * i, H, W), "sgr_encoder_conv_cat_fwd: negative or out-of-range plane strides");
  const EcSources tab = ec_table(S, xs, channels, strides);
  const int Ho = ec_out(H), Wo = ec_out(W), tilesX = (Wo + kEcTW - 1) / kEcTW, tilesY = (Ho + kEcTH - 1) / kEcTH;
  const dim3 grid(tilesX * tilesY, B, (O + kEcPassO - 1) / kEcPassO), block(kEcThreads);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Wo % 4 == 0 && aligned16({out});
  const int NT = O >= kEcPassO ? kEcPassNT : O / 16;
#define EC_FWD(N, V) hipLaunchKernelGGL((ec_fwd_kernel<N, V, EcSources>), grid, block, 0, st, (const float*)nullptr, EcStrides{}, weight, bias, out, C, O, H, W, tilesX, pad_mode, tab)
#define EC_FWD_N(N) do { if (vec) EC_FWD(N, true); else EC_FWD(N, false); } while (0)
  if (NT == 1) EC_FWD_N(1); else if (NT == 2) EC_FWD_N(2); else if (NT == 3) EC_FWD_N(3); else EC_FWD_N(4);
#undef EC_FWD_N
#undef EC_FWD
  return sgr_check((int)hipGetLastError(), "sgr_encoder_conv_cat_fwd");
}

extern "C" int sgr_encoder_conv_cat_bwd(int S, const float* g, const float* const* xs, const int* channels, const long long* strides, const float* weight,
                                        float* const* dxs, float* dweight, float* dbias, float* workspace, int B, int O, int H, int W, int pad_mode, void* stream) {
  EC_CAT_CHECK_LIST("sgr_encoder_conv_cat_bwd");
  SGR_REQUIRE(g, "sgr_encoder_conv_cat_bwd: NULL cotangent");
  bool any_dx = false;
  for (int i = 0; dxs && i < S; ++i) any_dx = any_dx || dxs[i];
  SGR_REQUIRE(any_dx || dweight || dbias, "sgr_encoder_conv_cat_bwd: no gradient requested");
  SGR_REQUIRE(!any_dx || weight, "sgr_encoder_conv_cat_bwd: NULL tensor");
  SGR_REQUIRE(!dweight || (xs && strides), "sgr_encoder_conv_cat_bwd: NULL tensor");
  for (int i = 0; dweight && i < S; ++i) SGR_REQUIRE(xs[i], "sgr_encoder_conv_cat_bwd: NULL tensor");
  SGR_REQUIRE(!(dweight || dbias) || workspace, "sgr_encoder_conv_cat_bwd: NULL tensor");
  if (S == 1) {      // launch for launch
    return sgr_encoder_conv_bwd(g, dweight ? xs[0] : nullptr, weight, any_dx ? dxs[0] : nullptr, dweight, dbias, workspace, B, C, O, H, W, strides, pad_mode, stream);
  }
  EC_CHECK_SIZES_C("sgr_encoder_conv_cat_bwd", EC_CAT_COMPOSE);
  for (int i = 0; dweight && i < S; ++i) SGR_SUPPORTED(ec_plane_fits(strides + 4 * i, H, W), "sgr_encoder_conv_cat_bwd: negative or out-of-range plane strides");
  SGR_SUPPORTED(!any_dx || (long long)H * W < (1ll << 30), "sgr_encoder_conv_cat_bwd: H * W out of range for dx");
  SGR_SUPPORTED(!dweight || (long long)B * ec_w_strips(H, W) < (1ll << 31), "sgr_encoder_conv_cat_bwd: B * Ho * Wo out of range for dweight");
  hipStream_t st = (hipStream_t)stream;
  const int Ho = ec_out(H), Wo = ec_out(W);
  // the data gradient: one launch (two in replicate mode) per source that wants one, over that source's channels alone
  for (int i = 0, cbase = 0; i < S; cbase += channels[i], ++i) {
    float* dx = any_dx ? dxs[i] : nullptr;
    if (!dx) continue;
    const int Ci = channels[i];
    const int tilesX = ((W + 1) / 2 + kEcDW - 1) / kEcDW, tilesY = ((H + 1) / 2 + kEcDH - 1) / kEcDH;
    const dim3 grid(tilesX * tilesY, B, (Ci + kEcDPassC - 1) / kEcDPassC), block(kEcThreads);
    const bool vec = W % 4 == 0 && aligned16({dx});
    const int NT = Ci >= kEcDPassC ? kEcDPassNT : (Ci + 15) / 16;
#define EC_DX(N, V) hipLaunchKernelGGL((ec_bwd_data_kernel<N, V, EcRange>), grid, block, 0, st, g, weight, dx, Ci, O, H, W, tilesX, EcRange{cbase, C})
#define EC_DX_N(N) do { if (vec) EC_DX(N, true); else EC_DX(N, false); } while (0)
    if (NT == 1) EC_DX_N(1); else if (NT == 2) EC_DX_N(2); else if (NT == 3) EC_DX_N(3); else EC_DX_N(4);
#undef EC_DX_N
#undef EC_DX
    if (pad_mode == kEcReplicate) {
      const long long n = (long long)(2 * W + 2 * (H - 2)) * Ci;
      hipLaunchKernelGGL(ec_bwd_data_border_cat_kernel, dim3((unsigned)((n + kEcThreads - 1) / kEcThreads), B), block, 0, st, g, weight, dx, Ci, O, H, W, cbase, C);
    }
  }
  if (dweight) {
    const EcSources tab = ec_table(S, xs, channels, strides);
    const int tilesX = (Wo + kEcWW - 1) / kEcWW, tiles = tilesX * ((Ho + kEcWH - 1) / kEcWH), strips = (int)ec_w_strips(H, W);
    const int opasses = (O + kEcPassO - 1) / kEcPassO, cblocks = (C + kEcWCB - 1) / kEcWCB;
    const int NT = O >= kEcPassO ? kEcPassNT : O / 16, CW = C >= kEcWCB ? kEcWCB / 4 : (C + 3) / 4;
    ec_launch_w_cat(dim3(strips, cblocks * opasses, B), st, NT, CW, g, tab, workspace, C, O, H, W, tilesX, tiles, opasses, pad_mode);
    const int n = C * 16 * O;
    hipLaunchKernelGGL(ec_bwd_w_fold_kernel, dim3((n + kEcThreads - 1) / kEcThreads), dim3(kEcThreads), 0, st, workspace, dweight, B * strips, C, O);
  }
  if (dbias) {
    const int Sl = (int)ec_b_slices(H, W);
    float* partial_b = workspace + ec_w_floats(B, C, O, H, W);
    hipLaunchKernelGGL(ec_bwd_b_kernel, dim3(Sl, O, B), dim3(kEcThreads), 0, st, g, partial_b, O, (long long)Ho * Wo);
    hipLaunchKernelGGL(ec_bwd_b_fold_kernel, dim3(O), dim3(64), 0, st, partial_b, dbias, B, O, Sl);
  }
  return sgr_check((int)hipGetLastError(), "sgr_encoder_conv_cat_bwd");
}
