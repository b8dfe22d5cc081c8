// The BRDF decoders' last step on gfx950: x_orig = dconvFinal(dpadFinal(dx6)), models.py:155-156, 187 -- ReplicationPad2d(1) followed by
// Conv2d(C -> 3, k = 3, stride 1), as one operator without the padded copy, optionally with GroupNorm + ReLU of models.py:183 as the load
// prologue, so that dx6 = relu(dgn6(x)) is never written either.  DESIGN.md section 8g states the contract; the index rule and the
// accumulation orders are sgr_final_conv.h.
//
// Forward, one launch: a workgroup makes a 64 x 32 tile of the three output planes.  Input channel by input channel the tile and its halo
// (66 x 34, 1.10 x the tile) go from HBM to LDS -- through x's strides, clamped at the map's border, which is the pad, and through the
// prologue -- while the previous channel is consumed from the other buffer; a thread owns 4 columns of 2 rows and keeps their 24 running
// sums.  The weights [C][3][3][3] sit in LDS for the whole kernel and reach every lane as a broadcast.
// Backward, data, one launch: the cotangent's 64 x 16 tile (3 channels, with halo) in LDS, a thread gathers the 27 per-tap sums of each of
// its 4 pixels once and then streams the C planes of dy out, 27 fmaf per element and a 128-bit store where the layout allows.
// Backward, weights and bias, two launches: a workgroup takes a strip of one (image, input channel) plane -- a thread 8 runs of 4 pixels
// -- with y recomputed from x by the prologue, leaves 27 fp32 sums (and, for channel 0, the three of dbias) in the workspace, and one wave
// per weight folds the partials in double in index order.  No atomics anywhere: two runs give the same bits.
#include "sgr_final_conv.h"
#include "sgr_gn_stage.h"      // gn_xhat, gn_pre: the prologue is group_norm_relu's arithmetic, bit for bit
#include "sgr_launch.h"
#include "sgr_reduce.h"        // block_sum, wave_sum, Vec<4>, aligned16

namespace sgr {

constexpr int kFcThreads = 256;
constexpr int kFcTW = 64;                     // tile width: 16 threads x 4 columns
constexpr int kFcTH = 32;                     // forward tile height: 16 threads x 2 rows
constexpr int kFcTHb = 16;                    // backward (data) tile height: 16 threads x 1 row
constexpr int kFcLW = kFcTW + 2;              // loaded columns of a tile row
constexpr int kFcPitch = 68;                  // LDS row pitch in floats: a multiple of 4, so a thread's window starts on 16 bytes
constexpr int kFcTile = (kFcTH + 2) * kFcPitch;       // floats of one forward buffer
constexpr int kFcTileB = (kFcTHb + 2) * kFcPitch;     // floats of one cotangent plane's tile
constexpr int kFcLoads = ((kFcTH + 2) * kFcLW + kFcThreads - 1) / kFcThreads;      // 9 elements per thread and channel
constexpr int kFcRounds = 8;                  // runs of four pixels per thread in the weights pass

struct FcStrides { long long b, c, h, w; };

// wl[c * 28 + (o * 9 + kh * 3 + kw)] = Wt[o, c, kh, kw]
__device__ __forceinline__ void fc_stage_weights(const float* __restrict__ Wt, float* __restrict__ wl, int C) {
  for (int idx = threadIdx.x; idx < C * 27; idx += kFcThreads) {
    const int c = idx / 27, r = idx - c * 27, o = r / 9, k = r - 9 * o;
    wl[c * kFcWPitch + r] = Wt[((long long)o * C + c) * 9 + k];
  }
}
// the 27 weights of channel c into registers: seven 128-bit broadcasts
__device__ __forceinline__ void fc_channel_weights(const float* __restrict__ wl, int c, float (&w)[28]) {
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const Vec<4> t = *reinterpret_cast<const Vec<4>*>(wl + c * kFcWPitch + 4 * q);
#pragma unroll
    for (int u = 0; u < 4; ++u) w[4 * q + u] = t.v[u];
  }
}

template <bool PROLOGUE, bool VEC>
__global__ __launch_bounds__(kFcThreads) void fc_fwd_kernel(const float* __restrict__ x, FcStrides xs, const float* __restrict__ Wt,
                                                            const float* __restrict__ bias, const float* __restrict__ gnw, const float* __restrict__ gnb,
                                                            const float* __restrict__ stats, float* __restrict__ out, int C, int cpg, int H, int W,
                                                            int tilesX) {
  extern __shared__ float4 fc_smem4[];
  float* wl = reinterpret_cast<float*>(fc_smem4);      // [C][28]
  float* tile = wl + C * kFcWPitch;                    // [2][kFcTile]
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int x0 = txi * kFcTW, y0 = tyi * kFcTH;
  const int G = PROLOGUE ? C / cpg : 1;
  fc_stage_weights(Wt, wl, C);
  // what this thread carries from HBM to LDS for every channel: element e = t + 256 k of the 34 x 66 halo tile
  unsigned off[kFcLoads];
  int lidx[kFcLoads];
#pragma unroll
  for (int k = 0; k < kFcLoads; ++k) {
    const int e = threadIdx.x + k * kFcThreads;
    const bool valid = e < (kFcTH + 2) * kFcLW;
    const int r = valid ? e / kFcLW : 0, col = valid ? e - r * kFcLW : 0;
    off[k] = (unsigned)fc_cl(y0 - 1 + r, H) * (unsigned)xs.h + (unsigned)fc_cl(x0 - 1 + col, W) * (unsigned)xs.w;      // fits 31 bits (host check)
    lidx[k] = valid ? r * kFcPitch + col : -1;
  }
  const float* xb = x + (long long)b * xs.b;
  float regs[kFcLoads];
  auto fetch = [&](int c) {
    const float* xp = xb + (long long)c * xs.c;
#pragma unroll
    for (int k = 0; k < kFcLoads; ++k) regs[k] = lidx[k] >= 0 ? xp[off[k]] : 0.0f;
  };
  auto put = [&](int c) {
    float* dst = tile + (c & 1) * kFcTile;
    float mh = 0.0f, ml = 0.0f, rstd = 1.0f, wc = 1.0f, bc = 0.0f;
    if (PROLOGUE) {
      const float* st = stats + 4 * ((long long)b * G + c / cpg);
      mh = st[0]; ml = st[1]; rstd = st[2];
      wc = gnw[c]; bc = gnb[c];
    }
#pragma unroll
    for (int k = 0; k < kFcLoads; ++k)
      if (lidx[k] >= 0) dst[lidx[k]] = PROLOGUE ? fmaxf(gn_pre(gn_xhat(regs[k], mh, ml, rstd), wc, bc), 0.0f) : regs[k];
  };
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[2][4][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int o = 0; o < 3; ++o) acc[r][u][o] = 0.0f;
  fetch(0);
  put(0);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    if (c + 1 < C) fetch(c + 1);      // in flight while channel c is consumed
    const float* t = tile + (c & 1) * kFcTile + (2 * ty) * kFcPitch + 4 * tx;
    float v[4][6];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const Vec<4> a = *reinterpret_cast<const Vec<4>*>(t + r * kFcPitch);
      const float2 e = *reinterpret_cast<const float2*>(t + r * kFcPitch + 4);
      v[r][0] = a.v[0]; v[r][1] = a.v[1]; v[r][2] = a.v[2]; v[r][3] = a.v[3]; v[r][4] = e.x; v[r][5] = e.y;
    }
    float w[28];
    fc_channel_weights(wl, c, w);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v9[9] = {v[r][u], v[r][u + 1], v[r][u + 2], v[r + 1][u], v[r + 1][u + 1], v[r + 1][u + 2], v[r + 2][u], v[r + 2][u + 1], v[r + 2][u + 2]};
#pragma unroll
        for (int o = 0; o < 3; ++o) acc[r][u][o] += fc_taps(w + 9 * o, v9);
      }
    if (c + 1 < C) put(c + 1);        // the other buffer: channel c - 1's readers passed the barrier below
    __syncthreads();
  }
  const int gx = x0 + 4 * tx;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int gy = y0 + 2 * ty + r;
    if (gy >= H || gx >= W) continue;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      const float bo = bias[o];
      float* op = out + (((long long)b * kFcOut + o) * H + gy) * W + gx;
      if (VEC) {      // W % 4 == 0: a run that starts inside the map ends inside it
        Vec<4> q;
#pragma unroll
        for (int u = 0; u < 4; ++u) q.v[u] = acc[r][u][o] + bo;
        *reinterpret_cast<Vec<4>*>(op) = q;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (gx + u < W) op[u] = acc[r][u][o] + bo;
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kFcThreads) void fc_bwd_data_kernel(const float* __restrict__ g, const float* __restrict__ Wt, float* __restrict__ dy, int C,
                                                                 int H, int W, int tilesX) {
  extern __shared__ float4 fc_smem4[];
  float* wl = reinterpret_cast<float*>(fc_smem4);      // [C][28]
  float* gt = wl + C * kFcWPitch;                      // [3][kFcTileB]
  const int b = blockIdx.y, tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int x0 = txi * kFcTW, y0 = tyi * kFcTHb;
  fc_stage_weights(Wt, wl, C);
  constexpr int kPlane = (kFcTHb + 2) * kFcLW;
  for (int e = threadIdx.x; e < kFcOut * kPlane; e += kFcThreads) {
    const int o = e / kPlane, r2 = e - o * kPlane, r = r2 / kFcLW, col = r2 - r * kFcLW;
    gt[o * kFcTileB + r * kFcPitch + col] = g[(((long long)b * kFcOut + o) * H + fc_cl(y0 - 1 + r, H)) * W + fc_cl(x0 - 1 + col, W)];
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int h = y0 + ty, w0 = x0 + 4 * tx;
  // a thread outside the map works on the nearest pixel inside it and stores nothing: every LDS index below stays inside the tile
  const FcPairs rows = fc_pairs(fc_cl(h, H), H);
  float G[4][3][9];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const FcPairs cols = fc_pairs(fc_cl(w0 + u, W), W);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float gv[3][3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) gv[p][q] = gt[o * kFcTileB + (rows.i[p] - y0 + 1) * kFcPitch + (cols.i[q] - x0 + 1)];
      fc_gather_taps(gv, rows, cols, G[u][o]);
    }
  }
  if (h >= H || w0 >= W) return;      // no barrier below
  float* op = dy + ((long long)b * C * H + h) * W + w0;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    float w[28];
    fc_channel_weights(wl, c, w);
    Vec<4> d;
#pragma unroll
    for (int u = 0; u < 4; ++u) d.v[u] = fc_dy(w, G[u]);
    float* o = op + (long long)c * H * W;
    if (VEC) {
      *reinterpret_cast<Vec<4>*>(o) = d;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (w0 + u < W) o[u] = d.v[u];
    }
  }
}

// partial_w[((b C + c) S + s) 28 + o 9 + kh 3 + kw], partial_b[(b S + s) 4 + o] (from the workgroups of channel 0).  want_w == 0: only dbias,
// launched with one channel.
template <bool PROLOGUE>
__global__ __launch_bounds__(kFcThreads) void fc_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ x, FcStrides xs,
                                                              const float* __restrict__ gnw, const float* __restrict__ gnb, const float* __restrict__ stats,
                                                              float* __restrict__ partial_w, float* __restrict__ partial_b, int C, int cpg, int H, int W,
                                                              int want_w) {
  __shared__ float lds[4 * 27];
  const int s = blockIdx.x, c = blockIdx.y, b = blockIdx.z, S = gridDim.x;
  float mh = 0.0f, ml = 0.0f, rstd = 1.0f, wc = 1.0f, bc = 0.0f;
  if (PROLOGUE && want_w) {
    const float* st = stats + 4 * ((long long)b * (C / cpg) + c / cpg);
    mh = st[0]; ml = st[1]; rstd = st[2];
    wc = gnw[c]; bc = gnb[c];
  }
  const float* xp = want_w ? x + (long long)b * xs.b + (long long)c * xs.c : nullptr;
  const float* gp = g + (long long)b * kFcOut * H * W;
  const unsigned sh = (unsigned)xs.h, sw = (unsigned)xs.w;      // in-plane offsets fit 31 bits (host check)
  float acc[27], gb[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0f;
  const int W4 = (W + 3) >> 2;
  const int q0 = s * kFcRounds * kFcThreads + threadIdx.x, di = kFcThreads / W4, dj = kFcThreads - di * W4;
  int i = q0 / W4, jq = q0 - i * W4;
#pragma unroll 1
  for (int r = 0; r < kFcRounds && i < H; ++r) {
    const int c0 = 4 * jq;
    float g3[4][3];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int o = 0; o < 3; ++o) g3[u][o] = c0 + u < W ? gp[((long long)o * H + i) * W + c0 + u] : 0.0f;      // past the row: exact zeros
    if (want_w) {
      const unsigned ro[3] = {(unsigned)fc_cl(i - 1, H) * sh, (unsigned)i * sh, (unsigned)fc_cl(i + 1, H) * sh};
      float v[3][6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const unsigned co = (unsigned)fc_cl(c0 - 1 + k, W) * sw;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float t = xp[ro[a] + co];
          v[a][k] = PROLOGUE ? fmaxf(gn_pre(gn_xhat(t, mh, ml, rstd), wc, bc), 0.0f) : t;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v9[9] = {v[0][u], v[0][u + 1], v[0][u + 2], v[1][u], v[1][u + 1], v[1][u + 2], v[2][u], v[2][u + 1], v[2][u + 2]};
        fc_dw_pixel(g3[u], v9, acc);
      }
    }
    if (c == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int o = 0; o < 3; ++o) gb[o] += g3[u][o];
    }
    i += di;
    jq += dj;
    if (jq >= W4) { jq -= W4; ++i; }
  }
  if (want_w) {
    block_sum(acc, lds);
    if (threadIdx.x == 0) {
      float* o = partial_w + (((long long)b * C + c) * S + s) * kFcWPitch;
#pragma unroll
      for (int k = 0; k < 27; ++k) o[k] = acc[k];
    }
  }
  if (c == 0 && partial_b) {      // uniform in the workgroup
    __syncthreads();
    block_sum(gb, lds);
    if (threadIdx.x == 0) {
      float* o = partial_b + ((long long)b * S + s) * 4;
      o[0] = gb[0]; o[1] = gb[1]; o[2] = gb[2];
    }
  }
}

// One wave per job.  Jobs [0, nw): dWt[job] (job = (o C + c) 9 + k, the layout of Wt) = the sum over (b, s) of its partials; jobs
// [nw, nw + 3): dbias.  Lane l takes the entries l, l + 64, .. of the (b, s) list in order, in double; the lanes are added by wave_sum.
__global__ __launch_bounds__(64) void fc_bwd_fold_kernel(const float* __restrict__ partial_w, const float* __restrict__ partial_b, float* __restrict__ dWt,
                                                         float* __restrict__ dbias, int B, int C, int S, int nw) {
  const int job = blockIdx.x, lane = threadIdx.x;
  double a = 0.0;
  if (job < nw) {
    const int o = job / (C * 9), rem = job - o * C * 9, c = rem / 9, k = rem - 9 * c;
    for (int e = lane; e < B * S; e += 64) {
      const int b = e / S, s = e - b * S;
      a += (double)partial_w[(((long long)b * C + c) * S + s) * kFcWPitch + 9 * o + k];
    }
    a = wave_sum(a);
    if (lane == 0) dWt[job] = (float)a;
  } else {
    const int o = job - nw;
    for (int e = lane; e < B * S; e += 64) a += (double)partial_b[(long long)e * 4 + o];
    a = wave_sum(a);
    if (lane == 0) dbias[o] = (float)a;
  }
}

static bool fc_plane_fits(const long long* s, int H, int W) {
  return s[2] >= 0 && s[3] >= 0 && (long long)(H - 1) * s[2] + (long long)(W - 1) * s[3] < (1ll << 31);
}
static int fc_w_slices(int H, int W) {
  const long long runs = (long long)H * ((W + 3) / 4), per = (long long)kFcThreads * kFcRounds;
  return (int)((runs + per - 1) / per);
}
static size_t fc_lds_bytes(int C, int tile_floats) { return sizeof(float) * ((size_t)C * kFcWPitch + tile_floats); }

#define FC_COMPOSE "; compose F.pad(., (1, 1, 1, 1), mode='replicate') and F.conv2d instead"
#define FC_CHECK_SIZES(who)                                                                                             \
  SGR_REQUIRE(B > 0 && C > 0 && O > 0 && H > 0 && W > 0, who ": non-positive size");                                    \
  SGR_SUPPORTED(O == kFcOut, who ": the output channels must be exactly 3 (dconvFinal)" FC_COMPOSE);                    \
  SGR_SUPPORTED(C <= kFcMaxC, who ": more than 256 input channels do not fit the weight tile" FC_COMPOSE);              \
  SGR_SUPPORTED(B <= 65535, who ": B > 65535");                                                                         \
  SGR_SUPPORTED((long long)H * W < (1ll << 26), who ": H * W out of range")

}  // namespace sgr

using namespace sgr;

extern "C" long long sgr_final_conv_workspace_floats(int B, int C, int O, int H, int W) {
  if (!(B > 0 && C > 0 && H > 0 && W > 0) || O != kFcOut || C > kFcMaxC || B > 65535 || (long long)H * W >= (1ll << 26)) return 0;
  const long long S = fc_w_slices(H, W);
  return (long long)B * C * S * kFcWPitch + (long long)B * S * 4;
}

extern "C" int sgr_final_conv_fwd(const float* x, const float* weight, const float* bias, const float* gn_weight, const float* gn_bias, const float* stats,
                                  float* out, int B, int C, int O, int G, int H, int W, const long long* x_strides, void* stream) {
  SGR_REQUIRE(x && weight && bias && out && x_strides, "sgr_final_conv_fwd: NULL tensor");
  SGR_REQUIRE(!stats || (gn_weight && gn_bias), "sgr_final_conv_fwd: the prologue needs the GroupNorm weight and bias with the statistics");
  FC_CHECK_SIZES("sgr_final_conv_fwd");
  SGR_REQUIRE(!stats || (G > 0 && C % G == 0), "sgr_final_conv_fwd: C is not a multiple of num_groups");
  SGR_SUPPORTED(fc_plane_fits(x_strides, H, W), "sgr_final_conv_fwd: negative or out-of-range plane strides");
  const FcStrides xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
  const int tilesX = (W + kFcTW - 1) / kFcTW, tilesY = (H + kFcTH - 1) / kFcTH, cpg = stats ? C / G : C;
  const dim3 grid(tilesX * tilesY, B), block(kFcThreads);
  const size_t lds = fc_lds_bytes(C, 2 * kFcTile);
  hipStream_t st = (hipStream_t)stream;
  with_flag(stats != nullptr, [&](auto PROLOGUE) {
    with_flag(W % 4 == 0 && aligned16({out}), [&](auto VEC) {
      hipLaunchKernelGGL((fc_fwd_kernel<PROLOGUE(), VEC()>), grid, block, lds, st, x, xs, weight, bias, gn_weight, gn_bias, stats, out, C, cpg, H, W, tilesX);
    });
  });
  return sgr_check((int)hipGetLastError(), "sgr_final_conv_fwd");
}

extern "C" int sgr_final_conv_bwd(const float* g, const float* x, const float* weight, const float* gn_weight, const float* gn_bias, const float* stats,
                                  float* dy, float* dweight, float* dbias, float* workspace, int B, int C, int O, int G, int H, int W,
                                  const long long* x_strides, void* stream) {
  SGR_REQUIRE(g, "sgr_final_conv_bwd: NULL cotangent");
  SGR_REQUIRE(dy || dweight || dbias, "sgr_final_conv_bwd: no gradient requested");
  SGR_REQUIRE(!dy || weight, "sgr_final_conv_bwd: NULL tensor");
  SGR_REQUIRE(!dweight || (x && x_strides), "sgr_final_conv_bwd: NULL tensor");
  SGR_REQUIRE(!(dweight || dbias) || workspace, "sgr_final_conv_bwd: NULL tensor");
  SGR_REQUIRE(!(dweight && stats) || (gn_weight && gn_bias), "sgr_final_conv_bwd: the prologue needs the GroupNorm weight and bias with the statistics");
  FC_CHECK_SIZES("sgr_final_conv_bwd");
  SGR_REQUIRE(!(dweight && stats) || (G > 0 && C % G == 0), "sgr_final_conv_bwd: C is not a multiple of num_groups");
  SGR_SUPPORTED(!dweight || fc_plane_fits(x_strides, H, W), "sgr_final_conv_bwd: negative or out-of-range plane strides");
  hipStream_t st = (hipStream_t)stream;
  if (dy) {
    const int tilesX = (W + kFcTW - 1) / kFcTW, tilesY = (H + kFcTHb - 1) / kFcTHb;
    const dim3 grid(tilesX * tilesY, B), block(kFcThreads);
    const size_t lds = fc_lds_bytes(C, kFcOut * kFcTileB);
    with_flag(W % 4 == 0 && aligned16({dy}), [&](auto VEC) {
      hipLaunchKernelGGL(fc_bwd_data_kernel<VEC()>, grid, block, lds, st, g, weight, dy, C, H, W, tilesX);
    });
  }
  if (dweight || dbias) {
    const int S = fc_w_slices(H, W), want_w = dweight != nullptr, cpg = (want_w && stats) ? C / G : C;
    float* partial_w = workspace;
    float* partial_b = dbias ? workspace + (long long)B * C * S * kFcWPitch : nullptr;
    const FcStrides xs = want_w ? FcStrides{x_strides[0], x_strides[1], x_strides[2], x_strides[3]} : FcStrides{0, 0, 0, 0};
    const dim3 grid(S, want_w ? C : 1, B);
    with_flag(want_w && stats, [&](auto PROLOGUE) {
      hipLaunchKernelGGL(fc_bwd_w_kernel<PROLOGUE()>, grid, dim3(kFcThreads), 0, st, g, x, xs, gn_weight, gn_bias, stats, partial_w, partial_b, C, cpg, H, W, want_w);
    });
    const int nw = want_w ? kFcOut * C * 9 : 0;
    hipLaunchKernelGGL(fc_bwd_fold_kernel, dim3(nw + (dbias ? 3 : 0)), dim3(64), 0, st, partial_w, partial_b, dweight, dbias, B, C, S, nw);
  }
  return sgr_check((int)hipGetLastError(), "sgr_final_conv_bwd");
}
