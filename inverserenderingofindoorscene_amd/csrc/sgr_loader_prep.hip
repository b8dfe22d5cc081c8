// The synthetic loader's batch preparation on gfx950: the per-sample arithmetic of dataLoader.BatchLoader.__getitem__ (dataLoader.py:118-154,
// 251-259, 286-310) between what the host has decoded and resized and the `dataBatch` tensors, for a whole batch.  Inputs, so no adjoints.
//
//   masks     seg_u8 [bn,H,W,Cin] (channel 0) -> segArea, segEnv, segObj [bn,1,H,W]; segObj eroded by a 7 x 7 box, outside = set      :120-131
//   scale     v[b] = element k of sort(hdr * seg), a radix select, one workgroup per image; scale[b] = num[b] / max(v, 0.1)            :251-257
//   im        clip(scale hdr, 0, 1), HWC -> CHW with the channel axis reversed                                                          :247-248, 258-259
//   maps      albedo = seg(u8)^2.2, normal = n / sqrt(max(|n|^2, 1e-5)), rough = channel 0, HWC uint8 -> CHW fp32                       :139-147
//   envmaps   [bn, R 16, C 32, 3] -> [bn,3,R,C,eh,ew]: a transpose, for 8 x 16 a 2 x 2 block mean, times scale[b]                      :153-154, 298-307
//
// Nothing reduces across workgroups and no float is added atomically (the select counts with integer LDS atomics), so two runs give the
// same bits and image b does not depend on the batch around it; nothing visits the host, so the calls capture in a HIP graph.
// DESIGN.md section 8l states the contracts; sgr_loader_prep.h holds the decisions the host build shares.
#include "sgr_launch.h"
#include "sgr_loader_prep.h"
#include "sgr_reduce.h"      // Vec / ldv / stv, aligned16

namespace sgr {

using namespace lp;

constexpr int kLThreads = 256;

// ---- masks ----------------------------------------------------------------------------------------------------------------------------
constexpr int kMTileH = 16, kMTileW = 64;      // outputs of a workgroup: four consecutive pixels of a row per thread
constexpr int kMHaloH = kMTileH + 2 * kErodeR, kMHaloW = kMTileW + 2 * kErodeR, kMPitch = 72;

template <int V, bool ERODE>
__global__ __launch_bounds__(kLThreads) void lp_masks(const unsigned char* __restrict__ seg, float* __restrict__ area, float* __restrict__ env, float* __restrict__ obj,
                                                      int H, int W, int Cin) {
  __shared__ unsigned char tile[kMHaloH * kMPitch];      // the mask bits; bit 0 (kObj) is what the erosion reads
  __shared__ unsigned char hrow[kMHaloH * kMTileW];      // the AND of 7 along x
  const int b = blockIdx.z, y0 = blockIdx.y * kMTileH, x0 = blockIdx.x * kMTileW;
  const unsigned char* sb = seg + (size_t)b * H * W * Cin;
  for (int i = threadIdx.x; i < kMHaloH * kMHaloW; i += kLThreads) {
    const int ty = i / kMHaloW, tx = i - ty * kMHaloW, y = y0 + ty - kErodeR, x = x0 + tx - kErodeR;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    tile[ty * kMPitch + tx] = in ? (unsigned char)seg_bits(sb[((size_t)y * W + x) * Cin]) : (unsigned char)kObj;      // border_value=1
  }
  __syncthreads();
  if (ERODE) {
    for (int i = threadIdx.x; i < kMHaloH * kMTileW; i += kLThreads) {
      const int ty = i / kMTileW, tx = i - ty * kMTileW;
      hrow[i] = (unsigned char)and7(tile + ty * kMPitch + tx, 1);
    }
    __syncthreads();
  }
  const int ly = threadIdx.x / (kMTileW / 4), lx = (threadIdx.x % (kMTileW / 4)) * 4, y = y0 + ly, x = x0 + lx;
  if (y >= H || x >= W) return;
  const size_t at = ((size_t)b * H + y) * W + x;
  Vec<4> a, e, o;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int bits = tile[(ly + kErodeR) * kMPitch + lx + u + kErodeR];
    a.v[u] = (bits & kArea) ? 1.0f : 0.0f;
    e.v[u] = (bits & kEnv) ? 1.0f : 0.0f;
    o.v[u] = (ERODE ? and7(hrow + ly * kMTileW + lx + u, kMTileW) : (bits & kObj)) ? 1.0f : 0.0f;
    if (V == 1 && x + u < W) {
      area[at + u] = a.v[u];
      env[at + u] = e.v[u];
      obj[at + u] = o.v[u];
    }
  }
  if (V == 4) {      // W % 4 == 0: the four pixels are inside the row
    stv<4>(area, at, a);
    stv<4>(env, at, e);
    stv<4>(obj, at, o);
  }
}

// ---- the order statistic behind scaleHdr --------------------------------------------------------------------------------------------
constexpr int kSThreads = 1024;

// One workgroup per image.  Four passes of eight bits over the keys of hdr * seg: a histogram of the pass's digit over the keys that carry
// the prefix found so far, then thread 0 walks the 256 counts to the bucket that holds rank k.  A thread folds a run of equal digits into
// one atomic, so an image of one value (or a masked background of zeros) does not serialise on one LDS word.
__global__ __launch_bounds__(kSThreads) void lp_select(const float* __restrict__ hdr, const unsigned char* __restrict__ seg, const float* __restrict__ num,
                                                       float* __restrict__ scale, float* __restrict__ v_out, int HW, int Cin, unsigned k) {
  __shared__ unsigned hist[kBuckets];
  __shared__ unsigned s_prefix, s_rank;
  const int b = blockIdx.x;
  const float* hb = hdr + (size_t)b * HW * 3;
  const unsigned char* sb = seg + (size_t)b * HW * Cin;
  if (threadIdx.x == 0) {
    s_prefix = 0;
    s_rank = k;
  }
  for (int pass = 0; pass < kPasses; ++pass) {
    if (threadIdx.x < kBuckets) hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    int last = -1;
    unsigned cnt = 0;
    for (int p = threadIdx.x; p < HW; p += kSThreads) {
      const float sv = byte_seg(sb[(size_t)p * Cin]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t key = key_of(hb[(size_t)p * 3 + c] * sv);
        if (!in_prefix(key, prefix, pass)) continue;
        const int d = digit_of(key, pass);
        if (d == last) {
          ++cnt;
        } else {
          if (cnt) atomicAdd(&hist[last], cnt);
          last = d;
          cnt = 1;
        }
      }
    }
    if (cnt) atomicAdd(&hist[last], cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned rank = s_rank;
      const int d = pick_bucket(hist, rank);
      s_rank = rank;
      s_prefix = (pass ? prefix << kRadixBits : 0u) | (unsigned)d;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = float_of(s_prefix);
    v_out[b] = v;
    scale[b] = (num ? num[b] : (float)(0.95 - 0.05)) / fmaxf(v, 0.1f);      // dataLoader.py:255 | :257
  }
}

// ---- im: HWC -> CHW, channels reversed ----------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kLThreads) void lp_im(const float* __restrict__ hdr, const float* __restrict__ scale, float* __restrict__ im, int HW) {
  const int b = blockIdx.y;
  const float s = scale[b];
  const float* hb = hdr + (size_t)b * HW * 3;
  float* ob = im + (size_t)b * HW * 3;
  for (int o = (blockIdx.x * kLThreads + threadIdx.x) * V; o < HW; o += gridDim.x * kLThreads * V) {
    float f[3 * V];
    if (V == 4) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const Vec<4> x = ldv<4>(hb, (size_t)o * 3 + 4 * q);
#pragma unroll
        for (int u = 0; u < 4; ++u) f[4 * q + u] = x.v[u];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) f[q] = hb[(size_t)o * 3 + q];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vec<V> x;
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = fminf(fmaxf(s * f[3 * u + c], 0.0f), 1.0f);
      stv<V>(ob, (size_t)(2 - c) * HW + o, x);      // im[::-1]
    }
  }
}

// ---- albedo / normal / rough: HWC uint8 -> CHW fp32 ------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kLThreads) void lp_brdf(const unsigned char* __restrict__ a8, const unsigned char* __restrict__ n8, const unsigned char* __restrict__ r8,
                                                     float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ rough, int HW, int Cr) {
  __shared__ float lut[256];      // the albedo is a function of a byte: 256 powf per workgroup instead of three per pixel
  if (a8) lut[threadIdx.x] = powf(byte_seg(threadIdx.x), 2.2f);
  __syncthreads();
  const int b = blockIdx.y;
  for (int o = (blockIdx.x * kLThreads + threadIdx.x) * V; o < HW; o += gridDim.x * kLThreads * V) {
    const size_t px = (size_t)b * HW + o;
    if (a8) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Vec<V> x;
#pragma unroll
        for (int u = 0; u < V; ++u) x.v[u] = lut[a8[(px + u) * 3 + c]];
        stv<V>(albedo, ((size_t)b * 3 + c) * HW + o, x);
      }
    }
    if (n8) {
      Vec<V> x[3];
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float n0 = byte_unit(n8[(px + u) * 3]), n1 = byte_unit(n8[(px + u) * 3 + 1]), n2 = byte_unit(n8[(px + u) * 3 + 2]);
        // np.sum(normal * normal, axis=0): products rounded, added in channel order (no contraction)
        const float ss = __fadd_rn(__fadd_rn(__fmul_rn(n0, n0), __fmul_rn(n1, n1)), __fmul_rn(n2, n2));
        const float len = sqrtf(fmaxf(ss, 1e-5f));
        x[0].v[u] = n0 / len;
        x[1].v[u] = n1 / len;
        x[2].v[u] = n2 / len;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) stv<V>(normal, ((size_t)b * 3 + c) * HW + o, x[c]);
    }
    if (r8) {
      Vec<V> x;
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = byte_unit(r8[(px + u) * Cr]);
      stv<V>(rough, px, x);
    }
  }
}

// ---- env maps ---------------------------------------------------------------------------------------------------------------------------
// The file keeps, per cell (r, c), 16 rows of 32 RGB texels, a cell row of the file being one contiguous run of C * 96 floats; the result
// keeps per (k, r, c) one contiguous block of eh * ew floats.  A workgroup takes kEnvCells cells of one cell row: every thread reads 12
// consecutive floats (four texels) of a file row as three 128-bit loads, parts the channels in registers -- for 8 x 16 it adds the two
// horizontal pairs there -- and puts them down in LDS cell by cell, channel by channel; after the barrier the blocks leave as 128-bit
// stores, for 8 x 16 the sum of two LDS rows each.  Every input byte is read once.
constexpr int kEnvH0 = 16, kEnvW0 = 32, kEnvCells = 4;
constexpr int kEnvGroups = kEnvH0 * kEnvCells * (kEnvW0 / 4);      // 12-float groups of a workgroup: 512, two per thread
template <int RATIO> struct EnvLds {
  static constexpr int kW = kEnvW0 / RATIO;                    // floats of a row of a cell in LDS
  static constexpr int kCell = 3 * kEnvH0 * kW + 8;            // + 8: the cells start eight banks apart
};

template <int RATIO>
__global__ __launch_bounds__(kLThreads) void lp_env(const float* __restrict__ raw, const float* __restrict__ scale, const float* __restrict__ ind, float* __restrict__ out,
                                                    int R, int C) {
  using L = EnvLds<RATIO>;
  __shared__ __attribute__((aligned(16))) float lds[kEnvCells * L::kCell];
  const int b = blockIdx.z, r = blockIdx.y, c0 = blockIdx.x * kEnvCells;
  const int ncell = C - c0 < kEnvCells ? C - c0 : kEnvCells;
  const bool live = ind == nullptr || ind[b] != 0.0f;      // workgroup-uniform: an image without an env map is never read
  if (live) {
    constexpr int kPer = kEnvGroups / kLThreads;
    float f[kPer][12];
    int at[kPer];
    const size_t pitch = (size_t)C * kEnvW0 * 3;
    const float* rb = raw + ((size_t)b * R + r) * kEnvH0 * pitch + (size_t)c0 * kEnvW0 * 3;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int g = threadIdx.x + m * kLThreads, row = g / (kEnvCells * 8), rem = g % (kEnvCells * 8), cell = rem / 8, gx = rem % 8;
      at[m] = -1;
      if (cell < ncell) {
        at[m] = cell * L::kCell + row * L::kW + gx * (4 / RATIO);
        const size_t src = (size_t)row * pitch + (size_t)cell * kEnvW0 * 3 + gx * 12;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const Vec<4> x = ldv<4>(rb, src + 4 * q);
#pragma unroll
          for (int u = 0; u < 4; ++u) f[m][4 * q + u] = x.v[u];
        }
      }
    }
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      if (at[m] < 0) continue;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float* dst = lds + at[m] + k * kEnvH0 * L::kW;
        if (RATIO == 2) {
          *reinterpret_cast<float2*>(dst) = make_float2(f[m][k] + f[m][3 + k], f[m][6 + k] + f[m][9 + k]);      // a00 + a01: horizontal neighbours
        } else {
          *reinterpret_cast<float4*>(dst) = make_float4(f[m][k], f[m][3 + k], f[m][6 + k], f[m][9 + k]);
        }
      }
    }
  }
  __syncthreads();
  constexpr int kBlock4 = kEnvH0 * kEnvW0 / (RATIO * RATIO) / 4;      // 128-bit stores per (k, r, c) block: 32 | 128
  const float s = scale[b];
  for (int o = threadIdx.x; o < ncell * 3 * kBlock4; o += kLThreads) {
    const int cell = o / (3 * kBlock4), rem = o - cell * 3 * kBlock4, k = rem / kBlock4, q = rem - k * kBlock4;
    Vec<4> y;
    if (!live) {
#pragma unroll
      for (int u = 0; u < 4; ++u) y.v[u] = 0.0f;
    } else if (RATIO == 2) {
      const int i = q / 4, jq = q % 4;
      const float* p = lds + cell * L::kCell + (k * kEnvH0 + 2 * i) * L::kW + 4 * jq;
      const float4 t = *reinterpret_cast<const float4*>(p), u2 = *reinterpret_cast<const float4*>(p + L::kW);
      y.v[0] = (t.x + u2.x) * 0.25f * s;
      y.v[1] = (t.y + u2.y) * 0.25f * s;
      y.v[2] = (t.z + u2.z) * 0.25f * s;
      y.v[3] = (t.w + u2.w) * 0.25f * s;
    } else {
      const float4 t = *reinterpret_cast<const float4*>(lds + cell * L::kCell + k * kEnvH0 * L::kW + 4 * q);
      y.v[0] = t.x * s;
      y.v[1] = t.y * s;
      y.v[2] = t.z * s;
      y.v[3] = t.w * s;
    }
    stv<4>(out, ((((size_t)b * 3 + k) * R + r) * C + c0 + cell) * (4 * kBlock4) + 4 * q, y);
  }
}

// workgroups per image of a streaming pass: one round of V pixels per thread, up to about 2048 workgroups in all, beyond which the threads stride
static dim3 stream_grid(int HW, int V, int bn) {
  const int want = (HW / V + kLThreads - 1) / kLThreads, cap = 2048 / bn > 64 ? 2048 / bn : 64;
  return dim3(want < cap ? want : cap, bn);
}

}  // namespace sgr

using namespace sgr;

#define SGR_LOADER_NUMPY "do it on the host as dataLoader.py does: "

extern "C" int sgr_loader_masks(const unsigned char* seg_u8, float* segArea, float* segEnv, float* segObj, int bn, int H, int W, int Cin, int erode, void* stream) {
  SGR_REQUIRE(seg_u8 && segArea && segEnv && segObj, "sgr_loader_masks: NULL tensor");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && Cin > 0, "sgr_loader_masks: non-positive size");
  SGR_SUPPORTED(bn <= 65535 && (H + kMTileH - 1) / kMTileH <= 65535 && (long long)H * W < (1ll << 28) && Cin <= 4,
                "sgr_loader_masks: size out of range (bn <= 65535, H <= 1048560, H W < 2^28, at most 4 channels); " SGR_LOADER_NUMPY
                "0.5 * ((u8 - 127.5) / 127.5 + 1), three comparisons and scipy.ndimage.binary_erosion(segObj, np.ones((7, 7)), border_value=1)");
  const dim3 grid((W + kMTileW - 1) / kMTileW, (H + kMTileH - 1) / kMTileH, bn), block(kLThreads);
  const bool vec = W % 4 == 0 && aligned16({segArea, segEnv, segObj});
  const hipStream_t st = (hipStream_t)stream;
  with_flag(vec, [&](auto VEC) {
    with_flag(erode != 0, [&](auto ERODE) { hipLaunchKernelGGL((lp_masks<VEC() ? 4 : 1, ERODE()>), grid, block, 0, st, seg_u8, segArea, segEnv, segObj, H, W, Cin); });
  });
  return sgr_check((int)hipGetLastError(), "sgr_loader_masks");
}

extern "C" int sgr_loader_scale_hdr(const float* hdr, const unsigned char* seg_u8, const float* num, float* im, float* scale, float* v, int bn, int H, int W, int Cin,
                                    long long k, void* stream) {
  SGR_REQUIRE(hdr && seg_u8 && im && scale && v, "sgr_loader_scale_hdr: NULL tensor");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && Cin > 0, "sgr_loader_scale_hdr: non-positive size");
  SGR_REQUIRE(k >= 0 && k < 3ll * H * W, "sgr_loader_scale_hdr: the rank k must lie in [0, 3 H W)");
  SGR_SUPPORTED(bn <= 65535 && (long long)H * W < (1ll << 28) && Cin <= 4,
                "sgr_loader_scale_hdr: size out of range (bn <= 65535, H W < 2^28, at most 4 channels); " SGR_LOADER_NUMPY
                "np.sort((hdr * seg).flatten())[k], scale = (0.95 - 0.1 u) / max(v, 0.1), np.clip(scale * hdr, 0, 1)");
  const int HW = H * W;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lp_select, dim3(bn), dim3(kSThreads), 0, st, hdr, seg_u8, num, scale, v, HW, Cin, (unsigned)k);
  const bool vec = HW % 4 == 0 && aligned16({hdr, im});
  if (vec)
    hipLaunchKernelGGL(lp_im<4>, stream_grid(HW, 4, bn), dim3(kLThreads), 0, st, hdr, scale, im, HW);
  else
    hipLaunchKernelGGL(lp_im<1>, stream_grid(HW, 1, bn), dim3(kLThreads), 0, st, hdr, scale, im, HW);
  return sgr_check((int)hipGetLastError(), "sgr_loader_scale_hdr");
}

extern "C" int sgr_loader_brdf_maps(const unsigned char* albedo_u8, const unsigned char* normal_u8, const unsigned char* rough_u8, float* albedo, float* normal,
                                    float* rough, int bn, int H, int W, int rough_channels, void* stream) {
  SGR_REQUIRE(albedo_u8 || normal_u8 || rough_u8, "sgr_loader_brdf_maps: NULL tensor: at least one map is needed");
  SGR_REQUIRE((!albedo_u8 || albedo) && (!normal_u8 || normal) && (!rough_u8 || rough), "sgr_loader_brdf_maps: NULL tensor: a map that is given needs its output");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && (!rough_u8 || rough_channels > 0), "sgr_loader_brdf_maps: non-positive size");
  SGR_SUPPORTED(bn <= 65535 && (long long)H * W < (1ll << 28) && rough_channels <= 4,
                "sgr_loader_brdf_maps: size out of range (bn <= 65535, H W < 2^28, at most 4 channels); " SGR_LOADER_NUMPY
                "(0.5 * ((u8 - 127.5) / 127.5 + 1)) ** 2.2, n / np.sqrt(np.maximum(np.sum(n * n, axis=0), 1e-5)), ((u8 - 127.5) / 127.5)[0:1]");
  const int HW = H * W;
  const bool vec = HW % 4 == 0 && aligned16({albedo, normal, rough});
  const hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(lp_brdf<4>, stream_grid(HW, 4, bn), dim3(kLThreads), 0, st, albedo_u8, normal_u8, rough_u8, albedo, normal, rough, HW, rough_channels);
  else
    hipLaunchKernelGGL(lp_brdf<1>, stream_grid(HW, 1, bn), dim3(kLThreads), 0, st, albedo_u8, normal_u8, rough_u8, albedo, normal, rough, HW, rough_channels);
  return sgr_check((int)hipGetLastError(), "sgr_loader_brdf_maps");
}

extern "C" int sgr_loader_envmaps(const float* env_raw, const float* scale, const float* env_ind, float* out, int bn, int rawH, int rawW, int envHeight, int envWidth,
                                  void* stream) {
  SGR_REQUIRE(env_raw && scale && out, "sgr_loader_envmaps: NULL tensor");
  SGR_REQUIRE(bn > 0 && rawH > 0 && rawW > 0 && envHeight > 0 && envWidth > 0, "sgr_loader_envmaps: non-positive size");
#define SGR_ENV_NUMPY SGR_LOADER_NUMPY "env.reshape(R, 16, C, 32, 3).transpose(4, 0, 2, 1, 3), then the mean over non-overlapping blocks, times scale"
  SGR_SUPPORTED((envHeight == 8 && envWidth == 16) || (envHeight == 16 && envWidth == 32),
                "sgr_loader_envmaps: envHeight x envWidth must be 8 x 16 or 16 x 32 (the file's 16 x 32 cells at ratio 2 or 1); " SGR_ENV_NUMPY);
  SGR_SUPPORTED(rawH % kEnvH0 == 0 && rawW % kEnvW0 == 0, "sgr_loader_envmaps: the raw map must be [R * 16, C * 32, 3]; " SGR_ENV_NUMPY);
  SGR_SUPPORTED(bn <= 65535 && rawH / kEnvH0 <= 65535 && rawW / kEnvW0 <= 65535, "sgr_loader_envmaps: size out of range (bn, R, C <= 65535); " SGR_ENV_NUMPY);
  SGR_SUPPORTED(aligned16({env_raw, out}), "sgr_loader_envmaps: env_raw and out must be 16-byte aligned; " SGR_ENV_NUMPY);
#undef SGR_ENV_NUMPY
  const int R = rawH / kEnvH0, C = rawW / kEnvW0;
  const dim3 grid((C + kEnvCells - 1) / kEnvCells, R, bn), block(kLThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (envHeight == 8)
    hipLaunchKernelGGL(lp_env<2>, grid, block, 0, st, env_raw, scale, env_ind, out, R, C);
  else
    hipLaunchKernelGGL(lp_env<1>, grid, block, 0, st, env_raw, scale, env_ind, out, R, C);
  return sgr_check((int)hipGetLastError(), "sgr_loader_envmaps");
}
