// testReal's output stage and the image writers on gfx950 (testReal.py:542-657, utils.py:65-76, 102-154): from the fp32 predictions, in the
// layouts the operators produce, to tensors that are ready to write.  No adjoints.
//
//   image     x [B,C,h,w], any strides -> uint8 [B,nh,nw,Cout]: a per-image statistic (depth, shading: the mean; rendered: the maximum), a
//             point map, OpenCV's INTER_LINEAR resize, a point map, truncation to a byte, the channels reversed on request
//   mosaic    env [B,3,R,C,eh,ew], any strides -> uint8 [B,Hm,Wm,3]: every interY-th / interX-th cell on a background of 255     utils.py:102-128
//   env_hwc   env [B,3,R,C,eh,ew] -> fp32 [B,R,C,eh,ew,3], the channels reversed on request: the .npz layout                      testReal.py:626-631
//
// The statistic is one launch of kExSplit workgroups per image, each leaving ONE partial in the workspace; the image kernel's prologue
// folds the 64 partials in double (fold_lanes of sgr_reduce.h; the maximum alike).  No float atomics and nothing across images, so two
// runs give the same bits and image b does not depend on its batch; nothing visits the host, so the calls capture in a HIP graph.
// DESIGN.md section 8m states the contracts; sgr_export.h holds the decisions the host build shares.
#include "sgr_export.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"      // block_sum, fold_lanes, Vec / ldv / stv, aligned16

namespace sgr {

using namespace ex;

constexpr int kExThreads = 256, kExSplit = 64;

struct ExStrides4 { long long v[4]; };
struct ExStrides6 { long long v[6]; };

// ---- statistics ------------------------------------------------------------------------------------------------------------------------
// Workgroup (blk, b) takes elements blk * 256 + t, + 64 * 256, .. of image b's C * h * w, in (c, y, x) order whatever the strides.  MAX:
// the same walk and ladder with fmaxf for +; fmaxf drops a NaN.
template <bool MAX>
__global__ __launch_bounds__(kExThreads) void ex_stat(const float* __restrict__ x, ExStrides4 st, float* __restrict__ ws, int C, int h, int w) {
  __shared__ float lds[4];
  const int b = blockIdx.y, n = C * h * w, hw = h * w;
  const float* xb = x + (size_t)b * st.v[0];
  float acc = MAX ? -INFINITY : 0.0f;
  for (int i = blockIdx.x * kExThreads + threadIdx.x; i < n; i += kExSplit * kExThreads) {
    const int c = i / hw, r = i - c * hw, y = r / w, xx = r - y * w;
    const float v = xb[c * st.v[1] + y * st.v[2] + xx * st.v[3]];
    acc = MAX ? fmaxf(acc, v) : acc + v;
  }
  if (MAX) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = fmaxf(acc, __shfl_down(acc, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[b * kExSplit + blockIdx.x] = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  } else {
    float v[1] = {acc};
    block_sum(v, lds);
    if (threadIdx.x == 0) ws[b * kExSplit + blockIdx.x] = v[0];
  }
}

// the maximum of image b's 64 partials, in every lane (fold_lanes with fmax for +)
__device__ __forceinline__ double fold_lanes_max(const float* __restrict__ ws, int b) {
  double x = (double)ws[(size_t)b * kExSplit + (threadIdx.x & 63)];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x = fmax(x, __shfl_xor(x, off, 64));
  return x;
}

// ---- bytes of four consecutive pixels --------------------------------------------------------------------------------------------------
// Dwords packs the four pixels' COUT channels (COUT dwords hold 4 * COUT bytes, little end first).  A full group on a dword boundary
// leaves as one COUT-dword store; the others (the row's tail, rows that start off a boundary) byte by byte.
template <int COUT> struct alignas(4) Dwords { uint32_t v[COUT]; };
template <int COUT>
__device__ __forceinline__ void put_byte(Dwords<COUT>& d, int j /* compile-time */, unsigned q) { d.v[j >> 2] |= q << (8 * (j & 3)); }
template <int COUT>
__device__ __forceinline__ void store_group(unsigned char* __restrict__ p, const Dwords<COUT>& d, int npix) {
  if (npix == 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<Dwords<COUT>*>(p) = d;
  } else {
#pragma unroll
    for (int j = 0; j < 4 * COUT; ++j)
      if (j < npix * COUT) p[j] = (unsigned char)((d.v[j >> 2] >> (8 * (j & 3))) & 255u);
  }
}

// ---- the image kernel --------------------------------------------------------------------------------------------------------------------
// A workgroup forms a tile of kExTileH x kExTileW output pixels, a thread four consecutive pixels of a row.  STAGE: the source pixels the
// tile reads -- rows src(y0).s .. src(ylast).s + 1, columns alike -- go through the before-resize map into LDS once (one powf per source
// pixel instead of four per output pixel); the host has checked that the extent fits (export_stage_fits).  Otherwise (a reduction by more
// than the tile allows) the four neighbours come from memory through the same map and the bytes leave one by one: the same bits either way.
constexpr int kExTileH = 16, kExTileW = 64;
constexpr int kExSrcH = 24, kExSrcW = 72, kExPitch = kExSrcW + 1;

struct ExImage {
  int kind, C, h, w, nh, nw, bgr, stat;
};

template <int C, int COUT, bool STAGE>
__global__ __launch_bounds__(kExThreads) void ex_image(const float* __restrict__ x, ExStrides4 st, const float* __restrict__ scale, const float* __restrict__ ws,
                                                       unsigned char* __restrict__ out, ExImage a) {
  __shared__ float tile[STAGE ? C * kExSrcH * kExPitch : 1];
  const int b = blockIdx.z, y0 = blockIdx.y * kExTileH, x0 = blockIdx.x * kExTileW;
  const float* xb = x + (size_t)b * st.v[0];
  float p = 1.0f;
  if (a.stat == kMean)
    p = stat_param(a.kind, fold_lanes<kExSplit>(ws, b, 1, 0), (double)C * a.h * a.w);
  else if (a.stat == kMax)
    p = stat_param(a.kind, fold_lanes_max(ws, b), 1.0);
  else if (scale)
    p = scale[b];
  int sy0 = 0, sx0 = 0;
  if (STAGE) {
    const int ylast = min(y0 + kExTileH, a.nh) - 1, xlast = min(x0 + kExTileW, a.nw) - 1;
    sy0 = src_of(y0, a.h, a.nh).s;
    sx0 = src_of(x0, a.w, a.nw).s;
    const int th = min(src_of(ylast, a.h, a.nh).s + 1, a.h - 1) - sy0 + 1, tw = min(src_of(xlast, a.w, a.nw).s + 1, a.w - 1) - sx0 + 1;
    for (int i = threadIdx.x; i < C * th * tw; i += kExThreads) {
      const int c = i / (th * tw), r = i - c * th * tw, ty = r / tw, tx = r - ty * tw;
      tile[(c * kExSrcH + ty) * kExPitch + tx] = pre_map(a.kind, xb[c * st.v[1] + (sy0 + ty) * st.v[2] + (sx0 + tx) * st.v[3]], p);
    }
    __syncthreads();
  }
  const int y = y0 + threadIdx.x / (kExTileW / 4), xg = x0 + (threadIdx.x % (kExTileW / 4)) * 4;
  if (y >= a.nh || xg >= a.nw) return;
  const Src sy = src_of(y, a.h, a.nh);
  const int yA = sy.s, yB = min(sy.s + 1, a.h - 1);
  Dwords<COUT> d;
#pragma unroll
  for (int j = 0; j < COUT; ++j) d.v[j] = 0;
  const int npix = min(4, a.nw - xg);
  unsigned char* po = out + (((size_t)b * a.nh + y) * a.nw + xg) * COUT;
#pragma unroll STAGE ? 4 : 1
  for (int u = 0; u < 4; ++u) {
    const Src sx = src_of(min(xg + u, a.nw - 1), a.w, a.nw);
    const int xA = sx.s, xB = min(sx.s + 1, a.w - 1);
    // the byte of source channel c (named values, constant channels: nothing here is an indexed array)
    const auto byte_of = [&](int c) -> unsigned {
      float v00, v01, v10, v11;
      if (STAGE) {
        const float* t = tile + c * kExSrcH * kExPitch;
        v00 = t[(yA - sy0) * kExPitch + xA - sx0];
        v01 = t[(yA - sy0) * kExPitch + xB - sx0];
        v10 = t[(yB - sy0) * kExPitch + xA - sx0];
        v11 = t[(yB - sy0) * kExPitch + xB - sx0];
      } else {
        const float* s = xb + c * st.v[1];
        v00 = pre_map(a.kind, s[yA * st.v[2] + xA * st.v[3]], p);
        v01 = pre_map(a.kind, s[yA * st.v[2] + xB * st.v[3]], p);
        v10 = pre_map(a.kind, s[yB * st.v[2] + xA * st.v[3]], p);
        v11 = pre_map(a.kind, s[yB * st.v[2] + xB * st.v[3]], p);
      }
      const float top = lerp2(v00, v01, sx.f), bot = lerp2(v10, v11, sx.f);      // columns first, then rows
      return quantise(post_map(a.kind, lerp2(top, bot, sy.f), p));
    };
    const unsigned q0 = byte_of(0), q1 = C == 3 ? byte_of(1) : q0, q2 = C == 3 ? byte_of(2) : q0;
    if (STAGE) {
      put_byte<COUT>(d, u * COUT, a.bgr ? q2 : q0);
      if (COUT == 3) {
        put_byte<COUT>(d, u * COUT + 1, q1);
        put_byte<COUT>(d, u * COUT + 2, a.bgr ? q0 : q2);
      }
    } else if (u < npix) {      // the loop is not unrolled here (four maps per channel and pixel): the bytes leave one by one
      po[u * COUT] = (unsigned char)(a.bgr ? q2 : q0);
      if (COUT == 3) {
        po[u * COUT + 1] = (unsigned char)q1;
        po[u * COUT + 2] = (unsigned char)(a.bgr ? q0 : q2);
      }
    }
  }
  if (STAGE) store_group<COUT>(po, d, npix);
}

// does every tile's source extent fit the LDS tile?  The same src_of the kernel evaluates, at the tiles' first and last pixels.
static bool export_stage_fits(int in, int out, int tile, int cap) {
  for (int d0 = 0; d0 < out; d0 += tile) {
    const int last = (d0 + tile < out ? d0 + tile : out) - 1;
    int hi = src_of(last, in, out).s + 1;
    if (hi > in - 1) hi = in - 1;
    if (hi - src_of(d0, in, out).s + 1 > cap) return false;
  }
  return true;
}

// ---- the env mosaic ------------------------------------------------------------------------------------------------------------------------
// One thread per four consecutive pixels of an output row; a pixel inside a tile reads its three channels of the sampled cell, the
// others are background.  Cells that are not sampled are never read.
__global__ __launch_bounds__(kExThreads) void ex_mosaic(const float* __restrict__ env, ExStrides6 st, unsigned char* __restrict__ out, Mosaic m, int eh, int ew, int gap,
                                                        int bgr) {
  const int b = blockIdx.z, y = blockIdx.y, xg = (blockIdx.x * kExThreads + threadIdx.x) * 4;
  if (xg >= m.Wm) return;
  int r, iy;
  const bool row_in = mosaic_src(y, eh, gap, m.tilesY, m.interY, r, iy);
  const float* eb = env + (size_t)b * st.v[0] + (row_in ? r * st.v[2] + iy * st.v[4] : 0);
  Dwords<3> d;
#pragma unroll
  for (int j = 0; j < 3; ++j) d.v[j] = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int c, ix;
    const bool in = mosaic_src(xg + u, ew, gap, m.tilesX, m.interX, c, ix) && row_in && xg + u < m.Wm;
    unsigned q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = in ? quantise(post_map(kImageGamma, eb[k * st.v[1] + c * st.v[3] + ix * st.v[5]], 1.0f)) : 255u;
    if (bgr) {
      const unsigned t = q[0];
      q[0] = q[2];
      q[2] = t;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) put_byte<3>(d, u * 3 + k, q[k]);
  }
  store_group<3>(out + (((size_t)b * m.Hm + y) * m.Wm + xg) * 3, d, min(4, m.Wm - xg));
}

// ---- env_hwc -------------------------------------------------------------------------------------------------------------------------------
// A cell's three planes of P = eh * ew floats become P texels of three.  V == 4: a thread reads four texels of each plane as 128-bit
// loads, interleaves them in registers and writes twelve floats as three 128-bit stores (P % 4 == 0 keeps both sides on 16-byte
// boundaries).  V == 1: one texel at a time.  Every byte is read once and written once.
template <int V>
__global__ __launch_bounds__(kExThreads) void ex_env_hwc(const float* __restrict__ env, float* __restrict__ out, long long cells, int RC, int P, int flip) {
  const long long groups = cells * (P / V);
  for (long long g = (long long)blockIdx.x * kExThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kExThreads) {
    const long long cell = g / (P / V);
    const int t = (int)(g - cell * (P / V)) * V;
    const long long b = cell / RC, rc = cell - b * RC;
    Vec<V> pl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) pl[k] = ldv<V>(env, (size_t)(((b * 3 + k) * RC + rc) * P + t));
    float f[3 * V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      f[3 * u] = flip ? pl[2].v[u] : pl[0].v[u];
      f[3 * u + 1] = pl[1].v[u];
      f[3 * u + 2] = flip ? pl[0].v[u] : pl[2].v[u];
    }
    const size_t o = (size_t)(cell * P + t) * 3;
    if (V == 4) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        Vec<V> y;
#pragma unroll
        for (int u = 0; u < V; ++u) y.v[u] = f[V * s + u];
        stv<V>(out, o + V * s, y);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3 * V; ++j) out[o + j] = f[j];
    }
  }
}

}  // namespace sgr

using namespace sgr;

#define SGR_EXPORT_NUMPY "do it on the host as testReal.py does: "

extern "C" long long sgr_export_image_workspace_floats(int kind, int B) {
  if (kind < 0 || kind >= kKinds || B <= 0) return -1;
  return kind_stat(kind) == kNoStat ? 0 : (long long)B * kExSplit;
}

extern "C" int sgr_export_image(const float* x, const long long* x_strides, const float* scale, unsigned char* out, float* workspace, int kind, int B, int C, int h, int w,
                                int nh, int nw, int bgr, void* stream) {
  SGR_REQUIRE(x && x_strides && out, "sgr_export_image: NULL tensor");
  SGR_REQUIRE(kind >= 0 && kind < kKinds, "sgr_export_image: unknown kind (SGR_EXPORT_ALBEDO .. SGR_EXPORT_IMAGE_GAMMA)");
  SGR_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && nh > 0 && nw > 0, "sgr_export_image: non-positive size");
  SGR_REQUIRE(kind_takes(kind, C), "sgr_export_image: wrong channel count for the kind (albedo, normal, rendered, shading: 3; rough, depth: 1; image: 1 or 3)");
  SGR_REQUIRE(kind_resizes(kind) || (nh == h && nw == w), "sgr_export_image: shading and image are written at the source's size (no resize)");
  SGR_REQUIRE(scale == nullptr || kind == kAlbedo, "sgr_export_image: scale (cAlbedo) belongs to the albedo kind");
  SGR_REQUIRE(kind_stat(kind) == kNoStat || workspace, "sgr_export_image: NULL workspace (sgr_export_image_workspace_floats)");
  SGR_SUPPORTED(B <= 65535 && (long long)C * h * w < (1ll << 30) && (long long)nh * nw < (1ll << 30) && (nh + kExTileH - 1) / kExTileH <= 65535,
                "sgr_export_image: size out of range (B <= 65535, C h w < 2^30, nh nw < 2^30, nh <= 1048560); " SGR_EXPORT_NUMPY
                "the map of the kind, cv2.resize(INTER_LINEAR), np.clip and astype(np.uint8)");
  const hipStream_t s = (hipStream_t)stream;
  ExStrides4 st;
  for (int i = 0; i < 4; ++i) st.v[i] = x_strides[i];
  const int stat = kind_stat(kind);
  if (stat == kMean)
    hipLaunchKernelGGL(ex_stat<false>, dim3(kExSplit, B), dim3(kExThreads), 0, s, x, st, workspace, C, h, w);
  else if (stat == kMax)
    hipLaunchKernelGGL(ex_stat<true>, dim3(kExSplit, B), dim3(kExThreads), 0, s, x, st, workspace, C, h, w);
  const ExImage a{kind, C, h, w, nh, nw, bgr != 0, stat};
  const dim3 grid((nw + kExTileW - 1) / kExTileW, (nh + kExTileH - 1) / kExTileH, B), block(kExThreads);
  const bool stage = export_stage_fits(h, nh, kExTileH, kExSrcH) && export_stage_fits(w, nw, kExTileW, kExSrcW);
  const int cout = kind_out_channels(kind, C);
  with_flag(stage, [&](auto STAGE) {
    if (C == 3)
      hipLaunchKernelGGL((ex_image<3, 3, STAGE()>), grid, block, 0, s, x, st, scale, workspace, out, a);
    else if (cout == 3)
      hipLaunchKernelGGL((ex_image<1, 3, STAGE()>), grid, block, 0, s, x, st, scale, workspace, out, a);
    else
      hipLaunchKernelGGL((ex_image<1, 1, STAGE()>), grid, block, 0, s, x, st, scale, workspace, out, a);
  });
  return sgr_check((int)hipGetLastError(), "sgr_export_image");
}

extern "C" int sgr_export_env_mosaic(const float* env, const long long* env_strides, unsigned char* out, int B, int R, int C, int eh, int ew, int nrows, int ncols, int gap,
                                     int bgr, void* stream) {
  SGR_REQUIRE(env && env_strides && out, "sgr_export_env_mosaic: NULL tensor");
  SGR_REQUIRE(B > 0 && R > 0 && C > 0 && eh > 0 && ew > 0, "sgr_export_env_mosaic: non-positive size");
  SGR_REQUIRE(nrows > 0 && ncols > 0 && gap >= 0, "sgr_export_env_mosaic: nrows and ncols must be positive, gap not negative");
  SGR_REQUIRE(nrows <= R && ncols <= C, "sgr_export_env_mosaic: nrows > R or ncols > C (int(R / nrows) would be 0: the reference divides by zero there)");
  const Mosaic m = mosaic_of(R, C, eh, ew, nrows, ncols, gap);
  SGR_SUPPORTED(B <= 65535 && m.Hm <= 65535 && (long long)m.Hm * m.Wm < (1ll << 29),
                "sgr_export_env_mosaic: size out of range (B, Hm <= 65535, Hm Wm < 2^29); " SGR_EXPORT_NUMPY "utils.writeEnvToFile");
  ExStrides6 st;
  for (int i = 0; i < 6; ++i) st.v[i] = env_strides[i];
  const dim3 grid(((m.Wm + 3) / 4 + kExThreads - 1) / kExThreads, m.Hm, B);
  hipLaunchKernelGGL(ex_mosaic, grid, dim3(kExThreads), 0, (hipStream_t)stream, env, st, out, m, eh, ew, gap, bgr != 0);
  return sgr_check((int)hipGetLastError(), "sgr_export_env_mosaic");
}

extern "C" int sgr_export_env_hwc(const float* env, float* out, int B, int R, int C, int eh, int ew, int flip, void* stream) {
  SGR_REQUIRE(env && out, "sgr_export_env_hwc: NULL tensor");
  SGR_REQUIRE(B > 0 && R > 0 && C > 0 && eh > 0 && ew > 0, "sgr_export_env_hwc: non-positive size");
  SGR_SUPPORTED((long long)R * C < (1ll << 31) && (long long)eh * ew < (1ll << 28),
                "sgr_export_env_hwc: size out of range (R C < 2^31, eh ew < 2^28); " SGR_EXPORT_NUMPY "np.ascontiguousarray(env.transpose(1, 2, 3, 4, 0)[..., ::-1])");
  const long long cells = (long long)B * R * C;
  const int P = eh * ew;
  const bool vec = P % 4 == 0 && aligned16({env, out});
  const long long groups = cells * (vec ? P / 4 : P), want = (groups + kExThreads - 1) / kExThreads;
  const dim3 grid((unsigned)(want < 8192 ? want : 8192));
  if (vec)
    hipLaunchKernelGGL(ex_env_hwc<4>, grid, dim3(kExThreads), 0, (hipStream_t)stream, env, out, cells, R * C, P, flip != 0);
  else
    hipLaunchKernelGGL(ex_env_hwc<1>, grid, dim3(kExThreads), 0, (hipStream_t)stream, env, out, cells, R * C, P, flip != 0);
  return sgr_check((int)hipGetLastError(), "sgr_export_env_hwc");
}
