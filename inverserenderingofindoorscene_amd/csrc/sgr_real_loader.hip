// The real-image loaders' batch preparation on gfx950 (nyuDataLoader.py:75-131, iiwDataLoader.py:136-137, 205-214): from the decoded files,
// in the readers' layout, to the fp32 CHW tensors of the batch.  Inputs of the training step: no adjoints.
//
//   nyu_prepare   im / normal / seg uint8 [bn,Hs,Ws,3] (cv2.imread's channel order), depth fp32 [bn,Hs,Ws], one crop rectangle, flip flag and
//                 colour scale per image -> normal [bn,3,H,W], depth, segNormal, segDepth [bn,1,H,W], im [bn,3,H,W]: ONE launch
//   iiw_image     uint8 [bn,H,W,3] (PIL's channel order) -> (u8 / 255)^2.2 / its maximum over the image, [bn,3,H,W]: a reduction over the
//                 bytes (one partial per workgroup) and a writing pass
//
// Every byte -> value map has 256 inputs, so a workgroup starts by putting the results into LDS (one powf per thread) and the pixels index
// the tables.  The crop rectangle, the flip flag and the colour scale are read from device memory by every workgroup of the image: nothing
// visits the host, so the calls capture in a HIP graph.  No atomics and nothing across images: two runs give the same bits and image b
// does not depend on its batch.  DESIGN.md section 8n states the contracts; sgr_real_loader.h holds the decisions the host build shares.
#include "sgr_real_loader.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"      // Vec / stv, aligned16

namespace sgr {

using namespace rl;

constexpr int kRlThreads = 256;

// ---- nyu_prepare -------------------------------------------------------------------------------------------------------------------------
// A workgroup forms a tile of kRlTileH x kRlTileW output pixels of one image, a thread four consecutive pixels of a row: nine planes, nine
// 128-bit stores.  A source pixel after the before-resize maps is eight floats (Pix).  Direct: each output pixel maps its own 2 x 2 source
// pixels from memory.  STAGE: the source pixels the tile reads -- rows tap(y0).a .. tap(ylast).b of the crop, columns alike, of the mirrored
// range where the image is flipped -- are mapped once into LDS (the two square roots and three divisions of the normal once per source
// pixel instead of up to four times); a tile whose extent does not fit (a reduction by more than 1.5 or so) takes the direct path, decided
// per workgroup because the rectangle is per image.  The same bits either way.
constexpr int kRlTileH = 16, kRlTileW = 64;
constexpr int kRlSrcH = 24, kRlSrcW = 72, kRlPitch = kRlSrcW + 1, kRlPlane = kRlSrcH * kRlPitch;

struct Pix { float im0, im1, im2, n0, n1, n2, sn, d; };
struct NyuIn {
  const unsigned char *im, *normal, *seg;
  const float* depth;
  const int* crop;
  const unsigned char* flip;
  const double* colour;
};
struct NyuOut { float *normal, *depth, *seg_normal, *seg_depth, *im; };
struct NyuDims { int Hs, Ws, H, W, vec; };

// tab: byte_im | byte_unit | byte_seg, 256 entries each.  p: the pixel's index in the batch.
__device__ __forceinline__ Pix load_pix(const NyuIn& in, const float* tab, size_t p) {
  const unsigned char *a = in.im + p * 3, *n = in.normal + p * 3, *s = in.seg + p * 3;
  Pix q;
  q.im0 = tab[a[file_channel(0)]];
  q.im1 = tab[a[file_channel(1)]];
  q.im2 = tab[a[file_channel(2)]];
  q.n0 = tab[256 + n[file_channel(0)]];
  q.n1 = tab[256 + n[file_channel(1)]];
  q.n2 = tab[256 + n[file_channel(2)]];
  unit_normal(q.n0, q.n1, q.n2);
  q.sn = tab[512 + s[kSegFileChannel]];
  q.d = in.depth[p];
  return q;
}

template <bool STAGE>
__global__ __launch_bounds__(kRlThreads) void nyu_prepare_kernel(NyuIn in, NyuOut out, NyuDims a) {
  __shared__ float tab[3 * 256];
  __shared__ float tile[STAGE ? 8 * kRlPlane : 1];
  const int t = threadIdx.x, b = blockIdx.z, y0 = blockIdx.y * kRlTileH, x0 = blockIdx.x * kRlTileW;
  tab[t] = byte_im(t);
  tab[256 + t] = byte_unit(t);
  tab[512 + t] = byte_seg(t);
  Rect r{0, 0, a.Hs, a.Ws};
  if (in.crop) r = clamp_rect(in.crop[4 * b], in.crop[4 * b + 1], in.crop[4 * b + 2], in.crop[4 * b + 3], a.Hs, a.Ws);
  const bool fl = in.flip != nullptr && in.flip[b] != 0;
  const size_t base = (size_t)b * a.Hs * a.Ws + (size_t)r.rs * a.Ws + r.cs;      // the crop's first pixel
  __syncthreads();
  bool staged = false;
  int sy0 = 0, sx0 = 0;
  if (STAGE) {
    const int ylast = min(y0 + kRlTileH, a.H) - 1, xlast = min(x0 + kRlTileW, a.W) - 1;
    const int rx0 = fl ? a.W - 1 - xlast : x0, rx1 = fl ? a.W - 1 - x0 : xlast;      // the tile's columns of the resized image
    sy0 = tap_of(y0, r.h, a.H).a;
    sx0 = tap_of(rx0, r.w, a.W).a;
    const int th = tap_of(ylast, r.h, a.H).b - sy0 + 1, tw = tap_of(rx1, r.w, a.W).b - sx0 + 1;
    staged = th <= kRlSrcH && tw <= kRlSrcW;      // the same for every thread of the workgroup
    if (staged) {
      for (int i = t; i < th * tw; i += kRlThreads) {
        const int ty = i / tw, tx = i - ty * tw;
        const Pix q = load_pix(in, tab, base + (size_t)(sy0 + ty) * a.Ws + sx0 + tx);
        float* p = tile + ty * kRlPitch + tx;
        p[0] = q.im0;
        p[kRlPlane] = q.im1;
        p[2 * kRlPlane] = q.im2;
        p[3 * kRlPlane] = q.n0;
        p[4 * kRlPlane] = q.n1;
        p[5 * kRlPlane] = q.n2;
        p[6 * kRlPlane] = q.sn;
        p[7 * kRlPlane] = q.d;
      }
      __syncthreads();
    }
  }
  const int y = y0 + t / (kRlTileW / 4), xg = x0 + (t % (kRlTileW / 4)) * 4;
  if (y >= a.H || xg >= a.W) return;
  // crop-relative source pixel (yy, xx) after the before-resize maps
  const auto fetch = [&](int yy, int xx) -> Pix {
    if (STAGE && staged) {
      const float* p = tile + (yy - sy0) * kRlPitch + xx - sx0;
      return Pix{p[0], p[kRlPlane], p[2 * kRlPlane], p[3 * kRlPlane], p[4 * kRlPlane], p[5 * kRlPlane], p[6 * kRlPlane], p[7 * kRlPlane]};
    }
    return load_pix(in, tab, base + (size_t)yy * a.Ws + xx);
  };
  const Tap ty = tap_of(y, r.h, a.H);
  const int npix = min(4, a.W - xg);
  double k0 = 1.0, k1 = 1.0, k2 = 1.0;
  if (in.colour) {
    k0 = in.colour[3 * b];
    k1 = in.colour[3 * b + 1];
    k2 = in.colour[3 * b + 2];
  }
  float o[9][4];      // normal 0..2, depth, segNormal, segDepth, im 0..2; constant indices after unrolling
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const Tap tx = tap_of(mirrored(min(xg + u, a.W - 1), a.W, fl), r.w, a.W);
    const Pix q00 = fetch(ty.a, tx.a), q01 = fetch(ty.a, tx.b), q10 = fetch(ty.b, tx.a), q11 = fetch(ty.b, tx.b);
    float n0 = bilerp(q00.n0, q01.n0, q10.n0, q11.n0, tx.f, ty.f), n1 = bilerp(q00.n1, q01.n1, q10.n1, q11.n1, tx.f, ty.f),
          n2 = bilerp(q00.n2, q01.n2, q10.n2, q11.n2, tx.f, ty.f);
    renormalise(n0, n1, n2);
    const float d = bilerp(q00.d, q01.d, q10.d, q11.d, tx.f, ty.f);
    float i0 = bilerp(q00.im0, q01.im0, q10.im0, q11.im0, tx.f, ty.f), i1 = bilerp(q00.im1, q01.im1, q10.im1, q11.im1, tx.f, ty.f),
          i2 = bilerp(q00.im2, q01.im2, q10.im2, q11.im2, tx.f, ty.f);
    if (in.colour) {
      i0 = colour_scale(i0, k0);
      i1 = colour_scale(i1, k1);
      i2 = colour_scale(i2, k2);
    }
    o[0][u] = fl ? -n0 : n0;
    o[1][u] = n1;
    o[2][u] = n2;
    o[3][u] = d;
    o[4][u] = bilerp(q00.sn, q01.sn, q10.sn, q11.sn, tx.f, ty.f);
    o[5][u] = seg_depth(d);
    o[6][u] = i0;
    o[7][u] = i1;
    o[8][u] = i2;
  }
  const size_t HW = (size_t)a.H * a.W, at = (size_t)y * a.W + xg;
  float* planes[9] = {out.normal + (size_t)b * 3 * HW, out.normal + ((size_t)b * 3 + 1) * HW, out.normal + ((size_t)b * 3 + 2) * HW,
                      out.depth + (size_t)b * HW,      out.seg_normal + (size_t)b * HW,       out.seg_depth + (size_t)b * HW,
                      out.im + (size_t)b * 3 * HW,     out.im + ((size_t)b * 3 + 1) * HW,     out.im + ((size_t)b * 3 + 2) * HW};
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    if (a.vec && npix == 4) {      // vec: W % 4 == 0 and every plane on a 16-byte boundary (the host has checked)
      Vec<4> v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v.v[u] = o[j][u];
      stv<4>(planes[j], at, v);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < npix) planes[j][at + u] = o[j][u];
    }
  }
}

// ---- iiw_image ---------------------------------------------------------------------------------------------------------------------------
// The map is monotone, so the image's maximum is the table entry of its largest byte.  Pass 1: workgroup (blk, b) takes bytes blk * 256 + t,
// + 64 * 256, .. of image b and leaves ONE partial (the byte as a float: exact) in the workspace.  Pass 2 folds the 64 partials in every
// lane and writes tab[u8] / tab[max], a [P,3] -> [3,P] transposition per image, four pixels per thread.
constexpr int kIiwSplit = 64;

__global__ __launch_bounds__(kRlThreads) void iiw_max_kernel(const unsigned char* __restrict__ im, float* __restrict__ ws, long long n) {
  __shared__ unsigned lds[4];
  const unsigned char* p = im + (size_t)blockIdx.y * n;
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * kRlThreads + threadIdx.x; i < n; i += (long long)kIiwSplit * kRlThreads) m = max(m, (unsigned)p[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_down((int)m, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) ws[(size_t)blockIdx.y * kIiwSplit + blockIdx.x] = (float)max(max(lds[0], lds[1]), max(lds[2], lds[3]));
}

// V == 4: P % 4 == 0, `im` on a 4-byte and `out` on a 16-byte boundary -- twelve bytes as three dword loads, three 128-bit stores.
// V == 1: byte loads and scalar stores, any P and alignment.  The same bits either way.
template <int V>
__global__ __launch_bounds__(kRlThreads) void iiw_write_kernel(const unsigned char* __restrict__ im, const float* __restrict__ ws, float* __restrict__ out, long long P) {
  __shared__ float tab[256];
  const int b = blockIdx.y;
  tab[threadIdx.x] = byte_gamma(threadIdx.x);
  float mb = ws[(size_t)b * kIiwSplit + (threadIdx.x & 63)];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) mb = fmaxf(mb, __shfl_xor(mb, off, 64));
  __syncthreads();
  const float m = tab[(int)mb];      // an all-black image: 0, and 0 / 0 = NaN below, as numpy gives
  const unsigned char* src = im + (size_t)b * P * 3;
  float* dst = out + (size_t)b * P * 3;
  const long long groups = (P + 3) / 4;
  for (long long g = (long long)blockIdx.x * kRlThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kRlThreads) {
    const long long p0 = g * 4;
    const int npix = (int)(P - p0 < 4 ? P - p0 : 4);
    unsigned w[3] = {0u, 0u, 0u};      // the twelve bytes, little end first
    if (V == 4) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(src + p0 * 3);
      w[0] = s[0];
      w[1] = s[1];
      w[2] = s[2];
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < npix * 3) w[j >> 2] |= (unsigned)src[p0 * 3 + j] << (8 * (j & 3));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vec<4> v;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = u * 3 + c;
        v.v[u] = tab[(w[j >> 2] >> (8 * (j & 3))) & 255u] / m;
      }
      if (V == 4) {
        stv<4>(dst, (size_t)(c * P + p0), v);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < npix) dst[c * P + p0 + u] = v.v[u];
      }
    }
  }
}

// Which form runs (DESIGN.md section 8n has the figures): the staged one.  At batch 16, crops of 560..600 columns to 480 x 640 it measured
// 107 us against the direct form's 145 us; to 240 x 320 the tiles' extents do not fit, every workgroup takes the direct path and the two
// forms measure the same (64 us, 63 us).  SGR_NYU_STAGE=0 forces the direct form (A/B runs, the tests' bit comparison); read at every call.
static bool nyu_stage() {
  const char* e = getenv("SGR_NYU_STAGE");
  return !(e != nullptr && e[0] == '0' && e[1] == 0);
}

}  // namespace sgr

using namespace sgr;

#define SGR_RL_NUMPY "do it on the host as nyuDataLoader.py does: the crop, loadImage's maps, cv2.resize(INTER_LINEAR), the two normalisations"

extern "C" int sgr_nyu_prepare(const unsigned char* im_u8, const unsigned char* normal_u8, const unsigned char* seg_u8, const float* depth, const int* crop,
                               const unsigned char* flip, const double* colour, float* out_normal, float* out_depth, float* out_seg_normal, float* out_seg_depth,
                               float* out_im, int bn, int Hs, int Ws, int H, int W, void* stream) {
  SGR_REQUIRE(im_u8 && normal_u8 && seg_u8 && depth && out_normal && out_depth && out_seg_normal && out_seg_depth && out_im, "sgr_nyu_prepare: NULL tensor");
  SGR_REQUIRE(bn > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "sgr_nyu_prepare: non-positive size");
  SGR_REQUIRE((crop != nullptr) == (flip != nullptr) && (crop != nullptr) == (colour != nullptr),
              "sgr_nyu_prepare: crop, flip and colour come all three (the TRAIN phase) or not at all (TEST)");
  SGR_SUPPORTED(bn <= 65535 && (long long)Hs * Ws < (1ll << 28) && (long long)H * W < (1ll << 28) && (H + kRlTileH - 1) / kRlTileH <= 65535,
                "sgr_nyu_prepare: size out of range (bn <= 65535, Hs Ws < 2^28, H W < 2^28, H <= 1048560); " SGR_RL_NUMPY);
  const NyuIn in{im_u8, normal_u8, seg_u8, depth, crop, flip, colour};
  const NyuOut out{out_normal, out_depth, out_seg_normal, out_seg_depth, out_im};
  const NyuDims a{Hs, Ws, H, W, (W % 4 == 0 && aligned16({out_normal, out_depth, out_seg_normal, out_seg_depth, out_im})) ? 1 : 0};
  const dim3 grid((W + kRlTileW - 1) / kRlTileW, (H + kRlTileH - 1) / kRlTileH, bn), block(kRlThreads);
  with_flag(nyu_stage(), [&](auto STAGE) { hipLaunchKernelGGL((nyu_prepare_kernel<STAGE()>), grid, block, 0, (hipStream_t)stream, in, out, a); });
  return sgr_check((int)hipGetLastError(), "sgr_nyu_prepare");
}

extern "C" int sgr_iiw_image(const unsigned char* im_u8, float* out, float* workspace, int bn, int H, int W, void* stream) {
  SGR_REQUIRE(im_u8 && out, "sgr_iiw_image: NULL tensor");
  SGR_REQUIRE(workspace, "sgr_iiw_image: NULL workspace (64 * bn floats)");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0, "sgr_iiw_image: non-positive size");
  SGR_SUPPORTED(bn <= 65535 && (long long)H * W < (1ll << 28),
                "sgr_iiw_image: size out of range (bn <= 65535, H W < 2^28); do it on the host as iiwDataLoader.py does: (im / 255.0) ** 2.2, np.transpose(im, [2, 0, 1]), "
                "im / im.max()");
  const long long P = (long long)H * W;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(iiw_max_kernel, dim3(kIiwSplit, bn), dim3(kRlThreads), 0, s, im_u8, workspace, P * 3);
  const bool vec = P % 4 == 0 && ((uintptr_t)im_u8 & 3) == 0 && aligned16({out});
  const long long want = ((P + 3) / 4 + kRlThreads - 1) / kRlThreads;
  const dim3 grid((unsigned)(want < 1024 ? want : 1024), bn);
  if (vec)
    hipLaunchKernelGGL(iiw_write_kernel<4>, grid, dim3(kRlThreads), 0, s, im_u8, workspace, out, P);
  else
    hipLaunchKernelGGL(iiw_write_kernel<1>, grid, dim3(kRlThreads), 0, s, im_u8, workspace, out, P);
  return sgr_check((int)hipGetLastError(), "sgr_iiw_image");
}
