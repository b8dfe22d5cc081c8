// PIL's antialiased resize of 8-bit images on gfx950 (dataLoader.py:223-224, iiwDataLoader.py:112-134: Image.resize(size, Image.ANTIALIAS)):
// uint8 HWC in, uint8 HWC out, the bytes Pillow's ImagingResample gives.  The coefficients are integers (22 fractional bits) from a table the
// host builds in double, the sums are int32: nothing here rounds differently from the host, so the contract is ==.
//
//   two_pass   a launch per pass that runs: columns first over the source rows the output rows read, into a uint8 workspace, then rows
//   tiled      ONE launch; a workgroup stages its tile's source extent in LDS, resizes it horizontally into a second LDS tile and runs the
//              vertical pass from there -- for geometries whose tiles fit (pr::plan_tiles), both passes running, ksize <= 32
//
// The threads' bodies, with every index they form, live in sgr_pil_resize.h, which the host test program compiles too.  No atomics, nothing
// across images: two runs give the same bits and image b does not depend on its batch.  Nothing visits the host during a call (the tile
// decision is a few double operations on the sizes), so a call captures in a HIP graph.  DESIGN.md section 8p states the contract.
#include <stdio.h>

#include "sgr_pil_resize.h"
#include "sgr_launch.h"

namespace sgr {

using namespace pr;

template <int C, bool REG>
__global__ __launch_bounds__(kThreads) void pr_hpass_kernel(Job j, const unsigned char* __restrict__ src, const int* __restrict__ htab, unsigned char* __restrict__ out,
                                                            int opitch, size_t out_stride) {
  const unsigned char* s = src + (size_t)blockIdx.z * j.H * j.W * C;
  unsigned char* o = out + (size_t)blockIdx.z * out_stride;
  if (htab[1])
    hpass_global_thread<C, REG, false>(j, s, htab, o, opitch, blockIdx.x, blockIdx.y, threadIdx.x);
  else
    hpass_global_thread<C, REG, true>(j, s, htab, o, opitch, blockIdx.x, blockIdx.y, threadIdx.x);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void pr_vpass_kernel(Job j, const unsigned char* __restrict__ in, size_t in_stride, int ipitch, const int* __restrict__ vtab,
                                                            unsigned char* __restrict__ dst) {
  const unsigned char* s = in + (size_t)blockIdx.z * in_stride;
  unsigned char* o = dst + (size_t)blockIdx.z * j.wh * j.ww * j.C;
  if (vtab[1])
    vpass_global_thread<VEC, false>(j, s, ipitch, vtab, o, blockIdx.y, blockIdx.x, threadIdx.x);
  else
    vpass_global_thread<VEC, true>(j, s, ipitch, vtab, o, blockIdx.y, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(kThreads) void pr_copy_kernel(Job j, const unsigned char* __restrict__ src, unsigned char* __restrict__ dst) {
  copy_thread(j, src + (size_t)blockIdx.z * j.H * j.W * j.C, dst + (size_t)blockIdx.z * j.wh * j.ww * j.C, blockIdx.y, blockIdx.x, threadIdx.x);
}

template <int C, bool REG>
__global__ __launch_bounds__(kThreads) void pr_tiled_kernel(Job j, TilePlan p, const unsigned char* __restrict__ src, const int* __restrict__ htab, const int* __restrict__ vtab,
                                                            unsigned char* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) unsigned char S[kSrcBytes];
  __shared__ __attribute__((aligned(16))) unsigned char M[kMidBytes];
  __shared__ int VT[kTileH * kKTile];
  __shared__ int HT[REG ? 1 : kKTile * kTileW];
  const unsigned char* s = src + (size_t)blockIdx.z * j.H * j.W * C;
  unsigned char* o = dst + (size_t)blockIdx.z * j.wh * j.ww * C;
  const int tid = threadIdx.x;
  const Tile t = tile_of(j, p, htab, vtab, blockIdx.x, blockIdx.y);
  tile_stage_thread<REG>(j, p, t, s, htab, vtab, S, VT, HT, tid);
  __syncthreads();
  if (htab[1])
    tile_hpass_thread<C, REG, false>(j, p, t, s, htab, S, HT, M, tid);
  else
    tile_hpass_thread<C, REG, true>(j, p, t, s, htab, S, HT, M, tid);
  __syncthreads();
  if (vtab[1])
    tile_vpass_thread<C, false>(j, t, vtab, M, VT, o, tid);
  else
    tile_vpass_thread<C, true>(j, t, vtab, M, VT, o, tid);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
#define SGR_PR_HOST "; on the host it is PIL's Image.resize(size, Image.LANCZOS) (Image.ANTIALIAS in the reference) of the decoded image"

struct PrGeom { Job j; bool hpass, vpass; };

// the checks every entry shares; fills g
static int pr_check(const char* who, int bn, int H, int W, int C, int outH, int outW, const int* window, int filter, PrGeom* g) {
  static thread_local char msg[384];
  const auto fail = [&](int code, const char* text) {
    snprintf(msg, sizeof msg, "%s: %s", who, text);
    set_error(msg);
    return code;
  };
  if (!(bn > 0 && H > 0 && W > 0 && outH > 0 && outW > 0)) return fail(SGR_ERR_BAD_ARG, "zero-sized or negative input or output size");
  if (!(C == 1 || C == 3))
    return fail(SGR_ERR_UNSUPPORTED, "C must be 1 ('L') or 3 ('RGB'): PIL resizes LA / RGBA on its premultiplied-alpha route, which is not offered" SGR_PR_HOST);
  if (filter == 0) return fail(SGR_ERR_UNSUPPORTED, "filter 0 (nearest) is a different PIL code path without coefficients: not offered; 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming");
  if (!filter_known(filter)) return fail(SGR_ERR_BAD_ARG, "unknown filter (PIL's codes: 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)");
  if (!(bn <= 65535 && H <= kMaxSize && W <= kMaxSize && outH <= kMaxSize && outW <= kMaxSize && (long long)H * W * C < (1ll << 31) && (long long)outH * outW * C < (1ll << 31)))
    return fail(SGR_ERR_UNSUPPORTED, "size out of range (bn <= 65535, every side <= 2^24, H W C < 2^31, outH outW C < 2^31)" SGR_PR_HOST);
  Job& j = g->j;
  j.H = H; j.W = W; j.C = C; j.outH = outH; j.outW = outW;
  j.r0 = 0; j.c0 = 0; j.wh = outH; j.ww = outW;
  if (window) {
    j.r0 = window[0]; j.c0 = window[1]; j.wh = window[2]; j.ww = window[3];
    if (!(j.wh > 0 && j.ww > 0)) return fail(SGR_ERR_BAD_ARG, "window (r0, c0, h, w): zero-sized or negative h or w");
    if (!(j.r0 >= 0 && j.c0 >= 0 && (long long)j.r0 + j.wh <= outH && (long long)j.c0 + j.ww <= outW)) return fail(SGR_ERR_BAD_ARG, "window (r0, c0, h, w) leaves the resized image");
  }
  g->hpass = outW != W;
  g->vpass = outH != H;
  j.ksH = g->hpass ? axis_of(W, outW, filter).ksize : 0;
  j.ksV = g->vpass ? axis_of(H, outH, filter).ksize : 0;
  if (g->vpass) {
    needed_rows(H, outH, filter, j.r0, j.wh, &j.ya, &j.yb);
  } else {
    j.ya = j.r0;
    j.yb = j.r0 + j.wh;
  }
  if (!((j.wh + 0ll) <= 1048560 && (long long)(j.yb - j.ya) <= 1048560)) return fail(SGR_ERR_UNSUPPORTED, "window higher than 1048560 rows" SGR_PR_HOST);
  return SGR_OK;
}
static int tmp_pitch(const Job& j) { return round4(j.ww * j.C); }

}  // namespace sgr

using namespace sgr;

extern "C" long long sgr_pil_resize_table_ints(int in_size, int out_size, int filter) {
  SGR_REQUIRE(in_size > 0 && out_size > 0 && in_size <= kMaxSize && out_size <= kMaxSize, "sgr_pil_resize_table_ints: sizes must be in 1 .. 2^24");
  SGR_REQUIRE(filter != 0, "sgr_pil_resize_table_ints: filter 0 (nearest) is a different PIL code path without coefficients: not offered");
  SGR_REQUIRE(filter_known(filter), "sgr_pil_resize_table_ints: unknown filter (PIL's codes: 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)");
  return table_ints(in_size, out_size, filter);
}

extern "C" int sgr_pil_resize_table(int in_size, int out_size, int filter, int* table) {
  SGR_REQUIRE(table, "sgr_pil_resize_table: NULL table");
  SGR_REQUIRE(in_size > 0 && out_size > 0 && in_size <= kMaxSize && out_size <= kMaxSize, "sgr_pil_resize_table: sizes must be in 1 .. 2^24");
  SGR_REQUIRE(filter != 0, "sgr_pil_resize_table: filter 0 (nearest) is a different PIL code path without coefficients: not offered");
  SGR_REQUIRE(filter_known(filter), "sgr_pil_resize_table: unknown filter (PIL's codes: 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)");
  SGR_SUPPORTED(build_table(in_size, out_size, filter, table) == 0, "sgr_pil_resize_table: a row of coefficients has 2^21 + 255 sum |k| > 2^31 - 1: the int32 sum could overflow");
  return SGR_OK;
}

extern "C" long long sgr_pil_resize_workspace_bytes(int bn, int H, int W, int C, int outH, int outW, const int* window, int filter) {
  note_pending_error();
  PrGeom g;
  const int rc = pr_check("sgr_pil_resize_workspace_bytes", bn, H, W, C, outH, outW, window, filter, &g);
  if (rc != SGR_OK) return rc;
  if (!(g.hpass && g.vpass)) return 0;
  return (long long)bn * (g.j.yb - g.j.ya) * tmp_pitch(g.j);
}

extern "C" int sgr_pil_resize_tiled_fits(int H, int W, int C, int outH, int outW, const int* window, int filter) {
  note_pending_error();
  PrGeom g;
  const int rc = pr_check("sgr_pil_resize_tiled_fits", 1, H, W, C, outH, outW, window, filter, &g);
  if (rc != SGR_OK) return rc;
  return plan_tiles(g.j, filter).fits ? 1 : 0;
}

extern "C" int sgr_pil_resize_route(int bn, int H, int W, int C, int outH, int outW, const int* window, int filter) {
  note_pending_error();
  PrGeom g;
  const int rc = pr_check("sgr_pil_resize_route", bn, H, W, C, outH, outW, window, filter, &g);
  if (rc != SGR_OK) return rc;
  return auto_tiled(g.j, plan_tiles(g.j, filter), bn) ? SGR_PIL_RESIZE_TILED : SGR_PIL_RESIZE_TWO_PASS;
}

extern "C" int sgr_pil_resize_u8(const unsigned char* src, int bn, int H, int W, int C, unsigned char* dst, int outH, int outW, const int* window, int filter,
                                 const int* htable, const int* vtable, unsigned char* workspace, int path, void* stream) {
  SGR_REQUIRE(src && dst, "sgr_pil_resize_u8: NULL tensor");
  PrGeom g;
  const int rc = pr_check("sgr_pil_resize_u8", bn, H, W, C, outH, outW, window, filter, &g);
  if (rc != SGR_OK) return rc;
  SGR_REQUIRE(path == SGR_PIL_RESIZE_AUTO || path == SGR_PIL_RESIZE_TWO_PASS || path == SGR_PIL_RESIZE_TILED, "sgr_pil_resize_u8: path must be 0 (auto), 1 (two_pass) or 2 (tiled)");
  SGR_REQUIRE((!g.hpass || htable) && (!g.vpass || vtable), "sgr_pil_resize_u8: NULL table for a pass that runs (sgr_pil_resize_table builds it; device memory)");
  const Job& j = g.j;
  const TilePlan plan = plan_tiles(j, filter);
  SGR_SUPPORTED(path != SGR_PIL_RESIZE_TILED || plan.fits,
                "sgr_pil_resize_u8: path tiled: this geometry does not fit the tiles (both passes must run, ksize <= 32 on both axes, the source extent of a 16 x 64 tile within "
                "24 KiB); use auto or two_pass");
  const bool tiled = path == SGR_PIL_RESIZE_TILED || (path == SGR_PIL_RESIZE_AUTO && auto_tiled(j, plan, bn));
  SGR_REQUIRE(tiled || !(g.hpass && g.vpass) || workspace, "sgr_pil_resize_u8: NULL workspace (sgr_pil_resize_workspace_bytes)");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  const int words = (j.ww * C + 3) / 4;
  const dim3 row_grid(j.wh, (words + kThreads - 1) / kThreads, bn);
  if (!g.hpass && !g.vpass) {
    hipLaunchKernelGGL(pr_copy_kernel, row_grid, block, 0, s, j, src, dst);
  } else if (tiled) {
    const dim3 grid((j.ww + kTileW - 1) / kTileW, (j.wh + kTileH - 1) / kTileH, bn);
    with_flag(C == 3, [&](auto C3) {
      with_flag(j.ksH <= kKReg, [&](auto REG) { hipLaunchKernelGGL((pr_tiled_kernel<C3() ? 3 : 1, REG()>), grid, block, 0, s, j, plan, src, htable, vtable, dst); });
    });
  } else {
    const unsigned char* vin = src + (size_t)j.c0 * C;      // the vertical pass alone reads the window's columns of the source
    size_t vin_stride = (size_t)H * W * C;
    int vpitch = W * C;
    Job jv = j;
    if (g.hpass) {
      unsigned char* out = g.vpass ? workspace : dst;
      const int opitch = g.vpass ? tmp_pitch(j) : j.ww * C;
      const size_t out_stride = (size_t)(j.yb - j.ya) * opitch;
      const dim3 grid((j.ww + kHCols - 1) / kHCols, (j.yb - j.ya + kHRows - 1) / kHRows, bn);
      with_flag(C == 3, [&](auto C3) {
        with_flag(j.ksH <= kKReg, [&](auto REG) { hipLaunchKernelGGL((pr_hpass_kernel<C3() ? 3 : 1, REG()>), grid, block, 0, s, j, src, htable, out, opitch, out_stride); });
      });
      vin = workspace;
      vin_stride = out_stride;
      vpitch = opitch;
    } else {
      jv.ya = 0;      // the rows the pass may read: the whole source
      jv.yb = H;
    }
    if (g.vpass) {
      const bool vec = vpitch % 4 == 0 && vin_stride % 4 == 0 && ((uintptr_t)vin & 3) == 0;
      with_flag(vec, [&](auto VEC) { hipLaunchKernelGGL((pr_vpass_kernel<VEC()>), row_grid, block, 0, s, jv, vin, vin_stride, vpitch, vtable, dst); });
    }
  }
  return sgr_check((int)hipGetLastError(), "sgr_pil_resize_u8");
}
