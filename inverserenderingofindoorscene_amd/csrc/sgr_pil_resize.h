// PIL's antialiased resize of 8-bit images (Pillow's ImagingResample, libImaging/Resample.c) -- the arithmetic, the coefficient tables, the tile
// decisions and the per-thread bodies of the kernels, as host / device inline code.  sgr_pil_resize.hip wraps the bodies in kernels; the host
// test program (tests/host_emul/pil_resize_main.cpp) runs the SAME bodies thread by thread over exactly-sized heap buffers under the address
// and undefined-behaviour sanitizers, which is how "no index leaves the source or the tiles" is shown.  DESIGN.md section 8p has the contract.
//
// A table for one axis (ints): [0] ksize, [1] wide (1: some |k| >= 2^23, the kernels then multiply in 32 bits instead of 24), [2] inSize,
// [3] outSize, then bounds [out][2] = (xmin, xmax), then kk [out][ksize] (fixed point, 22 fractional bits; zero past xmax).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SGR_PR_HD __host__ __device__ __forceinline__
#define SGR_PR_UNROLL _Pragma("unroll")
#else
#define SGR_PR_HD inline
#define SGR_PR_UNROLL
#endif

namespace sgr {
namespace pr {

constexpr int kPrecisionBits = 22;
constexpr int kHeader = 4;
constexpr int kMaxSize = 1 << 24;      // per axis, source and target
// PIL's filter codes (Image.Resampling); 0 is NEAREST, another code path of PIL's (no coefficients): not offered
enum { kLanczos = 1, kBilinear = 2, kBicubic = 3, kBox = 4, kHamming = 5 };

// ---- the table (host, double, libm's sin / cos as PIL) --------------------------------------------------------------------------------------
static inline bool filter_known(int filter) { return filter >= kLanczos && filter <= kHamming; }
static inline double support_of(int filter) {
  switch (filter) {
    case kLanczos: return 3.0;
    case kBilinear: return 1.0;
    case kBicubic: return 2.0;
    case kBox: return 0.5;
    case kHamming: return 1.0;
  }
  return 0.0;
}

// No fused multiply-add in the filters: PIL's build evaluates them operation by operation.
#if defined(__clang__)
#define SGR_PR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SGR_PR_NO_CONTRACT
#endif

static inline double sinc_filter(double x) {
  SGR_PR_NO_CONTRACT
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
static inline double filter_value(int filter, double x) {
  SGR_PR_NO_CONTRACT
  switch (filter) {
    case kLanczos:
      if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
      return 0.0;
    case kBilinear:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case kBicubic: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    case kBox:
      return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case kHamming:
      if (x < 0.0) x = -x;
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54 + 0.46 * cos(x));
  }
  return 0.0;
}

struct Axis { double scale, filterscale, support; int in, out, ksize; };
struct Bound { int xmin, xmax; };

static inline Axis axis_of(int in, int out, int filter) {
  SGR_PR_NO_CONTRACT
  Axis a;
  a.in = in;
  a.out = out;
  a.scale = a.filterscale = (double)in / out;
  if (a.filterscale < 1.0) a.filterscale = 1.0;
  a.support = support_of(filter) * a.filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}
static inline double center_of(const Axis& a, int xx) {
  SGR_PR_NO_CONTRACT
  return 0.0 + (xx + 0.5) * a.scale;
}
static inline Bound bound_of(const Axis& a, int xx) {
  SGR_PR_NO_CONTRACT
  const double center = center_of(a, xx);
  Bound b;
  b.xmin = (int)(center - a.support + 0.5);
  if (b.xmin < 0) b.xmin = 0;
  b.xmax = (int)(center + a.support + 0.5);
  if (b.xmax > a.in) b.xmax = a.in;
  b.xmax -= b.xmin;
  return b;
}
static inline long long table_ints(int in, int out, int filter) { return kHeader + 2ll * out + (long long)out * axis_of(in, out, filter).ksize; }

// 0: built.  1: a row's sum could leave int32 (2^21 + 255 sum |k| > 2^31 - 1): refused, the table is not to be used.
static inline int build_table(int in, int out, int filter, int* table) {
  SGR_PR_NO_CONTRACT
  const Axis a = axis_of(in, out, filter);
  int* bounds = table + kHeader;
  int* kk = bounds + 2 * (size_t)out;
  double* w = (double*)malloc(sizeof(double) * (size_t)a.ksize);
  const double ss = 1.0 / a.filterscale;      // PIL multiplies by the reciprocal
  long long max_abs = 0, max_sum = 0;
  for (int xx = 0; xx < out; ++xx) {
    const double center = center_of(a, xx);
    const Bound b = bound_of(a, xx);
    double ww = 0.0;
    for (int x = 0; x < b.xmax; ++x) {
      w[x] = filter_value(filter, (x + b.xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int* k = kk + (size_t)xx * a.ksize;
    long long sum = 0;
    for (int x = 0; x < a.ksize; ++x) {
      int v = 0;
      if (x < b.xmax) {
        double c = w[x];
        if (ww != 0.0) c /= ww;
        v = c < 0 ? (int)(-0.5 + c * (1 << kPrecisionBits)) : (int)(0.5 + c * (1 << kPrecisionBits));
      }
      k[x] = v;
      const long long av = v < 0 ? -(long long)v : (long long)v;
      sum += av;
      if (av > max_abs) max_abs = av;
    }
    if (sum > max_sum) max_sum = sum;
    bounds[2 * xx] = b.xmin;
    bounds[2 * xx + 1] = b.xmax;
  }
  free(w);
  table[0] = a.ksize;
  table[1] = max_abs >= (1ll << 23) ? 1 : 0;
  table[2] = in;
  table[3] = out;
  return (1ll << (kPrecisionBits - 1)) + 255 * max_sum > 2147483647ll ? 1 : 0;
}

// ---- the pass arithmetic ---------------------------------------------------------------------------------------------------------------------
// acc + px * k; M24: |k| < 2^23 (the table's header says so) and px is a byte, so the 24-bit multiply-add holds the product
template <bool M24>
SGR_PR_HD int mac(int acc, int px, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return M24 ? __mul24(px, k) + acc : px * k + acc;
#else
  return px * k + acc;
#endif
}
constexpr int kHalf = 1 << (kPrecisionBits - 1);
SGR_PR_HD int clip8(int ss) {
  const int v = ss >> kPrecisionBits;      // arithmetic shift of the signed sum
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
SGR_PR_HD int imin(int a, int b) { return a < b ? a : b; }
SGR_PR_HD int imax(int a, int b) { return a > b ? a : b; }
SGR_PR_HD int iclamp(int v, int lo, int hi) { return imin(imax(v, lo), hi); }
SGR_PR_HD int round4(int v) { return (v + 3) & ~3; }

// What one launch works on: image b of the batch.  The output window is rows r0 .. r0 + wh - 1, columns c0 .. c0 + ww - 1 of the resized image.
struct Job {
  int H, W, C;            // source
  int outH, outW;         // the whole resized image
  int r0, c0, wh, ww;     // the window
  int ksH, ksV;           // the tables' ksize (0: that pass does not run)
  int ya, yb;             // the source rows the window's rows read (both passes: the rows the horizontal pass visits)
};

// The source rows [ya, yb) of output rows r0 .. r0 + wh - 1 (xmin and xmin + xmax do not decrease with the output index).
static inline void needed_rows(int H, int outH, int filter, int r0, int wh, int* ya, int* yb) {
  const Axis a = axis_of(H, outH, filter);
  const Bound f = bound_of(a, r0), l = bound_of(a, r0 + wh - 1);
  *ya = f.xmin;
  *yb = l.xmin + l.xmax;
}

// ---- the two-pass route ----------------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kKReg = 16;             // taps a lane of the horizontal pass keeps in registers
constexpr int kHRowsPerWave = 8, kHRows = 4 * kHRowsPerWave, kHCols = 64;

// Bounds from a table on the device, cut to what may be read: a genuine table passes unchanged, any other cannot leave the source.
SGR_PR_HD Bound safe_bound(const int* table, int xx, int in, int ksize) {
  const int* b = table + kHeader + 2 * (size_t)xx;
  Bound r;
  r.xmin = iclamp(b[0], 0, in);
  r.xmax = iclamp(b[1], 0, imin(ksize, in - r.xmin));
  return r;
}
SGR_PR_HD const int* taps_of(const int* table, int out, int xx, int ksize) { return table + kHeader + 2 * (size_t)out + (size_t)xx * ksize; }

// Horizontal pass from global memory: workgroup (bx, by) forms columns c0 + bx * 64 .. of source rows ya + by * 32 ..; a lane owns one output
// column and walks its wave's eight rows with the taps in registers (ksize <= 16) or from the table.  src: image b; out: row (y - ya) of
// `out` starts at out + (y - ya) * opitch, column (xx - c0) at byte (xx - c0) * C.
template <int C, bool REG, bool M24>
SGR_PR_HD void hpass_global_thread(const Job& j, const unsigned char* src, const int* htab, unsigned char* out, int opitch, int bx, int by, int t) {
  const int lane = t & 63, wave = t >> 6;
  const int col = bx * kHCols + lane;
  if (col >= j.ww) return;
  const int xx = j.c0 + col;
  const Bound b = safe_bound(htab, xx, j.W, j.ksH);
  const int* kp = taps_of(htab, j.outW, xx, j.ksH);
  int k[kKReg] = {};
  if (REG) {
SGR_PR_UNROLL
    for (int x = 0; x < kKReg; ++x) k[x] = x < b.xmax ? kp[x] : 0;
  }
  const int row0 = j.ya + by * kHRows + wave * kHRowsPerWave;
  for (int r = 0; r < kHRowsPerWave; ++r) {
    const int y = row0 + r;
    if (y >= j.yb) break;
    const unsigned char* s = src + ((size_t)y * j.W + b.xmin) * C;
    int acc[C];
SGR_PR_UNROLL
    for (int c = 0; c < C; ++c) acc[c] = kHalf;
    if (REG) {
      if (b.xmax > 0) {
SGR_PR_UNROLL
        for (int x = 0; x < kKReg; ++x) {
          const int xi = imin(x, b.xmax - 1) * C;      // past xmax the tap is zero and the pixel read again is the last one
SGR_PR_UNROLL
          for (int c = 0; c < C; ++c) acc[c] = mac<M24>(acc[c], s[xi + c], k[x]);
        }
      }
    } else {
      for (int x = 0; x < b.xmax; ++x) {
        const int kx = kp[x];
SGR_PR_UNROLL
        for (int c = 0; c < C; ++c) acc[c] = mac<M24>(acc[c], s[x * C + c], kx);
      }
    }
    unsigned char* o = out + (size_t)(y - j.ya) * opitch + (size_t)col * C;
SGR_PR_UNROLL
    for (int c = 0; c < C; ++c) o[c] = (unsigned char)clip8(acc[c]);
  }
}

// Four consecutive bytes of an output row to global memory: one 32-bit store where the address allows, bytes otherwise.  n: how many are valid.
SGR_PR_HD void store4(unsigned char* p, const int v[4], int n) {
  if (n >= 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
    for (int i = 0; i < 4; ++i)
      if (i < n) p[i] = (unsigned char)v[i];
  }
}

// Vertical pass from global memory: workgroup (bx, row) forms bytes bx * 1024 .. of output row r0 + row; a thread owns four consecutive
// bytes (columns times channel).  The taps and ymin depend on the row alone: uniform over the workgroup.  in: row y of the pass's input starts
// at in + (y - j.ya) * ipitch (the window's first byte already added by the caller).  VEC: ipitch % 4 == 0 and `in` on a 4-byte boundary.
template <bool VEC, bool M24>
SGR_PR_HD void vpass_global_thread(const Job& j, const unsigned char* in, int ipitch, const int* vtab, unsigned char* dst, int bx, int row, int t) {
  const int nbytes = j.ww * j.C;
  const int b0 = (bx * kThreads + t) * 4;
  if (b0 >= nbytes) return;
  const int n = imin(4, nbytes - b0);
  const int yy = j.r0 + row;
  Bound b = safe_bound(vtab, yy, j.H, j.ksV);
  b.xmin = iclamp(b.xmin, j.ya, j.yb);      // a genuine table stays inside the rows [ya, yb) the caller holds
  b.xmax = imin(b.xmax, j.yb - b.xmin);
  const int* kp = taps_of(vtab, j.outH, yy, j.ksV);
  int acc[4] = {kHalf, kHalf, kHalf, kHalf};
  const unsigned char* s = in + (size_t)(b.xmin - j.ya) * ipitch + b0;
  for (int x = 0; x < b.xmax; ++x, s += ipitch) {
    const int kx = kp[x];
    if (VEC && n == 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(s);
      acc[0] = mac<M24>(acc[0], (int)(w & 255u), kx);
      acc[1] = mac<M24>(acc[1], (int)((w >> 8) & 255u), kx);
      acc[2] = mac<M24>(acc[2], (int)((w >> 16) & 255u), kx);
      acc[3] = mac<M24>(acc[3], (int)(w >> 24), kx);
    } else {
      for (int i = 0; i < 4; ++i)
        if (i < n) acc[i] = mac<M24>(acc[i], s[i], kx);
    }
  }
  int v[4];
  for (int i = 0; i < 4; ++i) v[i] = clip8(acc[i]);
  store4(dst + (size_t)row * nbytes + b0, v, n);
}

// Equal sizes: the window's bytes, copied.
SGR_PR_HD void copy_thread(const Job& j, const unsigned char* src, unsigned char* dst, int bx, int row, int t) {
  const int nbytes = j.ww * j.C;
  const int b0 = (bx * kThreads + t) * 4;
  if (b0 >= nbytes) return;
  const int n = imin(4, nbytes - b0);
  const unsigned char* s = src + ((size_t)(j.r0 + row) * j.W + j.c0) * j.C + b0;
  int v[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i)
    if (i < n) v[i] = s[i];
  store4(dst + (size_t)row * nbytes + b0, v, n);
}

// ---- the tiled route -------------------------------------------------------------------------------------------------------------------------
// A workgroup owns kTileH x kTileW output pixels.  S: the tile's source extent, packed bytes, each row at the SAME offset from a 4-byte boundary
// as in global memory (so the staging moves aligned 32-bit words); M: the horizontally resized rows as uint8, kTileW * C bytes a row; VT: the
// vertical taps of the tile's rows; HT (ksize > 16 only): the horizontal taps of the tile's columns, tap-major.
constexpr int kTileH = 16, kTileW = 64;
constexpr int kSrcBytes = 24 * 1024, kMidBytes = 12 * 1024;
constexpr int kKTile = 32;            // the largest ksize, either axis, the tiled route takes

struct TilePlan { int fits, pitch, cap_rows, cap_cols; };

// Does every tile of the window fit?  From the bounds alone (host, double: the same expressions the tables were built from).
static inline TilePlan plan_tiles(const Job& j, int filter) {
  TilePlan p = {0, 0, 0, 0};
  if (j.ksH <= 0 || j.ksV <= 0 || j.ksH > kKTile || j.ksV > kKTile) return p;      // both passes run, taps fit
  const Axis av = axis_of(j.H, j.outH, filter), ah = axis_of(j.W, j.outW, filter);
  int rows = 0, cols = 0;
  for (int y = j.r0; y < j.r0 + j.wh; y += kTileH) {
    const int yl = imin(y + kTileH, j.r0 + j.wh) - 1;
    const Bound f = bound_of(av, y), l = bound_of(av, yl);
    rows = imax(rows, l.xmin + l.xmax - f.xmin);
  }
  for (int x = j.c0; x < j.c0 + j.ww; x += kTileW) {
    const int xl = imin(x + kTileW, j.c0 + j.ww) - 1;
    const Bound f = bound_of(ah, x), l = bound_of(ah, xl);
    cols = imax(cols, l.xmin + l.xmax - f.xmin);
  }
  p.cap_rows = rows;
  p.cap_cols = cols;
  p.pitch = round4(cols * j.C + 3);
  p.fits = (long long)rows * p.pitch <= kSrcBytes && (long long)rows * kTileW * j.C <= kMidBytes;
  return p;
}

// What `auto` takes: the tiled route where it fits AND the launch has at least kAutoTiles workgroups.  Measured: at 1200
// tiles (batch 16 of 480 x 640 to 240 x 320) tiled is faster beyond the spread, at 75 (one IIW photograph) the spreads overlap; the threshold
// between the two measured points is one workgroup per compute unit of the MI355X.
constexpr int kAutoTiles = 256;
static inline bool auto_tiled(const Job& j, const TilePlan& p, int bn) {
  return p.fits && (long long)bn * ((j.ww + kTileW - 1) / kTileW) * ((j.wh + kTileH - 1) / kTileH) >= kAutoTiles;
}

struct Tile {
  int y0, ny, x0, nx;      // the tile's output rows and columns (indices of the resized image) and how many
  int ys0, nys;            // source rows staged
  int xs0, nxs;            // source columns staged
};
SGR_PR_HD Tile tile_of(const Job& j, const TilePlan& p, const int* htab, const int* vtab, int tx, int ty) {
  Tile t;
  t.y0 = j.r0 + ty * kTileH;
  t.ny = imin(kTileH, j.r0 + j.wh - t.y0);
  t.x0 = j.c0 + tx * kTileW;
  t.nx = imin(kTileW, j.c0 + j.ww - t.x0);
  const Bound yf = safe_bound(vtab, t.y0, j.H, j.ksV), yl = safe_bound(vtab, t.y0 + t.ny - 1, j.H, j.ksV);
  t.ys0 = yf.xmin;
  t.nys = iclamp(yl.xmin + yl.xmax - t.ys0, 0, p.cap_rows);
  const Bound xf = safe_bound(htab, t.x0, j.W, j.ksH), xl = safe_bound(htab, t.x0 + t.nx - 1, j.W, j.ksH);
  t.xs0 = xf.xmin;
  t.nxs = iclamp(xl.xmin + xl.xmax - t.xs0, 0, p.cap_cols);
  return t;
}
// where staged row r begins in global memory, and how far that is from the 4-byte boundary below it
SGR_PR_HD const unsigned char* row_start(const Job& j, const unsigned char* src, const Tile& t, int r) { return src + ((size_t)(t.ys0 + r) * j.W + t.xs0) * j.C; }
SGR_PR_HD int row_shift(const Job& j, const unsigned char* src, const Tile& t, int r) { return (int)((uintptr_t)row_start(j, src, t, r) & 3); }

// Phase 1: the source extent into S as aligned 32-bit words (bytes where a word would leave the image's memory), the vertical taps into VT
// and, for ksize > 16, the horizontal taps into HT.  lo / hi: the first byte of the image and the one past its last.
template <bool REG>
SGR_PR_HD void tile_stage_thread(const Job& j, const TilePlan& p, const Tile& t, const unsigned char* src, const int* htab, const int* vtab, unsigned char* S, int* VT,
                                 int* HT, int tid) {
  const unsigned char *lo = src, *hi = src + (size_t)j.H * j.W * j.C;
  const int words = p.pitch >> 2;
  for (int i = tid; i < t.nys * words; i += kThreads) {
    const int r = i / words, w = i - r * words;
    const unsigned char* g = row_start(j, src, t, r);
    const int shift = (int)((uintptr_t)g & 3);
    if (4 * w >= shift + t.nxs * j.C) continue;
    const unsigned char* a = g - shift + 4 * w;
    uint32_t v = 0;
    if (a >= lo && a + 4 <= hi) {
      v = *reinterpret_cast<const uint32_t*>(a);
    } else {
      for (int q = 0; q < 4; ++q)
        if (a + q >= lo && a + q < hi) v |= (uint32_t)a[q] << (8 * q);
    }
    *reinterpret_cast<uint32_t*>(S + (size_t)r * p.pitch + 4 * w) = v;
  }
  for (int i = tid; i < t.ny * j.ksV; i += kThreads) {
    const int ty = i / j.ksV, x = i - ty * j.ksV;
    VT[i] = taps_of(vtab, j.outH, t.y0 + ty, j.ksV)[x];
  }
  if (!REG) {
    for (int i = tid; i < j.ksH * kTileW; i += kThreads) {
      const int x = i / kTileW, lane = i - x * kTileW;
      HT[i] = lane < t.nx ? taps_of(htab, j.outW, t.x0 + lane, j.ksH)[x] : 0;
    }
  }
}

// Phase 2: the horizontal pass, S -> M.  A lane owns one output column of the tile, a wave every fourth staged row.
template <int C, bool REG, bool M24>
SGR_PR_HD void tile_hpass_thread(const Job& j, const TilePlan& p, const Tile& t, const unsigned char* src, const int* htab, const unsigned char* S, const int* HT,
                                 unsigned char* M, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  int xoff = 0, xmax = 0;
  int k[kKReg] = {};
  if (lane < t.nx) {
    const Bound b = safe_bound(htab, t.x0 + lane, j.W, j.ksH);
    xoff = iclamp(b.xmin - t.xs0, 0, t.nxs);
    xmax = imin(b.xmax, t.nxs - xoff);
    if (REG) {
      const int* kp = taps_of(htab, j.outW, t.x0 + lane, j.ksH);
SGR_PR_UNROLL
      for (int x = 0; x < kKReg; ++x) k[x] = x < xmax ? kp[x] : 0;
    }
  }
  for (int r = wave; r < t.nys; r += 4) {
    int acc[C];
SGR_PR_UNROLL
    for (int c = 0; c < C; ++c) acc[c] = kHalf;
    if (xmax > 0) {
      const unsigned char* s = S + (size_t)r * p.pitch + row_shift(j, src, t, r) + xoff * C;
      if (REG) {
SGR_PR_UNROLL
        for (int x = 0; x < kKReg; ++x) {
          const int xi = imin(x, xmax - 1) * C;
SGR_PR_UNROLL
          for (int c = 0; c < C; ++c) acc[c] = mac<M24>(acc[c], s[xi + c], k[x]);
        }
      } else {
        for (int x = 0; x < xmax; ++x) {
          const int kx = HT[x * kTileW + lane];
SGR_PR_UNROLL
          for (int c = 0; c < C; ++c) acc[c] = mac<M24>(acc[c], s[x * C + c], kx);
        }
      }
    }
    unsigned char* m = M + (size_t)r * (kTileW * C) + lane * C;
SGR_PR_UNROLL
    for (int c = 0; c < C; ++c) m[c] = lane < t.nx ? (unsigned char)clip8(acc[c]) : (unsigned char)0;
  }
}

// Phase 3: the vertical pass, M -> dst.  A thread owns four consecutive bytes of a tile row (one aligned word of M per tap); the taps come
// from VT, the same address for every lane of a row.
template <int C, bool M24>
SGR_PR_HD void tile_vpass_thread(const Job& j, const Tile& t, const int* vtab, const unsigned char* M, const int* VT, unsigned char* dst, int tid) {
  constexpr int kWords = kTileW * C / 4, kRowsPerIter = kThreads / kWords;
  const int w = tid % kWords, rr = tid / kWords;
  if (rr >= kRowsPerIter) return;
  const int n = iclamp(t.nx * C - 4 * w, 0, 4);
  if (n == 0) return;
  for (int ty = rr; ty < t.ny; ty += kRowsPerIter) {
    const int yy = t.y0 + ty;
    const Bound b = safe_bound(vtab, yy, j.H, j.ksV);
    const int yoff = iclamp(b.xmin - t.ys0, 0, t.nys);
    const int ymax = imin(b.xmax, t.nys - yoff);
    int acc[4] = {kHalf, kHalf, kHalf, kHalf};
    const unsigned char* m = M + (size_t)yoff * (kTileW * C) + 4 * w;
    const int* kp = VT + ty * j.ksV;
    for (int x = 0; x < ymax; ++x, m += kTileW * C) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(m);
      const int kx = kp[x];
      acc[0] = mac<M24>(acc[0], (int)(v & 255u), kx);
      acc[1] = mac<M24>(acc[1], (int)((v >> 8) & 255u), kx);
      acc[2] = mac<M24>(acc[2], (int)((v >> 16) & 255u), kx);
      acc[3] = mac<M24>(acc[3], (int)(v >> 24), kx);
    }
    int o[4];
    for (int i = 0; i < 4; ++i) o[i] = clip8(acc[i]);
    store4(dst + ((size_t)(yy - j.r0) * j.ww + (t.x0 - j.c0)) * C + 4 * w, o, n);
  }
}

}  // namespace pr
}  // namespace sgr
