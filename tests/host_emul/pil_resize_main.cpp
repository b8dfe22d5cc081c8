// Stand-alone host build of csrc/sgr_pil_resize.h: the kernels' per-thread bodies run thread by thread, workgroup by workgroup, over heap
// buffers of exactly the sizes the device code is given (the image at `misalign` bytes past an aligned address, the LDS tiles at the sizes the
// tile plan allows), so that the address and undefined-behaviour sanitizers see every index and every 32-bit access the kernels form.
//
//   pil_resize_main in.bin out.bin
//
// in.bin: 14 ints (bn, H, W, C, outH, outW, r0, c0, wh, ww, filter, path 1 two_pass | 2 tiled, misalign 0..3, tables 0 | 1) then the source
// bytes [bn,H,W,C].  out.bin: the window's bytes [bn,wh,ww,C]; with tables == 1 they are followed by the two tables' ints (horizontal,
// vertical; a pass that does not run has none).  Exit code 3: path tiled on a geometry that does not fit; 4: a table was refused.
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_pil_resize.h"

using namespace sgr::pr;

template <class F>
static void with_c_reg(int C, bool reg, F&& f) {
  if (C == 3) {
    if (reg) f(std::integral_constant<int, 3>{}, std::true_type{});
    else f(std::integral_constant<int, 3>{}, std::false_type{});
  } else {
    if (reg) f(std::integral_constant<int, 1>{}, std::true_type{});
    else f(std::integral_constant<int, 1>{}, std::false_type{});
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[14];
  if (fread(hd, sizeof(int), 14, f) != 14) return 2;
  const int bn = hd[0], H = hd[1], W = hd[2], C = hd[3], outH = hd[4], outW = hd[5], filter = hd[10], path = hd[11], misalign = hd[12], want_tables = hd[13];
  const size_t image = (size_t)H * W * C, n_src = image * bn;
  unsigned char* src_buf = (unsigned char*)malloc(n_src + misalign);      // the last image ends where the allocation ends
  unsigned char* src = src_buf + misalign;
  if (fread(src, 1, n_src, f) != n_src) return 2;
  fclose(f);

  Job j;
  j.H = H; j.W = W; j.C = C; j.outH = outH; j.outW = outW;
  j.r0 = hd[6]; j.c0 = hd[7]; j.wh = hd[8]; j.ww = hd[9];
  const bool hpass = outW != W, vpass = outH != H;
  j.ksH = hpass ? axis_of(W, outW, filter).ksize : 0;
  j.ksV = vpass ? axis_of(H, outH, filter).ksize : 0;
  if (vpass) {
    needed_rows(H, outH, filter, j.r0, j.wh, &j.ya, &j.yb);
  } else {
    j.ya = j.r0;
    j.yb = j.r0 + j.wh;
  }
  std::vector<int> htab(hpass ? (size_t)table_ints(W, outW, filter) : 0), vtab(vpass ? (size_t)table_ints(H, outH, filter) : 0);
  if (hpass && build_table(W, outW, filter, htab.data()) != 0) return 4;
  if (vpass && build_table(H, outH, filter, vtab.data()) != 0) return 4;

  const size_t out_image = (size_t)j.wh * j.ww * C;
  unsigned char* dst_buf = (unsigned char*)malloc(out_image * bn + misalign);
  unsigned char* dst = dst_buf + misalign;
  const int words = (j.ww * C + 3) / 4, row_blocks = (words + kThreads - 1) / kThreads;
  const TilePlan plan = plan_tiles(j, filter);
  if (path == 2 && !plan.fits) {
    free(src_buf);
    free(dst_buf);
    return 3;
  }

  for (int b = 0; b < bn; ++b) {
    const unsigned char* s = src + b * image;
    unsigned char* o = dst + b * out_image;
    if (!hpass && !vpass) {
      for (int row = 0; row < j.wh; ++row)
        for (int bx = 0; bx < row_blocks; ++bx)
          for (int t = 0; t < kThreads; ++t) copy_thread(j, s, o, bx, row, t);
    } else if (path == 2) {
      // the LDS tiles at exactly what the plan says a workgroup may touch
      unsigned char* S = (unsigned char*)malloc((size_t)plan.cap_rows * plan.pitch);
      unsigned char* M = (unsigned char*)malloc((size_t)plan.cap_rows * kTileW * C);
      int* VT = (int*)malloc(sizeof(int) * kTileH * j.ksV);
      int* HT = (int*)malloc(sizeof(int) * j.ksH * kTileW);
      if ((long long)plan.cap_rows * plan.pitch > kSrcBytes || (long long)plan.cap_rows * kTileW * C > kMidBytes || j.ksV > kKTile || j.ksH > kKTile) return 5;
      const int gx = (j.ww + kTileW - 1) / kTileW, gy = (j.wh + kTileH - 1) / kTileH;
      with_c_reg(C, j.ksH <= kKReg, [&](auto CC, auto REG) {
        for (int ty = 0; ty < gy; ++ty)
          for (int tx = 0; tx < gx; ++tx) {
            const Tile t = tile_of(j, plan, htab.data(), vtab.data(), tx, ty);
            for (int tid = 0; tid < kThreads; ++tid) tile_stage_thread<REG()>(j, plan, t, s, htab.data(), vtab.data(), S, VT, HT, tid);
            for (int tid = 0; tid < kThreads; ++tid) tile_hpass_thread<CC(), REG(), true>(j, plan, t, s, htab.data(), S, HT, M, tid);
            for (int tid = 0; tid < kThreads; ++tid) tile_vpass_thread<CC(), true>(j, t, vtab.data(), M, VT, o, tid);
          }
      });
      free(S);
      free(M);
      free(VT);
      free(HT);
    } else {
      const int opitch = vpass ? round4(j.ww * C) : j.ww * C;
      const size_t tmp_bytes = (size_t)(j.yb - j.ya) * opitch;
      unsigned char* tmp = hpass && vpass ? (unsigned char*)malloc(tmp_bytes) : nullptr;
      const unsigned char* vin = s + (size_t)j.c0 * C;
      int vpitch = W * C;
      Job jv = j;
      if (hpass) {
        unsigned char* out = vpass ? tmp : o;
        const int gx = (j.ww + kHCols - 1) / kHCols, gy = (j.yb - j.ya + kHRows - 1) / kHRows;
        with_c_reg(C, j.ksH <= kKReg, [&](auto CC, auto REG) {
          for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
              for (int t = 0; t < kThreads; ++t) hpass_global_thread<CC(), REG(), true>(j, s, htab.data(), out, opitch, bx, by, t);
        });
        vin = tmp;
        vpitch = opitch;
      } else {
        jv.ya = 0;
        jv.yb = H;
      }
      if (vpass) {
        const bool vec = vpitch % 4 == 0 && ((uintptr_t)vin & 3) == 0;      // per image here: its own first byte decides
        for (int row = 0; row < j.wh; ++row)
          for (int bx = 0; bx < row_blocks; ++bx)
            for (int t = 0; t < kThreads; ++t) {
              if (vec) vpass_global_thread<true, true>(jv, vin, vpitch, vtab.data(), o, bx, row, t);
              else vpass_global_thread<false, true>(jv, vin, vpitch, vtab.data(), o, bx, row, t);
            }
      }
      free(tmp);
    }
  }

  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(dst, 1, out_image * bn, f);
  if (want_tables) {
    fwrite(htab.data(), sizeof(int), htab.size(), f);
    fwrite(vtab.data(), sizeof(int), vtab.size(), f);
  }
  fclose(f);
  free(src_buf);
  free(dst_buf);
  return 0;
}
