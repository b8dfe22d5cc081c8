// Host build of the loader-preparation kernels' decisions (csrc/sgr_loader_prep.h): a stand-alone program, so that it can run under
// -fsanitize=address,undefined (tests/test_loader_prep.py compiles and runs it; nothing here is loaded into python).
//
//   loader_prep_main <input> : the input file holds   int32 n, int32 k, float[n]      -- a radix select as lp_select walks it
//                                                      int32 H, int32 W, uint8[H*W]    -- the mask codes of a plane
//   stdout: "v <bits of element k as hex>", "bits <256 x the mask bits of each byte value>", "obj <H*W x 0|1>" the eroded object mask,
//   built as lp_masks builds it: a plane padded by 3 with the set bit, the AND of 7 along x, then of 7 along y.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../inverserenderingofindoorscene_amd/csrc/sgr_loader_prep.h"

using namespace sgr::lp;

static float select_k(const std::vector<float>& x, unsigned k) {
  uint32_t prefix = 0;
  unsigned rank = k;
  for (int pass = 0; pass < kPasses; ++pass) {
    unsigned hist[kBuckets] = {0};
    for (float f : x) {
      const uint32_t key = key_of(f);
      if (in_prefix(key, prefix, pass)) ++hist[digit_of(key, pass)];
    }
    const int d = pick_bucket(hist, rank);
    prefix = (pass ? prefix << kRadixBits : 0u) | (unsigned)d;
  }
  return float_of(prefix);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0, k = 0, H = 0, W = 0;
  if (fread(&n, 4, 1, f) != 1 || fread(&k, 4, 1, f) != 1 || n <= 0 || k < 0 || k >= n) return 3;
  std::vector<float> x(n);
  if (fread(x.data(), 4, n, f) != (size_t)n) return 3;
  if (fread(&H, 4, 1, f) != 1 || fread(&W, 4, 1, f) != 1 || H <= 0 || W <= 0) return 3;
  std::vector<unsigned char> code((size_t)H * W);
  if (fread(code.data(), 1, code.size(), f) != code.size()) return 3;
  fclose(f);

  const float v = select_k(x, (unsigned)k);
  uint32_t vb;
  memcpy(&vb, &v, 4);
  printf("v %08x\n", vb);

  printf("bits");
  for (int u = 0; u < 256; ++u) printf(" %d", seg_bits(u));
  printf("\n");

  const int PW = W + 2 * kErodeR, PH = H + 2 * kErodeR;
  std::vector<unsigned char> tile((size_t)PH * PW, (unsigned char)kObj), hrow((size_t)PH * W);
  for (int y = 0; y < H; ++y)
    for (int xx = 0; xx < W; ++xx) tile[(size_t)(y + kErodeR) * PW + xx + kErodeR] = (unsigned char)seg_bits(code[(size_t)y * W + xx]);
  for (int y = 0; y < PH; ++y)
    for (int xx = 0; xx < W; ++xx) hrow[(size_t)y * W + xx] = (unsigned char)and7(&tile[(size_t)y * PW + xx], 1);
  printf("obj ");
  for (int y = 0; y < H; ++y)
    for (int xx = 0; xx < W; ++xx) putchar(and7(&hrow[(size_t)y * W + xx], W) ? '1' : '0');
  printf("\n");
  return 0;
}
