// Which number meets which in the light decoders' final pad + 3x3 convolution (sgr_light_final_conv.hip): ReplicationPad2d(1) followed by
// Conv2d(C -> O, k = 3), models.py:297-302, 334, with O = SGNum or 3 SGNum.  All three products run on the fp32-input matrix
// instruction v_mfma_f32_16x16x4_f32, which is bit for bit a k-ordered fmaf chain, so the fragment maps, the K orderings, the LDS addresses a
// lane reads and the accumulation orders below ARE the arithmetic.  `__host__ __device__`: the gfx950 kernels call these functions and so
// does the host emulation (tests/host_emul/light_final_conv_emul.cpp, test infrastructure only -- the product has no CPU path).  The index
// rule (fc_cl, fc_pairs, fc_gather_taps) is sgr_final_conv.h's.  DESIGN.md
// section 8h states the contract.
#pragma once

#include "sgr_final_conv.h"

namespace sgr {

constexpr int kLfMaxO = 48;        // output channels, at most: three N tiles of 16
constexpr int kLfMinC = 16;        // input channels: a multiple of 16 in [16, 256]
constexpr int kLfMaxC = 256;

// ---- v_mfma_f32_16x16x4_f32, D = A B + C with A [16 x 4], B [4 x 16], C / D [16 x 16]: what lane l of the wave holds --------------------
// A: one float, A[row = l & 15][k = l >> 4].  B: one float, B[k = l >> 4][col = l & 15].  C / D: four floats, register r is
// D[row = 4 (l >> 4) + r][col = l & 15].  D[i][j] = fmaf(A[i][3], B[3][j], fmaf(A[i][2], B[2][j], fmaf(A[i][1], B[1][j], fmaf(A[i][0], B[0][j], C[i][j])))).
SGR_HD int lf_a_row(int l) { return l & 15; }
SGR_HD int lf_a_k(int l) { return l >> 4; }
SGR_HD int lf_b_k(int l) { return l >> 4; }
SGR_HD int lf_b_col(int l) { return l & 15; }
SGR_HD int lf_d_row(int l, int r) { return 4 * (l >> 4) + r; }
SGR_HD int lf_d_col(int l) { return l & 15; }

// ---- FORWARD: M = pixels, N = O padded to 16 NT with zero weights, K = 9 C ---------------------------------------------------------------
// A workgroup (4 waves) owns a 32 x 8 pixel tile of one image; wave w owns rows 2w and 2w + 1 as four M tiles of 16 pixels: M tile m is
// row 2w + (m >> 1), columns 16 (m & 1) .. + 15, and row i of the MFMA is column 16 (m & 1) + i.  Column j of N tile n is output 16 n + j.
// The channels are walked in chunks of 8.  Inside a chunk the k index is q = tap * 8 + cc (tap = 3 kh + kw, cc the channel in the chunk),
// 72 of them = 18 MFMA steps; step s holds q = 4 s + (l >> 4): one tap, four channels.
// ORDER, one output:  run = 0;  for every chunk in turn:  t = 0;  for q = 0 .. 71:  t = fmaf(y[c0 + cc, cl(i+kh-1), cl(j+kw-1)], Wt[o, c0 + cc, kh, kw], t);
//                     run += t;   out = run + bias[o]
// (a chain of 72, then 16 additions at C = 128: one chain of 9 C terms loses about three times as much to rounding)
constexpr int kLfTW = 32, kLfTH = 8;            // the workgroup's pixel tile
constexpr int kLfKC = 8;                        // channels per chunk
constexpr int kLfSteps = 9 * kLfKC / 4;         // MFMA steps per chunk
constexpr int kLfPitch = kLfTW + 2;             // LDS row pitch of the map tile with its halo, floats
constexpr int kLfRows = kLfTH + 2;
constexpr int kLfPlane = 368;                   // floats per channel: 340 padded so that 368 mod 64 = 48 -- the four channels of a step start
                                                // 48, 32, 16 banks apart and a wave's 64 reads (16 consecutive floats each) hit 64 banks
SGR_HD int lf_fwd_tile_row(int wave, int m) { return 2 * wave + (m >> 1); }
SGR_HD int lf_fwd_tile_col(int m) { return 16 * (m & 1); }
SGR_HD int lf_fwd_q_tap(int q) { return q / kLfKC; }
SGR_HD int lf_fwd_q_cc(int q) { return q % kLfKC; }
// LDS index of halo element (row r of 10, column col of 34) of channel cc of the chunk
SGR_HD int lf_fwd_tile_idx(int cc, int r, int col) { return cc * kLfPlane + r * kLfPitch + col; }
// pitch of the weight tile [q][o]: 16 NT, except 48 for NT = 2 (32 would put steps' k = 0, 2 and k = 1, 3 on the same banks)
SGR_HD constexpr int lf_wpitch(int NT) { return NT == 2 ? 48 : 16 * NT; }
SGR_HD int lf_fwd_w_idx(int q, int o, int wp) { return q * wp + o; }
// what lane l reads for step s: its A operand for M tile m of wave `wave`, its B operand for N tile n
SGR_HD int lf_fwd_a_addr(int l, int s, int wave, int m) {
  const int q = 4 * s + lf_a_k(l), tap = lf_fwd_q_tap(q), kh = tap / 3, kw = tap - 3 * kh;
  return lf_fwd_tile_idx(lf_fwd_q_cc(q), lf_fwd_tile_row(wave, m) + kh, lf_fwd_tile_col(m) + lf_a_row(l) + kw);
}
SGR_HD int lf_fwd_b_addr(int l, int s, int n, int wp) { return lf_fwd_w_idx(4 * s + lf_b_k(l), 16 * n + lf_b_col(l), wp); }

// ---- BACKWARD, DATA: M = pixels, N = C, K = 9 O ------------------------------------------------------------------------------------------
// A workgroup owns a 32 x 4 pixel tile; wave w owns row w as two M tiles of 16 columns (row i of the MFMA is column 16 m + i); column j of N
// tile n is channel c0p + 16 n + j, at most 8 N tiles (128 channels) per workgroup -- C = 256 takes two.  The outputs are walked in groups
// of 4: group jg holds o = 4 jg + u, u = 0 .. 3 (an o >= O contributes exact zeros).  Inside a group the k index is q = tap * 4 + u, 36 of
// them = 9 MFMA steps; step `tap` holds u = l >> 4.  The A operand is G[o][tap] of fc_gather_taps at the lane's pixel, the B operand
// Wt[o, c, tap].
// ORDER, one dy:  run = 0;  for every group in turn:  t = 0;  for tap, for u:  t = fmaf(G[4 jg + u][tap], Wt[4 jg + u, c, tap], t);   run += t
constexpr int kLfTHb = 4;
constexpr int kLfGRows = kLfTHb + 2;
constexpr int kLfGPlane = 208;                  // floats per cotangent plane of a group: 6 x 34 = 204 padded, 208 mod 64 = 16
constexpr int kLfCP = 144;                      // pitch of the weight tile [q][c]: 128 + 16, 144 mod 64 = 16
constexpr int kLfPassC = 128;                   // channels per workgroup
SGR_HD int lf_bwd_g_idx(int u, int r, int col) { return u * kLfGPlane + r * kLfPitch + col; }
SGR_HD int lf_bwd_w_idx(int tap, int u, int c) { return (tap * 4 + u) * kLfCP + c; }
SGR_HD int lf_bwd_b_addr(int l, int tap, int n) { return lf_bwd_w_idx(tap, lf_b_k(l), 16 * n + lf_b_col(l)); }
// the A operands of one lane for the nine steps of a group: its pixel (h, w) -- clamped into the map by the caller --, the tile's origin
// (y0, x0), gt the group's cotangent tile with halo; plane u = l >> 4
SGR_HD void lf_bwd_a_operands(const float* gt, int l, int h, int w, int y0, int x0, int H, int W, float (&G)[9]) {
  const FcPairs rows = fc_pairs(h, H), cols = fc_pairs(w, W);
  float gv[3][3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) gv[p][q] = gt[lf_bwd_g_idx(lf_a_k(l), rows.i[p] - y0 + 1, cols.i[q] - x0 + 1)];
  fc_gather_taps(gv, rows, cols, G);
}

// ---- BACKWARD, WEIGHTS: M = 9 C, N = O padded to 16 NT, K = pixels -------------------------------------------------------------------------
// A workgroup owns one image, a block of 16 CBT channels and a strip of 10 consecutive 32 x 4 pixel tiles (in the raster order of the
// tiles).  An accumulator tile is (channel sub-block cb, tap, N tile n): row i of the MFMA is channel 16 cb + i, column j is output 16 n + j;
// the NT tiles of pair pr = cb * 9 + tap belong to wave pr mod 4, which reads the pair's A operand once for all of them.  The A operand is y[c, cl(i+kh-1), cl(j+kw-1)] from the map tile with its halo,
// the B operand g[o, i, j] from the cotangent tile, which holds exact zeros outside the map and for o >= O.  Inside a pixel tile the k
// index is the pixel p = 32 row + column, in two halves of 64 = 16 MFMA steps each; step s of half hf holds p = 64 hf + 4 s + (l >> 4).
// ORDER, one dWt:  run = 0;  for every tile of the strip, for hf = 0, 1:  t = 0;  for p = 64 hf .. 64 hf + 63:  t = fmaf(y.., g[o, p], t);   run += t
//                  then the strips' fp32 partials are added in double in index order (b, then strip)
constexpr int kLfTHw = 4;
constexpr int kLfWRows = kLfTHw + 2;
constexpr int kLfWPlane = 260;                  // floats per channel of the map tile: 6 x 34 = 204 padded, 260 mod 64 = 4 -- the 16 channels of
constexpr int kLfWGP = 132;                     // a step start 4 banks apart, its 4 pixels are consecutive; the cotangent tile [o][128 + 4] likewise
constexpr int kLfWStrip = 10;                   // pixel tiles per workgroup
SGR_HD int lf_w_y_idx(int cc, int r, int col) { return cc * kLfWPlane + r * kLfPitch + col; }
SGR_HD int lf_w_g_idx(int o, int p) { return o * kLfWGP + p; }
SGR_HD int lf_w_pair_cb(int pr) { return pr / 9; }
SGR_HD int lf_w_pair_tap(int pr) { return pr % 9; }
SGR_HD int lf_w_a_addr(int l, int s, int hf, int cb, int tap) {
  const int p = 64 * hf + 4 * s + lf_a_k(l), kh = tap / 3, kw = tap - 3 * kh;
  return lf_w_y_idx(16 * cb + lf_a_row(l), (p >> 5) + kh, (p & 31) + kw);
}
SGR_HD int lf_w_b_addr(int l, int s, int hf, int n) { return lf_w_g_idx(16 * n + lf_b_col(l), 64 * hf + 4 * s + lf_b_k(l)); }

// ---- BACKWARD, BIAS: on the vector ALU, three outputs at a time ----------------------------------------------------------------------------
// A thread adds the cotangents of its strip (8 runs of 4 pixels) in raster order in fp32, the threads of a workgroup are added by block_sum
// and the workgroups' partials in double in index order (b, then strip).  Output triplet t holds o = 3 t .. 3 t + 2.
SGR_HD int lf_triplets(int O) { return (O + 2) / 3; }

}  // namespace sgr
