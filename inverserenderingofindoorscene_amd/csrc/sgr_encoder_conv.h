// Which number meets which in the encoders' pad + 4x4 stride-2 convolution (sgr_encoder_conv.hip): ReplicationPad2d(1) or ZeroPad2d(1)
// followed by Conv2d(C -> O, k = 4, stride = 2), models.py:93-115, 122-126, 213-246, 254-266.  The forward, the data gradient and the
// weight gradient run on the fp32-input matrix instruction v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain, so the index rule, the tile
// loops, the LDS addresses a lane reads, the K orderings and the accumulation orders below ARE the arithmetic.  `__host__ __device__`: the
// gfx950 kernels call these functions and so does the host emulation (tests/host_emul/encoder_conv_emul.cpp, test infrastructure only --
// the product has no CPU path).  The fragment maps (lf_a_row .. lf_d_col) are sgr_light_final_conv.h's.  DESIGN.md section 8i states the
// contract.
#pragma once

#include "sgr_light_final_conv.h"

namespace sgr {

constexpr int kEcMaxC = 160;       // input channels: 1 .. 160
constexpr int kEcMinO = 16;        // output channels: a multiple of 16 in 16 .. 128
constexpr int kEcMaxO = 128;
constexpr int kEcReplicate = 0, kEcZeros = 1;      // pad_mode

// ---- the index rule ------------------------------------------------------------------------------------------------------------------------
// the source index of padded index t - 1 (t = 2 i + kh - 1): clamped into the map (replicate), or -1 = absent, an exact zero (zeros)
SGR_HD int ec_src(int t, int n, int mode) {
  if (mode == kEcReplicate) return t < 0 ? 0 : t > n - 1 ? n - 1 : t;
  return t >= 0 && t < n ? t : -1;
}
SGR_HD int ec_out(int n) { return n >> 1; }      // floor((n + 2 - 4) / 2) + 1 for n >= 2

// ---- several sources: the convolution of their concatenation along the channels, which is never written ------------------------------------
// Source i holds the channels first .. first + C_i - 1 of the concatenation and is read through its own four strides.  The table travels in
// the kernel arguments (S <= 4); an unused entry has first = kEcNoSource, which no channel reaches.  The chunks, blocks and passes of the
// tile loops below are those of the concatenation, so a chunk may hold channels of two sources: the source is looked up per channel, where
// the channel is uniform across a wave (a scalar select chain, no indexed copy of the table).
// WHY THE BITS ARE THOSE OF THE CONCATENATION: which tensor a number is read from does not enter any ORDER below.  The forward and the
// weight gradient keep the concatenation's chunk and block boundaries, so every chain has the same terms in the same order.  The data
// gradient's chain of one element runs over k = (o, tap) only -- no channel is summed -- so a launch over one source's channel range
// (channel base `first`, the weight's row length still the total channel count) writes the bits of that slice of the concatenation's dx,
// whatever 64-channel pass the channel falls in.
constexpr int kEcMaxSources = 4;
constexpr int kEcNoSource = 0x7fffffff;
struct EcSource {
  const float* p;
  long long sb, sc, sh, sw;      // element strides of [B, C_i, H, W]
  int first;                     // the source's first channel in the concatenation
};
struct EcSources { EcSource s[kEcMaxSources]; };
// the source of channel c (0 <= c < the total): the last one whose first channel is <= c
SGR_HD EcSource ec_source_of(const EcSources& t, int c) {
  const float* p = t.s[0].p;
  long long sb = t.s[0].sb, sc = t.s[0].sc, sh = t.s[0].sh, sw = t.s[0].sw;
  int first = t.s[0].first;
#pragma unroll
  for (int i = 1; i < kEcMaxSources; ++i) {      // field by field: selects on scalars, never a copy of the table
    const bool hit = c >= t.s[i].first;
    p = hit ? t.s[i].p : p;
    sb = hit ? t.s[i].sb : sb;
    sc = hit ? t.s[i].sc : sc;
    sh = hit ? t.s[i].sh : sh;
    sw = hit ? t.s[i].sw : sw;
    first = hit ? t.s[i].first : first;
  }
  return EcSource{p, sb, sc, sh, sw, first};
}
// plane (b, c) of the concatenation: where it starts, in its source
SGR_HD const float* ec_source_plane(const EcSource& s, int b, int c) { return s.p + (long long)b * s.sb + (long long)(c - s.first) * s.sc; }
// element (sr, sc) of a plane of source s; sr or sc < 0 is an absent pad element (zeros mode): an exact zero.  Fits 31 bits (host check)
SGR_HD float ec_source_at(const EcSource& s, const float* plane, int sr, int sc) {
  return (sr < 0 || sc < 0) ? 0.0f : plane[(unsigned)sr * (unsigned)s.sh + (unsigned)sc * (unsigned)s.sw];
}

// R_n(h) = {(i, k): 0 <= i < n div 2, 0 <= k < 4, src(2 i + k - 1, n) == h}: never more than two members.  Slot 0 is the tap of h's own
// parity class k0 = (h + 1) & 1, slot 1 the tap k0 + 2; i = -1 marks a slot without a member.  In replicate mode row 0 gains (0, 0) and
// the last row of an even map gains (n/2 - 1, 3): the other parity's taps, in the slot the class leaves empty there.
struct EcPairs { int i[2], k[2]; };
SGR_HD EcPairs ec_pairs(int h, int n, int mode) {
  const int no = ec_out(n), k0 = (h + 1) & 1;
  EcPairs p;
  p.k[0] = k0;
  p.i[0] = (h + 1 - k0) >> 1;
  if (p.i[0] >= no) p.i[0] = -1;
  p.k[1] = k0 + 2;
  p.i[1] = h - 1 - k0 >= 0 ? (h - 1 - k0) >> 1 : -1;
  if (p.i[1] >= no) p.i[1] = -1;
  if (mode == kEcReplicate) {
    if (h == 0) { p.i[1] = 0; p.k[1] = 0; }
    else if (h == n - 1 && !(n & 1)) { p.i[0] = no - 1; p.k[0] = 3; }
  }
  return p;
}

// ---- FORWARD: M = output pixels, N = O, K = 16 C ---------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns a 32 x 8 tile of output pixels of one image and a pass of up to 64 outputs (O = 128 takes two workgroups);
// wave w owns output rows 2w and 2w + 1 as four M tiles of 16 pixels: M tile m is row 2w + (m >> 1), columns 16 (m & 1) .. + 15, and row
// jj of the MFMA is column 16 (m & 1) + jj.  Column j of N tile n is output o0 + 16 n + j.  The channels are walked in chunks of 4 (a
// channel >= C is a plane of exact zeros with zero weights).  Inside a chunk the k index is q = (cc * 4 + kh) * 4 + kw, 64 of them = 16
// MFMA steps; step s holds cc = s >> 2, kh = s & 3 and kw = l >> 4: the four kw taps of one (c, kh).
// ORDER, one output:  run = 0;  for every chunk in turn:  t = 0;  for q = 0 .. 63:  t = fmaf(x[c0 + cc, src(2i+kh-1), src(2j+kw-1)], Wt[o, c0 + cc, kh, kw], t);
//                     run += t;   out = run + bias[o]
// The input tile with its halo, 18 rows x 66 columns (tile column tc is map column 2 j0 - 1 + tc), lies in LDS as two planes per
// channel: the even tile columns and the odd ones, 33 floats a row.  Output column jj reads tile column 2 jj + kw = plane kw & 1, index
// jj + (kw >> 1): the 64 lanes of a step read indices x .. x + 16 of plane 0 and of plane 1, and the planes lie 608 = 32 (mod 64) floats
// apart -- 34 distinct addresses on banks x .. x + 16 and x + 32 .. x + 48, no two on one bank.
constexpr int kEcTW = 32, kEcTH = 8;             // the workgroup's output tile
constexpr int kEcKC = 4;                         // channels per chunk
constexpr int kEcSteps = 16 * kEcKC / 4;         // MFMA steps per chunk
constexpr int kEcPassO = 64, kEcPassNT = 4;      // outputs per workgroup
constexpr int kEcRows = 2 * kEcTH + 2;           // 18
constexpr int kEcCols = 2 * kEcTW + 2;           // 66
constexpr int kEcRP = kEcTW + 1;                 // 33: row pitch of a parity plane
constexpr int kEcEP = 608;                       // 18 x 33 = 594 padded: floats per parity plane
constexpr int kEcCHP = 2 * kEcEP;                // floats per channel
constexpr int kEcWP = 80;                        // pitch of the weight tile [q][o]: 64 + 16, the four k of a step start 16 banks apart
SGR_HD int ec_fwd_tile_row(int wave, int m) { return 2 * wave + (m >> 1); }
SGR_HD int ec_fwd_tile_col(int m) { return 16 * (m & 1); }
SGR_HD int ec_fwd_tile_idx(int cc, int r, int tc) { return cc * kEcCHP + (tc & 1) * kEcEP + r * kEcRP + (tc >> 1); }
SGR_HD int ec_fwd_w_idx(int q, int o) { return q * kEcWP + o; }
SGR_HD int ec_fwd_a_addr(int l, int s, int wave, int m) {
  const int cc = s >> 2, kh = s & 3, kw = lf_a_k(l);
  return ec_fwd_tile_idx(cc, 2 * ec_fwd_tile_row(wave, m) + kh, 2 * (ec_fwd_tile_col(m) + lf_a_row(l)) + kw);
}
SGR_HD int ec_fwd_b_addr(int l, int s, int n) { return ec_fwd_w_idx(4 * s + lf_b_k(l), 16 * n + lf_b_col(l)); }

// ---- BACKWARD, DATA: per parity class of the source pixel, M = source pixels, N = C, K = 4 O -------------------------------------------------
// Source pixel (h, w) = (2 a + ph, 2 b + pw) of class (ph, pw) is read, under the zeros rule, by the four members (p, q) in {0, 1}^2:
// output (a + ph - p, b + pw - q) through tap (kh, kw) = (1 - ph + 2 p, 1 - pw + 2 q); an output outside the map is an exact zero.  That
// is ec_pairs without its replicate members.  A workgroup owns a 16 x 4 tile of the (a, b) grid of one image and a pass of up to 64
// channels; wave w owns ph = w & 1 and the tile rows 2 (w >> 1) and 2 (w >> 1) + 1, both pw: M tile (m, pw), row bb of the MFMA is
// b0 + bb; column j of N tile n is channel c0p + 16 n + j.  The outputs are walked in chunks of 4.  Inside a chunk the k index is
// oc * 4 + 2 p + q, 16 of them = 4 MFMA steps; step oc holds (p, q) = (l >> 5, (l >> 4) & 1).
// ORDER, one dx:  run = 0;  for every chunk in turn:  t = 0;  for oc, for p, for q:  t = fmaf(g[o, a+ph-p, b+pw-q], Wt[o, c, 1-ph+2p, 1-pw+2q], t);   run += t
// In replicate mode the pixels of the first and last row and column are then written again by ec_dx_border below (the vector ALU, a
// gather over ec_pairs), whose extra members have the other class's taps.
// The cotangent tile of a chunk is [oc][6 rows a0 - 1 .. a0 + 4][18 columns b0 - 1 .. b0 + 16]: the 64 lanes of a step read 35
// consecutive floats.  The weight tile is [oc][class][k][c] with pitch 80: the four k of a step start 16 banks apart.
constexpr int kEcDW = 16, kEcDH = 4;             // the workgroup's tile of the (a, b) grid
constexpr int kEcDOC = 4;                        // outputs per chunk
constexpr int kEcDPassC = 64, kEcDPassNT = 4;    // channels per workgroup
constexpr int kEcDGRows = kEcDH + 2, kEcDGCols = kEcDW + 2;
constexpr int kEcDGPlane = kEcDGRows * kEcDGCols;      // 108
constexpr int kEcDCP = 80;
SGR_HD int ec_dx_kh(int ph, int k) { return 1 - ph + 2 * (k >> 1); }
SGR_HD int ec_dx_kw(int pw, int k) { return 1 - pw + 2 * (k & 1); }
SGR_HD int ec_dx_g_idx(int oc, int r, int col) { return oc * kEcDGPlane + r * kEcDGCols + col; }
SGR_HD int ec_dx_w_idx(int oc, int cls, int k, int c) { return ((oc * 4 + cls) * 4 + k) * kEcDCP + c; }
// where tap (kh, kw) of the weight tile goes: class (1 - (kh & 1), 1 - (kw & 1)), k = 2 (kh >> 1) + (kw >> 1)
SGR_HD int ec_dx_w_idx_of_tap(int oc, int kh, int kw, int c) {
  return ec_dx_w_idx(oc, 2 * (1 - (kh & 1)) + 1 - (kw & 1), 2 * (kh >> 1) + (kw >> 1), c);
}
SGR_HD int ec_dx_a_addr(int l, int oc, int ph, int pw, int m) {
  const int k = lf_a_k(l);
  return ec_dx_g_idx(oc, m + ph - (k >> 1) + 1, lf_a_row(l) + pw - (k & 1) + 1);
}
SGR_HD int ec_dx_b_addr(int l, int oc, int ph, int pw, int n) { return ec_dx_w_idx(oc, 2 * ph + pw, lf_b_k(l), 16 * n + lf_b_col(l)); }
// one border pixel in replicate mode, from global memory: g is image b's cotangent [O][Ho][Wo], Wt [O][C][4][4]
// ORDER, as the matrix path's:  d = 0;  for every chunk of 4 outputs in turn:  t = 0;  for o, for the row members in slot order, for the
//         column members in slot order:  t = fmaf(Wt[o, c, kh, kw], g[o, i, j], t);   d += t
SGR_HD float ec_dx_border(const float* g, const float* Wt, int c, int h, int w, int C, int O, int H, int W) {
  const EcPairs rows = ec_pairs(h, H, kEcReplicate), cols = ec_pairs(w, W, kEcReplicate);
  const int Ho = ec_out(H), Wo = ec_out(W);
  // the four (row member, column member) combinations: where they read, and whether they exist.  One that does not reads element 0 and
  // enters as fmaf(0, 0, t) = t, so that the loads of a chunk do not wait for each other
  int wo[4], go[4];
  bool ok[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int p = m >> 1, q = m & 1;
    ok[m] = rows.i[p] >= 0 && cols.i[q] >= 0;
    wo[m] = ok[m] ? (c * 4 + rows.k[p]) * 4 + cols.k[q] : 0;
    go[m] = ok[m] ? rows.i[p] * Wo + cols.i[q] : 0;
  }
  const long long wstep = (long long)C * 16, gstep = (long long)Ho * Wo;
  float d = 0.0f;
  for (int og = 0; og < O; og += kEcDOC) {
    float a[kEcDOC][4], b[kEcDOC][4];
#pragma unroll
    for (int oc = 0; oc < kEcDOC; ++oc)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        a[oc][m] = Wt[(og + oc) * wstep + wo[m]];
        b[oc][m] = g[(og + oc) * gstep + go[m]];
      }
    float t = 0.0f;
#pragma unroll
    for (int oc = 0; oc < kEcDOC; ++oc)
#pragma unroll
      for (int m = 0; m < 4; ++m) t = fmaf(ok[m] ? a[oc][m] : 0.0f, ok[m] ? b[oc][m] : 0.0f, t);
    d += t;
  }
  return d;
}

// ---- BACKWARD, WEIGHTS: M = 16 C, N = O, K = output pixels -----------------------------------------------------------------------------------
// A workgroup owns one image, a block of 16 channels, a pass of up to 64 outputs and a strip of 25 consecutive 16 x 4 tiles of output
// pixels (in the raster order of the tiles).  An accumulator tile is (channel cc, N tile n): row of the MFMA = tap 4 kh + kw, column j =
// output o0 + 16 n + j; the channels cc = wave, wave + 4, .. belong to wave `wave`.  The A operand is x[c, src(2i+kh-1), src(2j+kw-1)]
// from the input tile with its halo, the B operand g[o, i, j] from the cotangent tile, which holds exact zeros outside the map.  Inside a
// pixel tile the k index is the pixel p = 16 row + column, 64 = 16 MFMA steps; step s holds p = 4 s + (l >> 4).
// ORDER, one dWt:  run = 0;  for every tile of the strip:  t = 0;  for p = 0 .. 63:  t = fmaf(x.., g[o, p], t);   run += t
//                  then the strips' fp32 partials are added in double in index order (b, then strip)
// The input tile of a channel is 10 rows of 48 floats: the even tile columns at 0 .. 16, the odd ones at 24 .. 40.  The 64 lanes of a
// step read, for each (kh, kw & 1), 5 consecutive floats starting at 48 kh + 24 (kw & 1) = 0, 8, .., 56 (mod 64): 40 banks, none
// twice.  The cotangent tile is [o][64 + 4]: output o starts 4 banks after o - 1 and a step's 4 pixels are consecutive.
constexpr int kEcWW = 16, kEcWH = 4;             // the pixel tile
constexpr int kEcWCB = 16;                       // channels per workgroup
constexpr int kEcWRows = 2 * kEcWH + 2;          // 10
constexpr int kEcWCols = 2 * kEcWW + 2;          // 34
constexpr int kEcWRP = 48, kEcWEP = 24;
constexpr int kEcWCHP = kEcWRows * kEcWRP;       // 480
constexpr int kEcWGP = 68;
constexpr int kEcWStrip = 25;                    // pixel tiles per workgroup
SGR_HD int ec_w_x_idx(int cc, int r, int tc) { return cc * kEcWCHP + r * kEcWRP + (tc & 1) * kEcWEP + (tc >> 1); }
SGR_HD int ec_w_g_idx(int o, int p) { return o * kEcWGP + p; }
SGR_HD int ec_w_a_addr(int l, int s, int cc) {
  const int tap = lf_a_row(l), kh = tap >> 2, kw = tap & 3, p = 4 * s + lf_a_k(l);
  return ec_w_x_idx(cc, 2 * (p >> 4) + kh, 2 * (p & 15) + kw);
}
SGR_HD int ec_w_b_addr(int l, int s, int n) { return ec_w_g_idx(16 * n + lf_b_col(l), 4 * s + lf_b_k(l)); }

// ---- BACKWARD, BIAS: on the vector ALU, sgr_final_conv.hip's scheme ------------------------------------------------------------------------
// A thread adds the cotangents of its share of a slice (8 runs of 4 consecutive pixels of the flat plane, run (8 s + r) 256 + thread) in
// order in fp32, the threads of a workgroup are added by block_sum and the workgroups' partials in double in index order (b, then slice).
constexpr int kEcBRounds = 8;
constexpr int kEcBSlice = 256 * kEcBRounds * 4;      // pixels per workgroup

}  // namespace sgr
