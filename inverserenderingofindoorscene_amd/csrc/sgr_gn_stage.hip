// The repeated stage of the reference's four network classes (models.py:87-346) around its convolution, on gfx950:
//   plain   y  [B,C,H,W]        = relu(group_norm(x, G, weight, bias, eps))                                  (encoder0 / encoderLight, :122-127)
//   upcat   up [B,C+Cs,2H,2W]   = interpolate(cat([y, skip], 1), scale_factor=2, mode='bilinear')            (decoder0 / decoderLight, :160-183)
//   resize  the same two with relu(group_norm(x)) resized to [Hs, Ws] first, H <= Hs <= 2H, W <= Ws <= 2W: the decoders' stage against a
//           skip of another size and the final stage's resize to the image (:165-166 and its siblings, :185-186, :312-333); second half
//           of this file, entry points sgr_gn_resize_*
//   siblings  the upcat and resize forms for D <= 8 decoders that share their shapes and their skip, in the launches of one (the reference
//           runs four decoder0 and three decoderLight instances on the same features): end of this file, entry points
//           sgr_gn_stage_siblings_* / sgr_gn_resize_siblings_*, DESIGN.md section 8k
// DESIGN.md section 8e states the contract; the per-element arithmetic is sgr_gn_stage.h.
//
// Forward, two launches: the moments of every (b, g) as double-precision (sum, sum of squares) partials, one per slice of the group, then
// the apply kernel, which folds the partials of its group in a fixed order (every workgroup the same bits), writes the saved statistics
// and streams the result: a thread produces two output rows of four columns from a 3 x 4 source neighbourhood, the skip channels through
// the same code with the normalisation switched off.
// Backward, three launches: pass 1 gathers the upsample's adjoint (4 x 4 output pixels per source pixel, no atomics), masks it with
// y > 0 (y recomputed from x and the saved statistics), stores it (`dy`, C H W floats per image) and leaves double-precision partial sums
// of dy and dy xhat per (b, c) slice; the skip channels leave pass 1 as dskip.  The fold makes the two per-(b, g) sums, dweight and
// dbias, each by one wave in a fixed order.  Pass 2 writes dx.  Without a skip there is no adjoint and no `dy`: pass 2 masks the cotangent.
//
// x and skip are read through their strides (channels-last convolution outputs); every sum runs over logical indices, so the layout
// changes no bit.  128-bit loads and stores where the layout and the alignment allow them, the same arithmetic element by element elsewhere.
// The wave ladder of the sums (wave_sum), the 128-bit vector (Vec<4>) and its alignment test (aligned16) are sgr_reduce.h's.
//
// The kernels of the same-size forms are templates on the I/O type T of x, skip, the result, the cotangent, dx and dskip: float, or bf16
// (sgr_gn_stage_fwd_bf16 / _bwd_bf16).  Loads convert to fp32 (gn_in), stores round once (gn_out); the arithmetic, the
// mapping of logical elements to threads and the order of every sum are the same, so a bf16 result is the fp32 result on the upcast input,
// rounded once.  A run of four bf16 values is one 64-bit access (Vec4h / aligned8).  The resize forms are fp32 only.
#include "sgr_gn_stage.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"       // wave_sum, Vec<4>, aligned16

namespace sgr {

constexpr int kGThreads = 256;
constexpr int kGRounds = 8;            // positions per thread in the apply and backward kernels
constexpr int kGSliceMin = 32768;      // elements of a group per moments workgroup, at least
constexpr int kGSliceMax = 64;         // moments workgroups per (b, g), at most: one wave folds them

struct GnStrides { long long b, c, h, w; };

// A run of four consecutive elements of the I/O type T as one access, to and from fp32: 128 bits of an fp32 tensor (Vec<4>), 64 bits of a
// bf16 one (Vec4h).  The same four logical elements either way, so the sums below take them in the same order.
__device__ __forceinline__ void ld4(const float* __restrict__ p, float (&v)[4]) {
  const Vec<4> q = *reinterpret_cast<const Vec<4>*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = q.v[u];
}
__device__ __forceinline__ void ld4(const bf16* __restrict__ p, float (&v)[4]) {
  const Vec4h q = *reinterpret_cast<const Vec4h*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = bf16_up(q.v[u]);
}
__device__ __forceinline__ void st4(float* __restrict__ p, const float (&v)[4]) {
  Vec<4> q;
#pragma unroll
  for (int u = 0; u < 4; ++u) q.v[u] = v[u];
  *reinterpret_cast<Vec<4>*>(p) = q;
}
__device__ __forceinline__ void st4(bf16* __restrict__ p, const float (&v)[4]) {
  Vec4h q;
#pragma unroll
  for (int u = 0; u < 4; ++u) q.v[u] = bf16_round(v[u]);
  *reinterpret_cast<Vec4h*>(p) = q;
}
// host side: every pointer on the boundary a run of four T needs
template <typename T>
static bool aligned_run(std::initializer_list<const void*> ptrs) { return sizeof(T) == 4 ? aligned16(ptrs) : aligned8(ptrs); }

// the block's sums in thread 0: wave_sum per wave, then the waves added in order (their number comes from blockDim: 64 or 256 threads)
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { lds[2 * wave] = a; lds[2 * wave + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = lds[0]; b = lds[1];
    for (int k = 1; k < nw; ++k) { a += lds[2 * k]; b += lds[2 * k + 1]; }
  }
}

// slices of a group of n elements: a function of n alone, so that an image's sums do not depend on its batch
static int gn_slices(long long n) {
  long long s = (n + kGSliceMin - 1) / kGSliceMin;
  return (int)(s < 1 ? 1 : s > kGSliceMax ? kGSliceMax : s);
}
static long long gn_slice_len(long long n) {
  const long long per = (n + gn_slices(n) - 1) / gn_slices(n);
  return (per + 4 * kGThreads - 1) / (4 * kGThreads) * (4 * kGThreads);
}

// partials[(b G + g) S + s] = (sum, sum of squares) over the logical elements [s L, (s+1) L) of the group; thread t takes the runs of four
// at s L + 4 (k T + t), k = 0, 1, ..
// The kernels below are bodies (`*_body`: the work of one workgroup, its channel or group and its image given by the caller) and the
// `__global__` functions that place them on a grid: one per operator here, one per set of sibling operators at the end of the file.
template <bool VEC, typename T>
__device__ __forceinline__ void gn_moments_body(const T* __restrict__ x, GnStrides xs, double* __restrict__ partials, int cpg, int W, int HW, long long L,
                                                int g, int b, int G) {
  __shared__ double lds[2 * kGThreads / 64];
  const int s = blockIdx.x, S = gridDim.x;
  const long long n = (long long)cpg * HW;
  const long long e0 = (long long)s * L, e1 = e0 + L < n ? e0 + L : n;
  const T* xb = x + (long long)b * xs.b + (long long)g * cpg * xs.c;
  double sum = 0.0, sq = 0.0;
  for (long long e = e0 + 4ll * threadIdx.x; e < e1; e += 4ll * blockDim.x) {
    int c = (int)(e / HW), p = (int)(e - (long long)c * HW);
    float v[4];
    if (VEC) {
      ld4(xb + (long long)c * xs.c + p, v);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = 0.0f;
        if (e + u < e1) {
          const int h = p / W, w = p - h * W;
          v[u] = gn_in(xb[(long long)c * xs.c + (long long)h * xs.h + (long long)w * xs.w]);
        }
        if (++p == HW) { p = 0; ++c; }
      }
    }
    // a run past the end adds exact zeros: the bits do not depend on the path
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double d = (double)v[u];
      sum += d;
      sq = fma(d, d, sq);
    }
  }
  block_sum2(sum, sq, lds);
  if (threadIdx.x == 0) {
    double* o = partials + 2 * (((long long)b * G + g) * S + s);
    o[0] = sum;
    o[1] = sq;
  }
}
template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_moments_kernel(const T* __restrict__ x, GnStrides xs, double* __restrict__ partials, int cpg, int W,
                                                               int HW, long long L) {
  gn_moments_body<VEC>(x, xs, partials, cpg, W, HW, L, blockIdx.y, blockIdx.z, gridDim.y);
}

// the statistics of group (b, g) from its S <= 64 partials, by the first wave: lane s holds slice s, the lanes are added by wave_sum's tree
__device__ __forceinline__ void gn_group_stat(const double* __restrict__ partials, int bg, int S, double n, float eps, float* sh) {
  if (threadIdx.x < 64) {
    double a = 0.0, q = 0.0;
    if ((int)threadIdx.x < S) {
      a = partials[2 * ((long long)bg * S + threadIdx.x)];
      q = partials[2 * ((long long)bg * S + threadIdx.x) + 1];
    }
    a = wave_sum(a);
    q = wave_sum(q);
    if (threadIdx.x == 0) gn_finish(a, q, n, eps, sh[0], sh[1], sh[2], sh[3]);
  }
  __syncthreads();
}

// the statistics alone (sgr_gn_moments): one wave per (b, g) does the fold the apply kernels do and writes what they write
__global__ __launch_bounds__(64) void gn_stats_kernel(const double* __restrict__ partials, float* __restrict__ stats, int S, double n, float eps) {
  __shared__ float sh[4];
  gn_group_stat(partials, blockIdx.x, S, n, eps, sh);
  if (threadIdx.x == 0) {
    float* st = stats + 4 * (long long)blockIdx.x;
    st[0] = sh[0]; st[1] = sh[1]; st[2] = sh[2]; st[3] = sh[3];
  }
}

// plain form: y = relu(gn(x)); a thread takes runs of four plane elements
template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_apply_plain_kernel(const T* __restrict__ x, GnStrides xs, const float* __restrict__ weight,
                                                                   const float* __restrict__ bias, const double* __restrict__ partials,
                                                                   float* __restrict__ stats, T* __restrict__ y, int C, int cpg, int W, int HW,
                                                                   int S, float eps) {
  __shared__ float sh[4];
  const int c = blockIdx.y, b = blockIdx.z, G = C / cpg, g = c / cpg;
  gn_group_stat(partials, b * G + g, S, (double)cpg * HW, eps, sh);
  const float mh = sh[0], ml = sh[1], rstd = sh[2];
  if (blockIdx.x == 0 && c == g * cpg && threadIdx.x == 0) {
    float* st = stats + 4 * ((long long)b * G + g);
    st[0] = mh; st[1] = ml; st[2] = rstd; st[3] = sh[3];
  }
  const float wc = weight[c], bc = bias[c];
  const T* xp = x + (long long)b * xs.b + (long long)c * xs.c;
  T* yp = y + ((long long)b * C + c) * HW;
#pragma unroll 1
  for (int r = 0; r < kGRounds; ++r) {
    const int p = 4 * ((blockIdx.x * kGRounds + r) * kGThreads + threadIdx.x);
    if (p >= HW) break;
    float q[4];
    if (VEC) {
      ld4(xp + p, q);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pu = p + u < HW ? p + u : HW - 1, h = pu / W, w = pu - h * W;
        q[u] = gn_in(xp[(long long)h * xs.h + (long long)w * xs.w]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = fmaxf(gn_pre(gn_xhat(q[u], mh, ml, rstd), wc, bc), 0.0f);
    if (VEC) {
      st4(yp + p, q);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + u < HW) yp[p + u] = gn_out<T>(q[u]);
    }
  }
}

// upcat form: channel ch < C is normalised x, ch >= C is skip as it is.  A thread at (i, jj) reads source rows i-1 .. i+1 x columns
// 2jj-1 .. 2jj+2 (clamped) and writes output rows 2i, 2i+1 x columns 4jj .. 4jj+3.  VEC: one store per run of four (W even, a result aligned for st4).
// two output rows of four columns at o0 (row length OW; jj: the thread's column position)
template <bool VEC, typename T>
__device__ __forceinline__ void up_store(T* __restrict__ o0, int jj, int OW, const float (&top)[4], const float (&bot)[4]) {
  if (VEC) {
    st4(o0, top);
    st4(o0 + OW, bot);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * jj + k < OW) { o0[k] = gn_out<T>(top[k]); o0[OW + k] = gn_out<T>(bot[k]); }
  }
}

// store(o, jj, top, bot): writes the two rows at element o of the result -- of one result here, of every sibling's for a skip channel of
// the sibling form
template <bool VEC, typename T, typename Store>
__device__ __forceinline__ void gn_apply_up_body(const T* __restrict__ x, GnStrides xs, const T* __restrict__ skip, GnStrides ss,
                                                 const float* __restrict__ weight, const float* __restrict__ bias, const double* __restrict__ partials,
                                                 float* __restrict__ stats, Store store, int C, int Cs, int cpg, int H, int W, int S, float eps, int ch,
                                                 int b) {
  __shared__ float sh[4];
  const bool norm = ch < C;      // uniform in the workgroup
  float mh = 0.0f, ml = 0.0f, rstd = 1.0f, wc = 1.0f, bc = 0.0f;
  const T* src;
  GnStrides st;
  if (norm) {
    const int G = C / cpg, g = ch / cpg;
    gn_group_stat(partials, b * G + g, S, (double)cpg * H * W, eps, sh);
    mh = sh[0]; ml = sh[1]; rstd = sh[2];
    if (blockIdx.x == 0 && ch == g * cpg && threadIdx.x == 0) {
      float* o = stats + 4 * ((long long)b * G + g);
      o[0] = mh; o[1] = ml; o[2] = rstd; o[3] = sh[3];
    }
    wc = weight[ch]; bc = bias[ch];
    src = x + (long long)b * xs.b + (long long)ch * xs.c;
    st = xs;
  } else {
    src = skip + (long long)b * ss.b + (long long)(ch - C) * ss.c;
    st = ss;
  }
  const int W2 = (W + 1) >> 1, OW = 2 * W;
  const long long op = ((long long)b * (C + Cs) + ch) * 4ll * H * W;
  const unsigned sth = (unsigned)st.h, stw = (unsigned)st.w;      // in-plane offsets fit 31 bits (checked on the host)
  const UpTaps taps = up_taps();
  // the position (i, jj) of round 0 by one division, of the later rounds by steps of 256
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W2, dj = kGThreads - di * W2;
  int i = q0 / W2, jj = q0 - i * W2;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < H; ++r) {
    const int c0 = 2 * jj;
    const unsigned ro[3] = {(unsigned)(i > 0 ? i - 1 : 0) * sth, (unsigned)i * sth, (unsigned)(i + 1 < H ? i + 1 : H - 1) * sth};
    const unsigned co[4] = {(unsigned)(c0 > 0 ? c0 - 1 : 0) * stw, (unsigned)c0 * stw, (unsigned)(c0 + 1 < W ? c0 + 1 : W - 1) * stw,
                            (unsigned)(c0 + 2 < W ? c0 + 2 : W - 1) * stw};
    float v[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float t = gn_in(src[ro[a] + co[k]]);
        v[a][k] = norm ? fmaxf(gn_pre(gn_xhat(t, mh, ml, rstd), wc, bc), 0.0f) : t;
      }
    const UpTap tc[4] = {up_pick(taps, 4 * jj), taps.odd, taps.even, taps.odd};
    float top[4], bot[4];
    up_quad(v, tc, up_pick(taps, 2 * i), taps.odd, top, bot);
    store(op + (long long)(2 * i) * OW + 4 * jj, jj, top, bot);
    i += di;
    jj += dj;
    if (jj >= W2) { jj -= W2; ++i; }
  }
}
template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_apply_up_kernel(const T* __restrict__ x, GnStrides xs, const T* __restrict__ skip, GnStrides ss,
                                                                const float* __restrict__ weight, const float* __restrict__ bias,
                                                                const double* __restrict__ partials, float* __restrict__ stats,
                                                                T* __restrict__ out, int C, int Cs, int cpg, int H, int W, int S, float eps) {
  const int OW = 2 * W;
  gn_apply_up_body<VEC>(x, xs, skip, ss, weight, bias, partials, stats,
                        [&](long long o, int jj, const float (&top)[4], const float (&bot)[4]) { up_store<VEC>(out + o, jj, OW, top, bot); }, C, Cs, cpg, H, W,
                        S, eps, blockIdx.y, blockIdx.z);
}

// The upsample's adjoint at the source pixels (i, 2jj) and (i, 2jj+1) of an H x W plane: gp is the cotangent's plane [2H, 2W], the six weight
// sets are up_adj_sets' of either axis.  VEC: the four inner columns of a row as one load (W even, a cotangent aligned for runs of four).
template <bool VEC, typename T>
__device__ __forceinline__ void up_gather(const T* __restrict__ gp, int i, int jj, int H, int W, const float (&rl)[4], const float (&rm)[4],
                                          const float (&rh)[4], const float (&cl)[4], const float (&cm)[4], const float (&chi)[4], float& a0,
                                          float& a1) {
  const int c0 = 2 * jj, OW = 2 * W, OH = 2 * H;
  const bool two = c0 + 1 < W;
  float gv[4][6];
  float wr[4], wa[4], wb[4];
  up_adj_pick(rl, rm, rh, i, H, wr);
  up_adj_pick(cl, cm, chi, c0, W, wa);
  up_adj_pick(cl, cm, chi, c0 + 1, W, wb);
#pragma unroll
  for (int k = 0; k < 4; ++k) wb[k] = two ? wb[k] : 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int orow = 2 * i - 1 + k;
    const bool in = orow >= 0 && orow < OH;
    const T* row = gp + (long long)(in ? orow : 0) * OW;
    const int o = 4 * jj;
    gv[k][0] = in && o > 0 ? gn_in(row[o - 1]) : 0.0f;
    if (VEC) {
      float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (in) ld4(row + o, t);
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[k][1 + u] = t[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[k][1 + u] = in && o + u < OW ? gn_in(row[o + u]) : 0.0f;
    }
    gv[k][5] = in && o + 4 < OW ? gn_in(row[o + 4]) : 0.0f;
  }
  up_adjoint(gv, wr, wa, wb, a0, a1);
}

// Backward pass 1 over the channels [c_begin, c_begin + gridDim.y) of cat([y, skip]).  UP: g is [B,C+Cs,2H,2W] and the adjoint is gathered;
// otherwise g is [B,C,H,W] and taken as it is.  ch < C: dy = (y > 0) adjoint, stored to `dy` (if given) and summed; ch >= C: dskip = adjoint.
// The cotangent, x and dskip have the I/O type T; `dy` is workspace and stays fp32 (the unrounded masked adjoint, as in the fp32 operator).
// adjoint(i, jj, a0, a1): the cotangent's adjoint at the source pixels (i, 2jj) and (i, 2jj+1) of channel ch of image b -- of one cotangent
// here, the ordered sum over the siblings' for a skip channel of the sibling form
template <typename T, typename Adjoint>
__device__ __forceinline__ void gn_bwd_pass1_body(Adjoint adjoint, const T* __restrict__ x, GnStrides xs, const float* __restrict__ weight,
                                                  const float* __restrict__ bias, const float* __restrict__ stats, float* __restrict__ dy,
                                                  T* __restrict__ dskip, double* __restrict__ partials, int C, int Cs, int cpg, int H, int W, int ch, int b) {
  __shared__ double lds[2 * kGThreads / 64];
  const int P = gridDim.x;
  const bool norm = ch < C;
  float mh = 0.0f, ml = 0.0f, rstd = 1.0f, wc = 1.0f, bc = 0.0f;
  const T* xp = nullptr;
  if (norm) {
    const float* st = stats + 4 * ((long long)b * (C / cpg) + ch / cpg);
    mh = st[0]; ml = st[1]; rstd = st[2];
    wc = weight[ch]; bc = bias[ch];
    xp = x + (long long)b * xs.b + (long long)ch * xs.c;
  }
  const int W2 = (W + 1) >> 1;
  float* dyp = norm && dy ? dy + ((long long)b * C + ch) * H * W : nullptr;
  T* dsp = norm ? nullptr : dskip + ((long long)b * Cs + (ch - C)) * H * W;
  double s1 = 0.0, s2 = 0.0;
  const unsigned sh = (unsigned)xs.h, sw = (unsigned)xs.w;      // in-plane offsets fit 31 bits (checked on the host)
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W2, dj = kGThreads - di * W2;
  int i = q0 / W2, jj = q0 - i * W2;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < H; ++r) {
    const int c0 = 2 * jj;
    const bool two = c0 + 1 < W;
    float a0, a1;
    adjoint(i, jj, a0, a1);
    if (norm) {
      const float x0 = gn_in(xp[(unsigned)i * sh + (unsigned)c0 * sw]);
      const float x1 = two ? gn_in(xp[(unsigned)i * sh + (unsigned)(c0 + 1) * sw]) : 0.0f;
      const float h0 = gn_xhat(x0, mh, ml, rstd), h1 = gn_xhat(x1, mh, ml, rstd);
      a0 = gn_pre(h0, wc, bc) > 0.0f ? a0 : 0.0f;
      a1 = two && gn_pre(h1, wc, bc) > 0.0f ? a1 : 0.0f;
      s1 += (double)a0;
      s1 += (double)a1;
      s2 = fma((double)a0, (double)h0, s2);
      s2 = fma((double)a1, (double)h1, s2);
    }
    if (dyp) {
      dyp[(long long)i * W + c0] = a0;
      if (two) dyp[(long long)i * W + c0 + 1] = a1;
    } else if (dsp) {
      dsp[(long long)i * W + c0] = gn_out<T>(a0);
      if (two) dsp[(long long)i * W + c0 + 1] = gn_out<T>(a1);
    }
    i += di;
    jj += dj;
    if (jj >= W2) { jj -= W2; ++i; }
  }
  if (norm) {      // uniform in the workgroup
    block_sum2(s1, s2, lds);
    if (threadIdx.x == 0) {
      double* o = partials + 2 * (((long long)b * C + ch) * P + blockIdx.x);
      o[0] = s1;
      o[1] = s2;
    }
  }
}
template <bool VEC, bool UP, typename T>
__global__ __launch_bounds__(kGThreads) void gn_bwd_pass1_kernel(const T* __restrict__ g, const T* __restrict__ x, GnStrides xs,
                                                                 const float* __restrict__ weight, const float* __restrict__ bias,
                                                                 const float* __restrict__ stats, float* __restrict__ dy, T* __restrict__ dskip,
                                                                 double* __restrict__ partials, int C, int Cs, int cpg, int H, int W, int c_begin) {
  const int ch = c_begin + blockIdx.y, b = blockIdx.z;
  const int OW = UP ? 2 * W : W, OH = UP ? 2 * H : H;
  const T* gp = g + ((long long)b * (C + Cs) + ch) * (long long)OH * OW;
  float rl[4], rm[4], rh[4], cl[4], cm[4], chi[4];      // the adjoint weights at the low edge, inside and at the high edge of either axis
  if (UP) { up_adj_sets(H, rl, rm, rh); up_adj_sets(W, cl, cm, chi); }
  gn_bwd_pass1_body(
      [&](int i, int jj, float& a0, float& a1) {
        if (UP) {
          up_gather<VEC>(gp, i, jj, H, W, rl, rm, rh, cl, cm, chi, a0, a1);
        } else {
          a0 = gn_in(gp[(long long)i * W + 2 * jj]);
          a1 = 2 * jj + 1 < W ? gn_in(gp[(long long)i * W + 2 * jj + 1]) : 0.0f;
        }
      },
      x, xs, weight, bias, stats, dy, dskip, partials, C, Cs, cpg, H, W, ch, b);
}

// One wave per job.  Jobs [0, B G): (c1, c2) of group (b, g) = sum over its channels and slices of w_c (s1, s2), over n.  Jobs
// [B G, B G + C): dweight_c = sum over b and slices of s2, dbias_c of s1.  Lane l takes the entries l, l + 64, .. in order.
__device__ __forceinline__ void gn_bwd_fold_body(const double* __restrict__ partials, const float* __restrict__ weight, float* __restrict__ coef,
                                                 float* __restrict__ dweight, float* __restrict__ dbias, int B, int C, int cpg, int P, double n) {
  const int G = C / cpg, job = blockIdx.x, lane = threadIdx.x;
  double a = 0.0, q = 0.0;
  if (job < B * G) {
    const int b = job / G, g = job - b * G;
    const double* base = partials + 2 * ((long long)b * C + (long long)g * cpg) * P;
    for (int k = lane; k < cpg * P; k += 64) {
      const double w = (double)weight[g * cpg + k / P];
      a = fma(w, base[2 * k], a);
      q = fma(w, base[2 * k + 1], q);
    }
    a = wave_sum(a);
    q = wave_sum(q);
    if (lane == 0 && coef) {
      coef[2 * job] = (float)(a / n);
      coef[2 * job + 1] = (float)(q / n);
    }
  } else {
    const int c = job - B * G;
    for (int k = lane; k < B * P; k += 64) {
      const int b = k / P, s = k - b * P;
      const double* e = partials + 2 * (((long long)b * C + c) * P + s);
      a += e[0];
      q += e[1];
    }
    a = wave_sum(a);
    q = wave_sum(q);
    if (lane == 0) {
      if (dbias) dbias[c] = (float)a;
      if (dweight) dweight[c] = (float)q;
    }
  }
}
__global__ __launch_bounds__(64) void gn_bwd_fold_kernel(const double* __restrict__ partials, const float* __restrict__ weight, float* __restrict__ coef,
                                                         float* __restrict__ dweight, float* __restrict__ dbias, int B, int C, int cpg, int P,
                                                         double n) {
  gn_bwd_fold_body(partials, weight, coef, dweight, dbias, B, C, cpg, P, n);
}

// dx from dy (MASK = false: pass 1's masked adjoint) or from the cotangent itself (MASK = true: the plain form, masked here)
// x and dx have the I/O type T; dy has TD: float for pass 1's workspace, T for the cotangent
template <bool VEC, bool MASK, typename T, typename TD>
__device__ __forceinline__ void gn_bwd_pass2_body(const TD* __restrict__ dy, const T* __restrict__ x, GnStrides xs, const float* __restrict__ weight,
                                                  const float* __restrict__ bias, const float* __restrict__ stats, const float* __restrict__ coef,
                                                  T* __restrict__ dx, int C, int cpg, int W, int HW, int c, int b) {
  const int G = C / cpg, g = c / cpg;
  const float* st = stats + 4 * ((long long)b * G + g);
  const float mh = st[0], ml = st[1], rstd = st[2], wc = weight[c], bc = bias[c];
  const float c1 = coef[2 * (b * G + g)], c2 = coef[2 * (b * G + g) + 1];
  const T* xp = x + (long long)b * xs.b + (long long)c * xs.c;
  const TD* dp = dy + ((long long)b * C + c) * HW;
  T* op = dx + ((long long)b * C + c) * HW;
#pragma unroll 1
  for (int r = 0; r < kGRounds; ++r) {
    const int p = 4 * ((blockIdx.x * kGRounds + r) * kGThreads + threadIdx.x);
    if (p >= HW) break;
    float xv[4], dv[4];
    if (VEC) {
      ld4(xp + p, xv);
      ld4(dp + p, dv);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pu = p + u < HW ? p + u : HW - 1, h = pu / W, w = pu - h * W;
        xv[u] = gn_in(xp[(long long)h * xs.h + (long long)w * xs.w]);
        dv[u] = gn_in(dp[pu]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float xh = gn_xhat(xv[u], mh, ml, rstd);
      const float d = !MASK || gn_pre(xh, wc, bc) > 0.0f ? dv[u] : 0.0f;
      dv[u] = gn_dx(d, xh, wc, rstd, c1, c2);
    }
    if (VEC) {
      st4(op + p, dv);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + u < HW) op[p + u] = gn_out<T>(dv[u]);
    }
  }
}
template <bool VEC, bool MASK, typename T, typename TD>
__global__ __launch_bounds__(kGThreads) void gn_bwd_pass2_kernel(const TD* __restrict__ dy, const T* __restrict__ x, GnStrides xs,
                                                                 const float* __restrict__ weight, const float* __restrict__ bias,
                                                                 const float* __restrict__ stats, const float* __restrict__ coef,
                                                                 T* __restrict__ dx, int C, int cpg, int W, int HW) {
  gn_bwd_pass2_body<VEC, MASK>(dy, x, xs, weight, bias, stats, coef, dx, C, cpg, W, HW, blockIdx.y, blockIdx.z);
}

// ---- the resize-to-skip forms (models.py:165-166 and its siblings; 185-186): y is resized from H x W to the skip's Hs x Ws before the
// concatenation, H <= Hs <= 2H and W <= Ws <= 2W.  The arithmetic is the rs_* part of sgr_gn_stage.h; sch / scw are the fp32 scales
// (float)H / (float)Hs and (float)W / (float)Ws, formed on the host.  SAMEW (W == Ws, the usual case: only the floor-halved height is off):
// the scale is exactly 1, a column's second tap has the weight 0 and is not loaded -- the same bits.

// relu(gn(.)) of the x plane at the taps (tr) x (tc): the resized value
template <bool SAMEW>
__device__ __forceinline__ float rs_gn_value(const float* __restrict__ src, unsigned sth, unsigned stw, const RsTap& tr, const RsTap& tc, float mh, float ml,
                                             float rstd, float wc, float bc) {
  auto y = [&](int r, int c) { return fmaxf(gn_pre(gn_xhat(src[(unsigned)r * sth + (unsigned)c * stw], mh, ml, rstd), wc, bc), 0.0f); };
  const float p00 = y(tr.i0, tc.i0), p10 = y(tr.i1, tc.i0);
  const float p01 = SAMEW ? p00 : y(tr.i0, tc.i1), p11 = SAMEW ? p10 : y(tr.i1, tc.i1);
  return rs_value(p00, p01, p10, p11, tr, tc);
}

// resize + upcat: gn_apply_up_kernel at the skip's resolution, the 3 x 4 neighbourhood of a normalised channel formed from x on the fly
// (store: as gn_apply_up_body's)
template <bool SAMEW, typename Store>
__device__ __forceinline__ void gn_apply_rsup_body(const float* __restrict__ x, GnStrides xs, const float* __restrict__ skip, GnStrides ss,
                                                   const float* __restrict__ weight, const float* __restrict__ bias, const double* __restrict__ partials,
                                                   float* __restrict__ stats, Store store, int C, int Cs, int cpg, int H, int W, int Hs, int Ws, float sch,
                                                   float scw, int S, float eps, int ch, int b) {
  __shared__ float sh[4];
  const bool norm = ch < C;      // uniform in the workgroup
  float mh = 0.0f, ml = 0.0f, rstd = 1.0f, wc = 1.0f, bc = 0.0f;
  const float* src;
  GnStrides st;
  if (norm) {
    const int G = C / cpg, g = ch / cpg;
    gn_group_stat(partials, b * G + g, S, (double)cpg * H * W, eps, sh);
    mh = sh[0]; ml = sh[1]; rstd = sh[2];
    if (blockIdx.x == 0 && ch == g * cpg && threadIdx.x == 0) {
      float* o = stats + 4 * ((long long)b * G + g);
      o[0] = mh; o[1] = ml; o[2] = rstd; o[3] = sh[3];
    }
    wc = weight[ch]; bc = bias[ch];
    src = x + (long long)b * xs.b + (long long)ch * xs.c;
    st = xs;
  } else {
    src = skip + (long long)b * ss.b + (long long)(ch - C) * ss.c;
    st = ss;
  }
  const int W2 = (Ws + 1) >> 1, OW = 2 * Ws;
  const long long op = ((long long)b * (C + Cs) + ch) * 4ll * Hs * Ws;
  const unsigned sth = (unsigned)st.h, stw = (unsigned)st.w;      // in-plane offsets fit 31 bits (checked on the host)
  const UpTaps taps = up_taps();
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W2, dj = kGThreads - di * W2;
  int i = q0 / W2, jj = q0 - i * W2;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < Hs; ++r) {
    const int c0 = 2 * jj;
    const int rr[3] = {i > 0 ? i - 1 : 0, i, i + 1 < Hs ? i + 1 : Hs - 1};
    const int cc[4] = {c0 > 0 ? c0 - 1 : 0, c0, c0 + 1 < Ws ? c0 + 1 : Ws - 1, c0 + 2 < Ws ? c0 + 2 : Ws - 1};
    float v[3][4];
    if (norm) {
      RsTap tcol[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) tcol[k] = rs_tap(cc[k], scw, W);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const RsTap trow = rs_tap(rr[a], sch, H);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[a][k] = rs_gn_value<SAMEW>(src, sth, stw, trow, tcol[k], mh, ml, rstd, wc, bc);
      }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[a][k] = src[(unsigned)rr[a] * sth + (unsigned)cc[k] * stw];
    }
    const UpTap tc[4] = {up_pick(taps, 4 * jj), taps.odd, taps.even, taps.odd};
    float top[4], bot[4];
    up_quad(v, tc, up_pick(taps, 2 * i), taps.odd, top, bot);
    store(op + (long long)(2 * i) * OW + 4 * jj, jj, top, bot);
    i += di;
    jj += dj;
    if (jj >= W2) { jj -= W2; ++i; }
  }
}
template <bool VEC, bool SAMEW>
__global__ __launch_bounds__(kGThreads) void gn_apply_rsup_kernel(const float* __restrict__ x, GnStrides xs, const float* __restrict__ skip, GnStrides ss,
                                                                  const float* __restrict__ weight, const float* __restrict__ bias,
                                                                  const double* __restrict__ partials, float* __restrict__ stats,
                                                                  float* __restrict__ out, int C, int Cs, int cpg, int H, int W, int Hs, int Ws,
                                                                  float sch, float scw, int S, float eps) {
  const int OW = 2 * Ws;
  gn_apply_rsup_body<SAMEW>(x, xs, skip, ss, weight, bias, partials, stats,
                            [&](long long o, int jj, const float (&top)[4], const float (&bot)[4]) { up_store<VEC>(out + o, jj, OW, top, bot); }, C, Cs, cpg,
                            H, W, Hs, Ws, sch, scw, S, eps, blockIdx.y, blockIdx.z);
}

// resize alone (the final stage): a thread makes the columns 4jq .. 4jq+3 of resized row i.  VEC: 128-bit stores (Ws % 4 == 0, aligned result).
template <bool VEC, bool SAMEW>
__global__ __launch_bounds__(kGThreads) void gn_apply_rs_kernel(const float* __restrict__ x, GnStrides xs, const float* __restrict__ weight,
                                                                const float* __restrict__ bias, const double* __restrict__ partials,
                                                                float* __restrict__ stats, float* __restrict__ out, int C, int cpg, int H, int W, int Hs,
                                                                int Ws, float sch, float scw, int S, float eps) {
  __shared__ float sh[4];
  const int c = blockIdx.y, b = blockIdx.z, G = C / cpg, g = c / cpg;
  gn_group_stat(partials, b * G + g, S, (double)cpg * H * W, eps, sh);
  const float mh = sh[0], ml = sh[1], rstd = sh[2];
  if (blockIdx.x == 0 && c == g * cpg && threadIdx.x == 0) {
    float* o = stats + 4 * ((long long)b * G + g);
    o[0] = mh; o[1] = ml; o[2] = rstd; o[3] = sh[3];
  }
  const float wc = weight[c], bc = bias[c];
  const float* src = x + (long long)b * xs.b + (long long)c * xs.c;
  float* op = out + ((long long)b * C + c) * (long long)Hs * Ws;
  const unsigned sth = (unsigned)xs.h, stw = (unsigned)xs.w;
  const int W4 = (Ws + 3) >> 2;
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W4, dj = kGThreads - di * W4;
  int i = q0 / W4, jq = q0 - i * W4;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < Hs; ++r) {
    const RsTap trow = rs_tap(i, sch, H);
    Vec<4> q;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * jq + k < Ws ? 4 * jq + k : Ws - 1;
      q.v[k] = rs_gn_value<SAMEW>(src, sth, stw, trow, rs_tap(col, scw, W), mh, ml, rstd, wc, bc);
    }
    float* o0 = op + (long long)i * Ws + 4 * jq;
    if (VEC) {
      *reinterpret_cast<Vec<4>*>(o0) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * jq + k < Ws) o0[k] = q.v[k];
    }
    i += di;
    jq += dj;
    if (jq >= W4) { jq -= W4; ++i; }
  }
}

// Backward, step 1 of the resize + upcat form: the upsample's adjoint at the skip's resolution, unmasked, over the channels
// [c_begin, c_begin + gridDim.y) of the concatenation.  ch < C goes to `da` [B,C,Hs,Ws] (workspace), ch >= C is dskip.
// (adjoint: as gn_bwd_pass1_body's)
template <typename Adjoint>
__device__ __forceinline__ void gn_up_adjoint_body(Adjoint adjoint, float* __restrict__ da, float* __restrict__ dskip, int C, int Cs, int Hs, int Ws, int ch,
                                                   int b) {
  const int W2 = (Ws + 1) >> 1;
  float* dst = ch < C ? da + ((long long)b * C + ch) * Hs * Ws : dskip + ((long long)b * Cs + (ch - C)) * Hs * Ws;
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W2, dj = kGThreads - di * W2;
  int i = q0 / W2, jj = q0 - i * W2;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < Hs; ++r) {
    float a0, a1;
    adjoint(i, jj, a0, a1);
    dst[(long long)i * Ws + 2 * jj] = a0;
    if (2 * jj + 1 < Ws) dst[(long long)i * Ws + 2 * jj + 1] = a1;
    i += di;
    jj += dj;
    if (jj >= W2) { jj -= W2; ++i; }
  }
}
template <bool VEC>
__global__ __launch_bounds__(kGThreads) void gn_up_adjoint_kernel(const float* __restrict__ g, float* __restrict__ da, float* __restrict__ dskip, int C,
                                                                  int Cs, int Hs, int Ws, int c_begin) {
  const int ch = c_begin + blockIdx.y, b = blockIdx.z;
  const float* gp = g + ((long long)b * (C + Cs) + ch) * 4ll * Hs * Ws;
  float rl[4], rm[4], rh[4], cl[4], cm[4], chi[4];
  up_adj_sets(Hs, rl, rm, rh);
  up_adj_sets(Ws, cl, cm, chi);
  gn_up_adjoint_body([&](int i, int jj, float& a0, float& a1) { up_gather<VEC>(gp, i, jj, Hs, Ws, rl, rm, rh, cl, cm, chi, a0, a1); }, da, dskip, C, Cs, Hs,
                     Ws, ch, b);
}

// Backward, the resize's adjoint gathered at the source resolution, one source pixel per thread and round: a [B,C,Hs,Ws] is step 1's `da`
// or, in the form without a skip, the cotangent itself.  dy = (y > 0) adjoint, stored (if given) and summed as gn_bwd_pass1_kernel does:
// the fold and pass 2 that follow are the existing ones.  FC: the columns of the window (1 with W == Ws: the pixel's own column).
template <int FC>
__device__ __forceinline__ void gn_rs_bwd_pass1_body(const float* __restrict__ a, const float* __restrict__ x, GnStrides xs, const float* __restrict__ weight,
                                                     const float* __restrict__ bias, const float* __restrict__ stats, float* __restrict__ dy,
                                                     double* __restrict__ partials, int C, int cpg, int H, int W, int Hs, int Ws, float sch, float scw,
                                                     float inh, float inw, int ch, int b) {
  __shared__ double lds[2 * kGThreads / 64];
  const int P = gridDim.x;
  const float* st = stats + 4 * ((long long)b * (C / cpg) + ch / cpg);
  const float mh = st[0], ml = st[1], rstd = st[2], wc = weight[ch], bc = bias[ch];
  const float* xp = x + (long long)b * xs.b + (long long)ch * xs.c;
  const float* ap = a + ((long long)b * C + ch) * (long long)Hs * Ws;
  float* dst = dy ? dy + ((long long)b * C + ch) * H * W : nullptr;
  const unsigned sh = (unsigned)xs.h, sw = (unsigned)xs.w;      // in-plane offsets fit 31 bits (checked on the host)
  double s1 = 0.0, s2 = 0.0;
  const int q0 = blockIdx.x * kGRounds * kGThreads + threadIdx.x, di = kGThreads / W, dj = kGThreads - di * W;
  int i = q0 / W, j = q0 - i * W;
#pragma unroll 1
  for (int r = 0; r < kGRounds && i < H; ++r) {
    int fr, fc;
    float wr[kRsFan], wcol[kRsFan];
    rs_adj_weights(i, sch, inh, H, Hs, fr, wr);
    if (FC == kRsFan) rs_adj_weights(j, scw, inw, W, Ws, fc, wcol);
    float d = 0.0f;
    if (FC == kRsFan) {
      float av[kRsFan][kRsFan];
#pragma unroll
      for (int kr = 0; kr < kRsFan; ++kr) {
        const int row = fr + kr < 0 ? 0 : fr + kr < Hs ? fr + kr : Hs - 1;
#pragma unroll
        for (int kc = 0; kc < kRsFan; ++kc) {
          const int col = fc + kc < 0 ? 0 : fc + kc < Ws ? fc + kc : Ws - 1;
          av[kr][kc] = ap[row * Ws + col];
        }
      }
      d = rs_adjoint(av, wr, wcol);
    } else {
#pragma unroll
      for (int kr = 0; kr < kRsFan; ++kr) {
        const int row = fr + kr < 0 ? 0 : fr + kr < Hs ? fr + kr : Hs - 1;
        d = fmaf(wr[kr], ap[row * Ws + j], d);
      }
    }
    const float xh = gn_xhat(xp[(unsigned)i * sh + (unsigned)j * sw], mh, ml, rstd);
    d = gn_pre(xh, wc, bc) > 0.0f ? d : 0.0f;
    s1 += (double)d;
    s2 = fma((double)d, (double)xh, s2);
    if (dst) dst[i * W + j] = d;
    i += di;
    j += dj;
    if (j >= W) { j -= W; ++i; }
  }
  block_sum2(s1, s2, lds);
  if (threadIdx.x == 0) {
    double* o = partials + 2 * (((long long)b * C + ch) * P + blockIdx.x);
    o[0] = s1;
    o[1] = s2;
  }
}
template <int FC>
__global__ __launch_bounds__(kGThreads) void gn_rs_bwd_pass1_kernel(const float* __restrict__ a, const float* __restrict__ x, GnStrides xs,
                                                                    const float* __restrict__ weight, const float* __restrict__ bias,
                                                                    const float* __restrict__ stats, float* __restrict__ dy, double* __restrict__ partials,
                                                                    int C, int cpg, int H, int W, int Hs, int Ws, float sch, float scw, float inh,
                                                                    float inw) {
  gn_rs_bwd_pass1_body<FC>(a, x, xs, weight, bias, stats, dy, partials, C, cpg, H, W, Hs, Ws, sch, scw, inh, inw, blockIdx.y, blockIdx.z);
}

// ---- host side: what stands between the C entry points and hipLaunchKernelGGL, each refusal sequence and each shared launch once ------------

// the planes of t are rows of W consecutive elements, H W % 4 == 0, and every plane starts on the boundary of a run of four (16 bytes of
// fp32, 8 of bf16)
template <typename T>
static bool g_plane_vec(const T* t, const GnStrides& s, int H, int W) {
  return s.w == 1 && s.h == W && (long long)H * W % 4 == 0 && s.c % 4 == 0 && s.b % 4 == 0 && aligned_run<T>({t});
}
// non-negative strides whose largest in-plane offset fits 31 bits: the kernels index a plane with 32-bit offsets
static bool g_plane_fits(const long long* s, int H, int W) {
  return s[2] >= 0 && s[3] >= 0 && (long long)(H - 1) * s[2] + (long long)(W - 1) * s[3] < (1ll << 31);
}
// the four strides of the C ABI as the kernels take them; nullptr (a tensor nobody reads) gives zeros
static GnStrides g_strides(const long long* s) { return s ? GnStrides{s[0], s[1], s[2], s[3]} : GnStrides{0, 0, 0, 0}; }
static int g_rounds_grid(long long items) { return (int)((items + (long long)kGThreads * kGRounds - 1) / ((long long)kGThreads * kGRounds)); }
// slices of a plane in backward pass 1
static int g_bwd_slices(int H, int W) { return g_rounds_grid((long long)H * ((W + 1) / 2)); }
// slices of a plane in the resize backward's gather: one source pixel per thread and round
static int rs_bwd_slices(int H, int W) { return g_rounds_grid((long long)H * W); }
static bool rs_domain(int H, int W, int Hs, int Ws) { return Hs >= H && Hs <= 2 * H && Ws >= W && Ws <= 2 * W; }

// floats of the group coefficients in the backward workspace, a multiple of four: what follows keeps the 16-byte alignment
static long long g_coef_floats(int B, int G) { return (2ll * B * G + 3) / 4 * 4; }

// The refusals.  Every macro names the entry point's own arguments; the order inside a macro and of the macros in an entry point is the
// order of the checks, so it decides which message wins when two things are wrong.
#define GN_CHECK_SIZES(who)                                                                              \
  SGR_REQUIRE(B > 0 && C > 0 && G > 0 && H > 0 && W > 0 && Cs >= 0, who ": non-positive size");          \
  SGR_REQUIRE(C % G == 0, who ": C is not a multiple of num_groups");                                    \
  SGR_SUPPORTED(B <= 65535 && C + Cs <= 65535, who ": B or C + Cs > 65535");                             \
  SGR_SUPPORTED((long long)H * W < (1ll << 26), who ": H * W out of range")
// the resize forms' target size, after the sizes of the single (GN_CHECK_SIZES) or the sibling form (SIB_CHECK_SIZES)
#define RS_CHECK_TARGET(who)                                                                                             \
  SGR_REQUIRE(Hs > 0 && Ws > 0, who ": non-positive size");                                                              \
  SGR_SUPPORTED(rs_domain(H, W, Hs, Ws), who ": outside the resize domain (H <= Hs <= 2H and W <= Ws <= 2W)");            \
  SGR_SUPPORTED((long long)Hs * Ws < (1ll << 26), who ": Hs * Ws out of range")
#define RS_CHECK_SIZES(who) \
  GN_CHECK_SIZES(who);      \
  RS_CHECK_TARGET(who)
// every forward after its NULL checks: SIZES is the family's *_CHECK_SIZES, strides_fit its test of the plane strides
#define GN_CHECK_FWD(who, SIZES, strides_fit)                                               \
  SIZES(who);                                                                               \
  SGR_REQUIRE(eps > 0.0f, who ": eps must be positive");                                    \
  SGR_SUPPORTED(strides_fit, who ": negative or out-of-range plane strides");               \
  SGR_REQUIRE(((uintptr_t)workspace & 7) == 0, who ": the workspace must be 8-byte aligned")
// the single operators' forward; the skip's planes are SH x SW
#define GN_CHECK_SINGLE_FWD(who, SIZES, SH, SW)                                                                                      \
  SGR_REQUIRE(x && weight && bias && out && stats && workspace && x_strides, who ": NULL tensor");                                   \
  SGR_REQUIRE((Cs == 0) == (skip == nullptr) && (!skip || skip_strides), who ": skip and its channel count do not agree");           \
  GN_CHECK_FWD(who, SIZES, g_plane_fits(x_strides, H, W) && (!skip || g_plane_fits(skip_strides, SH, SW)))
// the single operators' backward; side = dx || dweight || dbias, anything behind the normalisation
#define GN_CHECK_SINGLE_BWD(who, SIZES)                                                                           \
  SGR_REQUIRE(g, who ": NULL cotangent");                                                                         \
  SGR_REQUIRE(dx || dweight || dbias || dskip, who ": no gradient requested");                                    \
  SGR_REQUIRE(!side || (x && weight && bias && stats && workspace && x_strides), who ": NULL tensor");            \
  SGR_REQUIRE(!dskip || Cs > 0, who ": dskip requested without skip channels");                                   \
  SIZES(who);                                                                                                     \
  SGR_REQUIRE(!side || ((uintptr_t)workspace & 7) == 0, who ": the workspace must be 8-byte aligned");            \
  SGR_SUPPORTED(!side || g_plane_fits(x_strides, H, W), who ": negative or out-of-range plane strides")

// The forward's first launch: the (sum, sum of squares) partials of every (b, g), gn_slices(n) per group of n elements.  Small groups
// take one wave per workgroup.
static dim3 g_moments_block(long long n) { return dim3(n <= 2048 ? 64 : kGThreads); }
template <typename T>
static void launch_moments(const T* x, const GnStrides& xs, double* partials, int B, int G, int cpg, int H, int W, hipStream_t st) {
  const int HW = H * W;
  const long long n = (long long)cpg * HW;
  with_flag(g_plane_vec(x, xs, H, W), [&](auto VEC) {
    hipLaunchKernelGGL((gn_moments_kernel<VEC(), T>), dim3(gn_slices(n), G, B), g_moments_block(n), 0, st, x, xs, partials, cpg, W, HW, gn_slice_len(n));
  });
}
// The backward's fold: one wave per (b, g), and one per channel where dweight or dbias is wanted.
static void launch_fold(const double* partials, const float* weight, float* coef, float* dweight, float* dbias, int B, int C, int cpg, int HW, int P,
                        hipStream_t st) {
  const int jobs = B * (C / cpg) + ((dweight || dbias) ? C : 0);
  hipLaunchKernelGGL(gn_bwd_fold_kernel, dim3(jobs), dim3(64), 0, st, partials, weight, coef, dweight, dbias, B, C, cpg, P, (double)cpg * HW);
}
// Pass 2 from d: pass 1's fp32 `dy` (MASK = false, TD = float) or the cotangent itself (MASK = true, TD = T).  Runs of four where the
// planes of x, dx and d all allow them.
template <bool MASK, typename T, typename TD>
static void launch_pass2(const TD* d, const T* x, const GnStrides& xs, const float* weight, const float* bias, const float* stats, const float* coef, T* dx,
                         int B, int C, int cpg, int H, int W, hipStream_t st) {
  const int HW = H * W;
  const dim3 grid(g_rounds_grid(((long long)HW + 3) / 4), C, B);
  with_flag(g_plane_vec(x, xs, H, W) && aligned_run<T>({dx}) && aligned_run<TD>({d}), [&](auto VEC) {
    hipLaunchKernelGGL((gn_bwd_pass2_kernel<VEC(), MASK, T, TD>), grid, dim3(kGThreads), 0, st, d, x, xs, weight, bias, stats, coef, dx, C, cpg, W, HW);
  });
}

}  // namespace sgr

using namespace sgr;

extern "C" long long sgr_gn_stage_workspace_floats(int B, int C, int G, int H, int W, int upcat, int backward) {
  if (!(B > 0 && C > 0 && G > 0 && H > 0 && W > 0) || C % G != 0) return 0;
  const long long HW = (long long)H * W;
  if (!backward) return 4ll * B * G * gn_slices((long long)(C / G) * HW);
  // partials (doubles), the group coefficients, then pass 1's masked adjoint where there is one
  return 4ll * B * C * g_bwd_slices(H, W) + g_coef_floats(B, G) + (upcat ? (long long)B * C * HW : 0);
}

// sgr_gn_stage_fwd / _bwd and their bf16 forms: one body, instantiated on the type T of x, skip, the result, the cotangent, dx and dskip.
// The refusals and their messages are the fp32 entry points' for both.
template <typename T>
static int gn_stage_fwd_t(const T* x, const float* weight, const float* bias, const T* skip, T* out, float* stats, float* workspace, int B, int C, int G, int Cs,
                          int H, int W, const long long* x_strides, const long long* skip_strides, float eps, void* stream) {
  GN_CHECK_SINGLE_FWD("sgr_gn_stage_fwd", GN_CHECK_SIZES, H, W);
  const GnStrides xs = g_strides(x_strides), ss = g_strides(skip ? skip_strides : nullptr);
  const int cpg = C / G, HW = H * W, S = gn_slices((long long)cpg * HW);
  double* partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  launch_moments(x, xs, partials, B, G, cpg, H, W, st);
  if (!skip) {
    const dim3 grid(g_rounds_grid(((long long)HW + 3) / 4), C, B);
    with_flag(g_plane_vec(x, xs, H, W) && aligned_run<T>({out}), [&](auto VEC) {
      hipLaunchKernelGGL((gn_apply_plain_kernel<VEC(), T>), grid, dim3(kGThreads), 0, st, x, xs, weight, bias, partials, stats, out, C, cpg, W, HW, S, eps);
    });
  } else {
    const dim3 grid(g_rounds_grid((long long)H * ((W + 1) / 2)), C + Cs, B);
    with_flag(W % 2 == 0 && aligned_run<T>({out}), [&](auto VEC) {
      hipLaunchKernelGGL((gn_apply_up_kernel<VEC(), T>), grid, dim3(kGThreads), 0, st, x, xs, skip, ss, weight, bias, partials, stats, out, C, Cs, cpg, H, W, S, eps);
    });
  }
  return sgr_check((int)hipGetLastError(), "sgr_gn_stage_fwd");
}

template <typename T>
static int gn_stage_bwd_t(const T* g, const T* x, const float* weight, const float* bias, const float* stats, T* dx, float* dweight, float* dbias, T* dskip,
                          float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides, void* stream) {
  const bool side = dx || dweight || dbias;
  GN_CHECK_SINGLE_BWD("sgr_gn_stage_bwd", GN_CHECK_SIZES);
  const bool up = Cs > 0;
  const int cpg = C / G, HW = H * W, P = g_bwd_slices(H, W);
  const GnStrides xs = g_strides(side ? x_strides : nullptr);
  hipStream_t st = (hipStream_t)stream;
  double* partials = reinterpret_cast<double*>(workspace);
  float* coef = side ? workspace + 4ll * B * C * P : nullptr;
  float* dy = side && up && dx ? coef + g_coef_floats(B, G) : nullptr;
  // pass 1: the channels somebody wants
  const int c_begin = side ? 0 : C, c_end = dskip ? C + Cs : C;
  const dim3 grid1(P, c_end - c_begin, B);
  auto pass1 = [&](auto VEC, auto UP) {
    hipLaunchKernelGGL((gn_bwd_pass1_kernel<VEC(), UP(), T>), grid1, dim3(kGThreads), 0, st, g, x, xs, weight, bias, stats, dy, dskip, partials, C, Cs, cpg, H, W,
                       c_begin);
  };
  if (up) with_flag(W % 2 == 0 && aligned_run<T>({g}), [&](auto VEC) { pass1(VEC, std::true_type{}); });
  else pass1(std::false_type{}, std::false_type{});
  if (side) launch_fold(partials, weight, coef, dweight, dbias, B, C, cpg, HW, P, st);
  if (dx) {
    if (up) launch_pass2<false, T, float>(dy, x, xs, weight, bias, stats, coef, dx, B, C, cpg, H, W, st);
    else launch_pass2<true, T, T>(g, x, xs, weight, bias, stats, coef, dx, B, C, cpg, H, W, st);
  }
  return sgr_check((int)hipGetLastError(), "sgr_gn_stage_bwd");
}

extern "C" int sgr_gn_stage_fwd(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, float* workspace,
                                int B, int C, int G, int Cs, int H, int W, const long long* x_strides, const long long* skip_strides, float eps,
                                void* stream) {
  return gn_stage_fwd_t<float>(x, weight, bias, skip, out, stats, workspace, B, C, G, Cs, H, W, x_strides, skip_strides, eps, stream);
}
extern "C" int sgr_gn_stage_bwd(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight,
                                float* dbias, float* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides,
                                void* stream) {
  return gn_stage_bwd_t<float>(g, x, weight, bias, stats, dx, dweight, dbias, dskip, workspace, B, C, G, Cs, H, W, x_strides, stream);
}
// bf16 bit patterns travel as unsigned short through the C ABI
extern "C" int sgr_gn_stage_fwd_bf16(const unsigned short* x, const float* weight, const float* bias, const unsigned short* skip, unsigned short* out,
                                     float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides,
                                     const long long* skip_strides, float eps, void* stream) {
  return gn_stage_fwd_t<bf16>(reinterpret_cast<const bf16*>(x), weight, bias, reinterpret_cast<const bf16*>(skip), reinterpret_cast<bf16*>(out), stats, workspace, B,
                              C, G, Cs, H, W, x_strides, skip_strides, eps, stream);
}
extern "C" int sgr_gn_stage_bwd_bf16(const unsigned short* g, const unsigned short* x, const float* weight, const float* bias, const float* stats,
                                     unsigned short* dx, float* dweight, float* dbias, unsigned short* dskip, float* workspace, int B, int C, int G, int Cs,
                                     int H, int W, const long long* x_strides, void* stream) {
  return gn_stage_bwd_t<bf16>(reinterpret_cast<const bf16*>(g), reinterpret_cast<const bf16*>(x), weight, bias, stats, reinterpret_cast<bf16*>(dx), dweight, dbias,
                              reinterpret_cast<bf16*>(dskip), workspace, B, C, G, Cs, H, W, x_strides, stream);
}

// ---- resize-to-skip entry points ------------------------------------------------------------------------------------------------------------

extern "C" long long sgr_gn_resize_workspace_floats(int B, int C, int G, int H, int W, int Hs, int Ws, int upcat, int backward) {
  if (!(B > 0 && C > 0 && G > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0) || C % G != 0 || !rs_domain(H, W, Hs, Ws)) return 0;
  const long long HW = (long long)H * W;
  if (!backward) return 4ll * B * G * gn_slices((long long)(C / G) * HW);
  // partials (doubles), the group coefficients, the masked adjoint at the source resolution, then (upcat) the upsample's adjoint
  return 4ll * B * C * rs_bwd_slices(H, W) + g_coef_floats(B, G) + (long long)B * C * HW + (upcat ? (long long)B * C * Hs * Ws : 0);
}

extern "C" int sgr_gn_resize_fwd(const float* x, const float* weight, const float* bias, const float* skip, float* out, float* stats, float* workspace,
                                 int B, int C, int G, int Cs, int H, int W, int Hs, int Ws, const long long* x_strides, const long long* skip_strides,
                                 float eps, void* stream) {
  GN_CHECK_SINGLE_FWD("sgr_gn_resize_fwd", RS_CHECK_SIZES, Hs, Ws);
  const GnStrides xs = g_strides(x_strides), ss = g_strides(skip ? skip_strides : nullptr);
  const int cpg = C / G, S = gn_slices((long long)cpg * H * W);
  const float sch = (float)H / (float)Hs, scw = (float)W / (float)Ws;
  double* partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  launch_moments(x, xs, partials, B, G, cpg, H, W, st);
  if (!skip) {
    const dim3 grid(g_rounds_grid((long long)Hs * ((Ws + 3) / 4)), C, B);
    with_flag(Ws % 4 == 0 && aligned16({out}), [&](auto VEC) {
      with_flag(W == Ws, [&](auto SAMEW) {
        hipLaunchKernelGGL((gn_apply_rs_kernel<VEC(), SAMEW()>), grid, dim3(kGThreads), 0, st, x, xs, weight, bias, partials, stats, out, C, cpg, H, W, Hs, Ws, sch,
                           scw, S, eps);
      });
    });
  } else {
    const dim3 grid(g_rounds_grid((long long)Hs * ((Ws + 1) / 2)), C + Cs, B);
    with_flag(Ws % 2 == 0 && aligned16({out}), [&](auto VEC) {
      with_flag(W == Ws, [&](auto SAMEW) {
        hipLaunchKernelGGL((gn_apply_rsup_kernel<VEC(), SAMEW()>), grid, dim3(kGThreads), 0, st, x, xs, skip, ss, weight, bias, partials, stats, out, C, Cs, cpg, H,
                           W, Hs, Ws, sch, scw, S, eps);
      });
    });
  }
  return sgr_check((int)hipGetLastError(), "sgr_gn_resize_fwd");
}

extern "C" int sgr_gn_resize_bwd(const float* g, const float* x, const float* weight, const float* bias, const float* stats, float* dx, float* dweight,
                                 float* dbias, float* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws,
                                 const long long* x_strides, void* stream) {
  const bool side = dx || dweight || dbias;
  GN_CHECK_SINGLE_BWD("sgr_gn_resize_bwd", RS_CHECK_SIZES);
  const bool up = Cs > 0;
  const int cpg = C / G, HW = H * W, P = rs_bwd_slices(H, W);
  hipStream_t st = (hipStream_t)stream;
  double* partials = reinterpret_cast<double*>(workspace);
  float* coef = side ? workspace + 4ll * B * C * P : nullptr;
  float* dy = side ? coef + g_coef_floats(B, G) : nullptr;
  float* da = side && up ? dy + (long long)B * C * HW : nullptr;
  if (up) {      // step 1: the upsample's adjoint of the channels somebody wants
    const int c_begin = side ? 0 : C, c_end = dskip ? C + Cs : C;
    const dim3 grid(g_bwd_slices(Hs, Ws), c_end - c_begin, B);
    with_flag(Ws % 2 == 0 && aligned16({g}), [&](auto VEC) {
      hipLaunchKernelGGL(gn_up_adjoint_kernel<VEC()>, grid, dim3(kGThreads), 0, st, g, da, dskip, C, Cs, Hs, Ws, c_begin);
    });
  }
  if (side) {
    const GnStrides xs = g_strides(x_strides);
    const float sch = (float)H / (float)Hs, scw = (float)W / (float)Ws, inh = (float)Hs / (float)H, inw = (float)Ws / (float)W;
    const float* a = up ? da : g;
    float* dyo = dx ? dy : nullptr;
    choose<Int<1>, Int<kRsFan>>(W == Ws, [&](auto FC) {
      hipLaunchKernelGGL(gn_rs_bwd_pass1_kernel<FC()>, dim3(P, C, B), dim3(kGThreads), 0, st, a, x, xs, weight, bias, stats, dyo, partials, C, cpg, H, W, Hs, Ws, sch,
                         scw, inh, inw);
    });
    launch_fold(partials, weight, coef, dweight, dbias, B, C, cpg, HW, P, st);
    if (dx) launch_pass2<false, float, float>(dy, x, xs, weight, bias, stats, coef, dx, B, C, cpg, H, W, st);
  }
  return sgr_check((int)hipGetLastError(), "sgr_gn_resize_bwd");
}

// ---- the statistics without the apply pass: what a consumer that normalises on load (sgr_final_conv_fwd) needs ------------------------------

extern "C" int sgr_gn_moments(const float* x, float* stats, float* workspace, int B, int C, int G, int H, int W, const long long* x_strides, float eps,
                              void* stream) {
  SGR_REQUIRE(x && stats && workspace && x_strides, "sgr_gn_moments: NULL tensor");
  const int Cs = 0;
  GN_CHECK_FWD("sgr_gn_moments", GN_CHECK_SIZES, g_plane_fits(x_strides, H, W));
  const int cpg = C / G;
  const long long n = (long long)cpg * H * W;
  double* partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  // the launch of sgr_gn_stage_fwd: the same partials, and gn_group_stat folds them to the same bits
  launch_moments(x, g_strides(x_strides), partials, B, G, cpg, H, W, st);
  hipLaunchKernelGGL(gn_stats_kernel, dim3(B * G), dim3(64), 0, st, partials, stats, gn_slices(n), (double)n, eps);
  return sgr_check((int)hipGetLastError(), "sgr_gn_moments");
}

// ---- the sibling forms: D <= 8 decoders at the same stage, one shape, one skip ----------------------------------------
// The bodies above on a grid that carries the sibling index on its y axis: D C normalised channels (sibling d, channel c at d C + c), then
// the Cs skip channels once.  A skip channel is read once and written into all D results (forward); in the backward its adjoint is formed
// in registers per sibling, as the single operators form it, and added in sibling order.  The siblings' tensors and parameters travel as
// a table in the kernel arguments; the workspace holds D blocks, each laid out as the single operator's.

namespace sgr {

constexpr int kGSiblings = SGR_GN_MAX_SIBLINGS;

template <typename T>
struct SibFwd {
  const T* x[kGSiblings];
  GnStrides xs[kGSiblings];
  const float* weight[kGSiblings];
  const float* bias[kGSiblings];
  T* out[kGSiblings];
};
// g[d] == nullptr: sibling d has no cotangent (and then no dx / dweight / dbias either: the host clears them)
template <typename T>
struct SibBwd {
  const T* g[kGSiblings];
  const T* x[kGSiblings];
  GnStrides xs[kGSiblings];
  const float* weight[kGSiblings];
  const float* bias[kGSiblings];
  T* dx[kGSiblings];
  float* dweight[kGSiblings];
  float* dbias[kGSiblings];
  __device__ bool side(int d) const { return dx[d] || dweight[d] || dbias[d]; }
};
// sibling d's block of the backward workspace: partials (doubles), the group coefficients, dy, then (resize) da
struct SibWs {
  float* base;
  long long stride, coef, dy, da;      // floats
  __device__ double* partials(int d) const { return reinterpret_cast<double*>(base + d * stride); }
  __device__ float* coefs(int d) const { return base + d * stride + coef; }
  __device__ float* dys(int d) const { return base + d * stride + dy; }
  __device__ float* das(int d) const { return base + d * stride + da; }
};

// y of the grid -> (first sibling, one past the last sibling, channel of cat([y, skip])): a normalised channel belongs to one sibling, a
// skip channel to all of them
struct SibChannel { int d0, d1, ch; };
__device__ __forceinline__ SibChannel sib_channel(int y, int C, int D) {
  if (y < C * D) {
    const int d = y / C;
    return {d, d + 1, y - d * C};
  }
  return {0, D, C + (y - C * D)};
}

template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_sib_moments_kernel(SibFwd<T> t, double* __restrict__ partials, long long stride, int G, int cpg, int W, int HW,
                                                                   long long L) {
  const int d = blockIdx.y / G, g = blockIdx.y - d * G;
  gn_moments_body<VEC>(t.x[d], t.xs[d], partials + d * stride, cpg, W, HW, L, g, blockIdx.z, G);
}

template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_sib_apply_up_kernel(SibFwd<T> t, int D, const T* __restrict__ skip, GnStrides ss,
                                                                    const double* __restrict__ partials, long long stride, float* __restrict__ stats, int C,
                                                                    int Cs, int cpg, int H, int W, int S, float eps) {
  const SibChannel k = sib_channel(blockIdx.y, C, D);
  const int OW = 2 * W, d = k.d0, BG = gridDim.z * (C / cpg);
  gn_apply_up_body<VEC>(t.x[d], t.xs[d], skip, ss, t.weight[d], t.bias[d], partials + d * stride, stats + 4ll * d * BG,
                        [&](long long o, int jj, const float (&top)[4], const float (&bot)[4]) {
                          for (int e = k.d0; e < k.d1; ++e) up_store<VEC>(t.out[e] + o, jj, OW, top, bot);
                        },
                        C, Cs, cpg, H, W, S, eps, k.ch, blockIdx.z);
}

template <bool VEC, bool SAMEW>
__global__ __launch_bounds__(kGThreads) void gn_sib_apply_rsup_kernel(SibFwd<float> t, int D, const float* __restrict__ skip, GnStrides ss,
                                                                      const double* __restrict__ partials, long long stride, float* __restrict__ stats,
                                                                      int C, int Cs, int cpg, int H, int W, int Hs, int Ws, float sch, float scw, int S,
                                                                      float eps) {
  const SibChannel k = sib_channel(blockIdx.y, C, D);
  const int OW = 2 * Ws, d = k.d0, BG = gridDim.z * (C / cpg);
  gn_apply_rsup_body<SAMEW>(t.x[d], t.xs[d], skip, ss, t.weight[d], t.bias[d], partials + d * stride, stats + 4ll * d * BG,
                            [&](long long o, int jj, const float (&top)[4], const float (&bot)[4]) {
                              for (int e = k.d0; e < k.d1; ++e) up_store<VEC>(t.out[e] + o, jj, OW, top, bot);
                            },
                            C, Cs, cpg, H, W, Hs, Ws, sch, scw, S, eps, k.ch, blockIdx.z);
}

// The upsample's adjoint of channel k.ch of image b at (i, 2jj), (i, 2jj+1) of an H x W plane: one sibling's for a normalised channel; for
// a skip channel ((s_0 + s_1) + s_2) + ... over the siblings that have a cotangent, each s_d formed as the single operator forms it
template <bool VEC, typename T>
__device__ __forceinline__ void sib_adjoint(const SibBwd<T>& t, const SibChannel& k, long long plane, int i, int jj, int H, int W, const float (&rl)[4],
                                            const float (&rm)[4], const float (&rh)[4], const float (&cl)[4], const float (&cm)[4], const float (&chi)[4],
                                            float& a0, float& a1) {
  bool first = true;
  a0 = 0.0f;
  a1 = 0.0f;
  for (int e = k.d0; e < k.d1; ++e) {
    const T* g = t.g[e];
    if (!g) continue;      // uniform in the workgroup
    float u0, u1;
    up_gather<VEC>(g + plane, i, jj, H, W, rl, rm, rh, cl, cm, chi, u0, u1);
    a0 = first ? u0 : a0 + u0;
    a1 = first ? u1 : a1 + u1;
    first = false;
  }
}

template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_sib_bwd_pass1_kernel(SibBwd<T> t, int D, const float* __restrict__ stats, SibWs ws, T* __restrict__ dskip,
                                                                     int C, int Cs, int cpg, int H, int W, int y_begin) {
  const SibChannel k = sib_channel(y_begin + blockIdx.y, C, D);
  const int d = k.d0, b = blockIdx.z, BG = gridDim.z * (C / cpg);
  if (k.ch < C && !t.side(d)) return;      // a sibling without a cotangent, or with nothing wanted behind its normalisation
  const long long plane = ((long long)b * (C + Cs) + k.ch) * 4ll * H * W;
  float rl[4], rm[4], rh[4], cl[4], cm[4], chi[4];
  up_adj_sets(H, rl, rm, rh);
  up_adj_sets(W, cl, cm, chi);
  gn_bwd_pass1_body([&](int i, int jj, float& a0, float& a1) { sib_adjoint<VEC>(t, k, plane, i, jj, H, W, rl, rm, rh, cl, cm, chi, a0, a1); }, t.x[d], t.xs[d],
                    t.weight[d], t.bias[d], stats + 4ll * d * BG, t.dx[d] ? ws.dys(d) : nullptr, dskip, ws.partials(d), C, Cs, cpg, H, W, k.ch, b);
}

__global__ __launch_bounds__(64) void gn_sib_bwd_fold_kernel(SibBwd<float> t, SibWs ws, int B, int C, int cpg, int P, double n) {
  const int d = blockIdx.y;
  if (!t.side(d)) return;
  gn_bwd_fold_body(ws.partials(d), t.weight[d], ws.coefs(d), t.dweight[d], t.dbias[d], B, C, cpg, P, n);
}

template <bool VEC, typename T>
__global__ __launch_bounds__(kGThreads) void gn_sib_bwd_pass2_kernel(SibBwd<T> t, const float* __restrict__ stats, SibWs ws, int C, int cpg, int W, int HW) {
  const int d = blockIdx.y / C, c = blockIdx.y - d * C, BG = gridDim.z * (C / cpg);
  if (!t.dx[d]) return;
  gn_bwd_pass2_body<VEC, false, T, float>(ws.dys(d), t.x[d], t.xs[d], t.weight[d], t.bias[d], stats + 4ll * d * BG, ws.coefs(d), t.dx[d], C, cpg, W, HW, c,
                                          blockIdx.z);
}

// resize form, step 1: the upsample's adjoint at the skip's resolution; sibling d's normalised channels go to its `da`
template <bool VEC>
__global__ __launch_bounds__(kGThreads) void gn_sib_up_adjoint_kernel(SibBwd<float> t, int D, SibWs ws, float* __restrict__ dskip, int C, int Cs, int Hs, int Ws,
                                                                      int y_begin) {
  const SibChannel k = sib_channel(y_begin + blockIdx.y, C, D);
  const int b = blockIdx.z;
  if (k.ch < C && !t.side(k.d0)) return;
  const long long plane = ((long long)b * (C + Cs) + k.ch) * 4ll * Hs * Ws;
  float rl[4], rm[4], rh[4], cl[4], cm[4], chi[4];
  up_adj_sets(Hs, rl, rm, rh);
  up_adj_sets(Ws, cl, cm, chi);
  gn_up_adjoint_body([&](int i, int jj, float& a0, float& a1) { sib_adjoint<VEC>(t, k, plane, i, jj, Hs, Ws, rl, rm, rh, cl, cm, chi, a0, a1); },
                     ws.das(k.d0), dskip, C, Cs, Hs, Ws, k.ch, b);
}

template <int FC>
__global__ __launch_bounds__(kGThreads) void gn_sib_rs_bwd_pass1_kernel(SibBwd<float> t, const float* __restrict__ stats, SibWs ws, int C, int cpg, int H, int W,
                                                                        int Hs, int Ws, float sch, float scw, float inh, float inw) {
  const int d = blockIdx.y / C, ch = blockIdx.y - d * C, BG = gridDim.z * (C / cpg);
  if (!t.side(d)) return;
  gn_rs_bwd_pass1_body<FC>(ws.das(d), t.x[d], t.xs[d], t.weight[d], t.bias[d], stats + 4ll * d * BG, t.dx[d] ? ws.dys(d) : nullptr, ws.partials(d), C, cpg, H,
                           W, Hs, Ws, sch, scw, inh, inw, ch, blockIdx.z);
}

// ---- host side of the sibling forms -----------------------------------------------------------------------------------------------------------

// a block of the sibling workspace: the single operator's floats, rounded up so that every block starts on 16 bytes
static long long sib_block(long long single) { return (single + 3) / 4 * 4; }
// The backward workspace: D blocks of partials, coefficients, dy and (resize form: da_floats of) da, each laid out as the single operator's.
static SibWs sib_ws(float* workspace, int B, int C, int G, int HW, int P, long long da_floats) {
  SibWs ws;
  ws.base = workspace;
  ws.coef = 4ll * B * C * P;
  ws.dy = ws.coef + g_coef_floats(B, G);
  ws.da = da_floats ? ws.dy + (long long)B * C * HW : 0;
  ws.stride = sib_block(ws.dy + (long long)B * C * HW + da_floats);
  return ws;
}

template <typename T>
static bool sib_fwd_table(SibFwd<T>& t, int D, const T* const* xs, const float* const* weights, const float* const* biases, T* const* outs,
                          const long long* x_strides, int H, int W, bool& xvec, bool& ovec) {
  xvec = ovec = true;
  for (int d = 0; d < kGSiblings; ++d) {
    const int e = d < D ? d : 0;      // the unused entries repeat sibling 0: no kernel reads them
    if (!xs[e] || !weights[e] || !biases[e] || !outs[e]) return false;
    t.x[d] = xs[e]; t.weight[d] = weights[e]; t.bias[d] = biases[e]; t.out[d] = outs[e];
    t.xs[d] = g_strides(x_strides + 4 * e);
    xvec = xvec && g_plane_vec(t.x[d], t.xs[d], H, W);
    ovec = ovec && aligned_run<T>({t.out[d]});
  }
  return true;
}
static bool sib_strides_fit(int D, const long long* x_strides, int H, int W) {
  for (int d = 0; d < D; ++d)
    if (!g_plane_fits(x_strides + 4 * d, H, W)) return false;
  return true;
}

// The backward's table: a sibling without a cotangent gets no gradient; `any` = some sibling wants dx, dweight or dbias.
template <typename T>
static bool sib_bwd_table(SibBwd<T>& t, int D, const T* const* gs, const T* const* xs, const float* const* weights, const float* const* biases, T* const* dxs,
                          float* const* dweights, float* const* dbiases, const long long* x_strides, bool& any, bool& anyg, bool& anyw, bool& anydx) {
  any = anyg = anyw = anydx = false;
  for (int d = 0; d < kGSiblings; ++d) {
    t.g[d] = d < D ? gs[d] : nullptr;
    const bool has = t.g[d] != nullptr;
    t.dx[d] = has && dxs ? dxs[d] : nullptr;
    t.dweight[d] = has && dweights ? dweights[d] : nullptr;
    t.dbias[d] = has && dbiases ? dbiases[d] : nullptr;
    t.x[d] = nullptr; t.weight[d] = nullptr; t.bias[d] = nullptr;
    t.xs[d] = g_strides(nullptr);
    anyg = anyg || has;
    if (t.dx[d] || t.dweight[d] || t.dbias[d]) {
      if (!xs || !weights || !biases || !x_strides || !xs[d] || !weights[d] || !biases[d]) return false;
      t.x[d] = xs[d]; t.weight[d] = weights[d]; t.bias[d] = biases[d];
      t.xs[d] = g_strides(x_strides + 4 * d);
      any = true;
      anyw = anyw || t.dweight[d] || t.dbias[d];
      anydx = anydx || t.dx[d];
    }
  }
  return true;
}
template <typename T>
static bool sib_bwd_strides_fit(const SibBwd<T>& t, int D, int H, int W) {
  for (int d = 0; d < D; ++d) {
    const long long s[4] = {t.xs[d].b, t.xs[d].c, t.xs[d].h, t.xs[d].w};
    if (t.x[d] && !g_plane_fits(s, H, W)) return false;
  }
  return true;
}
// 128-bit (64-bit) accesses in the kernels that take them: every cotangent, or every (dy, x, dx) of the siblings that want dx
template <typename T>
static bool sib_g_vec(const SibBwd<T>& t, int D) {
  for (int d = 0; d < D; ++d)
    if (t.g[d] && !aligned_run<T>({t.g[d]})) return false;
  return true;
}
template <typename T>
static bool sib_dx_vec(const SibBwd<T>& t, int D, int H, int W) {
  for (int d = 0; d < D; ++d)
    if (t.dx[d] && !(g_plane_vec(t.x[d], t.xs[d], H, W) && aligned_run<T>({t.dx[d]}))) return false;
  return true;
}
// the fold runs on the parameters alone: one instantiation serves both I/O types
template <typename T>
static SibBwd<float> sib_fold_table(const SibBwd<T>& t) {
  SibBwd<float> f{};
  for (int d = 0; d < kGSiblings; ++d) {
    f.weight[d] = t.weight[d]; f.dweight[d] = t.dweight[d]; f.dbias[d] = t.dbias[d];
    f.dx[d] = t.dx[d] ? reinterpret_cast<float*>(t.dx[d]) : nullptr;      // only tested against nullptr
  }
  return f;
}

// The refusals of the sibling forms, in the order of the single forms' (above) around the two tables.
#define SIB_CHECK_SIZES(who)                                                                                     \
  SGR_REQUIRE(D >= 1 && D <= kGSiblings, who ": the number of siblings must be 1 .. 8");                          \
  GN_CHECK_SIZES(who);                                                                                           \
  SGR_REQUIRE(Cs > 0, who ": the sibling forms need a skip");                                                     \
  SGR_SUPPORTED((long long)C * D + Cs <= 65535 && (long long)G * D <= 65535, who ": D * C + Cs or D * G > 65535")
#define SIB_RS_CHECK_SIZES(who) \
  SIB_CHECK_SIZES(who);         \
  RS_CHECK_TARGET(who)
// the forward: fills the table t and the predicates xvec, ovec of the caller; the skip's planes are SH x SW
#define SIB_CHECK_FWD(who, SIZES, SH, SW)                                                                                           \
  SGR_REQUIRE(xs && weights && biases && skip && outs && stats && workspace && x_strides && skip_strides, who ": NULL tensor");     \
  GN_CHECK_FWD(who, SIZES, sib_strides_fit(D, x_strides, H, W) && g_plane_fits(skip_strides, SH, SW));                              \
  SGR_REQUIRE(sib_fwd_table(t, D, xs, weights, biases, outs, x_strides, H, W, xvec, ovec), who ": NULL tensor of a sibling")
// the backward: fills the table t and side, anyg, anyw, anydx of the caller
#define SIB_CHECK_BWD(who, SIZES)                                                                                                                 \
  SGR_REQUIRE(gs, who ": NULL cotangent");                                                                                                        \
  SIZES(who);                                                                                                                                     \
  SGR_REQUIRE(sib_bwd_table(t, D, gs, xs, weights, biases, dxs, dweights, dbiases, x_strides, side, anyg, anyw, anydx), who ": NULL tensor");     \
  SGR_REQUIRE(anyg, who ": NULL cotangent");                                                                                                      \
  SGR_REQUIRE(side || dskip, who ": no gradient requested");                                                                                      \
  SGR_REQUIRE(!side || (stats && workspace), who ": NULL tensor");                                                                                \
  SGR_REQUIRE(!side || ((uintptr_t)workspace & 7) == 0, who ": the workspace must be 8-byte aligned");                                            \
  SGR_SUPPORTED(sib_bwd_strides_fit(t, D, H, W), who ": negative or out-of-range plane strides")

// launch_moments for D siblings: sibling d's partials start at d * stride doubles, the single forward's workspace
template <typename T>
static void launch_sib_moments(const SibFwd<T>& t, bool xvec, double* partials, long long stride, int D, int B, int G, int cpg, int H, int W, hipStream_t st) {
  const int HW = H * W;
  const long long n = (long long)cpg * HW;
  with_flag(xvec, [&](auto VEC) {
    hipLaunchKernelGGL((gn_sib_moments_kernel<VEC(), T>), dim3(gn_slices(n), G * D, B), g_moments_block(n), 0, st, t, partials, stride, G, cpg, W, HW,
                       gn_slice_len(n));
  });
}
// launch_fold for D siblings; f is the table or its sib_fold_table
static void launch_sib_fold(const SibBwd<float>& f, const SibWs& ws, bool anyw, int D, int B, int C, int cpg, int HW, int P, hipStream_t st) {
  hipLaunchKernelGGL(gn_sib_bwd_fold_kernel, dim3(B * (C / cpg) + (anyw ? C : 0), D), dim3(64), 0, st, f, ws, B, C, cpg, P, (double)cpg * HW);
}
// launch_pass2 (from pass 1's `dy`) for D siblings
template <typename T>
static void launch_sib_pass2(const SibBwd<T>& t, const float* stats, const SibWs& ws, int D, int B, int C, int cpg, int H, int W, hipStream_t st) {
  const int HW = H * W;
  const dim3 grid(g_rounds_grid(((long long)HW + 3) / 4), C * D, B);
  // sib_dx_vec has HW % 4 == 0: every block's dy is on 16 bytes with the workspace
  with_flag(sib_dx_vec(t, D, H, W) && aligned16({ws.base}), [&](auto VEC) {
    hipLaunchKernelGGL((gn_sib_bwd_pass2_kernel<VEC(), T>), grid, dim3(kGThreads), 0, st, t, stats, ws, C, cpg, W, HW);
  });
}

template <typename T>
static int gn_stage_siblings_fwd_t(int D, const T* const* xs, const float* const* weights, const float* const* biases, const T* skip, T* const* outs, float* stats,
                                   float* workspace, int B, int C, int G, int Cs, int H, int W, const long long* x_strides, const long long* skip_strides,
                                   float eps, void* stream) {
  SibFwd<T> t;
  bool xvec, ovec;
  SIB_CHECK_FWD("sgr_gn_stage_siblings_fwd", SIB_CHECK_SIZES, H, W);
  const GnStrides ss = g_strides(skip_strides);
  const int cpg = C / G, S = gn_slices((long long)cpg * H * W);
  const long long stride = 2ll * B * G * S;      // doubles: the single forward's workspace
  double* partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  launch_sib_moments(t, xvec, partials, stride, D, B, G, cpg, H, W, st);
  const dim3 grid(g_rounds_grid((long long)H * ((W + 1) / 2)), C * D + Cs, B);
  with_flag(W % 2 == 0 && ovec, [&](auto VEC) {
    hipLaunchKernelGGL((gn_sib_apply_up_kernel<VEC(), T>), grid, dim3(kGThreads), 0, st, t, D, skip, ss, partials, stride, stats, C, Cs, cpg, H, W, S, eps);
  });
  return sgr_check((int)hipGetLastError(), "sgr_gn_stage_siblings_fwd");
}

template <typename T>
static int gn_stage_siblings_bwd_t(int D, const T* const* gs, const T* const* xs, const float* const* weights, const float* const* biases, const float* stats,
                                   T* const* dxs, float* const* dweights, float* const* dbiases, T* dskip, float* workspace, int B, int C, int G, int Cs, int H,
                                   int W, const long long* x_strides, void* stream) {
  SibBwd<T> t;
  bool side, anyg, anyw, anydx;
  SIB_CHECK_BWD("sgr_gn_stage_siblings_bwd", SIB_CHECK_SIZES);
  const int cpg = C / G, HW = H * W, P = g_bwd_slices(H, W);
  hipStream_t st = (hipStream_t)stream;
  const SibWs ws = sib_ws(workspace, B, C, G, HW, P, 0);
  // pass 1: the channels somebody wants
  const int y_begin = side ? 0 : C * D, y_end = dskip ? C * D + Cs : C * D;
  const dim3 grid1(P, y_end - y_begin, B);
  with_flag(W % 2 == 0 && sib_g_vec(t, D), [&](auto VEC) {
    hipLaunchKernelGGL((gn_sib_bwd_pass1_kernel<VEC(), T>), grid1, dim3(kGThreads), 0, st, t, D, stats, ws, dskip, C, Cs, cpg, H, W, y_begin);
  });
  if (side) launch_sib_fold(sib_fold_table(t), ws, anyw, D, B, C, cpg, HW, P, st);
  if (anydx) launch_sib_pass2(t, stats, ws, D, B, C, cpg, H, W, st);
  return sgr_check((int)hipGetLastError(), "sgr_gn_stage_siblings_bwd");
}

}  // namespace sgr

extern "C" long long sgr_gn_stage_siblings_workspace_floats(int D, int B, int C, int G, int H, int W, int backward) {
  if (D < 1 || D > kGSiblings) return 0;
  const long long single = sgr_gn_stage_workspace_floats(B, C, G, H, W, 1, backward);
  return single > 0 ? D * sib_block(single) : 0;
}
extern "C" int sgr_gn_stage_siblings_fwd(int D, const float* const* xs, const float* const* weights, const float* const* biases, const float* skip,
                                         float* const* outs, float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W,
                                         const long long* x_strides, const long long* skip_strides, float eps, void* stream) {
  return gn_stage_siblings_fwd_t<float>(D, xs, weights, biases, skip, outs, stats, workspace, B, C, G, Cs, H, W, x_strides, skip_strides, eps, stream);
}
extern "C" int sgr_gn_stage_siblings_bwd(int D, const float* const* gs, const float* const* xs, const float* const* weights, const float* const* biases,
                                         const float* stats, float* const* dxs, float* const* dweights, float* const* dbiases, float* dskip, float* workspace,
                                         int B, int C, int G, int Cs, int H, int W, const long long* x_strides, void* stream) {
  return gn_stage_siblings_bwd_t<float>(D, gs, xs, weights, biases, stats, dxs, dweights, dbiases, dskip, workspace, B, C, G, Cs, H, W, x_strides, stream);
}
extern "C" int sgr_gn_stage_siblings_fwd_bf16(int D, const unsigned short* const* xs, const float* const* weights, const float* const* biases,
                                              const unsigned short* skip, unsigned short* const* outs, float* stats, float* workspace, int B, int C, int G,
                                              int Cs, int H, int W, const long long* x_strides, const long long* skip_strides, float eps, void* stream) {
  return gn_stage_siblings_fwd_t<bf16>(D, reinterpret_cast<const bf16* const*>(xs), weights, biases, reinterpret_cast<const bf16*>(skip),
                                       reinterpret_cast<bf16* const*>(outs), stats, workspace, B, C, G, Cs, H, W, x_strides, skip_strides, eps, stream);
}
extern "C" int sgr_gn_stage_siblings_bwd_bf16(int D, const unsigned short* const* gs, const unsigned short* const* xs, const float* const* weights,
                                              const float* const* biases, const float* stats, unsigned short* const* dxs, float* const* dweights,
                                              float* const* dbiases, unsigned short* dskip, float* workspace, int B, int C, int G, int Cs, int H, int W,
                                              const long long* x_strides, void* stream) {
  return gn_stage_siblings_bwd_t<bf16>(D, reinterpret_cast<const bf16* const*>(gs), reinterpret_cast<const bf16* const*>(xs), weights, biases, stats,
                                       reinterpret_cast<bf16* const*>(dxs), dweights, dbiases, reinterpret_cast<bf16*>(dskip), workspace, B, C, G, Cs, H, W,
                                       x_strides, stream);
}

extern "C" long long sgr_gn_resize_siblings_workspace_floats(int D, int B, int C, int G, int H, int W, int Hs, int Ws, int backward) {
  if (D < 1 || D > kGSiblings) return 0;
  const long long single = sgr_gn_resize_workspace_floats(B, C, G, H, W, Hs, Ws, 1, backward);
  return single > 0 ? D * sib_block(single) : 0;
}

extern "C" int sgr_gn_resize_siblings_fwd(int D, const float* const* xs, const float* const* weights, const float* const* biases, const float* skip,
                                          float* const* outs, float* stats, float* workspace, int B, int C, int G, int Cs, int H, int W, int Hs, int Ws,
                                          const long long* x_strides, const long long* skip_strides, float eps, void* stream) {
  SibFwd<float> t;
  bool xvec, ovec;
  SIB_CHECK_FWD("sgr_gn_resize_siblings_fwd", SIB_RS_CHECK_SIZES, Hs, Ws);
  const GnStrides ss = g_strides(skip_strides);
  const int cpg = C / G, S = gn_slices((long long)cpg * H * W);
  const long long stride = 2ll * B * G * S;
  const float sch = (float)H / (float)Hs, scw = (float)W / (float)Ws;
  double* partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  launch_sib_moments(t, xvec, partials, stride, D, B, G, cpg, H, W, st);
  const dim3 grid(g_rounds_grid((long long)Hs * ((Ws + 1) / 2)), C * D + Cs, B);
  with_flag(Ws % 2 == 0 && ovec, [&](auto VEC) {
    with_flag(W == Ws, [&](auto SAMEW) {
      hipLaunchKernelGGL((gn_sib_apply_rsup_kernel<VEC(), SAMEW()>), grid, dim3(kGThreads), 0, st, t, D, skip, ss, partials, stride, stats, C, Cs, cpg, H, W, Hs, Ws,
                         sch, scw, S, eps);
    });
  });
  return sgr_check((int)hipGetLastError(), "sgr_gn_resize_siblings_fwd");
}

extern "C" int sgr_gn_resize_siblings_bwd(int D, const float* const* gs, const float* const* xs, const float* const* weights, const float* const* biases,
                                          const float* stats, float* const* dxs, float* const* dweights, float* const* dbiases, float* dskip, float* workspace,
                                          int B, int C, int G, int Cs, int H, int W, int Hs, int Ws, const long long* x_strides, void* stream) {
  SibBwd<float> t;
  bool side, anyg, anyw, anydx;
  SIB_CHECK_BWD("sgr_gn_resize_siblings_bwd", SIB_RS_CHECK_SIZES);
  const int cpg = C / G, HW = H * W, P = rs_bwd_slices(H, W);
  hipStream_t st = (hipStream_t)stream;
  const SibWs ws = sib_ws(workspace, B, C, G, HW, P, (long long)B * C * Hs * Ws);
  {      // step 1: the upsample's adjoint of the channels somebody wants
    const int y_begin = side ? 0 : C * D, y_end = dskip ? C * D + Cs : C * D;
    const dim3 grid(g_bwd_slices(Hs, Ws), y_end - y_begin, B);
    with_flag(Ws % 2 == 0 && sib_g_vec(t, D), [&](auto VEC) {
      hipLaunchKernelGGL(gn_sib_up_adjoint_kernel<VEC()>, grid, dim3(kGThreads), 0, st, t, D, ws, dskip, C, Cs, Hs, Ws, y_begin);
    });
  }
  if (side) {
    const float sch = (float)H / (float)Hs, scw = (float)W / (float)Ws, inh = (float)Hs / (float)H, inw = (float)Ws / (float)W;
    choose<Int<1>, Int<kRsFan>>(W == Ws, [&](auto FC) {
      hipLaunchKernelGGL(gn_sib_rs_bwd_pass1_kernel<FC()>, dim3(P, C * D, B), dim3(kGThreads), 0, st, t, stats, ws, C, cpg, H, W, Hs, Ws, sch, scw, inh, inw);
    });
    launch_sib_fold(t, ws, anyw, D, B, C, cpg, HW, P, st);
    if (anydx) launch_sib_pass2(t, stats, ws, D, B, C, cpg, H, W, st);
  }
  return sgr_check((int)hipGetLastError(), "sgr_gn_resize_siblings_bwd");
}
