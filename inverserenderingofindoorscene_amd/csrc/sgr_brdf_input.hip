// The cascade-1 BRDF encoder's input on gfx950: wrapperBRDF.py:56-100 (= wrapperBRDFLight.py:58-92,106-108), the in-memory form of
// trainFineTune{NYU,IIW}_cascade1.py:368-374 and the inference form of testReal.py:439-449.
//
//   out [bn,17,H,W] = cat( im, norm(resize(albedo)), resize(normal'), resize(rough'), norm(resize(depth)),
//                          resize(c_im (c_d diffuse)), resize(c_im (c_s specular)) )
//   resize = F.interpolate(., [H,W], mode='bilinear') (align_corners=False) when the map is smaller than H x W along an axis, the identity
//   when it is H x W;  x' = 0.5 (x + 1) with `remap`;  norm(x) = x / max(mean_b(x), 1e-10) / 3.0 (the mean over the RESIZED map);
//   (c_d, c_s, c_im) = models.LSregressDiffSpec against adaptive_avg_pool2d(im, (R,C)).  DESIGN.md section 8c states the contract.
//
// The reference spends about 30 eager launches on this; here it is at most three, in the scheme of sgr_reduce.h: grid = (kISplit, bn)
// workgroups, fp32 per-thread partials, ONE partial set per workgroup in a workspace (block_sum), folded in double in a fixed order by the
// consumer's prologue (fold_lanes) -- no float atomics, no host synchronisation, bit-identical runs, image b's result independent of the
// batch around it.
//
//   pass A   env grid: the pooled image formed on the fly from its window, the five masked regression sums;
//            output grid: the sums of the resized albedo and depth, taps formed on the fly            (skipped: !regress && !normalize)
//   pass B   folds A's five sums into (c_d, c_s); the two sums of the second rescale over the env grid (skipped: !regress)
//   pass C   folds c_im and the two means; writes the 17 planes, V pixels of a row per thread: 128-bit stores when W % 4 == 0 and the
//            tensors are 16-byte aligned, the same kernel element by element otherwise
//
// Nothing is kept between the passes but the partials, so pass B forms the pooled image a second time (a re-read of `im` through the
// cache) and pass C forms the albedo / depth taps a second time.
#include "sgr_launch.h"
#include "sgr_reduce.h"       // block_sum, fold_lanes, Vec / ldv / stv, aligned16
#include "sgr_regress.h"

namespace sgr {

constexpr int kIThreads = 256;        // four waves: what block_sum (sgr_reduce.h) is written for
constexpr int kISplit = 64;          // workgroups per image of the two reducing passes = lanes of a wave (fold_lanes)
constexpr int kIWaves = 4;           // waves per SIMD the passes are compiled for (<= 128 VGPRs), as sgr_brdf_loss.hip
constexpr int kINA = 7;              // pass A's partials per workgroup
constexpr int kINB = 2;              // pass B's
enum { S_DD = 0, S_SS, S_DS, S_DI, S_SI, S_ALB, S_DEP };

struct BrdfIn {
  const float *im, *albedo, *normal, *rough, *depth, *diffuse, *spec;
  int H, W;      // the image = the output planes
  int h, w;      // the four BRDF maps
  int R, C;      // diffuse / specular = the env grid
  int regress, normalize, remap;
};

__device__ __forceinline__ void in_coefs(const float* __restrict__ wsA, int b, int n, float& cd, float& cs) {
  const double s5[5] = {fold_lanes<kISplit>(wsA, b, kINA, S_DD), fold_lanes<kISplit>(wsA, b, kINA, S_SS), fold_lanes<kISplit>(wsA, b, kINA, S_DS), fold_lanes<kISplit>(wsA, b, kINA, S_DI),
                        fold_lanes<kISplit>(wsA, b, kINA, S_SI)};
  diffspec_coefs(s5, (float)n, cd, cs);
}

// adaptive_avg_pool2d's cell (r, c) of one plane: torch's window start = floor(i H / R), end = ceil((i + 1) H / R), rows outermost
__device__ __forceinline__ float in_pooled(const float* __restrict__ plane, int r, int c, int H, int W, int R, int C) {
  const int y0 = (r * H) / R, y1 = ((r + 1) * H + R - 1) / R, x0 = (c * W) / C, x1 = ((c + 1) * W + C - 1) / C;
  float s = 0.0f;
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) s += plane[(size_t)y * W + x];
  return s / (float)(y1 - y0) / (float)(x1 - x0);
}

// the four taps of one output pixel in a source plane of h x w
struct Taps { int i00, i01, i10, i11; float ly0, ly1, lx0, lx1; };
__device__ __forceinline__ Taps in_taps(int oy, int ox, int h, int w, float sy, float sx) {
  Taps t;
  int y0, y1, x0, x1;
  src_index(oy, sy, h, y0, y1, t.ly0, t.ly1);
  src_index(ox, sx, w, x0, x1, t.lx0, t.lx1);
  t.i00 = y0 * w + x0; t.i01 = y0 * w + x1; t.i10 = y1 * w + x0; t.i11 = y1 * w + x1;
  return t;
}
template <typename F>
__device__ __forceinline__ float in_tap(const float* __restrict__ p, const Taps& t, F f) {
  return t.ly0 * (t.lx0 * f(p[t.i00]) + t.lx1 * f(p[t.i01])) + t.ly1 * (t.lx0 * f(p[t.i10]) + t.lx1 * f(p[t.i11]));
}
struct AsIs { __device__ __forceinline__ float operator()(float x) const { return x; } };
struct Remap { bool on; __device__ __forceinline__ float operator()(float x) const { return on ? 0.5f * (x + 1.0f) : x; } };       // trainFineTuneNYU_cascade1.py:369-370
struct Scaled { float c, cim; __device__ __forceinline__ float operator()(float x) const { return cim * (c * x); } };           // models.py:67-68, 81-82

// sum of n contiguous floats, this thread's share: elements 4 t0 .. 4 t0 + 3, then a grid stride on.  V = 4 reads them as one 128-bit
// vector (n % 4 == 0, aligned), V = 1 one by one -- the same elements in the same order, so the sum does not depend on the alignment
template <int V>
__device__ __forceinline__ void in_stream_sum(const float* __restrict__ p, int n, int t0, float& acc) {
  for (int i = t0 * 4; i < n; i += kISplit * kIThreads * 4) {
    if (V == 4) {
      const Vec<4> x = ldv<4>(p, i);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += x.v[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u < n) acc += p[i + u];
    }
  }
}

// ---- pass A -------------------------------------------------------------------------------------------------------------------------
// V: elements per load of the identity branch's albedo / depth streams (in_stream_sum)
template <int V>
__global__ __launch_bounds__(kIThreads, kIWaves) void brdfin_pass_a(BrdfIn A, float* __restrict__ wsA /* [bn,kISplit,kINA] */) {
  __shared__ float lds[4 * kINA];
  const int b = blockIdx.y;
  float acc[kINA];
#pragma unroll
  for (int k = 0; k < kINA; ++k) acc[k] = 0.0f;
  const int t0 = blockIdx.x * kIThreads + threadIdx.x;
  constexpr int stride = kISplit * kIThreads;
  if (A.regress) {
    const int RC = A.R * A.C, n = 3 * RC;
    const size_t plane = (size_t)A.H * A.W;
    for (int i = t0; i < n; i += stride) {
      const int ch = i / RC, p = i - ch * RC, r = p / A.C, c = p - r * A.C;
      const float dv = A.diffuse[(size_t)b * n + i], sv = A.spec[(size_t)b * n + i];
      const float v = in_pooled(A.im + ((size_t)b * 3 + ch) * plane, r, c, A.H, A.W, A.R, A.C);
      const float m = v < 0.9f ? 1.0f : 0.0f;      // models.py:27
      const float d = dv * m, s = sv * m, vm = v * m;
      acc[S_DD] = fmaf(d, d, acc[S_DD]); acc[S_SS] = fmaf(s, s, acc[S_SS]); acc[S_DS] = fmaf(d, s, acc[S_DS]);
      acc[S_DI] = fmaf(d, vm, acc[S_DI]); acc[S_SI] = fmaf(s, vm, acc[S_SI]);
    }
  }
  if (A.normalize) {
    const int hw = A.h * A.w, HW = A.H * A.W;
    const float* al = A.albedo + (size_t)b * 3 * hw;
    const float* dp = A.depth + (size_t)b * hw;
    if (A.h == A.H && A.w == A.W) {      // the maps are taken as they are: two contiguous streams, four consecutive elements per thread and round
      in_stream_sum<V>(al, 3 * hw, t0, acc[S_ALB]);
      in_stream_sum<V>(dp, hw, t0, acc[S_DEP]);
    } else {
      const float sy = (float)A.h / (float)A.H, sx = (float)A.w / (float)A.W;
      for (int o = t0; o < HW; o += stride) {
        const int oy = o / A.W, ox = o - oy * A.W;
        const Taps t = in_taps(oy, ox, A.h, A.w, sy, sx);
        const float a0 = in_tap(al, t, AsIs{}), a1 = in_tap(al + hw, t, AsIs{}), a2 = in_tap(al + 2 * (size_t)hw, t, AsIs{}), d0 = in_tap(dp, t, AsIs{});
        acc[S_ALB] += (a0 + a1) + a2;
        acc[S_DEP] += d0;
      }
    }
  }
  block_sum<kINA>(acc, lds);
  if (threadIdx.x == 0) {      // a workgroup that received no element writes zeros
#pragma unroll
    for (int k = 0; k < kINA; ++k) wsA[((size_t)b * kISplit + blockIdx.x) * kINA + k] = acc[k];
  }
}

// ---- pass B: the second rescale (models.py:70-77), unmasked ---------------------------------------------------------------------------
__global__ __launch_bounds__(kIThreads, kIWaves) void brdfin_pass_b(BrdfIn A, const float* __restrict__ wsA, float* __restrict__ wsB /* [bn,kISplit,kINB] */) {
  __shared__ float lds[4 * kINB];
  const int b = blockIdx.y;
  const int RC = A.R * A.C, n = 3 * RC;
  float cd, cs;
  in_coefs(wsA, b, n, cd, cs);
  float acc[kINB] = {0.0f, 0.0f};
  const size_t plane = (size_t)A.H * A.W;
  for (int i = blockIdx.x * kIThreads + threadIdx.x; i < n; i += kISplit * kIThreads) {
    const int ch = i / RC, p = i - ch * RC, r = p / A.C, c = p - r * A.C;
    const float dv = A.diffuse[(size_t)b * n + i], sv = A.spec[(size_t)b * n + i];
    const float v = in_pooled(A.im + ((size_t)b * 3 + ch) * plane, r, c, A.H, A.W, A.R, A.C);
    const float rr = fminf(fmaxf(cd * dv + cs * sv, 0.0f), 1.0f);
    acc[0] = fmaf(rr, v, acc[0]);
    acc[1] = fmaf(rr, rr, acc[1]);
  }
  block_sum<kINB>(acc, lds);
  if (threadIdx.x == 0) {
    wsB[((size_t)b * kISplit + blockIdx.x) * kINB + 0] = acc[0];
    wsB[((size_t)b * kISplit + blockIdx.x) * kINB + 1] = acc[1];
  }
}

// ---- pass C: the 17 planes --------------------------------------------------------------------------------------------------------------
// V consecutive pixels of one row (W % V == 0) of one source plane -> V output values; `same`: the plane already is H x W
template <int V, typename F>
__device__ __forceinline__ Vec<V> in_fetch(const float* __restrict__ p, bool same, int o, const Taps (&t)[V], F f) {
  Vec<V> x;
  if (same) {
    x = ldv<V>(p, o);
#pragma unroll
    for (int u = 0; u < V; ++u) x.v[u] = f(x.v[u]);
  } else {
#pragma unroll
    for (int u = 0; u < V; ++u) x.v[u] = in_tap(p, t[u], f);
  }
  return x;
}

template <int V>
__global__ __launch_bounds__(kIThreads, kIWaves) void brdfin_pass_c(BrdfIn A, const float* __restrict__ wsA, const float* __restrict__ wsB, float* __restrict__ out,
                                                                    float* __restrict__ coef /* [bn,2] */) {
  const int b = blockIdx.y;
  const int HW = A.H * A.W, hw = A.h * A.w, RC = A.R * A.C;
  float cd = 1.0f, cs = 1.0f, cim = 1.0f, ma = 1.0f, md = 1.0f;
  if (A.regress) {
    in_coefs(wsA, b, 3 * RC, cd, cs);
    cim = unit_coef(fold_lanes<kISplit>(wsB, b, kINB, 0), fold_lanes<kISplit>(wsB, b, kINB, 1));
  }
  if (A.normalize) {      // wrapperBRDF.py:84,89: the mean over the resized map
    ma = fmaxf((float)(fold_lanes<kISplit>(wsA, b, kINA, S_ALB) / (double)(3 * (size_t)HW)), 1e-10f);
    md = fmaxf((float)(fold_lanes<kISplit>(wsA, b, kINA, S_DEP) / (double)HW), 1e-10f);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    coef[2 * b] = cim * cd;
    coef[2 * b + 1] = cim * cs;
  }
  const bool sameM = A.h == A.H && A.w == A.W, sameE = A.R == A.H && A.C == A.W, norm = A.normalize != 0;
  const float sy = (float)A.h / (float)A.H, sx = (float)A.w / (float)A.W, ey = (float)A.R / (float)A.H, ex = (float)A.C / (float)A.W;
  const Remap remap{A.remap != 0};
  const float* im = A.im + (size_t)b * 3 * HW;
  const float* al = A.albedo + (size_t)b * 3 * hw;
  const float* nr = A.normal + (size_t)b * 3 * hw;
  const float* ro = A.rough + (size_t)b * hw;
  const float* dp = A.depth + (size_t)b * hw;
  const float* df = A.diffuse + (size_t)b * 3 * RC;
  const float* sp = A.spec + (size_t)b * 3 * RC;
  float* ob = out + (size_t)b * 17 * HW;
  for (int o = (blockIdx.x * kIThreads + threadIdx.x) * V; o < HW; o += gridDim.x * kIThreads * V) {
    const int oy = o / A.W, ox = o - oy * A.W;
    Taps tm[V] = {}, te[V] = {};
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if (!sameM) tm[u] = in_taps(oy, ox + u, A.h, A.w, sy, sx);
      if (!sameE) te[u] = in_taps(oy, ox + u, A.R, A.C, ey, ex);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) stv<V>(ob, (size_t)c * HW + o, ldv<V>(im, (size_t)c * HW + o));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vec<V> x = in_fetch<V>(al + (size_t)c * hw, sameM, o, tm, AsIs{});
      if (norm) {
#pragma unroll
        for (int u = 0; u < V; ++u) x.v[u] = x.v[u] / ma / 3.0f;
      }
      stv<V>(ob, (size_t)(3 + c) * HW + o, x);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) stv<V>(ob, (size_t)(6 + c) * HW + o, in_fetch<V>(nr + (size_t)c * hw, sameM, o, tm, remap));
    stv<V>(ob, (size_t)9 * HW + o, in_fetch<V>(ro, sameM, o, tm, remap));
    {
      Vec<V> x = in_fetch<V>(dp, sameM, o, tm, AsIs{});
      if (norm) {
#pragma unroll
        for (int u = 0; u < V; ++u) x.v[u] = x.v[u] / md / 3.0f;
      }
      stv<V>(ob, (size_t)10 * HW + o, x);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) stv<V>(ob, (size_t)(11 + c) * HW + o, in_fetch<V>(df + (size_t)c * RC, sameE, o, te, Scaled{cd, cim}));
#pragma unroll
    for (int c = 0; c < 3; ++c) stv<V>(ob, (size_t)(14 + c) * HW + o, in_fetch<V>(sp + (size_t)c * RC, sameE, o, te, Scaled{cs, cim}));
  }
}

// wrapperBRDF.py:56-63,73-76: a source of the output's size is taken as it is, one smaller along an axis is resized; anything else would
// fail in the reference's torch.cat
static bool in_size_legal(int h, int w, int H, int W) { return (h == H && w == W) || h < H || w < W; }

}  // namespace sgr

using namespace sgr;

extern "C" int sgr_brdf_input_workspace_floats(int bn) { return bn > 0 ? bn * kISplit * (kINA + kINB) : 0; }

extern "C" int sgr_brdf_input_fwd(const float* im, const float* albedo, const float* normal, const float* rough, const float* depth, const float* diffuse,
                                  const float* spec, float* out, float* coef, float* workspace, int bn, int H, int W, int h, int w, int R, int C, int regress,
                                  int normalize, int remap, void* stream) {
  SGR_REQUIRE(im && albedo && normal && rough && depth && diffuse && spec && out && coef && workspace, "sgr_brdf_input_fwd: NULL tensor");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && h > 0 && w > 0 && R > 0 && C > 0, "sgr_brdf_input_fwd: non-positive size");
  constexpr int kMaxSide = 32768;      // (i + 1) * H of the pooling windows stays an int
  SGR_REQUIRE(bn <= 65535 && H <= kMaxSide && W <= kMaxSide && h <= kMaxSide && w <= kMaxSide && R <= kMaxSide && C <= kMaxSide && (long long)H * W < (1ll << 28) &&
                  (long long)h * w < (1ll << 28) && (long long)R * C < (1ll << 28),
              "sgr_brdf_input_fwd: size out of range");
  SGR_REQUIRE(in_size_legal(h, w, H, W), "sgr_brdf_input_fwd: illegal source size: the BRDF maps must be H x W, or smaller than it along an axis");
  SGR_REQUIRE(in_size_legal(R, C, H, W), "sgr_brdf_input_fwd: illegal source size: diffuse / specular must be H x W, or smaller than it along an axis");
  const hipStream_t st = (hipStream_t)stream;
  const BrdfIn A{im, albedo, normal, rough, depth, diffuse, spec, H, W, h, w, R, C, regress != 0, normalize != 0, remap != 0};
  float* wsA = workspace;
  float* wsB = wsA + (size_t)bn * kISplit * kINA;
  const dim3 grid(kISplit, bn), block(kIThreads);
  const bool sameM = h == H && w == W, sameE = R == H && C == W;
  if (regress || normalize) {
    if (sameM && (h * w) % 4 == 0 && aligned16({albedo, depth}))
      hipLaunchKernelGGL(brdfin_pass_a<4>, grid, block, 0, st, A, wsA);
    else
      hipLaunchKernelGGL(brdfin_pass_a<1>, grid, block, 0, st, A, wsA);
  }
  if (regress) hipLaunchKernelGGL(brdfin_pass_b, grid, block, 0, st, A, wsA, wsB);
  // 128-bit accesses: W % 4 == 0 (four pixels of one row; every plane of every image then keeps its tensor's alignment) and aligned
  // tensors -- the output and the image always, a source only where it is read as it is
  const bool vec = W % 4 == 0 && aligned16({out, im}) && (!sameM || aligned16({albedo, normal, rough, depth})) && (!sameE || aligned16({diffuse, spec}));
  const int V = vec ? 4 : 1;
  const int want = (H * W / V + kIThreads - 1) / kIThreads;      // workgroups per image: one round of V pixels per thread ...
  const int cap = 2048 / bn > kISplit ? 2048 / bn : kISplit;      // ... up to about 2048 in all, beyond which the threads stride
  const dim3 gridC(want < cap ? want : cap, bn);
  if (vec)
    hipLaunchKernelGGL(brdfin_pass_c<4>, gridC, block, 0, st, A, wsA, wsB, out, coef);
  else
    hipLaunchKernelGGL(brdfin_pass_c<1>, gridC, block, 0, st, A, wsA, wsB, out, coef);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_input_fwd");
}
