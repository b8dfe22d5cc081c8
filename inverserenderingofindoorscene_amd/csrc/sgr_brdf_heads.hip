// Output activations of the four BRDF decoders (models.decoder0.forward, models.py:189-203) on gfx950, with the 0.5 (x + 1) the wrappers
// put on top of the albedo and depth decoders (wrapperBRDF.py, wrapperBRDFLight.py:112-115, wrapperNYU.py:89-92, wrapperIIW.py:83-86,
// testReal.py:360-363,452-455).  With s(x) = clamp(1.01 tanh(x), -1, 1):
//   albedo [bn,3,H,W] = s(x_c)                                  (mode 0; `unit`: 0.5 (. + 1))
//   normal [bn,3,H,W] = t_c / max(|t|, 1e-6),  t_c = s(x_c)     (mode 1)
//   rough  [bn,1,H,W] = (s(x_0) + s(x_1) + s(x_2)) / 3          (mode 2: the activation, then the mean)
//   depth  [bn,1,H,W] = s((x_0 + x_1 + x_2) / 3)                (mode 4: the mean, then the activation; `unit`: 0.5 (. + 1))
// x_* are the dconvFinal outputs, [bn,3,H,W] each; a NULL x leaves that decoder out.  DESIGN.md section 8d states the contract.
//
// About 22 eager launches each way in the reference; here one launch each way.  A thread owns V consecutive pixels of one image across
// the planes of every decoder present (Vec<V> of sgr_reduce.h): V = 4 with 128-bit loads and stores when H W % 4 == 0 and every tensor is 16-byte aligned, the same
// kernel element by element otherwise.  No reductions: no workspace, no atomics, bit-identical runs, image b independent of its batch.
// The backward recomputes tanh from x.
#include "sgr_launch.h"
#include "sgr_math.h"
#include "sgr_reduce.h"       // Vec / ldv / stv, aligned16
#include "sgr_tanh.h"

namespace sgr {

constexpr int kHThreads = 256;
constexpr int kHWaves = 4;      // waves per SIMD the kernels are compiled for (<= 128 VGPRs)
enum { T_ALBEDO = 0, T_NORMAL, T_ROUGH, T_DEPTH };

struct BrdfHeadsFwd { const float* x[4]; float* y[4]; };
struct BrdfHeadsBwd { const float* x[4]; const float* g[4]; float* gx[4]; };

// s(x); the product is rounded on its own: the clamp's kinks sit on its bits
__device__ __forceinline__ float h_act(float x) { return fminf(fmaxf(fmul_rn(1.01f, tanh_f(x)), -1.0f), 1.0f); }
// s(x) and s'(x) = 1.01 (1 - tanh^2 x) on -1 <= 1.01 tanh x <= 1 (closed, like torch's clamp), 0 outside
__device__ __forceinline__ float h_act_d(float x, float& d) {
  const float t = tanh_f(x), a = fmul_rn(1.01f, t);
  d = (a >= -1.0f && a <= 1.0f) ? 1.01f * (1.0f - t * t) : 0.0f;
  return fminf(fmaxf(a, -1.0f), 1.0f);
}
// the wrappers' 0.5 * (y + 1), each operation rounded as torch does (unit_pre of sgr_heads.hip)
__device__ __forceinline__ float h_unit(float y) { return fmul_rn(0.5f, fadd_rn(y, 1.0f)); }
__device__ __forceinline__ float h_norm(float t0, float t1, float t2) {
  return sqrtf(fadd_rn(fadd_rn(fmul_rn(t0, t0), fmul_rn(t1, t1)), fmul_rn(t2, t2)));
}

template <int V>
__global__ __launch_bounds__(kHThreads, kHWaves) void brdf_heads_fwd_kernel(BrdfHeadsFwd A, int HW, int unit) {
  const size_t i3 = (size_t)blockIdx.y * 3 * HW, i1 = (size_t)blockIdx.y * HW;
  for (int o = (blockIdx.x * kHThreads + threadIdx.x) * V; o < HW; o += gridDim.x * kHThreads * V) {
    if (A.x[T_ALBEDO]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Vec<V> x = ldv<V>(A.x[T_ALBEDO], i3 + (size_t)c * HW + o);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          const float y = h_act(x.v[u]);
          x.v[u] = unit ? h_unit(y) : y;
        }
        stv<V>(A.y[T_ALBEDO], i3 + (size_t)c * HW + o, x);
      }
    }
    if (A.x[T_NORMAL]) {
      Vec<V> x0 = ldv<V>(A.x[T_NORMAL], i3 + o), x1 = ldv<V>(A.x[T_NORMAL], i3 + HW + o), x2 = ldv<V>(A.x[T_NORMAL], i3 + 2 * (size_t)HW + o);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float t0 = h_act(x0.v[u]), t1 = h_act(x1.v[u]), t2 = h_act(x2.v[u]);
        const float n = fmaxf(h_norm(t0, t1, t2), 1e-6f);
        x0.v[u] = t0 / n; x1.v[u] = t1 / n; x2.v[u] = t2 / n;
      }
      stv<V>(A.y[T_NORMAL], i3 + o, x0); stv<V>(A.y[T_NORMAL], i3 + HW + o, x1); stv<V>(A.y[T_NORMAL], i3 + 2 * (size_t)HW + o, x2);
    }
    if (A.x[T_ROUGH]) {
      const Vec<V> x0 = ldv<V>(A.x[T_ROUGH], i3 + o), x1 = ldv<V>(A.x[T_ROUGH], i3 + HW + o), x2 = ldv<V>(A.x[T_ROUGH], i3 + 2 * (size_t)HW + o);
      Vec<V> y;
#pragma unroll
      for (int u = 0; u < V; ++u) y.v[u] = fadd_rn(fadd_rn(h_act(x0.v[u]), h_act(x1.v[u])), h_act(x2.v[u])) / 3.0f;
      stv<V>(A.y[T_ROUGH], i1 + o, y);
    }
    if (A.x[T_DEPTH]) {
      const Vec<V> x0 = ldv<V>(A.x[T_DEPTH], i3 + o), x1 = ldv<V>(A.x[T_DEPTH], i3 + HW + o), x2 = ldv<V>(A.x[T_DEPTH], i3 + 2 * (size_t)HW + o);
      Vec<V> y;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float s = h_act(fadd_rn(fadd_rn(x0.v[u], x1.v[u]), x2.v[u]) / 3.0f);
        y.v[u] = unit ? h_unit(s) : s;
      }
      stv<V>(A.y[T_DEPTH], i1 + o, y);
    }
  }
}

// A term is worked on only where its gradient is wanted (gx != NULL); a NULL cotangent is zero and gives a zero gradient without a read.
template <int V>
__global__ __launch_bounds__(kHThreads, kHWaves) void brdf_heads_bwd_kernel(BrdfHeadsBwd A, int HW, int unit) {
  const size_t i3 = (size_t)blockIdx.y * 3 * HW, i1 = (size_t)blockIdx.y * HW;
  const float us = unit ? 0.5f : 1.0f;
  Vec<V> zero;
#pragma unroll
  for (int u = 0; u < V; ++u) zero.v[u] = 0.0f;
  for (int o = (blockIdx.x * kHThreads + threadIdx.x) * V; o < HW; o += gridDim.x * kHThreads * V) {
    if (A.gx[T_ALBEDO]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t i = i3 + (size_t)c * HW + o;
        Vec<V> r = zero;
        if (A.g[T_ALBEDO]) {
          const Vec<V> x = ldv<V>(A.x[T_ALBEDO], i), g = ldv<V>(A.g[T_ALBEDO], i);
#pragma unroll
          for (int u = 0; u < V; ++u) {
            float d;
            h_act_d(x.v[u], d);
            r.v[u] = us * g.v[u] * d;
          }
        }
        stv<V>(A.gx[T_ALBEDO], i, r);
      }
    }
    if (A.gx[T_NORMAL]) {
      Vec<V> r0 = zero, r1 = zero, r2 = zero;
      if (A.g[T_NORMAL]) {
        const Vec<V> x0 = ldv<V>(A.x[T_NORMAL], i3 + o), x1 = ldv<V>(A.x[T_NORMAL], i3 + HW + o), x2 = ldv<V>(A.x[T_NORMAL], i3 + 2 * (size_t)HW + o);
        const Vec<V> g0 = ldv<V>(A.g[T_NORMAL], i3 + o), g1 = ldv<V>(A.g[T_NORMAL], i3 + HW + o), g2 = ldv<V>(A.g[T_NORMAL], i3 + 2 * (size_t)HW + o);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float d0, d1, d2;
          const float t0 = h_act_d(x0.v[u], d0), t1 = h_act_d(x1.v[u], d1), t2 = h_act_d(x2.v[u], d2);
          const float nr = h_norm(t0, t1, t2);
          const float inv = 1.0f / fmaxf(nr, 1e-6f);
          // gt = (g - y (y . g)) / n, y = t / n; below 1e-6 the min-clamp blocks the norm path: gt = g / 1e-6 (heads_bwd_kernel's rule)
          const float dot = nr >= 1e-6f ? (t0 * g0.v[u] + t1 * g1.v[u] + t2 * g2.v[u]) * inv * inv : 0.0f;
          r0.v[u] = (g0.v[u] - t0 * dot) * inv * d0;
          r1.v[u] = (g1.v[u] - t1 * dot) * inv * d1;
          r2.v[u] = (g2.v[u] - t2 * dot) * inv * d2;
        }
      }
      stv<V>(A.gx[T_NORMAL], i3 + o, r0); stv<V>(A.gx[T_NORMAL], i3 + HW + o, r1); stv<V>(A.gx[T_NORMAL], i3 + 2 * (size_t)HW + o, r2);
    }
    if (A.gx[T_ROUGH]) {
      Vec<V> r0 = zero, r1 = zero, r2 = zero;
      if (A.g[T_ROUGH]) {
        const Vec<V> x0 = ldv<V>(A.x[T_ROUGH], i3 + o), x1 = ldv<V>(A.x[T_ROUGH], i3 + HW + o), x2 = ldv<V>(A.x[T_ROUGH], i3 + 2 * (size_t)HW + o);
        const Vec<V> g = ldv<V>(A.g[T_ROUGH], i1 + o);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float d0, d1, d2;
          h_act_d(x0.v[u], d0); h_act_d(x1.v[u], d1); h_act_d(x2.v[u], d2);
          const float g3 = g.v[u] / 3.0f;
          r0.v[u] = g3 * d0; r1.v[u] = g3 * d1; r2.v[u] = g3 * d2;
        }
      }
      stv<V>(A.gx[T_ROUGH], i3 + o, r0); stv<V>(A.gx[T_ROUGH], i3 + HW + o, r1); stv<V>(A.gx[T_ROUGH], i3 + 2 * (size_t)HW + o, r2);
    }
    if (A.gx[T_DEPTH]) {
      Vec<V> r = zero;
      if (A.g[T_DEPTH]) {
        const Vec<V> x0 = ldv<V>(A.x[T_DEPTH], i3 + o), x1 = ldv<V>(A.x[T_DEPTH], i3 + HW + o), x2 = ldv<V>(A.x[T_DEPTH], i3 + 2 * (size_t)HW + o);
        const Vec<V> g = ldv<V>(A.g[T_DEPTH], i1 + o);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          float d;
          h_act_d(fadd_rn(fadd_rn(x0.v[u], x1.v[u]), x2.v[u]) / 3.0f, d);
          r.v[u] = us * g.v[u] * d / 3.0f;
        }
      }
      stv<V>(A.gx[T_DEPTH], i3 + o, r); stv<V>(A.gx[T_DEPTH], i3 + HW + o, r); stv<V>(A.gx[T_DEPTH], i3 + 2 * (size_t)HW + o, r);
    }
  }
}

// workgroups per image: one round of V pixels per thread up to about 2048 in all, beyond which the threads stride (brdfin_pass_c's rule)
static dim3 h_grid(int bn, int HW, int V) {
  const int want = (HW / V + kHThreads - 1) / kHThreads;
  const int cap = 2048 / bn > 64 ? 2048 / bn : 64;
  return dim3(want < cap ? want : cap, bn);
}

}  // namespace sgr

using namespace sgr;

extern "C" int sgr_brdf_heads_fwd(const float* x_albedo, const float* x_normal, const float* x_rough, const float* x_depth, float* albedo, float* normal,
                                  float* rough, float* depth, int bn, int H, int W, int unit, void* stream) {
  SGR_REQUIRE(x_albedo || x_normal || x_rough || x_depth, "sgr_brdf_heads_fwd: every decoder output is NULL");
  SGR_REQUIRE((!x_albedo || albedo) && (!x_normal || normal) && (!x_rough || rough) && (!x_depth || depth),
              "sgr_brdf_heads_fwd: NULL output for a decoder output that is given");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0, "sgr_brdf_heads_fwd: non-positive size");
  SGR_SUPPORTED(bn <= 65535, "sgr_brdf_heads_fwd: bn > 65535");
  SGR_SUPPORTED((long long)H * W < (1ll << 28), "sgr_brdf_heads_fwd: H * W out of range");
  const int HW = H * W;
  const BrdfHeadsFwd A{{x_albedo, x_normal, x_rough, x_depth}, {x_albedo ? albedo : nullptr, x_normal ? normal : nullptr, x_rough ? rough : nullptr, x_depth ? depth : nullptr}};
  const bool vec = HW % 4 == 0 && aligned16({A.x[0], A.x[1], A.x[2], A.x[3], A.y[0], A.y[1], A.y[2], A.y[3]});      // a decoder left out: NULL, aligned
  if (vec)
    hipLaunchKernelGGL(brdf_heads_fwd_kernel<4>, h_grid(bn, HW, 4), dim3(kHThreads), 0, (hipStream_t)stream, A, HW, unit != 0);
  else
    hipLaunchKernelGGL(brdf_heads_fwd_kernel<1>, h_grid(bn, HW, 1), dim3(kHThreads), 0, (hipStream_t)stream, A, HW, unit != 0);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_heads_fwd");
}

extern "C" int sgr_brdf_heads_bwd(const float* x_albedo, const float* x_normal, const float* x_rough, const float* x_depth, const float* g_albedo,
                                  const float* g_normal, const float* g_rough, const float* g_depth, float* gx_albedo, float* gx_normal, float* gx_rough,
                                  float* gx_depth, int bn, int H, int W, int unit, void* stream) {
  SGR_REQUIRE(x_albedo || x_normal || x_rough || x_depth, "sgr_brdf_heads_bwd: every decoder output is NULL");
  SGR_REQUIRE((x_albedo || !gx_albedo) && (x_normal || !gx_normal) && (x_rough || !gx_rough) && (x_depth || !gx_depth),
              "sgr_brdf_heads_bwd: gradient requested for a decoder output that is NULL");
  SGR_REQUIRE(gx_albedo || gx_normal || gx_rough || gx_depth, "sgr_brdf_heads_bwd: no gradient requested");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0, "sgr_brdf_heads_bwd: non-positive size");
  SGR_SUPPORTED(bn <= 65535, "sgr_brdf_heads_bwd: bn > 65535");
  SGR_SUPPORTED((long long)H * W < (1ll << 28), "sgr_brdf_heads_bwd: H * W out of range");
  const int HW = H * W;
  BrdfHeadsBwd A{{x_albedo, x_normal, x_rough, x_depth}, {g_albedo, g_normal, g_rough, g_depth}, {gx_albedo, gx_normal, gx_rough, gx_depth}};
  for (int k = 0; k < 4; ++k) {
    if (!A.gx[k]) A.x[k] = A.g[k] = nullptr;      // neither read nor considered for the alignment
    if (!A.g[k]) A.x[k] = nullptr;
  }
  const bool vec = HW % 4 == 0 && aligned16({A.x[0], A.x[1], A.x[2], A.x[3], A.g[0], A.g[1], A.g[2], A.g[3], A.gx[0], A.gx[1], A.gx[2], A.gx[3]});
  if (vec)
    hipLaunchKernelGGL(brdf_heads_bwd_kernel<4>, h_grid(bn, HW, 4), dim3(kHThreads), 0, (hipStream_t)stream, A, HW, unit != 0);
  else
    hipLaunchKernelGGL(brdf_heads_bwd_kernel<1>, h_grid(bn, HW, 1), dim3(kHThreads), 0, (hipStream_t)stream, A, HW, unit != 0);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_heads_bwd");
}
