// The three evaluation metrics of the reference on gfx950 (CompareWHDR.py:8-66, CompareNormal.py:18-42, CompareDepth.py:16-32): from the
// predictions on the device to one number per image, with no visit to the host.
//
//   whdr           one workgroup per image: the judgements in a grid-stride loop (any N), six weighted sums in double through the block
//                  tree of sgr_reduce.h, the three ratios by thread 0
//   normal angle   pass 1, 64 workgroups per image: the prediction resized by OpenCV's rule (the 2 x 2 read directly), the angle to the
//                  unit ground truth, its key (uncounted pixels: the sentinel), and ONE partial (sum, count, NaN count) per workgroup;
//                  pass 2, one workgroup per image: the 64 partials folded in double in index order, and the two middle ranks in ONE
//                  radix select over the keys (four passes of eight bits, as lp_select of sgr_loader_prep.hip)
//   depth          one pass, 64 workgroups per image, five double sums per workgroup; a second launch folds them in index order
//
// No float atomics (the select's histograms are integer LDS atomics) and nothing across images: two runs give the same bits and image b does
// not depend on its batch.  Nothing visits the host, so the calls capture in a HIP graph.  DESIGN.md section 8o states the contracts;
// sgr_eval_metrics.h holds the decisions the host build shares.
#include "sgr_eval_metrics.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"

namespace sgr {

using namespace em;

constexpr int kEmThreads = 256;
constexpr int kEmSplit = 64;      // partials per image

struct Strides4L { long long b, c, h, w; };
struct Strides3L { long long b, h, w; };

// ---- WHDR ------------------------------------------------------------------------------------------------------------------------------
template <bool U8>
__device__ __forceinline__ float whdr_lightness(const void* __restrict__ refl, const Strides4L& st, int b, int r, int c) {
  const long long at = b * st.b + r * st.h + c * st.w;
  if (U8) {
    const unsigned char* p = static_cast<const unsigned char*>(refl) + at;
    return lightness(byte_reflectance(p[0]), byte_reflectance(p[st.c]), byte_reflectance(p[2 * st.c]));
  }
  const float* p = static_cast<const float*>(refl) + at;
  return lightness(p[0], p[st.c], p[2 * st.c]);
}

template <bool U8>
__global__ __launch_bounds__(kEmThreads) void em_whdr(const void* __restrict__ refl, Strides4L st, const int* __restrict__ point, const float* __restrict__ weight,
                                                      const int* __restrict__ label, const int* __restrict__ num, double* __restrict__ sums, float* __restrict__ out3,
                                                      int B, int H, int W, int N, float delta) {
  __shared__ double lds[kEmThreads * kSums];
  const int b = blockIdx.x;
  const int n = min(max(num[b], 0), N);
  double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < n; j += kEmThreads) {
    const size_t at = (size_t)b * N + j;
    const int* pt = point + at * 4;
    const int r1 = pt[0], c1 = pt[1], r2 = pt[2], c2 = pt[3], lab = label[at];
    const float w = weight[at];
    if (!judgement_counts(w, lab, inside(r1, c1, H, W) && inside(r2, c2, H, W))) continue;
    const float l1 = whdr_lightness<U8>(refl, st, b, r1, c1), l2 = whdr_lightness<U8>(refl, st, b, r2, c2);
    whdr_add(s, lab, whdr_class(l1, l2, delta), (double)w);
  }
  block_sum_double<kEmThreads, kSums>(s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kSums; ++i) sums[(size_t)b * kSums + i] = s[i];
    float a, e, q;
    whdr_ratios(s, a, e, q);
    out3[b] = a;
    out3[B + b] = e;
    out3[2 * B + b] = q;
  }
}

// ---- the resized prediction: the 2 x 2 read directly ------------------------------------------------------------------------------------
struct Tap2 { int a, b; float f; };
__device__ __forceinline__ Tap2 tap2(int d, int in, int out) {
  const ex::Src s = ex::src_of(d, in, out);
  return Tap2{s.s, s.s + 1 < in ? s.s + 1 : in - 1, s.f};
}
// columns first, then rows, as OpenCV
__device__ __forceinline__ float resized(const float* __restrict__ p, long long sh, long long sw, const Tap2& ty, const Tap2& tx) {
  const float top = ex::lerp2(p[ty.a * sh + tx.a * sw], p[ty.a * sh + tx.b * sw], tx.f);
  const float bot = ex::lerp2(p[ty.b * sh + tx.a * sw], p[ty.b * sh + tx.b * sw], tx.f);
  return ex::lerp2(top, bot, ty.f);
}

// ---- normal angle, pass 1 ---------------------------------------------------------------------------------------------------------------
// Workgroup (blk, b) takes pixels blk * 256 + t, + 64 * 256, .. of image b.  partials [B,64,3] doubles: sum of the counted angles, the
// count, the NaNs among the counted angles.
__global__ __launch_bounds__(kEmThreads) void em_normal_pass1(const float* __restrict__ pred, Strides4L st, const unsigned char* __restrict__ gt,
                                                              const unsigned char* __restrict__ mask, int Cm, float* __restrict__ theta, uint32_t* __restrict__ keys,
                                                              double* __restrict__ partials, int h, int w, int H, int W) {
  __shared__ double lds[kEmThreads * 3];
  const int b = blockIdx.y, HW = H * W;
  const float* pb = pred + b * st.b;
  double s[3] = {0.0, 0.0, 0.0};
  for (int p = blockIdx.x * kEmThreads + threadIdx.x; p < HW; p += kEmSplit * kEmThreads) {
    const int y = p / W, x = p - y * W;
    const Tap2 ty = tap2(y, h, H), tx = tap2(x, w, W);
    const float p0 = resized(pb, st.h, st.w, ty, tx), p1 = resized(pb + st.c, st.h, st.w, ty, tx), p2 = resized(pb + 2 * st.c, st.h, st.w, ty, tx);
    const size_t at = (size_t)b * HW + p;
    const unsigned char* g = gt + at * 3;
    float g0, g1, g2;
    gt_normal(g[0], g[1], g[2], g0, g1, g2);
    const float th = angle_deg(p0, p1, p2, g0, g1, g2);
    const unsigned char* m = mask + at * Cm;
    const bool counts = Cm == 3 ? mask_counts(m[0], m[1], m[2]) : m[0] == 255;
    theta[at] = th;
    keys[at] = counts ? lp::key_of(th) : kSentinel;
    if (counts) {
      s[1] += 1.0;
      if (th != th)
        s[2] += 1.0;
      else
        s[0] += (double)th;
    }
  }
  block_sum_double<kEmThreads, 3>(s, lds);
  if (threadIdx.x == 0) {
    double* o = partials + ((size_t)b * kEmSplit + blockIdx.x) * 3;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
  }
}

// ---- normal angle, pass 2: the fold and the two-rank select ------------------------------------------------------------------------------
constexpr int kSelThreads = 1024;

// one key into the pass's histograms; a thread folds a run of equal digits into one atomic (ties and the sentinels of a masked region do not
// serialise on one LDS word)
struct Run { int last; unsigned cnt; };
__device__ __forceinline__ void run_add(Run& r, unsigned* hist, int d) {
  if (d == r.last) {
    ++r.cnt;
  } else {
    if (r.cnt) atomicAdd(&hist[r.last], r.cnt);
    r.last = d;
    r.cnt = 1;
  }
}
__device__ __forceinline__ void run_flush(Run& r, unsigned* hist) {
  if (r.cnt) atomicAdd(&hist[r.last], r.cnt);
}
__device__ __forceinline__ void sel_key(uint32_t key, const Sel2& s, bool shared, int pass, unsigned* hist0, unsigned* hist1, Run& r0, Run& r1) {
  if (lp::in_prefix(key, s.prefix[0], pass)) run_add(r0, hist0, lp::digit_of(key, pass));
  if (!shared && lp::in_prefix(key, s.prefix[1], pass)) run_add(r1, hist1, lp::digit_of(key, pass));
}

__global__ __launch_bounds__(kSelThreads) void em_normal_pass2(const uint32_t* __restrict__ keys, const double* __restrict__ partials, float* __restrict__ mean,
                                                               float* __restrict__ median, int* __restrict__ count, int HW, int vec) {
  __shared__ unsigned hist[2][lp::kBuckets];
  __shared__ Sel2 sel;
  __shared__ unsigned s_count, s_nans;
  const int b = blockIdx.x;
  const uint32_t* kb = keys + (size_t)b * HW;
  if (threadIdx.x == 0) {
    double sum = 0.0, cnt = 0.0, nans = 0.0;
    const double* p = partials + (size_t)b * kEmSplit * 3;
    for (int i = 0; i < kEmSplit; ++i) {      // in index order
      sum += p[3 * i];
      cnt += p[3 * i + 1];
      nans += p[3 * i + 2];
    }
    const unsigned n = (unsigned)cnt;
    s_count = n;
    s_nans = (unsigned)nans;
    count[b] = (int)n;
    mean[b] = nans != 0.0 ? NAN : (float)(sum / cnt);      // 0 / 0 = NaN for an empty mask, as numpy
    sel.prefix[0] = sel.prefix[1] = 0;
    sel.rank[0] = n ? rank_lo(n) : 0;
    sel.rank[1] = n ? rank_hi(n) : 0;
  }
  __syncthreads();
  if (s_count == 0 || s_nans != 0) {      // the same for every thread of the workgroup
    if (threadIdx.x == 0) median[b] = NAN;
    return;
  }
  for (int pass = 0; pass < lp::kPasses; ++pass) {
    if (threadIdx.x < 2 * lp::kBuckets) hist[threadIdx.x >> lp::kRadixBits][threadIdx.x & (lp::kBuckets - 1)] = 0;
    __syncthreads();
    const Sel2 s = sel;
    const bool shared = sel2_shared(s, pass);
    Run r0{-1, 0}, r1{-1, 0};
    if (vec) {      // HW % 4 == 0 and the keys on a 16-byte boundary: every image starts on one
      const uint4* k4 = reinterpret_cast<const uint4*>(kb);
      for (int i = threadIdx.x; i < HW / 4; i += kSelThreads) {
        const uint4 k = k4[i];
        sel_key(k.x, s, shared, pass, hist[0], hist[1], r0, r1);
        sel_key(k.y, s, shared, pass, hist[0], hist[1], r0, r1);
        sel_key(k.z, s, shared, pass, hist[0], hist[1], r0, r1);
        sel_key(k.w, s, shared, pass, hist[0], hist[1], r0, r1);
      }
    } else {
      for (int i = threadIdx.x; i < HW; i += kSelThreads) sel_key(kb[i], s, shared, pass, hist[0], hist[1], r0, r1);
    }
    run_flush(r0, hist[0]);
    run_flush(r1, hist[1]);
    __syncthreads();
    if (threadIdx.x == 0) {
      Sel2 t = s;
      sel2_step(t, hist[0], hist[1], pass);
      sel = t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) median[b] = median_of(sel.prefix[0], sel.prefix[1], s_count, s_nans);
}

// ---- log-depth RMSE ---------------------------------------------------------------------------------------------------------------------
// partials [B,64,5] doubles
__global__ __launch_bounds__(kEmThreads) void em_depth_pass1(const float* __restrict__ pred, Strides3L ps, const float* __restrict__ gt, Strides3L gs,
                                                             double* __restrict__ partials, int h, int w, int H, int W) {
  __shared__ double lds[kEmThreads * kDepthSums];
  const int b = blockIdx.y, HW = H * W;
  const float* pb = pred + b * ps.b;
  const float* gb = gt + b * gs.b;
  double s[kDepthSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int p = blockIdx.x * kEmThreads + threadIdx.x; p < HW; p += kEmSplit * kEmThreads) {
    const int y = p / W, x = p - y * W;
    const float d = resized(pb, ps.h, ps.w, tap2(y, h, H), tap2(x, w, W));
    depth_add(s, d, gb[y * gs.h + x * gs.w]);
  }
  block_sum_double<kEmThreads, kDepthSums>(s, lds);
  if (threadIdx.x == 0) {
    double* o = partials + ((size_t)b * kEmSplit + blockIdx.x) * kDepthSums;
#pragma unroll
    for (int i = 0; i < kDepthSums; ++i) o[i] = s[i];
  }
}

// thread b folds image b's 64 partials in index order
__global__ __launch_bounds__(kEmThreads) void em_depth_finish(const double* __restrict__ partials, float* __restrict__ rmse, int* __restrict__ count, int B, double n) {
  const int b = blockIdx.x * kEmThreads + threadIdx.x;
  if (b >= B) return;
  double s[kDepthSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const double* p = partials + (size_t)b * kEmSplit * kDepthSums;
  for (int i = 0; i < kEmSplit; ++i) {
#pragma unroll
    for (int k = 0; k < kDepthSums; ++k) s[k] += p[i * kDepthSums + k];
  }
  rmse[b] = depth_rmse(s, n);
  count[b] = (int)s[kSm];
}

}  // namespace sgr

using namespace sgr;

#define SGR_EM_RANGE "(B <= 65535, h w < 2^28, H W < 2^28)"

extern "C" int sgr_eval_whdr(const void* reflectance, const long long* strides, int is_u8, const int* point, const float* weight, const int* label, const int* num,
                             double* sums, float* out3, int B, int H, int W, int N, float delta, void* stream) {
  SGR_REQUIRE(reflectance && strides && point && weight && label && num && sums && out3, "sgr_eval_whdr: NULL tensor");
  SGR_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "sgr_eval_whdr: non-positive size");
  SGR_REQUIRE(delta >= 0.0f, "sgr_eval_whdr: delta must not be negative");
  SGR_SUPPORTED(B <= 65535 && (long long)H * W < (1ll << 28) && N < (1 << 28),
                "sgr_eval_whdr: size out of range (B <= 65535, H W < 2^28, N < 2^28); on the host it is CompareWHDR.compute_whdr");
  const Strides4L st{strides[0], strides[1], strides[2], strides[3]};
  with_flag(is_u8 != 0, [&](auto U8) {
    hipLaunchKernelGGL((em_whdr<U8()>), dim3(B), dim3(kEmThreads), 0, (hipStream_t)stream, reflectance, st, point, weight, label, num, sums, out3, B, H, W, N, delta);
  });
  return sgr_check((int)hipGetLastError(), "sgr_eval_whdr");
}

extern "C" long long sgr_eval_partials_doubles(int B, int per) { return B > 0 && per > 0 ? (long long)B * kEmSplit * per : 0; }

extern "C" int sgr_eval_normal_angle(const float* normal_pred, const long long* strides, const unsigned char* normal_gt, const unsigned char* mask, int mask_channels,
                                     float* theta, unsigned* keys, double* partials, float* mean, float* median, int* count, int B, int h, int w, int H, int W,
                                     void* stream) {
  SGR_REQUIRE(normal_pred && strides && normal_gt && mask && mean && median && count, "sgr_eval_normal_angle: NULL tensor");
  SGR_REQUIRE(theta && keys && partials, "sgr_eval_normal_angle: NULL workspace (theta and keys B H W each, partials 64 * 3 * B doubles)");
  SGR_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "sgr_eval_normal_angle: non-positive size");
  SGR_REQUIRE(mask_channels == 1 || mask_channels == 3, "sgr_eval_normal_angle: the mask has 1 or 3 channels");
  SGR_SUPPORTED(B <= 65535 && (long long)h * w < (1ll << 28) && (long long)H * W < (1ll << 28),
                "sgr_eval_normal_angle: size out of range " SGR_EM_RANGE "; on the host it is the loop body of CompareNormal.py");
  const Strides4L st{strides[0], strides[1], strides[2], strides[3]};
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(em_normal_pass1, dim3(kEmSplit, B), dim3(kEmThreads), 0, s, normal_pred, st, normal_gt, mask, mask_channels, theta, keys, partials, h, w, H, W);
  const int vec = ((long long)H * W) % 4 == 0 && aligned16({keys}) ? 1 : 0;
  hipLaunchKernelGGL(em_normal_pass2, dim3(B), dim3(kSelThreads), 0, s, keys, partials, mean, median, count, H * W, vec);
  return sgr_check((int)hipGetLastError(), "sgr_eval_normal_angle");
}

extern "C" int sgr_eval_depth_log_rmse(const float* depth_pred, const long long* pred_strides, const float* depth_gt, const long long* gt_strides, double* partials,
                                       float* rmse, int* count, int B, int h, int w, int H, int W, void* stream) {
  SGR_REQUIRE(depth_pred && pred_strides && depth_gt && gt_strides && rmse && count, "sgr_eval_depth_log_rmse: NULL tensor");
  SGR_REQUIRE(partials, "sgr_eval_depth_log_rmse: NULL workspace (64 * 5 * B doubles)");
  SGR_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "sgr_eval_depth_log_rmse: non-positive size");
  SGR_SUPPORTED(B <= 65535 && (long long)h * w < (1ll << 28) && (long long)H * W < (1ll << 28),
                "sgr_eval_depth_log_rmse: size out of range " SGR_EM_RANGE "; on the host it is the loop body of CompareDepth.py");
  const Strides3L ps{pred_strides[0], pred_strides[1], pred_strides[2]}, gs{gt_strides[0], gt_strides[1], gt_strides[2]};
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(em_depth_pass1, dim3(kEmSplit, B), dim3(kEmThreads), 0, s, depth_pred, ps, depth_gt, gs, partials, h, w, H, W);
  hipLaunchKernelGGL(em_depth_finish, dim3((B + kEmThreads - 1) / kEmThreads), dim3(kEmThreads), 0, s, partials, rmse, count, B, (double)H * (double)W);
  return sgr_check((int)hipGetLastError(), "sgr_eval_depth_log_rmse");
}
