// The reduction scheme and the 1-or-4 float (or 4 bf16) vector access of the streaming operators (sgr_loss.hip, sgr_brdf_loss.hip, sgr_brdf_input.hip,
// sgr_glue.hip, sgr_brdf_heads.hip, sgr_gn_stage.hip, sgr_final_conv.hip, sgr_recon.hip / sgr_recon_fold.h), one definition each:
//   fp32 per-thread partials -> wave ladder -> the four wave sums through LDS -> ONE partial per workgroup in a workspace -> folded in
//   double, in a fixed order, by the consumer's prologue.  No float atomics, no host synchronisation.
// Bit-identical runs and results that do not depend on the batch rest on the ORDER of the additions, so every function below states
// its order, and that order is its contract: changing it changes the bits of every operator that uses it.
// Device code: for the .hip translation units only.  The headers that also compile with g++ (sgr_gn_stage.h, sgr_regress.h, sgr_math.h)
// must not include this one.
// (Not here: bs_block_sum of sgr_bilateral.hip -- a leading barrier and the result in every thread, one user; it stays where it is.)
#pragma once

#if defined(__HIPCC__)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

namespace sgr {

// ---- wave ladder ---------------------------------------------------------------------------------------------------------------------
// v += lane (l + off)'s v for off = 32, 16, 8, 4, 2, 1, each of the N values through all six steps before the next.  The wave's sum is in
// LANE 0 ONLY (the other lanes hold partial trees).  float and double.
template <typename T, int N>
__device__ __forceinline__ void wave_sum(T (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
  }
}
// one value (an array argument picks the form above: it is the more specialised of the two)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  T a[1] = {v};
  wave_sum(a);
  return a[0];
}

// ---- workgroup sum, 256 threads ------------------------------------------------------------------------------------------------------
// N sums at once: the ladder per wave, the four wave sums l0..l3 through lds, then (l0 + l1) + (l2 + l3).  The result is in THREAD 0
// ONLY.  The workgroup must be 256 threads (four waves): the caller's __launch_bounds__ and launch say so.  One barrier inside and
// none at the end: a caller that writes lds again after the call puts its own __syncthreads() in between.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float* lds /* [4*N] */) {
  wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (lds[i] + lds[N + i]) + (lds[2 * N + i] + lds[3 * N + i]);
  }
}

// ---- fold of one partial per lane ----------------------------------------------------------------------------------------------------
// The SPLIT = 64 partials of image b, components k .. k + N - 1 of `stride`: lane l takes partial l as doubles, then for off = 1, 2, 4,
// .., 32 every component adds lane (l ^ off)'s.  Every step adds a pair both ways round and addition commutes, so EVERY lane of every
// wave of every workgroup ends with the same bits.
template <int SPLIT, int N>
__device__ __forceinline__ void fold_lanes(const float* __restrict__ ws, int b, int stride, int k, double (&out)[N]) {
  static_assert(SPLIT == 64, "one partial per lane");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = (double)ws[((size_t)b * SPLIT + lane) * stride + k + i];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] += __shfl_xor(out[i], off, 64);
  }
}
// one component: the same loads and the same tree as N = 1 above (written out: through the array form the kernels that fold one
// component at a time come out with their instructions in another order)
template <int SPLIT>
__device__ __forceinline__ double fold_lanes(const float* __restrict__ ws, int b, int stride, int k) {
  static_assert(SPLIT == 64, "one partial per lane");
  double x = (double)ws[((size_t)b * SPLIT + (threadIdx.x & 63)) * stride + k];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// ---- workgroup sum in double, THREADS threads ----------------------------------------------------------------------------------------
// N sums at once through lds[THREADS * N]: thread t puts down its v, then for s = THREADS / 2, .., 2, 1 thread t < s adds entry t + s to
// entry t.  The result is in EVERY thread.  It ends on the tree's barrier, after which every thread reads entry 0: a caller that
// writes lds again puts its own __syncthreads() in between.
template <int THREADS, int N>
__device__ __forceinline__ void block_sum_double(double (&v)[N], double* lds /* [THREADS*N] */) {
#pragma unroll
  for (int i = 0; i < N; ++i) lds[threadIdx.x * N + i] = v[i];
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int i = 0; i < N; ++i) lds[threadIdx.x * N + i] += lds[(threadIdx.x + s) * N + i];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = lds[i];
}

// ---- V = 1 or 4 consecutive floats as one access --------------------------------------------------------------------------------------
// Vec<4> is a 128-bit load / store: the address must be 16-byte aligned (aligned16 below, and an element offset that is a multiple of
// four).  Vec<1> is one float.  A kernel templated on V does the same arithmetic on the same elements in the same order either way.
template <int V> struct Vec;
template <> struct Vec<1> { float v[1]; };
template <> struct alignas(16) Vec<4> { float v[4]; };
template <int V>
__device__ __forceinline__ Vec<V> ldv(const float* __restrict__ p, size_t i) { return *reinterpret_cast<const Vec<V>*>(p + i); }
template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, size_t i, const Vec<V>& x) { *reinterpret_cast<Vec<V>*>(p + i) = x; }

// host side: every pointer on a 16-byte boundary; NULL (a tensor that is left out) counts as aligned
static inline bool aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return false;
  return true;
}

// ---- four consecutive 16-bit elements (bf16 bit patterns) as one access -----------------------------------------------------------------
// Vec4h is a 64-bit load / store: the address must be 8-byte aligned (aligned8 below, and an element offset that is a multiple of four).
// It covers the four elements Vec<4> covers of an fp32 tensor, so a kernel instantiated on either type gives a thread the same run.
struct alignas(8) Vec4h { unsigned short v[4]; };
static inline bool aligned8(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 7) return false;
  return true;
}

}  // namespace sgr

#endif  // __HIPCC__
