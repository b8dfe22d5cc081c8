// The BRDF-stage training objectives on gfx950.
//
//   synthetic objective ...... wrapperBRDF.py:109-130 (= trainBRDF.py:248-286)      NYU objective ... wrapperNYU.py:97-111
//   IIW ranking objective .... wrapperIIW.py:88-109 with models.BatchRankingLoss (models.py:526-563)
//
// The objective is a streaming reduction over up to 18 full-resolution planes (88 MB at 16 x 240 x 320), so unlike the render loss of
// sgr_loss.hip it is bandwidth territory, not launch territory.  Same scheme otherwise, the one sgr_reduce.h defines: grid = (kBSplit, bn)
// workgroups, fp32 per-thread partials, block_sum, ONE partial per workgroup written to a workspace; the next kernel's prologue folds the
// partials it needs with fold_lanes -- no float atomics, no host synchronisation (the reference's two `.item()` on the mask sums,
// wrapperBRDF.py:118-119, stay on the device), two runs are bit-identical.
//
//   pass A     every plane once: the two LSregress sum pairs, the three mask sums, the normal / rough / angle numerators
//   pass B     folds the regression sums of its image, re-reads the albedo and depth planes: the two numerators that need a coefficient
//   totals     one workgroup: the batch totals `parts[8]` and (one rank) the six reported values
//   backward   one pass, launched by the autograd node: reads the five upstream gradients from device memory, writes the gradients of
//              the predictions that require one (a separate launch, not pass B's epilogue: five scalars carry gradient separately, so
//              there is no single "unit upstream" to pre-apply, and a forward-only evaluation writes no gradient plane at all)
//
// Absent terms (NULL prediction) are neither read nor written.  Planes are read as 128-bit vectors when H*W is a multiple of four
// (every plane of every image then starts on a 16-byte boundary), element by element otherwise.
#include <stdio.h>

#include "sgr_launch.h"
#include "sgr_reduce.h"       // block_sum, fold_lanes, Vec / ldv / stv, aligned16
#include "sgr_regress.h"      // unit_coef

namespace sgr {

constexpr int kBThreads = 256;        // four waves: what block_sum (sgr_reduce.h) is written for
constexpr int kBSplit = 64;          // workgroups per image of every pass = lanes of a wave (fold_lanes): 1024 workgroups at batch 16, below the ~2048 beyond
                                     // which a grid should stride instead; measured at 16 x 480 x 640: pass A 4.6-6.4 TB/s, the backward 6.35
constexpr int kBWaves = 4;           // waves per SIMD the streaming passes are compiled for (<= 128 VGPRs): four workgroups per CU, so the 1024
                                     // workgroups of batch 16 are ONE round on 256 CUs (at three per CU the second round ran a third full)
constexpr int kNA = 10;              // pass A's partials per workgroup
constexpr int kNB = 2;               // pass B's
enum { A_PG = 0, A_PP, D_PG, D_PP, N_OBJ, N_ALL, N_DEP, NUM_N, NUM_R, NUM_ANG };

struct BrdfPlanes {
  const float *aP, *aG, *nP, *nG, *rP, *rG, *dP, *dG;      // predictions / ground truth; a NULL prediction = term absent
  const float *sB, *sA, *sD;                             // segBRDF, segAll, the depth mask (== sA unless the caller has a separate one)
};

// ---- pass A -------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBThreads, kBWaves) void brdf_pass_a(BrdfPlanes P, float* __restrict__ wsA /* [bn,kBSplit,kNA] */, int HW) {
  __shared__ float lds[4 * kNA];
  const int b = blockIdx.y;
  const bool hasA = P.aP, hasN = P.nP, hasR = P.rP, hasD = P.dP, sepD = hasD && P.sD != P.sA;
  float acc[kNA];
#pragma unroll
  for (int k = 0; k < kNA; ++k) acc[k] = 0.0f;
  const size_t o1 = (size_t)b * HW, o3 = (size_t)b * 3 * HW;
  for (int i = (blockIdx.x * kBThreads + threadIdx.x) * V; i < HW; i += kBSplit * kBThreads * V) {
    // the masks first, then term by term: a block's loads are issued before its first use, and the compiler hoists the next block's as
    // far as the 128 registers of kBWaves allow
    Vec<V> sb{}, sa{}, sd{};
    if (hasA || hasR) sb = ldv<V>(P.sB, o1 + i);
    if (hasN || hasD) sa = ldv<V>(P.sA, o1 + i);
    if (sepD) sd = ldv<V>(P.sD, o1 + i);
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if (hasA || hasR) acc[N_OBJ] += sb.v[u];
      if (hasN || hasD) acc[N_ALL] += sa.v[u];
      if (hasD) acc[N_DEP] += sepD ? sd.v[u] : sa.v[u];
    }
    if (hasA) {
      Vec<V> ap[3], ag[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ap[c] = ldv<V>(P.aP, o3 + (size_t)c * HW + i); ag[c] = ldv<V>(P.aG, o3 + (size_t)c * HW + i); }
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float mB = sb.v[u];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float p = ap[c].v[u] * mB, g = (mB * ag[c].v[u]) * mB;      // wrapperBRDF.py:109-111: the mask enters the ground truth twice
          acc[A_PG] = fmaf(p, g, acc[A_PG]);
          acc[A_PP] = fmaf(p, p, acc[A_PP]);
        }
      }
    }
    if (hasN) {
      Vec<V> np[3], ng[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { np[c] = ldv<V>(P.nP, o3 + (size_t)c * HW + i); ng[c] = ldv<V>(P.nG, o3 + (size_t)c * HW + i); }
#pragma unroll
      for (int u = 0; u < V; ++u) {
        float dot = 0.0f, sq = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float e = np[c].v[u] - ng[c].v[u];
          sq = fmaf(e, e, sq);
          dot = fmaf(np[c].v[u], ng[c].v[u], dot);
        }
        acc[NUM_N] = fmaf(sq, sa.v[u], acc[NUM_N]);
        acc[NUM_ANG] = fmaf(acosf(fminf(fmaxf(dot, -1.0f), 1.0f)) / 3.14159265358979323846f * 180.0f, sa.v[u], acc[NUM_ANG]);      // wrapperNYU.py:111
      }
    }
    if (hasR) {
      const Vec<V> rp = ldv<V>(P.rP, o1 + i), rg = ldv<V>(P.rG, o1 + i);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float e = rp.v[u] - rg.v[u];
        acc[NUM_R] = fmaf(e * e, sb.v[u], acc[NUM_R]);
      }
    }
    if (hasD) {
      const Vec<V> dp = ldv<V>(P.dP, o1 + i), dg = ldv<V>(P.dG, o1 + i);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float mD = sepD ? sd.v[u] : sa.v[u];
        const float p = dp.v[u] * mD, g = dg.v[u] * mD;
        acc[D_PG] = fmaf(p, g, acc[D_PG]);
        acc[D_PP] = fmaf(p, p, acc[D_PP]);
      }
    }
  }
  block_sum<kNA>(acc, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kNA; ++k) wsA[((size_t)b * kBSplit + blockIdx.x) * kNA + k] = acc[k];
  }
}

// ---- pass B: the albedo and depth numerators (they need the image's coefficients) -------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBThreads, kBWaves) void brdf_pass_b(BrdfPlanes P, const float* __restrict__ wsA, float* __restrict__ wsB /* [bn,kBSplit,kNB] */,
                                                         float* __restrict__ coef /* [bn,2] */, int HW, float off) {
  __shared__ float lds[4 * kNB];
  const int b = blockIdx.y;
  const bool hasA = P.aP, hasD = P.dP;
  const float cA = hasA ? unit_coef(fold_lanes<kBSplit>(wsA, b, kNA, A_PG), fold_lanes<kBSplit>(wsA, b, kNA, A_PP)) : 0.0f;
  const float cD = hasD ? unit_coef(fold_lanes<kBSplit>(wsA, b, kNA, D_PG), fold_lanes<kBSplit>(wsA, b, kNA, D_PP)) : 0.0f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    coef[2 * b] = cA;
    coef[2 * b + 1] = cD;
  }
  float acc[kNB] = {0.0f, 0.0f};
  const size_t o1 = (size_t)b * HW, o3 = (size_t)b * 3 * HW;
  for (int i = (blockIdx.x * kBThreads + threadIdx.x) * V; i < HW; i += kBSplit * kBThreads * V) {
    Vec<V> sb{}, sd{}, ap[3], ag[3], dp{}, dg{};
    if (hasA) {
      sb = ldv<V>(P.sB, o1 + i);
#pragma unroll
      for (int c = 0; c < 3; ++c) { ap[c] = ldv<V>(P.aP, o3 + (size_t)c * HW + i); ag[c] = ldv<V>(P.aG, o3 + (size_t)c * HW + i); }
    }
    if (hasD) { sd = ldv<V>(P.sD, o1 + i); dp = ldv<V>(P.dP, o1 + i); dg = ldv<V>(P.dG, o1 + i); }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if (hasA) {
        const float mB = sb.v[u];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float e = fminf(fmaxf(ap[c].v[u] * cA, 0.0f), 1.0f) - mB * ag[c].v[u];      // wrapperBRDF.py:112,121
          acc[0] = fmaf(e * e, mB, acc[0]);
        }
      }
      if (hasD) {
        const float e = logf(dp.v[u] * cD + off) - logf(dg.v[u] + off);      // the accurate logf (wrapperBRDF.py:129, wrapperNYU.py:108)
        acc[1] = fmaf(e * e, sd.v[u], acc[1]);
      }
    }
  }
  block_sum<kNB>(acc, lds);
  if (threadIdx.x == 0) {
    wsB[((size_t)b * kBSplit + blockIdx.x) * kNB + 0] = acc[0];
    wsB[((size_t)b * kBSplit + blockIdx.x) * kNB + 1] = acc[1];
  }
}

// ---- the reported values from the (rank-summed) totals -------------------------------------------------------------------------------
//   parts  = (numAlbedo, numNormal, numRough, numDepth, numAngle, nObj, nAll, nDep)
//   values = (total, albedoErr, normalErr, roughErr, depthErr, angleMean);  denominators through max(., 1e-5): an empty term is 0
__device__ __forceinline__ void brdf_values(const float* parts, float wA, float wN, float wR, float wD, float* values) {
  const float nObj = fmaxf(parts[5], 1e-5f), nAll = fmaxf(parts[6], 1e-5f), nDep = fmaxf(parts[7], 1e-5f);
  const float eA = parts[0] / nObj / 3.0f, eN = parts[1] / nAll / 3.0f, eR = parts[2] / nObj, eD = parts[3] / nDep;
  values[0] = ((wA * eA + wN * eN) + wR * eR) + wD * eD;
  values[1] = eA; values[2] = eN; values[3] = eR; values[4] = eD;
  values[5] = parts[4] / nAll;
}

// one workgroup: the eight batch totals of this rank's shard.  Thread t takes partials t, t + 256, ... of all eight components (every load
// issued before the first use), adds them in double, then the tree of sgr_reduce.h's block_sum in double (the ladder per wave, the four waves as (w0 + w1) + (w2 + w3)).
__global__ __launch_bounds__(kBThreads) void brdf_totals(const float* __restrict__ wsA, const float* __restrict__ wsB, int nparts, float* __restrict__ parts,
                                                         float* __restrict__ values /* nullable */, float wA, float wN, float wR, float wD) {
  __shared__ double lds[(kBThreads / 64) * 8];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += kBThreads) {
    const float* a = wsA + (size_t)i * kNA;
    const float* b = wsB + (size_t)i * kNB;
    const float v[8] = {b[0], a[NUM_N], a[NUM_R], b[1], a[NUM_ANG], a[N_OBJ], a[N_ALL], a[N_DEP]};
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += (double)v[k];
  }
  // wave_sum's ladder and block_sum's fold, in double.  Written out: through wave_sum(s) the kernel comes out with its instructions in
  // another order and four s_waitcnt fewer -- the same bits, but not the listing that was measured.
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) lds[wave * 8 + k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      tot[k] = (float)((lds[k] + lds[8 + k]) + (lds[16 + k] + lds[24 + k]));
      parts[k] = tot[k];
    }
    if (values) brdf_values(tot, wA, wN, wR, wD, values);
  }
}
__global__ void brdf_finalize(const float* __restrict__ parts, float* __restrict__ values, float wA, float wN, float wR, float wD) {
  brdf_values(parts, wA, wN, wR, wD, values);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
struct BrdfUpstream { const float *total, *albedo, *normal, *rough, *depth; };      // 0-d device tensors, each nullable (= 0)
struct BrdfGrads { float *aP, *nP, *rP, *dP; };                                      // nullable: not wanted

template <int V>
__global__ __launch_bounds__(kBThreads, kBWaves) void brdf_bwd(BrdfPlanes P, BrdfUpstream U, BrdfGrads G, const float* __restrict__ coef, const float* __restrict__ parts,
                                                      int HW, float wA, float wN, float wR, float wD, float off) {
  const int b = blockIdx.y;
  const float gt = U.total ? U.total[0] : 0.0f;
  const float nObj = fmaxf(parts[5], 1e-5f), nAll = fmaxf(parts[6], 1e-5f), nDep = fmaxf(parts[7], 1e-5f);
  const float cA = coef[2 * b], cD = coef[2 * b + 1];
  const float kA = (gt * wA + (U.albedo ? U.albedo[0] : 0.0f)) * 2.0f / (3.0f * nObj);
  const float kN = (gt * wN + (U.normal ? U.normal[0] : 0.0f)) * 2.0f / (3.0f * nAll);
  const float kR = (gt * wR + (U.rough ? U.rough[0] : 0.0f)) * 2.0f / nObj;
  const float kD = (gt * wD + (U.depth ? U.depth[0] : 0.0f)) * 2.0f / nDep;
  const size_t o1 = (size_t)b * HW, o3 = (size_t)b * 3 * HW;
  for (int i = (blockIdx.x * kBThreads + threadIdx.x) * V; i < HW; i += kBSplit * kBThreads * V) {
    // term by term (no reduction ties them together): each block's loads are issued before its first use, and the live set stays
    // within the 128 registers of kBWaves
    Vec<V> sb{};
    if (G.aP || G.rP) sb = ldv<V>(P.sB, o1 + i);
    if (G.aP) {
      Vec<V> ap[3], ag[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ap[c] = ldv<V>(P.aP, o3 + (size_t)c * HW + i); ag[c] = ldv<V>(P.aG, o3 + (size_t)c * HW + i); }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Vec<V> g;
#pragma unroll
        for (int u = 0; u < V; ++u) {
          const float raw = ap[c].v[u] * cA, mB = sb.v[u];
          const float e = fminf(fmaxf(raw, 0.0f), 1.0f) - mB * ag[c].v[u];
          g.v[u] = (raw >= 0.0f && raw <= 1.0f) ? kA * e * mB * cA : 0.0f;      // the clamp passes gradient on the closed interval
        }
        stv<V>(G.aP, o3 + (size_t)c * HW + i, g);
      }
    }
    if (G.rP) {
      const Vec<V> rp = ldv<V>(P.rP, o1 + i), rg = ldv<V>(P.rG, o1 + i);
      Vec<V> g;
#pragma unroll
      for (int u = 0; u < V; ++u) g.v[u] = kR * (rp.v[u] - rg.v[u]) * sb.v[u];
      stv<V>(G.rP, o1 + i, g);
    }
    if (G.nP) {
      const Vec<V> sa = ldv<V>(P.sA, o1 + i);
      Vec<V> np[3], ng[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { np[c] = ldv<V>(P.nP, o3 + (size_t)c * HW + i); ng[c] = ldv<V>(P.nG, o3 + (size_t)c * HW + i); }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Vec<V> g;
#pragma unroll
        for (int u = 0; u < V; ++u) g.v[u] = kN * (np[c].v[u] - ng[c].v[u]) * sa.v[u];
        stv<V>(G.nP, o3 + (size_t)c * HW + i, g);
      }
    }
    if (G.dP) {
      const Vec<V> sd = ldv<V>(P.sD, o1 + i), dp = ldv<V>(P.dP, o1 + i), dg = ldv<V>(P.dG, o1 + i);
      Vec<V> g;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const float d1 = dp.v[u] * cD + off;
        g.v[u] = kD * (logf(d1) - logf(dg.v[u] + off)) * cD / d1 * sd.v[u];
      }
      stv<V>(G.dP, o1 + i, g);
    }
  }
}

// ---- the IIW ranking objective ------------------------------------------------------------------------------------------------------------
// One workgroup per image.  Forward: the judgements strided over the threads, a fixed reduction tree.  Backward: the gradient is dense and
// judgements share pixels, so the (up to 2 (Ne + Nd)) endpoint records of the image are sorted in LDS by (pixel, record index) -- a total
// order, bitonic network -- and the first record of every pixel adds that pixel's records in sorted order: no float atomics, bit-identical runs.
constexpr int kRankThreads = 1024;
constexpr int kRankCap = 4096;      // endpoint records per image (iiwDataLoader.py pads to 800 + 800 judgements: 3200)

__device__ __forceinline__ float rank_mean(const float* __restrict__ alb, int HW, int p) { return (alb[p] + alb[HW + p] + alb[2 * HW + p]) / 3.0f; }

// pixel indices of judgement i, or false when it is to be ignored (row / column outside the image: never dereferenced)
__device__ __forceinline__ bool rank_pixels(const int* __restrict__ pt, int i, int H, int W, int& p1, int& p2) {
  const int r1 = pt[4 * i], c1 = pt[4 * i + 1], r2 = pt[4 * i + 2], c2 = pt[4 * i + 3];
  if (r1 < 0 || r1 >= H || r2 < 0 || r2 >= H || c1 < 0 || c1 >= W || c2 < 0 || c2 >= W) return false;
  p1 = r1 * W + c1;
  p2 = r2 * W + c2;
  return true;
}
__device__ __forceinline__ int rank_count(const int* __restrict__ num, int b, int N) { return min(max(num[b], 0), N); }

__global__ __launch_bounds__(kRankThreads) void rank_fwd(const float* __restrict__ albedo, const int* __restrict__ eqP, const float* __restrict__ eqW,
                                                         const int* __restrict__ eqN, const int* __restrict__ dkP, const float* __restrict__ dkW,
                                                         const int* __restrict__ dkN, float* __restrict__ per_image /* [B,2] */, int H, int W, int Ne, int Nd,
                                                         float tau) {
  __shared__ float lds[2 * (kRankThreads / 64)];
  const int b = blockIdx.x, HW = H * W;
  const float* alb = albedo + (size_t)b * 3 * HW;
  const int ne = rank_count(eqN, b, Ne), nd = rank_count(dkN, b, Nd);
  float acc[2] = {0.0f, 0.0f};
  for (int i = threadIdx.x; i < ne + nd; i += kRankThreads) {
    const bool eq = i < ne;
    const int j = eq ? i : i - ne;
    int p1, p2;
    if (!rank_pixels((eq ? eqP : dkP) + (size_t)b * (eq ? Ne : Nd) * 4, j, H, W, p1, p2)) continue;
    const float w = eq ? eqW[(size_t)b * Ne + j] : dkW[(size_t)b * Nd + j];
    const float f1 = logf(rank_mean(alb, HW, p1) + 0.001f), f2 = logf(rank_mean(alb, HW, p2) + 0.001f);
    if (eq) {
      const float d = f1 - f2;
      acc[0] = fmaf(w, d * d, acc[0]);
    } else {
      const float h = fmaxf(f2 - f1 + tau, 0.0f);
      acc[1] = fmaf(w, h * h, acc[1]);
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {      // wave_sum's ladder, written out: as a call the kernel's instructions come out in another order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { lds[2 * wave] = acc[0]; lds[2 * wave + 1] = acc[1]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s0 = 0.0f, s1 = 0.0f;
    for (int v = 0; v < kRankThreads / 64; ++v) { s0 += lds[2 * v]; s1 += lds[2 * v + 1]; }
    per_image[2 * b] = ne > 0 ? s0 / (float)ne : 0.0f;           // an image without judgements contributes 0 (the reference: mean of nothing)
    per_image[2 * b + 1] = nd > 0 ? s1 / (float)nd : 0.0f;
  }
}
__global__ void rank_finish(const float* __restrict__ per_image, float* __restrict__ out2, int B) {      // wrapperIIW.py:105-109
  double s0 = 0.0, s1 = 0.0;
  for (int b = 0; b < B; ++b) { s0 += (double)per_image[2 * b]; s1 += (double)per_image[2 * b + 1]; }
  out2[0] = (float)s0 / (float)B;
  out2[1] = (float)s1 / (float)B;
}

__global__ __launch_bounds__(kRankThreads) void rank_bwd(const float* __restrict__ g_eq, const float* __restrict__ g_dk, const float* __restrict__ albedo,
                                                         const int* __restrict__ eqP, const float* __restrict__ eqW, const int* __restrict__ eqN,
                                                         const int* __restrict__ dkP, const float* __restrict__ dkW, const int* __restrict__ dkN,
                                                         float* __restrict__ g_albedo /* zero-filled */, int B, int H, int W, int Ne, int Nd, float tau, int nsort) {
  __shared__ unsigned long long keys[kRankCap];
  __shared__ float vals[kRankCap];
  const int b = blockIdx.x, HW = H * W;
  const float* alb = albedo + (size_t)b * 3 * HW;
  const int ne = rank_count(eqN, b, Ne), nd = rank_count(dkN, b, Nd);
  const float ge = (g_eq ? g_eq[0] : 0.0f) / (float)B, gd = (g_dk ? g_dk[0] : 0.0f) / (float)B;
  constexpr unsigned long long kNone = ~0ull;
  for (int i = threadIdx.x; i < nsort / 2; i += kRankThreads) {      // judgement i -> records 2i (first point), 2i + 1 (second point)
    unsigned long long k1 = kNone, k2 = kNone;
    float v = 0.0f;
    const bool eq = i < ne, live = i < ne + nd;
    const int j = eq ? i : i - ne;
    int p1, p2;
    if (live && rank_pixels((eq ? eqP : dkP) + (size_t)b * (eq ? Ne : Nd) * 4, j, H, W, p1, p2)) {
      const float w = eq ? eqW[(size_t)b * Ne + j] : dkW[(size_t)b * Nd + j];
      const float f1 = logf(rank_mean(alb, HW, p1) + 0.001f), f2 = logf(rank_mean(alb, HW, p2) + 0.001f);
      // d loss / d rho(first point); the second point receives the negative
      v = eq ? ge / (float)ne * w * 2.0f * (f1 - f2) : -(gd / (float)nd * w * 2.0f * fmaxf(f2 - f1 + tau, 0.0f));
      k1 = ((unsigned long long)p1 << 32) | (unsigned)(2 * i);
      k2 = ((unsigned long long)p2 << 32) | (unsigned)(2 * i + 1);
    }
    keys[2 * i] = k1; keys[2 * i + 1] = k2;
    vals[2 * i] = v; vals[2 * i + 1] = -v;
  }
  __syncthreads();
  for (int k = 2; k <= nsort; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < nsort; t += kRankThreads) {
        const int x = t ^ j;
        if (x > t) {
          const unsigned long long a = keys[t], c = keys[x];
          if ((a > c) == ((t & k) == 0)) { keys[t] = c; keys[x] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < nsort; t += kRankThreads) {
    const unsigned long long key = keys[t];
    if (key == kNone) continue;
    const unsigned p = (unsigned)(key >> 32);
    if (t > 0 && (unsigned)(keys[t - 1] >> 32) == p) continue;      // not the first record of its pixel
    float s = 0.0f;
    for (int u = t; u < nsort && (unsigned)(keys[u] >> 32) == p; ++u) s += vals[(unsigned)keys[u]];
    const float g = s / (3.0f * (rank_mean(alb, HW, (int)p) + 0.001f));      // d rho / d albedo_c
    float* out = g_albedo + (size_t)b * 3 * HW + p;
    out[0] = g; out[HW] = g; out[2 * HW] = g;
  }
}

static int brdf_planes_check(const BrdfPlanes& P, const char*& why) {
  if (!P.aP && !P.nP && !P.rP && !P.dP) { why = "every term is absent"; return 0; }
  if ((P.aP == nullptr) != (P.aG == nullptr) || (P.nP == nullptr) != (P.nG == nullptr) || (P.rP == nullptr) != (P.rG == nullptr) ||
      (P.dP == nullptr) != (P.dG == nullptr)) { why = "a prediction and its ground truth must be given (or left out) together"; return 0; }
  if ((P.aP || P.rP) && !P.sB) { why = "NULL seg_brdf (the albedo / roughness mask)"; return 0; }
  if ((P.nP || P.dP) && !P.sA) { why = "NULL seg_all (the normal / depth mask)"; return 0; }
  return 1;
}

}  // namespace sgr

using namespace sgr;

static BrdfPlanes brdf_planes(const float* aP, const float* aG, const float* nP, const float* nG, const float* rP, const float* rG, const float* dP, const float* dG,
                              const float* sB, const float* sA, const float* sD) {
  return BrdfPlanes{aP, aG, nP, nG, rP, rG, dP, dG, sB, sA, sD ? sD : sA};
}
// 128-bit accesses need H*W % 4 == 0 (then every plane of every image keeps its tensor's alignment) and 16-byte aligned tensors
static bool brdf_vec4(int HW, std::initializer_list<const void*> ptrs) { return HW % 4 == 0 && aligned16(ptrs); }
#define BRDF_PLANE_PTRS(P) P.aP, P.aG, P.nP, P.nG, P.rP, P.rG, P.dP, P.dG, P.sB, P.sA, P.sD
static thread_local char brdf_msg[160];
#define BRDF_CHECK_PLANES(P, who)                                   \
  do {                                                              \
    const char* why = nullptr;                                      \
    ::sgr::note_pending_error();                                    \
    if (!brdf_planes_check(P, why)) {                               \
      snprintf(brdf_msg, sizeof brdf_msg, who ": %s", why);         \
      ::sgr::set_error(brdf_msg);                                   \
      return SGR_ERR_BAD_ARG;                                       \
    }                                                               \
  } while (0)

extern "C" int sgr_brdf_objective_workspace_floats(int bn) { return bn > 0 ? bn * kBSplit * (kNA + kNB) : 0; }

extern "C" int sgr_brdf_objective_fwd(const float* albedo_pred, const float* albedo, const float* normal_pred, const float* normal, const float* rough_pred,
                                      const float* rough, const float* depth_pred, const float* depth, const float* seg_brdf, const float* seg_all,
                                      const float* seg_depth, float* coef, float* parts, float* values, float* workspace, int bn, int H, int W, float w_albedo,
                                      float w_normal, float w_rough, float w_depth, float depth_offset, void* stream) {
  const BrdfPlanes P = brdf_planes(albedo_pred, albedo, normal_pred, normal, rough_pred, rough, depth_pred, depth, seg_brdf, seg_all, seg_depth);
  BRDF_CHECK_PLANES(P, "sgr_brdf_objective_fwd");
  SGR_REQUIRE(coef && parts && workspace, "sgr_brdf_objective_fwd: NULL output or workspace");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 30) && bn <= 65535, "sgr_brdf_objective_fwd: size out of range");
  SGR_REQUIRE(depth_offset > 0.0f, "sgr_brdf_objective_fwd: depth_offset must be positive");
  const hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  float* wsA = workspace;
  float* wsB = wsA + (size_t)bn * kBSplit * kNA;
  const dim3 grid(kBSplit, bn), block(kBThreads);
  if (brdf_vec4(HW, {BRDF_PLANE_PTRS(P)})) {
    hipLaunchKernelGGL(brdf_pass_a<4>, grid, block, 0, st, P, wsA, HW);
    hipLaunchKernelGGL(brdf_pass_b<4>, grid, block, 0, st, P, wsA, wsB, coef, HW, depth_offset);
  } else {
    hipLaunchKernelGGL(brdf_pass_a<1>, grid, block, 0, st, P, wsA, HW);
    hipLaunchKernelGGL(brdf_pass_b<1>, grid, block, 0, st, P, wsA, wsB, coef, HW, depth_offset);
  }
  hipLaunchKernelGGL(brdf_totals, dim3(1), block, 0, st, wsA, wsB, bn * kBSplit, parts, values, w_albedo, w_normal, w_rough, w_depth);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_objective_fwd");
}

extern "C" int sgr_brdf_objective_finalize(const float* parts, float* values, float w_albedo, float w_normal, float w_rough, float w_depth, void* stream) {
  SGR_REQUIRE(parts && values, "sgr_brdf_objective_finalize: NULL tensor");
  hipLaunchKernelGGL(brdf_finalize, dim3(1), dim3(1), 0, (hipStream_t)stream, parts, values, w_albedo, w_normal, w_rough, w_depth);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_objective_finalize");
}

extern "C" int sgr_brdf_objective_bwd(const float* g_total, const float* g_albedo_err, const float* g_normal_err, const float* g_rough_err,
                                      const float* g_depth_err, const float* albedo_pred, const float* albedo, const float* normal_pred, const float* normal,
                                      const float* rough_pred, const float* rough, const float* depth_pred, const float* depth, const float* seg_brdf,
                                      const float* seg_all, const float* seg_depth, const float* coef, const float* parts, float* g_albedo_pred,
                                      float* g_normal_pred, float* g_rough_pred, float* g_depth_pred, int bn, int H, int W, float w_albedo, float w_normal,
                                      float w_rough, float w_depth, float depth_offset, void* stream) {
  const BrdfPlanes P = brdf_planes(albedo_pred, albedo, normal_pred, normal, rough_pred, rough, depth_pred, depth, seg_brdf, seg_all, seg_depth);
  BRDF_CHECK_PLANES(P, "sgr_brdf_objective_bwd");
  SGR_REQUIRE(coef && parts, "sgr_brdf_objective_bwd: NULL coef / parts");
  SGR_REQUIRE(g_albedo_pred || g_normal_pred || g_rough_pred || g_depth_pred, "sgr_brdf_objective_bwd: no gradient requested");
  SGR_REQUIRE((!g_albedo_pred || albedo_pred) && (!g_normal_pred || normal_pred) && (!g_rough_pred || rough_pred) && (!g_depth_pred || depth_pred),
              "sgr_brdf_objective_bwd: gradient requested for an absent term");
  SGR_REQUIRE(bn > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 30) && bn <= 65535, "sgr_brdf_objective_bwd: size out of range");
  SGR_REQUIRE(depth_offset > 0.0f, "sgr_brdf_objective_bwd: depth_offset must be positive");
  const BrdfUpstream U{g_total, g_albedo_err, g_normal_err, g_rough_err, g_depth_err};
  const BrdfGrads G{g_albedo_pred, g_normal_pred, g_rough_pred, g_depth_pred};
  const int HW = H * W;
  const dim3 grid(kBSplit, bn), block(kBThreads);
  if (brdf_vec4(HW, {BRDF_PLANE_PTRS(P), G.aP, G.nP, G.rP, G.dP}))
    hipLaunchKernelGGL(brdf_bwd<4>, grid, block, 0, (hipStream_t)stream, P, U, G, coef, parts, HW, w_albedo, w_normal, w_rough, w_depth, depth_offset);
  else
    hipLaunchKernelGGL(brdf_bwd<1>, grid, block, 0, (hipStream_t)stream, P, U, G, coef, parts, HW, w_albedo, w_normal, w_rough, w_depth, depth_offset);
  return sgr_check((int)hipGetLastError(), "sgr_brdf_objective_bwd");
}

extern "C" int sgr_ranking_loss_workspace_floats(int B) { return B > 0 ? 2 * B : 0; }

#define RANK_REQUIRE(who)                                                                                                                       \
  SGR_REQUIRE(albedo_pred && eq_point && eq_weight && eq_num && darker_point && darker_weight && darker_num, who ": NULL tensor");              \
  SGR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 30) && n_eq >= 0 && n_darker >= 0, who ": size out of range"); \
  SGR_SUPPORTED(2 * (n_eq + n_darker) <= kRankCap, who ": more than 2048 judgements per image (equal + darker, padded)")

extern "C" int sgr_ranking_loss_fwd(const float* albedo_pred, const int* eq_point, const float* eq_weight, const int* eq_num, const int* darker_point,
                                    const float* darker_weight, const int* darker_num, float* out2, float* workspace, int B, int H, int W, int n_eq,
                                    int n_darker, float tau, void* stream) {
  RANK_REQUIRE("sgr_ranking_loss_fwd");
  SGR_REQUIRE(out2 && workspace, "sgr_ranking_loss_fwd: NULL output or workspace");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rank_fwd, dim3(B), dim3(kRankThreads), 0, st, albedo_pred, eq_point, eq_weight, eq_num, darker_point, darker_weight, darker_num, workspace, H, W,
                     n_eq, n_darker, tau);
  hipLaunchKernelGGL(rank_finish, dim3(1), dim3(1), 0, st, workspace, out2, B);
  return sgr_check((int)hipGetLastError(), "sgr_ranking_loss_fwd");
}

extern "C" int sgr_ranking_loss_bwd(const float* g_eq, const float* g_darker, const float* albedo_pred, const int* eq_point, const float* eq_weight,
                                    const int* eq_num, const int* darker_point, const float* darker_weight, const int* darker_num, float* g_albedo_pred, int B,
                                    int H, int W, int n_eq, int n_darker, float tau, void* stream) {
  RANK_REQUIRE("sgr_ranking_loss_bwd");
  SGR_REQUIRE(g_albedo_pred, "sgr_ranking_loss_bwd: NULL output");
  const hipStream_t st = (hipStream_t)stream;
  int nsort = 2;
  while (nsort < 2 * (n_eq + n_darker)) nsort <<= 1;      // <= kRankCap
  int rc = (int)hipMemsetAsync(g_albedo_pred, 0, (size_t)B * 3 * H * W * sizeof(float), st);
  if (rc != 0) return sgr_check(rc, "sgr_ranking_loss_bwd");
  hipLaunchKernelGGL(rank_bwd, dim3(B), dim3(kRankThreads), 0, st, g_eq, g_darker, albedo_pred, eq_point, eq_weight, eq_num, darker_point, darker_weight, darker_num,
                     g_albedo_pred, B, H, W, n_eq, n_darker, tau, nsort);
  return sgr_check((int)hipGetLastError(), "sgr_ranking_loss_bwd");
}
