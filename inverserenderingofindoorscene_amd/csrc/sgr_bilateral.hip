// The bilateral solver layer (BilateralLayer.py / BilateralGrid.py of the reference) on gfx950.
//
//   grid ............... BilateralGrid.__init__ / _compute_factorization      BilateralGrid.py:43-83
//   bistochastisation .. bistochastize                                        BilateralGrid.py:106-118
//   forward solve ...... BilateralSolver.solve   (scipy cg written out)       BilateralGrid.py:126-153
//   backward solve ..... BilateralSolver.solveGrad                            BilateralGrid.py:155-191
//
// The reference builds the grid with numpy and solves it with scipy's sparse CG on the host, per image, in fp64, in forward and again
// in backward.  Here the whole batch is one set of launches on the caller's stream with static shapes: nvertices <= H*W, so image b
// owns the slots [b*N, (b+1)*N) (N = H*W) of every per-vertex array and its vertex count stays on the device (nvert[b]).  Nothing is
// read back: the PCG's scalars (rho, alpha, beta, |b|, the per-(image, channel) "stopped" flag) live on the device, all cg_maxiter
// iterations are enqueued, and a stopped system's updates are masked.
//
// Deterministic and batch-invariant: the splat is a segmented sum over the pixels sorted by vertex (ascending pixel index inside a
// vertex: the sort is stable), never a floating-point atomic; every dot product is bs_split(N) block partials per image -- a function of
// the image size alone -- folded in a fixed order by each consumer block's prologue (the scheme of sgr_loss.hip).  An image of a batch
// therefore gives bit for bit what it gives alone.
//
// Vertex vectors are fp64, [vertex][C]: parity with the reference's fp64 solve is then limited by summation order alone, and a constant
// target channel -- where lam (m y - n blur(n y)) cancels to rounding -- stops at iteration 0 as it does in the reference instead of
// iterating on fp32 noise.
//
// PCG iteration = three launches:  bs_p (fold r.z, r.r -> stop test, beta; p = z + beta p; np = n p)
//                                  bs_stencil (q = A p, gathers np of 10 neighbours for C channels; p.q partials)
//                                  bs_update (fold p.q -> alpha; y += alpha p; r -= alpha q; z = M r; r.z, r.r partials)
#include "sgr_launch.h"

namespace sgr {

constexpr int kBsThreads = 256;
constexpr int kBsMaxSplit = 1024;             // blocks per image of the reducing kernels
constexpr int kBsChunk = 1024;                // sorted positions per block of the vertex-numbering scan (4 per thread)
constexpr int kBsMaxIter = 64;                // cg_maxiter bound (sizes the per-iteration scalars)
constexpr int kBsNbr = 10;
constexpr long long kBsImgStride = 1LL << 44; // key = image * 2^44 + hash + 2^43: one sort serves the batch
constexpr long long kBsHashBias = 1LL << 43;
constexpr double kBsColourClamp = 1024.0;     // |colour coordinate| bound (255.5 / sigma with sigma >= 0.25): 1024 * 255^4 < 2^43
constexpr double kBsSpatialClamp = 1048576.0;

static inline int bs_split(int N) {
  const int s = (N + kBsThreads - 1) / kBsThreads;
  return s < kBsMaxSplit ? s : kBsMaxSplit;
}
static inline int bs_chunks(int N) { return (N + kBsChunk - 1) / kBsChunk; }
static inline size_t bs_align(size_t n) { return (n + 15) / 16 * 16; }

// a product rounded on its own, never contracted into a fused multiply-add with a neighbouring sum: the build contracts globally
// (-ffp-contract=fast, where neither a contract pragma nor HIP's __dmul_rn -- a plain multiplication -- holds it back), so the product
// passes through an empty asm statement the optimiser cannot see through
__device__ __forceinline__ double bs_mul(double a, double b) {
  double x = a * b;
  asm volatile("" : "+v"(x));
  return x;
}

// reductions: butterfly inside a wave, four wave sums through LDS, added in a fixed order; every thread gets the result
template <int N>
__device__ __forceinline__ void bs_block_sum(double (&v)[N], double* lds /* [4*N] */) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (lds[i] + lds[N + i]) + (lds[2 * N + i] + lds[3 * N + i]);
}

// fold the S block partials ([S][STRIDE], the first N of each) of one image
template <int N, int STRIDE>
__device__ __forceinline__ void bs_fold(const double* __restrict__ part, int S, double (&out)[N], double* lds) {
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = 0.0;
  for (int j = threadIdx.x; j < S; j += kBsThreads)
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] += part[(size_t)j * STRIDE + i];
  bs_block_sum<N>(out, lds);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// grid build
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long bs_trunc(double v, double bound) {
  v = v < bound ? v : bound;          // NaN -> bound
  v = v > -bound ? v : -bound;
  return (long long)v;                // truncation toward zero, numpy's astype(int)
}

// BilateralGrid.py:12-26,43-60: im255 = image * 255 in fp32, everything after in fp64; IEEE divisions (7 / 7 must be exactly 1)
__global__ __launch_bounds__(kBsThreads) void bs_keys(const float* __restrict__ image /* [B,3,H,W] */, long long* __restrict__ keys,
                                                       int B, int H, int W, double sl, double sc, double ss) {
  const int N = H * W;
  const long long g = (long long)blockIdx.x * kBsThreads + threadIdx.x;
  if (g >= (long long)B * N) return;
  const int b = (int)(g / N), p = (int)(g - (long long)b * N);
  const int y = p / W, x = p - y * W;
  const float* im = image + (size_t)b * 3 * N;
  const double r = (double)(im[p] * 255.0f), gr = (double)(im[N + p] * 255.0f), bl = (double)(im[2 * (size_t)N + p] * 255.0f);
  const double Y = (0.299 * r + 0.587 * gr) + 0.114 * bl;
  const double U = ((-0.168736 * r + -0.331264 * gr) + 0.5 * bl) + 128.0;
  const double V = ((0.5 * r + -0.418688 * gr) + -0.081312 * bl) + 128.0;
  const long long c0 = bs_trunc((double)x / ss, kBsSpatialClamp), c1 = bs_trunc((double)y / ss, kBsSpatialClamp);
  const long long c2 = bs_trunc(Y / sl, kBsColourClamp), c3 = bs_trunc(U / sc, kBsColourClamp), c4 = bs_trunc(V / sc, kBsColourClamp);
  long long h = c0 + 255LL * (c1 + 255LL * (c2 + 255LL * (c3 + 255LL * c4)));
  h = h < kBsHashBias - 1 ? h : kBsHashBias - 1;
  h = h > -kBsHashBias ? h : -kBsHashBias;
  keys[g] = (long long)b * kBsImgStride + (h + kBsHashBias);
}

__device__ __forceinline__ int bs_flag(const long long* __restrict__ k, int i) { return i == 0 || k[i] != k[i - 1]; }

// vertices = distinct keys in ascending order: count the segment heads per chunk of sorted positions ...
__global__ __launch_bounds__(kBsThreads) void bs_scan_count(const long long* __restrict__ keys, int* __restrict__ chunkcnt, int N, int nchunk) {
  __shared__ int lds[4];
  const int b = blockIdx.y;
  const long long* k = keys + (size_t)b * N;
  const int base = blockIdx.x * kBsChunk + threadIdx.x * 4;
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (base + j < N) c += bs_flag(k, base + j);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunkcnt[b * nchunk + blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
// ... exclusive scan of the chunk counts of each image (a few hundred values: one thread), nvert[b] ...
__global__ void bs_scan_chunks(int* __restrict__ chunkcnt, int* __restrict__ nvert, int nchunk) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  int run = 0;
  for (int j = 0; j < nchunk; ++j) {
    const int c = chunkcnt[b * nchunk + j];
    chunkcnt[b * nchunk + j] = run;
    run += c;
  }
  nvert[b] = run;
}
// ... and number them: pixel -> vertex, vertex -> first sorted position, vertex -> key; the sort's index becomes the per-image permutation
__global__ __launch_bounds__(kBsThreads) void bs_scan_assign(const long long* __restrict__ keys, const long long* __restrict__ index,
                                                              const int* __restrict__ chunkoff, int* __restrict__ pix2vert, int* __restrict__ perm,
                                                              int* __restrict__ seg, long long* __restrict__ vkey, int N, int nchunk) {
  __shared__ int lds[kBsThreads];
  const int b = blockIdx.y;
  const size_t o = (size_t)b * N;
  const long long* k = keys + o;
  const int base = blockIdx.x * kBsChunk + threadIdx.x * 4;
  int f[4], c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = base + j < N ? bs_flag(k, base + j) : 0;
    c += f[j];
  }
  lds[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < kBsThreads; off <<= 1) {      // inclusive Hillis-Steele scan of the 256 thread counts
    const int add = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
    __syncthreads();
    lds[threadIdx.x] += add;
    __syncthreads();
  }
  int run = chunkoff[b * nchunk + blockIdx.x] + lds[threadIdx.x] - c;    // heads before this thread's first position
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = base + j;
    if (i < N) {
      run += f[j];
      const int v = run - 1;
      long long pl = index[o + i] - (long long)o;
      pl = pl < 0 ? 0 : (pl >= N ? N - 1 : pl);          // a well-formed sort index is in range; never write outside the image
      const int p = (int)pl;
      perm[o + i] = p;
      pix2vert[o + p] = v;
      if (f[j]) {
        seg[o + v] = i;
        vkey[o + v] = k[i];
      }
    }
  }
}

// BilateralGrid.py:66-83: the neighbour of a vertex along +-d is the vertex whose hash is the hash of its coordinates +- 1 in d.  The hash is
// linear in the coordinates, so that is the vertex's own hash +- 255^d whichever of its pixels supplies the coordinates (with colliding
// hashes too: np.unique's lowest-index pixel hashes to the same value as every other pixel of the vertex).  Binary search in the image's keys.
__global__ __launch_bounds__(kBsThreads) void bs_neighbours(const long long* __restrict__ vkey, const int* __restrict__ nvert, int* __restrict__ nbr, int N) {
  const int b = blockIdx.y, nv = nvert[b];
  const int v = blockIdx.x * kBsThreads + threadIdx.x;
  if (v >= nv) return;
  const long long* k = vkey + (size_t)b * N;
  const long long key = k[v];
  int* out = nbr + ((size_t)b * N + v) * kBsNbr;
  long long step = 1;
#pragma unroll
  for (int d = 0; d < 5; ++d) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const long long want = key + (s ? step : -step);
      int lo = 0, hi = nv;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k[mid] < want) lo = mid + 1; else hi = mid;
      }
      out[2 * d + s] = (lo < nv && k[lo] == want) ? lo : -1;
    }
    step *= 255;
  }
}

__device__ __forceinline__ int bs_seg_end(const int* __restrict__ seg, int v, int nv, int N) { return v + 1 < nv ? seg[v + 1] : N; }

// BilateralGrid.py:106-118: one sweep n <- sqrt(n m / blur(n)) (first: n = 1), or the closing m <- n blur(n)
template <int MODE /* 0 first sweep, 1 sweep, 2 final m */>
__global__ __launch_bounds__(kBsThreads) void bs_bistoch(const int* __restrict__ seg, const int* __restrict__ nbr, const int* __restrict__ nvert,
                                                          const double* __restrict__ n_in, double* __restrict__ out, int N) {
  const int b = blockIdx.y, nv = nvert[b];
  const int v = blockIdx.x * kBsThreads + threadIdx.x;
  if (v >= nv) return;
  const size_t o = (size_t)b * N;
  const int* nb = nbr + (o + v) * kBsNbr;
  const double nvv = MODE == 0 ? 1.0 : n_in[o + v];
  double blur = bs_mul(10.0, nvv);      // products rounded on their own (no contraction): see the diagonal in bs_splat_init
#pragma unroll
  for (int k = 0; k < kBsNbr; ++k) {
    const int u = nb[k];
    if (u >= 0) blur += MODE == 0 ? 1.0 : n_in[o + u];
  }
  if (MODE == 2) {
    out[o + v] = bs_mul(nvv, blur);
  } else {
    const double m0 = (double)(bs_seg_end(seg + o, v, nv, N) - seg[o + v]);
    out[o + v] = sqrt(nvv * m0 / blur);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// solve
// ---------------------------------------------------------------------------------------------------------------------------------
struct BsGrid {
  const int* pix2vert; const int* perm; const int* seg; const int* nbr; const int* nvert; const double* m; const double* n;
};
struct BsWork {
  double *r, *z, *p, *np, *q, *dA, *minv, *part_r /* [B][S][3C]: r.z, r.r, b.b */, *part_q /* [B][S][C] */, *rho /* [iter][B][C] */, *atol /* [B][C] */;
  int* stopped /* [iter][B][C] */;
};

// splat of the right-hand side and the weights, the diagonal, the preconditioner and the start vector (BilateralGrid.py:133-146 / :162-173)
template <int C, bool BWD>
__global__ __launch_bounds__(kBsThreads) void bs_splat_init(BsGrid g, BsWork w, const float* __restrict__ x /* pred | g_out [B,C,H,W] */,
                                                            const float* __restrict__ conf /* [B,H,W] */, double* __restrict__ y, int N, double lam,
                                                            double amin) {
  const int b = blockIdx.y, nv = g.nvert[b];
  const int v = blockIdx.x * kBsThreads + threadIdx.x;
  if (v >= nv) return;
  const size_t o = (size_t)b * N;
  const int s0 = g.seg[o + v], s1 = bs_seg_end(g.seg + o, v, nv, N);
  double ws = 0.0, bs[C];
#pragma unroll
  for (int c = 0; c < C; ++c) bs[c] = 0.0;
  for (int i = s0; i < s1; ++i) {
    const int p = g.perm[o + i];
    const double cw = (double)conf[o + p];
    ws += cw;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double xv = (double)x[((size_t)b * C + c) * N + p];
      bs[c] += BWD ? xv : xv * cw;
    }
  }
  const double m = g.m[o + v], n = g.n[o + v];
  // the reference forms A as a matrix: its diagonal is this one number.  Separately rounded products, as numpy evaluates them: on a vertex
  // without neighbours m = n (10 n) and the difference is EXACTLY zero there; a fused multiply-add would leave the product's rounding
  // residue instead, and with zero confidence that residue times 1 / A_diag_min is what the PCG would then iterate on
  const double diag = bs_mul(lam, m - bs_mul(bs_mul(10.0, n), n)) + ws;
  w.dA[o + v] = diag;
  w.minv[o + v] = 1.0 / (diag > amin ? diag : amin);
  const double den = BWD ? (double)(s1 - s0) : (ws > 1e-10 ? ws : 1e-10);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double y0 = bs[c] / den;
    y[(o + v) * C + c] = y0;
    w.r[(o + v) * C + c] = bs[c];
    w.np[(o + v) * C + c] = n * y0;
  }
}

// (A x)_v = (lam (m_v - 10 n_v^2) + ws_v) x_v - lam n_v sum over neighbours (n x)_u -- the matrix as the reference forms it; applying
// lam (m x - n blur(n x)) term by term leaves another rounding residue where m = 10 n^2 (no neighbours), which 1 / A_diag_min amplifies
template <int C>
__device__ __forceinline__ void bs_apply(const BsGrid& g, const BsWork& w, const double* __restrict__ x, size_t o, int v, double lam, double (&out)[C]) {
  const int* nb = g.nbr + (o + v) * kBsNbr;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
  for (int k = 0; k < kBsNbr; ++k) {
    const int u = nb[k];
    if (u >= 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += w.np[(o + u) * C + c];
    }
  }
  const double dA = w.dA[o + v], ln = lam * g.n[o + v];
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = dA * x[(o + v) * C + c] - ln * acc[c];
}

// r = b - A y0, z = M r; partials of r.z, r.r, b.b
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_init_residual(BsGrid g, BsWork w, const double* __restrict__ y, int N, int S, double lam) {
  __shared__ double lds[4 * 3 * C];
  const int b = blockIdx.y, nv = g.nvert[b];
  const size_t o = (size_t)b * N;
  double acc[3 * C];
#pragma unroll
  for (int i = 0; i < 3 * C; ++i) acc[i] = 0.0;
  for (int v = blockIdx.x * kBsThreads + threadIdx.x; v < nv; v += S * kBsThreads) {
    double ay[C];
    bs_apply<C>(g, w, y, o, v, lam, ay);
    const double mi = w.minv[o + v];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double bv = w.r[(o + v) * C + c], r = bv - ay[c], z = mi * r;
      w.r[(o + v) * C + c] = r;
      w.z[(o + v) * C + c] = z;
      acc[c] += r * z; acc[C + c] += r * r; acc[2 * C + c] += bv * bv;
    }
  }
  bs_block_sum<3 * C>(acc, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 3 * C; ++i) w.part_r[((size_t)b * S + blockIdx.x) * 3 * C + i] = acc[i];
}

// top of iteration `it` (scipy cg): stop test |r| < cg_tol |b| (sticky; |b| = 0 stops before the first iteration and returns b = y0),
// rho = r.z, beta = rho / rho_prev, p = z + beta p, np = n p
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_p(BsGrid g, BsWork w, int N, int S, int B, int it, double tol) {
  __shared__ double lds[4 * 3 * C];
  const int b = blockIdx.y, nv = g.nvert[b];
  const size_t o = (size_t)b * N;
  double f[3 * C];
  bs_fold<3 * C, 3 * C>(w.part_r + (size_t)b * S * 3 * C, S, f, lds);
  double beta[C];
  bool stop[C], all = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double atol = it == 0 ? tol * sqrt(f[2 * C + c]) : w.atol[b * C + c];
    const bool prev = it == 0 ? f[2 * C + c] == 0.0 : w.stopped[((size_t)(it - 1) * B + b) * C + c] != 0;
    stop[c] = prev || sqrt(f[C + c]) < atol;
    beta[c] = it == 0 ? 0.0 : f[c] / w.rho[((size_t)(it - 1) * B + b) * C + c];
    all = all && stop[c];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (it == 0) w.atol[b * C + c] = atol;
      w.rho[((size_t)it * B + b) * C + c] = f[c];
      w.stopped[((size_t)it * B + b) * C + c] = stop[c] ? 1 : 0;
    }
  }
  if (all) return;
  for (int v = blockIdx.x * kBsThreads + threadIdx.x; v < nv; v += S * kBsThreads) {
    const double n = g.n[o + v];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (stop[c]) continue;
      const size_t i = (o + v) * C + c;
      const double p = it == 0 ? w.z[i] : w.z[i] + beta[c] * w.p[i];
      w.p[i] = p;
      w.np[i] = n * p;
    }
  }
}

// q = A p and the p.q partials
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_stencil(BsGrid g, BsWork w, int N, int S, int B, int it, double lam) {
  __shared__ double lds[4 * C];
  const int b = blockIdx.y, nv = g.nvert[b];
  const size_t o = (size_t)b * N;
  bool all = true;
#pragma unroll
  for (int c = 0; c < C; ++c) all = all && w.stopped[((size_t)it * B + b) * C + c] != 0;
  if (all) return;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
  for (int v = blockIdx.x * kBsThreads + threadIdx.x; v < nv; v += S * kBsThreads) {
    double q[C];
    bs_apply<C>(g, w, w.p, o, v, lam, q);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      w.q[(o + v) * C + c] = q[c];
      acc[c] += w.p[(o + v) * C + c] * q[c];
    }
  }
  bs_block_sum<C>(acc, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < C; ++c) w.part_q[((size_t)b * S + blockIdx.x) * C + c] = acc[c];
}

// alpha = rho / p.q; y += alpha p; r -= alpha q; z = M r; partials of r.z, r.r.  A stopped channel is left untouched.
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_update(BsGrid g, BsWork w, double* __restrict__ y, int N, int S, int B, int it) {
  __shared__ double lds[4 * 2 * C];
  const int b = blockIdx.y, nv = g.nvert[b];
  const size_t o = (size_t)b * N;
  bool stop[C], all = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    stop[c] = w.stopped[((size_t)it * B + b) * C + c] != 0;
    all = all && stop[c];
  }
  if (all) return;
  double pq[C], alpha[C];
  bs_fold<C, C>(w.part_q + (size_t)b * S * C, S, pq, lds);
#pragma unroll
  for (int c = 0; c < C; ++c) alpha[c] = w.rho[((size_t)it * B + b) * C + c] / pq[c];
  double acc[2 * C];
#pragma unroll
  for (int i = 0; i < 2 * C; ++i) acc[i] = 0.0;
  for (int v = blockIdx.x * kBsThreads + threadIdx.x; v < nv; v += S * kBsThreads) {
    const double mi = w.minv[o + v];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (stop[c]) continue;
      const size_t i = (o + v) * C + c;
      y[i] += alpha[c] * w.p[i];
      const double r = w.r[i] - alpha[c] * w.q[i], z = mi * r;
      w.r[i] = r;
      w.z[i] = z;
      acc[c] += r * z; acc[C + c] += r * r;
    }
  }
  bs_block_sum<2 * C>(acc, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (stop[c]) continue;          // a stopped channel's partials are never used again (the flag is sticky)
      w.part_r[((size_t)b * S + blockIdx.x) * 3 * C + c] = acc[c];
      w.part_r[((size_t)b * S + blockIdx.x) * 3 * C + C + c] = acc[C + c];
    }
}

// output = slice(yhat) as fp32
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_slice_fwd(const int* __restrict__ pix2vert, const double* __restrict__ y, float* __restrict__ out, int N) {
  const int b = blockIdx.y, p = blockIdx.x * kBsThreads + threadIdx.x;
  if (p >= N) return;
  const size_t o = (size_t)b * N;
  const int v = pix2vert[o + p];
#pragma unroll
  for (int c = 0; c < C; ++c) out[((size_t)b * C + c) * N + p] = (float)y[(o + v) * C + c];
}

// grad_pred = slice(yb) w;  grad_conf = sum_c slice(-yb yhat) + slice(yb) t          (BilateralGrid.py:177-190, :219-222)
template <int C>
__global__ __launch_bounds__(kBsThreads) void bs_slice_bwd(const int* __restrict__ pix2vert, const double* __restrict__ yb, const double* __restrict__ yhat,
                                                            const float* __restrict__ pred, const float* __restrict__ conf, float* __restrict__ g_pred,
                                                            float* __restrict__ g_conf, int N) {
  const int b = blockIdx.y, p = blockIdx.x * kBsThreads + threadIdx.x;
  if (p >= N) return;
  const size_t o = (size_t)b * N;
  const int v = pix2vert[o + p];
  const double cw = (double)conf[o + p];
  double gc = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = yb[(o + v) * C + c];
    g_pred[((size_t)b * C + c) * N + p] = (float)(s * cw);
    gc += -1.0 * (s * yhat[(o + v) * C + c]) + s * (double)pred[((size_t)b * C + c) * N + p];
  }
  g_conf[o + p] = (float)gc;
}

// workspace layouts --------------------------------------------------------------------------------------------------------------
struct BsBuildWs { long long* vkey; double* n_tmp; int* chunk; };
static size_t bs_build_ws(char* base, int B, int N, BsBuildWs* out) {
  const size_t P = (size_t)B * N;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += bs_align(bytes); return p; };
  BsBuildWs w;
  w.vkey = (long long*)take(P * sizeof(long long));
  w.n_tmp = (double*)take(P * sizeof(double));
  w.chunk = (int*)take((size_t)B * bs_chunks(N) * sizeof(int));
  if (out) *out = w;
  return off;
}
static size_t bs_solve_ws(char* base, int B, int N, int C, BsWork* out, double** y_bwd) {
  const size_t P = (size_t)B * N, S = (size_t)bs_split(N);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += bs_align(bytes); return p; };
  BsWork w;
  w.r = (double*)take(P * C * sizeof(double));
  w.z = (double*)take(P * C * sizeof(double));
  w.p = (double*)take(P * C * sizeof(double));
  w.np = (double*)take(P * C * sizeof(double));
  w.q = (double*)take(P * C * sizeof(double));
  double* yb = (double*)take(P * C * sizeof(double));
  w.dA = (double*)take(P * sizeof(double));
  w.minv = (double*)take(P * sizeof(double));
  w.part_r = (double*)take((size_t)B * S * 3 * C * sizeof(double));
  w.part_q = (double*)take((size_t)B * S * C * sizeof(double));
  w.rho = (double*)take((size_t)kBsMaxIter * B * C * sizeof(double));
  w.atol = (double*)take((size_t)B * C * sizeof(double));
  w.stopped = (int*)take((size_t)kBsMaxIter * B * C * sizeof(int));
  if (out) *out = w;
  if (y_bwd) *y_bwd = yb;
  return off;
}

static bool bs_shape_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 26) && (long long)B * H * W <= (1LL << 28) && B < (1 << 18);
}

template <int C, bool BWD>
static int bs_pcg(const BsGrid& g, const BsWork& w, const float* x, const float* conf, double* y, int B, int N, double lam, double amin, double tol,
                  int maxiter, hipStream_t st) {
  const int S = bs_split(N);
  const dim3 gv((N + kBsThreads - 1) / kBsThreads, B), gs(S, B);
  hipLaunchKernelGGL((bs_splat_init<C, BWD>), gv, dim3(kBsThreads), 0, st, g, w, x, conf, y, N, lam, amin);
  hipLaunchKernelGGL((bs_init_residual<C>), gs, dim3(kBsThreads), 0, st, g, w, (const double*)y, N, S, lam);
  for (int it = 0; it < maxiter; ++it) {
    hipLaunchKernelGGL((bs_p<C>), gs, dim3(kBsThreads), 0, st, g, w, N, S, B, it, tol);
    hipLaunchKernelGGL((bs_stencil<C>), gs, dim3(kBsThreads), 0, st, g, w, N, S, B, it, lam);
    hipLaunchKernelGGL((bs_update<C>), gs, dim3(kBsThreads), 0, st, g, w, y, N, S, B, it);
  }
  return (int)hipGetLastError();
}

}  // namespace sgr

using namespace sgr;

extern "C" long long sgr_bs_workspace_bytes(int B, int H, int W, int C) {
  SGR_REQUIRE(bs_shape_ok(B, H, W) && C >= 1 && C <= 3, "sgr_bs_workspace_bytes: bad argument (B, H, W > 0, B*H*W <= 2^28, C in 1..3)");
  const size_t a = bs_build_ws(nullptr, B, H * W, nullptr), s = bs_solve_ws(nullptr, B, H * W, C, nullptr, nullptr);
  return (long long)(a > s ? a : s);
}

extern "C" int sgr_bs_grid_keys(const float* image, long long* keys, int B, int H, int W, double sigma_luma, double sigma_chroma,
                                double sigma_spatial, void* stream) {
  SGR_REQUIRE(image && keys, "sgr_bs_grid_keys: NULL tensor");
  SGR_REQUIRE(bs_shape_ok(B, H, W), "sgr_bs_grid_keys: bad shape (B, H, W > 0, B*H*W <= 2^28)");
  SGR_REQUIRE(sigma_luma > 0 && sigma_chroma > 0 && sigma_spatial > 0, "sgr_bs_grid_keys: the bandwidths (sigma) must be positive");
  SGR_SUPPORTED(sigma_luma >= 0.25 && sigma_chroma >= 0.25, "sgr_bs_grid_keys: colour bandwidths (sigma) below 0.25 overflow the 5-D hash");
  const long long P = (long long)B * H * W;
  hipLaunchKernelGGL(bs_keys, dim3((unsigned)((P + kBsThreads - 1) / kBsThreads)), dim3(kBsThreads), 0, (hipStream_t)stream, image, keys, B, H, W,
                     sigma_luma, sigma_chroma, sigma_spatial);
  return sgr_check((int)hipGetLastError(), "sgr_bs_grid_keys");
}

extern "C" int sgr_bs_grid_build(const long long* sorted_keys, const long long* sorted_index, int* pix2vert, int* perm, int* seg, int* nbr,
                                 int* nvert, double* m, double* n, void* workspace, int B, int H, int W, void* stream) {
  SGR_REQUIRE(sorted_keys && sorted_index && pix2vert && perm && seg && nbr && nvert && m && n && workspace, "sgr_bs_grid_build: NULL tensor");
  SGR_REQUIRE(bs_shape_ok(B, H, W), "sgr_bs_grid_build: bad shape (B, H, W > 0, B*H*W <= 2^28)");
  const int N = H * W, nchunk = bs_chunks(N);
  hipStream_t st = (hipStream_t)stream;
  BsBuildWs w;
  bs_build_ws((char*)workspace, B, N, &w);
  const dim3 gc(nchunk, B), gv((N + kBsThreads - 1) / kBsThreads, B), th(kBsThreads);
  hipLaunchKernelGGL(bs_scan_count, gc, th, 0, st, sorted_keys, w.chunk, N, nchunk);
  hipLaunchKernelGGL(bs_scan_chunks, dim3(B), dim3(64), 0, st, w.chunk, nvert, nchunk);
  hipLaunchKernelGGL(bs_scan_assign, gc, th, 0, st, sorted_keys, sorted_index, (const int*)w.chunk, pix2vert, perm, seg, w.vkey, N, nchunk);
  hipLaunchKernelGGL(bs_neighbours, gv, th, 0, st, (const long long*)w.vkey, (const int*)nvert, nbr, N);
  // ten sweeps, ping-pong between the workspace and the output: the tenth lands in `n`
  hipLaunchKernelGGL(bs_bistoch<0>, gv, th, 0, st, (const int*)seg, (const int*)nbr, (const int*)nvert, (const double*)nullptr, w.n_tmp, N);
  for (int k = 2; k <= 10; ++k) {
    const double* src = (k & 1) ? n : w.n_tmp;
    double* dst = (k & 1) ? w.n_tmp : n;
    hipLaunchKernelGGL(bs_bistoch<1>, gv, th, 0, st, (const int*)seg, (const int*)nbr, (const int*)nvert, src, dst, N);
  }
  hipLaunchKernelGGL(bs_bistoch<2>, gv, th, 0, st, (const int*)seg, (const int*)nbr, (const int*)nvert, (const double*)n, m, N);
  return sgr_check((int)hipGetLastError(), "sgr_bs_grid_build");
}

#define BS_SOLVE_CHECKS(who)                                                                                                              \
  SGR_REQUIRE(pix2vert && perm && seg && nbr && nvert && m && n, who ": NULL grid tensor");                                                \
  SGR_REQUIRE(bs_shape_ok(B, H, W), who ": bad shape (B, H, W > 0, B*H*W <= 2^28)");                                                       \
  SGR_REQUIRE(cg_maxiter >= 0 && lam >= 0 && A_diag_min > 0 && cg_tol >= 0, who ": bad solver parameter (lam, cg_tol, cg_maxiter >= 0, A_diag_min > 0)"); \
  SGR_SUPPORTED(C >= 1 && C <= 3, who ": 1 to 3 target channels are supported");                                                          \
  SGR_SUPPORTED(cg_maxiter <= kBsMaxIter, who ": cg_maxiter above 64 is not supported")

extern "C" int sgr_bs_solve_fwd(const int* pix2vert, const int* perm, const int* seg, const int* nbr, const int* nvert, const double* m,
                                const double* n, const float* pred, const float* conf, float* out, double* yhat, void* workspace, int B, int C,
                                int H, int W, double lam, double A_diag_min, double cg_tol, int cg_maxiter, void* stream) {
  SGR_REQUIRE(pred && conf && out && yhat && workspace, "sgr_bs_solve_fwd: NULL tensor");
  BS_SOLVE_CHECKS("sgr_bs_solve_fwd");
  const int N = H * W;
  hipStream_t st = (hipStream_t)stream;
  const BsGrid g{pix2vert, perm, seg, nbr, nvert, m, n};
  BsWork w;
  bs_solve_ws((char*)workspace, B, N, C, &w, nullptr);
  const dim3 gp((N + kBsThreads - 1) / kBsThreads, B), th(kBsThreads);
  int rc;
  switch (C) {
    case 1:
      rc = bs_pcg<1, false>(g, w, pred, conf, yhat, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_fwd<1>, gp, th, 0, st, pix2vert, (const double*)yhat, out, N);
      break;
    case 2:
      rc = bs_pcg<2, false>(g, w, pred, conf, yhat, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_fwd<2>, gp, th, 0, st, pix2vert, (const double*)yhat, out, N);
      break;
    default:
      rc = bs_pcg<3, false>(g, w, pred, conf, yhat, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_fwd<3>, gp, th, 0, st, pix2vert, (const double*)yhat, out, N);
      break;
  }
  if (rc == 0) rc = (int)hipGetLastError();
  return sgr_check(rc, "sgr_bs_solve_fwd");
}

extern "C" int sgr_bs_solve_bwd(const int* pix2vert, const int* perm, const int* seg, const int* nbr, const int* nvert, const double* m,
                                const double* n, const float* g_out, const float* pred, const float* conf, const double* yhat, float* g_pred,
                                float* g_conf, void* workspace, int B, int C, int H, int W, double lam, double A_diag_min, double cg_tol,
                                int cg_maxiter, void* stream) {
  SGR_REQUIRE(g_out && pred && conf && yhat && g_pred && g_conf && workspace, "sgr_bs_solve_bwd: NULL tensor");
  BS_SOLVE_CHECKS("sgr_bs_solve_bwd");
  const int N = H * W;
  hipStream_t st = (hipStream_t)stream;
  const BsGrid g{pix2vert, perm, seg, nbr, nvert, m, n};
  BsWork w;
  double* yb;
  bs_solve_ws((char*)workspace, B, N, C, &w, &yb);
  const dim3 gp((N + kBsThreads - 1) / kBsThreads, B), th(kBsThreads);
  int rc;
  switch (C) {
    case 1:
      rc = bs_pcg<1, true>(g, w, g_out, conf, yb, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_bwd<1>, gp, th, 0, st, pix2vert, (const double*)yb, yhat, pred, conf, g_pred, g_conf, N);
      break;
    case 2:
      rc = bs_pcg<2, true>(g, w, g_out, conf, yb, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_bwd<2>, gp, th, 0, st, pix2vert, (const double*)yb, yhat, pred, conf, g_pred, g_conf, N);
      break;
    default:
      rc = bs_pcg<3, true>(g, w, g_out, conf, yb, B, N, lam, A_diag_min, cg_tol, cg_maxiter, st);
      hipLaunchKernelGGL(bs_slice_bwd<3>, gp, th, 0, st, pix2vert, (const double*)yb, yhat, pred, conf, g_pred, g_conf, N);
      break;
  }
  if (rc == 0) rc = (int)hipGetLastError();
  return sgr_check(rc, "sgr_bs_solve_bwd");
}
