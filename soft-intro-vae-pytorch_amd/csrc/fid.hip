// The image variants' validation metric, FID (reference: soft_intro_vae/metrics/fid_score.py): everything around the
// Inception network.  The reference copies every activation batch to the host (:197, :262), keeps 2 x 50 000 x 2048
// float64 there, takes np.mean / np.cov (:349-350, :375-376) and scipy's sqrtm of a non-symmetric product (:307).  Here
// the activations are reduced to their moments (n, s = sum of rows, G = A^T A) as they are produced, in fp64 on the fp64
// matrix pipe (v_mfma_f64_16x16x4_f64), and the distance comes from symmetric eigenvalue problems whose three d x d
// products run on the same tile body (include/sivae_hip.h states the entries).
//
// ONE tile body, fd_tile_xty: a 64 x 64 tile of C = X^T Y, X [K][M] and Y [K][N] row-major, any element type that
// converts to double.  X^T Y is the orientation in which both operands are read along their rows: lane l of an MFMA
// holds A[i = l & 15][k = l >> 4] = X[k][i] and B[k = l >> 4][j = l & 15] = Y[k][j], sixteen consecutive elements of a
// row each.  A block of four waves owns the tile (a wave a 32 x 32 quarter: 2 x 2 MFMA tiles, 16 fp64 accumulators a lane)
// and walks K in ascending chunks of 16 rows, staged as fp64 in LDS, the next chunk's global loads in flight over the
// current chunk's MFMAs.  Rows >= K and columns >= M / N are zeros that are never read.  No atomics, no split of K: one
// block owns each output tile, so two runs are bit-identical.
#include "common.h"

#define FD_NT 256     // threads per block: 4 waves, 2 x 2 over the tile
#define FD_TILE 64    // output tile edge
#define FD_KC 16      // rows of X and Y per staged chunk (4 MFMA k-steps)
#define FD_LDW 80     // LDS row stride in doubles: the 4 k-rows of a k-step start 32 banks apart (2 passes per ds_read_b64)
#define FD_MAX_D 8192 // largest M, N (and the activation dimension)
#define FD_RPT (FD_KC * FD_TILE / FD_NT)  // staged elements per thread and operand: 4
#define FD_TILES(w) (((w) + FD_TILE - 1) / FD_TILE)  // tiles along an edge of w elements

typedef double f64x4 __attribute__((ext_vector_type(4)));

// thread tid's FD_RPT elements of the chunk at row k0, columns c0 .. c0 + 63 of P [K][W] (row stride ld), as doubles
template <typename T>
__device__ __forceinline__ void fd_fetch(const T* __restrict__ P, long long ld, int K, int W, int k0, int c0, int tid,
                                         double (&r)[FD_RPT]) {
  const int col = c0 + (tid & 63);
#pragma unroll
  for (int u = 0; u < FD_RPT; ++u) {
    const int k = k0 + (tid >> 6) + 4 * u;
    r[u] = (k < K && col < W) ? (double)P[(long long)k * ld + col] : 0.0;
  }
}

__device__ __forceinline__ void fd_stash(double* __restrict__ L, int tid, const double (&r)[FD_RPT]) {
#pragma unroll
  for (int u = 0; u < FD_RPT; ++u) L[((tid >> 6) + 4 * u) * FD_LDW + (tid & 63)] = r[u];
}

// acc[mi][ni] = the wave's 16 x 16 tiles of X^T Y at rows i0 + wm + 16 mi, columns j0 + wn + 16 ni (zeroed here).
// SUMS: thread t < 64 also returns in colsum the sum over k (ascending) of Y[k][j0 + t].
template <typename T, bool SUMS>
__device__ __forceinline__ void fd_tile_xty(const T* __restrict__ X, long long ldx, int M, const T* __restrict__ Y,
                                            long long ldy, int N, int K, int i0, int j0, double* __restrict__ lx,
                                            double* __restrict__ ly, f64x4 (&acc)[2][2], double& colsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  double rx[FD_RPT], ry[FD_RPT];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  colsum = 0.0;
  fd_fetch(X, ldx, K, M, 0, i0, tid, rx);
  fd_fetch(Y, ldy, K, N, 0, j0, tid, ry);
  for (int k0 = 0; k0 < K; k0 += FD_KC) {
    fd_stash(lx, tid, rx);
    fd_stash(ly, tid, ry);
    __syncthreads();
    if (k0 + FD_KC < K) {
      fd_fetch(X, ldx, K, M, k0 + FD_KC, i0, tid, rx);
      fd_fetch(Y, ldy, K, N, k0 + FD_KC, j0, tid, ry);
    }
    if (SUMS && tid < 64) {  // (wave 0 alone)
#pragma unroll
      for (int k = 0; k < FD_KC; ++k) colsum += ly[k * FD_LDW + tid];
    }
#pragma unroll
    for (int kk = 0; kk < FD_KC; kk += 4) {
      const int kr = (kk + (lane >> 4)) * FD_LDW + (lane & 15);
      const double a0 = lx[kr + wm], a1 = lx[kr + wm + 16], b0 = ly[kr + wn], b1 = ly[kr + wn + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

// what a block does with its tile: C += acc (the moments), C = acc, or C = acc on and above the diagonal with the mirror
enum { FD_ACCUMULATE = 0, FD_ASSIGN = 1, FD_MIRROR = 2 };

// the fp64 MFMA's own result map (not the other forms'): register r of lane l is row (l >> 4) + 4 r, column l & 15
template <int MODE>
__device__ __forceinline__ void fd_store(double* __restrict__ C, long long ldc, int M, int N, int i0, int j0,
                                         const f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wm + 16 * mi + (lane >> 4) + 4 * r, col = j0 + wn + 16 * ni + (lane & 15);
        if (row >= M || col >= N) continue;
        const double v = acc[mi][ni][r];
        if (MODE == FD_ACCUMULATE) {
          C[(long long)row * ldc + col] += v;
        } else if (MODE == FD_ASSIGN) {
          C[(long long)row * ldc + col] = v;
        } else if (col >= row) {
          C[(long long)row * ldc + col] = v;
          C[(long long)col * ldc + row] = v;
        }
      }
}

// block b of the nt (nt + 1) / 2 tiles on and above the diagonal, by rows: -> (bi, bj >= bi)
__device__ __forceinline__ void fd_upper_tile(int b, int nt, int& bi, int& bj) {
  bi = 0;
  while (b >= nt - bi) {
    b -= nt - bi;
    ++bi;
  }
  bj = bi + b;
}

// G [d][d] += A^T A on the block tiles bj >= bi (the others are never touched), s [d] += column sums (by the diagonal
// blocks); A [n][d] fp32, converted on load
__global__ void __launch_bounds__(FD_NT) fid_moments_kernel(const float* __restrict__ A, long long lda, int n, int d,
                                                            double* __restrict__ G, double* __restrict__ s) {
  __shared__ double lx[FD_KC * FD_LDW], ly[FD_KC * FD_LDW];
  int bi, bj;
  fd_upper_tile((int)blockIdx.x, FD_TILES(d), bi, bj);
  const int i0 = bi * FD_TILE, j0 = bj * FD_TILE;
  f64x4 acc[2][2];
  double colsum;
  if (bi == bj) {
    fd_tile_xty<float, true>(A, lda, d, A, lda, d, n, i0, j0, lx, ly, acc, colsum);
    if (threadIdx.x < 64 && j0 + (int)threadIdx.x < d) s[j0 + threadIdx.x] += colsum;
  } else {
    fd_tile_xty<float, false>(A, lda, d, A, lda, d, n, i0, j0, lx, ly, acc, colsum);
  }
  fd_store<FD_ACCUMULATE>(G, d, d, d, i0, j0, acc);
}

// C [M][N] = X^T Y in fp64; symmetric (M == N, the product known to be symmetric): the tiles bj >= bi only, each entry on
// or above the diagonal stored at (i, j) and (j, i)
__global__ void __launch_bounds__(FD_NT) fid_xty_kernel(const double* __restrict__ X, long long ldx,
                                                        const double* __restrict__ Y, long long ldy,
                                                        double* __restrict__ C, long long ldc, int K, int M, int N,
                                                        int symmetric) {
  __shared__ double lx[FD_KC * FD_LDW], ly[FD_KC * FD_LDW];
  int bi, bj;
  if (symmetric) {
    fd_upper_tile((int)blockIdx.x, FD_TILES(N), bi, bj);
  } else {
    const int ntn = FD_TILES(N);
    bi = (int)blockIdx.x / ntn, bj = (int)blockIdx.x % ntn;
  }
  const int i0 = bi * FD_TILE, j0 = bj * FD_TILE;
  f64x4 acc[2][2];
  double unused;
  fd_tile_xty<double, false>(X, ldx, M, Y, ldy, N, K, i0, j0, lx, ly, acc, unused);
  if (symmetric)
    fd_store<FD_MIRROR>(C, ldc, M, N, i0, j0, acc);
  else
    fd_store<FD_ASSIGN>(C, ldc, M, N, i0, j0, acc);
}

// mu = s / n, sigma = (G - s s^T / n) / (n - 1) as the full symmetric matrix, from G's entries on and above the diagonal
// (both halves of sigma come from the same expression: exactly symmetric); n = 1 gives NaN, as np.cov does
__global__ void __launch_bounds__(256) fid_finalize_kernel(const double* __restrict__ G, const double* __restrict__ s,
                                                           double n, int d, double* __restrict__ mu,
                                                           double* __restrict__ sigma) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)d * d) return;
  const int i = (int)(e / d), j = (int)(e % d);
  const int lo = min(i, j), hi = max(i, j);
  if (e < d) mu[e] = s[e] / n;
  sigma[e] = n == 1.0 ? (double)NAN : (G[(long long)lo * d + hi] - s[lo] * s[hi] / n) / (n - 1.0);
}

static inline bool fd_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
static inline long long fd_upper_tiles(int d) {
  const long long nt = cdiv(d, FD_TILE);
  return nt * (nt + 1) / 2;
}

extern "C" int sivae_fid_moments(const float* A, long long row_stride, int n, int d, double* G, double* s,
                                 hipStream_t stream) {
  if (!A || !G || !s) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FD_MAX_D || n < 0 || row_stride < d) return SIVAE_ERR_SHAPE;
  if (fd_misaligned(A, 4) || fd_misaligned(G, 8) || fd_misaligned(s, 8)) return SIVAE_ERR_SHAPE;
  if (n == 0) return SIVAE_OK;  // (nothing to add)
  hipLaunchKernelGGL(fid_moments_kernel, dim3((unsigned)fd_upper_tiles(d)), dim3(FD_NT), 0, stream, A, row_stride, n, d, G,
                     s);
  return sivae_launch_status();
}

extern "C" int sivae_fid_xty_f64(const double* X, long long ldx, const double* Y, long long ldy, double* C, long long ldc,
                                 int K, int M, int N, int symmetric, hipStream_t stream) {
  if (!X || !Y || !C) return SIVAE_ERR_NULL;
  if (K <= 0 || M <= 0 || N <= 0 || M > FD_MAX_D || N > FD_MAX_D || ldx < M || ldy < N || ldc < N) return SIVAE_ERR_SHAPE;
  if (symmetric != 0 && symmetric != 1) return SIVAE_ERR_MODE;
  if (symmetric && M != N) return SIVAE_ERR_SHAPE;
  if (fd_misaligned(X, 8) || fd_misaligned(Y, 8) || fd_misaligned(C, 8)) return SIVAE_ERR_SHAPE;
  const long long blocks = symmetric ? fd_upper_tiles(N) : (long long)cdiv(M, FD_TILE) * cdiv(N, FD_TILE);
  hipLaunchKernelGGL(fid_xty_kernel, dim3((unsigned)blocks), dim3(FD_NT), 0, stream, X, ldx, Y, ldy, C, ldc, K, M, N,
                     symmetric);
  return sivae_launch_status();
}

extern "C" int sivae_fid_finalize(const double* G, const double* s, long long n, int d, double* mu, double* sigma,
                                  hipStream_t stream) {
  if (!G || !s || !mu || !sigma) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FD_MAX_D || n <= 0) return SIVAE_ERR_SHAPE;
  if (fd_misaligned(G, 8) || fd_misaligned(s, 8) || fd_misaligned(mu, 8) || fd_misaligned(sigma, 8)) return SIVAE_ERR_SHAPE;
  hipLaunchKernelGGL(fid_finalize_kernel, dim3((unsigned)cdiv((long long)d * d, 256)), dim3(256), 0, stream, G, s,
                     (double)n, d, mu, sigma);
  return sivae_launch_status();
}
