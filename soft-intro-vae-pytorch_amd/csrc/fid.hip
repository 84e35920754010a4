// The image variants' validation metric, FID (reference: soft_intro_vae/metrics/fid_score.py): everything around the
// Inception network.  The reference copies every activation batch to the host (:197, :262), keeps 2 x 50 000 x 2048
// float64 there, takes np.mean / np.cov (:349-350, :375-376) and scipy's sqrtm of a non-symmetric product (:307).  Here
// the activations are reduced to their moments (n, s = sum of rows, G = A^T A) as they are produced, in fp64 on the fp64
// matrix pipe (v_mfma_f64_16x16x4_f64), and the distance comes from symmetric eigenvalue problems whose three d x d
// products run on the same tile body (include/sivae_hip.h states the entries).
//
// The tile body is f64_tile.h's ft_tile with both operands as ft_cols: a 64 x 64 tile of C = X^T Y, X [K][M] and Y [K][N]
// row-major, any element type that converts to double.  X^T Y is the orientation in which both operands are read along
// their rows.  Rows >= K and columns >= M / N are zeros that are never read.  One block owns each output tile, so two
// runs are bit-identical.
#include "f64_tile.h"

#define FD_MAX_D 8192 // largest M, N (and the activation dimension)

// what a block does with its tile: C += acc (the moments), C = acc, or C = acc on and above the diagonal with the mirror
enum { FD_ACCUMULATE = 0, FD_ASSIGN = 1, FD_MIRROR = 2 };

// (which entry of the tile a register holds: f64_tile.h's FT_ROW / FT_COL, the fp64 MFMA's own result map)
template <int MODE>
__device__ __forceinline__ void fd_store(double* __restrict__ C, long long ldc, int M, int N, int i0, int j0,
                                         const f64x4 (&acc)[2][2]) {
  FT_PLACE;
  FT_FOR_ACC(mi, ni, r) {
    const int row = i0 + FT_ROW(mi, r), col = j0 + FT_COL(ni);
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
__global__ void __launch_bounds__(FT_NT) fid_moments_kernel(const float* __restrict__ A, long long lda, int n, int d,
                                                            double* __restrict__ G, double* __restrict__ s) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW];
  int bi, bj;
  fd_upper_tile((int)blockIdx.x, FT_TILES(d), bi, bj);
  const int i0 = bi * FT_TILE, j0 = bj * FT_TILE;
  const ft_cols<float> a = {A, lda, d};
  f64x4 acc[2][2];
  if (bi == bj) {
    const double colsum = ft_tile<true>(a, a, n, i0, j0, lx, ly, acc);
    if (threadIdx.x < 64 && j0 + (int)threadIdx.x < d) s[j0 + threadIdx.x] += colsum;
  } else {
    ft_tile<false>(a, a, n, i0, j0, lx, ly, acc);
  }
  fd_store<FD_ACCUMULATE>(G, d, d, d, i0, j0, acc);
}

// C [M][N] = X^T Y in fp64; symmetric (M == N, the product known to be symmetric): the tiles bj >= bi only, each entry on
// or above the diagonal stored at (i, j) and (j, i)
__global__ void __launch_bounds__(FT_NT) fid_xty_kernel(const double* __restrict__ X, long long ldx,
                                                        const double* __restrict__ Y, long long ldy,
                                                        double* __restrict__ C, long long ldc, int K, int M, int N,
                                                        int symmetric) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW];
  int bi, bj;
  if (symmetric) {
    fd_upper_tile((int)blockIdx.x, FT_TILES(N), bi, bj);
  } else {
    const int ntn = FT_TILES(N);
    bi = (int)blockIdx.x / ntn, bj = (int)blockIdx.x % ntn;
  }
  const int i0 = bi * FT_TILE, j0 = bj * FT_TILE;
  const ft_cols<double> x = {X, ldx, M}, y = {Y, ldy, N};
  f64x4 acc[2][2];
  ft_tile<false>(x, y, K, i0, j0, lx, ly, acc);
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

static inline long long fd_upper_tiles(int d) {
  const long long nt = cdiv(d, FT_TILE);
  return nt * (nt + 1) / 2;
}

extern "C" int sivae_fid_moments(const float* A, long long row_stride, int n, int d, double* G, double* s,
                                 hipStream_t stream) {
  if (!A || !G || !s) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FD_MAX_D || n < 0 || row_stride < d) return SIVAE_ERR_SHAPE;
  if (sivae_misaligned(A, 4) || sivae_misaligned(G, 8) || sivae_misaligned(s, 8)) return SIVAE_ERR_SHAPE;
  if (n == 0) return SIVAE_OK;  // (nothing to add)
  hipLaunchKernelGGL(fid_moments_kernel, dim3((unsigned)fd_upper_tiles(d)), dim3(FT_NT), 0, stream, A, row_stride, n, d, G,
                     s);
  return sivae_launch_status();
}

extern "C" int sivae_fid_xty_f64(const double* X, long long ldx, const double* Y, long long ldy, double* C, long long ldc,
                                 int K, int M, int N, int symmetric, hipStream_t stream) {
  if (!X || !Y || !C) return SIVAE_ERR_NULL;
  if (K <= 0 || M <= 0 || N <= 0 || M > FD_MAX_D || N > FD_MAX_D || ldx < M || ldy < N || ldc < N) return SIVAE_ERR_SHAPE;
  if (symmetric != 0 && symmetric != 1) return SIVAE_ERR_MODE;
  if (symmetric && M != N) return SIVAE_ERR_SHAPE;
  if (sivae_misaligned(X, 8) || sivae_misaligned(Y, 8) || sivae_misaligned(C, 8)) return SIVAE_ERR_SHAPE;
  const long long blocks = symmetric ? fd_upper_tiles(N) : (long long)cdiv(M, FT_TILE) * cdiv(N, FT_TILE);
  hipLaunchKernelGGL(fid_xty_kernel, dim3((unsigned)blocks), dim3(FT_NT), 0, stream, X, ldx, Y, ldy, C, ldc, K, M, N,
                     symmetric);
  return sivae_launch_status();
}

extern "C" int sivae_fid_finalize(const double* G, const double* s, long long n, int d, double* mu, double* sigma,
                                  hipStream_t stream) {
  if (!G || !s || !mu || !sigma) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FD_MAX_D || n <= 0) return SIVAE_ERR_SHAPE;
  if (sivae_misaligned(G, 8) || sivae_misaligned(s, 8) || sivae_misaligned(mu, 8) || sivae_misaligned(sigma, 8))
    return SIVAE_ERR_SHAPE;
  hipLaunchKernelGGL(fid_finalize_kernel, dim3((unsigned)cdiv((long long)d * d, 256)), dim3(256), 0, stream, G, s,
                     (double)n, d, mu, sigma);
  return sivae_launch_status();
}
