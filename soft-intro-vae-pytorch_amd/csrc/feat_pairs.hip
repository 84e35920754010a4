// Pairwise figures on the FID features: improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem
// et al. 2020) and KID (Binkowski et al. 2018) all come from X Y^T of two sets of Inception rows.  At 50 000 x 50 000 rows
// the matrix cannot be stored (20 GB in fp64), so every reduction over it (the k smallest distances of a row, the number
// of balls a row lies in, the sum of a polynomial kernel) runs in the epilogue of the tile that produced the entries
// (include/sivae_hip.h states the entries).
//
// The tile body is f64_tile.h's ft_tile with both operands as ft_rows: a 64 x 64 tile of C = X Y^T, X [nx][d] and
// Y [ny][d] fp32 with unit column stride, every element converted to double on load.  The contraction runs along the
// CONTIGUOUS dimension, the other orientation from fid.hip's; the k-step and the result map (FT_ROW / FT_COL) are the
// same code.  Rows >= n and k >= d are zeros that are never read out.  A product of two fp32 values is exact in fp64, so
// the accumulation (k ascending) is the only rounding.  No atomics: every output has one owner, two runs are
// bit-identical.
#include "f64_tile.h"

#define FP_MAX_D 8192 // largest feature dimension
#define FP_MAX_K 8    // largest number of neighbours kept per row
#define FP_DTW 65     // row stride of the staged distance tile in doubles (a thread walking a row: no bank conflict)

__device__ __forceinline__ double fp_sqdist(double nx, double ny, double dot) { return fmax(0.0, nx + ny - 2.0 * dot); }

// out[i] = sum_k X[i][k]^2 in fp64, k ascending: one thread per row
__global__ void __launch_bounds__(256) feat_row_sqnorm_kernel(ft_rows X, int d, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n) return;
  const float* q = X.p + i * X.ld;
  double s = 0.0;
  int k = 0;
  if (X.vec) {
    for (; k + 3 < d; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(q + k);
      s += (double)v.x * (double)v.x;
      s += (double)v.y * (double)v.y;
      s += (double)v.z * (double)v.z;
      s += (double)v.w * (double)v.w;
    }
  }
  for (; k < d; ++k) s += (double)q[k] * (double)q[k];
  out[i] = s;
}

// D[i][j] = sqdist(x_i, y_j): one block per output tile
__global__ void __launch_bounds__(FT_NT) feat_sqdist_kernel(ft_rows X, const double* __restrict__ nrmx, ft_rows Y,
                                                            const double* __restrict__ nrmy, int d,
                                                            double* __restrict__ D, long long ldd) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW];
  const int ntj = FT_TILES(Y.n);
  const int i0 = ((int)blockIdx.x / ntj) * FT_TILE, j0 = ((int)blockIdx.x % ntj) * FT_TILE;
  FT_PLACE;
  f64x4 acc[2][2];
  ft_tile<false>(X, Y, d, i0, j0, lx, ly, acc);
  FT_FOR_ACC(mi, ni, r) {
    const int row = i0 + FT_ROW(mi, r), col = j0 + FT_COL(ni);
    if (row < X.n && col < Y.n) D[(long long)row * ldd + col] = fp_sqdist(nrmx[row], nrmy[col], acc[mi][ni][r]);
  }
}

// best [nx][k] (ascending) <- the k smallest of best and sqdist(x_i, y_j), j in [c0, c1) (j != i when self): one block
// owns 64 rows of X and walks the column tiles; the distance tile is staged in LDS and thread t < 64 merges row t.
// Eight slots are kept whatever k is (those >= k start at +inf): the first k of them are the k smallest.
__global__ void __launch_bounds__(FT_NT) feat_knn_kernel(ft_rows X, const double* __restrict__ nrmx, ft_rows Y,
                                                         const double* __restrict__ nrmy, int c0, int c1, int d, int k,
                                                         int self, double* __restrict__ best) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW], dt[FT_TILE * FP_DTW];
  const int tid = threadIdx.x;
  FT_PLACE;
  const int i0 = (int)blockIdx.x * FT_TILE;
  const int mine = i0 + tid;  // the row thread tid < 64 merges
  const bool merges = tid < FT_TILE && mine < X.n;
  double b[FP_MAX_K];
#pragma unroll
  for (int u = 0; u < FP_MAX_K; ++u) b[u] = (merges && u < k) ? best[(long long)mine * k + u] : (double)INFINITY;
  double nr[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + FT_ROW(mi, r);
      nr[mi][r] = row < X.n ? nrmx[row] : 0.0;
    }
  f64x4 acc[2][2];
  for (int j0 = c0; j0 < c1; j0 += FT_TILE) {
    ft_tile<false>(X, Y, d, i0, j0, lx, ly, acc);
    // (the merge of the previous tile read dt before the barriers inside ft_tile)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = j0 + FT_COL(ni);
      const double nc = col < c1 ? nrmy[col] : 0.0;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dt[FT_ROW(mi, r) * FP_DTW + FT_COL(ni)] = col < c1 ? fp_sqdist(nr[mi][r], nc, acc[mi][ni][r]) : (double)INFINITY;
    }
    __syncthreads();
    if (merges) {
      const int skip = self ? mine - j0 : -1;  // the tile column of the row itself, by index
      for (int c = 0; c < FT_TILE; ++c) {
        const double v = dt[tid * FP_DTW + c];
        if (c == skip || !(v < b[FP_MAX_K - 1])) continue;
        b[FP_MAX_K - 1] = v;
#pragma unroll
        for (int u = FP_MAX_K - 1; u > 0; --u) {
          const double lo = b[u] < b[u - 1] ? b[u] : b[u - 1], hi = b[u] < b[u - 1] ? b[u - 1] : b[u];
          b[u - 1] = lo, b[u] = hi;
        }
      }
    }
  }
  if (merges) {
#pragma unroll
    for (int u = 0; u < FP_MAX_K; ++u)
      if (u < k) best[(long long)mine * k + u] = b[u];
  }
}

// count[j] += #{ i in [c0, c1) : sqdist(q_j, x_i) <= radius[i] }: one block owns 64 rows of Q and walks the column tiles
// (rows of X); a lane counts its own entries, the counts of a row are added through LDS at the end (integers: exact in
// any order)
__global__ void __launch_bounds__(FT_NT) feat_within_kernel(ft_rows Q, const double* __restrict__ nrmq, ft_rows X,
                                                            const double* __restrict__ nrmx,
                                                            const double* __restrict__ radius, int c0, int c1, int d,
                                                            int* __restrict__ count) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW];
  const int tid = threadIdx.x;
  FT_PLACE;
  const int i0 = (int)blockIdx.x * FT_TILE;
  double nr[2][4];
  int cnt[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + FT_ROW(mi, r);
      nr[mi][r] = row < Q.n ? nrmq[row] : 0.0;
      cnt[mi][r] = 0;
    }
  f64x4 acc[2][2];
  for (int j0 = c0; j0 < c1; j0 += FT_TILE) {
    ft_tile<false>(Q, X, d, i0, j0, lx, ly, acc);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = j0 + FT_COL(ni);
      if (col >= c1) continue;
      const double nc = nrmx[col], rad = radius[col];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt[mi][r] += fp_sqdist(nr[mi][r], nc, acc[mi][ni][r]) <= rad ? 1 : 0;
    }
  }
  // (ft_tile ended behind a barrier, or never ran: lx is free) 32 partial counts per tile row: a slot for each of the 16
  // lanes of the row in the two waves that share it
  int* red = reinterpret_cast<int*>(lx);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[FT_ROW(mi, r) * 32 + (wave & 1) * 16 + (lane & 15)] = cnt[mi][r];
  __syncthreads();
  if (tid < FT_TILE && i0 + tid < Q.n) {
    int s = 0;
    for (int u = 0; u < 32; ++u) s += red[tid * 32 + u];
    count[i0 + tid] += s;
  }
}

__device__ __forceinline__ double fp_poly(double dot, double gamma, double coef0, int degree) {
  const double t = gamma * dot + coef0;
  double v = t;
  for (int e = 1; e < degree; ++e) v *= t;
  return v;
}

// part[s][strip] = sum over the strip's 64 rows i and all columns j (j != i with skip_diag) of
// (gamma x_si . y_sj + coef0)^degree: one block per (subset, strip).  A lane adds its own entries in tile order, the 256
// lane sums are folded in a fixed order.
__global__ void __launch_bounds__(FT_NT) feat_poly_kernel(const float* __restrict__ Xp, long long xs, long long ldx,
                                                          int vx, const float* __restrict__ Yp, long long ys,
                                                          long long ldy, int vy, int m, int n, int d, double gamma,
                                                          double coef0, int degree, int skip_diag,
                                                          double* __restrict__ part) {
  __shared__ double lx[FT_KC * FT_LDW], ly[FT_KC * FT_LDW];
  const int tid = threadIdx.x;
  FT_PLACE;
  const int strips = FT_TILES(m);
  const int s = (int)blockIdx.x / strips, i0 = ((int)blockIdx.x % strips) * FT_TILE;
  const ft_rows X = {Xp + (long long)s * xs, ldx, m, vx}, Y = {Yp + (long long)s * ys, ldy, n, vy};
  double sum = 0.0;
  f64x4 acc[2][2];
  for (int j0 = 0; j0 < n; j0 += FT_TILE) {
    ft_tile<false>(X, Y, d, i0, j0, lx, ly, acc);
    FT_FOR_ACC(mi, ni, r) {
      const int row = i0 + FT_ROW(mi, r), col = j0 + FT_COL(ni);
      if (row < m && col < n && !(skip_diag && row == col)) sum += fp_poly(acc[mi][ni][r], gamma, coef0, degree);
    }
  }
  lx[tid] = sum;
  __syncthreads();
  if (tid < 64) lx[tid] = (lx[tid] + lx[tid + 64]) + (lx[tid + 128] + lx[tid + 192]);
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int u = 0; u < 64; ++u) t += lx[u];
    part[blockIdx.x] = t;
  }
}

// out[s] = sum of part[s][strip], strips ascending
__global__ void __launch_bounds__(64) feat_poly_fold_kernel(const double* __restrict__ part, int S, int strips,
                                                            double* __restrict__ out) {
  const int s = (int)blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  double t = 0.0;
  for (int u = 0; u < strips; ++u) t += part[(long long)s * strips + u];
  out[s] = t;
}

static inline int fp_vec(const void* p, long long ld) { return !sivae_misaligned(p, 16) && ld % 4 == 0; }
// rows [n][d] with stride ld: the checks every entry shares (n < 2^31 - 64: tile starts stay ints)
static inline int fp_check_rows(const float* p, long long ld, int n, int d) {
  if (!p) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FP_MAX_D || n <= 0 || n > 0x7FFFFFFF - FT_TILE || ld < d || sivae_misaligned(p, 4))
    return SIVAE_ERR_SHAPE;
  return SIVAE_OK;
}

extern "C" int sivae_feat_row_sqnorm(const float* X, long long ld, int n, int d, double* out, hipStream_t stream) {
  if (!out) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(X, ld, n, d)) return rc;
  if (sivae_misaligned(out, 8)) return SIVAE_ERR_SHAPE;
  const ft_rows x = {X, ld, n, fp_vec(X, ld)};
  hipLaunchKernelGGL(feat_row_sqnorm_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, x, d, out);
  return sivae_launch_status();
}

extern "C" int sivae_feat_sqdist(const float* X, long long ldx, int nx, const double* nrmx, const float* Y, long long ldy,
                                 int ny, const double* nrmy, int d, double* D, long long ldd, hipStream_t stream) {
  if (!nrmx || !nrmy || !D) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(X, ldx, nx, d)) return rc;
  if (int rc = fp_check_rows(Y, ldy, ny, d)) return rc;
  if (ldd < ny || sivae_misaligned(nrmx, 8) || sivae_misaligned(nrmy, 8) || sivae_misaligned(D, 8)) return SIVAE_ERR_SHAPE;
  const long long blocks = (long long)cdiv(nx, FT_TILE) * cdiv(ny, FT_TILE);
  if (blocks > 0x7FFFFFFF) return SIVAE_ERR_RANGE;
  const ft_rows x = {X, ldx, nx, fp_vec(X, ldx)}, y = {Y, ldy, ny, fp_vec(Y, ldy)};
  hipLaunchKernelGGL(feat_sqdist_kernel, dim3((unsigned)blocks), dim3(FT_NT), 0, stream, x, nrmx, y, nrmy, d, D, ldd);
  return sivae_launch_status();
}

extern "C" int sivae_feat_knn_update(const float* X, long long ldx, int nx, const double* nrmx, const float* Y,
                                     long long ldy, int ny, const double* nrmy, int c0, int c1, int d, int k, int self,
                                     double* best, hipStream_t stream) {
  if (!nrmx || !nrmy || !best) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(X, ldx, nx, d)) return rc;
  if (int rc = fp_check_rows(Y, ldy, ny, d)) return rc;
  if (k < 1 || k > FP_MAX_K || c0 < 0 || c1 < c0 || c1 > ny) return SIVAE_ERR_SHAPE;
  if (self != 0 && self != 1) return SIVAE_ERR_MODE;
  if (sivae_misaligned(nrmx, 8) || sivae_misaligned(nrmy, 8) || sivae_misaligned(best, 8)) return SIVAE_ERR_SHAPE;
  if (c0 == c1) return SIVAE_OK;  // (nothing to merge)
  const ft_rows x = {X, ldx, nx, fp_vec(X, ldx)}, y = {Y, ldy, ny, fp_vec(Y, ldy)};
  hipLaunchKernelGGL(feat_knn_kernel, dim3((unsigned)cdiv(nx, FT_TILE)), dim3(FT_NT), 0, stream, x, nrmx, y, nrmy, c0, c1,
                     d, k, self, best);
  return sivae_launch_status();
}

extern "C" int sivae_feat_within_update(const float* Q, long long ldq, int nq, const double* nrmq, const float* X,
                                        long long ldx, int nx, const double* nrmx, const double* radius, int c0, int c1,
                                        int d, int* count, hipStream_t stream) {
  if (!nrmq || !nrmx || !radius || !count) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(Q, ldq, nq, d)) return rc;
  if (int rc = fp_check_rows(X, ldx, nx, d)) return rc;
  if (c0 < 0 || c1 < c0 || c1 > nx) return SIVAE_ERR_SHAPE;
  if (sivae_misaligned(nrmq, 8) || sivae_misaligned(nrmx, 8) || sivae_misaligned(radius, 8) || sivae_misaligned(count, 4))
    return SIVAE_ERR_SHAPE;
  if (c0 == c1) return SIVAE_OK;  // (nothing to count)
  const ft_rows q = {Q, ldq, nq, fp_vec(Q, ldq)}, x = {X, ldx, nx, fp_vec(X, ldx)};
  hipLaunchKernelGGL(feat_within_kernel, dim3((unsigned)cdiv(nq, FT_TILE)), dim3(FT_NT), 0, stream, q, nrmq, x, nrmx,
                     radius, c0, c1, d, count);
  return sivae_launch_status();
}

extern "C" size_t sivae_feat_poly_workspace_bytes(int S, int m) {
  if (S <= 0 || m <= 0) return 0;
  return (size_t)S * (size_t)cdiv(m, FT_TILE) * sizeof(double);
}

extern "C" int sivae_feat_poly_sums(const float* X, long long x_stride_s, long long ldx, const float* Y,
                                    long long y_stride_s, long long ldy, int S, int m, int n, int d, double gamma,
                                    double coef0, int degree, int skip_diag, double* out, void* workspace,
                                    size_t workspace_bytes, hipStream_t stream) {
  if (!out || !workspace) return SIVAE_ERR_NULL;
  if (S <= 0) return SIVAE_ERR_SHAPE;
  if (int rc = fp_check_rows(X, ldx, m, d)) return rc;
  if (int rc = fp_check_rows(Y, ldy, n, d)) return rc;
  if (x_stride_s < 0 || y_stride_s < 0 || sivae_misaligned(out, 8) || sivae_misaligned(workspace, 8)) return SIVAE_ERR_SHAPE;
  if (degree < 1 || degree > 4 || (skip_diag != 0 && skip_diag != 1)) return SIVAE_ERR_MODE;
  const int strips = cdiv(m, FT_TILE);
  if ((long long)S * strips > 0x7FFFFFFF) return SIVAE_ERR_RANGE;
  if (workspace_bytes < sivae_feat_poly_workspace_bytes(S, m)) return SIVAE_ERR_WORKSPACE;
  const int vx = fp_vec(X, ldx) && x_stride_s % 4 == 0, vy = fp_vec(Y, ldy) && y_stride_s % 4 == 0;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(feat_poly_kernel, dim3((unsigned)(S * strips)), dim3(FT_NT), 0, stream, X, x_stride_s, ldx, vx, Y,
                     y_stride_s, ldy, vy, m, n, d, gamma, coef0, degree, skip_diag, part);
  hipLaunchKernelGGL(feat_poly_fold_kernel, dim3((unsigned)cdiv(S, 64)), dim3(64), 0, stream, part, S, strips, out);
  return sivae_launch_status();
}
