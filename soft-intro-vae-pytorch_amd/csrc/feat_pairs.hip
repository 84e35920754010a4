// Pairwise figures on the FID features: improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem
// et al. 2020) and KID (Binkowski et al. 2018) all come from X Y^T of two sets of Inception rows.  At 50 000 x 50 000 rows
// the matrix cannot be stored (20 GB in fp64), so every reduction over it (the k smallest distances of a row, the number
// of balls a row lies in, the sum of a polynomial kernel) runs in the epilogue of the tile that produced the entries
// (include/sivae_hip.h states the entries).
//
// ONE tile body, fp_tile_xyt: a 64 x 64 tile of C = X Y^T, X [nx][d] and Y [ny][d] fp32 with unit column stride, every
// element converted to double on load.  The contraction runs along the CONTIGUOUS dimension: the other orientation from
// fid.hip's fd_tile_xty, and the only difference is the fetch and the stash.  A thread loads four consecutive k of one
// row (one 16-byte load where the row base and the row stride allow, scalar loads otherwise) and stores them transposed
// into fid.hip's [k][row] LDS layout; the four-MFMA k-step (v_mfma_f64_16x16x4_f64) and the result map are fid.hip's
// (duplicated, not shared: see NOTES_NEXT_ROUND.md).  Rows >= n and k >= d are zeros that are never read out.  A product
// of two fp32 values is exact in fp64, so the accumulation (k ascending) is the only rounding.  No atomics: every output
// has one owner, two runs are bit-identical.
#include "common.h"

#define FP_NT 256     // threads per block: 4 waves, 2 x 2 over the tile
#define FP_TILE 64    // output tile edge
#define FP_KC 16      // k per staged chunk (4 MFMA k-steps)
#define FP_LDW 80     // LDS row stride in doubles (fid.hip's FD_LDW: the 4 k-rows of a k-step start 32 banks apart)
#define FP_MAX_D 8192 // largest feature dimension
#define FP_MAX_K 8    // largest number of neighbours kept per row
#define FP_DTW 65     // row stride of the staged distance tile in doubles (a thread walking a row: no bank conflict)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// One operand of the tile body: rows [n][d], row stride ld (elements), vec != 0 when the base is 16-byte aligned and
// ld % 4 == 0 (then every whole k-quad of every row is 16-byte aligned)
struct fp_rows {
  const float* p;
  long long ld;
  int n, vec;
};

// thread tid's four elements of the chunk at k0: row r0 + 16 (tid >> 6) + (tid & 15), k = k0 + 4 ((tid >> 4) & 3) + u.
// (16 consecutive lanes hold 16 rows at one k-quad: their ds_write_b64 of one u go to 16 different bank pairs.)
__device__ __forceinline__ void fp_fetch(const fp_rows& P, int d, int r0, int k0, int tid, float (&r)[4]) {
  const int row = r0 + 16 * (tid >> 6) + (tid & 15), k = k0 + 4 * ((tid >> 4) & 3);
  r[0] = r[1] = r[2] = r[3] = 0.f;
  if (row >= P.n || k >= d) return;
  const float* q = P.p + (long long)row * P.ld + k;
  if (P.vec && k + 3 < d) {
    const float4 v = *reinterpret_cast<const float4*>(q);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k + u < d) r[u] = q[u];
  }
}

__device__ __forceinline__ void fp_stash(double* __restrict__ L, int tid, const float (&r)[4]) {
  const int row = 16 * (tid >> 6) + (tid & 15), kq = 4 * ((tid >> 4) & 3);
#pragma unroll
  for (int u = 0; u < 4; ++u) L[(kq + u) * FP_LDW + row] = (double)r[u];
}

// acc[mi][ni] = the wave's 16 x 16 tiles of X Y^T at rows i0 + wm + 16 mi of X, rows j0 + wn + 16 ni of Y (zeroed
// here).  Ends behind a barrier: lx / ly may be rewritten at once.
__device__ __forceinline__ void fp_tile_xyt(const fp_rows& X, const fp_rows& Y, int d, int i0, int j0,
                                            double* __restrict__ lx, double* __restrict__ ly, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  float rx[4], ry[4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  fp_fetch(X, d, i0, 0, tid, rx);
  fp_fetch(Y, d, j0, 0, tid, ry);
  for (int k0 = 0; k0 < d; k0 += FP_KC) {
    fp_stash(lx, tid, rx);
    fp_stash(ly, tid, ry);
    __syncthreads();
    if (k0 + FP_KC < d) {
      fp_fetch(X, d, i0, k0 + FP_KC, tid, rx);
      fp_fetch(Y, d, j0, k0 + FP_KC, tid, ry);
    }
#pragma unroll
    for (int kk = 0; kk < FP_KC; kk += 4) {
      const int kr = (kk + (lane >> 4)) * FP_LDW + (lane & 15);
      const double a0 = lx[kr + wm], a1 = lx[kr + wm + 16], b0 = ly[kr + wn], b1 = ly[kr + wn + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

// The fp64 MFMA's own result map (fid.hip's fd_store): register r of acc[mi][ni] in lane l is tile row
// wm + 16 mi + (l >> 4) + 4 r, tile column wn + 16 ni + (l & 15).
#define FP_ROW(mi, r) (wm + 16 * (mi) + (lane >> 4) + 4 * (r))
#define FP_COL(ni) (wn + 16 * (ni) + (lane & 15))
#define FP_FOR_ACC(mi, ni, r)               \
  _Pragma("unroll") for (int mi = 0; mi < 2; ++mi) \
  _Pragma("unroll") for (int ni = 0; ni < 2; ++ni) \
  _Pragma("unroll") for (int r = 0; r < 4; ++r)

__device__ __forceinline__ double fp_sqdist(double nx, double ny, double dot) { return fmax(0.0, nx + ny - 2.0 * dot); }

// out[i] = sum_k X[i][k]^2 in fp64, k ascending: one thread per row
__global__ void __launch_bounds__(256) feat_row_sqnorm_kernel(fp_rows X, int d, double* __restrict__ out) {
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
__global__ void __launch_bounds__(FP_NT) feat_sqdist_kernel(fp_rows X, const double* __restrict__ nrmx, fp_rows Y,
                                                            const double* __restrict__ nrmy, int d,
                                                            double* __restrict__ D, long long ldd) {
  __shared__ double lx[FP_KC * FP_LDW], ly[FP_KC * FP_LDW];
  const int ntj = (Y.n + FP_TILE - 1) / FP_TILE;
  const int i0 = ((int)blockIdx.x / ntj) * FP_TILE, j0 = ((int)blockIdx.x % ntj) * FP_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  f64x4 acc[2][2];
  fp_tile_xyt(X, Y, d, i0, j0, lx, ly, acc);
  FP_FOR_ACC(mi, ni, r) {
    const int row = i0 + FP_ROW(mi, r), col = j0 + FP_COL(ni);
    if (row < X.n && col < Y.n) D[(long long)row * ldd + col] = fp_sqdist(nrmx[row], nrmy[col], acc[mi][ni][r]);
  }
}

// best [nx][k] (ascending) <- the k smallest of best and sqdist(x_i, y_j), j in [c0, c1) (j != i when self): one block
// owns 64 rows of X and walks the column tiles; the distance tile is staged in LDS and thread t < 64 merges row t.
// Eight slots are kept whatever k is (those >= k start at +inf): the first k of them are the k smallest.
__global__ void __launch_bounds__(FP_NT) feat_knn_kernel(fp_rows X, const double* __restrict__ nrmx, fp_rows Y,
                                                         const double* __restrict__ nrmy, int c0, int c1, int d, int k,
                                                         int self, double* __restrict__ best) {
  __shared__ double lx[FP_KC * FP_LDW], ly[FP_KC * FP_LDW], dt[FP_TILE * FP_DTW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int i0 = (int)blockIdx.x * FP_TILE;
  const int mine = i0 + tid;  // the row thread tid < 64 merges
  const bool merges = tid < FP_TILE && mine < X.n;
  double b[FP_MAX_K];
#pragma unroll
  for (int u = 0; u < FP_MAX_K; ++u) b[u] = (merges && u < k) ? best[(long long)mine * k + u] : (double)INFINITY;
  double nr[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + FP_ROW(mi, r);
      nr[mi][r] = row < X.n ? nrmx[row] : 0.0;
    }
  f64x4 acc[2][2];
  for (int j0 = c0; j0 < c1; j0 += FP_TILE) {
    fp_tile_xyt(X, Y, d, i0, j0, lx, ly, acc);
    // (the merge of the previous tile read dt before the barriers inside fp_tile_xyt)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = j0 + FP_COL(ni);
      const double nc = col < c1 ? nrmy[col] : 0.0;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dt[FP_ROW(mi, r) * FP_DTW + FP_COL(ni)] = col < c1 ? fp_sqdist(nr[mi][r], nc, acc[mi][ni][r]) : (double)INFINITY;
    }
    __syncthreads();
    if (merges) {
      const int skip = self ? mine - j0 : -1;  // the tile column of the row itself, by index
      for (int c = 0; c < FP_TILE; ++c) {
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
__global__ void __launch_bounds__(FP_NT) feat_within_kernel(fp_rows Q, const double* __restrict__ nrmq, fp_rows X,
                                                            const double* __restrict__ nrmx,
                                                            const double* __restrict__ radius, int c0, int c1, int d,
                                                            int* __restrict__ count) {
  __shared__ double lx[FP_KC * FP_LDW], ly[FP_KC * FP_LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int i0 = (int)blockIdx.x * FP_TILE;
  double nr[2][4];
  int cnt[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + FP_ROW(mi, r);
      nr[mi][r] = row < Q.n ? nrmq[row] : 0.0;
      cnt[mi][r] = 0;
    }
  f64x4 acc[2][2];
  for (int j0 = c0; j0 < c1; j0 += FP_TILE) {
    fp_tile_xyt(Q, X, d, i0, j0, lx, ly, acc);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = j0 + FP_COL(ni);
      if (col >= c1) continue;
      const double nc = nrmx[col], rad = radius[col];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt[mi][r] += fp_sqdist(nr[mi][r], nc, acc[mi][ni][r]) <= rad ? 1 : 0;
    }
  }
  // (fp_tile_xyt ended behind a barrier, or never ran: lx is free) 32 partial counts per tile row
  int* red = reinterpret_cast<int*>(lx);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[FP_ROW(mi, r) * 32 + (wave & 1) * 16 + (lane & 15)] = cnt[mi][r];
  __syncthreads();
  if (tid < FP_TILE && i0 + tid < Q.n) {
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
__global__ void __launch_bounds__(FP_NT) feat_poly_kernel(const float* __restrict__ Xp, long long xs, long long ldx,
                                                          int vx, const float* __restrict__ Yp, long long ys,
                                                          long long ldy, int vy, int m, int n, int d, double gamma,
                                                          double coef0, int degree, int skip_diag,
                                                          double* __restrict__ part) {
  __shared__ double lx[FP_KC * FP_LDW], ly[FP_KC * FP_LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int strips = (m + FP_TILE - 1) / FP_TILE;
  const int s = (int)blockIdx.x / strips, i0 = ((int)blockIdx.x % strips) * FP_TILE;
  const fp_rows X = {Xp + (long long)s * xs, ldx, m, vx}, Y = {Yp + (long long)s * ys, ldy, n, vy};
  double sum = 0.0;
  f64x4 acc[2][2];
  for (int j0 = 0; j0 < n; j0 += FP_TILE) {
    fp_tile_xyt(X, Y, d, i0, j0, lx, ly, acc);
    FP_FOR_ACC(mi, ni, r) {
      const int row = i0 + FP_ROW(mi, r), col = j0 + FP_COL(ni);
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

static inline bool fp_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
static inline int fp_vec(const void* p, long long ld) { return !fp_misaligned(p, 16) && ld % 4 == 0; }
// rows [n][d] with stride ld: the checks every entry shares (n < 2^31 - 64: tile starts stay ints)
static inline int fp_check_rows(const float* p, long long ld, int n, int d) {
  if (!p) return SIVAE_ERR_NULL;
  if (d <= 0 || d > FP_MAX_D || n <= 0 || n > 0x7FFFFFFF - FP_TILE || ld < d || fp_misaligned(p, 4)) return SIVAE_ERR_SHAPE;
  return SIVAE_OK;
}

extern "C" int sivae_feat_row_sqnorm(const float* X, long long ld, int n, int d, double* out, hipStream_t stream) {
  if (!out) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(X, ld, n, d)) return rc;
  if (fp_misaligned(out, 8)) return SIVAE_ERR_SHAPE;
  const fp_rows x = {X, ld, n, fp_vec(X, ld)};
  hipLaunchKernelGGL(feat_row_sqnorm_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, x, d, out);
  return sivae_launch_status();
}

extern "C" int sivae_feat_sqdist(const float* X, long long ldx, int nx, const double* nrmx, const float* Y, long long ldy,
                                 int ny, const double* nrmy, int d, double* D, long long ldd, hipStream_t stream) {
  if (!nrmx || !nrmy || !D) return SIVAE_ERR_NULL;
  if (int rc = fp_check_rows(X, ldx, nx, d)) return rc;
  if (int rc = fp_check_rows(Y, ldy, ny, d)) return rc;
  if (ldd < ny || fp_misaligned(nrmx, 8) || fp_misaligned(nrmy, 8) || fp_misaligned(D, 8)) return SIVAE_ERR_SHAPE;
  const long long blocks = (long long)cdiv(nx, FP_TILE) * cdiv(ny, FP_TILE);
  if (blocks > 0x7FFFFFFF) return SIVAE_ERR_RANGE;
  const fp_rows x = {X, ldx, nx, fp_vec(X, ldx)}, y = {Y, ldy, ny, fp_vec(Y, ldy)};
  hipLaunchKernelGGL(feat_sqdist_kernel, dim3((unsigned)blocks), dim3(FP_NT), 0, stream, x, nrmx, y, nrmy, d, D, ldd);
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
  if (fp_misaligned(nrmx, 8) || fp_misaligned(nrmy, 8) || fp_misaligned(best, 8)) return SIVAE_ERR_SHAPE;
  if (c0 == c1) return SIVAE_OK;  // (nothing to merge)
  const fp_rows x = {X, ldx, nx, fp_vec(X, ldx)}, y = {Y, ldy, ny, fp_vec(Y, ldy)};
  hipLaunchKernelGGL(feat_knn_kernel, dim3((unsigned)cdiv(nx, FP_TILE)), dim3(FP_NT), 0, stream, x, nrmx, y, nrmy, c0, c1,
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
  if (fp_misaligned(nrmq, 8) || fp_misaligned(nrmx, 8) || fp_misaligned(radius, 8) || fp_misaligned(count, 4))
    return SIVAE_ERR_SHAPE;
  if (c0 == c1) return SIVAE_OK;  // (nothing to count)
  const fp_rows q = {Q, ldq, nq, fp_vec(Q, ldq)}, x = {X, ldx, nx, fp_vec(X, ldx)};
  hipLaunchKernelGGL(feat_within_kernel, dim3((unsigned)cdiv(nq, FP_TILE)), dim3(FP_NT), 0, stream, q, nrmq, x, nrmx,
                     radius, c0, c1, d, count);
  return sivae_launch_status();
}

extern "C" size_t sivae_feat_poly_workspace_bytes(int S, int m) {
  if (S <= 0 || m <= 0) return 0;
  return (size_t)S * (size_t)cdiv(m, FP_TILE) * sizeof(double);
}

extern "C" int sivae_feat_poly_sums(const float* X, long long x_stride_s, long long ldx, const float* Y,
                                    long long y_stride_s, long long ldy, int S, int m, int n, int d, double gamma,
                                    double coef0, int degree, int skip_diag, double* out, void* workspace,
                                    size_t workspace_bytes, hipStream_t stream) {
  if (!out || !workspace) return SIVAE_ERR_NULL;
  if (S <= 0) return SIVAE_ERR_SHAPE;
  if (int rc = fp_check_rows(X, ldx, m, d)) return rc;
  if (int rc = fp_check_rows(Y, ldy, n, d)) return rc;
  if (x_stride_s < 0 || y_stride_s < 0 || fp_misaligned(out, 8) || fp_misaligned(workspace, 8)) return SIVAE_ERR_SHAPE;
  if (degree < 1 || degree > 4 || (skip_diag != 0 && skip_diag != 1)) return SIVAE_ERR_MODE;
  const int strips = cdiv(m, FP_TILE);
  if ((long long)S * strips > 0x7FFFFFFF) return SIVAE_ERR_RANGE;
  if (workspace_bytes < sivae_feat_poly_workspace_bytes(S, m)) return SIVAE_ERR_WORKSPACE;
  const int vx = fp_vec(X, ldx) && x_stride_s % 4 == 0, vy = fp_vec(Y, ldy) && y_stride_s % 4 == 0;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(feat_poly_kernel, dim3((unsigned)(S * strips)), dim3(FP_NT), 0, stream, X, x_stride_s, ldx, vx, Y,
                     y_stride_s, ldy, vy, m, n, d, gamma, coef0, degree, skip_diag, part);
  hipLaunchKernelGGL(feat_poly_fold_kernel, dim3((unsigned)cdiv(S, 64)), dim3(64), 0, stream, part, S, strips, out);
  return sivae_launch_status();
}
