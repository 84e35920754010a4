// The ONE fp64 MFMA tile body of the metric kernels (fid.hip: C = X^T Y; feat_pairs.hip: C = X Y^T) and the only place
// that knows the tile: its constants, its LDS layout, the four-MFMA k-step (v_mfma_f64_16x16x4_f64) and the
// instruction's result map.
//
// ft_tile: a 64 x 64 tile of C, contraction length K.  A block of four waves owns the tile (a wave a 32 x 32 quarter:
// 2 x 2 MFMA tiles, 16 fp64 accumulators a lane) and walks K in ascending chunks of 16, staged as fp64 in LDS as
// [k][tile row] (X) and [k][tile column] (Y), the next chunk's global loads in flight over the current chunk's MFMAs.
// Lane l of an MFMA holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]: sixteen consecutive elements of an LDS
// row each.  Everything outside the operands is staged as zeros that are never read out.  No atomics, no split of K: the
// accumulation of a result is k-ascending whatever the operands, so two runs are bit-identical.
//
// Of the two orientations only fetch and stash differ, and they live in the operand types: ft_cols (the contraction runs
// over the rows of a row-major matrix, both operands read along their rows) and ft_rows (the contraction runs along the
// contiguous dimension of fp32 rows, stored transposed into the same LDS layout).
#pragma once
#include "common.h"

#define FT_NT 256     // threads per block: 4 waves, 2 x 2 over the tile
#define FT_TILE 64    // output tile edge
#define FT_KC 16      // k per staged chunk (4 MFMA k-steps)
#define FT_LDW 80     // LDS row stride in doubles: the 4 k-rows of a k-step start 32 banks apart (2 passes per ds_read_b64)
#define FT_RPT (FT_KC * FT_TILE / FT_NT)  // staged elements per thread and operand: 4
#define FT_TILES(w) (((w) + FT_TILE - 1) / FT_TILE)  // tiles along an edge of w elements

typedef double f64x4 __attribute__((ext_vector_type(4)));

// The fp64 MFMA's own result map (not the other forms'): register r of acc[mi][ni] in lane l is tile row
// wm + 16 mi + (l >> 4) + 4 r, tile column wn + 16 ni + (l & 15), (wm, wn) the wave's quarter.  The (l >> 4) * 4 + r of
// every other MFMA form runs clean here and misplaces three of four results.
// FT_PLACE declares where the thread is (lane, wave, wm, wn) for FT_ROW / FT_COL: plain locals at the top of a kernel.
// (A struct with row() / col() members or functions that rederive the place were tried for the fold: each moved the
// strip kernels' index arithmetic, and feat_within_kernel then ran 0.9 % slower; see profiles/f64_tile_fold.txt.)
#define FT_PLACE                                              \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6; \
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32
#define FT_ROW(mi, r) (wm + 16 * (mi) + (lane >> 4) + 4 * (r))
#define FT_COL(ni) (wn + 16 * (ni) + (lane & 15))
// every result of a lane: acc[mi][ni][r] is the entry (FT_ROW(mi, r), FT_COL(ni)) of the tile
#define FT_FOR_ACC(mi, ni, r)                      \
  _Pragma("unroll") for (int mi = 0; mi < 2; ++mi) \
  _Pragma("unroll") for (int ni = 0; ni < 2; ++ni) \
  _Pragma("unroll") for (int r = 0; r < 4; ++r)

// Operand "columns": P [K][w] row-major (row stride ld), any element type that converts to double; the tile's 64 rows
// (X) or columns (Y) are the columns c0 .. c0 + 63 of P.  Sixteen consecutive lanes read consecutive elements of a row:
// coalesced, and no transpose is staged.
template <typename T>
struct ft_cols {
  const T* p;
  long long ld;
  int w;
  typedef double regs[FT_RPT];

  // thread tid's FT_RPT elements of the chunk at row k0, as doubles
  __device__ __forceinline__ void fetch(int K, int k0, int c0, int tid, regs& r) const {
    const int col = c0 + (tid & 63);
#pragma unroll
    for (int u = 0; u < FT_RPT; ++u) {
      const int k = k0 + (tid >> 6) + 4 * u;
      r[u] = (k < K && col < w) ? (double)p[(long long)k * ld + col] : 0.0;
    }
  }
  static __device__ __forceinline__ void stash(double* __restrict__ L, int tid, const regs& r) {
#pragma unroll
    for (int u = 0; u < FT_RPT; ++u) L[((tid >> 6) + 4 * u) * FT_LDW + (tid & 63)] = r[u];
  }
};

// Operand "rows": fp32 rows [n][K] with unit column stride and row stride ld (elements), converted to double on the way
// into LDS; the tile's 64 rows (X) or columns (Y) are the rows c0 .. c0 + 63.  vec != 0 when the base is 16-byte aligned
// and ld % 4 == 0 (then every whole k-quad of every row is 16-byte aligned).
struct ft_rows {
  const float* p;
  long long ld;
  int n, vec;
  typedef float regs[4];

  // thread tid's four elements of the chunk at k0: row c0 + 16 (tid >> 6) + (tid & 15), k = k0 + 4 ((tid >> 4) & 3) + u
  // (one 16-byte load where vec allows, scalar loads otherwise).
  // (16 consecutive lanes hold 16 rows at one k-quad: their ds_write_b64 of one u go to 16 different bank pairs.)
  __device__ __forceinline__ void fetch(int K, int k0, int c0, int tid, regs& r) const {
    const int row = c0 + 16 * (tid >> 6) + (tid & 15), k = k0 + 4 * ((tid >> 4) & 3);
    r[0] = r[1] = r[2] = r[3] = 0.f;
    if (row >= n || k >= K) return;
    const float* q = p + (long long)row * ld + k;
    if (vec && k + 3 < K) {
      const float4 v = *reinterpret_cast<const float4*>(q);
      r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k + u < K) r[u] = q[u];
    }
  }
  // transposed: into the [k][row] layout
  static __device__ __forceinline__ void stash(double* __restrict__ L, int tid, const regs& r) {
    const int row = 16 * (tid >> 6) + (tid & 15), kq = 4 * ((tid >> 4) & 3);
#pragma unroll
    for (int u = 0; u < 4; ++u) L[(kq + u) * FT_LDW + row] = (double)r[u];
  }
};

// acc[mi][ni] = the wave's 16 x 16 tiles of C at tile rows i0 + FT_ROW(mi, .) and tile columns j0 + FT_COL(ni) (zeroed
// here); lx, ly: FT_KC * FT_LDW doubles of LDS each.  Ends behind a barrier: lx / ly may be rewritten at once.
// SUMS: thread t < 64 returns the sum over k (ascending) of Y's tile column t; every other return value is 0.
template <bool SUMS, class OX, class OY>
__device__ __forceinline__ double ft_tile(const OX& X, const OY& Y, int K, int i0, int j0, double* __restrict__ lx,
                                          double* __restrict__ ly, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x;
  FT_PLACE;
  typename OX::regs rx;
  typename OY::regs ry;
  double colsum = 0.0;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  X.fetch(K, 0, i0, tid, rx);
  Y.fetch(K, 0, j0, tid, ry);
  for (int k0 = 0; k0 < K; k0 += FT_KC) {
    OX::stash(lx, tid, rx);
    OY::stash(ly, tid, ry);
    __syncthreads();
    if (k0 + FT_KC < K) {
      X.fetch(K, k0 + FT_KC, i0, tid, rx);
      Y.fetch(K, k0 + FT_KC, j0, tid, ry);
    }
    if (SUMS && tid < 64) {  // (wave 0 alone)
#pragma unroll
      for (int k = 0; k < FT_KC; ++k) colsum += ly[k * FT_LDW + tid];
    }
#pragma unroll
    for (int kk = 0; kk < FT_KC; kk += 4) {
      const int kr = (kk + (lane >> 4)) * FT_LDW + (lane & 15);
      const double a0 = lx[kr + wm], a1 = lx[kr + wm + 16], b0 = ly[kr + wn], b1 = ly[kr + wn + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  return colsum;
}
