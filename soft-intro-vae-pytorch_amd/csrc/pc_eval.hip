// The 3-D variant's set-to-set evaluation (reference: soft_intro_vae_3d/README.md:47-48 and
// evaluation/generate_data_for_metrics.py, whose arrays go to the minimum-matching-distance and coverage functions): the
// all-pairs Chamfer matrix D[s][r] = CD(sample_s, ref_r) of two sets of clouds, and the row / column minima of such a
// matrix with their indices; for 1-nearest-neighbour accuracy, the matrix of one set against itself (its upper triangle,
// mirrored) and the leave-one-out nearest neighbour over the union of the two sets.  VALU / LDS only: no MFMA (K = 3 and the expanded form cancels, DESIGN.md "Point clouds"), no
// global floating-point atomics, no grid barrier, no nearest-neighbour indices.  Minima are taken on the bit patterns of
// the distances as unsigned integers: a direct-form distance is +0, positive, +inf or a NaN, for which the unsigned order
// is the float order with every NaN above +inf — an integer minimum starting at +inf drops NaNs and is independent of
// the order.  Sums have a fixed shape in fp64 (lane partials, wave butterfly, waves in index order): two runs are
// bit-identical.
#include "common.h"

#define PE_NT 256                      // threads per block
#define PE_QPL 8                       // query points a lane keeps in registers (4 pairs for the packed fp32 forms)
#define PE_QCHUNK (PE_NT * PE_QPL)     // 2048 query points per register set
#define PE_CHUNK 1024                  // reference points staged in LDS at a time (16 KB of float4 + 20 KB of minima)
#define PE_MAX_BLOCKS 2048             // a block walks the cloud pairs blockIdx.x, + gridDim.x, ...
#define PE_INF 0x7f800000u
#ifndef PE_PACKED
#define PE_PACKED 1  // 0 (with -fno-slp-vectorize): the distance arithmetic in scalar fp32 operations, for the A/B in DESIGN.md
#endif

typedef float pe_f32x2 __attribute__((ext_vector_type(2)));

struct PeArgs {
  const float* a;  // sample clouds
  long long as, an, ac;
  const float* b;  // reference clouds
  long long bs, bn, bc;
  float* D;
  unsigned* ws;
  int s0, rows, R, M, N, normalize, use_sqrt;
};

// minimum over the wave, valid in LANE 63 ONLY: quad butterflies, the two row mirrors, row_bcast15 into rows 1 and 3,
// row_bcast31 into rows 2 and 3.  A lane without a source takes the minimum's identity (old = all ones, which lets the
// compiler fold the move into a v_min_u32_dpp).  Whole wave active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned pe_dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned pe_wave_min_hi(unsigned v) {
  v = min(v, pe_dpp<0xB1, 0xf>(v));   // quad_perm [1,0,3,2]
  v = min(v, pe_dpp<0x4E, 0xf>(v));   // quad_perm [2,3,0,1]
  v = min(v, pe_dpp<0x141, 0xf>(v));  // row_half_mirror
  v = min(v, pe_dpp<0x140, 0xf>(v));  // row_mirror
  v = min(v, pe_dpp<0x142, 0xa>(v));  // row_bcast15
  v = min(v, pe_dpp<0x143, 0xc>(v));  // row_bcast31
  return v;
}

// one reference point against the lane's 2 NP query points, each distance computed ONCE: it enters the query's row
// minimum and the point's column minimum -> the lane's share of the latter.  Queries sit in pairs so that the six
// operations of a distance are three packed ones (v_pk_add / v_pk_mul / v_pk_fma_f32).
template <int NP>
__device__ __forceinline__ unsigned pe_point(const float4 g, const pe_f32x2 (&qx)[PE_QPL / 2], const pe_f32x2 (&qy)[PE_QPL / 2],
                                             const pe_f32x2 (&qz)[PE_QPL / 2], unsigned (&rmin)[PE_QPL]) {
  unsigned c = 0xffffffffu;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#if PE_PACKED
    const pe_f32x2 dx = qx[p] - g.x, dy = qy[p] - g.y, dz = qz[p] - g.z;
    pe_f32x2 d = dx * dx;
    d = __builtin_elementwise_fma(dy, dy, d);
    d = __builtin_elementwise_fma(dz, dz, d);
#else
    pe_f32x2 d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float dx = qx[p][h] - g.x, dy = qy[p][h] - g.y, dz = qz[p][h] - g.z;
      d[h] = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    }
#endif
    const unsigned u0 = __float_as_uint(d[0]), u1 = __float_as_uint(d[1]);
    rmin[2 * p] = min(rmin[2 * p], u0);
    rmin[2 * p + 1] = min(rmin[2 * p + 1], u1);
    c = min(min(c, u0), u1);
  }
  return c;
}

// cw: this wave's row of column minima, one plain store per point (four points: one 16-byte store) by lane 63
template <int NP>
__device__ __forceinline__ void pe_scan(const float4* __restrict__ tg, unsigned* __restrict__ cw, int cnt, int lane,
                                        const pe_f32x2 (&qx)[PE_QPL / 2], const pe_f32x2 (&qy)[PE_QPL / 2],
                                        const pe_f32x2 (&qz)[PE_QPL / 2], unsigned (&rmin)[PE_QPL]) {
  int t = 0;
  for (; t + 4 <= cnt; t += 4) {
    float4 g[4];
    unsigned c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = tg[t + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = pe_point<NP>(g[j], qx, qy, qz, rmin);
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = pe_wave_min_hi(c[j]);
    if (lane == 63) *reinterpret_cast<uint4*>(cw + t) = make_uint4(c[0], c[1], c[2], c[3]);
  }
  for (; t < cnt; ++t) {
    const unsigned c = pe_wave_min_hi(pe_point<NP>(tg[t], qx, qy, qz, rmin));
    if (lane == 63) cw[t] = c;
  }
}

__device__ __forceinline__ double pe_term(unsigned bits, int use_sqrt) {
  const double v = (double)__uint_as_float(bits);
  return use_sqrt ? sqrt(v) : v;
}

// One cloud pair: P (M points) against Q (N points), both read through a's strides -> CD(P, Q), in every thread.  The
// one definition of the pair's arithmetic: chamfer_matrix_kernel and chamfer_matrix_self_kernel differ only in which
// pairs they walk and where the result goes.  P's points go into registers, PE_QCHUNK at a time; Q's go through LDS,
// PE_CHUNK at a time.  Each wave leaves the column minima over ITS queries in its own LDS
// row (plain stores: a wave meets a staged point once per pass); after the pass thread t folds the four rows for the points
// t, t + 256, ... .  Row minima live in registers across the reference chunks of one query chunk.  Between the query
// chunks the folded column minima rest in LDS (acc) when the reference cloud is a single chunk, and in the block's own
// stretch of the workspace (wsb) when both clouds need several chunks; thread t alone writes and reads its entries of
// either.  Thread t sums the minima of the points t, t + 256, ... in ascending order on BOTH sides: for M = N the result
// is symmetric in (P, Q) bit for bit.
__device__ __forceinline__ float pe_pair(const PeArgs& a, const float* __restrict__ P, const float* __restrict__ Q,
                                         unsigned* __restrict__ wsb) {
  __shared__ float4 tg[PE_CHUNK];
  __shared__ __align__(16) unsigned cw[PE_NT / 64][PE_CHUNK];
  __shared__ unsigned acc[PE_CHUNK];
  __shared__ double red[2 * PE_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int M = a.M, N = a.N;
  const int nqc = (M - 1) / PE_QCHUNK + 1, ntc = (N - 1) / PE_CHUNK + 1;
  const bool spill = nqc > 1 && ntc > 1;
  double rowsum = 0.0, colsum = 0.0;
  for (int qc = 0; qc < nqc; ++qc) {
    const int q0 = qc * PE_QCHUNK;
    const int qcnt = min(PE_QCHUNK, M - q0);
    const int np = (qcnt + 2 * PE_NT - 1) / (2 * PE_NT);  // pairs of queries in use, 1 .. 4 (block-uniform)
    // query u of this lane is point q0 + u * PE_NT + tid; a slot without a point holds NaNs: all its distances are
    // NaNs, which no minimum takes
    pe_f32x2 qx[PE_QPL / 2], qy[PE_QPL / 2], qz[PE_QPL / 2];
    unsigned rmin[PE_QPL];
#pragma unroll
    for (int u = 0; u < PE_QPL; ++u) {
      const int q = q0 + u * PE_NT + tid;
      float x = NAN, y = NAN, z = NAN;
      if (q < M) {
        const float* p = P + (long long)q * a.an;
        x = p[0], y = p[a.ac], z = p[2 * a.ac];
      }
      qx[u >> 1][u & 1] = x, qy[u >> 1][u & 1] = y, qz[u >> 1][u & 1] = z;
      rmin[u] = PE_INF;
    }
    for (int tc = 0; tc < ntc; ++tc) {
      const int c0 = tc * PE_CHUNK;
      const int cnt = min(PE_CHUNK, N - c0);
      __syncthreads();  // (the previous pass's fold has read tg's minima rows)
      if (qc == 0 || ntc > 1) {  // (otherwise the reference cloud is one chunk, still staged)
        for (int t = tid; t < cnt; t += PE_NT) {
          const float* p = Q + (long long)(c0 + t) * a.bn;
          tg[t] = make_float4(p[0], p[a.bc], p[2 * a.bc], 0.f);
        }
        __syncthreads();
      }
      unsigned* mine = cw[tid >> 6];
      switch (np) {  // (block-uniform)
        case 1: pe_scan<1>(tg, mine, cnt, lane, qx, qy, qz, rmin); break;
        case 2: pe_scan<2>(tg, mine, cnt, lane, qx, qy, qz, rmin); break;
        case 3: pe_scan<3>(tg, mine, cnt, lane, qx, qy, qz, rmin); break;
        default: pe_scan<4>(tg, mine, cnt, lane, qx, qy, qz, rmin); break;
      }
      __syncthreads();  // (every wave's minima are in)
      for (int t = tid; t < cnt; t += PE_NT) {
        unsigned v = min(min(cw[0][t], cw[1][t]), min(cw[2][t], cw[3][t]));
        if (qc > 0) v = min(v, spill ? wsb[c0 + t] : acc[t]);
        if (qc == nqc - 1)
          colsum += pe_term(v, a.use_sqrt);
        else if (spill)
          wsb[c0 + t] = v;
        else
          acc[t] = v;
      }
    }
#pragma unroll
    for (int u = 0; u < PE_QPL; ++u)
      if (q0 + u * PE_NT + tid < M) rowsum += pe_term(rmin[u], a.use_sqrt);
  }
  block_sum2<PE_NT>(rowsum, colsum, red);
  const double m = a.normalize ? (double)M : 1.0, n = a.normalize ? (double)N : 1.0;
  return (float)(rowsum / m + colsum / n);
}

// this block's stretch of the workspace: N words, used only when both clouds need several chunks
__device__ __forceinline__ unsigned* pe_block_ws(const PeArgs& a) {
  return (a.M > PE_QCHUNK && a.N > PE_CHUNK) ? a.ws + (size_t)blockIdx.x * (size_t)a.N : nullptr;
}

// A block takes one cloud pair (s, r) at a time: the pairs of the rows s0 <= s < s0 + rows, in row-major order.
__global__ void __launch_bounds__(PE_NT) chamfer_matrix_kernel(PeArgs a) {
  unsigned* wsb = pe_block_ws(a);
  const long long npairs = (long long)a.rows * a.R;
  for (long long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int s = a.s0 + (int)(pair / a.R), r = (int)(pair % a.R);
    const float d = pe_pair(a, a.a + (long long)s * a.as, a.b + (long long)r * a.bs, wsb);
    if (threadIdx.x == 0) a.D[(size_t)s * a.R + r] = d;
  }
}

// A set against itself (a.b = a.a, a.R = the set's size S, a.N = a.M): only the pairs s <= r are computed, each result is
// stored to D[s][r] and D[r][s] (pe_pair is symmetric bit for bit when M = N).  The triangle is walked by FOLDED rows,
// each of S + 1 columns: folded row f is row f of the triangle (S - f pairs (f, f + c)) followed by row S - 1 - f (f + 1
// pairs) — every unit of the walk has the same length and the index arithmetic is exact.  For odd S the middle folded
// row is its own partner and has only its first S - f columns.  a.s0 / a.rows are the first folded row and their count.
__global__ void __launch_bounds__(PE_NT) chamfer_matrix_self_kernel(PeArgs a) {
  unsigned* wsb = pe_block_ws(a);
  const int S = a.R;
  const long long units = (long long)a.rows * (S + 1);
  for (long long lin = blockIdx.x; lin < units; lin += gridDim.x) {
    const int f = a.s0 + (int)(lin / (S + 1)), c = (int)(lin % (S + 1));
    int s = f, r = f + c;
    if (c >= S - f) {
      s = S - 1 - f;
      if (s == f) continue;  // (block-uniform: the middle row of an odd S, already walked)
      r = s + c - (S - f);
    }
    const float d = pe_pair(a, a.a + (long long)s * a.as, a.a + (long long)r * a.as, wsb);
    if (threadIdx.x == 0) {
      a.D[(size_t)s * S + r] = d;
      a.D[(size_t)r * S + s] = d;
    }
  }
}

static int pe_check(int rows, int R, int M, int N) {
  if (rows <= 0 || R <= 0 || M <= 0 || N <= 0) return SIVAE_ERR_SHAPE;
  if ((long long)rows * R >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

static int pe_blocks(int rows, int R) {
  const long long npairs = (long long)rows * R;
  return (int)(npairs < PE_MAX_BLOCKS ? npairs : PE_MAX_BLOCKS);
}

extern "C" size_t sivae_chamfer_matrix_workspace_bytes(int rows, int R, int M, int N) {
  if (pe_check(rows, R, M, N) != SIVAE_OK) return 0;
  if (M <= PE_QCHUNK || N <= PE_CHUNK) return 0;
  return (size_t)pe_blocks(rows, R) * (size_t)N * sizeof(unsigned);
}

extern "C" int sivae_chamfer_matrix(const float* sample, long long sample_stride_s, long long sample_stride_n,
                                    long long sample_stride_c, const float* ref, long long ref_stride_s,
                                    long long ref_stride_n, long long ref_stride_c, float* D, int S, int R, int M, int N,
                                    int s0, int s1, int normalize, int use_sqrt, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream) {
  if (!sample || !ref || !D) return SIVAE_ERR_NULL;
  if (S <= 0 || R <= 0 || M <= 0 || N <= 0 || s0 < 0 || s1 > S || s0 >= s1) return SIVAE_ERR_SHAPE;
  if ((long long)S * R >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  if ((normalize != 0 && normalize != 1) || (use_sqrt != 0 && use_sqrt != 1)) return SIVAE_ERR_MODE;
  const int rows = s1 - s0;
  if (!workspace || workspace_bytes < sivae_chamfer_matrix_workspace_bytes(rows, R, M, N)) return SIVAE_ERR_WORKSPACE;
  PeArgs a = {sample, sample_stride_s, sample_stride_n, sample_stride_c, ref, ref_stride_s, ref_stride_n, ref_stride_c, D,
              (unsigned*)workspace, s0, rows, R, M, N, normalize, use_sqrt};
  hipLaunchKernelGGL(chamfer_matrix_kernel, dim3(pe_blocks(rows, R)), dim3(PE_NT), 0, stream, a);
  return sivae_launch_status();
}

// the self form: frows folded rows of S + 1 columns each (chamfer_matrix_self_kernel)
static int pe_self_check(int frows, int S, int M) {
  if (frows <= 0 || S <= 0 || M <= 0 || frows > (S + 1) / 2) return SIVAE_ERR_SHAPE;
  if ((long long)S * S >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

extern "C" size_t sivae_chamfer_matrix_self_workspace_bytes(int frows, int S, int M) {
  if (pe_self_check(frows, S, M) != SIVAE_OK) return 0;
  if (M <= PE_QCHUNK || M <= PE_CHUNK) return 0;
  return (size_t)pe_blocks(frows, S + 1) * (size_t)M * sizeof(unsigned);
}

extern "C" int sivae_chamfer_matrix_self(const float* clouds, long long stride_s, long long stride_n, long long stride_c,
                                         float* D, int S, int M, int f0, int f1, int normalize, int use_sqrt,
                                         void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!clouds || !D) return SIVAE_ERR_NULL;
  if (S <= 0 || M <= 0 || f0 < 0 || f1 > (S + 1) / 2 || f0 >= f1) return SIVAE_ERR_SHAPE;
  if ((long long)S * S >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  if ((normalize != 0 && normalize != 1) || (use_sqrt != 0 && use_sqrt != 1)) return SIVAE_ERR_MODE;
  const int frows = f1 - f0;
  if (!workspace || workspace_bytes < sivae_chamfer_matrix_self_workspace_bytes(frows, S, M)) return SIVAE_ERR_WORKSPACE;
  PeArgs a = {clouds, stride_s, stride_n, stride_c, clouds, stride_s, stride_n, stride_c, D,
              (unsigned*)workspace, f0, frows, S, M, M, normalize, use_sqrt};
  hipLaunchKernelGGL(chamfer_matrix_self_kernel, dim3(pe_blocks(frows, S + 1)), dim3(PE_NT), 0, stream, a);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ row / column minima
// One launch over D [S][R]: the first cdiv(S, 4) blocks take a row per wave (lanes walk the row in ascending order, then a
// lexicographic (value, index) butterfly), the others 64 columns each (wave w walks the rows w, w + 4, ..., the four
// partials are folded in LDS).  Strict compare on an ascending walk, the lower index among equal values across lanes: the
// lowest index wins a tie.  +inf and NaN never win; a row or column without a candidate yields (+inf, 0).
#define PM_NT 256
#define PM_NONE 0x7fffffff

__device__ __forceinline__ void pm_take(float& bv, int& bi, float v, int i) {
  if (v < bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__global__ void __launch_bounds__(PM_NT) match_min_kernel(const float* __restrict__ D, int S, int R, int row_blocks,
                                                          float* __restrict__ row_min, int* __restrict__ row_arg,
                                                          float* __restrict__ col_min, int* __restrict__ col_arg) {
  __shared__ float sv[PM_NT / 64][64];
  __shared__ int si[PM_NT / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float bv = INFINITY;
  int bi = PM_NONE;
  if ((int)blockIdx.x < row_blocks) {
    const int s = blockIdx.x * (PM_NT / 64) + wave;
    if (s >= S) return;  // (wave-uniform; no barrier on this side)
    const float* p = D + (size_t)s * R;
    for (int r = lane; r < R; r += 64) {
      const float v = p[r];
      if (v < bv) {
        bv = v;
        bi = r;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      pm_take(bv, bi, ov, oi);
    }
    if (lane == 0) {
      row_min[s] = bv;
      row_arg[s] = bi == PM_NONE ? 0 : bi;
    }
  } else {
    const int r = ((int)blockIdx.x - row_blocks) * 64 + lane;
    if (r < R) {
      for (int s = wave; s < S; s += PM_NT / 64) {
        const float v = D[(size_t)s * R + r];
        if (v < bv) {
          bv = v;
          bi = s;
        }
      }
    }
    sv[wave][lane] = bv;
    si[wave][lane] = bi;
    __syncthreads();
    if (wave == 0 && r < R) {
#pragma unroll
      for (int w = 1; w < PM_NT / 64; ++w) pm_take(bv, bi, sv[w][lane], si[w][lane]);
      col_min[r] = bv;
      col_arg[r] = bi == PM_NONE ? 0 : bi;
    }
  }
}

extern "C" int sivae_match_min(const float* D, int S, int R, float* row_min, int* row_arg, float* col_min, int* col_arg,
                               hipStream_t stream) {
  if (!D || !row_min || !row_arg || !col_min || !col_arg) return SIVAE_ERR_NULL;
  if (S <= 0 || R <= 0) return SIVAE_ERR_SHAPE;
  if ((long long)S * R >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  const int row_blocks = cdiv(S, PM_NT / 64);
  hipLaunchKernelGGL(match_min_kernel, dim3(row_blocks + cdiv(R, 64)), dim3(PM_NT), 0, stream, D, S, R, row_blocks, row_min,
                     row_arg, col_min, col_arg);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------ joint leave-one-out nearest neighbour (1-NNA)
// The T = S + R items are the samples 0 .. S - 1 and the references S .. T - 1; item t's distances are ROW t of the joint
// matrix [[Dss, Dsr], [Dsr^T, Drr]]: a stretch over the samples (a row of Dss, or a column of Dsr: stride R) and a stretch
// over the references (a row of Dsr or of Drr).  One wave per item: lanes walk u = lane, lane + 64, ... in ascending order
// with a strict compare and never look at u = t, then the (value, index) butterfly of match_min_kernel.  +inf and NaN never
// win; an item without a candidate yields (+inf, -1).  No atomics, no workspace: two runs are bit-identical.
__device__ __forceinline__ void nn1_walk(const float* __restrict__ p, size_t stride, int len, int u0, int t, int lane,
                                         float& bv, int& bi) {
  for (int k = lane; k < len; k += 64) {
    const float v = p[(size_t)k * stride];
    if (u0 + k != t && v < bv) {
      bv = v;
      bi = u0 + k;
    }
  }
}

__global__ void __launch_bounds__(PM_NT) nn1_loo_kernel(const float* __restrict__ Dss, const float* __restrict__ Dsr,
                                                        const float* __restrict__ Drr, int S, int R,
                                                        float* __restrict__ nn_val, int* __restrict__ nn_arg) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (PM_NT / 64) + (threadIdx.x >> 6);
  if (t >= S + R) return;  // (wave-uniform; the kernel has no barrier)
  float bv = INFINITY;
  int bi = PM_NONE;
  if (t < S) {
    nn1_walk(Dss + (size_t)t * S, 1, S, 0, t, lane, bv, bi);
    nn1_walk(Dsr + (size_t)t * R, 1, R, S, t, lane, bv, bi);
  } else {
    nn1_walk(Dsr + (t - S), (size_t)R, S, 0, t, lane, bv, bi);
    nn1_walk(Drr + (size_t)(t - S) * R, 1, R, S, t, lane, bv, bi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    pm_take(bv, bi, ov, oi);
  }
  if (lane == 0) {
    nn_val[t] = bv;
    nn_arg[t] = bi == PM_NONE ? -1 : bi;
  }
}

extern "C" int sivae_nn1_loo(const float* Dss, const float* Dsr, const float* Drr, int S, int R, float* nn_val, int* nn_arg,
                             hipStream_t stream) {
  if (!Dss || !Dsr || !Drr || !nn_val || !nn_arg) return SIVAE_ERR_NULL;
  if (S <= 0 || R <= 0) return SIVAE_ERR_SHAPE;
  if (((long long)S + R) * ((long long)S + R) >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  hipLaunchKernelGGL(nn1_loo_kernel, dim3(cdiv(S + R, PM_NT / 64)), dim3(PM_NT), 0, stream, Dss, Dsr, Drr, S, R, nn_val,
                     nn_arg);
  return sivae_launch_status();
}
