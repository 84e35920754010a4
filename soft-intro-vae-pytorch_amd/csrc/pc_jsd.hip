// The 3-D variant's validation metric (reference: soft_intro_vae_3d/metrics/jsd.py): the occupancy grid of a set of point
// clouds (nearest grid-cell centre per point, per-cell point counts and per-cell "clouds that touched it" counts), the
// voxel histogram of js_divercence_between_pc, and the Jensen-Shannon divergence of two count vectors.  The counters are
// int32 and are accumulated with vector integer atomics (LDS first, global once per block where the grid fits): integer
// sums do not depend on the order, two runs are bit-identical.  Plain HIP C++, VALU / LDS only.
#include "common.h"

#define PJ_NT 1024     // threads per block of the occupancy kernel (one block per CU: its LDS footprint is 64 KB + grid)
#define PJ_NW (PJ_NT / 64)
#define PJ_CHUNK 2048  // cell centres staged in LDS at a time (2048 x float4 = 32 KB), as chamfer_fwd_kernel does
#define PJ_FB 2048     // points waiting for the exhaustive route (2048 x float4 = 32 KB)
#define PJ_P 4         // points a wave scans the table for at a time
#define PJ_MAX_RES 64  // the cube lookup table and the LDS bitmap (G bits <= 32 KB) are sized for res <= 64
#define PJ_LDS_MAX (160 * 1024 - 512)

// ------------------------------------------------------------------------------------------------ occupancy grid
// _entropy_of_occupancy_grid (metrics/jsd.py:97-126).  A block owns whole clouds (cloud s = blockIdx.x, + gridDim.x, ...).
//
// Fast route: per axis the nearest of the res centre coordinates (rounding proposes an index, the two neighbours are
// compared by |x - a_i| on the float32 centres themselves, the lower index wins a tie); distances are separable, so this
// is the nearest cell of the full cube, and if the lookup table says that cell is in the table it is the nearest cell
// of the table.
//
// Exhaustive route: every other point is appended to an LDS list.  When the list may overflow, or the cloud ends, the
// WHOLE BLOCK scans the table for the listed points: a wave takes up to PJ_P points (round-robin over the waves, so few
// points still spread over many waves), its 64 lanes each take every 64th cell of the staged chunk, and a lexicographic
// (distance, index) butterfly picks the winner — the result of an ascending scan with a strict compare.  No lane ever
// scans alone: the cost is (listed points) x G / 1024 per lane however the listed points were spread over the lanes.
//
// HIST: per-block int32 histogram in LDS (and a 16-bit one for the per-cloud counts: a block owns <= 65535 clouds),
// flushed once with global atomics; otherwise global atomics per point.
struct PjArgs {
  const float* pcs;
  long long ss, sn, sc;
  int S, N;
  const float* cells;
  const int* lut;
  const float* axis;
  int res, G;
  int* counters;
  int* bernoulli;
  int* status;
};

template <int NP>
__device__ __forceinline__ void pj_scan_chunk(const float4* __restrict__ tg, int cnt, int c0, int lane, const float (&qx)[PJ_P],
                                              const float (&qy)[PJ_P], const float (&qz)[PJ_P], float (&best)[PJ_P],
                                              int (&bi)[PJ_P]) {
#pragma unroll 2
  for (int t = lane; t < cnt; t += 64) {
    const float4 g = tg[t];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const float dx = qx[u] - g.x, dy = qy[u] - g.y, dz = qz[u] - g.z;
      const float d = dx * dx + dy * dy + dz * dz;
      if (d < best[u]) {
        best[u] = d;
        bi[u] = c0 + t;
      }
    }
  }
}

__device__ __forceinline__ int pj_axis_index(float x, const float* __restrict__ ax, int res) {
  const float t = fminf(fmaxf((x + 0.5f) * (float)(res - 1), 0.f), (float)(res - 1));
  int i = (int)rintf(t);
  const float d0 = fabsf(x - ax[i]);
  if (i + 1 < res && fabsf(x - ax[i + 1]) < d0) return i + 1;
  if (i > 0 && fabsf(x - ax[i - 1]) <= d0) return i - 1;
  return i;
}

template <bool HIST>
__global__ void __launch_bounds__(PJ_NT) occupancy_grid_kernel(PjArgs a) {
  extern __shared__ __align__(16) unsigned char pj_smem[];
  __shared__ int nfb_s;
  const int G = a.G, res = a.res;
  const int nwords = (G + 31) >> 5;
  float4* tg = reinterpret_cast<float4*>(pj_smem);
  float4* fb = tg + PJ_CHUNK;
  float* ax = reinterpret_cast<float*>(fb + PJ_FB);
  unsigned* bitmap = reinterpret_cast<unsigned*>(ax + PJ_MAX_RES);
  int* hist = reinterpret_cast<int*>(bitmap + nwords);
  unsigned* bhist = reinterpret_cast<unsigned*>(hist + G);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool bern = a.bernoulli != nullptr;

  if (tid < res) ax[tid] = a.axis[tid];
  if (tid == 0) nfb_s = 0;
  if (HIST) {
    for (int i = tid; i < G; i += PJ_NT) hist[i] = 0;
    if (bern)
      for (int i = tid; i < (G + 1) / 2; i += PJ_NT) bhist[i] = 0u;
  }

  auto count = [&](int li) {
    if (HIST)
      atomicAdd(&hist[li], 1);
    else
      atomicAdd(&a.counters[li], 1);
    if (bern) {
      const unsigned bit = 1u << (li & 31);
      const unsigned old = atomicOr(&bitmap[li >> 5], bit);
      if (!(old & bit)) {
        if (HIST)
          atomicAdd(&bhist[li >> 1], 1u << ((li & 1) * 16));
        else
          atomicAdd(&a.bernoulli[li], 1);
      }
    }
  };

  for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
    if (bern)
      for (int i = tid; i < nwords; i += PJ_NT) bitmap[i] = 0u;
    __syncthreads();
    const float* cloud = a.pcs + (long long)s * a.ss;
    for (int p0 = 0; p0 < a.N; p0 += PJ_NT) {
      // (here nfb_s + PJ_NT <= PJ_FB: this tile's points fit the list)
      const int p = p0 + tid;
      if (p < a.N) {
        const float* q = cloud + (long long)p * a.sn;
        const float x = q[0], y = q[a.sc], z = q[2 * a.sc];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
          atomicAdd(&a.status[0], 1);
        } else {
          const int ix = pj_axis_index(x, ax, res), iy = pj_axis_index(y, ax, res), iz = pj_axis_index(z, ax, res);
          const int li = a.lut[(ix * res + iy) * res + iz];
          if ((unsigned)li < (unsigned)G) {
            count(li);
          } else {
            fb[atomicAdd(&nfb_s, 1)] = make_float4(x, y, z, 0.f);
          }
        }
      }
      __syncthreads();
      const int n = nfb_s;
      __syncthreads();  // (every thread has read n before anyone appends again)
      if (n == 0 || (p0 + PJ_NT < a.N && n + PJ_NT <= PJ_FB)) continue;  // (block-uniform)

      // ---- the exhaustive route for fb[0 .. n)
      if (tid == 0) {
        nfb_s = 0;
        atomicAdd(&a.status[1], n);
      }
      for (int g0 = 0; g0 < n; g0 += PJ_NW * PJ_P) {
        const int left = n - g0 - wave;
        const int np = left <= 0 ? 0 : min((left + PJ_NW - 1) / PJ_NW, PJ_P);
        float qx[PJ_P], qy[PJ_P], qz[PJ_P], best[PJ_P];
        int bi[PJ_P];
#pragma unroll
        for (int u = 0; u < PJ_P; ++u) {
          const float4 q = u < np ? fb[g0 + wave + PJ_NW * u] : make_float4(0.f, 0.f, 0.f, 0.f);
          qx[u] = q.x, qy[u] = q.y, qz[u] = q.z;
          best[u] = INFINITY;
          bi[u] = 0;
        }
        for (int c0 = 0; c0 < G; c0 += PJ_CHUNK) {
          const int cnt = min(PJ_CHUNK, G - c0);
          __syncthreads();
          for (int t = tid; t < cnt; t += PJ_NT) {
            const float* c = a.cells + (size_t)(c0 + t) * 3;
            tg[t] = make_float4(c[0], c[1], c[2], 0.f);
          }
          __syncthreads();
          switch (np) {  // (wave-uniform)
            case 1: pj_scan_chunk<1>(tg, cnt, c0, lane, qx, qy, qz, best, bi); break;
            case 2: pj_scan_chunk<2>(tg, cnt, c0, lane, qx, qy, qz, best, bi); break;
            case 3: pj_scan_chunk<3>(tg, cnt, c0, lane, qx, qy, qz, best, bi); break;
            case 4: pj_scan_chunk<4>(tg, cnt, c0, lane, qx, qy, qz, best, bi); break;
            default: break;
          }
        }
#pragma unroll
        for (int u = 0; u < PJ_P; ++u) {
          float b = best[u];
          int i = bi[u];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(b, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (ob < b || (ob == b && oi < i)) {
              b = ob;
              i = oi;
            }
          }
          if (lane == u && u < np) count(i);
        }
      }
      __syncthreads();  // (the list is free again, nfb_s = 0 is visible)
    }
    __syncthreads();  // (the bitmap is complete before the next cloud clears it)
  }

  if (HIST) {
    __syncthreads();
    for (int i = tid; i < G; i += PJ_NT) {
      const int v = hist[i];
      if (v) atomicAdd(&a.counters[i], v);
      if (bern) {
        const unsigned b = (bhist[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
        if (b) atomicAdd(&a.bernoulli[i], (int)b);
      }
    }
  }
}

static size_t pj_lds_bytes(int G, bool hist, bool bern) {
  size_t n = (size_t)(PJ_CHUNK + PJ_FB) * sizeof(float4) + PJ_MAX_RES * sizeof(float) + (size_t)((G + 31) / 32) * 4;
  if (hist) n += (size_t)G * 4 + (bern ? (size_t)((G + 1) / 2) * 4 : 0);
  return n;
}

extern "C" int sivae_occupancy_grid(const float* pcs, long long stride_s, long long stride_n, long long stride_c, int S, int N,
                                    const float* cells, const int* lut, const float* axis, int res, int G, int* counters,
                                    int* bernoulli, int* status, hipStream_t stream) {
  if (!pcs || !cells || !lut || !axis || !counters || !status) return SIVAE_ERR_NULL;
  if (S <= 0 || N <= 0 || G <= 0 || res < 2 || res > PJ_MAX_RES || G > res * res * res) return SIVAE_ERR_SHAPE;
  if ((long long)S * N >= 0x80000000LL) return SIVAE_ERR_RANGE;  // (an int32 counter could not hold every point)
  hipError_t e = hipMemsetAsync(counters, 0, (size_t)G * sizeof(int), stream);
  if (e == hipSuccess && bernoulli) e = hipMemsetAsync(bernoulli, 0, (size_t)G * sizeof(int), stream);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, 2 * sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  const bool hist = pj_lds_bytes(G, true, bernoulli != nullptr) <= PJ_LDS_MAX;
  const size_t lds = pj_lds_bytes(G, hist, bernoulli != nullptr);
  static size_t hw_hist = 0, hw_direct = 0;
  const int rc = hist ? sivae_ensure_lds((const void*)occupancy_grid_kernel<true>, lds, &hw_hist)
                      : sivae_ensure_lds((const void*)occupancy_grid_kernel<false>, lds, &hw_direct);
  if (rc != SIVAE_OK) return rc;
  const int cus = sivae_num_cus();
  int grid = S < cus ? S : cus;
  if (grid < cdiv(S, 65535)) grid = cdiv(S, 65535);  // (the 16-bit per-cloud histogram: <= 65535 clouds per block)
  PjArgs a = {pcs, stride_s, stride_n, stride_c, S, N, cells, lut, axis, res, G, counters, bernoulli, status};
  if (hist)
    hipLaunchKernelGGL(occupancy_grid_kernel<true>, dim3(grid), dim3(PJ_NT), lds, stream, a);
  else
    hipLaunchKernelGGL(occupancy_grid_kernel<false>, dim3(grid), dim3(PJ_NT), lds, stream, a);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ voxel histogram
// _pc_to_voxel_distribution (metrics/jsd.py:63-72): clamp(-0.5, 0.4999) + 0.5, * n, truncation, linear index.  The
// reference's fp32 operations one by one: round-to-nearest add and multiply, never contracted into an FMA (for an n that
// is no power of two the contracted form may land in another bin).  A NaN coordinate is counted and the point skipped.
__device__ __forceinline__ int pj_voxel(float x, int n) {
  const float c = fminf(fmaxf(x, -0.5f), 0.4999f);
  const int i = (int)__fmul_rn(__fadd_rn(c, 0.5f), (float)n);
  return min(max(i, 0), n - 1);  // (0.9999 n < n: the clamp only keeps a write inside the array)
}

__global__ void __launch_bounds__(256) voxel_histogram_kernel(const float* __restrict__ pc, long long ss, long long sn,
                                                              long long sc, long long total, int N, int n,
                                                              int* __restrict__ counts, int* __restrict__ status) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long s = e / N;
    const float* q = pc + s * ss + (e - s * N) * sn;
    const float x = q[0], y = q[sc], z = q[2 * sc];
    if (isnan(x) || isnan(y) || isnan(z)) {
      atomicAdd(&status[0], 1);
      continue;
    }
    atomicAdd(&counts[(pj_voxel(x, n) * n + pj_voxel(y, n)) * n + pj_voxel(z, n)], 1);
  }
}

extern "C" int sivae_voxel_histogram(const float* pc, long long stride_s, long long stride_n, long long stride_c, int S, int N,
                                     int n_voxels, int* counts, int* status, hipStream_t stream) {
  if (!pc || !counts || !status) return SIVAE_ERR_NULL;
  if (S <= 0 || N <= 0 || n_voxels <= 0) return SIVAE_ERR_SHAPE;
  if ((long long)S * N >= 0x80000000LL || (long long)n_voxels * n_voxels * n_voxels >= 0x80000000LL) return SIVAE_ERR_RANGE;
  const size_t bins = (size_t)n_voxels * n_voxels * n_voxels;
  hipError_t e = hipMemsetAsync(counts, 0, bins * sizeof(int), stream);
  if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  const long long total = (long long)S * N;
  const long long want = (total + 255) / 256;
  const int grid = (int)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(voxel_histogram_kernel, dim3(grid), dim3(256), 0, stream, pc, stride_s, stride_n, stride_c, total, N,
                     n_voxels, counts, status);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ JS divergence
// _js_divergence (metrics/jsd.py:25-42) from two count vectors, one block, fp64.  Fixed reduction shape: a thread adds its
// elements (tid, tid + 1024, ...) in ascending order, butterfly inside a wave, waves in index order.
__device__ __forceinline__ double pj_count(const void* p, int is_f64, int i) {
  return is_f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const int*>(p)[i];
}
__device__ __forceinline__ double pj_plogp(double p) { return p > 0.0 ? p * log2(p) : 0.0; }  // (0 log 0 = 0)

__global__ void __launch_bounds__(1024) js_divergence_kernel(const void* __restrict__ P, const void* __restrict__ Q, int p_f64,
                                                             int q_f64, int n, double* __restrict__ out) {
  __shared__ double red[2 * 1024 / 64];
  double sp = 0.0, sq = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    sp += pj_count(P, p_f64, i);
    sq += pj_count(Q, q_f64, i);
  }
  block_sum2<1024>(sp, sq, red);
  double e1 = 0.0, e2 = 0.0, es = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double p = pj_count(P, p_f64, i) / sp, q = pj_count(Q, q_f64, i) / sq;
    e1 -= pj_plogp(p);
    e2 -= pj_plogp(q);
    es -= pj_plogp((p + q) / 2.0);
  }
  block_sum2<1024>(e1, e2, red);
  es = block_sum<1024>(es, red);
  if (threadIdx.x == 0) {
    // (an all-zero vector: the reference divides 0 by 0 and returns NaN)
    out[0] = (sp == 0.0 || sq == 0.0 || sp != sp || sq != sq) ? (double)NAN : es - (e1 + e2) / 2.0;
  }
}

extern "C" int sivae_js_divergence(const void* P, const void* Q, int p_is_f64, int q_is_f64, int n, double* out,
                                   hipStream_t stream) {
  if (!P || !Q || !out) return SIVAE_ERR_NULL;
  if (n <= 0) return SIVAE_ERR_SHAPE;
  if ((p_is_f64 != 0 && p_is_f64 != 1) || (q_is_f64 != 0 && q_is_f64 != 1)) return SIVAE_ERR_MODE;
  hipLaunchKernelGGL(js_divergence_kernel, dim3(1), dim3(1024), 0, stream, P, Q, p_is_f64, q_is_f64, n, out);
  return sivae_launch_status();
}
