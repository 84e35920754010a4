// The 3-D variant's earth mover's evaluation (reference: soft_intro_vae_3d/README.md:47-48, whose arrays go to the
// minimum-matching-distance and coverage functions of the latent_3d_points notebook with use_EMD): the all-pairs matrix
// D[s][r] = EMD(left = ref_r, right = sample_s) of two sets of clouds, EMD being the cost of the approximate matching of
// Fan, Su and Guibas (include/sivae_hip.h states the ten levels).  VALU / LDS only.  Every sum of the definition runs over
// the points of ONE cloud for a point of the OTHER, so both clouds sit in LDS, every thread owns up to EM_PPL points of
// each in registers, and each of the thirty sweeps of a cloud pair is a walk of a lane's own points over the other cloud's
// staged ones in index order: no sum crosses lanes, no atomics, no workspace.  The cost total is taken in fp64 (lane
// partials, wave butterfly, waves in index order).  Two runs are bit-identical, whatever the grid, the slab or the strides.
#include "common.h"

#define EM_NT 512                      // threads per block
#define EM_PPL 8                       // points of either cloud a lane owns (4 pairs for the packed fp32 forms)
#define EM_MAX_POINTS (EM_NT * EM_PPL) // 4096 points per cloud: 2 x 64 KB of float4 in LDS
#define EM_MAX_BLOCKS 1024             // a block walks the cloud pairs blockIdx.x, + gridDim.x, ...
#define EM_LEVELS 10                   // j = 7 ... -2
#define EM_LOG2E 1.44269504088896340736f

typedef float em_f32x2 __attribute__((ext_vector_type(2)));

struct EmArgs {
  const float* a;  // sample clouds (the RIGHT side of the matching)
  long long as, an, ac;
  const float* b;  // reference clouds (the LEFT side)
  long long bs, bn, bc;
  float* D;
  int s0, rows, R, M, N, normalize;
};

// A lane's 2 NP own points against the cnt staged points st[t] = (x, y, z, s_t), in index order, with the weight
// w = exp2(c d2) = exp(level d2) of each point pair recomputed from the direct-form distance (three packed subtractions,
// a packed multiply, two packed FMAs, a packed multiply by c, one v_exp_f32 per weight):
//   a0[u] += w s_t                                             (COST = false: steps 1 and 2)
//   t = (w o[u]) s_t;  a0[u] += t;  a1[u] += t sqrt(d2)        (COST = true: step 3, o = the own points' ratioL)
// Step 3 forms t in the definition's order and adds the SAME rounded t to the mass and, times the distance, to the cost:
// with ratioL taken out of the sum the mass a point keeps (a difference of nearly equal numbers for a cloud against
// itself) came out 1e-5 off.
template <int NP, bool COST>
__device__ __forceinline__ void em_sweep(const float4* __restrict__ st, int cnt, float c, const em_f32x2 (&qx)[EM_PPL / 2],
                                         const em_f32x2 (&qy)[EM_PPL / 2], const em_f32x2 (&qz)[EM_PPL / 2],
                                         const em_f32x2 (&o)[EM_PPL / 2], em_f32x2 (&a0)[EM_PPL / 2],
                                         em_f32x2 (&a1)[EM_PPL / 2]) {
#pragma unroll
  for (int p = 0; p < EM_PPL / 2; ++p) a0[p] = a1[p] = em_f32x2{0.f, 0.f};
#pragma unroll 2
  for (int t = 0; t < cnt; ++t) {
    const float4 g = st[t];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const em_f32x2 dx = qx[p] - g.x, dy = qy[p] - g.y, dz = qz[p] - g.z;
      em_f32x2 d = dx * dx;
      d = __builtin_elementwise_fma(dy, dy, d);
      d = __builtin_elementwise_fma(dz, dz, d);
      const em_f32x2 e = d * c;
      em_f32x2 w;
      w[0] = __builtin_amdgcn_exp2f(e[0]);
      w[1] = __builtin_amdgcn_exp2f(e[1]);
      if (COST) {
#pragma clang fp contract(off)  // (t is rounded once, before it is used twice)
        const em_f32x2 u = (w * o[p]) * g.w;
        em_f32x2 q;
        q[0] = __builtin_amdgcn_sqrtf(d[0]);
        q[1] = __builtin_amdgcn_sqrtf(d[1]);
        a0[p] += u;
        a1[p] = __builtin_elementwise_fma(u, q, a1[p]);
      } else {
        a0[p] = __builtin_elementwise_fma(w, em_f32x2{g.w, g.w}, a0[p]);
      }
    }
  }
}

template <bool COST>
__device__ __forceinline__ void em_sweep_np(int np, const float4* __restrict__ st, int cnt, float c,
                                            const em_f32x2 (&qx)[EM_PPL / 2], const em_f32x2 (&qy)[EM_PPL / 2],
                                            const em_f32x2 (&qz)[EM_PPL / 2], const em_f32x2 (&o)[EM_PPL / 2],
                                            em_f32x2 (&a0)[EM_PPL / 2], em_f32x2 (&a1)[EM_PPL / 2]) {
  switch (np) {  // (block-uniform)
    case 1: em_sweep<1, COST>(st, cnt, c, qx, qy, qz, o, a0, a1); break;
    case 2: em_sweep<2, COST>(st, cnt, c, qx, qy, qz, o, a0, a1); break;
    case 3: em_sweep<3, COST>(st, cnt, c, qx, qy, qz, o, a0, a1); break;
    default: em_sweep<4, COST>(st, cnt, c, qx, qy, qz, o, a0, a1); break;
  }
}

// cloud P (cnt points, element strides sn / sc) -> st[i] = (x, y, z, w0), thread tid staging the points i = u EM_NT + tid;
// returns whether one of them has a coordinate that is not finite
__device__ __forceinline__ bool em_stage(const float* __restrict__ P, long long sn, long long sc, int cnt, float w0,
                                         float4* __restrict__ st, int tid) {
  bool bad = false;
#pragma unroll
  for (int u = 0; u < EM_PPL; ++u) {
    const int i = u * EM_NT + tid;
    if (i < cnt) {
      const float* p = P + (long long)i * sn;
      const float x = p[0], y = p[sc], z = p[2 * sc];
      bad |= !(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY);  // (false for a NaN too)
      st[i] = make_float4(x, y, z, w0);
    }
  }
  return bad;
}

// the lane's own points i = u EM_NT + tid of a staged cloud, in pairs (a slot without a point holds zeros; what it
// accumulates is never used)
__device__ __forceinline__ void em_own(const float4* __restrict__ st, int cnt, int tid, em_f32x2 (&qx)[EM_PPL / 2],
                                       em_f32x2 (&qy)[EM_PPL / 2], em_f32x2 (&qz)[EM_PPL / 2]) {
#pragma unroll
  for (int u = 0; u < EM_PPL; ++u) {
    const int i = u * EM_NT + tid;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < cnt) g = st[i];
    qx[u >> 1][u & 1] = g.x, qy[u >> 1][u & 1] = g.y, qz[u >> 1][u & 1] = g.z;
  }
}

// A block takes one cloud pair (s, r) at a time.  LA holds the left (reference) cloud with ratioL in .w, LB the right
// (sample) cloud with remR (steps 1, 2) or ratioR (step 3) in .w; a thread alone writes the .w of its own points, between
// barriers.  remL, ratioL, remR of a thread's own points stay in registers over the ten levels; their coordinates are
// read back from LDS before each sweep (holding both clouds' would cost the second block of a compute unit).
// (EM_NT, 4): at most 128 VGPRs, so that two blocks share a compute unit at 2048 + 2048 points (64 KB of LDS each).
__global__ void __launch_bounds__(EM_NT, 4) emd_matrix_kernel(EmArgs a) {
  extern __shared__ __align__(16) unsigned char em_lds[];
  __shared__ double red[EM_NT / 64];
  const int tid = threadIdx.x;
  const int n = a.N, m = a.M;  // left, right
  float4* LA = reinterpret_cast<float4*>(em_lds);
  float4* LB = LA + n;
  const int npl = (n + 2 * EM_NT - 1) / (2 * EM_NT), npr = (m + 2 * EM_NT - 1) / (2 * EM_NT);  // pairs in use, 1 .. 4
  const float big = (float)max(n, m);
  const float remL0 = big / (float)n, remR0 = big / (float)m;
  const long long npairs = (long long)a.rows * a.R;
  for (long long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int s = a.s0 + (int)(pair / a.R), r = (int)(pair % a.R);
    // (the previous pair's last sweep is behind the barriers of its block_sum)
    const bool badl = em_stage(a.b + (long long)r * a.bs, a.bn, a.bc, n, 0.f, LA, tid);
    const bool badr = em_stage(a.a + (long long)s * a.as, a.an, a.ac, m, remR0, LB, tid);
    if (__syncthreads_or(badl || badr)) {  // (also the barrier behind the staging)
      // a NaN or infinite coordinate: said outright, v_max_f32 would turn a NaN remainder into a zero
      if (tid == 0) a.D[(size_t)s * a.R + r] = NAN;
      continue;
    }
    float remL[EM_PPL], remR[EM_PPL];
    em_f32x2 ratioL[EM_PPL / 2];
#pragma unroll
    for (int u = 0; u < EM_PPL; ++u) remL[u] = remL0, remR[u] = remR0, ratioL[u >> 1][u & 1] = 0.f;
    double cost = 0.0;
    em_f32x2 qx[EM_PPL / 2], qy[EM_PPL / 2], qz[EM_PPL / 2], a0[EM_PPL / 2], a1[EM_PPL / 2];
    for (int lv = 0; lv < EM_LEVELS; ++lv) {
      // level = -4^j, j = 7 - lv, and 0 at the last; c = level log2(e) (the power of four scales it exactly)
      const float c = lv == EM_LEVELS - 1 ? 0.f : -ldexpf(EM_LOG2E, 2 * (7 - lv));
      // 1. suml[k] = 1e-9 + sum_l w remR[l], ratioL[k] = remL[k] / suml[k]
      em_own(LA, n, tid, qx, qy, qz);
      em_sweep_np<false>(npl, LB, m, c, qx, qy, qz, ratioL, a0, a1);
#pragma unroll
      for (int u = 0; u < EM_PPL; ++u) {
        const int k = u * EM_NT + tid;
        if (k < n) {
          ratioL[u >> 1][u & 1] = remL[u] / (1e-9f + a0[u >> 1][u & 1]);
          LA[k].w = ratioL[u >> 1][u & 1];
        }
      }
      __syncthreads();
      // 2. sumr[l] = remR[l] sum_k w ratioL[k], ratioR[l] = remR[l] min(remR[l] / (sumr[l] + 1e-9), 1), remR[l] -= sumr[l]
      em_own(LB, m, tid, qx, qy, qz);
      em_sweep_np<false>(npr, LA, n, c, qx, qy, qz, ratioL, a0, a1);
#pragma unroll
      for (int u = 0; u < EM_PPL; ++u) {
        const int l = u * EM_NT + tid;
        if (l < m) {
          const float sumr = remR[u] * a0[u >> 1][u & 1];
          LB[l].w = remR[u] * fminf(remR[u] / (sumr + 1e-9f), 1.f);
          remR[u] = fmaxf(0.f, remR[u] - sumr);
        }
      }
      __syncthreads();
      // 3. t = w ratioL[k] ratioR[l]: cost += sum t sqrt(d2), remL[k] -= sum_l t
      em_own(LA, n, tid, qx, qy, qz);
      em_sweep_np<true>(npl, LB, m, c, qx, qy, qz, ratioL, a0, a1);
#pragma unroll
      for (int u = 0; u < EM_PPL; ++u) {
        if (u * EM_NT + tid < n) {
          cost += (double)a1[u >> 1][u & 1];
          remL[u] = fmaxf(0.f, remL[u] - a0[u >> 1][u & 1]);
        }
      }
      __syncthreads();  // (every sweep over ratioR is done)
#pragma unroll
      for (int u = 0; u < EM_PPL; ++u) {
        const int l = u * EM_NT + tid;
        if (l < m) LB[l].w = remR[u];
      }
      __syncthreads();
    }
    cost = block_sum<EM_NT>(cost, red);
    if (tid == 0) a.D[(size_t)s * a.R + r] = (float)(a.normalize ? cost / (double)big : cost);
  }
}

// both clouds and every per-point state fit LDS and registers at any admitted size: no workspace is used
extern "C" size_t sivae_emd_matrix_workspace_bytes(int /*rows*/, int /*R*/, int /*M*/, int /*N*/) { return 0; }

extern "C" int sivae_emd_matrix(const float* sample, long long sample_stride_s, long long sample_stride_n,
                                long long sample_stride_c, const float* ref, long long ref_stride_s, long long ref_stride_n,
                                long long ref_stride_c, float* D, int S, int R, int M, int N, int s0, int s1, int normalize,
                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!sample || !ref || !D) return SIVAE_ERR_NULL;
  if (S <= 0 || R <= 0 || M <= 0 || N <= 0 || s0 < 0 || s1 > S || s0 >= s1) return SIVAE_ERR_SHAPE;
  if ((long long)S * R >= 0x7fffffffLL || M > EM_MAX_POINTS || N > EM_MAX_POINTS) return SIVAE_ERR_RANGE;
  if (normalize != 0 && normalize != 1) return SIVAE_ERR_MODE;
  const int rows = s1 - s0;
  if (!workspace || workspace_bytes < sivae_emd_matrix_workspace_bytes(rows, R, M, N)) return SIVAE_ERR_WORKSPACE;
  EmArgs a = {sample, sample_stride_s, sample_stride_n, sample_stride_c, ref, ref_stride_s, ref_stride_n, ref_stride_c, D,
              s0, rows, R, M, N, normalize};
  const size_t lds = (size_t)(M + N) * sizeof(float4);  // <= 128 KB
  static size_t lds_hwm = 0;
  const int rc_lds = sivae_ensure_lds(reinterpret_cast<const void*>(emd_matrix_kernel), lds, &lds_hwm);
  if (rc_lds != SIVAE_OK) return rc_lds;
  const long long npairs = (long long)rows * R;
  hipLaunchKernelGGL(emd_matrix_kernel, dim3((unsigned)(npairs < EM_MAX_BLOCKS ? npairs : EM_MAX_BLOCKS)), dim3(EM_NT), lds,
                     stream, a);
  return sivae_launch_status();
}
