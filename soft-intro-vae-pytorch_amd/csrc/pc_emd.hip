// The 3-D variant's earth mover's evaluation (reference: soft_intro_vae_3d/README.md:47-48, whose arrays go to the
// minimum-matching-distance and coverage functions of the latent_3d_points notebook with use_EMD): the all-pairs matrix
// D[s][r] = EMD(left = ref_r, right = sample_s) of two sets of clouds, EMD being the cost of the approximate matching of
// Fan, Su and Guibas (include/sivae_hip.h states the ten levels), and the same quantity as a reconstruction loss
// (reference: soft_intro_vae_3d/train_soft_intro_vae_3d.py:171-176, 'earth_mover'): cost[b] = EMD(left_b, right_b) of a
// batch of cloud pairs with matchcostgrad's gradients.  VALU / LDS only.  Every sum of the definition runs over
// the points of ONE cloud for a point of the OTHER, so both clouds sit in LDS, every thread owns up to EM_PPL points of
// each in registers, and each of the thirty sweeps of a cloud pair is a walk of a lane's own points over the other cloud's
// staged ones in index order: no sum crosses lanes, no atomics, no workspace.  The cost total is taken in fp64 (lane
// partials, wave butterfly, waves in index order).  Two runs are bit-identical, whatever the grid, the slab or the strides.
// One pair body (em_pair) serves both kernels, which only decide which pairs to walk and where the results go.
#include <cfloat>

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

// three sums per own point: a gradient row of each of a lane's points
struct EmGrad {
  em_f32x2 x[EM_PPL / 2], y[EM_PPL / 2], z[EM_PPL / 2];
};

enum { EM_SUM, EM_COST, EM_COST_GRAD, EM_GRAD };

// A lane's 2 NP own points against the cnt staged points st[t] = (x, y, z, s_t), in index order, with the weight
// w = exp2(c d2) = exp(level d2) of each point pair recomputed from the direct-form distance (three packed subtractions,
// a packed multiply, two packed FMAs, a packed multiply by c, one v_exp_f32 per weight):
//   a0[u] += w s_t                                             (EM_SUM: steps 1 and 2)
//   t = (w o[u]) s_t;  a0[u] += t;  a1[u] += t sqrt(d2)        (EM_COST: step 3, o = the own points' ratioL)
//   ... and g[u] += (t / sqrt(d2)) (own - staged)              (EM_COST_GRAD: step 3 with the left gradient)
//   t = (w s_t) o[u];  g[u] += (t / sqrt(d2)) (own - staged)   (EM_GRAD: the right gradient's sweep, own l over staged k
//                                                               with s_t = ratioL[k], o = the own points' ratioR)
// Step 3 forms t in the definition's order and adds the SAME rounded t to the mass and, times the distance, to the cost:
// with ratioL taken out of the sum the mass a point keeps (a difference of nearly equal numbers for a cloud against
// itself) came out 1e-5 off.  EM_GRAD forms the same t: d2 is the same bits from either side (the differences only change
// sign), and the product takes ratioL first, as step 3 does.  The reciprocal root is taken of max(d2, FLT_MIN), the
// original's max(d, 1e-20): where d2 == 0 the difference is zero and the pair contributes exactly zero; a denormal d2
// (which v_rsq_f32 would read as zero) contributes something finite.
template <int NP, int MODE, int UNR>
__device__ __forceinline__ void em_sweep(const float4* __restrict__ st, int cnt, float c, const em_f32x2 (&qx)[EM_PPL / 2],
                                         const em_f32x2 (&qy)[EM_PPL / 2], const em_f32x2 (&qz)[EM_PPL / 2],
                                         const em_f32x2 (&o)[EM_PPL / 2], em_f32x2 (&a0)[EM_PPL / 2],
                                         em_f32x2 (&a1)[EM_PPL / 2], EmGrad& gr) {
  if (MODE != EM_GRAD) {
#pragma unroll
    for (int p = 0; p < EM_PPL / 2; ++p) a0[p] = a1[p] = em_f32x2{0.f, 0.f};
  }
  if (MODE == EM_COST_GRAD || MODE == EM_GRAD) {
#pragma unroll
    for (int p = 0; p < EM_PPL / 2; ++p) gr.x[p] = gr.y[p] = gr.z[p] = em_f32x2{0.f, 0.f};
  }
#pragma unroll UNR
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
      if (MODE != EM_SUM) {
#pragma clang fp contract(off)  // (t is rounded once, before it is used twice)
        const em_f32x2 u = MODE == EM_GRAD ? (w * g.w) * o[p] : (w * o[p]) * g.w;
        if (MODE != EM_GRAD) {
          em_f32x2 q;
          q[0] = __builtin_amdgcn_sqrtf(d[0]);
          q[1] = __builtin_amdgcn_sqrtf(d[1]);
          a0[p] += u;
          a1[p] = __builtin_elementwise_fma(u, q, a1[p]);
        }
        if (MODE != EM_COST) {
          em_f32x2 i;
          i[0] = __builtin_amdgcn_rsqf(__builtin_fmaxf(d[0], FLT_MIN));
          i[1] = __builtin_amdgcn_rsqf(__builtin_fmaxf(d[1], FLT_MIN));
          const em_f32x2 ui = u * i;
          gr.x[p] = __builtin_elementwise_fma(ui, dx, gr.x[p]);
          gr.y[p] = __builtin_elementwise_fma(ui, dy, gr.y[p]);
          gr.z[p] = __builtin_elementwise_fma(ui, dz, gr.z[p]);
        }
      } else {
        a0[p] = __builtin_elementwise_fma(w, em_f32x2{g.w, g.w}, a0[p]);
      }
    }
  }
}

template <int MODE, int UNR = 2>
__device__ __forceinline__ void em_sweep_np(int np, const float4* __restrict__ st, int cnt, float c,
                                            const em_f32x2 (&qx)[EM_PPL / 2], const em_f32x2 (&qy)[EM_PPL / 2],
                                            const em_f32x2 (&qz)[EM_PPL / 2], const em_f32x2 (&o)[EM_PPL / 2],
                                            em_f32x2 (&a0)[EM_PPL / 2], em_f32x2 (&a1)[EM_PPL / 2], EmGrad& gr) {
  switch (np) {  // (block-uniform)
    case 1: em_sweep<1, MODE, UNR>(st, cnt, c, qx, qy, qz, o, a0, a1, gr); break;
    case 2: em_sweep<2, MODE, UNR>(st, cnt, c, qx, qy, qz, o, a0, a1, gr); break;
    case 3: em_sweep<3, MODE, UNR>(st, cnt, c, qx, qy, qz, o, a0, a1, gr); break;
    default: em_sweep<4, MODE, UNR>(st, cnt, c, qx, qy, qz, o, a0, a1, gr); break;
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

// ... and their .w (zero for a slot without a point)
__device__ __forceinline__ void em_own_w(const float4* __restrict__ st, int cnt, int tid, em_f32x2 (&o)[EM_PPL / 2]) {
#pragma unroll
  for (int u = 0; u < EM_PPL; ++u) {
    const int i = u * EM_NT + tid;
    o[u >> 1][u & 1] = i < cnt ? st[i].w : 0.f;
  }
}

// One cloud pair: the left cloud L (n points) against the right cloud R (m points) -> false when a coordinate is NaN
// or infinite (block-uniform; nothing else is computed then), else true with the unnormalised cost in `total` (every
// thread) and, where wanted, the unnormalised gradient rows of the thread's own points k, l = u EM_NT + tid in GL / GR.
// LA holds the left cloud with ratioL in .w, LB the right cloud with remR (steps 1, 2) or ratioR (step 3 and the right
// gradient's sweep) in .w; a thread alone writes the .w of its own points, between barriers.  remL, ratioL, remR of a
// thread's own points stay in registers over the ten levels; their coordinates are read back from LDS before each sweep
// (holding both clouds' would cost the second block of a compute unit).  A gradient row is summed per level in fp32 in
// index order (by the step-3 sweep for the left side, by a fourth sweep, own l over staged k, for the right side), and
// the levels are added in level order.  The cost's arithmetic does not depend on WL / WR.  The masses and the register-pair
// counts are worked out here, per pair, not once in the kernel: measured, the matrix kernel is 0.9 % faster that way than
// with them passed in (same instructions in the sweeps, another register assignment).
template <bool WL, bool WR>
__device__ __forceinline__ bool em_pair(const int n, const int m, const int tid, float4* LA, float4* LB, double* red,
                                        const float* L, long long ln, long long lc, const float* R, long long rn,
                                        long long rc, double& total, EmGrad& GL, EmGrad& GR) {
  const int npl = (n + 2 * EM_NT - 1) / (2 * EM_NT), npr = (m + 2 * EM_NT - 1) / (2 * EM_NT);  // pairs in use, 1 .. 4
  const float big = (float)max(n, m);
  const float remL0 = big / (float)n, remR0 = big / (float)m;
  // (the previous pair's last sweep is behind the barriers of its block_sum)
  const bool badl = em_stage(L, ln, lc, n, 0.f, LA, tid);
  const bool badr = em_stage(R, rn, rc, m, remR0, LB, tid);
  // (also the barrier behind the staging)  a NaN or infinite coordinate is said outright by the caller: v_max_f32 would
  // turn a NaN remainder into a zero
  if (__syncthreads_or(badl || badr)) return false;
  float remL[EM_PPL], remR[EM_PPL];
  em_f32x2 ratioL[EM_PPL / 2];
#pragma unroll
  for (int u = 0; u < EM_PPL; ++u) remL[u] = remL0, remR[u] = remR0, ratioL[u >> 1][u & 1] = 0.f;
  if (WL) {
#pragma unroll
    for (int p = 0; p < EM_PPL / 2; ++p) GL.x[p] = GL.y[p] = GL.z[p] = em_f32x2{0.f, 0.f};
  }
  if (WR) {
#pragma unroll
    for (int p = 0; p < EM_PPL / 2; ++p) GR.x[p] = GR.y[p] = GR.z[p] = em_f32x2{0.f, 0.f};
  }
  double cost = 0.0;
  em_f32x2 qx[EM_PPL / 2], qy[EM_PPL / 2], qz[EM_PPL / 2], a0[EM_PPL / 2], a1[EM_PPL / 2];
  EmGrad gl;  // one level's sums
  for (int lv = 0; lv < EM_LEVELS; ++lv) {
    // level = -4^j, j = 7 - lv, and 0 at the last; c = level log2(e) (the power of four scales it exactly)
    const float c = lv == EM_LEVELS - 1 ? 0.f : -ldexpf(EM_LOG2E, 2 * (7 - lv));
    // 1. suml[k] = 1e-9 + sum_l w remR[l], ratioL[k] = remL[k] / suml[k]
    em_own(LA, n, tid, qx, qy, qz);
    em_sweep_np<EM_SUM>(npl, LB, m, c, qx, qy, qz, ratioL, a0, a1, gl);
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
    em_sweep_np<EM_SUM>(npr, LA, n, c, qx, qy, qz, ratioL, a0, a1, gl);
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
    em_sweep_np<WL ? EM_COST_GRAD : EM_COST, WL && WR ? 1 : 2>(npl, LB, m, c, qx, qy, qz, ratioL, a0, a1, gl);
#pragma unroll
    for (int u = 0; u < EM_PPL; ++u) {
      if (u * EM_NT + tid < n) {
        cost += (double)a1[u >> 1][u & 1];
        remL[u] = fmaxf(0.f, remL[u] - a0[u >> 1][u & 1]);
      }
    }
    if (WL) {
#pragma unroll
      for (int p = 0; p < EM_PPL / 2; ++p) GL.x[p] += gl.x[p], GL.y[p] += gl.y[p], GL.z[p] += gl.z[p];
    }
    if (WR) {
      // the same t from the other side: own l (ratioR read back from the lane's own .w) over staged k (ratioL in .w)
      em_f32x2 ratioR[EM_PPL / 2];
      em_own(LB, m, tid, qx, qy, qz);
      em_own_w(LB, m, tid, ratioR);
      em_sweep_np<EM_GRAD, WL ? 1 : 2>(npr, LA, n, c, qx, qy, qz, ratioR, a0, a1, gl);
#pragma unroll
      for (int p = 0; p < EM_PPL / 2; ++p) GR.x[p] += gl.x[p], GR.y[p] += gl.y[p], GR.z[p] += gl.z[p];
    }
    __syncthreads();  // (every sweep over ratioR is done)
#pragma unroll
    for (int u = 0; u < EM_PPL; ++u) {
      const int l = u * EM_NT + tid;
      if (l < m) LB[l].w = remR[u];
    }
    __syncthreads();
  }
  total = block_sum<EM_NT>(cost, red);
  return true;
}

// A block takes one cloud pair (s, r) at a time.
// (EM_NT, 4): at most 128 VGPRs, so that two blocks share a compute unit at 2048 + 2048 points (64 KB of LDS each).
__global__ void __launch_bounds__(EM_NT, 4) emd_matrix_kernel(EmArgs a) {
  extern __shared__ __align__(16) unsigned char em_lds[];
  __shared__ double red[EM_NT / 64];
  const int tid = threadIdx.x;
  const int n = a.N, m = a.M;  // left, right
  float4* LA = reinterpret_cast<float4*>(em_lds);
  float4* LB = LA + n;
  const float big = (float)max(n, m);
  const long long npairs = (long long)a.rows * a.R;
  for (long long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int s = a.s0 + (int)(pair / a.R), r = (int)(pair % a.R);
    double cost;
    EmGrad none;
    const bool ok = em_pair<false, false>(n, m, tid, LA, LB, red, a.b + (long long)r * a.bs, a.bn, a.bc,
                                          a.a + (long long)s * a.as, a.an, a.ac, cost, none, none);
    if (!ok) {  // (block-uniform)
      if (tid == 0) a.D[(size_t)s * a.R + r] = NAN;
      continue;
    }
    if (tid == 0) a.D[(size_t)s * a.R + r] = (float)(a.normalize ? cost / (double)big : cost);
  }
}

struct EmLossArgs {
  const float* l;  // left clouds [B] x N points
  long long ls, ln, lc;
  const float* r;  // right clouds [B] x M points
  long long rs, rn, rc;
  float* cost;     // [B]
  float* dl;       // [B][N][3], used when WL
  float* dr;       // [B][M][3], used when WR
  int B, N, M, normalize;
};

// the gradient rows of a thread's own points, divided by big when normalised; NaN throughout for a pair refused
__device__ __forceinline__ void em_store_grad(float* __restrict__ g, int cnt, int tid, const EmGrad& G, bool ok, bool normalize,
                                              float big) {
#pragma unroll
  for (int u = 0; u < EM_PPL; ++u) {
    const int i = u * EM_NT + tid;
    if (i < cnt) {
      float x = NAN, y = NAN, z = NAN;
      if (ok) {  // (block-uniform; G holds nothing otherwise)
        x = G.x[u >> 1][u & 1], y = G.y[u >> 1][u & 1], z = G.z[u >> 1][u & 1];
        if (normalize) x /= big, y /= big, z /= big;
      }
      g[3 * (size_t)i] = x, g[3 * (size_t)i + 1] = y, g[3 * (size_t)i + 2] = z;
    }
  }
}

// A block takes the cloud pair b of the batch, then b + gridDim.x, ...
// (EM_NT, 2): up to 256 VGPRs, one block to a compute unit.  The per-level sums (24 registers) and the two sides' running
// rows (24 each) do not fit next to the matrix kernel's 127 under 128; a training batch is 32 - 64 pairs on 256 compute
// units, where a second resident block buys nothing, and with the rows in registers every output element is written
// once, by its owner, with no read-modify-write of global memory between the levels.
template <bool WL, bool WR>
__global__ void __launch_bounds__(EM_NT, 2) emd_loss_kernel(EmLossArgs a) {
  extern __shared__ __align__(16) unsigned char em_lds[];
  __shared__ double red[EM_NT / 64];
  const int tid = threadIdx.x;
  const int n = a.N, m = a.M;  // left, right
  float4* LA = reinterpret_cast<float4*>(em_lds);
  float4* LB = LA + n;
  const float big = (float)max(n, m);
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    double cost;
    EmGrad GL, GR;
    const bool ok = em_pair<WL, WR>(n, m, tid, LA, LB, red, a.l + (long long)b * a.ls, a.ln, a.lc, a.r + (long long)b * a.rs, a.rn,
                                    a.rc, cost, GL, GR);
    if (tid == 0) a.cost[b] = !ok ? NAN : (float)(a.normalize ? cost / (double)big : cost);
    if (WL) em_store_grad(a.dl + 3 * (size_t)b * n, n, tid, GL, ok, a.normalize != 0, big);
    if (WR) em_store_grad(a.dr + 3 * (size_t)b * m, m, tid, GR, ok, a.normalize != 0, big);
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

template <bool WL, bool WR>
static int em_launch_loss(const EmLossArgs& a, hipStream_t stream) {
  const size_t lds = (size_t)(a.M + a.N) * sizeof(float4);  // <= 128 KB
  static size_t lds_hwm = 0;                                // (one per instantiation, as the attribute is)
  const int rc_lds = sivae_ensure_lds(reinterpret_cast<const void*>(emd_loss_kernel<WL, WR>), lds, &lds_hwm);
  if (rc_lds != SIVAE_OK) return rc_lds;
  hipLaunchKernelGGL((emd_loss_kernel<WL, WR>), dim3((unsigned)(a.B < EM_MAX_BLOCKS ? a.B : EM_MAX_BLOCKS)), dim3(EM_NT), lds,
                     stream, a);
  return sivae_launch_status();
}

extern "C" size_t sivae_emd_loss_workspace_bytes(int /*B*/, int /*N*/, int /*M*/) { return 0; }

extern "C" int sivae_emd_loss(const float* left, long long left_stride_b, long long left_stride_n, long long left_stride_c,
                              const float* right, long long right_stride_b, long long right_stride_n,
                              long long right_stride_c, float* cost, float* dleft, float* dright, int B, int N, int M,
                              int normalize, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!left || !right || !cost) return SIVAE_ERR_NULL;
  if (B <= 0 || N <= 0 || M <= 0) return SIVAE_ERR_SHAPE;
  if (N > EM_MAX_POINTS || M > EM_MAX_POINTS || 3LL * B * (N > M ? N : M) >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  if (normalize != 0 && normalize != 1) return SIVAE_ERR_MODE;
  if (!workspace || workspace_bytes < sivae_emd_loss_workspace_bytes(B, N, M)) return SIVAE_ERR_WORKSPACE;
  const EmLossArgs a = {left, left_stride_b, left_stride_n, left_stride_c, right, right_stride_b, right_stride_n,
                        right_stride_c, cost, dleft, dright, B, N, M, normalize};
  if (dleft) return dright ? em_launch_loss<true, true>(a, stream) : em_launch_loss<true, false>(a, stream);
  return dright ? em_launch_loss<false, true>(a, stream) : em_launch_loss<false, false>(a, stream);
}
