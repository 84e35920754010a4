// Point-cloud primitives of the 3-D Soft-IntroVAE (soft_intro_vae_3d): the Chamfer distance with its nearest-neighbour
// indices and gradient, ReLU -> BatchNorm1d over [B][C][N] without ever storing relu(a), and the max over points with its
// scatter gradient.  All of them are VALU / streaming kernels: no MFMA, no atomics, no grid barrier.  Every reduction has
// a fixed shape (lane partials, wave butterfly, waves in index order, slices in index order): two runs are bit-identical.
#include "common.h"

#define PC_NT 256      // threads per block of every kernel here
#define PC_CHUNK 2048  // points of the other cloud staged in LDS at a time (2048 x float4 = 32 KB)

// ------------------------------------------------------------------------------------------------ Chamfer
// blockIdx.y is the direction: 0 = every prediction looks for its nearest ground-truth point, 1 = the other way round.
// A lane owns one query point; the other cloud is staged in LDS PC_CHUNK points at a time and read as wave-uniform
// (broadcast) 16-byte reads.  The distance is the direct form dx^2 + dy^2 + dz^2: the reference's |x|^2 + |y|^2 - 2 x.y
// cancels ("Point clouds").  Ascending scan with a strict compare: the lowest index wins a tie.
__global__ void __launch_bounds__(PC_NT) chamfer_fwd_kernel(const float* __restrict__ preds, const float* __restrict__ gts,
                                                            int* __restrict__ idx_p, int* __restrict__ idx_g,
                                                            float* __restrict__ part, int M, int N, int nblk_p, int nblk_g) {
  __shared__ float4 tg[PC_CHUNK];
  __shared__ float red[PC_NT / 64];
  const int dir = blockIdx.y, b = blockIdx.z;
  const int nq = dir == 0 ? M : N, nt = dir == 0 ? N : M;
  if ((int)blockIdx.x >= (dir == 0 ? nblk_p : nblk_g)) return;  // (block-uniform, before any barrier)
  const float* Q = (dir == 0 ? preds + (size_t)b * M * 3 : gts + (size_t)b * N * 3);
  const float* T = (dir == 0 ? gts + (size_t)b * N * 3 : preds + (size_t)b * M * 3);
  const int q = blockIdx.x * PC_NT + threadIdx.x;
  const bool active = q < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = Q[(size_t)q * 3 + 0];
    qy = Q[(size_t)q * 3 + 1];
    qz = Q[(size_t)q * 3 + 2];
  }
  float best = INFINITY;
  int bi = 0;
  for (int c0 = 0; c0 < nt; c0 += PC_CHUNK) {
    const int cnt = min(PC_CHUNK, nt - c0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += PC_NT) {
      const float* p = T + (size_t)(c0 + t) * 3;
      tg[t] = make_float4(p[0], p[1], p[2], 0.f);
    }
    __syncthreads();
    int t = 0;
    for (; t + 4 <= cnt; t += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 g = tg[t + u];
        const float dx = qx - g.x, dy = qy - g.y, dz = qz - g.z;
        const float d = dx * dx + dy * dy + dz * dz;
        if (d < best) {
          best = d;
          bi = c0 + t + u;
        }
      }
    }
    for (; t < cnt; ++t) {
      const float4 g = tg[t];
      const float dx = qx - g.x, dy = qy - g.y, dz = qz - g.z;
      const float d = dx * dx + dy * dy + dz * dz;
      if (d < best) {
        best = d;
        bi = c0 + t;
      }
    }
  }
  if (active) (dir == 0 ? idx_p + (size_t)b * M : idx_g + (size_t)b * N)[q] = bi;
  // masked lanes add nothing (no padding point can win a minimum: they never enter one)
  const float s = wave_sum(active ? best : 0.f);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < PC_NT / 64; ++w) tot += red[w];
    part[(size_t)b * (nblk_p + nblk_g) + (dir == 0 ? 0 : nblk_p) + blockIdx.x] = tot;
  }
}

// loss[b] = fold of the block partials of both directions, in index order, in fp64
__global__ void __launch_bounds__(64) chamfer_fold_kernel(const float* __restrict__ part, float* __restrict__ loss, int B,
                                                          int nblk) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += (double)part[(size_t)b * nblk + i];
  loss[b] = (float)s;
}

// gradient of one side (blockIdx.y = 0: preds, 1: gts).  For its own point j a lane adds
//   (Q_j - T_nn(j))                         its own nearest neighbour, and
//   sum over i with nn_T(i) == j (Q_j - T_i) every point of the other cloud that chose j,
// the second by scanning the other side's index array (staged in LDS in the .w of the point) in ascending order — the
// scatter without atomics, O(N M) integer compares like the forward.  The result is scaled by 2 g[b].
__global__ void __launch_bounds__(PC_NT) chamfer_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ preds,
                                                            const float* __restrict__ gts, const int* __restrict__ idx_p,
                                                            const int* __restrict__ idx_g, float* __restrict__ dpreds,
                                                            float* __restrict__ dgts, int M, int N) {
  __shared__ float4 tg[PC_CHUNK];
  const int dir = blockIdx.y, b = blockIdx.z;
  float* out = dir == 0 ? dpreds : dgts;
  const int nq = dir == 0 ? M : N, nt = dir == 0 ? N : M;
  if (out == nullptr || (int)blockIdx.x * PC_NT >= nq) return;  // (block-uniform, before any barrier)
  const float* Q = (dir == 0 ? preds + (size_t)b * M * 3 : gts + (size_t)b * N * 3);
  const float* T = (dir == 0 ? gts + (size_t)b * N * 3 : preds + (size_t)b * M * 3);
  const int* iq = (dir == 0 ? idx_p + (size_t)b * M : idx_g + (size_t)b * N);
  const int* it = (dir == 0 ? idx_g + (size_t)b * N : idx_p + (size_t)b * M);
  const int q = blockIdx.x * PC_NT + threadIdx.x;
  const bool active = q < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
  if (active) {
    qx = Q[(size_t)q * 3 + 0];
    qy = Q[(size_t)q * 3 + 1];
    qz = Q[(size_t)q * 3 + 2];
    const int a = min(max(iq[q], 0), nt - 1);  // (an index array from elsewhere must not make this read leave the cloud)
    ax = qx - T[(size_t)a * 3 + 0];
    ay = qy - T[(size_t)a * 3 + 1];
    az = qz - T[(size_t)a * 3 + 2];
  }
  const int me = active ? q : -1;
  for (int c0 = 0; c0 < nt; c0 += PC_CHUNK) {
    const int cnt = min(PC_CHUNK, nt - c0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += PC_NT) {
      const float* p = T + (size_t)(c0 + t) * 3;
      tg[t] = make_float4(p[0], p[1], p[2], __int_as_float(it[c0 + t]));
    }
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
      const float4 g = tg[t];
      if (__float_as_int(g.w) == me) {
        ax += qx - g.x;
        ay += qy - g.y;
        az += qz - g.z;
      }
    }
  }
  if (active) {
    const float s = 2.f * gout[b];
    float* o = out + ((size_t)b * nq + q) * 3;
    o[0] = s * ax;
    o[1] = s * ay;
    o[2] = s * az;
  }
}

static int chamfer_check(int B, int M, int N) {
  if (B <= 0 || M <= 0 || N <= 0 || B > 65535) return SIVAE_ERR_SHAPE;
  if ((long long)B * (M > N ? M : N) * 3 >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

extern "C" size_t sivae_chamfer_workspace_bytes(int B, int M, int N) {
  if (chamfer_check(B, M, N) != SIVAE_OK) return 0;
  return (size_t)B * (cdiv(M, PC_NT) + cdiv(N, PC_NT)) * sizeof(float);
}

extern "C" int sivae_chamfer_fwd(const float* preds, const float* gts, int* idx_p, int* idx_g, float* loss, int B, int M,
                                 int N, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!preds || !gts || !idx_p || !idx_g || !loss) return SIVAE_ERR_NULL;
  const int rc = chamfer_check(B, M, N);
  if (rc != SIVAE_OK) return rc;
  if (!workspace || workspace_bytes < sivae_chamfer_workspace_bytes(B, M, N)) return SIVAE_ERR_WORKSPACE;
  const int nbp = cdiv(M, PC_NT), nbg = cdiv(N, PC_NT);
  hipLaunchKernelGGL(chamfer_fwd_kernel, dim3(nbp > nbg ? nbp : nbg, 2, B), dim3(PC_NT), 0, stream, preds, gts, idx_p, idx_g,
                     (float*)workspace, M, N, nbp, nbg);
  hipLaunchKernelGGL(chamfer_fold_kernel, dim3(cdiv(B, 64)), dim3(64), 0, stream, (const float*)workspace, loss, B,
                     nbp + nbg);
  return sivae_launch_status();
}

extern "C" int sivae_chamfer_bwd(const float* g, const float* preds, const float* gts, const int* idx_p, const int* idx_g,
                                 float* dpreds, float* dgts, int B, int M, int N, hipStream_t stream) {
  if (!g || !preds || !gts || !idx_p || !idx_g || (!dpreds && !dgts)) return SIVAE_ERR_NULL;
  const int rc = chamfer_check(B, M, N);
  if (rc != SIVAE_OK) return rc;
  const int nq = (dpreds && dgts) ? (M > N ? M : N) : (dpreds ? M : N);
  hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(cdiv(nq, PC_NT), 2, B), dim3(PC_NT), 0, stream, g, preds, gts, idx_p, idx_g,
                     dpreds, dgts, M, N);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ ReLU -> BatchNorm1d
// A channel's B * N values are cut into S slices (a multiple of 1024 values each, so a 16-byte load never straddles a
// row when N % 4 == 0); block (c, s) reduces one slice in fp64, a one-thread-per-channel kernel folds the slices in
// index order.  C * S is about 2048 blocks where the tensor is large enough.
struct RbPlan {
  int S;
  long long len;
};
static RbPlan rb_plan(long long n, int C) {
  long long S = 2048 / C;
  if (S < 1) S = 1;
  const long long smax = (n + 4095) / 4096;
  if (S > smax) S = smax;
  RbPlan p;
  p.len = ((n + S - 1) / S + 1023) / 1024 * 1024;
  p.S = (int)((n + p.len - 1) / p.len);
  return p;
}

// relu with torch's NaN rule: a NaN activation stays a NaN (`v > 0 ? v : 0` would turn it into 0 and hide a diverged run
// behind finite statistics).  The derivative at 0 is 0: the backward's gate is `a > 0`.
__device__ __forceinline__ float relu0(float v) { return v <= 0.f ? 0.f : v; }

// BWD = false: (sum r, sum r^2) of r = relu(a);  BWD = true: (sum dy, sum dy * r)
template <bool VEC, bool BWD>
__global__ void __launch_bounds__(PC_NT) relu_bn_reduce_kernel(const float* __restrict__ a, const float* __restrict__ dy,
                                                               double* __restrict__ part, int C, int N, long long n_per_ch,
                                                               long long slice_len, int S) {
  __shared__ double red[2 * PC_NT / 64];
  const int c = blockIdx.x, s = blockIdx.y;
  const long long n0 = (long long)s * slice_len;
  long long n1 = n0 + slice_len;
  if (n1 > n_per_ch) n1 = n_per_ch;
  double s0 = 0.0, s1 = 0.0;
  if (VEC) {
    for (long long n = n0 + (long long)threadIdx.x * 4; n < n1; n += PC_NT * 4) {
      const long long b = n / N;
      const size_t o = ((size_t)b * C + c) * N + (size_t)(n - b * N);
      const float4 v = *reinterpret_cast<const float4*>(a + o);
      const float r0 = relu0(v.x), r1 = relu0(v.y), r2 = relu0(v.z), r3 = relu0(v.w);
      if (BWD) {
        const float4 g = *reinterpret_cast<const float4*>(dy + o);
        s0 += ((double)g.x + (double)g.y) + ((double)g.z + (double)g.w);
        s1 += ((double)g.x * r0 + (double)g.y * r1) + ((double)g.z * r2 + (double)g.w * r3);
      } else {
        s0 += ((double)r0 + (double)r1) + ((double)r2 + (double)r3);
        s1 += ((double)r0 * r0 + (double)r1 * r1) + ((double)r2 * r2 + (double)r3 * r3);
      }
    }
  } else {
    for (long long n = n0 + threadIdx.x; n < n1; n += PC_NT) {
      const long long b = n / N;
      const size_t o = ((size_t)b * C + c) * N + (size_t)(n - b * N);
      const float r = relu0(a[o]);
      if (BWD) {
        const float g = dy[o];
        s0 += (double)g;
        s1 += (double)g * r;
      } else {
        s0 += (double)r;
        s1 += (double)r * r;
      }
    }
  }
  block_sum2<PC_NT>(s0, s1, red);
  if (threadIdx.x == 0) {
    part[((size_t)c * S + s) * 2 + 0] = s0;
    part[((size_t)c * S + s) * 2 + 1] = s1;
  }
}

// the semantics of bn.hip's bn_finalize_kernel (sivae_bn_stats): biased variance for invstd, unbiased into running_var
__global__ void __launch_bounds__(64) relu_bn_finalize_kernel(const double* __restrict__ part, int S, int C, double count,
                                                              float eps, float momentum, float* running_mean,
                                                              float* running_var, long long* num_batches_tracked,
                                                              float* __restrict__ mean_out, float* __restrict__ invstd_out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
  if (c >= C) return;
  double sum = 0.0, sq = 0.0;
  for (int s = 0; s < S; ++s) {
    sum += part[((size_t)c * S + s) * 2];
    sq += part[((size_t)c * S + s) * 2 + 1];
  }
  const double mean = sum / count;
  double var = sq / count - mean * mean;
  if (var < 0.0) var = 0.0;
  mean_out[c] = (float)mean;
  invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
    running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
}

// dbeta = sum dy, dgamma = sum dy * rhat = invstd * (sum dy r - mean sum dy), from channel c's two fp64 sums
__device__ __forceinline__ void relu_bn_param_grads(int c, double sdy, double sdyr, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                    float* __restrict__ dbeta) {
  dbeta[c] = (float)sdy;
  dgamma[c] = (float)((double)invstd[c] * (sdyr - (double)mean[c] * sdy));
}

__global__ void __launch_bounds__(64) relu_bn_bwd_finalize_kernel(const double* __restrict__ part, int S, int C,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double sdy = 0.0, sdyr = 0.0;
  for (int s = 0; s < S; ++s) {
    sdy += part[((size_t)c * S + s) * 2];
    sdyr += part[((size_t)c * S + s) * 2 + 1];
  }
  relu_bn_param_grads(c, sdy, sdyr, mean, invstd, dgamma, dbeta);
}

// y = gamma (relu(a) - mean) invstd + beta as one FMA on relu(a), with sc = gamma invstd (one multiply) and
// sh = beta - mean sc (one FMA).  These two functions are the only place the forward's arithmetic is written:
// relu_bn_apply_kernel stores relu_bn_y, max_row<., true> walks over it, so the fused max sees the stored values bit for bit.
__device__ __forceinline__ void relu_bn_scale_shift(int c, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float& sc, float& sh) {
  const float mu = mean[c], is = invstd[c], ga = gamma[c];
  sc = ga * is;
  sh = beta[c] - mu * sc;
}
__device__ __forceinline__ float relu_bn_y(float v, float sc, float sh) { return relu0(v) * sc + sh; }

// One 16-byte access per tensor and thread (VEC; N % 4 == 0 keeps the four values in one row) — the store is the last
// thing a thread does, so nothing recycles its data registers behind it (the store-data note in common.h).
template <bool VEC>
__global__ void __launch_bounds__(PC_NT) relu_bn_apply_kernel(const float* __restrict__ a, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ y, int C,
                                                              int N, size_t total) {
  const size_t e = ((size_t)blockIdx.x * PC_NT + threadIdx.x) * (VEC ? 4 : 1);
  if (e >= total) return;
  float sc, sh;
  relu_bn_scale_shift((int)((e / (size_t)N) % (size_t)C), mean, invstd, gamma, beta, sc, sh);
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(a + e);
    *reinterpret_cast<float4*>(y + e) =
        make_float4(relu_bn_y(v.x, sc, sh), relu_bn_y(v.y, sc, sh), relu_bn_y(v.z, sc, sh), relu_bn_y(v.w, sc, sh));
  } else {
    y[e] = relu_bn_y(a[e], sc, sh);
  }
}

// da = [a > 0] gamma invstd (dy - dbeta / m - rhat dgamma / m) with k = gamma invstd, mb = dbeta / m, mg = dgamma / m: the
// only place the backward's arithmetic is written.  The gate is relu0's derivative (0 at a == 0 and at a NaN).
__device__ __forceinline__ float relu_bn_da(float a, float dy, float k, float mb, float mu, float is, float mg) {
  return a > 0.f ? k * (dy - mb - (a - mu) * is * mg) : 0.f;
}

// The backward's element-wise pass.  MAX = false: g is the dense dy [B][C][N] (sivae_relu_bn_bwd, arg unused).
// MAX = true: dy is the max's gradient, g[row] at arg[row] and zero elsewhere, formed in registers (sivae_relu_bn_max_bwd:
// one read of a, one write of da).  Accesses and the store as in relu_bn_apply_kernel.
template <bool VEC, bool MAX>
__global__ void __launch_bounds__(PC_NT) relu_bn_bwd_apply_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                                  const int* __restrict__ arg, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ dgamma,
                                                                  const float* __restrict__ dbeta, float* __restrict__ da,
                                                                  int C, int N, size_t total, float inv_m) {
  const size_t e = ((size_t)blockIdx.x * PC_NT + threadIdx.x) * (VEC ? 4 : 1);
  if (e >= total) return;
  const size_t row = e / (size_t)N;
  const int c = (int)(row % (size_t)C), i = (int)(e - row * (size_t)N), kk = MAX ? arg[row] : 0;
  const float gv = MAX ? g[row] : 0.f;
  const float mu = mean[c], is = invstd[c], ga = gamma[c];
  const float k = ga * is, mb = dbeta[c] * inv_m, mg = dgamma[c] * inv_m;
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(a + e);
    const float4 d = !MAX ? *reinterpret_cast<const float4*>(g + e)
                          : make_float4(i == kk ? gv : 0.f, i + 1 == kk ? gv : 0.f, i + 2 == kk ? gv : 0.f,
                                        i + 3 == kk ? gv : 0.f);
    *reinterpret_cast<float4*>(da + e) =
        make_float4(relu_bn_da(v.x, d.x, k, mb, mu, is, mg), relu_bn_da(v.y, d.y, k, mb, mu, is, mg),
                    relu_bn_da(v.z, d.z, k, mb, mu, is, mg), relu_bn_da(v.w, d.w, k, mb, mu, is, mg));
  } else {
    const float v = a[e];
    da[e] = relu_bn_da(v, MAX ? (i == kk ? gv : 0.f) : g[e], k, mb, mu, is, mg);
  }
}

// The 16-byte instantiations want N % 4 == 0 and every tensor they access that way on a 16-byte boundary.
template <class... P>
static inline bool pc_vec_ok(int N, const P*... ptrs) {
  return (N & 3) == 0 && ((((uintptr_t)ptrs & 15) == 0) && ...);
}

// Launch of KV (16-byte accesses) on gridv where vec, of KS (scalar) on grids otherwise, in blocks of PC_NT threads on
// `stream`; the argument list is written once.  PC_LAUNCH_ELEMS: an element-wise kernel, a thread owns four elements (KV)
// or one (KS); PC_LAUNCH_ROWS: one wave per row.
#define PC_LAUNCH(vec, KV, KS, gridv, grids, ...)                                  \
  do {                                                                             \
    if (vec) hipLaunchKernelGGL(KV, gridv, dim3(PC_NT), 0, stream, __VA_ARGS__);   \
    else hipLaunchKernelGGL(KS, grids, dim3(PC_NT), 0, stream, __VA_ARGS__);       \
  } while (0)
#define PC_LAUNCH_ELEMS(vec, KV, KS, total, ...) \
  PC_LAUNCH(vec, KV, KS, dim3(cdiv((total) / 4, PC_NT)), dim3(cdiv(total, PC_NT)), __VA_ARGS__)
#define PC_LAUNCH_ROWS(vec, KV, KS, rows, ...) \
  PC_LAUNCH(vec, KV, KS, dim3(cdiv(rows, PC_NT / 64)), dim3(cdiv(rows, PC_NT / 64)), __VA_ARGS__)

static int relu_bn_check(int B, int C, int N) {
  if (B <= 0 || C <= 0 || N <= 0) return SIVAE_ERR_SHAPE;
  if ((long long)B * C * N >= 0x7fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

extern "C" size_t sivae_relu_bn_workspace_bytes(int B, int C, int N) {
  if (relu_bn_check(B, C, N) != SIVAE_OK) return 0;
  return (size_t)C * rb_plan((long long)B * N, C).S * 2 * sizeof(double);
}

extern "C" int sivae_relu_bn_stats(const float* a, int B, int C, int N, float eps, float momentum, float* running_mean,
                                   float* running_var, long long* num_batches_tracked, float* mean_out, float* invstd_out,
                                   void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!a || !mean_out || !invstd_out) return SIVAE_ERR_NULL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  if (!workspace || workspace_bytes < sivae_relu_bn_workspace_bytes(B, C, N)) return SIVAE_ERR_WORKSPACE;
  const long long n = (long long)B * N;
  const RbPlan p = rb_plan(n, C);
  double* part = (double*)workspace;
  const dim3 grid(C, p.S);
  PC_LAUNCH(pc_vec_ok(N, a), (relu_bn_reduce_kernel<true, false>), (relu_bn_reduce_kernel<false, false>), grid, grid, a,
            (const float*)nullptr, part, C, N, n, p.len, p.S);
  hipLaunchKernelGGL(relu_bn_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, stream, (const double*)part, p.S, C, (double)n,
                     eps, momentum, running_mean, running_var, num_batches_tracked, mean_out, invstd_out);
  return sivae_launch_status();
}

extern "C" int sivae_relu_bn_apply(const float* a, const float* mean, const float* invstd, const float* gamma,
                                   const float* beta, float* y, int B, int C, int N, hipStream_t stream) {
  if (!a || !mean || !invstd || !gamma || !beta || !y) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  const size_t total = (size_t)B * C * N;
  PC_LAUNCH_ELEMS(pc_vec_ok(N, a, y), (relu_bn_apply_kernel<true>), (relu_bn_apply_kernel<false>), total, a, mean, invstd,
                  gamma, beta, y, C, N, total);
  return sivae_launch_status();
}

extern "C" int sivae_relu_bn_bwd(const float* dy, const float* a, const float* mean, const float* invstd,
                                 const float* gamma, float* da, float* dgamma, float* dbeta, int B, int C, int N,
                                 void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!dy || !a || !mean || !invstd || !gamma || !da || !dgamma || !dbeta) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  if (!workspace || workspace_bytes < sivae_relu_bn_workspace_bytes(B, C, N)) return SIVAE_ERR_WORKSPACE;
  const long long n = (long long)B * N;
  const RbPlan p = rb_plan(n, C);
  double* part = (double*)workspace;
  const size_t total = (size_t)B * C * N;
  const bool vec = pc_vec_ok(N, a, dy, da);
  const dim3 grid(C, p.S);
  PC_LAUNCH(vec, (relu_bn_reduce_kernel<true, true>), (relu_bn_reduce_kernel<false, true>), grid, grid, a, dy, part, C, N, n,
            p.len, p.S);
  hipLaunchKernelGGL(relu_bn_bwd_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, stream, (const double*)part, p.S, C, mean,
                     invstd, dgamma, dbeta);
  PC_LAUNCH_ELEMS(vec, (relu_bn_bwd_apply_kernel<true, false>), (relu_bn_bwd_apply_kernel<false, false>), total, a, dy,
                  (const int*)nullptr, mean, invstd, gamma, (const float*)dgamma, (const float*)dbeta, da, C, N, total,
                  (float)(1.0 / (double)n));
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ max over points
// One wave per [b][c] row: lanes walk the row (16-byte loads when N % 4 == 0) keeping (value, lowest index), then a
// butterfly on the pair.  The lowest index wins a tie, inside a lane (ascending walk, strict compare) and across lanes.
// A NaN is the maximum, as in torch.max: it beats every number, and among NaNs the lowest index wins — the same rule
// inside a lane and in the butterfly.  `!(v <= bv)` holds where v is greater or either side is a NaN; v then wins unless
// the NaN is bv's alone.
__device__ __forceinline__ void max_take(float& bv, int& bi, float v, int i) {
  if (!(v <= bv) ? (bv == bv || (v != v && i < bi)) : (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}
// max_take for a lane's ascending walk (i above every index taken so far): an equal value or a second NaN never takes
// over, so two compares decide — and the loop-carried chain compare -> select is no longer than a plain maximum's.
// (A lane that saw -inf only keeps the start index 0x7fffffff: -inf at a real index of another lane wins the tie.)
__device__ __forceinline__ void max_walk(float& bv, int& bi, float v, int i) {
  if (!(v <= bv) && bv == bv) {
    bv = v;
    bi = i;
  }
}

// The walk over one row p[0 .. N) by one wave, the butterfly and the store.  BN: the value at i is relu_bn_y(p[i], sc, sh)
// (the fused last encoder stage), else p[i] itself (sc, sh unused).
template <bool VEC, bool BN>
__device__ __forceinline__ void max_row(const float* p, int N, int lane, float sc, float sh, float* vals, int* arg, int row) {
  const auto y = [=](float v) { return BN ? relu_bn_y(v, sc, sh) : v; };
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if (VEC) {
    for (int i = lane * 4; i < N; i += 256) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      max_walk(bv, bi, y(v.x), i);
      max_walk(bv, bi, y(v.y), i + 1);
      max_walk(bv, bi, y(v.z), i + 2);
      max_walk(bv, bi, y(v.w), i + 3);
    }
  } else {
    for (int i = lane; i < N; i += 64) max_walk(bv, bi, y(p[i]), i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    max_take(bv, bi, ov, oi);
  }
  if (lane == 0) {
    vals[row] = bv;
    arg[row] = bi < N ? bi : 0;  // (a row of -inf only: no lane took an element; index 0)
  }
}

template <bool VEC>
__global__ void __launch_bounds__(PC_NT) max_points_fwd_kernel(const float* __restrict__ x, float* __restrict__ vals,
                                                               int* __restrict__ arg, int rows, int N) {
  const int row = blockIdx.x * (PC_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;  // (wave-uniform)
  max_row<VEC, false>(x + (size_t)row * N, N, lane, 0.f, 0.f, vals, arg, row);
}

// dx = g[row] at arg[row], zero elsewhere: one kernel writes both
template <bool VEC>
__global__ void __launch_bounds__(PC_NT) max_points_bwd_kernel(const float* __restrict__ g, const int* __restrict__ arg,
                                                               float* __restrict__ dx, int N, size_t total) {
  const size_t e = ((size_t)blockIdx.x * PC_NT + threadIdx.x) * (VEC ? 4 : 1);
  if (e >= total) return;
  const size_t row = e / (size_t)N;
  const int i = (int)(e - row * (size_t)N), k = arg[row];
  const float v = g[row];
  if (VEC)
    *reinterpret_cast<float4*>(dx + e) =
        make_float4(i == k ? v : 0.f, i + 1 == k ? v : 0.f, i + 2 == k ? v : 0.f, i + 3 == k ? v : 0.f);
  else
    dx[e] = i == k ? v : 0.f;
}

extern "C" int sivae_max_points_fwd(const float* x, float* vals, int* arg, int B, int C, int N, hipStream_t stream) {
  if (!x || !vals || !arg) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  const int rows = B * C;
  PC_LAUNCH_ROWS(pc_vec_ok(N, x), (max_points_fwd_kernel<true>), (max_points_fwd_kernel<false>), rows, x, vals, arg, rows, N);
  return sivae_launch_status();
}

extern "C" int sivae_max_points_bwd(const float* g, const int* arg, float* dx, int B, int C, int N, hipStream_t stream) {
  if (!g || !arg || !dx) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  const size_t total = (size_t)B * C * N;
  PC_LAUNCH_ELEMS(pc_vec_ok(N, dx), (max_points_bwd_kernel<true>), (max_points_bwd_kernel<false>), total, g, arg, dx, N, total);
  return sivae_launch_status();
}

// ------------------------------------------------------------------------------------------------ ReLU -> BatchNorm1d -> max
// The encoder's last stage: y = BatchNorm1d(ReLU(a)) is only ever looked at through its max over the points, so neither y
// nor the max's dense gradient has to exist.  Forward: max_row over relu_bn_y, the function relu_bn_apply_kernel stores
// (vals and arg are the composition's, bit for bit); nothing of size B C N is written.  The statistics stay
// sivae_relu_bn_stats.
template <bool VEC>
__global__ void __launch_bounds__(PC_NT) relu_bn_max_fwd_kernel(const float* __restrict__ a, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ vals, int* __restrict__ arg, int rows,
                                                                int C, int N) {
  const int row = blockIdx.x * (PC_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;  // (wave-uniform)
  float sc, sh;
  relu_bn_scale_shift(row % C, mean, invstd, gamma, beta, sc, sh);
  max_row<VEC, true>(a + (size_t)row * N, N, lane, sc, sh, vals, arg, row);
}

// Backward, first launch.  The max's gradient dy is g[b][c] at arg[b][c] and zero elsewhere, so BatchNorm's two sums over
// a channel's B N values are sums over B elements: sum dy = sum_b g, sum dy r = sum_b g relu(a[b][c][arg]).  One wave
// per channel, lane l takes b = l, l + 64, ... in fp64, then the butterfly: a fixed order, two runs are bit-identical.
__global__ void __launch_bounds__(PC_NT) relu_bn_max_bwd_sums_kernel(const float* __restrict__ g, const int* __restrict__ arg,
                                                                     const float* __restrict__ a,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ invstd,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                     int B, int C, int N) {
  const int c = blockIdx.x * (PC_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;  // (wave-uniform)
  double sdy = 0.0, sdyr = 0.0;
  for (int b = lane; b < B; b += 64) {
    const size_t row = (size_t)b * C + c;
    const int k = min(max(arg[row], 0), N - 1);  // (an index array from elsewhere must not make this read leave the row)
    const float gv = g[row], r = relu0(a[row * N + k]);
    sdy += (double)gv;
    sdyr += (double)gv * r;
  }
  sdy = wave_sum(sdy);
  sdyr = wave_sum(sdyr);
  if (lane == 0) relu_bn_param_grads(c, sdy, sdyr, mean, invstd, dgamma, dbeta);
}

// Backward, second launch: relu_bn_bwd_apply_kernel<., true>.
extern "C" int sivae_relu_bn_max_fwd(const float* a, const float* mean, const float* invstd, const float* gamma,
                                     const float* beta, float* vals, int* arg, int B, int C, int N, hipStream_t stream) {
  if (!a || !mean || !invstd || !gamma || !beta || !vals || !arg) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  const int rows = B * C;
  PC_LAUNCH_ROWS(pc_vec_ok(N, a), (relu_bn_max_fwd_kernel<true>), (relu_bn_max_fwd_kernel<false>), rows, a, mean, invstd, gamma,
                 beta, vals, arg, rows, C, N);
  return sivae_launch_status();
}

extern "C" int sivae_relu_bn_max_bwd(const float* g, const int* arg, const float* a, const float* mean, const float* invstd,
                                     const float* gamma, float* da, float* dgamma, float* dbeta, int B, int C, int N,
                                     hipStream_t stream) {
  if (!g || !arg || !a || !mean || !invstd || !gamma || !da || !dgamma || !dbeta) return SIVAE_ERR_NULL;
  const int rc = relu_bn_check(B, C, N);
  if (rc != SIVAE_OK) return rc;
  const size_t total = (size_t)B * C * N;
  const float inv_m = (float)(1.0 / (double)((long long)B * N));
  hipLaunchKernelGGL(relu_bn_max_bwd_sums_kernel, dim3(cdiv(C, PC_NT / 64)), dim3(PC_NT), 0, stream, g, arg, a, mean, invstd,
                     dgamma, dbeta, B, C, N);
  PC_LAUNCH_ELEMS(pc_vec_ok(N, a, da), (relu_bn_bwd_apply_kernel<true, true>), (relu_bn_bwd_apply_kernel<false, true>), total,
                  a, g, arg, mean, invstd, gamma, (const float*)dgamma, (const float*)dbeta, da, C, N, total, inv_m);
  return sivae_launch_status();
}
