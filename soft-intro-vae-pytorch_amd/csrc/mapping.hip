// What sits between the latent and the networks of the style variant (reference: style_soft_intro_vae/net.py and model.py):
//   row pixel-norm       net.py:29-30 (pixel_norm in front of Mapping / VAEMappingFromLatent), forward and backward;
//   LeakyReLU backward   the activation of a MappingBlock (net.py:748-751) taken back through its saved OUTPUT, together
//                        with the bias gradient of the linear layer in front of it, in one pass over dy;
//   style assembly       model.py:176-200: the repeat over the layers, the running average of the styles, style mixing and
//                        the truncation trick, forward and backward.
// The linear layers themselves, with the LeakyReLU as their epilogue, are linear.hip's.
//
// Partition.  Every kernel walks rows of fp32 in quads: thread t owns the 4 consecutive elements 4 q .. 4 q + 3 of a row,
// read and written with one 16-byte access where every row of every tensor of the call is 16-byte aligned (aligned bases
// and a row length that is a multiple of 4), with guarded scalar accesses over the SAME 4 elements anywhere else: the two
// instantiations differ in nothing but the width of the access, so the alignment changes no bit.
//   pixel-norm:  one wave per row; lane l owns the quads l, l + 64, ...; a lane adds its products in index order in fp32
//                (fmaf), the 64 lanes are added by the butterfly of common.h in fp64.
//   column sums (dbias, the batch mean of the styles): a block owns 16 quads (64 columns) x MAP_RG row groups; group g
//                adds its rows [g rpg, (g + 1) rpg), rpg = ceil(B / MAP_RG), in ascending b in fp64, thread 0 .. 15 of
//                group 0 then adds the groups' sums in ascending g in fp64: ascending b throughout, the bracketing fixed by B.
//   styles:      one thread per (sample, quad), the layers walked in ascending l.
// Plain grids, bounded loops, no atomics, no cooperative launch: every order is fixed by the shape alone, two runs are
// bit-identical, and a sample's pixel-norm / styles result (without the running average) does not depend on the batch.
#include "common.h"
#include "chunk4.h"

// No contraction of a * b + c by the optimiser anywhere in this file (it may differ between the two instantiations of one
// kernel); the multiply-adds that are wanted are written out as fmaf.
#pragma clang fp contract(off)

#define MAP_NT 256  // threads of a block
#define MAP_RG 16   // row groups of a column-sum block
#define MAP_CQ 16   // quads (of 4 columns) of a column-sum block

namespace {

// every row goes through the GLOBAL address space (chunk4.h); its quads are read and written with c4_load / c4_store
__device__ __forceinline__ c4_gcf32* map_g(const float* p) { return (c4_gcf32*)p; }
__device__ __forceinline__ c4_gf32* map_g(float* p) { return (c4_gf32*)p; }

// ---- pixel-norm ---------------------------------------------------------------------------------------------------------
// sum_z a[z] b[z] of one row by one wave: the lane's quads in ascending order, j ascending inside a quad, then the lanes
template <bool AL>
__device__ __forceinline__ double map_row_dot(c4_gcf32* __restrict__ a, c4_gcf32* __restrict__ b, int Z, int lane) {
  float acc = 0.f;
  for (int i = lane * 4; i < Z; i += 256) {
    float u[4], v[4];
    c4_load<AL>(a, i, Z, u);
    c4_load<AL>(b, i, Z, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(u[j], v[j], acc);
  }
  return wave_sum((double)acc);
}

// y = x r, r = 1 / sqrt(mean_z x^2 + eps); r [B] is kept for the backward
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) pixel_norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                float* __restrict__ rfac, int B, int Z, float eps) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * (MAP_NT / 64) + (threadIdx.x >> 6);
  if (b >= B) return;  // (whole waves leave: the butterfly below runs with every lane of its wave active)
  c4_gcf32* xr = map_g(x) + (size_t)b * Z;
  c4_gf32* yr = map_g(y) + (size_t)b * Z;
  const double ss = map_row_dot<AL>(xr, xr, Z, lane);
  const float r = (float)(1.0 / sqrt(ss / (double)Z + (double)eps));
  if (lane == 0) map_g(rfac)[b] = r;
  for (int i = lane * 4; i < Z; i += 256) {
    float v[4];
    c4_load<AL>(xr, i, Z, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * r;
    c4_store<AL>(yr, i, Z, v);
  }
}

// dx = r dy - x c, c = r^3 mean_z(dy x)
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) pixel_norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ rfac, float* __restrict__ dx, int B,
                                                                int Z) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * (MAP_NT / 64) + (threadIdx.x >> 6);
  if (b >= B) return;
  c4_gcf32* xr = map_g(x) + (size_t)b * Z;
  c4_gcf32* gr = map_g(dy) + (size_t)b * Z;
  c4_gf32* dr = map_g(dx) + (size_t)b * Z;
  const double dot = map_row_dot<AL>(gr, xr, Z, lane);
  const float r = map_g(rfac)[b];
  const double r3 = (double)r * (double)r * (double)r;
  const float c = (float)(r3 * (dot / (double)Z));
  for (int i = lane * 4; i < Z; i += 256) {
    float g[4], v[4];
    c4_load<AL>(gr, i, Z, g);
    c4_load<AL>(xr, i, Z, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = fmaf(-v[j], c, r * g[j]);
    c4_store<AL>(dr, i, Z, g);
  }
}

// ---- column sums over the batch ---------------------------------------------------------------------------------------
// the fold of the row groups' fp64 sums of one quad: group 0's thread returns true with the totals in s
__device__ __forceinline__ bool map_fold_groups(double (*red)[MAP_CQ][4], double (&s)[4], int cq, int rg) {
#pragma unroll
  for (int j = 0; j < 4; ++j) red[rg][cq][j] = s[j];
  __syncthreads();
  if (rg != 0) return false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double t = red[0][cq][j];
    for (int g = 1; g < MAP_RG; ++g) t += red[g][cq][j];
    s[j] = t;
  }
  return true;
}

// dz = dy (y > 0 ? 1 : slope) from the saved output y (y == nullptr: dz = dy, a layer without activation);
// dbias[n] = sum_b dz[b][n].  dz and dbias may each be null.
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) lrelu_bias_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                float slope, float* __restrict__ dz,
                                                                float* __restrict__ dbias, int B, int N) {
  __shared__ double red[MAP_RG][MAP_CQ][4];
  const int cq = threadIdx.x % MAP_CQ, rg = threadIdx.x / MAP_CQ;
  const int n = (blockIdx.x * MAP_CQ + cq) * 4;
  const int rpg = (B + MAP_RG - 1) / MAP_RG;
  const int b0 = rg * rpg, b1 = min(B, b0 + rpg);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (n < N) {
    for (int b = b0; b < b1; ++b) {
      const size_t row = (size_t)b * N;
      float g[4];
      c4_load<AL>(map_g(dy) + row, n, N, g);
      if (y) {
        float v[4];
        c4_load<AL>(map_g(y) + row, n, N, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] : g[j] * slope;
      }
      if (dz) c4_store<AL>(map_g(dz) + row, n, N, g);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)g[j];
    }
  }
  if (!dbias) return;
  if (!map_fold_groups(red, s, cq, rg) || n >= N) return;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n + j < N) map_g(dbias)[n + j] = (float)s[j];
}

// avg[l][z] <- lerp(avg[l][z], mean_b s[b][z], w) for every layer l (model.py:180-183)
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) styles_avg_kernel(const float* __restrict__ s, float* __restrict__ avg, float w,
                                                            int B, int L, int Z) {
  __shared__ double red[MAP_RG][MAP_CQ][4];
  const int cq = threadIdx.x % MAP_CQ, rg = threadIdx.x / MAP_CQ;
  const int z = (blockIdx.x * MAP_CQ + cq) * 4;
  const int rpg = (B + MAP_RG - 1) / MAP_RG;
  const int b0 = rg * rpg, b1 = min(B, b0 + rpg);
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  if (z < Z) {
    for (int b = b0; b < b1; ++b) {
      float v[4];
      c4_load<AL>(map_g(s) + (size_t)b * Z, z, Z, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] += (double)v[j];
    }
  }
  if (!map_fold_groups(red, t, cq, rg) || z >= Z) return;
  float m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = (float)(t[j] / (double)B);
  for (int l = 0; l < L; ++l) {
    float a[4];
    c4_load<AL>(map_g((const float*)avg) + (size_t)l * Z, z, Z, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = c4_lerp(a[j], m[j], w, 1.f - w);
    c4_store<AL>(map_g(avg) + (size_t)l * Z, z, Z, a);
  }
}

// ---- style assembly -----------------------------------------------------------------------------------------------------
struct StylesArgs {
  const float *s, *s2, *avg, *dstyles;
  float *styles, *ds, *ds2;
  int B, L, Z, qpr;     // qpr: quads per row, ceil(Z / 4)
  int mix_cutoff;       // layers l < mix_cutoff take s, the others s2 (L without s2)
  int trunc_cutoff;     // layers l < trunc_cutoff are truncated (0 without truncation)
  float psi;
};

// styles[b][l] = src_l[b] (l >= trunc_cutoff), lerp(avg[l], src_l[b], psi) below it (model.py:176-178, :194, :196-200)
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) styles_fwd_kernel(StylesArgs a) {
  const size_t e = (size_t)blockIdx.x * MAP_NT + threadIdx.x;
  if (e >= (size_t)a.B * a.qpr) return;
  const int b = (int)(e / a.qpr), z = (int)(e - (size_t)b * a.qpr) * 4, Z = a.Z;
  float v1[4], v2[4] = {0.f, 0.f, 0.f, 0.f};
  c4_load<AL>(map_g(a.s) + (size_t)b * Z, z, Z, v1);
  if (a.mix_cutoff < a.L) c4_load<AL>(map_g(a.s2) + (size_t)b * Z, z, Z, v2);
  c4_gf32* out = map_g(a.styles) + (size_t)b * a.L * Z;
  for (int l = 0; l < a.L; ++l) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = l < a.mix_cutoff ? v1[j] : v2[j];
    if (l < a.trunc_cutoff) {
      float m[4];
      c4_load<AL>(map_g(a.avg) + (size_t)l * Z, z, Z, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = c4_lerp(m[j], o[j], a.psi, 1.f - a.psi);
    }
    c4_store<AL>(out + (size_t)l * Z, z, Z, o);
  }
}

// ds[b] = sum_{l < mix_cutoff} c_l dstyles[b][l], ds2[b] = sum_{l >= mix_cutoff} c_l dstyles[b][l], c_l = psi below the
// truncation cutoff and 1 from it on (d lerp / d end = the weight on both branches), l ascending
template <bool AL>
__global__ void __launch_bounds__(MAP_NT) styles_bwd_kernel(StylesArgs a) {
  const size_t e = (size_t)blockIdx.x * MAP_NT + threadIdx.x;
  if (e >= (size_t)a.B * a.qpr) return;
  const int b = (int)(e / a.qpr), z = (int)(e - (size_t)b * a.qpr) * 4, Z = a.Z;
  c4_gcf32* g = map_g(a.dstyles) + (size_t)b * a.L * Z;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < a.L; ++l) {
    float v[4];
    c4_load<AL>(g + (size_t)l * Z, z, Z, v);
    const float c = l < a.trunc_cutoff ? a.psi : 1.f;
    if (l < a.mix_cutoff) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s1[j] = fmaf(c, v[j], s1[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) s2[j] = fmaf(c, v[j], s2[j]);
    }
  }
  if (a.ds) c4_store<AL>(map_g(a.ds) + (size_t)b * Z, z, Z, s1);
  if (a.ds2) c4_store<AL>(map_g(a.ds2) + (size_t)b * Z, z, Z, s2);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// rows x row length: a tensor of the call stays below 2^31 elements (the quad and block counts are 32-bit)
int map_check(long long rows, long long cols) {
  if (rows <= 0 || cols <= 0) return SIVAE_ERR_SHAPE;
  if (rows > 0x7fffffffLL / cols) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

#define MAP_LAUNCH(KERN, al, grid, stream, ...)                                              \
  do {                                                                                       \
    if (al) hipLaunchKernelGGL((KERN<true>), grid, dim3(MAP_NT), 0, stream, __VA_ARGS__);     \
    else hipLaunchKernelGGL((KERN<false>), grid, dim3(MAP_NT), 0, stream, __VA_ARGS__);       \
  } while (0)

}  // namespace

extern "C" int sivae_pixel_norm_fwd(const float* x, float* y, float* rfac, int B, int Z, float eps, hipStream_t stream) {
  if (!x || !y || !rfac) return SIVAE_ERR_NULL;
  const int rc = map_check(B, Z);
  if (rc != SIVAE_OK) return rc;
  if (!(eps >= 0.f) || !c4_al4({x, y, rfac})) return SIVAE_ERR_SHAPE;
  const bool al = c4_al16(Z, {x, y});
  MAP_LAUNCH(pixel_norm_fwd_kernel, al, dim3((unsigned)cdiv(B, MAP_NT / 64)), stream, x, y, rfac, B, Z, eps);
  return sivae_launch_status();
}

extern "C" int sivae_pixel_norm_bwd(const float* dy, const float* x, const float* rfac, float* dx, int B, int Z,
                                    hipStream_t stream) {
  if (!dy || !x || !rfac || !dx) return SIVAE_ERR_NULL;
  const int rc = map_check(B, Z);
  if (rc != SIVAE_OK) return rc;
  if (!c4_al4({dy, x, rfac, dx})) return SIVAE_ERR_SHAPE;
  const bool al = c4_al16(Z, {dy, x, dx});
  MAP_LAUNCH(pixel_norm_bwd_kernel, al, dim3((unsigned)cdiv(B, MAP_NT / 64)), stream, dy, x, rfac, dx, B, Z);
  return sivae_launch_status();
}

extern "C" int sivae_lrelu_bias_bwd(const float* dy, const float* y, float slope, float* dz, float* dbias, int B, int N,
                                    hipStream_t stream) {
  if (!dy) return SIVAE_ERR_NULL;
  const int rc = map_check(B, N);
  if (rc != SIVAE_OK) return rc;
  if (!(slope >= 0.f && slope <= 1.f)) return SIVAE_ERR_MODE;
  if (!c4_al4({dy, y, dz, dbias})) return SIVAE_ERR_SHAPE;
  if (!dz && !dbias) return SIVAE_OK;
  const bool al = c4_al16(N, {dy, y, dz});
  MAP_LAUNCH(lrelu_bias_bwd_kernel, al, dim3((unsigned)cdiv(N, 4 * MAP_CQ)), stream, dy, y, slope, dz, dbias, B, N);
  return sivae_launch_status();
}

static int styles_check(int has_s2, int mix_cutoff, int truncate, int trunc_cutoff, int B, int L, int Z) {
  const int rc = map_check((long long)B * L, Z);
  if (rc != SIVAE_OK) return rc;
  if (B <= 0 || L <= 0) return SIVAE_ERR_SHAPE;
  if (truncate != 0 && truncate != 1) return SIVAE_ERR_MODE;
  if (has_s2 && (mix_cutoff < 0 || mix_cutoff > L)) return SIVAE_ERR_SHAPE;
  if (truncate && (trunc_cutoff < 0 || trunc_cutoff > L)) return SIVAE_ERR_SHAPE;
  return SIVAE_OK;
}

extern "C" int sivae_styles_fwd(const float* s, const float* s2, int mix_cutoff, float* avg, int update_avg,
                                float avg_weight, int truncate, float psi, int trunc_cutoff, float* styles, int B, int L,
                                int Z, hipStream_t stream) {
  if (!s || !styles) return SIVAE_ERR_NULL;
  if (update_avg != 0 && update_avg != 1) return SIVAE_ERR_MODE;
  const int rc = styles_check(s2 != nullptr, mix_cutoff, truncate, trunc_cutoff, B, L, Z);
  if (rc != SIVAE_OK) return rc;
  if ((update_avg || truncate) && !avg) return SIVAE_ERR_NULL;
  if (update_avg && !(avg_weight >= 0.f && avg_weight <= 1.f)) return SIVAE_ERR_MODE;
  if (!c4_al4({s, s2, avg, styles})) return SIVAE_ERR_SHAPE;
  const bool al = c4_al16(Z, {s, s2, avg, styles});
  if (update_avg) {
    MAP_LAUNCH(styles_avg_kernel, al, dim3((unsigned)cdiv(Z, 4 * MAP_CQ)), stream, s, avg, avg_weight, B, L, Z);
    const int st = sivae_launch_status();
    if (st != SIVAE_OK) return st;
  }
  StylesArgs a = {};
  a.s = s, a.s2 = s2, a.avg = avg, a.styles = styles;
  a.B = B, a.L = L, a.Z = Z, a.qpr = cdiv(Z, 4);
  a.mix_cutoff = s2 ? mix_cutoff : L;
  a.trunc_cutoff = truncate ? trunc_cutoff : 0;
  a.psi = psi;
  MAP_LAUNCH(styles_fwd_kernel, al, dim3((unsigned)cdiv((long long)B * a.qpr, MAP_NT)), stream, a);
  return sivae_launch_status();
}

extern "C" int sivae_styles_bwd(const float* dstyles, int has_s2, int mix_cutoff, int truncate, float psi,
                                int trunc_cutoff, float* ds, float* ds2, int B, int L, int Z, hipStream_t stream) {
  if (!dstyles) return SIVAE_ERR_NULL;
  if (has_s2 != 0 && has_s2 != 1) return SIVAE_ERR_MODE;
  const int rc = styles_check(has_s2, mix_cutoff, truncate, trunc_cutoff, B, L, Z);
  if (rc != SIVAE_OK) return rc;
  if (ds2 && !has_s2) return SIVAE_ERR_MODE;
  if (!c4_al4({dstyles, ds, ds2})) return SIVAE_ERR_SHAPE;
  if (!ds && !ds2) return SIVAE_OK;
  const bool al = c4_al16(Z, {dstyles, ds, ds2});
  StylesArgs a = {};
  a.dstyles = dstyles, a.ds = ds, a.ds2 = ds2;
  a.B = B, a.L = L, a.Z = Z, a.qpr = cdiv(Z, 4);
  a.mix_cutoff = has_s2 ? mix_cutoff : L;
  a.trunc_cutoff = truncate ? trunc_cutoff : 0;
  a.psi = psi;
  MAP_LAUNCH(styles_bwd_kernel, al, dim3((unsigned)cdiv((long long)B * a.qpr, MAP_NT)), stream, a);
  return sivae_launch_status();
}
