// The style variant's RGB layers and the level-of-detail blend (reference: style_soft_intro_vae/net.py): ToRGB, a 1x1
// convolution of C feature planes to K image planes plus bias, blended while a resolution fades in with the previous
// level's image upsampled 2x (net.py:563-571), and FromRGB, a 1x1 convolution of K image planes to C feature planes plus
// bias and two LeakyReLU(0.2) (net.py:215-217 and :270-271), on the 2x2 average of the image and blended with the first
// block's output while fading in (net.py:289-294).  One forward and one backward kernel each.  fp32, NCHW, 1 <= K <= 4.
//
// Partition (all four kernels).  A block owns one sample's tile of 256 consecutive pixels of the H x W plane: lane l of
// every wave owns the 4 pixels (tile 64 + l) 4 ..., read with one 16-byte access per plane (every pointer 16-byte aligned
// and H W a multiple of 4) or with guarded scalar accesses over the SAME 4 pixels anywhere else.  The block's RGB_NW waves
// split the C feature planes into RGB_NW contiguous slices, wave v taking the channels [v cpw, (v + 1) cpw),
// cpw = ceil(C / RGB_NW).  Three bodies serve the four kernels:
//   contraction  C planes -> K  (to_rgb forward, from_rgb dimg): a wave adds its channels in ascending order into K x 4
//                registers; the waves' partial sums are added in wave order through LDS.
//   expansion    K planes -> C  (from_rgb forward, to_rgb dx): a pixel's K values are held, one result per channel.
//   plane-pair reduction (dw, dbias): per channel, a lane's 4 products, then the transposing wave sum of common.h, one
//                partial per (channel, block) in the workspace; a second launch adds the blocks' partials per channel in
//                block order in fp64.
// No atomics, every order is fixed by (C, H W) alone: two runs are bit-identical, a sample's forward result does not
// depend on the batch, and the alignment changes no bit.  The weights are read with wave-uniform indices (scalar loads).
#include "common.h"
#include "chunk4.h"

// No contraction of a * b + c by the optimiser anywhere in this file (it differs between the two instantiations of one
// kernel); the multiply-adds of the three bodies are written out as fmaf, which both instantiations execute alike.
#pragma clang fp contract(off)

#define RGB_NW 8            // waves of a block
#define RGB_NT (64 * RGB_NW)
#define RGB_TILE 256        // pixels of a block: 64 lanes x 4
#define RGB_SLOPE2 0.04f    // the slope of two LeakyReLU(0.2) below zero

__device__ __forceinline__ float rgb_lrelu2(float t) {
  const float u = t > 0.f ? t : t * 0.2f;
  return u > 0.f ? u : u * 0.2f;
}
// (a lane's 4 pixels are read and written with chunk4.h's c4_load / c4_store, the blends are its c4_lerp)

// ---- the three bodies --------------------------------------------------------------------------------------------------
// contraction: acc[k][j] += w[k ws] v[j], k ascending (w: wave-uniform)
template <int K>
__device__ __forceinline__ void rgb_contract(float (&acc)[K][4], const float* __restrict__ w, int ws, const float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float wk = w[(size_t)k * ws];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(wk, v[j], acc[k][j]);
  }
}
// expansion: out[j] = init + sum_k w[k ws] in[k][j], k ascending
template <int K>
__device__ __forceinline__ void rgb_expand(float (&out)[4], float init, const float* __restrict__ w, int ws,
                                           const float (&in)[K][4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = init;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float wk = w[(size_t)k * ws];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = fmaf(wk, in[k][j], out[j]);
  }
}
// plane-pair reduction: s[k] = sum_j a[k][j] v[j] over the lane's 4 pixels, j ascending
template <int K>
__device__ __forceinline__ void rgb_pair(float* __restrict__ s, const float (&a)[K][4], const float (&v)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float t = a[k][0] * v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) t = fmaf(a[k][j], v[j], t);
    s[k] = t;
  }
}
// ... and its wave step: vals holds 8 / KVP channels' KVP sums each (c, c + 1 for KVP = 4); the wave totals go to
// part[(c + ..) NB + blk][KVP].  Whole wave active.
template <int KVP>
__device__ __forceinline__ void rgb_wave_partials(float (&vals)[8], float* __restrict__ part, int c, int c1, size_t NB,
                                                  size_t blk, int lane) {
  wave_transpose_sum8(vals, lane);
  if (lane < 8) {
    const int cc = c + lane / KVP;
    if (cc < c1) part[((size_t)cc * NB + blk) * KVP + lane % KVP] = vals[0];
  }
}

// the sums of the waves' K x 4 partial results in wave order: wave k < K returns plane k's in out (true), the others false
template <int K>
__device__ __forceinline__ bool rgb_fold_waves(float4 (*red)[K][64], const float (&acc)[K][4], int wv, int lane,
                                               float (&out)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) red[wv][k][lane] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
  __syncthreads();
  if (wv >= K) return false;
  float4 s = red[0][wv][lane];
#pragma unroll
  for (int v = 1; v < RGB_NW; ++v) {
    const float4 q = red[v][wv][lane];
    s.x += q.x, s.y += q.y, s.z += q.z, s.w += q.w;
  }
  out[0] = s.x, out[1] = s.y, out[2] = s.z, out[3] = s.w;
  return true;
}

// the K image values of the lane's 4 pixels: planes of n pixels at img, or the 2 x 2 averages of planes of 4 n pixels
// (rows of 2 W), ((a + b) + (c + d)) / 4
template <int K, bool AL>
__device__ __forceinline__ void rgb_load_img(const float* __restrict__ img, bool pool, int i, int n, int W,
                                             float (&im)[K][4]) {
  if (!pool) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (i < n) c4_load<AL>(img + (size_t)k * n, i, n, im[k]);
      else im[k][0] = im[k][1] = im[k][2] = im[k][3] = 0.f;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = i + j, h = p / W, w = p - h * W;
    const size_t o = (size_t)(2 * h) * (2 * W) + 2 * w;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* q = img + (size_t)k * 4 * n + o;
      im[k][j] = p < n ? ((q[0] + q[1]) + (q[2 * W] + q[2 * W + 1])) * 0.25f : 0.f;
    }
  }
}

struct RgbArgs {
  const float *x;      // to_rgb: x;  from_rgb: the image
  const float *w, *bias;
  const float *aux;    // to_rgb: prev (or null);  from_rgb: other (or null)
  const float *dy;
  float *y;            // forward output
  float *dx;           // to_rgb: dx;  from_rgb: dimg
  float *daux;         // from_rgb: dother
  float *part;         // [C (+ 1)][NB][KVP] partial sums of dw (and dbias), or null
  int C, HW, W, cpw, pool, sums, blended;  // blended: the backward kernels' "the forward blended" (they read no aux)
  float blend, omb;    // omb = 1 - blend in fp32
};

// ---- to_rgb forward: the contraction, the epilogue adds the bias and blends with up2(prev) ------------------------------
template <int K, bool AL>
__global__ void __launch_bounds__(RGB_NT) rgb_to_fwd_kernel(RgbArgs a) {
  __shared__ float4 red[RGB_NW][K][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = a.HW, C = a.C, i = (blockIdx.x * 64 + lane) * 4, b = blockIdx.y;
  const int c0 = wv * a.cpw, c1 = min(C, c0 + a.cpw);
  float acc[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.f;
  if (i < n) {
    const float* xp = a.x + ((size_t)b * C + c0) * n;
#pragma unroll 4
    for (int c = c0; c < c1; ++c, xp += n) {
      float v[4];
      c4_load<AL>(xp, i, n, v);
      rgb_contract<K>(acc, a.w + c, C, v);
    }
  }
  float o[4];
  if (!rgb_fold_waves<K>(red, acc, wv, lane, o) || i >= n) return;
  const int k = wv;
  const float bk = a.bias[k];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = bk + o[j];
  if (a.aux) {
    const float* pv = a.aux + ((size_t)b * K + k) * (n / 4);
    const int W = a.W, W2 = W / 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = i + j, h = p / W, w = p - h * W;
      if (p < n) o[j] = c4_lerp(pv[(h / 2) * W2 + w / 2], o[j], a.blend, a.omb);
    }
  }
  c4_store<AL>(a.y + ((size_t)b * K + k) * n, i, n, o);
}

// ---- from_rgb forward: the expansion, prologue the 2 x 2 average, epilogue lrelu2 and the blend with other ----------------
template <int K, bool AL>
__global__ void __launch_bounds__(RGB_NT) rgb_from_fwd_kernel(RgbArgs a) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = a.HW, C = a.C, i = (blockIdx.x * 64 + lane) * 4, b = blockIdx.y;
  const int c0 = wv * a.cpw, c1 = min(C, c0 + a.cpw);
  if (i >= n) return;
  float im[K][4];
  rgb_load_img<K, AL>(a.x + (size_t)b * K * n * (a.pool ? 4 : 1), a.pool, i, n, a.W, im);
  const size_t base = ((size_t)b * C + c0) * n;
  float* yp = a.y + base;
  const float* op = a.aux ? a.aux + base : nullptr;
#pragma unroll 4
  for (int c = c0; c < c1; ++c, yp += n) {
    float t[4];
    rgb_expand<K>(t, a.bias[c], a.w + (size_t)c * K, 1, im);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = rgb_lrelu2(t[j]);
    if (op) {
      float ov[4];
      c4_load<AL>(op, i, n, ov);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = c4_lerp(t[j], ov[j], a.blend, a.omb);
      op += n;
    }
    c4_store<AL>(yp, i, n, t);
  }
}

// ---- to_rgb backward: g = dy dlerp/dconv; the expansion gives dx, the plane-pair reduction dw (rows 0 .. C - 1 of the
// partials) and dbias (row C, by wave 0).  x is read once, and only for dw. ---------------------------------------------------
template <int K, bool AL>
__global__ void __launch_bounds__(RGB_NT) rgb_to_bwd_kernel(RgbArgs a) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = a.HW, C = a.C, i = (blockIdx.x * 64 + lane) * 4, b = blockIdx.y;
  const int c0 = wv * a.cpw, c1 = min(C, c0 + a.cpw);
  const size_t NB = (size_t)gridDim.x * gridDim.y, blk = (size_t)b * gridDim.x + blockIdx.x;
  const bool live = i < n;
  const float cg = a.blended ? a.blend : 1.f;
  float g[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (live) c4_load<AL>(a.dy + ((size_t)b * K + k) * n, i, n, g[k]);
    else g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) g[k][j] *= cg;
  }
  if (a.part && (a.sums & 2) && wv == 0) {  // dbias[k] = sum g[k]
    float vals[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) vals[k] = ((g[k][0] + g[k][1]) + g[k][2]) + g[k][3];
    rgb_wave_partials<4>(vals, a.part, C, C + 1, NB, blk, lane);
  }
  const bool dw = a.part && (a.sums & 1);
  const size_t base = ((size_t)b * C + c0) * n;
  for (int c = c0; c < c1; c += 2) {
    float vals[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cc = c + u;
      if (cc >= c1) break;
      const size_t off = base + (size_t)(cc - c0) * n;
      if (a.dx && live) {
        float o[4];
        rgb_expand<K>(o, 0.f, a.w + cc, C, g);
        c4_store<AL>(a.dx + off, i, n, o);
      }
      if (dw) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) c4_load<AL>(a.x + off, i, n, v);
        rgb_pair<K>(vals + 4 * u, g, v);
      }
    }
    if (dw) rgb_wave_partials<4>(vals, a.part, c, c1, NB, blk, lane);
  }
}

// dprev[b][k][q] = (1 - blend) ((dy00 + dy01) + (dy10 + dy11)) over the four pixels of q
__global__ void __launch_bounds__(256) rgb_dprev_kernel(const float* __restrict__ dy, float* __restrict__ dprev, size_t total,
                                                        int H2, int W2, float omb) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = (int)(e % W2), h = (int)((e / W2) % H2);
  const size_t plane = e / ((size_t)W2 * H2);
  const float* q = dy + plane * 4 * ((size_t)W2 * H2) + (size_t)(2 * h) * (2 * W2) + 2 * w;
  dprev[e] = omb * ((q[0] + q[1]) + (q[2 * W2] + q[2 * W2 + 1]));
}

// ---- from_rgb backward: t recomputed from the image, da = dy dlerp/da lrelu2'(t); the contraction gives dimg, the
// plane-pair reduction (dw, dbias), and dother = dy blend is written on the way.  dy is read once. -----------------------------
template <int K, bool AL>
__global__ void __launch_bounds__(RGB_NT) rgb_from_bwd_kernel(RgbArgs a) {
  constexpr int KVP = K < 4 ? 4 : 8, CPS = 8 / KVP;  // values per channel in the partials; channels per wave sum
  __shared__ float4 red[RGB_NW][K][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = a.HW, C = a.C, i = (blockIdx.x * 64 + lane) * 4, b = blockIdx.y;
  const int c0 = wv * a.cpw, c1 = min(C, c0 + a.cpw);
  const size_t NB = (size_t)gridDim.x * gridDim.y, blk = (size_t)b * gridDim.x + blockIdx.x;
  const bool live = i < n;
  const float ca = a.blended ? a.omb : 1.f;
  float im[K][4], ones[1][4] = {{1.f, 1.f, 1.f, 1.f}};
  rgb_load_img<K, AL>(a.x + (size_t)b * K * n * (a.pool ? 4 : 1), a.pool, i, n, a.W, im);
  float acc[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.f;
  const size_t base = ((size_t)b * C + c0) * n;
  const bool need_da = a.dx || a.part;
  for (int c = c0; c < c1; c += CPS) {
    float vals[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < CPS; ++u) {
      const int cc = c + u;
      if (cc >= c1) break;
      const size_t off = base + (size_t)(cc - c0) * n;
      float dyv[4] = {0.f, 0.f, 0.f, 0.f}, da[4];
      if (live) c4_load<AL>(a.dy + off, i, n, dyv);
      if (a.daux && live) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = dyv[j] * a.blend;
        c4_store<AL>(a.daux + off, i, n, o);
      }
      if (!need_da) continue;
      float t[4];
      rgb_expand<K>(t, a.bias[cc], a.w + (size_t)cc * K, 1, im);
#pragma unroll
      for (int j = 0; j < 4; ++j) da[j] = (dyv[j] * ca) * (t[j] > 0.f ? 1.f : RGB_SLOPE2);
      if (a.dx) rgb_contract<K>(acc, a.w + (size_t)cc * K, 1, da);
      if (a.part) {
        rgb_pair<K>(vals + KVP * u, im, da);
        rgb_pair<1>(vals + KVP * u + K, ones, da);
      }
    }
    if (a.part) rgb_wave_partials<KVP>(vals, a.part, c, c1, NB, blk, lane);
  }
  if (!a.dx) return;
  float o[4];
  if (!rgb_fold_waves<K>(red, acc, wv, lane, o) || !live) return;
  const int k = wv;
  if (!a.pool) {
    c4_store<AL>(a.dx + ((size_t)b * K + k) * n, i, n, o);
    return;
  }
  float* q0 = a.dx + ((size_t)b * K + k) * 4 * n;
  const int W = a.W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = i + j, h = p / W, w = p - h * W;
    if (p >= n) break;
    float* q = q0 + (size_t)(2 * h) * (2 * W) + 2 * w;
    const float v = o[j] * 0.25f;
    q[0] = v, q[1] = v, q[2 * W] = v, q[2 * W + 1] = v;
  }
}

// ---- the merge of the partials: row r of part is [NB][KVP], s[v] its sum over the blocks.  Rows r < rows (one per feature
// channel): out_a[r sa + v ta] = s[v] for v < na, and with b_mode 0 (from_rgb's dbias) out_b[r] = s[na]; the row r == rows
// (to_rgb's dbias): out_b[v] = s[v] for v < na.  A thread adds its blocks in ascending order in fp64, then lanes and waves as
// block_sum does. -----------------------------------------------------------------------------------------------------------
template <int KVP>
__global__ void __launch_bounds__(256) rgb_merge_kernel(const float* __restrict__ part, size_t NB, int rows, float* out_a,
                                                        int na, int sa, int ta, float* out_b, int b_mode) {
  __shared__ double red[256 / 64];
  const int r = blockIdx.x;
  const float* p = part + (size_t)r * NB * KVP;
  double s[KVP];
#pragma unroll
  for (int v = 0; v < KVP; ++v) s[v] = 0.0;
  for (size_t q = threadIdx.x; q < NB; q += 256) {
#pragma unroll
    for (int v = 0; v < KVP; ++v) s[v] += (double)p[q * KVP + v];
  }
#pragma unroll
  for (int v = 0; v < KVP; ++v) s[v] = block_sum<256>(s[v], red);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int v = 0; v < KVP; ++v) {
    if (r < rows) {
      if (out_a && v < na) out_a[(size_t)r * sa + (size_t)v * ta] = (float)s[v];
      if (out_b && b_mode == 0 && v == na) out_b[r] = (float)s[v];
    } else if (out_b && v < na) {
      out_b[v] = (float)s[v];
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host side
static int rgb_check(int B, int C, int H, int W, int K) {
  if (K < 1 || K > 4) return SIVAE_ERR_SHAPE;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return SIVAE_ERR_SHAPE;
  if (B > 65535 || (long long)H * W > 0x3fffffffLL || C > 0x3fffffff) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}
static size_t rgb_blocks(int B, int HW) { return (size_t)B * (size_t)cdiv(HW, RGB_TILE); }

#define RGB_LAUNCH_K(KERN, K, al, grid, stream, args)                                   \
  do {                                                                                  \
    if (al) hipLaunchKernelGGL((KERN<K, true>), grid, dim3(RGB_NT), 0, stream, args);    \
    else hipLaunchKernelGGL((KERN<K, false>), grid, dim3(RGB_NT), 0, stream, args);      \
  } while (0)
#define RGB_LAUNCH(KERN, K, al, grid, stream, args)                 \
  do {                                                              \
    switch (K) {                                                    \
      case 1: RGB_LAUNCH_K(KERN, 1, al, grid, stream, args); break; \
      case 2: RGB_LAUNCH_K(KERN, 2, al, grid, stream, args); break; \
      case 3: RGB_LAUNCH_K(KERN, 3, al, grid, stream, args); break; \
      default: RGB_LAUNCH_K(KERN, 4, al, grid, stream, args); break; \
    }                                                               \
  } while (0)

extern "C" int sivae_to_rgb_fwd(const float* x, const float* w, const float* bias, const float* prev, float blend, float* y,
                                int B, int C, int H, int W, int K, hipStream_t stream) {
  if (!x || !w || !bias || !y) return SIVAE_ERR_NULL;
  const int rc = rgb_check(B, C, H, W, K);
  if (rc != SIVAE_OK) return rc;
  if (prev && ((H | W) & 1)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({x, w, bias, prev, y})) return SIVAE_ERR_SHAPE;
  const int HW = H * W;
  RgbArgs a = {};
  a.x = x, a.w = w, a.bias = bias, a.aux = prev, a.y = y;
  a.C = C, a.HW = HW, a.W = W, a.cpw = cdiv(C, RGB_NW), a.blend = blend, a.omb = 1.f - blend;
  const bool al = c4_al16(HW, {x, y});
  const dim3 grid((unsigned)cdiv(HW, RGB_TILE), (unsigned)B);
  RGB_LAUNCH(rgb_to_fwd_kernel, K, al, grid, stream, a);
  return sivae_launch_status();
}

extern "C" size_t sivae_to_rgb_bwd_workspace_bytes(int B, int C, int H, int W, int K) {
  if (rgb_check(B, C, H, W, K) != SIVAE_OK) return 0;
  return ((size_t)C + 1) * rgb_blocks(B, H * W) * 4 * sizeof(float);
}

extern "C" int sivae_to_rgb_bwd(const float* dy, const float* x, const float* w, int has_prev, float blend, float* dx,
                                float* dw, float* dbias, float* dprev, int B, int C, int H, int W, int K, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
  if (!dy || !w || (dw && !x)) return SIVAE_ERR_NULL;
  const int rc = rgb_check(B, C, H, W, K);
  if (rc != SIVAE_OK) return rc;
  if (has_prev != 0 && has_prev != 1) return SIVAE_ERR_MODE;
  if (dprev && !has_prev) return SIVAE_ERR_MODE;
  if (has_prev && ((H | W) & 1)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({dy, x, w, dx, dw, dbias, dprev})) return SIVAE_ERR_SHAPE;
  const bool sums = dw || dbias;
  if (sums && (!workspace || sivae_misaligned(workspace, 16) || workspace_bytes < sivae_to_rgb_bwd_workspace_bytes(B, C, H, W, K)))
    return SIVAE_ERR_WORKSPACE;
  if (!dx && !sums && !dprev) return SIVAE_OK;
  const int HW = H * W;
  if (dx || sums) {
    RgbArgs a = {};
    a.x = x, a.w = w, a.dy = dy, a.dx = dx, a.part = sums ? static_cast<float*>(workspace) : nullptr;
    a.blended = has_prev;
    a.C = C, a.HW = HW, a.W = W, a.cpw = cdiv(C, RGB_NW), a.sums = (dw ? 1 : 0) | (dbias ? 2 : 0);
    a.blend = blend, a.omb = 1.f - blend;
    const bool al = c4_al16(HW, {dy, dw ? x : nullptr, dx});
    const dim3 grid((unsigned)cdiv(HW, RGB_TILE), (unsigned)B);
    RGB_LAUNCH(rgb_to_bwd_kernel, K, al, grid, stream, a);
    if (sums) {
      const int r0 = dw ? 0 : C, r1 = dbias ? C + 1 : C;  // rows of the partials that were written and are wanted
      hipLaunchKernelGGL((rgb_merge_kernel<4>), dim3((unsigned)(r1 - r0)), dim3(256), 0, stream,
                         a.part + (size_t)r0 * rgb_blocks(B, HW) * 4, rgb_blocks(B, HW), C - r0, dw, K, 1, C, dbias, 1);
    }
  }
  if (dprev) {
    const size_t total = (size_t)B * K * (HW / 4);
    hipLaunchKernelGGL(rgb_dprev_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dy, dprev, total, H / 2,
                       W / 2, 1.f - blend);
  }
  return sivae_launch_status();
}

// (H, W: the image's; the features are H / 2 x W / 2 when pool)
extern "C" int sivae_from_rgb_fwd(const float* img, const float* w, const float* bias, int pool, const float* other,
                                  float blend, float* y, int B, int C, int H, int W, int K, hipStream_t stream) {
  if (!img || !w || !bias || !y) return SIVAE_ERR_NULL;
  const int rc = rgb_check(B, C, H, W, K);
  if (rc != SIVAE_OK) return rc;
  if (pool != 0 && pool != 1) return SIVAE_ERR_MODE;
  if (pool && ((H | W) & 1)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({img, w, bias, other, y})) return SIVAE_ERR_SHAPE;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, HW = Ho * Wo;
  RgbArgs a = {};
  a.x = img, a.w = w, a.bias = bias, a.aux = other, a.y = y;
  a.C = C, a.HW = HW, a.W = Wo, a.cpw = cdiv(C, RGB_NW), a.pool = pool, a.blend = blend, a.omb = 1.f - blend;
  const bool al = c4_al16(HW, {pool ? nullptr : img, other, y});
  const dim3 grid((unsigned)cdiv(HW, RGB_TILE), (unsigned)B);
  RGB_LAUNCH(rgb_from_fwd_kernel, K, al, grid, stream, a);
  return sivae_launch_status();
}

extern "C" size_t sivae_from_rgb_bwd_workspace_bytes(int B, int C, int H, int W, int K, int pool) {
  if (rgb_check(B, C, H, W, K) != SIVAE_OK || (pool && ((H | W) & 1))) return 0;
  const int HW = pool ? (H / 2) * (W / 2) : H * W;
  return (size_t)C * rgb_blocks(B, HW) * (K < 4 ? 4 : 8) * sizeof(float);
}

extern "C" int sivae_from_rgb_bwd(const float* dy, const float* img, const float* w, const float* bias, int pool,
                                  int has_other, float blend, float* dimg, float* dw, float* dbias, float* dother, int B,
                                  int C, int H, int W, int K, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!dy || !img || !w || !bias) return SIVAE_ERR_NULL;
  const int rc = rgb_check(B, C, H, W, K);
  if (rc != SIVAE_OK) return rc;
  if ((pool != 0 && pool != 1) || (has_other != 0 && has_other != 1)) return SIVAE_ERR_MODE;
  if (dother && !has_other) return SIVAE_ERR_MODE;
  if (pool && ((H | W) & 1)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({dy, img, w, bias, dimg, dw, dbias, dother})) return SIVAE_ERR_SHAPE;
  const bool sums = dw || dbias;
  if (sums && (!workspace || sivae_misaligned(workspace, 16) ||
               workspace_bytes < sivae_from_rgb_bwd_workspace_bytes(B, C, H, W, K, pool)))
    return SIVAE_ERR_WORKSPACE;
  if (!dimg && !sums && !dother) return SIVAE_OK;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, HW = Ho * Wo;
  RgbArgs a = {};
  a.x = img, a.w = w, a.bias = bias, a.dy = dy, a.dx = dimg, a.daux = dother;
  a.blended = has_other;
  a.part = sums ? static_cast<float*>(workspace) : nullptr;
  a.C = C, a.HW = HW, a.W = Wo, a.cpw = cdiv(C, RGB_NW), a.pool = pool, a.blend = blend, a.omb = 1.f - blend;
  const bool al = c4_al16(HW, {dy, pool ? nullptr : img, pool ? nullptr : dimg, dother});
  const dim3 grid((unsigned)cdiv(HW, RGB_TILE), (unsigned)B);
  RGB_LAUNCH(rgb_from_bwd_kernel, K, al, grid, stream, a);
  if (sums) {
    if (K < 4)
      hipLaunchKernelGGL((rgb_merge_kernel<4>), dim3((unsigned)C), dim3(256), 0, stream, a.part, rgb_blocks(B, HW), C, dw, K, K,
                         1, dbias, 0);
    else
      hipLaunchKernelGGL((rgb_merge_kernel<8>), dim3((unsigned)C), dim3(256), 0, stream, a.part, rgb_blocks(B, HW), C, dw, K, K,
                         1, dbias, 0);
  }
  return sivae_launch_status();
}
