// The style variant's non-conv layers (reference: style_soft_intro_vae/net.py): what follows every 3x3 convolution of the
// ALAE / StyleGAN-shaped generator (net.py:169-185 and :189-205: noise injection -> bias -> LeakyReLU(0.2) -> InstanceNorm
// -> style modulation) and of the encoder (net.py:94-101 and :113-121: bias -> LeakyReLU(0.2) -> (mean, std) ->
// InstanceNorm), each chain as ONE forward and ONE backward kernel, and the depthwise blur (net.py:49-60).  fp32, NCHW.
//
// One block owns one (b, c) plane.  A thread owns the 4-element chunks tid, tid + NT, ... of the plane; up to NT * EPT
// elements the chunks stay in registers between the statistics and the apply step (one read of the plane per direction),
// beyond that the plane is streamed again from memory.  The configuration (NT, EPT) depends on H * W alone, and a
// thread's chunks are the same whether they are read with 16-byte loads (every plane 16-byte aligned) or with guarded
// scalar loads (any other base or an H * W that is no multiple of 4, where the last chunk is the scalar tail): every sum
// is a thread's elements in index order in fp32, then the wave butterfly and the waves in index order in fp64.  So a
// plane's results depend neither on B, on C, on the other planes nor on the alignment, and two runs are bit-identical.
// No atomics.  The sums over the batch (dbias, dnoise_weight) go through per-plane fp64 partials in the workspace and a
// second small launch that adds them in ascending b.
#include <cmath>
#include <initializer_list>

#include "common.h"

// No contraction of a * b + c across this file: hipcc's default fuses them as the optimiser sees fit, which differs between
// the instantiations of one kernel (measured: the last bit of dx between the 16-byte and the scalar instantiation), and
// the alignment must change no bit.  The one fused multiply-add wanted (y) is written out.
#pragma clang fp contract(off)

#define ST_SLOPE 0.2f
#define ST_MAX_HELD_FWD 65536  // elements of the largest plane the forward kernels hold in registers (1024 x 64)
#define ST_MAX_HELD_BWD 16384  // ... and the backward kernels, which hold two tensors (1024 x 16 each)

// how the pre-activation is formed from x (block-uniform)
struct StPre {
  int mode;    // 0: x + c1 exp(c2 x^2);  1, 2: x + nw noise
  float nw;    // noise_weight[c]
  float bias;  // bias[c]
  float c1;    // s 0.8 / sqrt(2 pi), s = sqrt(layer + 1)
  float c2;    // -1 / (2 s^2)
  float c3;    // -(0.8 / sqrt(2 pi)) / s: d/dx of c1 exp(c2 x^2) is c3 x exp(c2 x^2)
};

__device__ __forceinline__ float st_lrelu(float p) { return p > 0.f ? p : p * ST_SLOPE; }

__device__ __forceinline__ float st_dec_t(float x, float nz, const StPre& p) {
  const float u = p.mode == 0 ? x + p.c1 * expf(p.c2 * x * x) : x + p.nw * nz;
  return st_lrelu(u + p.bias);
}

// the chunk of 4 elements at i of a plane of n: 16-byte access when AL (then n % 4 == 0 and i < n), else guarded scalars
template <bool AL>
__device__ __forceinline__ void st_load4(const float* __restrict__ p, int i, int n, float (&v)[4]) {
  if (AL) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.f;
  }
}
template <bool AL>
__device__ __forceinline__ void st_store4(float* __restrict__ p, int i, int n, const float (&v)[4]) {
  if (AL) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

// f(k, i) for every chunk of the thread: k the chunk's register slot (compile-time after unrolling, HELD only), i its
// first element.  HELD: the EPT / 4 slots, those at or past n skipped; streamed: as many as the plane has.
template <int NT, int EPT, typename F>
__device__ __forceinline__ void st_chunks(int n, int tid, F&& f) {
  if constexpr (EPT > 0) {
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const int i = (k * NT + tid) * 4;
      if (i < n) f(k, i);
    }
  } else {
    for (int i = tid * 4; i < n; i += NT * 4) f(0, i);
  }
}

struct StDecFwdArgs {
  const float *x, *noise, *nw, *bias, *style;
  float *y, *mean, *rstd;
  int C, HW, mode;
  float eps, c1, c2, c3;
};

__device__ __forceinline__ StPre st_pre(const float* nw, const float* bias, int c, int mode, float c1, float c2, float c3) {
  StPre p;
  p.mode = mode, p.nw = mode ? nw[c] : 0.f, p.bias = bias[c], p.c1 = c1, p.c2 = c2, p.c3 = c3;
  return p;
}

// reference: net.py:169-185 / :189-205
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_fwd_kernel(StDecFwdArgs a) {
  __shared__ double red[NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, b = plane / a.C, c = plane - b * a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  const float* nz = a.mode == 1 ? a.noise + (size_t)b * n : a.noise;  // (mode 2: one plane for the whole batch)
  float* y = a.y + (size_t)plane * n;
  const StPre p = st_pre(a.nw, a.bias, c, a.mode, a.c1, a.c2, a.c3);
  float t[HELD ? EPT : 4];

  auto load_t = [&](int i, float (&tv)[4]) {
    float xv[4], zv[4] = {0.f, 0.f, 0.f, 0.f};
    st_load4<AL>(x, i, n, xv);
    if (p.mode) st_load4<AL>(nz, i, n, zv);
#pragma unroll
    for (int j = 0; j < 4; ++j) tv[j] = st_dec_t(xv[j], zv[j], p);
  };

  float acc = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4];
    load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (HELD) t[4 * k + j] = tv[j];
      acc += (AL || i + j < n) ? tv[j] : 0.f;
    }
  });
  const float m = (float)(block_sum<NT>((double)acc, red) / (double)n);
  acc = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4];
    if (!HELD) load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (HELD ? t[4 * k + j] : tv[j]) - m;
      acc += (AL || i + j < n) ? d * d : 0.f;
    }
  });
  const double v = block_sum<NT>((double)acc, red) / (double)n;
  const float r = (float)(1.0 / sqrt(v + (double)a.eps));
  const float scale = a.style[(size_t)b * 2 * a.C + c] + 1.f, shift = a.style[(size_t)b * 2 * a.C + a.C + c];
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4], yv[4];
    if (!HELD) load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = fmaf(((HELD ? t[4 * k + j] : tv[j]) - m) * r, scale, shift);
    st_store4<AL>(y, i, n, yv);
  });
  if (tid == 0) a.mean[plane] = m, a.rstd[plane] = r;
}

struct StDecBwdArgs {
  const float *dy, *x, *noise, *nw, *bias, *style, *mean, *rstd;
  float *dx, *dstyle;
  double* part;  // [2][B C]: sum dp, sum dp noise per plane (null: neither dbias nor dnoise_weight is wanted)
  int C, HW, mode, planes;
  float c1, c2, c3;
};

template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_bwd_kernel(StDecBwdArgs a) {
  __shared__ double red[2 * NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, b = plane / a.C, c = plane - b * a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  const float* dy = a.dy + (size_t)plane * n;
  const float* nz = a.mode == 1 ? a.noise + (size_t)b * n : a.noise;
  const StPre p = st_pre(a.nw, a.bias, c, a.mode, a.c1, a.c2, a.c3);
  const float m = a.mean[plane], r = a.rstd[plane];
  float xs[HELD ? EPT : 4], gs[HELD ? EPT : 4];

  // sum dy and sum dy xh (a chunk's elements past n load as zero gradients)
  float s1 = 0.f, s2 = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float xv[4], gv[4], zv[4] = {0.f, 0.f, 0.f, 0.f};
    st_load4<AL>(x, i, n, xv);
    st_load4<AL>(dy, i, n, gv);
    if (p.mode) st_load4<AL>(nz, i, n, zv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (HELD) xs[4 * k + j] = xv[j], gs[4 * k + j] = gv[j];
      const float xh = (st_dec_t(xv[j], zv[j], p) - m) * r;
      s1 += gv[j];
      s2 += gv[j] * xh;
    }
  });
  double S1 = (double)s1, S2 = (double)s2;
  block_sum2<NT>(S1, S2, red);
  if (a.dstyle && tid == 0) {
    a.dstyle[(size_t)b * 2 * a.C + c] = (float)S2;
    a.dstyle[(size_t)b * 2 * a.C + a.C + c] = (float)S1;
  }
  if (!a.dx && !a.part) return;
  const float k1 = (float)(S1 / (double)n), k2 = (float)(S2 / (double)n);
  const float g = r * (a.style[(size_t)b * 2 * a.C + c] + 1.f);
  float* dx = a.dx ? a.dx + (size_t)plane * n : nullptr;
  float p1 = 0.f, p2 = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float xv[4], gv[4], zv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
    if (!HELD) {
      st_load4<AL>(x, i, n, xv);
      st_load4<AL>(dy, i, n, gv);
    }
    if (p.mode) st_load4<AL>(nz, i, n, zv);  // (one plane per sample at the most: re-read from cache, not held)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xe = HELD ? xs[4 * k + j] : xv[j], ge = HELD ? gs[4 * k + j] : gv[j];
      const float t = st_dec_t(xe, zv[j], p);
      const float xh = (t - m) * r;
      float dp = g * (ge - k1 - xh * k2) * (t > 0.f ? 1.f : ST_SLOPE);
      if (!AL && i + j >= n) dp = 0.f;
      p1 += dp;
      p2 += dp * zv[j];
      ov[j] = p.mode ? dp : dp * (1.f + p.c3 * xe * expf(p.c2 * xe * xe));
    }
    if (dx) st_store4<AL>(dx, i, n, ov);
  });
  if (a.part) {
    double P1 = (double)p1, P2 = (double)p2;
    block_sum2<NT>(P1, P2, red);
    if (tid == 0) a.part[plane] = P1, a.part[a.planes + plane] = P2;
  }
}

// out0[c] = sum_b part[b C + c], out1[c] = sum_b part[B C + b C + c], b ascending (either output may be null)
__global__ void __launch_bounds__(256) style_batch_sum_kernel(const double* __restrict__ part, float* __restrict__ out0,
                                                              float* __restrict__ out1, int B, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s0 = 0.0, s1 = 0.0;
  for (int b = 0; b < B; ++b) {
    s0 += part[(size_t)b * C + c];
    if (out1) s1 += part[(size_t)B * C + (size_t)b * C + c];
  }
  if (out0) out0[c] = (float)s0;
  if (out1) out1[c] = (float)s1;
}

struct StEncFwdArgs {
  const float *x, *bias;
  float *xn, *mean, *std;
  int C, HW;
  float eps;
};

// reference: net.py:94-101 / :113-121
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_fwd_kernel(StEncFwdArgs a) {
  __shared__ double red[NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, c = plane % a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  float* xn = a.xn + (size_t)plane * n;
  const float bias = a.bias[c];
  float t[HELD ? EPT : 4];

  auto load_t = [&](int i, float (&tv)[4]) {
    st_load4<AL>(x, i, n, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) tv[j] = st_lrelu(tv[j] + bias);
  };

  float acc = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4];
    load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (HELD) t[4 * k + j] = tv[j];
      acc += (AL || i + j < n) ? tv[j] : 0.f;
    }
  });
  const float m = (float)(block_sum<NT>((double)acc, red) / (double)n);
  acc = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4];
    if (!HELD) load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (HELD ? t[4 * k + j] : tv[j]) - m;
      acc += (AL || i + j < n) ? d * d : 0.f;
    }
  });
  const double v = block_sum<NT>((double)acc, red) / (double)n;
  const float r = (float)(1.0 / sqrt(v + (double)a.eps));
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float tv[4], yv[4];
    if (!HELD) load_t(i, tv);
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = ((HELD ? t[4 * k + j] : tv[j]) - m) * r;
    st_store4<AL>(xn, i, n, yv);
  });
  if (tid == 0) a.mean[plane] = m, a.std[plane] = (float)sqrt(v);
}

struct StEncBwdArgs {
  const float *dxn, *dmean, *dstd, *x, *bias, *mean, *std;
  float* dx;
  double* part;  // [B C]: sum dp per plane (null: dbias is not wanted)
  int C, HW;
  float eps;
};

template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_bwd_kernel(StEncBwdArgs a) {
  __shared__ double red[2 * NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, c = plane % a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  const float* dxn = a.dxn ? a.dxn + (size_t)plane * n : nullptr;
  const float bias = a.bias[c], m = a.mean[plane], sd = a.std[plane];
  const float r = (float)(1.0 / sqrt((double)sd * (double)sd + (double)a.eps));
  float xs[HELD ? EPT : 4], gs[HELD ? EPT : 4];

  float s1 = 0.f, s2 = 0.f;
  if (HELD || dxn) {
    st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
      float xv[4], gv[4] = {0.f, 0.f, 0.f, 0.f};
      st_load4<AL>(x, i, n, xv);
      if (dxn) st_load4<AL>(dxn, i, n, gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (HELD) xs[4 * k + j] = xv[j], gs[4 * k + j] = gv[j];
        s1 += gv[j];
        s2 += gv[j] * ((st_lrelu(xv[j] + bias) - m) * r);
      }
    });
  }
  double S1 = (double)s1, S2 = (double)s2;
  if (dxn) block_sum2<NT>(S1, S2, red);
  const float k1 = (float)(S1 / (double)n), k2 = (float)(S2 / (double)n);
  const float cm = a.dmean ? a.dmean[plane] / (float)n : 0.f;
  // std == 0 (a constant plane): the derivative of the square root does not exist there; the dstd term is dropped
  const float cs = (a.dstd && sd > 0.f) ? a.dstd[plane] / ((float)n * sd) : 0.f;
  float* dx = a.dx ? a.dx + (size_t)plane * n : nullptr;
  float p1 = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float xv[4], gv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
    if (!HELD) {
      st_load4<AL>(x, i, n, xv);
      if (dxn) st_load4<AL>(dxn, i, n, gv);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xe = HELD ? xs[4 * k + j] : xv[j], ge = HELD ? gs[4 * k + j] : gv[j];
      const float t = st_lrelu(xe + bias);
      const float d = t - m;
      float dp = (r * (ge - k1 - d * r * k2) + cm + cs * d) * (t > 0.f ? 1.f : ST_SLOPE);
      if (!AL && i + j >= n) dp = 0.f;
      p1 += dp;
      ov[j] = dp;
    }
    if (dx) st_store4<AL>(dx, i, n, ov);
  });
  if (a.part) {
    const double P1 = block_sum<NT>((double)p1, red);
    if (tid == 0) a.part[plane] = P1;
  }
}

// reference: net.py:49-60.  One thread per output element; rows first ((l + 2 c) + r), then ((top + 2 mid) + bottom) / 16.
__global__ void __launch_bounds__(256) style_blur_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total,
                                                         int H, int W) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = (int)(e % W), h = (int)((e / W) % H);
  float rows[3];
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    float s = 0.f;
    if (h + d >= 0 && h + d < H) {
      const float* p = x + ((ptrdiff_t)e + (ptrdiff_t)d * W);
      const float l = w > 0 ? p[-1] : 0.f, rr = w + 1 < W ? p[1] : 0.f;
      s = (l + 2.f * p[0]) + rr;
    }
    rows[d + 1] = s;
  }
  y[e] = ((rows[0] + 2.f * rows[1]) + rows[2]) * 0.0625f;
}

// ---------------------------------------------------------------------------------------------------- host side
static int st_check_shape(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)H * W < 2) return SIVAE_ERR_SHAPE;
  if ((long long)B * C > 0x7fffffffLL || (long long)H * W > 0x3fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
}

static bool st_al16(int HW, std::initializer_list<const void*> ptrs) {
  if (HW % 4) return false;
  for (const void* p : ptrs)
    if (p && sivae_misaligned(p, 16)) return false;
  return true;
}
static bool st_al4(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && sivae_misaligned(p, 4)) return false;
  return true;
}

static void st_mode0_consts(int layer, float* c1, float* c2, float* c3) {
  const double k = 0.8 / sqrt(2.0 * M_PI), s = sqrt((double)layer + 1.0);
  *c1 = (float)(s * k), *c2 = (float)(-1.0 / (2.0 * s * s)), *c3 = (float)(-k / s);
}

#define ST_LAUNCH(KERN, NT, EPT, al, planes, stream, args)                                         \
  do {                                                                                             \
    if (al)                                                                                        \
      hipLaunchKernelGGL((KERN<NT, EPT, true>), dim3((unsigned)(planes)), dim3(NT), 0, stream, args);  \
    else                                                                                           \
      hipLaunchKernelGGL((KERN<NT, EPT, false>), dim3((unsigned)(planes)), dim3(NT), 0, stream, args); \
  } while (0)

// forward: one tensor held (up to 64 elements a thread at 1024 threads)
#define ST_DISPATCH_FWD(KERN, HW, al, planes, stream, args)                        \
  do {                                                                             \
    if ((HW) <= 256) ST_LAUNCH(KERN, 64, 4, al, planes, stream, args);             \
    else if ((HW) <= 1024) ST_LAUNCH(KERN, 256, 4, al, planes, stream, args);      \
    else if ((HW) <= 4096) ST_LAUNCH(KERN, 256, 16, al, planes, stream, args);     \
    else if ((HW) <= 16384) ST_LAUNCH(KERN, 1024, 16, al, planes, stream, args);   \
    else if ((HW) <= ST_MAX_HELD_FWD) ST_LAUNCH(KERN, 1024, 64, al, planes, stream, args); \
    else ST_LAUNCH(KERN, 1024, 0, al, planes, stream, args);                       \
  } while (0)

// backward: two tensors held (up to 2 x 16 elements a thread); larger planes are read twice
#define ST_DISPATCH_BWD(KERN, HW, al, planes, stream, args)                        \
  do {                                                                             \
    if ((HW) <= 256) ST_LAUNCH(KERN, 64, 4, al, planes, stream, args);             \
    else if ((HW) <= 1024) ST_LAUNCH(KERN, 256, 4, al, planes, stream, args);      \
    else if ((HW) <= 4096) ST_LAUNCH(KERN, 256, 16, al, planes, stream, args);     \
    else if ((HW) <= ST_MAX_HELD_BWD) ST_LAUNCH(KERN, 1024, 16, al, planes, stream, args); \
    else ST_LAUNCH(KERN, 1024, 0, al, planes, stream, args);                       \
  } while (0)

extern "C" int sivae_style_dec_fwd(const float* x, const float* noise, const float* noise_weight, const float* bias,
                                   const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W,
                                   int mode, int layer, float eps, hipStream_t stream) {
  if (!x || !bias || !style || !y || !mean || !rstd) return SIVAE_ERR_NULL;
  if (mode < 0 || mode > 2) return SIVAE_ERR_MODE;
  if (mode != 0 && (!noise || !noise_weight)) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (layer < 0 || !(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!st_al4({x, noise, noise_weight, bias, style, y, mean, rstd})) return SIVAE_ERR_SHAPE;
  const int HW = H * W;
  StDecFwdArgs a = {x, mode ? noise : nullptr, noise_weight, bias, style, y, mean, rstd, C, HW, mode, eps, 0.f, 0.f, 0.f};
  st_mode0_consts(layer, &a.c1, &a.c2, &a.c3);
  const bool al = st_al16(HW, {x, a.noise, y});
  ST_DISPATCH_FWD(style_dec_fwd_kernel, HW, al, (long long)B * C, stream, a);
  return sivae_launch_status();
}

extern "C" size_t sivae_style_dec_bwd_workspace_bytes(int B, int C) {
  return B > 0 && C > 0 ? 2 * (size_t)B * (size_t)C * sizeof(double) : 0;
}

extern "C" int sivae_style_dec_bwd(const float* dy, const float* x, const float* noise, const float* noise_weight,
                                   const float* bias, const float* style, const float* mean, const float* rstd, float* dx,
                                   float* dnoise_weight, float* dbias, float* dstyle, int B, int C, int H, int W, int mode,
                                   int layer, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!dy || !x || !bias || !style || !mean || !rstd) return SIVAE_ERR_NULL;
  if (mode < 0 || mode > 2) return SIVAE_ERR_MODE;
  if (mode != 0 && (!noise || !noise_weight)) return SIVAE_ERR_NULL;
  if (mode == 0 && dnoise_weight) return SIVAE_ERR_MODE;  // (no noise tensor: noise_weight has no gradient)
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (layer < 0) return SIVAE_ERR_SHAPE;
  if (!st_al4({dy, x, noise, noise_weight, bias, style, mean, rstd, dx, dnoise_weight, dbias, dstyle}))
    return SIVAE_ERR_SHAPE;
  const bool sums = dbias || dnoise_weight;
  if (sums && (!workspace || sivae_misaligned(workspace, 8) || workspace_bytes < sivae_style_dec_bwd_workspace_bytes(B, C)))
    return SIVAE_ERR_WORKSPACE;
  if (!dx && !sums && !dstyle) return SIVAE_OK;
  const int HW = H * W;
  StDecBwdArgs a = {dy, x, mode ? noise : nullptr, noise_weight, bias, style, mean, rstd, dx, dstyle,
                    sums ? static_cast<double*>(workspace) : nullptr, C, HW, mode, B * C, 0.f, 0.f, 0.f};
  st_mode0_consts(layer, &a.c1, &a.c2, &a.c3);
  const bool al = st_al16(HW, {dy, x, a.noise, dx});
  ST_DISPATCH_BWD(style_dec_bwd_kernel, HW, al, (long long)B * C, stream, a);
  if (sums)
    hipLaunchKernelGGL(style_batch_sum_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, stream, a.part, dbias,
                       dnoise_weight, B, C);
  return sivae_launch_status();
}

extern "C" int sivae_style_enc_fwd(const float* x, const float* bias, float* xn, float* mean, float* stddev, int B, int C,
                                   int H, int W, float eps, hipStream_t stream) {
  if (!x || !bias || !xn || !mean || !stddev) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (!(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!st_al4({x, bias, xn, mean, stddev})) return SIVAE_ERR_SHAPE;
  const int HW = H * W;
  const StEncFwdArgs a = {x, bias, xn, mean, stddev, C, HW, eps};
  const bool al = st_al16(HW, {x, xn});
  ST_DISPATCH_FWD(style_enc_fwd_kernel, HW, al, (long long)B * C, stream, a);
  return sivae_launch_status();
}

extern "C" size_t sivae_style_enc_bwd_workspace_bytes(int B, int C) {
  return B > 0 && C > 0 ? (size_t)B * (size_t)C * sizeof(double) : 0;
}

extern "C" int sivae_style_enc_bwd(const float* dxn, const float* dmean, const float* dstd, const float* x, const float* bias,
                                   const float* mean, const float* stddev, float* dx, float* dbias, int B, int C, int H,
                                   int W, float eps, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!x || !bias || !mean || !stddev) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (!(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!st_al4({dxn, dmean, dstd, x, bias, mean, stddev, dx, dbias})) return SIVAE_ERR_SHAPE;
  if (dbias && (!workspace || sivae_misaligned(workspace, 8) || workspace_bytes < sivae_style_enc_bwd_workspace_bytes(B, C)))
    return SIVAE_ERR_WORKSPACE;
  if (!dx && !dbias) return SIVAE_OK;
  const int HW = H * W;
  const StEncBwdArgs a = {dxn, dmean, dstd, x, bias, mean, stddev, dx, dbias ? static_cast<double*>(workspace) : nullptr,
                          C, HW, eps};
  const bool al = st_al16(HW, {dxn, x, dx});
  ST_DISPATCH_BWD(style_enc_bwd_kernel, HW, al, (long long)B * C, stream, a);
  if (dbias)
    hipLaunchKernelGGL(style_batch_sum_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, stream, a.part, dbias,
                       static_cast<float*>(nullptr), B, C);
  return sivae_launch_status();
}

extern "C" int sivae_style_blur(const float* x, float* y, int B, int C, int H, int W, hipStream_t stream) {
  if (!x || !y) return SIVAE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return SIVAE_ERR_SHAPE;
  if (!st_al4({x, y})) return SIVAE_ERR_SHAPE;
  const size_t total = (size_t)B * C * H * W;
  if (total > 256ull * 0x7fffffffull) return SIVAE_ERR_RANGE;
  hipLaunchKernelGGL(style_blur_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, total, H, W);
  return sivae_launch_status();
}
