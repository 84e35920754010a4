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
//
// The blur in front of a decoder layer and behind an encoder norm is folded into the chains (the *_blur_* kernels, BL):
// where a chain reads a blurred tensor it takes the 9 taps from the unblurred one in memory (st_blur4: the decoder's x in
// both directions, the encoder backward's upstream gradient), where it writes one it applies the stencil before the store.
// The encoder forward recomputes the normalised neighbours from x.  The decoder backward's gradient with respect to
// blur(x) is made of other threads' registers: planes up to ST_BLUR_LDS_MAX elements are staged in LDS and blurred from
// there, larger ones are written as they are and the caller runs the blur kernel over them.  The stencil is st_blur9 for all
// of them and for style_blur_kernel, so a fused chain gives the bits of the two kernels it replaces.
#include <cmath>

#include "common.h"
#include "chunk4.h"

// No contraction of a * b + c across this file: hipcc's default fuses them as the optimiser sees fit, which differs between
// the instantiations of one kernel (measured: the last bit of dx between the 16-byte and the scalar instantiation), and
// the alignment must change no bit.  The one fused multiply-add wanted (y) is written out.
#pragma clang fp contract(off)

#define ST_SLOPE 0.2f
#define ST_MAX_HELD_FWD 65536  // elements of the largest plane the forward kernels hold in registers (1024 x 64)
#define ST_MAX_HELD_BWD 16384  // ... and the backward kernels, which hold two tensors (1024 x 16 each)
// elements of the largest plane whose gradient the decoder backward with the blur stages in LDS (one launch).  64 KiB of
// fp32: the static LDS a workgroup may declare, and with it the two 1024-thread blocks a CU holds still fit its 160 KiB,
// so the staging costs no occupancy.  The reduction scratch shares these bytes (they are never live together).
#define ST_BLUR_LDS_MAX 16384
static_assert(ST_BLUR_LDS_MAX <= ST_MAX_HELD_BWD && ST_BLUR_LDS_MAX % 4 == 0 && ST_BLUR_LDS_MAX * 4 <= 65536,
              "the staged plane is one the backward holds, in whole chunks, within a workgroup's static LDS");

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

// (the chunk of 4 elements at i of a plane of n is chunk4.h's c4_load / c4_store: 16-byte access when AL, else guarded scalars)

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

// reference: net.py:49-60.  The [1, 2, 1] x [1, 2, 1] / 16 filter at element e = h W + w of a plane [H][W] whose element q
// is at(q), zeros around the plane: rows first ((l + 2 c) + r), then ((top + 2 mid) + bottom) / 16.
template <typename I, typename F>
__device__ __forceinline__ float st_blur9(F&& at, I e, int h, int w, int H, int W) {
  float rows[3];
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    float s = 0.f;
    if (h + d >= 0 && h + d < H) {
      const I q = e + (I)d * W;
      const float l = w > 0 ? at(q - 1) : 0.f, rr = w + 1 < W ? at(q + 1) : 0.f;
      s = (l + 2.f * at(q)) + rr;
    }
    rows[d + 1] = s;
  }
  return ((rows[0] + 2.f * rows[1]) + rows[2]) * 0.0625f;
}

// The blurred chunk of 4 elements at i of a plane of n = H W (0 for those at or past n): one division a chunk, its
// elements are consecutive.  A chunk inside one row (every chunk where W % 4 == 0) takes 6 values a row for its 4
// elements, the 4 in the middle through at4(q, c) (c[j] = at(q + j)) as ONE 16-byte access where AL and W % 4 == 0 make q a
// multiple of 4 on a 16-byte aligned plane; each sum is st_blur9's, term for term.  A chunk over a row end goes element
// by element.
template <bool AL, typename F, typename F4>
__device__ __forceinline__ void st_blur4(F&& at, F4&& at4, int i, int n, int H, int W, float (&v)[4]) {
  int h = i / W, w = i - h * W;
  if (w + 3 < W) {
    float rows[3][4];
#pragma unroll
    for (int d = -1; d <= 1; ++d) {
      float(&s)[4] = rows[d + 1];
      s[0] = s[1] = s[2] = s[3] = 0.f;
      if (h + d >= 0 && h + d < H) {
        const int q = i + d * W;
        float c[4];
        if (AL && (W & 3) == 0) {
          at4(q, c);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) c[j] = at(q + j);
        }
        const float l = w > 0 ? at(q - 1) : 0.f, rr = w + 4 < W ? at(q + 4) : 0.f;
        s[0] = (l + 2.f * c[0]) + c[1];
        s[1] = (c[0] + 2.f * c[1]) + c[2];
        s[2] = (c[1] + 2.f * c[2]) + c[3];
        s[3] = (c[2] + 2.f * c[3]) + rr;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((rows[0][j] + 2.f * rows[1][j]) + rows[2][j]) * 0.0625f;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = i + j < n ? st_blur9(at, i + j, h, w, H, W) : 0.f;
    if (++w == W) w = 0, ++h;
  }
}
// ... of a plane in memory (global or LDS)
template <bool AL>
__device__ __forceinline__ void st_blur4_of(const float* __restrict__ p, int i, int n, int H, int W, float (&v)[4]) {
  st_blur4<AL>([&](int q) { return p[q]; }, [&](int q, float(&c)[4]) { c4_load<true>(p, q, n, c); }, i, n, H, W, v);
}

struct StDecFwdArgs {
  const float *x, *noise, *nw, *bias, *style;
  float *y, *mean, *rstd;
  int C, HW, mode;
  float eps, c1, c2, c3;
  int H, W;  // (read by the blur forms alone)
};

__device__ __forceinline__ StPre st_pre(const float* nw, const float* bias, int c, int mode, float c1, float c2, float c3) {
  StPre p;
  p.mode = mode, p.nw = mode ? nw[c] : 0.f, p.bias = bias[c], p.c1 = c1, p.c2 = c2, p.c3 = c3;
  return p;
}

// reference: net.py:169-185 / :189-205; BL: of blur(x) (net.py:49-60 in front of it, :166-168), read from x by 9 taps
template <int NT, int EPT, bool AL, bool BL>
__device__ __forceinline__ void st_dec_fwd(const StDecFwdArgs& a) {
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
    if constexpr (BL)
      st_blur4_of<AL>(x, i, n, a.H, a.W, xv);
    else
      c4_load<AL>(x, i, n, xv);
    if (p.mode) c4_load<AL>(nz, i, n, zv);
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
    c4_store<AL>(y, i, n, yv);
  });
  if (tid == 0) a.mean[plane] = m, a.rstd[plane] = r;
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_fwd_kernel(StDecFwdArgs a) {
  st_dec_fwd<NT, EPT, AL, false>(a);
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_blur_fwd_kernel(StDecFwdArgs a) {
  st_dec_fwd<NT, EPT, AL, true>(a);
}

struct StDecBwdArgs {
  const float *dy, *x, *noise, *nw, *bias, *style, *mean, *rstd;
  float *dx, *dstyle;
  double* part;  // [2][B C]: sum dp, sum dp noise per plane (null: neither dbias nor dnoise_weight is wanted)
  int C, HW, mode, planes;
  float c1, c2, c3;
  int H, W, stage;  // (the blur forms alone; stage: H W <= ST_BLUR_LDS_MAX, dx leaves blurred)
};

// BL: x is the UNBLURRED input, the layer's is blur(x) by 9 taps; the gradient with respect to blur(x) is formed as the
// plain form's dx and, where the plane is staged (a held plane up to ST_BLUR_LDS_MAX), blurred from LDS before the store
template <int NT, int EPT, bool AL, bool BL>
__device__ __forceinline__ void st_dec_bwd(const StDecBwdArgs& a) {
  constexpr bool HELD = EPT > 0;
  constexpr int STAGE = BL && HELD ? (NT * EPT < ST_BLUR_LDS_MAX ? NT * EPT : ST_BLUR_LDS_MAX) : 0;  // staged floats
  constexpr int RED = 2 * NT / 64;
  __shared__ __align__(16) double smem[RED > STAGE / 2 ? RED : STAGE / 2];
  double* red = smem;
  float* stage = reinterpret_cast<float*>(smem);  // (same bytes: separated from red's use by barriers)
  const int plane = blockIdx.x, b = plane / a.C, c = plane - b * a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  const float* dy = a.dy + (size_t)plane * n;
  const float* nz = a.mode == 1 ? a.noise + (size_t)b * n : a.noise;
  const StPre p = st_pre(a.nw, a.bias, c, a.mode, a.c1, a.c2, a.c3);
  const float m = a.mean[plane], r = a.rstd[plane];
  float xs[HELD ? EPT : 4], gs[HELD ? EPT : 4];

  auto load_x = [&](int i, float (&xv)[4]) {
    if constexpr (BL)
      st_blur4_of<AL>(x, i, n, a.H, a.W, xv);
    else
      c4_load<AL>(x, i, n, xv);
  };

  // sum dy and sum dy xh (a chunk's elements past n load as zero gradients)
  float s1 = 0.f, s2 = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float xv[4], gv[4], zv[4] = {0.f, 0.f, 0.f, 0.f};
    load_x(i, xv);
    c4_load<AL>(dy, i, n, gv);
    if (p.mode) c4_load<AL>(nz, i, n, zv);
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
  const bool staged = STAGE > 0 && a.stage && dx;  // (block-uniform)
  if (staged) __syncthreads();                     // (every thread has read red: its bytes take the plane now)
  float p1 = 0.f, p2 = 0.f;
  st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
    float xv[4], gv[4], zv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
    if (!HELD) {
      load_x(i, xv);
      c4_load<AL>(dy, i, n, gv);
    }
    if (p.mode) c4_load<AL>(nz, i, n, zv);  // (one plane per sample at the most: re-read from cache, not held)
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
    if (staged)
      c4_store<AL>(stage, i, n, ov);
    else if (dx)
      c4_store<AL>(dx, i, n, ov);
  });
  if (staged) {
    __syncthreads();
    st_chunks<NT, EPT>(n, tid, [&](int, int i) {
      float ov[4];
      st_blur4_of<AL>(stage, i, n, a.H, a.W, ov);
      c4_store<AL>(dx, i, n, ov);
    });
  }
  if (a.part) {
    double P1 = (double)p1, P2 = (double)p2;
    block_sum2<NT>(P1, P2, red);  // (its first barrier is behind every thread's reads of the staged plane)
    if (tid == 0) a.part[plane] = P1, a.part[a.planes + plane] = P2;
  }
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_bwd_kernel(StDecBwdArgs a) {
  st_dec_bwd<NT, EPT, AL, false>(a);
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_dec_blur_bwd_kernel(StDecBwdArgs a) {
  st_dec_bwd<NT, EPT, AL, true>(a);
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
  int H, W;  // (read by the blur form alone)
};

// reference: net.py:94-101 / :113-121; BL: xn leaves as blur(xn) (net.py:110), the neighbours' xn recomputed from x
template <int NT, int EPT, bool AL, bool BL>
__device__ __forceinline__ void st_enc_fwd(const StEncFwdArgs& a) {
  __shared__ double red[NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, c = plane % a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  float* xn = a.xn + (size_t)plane * n;
  const float bias = a.bias[c];
  float t[HELD ? EPT : 4];

  auto load_t = [&](int i, float (&tv)[4]) {
    c4_load<AL>(x, i, n, tv);
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
    if constexpr (BL) {
      auto xn_at = [&](int q) { return (st_lrelu(x[q] + bias) - m) * r; };  // (the expression the plain form stores)
      auto xn_at4 = [&](int q, float(&c)[4]) {
        c4_load<true>(x, q, n, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = (st_lrelu(c[j] + bias) - m) * r;
      };
      st_blur4<AL>(xn_at, xn_at4, i, n, a.H, a.W, yv);
    } else {
      if (!HELD) load_t(i, tv);
#pragma unroll
      for (int j = 0; j < 4; ++j) yv[j] = ((HELD ? t[4 * k + j] : tv[j]) - m) * r;
    }
    c4_store<AL>(xn, i, n, yv);
  });
  if (tid == 0) a.mean[plane] = m, a.std[plane] = (float)sqrt(v);
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_fwd_kernel(StEncFwdArgs a) {
  st_enc_fwd<NT, EPT, AL, false>(a);
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_blur_fwd_kernel(StEncFwdArgs a) {
  st_enc_fwd<NT, EPT, AL, true>(a);
}

struct StEncBwdArgs {
  const float *dxn, *dmean, *dstd, *x, *bias, *mean, *std;
  float* dx;
  double* part;  // [B C]: sum dp per plane (null: dbias is not wanted)
  int C, HW;
  float eps;
  int H, W;  // (read by the blur form alone)
};

// BL: dxn is the gradient of blur(xn); xn's is its blur (the filter is its own adjoint), read from it by 9 taps
template <int NT, int EPT, bool AL, bool BL>
__device__ __forceinline__ void st_enc_bwd(const StEncBwdArgs& a) {
  __shared__ double red[2 * NT / 64];
  constexpr bool HELD = EPT > 0;
  const int plane = blockIdx.x, c = plane % a.C, tid = threadIdx.x, n = a.HW;
  const float* x = a.x + (size_t)plane * n;
  const float* dxn = a.dxn ? a.dxn + (size_t)plane * n : nullptr;
  const float bias = a.bias[c], m = a.mean[plane], sd = a.std[plane];
  const float r = (float)(1.0 / sqrt((double)sd * (double)sd + (double)a.eps));
  float xs[HELD ? EPT : 4], gs[HELD ? EPT : 4];

  auto load_g = [&](int i, float (&gv)[4]) {
    if constexpr (BL)
      st_blur4_of<AL>(dxn, i, n, a.H, a.W, gv);
    else
      c4_load<AL>(dxn, i, n, gv);
  };

  float s1 = 0.f, s2 = 0.f;
  if (HELD || dxn) {
    st_chunks<NT, EPT>(n, tid, [&](int k, int i) {
      float xv[4], gv[4] = {0.f, 0.f, 0.f, 0.f};
      c4_load<AL>(x, i, n, xv);
      if (dxn) load_g(i, gv);
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
      c4_load<AL>(x, i, n, xv);
      if (dxn) load_g(i, gv);
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
    if (dx) c4_store<AL>(dx, i, n, ov);
  });
  if (a.part) {
    const double P1 = block_sum<NT>((double)p1, red);
    if (tid == 0) a.part[plane] = P1;
  }
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_bwd_kernel(StEncBwdArgs a) {
  st_enc_bwd<NT, EPT, AL, false>(a);
}
template <int NT, int EPT, bool AL>
__global__ void __launch_bounds__(NT) style_enc_blur_bwd_kernel(StEncBwdArgs a) {
  st_enc_bwd<NT, EPT, AL, true>(a);
}

// reference: net.py:49-60.  One thread per output element (st_blur9 around it; the taps are offsets from the element).
__global__ void __launch_bounds__(256) style_blur_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total,
                                                         int H, int W) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = (int)(e % W), h = (int)((e / W) % H);
  const float* p = x + e;
  y[e] = st_blur9([&](ptrdiff_t q) { return p[q]; }, (ptrdiff_t)0, h, w, H, W);
}

// ---------------------------------------------------------------------------------------------------- host side
static int st_check_shape(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)H * W < 2) return SIVAE_ERR_SHAPE;
  if ((long long)B * C > 0x7fffffffLL || (long long)H * W > 0x3fffffffLL) return SIVAE_ERR_RANGE;
  return SIVAE_OK;
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

// Each entry point and its *_blur_* twin share one host function: the same validation, the kernel chosen by `blur`.
static int st_dec_fwd_host(bool blur, const float* x, const float* noise, const float* noise_weight, const float* bias,
                           const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W, int mode,
                           int layer, float eps, hipStream_t stream) {
  if (!x || !bias || !style || !y || !mean || !rstd) return SIVAE_ERR_NULL;
  if (mode < 0 || mode > 2) return SIVAE_ERR_MODE;
  if (mode != 0 && (!noise || !noise_weight)) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (layer < 0 || !(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({x, noise, noise_weight, bias, style, y, mean, rstd})) return SIVAE_ERR_SHAPE;
  const int HW = H * W;
  StDecFwdArgs a = {x, mode ? noise : nullptr, noise_weight, bias, style, y, mean, rstd, C, HW, mode, eps, 0.f, 0.f, 0.f,
                    H, W};
  st_mode0_consts(layer, &a.c1, &a.c2, &a.c3);
  const bool al = c4_al16(HW, {x, a.noise, y});
  if (blur)
    ST_DISPATCH_FWD(style_dec_blur_fwd_kernel, HW, al, (long long)B * C, stream, a);
  else
    ST_DISPATCH_FWD(style_dec_fwd_kernel, HW, al, (long long)B * C, stream, a);
  return sivae_launch_status();
}

extern "C" int sivae_style_dec_fwd(const float* x, const float* noise, const float* noise_weight, const float* bias,
                                   const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W,
                                   int mode, int layer, float eps, hipStream_t stream) {
  return st_dec_fwd_host(false, x, noise, noise_weight, bias, style, y, mean, rstd, B, C, H, W, mode, layer, eps, stream);
}
extern "C" int sivae_style_dec_blur_fwd(const float* x, const float* noise, const float* noise_weight, const float* bias,
                                        const float* style, float* y, float* mean, float* rstd, int B, int C, int H, int W,
                                        int mode, int layer, float eps, hipStream_t stream) {
  return st_dec_fwd_host(true, x, noise, noise_weight, bias, style, y, mean, rstd, B, C, H, W, mode, layer, eps, stream);
}

extern "C" size_t sivae_style_dec_bwd_workspace_bytes(int B, int C) {
  return B > 0 && C > 0 ? 2 * (size_t)B * (size_t)C * sizeof(double) : 0;
}
extern "C" size_t sivae_style_dec_blur_bwd_workspace_bytes(int B, int C) { return sivae_style_dec_bwd_workspace_bytes(B, C); }

extern "C" int sivae_style_dec_blur_bwd_fused(int H, int W) {
  return H > 0 && W > 0 && (long long)H * W <= ST_BLUR_LDS_MAX ? 1 : 0;
}

static int st_dec_bwd_host(bool blur, const float* dy, const float* x, const float* noise, const float* noise_weight,
                           const float* bias, const float* style, const float* mean, const float* rstd, float* dx,
                           float* dnoise_weight, float* dbias, float* dstyle, int B, int C, int H, int W, int mode, int layer,
                           void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!dy || !x || !bias || !style || !mean || !rstd) return SIVAE_ERR_NULL;
  if (mode < 0 || mode > 2) return SIVAE_ERR_MODE;
  if (mode != 0 && (!noise || !noise_weight)) return SIVAE_ERR_NULL;
  if (mode == 0 && dnoise_weight) return SIVAE_ERR_MODE;  // (no noise tensor: noise_weight has no gradient)
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (layer < 0) return SIVAE_ERR_SHAPE;
  if (!c4_al4({dy, x, noise, noise_weight, bias, style, mean, rstd, dx, dnoise_weight, dbias, dstyle}))
    return SIVAE_ERR_SHAPE;
  const bool sums = dbias || dnoise_weight;
  if (sums && (!workspace || sivae_misaligned(workspace, 8) || workspace_bytes < sivae_style_dec_bwd_workspace_bytes(B, C)))
    return SIVAE_ERR_WORKSPACE;
  if (!dx && !sums && !dstyle) return SIVAE_OK;
  const int HW = H * W;
  StDecBwdArgs a = {dy, x, mode ? noise : nullptr, noise_weight, bias, style, mean, rstd, dx, dstyle,
                    sums ? static_cast<double*>(workspace) : nullptr, C, HW, mode, B * C, 0.f, 0.f, 0.f,
                    H, W, sivae_style_dec_blur_bwd_fused(H, W)};
  st_mode0_consts(layer, &a.c1, &a.c2, &a.c3);
  const bool al = c4_al16(HW, {dy, x, a.noise, dx});
  if (blur)
    ST_DISPATCH_BWD(style_dec_blur_bwd_kernel, HW, al, (long long)B * C, stream, a);
  else
    ST_DISPATCH_BWD(style_dec_bwd_kernel, HW, al, (long long)B * C, stream, a);
  if (sums)
    hipLaunchKernelGGL(style_batch_sum_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, stream, a.part, dbias,
                       dnoise_weight, B, C);
  return sivae_launch_status();
}

extern "C" int sivae_style_dec_bwd(const float* dy, const float* x, const float* noise, const float* noise_weight,
                                   const float* bias, const float* style, const float* mean, const float* rstd, float* dx,
                                   float* dnoise_weight, float* dbias, float* dstyle, int B, int C, int H, int W, int mode,
                                   int layer, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return st_dec_bwd_host(false, dy, x, noise, noise_weight, bias, style, mean, rstd, dx, dnoise_weight, dbias, dstyle, B, C,
                         H, W, mode, layer, workspace, workspace_bytes, stream);
}
extern "C" int sivae_style_dec_blur_bwd(const float* dy, const float* x, const float* noise, const float* noise_weight,
                                        const float* bias, const float* style, const float* mean, const float* rstd,
                                        float* dx, float* dnoise_weight, float* dbias, float* dstyle, int B, int C, int H,
                                        int W, int mode, int layer, void* workspace, size_t workspace_bytes,
                                        hipStream_t stream) {
  return st_dec_bwd_host(true, dy, x, noise, noise_weight, bias, style, mean, rstd, dx, dnoise_weight, dbias, dstyle, B, C,
                         H, W, mode, layer, workspace, workspace_bytes, stream);
}

static int st_enc_fwd_host(bool blur, const float* x, const float* bias, float* xn, float* mean, float* stddev, int B, int C,
                           int H, int W, float eps, hipStream_t stream) {
  if (!x || !bias || !xn || !mean || !stddev) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (!(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({x, bias, xn, mean, stddev})) return SIVAE_ERR_SHAPE;
  const int HW = H * W;
  const StEncFwdArgs a = {x, bias, xn, mean, stddev, C, HW, eps, H, W};
  const bool al = c4_al16(HW, {x, xn});
  if (blur)
    ST_DISPATCH_FWD(style_enc_blur_fwd_kernel, HW, al, (long long)B * C, stream, a);
  else
    ST_DISPATCH_FWD(style_enc_fwd_kernel, HW, al, (long long)B * C, stream, a);
  return sivae_launch_status();
}

extern "C" int sivae_style_enc_fwd(const float* x, const float* bias, float* xn, float* mean, float* stddev, int B, int C,
                                   int H, int W, float eps, hipStream_t stream) {
  return st_enc_fwd_host(false, x, bias, xn, mean, stddev, B, C, H, W, eps, stream);
}
extern "C" int sivae_style_enc_blur_fwd(const float* x, const float* bias, float* bxn, float* mean, float* stddev, int B,
                                        int C, int H, int W, float eps, hipStream_t stream) {
  return st_enc_fwd_host(true, x, bias, bxn, mean, stddev, B, C, H, W, eps, stream);
}

extern "C" size_t sivae_style_enc_bwd_workspace_bytes(int B, int C) {
  return B > 0 && C > 0 ? (size_t)B * (size_t)C * sizeof(double) : 0;
}
extern "C" size_t sivae_style_enc_blur_bwd_workspace_bytes(int B, int C) { return sivae_style_enc_bwd_workspace_bytes(B, C); }

static int st_enc_bwd_host(bool blur, const float* dxn, const float* dmean, const float* dstd, const float* x,
                           const float* bias, const float* mean, const float* stddev, float* dx, float* dbias, int B, int C,
                           int H, int W, float eps, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!x || !bias || !mean || !stddev) return SIVAE_ERR_NULL;
  const int rc = st_check_shape(B, C, H, W);
  if (rc != SIVAE_OK) return rc;
  if (!(eps >= 0.f)) return SIVAE_ERR_SHAPE;
  if (!c4_al4({dxn, dmean, dstd, x, bias, mean, stddev, dx, dbias})) return SIVAE_ERR_SHAPE;
  if (dbias && (!workspace || sivae_misaligned(workspace, 8) || workspace_bytes < sivae_style_enc_bwd_workspace_bytes(B, C)))
    return SIVAE_ERR_WORKSPACE;
  if (!dx && !dbias) return SIVAE_OK;
  const int HW = H * W;
  const StEncBwdArgs a = {dxn, dmean, dstd, x, bias, mean, stddev, dx, dbias ? static_cast<double*>(workspace) : nullptr,
                          C, HW, eps, H, W};
  const bool al = c4_al16(HW, {dxn, x, dx});
  if (blur)
    ST_DISPATCH_BWD(style_enc_blur_bwd_kernel, HW, al, (long long)B * C, stream, a);
  else
    ST_DISPATCH_BWD(style_enc_bwd_kernel, HW, al, (long long)B * C, stream, a);
  if (dbias)
    hipLaunchKernelGGL(style_batch_sum_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, stream, a.part, dbias,
                       static_cast<float*>(nullptr), B, C);
  return sivae_launch_status();
}

extern "C" int sivae_style_enc_bwd(const float* dxn, const float* dmean, const float* dstd, const float* x, const float* bias,
                                   const float* mean, const float* stddev, float* dx, float* dbias, int B, int C, int H,
                                   int W, float eps, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return st_enc_bwd_host(false, dxn, dmean, dstd, x, bias, mean, stddev, dx, dbias, B, C, H, W, eps, workspace,
                         workspace_bytes, stream);
}
extern "C" int sivae_style_enc_blur_bwd(const float* dbxn, const float* dmean, const float* dstd, const float* x,
                                        const float* bias, const float* mean, const float* stddev, float* dx, float* dbias,
                                        int B, int C, int H, int W, float eps, void* workspace, size_t workspace_bytes,
                                        hipStream_t stream) {
  return st_enc_bwd_host(true, dbxn, dmean, dstd, x, bias, mean, stddev, dx, dbias, B, C, H, W, eps, workspace,
                         workspace_bytes, stream);
}

extern "C" int sivae_style_blur(const float* x, float* y, int B, int C, int H, int W, hipStream_t stream) {
  if (!x || !y) return SIVAE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return SIVAE_ERR_SHAPE;
  if (!c4_al4({x, y})) return SIVAE_ERR_SHAPE;
  const size_t total = (size_t)B * C * H * W;
  if (total > 256ull * 0x7fffffffull) return SIVAE_ERR_RANGE;
  hipLaunchKernelGGL(style_blur_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, total, H, W);
  return sivae_launch_status();
}
