// The weight transform of the style variant's fused_scale convolutions (style_soft_intro_vae/net.py:77,:138, built with
// transform_kernel=True; lreq.py:142-164: F.conv_transpose2d / F.conv2d with stride 2 over the 4x4 kernel summed from four
// shifted copies of the 3x3 weight).
//
// Those layers ARE 3x3 convolutions around a nearest-2x upsample:
//   up,   w [Ci][Co][3][3]:  conv_transpose2d(x, S(w), stride 2, padding 1) = conv3x3(upsample2(x), T(w))
//   down, w [Co][Ci][3][3]:  conv2d(x, S(w) / 4, stride 2, padding 1)       = the adjoint of z -> conv3x3(upsample2(z), T(w) / 4)
// with T(w)[o][i][a][b] = w[i][o][2 - a][2 - b]: the two channel axes swapped, both kernel axes reversed.  The phase-form
// kernels (conv_wino_up*.hip) run both once they are handed T(w); this file is T, with a scale.  T is its own inverse up
// to the swap of the sizes, so the same kernel also carries the weight gradient of the effective weight back into the
// parameter's layout.
#include <hip/hip_runtime.h>

#include "common.h"

// One thread per DESTINATION element, so every store instruction of a wave covers 64 consecutive floats (dst may sit at
// any 4-byte-aligned address: the gradient slabs are views at arbitrary element offsets, hence no wider stores).  The
// reads walk src in runs of 9 contiguous floats (one 3x3 kernel, reversed) S * 36 bytes apart; the tensor is at most
// 512 * 512 * 9 floats and the neighbouring blocks consume the rest of each line from L2, so there is no LDS transpose.
__global__ __launch_bounds__(256) void conv3x3_flip_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                     int R, int S, float scale, unsigned total) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= total) return;
  const unsigned k = e % 9u, sr = e / 9u;  // dst[s][r][k / 3][k % 3]
  const unsigned r = sr % (unsigned)R, s = sr / (unsigned)R;
  dst[e] = scale * src[(r * (unsigned)S + s) * 9u + (8u - k)];
}

extern "C" int sivae_conv3x3_flip_transpose(const float* src, float* dst, int R, int S, float scale, hipStream_t stream) {
  if (!src || !dst) return SIVAE_ERR_NULL;
  if (R <= 0 || S <= 0) return SIVAE_ERR_SHAPE;
  if (sivae_misaligned(src, 4) || sivae_misaligned(dst, 4)) return SIVAE_ERR_SHAPE;
  const long long total = 9ll * R * S;
  if (total > 0x7fffffffLL) return SIVAE_ERR_RANGE;
  hipLaunchKernelGGL(conv3x3_flip_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, dst, R,
                     S, scale, (unsigned)total);
  return sivae_launch_status();
}
