// Multi-tensor launches for the style variant's optimizer (reference: style_soft_intro_vae/custom_adam.py:52-95, the
// LREQAdam step, and model.py:328-329, the weight average): one launch walks MANY tensors, where torch issues five
// element-wise launches per tensor for the step and one per tensor for the average.  fp32.
//
// The step, per element, every operation rounded to fp32 and none contracted (operation order as written):
//   gg = g * g;   a = beta2 * v;   b = one_minus_beta2 * gg;   v' = a + b
//   r = sqrtf(v');   d = r + eps;   q = g / d;   u = s_t * q;   p' = p - u
// sqrtf and / are the correctly rounded IEEE forms (hipcc's default for HIP; build.sh passes no fast-math flag: the
// code has v_sqrt_f32 with its fix-up and the v_div_scale / v_div_fmas / v_div_fixup sequence).  beta2, one_minus_beta2
// and the per-tensor step size s_t = lr sqrt(1 - beta2^step) coef arrive as the fp32 images of the host's doubles, which
// is what torch makes of the reference's Python scalars.  No clamps: a non-finite g gives a non-finite v' and p' in that
// element and nowhere else.
//
// The average p.lerp_(q, w), torch's formula (ATen/native/Lerp.h):
//   d = q - p;   |w| < 0.5:  p' = p + w * d;   otherwise:  p' = q - d * (1 - w)         (1 - w in fp32)
//
// A launch carries a fixed-size table BY VALUE in its kernel arguments: up to MT_T tensors (device addresses, element
// counts, step sizes) and a prefix sum of their chunk counts; a chunk is MT_C consecutive elements and belongs to one
// block, a launch has at most MT_K chunks.  Block b finds its tensor by binary search over the prefix sum: blockIdx.x
// is wave-uniform, so the table is read with scalar loads from the kernel-argument segment, and nothing lives in
// device memory: gradients are reallocated by every backward (zero_grad sets them to None), a device-resident table
// would cost a host-to-device copy per step.  The entry points split a longer list into as many launches as it needs; a
// tensor with more chunks than the launch has room for is continued in the next launch from an element offset that is
// a multiple of MT_C.  No atomics, no LDS, no workspace, no allocation, no copy, no synchronisation.
//
// 256 threads, four consecutive elements per thread per trip, MT_C / 1024 trips.  A tensor whose pointers are ALL
// 16-byte aligned (decided on the host, one bit per tensor) takes 16-byte loads and stores, any other the scalar
// instantiation of the same walk: thread t of trip k owns elements 1024 k + 4 t .. + 3 of the chunk in both, and the
// last n % 4 elements of a tensor are scalar in both.  An element's result depends on its own inputs only, so a tensor
// is bit-identical stepped alone, as one of many, from an odd element offset, or cut between two launches.
#include <cmath>

#include "common.h"
#include "chunk4.h"

// No contraction of a * b + c across this file (as in style.hip): hipcc's default fuses as the optimiser sees fit, and
// the reference's sequence of torch ops rounds after every operation.
#pragma clang fp contract(off)

#define MT_T 104    // tensors per launch
#define MT_K 4096   // chunks (blocks) per launch
#define MT_C 4096   // elements per chunk
#define MT_NT 256   // threads per block
#define MT_TRIPS (MT_C / (MT_NT * 4))

// one launch's worth of tensors; NP device addresses per tensor (step: p, g, v; average: p, q)
template <int NP>
struct MtTable {
  unsigned long long ptr[NP][MT_T];  // address of the tensor's first element IN THIS LAUNCH
  unsigned n[MT_T];                  // its elements in this launch (<= MT_K * MT_C)
  float s[MT_T];                     // step size (the average does not read it)
  int first[MT_T + 1];               // first[t]: the first block of tensor t; first[nt]: the grid
  unsigned al[(MT_T + 31) / 32];     // bit t: every pointer of tensor t is 16-byte aligned
  int nt;
};
// HIP's limit on the bytes of kernel arguments is 4096; the three scalars of the step travel next to the table
static_assert(sizeof(MtTable<3>) + 3 * sizeof(float) <= 4096, "the step's table must fit the kernel-argument limit");
static_assert(sizeof(MtTable<2>) + sizeof(float) <= 4096, "the average's table must fit the kernel-argument limit");
static_assert((unsigned long long)MT_K * MT_C < 0xFFFFFFFFull, "a launch's share of a tensor is a 32-bit count");
static_assert(MT_C % (MT_NT * 4) == 0 && (MT_C * sizeof(float)) % 16 == 0, "chunks are whole trips and keep alignment");

// the tensor of block b: first[t] <= b < first[t + 1]  (every tensor of a table has at least one chunk)
template <int NP>
__device__ __forceinline__ int mt_find(const MtTable<NP>& tab, int b) {
  int lo = 0, hi = tab.nt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// The table's addresses are integers: they are cast to the GLOBAL address space (chunk4.h).  Elements i .. i + 3 of a chunk
// with n elements left are chunk4.h's c4_load / c4_store in their !FULL form: one 16-byte access when AL and all four
// exist, else scalars (a tensor's alignment bit says nothing about its tail).
//
// reference: custom_adam.py:82-95
template <bool AL>
__device__ __forceinline__ void mt_adam_chunk(c4_gf32* __restrict__ p, c4_gcf32* __restrict__ g, c4_gf32* __restrict__ v,
                                              unsigned n, float s, float beta2, float omb, float eps) {
  float pv[MT_TRIPS][4], gv[MT_TRIPS][4], vv[MT_TRIPS][4];
#pragma unroll
  for (int k = 0; k < MT_TRIPS; ++k) {  // (every load of the chunk is issued before the first result is needed)
    const unsigned i = (k * MT_NT + threadIdx.x) * 4;
    if (i < n) {
      c4_load<AL, false>(g, i, n, gv[k]);
      c4_load<AL, false>(v, i, n, vv[k]);
      c4_load<AL, false>(p, i, n, pv[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < MT_TRIPS; ++k) {
    const unsigned i = (k * MT_NT + threadIdx.x) * 4;
    if (i < n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gi = gv[k][j];
        const float gg = gi * gi;
        const float a = beta2 * vv[k][j];
        const float b = omb * gg;
        const float vn = a + b;
        const float d = sqrtf(vn) + eps;
        const float q = gi / d;
        const float u = s * q;
        vv[k][j] = vn;
        pv[k][j] = pv[k][j] - u;
      }
      c4_store<AL, false>(v, i, n, vv[k]);
      c4_store<AL, false>(p, i, n, pv[k]);
    }
  }
}

__global__ void __launch_bounds__(MT_NT) mt_lreq_adam_kernel(MtTable<3> tab, float beta2, float omb, float eps) {
  const int b = blockIdx.x, t = mt_find(tab, b);
  const unsigned off = (unsigned)(b - tab.first[t]) * MT_C;  // (< MT_K * MT_C)
  const unsigned left = tab.n[t] - off, n = left < MT_C ? left : MT_C;
  c4_gf32* p = reinterpret_cast<c4_gf32*>(tab.ptr[0][t]) + off;
  c4_gcf32* g = reinterpret_cast<c4_gcf32*>(tab.ptr[1][t]) + off;
  c4_gf32* v = reinterpret_cast<c4_gf32*>(tab.ptr[2][t]) + off;
  const float s = tab.s[t];
  if ((tab.al[t >> 5] >> (t & 31)) & 1u)
    mt_adam_chunk<true>(p, g, v, n, s, beta2, omb, eps);
  else
    mt_adam_chunk<false>(p, g, v, n, s, beta2, omb, eps);
}

// reference: model.py:329 (torch's lerp_ with a scalar weight).  The formula is chunk4.h's c4_lerp with the branch on |w|
// taken once per block (`small`); calling c4_lerp per element gives the same values but another register allocation.
template <bool AL>
__device__ __forceinline__ void mt_lerp_chunk(c4_gf32* __restrict__ p, c4_gcf32* __restrict__ q, unsigned n, float w,
                                              float omw, bool small) {
  float pv[MT_TRIPS][4], qv[MT_TRIPS][4];
#pragma unroll
  for (int k = 0; k < MT_TRIPS; ++k) {
    const unsigned i = (k * MT_NT + threadIdx.x) * 4;
    if (i < n) {
      c4_load<AL, false>(q, i, n, qv[k]);
      c4_load<AL, false>(p, i, n, pv[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < MT_TRIPS; ++k) {
    const unsigned i = (k * MT_NT + threadIdx.x) * 4;
    if (i < n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = qv[k][j] - pv[k][j];
        const float m = small ? w * d : d * omw;
        pv[k][j] = small ? pv[k][j] + m : qv[k][j] - m;
      }
      c4_store<AL, false>(p, i, n, pv[k]);
    }
  }
}

__global__ void __launch_bounds__(MT_NT) mt_lerp_kernel(MtTable<2> tab, float w) {
  const int b = blockIdx.x, t = mt_find(tab, b);
  const unsigned off = (unsigned)(b - tab.first[t]) * MT_C;
  const unsigned left = tab.n[t] - off, n = left < MT_C ? left : MT_C;
  c4_gf32* p = reinterpret_cast<c4_gf32*>(tab.ptr[0][t]) + off;
  c4_gcf32* q = reinterpret_cast<c4_gcf32*>(tab.ptr[1][t]) + off;
  const bool small = fabsf(w) < 0.5f;
  const float omw = 1.f - w;
  if ((tab.al[t >> 5] >> (t & 31)) & 1u)
    mt_lerp_chunk<true>(p, q, n, w, omw, small);
  else
    mt_lerp_chunk<false>(p, q, n, w, omw, small);
}

// ---- host side: validation, then the list cut into tables --------------------------------------------------------------
// null arrays, then a null or misaligned device address of a non-empty tensor; nothing is launched before this passes
template <int NP>
static int mt_validate(const unsigned long long* const (&ptrs)[NP], const size_t* numel, int n_tensors) {
  if (n_tensors < 0) return SIVAE_ERR_SHAPE;
  if (!numel) return SIVAE_ERR_NULL;
  for (int a = 0; a < NP; ++a)
    if (!ptrs[a]) return SIVAE_ERR_NULL;
  for (int t = 0; t < n_tensors; ++t) {
    if (numel[t] == 0) continue;
    for (int a = 0; a < NP; ++a) {
      if (!ptrs[a][t]) return SIVAE_ERR_NULL;
      if (ptrs[a][t] & 3ull) return SIVAE_ERR_SHAPE;
    }
  }
  return SIVAE_OK;
}

// Cuts the list into launches: emit(tab, blocks) once per launch -> emit's first non-zero status; *launches counts them.
// `ptrs` / `steps` may be null (counting only: the addresses and step sizes are then left out of the table).
template <int NP, typename Emit>
static int mt_split(const unsigned long long* const* ptrs, const size_t* numel, const float* steps, int n_tensors,
                    int* launches, Emit&& emit) {
  MtTable<NP> tab = {};
  int nt = 0, blocks = 0;
  *launches = 0;
  auto flush = [&]() -> int {
    if (nt == 0) return SIVAE_OK;
    tab.first[nt] = blocks;
    tab.nt = nt;
    const int rc = emit(tab, blocks);
    ++*launches;
    tab = MtTable<NP>{};
    nt = blocks = 0;
    return rc;
  };
  for (int t = 0; t < n_tensors; ++t) {
    const size_t n = numel[t];
    bool al = ptrs != nullptr;
    if (ptrs)
      for (int a = 0; a < NP; ++a) al = al && (ptrs[a][t] & 15ull) == 0;
    for (size_t off = 0; off < n;) {  // (off stays a multiple of MT_C: the alignment of the tensor is that of every part)
      const size_t rem = n - off, chunks = (rem + MT_C - 1) / MT_C, room = (size_t)(MT_K - blocks);
      const size_t take = chunks < room ? chunks : room, elems = rem < take * MT_C ? rem : take * MT_C;
      if (ptrs)
        for (int a = 0; a < NP; ++a) tab.ptr[a][nt] = ptrs[a][t] + off * sizeof(float);
      tab.n[nt] = (unsigned)elems;
      tab.s[nt] = steps ? steps[t] : 0.f;
      tab.first[nt] = blocks;
      if (al) tab.al[nt >> 5] |= 1u << (nt & 31);
      ++nt;
      blocks += (int)take;
      off += elems;
      if (nt == MT_T || blocks == MT_K) {
        const int rc = flush();
        if (rc != SIVAE_OK) return rc;
      }
    }
  }
  return flush();
}

extern "C" int sivae_mt_max_tensors(void) { return MT_T; }
extern "C" int sivae_mt_max_chunks(void) { return MT_K; }
extern "C" int sivae_mt_chunk_elems(void) { return MT_C; }
extern "C" int sivae_mt_table_bytes(void) { return (int)(sizeof(MtTable<3>) + 3 * sizeof(float)); }

extern "C" int sivae_mt_launches(const void* numel, int n_tensors) {
  if (n_tensors < 0) return SIVAE_ERR_SHAPE;
  if (!numel) return SIVAE_ERR_NULL;
  int launches = 0;
  mt_split<2>(nullptr, static_cast<const size_t*>(numel), nullptr, n_tensors, &launches,
              [](const MtTable<2>&, int) { return SIVAE_OK; });
  return launches;
}

extern "C" int sivae_mt_lreq_adam(const void* params, const void* grads, const void* exp_avg_sq, const void* numel,
                                  const void* step_sizes, int n_tensors, float beta2, float one_minus_beta2, float eps,
                                  hipStream_t stream) {
  const unsigned long long* const ptrs[3] = {static_cast<const unsigned long long*>(params),
                                             static_cast<const unsigned long long*>(grads),
                                             static_cast<const unsigned long long*>(exp_avg_sq)};
  const size_t* n = static_cast<const size_t*>(numel);
  const int bad = mt_validate<3>(ptrs, n, n_tensors);
  if (bad != SIVAE_OK) return bad;
  if (!step_sizes) return SIVAE_ERR_NULL;
  if (!(beta2 >= 0.f && beta2 < 1.f) || !std::isfinite(one_minus_beta2) || !(eps >= 0.f) || !std::isfinite(eps))
    return SIVAE_ERR_RANGE;
  int launches = 0;
  return mt_split<3>(ptrs, n, static_cast<const float*>(step_sizes), n_tensors, &launches,
                     [&](const MtTable<3>& tab, int blocks) {
                       hipLaunchKernelGGL(mt_lreq_adam_kernel, dim3((unsigned)blocks), dim3(MT_NT), 0, stream, tab, beta2,
                                          one_minus_beta2, eps);
                       return sivae_launch_status();
                     });
}

extern "C" int sivae_mt_lerp(const void* dst, const void* src, const void* numel, int n_tensors, float weight,
                             hipStream_t stream) {
  const unsigned long long* const ptrs[2] = {static_cast<const unsigned long long*>(dst),
                                             static_cast<const unsigned long long*>(src)};
  const size_t* n = static_cast<const size_t*>(numel);
  const int bad = mt_validate<2>(ptrs, n, n_tensors);
  if (bad != SIVAE_OK) return bad;
  if (!std::isfinite(weight)) return SIVAE_ERR_RANGE;
  int launches = 0;
  return mt_split<2>(ptrs, n, nullptr, n_tensors, &launches, [&](const MtTable<2>& tab, int blocks) {
    hipLaunchKernelGGL(mt_lerp_kernel, dim3((unsigned)blocks), dim3(MT_NT), 0, stream, tab, weight);
    return sivae_launch_status();
  });
}
