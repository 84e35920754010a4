// The 4-element chunk of style.hip, rgb.hip, mapping.hip and multi_tensor.hip: "one partition, two instantiations".
// A thread owns 4 consecutive floats i .. i + 3 of a run of n (a plane, a row, a tensor's share of a launch).  It reads and
// writes them with ONE 16-byte access where the host found the call aligned (AL), and with guarded scalar accesses over the
// SAME 4 elements anywhere else (an element at or past n reads as 0 and is not written).  The two instantiations of a kernel
// differ in nothing but the width of the access, so the alignment changes no bit: every family's tests ask torch.equal
// across alignments.  This header is the one place that holds the access, the host's alignment pick and torch's lerp.
#pragma once
#include <initializer_list>

#include "common.h"

// A plain float* made from an integer address (multi_tensor.hip's table) or read out of a by-value argument struct is a
// generic pointer and every access through it a flat_ one: cast to the GLOBAL address space they become global_load /
// global_store.
typedef __attribute__((address_space(1))) float c4_gf32;
typedef __attribute__((address_space(1))) const float c4_gcf32;
typedef __attribute__((address_space(1))) f32x4 c4_gf32x4;
typedef __attribute__((address_space(1))) const f32x4 c4_gcf32x4;

// The 16-byte copy, one vector type per pointer kind: HIP's float4 through a plain pointer, f32x4 through an
// address-space-1 one.  Keep the two apart: f32x4 through the plain pointers as well means the same, but the compiler then
// forms the addresses in front of the loads of style.hip and rgb.hip differently and some of their kernels change their
// register counts (profiles/chunk4_fold.txt), which would have to be timed.
__device__ __forceinline__ void c4_get(const float* p, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void c4_get(c4_gcf32* p, float (&v)[4]) {
  const f32x4 q = *reinterpret_cast<c4_gcf32x4*>(p);
  v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
}
__device__ __forceinline__ void c4_put(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void c4_put(c4_gf32* p, const float (&v)[4]) {
  f32x4 q;
  q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
  *reinterpret_cast<c4_gf32x4*>(p) = q;
}

// The chunk at i of a run of n.  FULL: AL alone promises that all four elements exist (the host pick c4_al16 includes
// n % 4 == 0, and i < n).  !FULL: the 16-byte access also needs i + 4 <= n (multi_tensor.hip: a tensor's alignment bit
// says nothing about its tail, whose last n % 4 elements are scalar in both instantiations).  T: float or c4_gf32, const
// or not; I: int or unsigned.
template <bool AL, bool FULL = true, typename T, typename I>
__device__ __forceinline__ void c4_load(T* __restrict__ p, I i, I n, float (&v)[4]) {
  if (AL && (FULL || i + 4 <= n)) {
    c4_get(p + i, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.f;
  }
}
template <bool AL, bool FULL = true, typename T, typename I>
__device__ __forceinline__ void c4_store(T* __restrict__ p, I i, I n, const float (&v)[4]) {
  if (AL && (FULL || i + 4 <= n)) {
    c4_put(p + i, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

// The host's pick (null pointers are skipped).  c4_al4: what every entry point demands of its fp32 pointers.  c4_al16: the
// call takes the 16-byte instantiation: runs of a multiple of 4 elements, so that every run of an aligned tensor is aligned
// and has no tail, and every pointer that is accessed in chunks 16-byte aligned.
static inline bool c4_al4(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && sivae_misaligned(p, 4)) return false;
  return true;
}
static inline bool c4_al16(int n, std::initializer_list<const void*> ptrs) {
  if (n % 4) return false;
  for (const void* p : ptrs)
    if (p && sivae_misaligned(p, 16)) return false;
  return true;
}

// torch's lerp with a scalar weight (ATen/native/Lerp.h); omw is 1 - w formed in fp32.  No contraction, wherever this
// header is included: each product is rounded before it is added, as torch's two kernels round it.
__device__ __forceinline__ float c4_lerp(float a, float b, float w, float omw) {
#pragma clang fp contract(off)
  const float d = b - a;
  return fabsf(w) < 0.5f ? a + w * d : b - d * omw;
}
