// The arithmetic of the rotary embedding and of the per-head q/k RMSNorm, shared by the training kernels
// (elementwise_kernels.hip rope_kernel, qk_norm.hip) and the decode-step kernel (decode.hip kv_append):
// a cached key must be the same bits as the key the full forward computes, so there is one copy of each.
#pragma once

#include "common.h"

namespace dlion {

// ---------------------------------------------------------------- rotate-half RoPE
// a: a dim of the first half, b: its partner in the second half; ca / sa and cb / sb the table entries at
// the two dims.  rope_inverse is the transpose rotation.  The cos product is rounded and the sin product is
// fused into the sum: written out (it is what the compiler's contraction made of a ca - b sa in rope_kernel
// from the start), so that the bits do not depend on where these are inlined.
__device__ __forceinline__ void rope_forward(float a, float b, float ca, float cb, float sa, float sb, float& oa,
                                             float& ob) {
#pragma clang fp contract(off)
  oa = __builtin_fmaf(-b, sa, a * ca);
  ob = __builtin_fmaf(a, sb, b * cb);
}
__device__ __forceinline__ void rope_inverse(float a, float b, float ca, float cb, float sa, float sb, float& oa,
                                             float& ob) {
#pragma clang fp contract(off)
  oa = __builtin_fmaf(b, sb, a * ca);
  ob = __builtin_fmaf(-a, sa, b * cb);
}

// ---------------------------------------------------------------- head rows of D / 8 adjacent lanes
// A head row of D bf16 is LANES = D / 8 adjacent lanes with 8 dims each (qk_norm.hip's mapping).  Every
// function below is compiled without implicit FMA contraction, whatever the including file's setting: the
// result must not depend on where it is inlined.
constexpr int kQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]
constexpr int kQuadRev = 0x1B;      // quad_perm [3,2,1,0]
constexpr int kRowRor8 = 0x128;     // lane i <- lane (i + 8) % 16
constexpr int kHalfMirror = 0x141;  // lane i <- lane 7 - i of its 8
constexpr int kRowMirror = 0x140;   // lane i <- lane 15 - i of its 16

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// sum over the LANES lanes of a head row, bit-identical in all of them
template <int LANES>
__device__ __forceinline__ float head_sum(float v) {
#pragma clang fp contract(off)
  v += dpp_mov<kQuadXor1>(v);
  v += dpp_mov<kQuadXor2>(v);
  v += dpp_mov<kHalfMirror>(v);
  if (LANES == 16) v += dpp_mov<kRowMirror>(v);
  return v;
}

// the value of lane ^ (LANES / 2): the lane that holds the rotate-half partners
template <int LANES>
__device__ __forceinline__ float partner(float v) {
  if (LANES == 16) return dpp_mov<kRowRor8>(v);
  return dpp_mov<kQuadRev>(dpp_mov<kHalfMirror>(v));
}

__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
#pragma clang fp contract(off)
  return ((a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3])) +
         ((a[4] * b[4] + a[5] * b[5]) + (a[6] * b[6] + a[7] * b[7]));
}

// v_rsq_f32 is good to 1 ulp; one Newton step leaves about half of one
__device__ __forceinline__ float rsqrt_nr(float v) {
#pragma clang fp contract(off)
  const float r = __builtin_amdgcn_rsqf(v);
  const float e = __builtin_fmaf(-(v * r), r, 1.f);
  return __builtin_fmaf(0.5f * r, e, r);
}

// o = rope(v rsqrt(mean(v^2) + eps) w) for this lane's 8 dims of a head row (c / s: the tables at those dims;
// first: the lane holds dims of the first half); returns the row's rstd.  All LANES lanes must be active.
template <int LANES>
__device__ __forceinline__ float qk_norm_rope_row(const float (&v)[8], const float (&w)[8], const float (&c)[8],
                                                  const float (&s)[8], float eps, bool first, float (&o)[8]) {
#pragma clang fp contract(off)
  const float r = rsqrt_nr(head_sum<LANES>(dot8(v, v)) * (1.f / (LANES * 8)) + eps);
  float yv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) yv[j] = (v[j] * r) * w[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float p = partner<LANES>(yv[j]);
    o[j] = yv[j] * c[j] + (first ? -p : p) * s[j];
  }
  return r;
}

}  // namespace dlion
