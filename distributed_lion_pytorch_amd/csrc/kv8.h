// The fp8 (OCP e4m3fn) KV cache's quantiser and its inverse, shared by the three kernels that write a cached key
// (kv8_attention.hip kv_quantize, decode.hip kv_append, chunk_attention.hip kv_append_chunk) and by the
// attention kernel that reads it: a token's cached key is the same bits whichever kernel wrote it, so there is
// one copy of the arithmetic.
//
// A head row x of D bf16 values becomes D codes and one fp32 scale 2^e, e = ((bits(max|x|) + 0x00200000) >> 23)
// - 135 clamped into [-126, 126]: adding a quarter to the mantissa carries into the exponent from 1.75 on, so
// max|x| / scale lies in [224, 448) (448 is e4m3's largest finite value) wherever e is not clamped, i.e. for
// max|x| >= 2^-118.  code = e4m3_rne(x 2^-e); the product is exact (a power of two; where it leaves fp32's
// normal range the code is a zero either way).  Dequantisation, code 2^e, is exact in fp32 and, the scale
// aside, in bf16.
#pragma once

#include "common.h"
#include "rope_norm.h"

namespace dlion {

// maximum over the LANES (8 or 16) lanes of a head row, the same value in all of them
template <int LANES>
__device__ __forceinline__ float head_max(float v) {
  v = fmaxf(v, dpp_mov<kQuadXor1>(v));
  v = fmaxf(v, dpp_mov<kQuadXor2>(v));
  v = fmaxf(v, dpp_mov<kHalfMirror>(v));
  if (LANES == 16) v = fmaxf(v, dpp_mov<kRowMirror>(v));
  return v;
}

// This lane's 8 values of a head row held by LANES adjacent lanes (all of them active) -> their 8 codes, x[0..3]
// in .x and x[4..7] in .y, lowest byte first; scale is the row's, the same in every lane.
template <int LANES>
__device__ __forceinline__ uint2 kv8_quantize_row(const float (&x)[8], float& scale) {
  float a = fabsf(x[0]);
#pragma unroll
  for (int i = 1; i < 8; ++i) a = fmaxf(a, fabsf(x[i]));
  a = head_max<LANES>(a);
  int e = static_cast<int>((__float_as_uint(a) + 0x00200000u) >> 23) - 135;
  e = e < -126 ? -126 : (e > 126 ? 126 : e);
  scale = __uint_as_float(static_cast<uint32_t>(e + 127) << 23);
  // x 2^-e by v_ldexp_f32: exact, and no fp32 multiply for the compiler to pair into a packed one
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = __builtin_ldexpf(x[i], -e);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return make_uint2(static_cast<uint32_t>(lo), static_cast<uint32_t>(hi));
}

// four codes -> four bf16 (exact: e4m3 has 3 mantissa bits and a range inside bf16's), packed in order
__device__ __forceinline__ uint2 kv8_codes_to_bf16(uint32_t w) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), false);
  const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), true);
  uint2 r;
  r.x = (__float_as_uint(a[1]) & 0xffff0000u) | (__float_as_uint(a[0]) >> 16);
  r.y = (__float_as_uint(b[1]) & 0xffff0000u) | (__float_as_uint(b[0]) >> 16);
  return r;
}

}  // namespace dlion
