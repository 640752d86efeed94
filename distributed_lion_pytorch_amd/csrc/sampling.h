// The counter-based noise shared by the sampling kernels (lm_sample.hip, spec_verify.hip): one 24-bit draw per
// (key, row, column), n = mix32(mix32(column ^ key) + rowterm) >> 8, rowterm = row * 0x9E3779B1 + 0x85EBCA6B.
#pragma once

#include "common.h"

namespace dlion {

__device__ __forceinline__ uint32_t samp_rowterm(uint32_t row) { return row * 0x9E3779B1u + 0x85EBCA6Bu; }

__device__ __forceinline__ uint32_t samp_draw24(uint32_t col, uint32_t key, uint32_t rowterm) {
  return mix32(mix32(col ^ key) + rowterm) >> 8;
}

// g = -log(-log(u)), u = (n + 0.5) 2^-24 with n the hash's top 24 bits.  n + 0.5 has 25 significant bits from
// n = 2^23 on, so the upper half goes through 1 - u = (2^24 - n - 0.5) 2^-24, which is exact there, and log1p.
__device__ __forceinline__ float samp_gumbel(uint32_t col, uint32_t key, uint32_t rowterm) {
  const uint32_t n = samp_draw24(col, key, rowterm);
  float e;
  if (n < (1u << 23))
    e = -logf((static_cast<float>(n) + 0.5f) * 0x1p-24f);
  else
    e = -log1pf(-((static_cast<float>((1u << 24) - n) - 0.5f) * 0x1p-24f));
  return -logf(e);
}

// The column slot no column can occupy (vp <= 2^30): the row's uniform for an accept test, exact in fp64.
constexpr uint32_t kSampUniformSlot = 0xFFFFFFFFu;
__device__ __forceinline__ double samp_uniform(uint32_t key, uint32_t rowterm) {
  return (static_cast<double>(samp_draw24(kSampUniformSlot, key, rowterm)) + 0.5) * 0x1p-24;
}

}  // namespace dlion
