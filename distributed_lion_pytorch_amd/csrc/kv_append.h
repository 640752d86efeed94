// The cache-append kernels of the decode step (kv_append) and of a chunk of tokens (kv_append_chunk), and their
// launchers: decode.hip and chunk_attention.hip instantiate the bf16 stores, kv8_attention.hip the fp8 stores (kv8.h)
// of the same templates, so that the positions, the error flag, the clamped lanes and the q they return are one copy
// of the code whatever the cache holds.
#pragma once

#include "common.h"
#include "kernels.h"
#include "kv8.h"
#include "rope_norm.h"

namespace dlion {
namespace {

using E = Elem<kBF16>;

__device__ __forceinline__ void unpack8(const uint4& r, float (&o)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = bf16_to_f32(static_cast<uint16_t>(w[i] & 0xffffu));
    o[2 * i + 1] = bf16_to_f32(static_cast<uint16_t>(w[i] >> 16));
  }
}
__device__ __forceinline__ void unpack4(const uint2& r, float (&o)[4]) {
  o[0] = bf16_to_f32(static_cast<uint16_t>(r.x & 0xffffu));
  o[1] = bf16_to_f32(static_cast<uint16_t>(r.x >> 16));
  o[2] = bf16_to_f32(static_cast<uint16_t>(r.y & 0xffffu));
  o[3] = bf16_to_f32(static_cast<uint16_t>(r.y >> 16));
}
__device__ __forceinline__ uint2 pack4(const float (&o)[4]) {
  uint2 v;
  v.x = static_cast<uint32_t>(f32_to_bf16(o[0])) | (static_cast<uint32_t>(f32_to_bf16(o[1])) << 16);
  v.y = static_cast<uint32_t>(f32_to_bf16(o[2])) | (static_cast<uint32_t>(f32_to_bf16(o[3])) << 16);
  return v;
}

enum : int { kAppend = 0, kRope = 1, kNormRope = 2 };

// grid: ceil(B (H + 2 Hkv) / GROUPS) blocks of 256; a lane group of D / 8 lanes owns one head row of one
// sequence: slots [0, H) are q, [H, H + Hkv) k, the rest v
// FP8 (the fp8 cache, kv8.h): kc / vc are the code buffers (byte strides), ksc / vsc the scales [B, Tmax, Hkv]
// (strides sc_bs / sc_ts); k and v are rounded to bf16 as the bf16 cache stores them, then quantised
template <int D, int MODE, bool FP8>
__global__ void __launch_bounds__(256) kv_append_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t q_ld,
    int64_t k_ld, int64_t v_ld, const int* __restrict__ pos, const uint16_t* __restrict__ cs,
    const uint16_t* __restrict__ sn, const uint16_t* __restrict__ gq, const uint16_t* __restrict__ gk, float eps,
    uint16_t* __restrict__ q_out, void* __restrict__ kc_, void* __restrict__ vc_, int64_t kc_bs, int64_t kc_ts,
    int64_t vc_bs, int64_t vc_ts, float* __restrict__ ksc, float* __restrict__ vsc, int64_t sc_bs, int64_t sc_ts, int B,
    int H, int Hkv, int Tmax, int32_t* __restrict__ err) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
  uint16_t* const kc = static_cast<uint16_t*>(kc_);
  uint16_t* const vc = static_cast<uint16_t*>(vc_);
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int Hx = H + 2 * Hkv;
  const int64_t n_hr = static_cast<int64_t>(B) * Hx;
  const int64_t hr = static_cast<int64_t>(blockIdx.x) * GROUPS + grp;
  const bool valid = hr < n_hr;
  const int64_t hrc = valid ? hr : n_hr - 1;
  const int b = static_cast<int>(hrc / Hx);
  const int slot = static_cast<int>(hrc - static_cast<int64_t>(b) * Hx);
  int p = pos[b];
  if (p < 0 || p >= Tmax) {  // an error (flag checked once per step, ops/fused.py), never a write outside the cache
    if (valid && sub == 0 && slot == 0) atomicOr(err, kIndexErrCache);
    p = p < 0 ? 0 : Tmax - 1;
  }
  const bool is_q = slot < H, is_v = slot >= H + Hkv;
  const uint16_t* src = is_q    ? q + b * q_ld + static_cast<int64_t>(slot) * D
                        : is_v  ? v + b * v_ld + static_cast<int64_t>(slot - H - Hkv) * D
                                : k + b * k_ld + static_cast<int64_t>(slot - H) * D;
  uint16_t* dst = is_q   ? q_out + (static_cast<int64_t>(b) * H + slot) * D
                  : is_v ? vc + b * vc_bs + p * vc_ts + static_cast<int64_t>(slot - H - Hkv) * D
                         : kc + b * kc_bs + p * kc_ts + static_cast<int64_t>(slot - H) * D;
  // the fp8 cache's row of this k / v slot (unused for q)
  uint8_t* dst8 = nullptr;
  float* dsts = nullptr;
  if constexpr (FP8) {
    const int hkv = is_q ? 0 : (is_v ? slot - H - Hkv : slot - H);
    dst8 = static_cast<uint8_t*>(is_v ? vc_ : kc_) + b * (is_v ? vc_bs : kc_bs) + p * (is_v ? vc_ts : kc_ts) +
           static_cast<int64_t>(hkv) * D;
    dsts = (is_v ? vsc : ksc) + b * sc_bs + p * sc_ts + hkv;
  }
  if constexpr (MODE == kRope) {
    // rope_kernel's mapping: 4 dims of the first half and their partners in the second
    constexpr int hd = D / 2;
    const int d0 = sub * 4;
    const uint2 ra = *reinterpret_cast<const uint2*>(src + d0);
    const uint2 rb = *reinterpret_cast<const uint2*>(src + hd + d0);
    const int64_t tb = static_cast<int64_t>(p) * D + d0;
    float a[4], bb[4], ca[4], cb[4], sa[4], sb[4], oa[4], ob[4];
    unpack4(ra, a);
    unpack4(rb, bb);
    unpack4(*reinterpret_cast<const uint2*>(cs + tb), ca);
    unpack4(*reinterpret_cast<const uint2*>(cs + tb + hd), cb);
    unpack4(*reinterpret_cast<const uint2*>(sn + tb), sa);
    unpack4(*reinterpret_cast<const uint2*>(sn + tb + hd), sb);
#pragma unroll
    for (int j = 0; j < 4; ++j) rope_forward(a[j], bb[j], ca[j], cb[j], sa[j], sb[j], oa[j], ob[j]);
    if constexpr (FP8) {
      const uint2 wa = is_v ? ra : pack4(oa), wb = is_v ? rb : pack4(ob);
      float x[8], scale;
      unpack4(wa, a);
      unpack4(wb, bb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[j] = a[j];
        x[4 + j] = bb[j];
      }
      const uint2 c8 = kv8_quantize_row<LANES>(x, scale);
      if (valid && is_q) {
        *reinterpret_cast<uint2*>(dst + d0) = wa;
        *reinterpret_cast<uint2*>(dst + hd + d0) = wb;
      } else if (valid) {
        *reinterpret_cast<uint32_t*>(dst8 + d0) = c8.x;
        *reinterpret_cast<uint32_t*>(dst8 + hd + d0) = c8.y;
        if (sub == 0) *dsts = scale;
      }
    } else if (valid) {
      *reinterpret_cast<uint2*>(dst + d0) = is_v ? ra : pack4(oa);
      *reinterpret_cast<uint2*>(dst + hd + d0) = is_v ? rb : pack4(ob);
    }
  } else {
    const int d0 = sub * 8;
    const uint4 raw = *reinterpret_cast<const uint4*>(src + d0);
    if constexpr (MODE == kAppend) {
      if constexpr (FP8) {
        float x[8], scale;
        unpack8(raw, x);
        const uint2 c8 = kv8_quantize_row<LANES>(x, scale);
        if (valid && is_q) {
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        } else if (valid) {
          *reinterpret_cast<uint2*>(dst8 + d0) = c8;
          if (sub == 0) *dsts = scale;
        }
      } else if (valid) {
        *reinterpret_cast<uint4*>(dst + d0) = raw;
      }
    } else {
      // qk_norm.hip's mapping; v rows run the same lanes (their result is dropped) so that no DPP move
      // reads an inactive lane
      float x[8], w[8], c[8], s[8], o[8];
      unpack8(raw, x);
      E::load8((is_q ? gq : gk) + d0, w);
      E::load8(cs + static_cast<int64_t>(p) * D + d0, c);
      E::load8(sn + static_cast<int64_t>(p) * D + d0, s);
      qk_norm_rope_row<LANES>(x, w, c, s, eps, sub < LANES / 2, o);
      if constexpr (FP8) {
        float y[8], scale;
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = is_v ? x[j] : bf16_to_f32(f32_to_bf16(o[j]));
        const uint2 c8 = kv8_quantize_row<LANES>(y, scale);
        if (valid && is_q) {
          E::store8(dst + d0, o);
        } else if (valid) {
          *reinterpret_cast<uint2*>(dst8 + d0) = c8;
          if (sub == 0) *dsts = scale;
        }
      } else if (valid) {
        if (is_v)
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        else
          E::store8(dst + d0, o);
      }
    }
  }
}

// grid: ceil(B T (H + 2 Hkv) / GROUPS) blocks of 256; a lane group of D / 8 lanes owns one head row of one
// token: slots [0, H) are q, [H, H + Hkv) k, the rest v (kv_append_kernel's mapping with a token index)
// FP8 (the fp8 cache, kv8.h): kc / vc are the code buffers (byte strides), ksc / vsc the scales [B, Tmax, Hkv]
// (strides sc_bs / sc_ts); k and v are rounded to bf16 as the bf16 cache stores them, then quantised
template <int D, int MODE, bool FP8>
__global__ void __launch_bounds__(256) kv_append_chunk_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t q_bs,
    int64_t q_ts, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* __restrict__ pos,
    const int* __restrict__ n_new, const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn,
    const uint16_t* __restrict__ gq, const uint16_t* __restrict__ gk, float eps, uint16_t* __restrict__ q_out,
    void* __restrict__ kc_, void* __restrict__ vc_, int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts,
    float* __restrict__ ksc, float* __restrict__ vsc, int64_t sc_bs, int64_t sc_ts, int B, int T, int H, int Hkv,
    int Tmax, int32_t* __restrict__ err) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
  uint16_t* const kc = static_cast<uint16_t*>(kc_);
  uint16_t* const vc = static_cast<uint16_t*>(vc_);
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int Hx = H + 2 * Hkv;
  const int64_t n_hr = static_cast<int64_t>(B) * T * Hx;
  const int64_t hr = static_cast<int64_t>(blockIdx.x) * GROUPS + grp;
  const bool valid = hr < n_hr;
  const int64_t hrc = valid ? hr : n_hr - 1;
  const int bt = static_cast<int>(hrc / Hx);
  const int slot = static_cast<int>(hrc - static_cast<int64_t>(bt) * Hx);
  const int b = bt / T, t = bt - b * T;
  int n = n_new != nullptr ? n_new[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const bool live = t < n;  // the token is appended
  const int64_t p64 = static_cast<int64_t>(pos[b]) + t;
  const bool in_range = p64 >= 0 && p64 < Tmax;
  if (live && !in_range && valid && sub == 0 && slot == 0) atomicOr(err, kIndexErrCache);
  const int p = p64 < 0 ? 0 : (p64 >= Tmax ? Tmax - 1 : static_cast<int>(p64));  // the table row
  const bool is_q = slot < H, is_v = slot >= H + Hkv;
  const bool store = valid && (is_q || (live && in_range));
  const uint16_t* src = is_q    ? q + b * q_bs + t * q_ts + static_cast<int64_t>(slot) * D
                        : is_v  ? v + b * v_bs + t * v_ts + static_cast<int64_t>(slot - H - Hkv) * D
                                : k + b * k_bs + t * k_ts + static_cast<int64_t>(slot - H) * D;
  uint16_t* dst = is_q   ? q_out + (static_cast<int64_t>(bt) * H + slot) * D
                  : is_v ? vc + b * vc_bs + p * vc_ts + static_cast<int64_t>(slot - H - Hkv) * D
                         : kc + b * kc_bs + p * kc_ts + static_cast<int64_t>(slot - H) * D;
  // the fp8 cache's row of this k / v slot (unused for q)
  uint8_t* dst8 = nullptr;
  float* dsts = nullptr;
  if constexpr (FP8) {
    const int hkv = is_q ? 0 : (is_v ? slot - H - Hkv : slot - H);
    dst8 = static_cast<uint8_t*>(is_v ? vc_ : kc_) + b * (is_v ? vc_bs : kc_bs) + p * (is_v ? vc_ts : kc_ts) +
           static_cast<int64_t>(hkv) * D;
    dsts = (is_v ? vsc : ksc) + b * sc_bs + p * sc_ts + hkv;
  }
  if constexpr (MODE == kRope) {
    constexpr int hd = D / 2;
    const int d0 = sub * 4;
    const uint2 ra = *reinterpret_cast<const uint2*>(src + d0);
    const uint2 rb = *reinterpret_cast<const uint2*>(src + hd + d0);
    const int64_t tb = static_cast<int64_t>(p) * D + d0;
    float a[4], bb[4], ca[4], cb[4], sa[4], sb[4], oa[4], ob[4];
    unpack4(ra, a);
    unpack4(rb, bb);
    unpack4(*reinterpret_cast<const uint2*>(cs + tb), ca);
    unpack4(*reinterpret_cast<const uint2*>(cs + tb + hd), cb);
    unpack4(*reinterpret_cast<const uint2*>(sn + tb), sa);
    unpack4(*reinterpret_cast<const uint2*>(sn + tb + hd), sb);
#pragma unroll
    for (int j = 0; j < 4; ++j) rope_forward(a[j], bb[j], ca[j], cb[j], sa[j], sb[j], oa[j], ob[j]);
    if constexpr (FP8) {
      const uint2 wa = is_v ? ra : pack4(oa), wb = is_v ? rb : pack4(ob);
      float x[8], scale;
      unpack4(wa, a);
      unpack4(wb, bb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[j] = a[j];
        x[4 + j] = bb[j];
      }
      const uint2 c8 = kv8_quantize_row<LANES>(x, scale);
      if (store && is_q) {
        *reinterpret_cast<uint2*>(dst + d0) = wa;
        *reinterpret_cast<uint2*>(dst + hd + d0) = wb;
      } else if (store) {
        *reinterpret_cast<uint32_t*>(dst8 + d0) = c8.x;
        *reinterpret_cast<uint32_t*>(dst8 + hd + d0) = c8.y;
        if (sub == 0) *dsts = scale;
      }
    } else if (store) {
      *reinterpret_cast<uint2*>(dst + d0) = is_v ? ra : pack4(oa);
      *reinterpret_cast<uint2*>(dst + hd + d0) = is_v ? rb : pack4(ob);
    }
  } else {
    const int d0 = sub * 8;
    const uint4 raw = *reinterpret_cast<const uint4*>(src + d0);
    if constexpr (MODE == kAppend) {
      if constexpr (FP8) {
        float x[8], scale;
        unpack8(raw, x);
        const uint2 c8 = kv8_quantize_row<LANES>(x, scale);
        if (store && is_q) {
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        } else if (store) {
          *reinterpret_cast<uint2*>(dst8 + d0) = c8;
          if (sub == 0) *dsts = scale;
        }
      } else if (store) {
        *reinterpret_cast<uint4*>(dst + d0) = raw;
      }
    } else {
      // v rows run the same lanes (their result is dropped) so that no DPP move reads an inactive lane
      float x[8], w[8], c[8], s[8], o[8];
      unpack8(raw, x);
      E::load8((is_q ? gq : gk) + d0, w);
      E::load8(cs + static_cast<int64_t>(p) * D + d0, c);
      E::load8(sn + static_cast<int64_t>(p) * D + d0, s);
      qk_norm_rope_row<LANES>(x, w, c, s, eps, sub < LANES / 2, o);
      if constexpr (FP8) {
        float y[8], scale;
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = is_v ? x[j] : bf16_to_f32(f32_to_bf16(o[j]));
        const uint2 c8 = kv8_quantize_row<LANES>(y, scale);
        if (store && is_q) {
          E::store8(dst + d0, o);
        } else if (store) {
          *reinterpret_cast<uint2*>(dst8 + d0) = c8;
          if (sub == 0) *dsts = scale;
        }
      } else if (store) {
        if (is_v)
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        else
          E::store8(dst + d0, o);
      }
    }
  }
}

template <bool FP8>
hipError_t kv_append_any(const void* q, const void* k, const void* v, int64_t q_ld, int64_t k_ld, int64_t v_ld,
                         const int* pos, const void* cos, const void* sin, const void* q_gamma, const void* k_gamma,
                         float eps, void* q_out, void* k_cache, void* v_cache, int64_t kc_bs, int64_t kc_ts,
                         int64_t vc_bs, int64_t vc_ts, float* k_scales, float* v_scales, int64_t sc_bs, int64_t sc_ts,
                         int B, int H, int Hkv, int D, int Tmax, int32_t* err, hipStream_t st) {
  if (B <= 0 || H <= 0 || Hkv <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Tmax <= 0 || err == nullptr) return hipErrorInvalidValue;
  if ((cos == nullptr) != (sin == nullptr) || (q_gamma == nullptr) != (k_gamma == nullptr)) return hipErrorInvalidValue;
  if (q_gamma != nullptr && cos == nullptr) return hipErrorInvalidValue;
  const int groups = 256 / (D / 8);
  const int64_t n_hr = static_cast<int64_t>(B) * (H + 2 * Hkv);
  const dim3 grid(static_cast<unsigned>((n_hr + groups - 1) / groups));
  auto* Q = static_cast<const uint16_t*>(q);
  auto* K = static_cast<const uint16_t*>(k);
  auto* V = static_cast<const uint16_t*>(v);
  auto* C = static_cast<const uint16_t*>(cos);
  auto* S = static_cast<const uint16_t*>(sin);
  auto* GQ = static_cast<const uint16_t*>(q_gamma);
  auto* GK = static_cast<const uint16_t*>(k_gamma);
  auto* QO = static_cast<uint16_t*>(q_out);
#define DLION_KV_APPEND(DD, MODE)                                                                                     \
  hipLaunchKernelGGL((kv_append_kernel<DD, MODE, FP8>), grid, dim3(256), 0, st, Q, K, V, q_ld, k_ld, v_ld, pos, C, S, \
                     GQ, GK, eps, QO, k_cache, v_cache, kc_bs, kc_ts, vc_bs, vc_ts, k_scales, v_scales, sc_bs, sc_ts, \
                     B, H, Hkv, Tmax, err)
  const int mode = q_gamma != nullptr ? kNormRope : (cos != nullptr ? kRope : kAppend);
  if (D == 128) {
    if (mode == kNormRope) DLION_KV_APPEND(128, kNormRope);
    else if (mode == kRope) DLION_KV_APPEND(128, kRope);
    else DLION_KV_APPEND(128, kAppend);
  } else {
    if (mode == kNormRope) DLION_KV_APPEND(64, kNormRope);
    else if (mode == kRope) DLION_KV_APPEND(64, kRope);
    else DLION_KV_APPEND(64, kAppend);
  }
#undef DLION_KV_APPEND
  return hipGetLastError();
}


template <bool FP8>
hipError_t kv_append_chunk_any(const void* q, const void* k, const void* v, int64_t q_bs, int64_t q_ts, int64_t k_bs,
                               int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* pos, const int* n_new,
                               const void* cos, const void* sin, const void* q_gamma, const void* k_gamma, float eps,
                               void* q_out, void* k_cache, void* v_cache, int64_t kc_bs, int64_t kc_ts, int64_t vc_bs,
                               int64_t vc_ts, float* k_scales, float* v_scales, int64_t sc_bs, int64_t sc_ts, int B,
                               int T, int H, int Hkv, int D, int Tmax, int32_t* err, hipStream_t st) {
  if (B <= 0 || T <= 0 || H <= 0 || Hkv <= 0) return hipSuccess;
  // any T whose grid fits, on either cache (the extend kernels' forward)
  if ((D != 64 && D != 128) || Tmax <= 0 || err == nullptr) return hipErrorInvalidValue;
  if ((cos == nullptr) != (sin == nullptr) || (q_gamma == nullptr) != (k_gamma == nullptr)) return hipErrorInvalidValue;
  if (q_gamma != nullptr && cos == nullptr) return hipErrorInvalidValue;
  const int groups = 256 / (D / 8);
  const int64_t n_hr = static_cast<int64_t>(B) * T * (H + 2 * Hkv);
  if ((n_hr + groups - 1) / groups > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((n_hr + groups - 1) / groups));
  auto* Q = static_cast<const uint16_t*>(q);
  auto* K = static_cast<const uint16_t*>(k);
  auto* V = static_cast<const uint16_t*>(v);
  auto* C = static_cast<const uint16_t*>(cos);
  auto* S = static_cast<const uint16_t*>(sin);
  auto* GQ = static_cast<const uint16_t*>(q_gamma);
  auto* GK = static_cast<const uint16_t*>(k_gamma);
  auto* QO = static_cast<uint16_t*>(q_out);
#define DLION_KV_APPEND_CHUNK(DD, MODE)                                                                              \
  hipLaunchKernelGGL((kv_append_chunk_kernel<DD, MODE, FP8>), grid, dim3(256), 0, st, Q, K, V, q_bs, q_ts, k_bs,      \
                     k_ts, v_bs, v_ts, pos, n_new, C, S, GQ, GK, eps, QO, k_cache, v_cache, kc_bs, kc_ts, vc_bs,      \
                     vc_ts, k_scales, v_scales, sc_bs, sc_ts, B, T, H, Hkv, Tmax, err)
  const int mode = q_gamma != nullptr ? kNormRope : (cos != nullptr ? kRope : kAppend);
  if (D == 128) {
    if (mode == kNormRope) DLION_KV_APPEND_CHUNK(128, kNormRope);
    else if (mode == kRope) DLION_KV_APPEND_CHUNK(128, kRope);
    else DLION_KV_APPEND_CHUNK(128, kAppend);
  } else {
    if (mode == kNormRope) DLION_KV_APPEND_CHUNK(64, kNormRope);
    else if (mode == kRope) DLION_KV_APPEND_CHUNK(64, kRope);
    else DLION_KV_APPEND_CHUNK(64, kAppend);
  }
#undef DLION_KV_APPEND_CHUNK
  return hipGetLastError();
}


}  // namespace
}  // namespace dlion
