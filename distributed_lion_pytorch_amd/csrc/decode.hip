// Generation: the decode step's two kernels (bf16, head_dim 64 / 128) and their combine pass.
//
// kv_append.  One launch prepares a decode step's q / k / v (rows of the fused q|k|v projection output, one
// token per sequence): q and k are RMS-normalised over head_dim (Qwen3, optional) and rotated at the row's
// own position pos[b], v is copied; k and v go to cache[b, pos[b]] of the token-major [B, Tmax, Hkv, D]
// caches, q to a [B, H, D] buffer.  The rotation and the norm are rope_norm.h's functions, the ones
// rope_kernel and qk_norm.hip run: token t's key is the same bits whether the prefill or a decode step wrote
// it.  A head row is D / 8 adjacent lanes; head rows past the end are clamped (computed again, never
// stored), so the lanes a DPP move reads are always active.
//
// decode_attention.  One query per sequence against its cache: memory-bound, every K and V byte is needed
// once.  A block owns one (split, kv head, sequence): it streams its chunk of that kv head's keys and values
// straight from global memory into registers (16 bytes per lane, no LDS staging: nothing is shared between
// waves) and uses every loaded key for all G = H / Hkv query heads of the group, whose pre-scaled q sit in
// registers.  The group runs on VALU dot products: a key is D / 8 adjacent lanes with 8 dims each, a head's
// score is 8 FMAs and a DPP butterfly over those lanes.  (A 16-row MFMA would leave 16 - G rows idle and
// wants V transposed across lanes, i.e. an LDS round trip of every V byte; at G <= 4 the VALU form is
// already below the time the loads take.)  Each lane group keeps its own running max / sum / output per
// head (fp32, log2 domain); at the end the block merges its lane groups through LDS in a fixed order and
// writes one fp32 partial per head.  The combine kernel reduces the splits in index order.  No atomics
// anywhere: the same inputs give the same bits.
//
// Nothing at or beyond kv_len[b] is read: key indices are clamped into the block's own non-empty range
// before an address is formed and the clamped lanes' scores are -inf.  A block whose range is empty loads
// nothing and writes the neutral partial (max -inf, sum 0, output 0).
#include "common.h"
#include "kernels.h"
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
template <int D, int MODE>
__global__ void __launch_bounds__(256) kv_append_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t q_ld,
    int64_t k_ld, int64_t v_ld, const int* __restrict__ pos, const uint16_t* __restrict__ cs,
    const uint16_t* __restrict__ sn, const uint16_t* __restrict__ gq, const uint16_t* __restrict__ gk, float eps,
    uint16_t* __restrict__ q_out, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, int64_t kc_bs, int64_t kc_ts,
    int64_t vc_bs, int64_t vc_ts, int B, int H, int Hkv, int Tmax, int32_t* __restrict__ err) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
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
    if (valid) {
      *reinterpret_cast<uint2*>(dst + d0) = is_v ? ra : pack4(oa);
      *reinterpret_cast<uint2*>(dst + hd + d0) = is_v ? rb : pack4(ob);
    }
  } else {
    const int d0 = sub * 8;
    const uint4 raw = *reinterpret_cast<const uint4*>(src + d0);
    if constexpr (MODE == kAppend) {
      if (valid) *reinterpret_cast<uint4*>(dst + d0) = raw;
    } else {
      // qk_norm.hip's mapping; v rows run the same lanes (their result is dropped) so that no DPP move
      // reads an inactive lane
      float x[8], w[8], c[8], s[8], o[8];
      unpack8(raw, x);
      E::load8((is_q ? gq : gk) + d0, w);
      E::load8(cs + static_cast<int64_t>(p) * D + d0, c);
      E::load8(sn + static_cast<int64_t>(p) * D + d0, s);
      qk_norm_rope_row<LANES>(x, w, c, s, eps, sub < LANES / 2, o);
      if (valid) {
        if (is_v)
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        else
          E::store8(dst + d0, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------ decode attention
constexpr float kNegInf = -__builtin_huge_valf();

// keys in flight per lane group and iteration: 4 (2 at the widest group, whose q and outputs fill the registers)
template <int GP>
struct Unroll {
  static constexpr int value = GP == 8 ? 2 : 4;
};

// grid (splits, Hkv, B), 256 threads; GP = the group size G rounded up to 1 / 2 / 4 / 8 (heads past G repeat
// head G - 1 and are not stored).  chunk = keys per split; split s of row b owns the keys
// [lo + s chunk, lo + (s + 1) chunk) of the row's range [lo, len).
template <int D, int GP>
__global__ void __launch_bounds__(256) decode_attn_kernel(
    const uint16_t* __restrict__ q, int64_t q_ld, const uint16_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const uint16_t* __restrict__ vc, int64_t v_bs, int64_t v_ts, const int* __restrict__ kv_len,
    float* __restrict__ part_m, float* __restrict__ part_l, float* __restrict__ part_o, int H, int G, int Tmax,
    int max_len, int window, int chunk, float qscale) {
  constexpr int LANES = D / 8, KG = 256 / LANES, U = Unroll<GP>::value;
  __shared__ float sm_o[KG * D];
  __shared__ float sm_m[KG], sm_l[KG];
  const int sub = threadIdx.x % LANES, kg = threadIdx.x / LANES;
  const int d0 = sub * 8;
  const int s = blockIdx.x, S = gridDim.x, hk = blockIdx.y, b = blockIdx.z;
  int len = kv_len[b];
  len = len < max_len ? len : max_len;
  len = len < Tmax ? len : Tmax;
  len = len > 0 ? len : 0;
  const int lo = (window > 0 && len > window) ? len - window : 0;
  // s chunk <= span + chunk: no overflow for any cache that fits in memory
  const int64_t start64 = static_cast<int64_t>(lo) + static_cast<int64_t>(s) * chunk;
  const int start = start64 < len ? static_cast<int>(start64) : len;
  const int end = (len - start) > chunk ? start + chunk : len;
  const int h0 = hk * G;

  float acc[GP][8], m[GP], l[GP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    m[g] = kNegInf;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
  }

  if (start < end) {  // block-uniform
    float qf[GP][8];
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      const int hh = h0 + (g < G ? g : G - 1);
      E::load8(q + b * q_ld + static_cast<int64_t>(hh) * D + d0, qf[g]);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[g][i] *= qscale;
    }
    const uint16_t* kbase = kc + b * k_bs + static_cast<int64_t>(hk) * D + d0;
    const uint16_t* vbase = vc + b * v_bs + static_cast<int64_t>(hk) * D + d0;
    for (int j0 = start; j0 < end; j0 += U * KG) {  // block-uniform trip count
      uint4 kr[U], vr[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * KG + kg;
        ok[u] = j < end;
        const int64_t jc = ok[u] ? j : end - 1;  // a key of this block's own range: always below kv_len
        kr[u] = *reinterpret_cast<const uint4*>(kbase + jc * k_ts);
        vr[u] = *reinterpret_cast<const uint4*>(vbase + jc * v_ts);
      }
      float sc[GP][U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float kf[8];
        unpack8(kr[u], kf);
#pragma unroll
        for (int g = 0; g < GP; ++g) {
          float d = qf[g][0] * kf[0];
#pragma unroll
          for (int i = 1; i < 8; ++i) d = __builtin_fmaf(qf[g][i], kf[i], d);
          d = head_sum<LANES>(d);
          sc[g][u] = ok[u] ? d : kNegInf;
        }
      }
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        float mn = m[g];
#pragma unroll
        for (int u = 0; u < U; ++u) mn = fmaxf(mn, sc[g][u]);
        const float ms = mn == kNegInf ? 0.f : mn;  // a lane group that has seen no key yet
        const float alpha = __builtin_amdgcn_exp2f(m[g] - ms);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          sc[g][u] = __builtin_amdgcn_exp2f(sc[g][u] - ms);
          ps += sc[g][u];
        }
        l[g] = __builtin_fmaf(l[g], alpha, ps);
        m[g] = mn;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float vf[8];
        unpack8(vr[u], vf);
#pragma unroll
        for (int g = 0; g < GP; ++g)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(sc[g][u], vf[i], acc[g][i]);
      }
    }
  }

  // merge the block's KG lane groups, head by head, in lane-group order
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    if (g < G) {  // block-uniform
      __syncthreads();
      *reinterpret_cast<float4*>(&sm_o[kg * D + d0]) = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
      *reinterpret_cast<float4*>(&sm_o[kg * D + d0 + 4]) = make_float4(acc[g][4], acc[g][5], acc[g][6], acc[g][7]);
      if (sub == 0) {
        sm_m[kg] = m[g];
        sm_l[kg] = l[g];
      }
      __syncthreads();
      if (threadIdx.x < D) {
        float M = kNegInf;
        for (int i = 0; i < KG; ++i) M = fmaxf(M, sm_m[i]);
        const float Ms = M == kNegInf ? 0.f : M;
        float L = 0.f, O = 0.f;
        for (int i = 0; i < KG; ++i) {
          const float w = __builtin_amdgcn_exp2f(sm_m[i] - Ms);
          L = __builtin_fmaf(sm_l[i], w, L);
          O = __builtin_fmaf(sm_o[i * D + threadIdx.x], w, O);
        }
        const int64_t pi = (static_cast<int64_t>(b) * H + h0 + g) * S + s;
        part_o[pi * D + threadIdx.x] = O;
        if (threadIdx.x == 0) {
          part_m[pi] = M;
          part_l[pi] = L;
        }
      }
    }
  }
}

// grid B H blocks of D threads: out[b, h, d] = sum_s o_s[d] w_s / sum_s l_s w_s, w_s = 2^(m_s - max m), the
// splits in index order; a row without keys (all partials neutral) is zero
template <int D>
__global__ void __launch_bounds__(D) decode_combine_kernel(const float* __restrict__ part_m,
                                                          const float* __restrict__ part_l,
                                                          const float* __restrict__ part_o,
                                                          uint16_t* __restrict__ out, int S) {
  const int64_t bh = blockIdx.x;
  const float* pm = part_m + bh * S;
  const float* pl = part_l + bh * S;
  const float* po = part_o + bh * S * D + threadIdx.x;
  float M = kNegInf;
  for (int s = 0; s < S; ++s) M = fmaxf(M, pm[s]);
  const float Ms = M == kNegInf ? 0.f : M;
  float L = 0.f, O = 0.f;
  for (int s = 0; s < S; ++s) {
    const float w = __builtin_amdgcn_exp2f(pm[s] - Ms);
    L = __builtin_fmaf(pl[s], w, L);
    O = __builtin_fmaf(po[static_cast<int64_t>(s) * D], w, O);
  }
  out[bh * D + threadIdx.x] = f32_to_bf16(L > 0.f ? O / L : 0.f);
}

}  // namespace

hipError_t launch_kv_append(const void* q, const void* k, const void* v, int64_t q_ld, int64_t k_ld, int64_t v_ld,
                            const int* pos, const void* cos, const void* sin, const void* q_gamma,
                            const void* k_gamma, float eps, void* q_out, void* k_cache, void* v_cache, int64_t kc_bs,
                            int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, int B, int H, int Hkv, int D, int Tmax,
                            int32_t* err, hipStream_t st) {
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
  auto* KC = static_cast<uint16_t*>(k_cache);
  auto* VC = static_cast<uint16_t*>(v_cache);
#define DLION_KV_APPEND(DD, MODE)                                                                                    \
  hipLaunchKernelGGL((kv_append_kernel<DD, MODE>), grid, dim3(256), 0, st, Q, K, V, q_ld, k_ld, v_ld, pos, C, S, GQ, \
                     GK, eps, QO, KC, VC, kc_bs, kc_ts, vc_bs, vc_ts, B, H, Hkv, Tmax, err)
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

hipError_t launch_decode_attention(const void* q, int64_t q_ld, const void* k_cache, int64_t k_bs, int64_t k_ts,
                                   const void* v_cache, int64_t v_bs, int64_t v_ts, const int* kv_len, float* part_m,
                                   float* part_l, float* part_o, void* out, int B, int H, int Hkv, int D, int Tmax,
                                   int max_len, int window, int splits, int chunk, float scale, hipStream_t st) {
  if (B <= 0 || H <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Hkv <= 0 || H % Hkv != 0 || H / Hkv > 8) return hipErrorInvalidValue;
  if (Tmax <= 0 || max_len <= 0 || window < 0 || splits < 1 || splits > kDecodeMaxSplits || chunk < 1)
    return hipErrorInvalidValue;
  if (B > 65535 || Hkv > 65535) return hipErrorInvalidValue;
  const int span = (window > 0 && window < max_len) ? window : max_len;
  if (static_cast<int64_t>(splits) * chunk < span) return hipErrorInvalidValue;  // every key has a split
  const int G = H / Hkv;
  const dim3 grid(static_cast<unsigned>(splits), static_cast<unsigned>(Hkv), static_cast<unsigned>(B));
  auto* Q = static_cast<const uint16_t*>(q);
  auto* KC = static_cast<const uint16_t*>(k_cache);
  auto* VC = static_cast<const uint16_t*>(v_cache);
  const float qscale = scale * kLog2e;
#define DLION_DECODE(DD, GP)                                                                                        \
  hipLaunchKernelGGL((decode_attn_kernel<DD, GP>), grid, dim3(256), 0, st, Q, q_ld, KC, k_bs, k_ts, VC, v_bs, v_ts, \
                     kv_len, part_m, part_l, part_o, H, G, Tmax, max_len, window, chunk, qscale)
#define DLION_DECODE_D(DD)                  \
  if (G == 1) DLION_DECODE(DD, 1);          \
  else if (G == 2) DLION_DECODE(DD, 2);     \
  else if (G <= 4) DLION_DECODE(DD, 4);     \
  else DLION_DECODE(DD, 8)
  if (D == 128) {
    DLION_DECODE_D(128);
  } else {
    DLION_DECODE_D(64);
  }
#undef DLION_DECODE_D
#undef DLION_DECODE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 cgrid(static_cast<unsigned>(B * H));
  if (D == 128)
    hipLaunchKernelGGL(decode_combine_kernel<128>, cgrid, dim3(128), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  else
    hipLaunchKernelGGL(decode_combine_kernel<64>, cgrid, dim3(64), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  return hipGetLastError();
}

}  // namespace dlion
