// Generation: T tokens per sequence against the cache (speculative decoding's verification forward, a new
// turn on an existing cache, chunked prefill).  bf16, head_dim 64 / 128, 1 <= T <= 8, H / Hkv in 1..8.
//
// kv_append_chunk.  decode.hip's kv_append with a token index: the head row (b, t, slot) of the fused q|k|v
// projection output [B, T, ...] is normalised (Qwen3, optional) and rotated at position pos[b] + t by
// rope_norm.h's functions -- the bits of rope / qk_norm_rope at that position, whichever kernel wrote a key --
// and k / v go to cache[b, pos[b] + t].  Tokens t >= n_new[b] (ragged chunks) write nothing to the caches;
// their q row is computed by the same arithmetic and nothing depends on it.  A written token whose position
// lies outside [0, Tmax) raises kIndexErrCache and is not written at all.
//
// chunk_attention.  Query (b, t), t < n_new[b], attends the keys [lo_t, kv_len[b] + t + 1) of its cache, its
// own key included (kv_append_chunk ran first).  The grid and the reduction are decode.hip's: a block owns one
// (split, kv head, sequence) and a chunk of the row's key range [lo_0, kv_len + n_new) by a host rule that
// never reads device lengths; fp32 partials (max, sum, output) per split, a combine pass in index order, no
// atomics.  What differs is the arithmetic.  With T tokens there are R = T G query rows per kv head (up to
// 64): on VALU dot products a key would cost 2 R D FMAs, about 8 k at R = 32 and D = 128, against the ~38
// cycles per key and CU the load stream leaves, so the products run on v_mfma_f32_16x16x32_bf16 with the R
// rows (padded to MT 16-row tiles; padded rows repeat row R - 1, are masked and never stored) as one
// dimension.
//
//   S^T = K Q^T.  K is the A operand: lane l holds key l & 15, dims 32 ks + 8 (l >> 4) .. + 7 -- eight
//   contiguous bf16 of one key, a 16-byte global load straight into the operand registers.  Q^T is the B
//   operand (query l & 15, the same dims), loaded once per block; the scale is applied to the fp32 scores so
//   that q stays the bits kv_append_chunk wrote.  The result has the query on the lane and keys
//   4 (l >> 4) + r in its registers r = 0..3: the masks (causal inside the chunk, window, the block's range)
//   and the online softmax are lane-local up to one maximum over the four lane groups.
//
//   O^T = V^T P^T.  Two 16-key score tiles, converted to bf16, are the B operand of a k = 32 step as they
//   stand (P goes in as a bf16 high part and the bf16 of the remainder, two MFMAs: with P rounded to 8 bits the
//   cached forward's logits were measurably noisier than the decode kernel's, which keeps P in fp32; the loop is
//   bound by the K / V loads, not the MFMAs): element j of lane group g is key 16 (j >> 2) + 4 g + (j & 3), query l & 15.  The A operand must
//   hold V^T in that key order: V's 32 x D tile goes through LDS row-major and comes back through
//   ds_read_b64_tr_b16 (the approach of attention.hip's tr_frag), one read per 16-key tile giving lane i of a
//   group column d = 16 dt + i of keys 4 g .. 4 g + 3.  Rows are D + 16 elements apart: the eight rows a
//   32-lane half reads start 8 banks apart (conflict-free), every address is 8-byte aligned and the array is
//   16-byte aligned static LDS (the transposed read returns wrong data off alignment).  The accumulator has
//   the query on the lane again, so the rescale by 2^(m_old - m_new) is lane-local too.
//
// A block is 4 waves; wave w takes the 32-key tiles (at absolute multiples of 32) w, w + 4, ... and keeps its own
// running max / sum / output for all R rows, so the main loop has no block barrier: a wave stages, reads and
// overwrites only its own V tile (LDS operations of one wave execute in order).  K and V of a tile are loaded
// at the top of an iteration, 4 + 4 (D = 64) or 8 + 8 (D = 128) 16-byte loads per lane in flight; two blocks
// per CU overlap one block's softmax with the other's loads.  Registers: Q^T is MT D / 8 VGPRs and O^T
// MT D / 4, so MT >= 3 at D = 128 (T G > 32) needs more than the 256 registers two waves per SIMD leave and
// runs one block per CU (profiles/chunk_attention_resources.txt); every other shape keeps two.  At the end
// the waves' partials are merged through LDS (the V area, reused) in wave order, one 16-row tile at a time.
//
// Nothing at or beyond kv_len[b] + n_new[b] is read: key indices are clamped into the block's own non-empty
// range before an address is formed, and clamped or masked scores are -inf.  Queries t >= n_new[b] see no
// key: neutral partials (max -inf, sum 0, output 0), a zero output row.
#include "common.h"
#include "kernels.h"
#include "rope_norm.h"

namespace dlion {
namespace {

using E = Elem<kBF16>;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// grid: ceil(B T (H + 2 Hkv) / GROUPS) blocks of 256; a lane group of D / 8 lanes owns one head row of one
// token: slots [0, H) are q, [H, H + Hkv) k, the rest v (kv_append_kernel's mapping with a token index)
template <int D, int MODE>
__global__ void __launch_bounds__(256) kv_append_chunk_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t q_bs,
    int64_t q_ts, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* __restrict__ pos,
    const int* __restrict__ n_new, const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn,
    const uint16_t* __restrict__ gq, const uint16_t* __restrict__ gk, float eps, uint16_t* __restrict__ q_out,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts,
    int B, int T, int H, int Hkv, int Tmax, int32_t* __restrict__ err) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
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
    if (store) {
      *reinterpret_cast<uint2*>(dst + d0) = is_v ? ra : pack4(oa);
      *reinterpret_cast<uint2*>(dst + hd + d0) = is_v ? rb : pack4(ob);
    }
  } else {
    const int d0 = sub * 8;
    const uint4 raw = *reinterpret_cast<const uint4*>(src + d0);
    if constexpr (MODE == kAppend) {
      if (store) *reinterpret_cast<uint4*>(dst + d0) = raw;
    } else {
      // v rows run the same lanes (their result is dropped) so that no DPP move reads an inactive lane
      float x[8], w[8], c[8], s[8], o[8];
      unpack8(raw, x);
      E::load8((is_q ? gq : gk) + d0, w);
      E::load8(cs + static_cast<int64_t>(p) * D + d0, c);
      E::load8(sn + static_cast<int64_t>(p) * D + d0, s);
      qk_norm_rope_row<LANES>(x, w, c, s, eps, sub < LANES / 2, o);
      if (store) {
        if (is_v)
          *reinterpret_cast<uint4*>(dst + d0) = raw;
        else
          E::store8(dst + d0, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------- chunk attention
constexpr float kNegInf = -__builtin_huge_valf();
constexpr int kWaves = 4, kTileKeys = 32;

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld_frag(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p));
}
// maximum / sum over the four lane groups l >> 4 that share a query column
__device__ __forceinline__ float groups_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float groups_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// grid (splits, Hkv, B), 256 threads.  MT = ceil(T G / 16) query tiles.  q [B, T, H, D] contiguous.  Row b's
// key range is [lo, len + n), lo = the window's lower edge of query 0; split s owns [lo + s chunk, lo + (s + 1)
// chunk) of it.  Partials: part_m / part_l [B, T, H, S], part_o [B, T, H, S, D].
// The second launch bound asks for two waves per SIMD (256 registers) wherever the tiles allow it.
template <int D, int MT>
__global__ void __launch_bounds__(256, (D == 64 || MT <= 2) ? 2 : 1) chunk_attn_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const uint16_t* __restrict__ vc, int64_t v_bs, int64_t v_ts, const int* __restrict__ kv_len,
    const int* __restrict__ n_new, float* __restrict__ part_m, float* __restrict__ part_l,
    float* __restrict__ part_o, int T, int H, int G, int Tmax, int max_len, int window, int chunk, float qscale) {
  constexpr int KS = D / 32, DT = D / 16, VS = D + 16;  // k steps of Q K^T, 16-dim tiles of O^T, V row stride
  constexpr int LPK = D / 8, KPP = 64 / LPK, NP = kTileKeys / KPP;  // V staging: lanes per key, keys per pass
  __shared__ __attribute__((aligned(16))) uint16_t vs_[kWaves * kTileKeys * VS];
  __shared__ float sm_m[kWaves][16], sm_l[kWaves][16];
  static_assert(sizeof(uint16_t) * kWaves * kTileKeys * VS >= sizeof(float) * kWaves * 16 * D, "merge area");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c = lane & 15, grp = lane >> 4;
  const int s = blockIdx.x, S = gridDim.x, hk = blockIdx.y, b = blockIdx.z;
  const int R = T * G;
  const int cap = max_len < Tmax ? max_len : Tmax;
  int len = kv_len[b];
  len = len < cap ? len : cap;
  len = len > 0 ? len : 0;
  int n = n_new != nullptr ? n_new[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  n = n < cap - len ? n : cap - len;
  const int hi = len + n;
  const int lo = (window > 0 && len + 1 > window) ? len + 1 - window : 0;
  // s chunk <= span + chunk: no overflow for any cache that fits in memory
  const int64_t start64 = static_cast<int64_t>(lo) + static_cast<int64_t>(s) * chunk;
  int start = start64 < hi ? static_cast<int>(start64) : hi;
  const int end = (hi - start) > chunk ? start + chunk : hi;
  if (n == 0) start = end;
  const int h0 = hk * G;

  f32x4 o[MT][DT];
  float m[MT], l[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    m[mt] = kNegInf;
    l[mt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[mt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // tiles sit at absolute multiples of 32 keys and tile i belongs to wave i & 3 (keys below `start` in the first
  // tile are masked like those at and beyond `end`): with one split a query's arithmetic depends on its own key
  // range alone, not on the chunk it came in -- re-feeding tokens after a rollback reproduces their bits
  const int tile0 = start / kTileKeys;
  const int first = (tile0 + ((wave - tile0) & (kWaves - 1))) * kTileKeys;  // the wave's first tile, >= start - 31
  if (start < end && first < end) {  // wave-uniform
    bf16x8 qf[MT][KS];
    int klo[MT], khi[MT];  // the lane's query sees the keys [klo, khi) of this block
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = 16 * mt + c;
      const int rc = row < R ? row : R - 1;
      const int t = rc / G, g = rc - t * G;
      const int top = len + t + 1;
      const bool live = row < R && t < n;
      khi[mt] = live ? (top < end ? top : end) : 0;
      const int wlo = (window > 0 && top > window) ? top - window : 0;
      klo[mt] = wlo > start ? wlo : start;
      const uint16_t* qp = q + ((static_cast<int64_t>(b) * T + t) * H + h0 + g) * D + 8 * grp;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[mt][ks] = ld_frag(qp + 32 * ks);
    }
    const uint16_t* kbase = kc + b * k_bs + static_cast<int64_t>(hk) * D + 8 * grp;
    const uint16_t* vbase = vc + b * v_bs + static_cast<int64_t>(hk) * D + 8 * (lane % LPK);
    uint16_t* vw = vs_ + wave * (kTileKeys * VS);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

    for (int j0 = first; j0 < end; j0 += kTileKeys * kWaves) {  // wave-uniform
      bf16x8 kf[2][KS];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const int j = j0 + 16 * kt + c;
        // a key of this block's own range: below kv_len + n_new
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[kt][ks] = ld_frag(kbase + jc * k_ts + 32 * ks);
      }
      uint4 vr[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int j = j0 + p * KPP + lane / LPK;
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
        vr[p] = *reinterpret_cast<const uint4*>(vbase + jc * v_ts);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
        *reinterpret_cast<uint4*>(vw + (p * KPP + lane / LPK) * VS + 8 * (lane % LPK)) = vr[p];

      bf16x8 pf[MT], pl[MT];  // P as bf16 high and low parts: 16 bits of it reach the product
      float alpha[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 sc[2];
        float mx = kNegInf;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) sc[kt] = mfma16(kf[kt][ks], qf[mt][ks], sc[kt]);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = j0 + 16 * kt + 4 * grp + r;
            sc[kt][r] = (j >= klo[mt] && j < khi[mt]) ? sc[kt][r] * qscale : kNegInf;
            mx = fmaxf(mx, sc[kt][r]);
          }
        }
        mx = groups_max(mx);
        const float mn = fmaxf(m[mt], mx);
        const float ms = mn == kNegInf ? 0.f : mn;  // a query that has seen no key yet
        alpha[mt] = __builtin_amdgcn_exp2f(m[mt] - ms);
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(sc[kt][r] - ms);
            ps += e;
            const __bf16 eh = static_cast<__bf16>(e);
            pf[mt][4 * kt + r] = eh;
            pl[mt][4 * kt + r] = static_cast<__bf16>(e - static_cast<float>(eh));
          }
        l[mt] = __builtin_fmaf(l[mt], alpha[mt], ps);  // the lane's share of the sum; the groups are added at the end
        m[mt] = mn;
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        // V^T fragment: rows = keys 16 kt + 4 grp .. + 3, columns 16 dt .. 16 dt + 15; lane 4 q + p of a group
        // addresses row q, columns 4 p .. 4 p + 3 and receives column (lane & 15) of the four rows
        const uint16_t* vp = vw + (4 * grp + (c >> 2)) * VS + 16 * dt + 4 * (c & 3);
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp + 16 * VS));
        const i32x2 a0 = __builtin_bit_cast(i32x2, v0), a1 = __builtin_bit_cast(i32x2, v1);
        const i32x4 av = {a0[0], a0[1], a1[0], a1[1]};
        const bf16x8 vf = __builtin_bit_cast(bf16x8, av);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) o[mt][dt][r] *= alpha[mt];
          o[mt][dt] = mfma16(vf, pl[mt], mfma16(vf, pf[mt], o[mt][dt]));
        }
      }
    }
  }

  // merge the block's waves, one 16-row tile at a time, in wave order
  float* so = reinterpret_cast<float*>(vs_);  // [wave][query][D]
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const float lsum = groups_sum(l[mt]);
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      *reinterpret_cast<float4*>(&so[(wave * 16 + c) * D + 16 * dt + 4 * grp]) =
          make_float4(o[mt][dt][0], o[mt][dt][1], o[mt][dt][2], o[mt][dt][3]);
    if (grp == 0) {
      sm_m[wave][c] = m[mt];
      sm_l[wave][c] = lsum;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * D; idx += 256) {
      const int qc = idx / D, d = idx - qc * D;
      const int row = 16 * mt + qc;
      if (row < R) {
        float M = kNegInf;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) M = fmaxf(M, sm_m[w][qc]);
        const float Ms = M == kNegInf ? 0.f : M;
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          const float wt = __builtin_amdgcn_exp2f(sm_m[w][qc] - Ms);
          L = __builtin_fmaf(sm_l[w][qc], wt, L);
          O = __builtin_fmaf(so[(w * 16 + qc) * D + d], wt, O);
        }
        const int t = row / G, g = row - t * G;
        const int64_t pi = ((static_cast<int64_t>(b) * T + t) * H + h0 + g) * S + s;
        part_o[pi * D + d] = O;
        if (d == 0) {
          part_m[pi] = M;
          part_l[pi] = L;
        }
      }
    }
  }
}

// grid B T H blocks of D threads: decode.hip's combine over the rows (b, t, h); a query without keys is zero
template <int D>
__global__ void __launch_bounds__(D) chunk_combine_kernel(const float* __restrict__ part_m,
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

hipError_t launch_kv_append_chunk(const void* q, const void* k, const void* v, int64_t q_bs, int64_t q_ts,
                                  int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* pos,
                                  const int* n_new, const void* cos, const void* sin, const void* q_gamma,
                                  const void* k_gamma, float eps, void* q_out, void* k_cache, void* v_cache,
                                  int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, int B, int T, int H,
                                  int Hkv, int D, int Tmax, int32_t* err, hipStream_t st) {
  if (B <= 0 || T <= 0 || H <= 0 || Hkv <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Tmax <= 0 || err == nullptr || T > kChunkMaxTokens) return hipErrorInvalidValue;
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
  auto* KC = static_cast<uint16_t*>(k_cache);
  auto* VC = static_cast<uint16_t*>(v_cache);
#define DLION_KV_APPEND_CHUNK(DD, MODE)                                                                             \
  hipLaunchKernelGGL((kv_append_chunk_kernel<DD, MODE>), grid, dim3(256), 0, st, Q, K, V, q_bs, q_ts, k_bs, k_ts,    \
                     v_bs, v_ts, pos, n_new, C, S, GQ, GK, eps, QO, KC, VC, kc_bs, kc_ts, vc_bs, vc_ts, B, T, H, Hkv, \
                     Tmax, err)
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

hipError_t launch_chunk_attention(const void* q, const void* k_cache, int64_t k_bs, int64_t k_ts,
                                  const void* v_cache, int64_t v_bs, int64_t v_ts, const int* kv_len,
                                  const int* n_new, float* part_m, float* part_l, float* part_o, void* out, int B,
                                  int T, int H, int Hkv, int D, int Tmax, int max_len, int window, int splits,
                                  int chunk, float scale, hipStream_t st) {
  if (B <= 0 || H <= 0 || T <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Hkv <= 0 || H % Hkv != 0 || H / Hkv > 8 || T > kChunkMaxTokens)
    return hipErrorInvalidValue;
  if (Tmax <= 0 || max_len <= 0 || window < 0 || splits < 1 || splits > kDecodeMaxSplits || chunk < 1)
    return hipErrorInvalidValue;
  if (B > 65535 || Hkv > 65535) return hipErrorInvalidValue;
  // the keys of a row span [lo_0, len + n): at most max_len, and window + T - 1 under a window
  const int64_t wspan = static_cast<int64_t>(window) + T - 1;
  const int64_t span = (window > 0 && wspan < max_len) ? wspan : max_len;
  if (static_cast<int64_t>(splits) * chunk < span) return hipErrorInvalidValue;  // every key has a split
  const int G = H / Hkv;
  const int MT = (T * G + 15) / 16;
  const dim3 grid(static_cast<unsigned>(splits), static_cast<unsigned>(Hkv), static_cast<unsigned>(B));
  auto* Q = static_cast<const uint16_t*>(q);
  auto* KC = static_cast<const uint16_t*>(k_cache);
  auto* VC = static_cast<const uint16_t*>(v_cache);
  const float qscale = scale * kLog2e;
#define DLION_CHUNK(DD, MM)                                                                                        \
  hipLaunchKernelGGL((chunk_attn_kernel<DD, MM>), grid, dim3(256), 0, st, Q, KC, k_bs, k_ts, VC, v_bs, v_ts, kv_len, \
                     n_new, part_m, part_l, part_o, T, H, G, Tmax, max_len, window, chunk, qscale)
#define DLION_CHUNK_D(DD)                \
  if (MT == 1) DLION_CHUNK(DD, 1);       \
  else if (MT == 2) DLION_CHUNK(DD, 2);  \
  else if (MT == 3) DLION_CHUNK(DD, 3);  \
  else DLION_CHUNK(DD, 4)
  if (D == 128) {
    DLION_CHUNK_D(128);
  } else {
    DLION_CHUNK_D(64);
  }
#undef DLION_CHUNK_D
#undef DLION_CHUNK
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 cgrid(static_cast<unsigned>(B * T * H));
  if (D == 128)
    hipLaunchKernelGGL(chunk_combine_kernel<128>, cgrid, dim3(128), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  else
    hipLaunchKernelGGL(chunk_combine_kernel<64>, cgrid, dim3(64), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  return hipGetLastError();
}

}  // namespace dlion
