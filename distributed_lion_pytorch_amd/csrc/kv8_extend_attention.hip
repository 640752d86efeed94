// Generation on an fp8 KV cache, T new tokens per sequence, any T: extend_attention.hip's semantics on the operands
// of kv8_attention.hip.  Codes uint8 [B, Tmax, Hkv, D] (OCP e4m3fn) and scales fp32 [B, Tmax, Hkv] of k and v, both
// strided; q bf16 [B, T, H, D], head_dim 64 / 128, H / Hkv in 1..8.  Query (b, t), t < n_new[b], attends the keys
// [max(0, len + t + 1 - window), len + t + 1) of its cache, len = kv_len[b], its own key included (kv_append_chunk
// ran first); kv_len = 0 is causal self-attention read from the cache.  Only what is cached is quantised: q and P
// stay bf16 (P as a high and a low part) and the products run on v_mfma_f32_16x16x32_bf16, not on fp8 MFMAs.
//
// The split of the work is the bf16 extend kernel's, because its reasons carry over unchanged:
//
//   A block owns (a tile of kExtendTQ = 16 consecutive tokens, one kv head, one sequence, one key split).  Its
//   query rows are the 16 G (token, head-in-group) pairs, head-major: the 16-row MFMA tile g holds the 16 tokens of
//   query head h0 + g, so a lane's causal / window bounds depend on its token alone.  Wave w keeps Q, the running
//   max, sum and O^T of the tiles g = w and w + 4 (MT = 1 for G <= 4, 2 above).  The four waves share 64-key K / V
//   tiles at absolute multiples of 64 through double-buffered LDS, one barrier per tile.  Tiles wholly above the
//   diagonal or below the window are never loaded; a tile that every live query of the block sees in full takes
//   the step without the per-element compares.
//
// What is new is how the keys travel:
//
//   Global memory -> registers.  A lane loads 16 codes of one key in one 16-byte load (D / 16 lanes per key, 64
//   keys per pass at D = 64 and 32 at D = 128): D / 64 uint4 per lane for K and as many for V, half of what the
//   bf16 kernel parks.  The loads of tile i + 1 are issued before the MFMAs of tile i and parked in registers.
//
//   Registers -> LDS, converted once per block.  After the MFMAs of tile i each lane turns its parked codes into
//   bf16 (kv8_codes_to_bf16: v_cvt_pk_f32_fp8 and packs of the high halves; an e4m3 value is exact in bf16) and
//   stores them to the other buffer in the bf16 kernel's layouts, so the read side is that kernel's: K rows D + 8
//   elements apart (the 16 lanes of a group read 16 bytes of 16 consecutive keys, 4 banks further each,
//   conflict-free), V row-major with rows D + 16 elements apart so that ds_read_b64_tr_b16 brings back V^T (8-byte
//   aligned read addresses, 16-byte aligned static arrays).  Both row strides are multiples of 16 bytes (144 / 272
//   and 160 / 288), so a lane's 32 converted bytes go out as two 16-byte LDS stores.
//
//   The alternative -- raw codes in LDS, each wave converting what it reads -- halves the LDS bytes but repeats the
//   conversion VALU in all four waves, which read every key of the tile each.  kv8_attention.hip's header found
//   its loop bound by global loads and VALU, not by LDS, so the conversion is paid once per block, on the store
//   side, and LDS carries bf16.  The budget at D = 128: K 2 x 64 x 136 x 2 = 34,816 bytes and V 2 x 64 x 144 x 2 =
//   36,864, together 71,680 for the two double-buffered tiles, plus 1,024 for the scale rows: 72,704 per block,
//   two blocks in a CU's 160 KiB.  D = 64: 38,912 + 1,024.
//
//   Scales.  The 64 key scales and the 64 value scales of a tile are loaded by the block's first 128 lanes (wave 0
//   the keys', wave 1 the values') alongside the codes, at the same clamped key index, parked in one register and
//   stored to double-buffered LDS rows float [2][2][64]; the key's row is stored times log2(e) / sqrt(D).  They
//   fold in where kv8_attention.hip folds them, exactly, being powers of two: the key's scale into its fp32 score
//   in the multiply that applies log2(e) / sqrt(D), the value's into P before the bf16 high / low split.  A
//   lane's four score registers of a 16-key tile are four consecutive keys, so both come back as one float4.
//
// Splits over the keys (ops/fused.py extend_splits, a host rule that never reads device lengths): split s of a
// query tile owns [lo + s chunk, lo + (s + 1) chunk) of the tile's own range.  With one split the block divides by
// the sum and stores bf16 itself; otherwise fp32 partials in chunk_attention's layout (part_m / part_l
// [B, T, H, S], part_o [B, T, H, S, D]) and its combine pass in index order.  No atomics.
//
// Nothing at or beyond kv_len[b] + n_new[b] is read, neither a code nor a scale: key indices are clamped into the
// block's own non-empty range before an address is formed, and clamped or masked scores are -inf (P = 0 times a
// finite in-range value and scale).  Queries t >= n_new[b] store constants (neutral partials, zero rows), whatever
// their lanes computed.
//
// Resources (profiles/kv8_extend_resources.txt): no scratch in any of the four instantiations, two blocks per CU.
#include "common.h"
#include "kernels.h"
#include "kv8.h"

namespace dlion {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kNegInf = -__builtin_huge_valf();
constexpr int kTileKeys = 64, kStepKeys = 32, kTQ = kExtendTQ;
static_assert(kTQ == 16, "one 16-row MFMA tile per query head");

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
// 16 codes -> 16 bf16 at dst (16-byte aligned LDS): two 16-byte stores
__device__ __forceinline__ void store_codes(uint16_t* dst, const uint4& raw) {
  const uint2 a = kv8_codes_to_bf16(raw.x), b = kv8_codes_to_bf16(raw.y);
  const uint2 c = kv8_codes_to_bf16(raw.z), d = kv8_codes_to_bf16(raw.w);
  *reinterpret_cast<uint4*>(dst) = make_uint4(a.x, a.y, b.x, b.y);
  *reinterpret_cast<uint4*>(dst + 8) = make_uint4(c.x, c.y, d.x, d.y);
}

// One wave's state: MT query tiles (heads g = wave + 4 mt) of 16 tokens.
template <int D, int MT>
struct Rows {
  static constexpr int KS = D / 32, DT = D / 16;
  bf16x8 q[MT][KS];
  f32x4 o[MT][DT];
  float m[MT], l[MT];
};

// keys [kb, kb + 32) of the LDS tile at absolute key j0 + kb, their scales at ksc_ (times log2(e) / sqrt(D)) and
// vsc_; MASKED: the lane's query sees [klo, khi) only
template <int D, int MT, bool MASKED>
__device__ __forceinline__ void step32(Rows<D, MT>& w, const uint16_t* kt_, const uint16_t* vt_, const float* ksc_,
                                       const float* vsc_, int jb, int klo, int khi, int c, int grp) {
  constexpr int KS = D / 32, DT = D / 16, KSD = D + 8, VS = D + 16;
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  bf16x8 kf[2][KS];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[kt][ks] = ld_frag(kt_ + (16 * kt + c) * KSD + 32 * ks + 8 * grp);
  // the scales of the lane's keys 16 kt + 4 grp .. + 3
  float kq[2][4], vq[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const float4 a = *reinterpret_cast<const float4*>(ksc_ + 16 * kt + 4 * grp);
    const float4 b = *reinterpret_cast<const float4*>(vsc_ + 16 * kt + 4 * grp);
    kq[kt][0] = a.x, kq[kt][1] = a.y, kq[kt][2] = a.z, kq[kt][3] = a.w;
    vq[kt][0] = b.x, vq[kt][1] = b.y, vq[kt][2] = b.z, vq[kt][3] = b.w;
  }
  bf16x8 pf[MT], pl[MT];  // P times the value scale as bf16 high and low parts: 16 bits of it reach the product
  float alpha[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    f32x4 sc[2];
    float mx = kNegInf;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) sc[kt] = mfma16(kf[kt][ks], w.q[mt][ks], sc[kt]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MASKED) {
          const int j = jb + 16 * kt + 4 * grp + r;
          sc[kt][r] = (j >= klo && j < khi) ? sc[kt][r] * kq[kt][r] : kNegInf;
        } else {
          sc[kt][r] *= kq[kt][r];
        }
        mx = fmaxf(mx, sc[kt][r]);
      }
    }
    mx = groups_max(mx);
    const float mn = fmaxf(w.m[mt], mx);
    const float ms = mn == kNegInf ? 0.f : mn;  // a query that has seen no key yet
    alpha[mt] = __builtin_amdgcn_exp2f(w.m[mt] - ms);
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(sc[kt][r] - ms);
        ps += e;
        const float ev = e * vq[kt][r];
        const __bf16 eh = static_cast<__bf16>(ev);
        pf[mt][4 * kt + r] = eh;
        pl[mt][4 * kt + r] = static_cast<__bf16>(ev - static_cast<float>(eh));
      }
    w.l[mt] = __builtin_fmaf(w.l[mt], alpha[mt], ps);  // the lane's share of the sum; the groups are added at the end
    w.m[mt] = mn;
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    // V^T fragment: rows = keys 16 kt + 4 grp .. + 3, columns 16 dt .. 16 dt + 15; lane 4 q + p of a group
    // addresses row q, columns 4 p .. 4 p + 3 and receives column (lane & 15) of the four rows
    const uint16_t* vp = vt_ + (4 * grp + (c >> 2)) * VS + 16 * dt + 4 * (c & 3);
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp + 16 * VS));
    const i32x2 a0 = __builtin_bit_cast(i32x2, v0), a1 = __builtin_bit_cast(i32x2, v1);
    const i32x4 av = {a0[0], a0[1], a1[0], a1[1]};
    const bf16x8 vf = __builtin_bit_cast(bf16x8, av);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) w.o[mt][dt][r] *= alpha[mt];
      w.o[mt][dt] = mfma16(vf, pl[mt], mfma16(vf, pf[mt], w.o[mt][dt]));
    }
  }
}

// grid (ceil(T / 16) S, Hkv, B), 256 threads; block x = query tile * S + split.  q [B, T, H, D] contiguous.
// S == 1: out [B, T, H D] bf16 is written here; otherwise the partials.
template <int D, int MT>
__global__ void __launch_bounds__(256, 2) kv8_extend_attn_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const float* __restrict__ ksc, int64_t ks_bs, int64_t ks_ts, const uint8_t* __restrict__ vc, int64_t v_bs,
    int64_t v_ts, const float* __restrict__ vsc, int64_t vs_bs, int64_t vs_ts, const int* __restrict__ kv_len,
    const int* __restrict__ n_new, float* __restrict__ part_m, float* __restrict__ part_l,
    float* __restrict__ part_o, uint16_t* __restrict__ out, int T, int H, int G, int S, int Tmax, int max_len,
    int window, int chunk, float qscale) {
  constexpr int KS = D / 32, DT = D / 16, KSD = D + 8, VS = D + 16;
  constexpr int LPK = D / 16, KPP = 256 / LPK, NP = kTileKeys / KPP;  // staging: lanes per key, keys per pass, passes
  static_assert((KSD * 2) % 16 == 0 && (VS * 2) % 16 == 0, "16-byte LDS stores of the converted codes");
  __shared__ __attribute__((aligned(16))) uint16_t ks_[2][kTileKeys * KSD];
  __shared__ __attribute__((aligned(16))) uint16_t vs_[2][kTileKeys * VS];
  __shared__ __attribute__((aligned(16))) float sc_[2][2][kTileKeys];  // [buffer][k, v][key of the tile]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c = lane & 15, grp = lane >> 4;
  const int qt = blockIdx.x / S, s = blockIdx.x - qt * S, hk = blockIdx.y, b = blockIdx.z;
  const int cap = max_len < Tmax ? max_len : Tmax;
  int len = kv_len[b];
  len = len < cap ? len : cap;
  len = len > 0 ? len : 0;
  int n = n_new != nullptr ? n_new[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  n = n < cap - len ? n : cap - len;
  const int t0 = qt * kTQ;
  const int tn = t0 + kTQ < n ? t0 + kTQ : n;  // one past the tile's last live token
  // the tile's keys: [window edge of token t0, causal top of token tn - 1); empty when the tile has no live token
  int start = 0, end = 0;
  if (t0 < n) {
    const int hi = len + tn;
    const int lo = (window > 0 && len + t0 + 1 > window) ? len + t0 + 1 - window : 0;
    // s chunk <= span + chunk: no overflow for any cache that fits in memory
    const int64_t start64 = static_cast<int64_t>(lo) + static_cast<int64_t>(s) * chunk;
    start = start64 < hi ? static_cast<int>(start64) : hi;
    end = (hi - start) > chunk ? start + chunk : hi;
  }
  const int h0 = hk * G;
  const int t = t0 + c;  // the lane's token
  const bool live = t < n;

  Rows<D, MT> w;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    w.m[mt] = kNegInf;
    w.l[mt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) w.o[mt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  if (start < end) {  // block-uniform
    const int top = len + t + 1;
    const int khi = live ? (top < end ? top : end) : 0;  // the lane's query sees the keys [klo, khi) of this block
    const int wlo = (window > 0 && top > window) ? top - window : 0;
    const int klo = wlo > start ? wlo : start;
    // every live query of the tile sees all of [full_lo, full_hi)
    const int full_hi = (len + t0 + 1) < end ? (len + t0 + 1) : end;
    const int wlast = (window > 0 && len + tn > window) ? len + tn - window : 0;
    const int full_lo = wlast > start ? wlast : start;
    const bool has_rows = wave < G;  // wave-uniform: G < 4 leaves waves that only stage
    {
      const int tc = t < T ? t : T - 1;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int g = (wave + 4 * mt) < G ? wave + 4 * mt : G - 1;
        const uint16_t* qp = q + ((static_cast<int64_t>(b) * T + tc) * H + h0 + g) * D + 8 * grp;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) w.q[mt][ks] = ld_frag(qp + 32 * ks);
      }
    }
    const int skey = threadIdx.x / LPK, scol = 16 * (threadIdx.x % LPK);
    const uint8_t* kbase = kc + b * k_bs + static_cast<int64_t>(hk) * D + scol;
    const uint8_t* vbase = vc + b * v_bs + static_cast<int64_t>(hk) * D + scol;
    // the scales: wave 0 loads the keys', wave 1 the values', lane l that of key l of the tile
    const bool has_scale = wave < 2;
    const float* sbase = wave == 0 ? ksc + b * ks_bs + hk : vsc + b * vs_bs + hk;
    const int64_t s_ts = wave == 0 ? ks_ts : vs_ts;
    const float smul = wave == 0 ? qscale : 1.f;
    uint4 kr[NP], vr[NP];
    float sr = 0.f;
    auto load_tile = [&](int j0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int j = j0 + p * KPP + skey;
        // a key of this block's own range: below kv_len + n_new
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
        kr[p] = *reinterpret_cast<const uint4*>(kbase + jc * k_ts);
        vr[p] = *reinterpret_cast<const uint4*>(vbase + jc * v_ts);
      }
      if (has_scale) {
        const int j = j0 + lane;
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
        sr = sbase[jc * s_ts] * smul;
      }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        store_codes(&ks_[buf][(p * KPP + skey) * KSD + scol], kr[p]);
        store_codes(&vs_[buf][(p * KPP + skey) * VS + scol], vr[p]);
      }
      if (has_scale) sc_[buf][wave][lane] = sr;
    };
    const int first = (start / kTileKeys) * kTileKeys;
    load_tile(first);
    store_tile(0);
    __syncthreads();
    int buf = 0;
    for (int j0 = first; j0 < end; j0 += kTileKeys, buf ^= 1) {  // block-uniform
      const bool more = j0 + kTileKeys < end;
      if (more) load_tile(j0 + kTileKeys);
      if (has_rows) {
        const bool full = j0 >= full_lo && j0 + kTileKeys <= full_hi;
#pragma unroll
        for (int kb = 0; kb < kTileKeys; kb += kStepKeys) {
          const uint16_t* kt_ = &ks_[buf][kb * KSD];
          const uint16_t* vt_ = &vs_[buf][kb * VS];
          const float* ksc_ = &sc_[buf][0][kb];
          const float* vsc_ = &sc_[buf][1][kb];
          if (full)
            step32<D, MT, false>(w, kt_, vt_, ksc_, vsc_, j0 + kb, klo, khi, c, grp);
          else if (j0 + kb < end && j0 + kb + kStepKeys > start)
            step32<D, MT, true>(w, kt_, vt_, ksc_, vsc_, j0 + kb, klo, khi, c, grp);
        }
      }
      if (more) store_tile(buf ^ 1);
      __syncthreads();
    }
  }

  // every wave stores its own rows: no merge across waves
  if (t < T) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int g = wave + 4 * mt;
      if (g >= G) continue;
      const float lsum = groups_sum(w.l[mt]);
      const int64_t row = (static_cast<int64_t>(b) * T + t) * H + h0 + g;
      if (S == 1) {
        const float inv = (live && lsum > 0.f) ? 1.f / lsum : 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const f32x4 ov = w.o[mt][dt];
          uint2 pk = make_uint2(0u, 0u);
          if (live) {
            pk.x = static_cast<uint32_t>(f32_to_bf16(ov[0] * inv)) | (static_cast<uint32_t>(f32_to_bf16(ov[1] * inv)) << 16);
            pk.y = static_cast<uint32_t>(f32_to_bf16(ov[2] * inv)) | (static_cast<uint32_t>(f32_to_bf16(ov[3] * inv)) << 16);
          }
          *reinterpret_cast<uint2*>(out + row * D + 16 * dt + 4 * grp) = pk;
        }
      } else {
        const int64_t pi = row * S + s;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          *reinterpret_cast<float4*>(part_o + pi * D + 16 * dt + 4 * grp) =
              live ? make_float4(w.o[mt][dt][0], w.o[mt][dt][1], w.o[mt][dt][2], w.o[mt][dt][3])
                   : make_float4(0.f, 0.f, 0.f, 0.f);
        if (grp == 0) {
          part_m[pi] = live ? w.m[mt] : kNegInf;
          part_l[pi] = live ? lsum : 0.f;
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_extend_attention_fp8(const void* q, const uint8_t* k_codes, int64_t k_bs, int64_t k_ts,
                                       const float* k_scales, int64_t ks_bs, int64_t ks_ts, const uint8_t* v_codes,
                                       int64_t v_bs, int64_t v_ts, const float* v_scales, int64_t vs_bs, int64_t vs_ts,
                                       const int* kv_len, const int* n_new, float* part_m, float* part_l,
                                       float* part_o, void* out, int B, int T, int H, int Hkv, int D, int Tmax,
                                       int max_len, int window, int splits, int chunk, float scale, hipStream_t st) {
  if (B <= 0 || H <= 0 || T <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Hkv <= 0 || H % Hkv != 0 || H / Hkv > 8) return hipErrorInvalidValue;
  if (Tmax <= 0 || max_len <= 0 || window < 0 || splits < 1 || splits > kDecodeMaxSplits || chunk < 1)
    return hipErrorInvalidValue;
  if (B > 65535 || Hkv > 65535) return hipErrorInvalidValue;
  if (k_codes == nullptr || v_codes == nullptr || k_scales == nullptr || v_scales == nullptr)
    return hipErrorInvalidValue;
  if (splits > 1 && (part_m == nullptr || part_l == nullptr || part_o == nullptr)) return hipErrorInvalidValue;
  // the keys of a query tile span at most max_len, and window + 15 under a window
  const int64_t wspan = static_cast<int64_t>(window) + kExtendTQ - 1;
  const int64_t span = (window > 0 && wspan < max_len) ? wspan : max_len;
  if (static_cast<int64_t>(splits) * chunk < span) return hipErrorInvalidValue;  // every key has a split
  const int64_t tiles = (static_cast<int64_t>(T) + kExtendTQ - 1) / kExtendTQ;
  if (tiles * splits > 0x7fffffff) return hipErrorInvalidValue;
  const int G = H / Hkv;
  const dim3 grid(static_cast<unsigned>(tiles * splits), static_cast<unsigned>(Hkv), static_cast<unsigned>(B));
  auto* Q = static_cast<const uint16_t*>(q);
  const float qscale = scale * kLog2e;
#define DLION_KV8_EXTEND(DD, MM)                                                                                     \
  hipLaunchKernelGGL((kv8_extend_attn_kernel<DD, MM>), grid, dim3(256), 0, st, Q, k_codes, k_bs, k_ts, k_scales,      \
                     ks_bs, ks_ts, v_codes, v_bs, v_ts, v_scales, vs_bs, vs_ts, kv_len, n_new, part_m, part_l, part_o, \
                     static_cast<uint16_t*>(out), T, H, G, splits, Tmax, max_len, window, chunk, qscale)
  if (D == 128) {
    if (G <= 4) DLION_KV8_EXTEND(128, 1);
    else DLION_KV8_EXTEND(128, 2);
  } else {
    if (G <= 4) DLION_KV8_EXTEND(64, 1);
    else DLION_KV8_EXTEND(64, 2);
  }
#undef DLION_KV8_EXTEND
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || splits == 1) return e;
  return launch_chunk_combine(part_m, part_l, part_o, out, static_cast<int64_t>(B) * T * H, D, splits, st);
}

}  // namespace dlion
