// Generation on an fp8 KV cache: codes uint8 [B, Tmax, Hkv, D] (OCP e4m3fn) and scales fp32 [B, Tmax, Hkv], one
// power of two per (token, kv head); kv8.h has the format and the one quantiser every writer shares.
//
// The fp8 stores of kv_append / kv_append_chunk are instantiated here from kv_append.h's templates.
//
// kv_quantize.  The prefill's writer: bf16 head rows [B, T, Hkv, D] (a strided view of the fused q|k|v output or
// the rotated k) -> codes[:, :T] and scales[:, :T].  A head row is D / 8 adjacent lanes (kv_append's mapping):
// one 16-byte load, a DPP maximum, one 8-byte store per lane and one scale store per row.
//
// cached_attention_fp8.  T = 1..8 queries per row against the fp8 cache: the decode step and the speculative
// chunk in one kernel.  The grid, the split rule, the fp32 partials and the combine pass in index order are
// chunk_attention.hip's (a block owns one (split, kv head, row) by a host rule over host values; no atomics),
// and so is the arithmetic after dequantisation: S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16 with
// the R = T G query rows padded to MT 16-row tiles, P fed as a bf16 high part and the bf16 of the remainder.
// An e4m3 value is exact in bf16, so the operands carry the codes themselves; the scales, powers of two, fold
// in exactly where one multiply per (key, query) does it: the key's into its fp32 score (together with
// log2(e) / sqrt(D)), the value's into P before the high / low split.  What differs from the bf16 kernel:
//
//   A wave's tile is 64 keys (at absolute multiples of 64; wave w of the four takes tiles w, w + 4, ...), twice
//   the bf16 kernel's: at one byte per element the same number of 16-byte loads per lane (4 + 4 at D = 64,
//   8 + 8 at D = 128) keeps the same bytes in flight, and the online softmax rescales once per 64 keys.
//
//   K, global memory -> A operand.  The MFMA sums over its k index, so which dims a lane holds is free as long
//   as Q^T holds the same: lane (key c = l & 15, group g = l >> 4) loads the 16 codes of dims 64 h + 16 g ..
//   + 15 in one 16-byte load; their low 8 are its fragment of k step 2 h, the high 8 of step 2 h + 1, and the
//   query fragments are loaded once per block at those dims.  Eight codes become eight bf16 by four
//   v_cvt_pk_f32_fp8 and four packs of the high halves.
//
//   V, global memory -> LDS -> A operand.  A lane loads 16 codes of one key (D / 16 lanes per key), converts
//   them and stores 32 bytes of bf16 row-major; ds_read_b64_tr_b16 brings V^T back as in the bf16 kernel
//   (rows D + 16 elements apart, 16-byte aligned).  The tile's two 32-key halves go through the wave's area one
//   after the other, so the LDS footprint is the bf16 kernel's.  So is the LDS traffic, not half of it: the
//   8-bit transposed read would halve it, and the loop is bound by global loads and VALU, not LDS.
//
//   Scales.  Lane l loads the key and the value scale of key l of the tile; they go through a 64-float LDS row
//   per wave and come back four at a time (a lane's score registers are the keys 16 kt + 4 g .. + 3).
//
// Nothing at or beyond kv_len[b] + n_new[b] is read, neither a code nor a scale: key indices are clamped into
// the block's own non-empty range before an address is formed and clamped or masked scores are -inf (P = 0
// times a finite in-range value and scale).  Queries t >= n_new[b] give neutral partials and a zero row.
#include "common.h"
#include "kernels.h"
#include "kv8.h"
#include "kv_append.h"

namespace dlion {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------ kv_quantize
// grid: ceil(B T Hkv / GROUPS) blocks of 256; head rows past the end are clamped (computed again, never stored)
// so that the lanes a DPP move reads are always active
template <int D>
__global__ void __launch_bounds__(256) kv_quantize_kernel(const uint16_t* __restrict__ x, int64_t x_bs, int64_t x_ts,
                                                          uint8_t* __restrict__ codes, int64_t c_bs, int64_t c_ts,
                                                          float* __restrict__ scales, int64_t s_bs, int64_t s_ts,
                                                          int B, int T, int Hkv) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int64_t n_hr = static_cast<int64_t>(B) * T * Hkv;
  const int64_t hr = static_cast<int64_t>(blockIdx.x) * GROUPS + grp;
  const bool valid = hr < n_hr;
  const int64_t hrc = valid ? hr : n_hr - 1;
  const int64_t bt = hrc / Hkv;
  const int h = static_cast<int>(hrc - bt * Hkv);
  const int64_t b = bt / T, t = bt - b * T;
  float v[8], scale;
  Elem<kBF16>::load8(x + b * x_bs + t * x_ts + static_cast<int64_t>(h) * D + sub * 8, v);
  const uint2 c = kv8_quantize_row<LANES>(v, scale);
  if (valid) {
    *reinterpret_cast<uint2*>(codes + b * c_bs + t * c_ts + static_cast<int64_t>(h) * D + sub * 8) = c;
    if (sub == 0) scales[b * s_bs + t * s_ts + h] = scale;
  }
}

// --------------------------------------------------------------------------------- cached attention, fp8
constexpr float kNegInf = -__builtin_huge_valf();
constexpr int kWaves = 4, kTile = 64, kHalf = 32;

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld_frag(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p));
}
__device__ __forceinline__ bf16x8 codes_frag(uint32_t lo, uint32_t hi) {
  const uint2 a = kv8_codes_to_bf16(lo), b = kv8_codes_to_bf16(hi);
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
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

// grid (splits, Hkv, B), 256 threads.  MT = ceil(T G / 16) query tiles.  q [B, T, H, D] contiguous bf16.  Row
// b's key range is [lo, len + n), lo = the window's lower edge of query 0; split s owns [lo + s chunk, lo +
// (s + 1) chunk) of it.  Partials: part_m / part_l [B, T, H, S], part_o [B, T, H, S, D].
// The second launch bound asks for two waves per SIMD (256 registers) wherever the tiles allow it: with a 64-key
// tile's raw K and V in registers beside Q^T, O^T, the scores and P, D = 128 fits them at one query tile only
// (MT = 2 spilled 5 to 54 registers in every arrangement tried) and runs one block per CU from MT = 2 on.
template <int D, int MT>
__global__ void __launch_bounds__(256, (D == 64 || MT <= 1) ? 2 : 1) kv8_attn_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const float* __restrict__ ksc, int64_t ks_bs, int64_t ks_ts, const uint8_t* __restrict__ vc, int64_t v_bs,
    int64_t v_ts, const float* __restrict__ vsc, int64_t vs_bs, int64_t vs_ts, const int* __restrict__ kv_len,
    const int* __restrict__ n_new, float* __restrict__ part_m, float* __restrict__ part_l,
    float* __restrict__ part_o, int T, int H, int G, int Tmax, int max_len, int window, int chunk, float qscale) {
  constexpr int KH = D / 64, KS = D / 32, DT = D / 16, VS = D + 16;  // 16-byte K loads per key, k steps, O^T tiles, V row stride
  constexpr int LPK = D / 16, KPP = 64 / LPK, NP = kTile / KPP;     // V staging: lanes per key, keys per pass, passes
  constexpr int KT = kTile / 16;                                    // 16-key score tiles
  __shared__ __attribute__((aligned(16))) uint16_t vs_[kWaves * kHalf * VS];
  __shared__ __attribute__((aligned(16))) float sc_k[kWaves][kTile], sc_v[kWaves][kTile];
  __shared__ float sm_m[kWaves][16], sm_l[kWaves][16];
  static_assert(sizeof(uint16_t) * kWaves * kHalf * VS >= sizeof(float) * kWaves * 16 * D, "merge area");
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

  // tile i (keys [64 i, 64 i + 64)) belongs to wave i & 3; keys below `start` in the first tile are masked like
  // those at and beyond `end`: with one split a query's arithmetic depends on its own key range alone
  const int tile0 = start / kTile;
  const int first = (tile0 + ((wave - tile0) & (kWaves - 1))) * kTile;  // the wave's first tile, >= start - 63
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
      const uint16_t* qp = q + ((static_cast<int64_t>(b) * T + t) * H + h0 + g) * D + 16 * grp;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[mt][ks] = ld_frag(qp + 64 * (ks >> 1) + 8 * (ks & 1));
    }
    const uint8_t* kbase = kc + b * k_bs + static_cast<int64_t>(hk) * D + 16 * grp;
    const uint8_t* vbase = vc + b * v_bs + static_cast<int64_t>(hk) * D + 16 * (lane % LPK);
    const float* ksbase = ksc + b * ks_bs + hk;
    const float* vsbase = vsc + b * vs_bs + hk;
    uint16_t* vw = vs_ + wave * (kHalf * VS);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

    for (int j0 = first; j0 < end; j0 += kTile * kWaves) {  // wave-uniform
      uint4 kr[KT][KH], vr[NP];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int j = j0 + 16 * kt + c;
        // a key of this block's own range: below kv_len + n_new
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
#pragma unroll
        for (int h = 0; h < KH; ++h) kr[kt][h] = *reinterpret_cast<const uint4*>(kbase + jc * k_ts + 64 * h);
      }
      auto load_v = [&](int p0, int p1) {
#pragma unroll
        for (int p = p0; p < p1; ++p) {
          const int j = j0 + p * KPP + lane / LPK;
          const int64_t jc = j < start ? start : (j < end ? j : end - 1);
          vr[p] = *reinterpret_cast<const uint4*>(vbase + jc * v_ts);
        }
      };
      load_v(0, NP);
      {
        const int j = j0 + lane;
        const int64_t jc = j < start ? start : (j < end ? j : end - 1);
        sc_k[wave][lane] = ksbase[jc * ks_ts] * qscale;
        sc_v[wave][lane] = vsbase[jc * vs_ts];
      }
      // a 32-key half of V, converted, into the wave's LDS area (the first one here: its raw registers are free
      // before the scores need theirs)
      auto stage = [&](int hf) {
#pragma unroll
        for (int p = 0; p < NP / 2; ++p) {
          const uint4 raw = vr[hf * (NP / 2) + p];
          const uint2 a = kv8_codes_to_bf16(raw.x), bq = kv8_codes_to_bf16(raw.y);
          const uint2 cq = kv8_codes_to_bf16(raw.z), dq = kv8_codes_to_bf16(raw.w);
          uint16_t* dst = vw + (p * KPP + lane / LPK) * VS + 16 * (lane % LPK);
          *reinterpret_cast<uint4*>(dst) = make_uint4(a.x, a.y, bq.x, bq.y);
          *reinterpret_cast<uint4*>(dst + 8) = make_uint4(cq.x, cq.y, dq.x, dq.y);
        }
        __builtin_amdgcn_wave_barrier();  // the stores above and the reads that follow are this wave's own, in order
      };
      stage(0);

      // S^T: the 16-key tiles one after the other, a tile's K fragments converted once for all query tiles
      f32x4 sc[MT][KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        bf16x8 kf[KS];
#pragma unroll
        for (int h = 0; h < KH; ++h) {
          kf[2 * h] = codes_frag(kr[kt][h].x, kr[kt][h].y);
          kf[2 * h + 1] = codes_frag(kr[kt][h].z, kr[kt][h].w);
        }
        const float4 kq = *reinterpret_cast<const float4*>(&sc_k[wave][16 * kt + 4 * grp]);
        const float kqs[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = mfma16(kf[ks], qf[mt][ks], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = j0 + 16 * kt + 4 * grp + r;
            acc[r] = (j >= klo[mt] && j < khi[mt]) ? acc[r] * kqs[r] : kNegInf;
          }
          sc[mt][kt] = acc;
        }
      }

      bf16x8 pf[MT][2], pl[MT][2];  // P (times the value scale) as bf16 high and low parts, per 32-key half
      float alpha[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        float mx = kNegInf;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[mt][kt][r]);
        mx = groups_max(mx);
        const float mn = fmaxf(m[mt], mx);
        const float ms = mn == kNegInf ? 0.f : mn;  // a query that has seen no key yet
        alpha[mt] = __builtin_amdgcn_exp2f(m[mt] - ms);
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          const float4 vq = *reinterpret_cast<const float4*>(&sc_v[wave][16 * kt + 4 * grp]);
          const float vsq[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(sc[mt][kt][r] - ms);
            ps += e;
            const float ev = e * vsq[r];
            const __bf16 eh = static_cast<__bf16>(ev);
            pf[mt][kt >> 1][4 * (kt & 1) + r] = eh;
            pl[mt][kt >> 1][4 * (kt & 1) + r] = static_cast<__bf16>(ev - static_cast<float>(eh));
          }
        }
        l[mt] = __builtin_fmaf(l[mt], alpha[mt], ps);  // the lane's share of the sum; the groups are added at the end
        m[mt] = mn;
      }
      // O^T: the tile's two 32-key halves go through the wave's LDS area one after the other
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        if (hf == 1) stage(1);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          // V^T fragment: rows = keys 16 kt + 4 grp .. + 3 of the half, columns 16 dt .. 16 dt + 15; lane 4 q + p
          // of a group addresses row q, columns 4 p .. 4 p + 3 and receives column (lane & 15) of the four rows
          const uint16_t* vp = vw + (4 * grp + (c >> 2)) * VS + 16 * dt + 4 * (c & 3);
          const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp));
          const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp + 16 * VS));
          const i32x2 a0 = __builtin_bit_cast(i32x2, v0), a1 = __builtin_bit_cast(i32x2, v1);
          const i32x4 av = {a0[0], a0[1], a1[0], a1[1]};
          const bf16x8 vf = __builtin_bit_cast(bf16x8, av);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            if (hf == 0) {
#pragma unroll
              for (int r = 0; r < 4; ++r) o[mt][dt][r] *= alpha[mt];
            }
            o[mt][dt] = mfma16(vf, pl[mt][hf], mfma16(vf, pf[mt][hf], o[mt][dt]));
          }
        }
        __builtin_amdgcn_wave_barrier();  // the next half's stores come after these reads
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

// grid B T H blocks of D threads: the splits of a row (b, t, h) in index order; a query without keys is zero
template <int D>
__global__ void __launch_bounds__(D) kv8_combine_kernel(const float* __restrict__ part_m,
                                                       const float* __restrict__ part_l,
                                                       const float* __restrict__ part_o, uint16_t* __restrict__ out,
                                                       int S) {
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

hipError_t launch_kv_quantize(const void* x, int64_t x_bs, int64_t x_ts, uint8_t* codes, int64_t c_bs, int64_t c_ts,
                              float* scales, int64_t s_bs, int64_t s_ts, int B, int T, int Hkv, int D,
                              hipStream_t st) {
  if (B <= 0 || T <= 0 || Hkv <= 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  const int groups = 256 / (D / 8);
  const int64_t n_hr = static_cast<int64_t>(B) * T * Hkv;
  if ((n_hr + groups - 1) / groups > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((n_hr + groups - 1) / groups));
  auto* X = static_cast<const uint16_t*>(x);
  if (D == 128)
    hipLaunchKernelGGL(kv_quantize_kernel<128>, grid, dim3(256), 0, st, X, x_bs, x_ts, codes, c_bs, c_ts, scales, s_bs,
                       s_ts, B, T, Hkv);
  else
    hipLaunchKernelGGL(kv_quantize_kernel<64>, grid, dim3(256), 0, st, X, x_bs, x_ts, codes, c_bs, c_ts, scales, s_bs,
                       s_ts, B, T, Hkv);
  return hipGetLastError();
}

hipError_t launch_kv_append_fp8(const void* q, const void* k, const void* v, int64_t q_ld, int64_t k_ld, int64_t v_ld,
                                const int* pos, const void* cos, const void* sin, const void* q_gamma,
                                const void* k_gamma, float eps, void* q_out, uint8_t* k_codes, uint8_t* v_codes,
                                int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, float* k_scales,
                                float* v_scales, int64_t sc_bs, int64_t sc_ts, int B, int H, int Hkv, int D, int Tmax,
                                int32_t* err, hipStream_t st) {
  if (k_scales == nullptr || v_scales == nullptr) return hipErrorInvalidValue;
  return kv_append_any<true>(q, k, v, q_ld, k_ld, v_ld, pos, cos, sin, q_gamma, k_gamma, eps, q_out, k_codes, v_codes,
                             kc_bs, kc_ts, vc_bs, vc_ts, k_scales, v_scales, sc_bs, sc_ts, B, H, Hkv, D, Tmax, err, st);
}

hipError_t launch_kv_append_chunk_fp8(const void* q, const void* k, const void* v, int64_t q_bs, int64_t q_ts,
                                      int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* pos,
                                      const int* n_new, const void* cos, const void* sin, const void* q_gamma,
                                      const void* k_gamma, float eps, void* q_out, uint8_t* k_codes, uint8_t* v_codes,
                                      int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, float* k_scales,
                                      float* v_scales, int64_t sc_bs, int64_t sc_ts, int B, int T, int H, int Hkv,
                                      int D, int Tmax, int32_t* err, hipStream_t st) {
  if (k_scales == nullptr || v_scales == nullptr) return hipErrorInvalidValue;
  return kv_append_chunk_any<true>(q, k, v, q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, pos, n_new, cos, sin, q_gamma, k_gamma,
                                   eps, q_out, k_codes, v_codes, kc_bs, kc_ts, vc_bs, vc_ts, k_scales, v_scales, sc_bs,
                                   sc_ts, B, T, H, Hkv, D, Tmax, err, st);
}

hipError_t launch_cached_attention_fp8(const void* q, const uint8_t* k_codes, int64_t k_bs, int64_t k_ts,
                                       const float* k_scales, int64_t ks_bs, int64_t ks_ts, const uint8_t* v_codes,
                                       int64_t v_bs, int64_t v_ts, const float* v_scales, int64_t vs_bs, int64_t vs_ts,
                                       const int* kv_len, const int* n_new, float* part_m, float* part_l,
                                       float* part_o, void* out, int B, int T, int H, int Hkv, int D, int Tmax,
                                       int max_len, int window, int splits, int chunk, float scale, hipStream_t st) {
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
  const float qscale = scale * kLog2e;
#define DLION_KV8(DD, MM)                                                                                          \
  hipLaunchKernelGGL((kv8_attn_kernel<DD, MM>), grid, dim3(256), 0, st, Q, k_codes, k_bs, k_ts, k_scales, ks_bs,    \
                     ks_ts, v_codes, v_bs, v_ts, v_scales, vs_bs, vs_ts, kv_len, n_new, part_m, part_l, part_o, T, H, \
                     G, Tmax, max_len, window, chunk, qscale)
#define DLION_KV8_D(DD)                \
  if (MT == 1) DLION_KV8(DD, 1);       \
  else if (MT == 2) DLION_KV8(DD, 2);  \
  else if (MT == 3) DLION_KV8(DD, 3);  \
  else DLION_KV8(DD, 4)
  if (D == 128) {
    DLION_KV8_D(128);
  } else {
    DLION_KV8_D(64);
  }
#undef DLION_KV8_D
#undef DLION_KV8
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 cgrid(static_cast<unsigned>(B * T * H));
  if (D == 128)
    hipLaunchKernelGGL(kv8_combine_kernel<128>, cgrid, dim3(128), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  else
    hipLaunchKernelGGL(kv8_combine_kernel<64>, cgrid, dim3(64), 0, st, part_m, part_l, part_o,
                       static_cast<uint16_t*>(out), splits);
  return hipGetLastError();
}

}  // namespace dlion
