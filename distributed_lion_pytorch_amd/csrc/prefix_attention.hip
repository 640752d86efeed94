// Generation: beam search on a shared prompt cache.  bf16, head_dim 64 / 128, G = H / Hkv in 1..8, nb beams per
// prompt with R = nb G <= 64.
//
// The nb beams of prompt b share one prefix cache row kp / vp [Bp, Tp, Hkv, D] (prefix_len[b] keys) and own one
// suffix cache row each, ks / vs [Bp nb, Ts, Hkv, D] (suffix_len[r] keys, the token just appended included).  Beam
// row r = b nb + j attends prefix keys [0, prefix_len[b]) and then its suffix keys [0, suffix_len[r]); under a window
// w the key at total position t is visible iff t >= prefix_len[b] + suffix_len[r] - w.  Both lengths are clamped to
// the host bounds (max_prefix, max_suffix) and the cache widths first, and every formula runs on the clamped values.
//
// kv_append_suffix.  decode.hip's kv_append with two positions per row: q and k are normalised (Qwen3, optional) and
// rotated at rot_pos[r] (the total position) by rope_norm.h's functions -- the bits of kv_append at that absolute
// position -- and k / v go to suffix cache[r, write_pos[r]].  A write position outside [0, Ts) raises kIndexErrCache
// and nothing is written to the caches; a rotation position outside the tables raises it too and is clamped.
//
// prefix_attn_kernel.  The prompt's keys are the long stream, and the beams of a prompt share them the way a GQA
// group shares a kv head: a block owns one (split, kv head, prompt), streams its chunk of the prompt's K / V from
// HBM once and uses every key for all R = nb G query rows (row j G + g = beam j, head g of the group; the q rows come
// from nb different batch rows of q).  The products run on v_mfma_f32_16x16x32_bf16 with the R rows as one tile
// dimension, padded to MT = ceil(R / 16) tiles (padded rows repeat row R - 1, are masked and never stored):
//
//   S^T = K Q^T.  K is the A operand: lane l holds key l & 15, dims 32 ks + 8 (l >> 4) .. + 7, eight contiguous
//   bf16 of one key -- a 16-byte global load straight into the operand registers, no LDS.  Q^T is the B operand
//   (query row l & 15, the same dims), loaded once per block; the scale goes onto the fp32 scores.  The result has
//   the query row on the lane and keys 4 (l >> 4) + r in its registers r = 0..3.  There is no causal mask inside the
//   tile (every prefix key precedes every beam's query); the window's lower edge depends on the row's own
//   suffix_len, so it is a per-lane bound klo[mt], and the block's key range starts at the lowest edge among its rows.
//
//   O^T = V^T P^T.  Two 16-key score tiles are the B operand of a k = 32 step as they stand.  P goes in as a bf16
//   high part plus the bf16 of the remainder (two MFMAs, 16 bits of P: no noisier than decode.hip's fp32 P at the
//   bf16 output).  The A operand needs V^T in that key order: V's 32 x D tile goes through LDS row-major (rows
//   D + 16 elements apart: the eight rows a 32-lane half reads start 8 banks apart, every address 8-byte aligned) and
//   comes back through ds_read_b64_tr_b16, one read per 16-key tile.  The accumulator has the query row on the lane,
//   so the online softmax's rescale is lane-local.
//
// A block is 4 waves; wave w takes the 32-key tiles w, w + 4, ... of the block's chunk and keeps its own running
// max / sum / output for all R rows: a wave stages, reads and overwrites only its own V tile, so the main loop has
// no block barrier.  At the end the waves' partials are merged through LDS (the V area, reused) in wave order, one
// 16-row tile at a time, and the block writes one fp32 partial (log2 domain) per real row.  Registers: Q^T is
// MT D / 8 VGPRs and O^T MT D / 4; MT >= 3 at D = 128 runs one block per CU, every other shape two.  LDS:
// 4 x 32 x (D + 16) bf16 + 128 floats = 20.5 KiB (D = 64) / 36.5 KiB (D = 128).
//
// suffix_attn_kernel.  One (split, kv head, beam row) attends that row's own suffix keys for its G heads: a few
// keys and G <= 8 rows, so it is decode.hip's VALU form (a key is D / 8 adjacent lanes, a head's score 8 FMAs and a
// DPP butterfly), written here so that decode.hip stays as it is.
//
// One partial buffer: part_m / part_l [Bp nb, H, S1 + S2], part_o [.., D]; prefix blocks write the slots [0, S1),
// suffix blocks [S1, S1 + S2); an empty range writes the neutral partial (max -inf, sum 0, output 0).  The combine
// pass (chunk_attention.hip's launch_chunk_combine) reduces the slots in index order.  No atomics anywhere: the same
// inputs give the same bits.  Nothing at or beyond either length is read: key indices are clamped into the block's
// own non-empty range before an address is formed, and clamped or masked scores are -inf.
#include "common.h"
#include "kernels.h"
#include "kv_append.h"
#include "rope_norm.h"

namespace dlion {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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
__device__ __forceinline__ int clamp_len(int len, int cap) {
  len = len < cap ? len : cap;
  return len > 0 ? len : 0;
}

// ------------------------------------------------------------------------------------------ suffix append
// grid: ceil(rows (H + 2 Hkv) / GROUPS) blocks of 256; kv_append_kernel's mapping (a lane group of D / 8 lanes owns
// one head row of one beam row: slots [0, H) are q, [H, H + Hkv) k, the rest v) with the table row rot[r] and the
// cache index wr[r] apart.  n_pos: the tables' rows.
template <int D, int MODE>
__global__ void __launch_bounds__(256) kv_append_suffix_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t q_ld,
    int64_t k_ld, int64_t v_ld, const int* __restrict__ rot, const int* __restrict__ wr,
    const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn, const uint16_t* __restrict__ gq,
    const uint16_t* __restrict__ gk, float eps, uint16_t* __restrict__ q_out, uint16_t* __restrict__ kc,
    uint16_t* __restrict__ vc, int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, int rows, int H, int Hkv,
    int Ts, int n_pos, int32_t* __restrict__ err) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int Hx = H + 2 * Hkv;
  const int64_t n_hr = static_cast<int64_t>(rows) * Hx;
  const int64_t hr = static_cast<int64_t>(blockIdx.x) * GROUPS + grp;
  const bool valid = hr < n_hr;
  const int64_t hrc = valid ? hr : n_hr - 1;
  const int b = static_cast<int>(hrc / Hx);
  const int slot = static_cast<int>(hrc - static_cast<int64_t>(b) * Hx);
  int p = MODE == kAppend ? 0 : rot[b];  // the table row
  int wp = wr[b];                        // the cache index
  const bool in_cache = wp >= 0 && wp < Ts;
  const bool in_table = MODE == kAppend || (p >= 0 && p < n_pos);
  if ((!in_cache || !in_table) && valid && sub == 0 && slot == 0) atomicOr(err, kIndexErrCache);
  wp = wp < 0 ? 0 : (wp >= Ts ? Ts - 1 : wp);
  p = p < 0 ? 0 : (p >= n_pos ? n_pos - 1 : p);
  const bool is_q = slot < H, is_v = slot >= H + Hkv;
  const bool store = valid && (is_q || in_cache);
  const uint16_t* src = is_q    ? q + b * q_ld + static_cast<int64_t>(slot) * D
                        : is_v  ? v + b * v_ld + static_cast<int64_t>(slot - H - Hkv) * D
                                : k + b * k_ld + static_cast<int64_t>(slot - H) * D;
  uint16_t* dst = is_q   ? q_out + (static_cast<int64_t>(b) * H + slot) * D
                  : is_v ? vc + b * vc_bs + wp * vc_ts + static_cast<int64_t>(slot - H - Hkv) * D
                         : kc + b * kc_bs + wp * kc_ts + static_cast<int64_t>(slot - H) * D;
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
      // qk_norm.hip's mapping; v rows run the same lanes (their result is dropped) so that no DPP move reads an
      // inactive lane
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

// ------------------------------------------------------------------------------------------ prefix blocks
// grid (S1, Hkv, Bp), 256 threads.  MT = ceil(nb G / 16) query tiles.  Prompt b's key range is [lo, plen), lo the
// lowest window edge among its beams; split s owns [lo + s chunk, lo + (s + 1) chunk) of it.  Partials: slot s of
// part_m / part_l [Bp nb, H, S], part_o [Bp nb, H, S, D].
// The second launch bound asks for two waves per SIMD (256 registers) wherever the tiles allow it.
template <int D, int MT>
__global__ void __launch_bounds__(256, (D == 64 || MT <= 2) ? 2 : 1) prefix_attn_kernel(
    const uint16_t* __restrict__ q, int64_t q_ld, const uint16_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const uint16_t* __restrict__ vc, int64_t v_bs, int64_t v_ts, const int* __restrict__ prefix_len,
    const int* __restrict__ suffix_len, float* __restrict__ part_m, float* __restrict__ part_l,
    float* __restrict__ part_o, int nb, int H, int G, int pcap, int scap, int window, int chunk, int S, float qscale) {
  constexpr int KS = D / 32, DT = D / 16, VS = D + 16;  // k steps of Q K^T, 16-dim tiles of O^T, V row stride
  constexpr int LPK = D / 8, KPP = 64 / LPK, NP = kTileKeys / KPP;  // V staging: lanes per key, keys per pass
  __shared__ __attribute__((aligned(16))) uint16_t vs_[kWaves * kTileKeys * VS];
  __shared__ float sm_m[kWaves][16], sm_l[kWaves][16];
  static_assert(sizeof(uint16_t) * kWaves * kTileKeys * VS >= sizeof(float) * kWaves * 16 * D, "merge area");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c = lane & 15, grp = lane >> 4;
  const int s = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int R = nb * G;
  const int plen = clamp_len(prefix_len[b], pcap);
  int lo = 0;
  if (window > 0) {  // the lowest window edge among the prompt's beams (block-uniform)
    int smin = scap;
    for (int j = 0; j < nb; ++j) {
      const int sl = clamp_len(suffix_len[b * nb + j], scap);
      smin = sl < smin ? sl : smin;
    }
    const int64_t e = static_cast<int64_t>(plen) + smin - window;
    lo = e > 0 ? (e < plen ? static_cast<int>(e) : plen) : 0;
  }
  // s chunk <= span + chunk: no overflow for any cache that fits in memory
  const int64_t start64 = static_cast<int64_t>(lo) + static_cast<int64_t>(s) * chunk;
  const int start = start64 < plen ? static_cast<int>(start64) : plen;
  const int end = (plen - start) > chunk ? start + chunk : plen;
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

  const int first = start + wave * kTileKeys;  // the wave's first tile
  if (first < end) {                           // wave-uniform
    bf16x8 qf[MT][KS];
    int klo[MT], khi[MT];  // the lane's query row sees the keys [klo, khi) of this block
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = 16 * mt + c;
      const int rc = row < R ? row : R - 1;
      const int j = rc / G, g = rc - j * G;
      const int r = b * nb + j;
      int wlo = 0;
      if (window > 0) {
        const int64_t e = static_cast<int64_t>(plen) + clamp_len(suffix_len[r], scap) - window;
        wlo = e > 0 ? (e < plen ? static_cast<int>(e) : plen) : 0;
      }
      klo[mt] = wlo > start ? wlo : start;
      khi[mt] = row < R ? end : 0;
      const uint16_t* qp = q + r * q_ld + static_cast<int64_t>(h0 + g) * D + 8 * grp;
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
        const int64_t jc = j < end ? j : end - 1;  // a key of this block's own range: below prefix_len
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[kt][ks] = ld_frag(kbase + jc * k_ts + 32 * ks);
      }
      uint4 vr[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int j = j0 + p * KPP + lane / LPK;
        const int64_t jc = j < end ? j : end - 1;
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
        const float ms = mn == kNegInf ? 0.f : mn;  // a row that has seen no key yet
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
  float* so = reinterpret_cast<float*>(vs_);  // [wave][query row][D]
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
        const int j = row / G, g = row - j * G;
        const int64_t pi = ((static_cast<int64_t>(b) * nb + j) * H + h0 + g) * S + s;
        part_o[pi * D + d] = O;
        if (d == 0) {
          part_m[pi] = M;
          part_l[pi] = L;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ suffix blocks
// keys in flight per lane group and iteration: 4 (2 at the widest group, whose q and outputs fill the registers)
template <int GP>
struct Unroll {
  static constexpr int value = GP == 8 ? 2 : 4;
};

// grid (S2, Hkv, Bp nb), 256 threads; decode_attn_kernel's form over row r's own suffix keys [lo, slen), lo = the
// window's lower edge max(0, slen - window).  GP = G rounded up to 1 / 2 / 4 / 8 (heads past G repeat head G - 1
// and are not stored).  Partials: slot S1 + s of the buffers above.
template <int D, int GP>
__global__ void __launch_bounds__(256) suffix_attn_kernel(
    const uint16_t* __restrict__ q, int64_t q_ld, const uint16_t* __restrict__ kc, int64_t k_bs, int64_t k_ts,
    const uint16_t* __restrict__ vc, int64_t v_bs, int64_t v_ts, const int* __restrict__ suffix_len,
    float* __restrict__ part_m, float* __restrict__ part_l, float* __restrict__ part_o, int H, int G, int scap,
    int window, int chunk, int S1, int S, float qscale) {
  constexpr int LANES = D / 8, KG = 256 / LANES, U = Unroll<GP>::value;
  __shared__ float sm_o[KG * D];
  __shared__ float sm_m[KG], sm_l[KG];
  const int sub = threadIdx.x % LANES, kg = threadIdx.x / LANES;
  const int d0 = sub * 8;
  const int s = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int len = clamp_len(suffix_len[b], scap);
  const int lo = (window > 0 && len > window) ? len - window : 0;
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
        const int64_t jc = ok[u] ? j : end - 1;  // a key of this block's own range: always below suffix_len
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
        const int64_t pi = (static_cast<int64_t>(b) * H + h0 + g) * S + S1 + s;
        part_o[pi * D + threadIdx.x] = O;
        if (threadIdx.x == 0) {
          part_m[pi] = M;
          part_l[pi] = L;
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_kv_append_suffix(const void* q, const void* k, const void* v, int64_t q_ld, int64_t k_ld,
                                   int64_t v_ld, const int* rot_pos, const int* write_pos, const void* cos,
                                   const void* sin, int n_pos, const void* q_gamma, const void* k_gamma, float eps,
                                   void* q_out, void* k_cache, void* v_cache, int64_t kc_bs, int64_t kc_ts,
                                   int64_t vc_bs, int64_t vc_ts, int rows, int H, int Hkv, int D, int Ts,
                                   int32_t* err, hipStream_t st) {
  if (rows <= 0 || H <= 0 || Hkv <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Ts <= 0 || err == nullptr || write_pos == nullptr) return hipErrorInvalidValue;
  if ((cos == nullptr) != (sin == nullptr) || (q_gamma == nullptr) != (k_gamma == nullptr)) return hipErrorInvalidValue;
  if (q_gamma != nullptr && cos == nullptr) return hipErrorInvalidValue;
  if (cos != nullptr && (rot_pos == nullptr || n_pos <= 0)) return hipErrorInvalidValue;
  const int groups = 256 / (D / 8);
  const int64_t n_hr = static_cast<int64_t>(rows) * (H + 2 * Hkv);
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
  const int np = cos != nullptr ? n_pos : 1;
#define DLION_APPEND_SUFFIX(DD, MODE)                                                                                \
  hipLaunchKernelGGL((kv_append_suffix_kernel<DD, MODE>), grid, dim3(256), 0, st, Q, K, V, q_ld, k_ld, v_ld, rot_pos, \
                     write_pos, C, S, GQ, GK, eps, QO, KC, VC, kc_bs, kc_ts, vc_bs, vc_ts, rows, H, Hkv, Ts, np, err)
  const int mode = q_gamma != nullptr ? kNormRope : (cos != nullptr ? kRope : kAppend);
  if (D == 128) {
    if (mode == kNormRope) DLION_APPEND_SUFFIX(128, kNormRope);
    else if (mode == kRope) DLION_APPEND_SUFFIX(128, kRope);
    else DLION_APPEND_SUFFIX(128, kAppend);
  } else {
    if (mode == kNormRope) DLION_APPEND_SUFFIX(64, kNormRope);
    else if (mode == kRope) DLION_APPEND_SUFFIX(64, kRope);
    else DLION_APPEND_SUFFIX(64, kAppend);
  }
#undef DLION_APPEND_SUFFIX
  return hipGetLastError();
}

hipError_t launch_shared_prefix_attention(const void* q, int64_t q_ld, const void* k_prefix, int64_t kp_bs,
                                          int64_t kp_ts, const void* v_prefix, int64_t vp_bs, int64_t vp_ts,
                                          const int* prefix_len, const void* k_suffix, int64_t ks_bs, int64_t ks_ts,
                                          const void* v_suffix, int64_t vs_bs, int64_t vs_ts, const int* suffix_len,
                                          float* part_m, float* part_l, float* part_o, void* out, int Bp, int nb,
                                          int H, int Hkv, int D, int Tp, int Ts, int max_prefix, int max_suffix,
                                          int window, int splits1, int chunk1, int splits2, int chunk2, float scale,
                                          hipStream_t st) {
  if (Bp <= 0 || nb <= 0 || H <= 0) return hipSuccess;
  if ((D != 64 && D != 128) || Hkv <= 0 || H % Hkv != 0 || H / Hkv > 8) return hipErrorInvalidValue;
  const int G = H / Hkv;
  if (static_cast<int64_t>(nb) * G > kPrefixMaxRows) return hipErrorInvalidValue;
  if (Tp <= 0 || Ts <= 0 || max_prefix <= 0 || max_suffix <= 0 || window < 0) return hipErrorInvalidValue;
  if (splits1 < 1 || splits1 > kDecodeMaxSplits || chunk1 < 1 || splits2 < 1 || splits2 > kDecodeMaxSplits || chunk2 < 1)
    return hipErrorInvalidValue;
  const int64_t rows = static_cast<int64_t>(Bp) * nb;
  if (rows > 65535 || Hkv > 65535) return hipErrorInvalidValue;
  const int pcap = max_prefix < Tp ? max_prefix : Tp, scap = max_suffix < Ts ? max_suffix : Ts;
  // every key has a split: a prompt's range spans at most min(window, pcap), a row's suffix range min(window, scap)
  const int span1 = (window > 0 && window < pcap) ? window : pcap;
  const int span2 = (window > 0 && window < scap) ? window : scap;
  if (static_cast<int64_t>(splits1) * chunk1 < span1 || static_cast<int64_t>(splits2) * chunk2 < span2)
    return hipErrorInvalidValue;
  const int S = splits1 + splits2;
  const int MT = (nb * G + 15) / 16;
  auto* Q = static_cast<const uint16_t*>(q);
  auto* KP = static_cast<const uint16_t*>(k_prefix);
  auto* VP = static_cast<const uint16_t*>(v_prefix);
  auto* KS = static_cast<const uint16_t*>(k_suffix);
  auto* VS = static_cast<const uint16_t*>(v_suffix);
  const float qscale = scale * kLog2e;
  const dim3 grid1(static_cast<unsigned>(splits1), static_cast<unsigned>(Hkv), static_cast<unsigned>(Bp));
#define DLION_PREFIX(DD, MM)                                                                                       \
  hipLaunchKernelGGL((prefix_attn_kernel<DD, MM>), grid1, dim3(256), 0, st, Q, q_ld, KP, kp_bs, kp_ts, VP, vp_bs,   \
                     vp_ts, prefix_len, suffix_len, part_m, part_l, part_o, nb, H, G, pcap, scap, window, chunk1, S, \
                     qscale)
#define DLION_PREFIX_D(DD)               \
  if (MT == 1) DLION_PREFIX(DD, 1);      \
  else if (MT == 2) DLION_PREFIX(DD, 2); \
  else if (MT == 3) DLION_PREFIX(DD, 3); \
  else DLION_PREFIX(DD, 4)
  if (D == 128) {
    DLION_PREFIX_D(128);
  } else {
    DLION_PREFIX_D(64);
  }
#undef DLION_PREFIX_D
#undef DLION_PREFIX
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid2(static_cast<unsigned>(splits2), static_cast<unsigned>(Hkv), static_cast<unsigned>(rows));
#define DLION_SUFFIX(DD, GP)                                                                                      \
  hipLaunchKernelGGL((suffix_attn_kernel<DD, GP>), grid2, dim3(256), 0, st, Q, q_ld, KS, ks_bs, ks_ts, VS, vs_bs, \
                     vs_ts, suffix_len, part_m, part_l, part_o, H, G, scap, window, chunk2, splits1, S, qscale)
#define DLION_SUFFIX_D(DD)              \
  if (G == 1) DLION_SUFFIX(DD, 1);      \
  else if (G == 2) DLION_SUFFIX(DD, 2); \
  else if (G <= 4) DLION_SUFFIX(DD, 4); \
  else DLION_SUFFIX(DD, 8)
  if (D == 128) {
    DLION_SUFFIX_D(128);
  } else {
    DLION_SUFFIX_D(64);
  }
#undef DLION_SUFFIX_D
#undef DLION_SUFFIX
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_chunk_combine(part_m, part_l, part_o, out, rows * H, D, S, st);
}

}  // namespace dlion
