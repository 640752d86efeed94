// LoRA adapter path for the wide ranks r in {32, 64, 128}: the same three ops
// and the same arithmetic as lora.hip (out = o + s * (drop(x) A^T) B^T), with
// the rank dimension on the matrix cores instead of in registers -- lora.hip's
// acc[R][8] / bp[8][R/2] forms are at 256 VGPRs at r = 16.  Every product is
// v_mfma_f32_16x16x32_bf16 (A: lane l holds row l & 15, k = 8 (l >> 4) + e;
// B: column l & 15, the same k; D: column l & 15, rows 4 (l >> 4) + q):
//
//   rows   u^T tile  = W (A, r/16 row tiles) . x^T (B, 16 tokens): the scheme
//          of lora_rows_kernel with r/16 accumulators sharing one x fragment.
//   up     (u B^T)^T = b (A, rows = columns n) . u^T (B, tokens), contracting
//          over r; both fragments are 16-byte global loads.  The MFMA row m of
//          column tile nt stands for column 16 (m >> 2) + 4 nt + (m & 3) of
//          the wave's 64, so a lane ends up with 16 consecutive columns of one
//          token: o and out move in 16-byte pieces.
//   cols   dB / dA contract over tokens and both operands are token-major, so
//          a 32-token step of g [32][128] and y [32][r] is staged in LDS and
//          the fragments are read transposed (ds_read_b64_tr_b16, 4 token rows
//          x 16 columns per 16-lane group): D = y^T (A, rows = rank) . g (B,
//          columns = n).  Mode 1 stages the masked x (kept elements as they
//          are, dropped ones +0) and applies inv_keep once to the fp32 sum;
//          its dx = a^T (A, rows = n, read transposed from an [r][128] image
//          of a, once per block) . du^T (B, tokens, row reads of the y image)
//          uses the column permutation of `up` with 8 columns per lane.
//
// All 256 threads of a cols block run every transposed read (EXEC all ones):
// tail rows and tail columns are staged as zeros from clamped addresses and
// their results are discarded at the stores.
#include "common.h"

namespace dlion {

typedef __bf16 lw_bf16x8 __attribute__((ext_vector_type(8)));
typedef float lw_f32x4 __attribute__((ext_vector_type(4)));
typedef short lw_s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ lw_f32x4 lw_mfma(const uint4& a, const uint4& b, const lw_f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lw_bf16x8, a), __builtin_bit_cast(lw_bf16x8, b), c, 0,
                                                 0, 0);
}

// ------------------------------------------------------------------ rows
// out[t, j] = scale * sum_k in'[t, k] * w[j, k]; lora_rows_kernel with RT = R / 16
// row tiles of W per k-step and NB k-steps of loads in flight (4 + 4 RT VGPRs a
// step: 8 / 4 / 4 steps at r = 32 / 64 / 128 keep the kernel clear of scratch).
template <int R, bool DROP>
__global__ void __launch_bounds__(512) lora_wrows_kernel(const uint16_t* __restrict__ in, int64_t ldin,
                                                         const uint16_t* __restrict__ w, uint16_t* __restrict__ out,
                                                         int64_t rows, int K, float scale, uint32_t seed,
                                                         uint32_t thresh16, float inv_keep) {
  constexpr int NW = 8, RT = R / 16, NB = R == 32 ? 8 : 4;
  __shared__ lw_f32x4 red[NW][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 15, grp = lane >> 4;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * 16;
  const int64_t row = row0 + j;
  const bool rok = row < rows;
  const uint16_t* xr = in + (rok ? row : rows - 1) * ldin + grp * 8;
  const uint16_t* wr = w + static_cast<int64_t>(j) * K + grp * 8;
  const int steps = K / 32;
  lw_f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = lw_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = wv; s0 < steps; s0 += NW * NB) {
    uint4 xv[NB], wf[NB][RT];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int st = s0 + b * NW;
      const int sc = st < steps ? st : steps - 1;  // clamped: a step past the end is loaded and not used
      xv[b] = *reinterpret_cast<const uint4*>(xr + sc * 32);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) wf[b][rt] = *reinterpret_cast<const uint4*>(wr + static_cast<int64_t>(rt) * 16 * K + sc * 32);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int st = s0 + b * NW;
      if (st < steps) {  // wave-uniform
        uint4 xx = rok ? xv[b] : make_uint4(0u, 0u, 0u, 0u);
        if constexpr (DROP) {
          const uint32_t kp = keep8(seed, static_cast<uint64_t>(row) * K + st * 32 + grp * 8, thresh16);
          float f[8];
          Elem<kBF16>::load8(reinterpret_cast<const uint16_t*>(&xx), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = ((kp >> e) & 1u) ? f[e] * inv_keep : 0.f;
          Elem<kBF16>::store8(reinterpret_cast<uint16_t*>(&xx), f);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = lw_mfma(wf[b][rt], xx, acc[rt]);
      }
    }
  }
  // acc[rt][q] = partial out[row0 + (lane & 15)][16 rt + (lane >> 4) * 4 + q]; one rank tile at a time through LDS
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    red[wv][lane] = acc[rt];
    __syncthreads();
    if (threadIdx.x < 256) {
      const int l = threadIdx.x >> 2, q = threadIdx.x & 3;
      float sum = 0.f;
#pragma unroll
      for (int v = 0; v < NW; ++v) sum += red[v][l][q];
      const int tok = l & 15, r = rt * 16 + (l >> 4) * 4 + q;
      if (row0 + tok < rows) out[(row0 + tok) * R + r] = f32_to_bf16(sum * scale);
    }
    __syncthreads();
  }
}

// -------------------------------------------------------------------- up
// out[t, n] = o[t, n] + bf16(s * sum_j u[t, j] * b[n, j]).  A wave owns 64 columns
// (its b fragments stay in registers: R / 2 VGPRs) over `tiles` 16-token tiles,
// two tiles of loads at a time; the 4 waves of a block take 256 adjacent columns.
template <int R>
__global__ void __launch_bounds__(256) lora_wup_kernel(const uint16_t* __restrict__ o, int64_t ldo,
                                                       const uint16_t* __restrict__ u, const uint16_t* __restrict__ b,
                                                       uint16_t* __restrict__ out, int64_t rows, int N, int cblocks,
                                                       int tiles, float s) {
  constexpr int KS = R / 32;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tok = lane & 15, grp = lane >> 4;
  const int cb = blockIdx.x % cblocks;
  const int64_t tile0 = static_cast<int64_t>(blockIdx.x / cblocks) * tiles;
  const int wc0 = cb * 256 + wv * 64;
  uint4 bfr[4][KS];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = wc0 + (tok >> 2) * 16 + nt * 4 + (tok & 3);  // the column MFMA row `tok` of tile nt stands for
    const uint16_t* br = b + static_cast<int64_t>(col < N ? col : 0) * R + grp * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bfr[nt][ks] = *reinterpret_cast<const uint4*>(br + ks * 32);
  }
  const int c = wc0 + grp * 16;  // this lane's 16 columns: two 8-column pieces
  const bool ok0 = c < N, ok1 = c + 8 < N;
  const int cc0 = ok0 ? c : 0, cc1 = ok1 ? c + 8 : 0;
  for (int tb = 0; tb < tiles; tb += 2) {
    uint4 uf[2][KS], ov[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t t = (tile0 + tb + h) * 16 + tok;
      const int64_t tc = t < rows ? t : rows - 1;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) uf[h][ks] = *reinterpret_cast<const uint4*>(u + tc * R + ks * 32 + grp * 8);
      ov[h][0] = *reinterpret_cast<const uint4*>(o + tc * ldo + cc0);
      ov[h][1] = *reinterpret_cast<const uint4*>(o + tc * ldo + cc1);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t t = (tile0 + tb + h) * 16 + tok;
      lw_f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        acc[nt] = lw_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[nt] = lw_mfma(bfr[nt][ks], uf[h][ks], acc[nt]);
      }
      // acc[nt][q] = sum_j u[t, j] b[c + 4 nt + q, j]
      if (tb + h < tiles && t < rows) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          if (half == 0 ? ok0 : ok1) {
            float of[8];
            Elem<kBF16>::load8(reinterpret_cast<const uint16_t*>(&ov[h][half]), of);
            lw_bf16x8 ob;
#pragma unroll
            for (int e = 0; e < 8; ++e) {  // + the bf16 adapter output, as the unfused add sees it
              const float a = static_cast<float>(static_cast<__bf16>(acc[half * 2 + e / 4][e % 4] * s));
              ob[e] = static_cast<__bf16>(of[e] + a);
            }
            *reinterpret_cast<lw_bf16x8*>(out + t * N + c + half * 8) = ob;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------ cols
// byte offset of 16-byte chunk `chunk` of row `row` in a [rows][W] bf16 LDS image.
// The 32-byte chunk pairs of a row are XORed with row bits so that the 8 rows a
// 32-lane half reads in one transposed read (rows q and 8 + q, q = 0..3, one
// pair each) fall on 8 distinct 32-byte bank ranges: at W = 128 (256-byte rows)
// with bits (0, 1, 3) of the row, at W = 64 with bits (1, 3), at W = 32 with bit 3.
template <int W>
__device__ __forceinline__ int lw_off(int row, int chunk) {
  constexpr int NP = W / 16, RP = 8 / NP;
  const int f = ((row & 3) / RP) | (((row >> 3) & 1) * (4 / RP));
  return row * (W * 2) + (((chunk >> 1) ^ f) << 5) + ((chunk & 1) << 4);
}

__device__ __forceinline__ lw_s16x4 lw_tr(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lw_s16x4*)p);
}
// 16 columns x 8 consecutive rows as an MFMA fragment: two transposed reads, 4 rows (`step4` bytes) apart
__device__ __forceinline__ uint4 lw_tr_frag(const uint8_t* p, int step4) {
  const lw_s16x4 lo = lw_tr(p), hi = lw_tr(p + step4);
  return __builtin_bit_cast(uint4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

constexpr int kLwNC = 128;  // columns of a cols block (32 per wave)

// part = yscale * (sum over the rows t of range p of y[t, j] * g'(t, n)): [P][N][R] in
// mode 0 (g' = g), [P][R][N] in mode 1 (g' = drop(g), and dx is written on the way).
template <int R, int MODE>
__global__ void __launch_bounds__(256) lora_wcols_kernel(const uint16_t* __restrict__ g, int64_t ldg,
                                                         const uint16_t* __restrict__ y, const uint16_t* __restrict__ a,
                                                         uint16_t* __restrict__ dx, float* __restrict__ part,
                                                         int64_t rows, int N, int cblocks, int rpp, float yscale,
                                                         uint32_t seed, uint32_t thresh16, float inv_keep) {
  constexpr int RT = R / 16, KS = R / 32;
  constexpr int YCH = 4 * R;                  // 16-byte chunks of a y step
  constexpr int YC = (YCH + 255) / 256;       // per thread
  __shared__ __attribute__((aligned(16))) uint8_t gimg[32 * kLwNC * 2];
  __shared__ __attribute__((aligned(16))) uint8_t yimg[32 * R * 2];
  __shared__ __attribute__((aligned(16))) uint8_t aimg[MODE == 1 ? R * kLwNC * 2 : 16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, grp = lane >> 4;
  const int p = blockIdx.x / cblocks;
  const int c0 = (blockIdx.x % cblocks) * kLwNC;
  const int64_t t0 = static_cast<int64_t>(p) * rpp < rows ? static_cast<int64_t>(p) * rpp : rows;
  const int64_t t1 = t0 + rpp < rows ? t0 + rpp : rows;

  // staging: thread -> chunks (row tid / 16 and + 16, chunk tid % 16) of g, chunks tid, tid + 256 of y
  const int gch = tid & 15, grow = tid >> 4;
  const int gc = c0 + gch * 8;
  const bool gcok = gc < N;
  const int gcc = gcok ? gc : 0;
  uint4 gq[2], yq[YC];
  auto fetch = [&](int64_t tk) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t t = tk + grow + 16 * h;
      const int64_t tc = t < t1 ? t : rows - 1;
      uint4 v = *reinterpret_cast<const uint4*>(g + tc * ldg + gcc);
      if constexpr (MODE == 1) {  // kept elements as they are, dropped ones +0
        const uint32_t kp = keep8(seed, static_cast<uint64_t>(tc) * N + gcc, thresh16);
        uint32_t m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          m[i] = (((kp >> (2 * i)) & 1u) ? 0xffffu : 0u) | (((kp >> (2 * i + 1)) & 1u) ? 0xffff0000u : 0u);
        v.x &= m[0];
        v.y &= m[1];
        v.z &= m[2];
        v.w &= m[3];
      }
      gq[h] = (t < t1 && gcok) ? v : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int i = 0; i < YC; ++i) {
      const int id = tid + 256 * i;
      const int yr = id / (R / 8), ych = id % (R / 8);
      const int64_t t = tk + yr;
      const int64_t tc = t < t1 ? t : rows - 1;
      const uint4 v = *reinterpret_cast<const uint4*>(y + tc * R + ych * 8);  // id >= YCH (r = 32): loaded, not stored
      yq[i] = t < t1 ? v : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) *reinterpret_cast<uint4*>(gimg + lw_off<kLwNC>(grow + 16 * h, gch)) = gq[h];
#pragma unroll
    for (int i = 0; i < YC; ++i) {
      const int id = tid + 256 * i;
      if (YCH >= 256 || id < YCH) *reinterpret_cast<uint4*>(yimg + lw_off<R>(id / (R / 8), id % (R / 8))) = yq[i];
    }
  };

  // transposed-read addresses (lane 4 q + pp of a 16-lane group: row q, columns 4 pp .. 4 pp + 3)
  const int tq = li >> 2, tp = li & 3;
  const int trow = 8 * grp + tq;
  int goff[2], yoff[RT];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) goff[ct] = lw_off<kLwNC>(trow, (wv * 32 + ct * 16) / 8 + (tp >> 1)) + (tp & 1) * 8;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) yoff[rt] = lw_off<R>(trow, rt * 2 + (tp >> 1)) + (tp & 1) * 8;

  // mode 1: a [R][128 columns of this block] -> LDS -> this wave's fragments of a^T (rows = columns n, permuted:
  // MFMA row m of tile ct is column 8 (m >> 2) + 4 ct + (m & 3) of the wave's 32)
  uint4 afr[MODE == 1 ? 2 : 1][MODE == 1 ? KS : 1];
  if constexpr (MODE == 1) {
#pragma unroll
    for (int i = 0; i < R * 16 / 256; ++i) {
      const int id = tid + 256 * i;
      const int ar = id >> 4, ach = id & 15;
      const int ac = c0 + ach * 8;
      const uint4 v = *reinterpret_cast<const uint4*>(a + static_cast<int64_t>(ar) * N + (ac < N ? ac : 0));
      *reinterpret_cast<uint4*>(aimg + lw_off<kLwNC>(ar, ach)) = ac < N ? v : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        afr[ct][ks] = lw_tr_frag(aimg + lw_off<kLwNC>(ks * 32 + trow, wv * 4 + tp) + ct * 8, 4 * kLwNC * 2);
  }

  lw_f32x4 acc[RT][2];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = lw_f32x4{0.f, 0.f, 0.f, 0.f};

  if (t0 < t1) fetch(t0);  // block-uniform
  for (int64_t tk = t0; tk < t1; tk += 32) {
    stash();
    __syncthreads();
    if (tk + 32 < t1) fetch(tk + 32);  // in flight under the MFMAs
    uint4 gf[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) gf[ct] = lw_tr_frag(gimg + goff[ct], 4 * kLwNC * 2);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const uint4 yf = lw_tr_frag(yimg + yoff[rt], 4 * R * 2);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = lw_mfma(yf, gf[ct], acc[rt][ct]);
    }
    if constexpr (MODE == 1) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        lw_f32x4 d[2] = {lw_f32x4{0.f, 0.f, 0.f, 0.f}, lw_f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const uint4 df = *reinterpret_cast<const uint4*>(yimg + lw_off<R>(tt * 16 + li, ks * 4 + grp));
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) d[ct] = lw_mfma(afr[ct][ks], df, d[ct]);
        }
        // d[ct][q] = sum_j du[t, j] a[j, c + 4 ct + q]
        const int64_t t = tk + tt * 16 + li;
        const int c = c0 + wv * 32 + grp * 8;
        if (t < t1 && c < N) {
          const uint32_t kp = keep8(seed, static_cast<uint64_t>(t) * N + c, thresh16);
          lw_bf16x8 db;
#pragma unroll
          for (int e = 0; e < 8; ++e) db[e] = static_cast<__bf16>(((kp >> e) & 1u) ? d[e / 4][e % 4] * inv_keep : 0.f);
          *reinterpret_cast<lw_bf16x8*>(dx + t * N + c) = db;
        }
      }
    }
    __syncthreads();
  }

  // acc[rt][ct][q] = sum_t y[t, 16 rt + 4 grp + q] g'[t, c0 + 32 wv + 16 ct + li]
  const float sc = MODE == 1 ? inv_keep : 1.f;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int n = c0 + wv * 32 + ct * 16 + li;
    if (n < N) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const lw_f32x4 v = acc[rt][ct];
        if constexpr (MODE == 0) {  // [P][N][R]: the layout of B [N, r]
          *reinterpret_cast<float4*>(part + (static_cast<int64_t>(p) * N + n) * R + rt * 16 + grp * 4) =
              make_float4(v[0] * yscale, v[1] * yscale, v[2] * yscale, v[3] * yscale);
        } else {  // [P][R][N]: the layout of A [r, K]
          float* dst = part + (static_cast<int64_t>(p) * R + rt * 16 + grp * 4) * N + n;
#pragma unroll
          for (int q = 0; q < 4; ++q) dst[static_cast<int64_t>(q) * N] = v[q] * sc * yscale;
        }
      }
    }
  }
}

// ------------------------------------------------------------- launchers
#define LORA_WR_DISPATCH(R_VAL, ...)                         \
  switch (R_VAL) {                                           \
    case 32: { constexpr int R = 32; __VA_ARGS__; break; }   \
    case 64: { constexpr int R = 64; __VA_ARGS__; break; }   \
    case 128: { constexpr int R = 128; __VA_ARGS__; break; } \
    default: return hipErrorInvalidValue;                    \
  }

bool lora_wide_rank(int r) { return r == 32 || r == 64 || r == 128; }

hipError_t launch_lora_rows_wide(const void* in, int64_t ldin, const void* w, void* out, int64_t rows, int K, int r,
                                 float scale, uint32_t seed, uint32_t thresh16, float inv_keep, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  if (K % 32 != 0 || K < 32 || ldin % 8 != 0) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((rows + 15) / 16)), block(512);
  auto I = static_cast<const uint16_t*>(in);
  auto W = static_cast<const uint16_t*>(w);
  auto O = static_cast<uint16_t*>(out);
  if (thresh16) {
    LORA_WR_DISPATCH(r, hipLaunchKernelGGL((lora_wrows_kernel<R, true>), grid, block, 0, st, I, ldin, W, O, rows, K,
                                           scale, seed, thresh16, inv_keep));
  } else {
    LORA_WR_DISPATCH(r, hipLaunchKernelGGL((lora_wrows_kernel<R, false>), grid, block, 0, st, I, ldin, W, O, rows, K,
                                           scale, seed, thresh16, inv_keep));
  }
  return hipGetLastError();
}

hipError_t launch_lora_up_wide(const void* o, int64_t ldo, const void* u, const void* b, void* out, int64_t rows, int N,
                               int r, float s, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  if (N % 8 != 0 || N < 8 || ldo % 8 != 0) return hipErrorInvalidValue;
  const int cblocks = (N + 255) / 256, tiles = 4;  // 64 tokens x 256 columns per block
  const int64_t tchunks = (rows + 16 * tiles - 1) / (16 * tiles);
  const dim3 grid(static_cast<unsigned>(tchunks * cblocks)), block(256);
  LORA_WR_DISPATCH(r, hipLaunchKernelGGL((lora_wup_kernel<R>), grid, block, 0, st, static_cast<const uint16_t*>(o), ldo,
                                         static_cast<const uint16_t*>(u), static_cast<const uint16_t*>(b),
                                         static_cast<uint16_t*>(out), rows, N, cblocks, tiles, s));
  return hipGetLastError();
}

// Row ranges of the wide-rank partials: at most rows / (2 r) of them, so that the
// fp32 partials [P, N, r] never exceed the bytes of the bf16 g operand [rows, N],
// and no more than ~1024 blocks of 128 columns; one part is always allowed.
int lora_cols_parts_wide(int64_t rows, int N, int r) {
  const int cblocks = (N + kLwNC - 1) / kLwNC;
  int64_t p = (1024 + cblocks - 1) / cblocks;
  const int64_t pmax = rows / (2 * static_cast<int64_t>(r));
  if (p > pmax) p = pmax;
  return static_cast<int>(p < 1 ? 1 : p);
}

hipError_t launch_lora_cols_wide(const void* g, int64_t ldg, const void* y, const void* a, void* dx, float* part,
                                 int64_t rows, int N, int r, int parts, int mode, float yscale, uint32_t seed,
                                 uint32_t thresh16, float inv_keep, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  if (N % 8 != 0 || N < 8 || ldg % 8 != 0 || parts < 1) return hipErrorInvalidValue;
  const int rpp = static_cast<int>((rows + parts - 1) / parts);
  const int cblocks = (N + kLwNC - 1) / kLwNC;
  const dim3 grid(static_cast<unsigned>(parts) * cblocks), block(256);
  auto G = static_cast<const uint16_t*>(g);
  auto Y = static_cast<const uint16_t*>(y);
  auto A = static_cast<const uint16_t*>(a);
  auto DX = static_cast<uint16_t*>(dx);
  if (mode == 0) {
    LORA_WR_DISPATCH(r, hipLaunchKernelGGL((lora_wcols_kernel<R, 0>), grid, block, 0, st, G, ldg, Y, A, DX, part, rows, N,
                                           cblocks, rpp, yscale, seed, thresh16, inv_keep));
  } else {
    LORA_WR_DISPATCH(r, hipLaunchKernelGGL((lora_wcols_kernel<R, 1>), grid, block, 0, st, G, ldg, Y, A, DX, part, rows, N,
                                           cblocks, rpp, yscale, seed, thresh16, inv_keep));
  }
  return hipGetLastError();
}

}  // namespace dlion
