// Decode projections: out[M, N] = x[M, K] . w[N, K]^T (+ bias) for 1 <= M <= 16 rows (one token per sequence of a
// decode step), bf16 in / out with fp32 accumulation, the weight either bf16 or the 4-bit block store of quant.hip.
//
// The product is bound by the weight stream: every weight byte is needed once, x (at most 16 x K) is re-read by
// every block.  A wave owns 16 weight rows and a range of k.  It loads its weight bytes straight from global
// memory into registers, 16 bytes per lane, all loads of its 4 steps (512 k) of a chunk issued before the first
// wait (bf16: 16 per lane, 4-bit: 4 plus 4 scales) -- no LDS staging, nothing of the weight is shared between waves
// -- and feeds them to v_mfma_f32_16x16x32_bf16 as the A operand (row = weight row); the B operand is x with its
// rows padded to 16 by zero fragments.  The block stages its chunk of x in LDS once, in whole rows (full 128-byte
// lines), and every wave reads its B fragments from there with ds_read_b128.
//
// Two forms of one kernel.  Wide: the 4 waves of a block take 4 adjacent 16-row tiles and the same k.  Tall (an
// unsplit launch at N <= 4096): the 4 waves take one 16-row tile and split its k among themselves, their
// accumulator tiles added through LDS in wave order -- small weights get 4 times the blocks and finish in one
// launch, where a K split over blocks would need a partials buffer and the combine pass.
//
// k order.  A 16-byte load of the 4-bit store is 32 consecutive k of one row, so within a 128-k step the lane
// (row r, group g = lane >> 4) owns k = 32 g .. 32 g + 31, and MFMA i of the step takes the lane's k = 32 g + 8 i
// .. + 7 (the MFMA sums over its 32 (group, element) slots; which k sits in which slot is free as long as x uses
// the same assignment).  The bf16 kernel uses the same assignment: the lane's 64 contiguous bytes of its row are 4
// loads, issued back to back, which together consume two whole 128-byte lines of each of the 16 rows.  Both
// kernels are one template; only the way a lane's raw loads become the step's 4 operand fragments differs.  The
// 4-bit fragment is bf16_rne(code[idx] * absmax) -- dequant4_kernel's product and cast, through the same 256-entry
// byte-pair table -- so skinny_gemm_w4(x, q, absmax, code) and skinny_gemm_nt(x, dequant4(q, absmax, code)) put
// the same bits into the same MFMA slots in the same order: they are bit-identical.
//
// Decomposition (host, ops/fused.py skinny_splits): grid (ceil(N / 64) or ceil(N / 16), splits); split s owns the
// 128-k steps [s per, (s + 1) per).  One split writes bf16 (acc + bias, one rounding); more write fp32 partials
// [splits, M, N] and skinny_combine_kernel adds them in index order (+ bias, one rounding).  No atomics: same
// inputs, same bits.
//
// Addresses: weight rows are clamped into [0, N), a lane's k into its row (K % 64 == 0: the last step of a row may
// hold 64 k only; its upper two lane groups load the row's last 32 k again and their fragments are zeroed, as are
// x's), x rows >= M are never read (their LDS rows are zero), and only out[:M, :N] is stored.
#include "common.h"
#include "kernels.h"

namespace dlion {
namespace {

typedef __bf16 sk_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sk_bf16x2 __attribute__((ext_vector_type(2)));
typedef float sk_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepK = 128;                     // k of one step: 4 MFMAs, 32 k per lane
constexpr int kChunkSteps = 4;                  // steps per wave and chunk: their weight loads are in flight together
constexpr int kBlockRows = 64;                  // wide form: 4 waves x 16 weight rows
constexpr int kTallMaxN = 4096;                 // tall form (the 4 waves split K over one 16-row tile): unsplit N <= this

// bf16 weight [N, K]: the lane's 32 k are 4 loads, each already an operand fragment
struct WeightBf16 {
  static constexpr int kTab = 1;
  const uint16_t* w;
  struct Raw {
    uint4 v[4];
  };
  __device__ __forceinline__ Raw load(int64_t row, int K, int k) const {
    const uint4* p = reinterpret_cast<const uint4*>(w + row * K + k);
    Raw r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = p[i];
    return r;
  }
  __device__ __forceinline__ static void init(float2*, const float*) {}
  __device__ __forceinline__ static void frags(const Raw& r, const float2*, uint4 (&f)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = r.v[i];
  }
};

// 4-bit weight (quant.hip's store): the lane's 32 k are one 16-byte load and one scale; dword i holds the 8 k of
// MFMA i, byte b of it the elements 2 b (high nibble) and 2 b + 1
struct Weight4bit {
  static constexpr int kTab = 256;
  const uint8_t* q;
  const float* absmax;
  const float* code;
  struct Raw {
    uint4 v;
    float s;
  };
  __device__ __forceinline__ Raw load(int64_t row, int K, int k) const {
    const int64_t e = row * K + k;  // a multiple of 32
    Raw r;
    r.v = *reinterpret_cast<const uint4*>(q + (e >> 1));
    r.s = absmax[e >> 6];
    return r;
  }
  __device__ __forceinline__ static void init(float2* tab, const float* code) {
    tab[threadIdx.x] = make_float2(code[threadIdx.x >> 4], code[threadIdx.x & 15]);
  }
  __device__ __forceinline__ static void frags(const Raw& r, const float2* tab, uint4 (&f)[4]) {
    const uint32_t words[4] = {r.v.x, r.v.y, r.v.z, r.v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t o[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float2 c = tab[(words[i] >> (8 * b)) & 0xffu];
        sk_bf16x2 pr;
        pr[0] = static_cast<__bf16>(c.x * r.s);  // dequant4_kernel's product and rounding
        pr[1] = static_cast<__bf16>(c.y * r.s);
        o[b] = __builtin_bit_cast(uint32_t, pr);
      }
      f[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
};

// 256 threads; part == nullptr: bf16 out (splits == 1); else fp32 part[s, m, n].
// Wide form (TALL = false), grid (ceil(N / 64), splits): the 4 waves take 4 adjacent 16-row tiles and the same 4
// steps of a chunk.  Tall form (TALL = true), grid (ceil(N / 16), splits): the 4 waves take ONE 16-row tile and
// split the block's k among themselves -- a chunk is 16 steps, wave v takes its steps v, v + 4, v + 8, v + 12 -- and
// their 4 accumulator tiles are added through LDS in wave order.  It is the form for small N, where 64-row blocks
// would leave most CUs idle and a K split over blocks would cost a partials buffer and a second launch.
template <class W, bool TALL>
__global__ void __launch_bounds__(256) skinny_gemm_kernel(const uint16_t* __restrict__ x, int64_t ldx, W wt,
                                                          const uint16_t* __restrict__ bias,
                                                          uint16_t* __restrict__ out, int64_t ldo,
                                                          float* __restrict__ part, int M, int N, int K, int steps,
                                                          int per) {
  constexpr int kXSteps = TALL ? 4 * kChunkSteps : kChunkSteps;  // steps of the block's x chunk
  constexpr int kRowPieces = kXSteps * kStepK / 8;               // 16-byte pieces of one chunk row
  constexpr int kXRow = kXSteps * kStepK + 8;  // LDS row stride (elements): a multiple of 256 bytes plus 16, so the
                                               // 16 rows a ds_read_b128 takes start 16 bytes apart modulo 256
  constexpr int kXPieces = 16 * kRowPieces / 256;  // pieces per thread
  __shared__ __attribute__((aligned(16))) uint16_t xs[16 * kXRow];
  __shared__ float2 tab[W::kTab];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s = blockIdx.y;
  const int st_begin = s * per;
  const int st_end = (steps - st_begin) > per ? st_begin + per : steps;  // block-uniform, st_begin < st_end
  const int64_t n_tile = TALL ? static_cast<int64_t>(blockIdx.x) * 16
                              : static_cast<int64_t>(blockIdx.x) * kBlockRows + wv * 16;
  const int64_t row = (n_tile + r) < N ? n_tile + r : N - 1;  // clamped: always a row of the weight
  if constexpr (W::kTab > 1) W::init(tab, wt.code);  // ordered before its first use by the loop's barriers

  sk_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = st_begin; c0 < st_end; c0 += kXSteps) {
    // the block's x chunk [16, 512 or 2048]: thread t takes the 16-byte pieces t, t + 256, ... (whole rows, i.e.
    // full lines, per wave); rows >= M and k >= K are zero and load x[0, 0 .. 7] instead
    uint4 xr[kXPieces];
#pragma unroll
    for (int j = 0; j < kXPieces; ++j) {
      const int p = tid + j * 256;
      const int xrow = p / kRowPieces, k = c0 * kStepK + (p % kRowPieces) * 8;
      const bool ok = xrow < M && k < K;
      xr[j] = *reinterpret_cast<const uint4*>(x + (ok ? static_cast<int64_t>(xrow) * ldx + k : 0));
      if (!ok) xr[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    // the wave's weight bytes of the chunk, all in flight together; a step past the split's end repeats its last
    typename W::Raw wr[kChunkSteps];
#pragma unroll
    for (int u = 0; u < kChunkSteps; ++u) {
      const int su = TALL ? 4 * u + wv : u;  // the wave's u-th step of the chunk
      const int st = (c0 + su) < st_end ? c0 + su : st_end - 1;
      const int k = st * kStepK + 32 * g;
      wr[u] = wt.load(row, K, k < K ? k : K - 32);
    }
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < kXPieces; ++j) {
      const int p = tid + j * 256;
      *reinterpret_cast<uint4*>(&xs[(p / kRowPieces) * kXRow + (p % kRowPieces) * 8]) = xr[j];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kChunkSteps; ++u) {
      const int su = TALL ? 4 * u + wv : u;
      if (c0 + su < st_end) {  // wave-uniform
        uint4 f[4];
        W::frags(wr[u], tab, f);
        const uint16_t* xf = &xs[r * kXRow + su * kStepK + 32 * g];
        if ((c0 + su + 1) * kStepK <= K) {  // wave-uniform: a full step, every lane's 32 k are in the row
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sk_bf16x8, f[i]),
                                                          *reinterpret_cast<const sk_bf16x8*>(xf + 8 * i), acc, 0, 0, 0);
        } else {  // the 64-k last step of a row: the upper two lane groups hold no k, both their operands are zero
          const bool live = g < 2;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            uint4 a = f[i];
            uint4 b = *reinterpret_cast<const uint4*>(xf + 8 * i);
            if (!live) {
              a = make_uint4(0u, 0u, 0u, 0u);
              b = make_uint4(0u, 0u, 0u, 0u);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sk_bf16x8, a),
                                                          __builtin_bit_cast(sk_bf16x8, b), acc, 0, 0, 0);
          }
        }
      }
    }
  }
  if constexpr (TALL) {  // the 4 waves' tiles, added in wave order by wave 0
    sk_f32x4* red = reinterpret_cast<sk_f32x4*>(xs);
    __syncthreads();  // the last chunk's fragment reads are done
    if (wv > 0) red[(wv - 1) * 64 + lane] = acc;
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const sk_f32x4 o = red[v * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += o[j];
    }
  }
  // acc[j] = sum over the split of x[m = lane & 15, :] . w[n_tile + 4 (lane >> 4) + j, :]
  const int m = r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t n = n_tile + 4 * g + j;
    if (m < M && n < N) {
      if (part != nullptr) {
        part[(static_cast<int64_t>(s) * M + m) * N + n] = acc[j];
      } else {
        const float v = bias != nullptr ? acc[j] + bf16_to_f32(bias[n]) : acc[j];
        out[m * ldo + n] = f32_to_bf16(v);
      }
    }
  }
}

// out[m, n] = bf16(sum_s part[s, m, n] (+ bias[n])), the splits in index order
__global__ void __launch_bounds__(256) skinny_combine_kernel(const float* __restrict__ part,
                                                             const uint16_t* __restrict__ bias,
                                                             uint16_t* __restrict__ out, int64_t ldo, int M, int N,
                                                             int S) {
  const int64_t mn = static_cast<int64_t>(M) * N;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= mn) return;
  const int m = static_cast<int>(idx / N);
  const int64_t n = idx - static_cast<int64_t>(m) * N;
  float sum = part[idx];
  for (int s = 1; s < S; ++s) sum += part[s * mn + idx];
  if (bias != nullptr) sum += bf16_to_f32(bias[n]);
  out[m * ldo + n] = f32_to_bf16(sum);
}

bool bad_shape(int M, int N, int K, int splits, int per) {
  if (M < 1 || M > kSkinnyMaxM || N < 1 || K < 64 || K % 64) return true;
  const int steps = (K + kStepK - 1) / kStepK;
  // every split owns at least one step and the splits cover them all
  return splits < 1 || splits > kSkinnyMaxSplits || per < 1 || static_cast<int64_t>(splits - 1) * per >= steps ||
         static_cast<int64_t>(splits) * per < steps;
}

template <class W>
hipError_t launch(const void* x, int64_t ldx, W wt, const void* bias, void* out, int64_t ldo, float* part, int M,
                  int N, int K, int splits, int per, hipStream_t st) {
  if (bad_shape(M, N, K, splits, per) || (splits > 1 && part == nullptr)) return hipErrorInvalidValue;
  const int steps = (K + kStepK - 1) / kStepK;
  const bool tall = splits == 1 && N <= kTallMaxN;
  const int64_t nblk = tall ? (static_cast<int64_t>(N) + 15) / 16 : (static_cast<int64_t>(N) + kBlockRows - 1) / kBlockRows;
  const dim3 grid(static_cast<unsigned>(nblk), static_cast<unsigned>(splits));
  auto* X = static_cast<const uint16_t*>(x);
  auto* B = static_cast<const uint16_t*>(bias);
  auto* O = static_cast<uint16_t*>(out);
  float* P = splits > 1 ? part : nullptr;
  if (tall)
    hipLaunchKernelGGL((skinny_gemm_kernel<W, true>), grid, dim3(256), 0, st, X, ldx, wt, B, O, ldo, P, M, N, K, steps, per);
  else
    hipLaunchKernelGGL((skinny_gemm_kernel<W, false>), grid, dim3(256), 0, st, X, ldx, wt, B, O, ldo, P, M, N, K, steps, per);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || splits == 1) return e;
  const int64_t mn = static_cast<int64_t>(M) * N;
  hipLaunchKernelGGL(skinny_combine_kernel, dim3(static_cast<unsigned>((mn + 255) / 256)), dim3(256), 0, st, P, B, O,
                     ldo, M, N, splits);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_skinny_gemm_nt(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo,
                                 float* part, int M, int N, int K, int splits, int per, hipStream_t st) {
  return launch(x, ldx, WeightBf16{static_cast<const uint16_t*>(w)}, bias, out, ldo, part, M, N, K, splits, per, st);
}

hipError_t launch_skinny_gemm_w4(const void* x, int64_t ldx, const uint8_t* q, const float* absmax, const float* code,
                                 const void* bias, void* out, int64_t ldo, float* part, int M, int N, int K,
                                 int splits, int per, hipStream_t st) {
  return launch(x, ldx, Weight4bit{q, absmax, code}, bias, out, ldo, part, M, N, K, splits, per, st);
}

}  // namespace dlion
