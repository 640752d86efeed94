// Top-k of the LM head (gfx950): per row of a read-only [N, Vp] logit block the k best columns (greater value
// first, lower column first among equal values, compared as floats: -0.0 == +0.0), their stored values and the
// row's logsumexp.  Forward only, one launch, nothing written to the logits, no float atomics.
//
// One 512-thread block per row; the row is re-read from L2 / Infinity Cache in every pass (the GEMM has just
// written it).  Every decision is made on integers: a logit's key is the monotone integer image of its float
// (-0.0 canonicalised), cut to the bits the storage type can set (bf16 16, fp16 24, fp32 32), and a column's is
// its inverted index, so (key, inverted column) pairs are all distinct and their order is the contract's.
//   pass 1   online max / sum-of-exp (lm_score's form) and every thread's greatest value.  The k-th greatest of
//            the 512 thread maxima is a lower bound of the row's k-th greatest value: the later passes drop what
//            is below it with one float compare per logit (NaN is never below, so it stays in play), which on
//            ordinary rows leaves about k columns for the integer work and the LDS atomics.
//   select   radix select over the pair, 8 bits per pass from the top: an integer LDS histogram of the columns
//            still in play, a suffix scan, the bucket that holds the k-th pair.  It ends as soon as a bucket
//            holds exactly what is still needed -- after the value digits unless the k-th value is tied.
//   collect  the k pairs at or above the threshold go to LDS (slot order is arbitrary); one wave ranks each by
//            counting the pairs above it and writes it to its place, so the outputs are order-free.
#include "common.h"

#include <climits>

namespace dlion {

constexpr int kTopkThreads = 512;
constexpr int kTopkUnroll = 4;  // chunks of 8 logits in flight per thread
constexpr int kTopkMax = 64;    // the binding refuses a larger k
constexpr int kTopkBins = 256;  // 8-bit digits

template <int DT> struct TopkKey {  // bits of the fp32 image that the storage type can set
  static constexpr int bits = DT == kF32 ? 32 : (DT == kBF16 ? 16 : 24);
};

template <int DT> __device__ __forceinline__ uint32_t topk_key(float f) {
  uint32_t u = __float_as_uint(f);
  u = u == 0x80000000u ? 0u : u;  // -0.0 sorts as +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return u >> (32 - TopkKey<DT>::bits);
}

__device__ __forceinline__ float wave_min_f32(float x) {  // no NaN among the operands
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = fminf(x, __shfl_xor(x, off, 64));
  return x;
}

template <int DT>
__global__ void __launch_bounds__(kTopkThreads)
lm_topk_kernel(const typename Elem<DT>::S* __restrict__ logits, int64_t vp, int v, int k, float* __restrict__ values,
               int* __restrict__ ids, float* __restrict__ row_lse) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int T = kTopkThreads, W = kTopkThreads / 64, U = kTopkUnroll, KB = TopkKey<DT>::bits;
  __shared__ __attribute__((aligned(16))) float tmax[T];
  __shared__ int hist[2][kTopkBins];
  __shared__ float redm[W], reds[W];
  __shared__ float redk[W];
  __shared__ uint32_t sel_key[kTopkMax], sel_col[kTopkMax];
  __shared__ float sel_val[kTopkMax];
  __shared__ int ctl[4];  // bucket, still needed inside it, bucket holds exactly that, survivors appended
  const int64_t row = blockIdx.x;
  const S* x = logits + row * vp;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // f(values[8], first column, real columns in the chunk); columns at and past v take part in nothing
  auto sweep = [&](auto&& f) {
    for (int base = tid * 8; base < v; base += T * 8 * U) {
      float c[U][8];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int e = base + i * T * 8;
        if (e < v) E::load8(x + e, c[i]);  // v <= vp and vp % 8 == 0 keep every chunk inside the row
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int e = base + i * T * 8;
        if (e < v) f(c[i], e, min(8, v - e));
      }
    }
  };

  // ---- pass 1: logsumexp and the thread's greatest value (fmaxf skips NaN: -inf where a thread saw nothing else)
  float m = -INFINITY, sm = 0.f, tm = -INFINITY;
  sweep([&](const float (&f)[8], int, int nv) {
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = f[j];
    if (nv < 8) {  // the one chunk per row that straddles v
#pragma unroll
      for (int j = 1; j < 8; ++j) g[j] = j < nv ? f[j] : -INFINITY;
    }
    float cm = fmaxf(g[0], g[1]);
#pragma unroll
    for (int j = 2; j < 8; ++j) cm = fmaxf(cm, g[j]);
    tm = fmaxf(tm, cm);
    if (cm > m) {
      sm *= __expf(m - cm);
      m = cm;
    }
    if (m > -INFINITY) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm += __expf(g[j] - m);
    }
  });
  const float wm = wave_max_dpp(m);
  const float ws = wave_sum_dpp(m > -INFINITY ? sm * __expf(m - wm) : 0.f);
  if (lane == 0) {
    redm[wid] = wm;
    reds[wid] = ws;
  }
  tmax[tid] = tm;
  __syncthreads();
  if (tid == 0) {
    float mx = redm[0];
#pragma unroll
    for (int w = 1; w < W; ++w) mx = fmaxf(mx, redm[w]);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) sum += redm[w] > -INFINITY ? reds[w] * __expf(redm[w] - mx) : 0.f;
    row_lse[row] = mx + __logf(sum);
  }
  // the k-th greatest thread maximum: the least one with fewer than k above it.  At least k columns of the row
  // are not below it (one per such thread; every column when it is -inf), so nothing below it is among the k best.
  int above_me = 0;
  for (int j = 0; j < T; j += 4) {
    const float4 o = *reinterpret_cast<const float4*>(&tmax[j]);
    above_me += (o.x > tm ? 1 : 0) + (o.y > tm ? 1 : 0) + (o.z > tm ? 1 : 0) + (o.w > tm ? 1 : 0);
  }
  const float wl = wave_min_f32(above_me < k ? tm : INFINITY);
  if (lane == 0) redk[wid] = wl;
  __syncthreads();
  float floor_f = redk[0];
#pragma unroll
  for (int w = 1; w < W; ++w) floor_f = fminf(floor_f, redk[w]);
  // f(value, column) for the columns in play; a chunk without one costs eight compares
  auto sweep_in_play = [&](auto&& f) {
    sweep([&](const float (&c)[8], int e, int nv) {
      bool any = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) any |= !(c[j] < floor_f);
      if (any) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nv && !(c[j] < floor_f)) f(c[j], e + j);
      }
    });
  };

  // ---- radix select over (key, inverted column)
  const int cbits = v > 1 ? 32 - __builtin_clz(static_cast<unsigned>(v - 1)) : 0;
  const int cb8 = (cbits + 7) & ~7;
  const uint32_t cmax = cb8 >= 32 ? 0xffffffffu : (1u << cb8) - 1u;  // >= v - 1
  uint32_t vmask = 0, vval = 0, cmask = 0, cval = 0;
  int need = k;
  bool exact = false;

  // one digit: in_play(key, inverted column, digit&) -> bool; returns the bucket of the pair still looked for
  auto digit_pass = [&](auto&& in_play) -> uint32_t {
    if (tid < kTopkBins) hist[0][tid] = 0;
    __syncthreads();
    sweep_in_play([&](float f, int col) {
      uint32_t d;
      if (in_play(topk_key<DT>(f), cmax - static_cast<uint32_t>(col), d)) atomicAdd(&hist[0][d], 1);
    });
    __syncthreads();
    const int own = tid < kTopkBins ? hist[0][tid] : 0;
    int *a = hist[0], *b = hist[1];
#pragma unroll 1
    for (int off = 1; off < kTopkBins; off <<= 1) {  // inclusive suffix sums; 8 steps end in hist[0]
      if (tid < kTopkBins) b[tid] = a[tid] + (tid + off < kTopkBins ? a[tid + off] : 0);
      __syncthreads();
      int* t = a;
      a = b;
      b = t;
    }
    if (tid < kTopkBins) {
      const int above = a[tid] - own;
      if (above < need && need <= above + own) {  // one bucket: those in play are at least `need`
        ctl[0] = tid;
        ctl[1] = need - above;
        ctl[2] = own == need - above ? 1 : 0;
      }
    }
    __syncthreads();
    const uint32_t bucket = static_cast<uint32_t>(ctl[0]);
    need = ctl[1];
    exact = ctl[2] != 0;
    __syncthreads();
    return bucket;
  };

#pragma unroll 1
  for (int shift = KB - 8; shift >= 0 && !exact; shift -= 8) {
    const uint32_t b = digit_pass([&](uint32_t key, uint32_t, uint32_t& d) {
      d = (key >> shift) & 0xffu;
      return (key & vmask) == vval;
    });
    vmask |= 0xffu << shift;
    vval |= b << shift;
  }
  // the k-th value is tied: the lowest columns of that value, i.e. the greatest inverted columns
#pragma unroll 1
  for (int shift = cb8 - 8; shift >= 0 && !exact; shift -= 8) {
    const uint32_t b = digit_pass([&](uint32_t key, uint32_t ic, uint32_t& d) {
      d = (ic >> shift) & 0xffu;
      return key == vval && (ic & cmask) == cval;
    });
    cmask |= 0xffu << shift;
    cval |= b << shift;
  }

  // ---- collect the k pairs at or above (vval, cval), then order them
  if (tid == 0) ctl[3] = 0;
  __syncthreads();
  sweep_in_play([&](float f, int col) {
    const uint32_t key = topk_key<DT>(f), ic = cmax - static_cast<uint32_t>(col);
    if (key > vval || (key == vval && ic >= cval)) {
      const int slot = atomicAdd(&ctl[3], 1);
      if (slot < kTopkMax) {
        sel_key[slot] = key;
        sel_col[slot] = ic;
        sel_val[slot] = f;
      }
    }
  });
  __syncthreads();
  const int got = min(ctl[3], k);
  if (tid < got) {
    const uint32_t key = sel_key[tid], ic = sel_col[tid];
    int pos = 0;
    for (int j = 0; j < got; ++j) {
      const uint32_t kj = sel_key[j], cj = sel_col[j];
      pos += (kj > key || (kj == key && cj > ic)) ? 1 : 0;
    }
    if (pos < k) {
      values[row * k + pos] = sel_val[tid];
      ids[row * k + pos] = static_cast<int>(cmax - ic);
    }
  }
}

// 1 <= k <= 64, k <= v <= vp, vp % 8 == 0 are checked by the binding as well
hipError_t launch_lm_topk(int dt, const void* logits, int64_t n, int64_t vp, int v, int k, float* values, int* ids,
                          float* lse, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(logits) % 16 != 0 || vp % 8 != 0 || v <= 0 || v > vp || n > INT_MAX || k < 1 ||
      k > kTopkMax || k > v || vp > (int64_t{1} << 30))
    return hipErrorInvalidValue;
#define LM_TOPK(DT)                                                                                  \
  hipLaunchKernelGGL((lm_topk_kernel<DT>), dim3(n), dim3(kTopkThreads), 0, st,                       \
                     static_cast<const typename Elem<DT>::S*>(logits), vp, v, k, values, ids, lse)
  switch (dt) {
    case kF32: LM_TOPK(kF32); break;
    case kBF16: LM_TOPK(kBF16); break;
    case kF16: LM_TOPK(kF16); break;
    default: return hipErrorInvalidValue;
  }
#undef LM_TOPK
  return hipGetLastError();
}

}  // namespace dlion
